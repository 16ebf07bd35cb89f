// The filter stage's hand-out order (filters.hip): ticket t of a launch -> (picture, CTU row, CTU column).  Plain integer code that compiles
// for the device and for the host (tests/emul_ticket/ticket_emul.cpp checks it on the CPU: a wrong order is a workgroup that waits for a CTU no
// running workgroup will ever take -- a hang, not a wrong sample).
//
// The launch covers the CTU rows [row0, row1) of n_pictures pictures of wc CTUs a row.  Tickets go diagonal by diagonal of the BAND
// (d = cx + (cy - row0)); inside a diagonal picture by picture, inside a picture from the upper right CTU of the diagonal down to the
// lower left one.  So a CTU's left neighbour (diagonal d - 1), its upper neighbour (d - 1) and its upper right neighbour (diagonal d, one
// row up: handed out just before it) all hold smaller tickets, and with a workgroup per ticket -- or persistent workgroups that take
// tickets in order -- every flag a CTU waits for belongs to a CTU that is running or done.  Row row0 has no neighbour above INSIDE the
// launch: what it reads of row row0 - 1 is complete in the buffers before the launch (ctu_filter.h: filt_ctu::row0).
#pragma once

#if defined(__HIPCC__)
#define UVGI_TICKET_FN __host__ __device__ inline
#else
#define UVGI_TICKET_FN inline
#endif

struct uvgi_ticket_ctu { int pic, cy, cx; };

UVGI_TICKET_FN uvgi_ticket_ctu uvgi_filter_ticket(int t, int wc, int row0, int row1, int n_pictures)
{
  const int hb = row1 - row0;
  int d = 0;
  if (t < 0) return uvgi_ticket_ctu{-1, -1, -1};
  for (;; ++d) {
    const int lo = d - (wc - 1) > 0 ? d - (wc - 1) : 0, hi = d < hb - 1 ? d : hb - 1, cnt = (hi - lo + 1) * n_pictures;
    if (t < cnt) break;
    if (cnt <= 0) return uvgi_ticket_ctu{-1, -1, -1};          // past the last diagonal: no such ticket (t < 0 or t >= wc * (row1 - row0) * n_pictures)
    t -= cnt;
  }
  const int lo = d - (wc - 1) > 0 ? d - (wc - 1) : 0, hi = d < hb - 1 ? d : hb - 1, per = hi - lo + 1;
  const int pic = t / per, by = lo + (t - pic * per);
  return uvgi_ticket_ctu{pic, row0 + by, d - by};
}
