// Host build of the filter stage's ticket mapping (uvg266_amd/csrc/ctu_ticket.h) for tests/test_filter_ticket.py: the order in which a launch
// over the CTU rows [row0, row1) of n pictures hands its CTUs out, as [ticket] -> (picture, cy, cx).
#include "ctu_ticket.h"

extern "C" __attribute__((visibility("default"))) int ticket_emul_order(int wc, int row0, int row1, int n_pictures, int *out)
{
  const int total = wc * (row1 - row0) * n_pictures;
  for (int t = 0; t < total; ++t) {
    const uvgi_ticket_ctu c = uvgi_filter_ticket(t, wc, row0, row1, n_pictures);
    out[3 * t] = c.pic; out[3 * t + 1] = c.cy; out[3 * t + 2] = c.cx;
  }
  return total;
}

// a single ticket, valid or not (outside [0, total): (-1, -1, -1))
extern "C" __attribute__((visibility("default"))) void ticket_emul_one(int t, int wc, int row0, int row1, int n_pictures, int *out)
{
  const uvgi_ticket_ctu c = uvgi_filter_ticket(t, wc, row0, row1, n_pictures);
  out[0] = c.pic; out[1] = c.cy; out[2] = c.cx;
}
