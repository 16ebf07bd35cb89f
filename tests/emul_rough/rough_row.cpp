// ang_row8 / make_ang_mode of uvg266_amd/csrc/intra_pred_dev.h -- the branch-free angular row of the device's rough search
// (ctu_core.h rough_costs) -- compiled for the host and compared with predict_row<8> on make_mode_info, for every mode 2..66, every
// row and every tile column of an n x n block.  Built by tests/test_rough_row.py itself (into pytest's temporary directory).
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include "intra_pred_dev.h"

// counts[]: 0 rows compared, 1 rows that differ, 2 outputs whose unclamped tap sum lies outside [0, maxv], 3 samples taken from the
// projected side reference, 4 samples the angular PDPC changed, 5 samples the pure modes' PDPC changed, 6 rows predicted from the
// smoothed references.  first_bad[]: mode, yd, xd0, column of the first difference.
// top / left / ftop / fleft: 4 n + 8 entries each, as the kernel lays them out.
extern "C" __attribute__((visibility("default"))) void rough_row_compare(int n, int maxv, const uint16_t *top, const uint16_t *left, const uint16_t *ftop,
                                                                         const uint16_t *fleft, long long *counts, int *first_bad)
{
  uint32_t disp[17], cubic[32];      // the tables as ctu_leaf4.h leaf_tables packs them
  for (int i = 0; i < 17; ++i) disp[i] = (uint32_t)kSampleDisp[i] | (uint32_t)kInvDisp[i] << 8;
  for (int i = 0; i < 32; ++i)
    cubic[i] = (uint32_t)(uint8_t)kCubic[i][0] | (uint32_t)(uint8_t)kCubic[i][1] << 8 | (uint32_t)(uint8_t)kCubic[i][2] << 16 | (uint32_t)(uint8_t)kCubic[i][3] << 24;
  const ref_rows R = {top, left, ftop, fleft};
  const int log2n = ilog2_dev(n);
  for (int mode = 2; mode <= 66; ++mode) {
    const mode_info M = make_mode_info(mode, n, n, 0);
    mode_info M0 = M;
    M0.pdpc = 0;
    const auto A = make_ang_mode(R, (const uint32_t *)disp, mode, log2n);
    for (int yd = 0; yd < n; ++yd)
      for (int xd0 = 0; xd0 < n; xd0 += 8) {
        int want[8], plain[8], got[8];
        predict_row<8>(M, R, 0, 0, n, n, yd, xd0, maxv, want);
        predict_row<8>(M0, R, 0, 0, n, n, yd, xd0, maxv, plain);
        ang_row8(A, (const uint32_t *)cubic, n, yd, xd0, maxv, got);
        ++counts[0];
        counts[6] += M.filtered != 0;
        bool bad = false;
        for (int i = 0; i < 8; ++i) {
          if (got[i] != want[i] && !bad) {
            bad = true;
            if (counts[1] == 0) { first_bad[0] = mode; first_bad[1] = yd; first_bad[2] = xd0; first_bad[3] = i; }
          }
          if (want[i] != plain[i]) ++counts[M.sample_disp != 0 ? 4 : 5];
        }
        counts[1] += bad;
        // what the row reads and sums, restated: the reference samples di + xd0 + k of the main row (the projected side reference
        // for a negative index) and, for a fractional angle, the four-tap sum before its clamp
        const uint16_t *mainr = M.vertical ? (M.filtered ? ftop : top) : (M.filtered ? fleft : left);
        const uint16_t *side = M.vertical ? (M.filtered ? fleft : left) : (M.filtered ? ftop : top);
        const int delta = M.sample_disp * (yd + 1), di = delta >> 5, df = delta & 31;
        int p[11];
        for (int k = 0; k < 11; ++k) {
          const int idx = di + xd0 + k;
          if (idx >= 0) p[k] = mainr[idx];
          else {
            p[k] = side[min((-idx * M.inv_disp + 256) >> 9, n)];
            if (M.frac ? true : (k >= 1 && k <= 8)) ++counts[3];
          }
        }
        if (M.frac)
          for (int i = 0; i < 8; ++i) {
            int f[4];
            for (int j = 0; j < 4; ++j) f[j] = M.use_cubic ? kCubic[df][j] : (j == 0 ? 16 - (df >> 1) : j == 1 ? 32 - (df >> 1) : j == 2 ? 16 + (df >> 1) : df >> 1);
            const int sum = (f[0] * p[i] + f[1] * p[i + 1] + f[2] * p[i + 2] + f[3] * p[i + 3] + 32) >> 6;
            if (sum < 0 || sum > maxv) ++counts[2];
          }
      }
  }
}
