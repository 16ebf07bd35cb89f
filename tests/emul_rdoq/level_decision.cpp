// coded_level2 of uvg266_amd/csrc/ctu_core.h -- the device RDOQ's level decision as straight-line code -- compiled for the host and
// compared with coded_level (+ ic_rate), the transcription of uvg_get_coded_level / uvg_get_ic_rate that the host emulation keeps:
// level, coded_cost and coded_cost_sig as 64-bit patterns.  Built by tests/test_rdoq_level_decision.py itself (into pytest's
// temporary directory).
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <vector>
#include <algorithm>
#include "ctu_core.h"

namespace {

uint64_t bits_of(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }

struct sweep {
  ctu::rdoq_env E;
  long long *counts;
  long long *first_bad;
  // counts[]: 0 decisions compared, 1 that differ, 2 candidate kept, 3 candidate lowered by one, 4 "not significant" chosen for a
  // candidate >= 1, 5 a priced level with the exp-Golomb escape code (q >= 5), 6 ... with its prefix at the cap of 12,
  // 7 decisions of a last position, 8 bypass-priced decisions
  void one(int last, uint32_t reg_bins, int go_rice, int ctx_sig, int ctx_set, int32_t level_double, uint32_t mal)
  {
    const double c0 = (double)level_double * (double)level_double * E.error_scale;
    double cc_a = -1.0, cc_b = -1.0, cs_a = 0, cs_b = 0;          // (the callers hand coded_cost_sig in as 0)
    const uint32_t la = ctu::coded_level(E, &cc_a, c0, &cs_a, level_double, mal, ctx_sig, ctx_set, go_rice, reg_bins, last);
    const uint32_t lb = ctu::coded_level2(E, &cc_b, c0, &cs_b, level_double, mal, ctx_sig, ctx_set, go_rice, reg_bins, last);
    ++counts[0];
    if (la != lb || bits_of(cc_a) != bits_of(cc_b) || bits_of(cs_a) != bits_of(cs_b)) {
      if (counts[1] == 0) {
        const long long f[12] = {E.t, last, (long long)reg_bins, go_rice, ctx_sig, ctx_set, E.q_bits, level_double, (long long)mal, la, lb,
                                 (bits_of(cc_a) != bits_of(cc_b)) + 2 * (bits_of(cs_a) != bits_of(cs_b))};
        memcpy(first_bad, f, sizeof f);
      }
      ++counts[1];
    }
    if (mal >= 1) {
      counts[2] += la == mal;
      counts[3] += la + 1 == mal && la >= 1;
      counts[4] += la == 0;
    }
    counts[7] += last != 0;
    counts[8] += reg_bins < 4;
    // the escape codes priced on the way, restated from uvg_get_ic_rate
    for (uint32_t a = mal; a + 1 >= mal && a >= 1; --a) {
      int64_t symbol = -1;
      if (reg_bins < 4) symbol = a <= (1u << go_rice) ? a - 1 : a;
      else if (a >= 4) symbol = a - 4;
      if (symbol >= 0 && (symbol >> go_rice) >= 5) {
        ++counts[5];
        counts[6] += (symbol >> go_rice) - 5 > (2 << 11) - 2;
      }
    }
  }
  // level_double across the whole rounding interval of mal: (level_double + half) >> q_bits == mal
  void interval(int last, uint32_t reg_bins, int go_rice, int ctx_sig, int ctx_set, uint32_t mal, bool dense)
  {
    const int64_t half = (int64_t)1 << (E.q_bits - 1), centre = (int64_t)mal << E.q_bits;
    const int64_t lo = mal ? centre - half : 0, hi = centre + half - 1;
    if (hi > 0x7fffffff - half) return;          // beyond what the quantiser's cap lets through at this q_bits
    const int64_t dense_at[] = {lo, lo + 1, lo + (centre - lo) / 2, centre - 1, centre, centre + 1, centre + (hi - centre) / 2, hi - 1, hi,
                                lo + (hi - lo) / 3, lo + 2 * (hi - lo) / 3};
    const int64_t sparse_at[] = {lo, lo + (centre - lo) / 2, centre, centre + (hi - centre) / 2, hi};
    const int64_t *at = dense ? dense_at : sparse_at;
    const int n = dense ? 11 : 5;
    for (int i = 0; i < n; ++i) {
      const int64_t ld = at[i] < lo ? lo : at[i];
      one(last, reg_bins, go_rice, ctx_sig, ctx_set, (int32_t)ld, mal);
    }
  }
};

}  // namespace

// table: 2 * 244 bin costs (ctu::tab_rdoq_bits()'s layout); counts[9], first_bad[12]
extern "C" __attribute__((visibility("default"))) void level_decision_compare(const uint32_t *table, double lambda, double error_scale, long long *counts,
                                                                              long long *first_bad)
{
  memcpy(ctu::tab_rdoq_bits(), table, 2 * 244 * sizeof(uint32_t));
  // the candidates above the exhaustive range: 6..70, and around every change of the escape code's length -- the Rice code's end
  // ((q = 5) << rice) and each prefix (q - 4 = 2^p, the cap at p = 12), for the level itself (bypass) and for level - 4 (regular)
  std::vector<uint32_t> large;
  for (uint32_t a = 6; a <= 70; ++a) large.push_back(a);
  for (int p = 1; p <= 14; ++p)
    for (int r = 0; r <= 3; ++r) {
      const uint32_t base = ((1u << p) + 4) << r;
      for (uint32_t d : {0u, 1u, 4u, 5u}) large.push_back(base + d);
    }
  for (uint32_t a : {32766u, 32767u, 32768u, 65535u, 131000u}) large.push_back(a);
  std::sort(large.begin(), large.end());
  large.erase(std::unique(large.begin(), large.end()), large.end());

  sweep S;
  S.counts = counts; S.first_bad = first_bad;
  S.E.st = nullptr; S.E.lambda = lambda; S.E.error_scale = error_scale; S.E.q = 0;
  for (int t = 0; t < 2; ++t) {
    S.E.t = t;
    const int n_sig = t ? 8 : 12, n_set = t ? 11 : 21;          // ctx_sig 0..11 / 0..7; ctx_set 0 (last) and 1..20 / 1..10
    for (int q_bits = 14; q_bits <= 20; ++q_bits) {
      S.E.q_bits = q_bits;
      for (int last = 0; last < 2; ++last)
        for (uint32_t reg_bins = 0; reg_bins <= 4; reg_bins += 4)
          for (int go_rice = 0; go_rice < 4; ++go_rice) {
            // candidates 0..5: every context pair
            for (int ctx_sig = 0; ctx_sig < n_sig; ++ctx_sig)
              for (int ctx_set = 0; ctx_set < n_set; ++ctx_set)
                for (uint32_t mal = 0; mal <= 5; ++mal) S.interval(last, reg_bins, go_rice, ctx_sig, ctx_set, mal, true);
            // larger ones: every context of either kind, side by side
            for (int k = 0; k < n_set; ++k)
              for (uint32_t mal : large) S.interval(last, reg_bins, go_rice, k % n_sig, k, mal, false);
          }
    }
  }
}
