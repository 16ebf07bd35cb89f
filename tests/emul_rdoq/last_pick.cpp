// rq_last_lower / rq_last_pick of uvg266_amd/csrc/ctu_core.h -- the choice among a group's sixteen totals in the device RDOQ's
// last-position search, a reduction -- compiled for the host and compared with the reference's walk (rdo.c:1805-1825): positions in
// descending order, a candidate's total taken when it is strictly below the best cost so far.  The reduction runs in the order of the
// device's lanes (neighbour, pair, mirrored half, mirrored row).  Two mutants run beside it: one that prefers the lowest k among
// equal totals, one that takes <= against the incoming best_cost; the test asserts that both are caught.  Built by
// tests/test_rdoq_last_pick.py itself (into pytest's temporary directory).
#include <cstdint>
#include <cstring>
#include "ctu_core.h"

namespace {

uint64_t bits_of(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }

struct rng {
  uint64_t s;
  uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
  unsigned below(unsigned n) { return (unsigned)((next() >> 20) % n); }
};

struct choice { int k_p1; double best; };

// the reference's walk
choice walk(const double *total, unsigned cand, double best_cost)
{
  choice c = {0, best_cost};
  for (int k = 15; k >= 0; --k)
    if ((cand >> k & 1u) && total[k] < c.best) { c.k_p1 = k + 1; c.best = total[k]; }
  return c;
}

// the device's formulation: every lane enters its total (best_cost where it is no candidate), four exchanges leave the minimum in
// every lane, the candidates at the minimum are collected, rq_last_pick chooses.  mutant 1: the lowest k among equals; 2: <=
choice reduce(const double *total, unsigned cand, double best_cost, int mutant, bool *lanes_agree)
{
  double m[16], x[16];
  for (int i = 0; i < 16; ++i) m[i] = (cand >> i & 1u) ? total[i] : best_cost;
  for (int round = 0; round < 4; ++round) {
    for (int i = 0; i < 16; ++i) {
      const int from = round == 0 ? i ^ 1 : round == 1 ? i ^ 2 : round == 2 ? (i & 8) | (7 - (i & 7)) : 15 - i;
      x[i] = ctu::rq_last_lower(m[i], m[from]);
    }
    memcpy(m, x, sizeof m);
  }
  for (int i = 1; i < 16; ++i) if (bits_of(m[i]) != bits_of(m[0]) && !(m[i] == 0 && m[0] == 0)) *lanes_agree = false;
  unsigned at_min = 0;
  for (int i = 0; i < 16; ++i) at_min |= (unsigned)((cand >> i & 1u) && total[i] == m[i]) << i;
  int pick;
  if (mutant == 1) pick = (m[0] < best_cost && at_min) ? __builtin_ctz(at_min) + 1 : 0;
  else if (mutant == 2) pick = (m[0] <= best_cost && at_min) ? 32 - __builtin_clz(at_min) : 0;
  else pick = ctu::rq_last_pick(m[0], at_min, best_cost);
  const choice c = {pick, pick ? m[0] : best_cost};
  return c;
}

bool same(const choice &a, const choice &b) { return a.k_p1 == b.k_p1 && a.best == b.best; }

}  // namespace

// counts[32]: 0 cases, 1 cases where the reduction differs from the walk (or its lanes disagree), 2 best_cost stays, 3 a candidate
// wins, 4 ... that is the highest of several equal minimal totals, 5 the candidates' minimum equals the incoming best_cost (and
// loses), 6 no candidate, 7 one candidate, 8 cases that catch the lowest-k mutant, 9 ... the <= mutant, 10 + kstop: cases by kstop,
// 26 the winner is not the highest candidate.  first_bad[19]: cand, best_cost, the sixteen totals, kstop
extern "C" __attribute__((visibility("default"))) void last_pick_compare(uint64_t seed, long long cases, long long *counts, double *first_bad)
{
  rng R = {seed * 0x9E3779B97F4A7C15ull + 1};
  for (long long c = 0; c < cases; ++c) {
    double total[16];
    // totals: a few values only (built to tie), or spread out; costs are non-negative sums of squares and bit costs times lambda
    const int kind = (int)R.below(4);
    const unsigned vals = kind == 0 ? 2 : kind == 1 ? 4 : kind == 2 ? 16 : 1u << 20;
    for (int i = 0; i < 16; ++i) total[i] = 1000.0 + 0.37 * R.below(vals);
    // the levels of the group: none, one, few, many; the walk ends at the highest level above 1 (kstop)
    const int dens = (int)R.below(5);
    unsigned m_nz = 0, m_gt1 = 0;
    if (dens == 1) m_nz = 1u << R.below(16);
    else if (dens >= 2) for (int i = 0; i < 16; ++i) m_nz |= (unsigned)(R.below(dens == 2 ? 5 : dens == 3 ? 2 : 1) == 0) << i;
    if (R.below(2)) for (int i = 0; i < 16; ++i) m_gt1 |= (m_nz >> i & 1u) && R.below(4) == 0 ? 1u << i : 0u;
    if (m_nz && R.below(8) == 0) m_gt1 = 1u << (31 - __builtin_clz(m_nz));          // (the top level itself: one candidate)
    const int kstop = m_gt1 ? 31 - __builtin_clz(m_gt1) : 0;
    const unsigned cand = m_nz >> kstop << kstop;
    // the incoming best cost: below everything, above everything, in between, or exactly one of the totals
    const int bk = (int)R.below(4);
    const double best_cost = bk == 0 ? 999.0 : bk == 1 ? 1.0e9 : bk == 2 ? 1000.0 + 0.37 * R.below(vals) + 0.1 : total[R.below(16)];

    const choice w = walk(total, cand, best_cost);
    bool agree = true;
    const choice r = reduce(total, cand, best_cost, 0, &agree), lo = reduce(total, cand, best_cost, 1, &agree), le = reduce(total, cand, best_cost, 2, &agree);
    ++counts[0];
    if (!same(w, r) || !agree) {
      if (counts[1] == 0) {
        first_bad[0] = cand; first_bad[1] = best_cost; first_bad[18] = kstop;
        memcpy(first_bad + 2, total, sizeof total);
      }
      ++counts[1];
    }
    double lowest = 1.0e300;
    int at_lowest = 0;
    for (int i = 0; i < 16; ++i) if (cand >> i & 1u) {
      if (total[i] < lowest) { lowest = total[i]; at_lowest = 0; }
      at_lowest += total[i] == lowest;
    }
    counts[2] += w.k_p1 == 0;
    counts[3] += w.k_p1 != 0;
    counts[4] += w.k_p1 != 0 && at_lowest > 1;
    counts[5] += cand != 0 && lowest == best_cost;
    counts[6] += cand == 0;
    counts[7] += cand != 0 && (cand & (cand - 1)) == 0;
    counts[8] += !same(w, lo);
    counts[9] += !same(w, le);
    ++counts[10 + kstop];
    counts[26] += w.k_p1 != 0 && w.k_p1 != 32 - __builtin_clz(cand);
  }
}
