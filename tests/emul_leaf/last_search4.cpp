// lf_last_search of uvg266_amd/csrc/ctu_leaf4.h -- the last-position search of a 4x4 block down the sixteen lanes of its row --
// replayed on the host for one row and compared with the serial walk the leaf ran before it (rdo.c:1805-1825 over one group): the
// operands gathered into scan order (lane k takes raster lane SCAN[k]), the candidate mask from the ballots of "level != 0" and
// "level > 1", fifteen rounds of base_cost a lane down (lane 15 keeps the incoming value), the sixteen totals, then rq_last_lower /
// rq_last_pick of ctu_core.h, compiled here for the host, in the order of the device's exchanges.  The header with the device's own
// function is device only (DPP, ds_bpermute): this file restates its steps lane by lane and shares the two functions of the choice.
// Two mutants run beside it: the lowest position among equal totals, and <= against the incoming best cost.  Built by
// tests/test_leaf_last_search.py itself (into pytest's temporary directory).
#include <cstdint>
#include <cstring>
#include "ctu_core.h"

namespace {

const int SCAN[16] = {0, 4, 1, 8, 5, 2, 12, 9, 6, 3, 13, 10, 7, 14, 11, 15};       // raster position of scan index k (up-right diagonals)

uint64_t bits_of(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
bool same_bits(double a, double b) { return bits_of(a) == bits_of(b); }

struct rng {
  uint64_t s;
  uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
  unsigned below(unsigned n) { return (unsigned)((next() >> 20) % n); }
};

// a block as the leaf's lanes hold it behind the fixed point, by RASTER position: the level, the level-0 cost, the coded cost, the
// significance flag's cost, the bits of the position as the last one (0 without a level); beyond last_sp: level 0, cc = cs = 0
struct block { int lev[16]; double c0[16], cc[16], cs[16], klast[16]; int last_sp; double base_cost, best_cost; };
struct result { int idx_p1; double best, base; bool base_read; };

// the serial walk: leaf_rdoq's loop over k = 15..0 on the owners' values, as it stood.  totals: every candidate's total (or null)
result walk(const block &B, double *totals)
{
  result R = {0, B.best_cost, B.base_cost, true};
  bool found_last = false;
  for (int k = 15; k >= 0; --k) {
    if (found_last || k > B.last_sp) continue;
    const int level = B.lev[SCAN[k]];
    const double s_ = B.cs[SCAN[k]];
    if (level) {
      const double total = R.base + B.klast[SCAN[k]] - s_;
      if (totals) totals[k] = total;
      if (total < R.best) { R.idx_p1 = k + 1; R.best = total; }
      if (level > 1) { found_last = true; continue; }
      R.base -= B.cc[SCAN[k]];
      R.base += B.c0[SCAN[k]];
    } else {
      R.base -= s_;
    }
  }
  R.base_read = !found_last;          // after a level above 1 the walk's base_cost is what step kstop found: nobody reads it
  return R;
}

// the lanes' form.  mutant 1: the lowest position among equal totals; 2: <= against the incoming best cost
result lanes(const block &B, int mutant, bool *lanes_agree)
{
  int klev[16];
  double kx[16], k0[16], kl[16], kcs[16];
  for (int k = 0; k < 16; ++k) {          // the owners choose, lane k takes raster lane SCAN[k]'s
    const int r = SCAN[k];
    klev[k] = B.lev[r];
    kx[k] = B.lev[r] ? B.cc[r] : B.cs[r];
    k0[k] = B.lev[r] ? B.c0[r] : 0.0;
    kl[k] = B.klast[r];
    kcs[k] = B.cs[r];
  }
  unsigned m_nz = 0, m_gt1 = 0;
  for (int k = 0; k < 16; ++k) { m_nz |= (unsigned)(klev[k] != 0) << k; m_gt1 |= (unsigned)(klev[k] > 1) << k; }
  const int kstop = m_gt1 ? 31 - __builtin_clz(m_gt1) : 0;
  const unsigned cand = m_nz >> kstop << kstop;
  double before[16], after[16], x[16];
  for (int k = 0; k < 16; ++k) { before[k] = B.base_cost; after[k] = B.base_cost - kx[k] + k0[k]; }
  for (int round = 0; round < 15; ++round) {
    for (int k = 0; k < 16; ++k) x[k] = k < 15 ? after[k + 1] : B.base_cost;          // row_shl:1, lane 15 keeps the incoming value
    for (int k = 0; k < 16; ++k) { before[k] = x[k]; after[k] = before[k] - kx[k] + k0[k]; }
  }
  double total[16], m[16];
  for (int k = 0; k < 16; ++k) { total[k] = before[k] + kl[k] - kcs[k]; m[k] = (cand >> k & 1u) ? total[k] : B.best_cost; }
  for (int round = 0; round < 4; ++round) {
    for (int i = 0; i < 16; ++i) {
      const int from = round == 0 ? i ^ 1 : round == 1 ? i ^ 2 : round == 2 ? (i & 8) | (7 - (i & 7)) : 15 - i;
      x[i] = ctu::rq_last_lower(m[i], m[from]);
    }
    memcpy(m, x, sizeof m);
  }
  for (int i = 1; i < 16; ++i) if (!same_bits(m[i], m[0]) && !(m[i] == 0 && m[0] == 0)) *lanes_agree = false;
  unsigned at_min = 0;
  for (int k = 0; k < 16; ++k) at_min |= (unsigned)((cand >> k & 1u) && total[k] == m[k]) << k;
  int pick;
  if (mutant == 1) pick = (m[0] < B.best_cost && at_min) ? __builtin_ctz(at_min) + 1 : 0;
  else if (mutant == 2) pick = (m[0] <= B.best_cost && at_min) ? 32 - __builtin_clz(at_min) : 0;
  else pick = ctu::rq_last_pick(m[0], at_min, B.best_cost);
  const result R = {pick, pick ? m[0] : B.best_cost, after[0], m_gt1 == 0};
  return R;
}

bool same(const result &a, const result &b) { return a.idx_p1 == b.idx_p1 && same_bits(a.best, b.best); }

}  // namespace

// counts[64]: 0 cases, 1 cases where the lanes' form differs from the walk (or its lanes disagree, or base_cost after step 0 differs
// where the walk reads it), 2 cases that catch the lowest-position mutant, 3 ... the <= mutant, 4 no level at all, 5 all levels 1,
// 6 the winner is the highest of several candidates with the same minimal total, 7 a candidate's total equals the incoming best cost
// (the lowest of them: it loses), 8 zeros between levels, 9 no level above 1, 10 a candidate wins, 11 best cost stays although there
// is a candidate, 12 base_cost after step 0 compared, 16 + last_sp, 32 + kstop (of the cases with a level above 1).
// first_bad[100]: last_sp, base_cost, best_cost, then lev / c0 / cc / cs / klast by raster position, then the two idx_p1
extern "C" __attribute__((visibility("default"))) void last_search4_compare(uint64_t seed, long long cases, long long *counts, double *first_bad)
{
  rng R = {seed * 0x9E3779B97F4A7C15ull + 1};
  for (long long c = 0; c < cases; ++c) {
    block B;
    // costs: sums of squares times a scale and bit counts times lambda, all >= 0.  Quarters from a small set (sums stay exact: built
    // to tie), or spread out (every addition rounds: the order of the operations shows)
    const int kind = (int)R.below(4);
    const unsigned vals = kind == 0 ? 2 : kind == 1 ? 5 : kind == 2 ? 64 : 1u << 20;
    const double unit = kind == 3 ? 0.37 / 1024 : 0.25;
    B.last_sp = (int)R.below(16);
    // the levels: none, a lone one, few, many, all; all of them 1, or some above 1
    const int dens = (int)R.below(6), big = (int)R.below(4);
    for (int k = 0; k < 16; ++k) {
      const int r = SCAN[k];
      bool nz = dens == 0 ? false : dens == 1 ? k == B.last_sp : dens == 2 ? R.below(5) == 0 : dens == 3 ? R.below(2) == 0 : dens == 4 ? R.below(8) != 0 : true;
      if (k == B.last_sp && dens && R.below(8)) nz = true;          // (the last candidate mostly keeps a level; it need not)
      int level = nz ? 1 : 0;
      if (nz && big == 1 && R.below(4) == 0) level = 2 + (int)R.below(3);
      if (nz && big == 2 && R.below(12) == 0) level = 2 + (int)R.below(300);
      if (nz && big == 3) level = 2;
      const bool mine = k <= B.last_sp;
      B.lev[r] = mine ? level : 0;
      B.c0[r] = unit * R.below(vals);
      B.cc[r] = mine ? unit * R.below(vals) : 0.0;
      B.cs[r] = mine ? unit * R.below(vals) : 0.0;
      B.klast[r] = B.lev[r] ? unit * R.below(vals) : 0.0;
    }
    B.base_cost = unit * (40 + R.below(vals));
    B.best_cost = 1.0e300;
    double totals[16];
    for (int k = 0; k < 16; ++k) totals[k] = -1;
    walk(B, totals);
    unsigned cand = 0;
    double lowest = 1.0e300;
    int at_lowest = 0;
    for (int k = 0; k < 16; ++k) if (totals[k] != -1) {
      cand |= 1u << k;
      if (totals[k] < lowest) { lowest = totals[k]; at_lowest = 0; }
      at_lowest += totals[k] == lowest;
    }
    // the incoming best cost: below everything, above everything, around the base cost, or exactly a candidate's total (mostly the lowest)
    const int bk = (int)R.below(5);
    int some = (int)R.below(16);
    while (cand && !(cand >> some & 1u)) some = (some + 1) & 15;
    B.best_cost = bk == 0 ? 0.0 : bk == 1 ? 1.0e9 : bk == 2 ? B.base_cost + unit * ((int)R.below(vals) - (int)(vals / 2)) + unit / 2
                : (cand ? (bk == 3 ? lowest : totals[some]) : B.base_cost);

    const result w = walk(B, nullptr);
    bool agree = true;
    const result r = lanes(B, 0, &agree), lo = lanes(B, 1, &agree), le = lanes(B, 2, &agree);
    ++counts[0];
    const bool base_differs = w.base_read != r.base_read || (w.base_read && !same_bits(w.base, r.base) && !(w.base == 0 && r.base == 0));
    if (!same(w, r) || !agree || base_differs) {
      if (counts[1] == 0) {
        first_bad[0] = B.last_sp; first_bad[1] = B.base_cost; first_bad[2] = B.best_cost;
        for (int i = 0; i < 16; ++i) { first_bad[3 + i] = B.lev[i]; first_bad[19 + i] = B.c0[i]; first_bad[35 + i] = B.cc[i]; first_bad[51 + i] = B.cs[i]; first_bad[67 + i] = B.klast[i]; }
        first_bad[83] = w.idx_p1; first_bad[84] = r.idx_p1;
      }
      ++counts[1];
    }
    unsigned m_nz = 0, m_gt1 = 0;
    for (int k = 0; k < 16; ++k) { m_nz |= (unsigned)(B.lev[SCAN[k]] != 0) << k; m_gt1 |= (unsigned)(B.lev[SCAN[k]] > 1) << k; }
    counts[2] += !same(w, lo);
    counts[3] += !same(w, le);
    counts[4] += m_nz == 0;
    counts[5] += m_nz != 0 && m_gt1 == 0;
    counts[6] += w.idx_p1 != 0 && at_lowest > 1;
    counts[7] += cand != 0 && lowest == B.best_cost;
    {
      const unsigned inside = m_nz ? ((1u << (31 - __builtin_clz(m_nz))) - 1) & ~((1u << __builtin_ctz(m_nz)) - 1) : 0;       // between the lowest and the highest level
      counts[8] += (inside & ~m_nz) != 0;
    }
    counts[9] += m_gt1 == 0;
    counts[10] += w.idx_p1 != 0;
    counts[11] += w.idx_p1 == 0 && cand != 0;
    counts[12] += w.base_read;
    ++counts[16 + B.last_sp];
    if (m_gt1) ++counts[32 + 31 - __builtin_clz(m_gt1)];
  }
}
