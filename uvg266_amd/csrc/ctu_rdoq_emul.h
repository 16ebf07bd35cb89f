// The host emulation's uvg_rdoq (rdo.c:1449-1870) -- what rdoq_wave is in a build for the host (one emulated lane: tests/emul/).
// Included by ctu_core.h, inside namespace ctu, where the device build has its own rdoq_wave; the kernels never see this file.
// This is the reference's walk, position by position; the device decides a group's positions by a fixed-point iteration over the
// lanes' registers.  So the CPU tests hold the logic around RDOQ to the reference, and the GPU tests the device's formulation.
#pragma once
#if defined(CTU_RDOQ_START_STATS)
// tests/test_rdoq_start.py only (the test builds tests/emul/ctu_emul.cpp with this macro; no other build defines it).  Beside the
// walk, a plain transcription of the DEVICE's fixed point -- rdoq_wave's passes of up to four groups of a diagonal, the 4x4 leaf's one
// group with every position's own "regular" -- run from four starts: the candidates, rq_start_level's guess as the device places
// it, all zeros, and a seeded random start <= candidate.  Every start has to end at the walk's levels; the rounds are counted.
// Index of a block's class: 2 * (log2 size - 2) + (chroma ? 1 : 0).
struct rq_start_stats {
  int64_t passes, rounds[4], mismatches, zero_kept1, one_took0, last_cand1, passes_of[3], slow_groups;
};
struct rq_start_pass {
  int next_top, ng, on;                   // the group that opens the next pass; this pass's groups; decided by the fixed point
  int16_t want[4][16];                    // its groups' levels as the iteration leaves them (row r: group top - r)
};
inline rq_start_stats g_rq_start[8];
inline uint32_t g_rq_start_seed = 1;
extern "C" __attribute__((visibility("default"), used)) inline void ctu_emul_rdoq_start_stats(int64_t *out, int reset)
{
  if (out) memcpy(out, g_rq_start, sizeof g_rq_start);
  if (reset) { memset(g_rq_start, 0, sizeof g_rq_start); g_rq_start_seed = 1; }
}
struct rq_start_cand { int32_t level_double; int mal; };
CTU_DEV rq_start_cand rq_start_candidate(const rdoq_env &E, int32_t q, int coef)
{
  const int cap_half = 1 << (E.q_bits - 1);
  const int64_t prod = (int64_t)iabs_(coef) * q;
  const int32_t cap = 0x7fffffff - cap_half;
  rq_start_cand c;
  c.level_double = (int32_t)(prod < cap ? prod : cap);
  c.mal = (int)((uint32_t)(c.level_double + cap_half) >> E.q_bits);
  return c;
}
// one group from one start, in place (the group's positions of dst are undecided: they are put back as they were).  pass_regular:
// the pass's flag (n >= 8); n == 4: every position's own, from the bins the current levels later in scan order spend.
// -> rounds, the confirming one included; lev_out: the levels at the fixed point; start_out: the start.
inline int rq_start_iterate(const rdoq_env &E, int32_t q, const uint16_t *scan, const int16_t *coef, int16_t *dst, int n, int l2, int color, int cg,
                            int last_scanpos, bool pass_regular, int start, int16_t *lev_out, int16_t *start_out)
{
  int16_t keep[16], lev[16], nxt[16];
  for (int k = 0; k < 16; ++k) {
    const int scanpos = cg * 16 + k, blk = scan[scanpos];
    const rq_start_cand c = rq_start_candidate(E, q, coef[blk]);
    const bool mine = scanpos <= last_scanpos, is_last = scanpos == last_scanpos;
    keep[k] = dst[blk];
    int s = c.mal;
    if (start == 1) {
      const int g = rq_start_level(E, color, blk & (n - 1), blk >> l2, c.level_double, c.mal);
      s = (is_last || !(n == 4 || pass_regular)) ? c.mal : g;      // (rdoq_wave's pass without regular bins starts from the candidates)
    }
    if (start == 2) s = 0;
    if (start == 3) { g_rq_start_seed = g_rq_start_seed * 1664525u + 1013904223u; s = (int)((g_rq_start_seed >> 8) % (uint32_t)(c.mal + 1)); }
    lev[k] = (int16_t)(mine ? s : 0);
    start_out[k] = lev[k];
    dst[blk] = lev[k];
  }
  int rounds = 0;
  for (;;) {
    bool changed = false;
    ++rounds;
    for (int k = 0; k < 16; ++k) {
      const int scanpos = cg * 16 + k, blk = scan[scanpos];
      nxt[k] = lev[k];
      if (scanpos > last_scanpos) continue;
      const rq_start_cand c = rq_start_candidate(E, q, coef[blk]);
      const bool is_last = scanpos == last_scanpos;
      bool regular = pass_regular;
      if (n == 4) {
        int spent = 0;
        for (int j = k + 1; j < 16 && j <= last_scanpos; ++j) spent += (lev[j] < 2 ? lev[j] : 3) + (j == last_scanpos ? 0 : 1);
        regular = 28 - spent >= 4;
      }
      int go_rice = 0;
      if (regular && k != 15 && !is_last) {
        const int nb = scan[scanpos + 1];
        go_rice = go_rice_par(template_abs_sum(coef, 4, nb & (n - 1), nb >> l2, n));
      }
      const double c0 = (double)c.level_double * (double)c.level_double * E.error_scale;
      const rdoq_pos r = rdoq_decide_at(E, (const int16_t *)dst, n, color, blk & (n - 1), blk >> l2, is_last, regular, go_rice, c0, c.level_double, (uint32_t)c.mal);
      nxt[k] = (int16_t)r.level;
      changed |= nxt[k] != lev[k];
    }
    for (int k = 0; k < 16; ++k) { lev[k] = nxt[k]; dst[scan[cg * 16 + k]] = lev[k]; }
    if (!changed || rounds > 64) break;
  }
  for (int k = 0; k < 16; ++k) { lev_out[k] = lev[k]; dst[scan[cg * 16 + k]] = keep[k]; }
  return rounds;
}
// at a group the walk is about to enter: where it opens a pass, the pass as the device forms it
inline void rq_start_open(rq_start_pass &HS, const rdoq_env &E, int32_t q, const uint16_t *scan, const int16_t *coef, int16_t *dst, int n, int l2, int color,
                          int cgs, int last_scanpos, uint32_t reg_bins)
{
  if (cgs != HS.next_top) return;
  rq_start_stats &T = g_rq_start[2 * (l2 - 2) + (color ? 1 : 0)];
  const int cgw = n >> 2, top = cgs, ftop = scan[top * 16];
  const int dg = ((ftop & (n - 1)) >> 2) + ((ftop >> l2) >> 2);
  int ng = top - rdoq_diag_start(cgw, dg) + 1 < 4 ? top - rdoq_diag_start(cgw, dg) + 1 : 4;
  const bool regular = reg_bins >= 4;
  bool fast = !regular;
  if (n == 4) fast = true;                                  // the leaf: always the fixed point
  else if (regular) {
    int bound[4] = {0, 0, 0, 0};
    for (int r = 0; r < ng; ++r)
      for (int k = 0; k < 16; ++k) {
        const int scanpos = (top - r) * 16 + k;
        if (scanpos > last_scanpos) continue;
        const int mal = rq_start_candidate(E, q, coef[scan[scanpos]]).mal;
        bound[r] += (mal < 2 ? mal : 3) + (scanpos == last_scanpos ? 0 : 1);
      }
    fast = (int)reg_bins - (bound[0] + bound[1] + bound[2] + bound[3]) >= 4;
    if (!fast && ng > 1) { ng = 1; fast = (int)reg_bins - bound[0] >= 4; }
  }
  HS.ng = ng; HS.on = fast; HS.next_top = top - ng;
  if (!fast) { T.slow_groups += 1; return; }
  int rounds[4] = {0, 0, 0, 0};
  for (int r = 0; r < ng; ++r) {
    int16_t start_lv[16], got[16];
    for (int s = 0; s < 4; ++s) {
      const int k = rq_start_iterate(E, q, scan, coef, dst, n, l2, color, top - r, last_scanpos, regular, s, s == 0 ? HS.want[r] : got, start_lv);
      rounds[s] = k > rounds[s] ? k : rounds[s];
      if (s && memcmp(got, HS.want[r], sizeof got)) T.mismatches += 1;
      if (s == 1)
        for (int j = 0; j < 16; ++j) {
          const int scanpos = (top - r) * 16 + j;
          if (scanpos > last_scanpos) continue;
          const int mal = rq_start_candidate(E, q, coef[scan[scanpos]]).mal;
          if (mal == 1 && scanpos == last_scanpos) T.last_cand1 += 1;
          if (mal == 1 && start_lv[j] == 0 && got[j] == 1 && scanpos != last_scanpos) T.zero_kept1 += 1;
          if (mal == 1 && start_lv[j] == 1 && got[j] == 0) T.one_took0 += 1;
        }
    }
  }
  T.passes += 1;
  for (int s = 0; s < 4; ++s) T.rounds[s] += rounds[s];
  T.passes_of[rounds[1] < 3 ? rounds[1] - 1 : 2] += 1;
}
// behind a group's positions, before its zero-out: the walk's levels against the iteration's
inline void rq_start_check(const rq_start_pass &HS, const uint16_t *scan, const int16_t *dst, int l2, int color, int cgs)
{
  if (!HS.on) return;
  const int r = HS.next_top + HS.ng - cgs;
  for (int k = 0; k < 16; ++k)
    if (dst[scan[cgs * 16 + k]] != HS.want[r][k]) { g_rq_start[2 * (l2 - 2) + (color ? 1 : 0)].mismatches += 1; return; }
}
#endif
// uvg_rdoq as the reference walks it, of an n x n block (square: no sqrt2 scaling), no LFNST / MTS /
// sign hiding.  coef -> levels in dst (both n * n, raster).  root_cbf: "no coefficients" of a luma block is priced with the root cbf
// (a block of an inter CU, rdo.c:1774).  Returns whether any level survived.
CTU_NOINLINE CTU_DEV int rdoq_serial(const uint8_t *st, const uint16_t *scan, scratch *W, const int16_t *coef, int16_t *dst, int n, int color, int cbf_u,
                        int root_cbf, int qp_scaled, double lambda, int bitdepth)
{
  const int l2 = ilog2_dev(n);
  rdoq_env E;
  E.st = st; E.t = color ? 1 : 0; E.lambda = lambda;
  const int transform_shift = 15 - bitdepth - l2;
  uint32_t reg_bins = (uint32_t)(n * n * 28) >> 4;
  E.q_bits = 14 + qp_scaled / 6 + transform_shift;
  const int32_t q = kQuantScales[qp_scaled % 6];
  // scale = 32768 * 2^(-2 * transform_shift) (rdo.c:1527: pow() of an integer exponent, exact), error_scale = scale / q / q
  double scale = 32768;
  scale = transform_shift >= 0 ? scale / kPow2[2 * transform_shift] : scale * kPow2[-2 * transform_shift];
  E.error_scale = scale / q / q;
  double *cost_coeff = W->cost_coeff, *cost_sig = W->cost_sig, *cost_coeff0 = W->cost_coeff0;
  double block_uncoded_cost = 0, base_cost = 0;
  const int cg_num = (n * n) >> 4, cgw = n >> 2;
  double cost_cg_sig[64];
  uint8_t cg_flag[64];
  for (int i = 0; i < cg_num; ++i) cg_flag[i] = 0;
  for (int i = 0; i < n * n; ++i) dst[i] = 0;
  int ctx_set = 0, temp_diag = -1, temp_sum = -1;
  int go_rice = 0;
  int cg_last_scanpos = -1, last_scanpos = -1;
  const int cap_half = 1 << (E.q_bits - 1);
  int cgs;
  for (cgs = cg_num - 1; cgs >= 0; cgs--) {
    for (int sp = 15; sp >= 0; sp--) {
      const int scanpos = cgs * 16 + sp;
      const int blkpos = scan[scanpos];
      const int64_t prod = (int64_t)iabs_((int)coef[blkpos]) * q;
      const int32_t cap = 0x7fffffff - cap_half;
      const int32_t level_double = (int32_t)(prod < cap ? prod : cap);
      const uint32_t max_abs_level = (uint32_t)(level_double + cap_half) >> E.q_bits;
      const double err = (double)level_double;
      cost_coeff0[scanpos] = err * err * E.error_scale;
      dst[blkpos] = (int16_t)max_abs_level;
      if (max_abs_level > 0) { last_scanpos = scanpos; cg_last_scanpos = cgs; break; }
      block_uncoded_cost += cost_coeff0[scanpos];
      base_cost += cost_coeff0[scanpos];
    }
    if (last_scanpos != -1) break;
  }
  if (last_scanpos == -1) return 0;
  for (; cgs >= 0; cgs--) cost_cg_sig[cgs] = 0;
#if defined(CTU_RDOQ_START_STATS)
  rq_start_pass HS;
  HS.next_top = cg_last_scanpos; HS.ng = 0; HS.on = 0;
#endif

  for (cgs = cg_last_scanpos; cgs >= 0; cgs--) {
#if defined(CTU_RDOQ_START_STATS)
    rq_start_open(HS, E, q, scan, coef, dst, n, l2, color, cgs, last_scanpos, reg_bins);
#endif
    // the group's raster index = position of its first coefficient / 4
    const int first = scan[cgs * 16];
    const int cg_pos_x = (first & (n - 1)) >> 2, cg_pos_y = (first >> l2) >> 2;
    const int cg_blkpos = cg_pos_y * cgw + cg_pos_x;
    double rd_coded = 0, rd_uncoded = 0, rd_sig = 0, rd_sig0 = 0;
    int nnz_before_pos0 = 0;
    for (int sp = 15; sp >= 0; sp--) {
      const int scanpos = cgs * 16 + sp;
      if (scanpos > last_scanpos) continue;
      const int blkpos = scan[scanpos];
      const int64_t prod = (int64_t)iabs_((int)coef[blkpos]) * q;
      const int32_t cap = 0x7fffffff - cap_half;
      const int32_t level_double = (int32_t)(prod < cap ? prod : cap);
      const uint32_t max_abs_level = (uint32_t)(level_double + cap_half) >> E.q_bits;
      dst[blkpos] = (int16_t)max_abs_level;
      const double err = (double)level_double;
      cost_coeff0[scanpos] = err * err * E.error_scale;
      block_uncoded_cost += cost_coeff0[scanpos];
      {
        const int pos_y = blkpos >> l2, pos_x = blkpos - (pos_y << l2);
        int ctx_sig = 0;
        if (scanpos != last_scanpos) ctx_sig = sig_ctx_abs(dst, pos_x, pos_y, n, color, &temp_diag, &temp_sum);
        if (temp_diag != -1)
          ctx_set = ((temp_sum < 4 ? temp_sum : 4) + 1) +
                    (!temp_diag ? ((color == 0) ? 15 : 5) : (color == 0) ? (temp_diag < 3 ? 10 : (temp_diag < 10 ? 5 : 0)) : 0);
        else ctx_set = 0;
        if (reg_bins < 4) go_rice = go_rice_par(template_abs_sum(dst, 0, pos_x, pos_y, n));
        const int level = (int)coded_level(E, &cost_coeff[scanpos], cost_coeff0[scanpos], &cost_sig[scanpos], level_double, max_abs_level,
                                           scanpos == last_scanpos ? 0 : ctx_sig, ctx_set, go_rice, reg_bins, scanpos == last_scanpos);
        dst[blkpos] = (int16_t)level;
        base_cost += cost_coeff[scanpos];
        if ((scanpos % 16 == 0) && scanpos > 0) go_rice = 0;
        else if (reg_bins >= 4) {
          reg_bins -= (uint32_t)((level < 2 ? level : 3) + (scanpos != last_scanpos));
          go_rice = go_rice_par(template_abs_sum(coef, 4, pos_x, pos_y, n));       // sic: the INPUT coefficients (rdo.c:1697)
        }
      }
      rd_sig += cost_sig[scanpos];
      if (sp == 0) rd_sig0 = cost_sig[scanpos];
      if (dst[blkpos]) {
        cg_flag[cg_blkpos] = 1;
        rd_coded += cost_coeff[scanpos] - cost_sig[scanpos];
        rd_uncoded += cost_coeff0[scanpos];
        if (sp != 0) nnz_before_pos0++;
      }
    }
#if defined(CTU_RDOQ_START_STATS)
    rq_start_check(HS, scan, dst, l2, color, cgs);
#endif
    if (cgs) {
      unsigned right = 0, lower = 0;
      if (cg_pos_x + 1 < cgw) right = cg_flag[cg_blkpos + 1];
      if (cg_pos_y + 1 < cgw) lower = cg_flag[cg_blkpos + cgw];
      const int o_grp = M_SIGGRP + (E.t ? 2 : 0) + ((right || lower) ? 1 : 0);
      if (cg_flag[cg_blkpos] == 0) {
        cost_cg_sig[cgs] = lambda * rbits(E, o_grp, 0);
        base_cost += cost_cg_sig[cgs] - rd_sig;
      } else if (cgs < cg_last_scanpos) {
        if (nnz_before_pos0 == 0) { base_cost -= rd_sig0; rd_sig -= rd_sig0; }
        double cost_zero_cg = base_cost;
        cost_cg_sig[cgs] = lambda * rbits(E, o_grp, 1);
        base_cost += cost_cg_sig[cgs];
        cost_zero_cg += lambda * rbits(E, o_grp, 0);
        cost_zero_cg += rd_uncoded;
        cost_zero_cg -= rd_coded;
        cost_zero_cg -= rd_sig;
        if (cost_zero_cg < base_cost) {
          cg_flag[cg_blkpos] = 0;
          base_cost = cost_zero_cg;
          cost_cg_sig[cgs] = lambda * rbits(E, o_grp, 0);
          for (int sp = 15; sp >= 0; sp--) {
            const int scanpos = cgs * 16 + sp;
            const int blkpos = scan[scanpos];
            if (dst[blkpos]) { dst[blkpos] = 0; cost_coeff[scanpos] = cost_coeff0[scanpos]; cost_sig[scanpos] = 0; }
          }
        }
      }
    } else {
      cg_flag[cg_blkpos] = 1;
    }
  }

  double best_cost;
  int best_last_idx_p1 = 0;
  {
    const int o_cbf = color == 0 ? (root_cbf ? 243 : M_CBF_LUMA) : color == 1 ? M_CBF_CB : M_CBF_CR + (cbf_u ? 1 : 0);
    best_cost = block_uncoded_cost + lambda * rbits(E, o_cbf, 0);
    base_cost += lambda * rbits(E, o_cbf, 1);
  }
  // calc_last_bits (rdo.c:664-700)
  int32_t last_x_bits[32], last_y_bits[32];
  {
    const int prefix_ctx[8] = {0, 0, 0, 3, 6, 10, 15, 21};
    const int off = E.t ? 0 : prefix_ctx[l2];
    const int sh = E.t ? clampi(n >> 3, 0, 2) : ((l2 + 1) >> 2);
    int32_t bx = 0, by = 0;
    int ctx;
    for (ctx = 0; ctx < group_idx(n - 1); ctx++) {
      const int o = off + (ctx >> sh);
      const int mx = M_LASTX + (E.t ? 20 : 0) + o, my = M_LASTY + (E.t ? 20 : 0) + o;
      last_x_bits[ctx] = bx + rbits(E, mx, 0); bx += rbits(E, mx, 1);
      last_y_bits[ctx] = by + rbits(E, my, 0); by += rbits(E, my, 1);
    }
    last_x_bits[ctx] = bx; last_y_bits[ctx] = by;
  }
  int found_last = 0;
  for (cgs = cg_last_scanpos; cgs >= 0; cgs--) {
    const int first = scan[cgs * 16];
    const int cg_blkpos = ((first >> l2) >> 2) * cgw + ((first & (n - 1)) >> 2);
    base_cost -= cost_cg_sig[cgs];
    if (cg_flag[cg_blkpos]) {
      for (int sp = 15; sp >= 0; sp--) {
        const int scanpos = cgs * 16 + sp;
        if (scanpos > last_scanpos) continue;
        const int blkpos = scan[scanpos];
        if (dst[blkpos]) {
          const int pos_y = blkpos >> l2, pos_x = blkpos - (pos_y << l2);
          const int cx = group_idx(pos_x), cy = group_idx(pos_y);
          double cl = last_x_bits[cx] + last_y_bits[cy];
          if (cx > 3) cl += 32768 * ((cx - 2) >> 1);
          if (cy > 3) cl += 32768 * ((cy - 2) >> 1);
          const double cost_last = lambda * cl;
          const double total = base_cost + cost_last - cost_sig[scanpos];
          if (total < best_cost) { best_last_idx_p1 = scanpos + 1; best_cost = total; }
          if (dst[blkpos] > 1) { found_last = 1; break; }
          base_cost -= cost_coeff[scanpos];
          base_cost += cost_coeff0[scanpos];
        } else {
          base_cost -= cost_sig[scanpos];
        }
      }
      if (found_last) break;
    }
  }
  int any = 0;
  for (int scanpos = 0; scanpos < best_last_idx_p1; scanpos++) {
    const int b = scan[scanpos], level = dst[b];
    any |= level;
    dst[b] = (int16_t)((coef[b] < 0) ? -level : level);
  }
  for (int scanpos = best_last_idx_p1; scanpos <= last_scanpos; scanpos++) dst[scan[scanpos]] = 0;
  return any != 0;
}

// what rdoq_wave is on the host: the serial walk.  Result: V->rq_i[1] = whether any level survived; levels in dst.
template <typename PX> CTU_NOINLINE CTU_DEV void rdoq_wave(lds<PX> *S, scratch *W, const int16_t *coef, int16_t *dst, int n, int color, int cbf_u, int qp_scaled,
                                              double lambda, int bitdepth)
{
  wctx *const V = wv_of(S);
  V->rq_i[1] = rdoq_serial(S->rdoq_state, scan_of(S, ilog2_dev(n)), W, coef, dst, n, color, cbf_u, CTU_RQ_ROOT(V), qp_scaled, lambda, bitdepth);
}
