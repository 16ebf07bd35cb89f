// The host emulation's uvg_rdoq (rdo.c:1449-1870) -- what rdoq_wave is in a build for the host (one emulated lane: tests/emul/).
// Included by ctu_core.h, inside namespace ctu, where the device build has its own rdoq_wave; the kernels never see this file.
// The two are different formulations of the same walk (the device decides a group's positions by a fixed-point iteration over the
// lanes' registers), so the CPU tests check this one and the GPU tests the other.
//
// Same arithmetic as rdoq_serial, restructured around what is sequential in it:
//   * every position's quantisation candidates and its level-0 cost: one pass over the positions;
//   * a level decision reads only levels decided on later anti-diagonals (the context template looks right / down), so the <= 4
//     positions of one anti-diagonal of a 4x4 group are decided as a round whose levels appear together, 7 rounds per group -- as
//     long as the regular-bin budget cannot run out inside the group (an upper bound from the candidates says so) or has run out
//     for good; the one or two groups where it does run out are walked position by position;
//   * the double-precision sums the reference forms in scan order (base cost, group statistics), the group decision that compares
//     them, the final cbf / last-position search: from the group's staged costs, in the reference's order.
// Result: V->rq_i[1] = whether any level survived; levels in dst.  (RQ_T: the phase marks of the device's profile build, empty here;
// they stand where the device function has them.)
#pragma once
template <typename PX> CTU_NOINLINE CTU_DEV void rdoq_wave(lds<PX> *S, scratch *W, const int16_t *coef_, int16_t *dst_, int n, int color, int cbf_u, int qp_scaled,
                                              double lambda, int bitdepth)
{
  wctx *const V = wv_of(S);
  CTU_LDS const int16_t *const coef = LDSP(const int16_t, coef_);
  typename mg_ptr<PX, int16_t>::type const dst = MGP(PX, int16_t, dst_);
  const int l2 = ilog2_dev(n), nn = n * n, cgw = n >> 2;
  const uint16_t *scan = scan_of(S, l2);
  rdoq_env E;
  E.st = S->rdoq_state; E.t = color ? 1 : 0; E.lambda = lambda;
  const int transform_shift = 15 - bitdepth - l2;
  E.q_bits = 14 + qp_scaled / 6 + transform_shift;
  E.q = kQuantScales[qp_scaled % 6];
  double scale = 32768;
  scale = transform_shift >= 0 ? scale / kPow2[2 * transform_shift] : scale * kPow2[-2 * transform_shift];
  E.error_scale = scale / E.q / E.q;
  const bool small = V->rq_cc != nullptr;        // the per-position cost arrays are in LDS (this wave's depth has them)
  double *CC = small ? V->rq_cc : W->cost_coeff, *CS = small ? V->rq_cs : W->cost_sig, *C0 = W->cost_coeff0;
#define RQ_LD(p) (small ? *(p) : CTU_GLOAD(p))
  double *cost_cg_sig = (double *)V->t1;         // (the transform's other buffer: dead while a block is quantised; <= 64 groups)
  const int cap_half = 1 << (E.q_bits - 1);
  // ---- every position: candidate, level-0 cost; the last candidate in scan order ----
  int my_last = -1;
  PAR_FOR(sp, nn) {
    const int blk = scan[sp];
    const int64_t prod = (int64_t)iabs_((int)coef[blk]) * E.q;
    const int32_t cap = 0x7fffffff - cap_half;
    const int32_t level_double = (int32_t)(prod < cap ? prod : cap);
    const int mal = (int)((uint32_t)(level_double + cap_half) >> E.q_bits);
    const double err = (double)level_double;
    C0[sp] = err * err * E.error_scale;
    dst[blk] = (int16_t)mal;
    if (mal > 0 && sp > my_last) my_last = sp;
    if (sp < 64) V->cg_flag[sp] = 0;
  }
  const int last_scanpos = my_last;
  CTU_SYNC();
  if (last_scanpos < 0) { if (CTU_TID == 0) V->rq_i[1] = 0; CTU_SYNC(); return; }
  RQ_T(12);
  const int cg_last = last_scanpos >> 4;
  // lane 0's running sums (rdo.c:1556-1583: the positions behind the last candidate only add their level-0 cost)
  double block_uncoded_cost = 0, base_cost = 0;
  if (CTU_TID == 0) {
    for (int sp = nn - 1; sp > last_scanpos; --sp) { const double c = RQ_LD(&C0[sp]); block_uncoded_cost += c; base_cost += c; }
    for (int g = 0; g <= cg_last; ++g) cost_cg_sig[g] = 0;
    V->rq_i[4] = (int)((uint32_t)(nn * 28) >> 4);      // reg_bins
    V->rq_i[5] = 1;                                    // regular bins remain
  }
  CTU_SYNC();
  RQ_T(13);
  for (int cgs = cg_last; cgs >= 0; --cgs) {
    const int first = scan[cgs * 16];
    const int cg_pos_x = (first & (n - 1)) >> 2, cg_pos_y = (first >> l2) >> 2;
    const int cg_blkpos = cg_pos_y * cgw + cg_pos_x;
    int reg_bins = V->rq_i[4];
    const int regular = V->rq_i[5];
    // can the regular-bin budget run out inside this group?  (a position spends at most min(candidate, 2 -> 3) + 1 bins)
    int fast = !regular;
    if (regular) {
      int bound = 0;
      PAR_FOR(sp, 16) {
        const int scanpos = cgs * 16 + sp;
        if (scanpos <= last_scanpos) { const int mal = dst[scan[scanpos]]; bound += (mal < 2 ? mal : 3) + (scanpos != last_scanpos); }
      }
      fast = reg_bins - bound >= 4;
    }
    if (fast) {
      // a position can be decided once the positions of its context template that may keep a level are decided; the others hold
      // their final 0 already.  Lanes 0..15 own the group's scan positions; the rounds follow the chains of candidates (<= 7).
      {
        unsigned nz = 0, decided = 0, all = 0;
        for (int sp = 0; sp < 16; ++sp) { const int scanpos = cgs * 16 + sp; if (scanpos <= last_scanpos) { all |= 1u << sp; if (dst[scan[scanpos]] > 0) nz |= 1u << sp; } }
        decided = ~all & 0xffffu;
        while (decided != 0xffffu) {
          const unsigned before = decided;
          int16_t newlev[16];
          for (int sp = 0; sp < 16; ++sp) {
            if ((before >> sp) & 1) continue;
            if (((unsigned)S->deps4[sp] & nz) & ~before) continue;
            const int scanpos = cgs * 16 + sp, blk = scan[scanpos];
            int go_rice = 0;
            if (regular && sp != 15 && scanpos != last_scanpos) {
              const int nb = scan[scanpos + 1];
              go_rice = go_rice_par(template_abs_sum(coef, 4, nb & (n - 1), nb >> l2, n));
            }
            int mal;
            const rdoq_pos r = rdoq_decide(E, coef, dst, n, l2, color, blk, scanpos == last_scanpos, regular != 0, go_rice, RQ_LD(&C0[scanpos]), &mal);
            newlev[sp] = (int16_t)r.level;
            V->rq_stage[sp] = r.cc; V->rq_stage[16 + sp] = r.cs;
            decided |= 1u << sp;
          }
          for (int sp = 0; sp < 16; ++sp) if (((decided & ~before) >> sp) & 1) dst[scan[cgs * 16 + sp]] = newlev[sp];    // a round's levels appear together
        }
      }
    } else if (CTU_TID == 0) {
      // the budget may run out in this group: position by position, exactly as the reference walks
      int go_rice = 0;
      for (int sp = 15; sp >= 0; --sp) {
        const int scanpos = cgs * 16 + sp;
        if (scanpos > last_scanpos) continue;
        const int blk = scan[scanpos];
        int mal;
        const rdoq_pos r = rdoq_decide(E, coef, dst, n, l2, color, blk, scanpos == last_scanpos, reg_bins >= 4, go_rice, RQ_LD(&C0[scanpos]), &mal);
        dst[blk] = (int16_t)r.level;
        V->rq_stage[sp] = r.cc; V->rq_stage[16 + sp] = r.cs;
        if ((scanpos % 16 == 0) && scanpos > 0) go_rice = 0;
        else if (reg_bins >= 4) {
          reg_bins -= (r.level < 2 ? r.level : 3) + (scanpos != last_scanpos);
          go_rice = go_rice_par(template_abs_sum(coef, 4, blk & (n - 1), blk >> l2, n));
        }
      }
      V->rq_i[4] = reg_bins;
      V->rq_i[5] = reg_bins >= 4;
    }
    CTU_SYNC();
    RQ_T(14);
    if (CTU_TID == 0) {
      // the sums in scan order and the group's decision (rdo.c:1689-1772)
      double rd_coded = 0, rd_uncoded = 0, rd_sig = 0, rd_sig0 = 0;
      int nnz_before_pos0 = 0, flag = 0, spent = 0;
      for (int sp = 15; sp >= 0; --sp) {
        const int scanpos = cgs * 16 + sp;
        if (scanpos > last_scanpos) continue;
        const double cc = V->rq_stage[sp], cs = V->rq_stage[16 + sp], c0 = RQ_LD(&C0[scanpos]);
        const int level = dst[scan[scanpos]];
        block_uncoded_cost += c0;
        base_cost += cc;
        // (the first position of a group other than group 0 resets the Rice parameter INSTEAD of paying: rdo.c:1690-1697)
        if (!(sp == 0 && cgs > 0)) spent += (level < 2 ? level : 3) + (scanpos != last_scanpos);
        rd_sig += cs;
        if (sp == 0) rd_sig0 = cs;
        if (level) {
          flag = 1;
          rd_coded += cc - cs;
          rd_uncoded += c0;
          if (sp != 0) nnz_before_pos0++;
        }
      }
      if (fast && regular) V->rq_i[4] = reg_bins - spent;
      int zeroed = 0;
      if (cgs) {
        unsigned right = 0, lower = 0;
        if (cg_pos_x + 1 < cgw) right = V->cg_flag[cg_blkpos + 1];
        if (cg_pos_y + 1 < cgw) lower = V->cg_flag[cg_blkpos + cgw];
        const int o_grp = M_SIGGRP + (E.t ? 2 : 0) + ((right || lower) ? 1 : 0);
        if (!flag) {
          cost_cg_sig[cgs] = lambda * rbits(E, o_grp, 0);
          base_cost += cost_cg_sig[cgs] - rd_sig;
        } else if (cgs < cg_last) {
          if (nnz_before_pos0 == 0) { base_cost -= rd_sig0; rd_sig -= rd_sig0; }
          double cost_zero_cg = base_cost;
          cost_cg_sig[cgs] = lambda * rbits(E, o_grp, 1);
          base_cost += cost_cg_sig[cgs];
          cost_zero_cg += lambda * rbits(E, o_grp, 0);
          cost_zero_cg += rd_uncoded;
          cost_zero_cg -= rd_coded;
          cost_zero_cg -= rd_sig;
          if (cost_zero_cg < base_cost) {
            flag = 0;
            zeroed = 1;
            base_cost = cost_zero_cg;
            cost_cg_sig[cgs] = lambda * rbits(E, o_grp, 0);
          }
        }
      } else {
        flag = 1;
      }
      V->cg_flag[cg_blkpos] = (uint8_t)flag;
      V->rq_i[6] = zeroed;
    }
    CTU_SYNC();
    RQ_T(15);
    {
      // the group's costs go to the per-position arrays the last-position search reads; a zeroed group's positions fall back to level 0
      const int zeroed = V->rq_i[6];
      PAR_FOR(sp, 16) {
        const int scanpos = cgs * 16 + sp;
        if (scanpos <= last_scanpos) {
          const int blk = scan[scanpos];
          if (zeroed && dst[blk]) { dst[blk] = 0; CC[scanpos] = RQ_LD(&C0[scanpos]); CS[scanpos] = 0; }
          else { CC[scanpos] = V->rq_stage[sp]; CS[scanpos] = V->rq_stage[16 + sp]; }
        }
      }
    }
    CTU_SYNC();
  }
  RQ_T(16);
  // ---- coded block flag and the last significant position (rdo.c:1774-1833) ----
  if (CTU_TID == 0) {
    double best_cost;
    int best_last_idx_p1 = 0;
    {
      const int o_cbf = color == 0 ? (CTU_RQ_ROOT(V) ? 243 : M_CBF_LUMA) : color == 1 ? M_CBF_CB : M_CBF_CR + (cbf_u ? 1 : 0);
      best_cost = block_uncoded_cost + lambda * rbits(E, o_cbf, 0);
      base_cost += lambda * rbits(E, o_cbf, 1);
    }
    const int32_t *last_x_bits = S->last_bits + last_bits_off(E.t, l2, 0), *last_y_bits = S->last_bits + last_bits_off(E.t, l2, 1);
    int found_last = 0;
    for (int cgs = cg_last; cgs >= 0; cgs--) {
      const int first = scan[cgs * 16];
      const int cg_blkpos = ((first >> l2) >> 2) * cgw + ((first & (n - 1)) >> 2);
      base_cost -= cost_cg_sig[cgs];
      if (V->cg_flag[cg_blkpos]) {
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
            const double total = base_cost + cost_last - RQ_LD(&CS[scanpos]);
            if (total < best_cost) { best_last_idx_p1 = scanpos + 1; best_cost = total; }
            if (dst[blkpos] > 1) { found_last = 1; break; }
            base_cost -= RQ_LD(&CC[scanpos]);
            base_cost += RQ_LD(&C0[scanpos]);
          } else {
            base_cost -= RQ_LD(&CS[scanpos]);
          }
        }
        if (found_last) break;
      }
    }
    V->rq_i[0] = best_last_idx_p1;
    V->rq_i[1] = best_last_idx_p1 > 0;
  }
  CTU_SYNC();
  RQ_T(17);
  const int best_last_idx_p1 = V->rq_i[0];
  PAR_FOR(scanpos, last_scanpos + 1) {
    const int b = scan[scanpos];
    if (scanpos < best_last_idx_p1) { const int level = dst[b]; dst[b] = (int16_t)((coef[b] < 0) ? -level : level); }
    else dst[b] = 0;
  }
  CTU_SYNC();
  RQ_T(18);
}
