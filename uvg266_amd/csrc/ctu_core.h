// Closed-loop intra search of one CTU by one workgroup (uvg_search_lcu / search_cu, src/search.c:1299-2479, for the all-intra
// --preset medium configuration: quad-tree depths pu-depth-intra min..max, rd = 0, RDOQ, no MTS / LFNST / ISP / MRL / MIP / CCLM /
// JCCR / transform skip / dual tree, WPP), followed by the real coder's model adaptation (uvg_encode_coding_tree) so that the next
// CTU starts from the models the reference would hand it.
//
// NOT a translation of the reference's work tree.  The reference recurses with one lcu_t copy per depth and copies winners up;
// here ONE set of "decided" planes (D) lives in LDS with a one-sample border holding the neighbouring CTUs' samples, so every
// block's intra references -- inside or across the CTU edge -- are fetched the same way.  A CU is reconstructed straight into
// D; if its split will be tried the result is parked in a per-depth candidate buffer, the children overwrite D, and the parked
// candidate is put back only if the split loses (work_tree_copy_up inverted).  The walk is an explicit depth-first loop, not
// recursion.  Dead work of the reference is not done: the chroma blocks are reconstructed once per CU (the reference does it
// twice with the same inputs, search.c:1496 and :1572) and once per 8x8 area of 4x4 CUs (the reference redoes it for each of
// the four, only the last survives).
//
// Execution model: regions that touch many samples run on all lanes (PAR_FOR: predictions + SATD of the rough search, residual,
// transforms, dequantisation, reconstruction, SSD, copies); regions that are a recurrence through the CABAC models or through
// floating-point sums whose order the reference fixes (RDOQ walk, coefficient bit cost, mode bits, the RD comparisons) run on
// lane 0 (SERIAL).  Every hand-over between regions is a workgroup barrier.  The same source compiles for the host with one
// "lane" and no barriers -- the CPU tests run that emulation against the CPU restatement of the reference (tests/emul/); the product only ever runs the
// device build.
//
// All RD arithmetic is IEEE double in the reference's operation order; compile with -ffp-contract=off.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "intra_pred_dev.h"
#if defined(__HIPCC__)
#include "satd_dev.h"
#endif
#include "vvc_tables.h"
#include "vvc_ctx_init.h"
#include "vvc_rdoq_tables.h"
#include "../../include/uvg266_hip.h"
#if defined(CTU_PB)
#include "inter_cand_dev.h"
#endif

// ---- build configurations ------------------------------------------------------------------------------------------------------
// Two things select what this header, ctu_leaf4.h and ctu_pb.h compile to: the compiler (hipcc defines __HIPCC__: the device build;
// g++: the host emulation, one lane) and CTU_PB (the kernel of P / B pictures, ctu_pb.h).  What is really built:
//
//   configuration       translation units                                    built by
//   device, intra       ctu_search.hip, slice_coder.hip                      csrc/Makefile
//   device, CTU_PB      ctu_search_pb.hip (defines CTU_PB before including)  csrc/Makefile
//   host, intra         tests/emul/ctu_emul.cpp                              tests/emul/Makefile
//   host, CTU_PB        tests/emul/ctu_pb_emul.cpp (-DCTU_PB)                tests/emul/Makefile
//   ... each device build again with EXTRA=-DCTU_PROFILE (a library of its own for tools/dev/*, see tools/dev/README.md), and
//   ctu_search.hip / ctu_search_pb.hip with EXTRA=-DCTU_POISON_LDS=0xA5 (a debug build: the launch fills the LDS image first)
//
//   switch        what it changes
//   __HIPCC__     64 lanes and wave fences instead of one lane (the macros below); the 4x4 leaf on ctu_leaf4.h (lds::lf_*, eval_cu4,
//                 coder_area4, a 4x4 arena share without the rough search's and RDOQ's arrays) -- the host keeps eval_cu for it;
//                 the wave-level rdoq_wave, coeff_bits, rough_costs and search_intra_rough (the selection in the lanes' registers,
//                 rs_round) -- the host's are the reference's serial walks (rdoq_serial in ctu_rdoq_emul.h, coeff_bits_serial, a three-entry list in
//                 locals); the depth waves' mailboxes instead of calls in place; the slim images: lds_cfg<uint16_t>::slim of the intra kernel (cand_px, the 32x32 arena share and the two
//                 large scans in the workgroup's global scratch), lds_cfg<PX>::slim_scan with CTU_PB (the scans only)
//   CTU_PB        NMX = 257 + 18 models per set; level_state::mot / fl / cbf4; wctx::rq_root; lds::pb .. cur64 (the inter state, the
//                 leaf and depth waves' own) in place of lds::req64 .. h64 (the 64x64 candidate beside the walk, the coder's pass
//                 by model); one arena region for the depths 1..3; scratch::save_mot .. prof_pb; job::pb .. init_qp; the extra
//                 parameter of eval_cu (forced_mode) and of recon_tu / recon_tu_inl (flags)
//   CTU_PROFILE   lds::prof_w in front of the image; on the device the timer macros below count s_memtime ticks into
//                 scratch::prof / prof_lf / prof_pb (always there; read by slot number by tools/dev/*) -- with CTU_PROFILE_WALK the
//                 P / B phases of the walk's wave only
// Every macro that depends on these is defined here and nowhere else.
#if defined(__HIPCC__)
#define CTU_NOINLINE __attribute__((noinline))
#define CTU_INLINE __attribute__((always_inline))
#define CTU_INLINE1 __attribute__((always_inline))          // one call site: no call, no callee-saved registers through the stack
#define CTU_DEV static __device__
#define CTU_SHARED __shared__
// Everything the search computes is WAVE-local: a depth of the quad tree is worked by one wave (see search_ctu), so "all lanes"
// means the 64 lanes of that wave and a hand-over between regions is a wave-level fence, not a workgroup barrier.
#define CTU_TID ((int)(threadIdx.x & 63))
#define CTU_NT 64
// A wave's ROLE -- 0 walks the CTU, 1..3 evaluate the depths 3..1 -- is its index in the workgroup relative to S->rot, which the launcher
// picks so that the walkers of the workgroups sharing a CU spread over the SIMDs (four walkers on one SIMD cost 9 %,
// profiles/r04_simd_placement.txt).  The role must NOT be read off the hardware (HW_REG_HW_ID): with several queues busy the
// scheduler saves waves and restores them elsewhere, and a role that changes under a wave is a wrong CTU.  Where a wave sits
// when its workgroup starts is only a hint for S->rot.  `S` is in scope wherever the role is asked for.
#define CTU_WAVE (__builtin_amdgcn_readfirstlane((int)((threadIdx.x >> 6) - S->rot) & 3))
#define CTU_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
// the few workgroup-wide regions (CTU load / store)
#define BLK_TID ((int)threadIdx.x)
#define BLK_NT ((int)blockDim.x)
#define BLK_SYNC() __syncthreads()
// a load that must see what another wave of this workgroup stored to global memory earlier (served by L2, not by this CU's L1)
#define CTU_GLOAD(p) __builtin_nontemporal_load(p)
#define CTU_LDS __attribute__((address_space(3)))
#define CTU_GLB __attribute__((address_space(1)))
#else
#define CTU_NOINLINE
#define CTU_INLINE
#define CTU_INLINE1
#define CTU_DEV static inline
#define CTU_SHARED static
#define CTU_TID 0
#define CTU_NT 1
#define CTU_WAVE (ctu::g_emul_wave)
#define CTU_SYNC() ((void)0)
#define BLK_TID 0
#define BLK_NT 1
#define BLK_SYNC() ((void)0)
#define CTU_GLOAD(p) (*(p))
#define CTU_LDS
#define CTU_GLB
#endif
// RDOQ prices a luma block's "no coefficients" with the root cbf when the block belongs to an inter CU (wctx::rq_root)
#if defined(CTU_PB)
#define CTU_RQ_ROOT(V) ((V)->rq_root)
#else
#define CTU_RQ_ROOT(V) 0
#endif
// The phase timers of a CTU_PROFILE device build: lane 0 of the wave, s_memtime ticks.  No function body tests the switch itself.
//   CTU_T0 / CTU_T1(W, slot)   a bracketed phase into scratch::prof[wave][slot]; PB_T0 / PB_T1: into scratch::prof_pb[slot]
//   RQ_T0(W) ... RQ_T(slot)    consecutive phases of one function, each ending at its mark, into scratch::prof[wave][slot]
//   RQ_N(slot, v)              a count between RQ_T0 and the marks: v above the low 40 bits of that slot's cycles (rdoq_wave: 12
//                              fixed-point rounds, 13 passes the budget narrowed to one group, 14 passes, 15 groups decided)
//   LF_T0() ... LF_T(slot)     the same for the 4x4 leaf on the walk's wave, into scratch::prof_lf[slot] (`J` in scope); LF_TR():
//                              restart the interval after a step that counted itself; LF_TN(slot): a step that does not run for
//                              every CU -- its cycles in the low 40 bits, how often it ran above them
//   WAIT_EVAL(S, L)            wait_eval, and how long the walk stood in it, into scratch::prof_lf[14 / 15] for depths 1 + 2 / 3
//   PB_COUNT, CTU_PROF_RESET / PB_PROF_RESET: the counters and the reset that are not a phase
// RQ_T0, RQ_N and the last group stand as statements WITHOUT a semicolon of their own: a build without the switch has no token there.
#if defined(__HIPCC__) && defined(CTU_PROFILE)
#define CTU_T0() const unsigned long long ctu_t0__ = __builtin_amdgcn_s_memtime()
#define CTU_T1(W, slot) do { if (CTU_TID == 0) (W)->prof[CTU_WAVE][slot] += __builtin_amdgcn_s_memtime() - ctu_t0__; } while (0)
#define RQ_T0(W) scratch *const rq_w__ = (W); unsigned long long tq = __builtin_amdgcn_s_memtime();
#define RQ_T(slot) do { const unsigned long long t2 = __builtin_amdgcn_s_memtime(); if (CTU_TID == 0) rq_w__->prof[CTU_WAVE][slot] += t2 - tq; tq = t2; } while (0)
#define RQ_N(slot, v) if (CTU_TID == 0) rq_w__->prof[CTU_WAVE][slot] += (unsigned long long)(v) << 40;
#define LF_T0() unsigned long long tq = __builtin_amdgcn_s_memtime()
#define LF_T(slot) do { const unsigned long long t2 = __builtin_amdgcn_s_memtime(); if (CTU_TID == 0 && CTU_WAVE == 0) J.W->prof_lf[slot] += t2 - tq; tq = t2; } while (0)
#define LF_TR() do { tq = __builtin_amdgcn_s_memtime(); } while (0)          // restart: what ran since the last mark counted itself
#define LF_TN(slot) do { const unsigned long long t2 = __builtin_amdgcn_s_memtime(); if (CTU_TID == 0 && CTU_WAVE == 0) J.W->prof_lf[slot] += (1ull << 40) + (t2 - tq); tq = t2; } while (0)
#define WAIT_EVAL(S, L) do { LF_T0(); wait_eval(S, L); LF_T((L) <= 2 ? 14 : 15); } while (0)
#define CTU_PROF_RESET(S, J) BLK_FOR(i, 4 * 32) (J).W->prof[i >> 5][i & 31] = 0; BLK_FOR(i, 16) (J).W->prof_lf[i] = 0; (S)->prof_w = (J).W;
#define PB_T0() const unsigned long long pb_t0__ = __builtin_amdgcn_s_memtime()
#if defined(CTU_PROFILE_WALK)      // only the walk's wave counts the phases of eval_pb (slots < 14): they add up to its time
#define PB_T1(W, slot) do { if (CTU_TID == 0 && ((slot) >= 14 || CTU_WAVE == 0)) (W)->prof_pb[slot] += __builtin_amdgcn_s_memtime() - pb_t0__; } while (0)
#else
#define PB_T1(W, slot) do { if (CTU_TID == 0) (W)->prof_pb[slot] += __builtin_amdgcn_s_memtime() - pb_t0__; } while (0)
#endif
#define PB_COUNT(W, slot) SERIAL (W)->prof_pb[slot] += 1;
#define PB_PROF_RESET(S, J) BLK_FOR(i, 24) (J).W->prof_pb[i] = 0; BLK_FOR(i, 4 * 32) (J).W->prof[i >> 5][i & 31] = 0; (S)->prof_w = (J).W;
#else
#define CTU_T0() ((void)0)
#define CTU_T1(W, slot) ((void)0)
#define RQ_T0(W)
#define RQ_T(slot) ((void)0)
#define RQ_N(slot, v)
#define LF_T0() ((void)0)
#define LF_T(slot) ((void)0)
#define LF_TR() ((void)0)
#define LF_TN(slot) ((void)0)
#define WAIT_EVAL(S, L) wait_eval(S, L)
#define CTU_PROF_RESET(S, J)
#define PB_T0() ((void)0)
#define PB_T1(W, slot) ((void)0)
#define PB_COUNT(W, slot)
#define PB_PROF_RESET(S, J)
#endif
#define LDSP(T, p) ((CTU_LDS T *)(p))          // a pointer known to point into the workgroup's LDS image (device: ds_* instead of flat_*)
// ... and one that points into the LDS image OR, in a slim build (lds_cfg below), into the workgroup's global scratch: a generic pointer
// there (flat_*: the LDS aperture costs a lone wave the same 52 cycles as ds_read, profiles/r05_lat_probe.txt)
#define MGP(PX, T, p) ((typename ctu::mg_ptr<PX, T>::type)(p))
#define PAR_FOR(i, n) for (int i = CTU_TID; i < (n); i += CTU_NT)
#define BLK_FOR(i, n) for (int i = BLK_TID; i < (n); i += BLK_NT)
#define SERIAL if (CTU_TID == 0)

namespace ctu {

#if !defined(__HIPCC__)
static int g_emul_wave = 0;      // host emulation: which wave's scratch the code running now uses
static int g_emul_lazy = 0;      // host emulation: pretend a CU's own cost is never known before all its children are done
static int g_emul_depthwave = 0; // ... of its three-wave build: 32x32 / 16x16 CUs handed to the depth wave, the walk goes on into their children
static int g_emul_leafwave = 0;  // host emulation of the P / B kernel's two-wave build: the four 4x4 CUs of an 8x8 area go to the leaf wave (ctu_pb.h)
// Host emulation: there is one thread, so what another wave of the workgroup would do for a request happens where the request is
// posted -- `fn` runs right here as the wave of role `w` (CTU_WAVE: that wave's scratch).  The only place that switches the wave.
template <typename F> static inline void emul_on_wave(int w, F fn)
{
  const int me = g_emul_wave;
  g_emul_wave = w;
  fn();
  g_emul_wave = me;
}
#endif

enum { LCU = 64, LCU_C = 32, PY = 68, PC = 36, NMODELS = 257 };
// P / B pictures (ctu_pb.h, compiled with -DCTU_PB): the 18 models of the inter syntax sit behind the 257 in every LDS model set
#if defined(CTU_PB)
enum { NMX = NMODELS + 18 };
#else
enum { NMX = NMODELS };
#endif
enum { M_SIGGRP = 0, M_SIG = 4, M_PAR = 28, M_GT1 = 70, M_GT2 = 112, M_LASTX = 154, M_LASTY = 194, M_CBF_LUMA = 234, M_CBF_CB = 238,
       M_CBF_CR = 240, M_SPLIT = 244, M_MPM = 253, M_PLANAR = 254, M_CHROMA_PRED = 256 };
enum { CU_NOTSET = 0, CU_INTRA = 1, CU_INTER = 2 };
#define CTU_MAX_DOUBLE 1.7976931348623157e308

// what the search reads from encoder_state_t / encoder_control_t: the C ABI's own struct (include/uvg266_hip.h), taken as it is
using params = uvghip_ctu_params_t;

// one 4x4 unit of the CTU's side information while the search runs (the slice of cu_info_t this path reads back)
struct cu4 {
  uint8_t type, log2, cbf, luma_edges, chroma_edges, log2_c;
  int8_t mode, mode_chroma;
};

struct level_state {        // search_cu's locals, per depth
  double cost, split_cost, split_bits;
  int x, y;                 // picture coordinates
  int child;                // next child to visit
  int type, mode, cbf;      // the parked no-split candidate
  int has_chroma;           // carries the chroma of its area
  int pending;              // its unsplit evaluation was handed to the depth's wave
  int evalp, known, can;    // P / B depth wave (ctu_pb.h): evaluation posted; its result has been taken; can_inter | can_intra << 1 of the request
  uint32_t split_tree, mode_type_tree;
#if defined(CTU_PB)
  int32_t mot[8];           // the parked candidate's motion (icand::unit: type, mv[2][2], ref[2], dir)
  uint8_t fl[8];            // uvghip_inter4_t: skipped, merged, merge_idx, root_cbf, mv_cand0, mv_cand1, mv_ref0, mv_ref1
  int32_t cbf4[4];          // a 64x64 inter CU: the flags of its four transform units
#endif
};

// The LDS diet of the 10-bit I-picture kernel: with 2-byte samples the image is 8.9 KB over a quarter of the CU's 160 KB, which costs
// the fourth workgroup per CU.  A slim build keeps out of LDS what only the 32x32 depth (the least loaded wave) and the rare 64x64
// candidate touch: the depth-1 candidate's samples, the depth-1 scratch's levels, the 16x16 / 32x32 coefficient scans -- they live in
// the workgroup's global scratch (L1 / L2 resident) behind generic pointers.  8-bit, P / B and host builds are not slim.
// (slim_scan alone: only the two large scans move -- the P / B kernel, whose image also carries the inter state)
#if !defined(__HIPCC__)
template <typename PX> struct lds_cfg { enum { slim = 0, slim_scan = 0 }; };
#elif defined(CTU_PB)
template <typename PX> struct lds_cfg { enum { slim = 0, slim_scan = 1 }; };
#else
template <typename PX> struct lds_cfg { enum { slim = 0, slim_scan = 0 }; };
template <> struct lds_cfg<uint16_t> { enum { slim = 1, slim_scan = 1 }; };
#endif
template <typename PX, typename T, bool SLIM = (lds_cfg<PX>::slim != 0)> struct mg_ptr { typedef CTU_LDS T *type; };
template <typename PX, typename T> struct mg_ptr<PX, T, true> { typedef T *type; };

template <typename PX> struct px_info;
template <> struct px_info<uint8_t> { enum { depth = 8, maxv = 255 }; };
template <> struct px_info<uint16_t> { enum { depth = 10, maxv = 1023 }; };

// LDS image of a workgroup
// scratch of ONE wave (= one depth of the quad tree): pointers into the workgroup's arena, sized for that depth's blocks, and the
// small fixed-size pieces inline
struct wctx {
  uint16_t *top, *left, *ftop, *fleft;              // reference rows: 4 n + 8 entries each
  int16_t *t0, *t1;                                 // transform scratch, n * n each, adjacent (together also the n * n words of coeff_bits)
  int16_t *lv0, *lv1, *lv2;                         // levels of the transform blocks being evaluated (y, u, v)
  double *rq_cc, *rq_cs;                            // RDOQ per-position costs in LDS (nullptr: the depth uses the workgroup's global scratch)
  uint32_t *part;                                   // rough search: (satd, sad) per (listed mode, tile)
  uint32_t *cur;                                    // the models this wave's bit counting works on
  union {                                           // a wave is in one phase at a time
    double rq_stage[2 * 16];                        // RDOQ: costs of the coefficient group in flight (also the coefficient bit count's 64 group totals)
    struct { double rs_cand[3 + 24], rs_best_cost[2][3]; };      // rough search: [0] the winner's cost.  The rest, like u_d0, u_d1, rs_best_mode,
  };                                                // rs_chk, u_n_modes and lds::help below, has no reader or writer in any build: the layout was kept
  double u_d0, u_d1;                                // when the host emulation stopped using them (profiles/README.md, r14)
  int32_t rq_i[16];
  int32_t rs_list[24], rs_best_mode[2][3];          // rs_list: the modes listed in the round (rough_costs reads it)
  uint32_t rs_chk[3];
  int32_t red[8];
  int32_t u_avail_left, u_avail_top, u_mode, u_flag, u_n_modes;
  uint8_t cg_flag[64];
  int8_t mpm[6];
  int16_t refn;                                     // entries of a reference row
#if defined(CTU_PB)
  int32_t rq_root;                                  // RDOQ prices a luma block's "no coefficients" with the root cbf (a block of an inter CU, rdo.c:1774)
#endif
};

constexpr int arena_bytes(int n, bool slim = false)     // one depth's share of the arena (n = its luma block size)
{
  if (slim && n == 32) return (4 * (4 * n + 8) * 2 + 2 * n * n * 2 + 15) & ~15;      // (the levels live in scratch::lv32)
  // reference rows, two transform buffers, levels (y, u, v), [4x4 only: the rough search's partial costs -- larger blocks keep
  // them in the transform buffers, idle during the rough search], [<= 8x8: RDOQ's two per-position cost arrays]
#if defined(__HIPCC__)
  // (the 4x4 leaf keeps the rough search's costs and RDOQ's per-position costs in registers: reference rows, transform buffers, levels only)
  if (n == 4) return (4 * (4 * n + 8) * 2 + 2 * n * n * 2 + (n * n + 2 * 16) * 2 + 15) & ~15;
#endif
  return (4 * (4 * n + 8) * 2 + 2 * n * n * 2 + (n * n + 2 * ((n / 2) * (n / 2) < 16 ? 16 : (n / 2) * (n / 2))) * 2 +
          (n >= 8 ? 0 : 2 * 18 * 4) + (n <= 8 ? 8 + 2 * n * n * 8 : 0) + 15) & ~15;
}
#if defined(CTU_PB)
// one wave walks a P / B CTU, a depth at a time: the depths' scratch areas share ONE region sized for the largest (ctu_pb.h); the 4x4
// depth has its own behind it -- in the two-wave build the leaf wave works there while the walk evaluates the 8x8 CU above
enum { ARENA_BYTES = arena_bytes(32) + arena_bytes(4) };
#else
enum { ARENA_BYTES = arena_bytes(4) + arena_bytes(8) + arena_bytes(16) + arena_bytes(32) };
#endif
enum { ARENA_BYTES_SLIM = arena_bytes(4) + arena_bytes(8) + arena_bytes(16) + arena_bytes(32, true) };

struct scratch;
#if defined(CTU_PB)
// ---- P / B pictures: what the inter search keeps beside the intra state (ctu_pb.h) ----
struct pb_cand {            // one entry of the reference's unit_stats_map_t: a candidate motion with its cost
  icand::unit m;
  uint8_t merged, skipped, merge_idx, cand0, cand1, pad[3];
  double cost, bits;
};
struct pb_state {
  // motion of every 4x4 unit of the CTU and of the row / column before it ([289]: the CTU above right, unused with WPP) and the
  // uvghip_inter4_t of the same units: in the workgroup's global scratch (scratch::pb_mot / pb_fl) -- 11.6 KB of LDS were the fourth
  // workgroup per CU, and the tables are read a few entries per candidate list
  icand::unit *mot;
  uint8_t (*fl)[8];
  const int32_t *hm;                   // the history table the evaluation in progress reads: the one at the entry of its node (hmvp_entry[L])
  int32_t hmvp[41];                    // the row's history table as the search sees it: [0] entries, then 5 units, most recent first
  int32_t hmvp_entry[4][41];           // ... at the entry of the node of each depth 0..3 (search_cu's hmvp_lut)
  int32_t hmvp_coder[41];              // ... as the real coder leaves it (what the next CTU of the row starts from)
  uint32_t work0[NMX];                 // the models the 64x64 candidate works on (work[L - 1] of depth 0)
  uint32_t cnt_models[NMX];            // a counting-only bit cost adapts the last-position / group-flag models on this copy
  icand::frame_ctx f;                  // the call context of the candidate derivations
  icand::amvp_ws ws;
  icand::merge_cand mc[6];
  int32_t n_mc;
  pb_cand cur;                         // search_pu_inter's cur_pu
  pb_cand merge[6], amvp[3][8];
  int8_t merge_keys[8], amvp_keys[3][8];
  int32_t merge_size, amvp_size[3];
  int32_t mv_cand[2][2];               // info->mv_cand
  int32_t amvp_cache[2][8][4];         // the predictors of (list, reference index) for the CU being evaluated: derived once
  uint32_t amvp_have[2];
  int32_t amvp_key[3];                 // the CU (x, y, size) the cache belongs to
  int32_t colc[2][8];                  // the two positions of the collocated picture a CU's temporal candidate can come from, fetched once per CU
  int32_t colc_idx[2];                 // ... their indices on the 8x8 grid (-1: none)
  int32_t out4[4];
  int32_t ref_idx2[2];
  int32_t i0, i1, i2, i3;              // small hand-overs from lane 0 to the wave
  int32_t early_tag;                   // 1 + the merge index whose luma levels the early-skip test left in the CU's coefficient target (0: none)
  double d0, d1;
};
#endif
// LDS image of a workgroup
template <typename PX> struct lds {
#if defined(CTU_PROFILE)
  scratch *prof_w;
#endif
  PX Dy[65 * PY], Du[33 * PC], Dv[33 * PC];         // decided planes, index (y + 1) * pitch + x + 1
  PX cand_px[lds_cfg<PX>::slim ? 480 : 2016];       // a depth's CU while its split is being tried (depths 1..3; slim: 2..3, depth 1 in scratch::cand_px32)
  cu4 cu[17 * 17];                                  // index (y4 + 1) * 17 + x4 + 1
  scratch *scr;                                     // the workgroup's global scratch (the split / mode-type trees per 4x4 live there)
  uint32_t cur[NMX];                                // state->search_cabac models of the walk: state0 | state1 << 16
  uint32_t work[3][NMX];                            // [L - 1], L = 1..3: the models the depth-L candidate starts from (written by the walk when it
                                                    // posts the evaluation) and, adapted in place, leaves behind; [2] doubles as scratch for the 64x64 candidate
  uint32_t coder[NMX];                              // state->cabac models
  uint8_t rdoq_state[244];                          // CTX_STATE of the coder's models at the CTU's start (what uvg_rdoq prices with)
  uint16_t scan[lds_cfg<PX>::slim_scan ? 64 + 16 : 1024 + 256 + 64 + 16];      // coefficient scans of the four square shapes (slim: 8x8 and 4x4, the others in scratch::scan_g)
  uint8_t inv4[16];                                 // scan index of the 4x4 group's raster position y * 4 + x
  uint16_t deps4[16];                               // per scan index of a 4x4 group: the scan indices (bits) its context template reads inside the group
  int32_t last_bits[92];                            // RDOQ: bit cost of the last-position prefix per (luma/chroma, log2 size, x/y, group index): last_bits_off
  level_state lvl[5];
  wctx wv[4];                                       // [0] depth 4 (4x4), [1] depth 3, [2] depth 2, [3] depth 1 (32x32)
  int32_t vsel[4];                                  // which wv[] a wave is using (a wave may borrow a larger one while its owner idles)
  int32_t rot;                                      // index of the wave with role 0 (CTU_WAVE)
  int32_t req[4], done[4];                          // depth pipeline: evaluation requests / completions per depth
  int32_t help[4];                                  // unused (see wctx::rs_cand)
#if defined(__HIPCC__)
  // ctu_leaf4.h: the cubic interpolation filter (4 x int8 per phase), intraPredAngle | invAngle << 8 per |mode distance|, per raster
  // position of a 4x4 block (positions later in scan order | scan index << 16 | raster of the next scan index << 20), the 8x8 area
  // whose source samples are parked in lf_src ([0, 64) luma, [64, 80) Cb, [80, 96) Cr)
  uint32_t lf_cubic[32], lf_disp[17], lf_rq[16];
  double lf_escale[2];                              // uvg_rdoq's error scale of a 4x4 block: luma, chroma
  int32_t lf_qbits[2], lf_q[2];                     // ... q_bits, quantiser scale
  int32_t lf_tag;
  PX lf_src[96];
#endif
#if !defined(CTU_PB)
  // the 64x64 candidate (post64 / finish64): posted once the first 32x32 area is decided, its luma blocks taken by depth 1's wave and
  // its chroma blocks by depth 2's between their evaluations; the modes (luma, chroma) of the request; per 32x32 transform unit the
  // flags, the SSDs and the bit counts (bits: chroma, bits_y: luma)
  int32_t req64, done64[2], m64[2];
  int32_t creq, cdone[2];                           // the coder's pass by model (run_ctu): asked for; the flags / the chroma coefficients are done
  struct { int32_t cu, cv, ssd_u, ssd_v, cy, ssd_y; double bits, bits_y; } h64[4];
#endif
  alignas(16) unsigned char arena[lds_cfg<PX>::slim ? (int)ARENA_BYTES_SLIM : (int)ARENA_BYTES];
#if defined(CTU_PB)
  pb_state pb;
  // the leaf wave of the two-wave build (ctu_pb.h post_leaves): on / off, the costs of the four 4x4 CUs of the area it was handed
  int32_t leaf_wave;
  double leaf_cost[4];
  double leaf_limit;                   // the leaf wave stops when the costs of its 4x4 CUs exceed it (the walk lowers it when the 8x8 CU's cost is in);
                                       // (in front of pbx: the two-wave launch asks for the image up to there, pb_lds_bytes)
  // the three-wave build (ctu_pb.h): the wave that evaluates the 32x32 / 16x16 CUs ahead of the walk has its own search state (of `pb`
  // it reads the shared tables only: mot, fl, hmvp_entry) and the 8x8 depth its own scratch; the one- and two-wave launches ask for
  // the image up to here (pb_lds_bytes)
  int32_t depth_wave, skip_eval[4];
  pb_state pbx;
  alignas(16) unsigned char arena8[arena_bytes(8)];
  // ... and the 8x8 CU's batched merge analysis (ctu_pb.h merge_batch8) its own scratch: [candidate][list][15][8] intermediates, the
  // predictions [candidate][64], the SATDs (the one-wave build borrows the 32x32 depth's transform buffers for them)
  alignas(16) int16_t b8_tmp[6 * 2 * 120];
  PX b8_pred[6 * 64];
  int32_t b8_satd[8];
  // the four-wave build: 32x32 CUs on a wave of their own (search state and, for the 16x16 depth, scratch)
  pb_state pbx2;
  alignas(16) unsigned char arena16[arena_bytes(16)];
  // ... and the 64x64 CU evaluated there as well, beside the walk: its samples and levels (64x64 + 2 x 32x32) while the split is tried,
  // the walk's models as they were after the CU's split flag (what a pruned CTU goes on with)
  alignas(16) PX cand64_px[6144];
  int16_t cand64_co[6144];
  uint32_t cur64[NMX];
#endif
};
#if defined(CTU_PB)
template <typename PX> constexpr size_t pb_lds_bytes(int waves) { return waves >= 4 ? sizeof(lds<PX>) : (waves == 3 ? offsetof(lds<PX>, pbx2) : offsetof(lds<PX>, pbx)); }
// the search state of the wave that asks (roles 2, 3: the depth waves)
template <typename PX> CTU_DEV pb_state &pbq(lds<PX> *S) { const int r = CTU_WAVE; return r == 2 ? S->pbx : (r == 3 ? S->pbx2 : S->pb); }
#endif
template <typename PX> CTU_DEV wctx *wv_of(lds<PX> *S) { return &S->wv[S->vsel[CTU_WAVE]]; }

// per-workgroup scratch in global memory
struct scratch {
  double cost_coeff[1024], cost_sig[1024], cost_coeff0[1024];
  uint16_t save_px[6144];          // the 64x64 candidate's samples and levels beside the split's (I pictures: post64; P / B one-wave build: the
  int16_t save_co[6144];           // whole D of a CTU while the candidate is tried in place)
  cu4 save_cu[256];
  int16_t cand_co[2016];           // levels of the candidate CUs of depths 1..3 (cand_px_off)
  // a slim build (lds_cfg): the depth-1 candidate's samples, the levels of the depth-1 scratch (y, u, v), the scans of 32x32 and 16x16
  uint16_t cand_px32[1536];
  int16_t lv32[1536];
  uint16_t scan_g[1024 + 256];
  uint32_t save_tree[512];
  uint16_t tree[256], mtt[256];    // split_tree / mode_type_tree per 4x4 of the decided CTU (3 / 2 bits per depth, depths 0..4)
#if defined(CTU_PB)
  int32_t save_mot[256][8];        // the 64x64 candidate of a P / B picture while its split is tried: motion, flags
  uint8_t save_fl[256][8];
  int32_t pb_mot[17 * 17 + 1][8];  // pb_state::mot / fl (icand::unit is eight int32)
  uint8_t pb_fl[17 * 17][8];
  unsigned long long prof_pb[24];     // CTU_PROFILE, ctu_pb.h: cycles of the phases of the P / B walk (lane 0 of the wave); 16.. : waits of the walk, the other waves' busy time
#endif
  unsigned long long prof_lf[16];     // CTU_PROFILE, ctu_leaf4.h: cycles of the 4x4 leaf's steps (the walk's wave)
  unsigned long long prof[4][32];     // CTU_PROFILE: 0 rough search, 1 refs + prediction, 2 residual + transforms + reconstruction, 3 RDOQ, 4 SSD,
                                   // 5 RD cost (bits), 6 park / unpark / model copies, 7 64x64 candidate, 8 coder pass, 9 load, 10 store, 11 total
};

// everything one workgroup needs to know about its CTU
template <typename PX> struct job {
  params P;
  const PX *src_y, *src_u, *src_v;       // source planes
  int src_stride, src_stride_c;
  PX *rec_y, *rec_u, *rec_v;             // reconstruction before the in-loop filters (also the neighbours' samples)
  int rec_stride, rec_stride_c;
  uvghip_scu_t *cu_tab;                  // the picture's side information, one entry per 4x4
  int cu_stride;
  int16_t *coeff;                        // this CTU's lcu_coeff_t: y[64*64], u[32*32], v[32*32]
  uint32_t *models_out;                  // this CTU's three model sets [3][NMODELS]: at its start, after its search, after the coder
  const uint32_t *models_in;             // the coder's models this CTU starts from (NULL: initialise for an I slice at P.qp)
  scratch *W;
  int x, y;                              // CTU origin
#if defined(CTU_PB)
  const struct pb_job *pb;               // the picture's inter state (ctu_pb.h)
  uint32_t *pbm_out;                     // this CTU's three sets of the 18 inter-syntax models
  const uint32_t *pbm_in;                // ... of the CTU it starts from (NULL with models_in)
  int slice_type, init_qp;               // what the slice's models are initialised with (0 B, 1 P; state->frame->QP)
#endif
};

// the source samples of a block of `color` at CTU-local (bx, by) (in that plane's samples), read from the picture; -> pointer, pitch
// (blocks never reach outside the picture: a CU is only coded when it lies inside)
template <typename PX> CTU_DEV CTU_GLB const PX *src_block(const job<PX> &J, int color, int bx, int by, int *pitch)
{
  const PX *p = color == 0 ? J.src_y : (color == 1 ? J.src_u : J.src_v);
  const int st = color == 0 ? J.src_stride : J.src_stride_c, sh = color != 0;
  *pitch = st;
  return (CTU_GLB const PX *)(p + (size_t)((J.y >> sh) + by) * st + (J.x >> sh) + bx);
}


// ------------------------------------------------------------------------------------------------------------ models ------
// Tables every serial walk reads per bin live in LDS (a lone lane pays the full latency of every load: out of device memory the
// entropy table alone cost most of the search's time): the 512 bit costs, the models' window bytes, and the bit costs of the
// models uvg_rdoq prices with (fixed for the CTU).  Function-scope LDS, filled by load_ctu.
CTU_DEV uint32_t *tab_ebits() { CTU_SHARED uint32_t t[512]; return t; }
CTU_DEV uint8_t *tab_rate() { CTU_SHARED uint8_t t[(NMX + 7) & ~7]; return t; }
CTU_DEV uint32_t *tab_rdoq_bits() { CTU_SHARED uint32_t t[2 * 244]; return t; }
#define kRate (tab_rate())         // the window byte of every model (rate0 << 4 | rate1)

template <typename MP> CTU_DEV int m_state(MP m, int c) { return (int)(((m[c] & 0xffffu) + (m[c] >> 16)) >> 8); }
template <typename MP> CTU_DEV void m_update(MP m, int c, int bin)            // CTX_UPDATE, cabac.h:182-193
{
  const int r0 = kRate[c] >> 4, r1 = kRate[c] & 15;
  uint32_t s0 = m[c] & 0xffffu, s1 = m[c] >> 16;
  s0 -= (s0 >> r0) & 0x7fe0u;
  s1 -= (s1 >> r1) & 0x7ffeu;
  if (bin) { s0 += (0x7fffu >> r0) & 0x7fe0u; s1 += (0x7fffu >> r1) & 0x7ffeu; }
  m[c] = (s0 & 0xffffu) | (s1 << 16);
}
// uvg_f_entropy_bits (rdo.c:143, a float table) = uvg_entropy_bits / 2^15: every entry is an integer below 2^24 over 2^15, so the
// float and this double quotient are the same number
template <typename MP> CTU_DEV double m_fbits(MP m, int c, int bin) { return (double)tab_ebits()[(m_state(m, c) << 1) ^ bin] / 32768.0; }
// CABAC_FBITS_UPDATE with only_count = 1
template <typename MP> CTU_DEV void m_code(MP m, int update, int c, int bin, double &bits)
{
  bits += m_fbits(m, c, bin);
  if (update) m_update(m, c, bin);
}

CTU_DEV void models_init_one(uint32_t *m, int i, int qp, int slice)     // uvg_ctx_init, context.c:471-492
{
  const int v = k_ctx_init[slice][i];
  if (v == 255) { m[i] = 0; return; }
  const int slope = (v >> 3) - 4, offset = ((v & 7) * 18) + 1;
  int s = ((slope * (qp - 16)) >> 1) + offset;
  s = s < 1 ? 1 : (s > 127 ? 127 : s);
  const uint32_t p1 = (uint32_t)s << 8;
  m[i] = (p1 & 0x7fe0u) | ((p1 & 0x7ffeu) << 16);
}

// ------------------------------------------------------------------------------------------------------------- scans ------
CTU_DEV int scan_base(int log2n) { return log2n == 5 ? 0 : log2n == 4 ? 1024 : log2n == 3 ? 1280 : 1344; }
// the scan of the 1 << log2n square: the LDS table, or (slim build, 16x16 and 32x32) the workgroup's global copy
template <typename PX> CTU_DEV uint16_t *scan_of(lds<PX> *S, int log2n)
{
  if (lds_cfg<PX>::slim_scan) return log2n >= 4 ? S->scr->scan_g + (log2n == 5 ? 0 : 1024) : S->scan + (log2n == 3 ? 0 : 64);
  return S->scan + scan_base(log2n);
}
// last_bits: [luma 4, 8, 16, 32; chroma 4, 8, 16][x, y][group index 0 .. group_idx(n - 1)]
CTU_DEV int last_bits_off(int t, int log2n, int xy)
{
  const int cnt = 2 * log2n;                                       // 4, 6, 8, 10 entries
  const int base = log2n == 2 ? 0 : (log2n == 3 ? 8 : (log2n == 4 ? 20 : 36));
  return (t ? 56 : 0) + base + (xy ? cnt : 0);
}
// H.266 6.5.2 up-right diagonal scan of 4x4 groups, groups in diagonal order (tables.c g_scan_order, SCAN_DIAG)
CTU_DEV void diag_order(int n, uint8_t *out)      // out[i] = y * n + x of the i-th position of an n x n diagonal scan
{
  int i = 0;
  for (int d = 0; d < 2 * n - 1; ++d)
    for (int x = 0; x <= d; ++x) {
      const int y = d - x;
      if (x < n && y < n) out[i++] = (uint8_t)(y * n + x);
    }
}
// the index of the first position of diagonal d (x + y = d) in diag_order(n): d + 1 positions a diagonal up to the main one,
// 2n - 1 - d beyond it
CTU_DEV int rdoq_diag_start(int n, int d)
{
  return d < n ? d * (d + 1) / 2 : n * n - (2 * n - 1 - d) * (2 * n - d) / 2;
}
template <typename PX> CTU_DEV void build_scans(lds<PX> *S)
{
  SERIAL {
    uint8_t in[16], cg[64];
    diag_order(4, in);
    for (int l2 = 2; l2 <= 5; ++l2) {
      const int n = 1 << l2, cgw = n >> 2;
      diag_order(cgw, cg);
      uint16_t *sc = scan_of(S, l2);
      if (l2 == 2) {
        for (int k = 0; k < 16; ++k) S->inv4[in[k]] = (uint8_t)k;
        for (int k = 0; k < 16; ++k) {
          const int x = in[k] & 3, y = in[k] >> 2;
          unsigned m = 0;
          if (x + 1 < 4) m |= 1u << S->inv4[y * 4 + x + 1];
          if (x + 2 < 4) m |= 1u << S->inv4[y * 4 + x + 2];
          if (y + 1 < 4) m |= 1u << S->inv4[(y + 1) * 4 + x];
          if (y + 2 < 4) m |= 1u << S->inv4[(y + 2) * 4 + x];
          if (x + 1 < 4 && y + 1 < 4) m |= 1u << S->inv4[(y + 1) * 4 + x + 1];
          S->deps4[k] = (uint16_t)m;
        }
      }
      for (int g = 0; g < cgw * cgw; ++g) {
        const int gx = cg[g] % cgw, gy = cg[g] / cgw;
        for (int k = 0; k < 16; ++k) sc[g * 16 + k] = (uint16_t)((gy * 4 + in[k] / 4) * n + gx * 4 + in[k] % 4);
      }
    }
  }
  CTU_SYNC();
}

// ------------------------------------------------------------------------------------------- reference construction ------
CTU_DEV int16_t *lv_of(wctx *V, int color) { return color == 0 ? V->lv0 : (color == 1 ? V->lv1 : V->lv2); }
template <typename PX> CTU_DEV PX *plane(lds<PX> *S, int color) { return color == 0 ? S->Dy : (color == 1 ? S->Du : S->Dv); }
CTU_DEV int pitch_of(int color) { return color == 0 ? PY : PC; }
template <typename PX> CTU_DEV cu4 *cu_at(lds<PX> *S, int lx, int ly) { return &S->cu[((ly >> 2) + 1) * 17 + (lx >> 2) + 1]; }   // lx, ly >= -4

// uvg_count_available_edge_cus (cu.c:516-537) for a square CU at CTU-local (lx, ly)
template <typename PX> CTU_DEV int count_edge_cus(lds<PX> *S, int x, int y, int lx, int ly, int n, int left)
{
  if ((left && x == 0) || (!left && y == 0)) return 0;
  if (left && lx == 0) return (LCU - ly) / 4;
  if (!left && ly == 0) return n / 2;
  int amount = n & ~3;
  if (left) {
    if (ly == 0 && lx == 32 && cu_at(S, lx, ly)->log2 == 6) return 8;
    while (ly + amount < LCU && cu_at(S, lx - 4, ly + amount)->type != CU_NOTSET) amount += 4;
  } else {
    while (lx + amount < LCU && cu_at(S, lx + amount, ly - 4)->type != CU_NOTSET) amount += 4;
  }
  return (amount / 4) > (n / 4) ? amount / 4 : n / 4;
}

// uvg_intra_build_reference (intra.c:1344; _inner :1065-1341 when the block touches neither picture edge, _any :756-1063 else) for the
// w x w block of `color` whose luma position is (x, y) / CTU-local (lx, ly) with luma size n; + the smoothed rows (:190-225)
// cu_n: the size of the CU the block belongs to.  The smoothing filter covers 2 * (the CU's size) entries, not 2 * (the block's)
// (intra.c:715-725): in a 32x32 transform block of a 64x64 CU entry 2N is smoothed too, against the padding behind it.
template <typename PX> CTU_NOINLINE CTU_DEV void build_refs(lds<PX> *S, const params &P, int color, int x, int y, int lx, int ly, int n, int cu_n)
{
  wctx *const V = wv_of(S);
  const int c = color != 0;
  const int w = n >> c;
  const int px_x = lx >> c, px_y = ly >> c;
  const int pit = pitch_of(color);
  const PX *D = plane(S, color) + (px_y + 1) * pit + px_x + 1;     // the block's top-left sample
  SERIAL {
    int al = count_edge_cus(S, x, y, lx, ly, n, 1) * (c ? 2 : 4);
    if (al > 2 * w) al = 2 * w;
    if (al > ((P.pic_h - y) >> c)) al = (P.pic_h - y) >> c;
    int at = count_edge_cus(S, x, y, lx, ly, n, 0) * (c ? 2 : 4);
    if (at > 2 * w) at = 2 * w;
    if (at > ((P.pic_w - x) >> c)) at = (P.pic_w - x) >> c;
    if (x > 0 && y > 0 && P.wpp && px_y == 0 && at > (LCU >> c) - px_x) at = (LCU >> c) - px_x;
    V->u_avail_left = al; V->u_avail_top = at;
  }
  CTU_SYNC();
  const int al = V->u_avail_left, at = V->u_avail_top;
  const int dc = 1 << (px_info<PX>::depth - 1);
  CTU_LDS uint16_t *const r_top = LDSP(uint16_t, V->top), *const r_left = LDSP(uint16_t, V->left);
  CTU_LDS uint16_t *const r_ftop = LDSP(uint16_t, V->ftop), *const r_fleft = LDSP(uint16_t, V->fleft);
  PAR_FOR(i, V->refn - 1) {
    int lv, tv;
    if (x > 0) lv = D[(i < al ? i : al - 1) * pit - 1];
    else lv = y > 0 ? D[-pit] : dc;
    if (y > 0) tv = D[-pit + (i < at ? i : at - 1)];
    else tv = x > 0 ? D[-1] : dc;
    r_left[i + 1] = (uint16_t)lv;
    r_top[i + 1] = (uint16_t)tv;
  }
  SERIAL {
    int corner;
    if (x > 0 && y > 0) corner = D[-pit - 1];
    else corner = x > 0 ? D[-1] : (y > 0 ? D[-pit] : dc);       // "copy reference clockwise": left[1]
    r_left[0] = r_top[0] = (uint16_t)corner;
  }
  CTU_SYNC();
  const int flim = 2 * (cu_n >> c) < V->refn - 1 ? 2 * (cu_n >> c) : V->refn - 1;
  PAR_FOR(i, V->refn) {
    int fl, ft;
    if (i == 0) fl = ft = (r_left[1] + 2 * r_left[0] + r_top[1] + 2) >> 2;
    else {
      fl = i < flim ? (r_left[i - 1] + 2 * r_left[i] + r_left[i + 1] + 2) >> 2 : r_left[i];
      ft = i < flim ? (r_top[i - 1] + 2 * r_top[i] + r_top[i + 1] + 2) >> 2 : r_top[i];
    }
    r_fleft[i] = (uint16_t)fl;
    r_ftop[i] = (uint16_t)ft;
  }
  CTU_SYNC();
}

// prediction of the w x w block of `color` from the reference rows into dst (pitch dp)
template <typename PX> CTU_NOINLINE CTU_DEV void predict_block(lds<PX> *S, int mode, int color, int w, PX *dst_, int dp)
{
  wctx *const V = wv_of(S);
  const mode_info M = make_mode_info(mode, w, w, color != 0);
  const ref_rows_t<CTU_LDS const uint16_t *> R = {LDSP(const uint16_t, V->top), LDSP(const uint16_t, V->left), LDSP(const uint16_t, V->ftop), LDSP(const uint16_t, V->fleft)};
  const int dc = mode == 1 ? dc_value(R.top, R.left, w, w) : 0;
  typename mg_ptr<PX, PX>::type const dst = MGP(PX, PX, dst_);
  const int segs = w >> 2;
  PAR_FOR(t, w * segs) {
    const int yd = t / segs, xd0 = (t - yd * segs) * 4;
    int out[4];
    predict_row<4>(M, R, dc, color != 0, w, w, yd, xd0, (int)px_info<PX>::maxv, out);
    for (int i = 0; i < 4; ++i) {
      const int bx = M.vertical ? xd0 + i : yd, by = M.vertical ? yd : xd0 + i;
      dst[by * dp + bx] = (PX)out[i];
    }
  }
  CTU_SYNC();
}

// --------------------------------------------------------------------------------------------------- rough search ------
CTU_DEV int iabs_(int v) { return v < 0 ? -v : v; }
// 8x8 / 4x4 Hadamard SATD of a difference tile (picture-generic.c:118-200, 256-348); the magnitude multiset is transpose-invariant
CTU_DEV unsigned satd8_tile(int (&d)[64])
{
  for (int pass = 0; pass < 2; ++pass) {
    const int s = pass ? 8 : 1, t = pass ? 1 : 8;      // pass 0: along rows, pass 1: along columns
    for (int l = 0; l < 8; ++l) {
      int *v = &d[l * t];
      for (int half = 4; half >= 1; half >>= 1)
        for (int base = 0; base < 8; base += 2 * half)
          for (int i = 0; i < half; ++i) {
            const int p = v[(base + i) * s], q = v[(base + i + half) * s];
            v[(base + i) * s] = p + q;
            v[(base + i + half) * s] = p - q;
          }
    }
  }
  unsigned sad = 0;
  for (int i = 0; i < 64; ++i) sad += (unsigned)iabs_(d[i]);
  sad -= (unsigned)iabs_(d[0]);
  sad += (unsigned)iabs_(d[0]) >> 2;
  return (sad + 2) >> 2;
}
CTU_DEV unsigned satd4_tile(int (&d)[16])
{
  for (int pass = 0; pass < 2; ++pass) {
    const int s = pass ? 4 : 1, t = pass ? 1 : 4;
    for (int l = 0; l < 4; ++l) {
      int *v = &d[l * t];
      const int a = v[0] + v[2 * s], b = v[0] - v[2 * s], c2 = v[s] + v[3 * s], e = v[s] - v[3 * s];
      v[0] = a + c2; v[s] = a - c2; v[2 * s] = b + e; v[3 * s] = b - e;
    }
  }
  unsigned satd = 0;
  for (int i = 0; i < 16; ++i) satd += (unsigned)iabs_(d[i]);
  satd -= (unsigned)iabs_(d[0]);
  satd += (unsigned)iabs_(d[0]) >> 2;
  return (satd + 1) >> 1;
}

#if defined(__HIPCC__)
// the sum of v over the wave's lanes (wave-uniform).  All 64 lanes must be active.
CTU_DEV int rs_wave_sum(int v)
{
  v += dpp_xor1(v); v += dpp_xor2(v); v += dpp_mirror8(v); v += dpp_mirror16(v);          // every lane: the sum of its row of 16
  return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}
// rough_costs of a block of 8x8 or more on the device: 8x8 tiles, a lane per (mode, tile, row).  The angular modes of the list go
// through ang_row8 (intra_pred_dev.h) -- the eight modes of a sweep of an 8x8 block share one straight line of code, their
// parameters come from the leaf's LDS tables (lf_disp, lf_cubic), and whatever depends on the block's size alone is wave-uniform.
// Planar and DC, round 0's first two entries, are a short sweep of their own on predict_row; only there is the DC value needed:
// a sample per lane and a wave sum.  Sy: the block's source samples (pitch sps); modes: wctx::rs_list.
template <typename PX> CTU_INLINE1 CTU_DEV void rough_costs8(lds<PX> *S, CTU_GLB const PX *Sy, int sps_, int n_, const int32_t *modes_, int n_modes_)
{
  wctx *const V = wv_of(S);
  const int n = __builtin_amdgcn_readfirstlane(n_), n_modes = __builtin_amdgcn_readfirstlane(n_modes_), sps = __builtin_amdgcn_readfirstlane(sps_);
  const int log2n = 31 - __builtin_clz((unsigned)n), lt = log2n - 3, lt2 = 2 * lt;      // 1 << lt tiles in a row, 1 << lt2 in the block
  const int lane = CTU_TID, r = lane & 7, maxv = (int)px_info<PX>::maxv;
  CTU_LDS const int32_t *const modes = LDSP(const int32_t, modes_);
  CTU_LDS const uint32_t *const disp = LDSP(const uint32_t, S->lf_disp), *const cubic = LDSP(const uint32_t, S->lf_cubic);
  const ref_rows_t<CTU_LDS const uint16_t *> R = {LDSP(const uint16_t, V->top), LDSP(const uint16_t, V->left), LDSP(const uint16_t, V->ftop), LDSP(const uint16_t, V->fleft)};
  CTU_LDS uint32_t *const part = LDSP(uint32_t, V->part);
  const int n_flat = __builtin_amdgcn_readfirstlane((n_modes > 0 && modes[0] < 2) + (n_modes > 1 && modes[1] < 2));
  {
    const int total = (n_modes - n_flat) << (lt2 + 3);
    for (int base = 0; base < total; base += CTU_NT) {
      const int idx = base + lane;
      const bool on = idx < total;
      const int task = (on ? idx >> 3 : 0) + (n_flat << lt2);
      const int mi = task >> lt2, tile = task & ((1 << lt2) - 1), wy = (tile >> lt) * 8 + r, wx0 = (tile & ((1 << lt) - 1)) * 8;
      const auto M = make_ang_mode(R, disp, modes[mi], log2n);
      // the source samples of the work domain's row: a row of the block, or a column of it for the horizontal modes.  Every lane
      // loads (a lane past the end has the first task's address), and all eight loads are out before the row is predicted
      CTU_GLB const PX *const sp = Sy + (M.vertical ? wy * sps + wx0 : wx0 * sps + wy);
      const int step = M.vertical ? 1 : sps;
      int src[8], d[8], out[8], sad = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) src[i] = (int)sp[i * step];
      ang_row8(M, cubic, n, wy, wx0, maxv, out);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        d[i] = on ? src[i] - out[i] : 0;
        sad += iabs_(d[i]);
      }
      const int satd = satd8_cost(d, r);
      sad = dpp_group_sum<8>(sad);
      if (on && r == 0) { part[2 * task] = (uint32_t)satd; part[2 * task + 1] = (uint32_t)sad; }
    }
  }
  if (n_flat > 0) {
    int acc = 0;                                // dc_value (intra.c:236-273) of a square block: top[1 .. n] + left[1 .. n]
    for (int i = lane; i < 2 * n; i += CTU_NT) acc += (int)*(i < n ? R.top + 1 + i : R.left + 1 + i - n);
    const int dcv = (rs_wave_sum(acc) + n) >> (log2n + 1);
    const int total = n_flat << (lt2 + 3);
    for (int base = 0; base < total; base += CTU_NT) {
      const int idx = base + lane;
      const bool on = idx < total;
      const int task = on ? idx >> 3 : 0;
      const int mi = task >> lt2, tile = task & ((1 << lt2) - 1), wy = (tile >> lt) * 8 + r, wx0 = (tile & ((1 << lt) - 1)) * 8;
      const mode_info M = make_mode_info(modes[mi] != 0, n, n, 0);          // planar or DC
      int src[8], d[8], out[8], sad = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) src[i] = (int)Sy[wy * sps + wx0 + i];
      predict_row<8>(M, R, dcv, 0, n, n, wy, wx0, maxv, out);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        d[i] = on ? src[i] - out[i] : 0;
        sad += iabs_(d[i]);
      }
      const int satd = satd8_cost(d, r);
      sad = dpp_group_sum<8>(sad);
      if (on && r == 0) { part[2 * task] = (uint32_t)satd; part[2 * task + 1] = (uint32_t)sad; }
    }
  }
  CTU_SYNC();
}
#endif

// costs of the listed modes for the n x n luma block at (lx, ly); get_cost_dual (search_intra.c:133-192).
// Device: every (mode, tile, row) is one lane -- a lane predicts one row of the tile in registers (in the mode's work domain:
// transposed for the horizontal modes; SAD and the Hadamard magnitude multiset are transpose-invariant), the T lanes of a tile
// finish the Hadamard with DPP exchanges (satd_dev.h): rough_costs8 above, the loop below for a 4x4 block.  Host emulation: the
// tile as a whole.
template <typename PX> CTU_NOINLINE CTU_DEV void rough_costs(lds<PX> *S, const job<PX> &J, int lx, int ly, int n, const int32_t *modes, int n_modes)
{
  wctx *const V = wv_of(S);
  int sps;
  CTU_GLB const PX *Sy = src_block(J, 0, lx, ly, &sps);
  const int T = n >= 8 ? 8 : 4, tiles_x = n / T, tiles = tiles_x * tiles_x;
#if defined(__HIPCC__)
  if (T == 8) { rough_costs8(S, Sy, sps, n, modes, n_modes); return; }      // (no DC value unless DC is listed)
#endif
  const ref_rows_t<CTU_LDS const uint16_t *> R = {LDSP(const uint16_t, V->top), LDSP(const uint16_t, V->left), LDSP(const uint16_t, V->ftop), LDSP(const uint16_t, V->fleft)};
  const int dcv = dc_value(R.top, R.left, n, n);
  CTU_LDS uint32_t *const part = LDSP(uint32_t, V->part);
#if defined(__HIPCC__)
  // Two segments: the angular modes of the list, then planar / DC (the first round's list starts with them).  A pass whose lanes
  // are all of one kind skips the other kind's code (no lane enters it); mixed passes would run both for everybody -- for a 4x4
  // block 16 angular modes x 4 rows fill one pass exactly and planar + DC become a short second one.
  const int n_flat = (n_modes > 0 && modes[0] < 2) + (n_modes > 1 && modes[1] < 2);
  for (int seg = 0; seg < 2; ++seg) {
  const int m_first = seg ? 0 : n_flat, total = (seg ? n_flat : n_modes - n_flat) * tiles * T;
  for (int base = 0; base < total; base += CTU_NT) {
    const int idx = base + CTU_TID;
    const bool on = idx < total;
    const int task0 = on ? idx / T : 0, r = idx & (T - 1);
    const int task = task0 + m_first * tiles;
    const int mi = task / tiles;
    const mode_info M = make_mode_info(modes[mi], n, n, 0);
    int sad = 0, satd;
    {
      int d[4], out[4];
      predict_row<4>(M, R, dcv, 0, n, n, r, 0, (int)px_info<PX>::maxv, out);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int bx = M.vertical ? i : r, by = M.vertical ? r : i;
        d[i] = on ? (int)Sy[by * sps + bx] - out[i] : 0;
        sad += iabs_(d[i]);
      }
      satd = satd4_cost(d, r);
      sad = dpp_group_sum<4>(sad);
    }
    if (on && r == 0) { part[2 * task] = (uint32_t)satd; part[2 * task + 1] = (uint32_t)sad; }
  }
  }
  CTU_SYNC();
#else
  PAR_FOR(task, n_modes * tiles) {
    const int mi = task / tiles, tile = task - mi * tiles;
    const int mode = modes[mi];
    const mode_info M = make_mode_info(mode, n, n, 0);
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    unsigned sad = 0, satd;
    if (T == 8) {
      int d[64];
      for (int r = 0; r < 8; ++r) {
        int out[8];
        predict_row<8>(M, R, dcv, 0, n, n, ty * 8 + r, tx * 8, (int)px_info<PX>::maxv, out);
        for (int i = 0; i < 8; ++i) {
          const int wx = tx * 8 + i, wy = ty * 8 + r;
          const int bx = M.vertical ? wx : wy, by = M.vertical ? wy : wx;
          const int df = (int)Sy[by * sps + bx] - out[i];
          d[r * 8 + i] = df;
          sad += (unsigned)iabs_(df);
        }
      }
      satd = satd8_tile(d);
    } else {
      int d[16];
      for (int r = 0; r < 4; ++r) {
        int out[4];
        predict_row<4>(M, R, dcv, 0, n, n, r, 0, (int)px_info<PX>::maxv, out);
        for (int i = 0; i < 4; ++i) {
          const int bx = M.vertical ? i : r, by = M.vertical ? r : i;
          const int df = (int)Sy[by * sps + bx] - out[i];
          d[r * 4 + i] = df;
          sad += (unsigned)iabs_(df);
        }
      }
      satd = satd4_tile(d);
    }
    part[2 * task] = satd;
    part[2 * task + 1] = sad;
  }
  CTU_SYNC();
#endif
}

#if defined(__HIPCC__)
// ---- the rough search's selection on one wave, the candidates where their costs are: in the lanes' registers ----
// The reference keeps a three-entry list under strict "<" insertion (search_intra.c:1071-1215): the three smallest of everything
// listed so far under (cost, insertion sequence).  A cost is >= +0, so its bit pattern orders like its value: the key.
CTU_DEV uint64_t rs_key(double c) { return (uint64_t)(uint32_t)__double2hiint(c) << 32 | (uint32_t)__double2loint(c); }
// the smallest value of the wave's lanes (wave-uniform): six DPP steps, the last two across the rows of 16.  All 64 lanes must be
// active: a lane that is not reads as 0 in the first four steps.
CTU_DEV uint32_t rs_wave_min(uint32_t v)
{
#define RS_MIN(x) { const uint32_t o = (uint32_t)(x); v = o < v ? o : v; }
  RS_MIN(__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true));           // quad_perm [1,0,3,2]
  RS_MIN(__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true));           // quad_perm [2,3,0,1]
  RS_MIN(__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true));          // row_half_mirror
  RS_MIN(__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, true));          // row_mirror
  RS_MIN(__builtin_amdgcn_update_dpp((int)v, (int)v, 0x142, 0xa, 0xf, false));    // row_bcast:15 into rows 1 and 3
  RS_MIN(__builtin_amdgcn_update_dpp((int)v, (int)v, 0x143, 0xc, 0xf, false));    // row_bcast:31 into rows 2 and 3
#undef RS_MIN
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// a candidate that is not in a lane: wave-uniform
struct rs_extra { bool on; uint64_t key; int seq, mode; };
struct rs_pick { int who; uint64_t key; };              // who: the lane, 64: the extra; key ~0: there was no candidate
CTU_DEV bool rs_key_lt(uint32_t khi, uint32_t klo, uint64_t k) { return ((uint64_t)khi << 32 | klo) < k; }
// the smallest candidate under (key, seq) among the lanes (on; key = khi : klo; seq >= 0, no two candidates with the same) and,
// X, the extra: the minimum of the high words, among those that have it of the low words, among those of the sequence.  Most
// picks end early: a lone candidate needs no reduction, and a high word that only one candidate has decides (costs that differ
// at all nearly always differ there; the full ladder is for the ties of flat content).
template <bool X> CTU_DEV rs_pick rs_pick_min(bool on, uint32_t khi, uint32_t klo, int seq, const rs_extra &x)
{
  const uint32_t none = 0xffffffffu;
  const uint32_t xh = (uint32_t)(x.key >> 32), xl = (uint32_t)x.key;
  const bool xon = X && x.on;
  rs_pick r;
  const unsigned long long b_on = __ballot(on);
  const int n_on = __popcll(b_on) + (xon ? 1 : 0);
  if (n_on == 0) { r.who = 0; r.key = ~0ull; return r; }
  uint32_t mh = 0;
  unsigned long long b1 = b_on;
  bool y = xon;
  if (n_on > 1) {
    mh = rs_wave_min(on ? khi : none);
    if (xon && xh < mh) mh = xh;
    b1 = __ballot(on && khi == mh);
    y = xon && xh == mh;
  }
  if (__popcll(b1) + (y ? 1 : 0) == 1) {
    if (y) { r.who = 64; r.key = x.key; }
    else {
      r.who = __builtin_ctzll(b1);
      r.key = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)khi, r.who) << 32 | (uint32_t)__builtin_amdgcn_readlane((int)klo, r.who);
    }
    return r;
  }
  const bool t1 = on && khi == mh;
  uint32_t ml = rs_wave_min(t1 ? klo : none);
  if (y && xl < ml) ml = xl;
  const bool t2 = t1 && klo == ml, z = y && xl == ml;
  uint32_t ms = rs_wave_min(t2 ? (uint32_t)seq : none);
  r.key = (uint64_t)mh << 32 | ml;
  if (z && (uint32_t)x.seq < ms) r.who = 64;
  else {
    const unsigned long long w = __ballot(t2 && (uint32_t)seq == ms);
    r.who = w ? __builtin_ctzll(w) : 0;
  }
  return r;
}
// the survivors in rank order; a newcomer goes behind every entry that is not larger (strict "<", search_intra.c:1133-1142)
struct rs_top3 { int m[3]; uint64_t k[3]; };
CTU_DEV void rs_insert(rs_top3 &B, int mode, uint64_t key)
{
  if (key < B.k[0]) { B.k[2] = B.k[1]; B.m[2] = B.m[1]; B.k[1] = B.k[0]; B.m[1] = B.m[0]; B.k[0] = key; B.m[0] = mode; }
  else if (key < B.k[1]) { B.k[2] = B.k[1]; B.m[2] = B.m[1]; B.k[1] = key; B.m[1] = mode; }
  else if (key < B.k[2]) { B.k[2] = key; B.m[2] = mode; }
}
// one round's newcomers (a lane's: on, its key, sequence and mode; X: and the extra) into the survivors: their minima one at a
// time, inserted the way the reference inserts, until none is left below the third survivor -- what is not below it cannot enter,
// now or later in the round
template <bool X> CTU_DEV void rs_round(rs_top3 &B, bool on, uint32_t khi, uint32_t klo, int seq, int mode, rs_extra x)
{
  for (int i = 0; i < 3; ++i) {
    on = on && rs_key_lt(khi, klo, B.k[2]);
    if (X) x.on = x.on && x.key < B.k[2];
    const rs_pick pk = rs_pick_min<X>(on, khi, klo, seq, x);
    if (pk.key == ~0ull) break;
    rs_insert(B, pk.who < 64 ? __builtin_amdgcn_readlane(mode, pk.who) : x.mode, pk.key);
    on = on && CTU_TID != pk.who;
    if (X) x.on = x.on && pk.who != 64;
  }
}
#endif

// count_bits (search_intra.c:949-984)
CTU_DEV double count_bits(const int8_t *preds, double planar, double not_planar, double mpm_bit, double not_mpm_bit, int mode)
{
  int i = 0, smaller = 0;
  for (; i < 6; i++) {
    if (preds[i] == mode) break;
    if (mode > preds[i]) smaller += 1;
  }
  if (i == 0) return planar + mpm_bit;
  if (i < 6) return not_planar + mpm_bit + (i < 4 ? i : 4);
  return not_mpm_bit + 5 + (mode - smaller > 2);
}

// uvg_intra_get_dir_luma_predictor (intra.c:88-188), MIP off
CTU_DEV void dir_luma_predictor(int y, int8_t *preds, const cu4 *left_pu, const cu4 *above_pu)
{
  int left_dir = 0, above_dir = 0;
  if (left_pu && left_pu->type == CU_INTRA) left_dir = left_pu->mode;
  if (above_pu && above_pu->type == CU_INTRA && y % LCU != 0) above_dir = above_pu->mode;
  const int offset = 61, mod = 64;
  preds[0] = 0; preds[1] = 1; preds[2] = 50; preds[3] = 18; preds[4] = 46; preds[5] = 54;
  if (left_dir == above_dir) {
    if (left_dir > 1) {
      preds[0] = 0; preds[1] = (int8_t)left_dir;
      preds[2] = (int8_t)(((left_dir + offset) % mod) + 2); preds[3] = (int8_t)(((left_dir - 1) % mod) + 2);
      preds[4] = (int8_t)(((left_dir + offset - 1) % mod) + 2); preds[5] = (int8_t)((left_dir % mod) + 2);
    }
  } else if (left_dir > 1 && above_dir > 1) {
    preds[0] = 0; preds[1] = (int8_t)left_dir; preds[2] = (int8_t)above_dir;
    const int mx = preds[1] > preds[2] ? 1 : 2, mn = preds[1] > preds[2] ? 2 : 1;
    const int diff = preds[mx] - preds[mn];
    if (diff == 1) {
      preds[3] = (int8_t)(((preds[mn] + offset) % mod) + 2); preds[4] = (int8_t)(((preds[mx] - 1) % mod) + 2);
      preds[5] = (int8_t)(((preds[mn] + offset - 1) % mod) + 2);
    } else if (diff >= 62) {
      preds[3] = (int8_t)(((preds[mn] - 1) % mod) + 2); preds[4] = (int8_t)(((preds[mx] + offset) % mod) + 2);
      preds[5] = (int8_t)((preds[mn] % mod) + 2);
    } else if (diff == 2) {
      preds[3] = (int8_t)(((preds[mn] - 1) % mod) + 2); preds[4] = (int8_t)(((preds[mn] + offset) % mod) + 2);
      preds[5] = (int8_t)(((preds[mx] - 1) % mod) + 2);
    } else {
      preds[3] = (int8_t)(((preds[mn] + offset) % mod) + 2); preds[4] = (int8_t)(((preds[mn] - 1) % mod) + 2);
      preds[5] = (int8_t)(((preds[mx] + offset) % mod) + 2);
    }
  } else if (left_dir + above_dir >= 2) {
    preds[0] = 0;
    preds[1] = (int8_t)(left_dir < above_dir ? above_dir : left_dir);
    preds[2] = (int8_t)(((preds[1] + offset) % mod) + 2); preds[3] = (int8_t)(((preds[1] - 1) % mod) + 2);
    preds[4] = (int8_t)(((preds[1] + offset - 1) % mod) + 2); preds[5] = (int8_t)((preds[1] % mod) + 2);
  }
}
// the two neighbours uvg_search_cu_intra (search_intra.c:1792-1803) and uvg_encode_intra_luma_coding_unit (:1114-1150) look at
template <typename PX> CTU_DEV void mpm_neighbours(lds<PX> *S, int x, int y, int lx, int ly, int n, const cu4 **left, const cu4 **above)
{
  *left = x > 0 ? cu_at(S, lx - 1, ly + n - 1) : nullptr;
  *above = (ly > 0 && y > 0) ? cu_at(S, lx + n - 1, ly - 1) : nullptr;
}

// search_intra_rough (search_intra.c:986-1229), three survivors; the winner goes to V->u_mode, its cost to V->rs_cand[0]
#if defined(__HIPCC__)
// Device: a lane per listed mode keeps the mode's cost in its registers and the three survivors are wave-uniform values -- the
// minima of a round's newcomers are taken one at a time and inserted the way the reference inserts (rs_round), the
// next round's list is derived in the lanes 0..5, a lane per try.  Only the list itself goes through LDS (rough_costs reads it).
// The host emulation below is the reference's serial walk; the two agree only if this one is right.
template <typename PX> CTU_INLINE1 CTU_DEV void search_intra_rough(lds<PX> *S, const job<PX> &J, int x, int y, int lx, int ly, int n)
{
  wctx *const V = wv_of(S);
  const params &P = J.P;
  const int T = n >= 8 ? 8 : 4, tiles = (n / T) * (n / T);
  const int lane = CTU_TID;
  RQ_T0(J.W)
  SERIAL {
    const cu4 *l, *a;
    mpm_neighbours(S, x, y, lx, ly, n, &l, &a);
    dir_luma_predictor(y, V->mpm, l, a);
  }
  // round 0's list: planar, DC, every 2^levels-th angular mode from 2 + 2^levels / 2 (search_intra.c:1071-1143); the modes listed so
  // far are a bit each of h0 : h1 : h2 (the same pattern in every word: 32 is a multiple of the step)
  int offset = 1 << __builtin_amdgcn_readfirstlane(P.rough_levels);
  const int first_m = 2 + offset / 2;
  int nm = 2 + (66 - first_m) / offset + 1;
  if (lane < nm) V->rs_list[lane] = lane < 2 ? lane : first_m + (lane - 2) * offset;
  uint32_t pat = 1u << (first_m & (offset - 1));
  for (int sh = offset; sh < 32; sh <<= 1) pat |= pat << sh;
  uint32_t h0 = (pat & ~((1u << first_m) - 1u)) | 3u, h1 = pat, h2 = pat & 7u;
  CTU_SYNC();
  RQ_T(24);
  CTU_LDS const uint32_t *const mdl = LDSP(const uint32_t, V->cur), *const part = LDSP(const uint32_t, V->part);
  const double mpm_bit = m_fbits(mdl, M_MPM, 1), not_mpm_bit = m_fbits(mdl, M_MPM, 0);
  const double planar = m_fbits(mdl, M_PLANAR + 1, 0), not_planar = m_fbits(mdl, M_PLANAR + 1, 1);
  const rs_extra none = {false, 0, 0, 0};
  rs_top3 B = {{0, 0, 0}, {~0ull, ~0ull, ~0ull}};
  bool differs = false;
  for (int round = 0;; ++round) {
    rough_costs(S, J, lx, ly, n, V->rs_list, nm);
    RQ_T(25);
    bool on = lane < nm;
    int mode = 0;
    uint32_t khi = 0, klo = 0;
    if (on) {                                   // a lane per mode: tile sums, bit cost
      mode = V->rs_list[lane];
      unsigned satd = 0, sad = 0;
      for (int t = 0; t < tiles; ++t) { satd += part[2 * (lane * tiles + t)]; sad += part[2 * (lane * tiles + t) + 1]; }
      if (n >= 8) satd >>= (px_info<PX>::depth - 8);       // satd_NxN shifts, the 4x4 function does not (picture-generic.c:170)
      sad >>= (px_info<PX>::depth - 8);
      double c = (double)(satd < sad * 2 ? satd : sad * 2);
      c += count_bits(V->mpm, planar, not_planar, mpm_bit, not_mpm_bit, mode) * P.lambda_sqrt;
      khi = (uint32_t)__double2hiint(c); klo = (uint32_t)__double2loint(c);
    }
    RQ_T(26);
    // the newcomers in the order the reference inserts them: the list's order, DC ahead of planar (:1089-1106)
    const int seq = (round == 0 && lane < 2) ? 1 - lane : lane;
    if (round == 0)                             // min_cost != max_cost (:1082-1143): only the first round moves them
      differs = __ballot(on && (khi != (uint32_t)__builtin_amdgcn_readlane((int)khi, 0) || klo != (uint32_t)__builtin_amdgcn_readlane((int)klo, 0))) != 0;
    rs_round<false>(B, on, khi, klo, seq, mode, none);
    // next round's list (search_intra.c:1146-1215): lane j tries b - off (j even) / b + off (j odd) of survivor j / 2; a mode is
    // listed where it is first tried and only if it was never listed; a survivor outside 3..65 lists nothing
    offset >>= 1;
    if (!(offset > 0 && differs)) break;
    int tu[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int b = B.m[j >> 1], m = (j & 1) ? b + offset : b - offset;
      tu[j] = (b >= 3 && b <= 65 && m >= 2 && m <= 66) ? m : -1;
    }
    const int t = lane == 0 ? tu[0] : lane == 1 ? tu[1] : lane == 2 ? tu[2] : lane == 3 ? tu[3] : lane == 4 ? tu[4] : lane == 5 ? tu[5] : -1;
    bool listed = t >= 0 && !(((t < 32 ? h0 : (t < 64 ? h1 : h2)) >> (t & 31)) & 1u);
#pragma unroll
    for (int j = 0; j < 5; ++j) listed = listed && !(lane > j && tu[j] == t);
    const unsigned long long lm = __ballot(listed);
    if (listed) V->rs_list[__popcll(lm & ((1ull << lane) - 1ull))] = t;
    nm = __popcll(lm);
#pragma unroll
    for (int j = 0; j < 6; ++j)
      if (tu[j] >= 0) { const uint32_t bit = 1u << (tu[j] & 31); if (tu[j] < 32) h0 |= bit; else if (tu[j] < 64) h1 |= bit; else h2 |= bit; }
    CTU_SYNC();
    RQ_T(27);
  }
  SERIAL {
    V->u_mode = B.m[0];
    V->rs_cand[0] = __hiloint2double((int)(uint32_t)(B.k[0] >> 32), (int)(uint32_t)B.k[0]);
  }
  CTU_SYNC();
  RQ_T(27);
}
#else
// Host: the reference's walk as it stands (search_intra.c:1071-1215) -- one candidate at a time into a three-entry list.
template <typename PX> CTU_INLINE1 CTU_DEV void search_intra_rough(lds<PX> *S, const job<PX> &J, int x, int y, int lx, int ly, int n)
{
  wctx *const V = wv_of(S);
  const params &P = J.P;
  const int T = n >= 8 ? 8 : 4, tiles = (n / T) * (n / T);
  const cu4 *l, *a;
  mpm_neighbours(S, x, y, lx, ly, n, &l, &a);
  dir_luma_predictor(y, V->mpm, l, a);
  const double mpm_bit = m_fbits(V->cur, M_MPM, 1), not_mpm_bit = m_fbits(V->cur, M_MPM, 0);
  const double planar = m_fbits(V->cur, M_PLANAR + 1, 0), not_planar = m_fbits(V->cur, M_PLANAR + 1, 1);
  // round 0's list: planar, DC, every 2^levels-th angular mode from 2 + 2^levels / 2 (18 entries with rough_levels >= 2; the host
  // refuses smaller values)
  int offset = 1 << P.rough_levels;
  int32_t list[24];
  bool listed[67] = {};
  int nm = 0;
  list[nm++] = 0; list[nm++] = 1;
  for (int m = 2 + offset / 2; m <= 66; m += offset) list[nm++] = m;
  for (int i = 0; i < nm; ++i) listed[list[i]] = true;
  double best_cost[3] = {CTU_MAX_DOUBLE, CTU_MAX_DOUBLE, CTU_MAX_DOUBLE};
  int best_mode[3] = {0, 0, 0};
  bool differs = false;
  for (int round = 0;; ++round) {
    rough_costs(S, J, lx, ly, n, list, nm);
    double cost[24];
    for (int mi = 0; mi < nm; ++mi) {           // tile sums, bit cost
      unsigned satd = 0, sad = 0;
      for (int t = 0; t < tiles; ++t) { satd += V->part[2 * (mi * tiles + t)]; sad += V->part[2 * (mi * tiles + t) + 1]; }
      if (n >= 8) satd >>= (px_info<PX>::depth - 8);       // satd_NxN shifts, the 4x4 function does not (picture-generic.c:170)
      sad >>= (px_info<PX>::depth - 8);
      cost[mi] = (double)(satd < sad * 2 ? satd : sad * 2) + count_bits(V->mpm, planar, not_planar, mpm_bit, not_mpm_bit, list[mi]) * P.lambda_sqrt;
      if (round == 0) differs = differs || cost[mi] != cost[0];          // min_cost != max_cost (:1082-1143): only the first round moves them
    }
    for (int i = 0; i < nm; ++i) {
      const int mi = (round == 0 && i < 2) ? 1 - i : i;                  // DC ahead of planar (:1089-1106)
      for (int j = 0; j < 3; ++j)
        if (cost[mi] < best_cost[j]) {
          for (int k = 2; k > j; --k) { best_cost[k] = best_cost[k - 1]; best_mode[k] = best_mode[k - 1]; }
          best_cost[j] = cost[mi]; best_mode[j] = list[mi];
          break;
        }
    }
    // next round's list (:1146-1215): b -+ offset of each survivor in 3..65; a mode is listed where it is first tried and only if it
    // was never listed.  An empty list still runs the remaining rounds.
    offset >>= 1;
    if (!(offset > 0 && differs)) break;
    nm = 0;
    for (int j = 0; j < 3; ++j) {
      const int b = best_mode[j];
      if (b < 3 || b > 65) continue;
      for (int m = b - offset; m <= b + offset; m += 2 * offset)
        if (m >= 2 && m <= 66 && !listed[m]) { listed[m] = true; list[nm++] = m; }
    }
  }
  V->u_mode = best_mode[0];
  V->rs_cand[0] = best_cost[0];
}
#endif

// ---------------------------------------------------------------------------------------------------- transforms ------
CTU_DEV const int16_t *dct2_matrix(int n) { return n == 4 ? VVC_DCT2_4 : n == 8 ? VVC_DCT2_8 : n == 16 ? VVC_DCT2_16 : VVC_DCT2_32; }
// dct_NxN (dct-generic.c:396-419, 720-729): dst[j * n + i] = trunc16((sum_k T[j][k] * src[i][k] + add) >> shift), twice
CTU_NOINLINE CTU_DEV void fwd_pass(int n, const int16_t *src_, int16_t *dst_, int shift)
{
  CTU_LDS const int16_t *const src = LDSP(const int16_t, src_);
  CTU_LDS int16_t *const dst = LDSP(int16_t, dst_);
  const int16_t *T = dct2_matrix(n);
  const int add = shift > 0 ? 1 << (shift - 1) : 0;
  PAR_FOR(e, n * n) {
    const int j = e / n, i = e - j * n;
    int acc = 0;
    for (int k = 0; k < n; ++k) acc += (int)T[j * n + k] * src[i * n + k];
    dst[j * n + i] = (int16_t)((acc + add) >> shift);
  }
  CTU_SYNC();
}
// idct_NxN (:422-446, 731-740): dst[i * n + j] = clip16((sum_k src[k * n + i] * T[k][j] + add) >> shift), twice
CTU_NOINLINE CTU_DEV void inv_pass(int n, const int16_t *src_, int16_t *dst_, int shift)
{
  CTU_LDS const int16_t *const src = LDSP(const int16_t, src_);
  CTU_LDS int16_t *const dst = LDSP(int16_t, dst_);
  const int16_t *T = dct2_matrix(n);
  const int add = 1 << (shift - 1);
  PAR_FOR(e, n * n) {
    const int i = e / n, j = e - i * n;
    int acc = 0;
    for (int k = 0; k < n; ++k) acc += (int)src[k * n + i] * T[k * n + j];
    dst[i * n + j] = (int16_t)clampi((acc + add) >> shift, -32768, 32767);
  }
  CTU_SYNC();
}

// ----------------------------------------------------------------------------------------------------------- RDOQ ------
CTU_DEV int group_idx(int pos)
{
  if (pos < 4) return pos;
  int l = 0;
  while ((pos >> (l + 1)) != 0) ++l;
  return 2 * l + ((pos >> (l - 1)) & 1);
}
CTU_DEV int go_rice_par(unsigned s) { return (s >= 7) + (s >= 14) + (s >= 28); }

struct rdoq_env {
  const uint8_t *st;      // CTX_STATE per model
  int t;                  // 0 luma, 1 chroma
  double lambda, error_scale;
  int q_bits, q;
};
CTU_DEV int32_t rbits(const rdoq_env &E, int model, int bin) { return (int32_t)tab_rdoq_bits()[2 * model + bin]; }

// uvg_get_ic_rate (rdo.c:465-581), limited prefix length
CTU_DEV int32_t ic_rate(const rdoq_env &E, uint32_t abs_level, int ctx, int go_rice, uint32_t reg_bins)
{
  int32_t rate = 1 << 15;
  const uint32_t go_rice_zero = 1u << go_rice;
  const int max_log2 = 15, thr = 5;
  const int o_par = M_PAR + (E.t ? 21 : 0) + ctx, o_gt1 = M_GT1 + (E.t ? 21 : 0) + ctx, o_gt2 = M_GT2 + (E.t ? 21 : 0) + ctx;
  if (reg_bins < 4) {
    const uint32_t symbol = (abs_level == 0 ? go_rice_zero : abs_level <= go_rice_zero ? abs_level - 1 : abs_level);
    if (symbol < ((uint32_t)thr << go_rice)) {
      rate += (int32_t)(((symbol >> go_rice) + 1 + go_rice) << 15);
    } else {
      const uint32_t max_prefix = 32 - (thr + max_log2);
      uint32_t prefix = 0;
      const uint32_t suffix = (symbol >> go_rice) - thr;
      while (prefix < max_prefix && (int32_t)suffix > ((2 << prefix) - 2)) prefix++;
      const uint32_t suffix_len = prefix == max_prefix ? (uint32_t)(max_log2 - go_rice) : prefix + 1;
      rate += (int32_t)((thr + prefix + suffix_len + go_rice) << 15);
    }
    return rate;
  }
  if (abs_level >= 4) {
    const int32_t symbol = (int32_t)abs_level - 4;
    if (symbol < (thr << go_rice)) {
      rate += ((symbol >> go_rice) + 1 + go_rice) << 15;
    } else {
      const uint32_t max_prefix = 32 - (thr + max_log2);
      uint32_t prefix = 0;
      const uint32_t suffix = (uint32_t)(symbol >> go_rice) - thr;
      while (prefix < max_prefix && (int32_t)suffix > ((2 << prefix) - 2)) prefix++;
      const uint32_t suffix_len = prefix == max_prefix ? (uint32_t)(max_log2 - go_rice) : prefix + 1;
      rate += (int32_t)((thr + prefix + suffix_len + go_rice) << 15);
    }
    rate += rbits(E, o_par, (abs_level - 2) & 1);
    rate += rbits(E, o_gt1, 1);
    rate += rbits(E, o_gt2, 1);
  } else if (abs_level == 1) {
    rate += rbits(E, o_gt1, 0);
  } else if (abs_level == 2) {
    rate += rbits(E, o_par, 0); rate += rbits(E, o_gt1, 1); rate += rbits(E, o_gt2, 0);
  } else if (abs_level == 3) {
    rate += rbits(E, o_par, 1); rate += rbits(E, o_gt1, 1); rate += rbits(E, o_gt2, 0);
  } else {
    rate = 0;
  }
  return rate;
}

// uvg_get_coded_level (rdo.c:597-640)
CTU_DEV uint32_t coded_level(const rdoq_env &E, double *coded_cost, double coded_cost0, double *coded_cost_sig, int32_t level_double,
                             uint32_t max_abs_level, int ctx_sig, int ctx_set, int go_rice, uint32_t reg_bins, int last)
{
  double cur_cost_sig = 0;
  uint32_t best = 0;
  const int o_sig = M_SIG + (E.t ? 12 : 0) + ctx_sig;
  if (!last && max_abs_level < 3) {
    *coded_cost_sig = E.lambda * rbits(E, o_sig, 0);
    *coded_cost = coded_cost0 + *coded_cost_sig;
    if (max_abs_level == 0) return best;
  } else {
    *coded_cost = 1.7e+308;
  }
  if (!last) cur_cost_sig = E.lambda * rbits(E, o_sig, 1);
  const int32_t min_abs = max_abs_level > 1 ? (int32_t)max_abs_level - 1 : 1;
  for (int32_t a = (int32_t)max_abs_level; a >= min_abs; a--) {
    const double err = (double)(level_double - (a * (1 << E.q_bits)));
    double cur = err * err * E.error_scale + E.lambda * ic_rate(E, (uint32_t)a, ctx_set, go_rice, reg_bins);
    cur += cur_cost_sig;
    if (cur < *coded_cost) { best = (uint32_t)a; *coded_cost = cur; *coded_cost_sig = cur_cost_sig; }
  }
  return best;
}

// coded_level as straight-line code: what every lane of a wave runs when the lanes hold different levels (the device's call sites;
// the host emulation's rdoq_serial keeps coded_level, and tests/test_rdoq_level_decision.py holds the two together bit for bit).
//   * the two bin costs of a model lie side by side in tab_rdoq_bits(): the pairs of the significance, parity, greater-1 and
//     greater-2 models are read once, in front of everything, and serve both candidates and "not significant";
//   * both candidates -- a1 = max_abs_level, a2 = max_abs_level - 1, each >= 1 -- are priced, and a predicate says which count;
//   * the rate's terms are integers (their order is free); the doubles are the reference's, in the reference's order.
// The escape code of uvg_get_ic_rate (Golomb-Rice up to 5 << rice, then exp-Golomb with the prefix capped at 12) without its loop:
// the prefix is floor(log2(suffix + 1)).
CTU_DEV int32_t rq_escape_rate(int32_t symbol, int go_rice)
{
  const int32_t q = symbol >> go_rice;
  const bool rice_code = q < 5;
  const uint32_t arg = rice_code ? 1u : (uint32_t)(q - 4);          // (never 0: clz(0) is undefined)
  const int32_t log2 = 31 - (int32_t)__builtin_clz(arg);
  const int32_t prefix = log2 < 12 ? log2 : 12;
  const int32_t suffix_len = prefix == 12 ? 15 - go_rice : prefix + 1;
  return (rice_code ? q + 1 + go_rice : 5 + prefix + suffix_len + go_rice) << 15;
}
struct rq_pair { int32_t b0, b1; };
CTU_DEV rq_pair rbits2(int model)
{
  CTU_LDS const uint32_t *const p = LDSP(const uint32_t, tab_rdoq_bits()) + 2 * model;
  rq_pair r;
  r.b0 = (int32_t)p[0]; r.b1 = (int32_t)p[1];
  return r;
}
// uvg_get_ic_rate (limited prefix length) of a level a >= 1
CTU_DEV int32_t rq_level_rate(int32_t a, bool regular, int go_rice, rq_pair par, rq_pair gt1, rq_pair gt2)
{
  // regular: greater-1; from 2 on parity and greater-2; from 4 on the escape code of a - 4.  Bypass: the escape code of the level
  // itself, with the levels up to 1 << rice moved down by one (level 0 has their place)
  const int32_t s_reg = a - 4, s_byp = a <= (1 << go_rice) ? a - 1 : a;
  const int32_t s = regular ? (s_reg > 0 ? s_reg : 0) : s_byp;
  const int32_t esc = rq_escape_rate(s, go_rice);
  const int32_t flags = (a >= 2 ? gt1.b1 + ((a & 1) ? par.b1 : par.b0) + (a >= 4 ? gt2.b1 : gt2.b0) : gt1.b0) + (a >= 4 ? esc : 0);
  return (1 << 15) + (regular ? flags : esc);
}
CTU_DEV uint32_t coded_level2(const rdoq_env &E, double *coded_cost, double coded_cost0, double *coded_cost_sig, int32_t level_double,
                              uint32_t max_abs_level, int ctx_sig, int ctx_set, int go_rice, uint32_t reg_bins, int last)
{
  const int tofs = E.t ? 21 : 0;
  const rq_pair sig = rbits2(M_SIG + (E.t ? 12 : 0) + ctx_sig), par = rbits2(M_PAR + tofs + ctx_set), gt1 = rbits2(M_GT1 + tofs + ctx_set),
                gt2 = rbits2(M_GT2 + tofs + ctx_set);
  const bool regular = reg_bins >= 4;
  const int32_t mal = (int32_t)max_abs_level;
  const int32_t a1 = mal > 1 ? mal : 1, a2 = mal > 2 ? mal - 1 : 1;
  const int32_t rate1 = rq_level_rate(a1, regular, go_rice, par, gt1, gt2), rate2 = rq_level_rate(a2, regular, go_rice, par, gt1, gt2);
  // "not significant" where the reference allows it
  const bool zero_ok = !last && mal < 3;
  const double sig0 = E.lambda * sig.b0;
  const double cur_cost_sig = last ? 0.0 : E.lambda * sig.b1;
  double cost = zero_ok ? coded_cost0 + sig0 : 1.7e+308, cost_sig = zero_ok ? sig0 : *coded_cost_sig;
  uint32_t best = 0;
  const double err1 = (double)(level_double - (a1 * (1 << E.q_bits))), err2 = (double)(level_double - (a2 * (1 << E.q_bits)));
  double cur1 = err1 * err1 * E.error_scale + E.lambda * rate1, cur2 = err2 * err2 * E.error_scale + E.lambda * rate2;
  cur1 += cur_cost_sig;
  cur2 += cur_cost_sig;
  const bool take1 = mal >= 1 && cur1 < cost;
  best = take1 ? (uint32_t)a1 : best; cost = take1 ? cur1 : cost; cost_sig = take1 ? cur_cost_sig : cost_sig;
  const bool take2 = mal >= 2 && cur2 < cost;
  best = take2 ? (uint32_t)a2 : best; cost = take2 ? cur2 : cost; cost_sig = take2 ? cur_cost_sig : cost_sig;
  *coded_cost = cost;
  *coded_cost_sig = cost_sig;
  return best;
}

// context_get_sig_ctx_idx_abs / templateAbsSum on a level array (rdo.c:1400-1438, 846-871), no MTS zero-out
template <typename LP> CTU_DEV int sig_ctx_abs(LP lv, int px, int py, int n, int color, int *diag_out, int *sum_out)
{
  const auto d = lv + px + py * n;
  int num_pos = 0, sum_abs = 0;
#define CTU_UPD(v) { const int a = iabs_((int)(v)); sum_abs += (4 + (a & 1)) < a ? (4 + (a & 1)) : a; num_pos += a ? 1 : 0; }
  if (px < n - 1) {
    CTU_UPD(d[1]);
    if (px < n - 2) CTU_UPD(d[2]);
    if (py < n - 1) CTU_UPD(d[n + 1]);
  }
  if (py < n - 1) {
    CTU_UPD(d[n]);
    if (py < n - 2) CTU_UPD(d[n << 1]);
  }
#undef CTU_UPD
  const int diag = px + py;
  int ofs = (((sum_abs + 1) >> 1) < 3 ? ((sum_abs + 1) >> 1) : 3) + (diag < 2 ? 4 : 0);
  if (color == 0) ofs += diag < 5 ? 4 : 0;
  *diag_out = diag;
  *sum_out = sum_abs - num_pos;
  return ofs;
}
template <typename LP> CTU_DEV unsigned template_abs_sum(LP lv, int base_level, int px, int py, int n)
{
  const auto p = lv + px + py * n;
  int16_t sum = 0;                        // coeff_t accumulator, as in the reference (rdo.c:849)
  if (px < n - 1) {
    sum = (int16_t)(sum + iabs_(p[1]));
    if (px < n - 2) sum = (int16_t)(sum + iabs_(p[2]));
    if (py < n - 1) sum = (int16_t)(sum + iabs_(p[n + 1]));
  }
  if (py < n - 1) {
    sum = (int16_t)(sum + iabs_(p[n]));
    if (py < n - 2) sum = (int16_t)(sum + iabs_(p[n << 1]));
  }
  int v = sum - 5 * base_level;
  v = v < 31 ? v : 31;
  return (unsigned)(v > 0 ? v : 0);
}

__device__ static const int16_t kQuantScales[6] = {26214, 23302, 20560, 18396, 16384, 14564};      // uvg_g_quant_scales[0] (scalinglist.c:91)
__device__ static const int16_t kInvQuantScales[6] = {40, 45, 51, 57, 64, 72};                     // uvg_g_inv_quant_scales[0]
__device__ static const double kPow2[16] = {1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 256.0, 512.0, 1024.0, 2048.0, 4096.0, 8192.0, 16384.0, 32768.0};

// one position of uvg_rdoq's main walk (rdo.c:1600-1716): the level that survives, its cost and the cost of its significance flag.
// regular: regular bins remain (reg_bins >= 4), go_rice is then the value carried from the position coded before; otherwise the
// position is priced as bypass-coded and its Rice parameter comes from the levels decided around it.
struct rdoq_pos { int level; double cc, cs; };
// ... of a position whose candidate is known (level_double, max_abs_level): what a round of rdoq_wave's fixed point repeats.  The five
// levels of the context template (context_get_sig_ctx_idx_abs and template_abs_sum(dst, 0, ...) read the same ones: sig_ctx_abs,
// template_abs_sum above) are fetched in one batch, each from its own address where the block has it and from the position itself
// otherwise, and the block's edges mask the VALUES: no read waits behind a branch.  (The int16_t accumulator's wrap, rdo.c:849, is
// the wrap of the whole sum.)
template <typename DP> CTU_INLINE CTU_DEV rdoq_pos rdoq_decide_at(const rdoq_env &E, DP dst, int n, int color, int pos_x, int pos_y, bool is_last, bool regular, int go_rice,
                             double c0, int32_t level_double, uint32_t max_abs_level)
{
  const bool x1 = pos_x < n - 1, x2 = pos_x < n - 2, y1 = pos_y < n - 1, y2 = pos_y < n - 2;
  const auto d = dst + pos_x + pos_y * n;
  const int v1 = d[x1 ? 1 : 0], v2 = d[x2 ? 2 : 0], v5 = d[x1 && y1 ? n + 1 : 0], v4 = d[y1 ? n : 0], v8 = d[y2 ? n << 1 : 0];
  int num_pos = 0, sum_abs = 0, sum_lev = 0;
#define CTU_UPD(v, on) { const int a = (on) ? iabs_((int)(v)) : 0; sum_abs += (4 + (a & 1)) < a ? (4 + (a & 1)) : a; num_pos += a ? 1 : 0; sum_lev += a; }
  CTU_UPD(v1, x1) CTU_UPD(v2, x2) CTU_UPD(v5, x1 && y1) CTU_UPD(v4, y1) CTU_UPD(v8, y2)
#undef CTU_UPD
  const int diag = pos_x + pos_y, tsum = sum_abs - num_pos;
  int ctx_sig = (((sum_abs + 1) >> 1) < 3 ? ((sum_abs + 1) >> 1) : 3) + (diag < 2 ? 4 : 0);
  if (color == 0) ctx_sig += diag < 5 ? 4 : 0;
  int ctx_set = ((tsum < 4 ? tsum : 4) + 1) + (!diag ? ((color == 0) ? 15 : 5) : (color == 0) ? (diag < 3 ? 10 : (diag < 10 ? 5 : 0)) : 0);
  ctx_sig = is_last ? 0 : ctx_sig;
  ctx_set = is_last ? 0 : ctx_set;
  const int t16 = (int)(int16_t)sum_lev, tcap = t16 < 31 ? t16 : 31;
  go_rice = regular ? go_rice : go_rice_par((unsigned)(tcap > 0 ? tcap : 0));          // template_abs_sum(dst, 0, ...)
  rdoq_pos r;
  r.cs = 0;        // (the reference leaves cost_sig of the last position as it was: never read before it is written, see below)
  r.level = (int)coded_level2(E, &r.cc, c0, &r.cs, level_double, max_abs_level, ctx_sig, ctx_set, go_rice, regular ? 4u : 0u, is_last);
  return r;
}
template <typename DP> CTU_INLINE CTU_DEV rdoq_pos rdoq_decide_inl(const rdoq_env &E, CTU_LDS const int16_t *coef, DP dst, int n, int l2, int color, int blkpos, bool is_last,
                             bool regular, int go_rice, double c0, int *mal_out)
{
  const int cap_half = 1 << (E.q_bits - 1);
  const int64_t prod = (int64_t)iabs_((int)coef[blkpos]) * E.q;
  const int32_t cap = 0x7fffffff - cap_half;
  const int32_t level_double = (int32_t)(prod < cap ? prod : cap);
  const uint32_t max_abs_level = (uint32_t)(level_double + cap_half) >> E.q_bits;
  const int pos_y = blkpos >> l2, pos_x = blkpos - (pos_y << l2);
  *mal_out = (int)max_abs_level;
  return rdoq_decide_at(E, dst, n, color, pos_x, pos_y, is_last, regular, go_rice, c0, level_double, max_abs_level);
}
template <typename DP> CTU_NOINLINE CTU_DEV rdoq_pos rdoq_decide(const rdoq_env &E, CTU_LDS const int16_t *coef, DP dst, int n, int l2, int color, int blkpos, bool is_last,
                             bool regular, int go_rice, double c0, int *mal_out)
{
  return rdoq_decide_inl(E, coef, dst, n, l2, color, blkpos, is_last, regular, go_rice, c0, mal_out);
}

// the last-position search's choice among the sixteen totals of a group (rdo.c:1805-1825).  The reference walks the positions in
// descending scan order and takes a candidate's total when it is strictly below the best cost so far: the lowest total wins, among
// equal totals the first met -- the highest k -- and a total equal to the incoming best_cost loses to it.  That is a reduction whose
// result does not depend on its order: the lower of two totals (rq_last_lower; a lane that is no candidate enters best_cost, which
// can only tie), then the highest candidate at the minimum, if the minimum is below best_cost at all (rq_last_pick).  Plain C++:
// rdoq_wave runs both on the lanes' registers, tests/emul_rdoq/last_pick.cpp on the host against the walk.
CTU_DEV double rq_last_lower(double a, double b) { return b < a ? b : a; }
// at_min: the candidates whose total equals the minimum m (bit k: position k of the group).  -> k + 1 of the winner, 0: best_cost stays
CTU_DEV int rq_last_pick(double m, unsigned at_min, double best_cost) { return (m < best_cost && at_min) ? 32 - __builtin_clz(at_min) : 0; }

// the level a position's fixed point STARTS from.  The fixed point does not depend on it (a decision reads only levels later in
// scan order: after round k the last k positions of a pass hold the walk's values from any start), the number of rounds does: at
// the QPs of real use RDOQ turns a large share of the candidates of 1 into 0, and a pass that starts from the candidates pays a
// round that changes them and a round that confirms.  So a candidate of 1 starts at 0 where "not significant" is the cheaper of the
// two under a neutral context -- the significance model of template sum class 1, the greater-1 model of template sum 0, regular
// bins -- which is coded_level2's comparison with the squares taken apart:
//   c0 + lambda sig.b0 <= (level_double - Q)^2 error_scale + lambda (32768 + gt1.b0) + lambda sig.b1,   Q = 1 << q_bits
//   <=>  (2 level_double - Q) Q error_scale <= lambda (32768 + gt1.b0 + sig.b1 - sig.b0).
// Every other candidate starts as itself.  Bit-exact with nothing: a wrong guess costs a round, never a level.
CTU_DEV int rq_start_level(const rdoq_env &E, int color, int pos_x, int pos_y, int32_t level_double, int mal)
{
  const int diag = pos_x + pos_y;
  const int ctx_sig = 1 + (diag < 2 ? 4 : 0) + ((color == 0 && diag < 5) ? 4 : 0);
  const int ctx_set = 1 + (!diag ? ((color == 0) ? 15 : 5) : (color == 0) ? (diag < 3 ? 10 : (diag < 10 ? 5 : 0)) : 0);
  const rq_pair sig = rbits2(M_SIG + (E.t ? 12 : 0) + ctx_sig), gt1 = rbits2(M_GT1 + (E.t ? 21 : 0) + ctx_set);
  const double q = (double)(1 << E.q_bits);
  const bool zero = ((double)level_double * 2.0 - q) * (q * E.error_scale) <= E.lambda * (double)(32768 + gt1.b0 + sig.b1 - sig.b0);
  return (mal == 1 && zero) ? 0 : mal;
}

#if !defined(__HIPCC__)
#include "ctu_rdoq_emul.h"
#else
// uvg_rdoq (rdo.c:1449-1870) by one wave: the arithmetic of the reference's walk (the host emulation's rdoq_serial, ctu_rdoq_emul.h),
// restructured around what is sequential in it.
//   * every position's quantisation candidate: all positions at once;
//   * the positions of a 4x4 group are decided together by 16 lanes, up to four groups of one diagonal of the group grid at a time
//     (a group per row of lanes: see the loop).  A decision reads only levels of positions later in scan
//     order (the context template looks right / down), so the group's decisions are the unique solution of a set of equations over
//     a DAG: the lanes start from a rate-aware guess (rq_start_level: a candidate of 1 that a neutral context would drop starts at
//     0, every other one as itself; a pass without regular bins starts from the candidates), re-decide against each other's current
//     levels and stop when a round changes nothing -- at that point every position holds exactly what the reference's walk leaves
//     there, from any start; the start only sets the number of rounds (<= 8; from the candidates mostly 2, from the guess mostly 1).
//     This needs the regular-bin budget not to run out inside the group (an upper bound from the candidates says so) or to have run
//     out for good; the one or two groups where it does run out are walked position by position by lane 0;
//   * the double-precision sums the reference forms in scan order (base cost, group statistics, the last-position search): every
//     lane forms them, in the reference's order, from the owners' registers (v_readlane at fixed lanes, sixteen unrolled steps per
//     group; predicates applied by the owners, integers from ballots) -- no memory and no branch in the chain.  The last-position
//     search keeps one chain only, base_cost, and that one runs down the owners' lanes (a wave shift a step); the sixteen totals
//     are formed once, each in its lane, and the choice among them is a reduction (rq_last_lower, rq_last_pick) -- in the intra
//     kernel; with CTU_PB that search is still every lane's uniform chain (see there).
// Result: V->rq_i[1] = whether any level survived; levels in dst.
CTU_DEV double rl64(double v, int lane)
{
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
template <int CTRL> CTU_DEV double dpp64(double v)          // both halves through one DPP control; a lane without a source reads +0.0
{
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true), hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
CTU_DEV double shfl64(double v, int from)
{
  const int lo = __shfl(__double2loint(v), from, 64), hi = __shfl(__double2hiint(v), from, 64);
  return __hiloint2double(hi, lo);
}
template <typename PX> CTU_INLINE1 CTU_DEV void rdoq_wave(lds<PX> *S, scratch *W, const int16_t *coef_, int16_t *dst_, int n, int color, int cbf_u, int qp_scaled,
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
  CTU_LDS double *const CCl = LDSP(double, V->rq_cc), *const CSl = LDSP(double, V->rq_cs);
  // blocks larger than 8x8 keep them in the workgroup's global scratch, and TWO waves can be quantising such a block at the same
  // moment (depth 1: 32x32 luma, 16x16 chroma; depth 2: 16x16 luma): each depth has its own pair of arrays
  const bool d1 = S->vsel[CTU_WAVE] == 3;
  double *const CCg = d1 ? W->cost_coeff : W->cost_coeff0, *const CSg = d1 ? W->cost_sig : W->cost_coeff0 + 512;
  double *cost_cg_sig = (double *)V->t1;         // (the transform's other buffer: dead while a block is quantised; <= 64 groups)
  const int cap_half = 1 << (E.q_bits - 1);
  const int32_t cap = 0x7fffffff - cap_half;
  RQ_T0(W)
  // ---- every position: candidate; the last candidate in scan order ----
  int my_last = -1, my_last_mal = 0;
  PAR_FOR(sp, nn) {
    const int blk = scan[sp];
    const int64_t prod = (int64_t)iabs_((int)coef[blk]) * E.q;
    const int32_t level_double = (int32_t)(prod < cap ? prod : cap);
    const int mal = (int)((uint32_t)(level_double + cap_half) >> E.q_bits);
    // (what the passes start from: rq_start_level)
    dst[blk] = (int16_t)rq_start_level(E, color, blk & (n - 1), blk >> l2, level_double, mal);
    if (mal > 0 && sp > my_last) { my_last = sp; my_last_mal = mal; }
    if (sp < 64) V->cg_flag[sp] = 0;
  }
  const int own_last = my_last;
  for (int o = 32; o >= 1; o >>= 1) { const int v = __shfl_xor(my_last, o, 64); my_last = v > my_last ? v : my_last; }
  const int last_scanpos = my_last;
  // the last candidate cannot become 0: it starts as itself (its lane stored the guess above: the same lane, the same address)
  if (own_last >= 0 && own_last == last_scanpos) dst[scan[own_last]] = (int16_t)my_last_mal;
  CTU_SYNC();
  if (last_scanpos < 0) { if (CTU_TID == 0) V->rq_i[1] = 0; CTU_SYNC(); return; }
  RQ_T(12);
  const int cg_last = last_scanpos >> 4;
  const int lane = CTU_TID, sp = lane & 15;
  const bool own = lane < 16;
  // the positions behind the last candidate only add their level-0 cost (rdo.c:1556-1583), in descending scan order
  // The sums of this function run as sixteen unrolled steps per group on v_readlane at fixed lanes, without a branch in a step: the
  // owner applies a step's predicate and hands +0.0 where the reference's walk skips.  Adding +0.0 is exact: every sum starts at
  // +0.0 and x + y is -0.0 only for two negative zeros, so no sum here is ever -0.0 (and a zero's sign decides no comparison).
  // block_uncoded_cost and base_cost receive the same values in the same order here: one sum, copied.
  double tail_cost = 0;
  {
    const auto tail_c0 = [&](int top) -> double {
      const int scanpos = top + sp;
      const int64_t prod = (int64_t)iabs_((int)coef[scan[scanpos]]) * E.q;
      const double err = (double)(int32_t)(prod < cap ? prod : cap);
      return scanpos > last_scanpos ? err * err * E.error_scale : 0.0;
    };
    double nxt = nn - 1 > last_scanpos ? tail_c0(nn - 16) : 0.0;
    for (int top = nn - 16; top + 15 > last_scanpos; top -= 16) {
      const double c0 = nxt;
      if (top - 1 > last_scanpos) nxt = tail_c0(top - 16);          // (the next group's loads: in flight during this group's steps)
#pragma unroll
      for (int k = 15; k >= 8; --k) tail_cost += rl64(c0, k);
      if (top + 7 > last_scanpos) {                                // (wave-uniform: the lower half of the last candidate's group)
#pragma unroll
        for (int k = 7; k >= 0; --k) tail_cost += rl64(c0, k);
      }
    }
  }
  double block_uncoded_cost = tail_cost, base_cost = tail_cost;
  if (CTU_TID == 0) for (int g = 0; g <= cg_last; ++g) cost_cg_sig[g] = 0;
  int reg_bins = (int)((uint32_t)(nn * 28) >> 4);
  CTU_SYNC();
  RQ_T(13);
  // A PASS decides up to four groups of one diagonal of the group grid, a group per row of 16 lanes: row r holds group top - r.
  // Group (gx, gy) reads levels of itself and of (gx+1, gy), (gx, gy+1), (gx+1, gy+1) only -- the template looks right 1, 2,
  // below 1, 2 and below-right -- and the groups of the anti-diagonal gx + gy = d hold consecutive scan indices: none of them reads
  // another one's levels, and the groups behind them have had their zero-out.  What IS sequential across groups stays so: the
  // sums (one group after the other below, in scan order) and the regular-bin budget, which is additive -- a pass is wide when
  // the budget cannot run out anywhere in it (the rows' bounds together) or has run out for good; otherwise ng = 1: one group,
  // as it was before the rows, lane 0's walk included.
  // The loop itself runs over the groups in descending scan order: a pass where the rows have none left, then the group's sums.
  const int row = lane >> 4;
  double cc = 0, cs = 0, c0 = 0;                 // the numbers of the pass's positions; of the group whose sums run in lanes 0..15
  int lev = 0, ng = 0, r = 0, counted = 0;       // (counted: the bins the groups of this pass spend leave reg_bins)
  for (int cgs = cg_last; cgs >= 0; --cgs, ++r) {
    if (r == ng) {
      const int top = cgs;
      const int ftop = scan[top * 16];
      const int dg = ((ftop & (n - 1)) >> 2) + ((ftop >> l2) >> 2);
      const int dstart = rdoq_diag_start(cgw, dg);          // the first scan index of top's diagonal
      ng = top - dstart + 1 < 4 ? top - dstart + 1 : 4;
      r = 0;
      const int regular = reg_bins >= 4;
      const int cgr = row < ng ? top - row : top;          // this row's group
      const int scanpos = cgr * 16 + sp;
      const bool mine0 = row < ng && scanpos <= last_scanpos;
      const int blk = scan[mine0 ? scanpos : cgr * 16];
      const bool is_last = scanpos == last_scanpos;
      const int64_t prod = (int64_t)iabs_((int)coef[blk]) * E.q;
      const int32_t level_double = (int32_t)(prod < cap ? prod : cap);
      const int mal1 = (int)((uint32_t)(level_double + cap_half) >> E.q_bits);
      // can the regular-bin budget run out inside this pass?  (a position spends at most min(candidate, 2 -> 3) + 1 bins)
      int fast = !regular;
      if (regular) {
        int bound = mine0 ? (mal1 < 2 ? mal1 : 3) + (is_last ? 0 : 1) : 0;
        for (int o = 8; o >= 1; o >>= 1) bound += __shfl_xor(bound, o, 64);          // (stays inside a row)
        const int b0 = __builtin_amdgcn_readlane(bound, 0);
        const int all = b0 + __builtin_amdgcn_readlane(bound, 16) + __builtin_amdgcn_readlane(bound, 32) + __builtin_amdgcn_readlane(bound, 48);
        fast = reg_bins - all >= 4;
        if (!fast && ng > 1) { ng = 1; fast = reg_bins - b0 >= 4; RQ_N(13, 1) }
      }
      RQ_N(14, 1) RQ_N(15, ng)
      const bool mine = mine0 && row < ng;
      const int mal0 = mine ? mal1 : 0;
      c0 = mine ? (double)level_double * (double)level_double * E.error_scale : 0.0;
      cc = 0; cs = 0;
      lev = 0;
      counted = fast && regular;
      if (fast) {
        int go_rice = 0;
        if (mine && regular && sp != 15 && !is_last) {
          const int nb = scan[scanpos + 1];
          go_rice = go_rice_par(template_abs_sum(coef, 4, nb & (n - 1), nb >> l2, n));      // sic: the INPUT coefficients (rdo.c:1697)
        }
        // the start: dst holds rq_start_level's guess since the candidates' loop, and lev is what dst holds (read back: forming the
        // guess again here costs the all-intra kernels 16 to 64 B of stack per lane, over the ceilings of tests/test_abi.py).  The
        // guess prices regular bins: a pass behind the budget's end starts from the candidates, which go back into dst first.
        lev = mal0;
        if (regular) lev = mine ? (int)dst[blk] : 0;
        else { if (mine) dst[blk] = (int16_t)mal0; CTU_SYNC(); }
        for (;;) {                                  // (until no lane of any row changed)
          bool changed = false;
          RQ_N(12, 1)
          if (mine) {
            // (the candidate is the pass's level_double / mal1 again; handing those in instead keeps four more registers alive across
            // the loop and costs the 10-bit kernels 16 B of stack per lane, over the ceilings of tests/test_abi.py)
            int mal;
            const rdoq_pos r = rdoq_decide_inl(E, coef, dst, n, l2, color, blk, is_last, regular != 0, go_rice, c0, &mal);
            cc = r.cc; cs = r.cs;
            changed = r.level != lev;
            lev = r.level;
          }
          CTU_SYNC();                               // every lane has read the levels it needs
          if (changed) dst[blk] = (int16_t)lev;
          const bool any = __ballot(changed) != 0;
          CTU_SYNC();
          if (!any) break;
        }
      } else {
        // the budget may run out in this group (ng == 1): position by position, exactly as the reference walks
        if (CTU_TID == 0) {
          int go_rice = 0, rb = reg_bins;
          for (int k = 15; k >= 0; --k) {
            const int spos = top * 16 + k;
            if (spos > last_scanpos) continue;
            const int b = scan[spos];
            const int64_t pr = (int64_t)iabs_((int)coef[b]) * E.q;
            const double e0 = (double)(int32_t)(pr < cap ? pr : cap);
            int mal;
            const rdoq_pos r = rdoq_decide(E, coef, dst, n, l2, color, b, spos == last_scanpos, rb >= 4, go_rice, e0 * e0 * E.error_scale, &mal);
            dst[b] = (int16_t)r.level;
            V->rq_stage[k] = r.cc; V->rq_stage[16 + k] = r.cs;
            if ((spos % 16 == 0) && spos > 0) go_rice = 0;
            else if (rb >= 4) {
              rb -= (r.level < 2 ? r.level : 3) + (spos != last_scanpos);
              go_rice = go_rice_par(template_abs_sum(coef, 4, b & (n - 1), b >> l2, n));
            }
          }
          V->rq_i[4] = rb;
        }
        CTU_SYNC();
        if (mine) { cc = V->rq_stage[sp]; cs = V->rq_stage[16 + sp]; lev = dst[blk]; }
        reg_bins = V->rq_i[4];
        CTU_SYNC();
      }
      RQ_T(14);
    } else {                                      // the pass's next group: its numbers come down a row, to lanes 0..15
      const int from = (lane + 16) & 63;
      cc = shfl64(cc, from); cs = shfl64(cs, from); c0 = shfl64(c0, from); lev = __shfl(lev, from, 64);
    }
    // the sums in scan order and the group's decision (rdo.c:1689-1772): every lane, from the registers of lanes 0..15.
    // (cc, cs, c0 and lev are zero beyond the last candidate and in rows that hold no group.)  What does not depend on the order
    // comes from ballots: the bins spent, whether and where the group has levels.
    {
      const int first = scan[cgs * 16];
      const int cg_pos_x = (first & (n - 1)) >> 2, cg_pos_y = (first >> l2) >> 2;
      const int cg_blkpos = cg_pos_y * cgw + cg_pos_x;
      const int gpos = cgs * 16 + sp;
      const bool gmine = own && gpos <= last_scanpos;
      double rd_coded = 0, rd_uncoded = 0, rd_sig = 0;
      const unsigned m_nz = (unsigned)__ballot(lev != 0) & 0xffffu, m_gt1 = (unsigned)__ballot(lev > 1) & 0xffffu, m_mine = (unsigned)__ballot(gmine);
      // (the first position of a group other than group 0 resets the Rice parameter INSTEAD of paying: rdo.c:1690-1697; a position
      // pays min(level, 2 -> 3) bins and one more unless it is the last)
      const unsigned paying = cgs ? ~1u : ~0u, not_last = cgs == cg_last ? ~(1u << (last_scanpos & 15)) : ~0u;
      const int spent = __popc(m_nz & paying) + 2 * __popc(m_gt1 & paying) + __popc(m_mine & paying & not_last);
      const int nnz_before_pos0 = __popc(m_nz & ~1u);
      int flag = cgs && m_nz;
      const bool upper = cgs < cg_last || (last_scanpos & 15) >= 8;          // (wave-uniform: the last group may end in its lower half)
      if (cgs) {                                  // the group statistics only matter where a group can be zeroed out
        const double dc = lev ? cc - cs : 0.0, du = lev ? c0 : 0.0;
        if (upper) {
#pragma unroll
          for (int k = 15; k >= 8; --k) {
            block_uncoded_cost += rl64(c0, k); base_cost += rl64(cc, k);
            rd_sig += rl64(cs, k); rd_coded += rl64(dc, k); rd_uncoded += rl64(du, k);
          }
        }
#pragma unroll
        for (int k = 7; k >= 0; --k) {
          block_uncoded_cost += rl64(c0, k); base_cost += rl64(cc, k);
          rd_sig += rl64(cs, k); rd_coded += rl64(dc, k); rd_uncoded += rl64(du, k);
        }
      } else {
        if (upper) {
#pragma unroll
          for (int k = 15; k >= 8; --k) { block_uncoded_cost += rl64(c0, k); base_cost += rl64(cc, k); }
        }
#pragma unroll
        for (int k = 7; k >= 0; --k) { block_uncoded_cost += rl64(c0, k); base_cost += rl64(cc, k); }
      }
      const double rd_sig0 = rl64(cs, 0);
      if (counted) reg_bins -= spent;
      int zeroed = 0;
      if (cgs) {
        unsigned right = 0, lower = 0;
        if (cg_pos_x + 1 < cgw) right = V->cg_flag[cg_blkpos + 1];
        if (cg_pos_y + 1 < cgw) lower = V->cg_flag[cg_blkpos + cgw];
        const int o_grp = M_SIGGRP + (E.t ? 2 : 0) + ((right || lower) ? 1 : 0);
        double cgc = 0;
        if (!flag) {
          cgc = lambda * rbits(E, o_grp, 0);
          base_cost += cgc - rd_sig;
        } else if (cgs < cg_last) {
          if (nnz_before_pos0 == 0) { base_cost -= rd_sig0; rd_sig -= rd_sig0; }
          double cost_zero_cg = base_cost;
          cgc = lambda * rbits(E, o_grp, 1);
          base_cost += cgc;
          cost_zero_cg += lambda * rbits(E, o_grp, 0);
          cost_zero_cg += rd_uncoded;
          cost_zero_cg -= rd_coded;
          cost_zero_cg -= rd_sig;
          if (cost_zero_cg < base_cost) {
            flag = 0;
            zeroed = 1;
            base_cost = cost_zero_cg;
            cgc = lambda * rbits(E, o_grp, 0);
          }
        }
        CTU_SYNC();                                 // (the neighbours' flags are read)
        if (CTU_TID == 0) cost_cg_sig[cgs] = cgc;
      } else {
        flag = 1;
      }
      if (CTU_TID == 0) V->cg_flag[cg_blkpos] = (uint8_t)flag;
      // the group's costs go to the per-position arrays the last-position search reads; a zeroed group's positions fall back to level 0
      // (cg_last == 0 -- sparse blocks: the one group's numbers stay where they are, in cc, cs, c0 and lev, for the last-position
      // search: no cost arrays)
      if (cg_last != 0 && gmine) {
        const double wc = (zeroed && lev) ? c0 : cc, ws = (zeroed && lev) ? 0.0 : cs;
        if (zeroed && lev) dst[scan[gpos]] = 0;
        if (small) { CCl[gpos] = wc; CSl[gpos] = ws; } else { CCg[gpos] = wc; CSg[gpos] = ws; }
      }
      CTU_SYNC();
    }
    RQ_T(15);
  }
  RQ_T(16);
  // ---- coded block flag and the last significant position (rdo.c:1774-1833) ----
  double best_cost;
  int best_last_idx_p1 = 0;
  {
    const int o_cbf = color == 0 ? (CTU_RQ_ROOT(V) ? 243 : M_CBF_LUMA) : color == 1 ? M_CBF_CB : M_CBF_CR + (cbf_u ? 1 : 0);
    best_cost = block_uncoded_cost + lambda * rbits(E, o_cbf, 0);
    base_cost += lambda * rbits(E, o_cbf, 1);
  }
  const int32_t *last_x_bits = S->last_bits + last_bits_off(E.t, l2, 0), *last_y_bits = S->last_bits + last_bits_off(E.t, l2, 1);
  int found_last = 0;
  for (int cgs = cg_last; cgs >= 0 && !found_last; cgs--) {
    const int first = scan[cgs * 16];
    const int cg_blkpos = ((first >> l2) >> 2) * cgw + ((first & (n - 1)) >> 2);
    base_cost -= cost_cg_sig[cgs];
    if (!V->cg_flag[cg_blkpos]) continue;
    // the owners fetch their position's numbers, then the walk runs over registers
    const int scanpos = cgs * 16 + sp;
    const bool mine = own && scanpos <= last_scanpos;
    const int blkpos = scan[mine ? scanpos : cgs * 16];
    const int klev = cg_last == 0 ? lev : (mine ? (int)dst[blkpos] : 0);
    double kcs = 0, kcc = 0, k0 = 0, klast = 0;
    if (mine) {
      kcs = cg_last == 0 ? cs : (small ? CSl[scanpos] : CTU_GLOAD(&CSg[scanpos]));
      if (klev) {
        if (cg_last == 0) { kcc = cc; k0 = c0; }
        else {
          kcc = small ? CCl[scanpos] : CTU_GLOAD(&CCg[scanpos]);
          const int64_t prod = (int64_t)iabs_((int)coef[blkpos]) * E.q;
          const double err = (double)(int32_t)(prod < cap ? prod : cap);
          k0 = err * err * E.error_scale;
        }
        const int pos_y = blkpos >> l2, pos_x = blkpos - (pos_y << l2);
        const int cx = group_idx(pos_x), cy = group_idx(pos_y);
        double cl = last_x_bits[cx] + last_y_bits[cy];
        if (cx > 3) cl += 32768 * ((cx - 2) >> 1);
        if (cy > 3) cl += 32768 * ((cy - 2) >> 1);
        klast = lambda * cl;
      }
    }
    // A position with a level is a candidate for the last one: base_cost + its position's bits - its significance flag, the first
    // of equal totals in descending order wins; then its level's cost leaves base_cost and its level-0 cost comes back, while a
    // zero's significance flag leaves it (and +0.0 comes back: k0 is zero there).  The walk ends at the first level above 1: known
    // from a ballot, the positions below it are no candidates and base_cost is not read again.
    // Only base_cost is a chain here, and every step of it is in its owner's registers: lane k holds base_cost as its own step
    // leaves it (after), formed from what lane k + 1 left (before).  A round takes the neighbour's value down one lane and redoes
    // the step; lane 15's is right from the start, lane k's after 15 - k rounds, and a round more changes nothing.  The lanes above
    // 15 hold no position (kx and k0 are +0.0 there: base_cost passes through them as it came), so the shift runs over the whole
    // wave and lane 15 reads the incoming base_cost from lane 16; what enters at lane 63 gets as far as lane 49.
    const double kx = klev ? kcc : kcs;
    const unsigned m_nz = (unsigned)__ballot(klev != 0), m_gt1 = (unsigned)__ballot(klev > 1);
    const int kstop = m_gt1 ? 31 - __clz(m_gt1) : 0;
    const unsigned cand = m_nz >> kstop << kstop;
#if defined(CTU_PB)
    // The P / B kernel keeps the walk as every lane's uniform chain on v_readlane: built with the lanes' form below, its test met
    // an illegal memory access on the device whose cause was not found (profiles/README.md, tag r17).
    if (cgs < cg_last || (last_scanpos & 15) >= 8) {              // (wave-uniform, as is kstop < 8 below)
#pragma unroll
      for (int k = 15; k >= 8; --k) {
        const double total = base_cost + rl64(klast, k) - rl64(kcs, k);
        const bool better = (cand >> k & 1u) != 0 && total < best_cost;
        best_last_idx_p1 = better ? cgs * 16 + k + 1 : best_last_idx_p1;
        best_cost = better ? total : best_cost;
        base_cost = base_cost - rl64(kx, k) + rl64(k0, k);
      }
    }
    if (kstop < 8) {
#pragma unroll
      for (int k = 7; k >= 0; --k) {
        const double total = base_cost + rl64(klast, k) - rl64(kcs, k);
        const bool better = (cand >> k & 1u) != 0 && total < best_cost;
        best_last_idx_p1 = better ? cgs * 16 + k + 1 : best_last_idx_p1;
        best_cost = better ? total : best_cost;
        base_cost = base_cost - rl64(kx, k) + rl64(k0, k);
      }
    }
#else
    double before = base_cost, after = base_cost - kx + k0;
#pragma unroll
    for (int i = 0; i < 15; ++i) {
      before = dpp64<0x130>(after);                                 // wave_shl:1
      after = before - kx + k0;
    }
    // the sixteen totals in their lanes, the choice among them: rq_last_lower / rq_last_pick above
    const double total = before + klast - kcs;
    const bool is_cand = own && (cand >> sp & 1u) != 0;
    double m = is_cand ? total : best_cost;
    m = rq_last_lower(m, dpp64<0xB1>(m));                           // quad_perm [1,0,3,2]
    m = rq_last_lower(m, dpp64<0x4E>(m));                           // quad_perm [2,3,0,1]
    m = rq_last_lower(m, dpp64<0x141>(m));                          // row_half_mirror
    m = rq_last_lower(m, dpp64<0x140>(m));                          // row_mirror: every lane of the row has the row's minimum
    const int pick = rq_last_pick(rl64(m, 0), (unsigned)__ballot(is_cand && total == m), best_cost);
    if (pick) { best_last_idx_p1 = cgs * 16 + pick; best_cost = rl64(m, 0); }
    base_cost = rl64(after, 0);                                     // (after step 0: read again only when no level above 1 was met)
#endif
    found_last = m_gt1 != 0;
  }
  if (CTU_TID == 0) V->rq_i[1] = best_last_idx_p1 > 0;
  RQ_T(17);
  PAR_FOR(scanpos, last_scanpos + 1) {
    const int b = scan[scanpos];
    if (scanpos < best_last_idx_p1) { const int level = dst[b]; dst[b] = (int16_t)((coef[b] < 0) ? -level : level); }
    else dst[b] = 0;
  }
  CTU_SYNC();
  RQ_T(18);
}
#endif

// -------------------------------------------------------------------------------------------- coefficient bit cost ------
CTU_DEV int coeff_remain_bits(uint32_t remainder, uint32_t rice, unsigned cutoff)     // uvg_cabac_write_coeff_remain, cabac.c:318-354
{
  const unsigned threshold = cutoff << rice;
  if (remainder < threshold) return (int)((remainder >> rice) + 1 + rice);
  const unsigned max_prefix = 32 - cutoff - 15;
  unsigned prefix = 0, suffix_len;
  const unsigned code_value = (remainder >> rice) - cutoff;
  if ((int32_t)code_value >= ((1 << max_prefix) - 1)) { prefix = max_prefix; suffix_len = 15; }
  else { while ((int32_t)code_value > ((2 << prefix) - 2)) prefix++; suffix_len = prefix + rice + 1; }
  return (int)(prefix + cutoff + suffix_len);
}
template <typename LP> CTU_DEV int abs_sum_tmpl(LP coeff, int px, int py, int n, int baselevel)      // uvg_abs_sum, context.c:846-877
{
  const auto d = coeff + px + py * n;
  int sum = 0;
  if (px < n - 1) {
    sum += iabs_((int)d[1]);
    if (px < n - 2) sum += iabs_((int)d[2]);
    if (py < n - 1) sum += iabs_((int)d[n + 1]);
  }
  if (py < n - 1) {
    sum += iabs_((int)d[n]);
    if (py < n - 2) sum += iabs_((int)d[n << 1]);
  }
  int v = sum - 5 * baselevel;
  v = v < 31 ? v : 31;
  return v > 0 ? v : 0;
}

// uvg_encode_coeff_nxn in count mode (encode_coding_tree-generic.c:53-323, uvg_encode_last_significant_xy :415-470) on the models m,
// which adapt bin by bin (get_coeff_cabac_cost always lets its COPY adapt; the caller decides whether to keep it); lane 0 only.
// No dependent quantisation, no sign hiding, diagonal scan, regular residual coding.  Returns 0 for an all-zero block (rdo.c:312-320).
CTU_NOINLINE CTU_DEV double coeff_bits_serial(uint32_t *m, const uint16_t *scan, const int16_t *coeff, int n, int color)
{
  const int l2 = ilog2_dev(n);
  const int t = color ? 1 : 0;
  const int cgw = n >> 2;
  uint8_t sig_cg[64];
  for (int i = 0; i < cgw * cgw; ++i) sig_cg[i] = 0;
  int scan_pos_last = -1;
  for (int i = 0; i < n * n; ++i)
    if (coeff[scan[i]]) {
      scan_pos_last = i;
      const int f = scan[i & ~15];
      sig_cg[((f >> l2) >> 2) * cgw + ((f & (n - 1)) >> 2)] = 1;
    }
  if (scan_pos_last < 0) return 0;
  const int scan_cg_last = scan_pos_last >> 4;
  double bits_out = 0;
  {
    const int pos_last = scan[scan_pos_last];
    const int last_y = pos_last >> l2, last_x = pos_last - (last_y << l2);
    const int prefix_ctx[8] = {0, 0, 0, 3, 6, 10, 15, 21};
    const int off = t ? 0 : prefix_ctx[l2];
    const int sh = t ? clampi(n >> 3, 0, 2) : ((l2 + 1) >> 2);
    const int bx = M_LASTX + 20 * t + off, by = M_LASTY + 20 * t + off;
    const int gx = group_idx(last_x), gy = group_idx(last_y), gmax = group_idx(n - 1);
    double bits = 0;
    int k = 0;
    for (; k < gx; k++) m_code(m, 1, bx + (k >> sh), 1, bits);
    if (gx < gmax) m_code(m, 1, bx + (k >> sh), 0, bits);
    k = 0;
    for (; k < gy; k++) m_code(m, 1, by + (k >> sh), 1, bits);
    if (gy < gmax) m_code(m, 1, by + (k >> sh), 0, bits);
    if (gx > 3) bits += (gx - 2) / 2;
    if (gy > 3) bits += (gy - 2) / 2;
    bits_out += bits;
  }
  double bits = 0;
  uint8_t ctx_offset[16];
  int temp_diag = -1, temp_sum = -1;
  int32_t reg_bins = (n * n * 28) >> 4;
  for (int i = scan_cg_last; i >= 0; i--) {
    const int first = scan[i * 16];
    const int cg_pos_x = (first & (n - 1)) >> 2, cg_pos_y = (first >> l2) >> 2;
    const int cg_blk = cg_pos_y * cgw + cg_pos_x;
    if (i == scan_cg_last || i == 0) {
      sig_cg[cg_blk] = 1;
    } else {
      unsigned right = 0, lower = 0;
      if (cg_pos_x + 1 < cgw) right = sig_cg[cg_blk + 1];
      if (cg_pos_y + 1 < cgw) lower = sig_cg[cg_blk + cgw];
      m_code(m, 1, M_SIGGRP + 2 * t + ((right || lower) ? 1 : 0), sig_cg[cg_blk] != 0, bits);
    }
    if (!sig_cg[cg_blk]) continue;
    const int min_sub_pos = i << 4;
    const int first_sig_pos = (i == scan_cg_last) ? scan_pos_last : (min_sub_pos + 15);
    int next_sig_pos = first_sig_pos;
    const int infer_sig_pos = (next_sig_pos != scan_pos_last) ? ((i != 0) ? min_sub_pos : -1) : next_sig_pos;
    int num_non_zero = 0;
    for (next_sig_pos = first_sig_pos; next_sig_pos >= min_sub_pos && reg_bins >= 4; next_sig_pos--) {
      const int blk = scan[next_sig_pos];
      const int py = blk >> l2, px = blk - (py << l2);
      const int sig = coeff[blk] != 0;
      if (num_non_zero || next_sig_pos != infer_sig_pos) {
        const int ctx_sig = sig_ctx_abs(coeff, px, py, n, color, &temp_diag, &temp_sum);
        m_code(m, 1, M_SIG + 12 * t + (t ? (ctx_sig < 7 ? ctx_sig : 7) : ctx_sig), sig, bits);
        reg_bins--;
      } else if (next_sig_pos != scan_pos_last) {
        (void)sig_ctx_abs(coeff, px, py, n, color, &temp_diag, &temp_sum);
      }
      if (sig) {
        uint8_t *offset = &ctx_offset[next_sig_pos - min_sub_pos];
        num_non_zero++;
        *offset = 0;
        if (temp_diag != -1) {
          *offset = (uint8_t)((temp_sum < 4 ? temp_sum : 4) + 1);
          *offset = (uint8_t)(*offset + (!temp_diag ? (color == 0 ? 15 : 5) : color == 0 ? (temp_diag < 3 ? 10 : (temp_diag < 10 ? 5 : 0)) : 0));
        }
        int rem = iabs_((int)coeff[blk]) - 1;
        const int gt1 = rem ? 1 : 0;
        m_code(m, 1, M_GT1 + 21 * t + *offset, gt1, bits);
        reg_bins--;
        if (gt1) {
          rem -= 1;
          m_code(m, 1, M_PAR + 21 * t + *offset, rem & 1, bits);
          rem >>= 1;
          reg_bins--;
          m_code(m, 1, M_GT2 + 21 * t + *offset, rem ? 1 : 0, bits);
          reg_bins--;
        }
      }
    }
    for (int sp = first_sig_pos; sp > next_sig_pos; sp--) {
      const int blk = scan[sp];
      const unsigned a = (unsigned)iabs_((int)coeff[blk]);
      if (a >= 4) {
        const int py = blk >> l2, px = blk - (py << l2);
        const int rice = go_rice_par((unsigned)abs_sum_tmpl(coeff, px, py, n, 4));
        bits += coeff_remain_bits((a - 4) >> 1, (uint32_t)rice, 5);
      }
    }
    for (int sp = next_sig_pos; sp >= min_sub_pos; sp--) {
      const int blk = scan[sp];
      const int py = blk >> l2, px = blk - (py << l2);
      const unsigned a = (unsigned)iabs_((int)coeff[blk]);
      const int rice = go_rice_par((unsigned)abs_sum_tmpl(coeff, px, py, n, 0));
      const unsigned pos0 = 1u << rice;
      const unsigned remainder = a == 0 ? pos0 : (a <= pos0 ? a - 1 : a);
      bits += coeff_remain_bits(remainder, (uint32_t)rice, 5);
      if (a) num_non_zero++;
    }
    bits += num_non_zero;
  }
  return bits_out + bits;
}


// =================================================================================================== the CTU search ======
CTU_DEV int co_off(int color) { return color == 0 ? 0 : (color == 1 ? 4096 : 5120); }
// where the depth-L candidate's samples are kept: LDS, or (slim build, depth 1) the workgroup's global scratch
template <typename PX> CTU_DEV PX *cand_px_of(lds<PX> *S, const job<PX> &J, int L, int color);
CTU_DEV int cand_px_off(int L, int color)      // L = 1..3
{
  const int base = L == 1 ? 0 : (L == 2 ? 1536 : 1920);
  const int n = 64 >> L;
  return base + (color == 0 ? 0 : n * n + (color - 1) * (n / 2) * (n / 2));
}

template <typename PX> CTU_DEV PX *cand_px_of(lds<PX> *S, const job<PX> &J, int L, int color)
{
  if (lds_cfg<PX>::slim) return L == 1 ? (PX *)J.W->cand_px32 + cand_px_off(1, color) : S->cand_px + cand_px_off(L, color) - 1536;
  return S->cand_px + cand_px_off(L, color);
}

template <typename PX> CTU_DEV int scaled_qp(const params &P, int color) { return (color == 0 ? P.qp : P.qp_c) + 6 * ((int)px_info<PX>::depth - 8); }

// predict + uvg_quantize_residual (quant-generic.c:460-612, RDOQ branch) of one transform block straight into D; its levels stay in
// lv_of(V, color) and go to the CTU's coefficient array.  (x, y) / (lx, ly): luma position, n: luma size of the area.  -> has_coeffs
// CTU_PB, flags: 1 the prediction is already in dst (a block of an inter CU), 2 no reconstruction (the early-skip test only wants
// has_coeffs), 4 RDOQ prices "no luma coefficients" with the root cbf, 8 the levels are in co already (reconstruction only)
template <typename PX> CTU_NOINLINE CTU_DEV void rdoq_wave_ool(lds<PX> *S, scratch *W, const int16_t *coef_, int16_t *dst_, int n, int color, int cbf_u, int qp_scaled,
                                                           double lambda, int bitdepth)
{
  rdoq_wave(S, W, coef_, dst_, n, color, cbf_u, qp_scaled, lambda, bitdepth);
}
template <typename PX, bool OOL = false> CTU_INLINE1 CTU_DEV int recon_tu_inl(lds<PX> *S, const job<PX> &J, int color, int x, int y, int lx, int ly, int n, int mode, int cbf_u,
                                                            PX *dst_, int dp, int16_t *co, int cp, int cu_n
#if defined(CTU_PB)
                                                            , int flags = 0
#endif
                                                            )
{
  // dst / dp: where the block is reconstructed (the decided planes, or the depth's candidate buffer); co / cp: where its levels go
  wctx *const V = wv_of(S);
  typename mg_ptr<PX, PX>::type const dst = MGP(PX, PX, dst_);
  CTU_LDS int16_t *const t0 = LDSP(int16_t, V->t0);
  typename mg_ptr<PX, int16_t>::type const lv = MGP(PX, int16_t, lv_of(V, color));
  const int c = color != 0, w = n >> c, l2 = ilog2_dev(w);
  int sps;
  CTU_GLB const PX *Sp = src_block(J, color, lx >> c, ly >> c, &sps);
  const int depth = (int)px_info<PX>::depth;
#if defined(CTU_PB)
  SERIAL V->rq_root = (flags & 4) && color == 0;
  if (!(flags & 1))
#endif
  { CTU_T0();
  build_refs(S, J.P, color, x, y, lx, ly, n, cu_n);
  predict_block(S, mode, color, w, dst_, dp);
  CTU_T1(J.W, 1); }
  const int qps = scaled_qp<PX>(J.P, color);
#if defined(CTU_PB)
  if (flags & 8) {
    // the block's levels are in co already: an earlier call quantised this very residual (same prediction, same parameters -- the
    // early-skip test of the merge candidate that became the CU, ctu_pb.h finish_inter); only the reconstruction is left to do
    int nz = 0;
    PAR_FOR(e, w * w) { const int r = e >> l2, q = e & (w - 1); const int16_t v = co[r * cp + q]; lv[e] = v; nz |= v != 0; }
#if defined(__HIPCC__)
    nz = __ballot(nz) != 0;
#endif
    SERIAL V->rq_i[1] = nz;
    CTU_SYNC();
  } else
#endif
  {
  { CTU_T0();
  PAR_FOR(e, w * w) { const int r = e >> l2, q = e & (w - 1); t0[e] = (int16_t)((int)Sp[r * sps + q] - (int)dst[r * dp + q]); }
  CTU_SYNC();
  fwd_pass(w, V->t0, V->t1, l2 - 1 + depth - 8);
  fwd_pass(w, V->t1, V->t0, l2 + 6);                     // (two buffers: the coefficients end up where the residual was)
  CTU_T1(J.W, 2); }
  CTU_T0();
  {
    // chroma blocks: state->c_lambda as uvg_quantize_lcu_residual replaces it (transform.c:1575)
    const double lambda = c ? J.P.c_lambda_tu : J.P.lambda;
    if constexpr (OOL) rdoq_wave_ool(S, J.W, V->t0, lv_of(V, color), w, color, cbf_u, qps, lambda, depth);
    else rdoq_wave(S, J.W, V->t0, lv_of(V, color), w, color, cbf_u, qps, lambda, depth);
  }
  CTU_SYNC();
  CTU_T1(J.W, 3);
  }
  const int has = V->rq_i[1];
  PAR_FOR(e, w * w) { const int r = e >> l2, q = e & (w - 1); co[r * cp + q] = lv[e]; }
#if defined(CTU_PB)
  if (has && !(flags & 2)) {
#else
  if (has) {
#endif
    const int transform_shift = 15 - depth - l2;
    const int shift = 20 - 14 - transform_shift;
    const int32_t scale = (int32_t)kInvQuantScales[qps % 6] << (qps / 6);
    const int32_t add = 1 << (shift - 1);
    PAR_FOR(e, w * w) t0[e] = (int16_t)clampi((lv[e] * scale + add) >> shift, -32768, 32767);      // uvg_dequant, quant-generic.c:618-669
    CTU_SYNC();
    inv_pass(w, V->t0, V->t1, 7);
    inv_pass(w, V->t1, V->t0, 12 - (depth - 8));
    PAR_FOR(e, w * w) {
      const int r = e >> l2, q = e & (w - 1);
      const int16_t val = (int16_t)(t0[e] + (int)dst[r * dp + q]);
      dst[r * dp + q] = (PX)clampi(val, 0, (int)px_info<PX>::maxv);
    }
  }
  CTU_SYNC();
  return has;
}
// Called per block, a noinline function saves ~45 callee-saved VGPRs to the stack and reloads them (256 B each): with RDOQ and the
// rough search, 20 MB of stack traffic per CTU.  The CU evaluation therefore has ONE call site (a loop over the colours) with the body
// inlined; the P / B walk's blocks go through this out-of-line copy (the I pictures' 64x64 candidate has its own: recon_tu64).
template <typename PX> CTU_NOINLINE CTU_DEV int recon_tu(lds<PX> *S, const job<PX> &J, int color, int x, int y, int lx, int ly, int n, int mode, int cbf_u,
                                                         PX *dst_, int dp, int16_t *co, int cp, int cu_n
#if defined(CTU_PB)
                                                         , int flags = 0
#endif
                                                         )
{
#if defined(CTU_PB)
  return recon_tu_inl(S, J, color, x, y, lx, ly, n, mode, cbf_u, dst_, dp, co, cp, cu_n, flags);
#else
  return recon_tu_inl<PX, true>(S, J, color, x, y, lx, ly, n, mode, cbf_u, dst_, dp, co, cp, cu_n);      // (RDOQ through the copy it shares with recon_tu64)
#endif
}

// uvg_pixels_calc_ssd of a w x w block of D against the source, into V->red[slot] (valid after the barrier)
template <typename PX> CTU_NOINLINE CTU_DEV void ssd_block(lds<PX> *S, const job<PX> &J, int color, int lx, int ly, int n, int slot, const PX *rec_, int rp)
{
  wctx *const V = wv_of(S);
  typename mg_ptr<PX, const PX>::type const rec = MGP(PX, const PX, rec_);
  const int c = color != 0, w = n >> c, l2 = ilog2_dev(w);
  int sps;
  CTU_GLB const PX *Sp = src_block(J, color, lx >> c, ly >> c, &sps);
  int acc = 0;
  PAR_FOR(e, w * w) { const int r = e >> l2, q = e & (w - 1); const int d = (int)Sp[r * sps + q] - (int)rec[r * rp + q]; acc += d * d; }
#if defined(__HIPCC__)
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  SERIAL V->red[slot] = acc >> (2 * ((int)px_info<PX>::depth - 8));
#else
  V->red[slot] = acc >> (2 * ((int)px_info<PX>::depth - 8));
#endif
  CTU_SYNC();
}

// uvg_write_split_flag (encode_coding_tree.c:1240-1363) with the multi-type splits off: only split_cu_flag exists; lane 0
template <typename PX> CTU_DEV void split_flag_bits(lds<PX> *S, const params &P, uint32_t *m_, int update, int x, int y, int lx, int ly, int n, int split,
                                                    double &bits)
{
  CTU_LDS uint32_t *const m = LDSP(uint32_t, m_);
  const int inside = P.pic_w >= x + n && P.pic_h >= y + n;
  if (!inside || n <= 4) return;                      // implicit split, or nothing to split: no flag
  const cu4 *left = x > 0 ? cu_at(S, lx - 1, ly) : nullptr, *above = y > 0 ? cu_at(S, lx, ly - 1) : nullptr;
  int model = 0;
  if (left && (1 << left->log2) < n) model++;
  if (above && (1 << above->log2) < n) model++;
  m_code(m, update, M_SPLIT + model, split, bits);   // split_num = 1 -> + 3 * 0
}

// uvg_encode_intra_luma_coding_unit (encode_coding_tree.c:992-1238) in count mode; lane 0
template <typename PX> CTU_NOINLINE CTU_DEV void luma_mode_bits(lds<PX> *S, uint32_t *m_, int update, int x, int y, int lx, int ly, int n, int mode, double &bits_out)
{
  CTU_LDS uint32_t *const m = LDSP(uint32_t, m_);
  const cu4 *l, *a;
  int8_t preds[6];
  mpm_neighbours(S, x, y, lx, ly, n, &l, &a);
  dir_luma_predictor(y, preds, l, a);
  double bits = 0;
  int mpm = -1;
  for (int i = 0; i < 6; ++i) if (preds[i] == mode) { mpm = i; break; }
  m_code(m, update, M_MPM, mpm != -1, bits);
  if (mpm != -1) {
    m_code(m, update, M_PLANAR + 1, mpm > 0, bits);
    if (mpm > 0) bits += 1;
    if (mpm > 1) bits += 1;
    if (mpm > 2) bits += 1;
    if (mpm > 3) bits += 1;
  } else {
    // the reference sorts the list and steps the mode down past every smaller entry (:1197-1215): mode - #{entries < mode}
    int tmp = mode;
    for (int i = 0; i < 6; ++i) tmp -= preds[i] < mode;
    bits_out += (tmp < 3) ? 5 : 6;                    // truncated binary code of 61 symbols (cabac.c:203-229)
  }
  bits_out += bits;
}
CTU_DEV void chroma_mode_bits(uint32_t *m_, int update, int chroma_mode, int luma_dir, double &bits)     // encode_chroma_intra_cu, :902-990
{
  CTU_LDS uint32_t *const m = LDSP(uint32_t, m_);
  const int derived = chroma_mode == luma_dir;
  m_code(m, update, M_CHROMA_PRED, derived ? 0 : 1, bits);
  if (!derived) bits += 2;
}

// mark_deblocking (search.c:1075-1174) for an n x n CU; sep: a 4x4 CU of an 8x8 area, chroma: it carries the area's chroma; lane 0
template <typename PX> CTU_NOINLINE CTU_DEV void mark_deblocking(lds<PX> *S, int x, int y, int lx, int ly, int n, int sep, int chroma)
{
  if (x) {
    for (int xx = lx; xx < lx + n; xx += 32)
      for (int yy = ly; yy < ly + n; yy += 4) { cu_at(S, xx, yy)->luma_edges |= 1; if (!sep) cu_at(S, xx, yy)->chroma_edges |= 1; }
  } else if (n == 64) {
    for (int yy = ly; yy < ly + n; yy += 4) { cu_at(S, 32, yy)->luma_edges |= 1; if (!sep) cu_at(S, 32, yy)->chroma_edges |= 1; }
  }
  if (y) {
    for (int yy = ly; yy < ly + n; yy += 32)
      for (int xx = lx; xx < lx + n; xx += 4) { cu_at(S, xx, yy)->luma_edges |= 2; if (!sep) cu_at(S, xx, yy)->chroma_edges |= 2; }
  } else if (n == 64) {
    for (int xx = lx; xx < lx + n; xx += 4) { cu_at(S, xx, 32)->luma_edges |= 2; if (!sep) cu_at(S, xx, 32)->chroma_edges |= 2; }
  }
  if (sep && chroma) {
    const int cx = lx & ~7, cy = ly & ~7;
    if (x & ~7) for (int yy = cy; yy < cy + 8; yy += 4) cu_at(S, cx, yy)->chroma_edges |= 1;
    if (y & ~7) for (int xx = cx; xx < cx + 8; xx += 4) cu_at(S, xx, cy)->chroma_edges |= 2;
  }
}

// regular bins a scan position spends, from its record (level in bits 0..15, "its sig flag is coded" in bit 29)
CTU_DEV int rec_spend(uint32_t rec) { const uint32_t a = rec & 0xffffu; return (int)((rec >> 29) & 1u) + (a ? 1 + (a > 1 ? 2 : 0) : 0); }

// ---- the packed sweep's pieces (coeff_bits below, coeff_bits4r in ctu_leaf4.h, the slice coder's model sweep) ----
// CTX_UPDATE (m_update) on the packed state: both halves shifted by their own window (v_pk_lshrrev_b16); no borrow or carry crosses
// the halves (a state never exceeds 0x7fe0 / 0x7ffe, what is taken off never the state).  gate: 0x7ffe7fe0 where the model codes
// the bin, else 0; add: the windows' (0x7fff >> rate) & mask where that bin is 1, else 0.  Host: the two halves one after the other.
#if defined(__HIPCC__)
typedef unsigned short cb_u16x2 __attribute__((ext_vector_type(2)));
CTU_DEV uint32_t cb_step(uint32_t st, uint32_t rpk, uint32_t gate, uint32_t add)
{
  const cb_u16x2 sh = __builtin_bit_cast(cb_u16x2, st) >> __builtin_bit_cast(cb_u16x2, rpk);
  return st - (__builtin_bit_cast(uint32_t, sh) & gate) + add;
}
#else
CTU_DEV uint32_t cb_step(uint32_t st, uint32_t rpk, uint32_t gate, uint32_t add)
{
  uint32_t s0 = st & 0xffffu, s1 = st >> 16;
  s0 = s0 - ((s0 >> (rpk & 0xffffu)) & (gate & 0xffffu)) + (add & 0xffffu);
  s1 = s1 - ((s1 >> (rpk >> 16)) & (gate >> 16)) + (add >> 16);
  return (s0 & 0xffffu) | s1 << 16;
}
#endif
// the entropy table's entry of a bin coded with the packed state: (s0 + s1) >> 8 is the model's 8-bit state (m_state)
CTU_DEV uint32_t cb_idx(uint32_t st, bool one) { return ((((st & 0xffffu) + (st >> 16)) >> 8) << 1) ^ (one ? 1u : 0u); }
CTU_DEV uint32_t cb_rpk(int rw) { return (uint32_t)(rw >> 4) | (uint32_t)(rw & 15) << 16; }
CTU_DEV uint32_t cb_addpk(int rw) { return ((0x7fffu >> (rw >> 4)) & 0x7fe0u) | ((0x7fffu >> (rw & 15)) & 0x7ffeu) << 16; }

// A 4x4 block's sweep (coeff_bits4r): plain C++, compiled for the host too (tests/emul_leaf/coeff_bits_keys.cpp replays the sweep).
// The key word of a position, a byte per role (sig, greater-1, parity, greater-2): context << 1 | bin, 0xff where the position
// codes no such bin.  a: the absolute level, ctx_sig: its significance context, ofs: its greater-1 context set (0 at the last position),
// sig_coded: its sig flag is coded (not the last position's), swept: not beyond the last position and not behind the budget's end --
// a position that is not swept has the key 0xffffffff, which no swept position has (it codes a sig flag or has a level)
CTU_DEV uint32_t lf4_key(uint32_t a, int ctx_sig, int ofs, bool sig_coded, bool swept)
{
  const uint32_t of2 = (uint32_t)ofs << 1;
  const uint32_t key = (sig_coded ? (uint32_t)ctx_sig << 1 | (a != 0 ? 1u : 0u) : 0xffu) | (a != 0 ? of2 | (a > 1 ? 1u : 0u) : 0xffu) << 8 |
                       (a > 1 ? of2 | (a & 1u) : 0xffu) << 16 | (a > 1 ? of2 | (a >= 4 ? 1u : 0u) : 0xffu) << 24;
  return swept ? key : 0xffffffffu;
}
// lane -> the model it sweeps: role 0 sig (luma 12, chroma 8 lanes), then 1 greater-1, 2 parity, 3 greater-2 (luma 16, chroma 11
// lanes each; a 4x4 luma block has the context sets 0 and 6..20), -1: none.  The model codes a bin where the byte of its role is 2 k
// or 2 k + 1
struct lf4_owner { int role, k, model; };
CTU_DEV lf4_owner lf4_lane_model(int lane, int t)
{
  const int nk0 = t ? 8 : 12, nks = t ? 11 : 16;
  lf4_owner o = {-1, 0, 0};
  if (lane < nk0) { o.role = 0; o.k = lane; }
  else if (lane < nk0 + 3 * nks) { o.role = 1 + (lane - nk0) / nks; o.k = (lane - nk0) % nks; }
  if (!t && o.role > 0 && o.k > 0) o.k += 5;
  o.model = o.role < 0 ? 0 : (o.role == 0 ? M_SIG + 12 * t : o.role == 1 ? M_GT1 + 21 * t : o.role == 2 ? M_PAR + 21 * t : M_GT2 + 21 * t) + o.k;
  return o;
}

#if defined(__HIPCC__)
#include "ctu_leaf4.h"
#endif

// Coefficient bit cost by the first wave (same bins, same model adaptation as coeff_bits_serial).  What is sequential in the
// reference's coder is only the adaptation of each context model along ITS OWN bins, and the bit count is a sum of exact
// multiples of 2^-15 (order-free).  So: every position's contexts / Rice parameters / bin values are derived by all lanes from the
// levels (they depend on nothing else) and kept as a record per position; whether the regular-bin budget can run out at all is told
// by seven ballots over the coded groups' totals, and only then lane 0 walks to the point where it does.  Every model then lives in
// a lane's registers as a packed state:
// * the sweep: sig / greater-1 / parity (chroma: / greater-2) a lane each, luma's greater-2 models a second one in the lanes 0..20.
//   The sixteen lanes that hold a group's records pack a position's four (context << 1 | bin) bytes into a key word; the sixteen
//   steps of a group are unrolled on v_readlane at fixed lanes, each a byte compare and a packed state update (cb_step), with the
//   next coded group's records in flight meanwhile;
// * the last-position prefix: a model a lane (0..7: x, 8..15: y), at most four bins each; the two group-flag contexts: the lanes 16
//   and 17, stepped through the groups from ballots.
// A bin's cost is the entropy table's entry of the state BEFORE the step (cb_idx); a state does not depend on a cost, so the lookup
// goes out in the step and is added a step later -- no step waits for LDS.  Only models that coded a bin are written back, and with
// update == 0 (the 64x64 candidate's blocks) none: nothing is copied.  The bypass-coded bits come from the records.
// All 64 lanes of wave 0 call it; the returned value is the same on every lane.  Host emulation: the serial walk.
// BITS = false: the models' adaptation only (the coder's pass: nobody reads the count; returns 0): the same steps without the Rice
// parameters, the entropy-table lookups, the bypass pass and the sums.
template <typename PX, bool BITS = true> CTU_NOINLINE CTU_DEV double coeff_bits(lds<PX> *S, uint32_t *m_, int update, const int16_t *coeff_, int n, int color)
{
  wctx *const V = wv_of(S);
#if !defined(__HIPCC__)
  uint32_t *const m = m_; const int16_t *const coeff = coeff_;
  uint32_t tmp[NMODELS];
  uint32_t *mm = m;
  if (!update) { for (int i = 0; i < NMODELS; ++i) tmp[i] = m[i]; mm = tmp; }
  return coeff_bits_serial(mm, scan_of(S, ilog2_dev(n)), coeff, n, color);
#else
  const int lane = CTU_TID;
  const int l2 = ilog2_dev(n), nn = n * n, cgw = n >> 2, ncg = nn >> 4, t = color ? 1 : 0;
  const uint16_t *scan = scan_of(S, l2);
  CTU_LDS uint32_t *const m = (CTU_LDS uint32_t *)m_;
  typename mg_ptr<PX, const int16_t>::type const coeff = MGP(PX, const int16_t, coeff_);
  if (n == 4) return coeff_bits4r<PX, BITS>(S, m, update, (int)coeff[lane & 15], color);          // (ctu_leaf4.h: the block from registers)
  CTU_LDS uint32_t *recs = (CTU_LDS uint32_t *)(V->t0);       // t0 + t1: 1024 words, free while costs are counted
  CTU_LDS uint8_t *cgf = (CTU_LDS uint8_t *)V->cg_flag;                                   // per group (raster): has a level
  CTU_LDS int32_t *gtot = (CTU_LDS int32_t *)(V->rq_stage);   // per group (scan order): regular bins it would spend, bit 30: a level among k = 1..15
  RQ_T0(S->prof_w)
  // ---- last significant position, group flags ----
  int my_last = -1;
  for (int sp = lane; sp < nn; sp += 64) if (coeff[scan[sp]]) my_last = sp;
  for (int o = 32; o >= 1; o >>= 1) { const int v = __shfl_xor(my_last, o, 64); my_last = v > my_last ? v : my_last; }
  const int last = my_last;
  if (last < 0) return 0.0;
  const int cg_last = last >> 4;
  for (int g = lane; g < ncg; g += 64) {
    int any0 = coeff[scan[g * 16]] != 0, anyr = 0;
    for (int k = 1; k < 16; ++k) anyr |= coeff[scan[g * 16 + k]] != 0;
    const int f = scan[g * 16];
    cgf[((f >> l2) >> 2) * cgw + ((f & (n - 1)) >> 2)] = (uint8_t)(any0 | anyr);
    gtot[g] = anyr << 30;
  }
  CTU_SYNC();
  RQ_T(28);
  // ---- per position: level, contexts, Rice parameters, whether its sig flag is coded, the regular bins it would spend ----
  for (int sp = lane; sp <= last; sp += 64) {
    const int blk = scan[sp], py = blk >> l2, px = blk - (py << l2), g = sp >> 4;
    const int a = iabs_((int)coeff[blk]);
    int diag, tsum;
    int ctx_sig = sig_ctx_abs(coeff, px, py, n, color, &diag, &tsum);
    if (t && ctx_sig > 7) ctx_sig = 7;
    int ofs = 0;
    if (sp != last) ofs = ((tsum < 4 ? tsum : 4) + 1) + (!diag ? (color == 0 ? 15 : 5) : color == 0 ? (diag < 3 ? 10 : (diag < 10 ? 5 : 0)) : 0);
    int r4 = 0, r0 = 0;
    if constexpr (BITS) { r4 = go_rice_par((unsigned)abs_sum_tmpl(coeff, px, py, n, 4)); r0 = go_rice_par((unsigned)abs_sum_tmpl(coeff, px, py, n, 0)); }
    const int inferred = (sp & 15) == 0 && g != 0 && g != cg_last && !((gtot[g] >> 30) & 1);
    const int sig_coded = sp != last && !inferred;
    const int spend = sig_coded + (a ? 1 + (a > 1 ? 2 : 0) : 0);
    recs[sp] = (uint32_t)(a > 0xffff ? 0xffff : a) | (uint32_t)ctx_sig << 16 | (uint32_t)ofs << 20 | (uint32_t)r4 << 25 | (uint32_t)r0 << 27 |
               (uint32_t)sig_coded << 29;
  }
  CTU_SYNC();
  for (int g = lane; g <= cg_last; g += 64) {
    int tot = 0;
    for (int k = 0; k < 16; ++k) if (g * 16 + k <= last) tot += rec_spend(recs[g * 16 + k]);
    gtot[g] = (gtot[g] & (1 << 30)) | tot;
  }
  CTU_SYNC();
  // ---- where the regular-bin budget runs out (lane 0; whole groups while they fit) ----
  bool walk;
  {
    // every coded group passes whole while the coded groups' bins together leave 4 of the budget: then the walk below ends with -1
    int mine = 0;
    if (lane <= cg_last) { const int f = scan[lane * 16]; if (cgf[((f >> l2) >> 2) * cgw + ((f & (n - 1)) >> 2)] || lane == 0) mine = gtot[lane] & 0xffff; }
    int all = 0;
#pragma unroll
    for (int b = 0; b < 7; ++b) all += __popcll(__ballot((mine >> b) & 1)) << b;          // (16 positions of at most 4 bins: 7 bits)
    walk = ((nn * 28) >> 4) - all < 4;
  }
  if (walk) {
    if (lane == 0) {
      int rb = (nn * 28) >> 4, sw = -1;
      for (int g = cg_last; g >= 0 && sw < 0; --g) {
        const int f = scan[g * 16];
        const int sig_grp = cgf[((f >> l2) >> 2) * cgw + ((f & (n - 1)) >> 2)] || g == 0;
        if (!sig_grp) continue;
        const int tot = gtot[g] & 0xffff;
        if (rb - tot >= 4) { rb -= tot; continue; }
        for (int sp = (g == cg_last ? last : g * 16 + 15); sp >= g * 16; --sp) {
          if (rb < 4) { sw = sp; break; }
          rb -= rec_spend(recs[sp]);
        }
        if (sw < 0 && rb < 4) sw = g * 16 - 1;          // ran out exactly at the group's end: everything below is bypass-coded
      }
      V->rq_i[8] = sw;
    }
    CTU_SYNC();
  }
  const int sw = walk ? V->rq_i[8] : -1;          // scan positions <= sw are bypass-coded
  RQ_T(29);
  unsigned long long coded;           // bit g: group g (scan order) is coded
  uint32_t acc = 0;                   // BITS: the costs of the bins this lane's models code, in units of 2^-15
  int ibits = 0;                      // BITS: bypass-coded bits
  {
    // ---- the models, in lanes' registers ----
    CTU_LDS const uint32_t *const ebits = LDSP(const uint32_t, tab_ebits());
    (void)ebits;
    const int last_u = __builtin_amdgcn_readfirstlane(last), sw_u = __builtin_amdgcn_readfirstlane(sw), cgl = last_u >> 4, l15 = lane & 15;
    CTU_LDS const uint8_t *const rate = LDSP(const uint8_t, kRate);
    const uint32_t kGate = 0x7ffe7fe0u;
    // per group (lane g, scan order; ncg <= 64): coded; its flag and the context of its flag (right or lower neighbour coded)
    unsigned long long todo, flg_ctx, flg_bin;
    {
      int on = 0, ctx = 0, bin = 0;
      if (lane <= cgl) {
        const int f = scan[lane * 16], cx = (f & (n - 1)) >> 2, cy = (f >> l2) >> 2, cb = cy * cgw + cx;
        bin = cgf[cb] != 0;
        on = bin || lane == 0;
        if (cx + 1 < cgw) ctx |= cgf[cb + 1] != 0;
        if (cy + 1 < cgw) ctx |= cgf[cb + cgw] != 0;
      }
      const int gmin = (sw_u + 1) >> 4;                        // groups below it lie behind the budget's end
      coded = __ballot(on);
      todo = coded & (gmin < 64 ? ~0ull << gmin : 0ull);
      flg_ctx = __ballot(ctx);
      flg_bin = __ballot(bin);
    }
    // the sweep's models: sig / greater-1 / parity (/ greater-2: chroma) a lane each; luma: the lanes 0..20 own a greater-2 model too
    int role = -1, k = 0;
    if (t) { if (lane < 8) { role = 0; k = lane; } else if (lane < 41) { role = 1 + (lane - 8) / 11; k = (lane - 8) % 11; } }
    else { if (lane < 12) { role = 0; k = lane; } else if (lane < 33) { role = 1; k = lane - 12; } else if (lane < 54) { role = 2; k = lane - 33; } }
    const bool luma = __builtin_amdgcn_readfirstlane(t) == 0, two = luma && lane < 21;
    const int model = role < 0 ? 0 : (role == 0 ? M_SIG + 12 * t : role == 1 ? M_GT1 + 21 * t : role == 2 ? M_PAR + 21 * t : M_GT2 + 21 * t) + k;
    const int model2 = M_GT2 + 21 * t + (two ? lane : 0);
    uint32_t st = m[model], st2 = m[model2];
    const int rw = rate[model], rw2 = rate[model2];
    const uint32_t rpk = cb_rpk(rw), addpk = cb_addpk(rw), rpk2 = cb_rpk(rw2), addpk2 = cb_addpk(rw2);
    // a position's key per role, a byte each (sig, greater-1, parity, greater-2): context << 1 | bin, 0xff where it codes no such
    // bin; a lane's model codes the bin where the byte of its role is 2 k or 2 k + 1
    const uint32_t sh8 = role < 0 ? 0u : (uint32_t)role * 8u, k2 = role < 0 ? 0x1000u : (uint32_t)k << 1, l2k = two ? (uint32_t)lane << 1 : 0x1000u;
    // BITS: a bin costs ebits[] of its model's state BEFORE the step.  The lookup goes out in the step and its result is added in
    // the next step that runs (pc, gated by ph: the lane's model coded the bin), so no step waits for LDS: the state does not
    // depend on the cost, and the sum is order-free
    uint32_t pc = 0, pc2 = 0;
    bool ph = false, ph2 = false;
    {
      int g = 63 - __builtin_clzll(todo);                      // (the last position's group is coded and in front of the budget's end)
      uint32_t nxt = recs[g * 16 + l15];
      for (;;) {
        const uint32_t rec = nxt;
        const int spl = g * 16 + l15;
        todo &= ~(1ull << g);
        const bool more = todo != 0;
        if (more) { g = 63 - __builtin_clzll(todo); nxt = recs[g * 16 + l15]; }          // (the next group's records: in flight during this group's steps)
        const uint32_t a = rec & 0xffffu, cs = (rec >> 16) & 15u, of2 = ((rec >> 20) & 31u) << 1;
        uint32_t keys = ((rec >> 29) & 1u ? cs << 1 | (a != 0 ? 1u : 0u) : 0xffu) | (a != 0 ? of2 | (a > 1 ? 1u : 0u) : 0xffu) << 8 |
                        (a > 1 ? of2 | (a & 1u) : 0xffu) << 16 | (a > 1 ? of2 | (a >= 4 ? 1u : 0u) : 0xffu) << 24;
        if (spl > last_u || spl <= sw_u) keys = 0xffffffffu;
#pragma unroll
        for (int j = 15; j >= 0; --j) {
          const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)keys, j);
          if (kj == 0xffffffffu) continue;                     // (wave-uniform)
          const uint32_t d = ((kj >> sh8) & 0xffu) - k2;
          if constexpr (BITS) { acc += ph ? pc : 0u; pc = ebits[cb_idx(st, d == 1u)]; ph = d < 2u; }
          st = cb_step(st, rpk, d < 2u ? kGate : 0u, d == 1u ? addpk : 0u);
          if (luma && (kj >> 24) != 0xffu) {                   // (wave-uniform: the position codes a greater-2 bin)
            const uint32_t d2 = (kj >> 24) - l2k;
            if constexpr (BITS) { acc += ph2 ? pc2 : 0u; pc2 = ebits[cb_idx(st2, d2 == 1u)]; ph2 = d2 < 2u; }
            st2 = cb_step(st2, rpk2, d2 < 2u ? kGate : 0u, d2 == 1u ? addpk2 : 0u);
          }
        }
        if (!more) break;
      }
    }
    if constexpr (BITS) acc += (ph ? pc : 0u) + (ph2 ? pc2 : 0u);
    if (role >= 0 && update) m[model] = st;
    if (two && update) m[model2] = st2;
    RQ_T(30);
    // ---- last-position prefix (lanes 0..7: x, 8..15: y; model q of an axis sees the bins k >> sh == q: 1 below the position's
    // group index, 0 at it unless it is the largest) and the group flags (lanes 16, 17: context 0, 1) ----
    {
      const int pos_last = scan[last_u];
      const int last_y = pos_last >> l2, last_x = pos_last - (last_y << l2);
      const int off = t ? 0 : (l2 == 3 ? 3 : (l2 == 4 ? 6 : 10));          // (prefix_ctx[l2] of the counting variant; n is 8, 16 or 32 here)
      const int sh = t ? clampi(n >> 3, 0, 2) : ((l2 + 1) >> 2);
      const int gmax = group_idx(n - 1), ax = (lane >> 3) & 1, q = lane & 7, gp = group_idx(ax ? last_y : last_x);
      const int amodel = lane < 16 ? (ax ? M_LASTY : M_LASTX) + 20 * t + off + q : M_SIGGRP + 2 * t + (lane & 1);
      uint32_t ast = m[amodel];
      const int arw = rate[amodel];
      const uint32_t arpk = cb_rpk(arw), aaddpk = cb_addpk(arw);
      bool dirty = false;
      uint32_t ac[4];                                // BITS: the prefix bins' costs, the four lookups in flight together
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int kk = (q << sh) + i;
        const bool in = lane < 16 && i < (1 << sh), one = in && kk < gp, zero = in && kk == gp && gp < gmax;
        if constexpr (BITS) ac[i] = one || zero ? cb_idx(ast, one) : ~0u;
        ast = cb_step(ast, arpk, one || zero ? kGate : 0u, one ? aaddpk : 0u);
        dirty |= one || zero;
      }
      if constexpr (BITS) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { const uint32_t c = ebits[ac[i] & 511u]; acc += ac[i] != ~0u ? c : 0u; }
        if ((lane == 0 || lane == 8) && gp > 3) ibits += (gp - 2) / 2;          // the prefix's bypass bits of x and of y
      }
      unsigned long long rem = cgl >= 2 ? ((1ull << cgl) - 1) & ~1ull : 0ull;          // the groups cgl - 1 .. 1 code a flag
      const int my = lane - 16;
      uint32_t fc = 0;                               // BITS: the previous flag's cost, added a step later as in the sweep
      bool fh = false;
      while (rem) {
        const int g = 63 - __builtin_clzll(rem);
        rem &= ~(1ull << g);
        const int c = (int)((flg_ctx >> g) & 1), b = (int)((flg_bin >> g) & 1);
        const bool hit = my == c;
        if constexpr (BITS) { acc += fh ? fc : 0u; fc = ebits[cb_idx(ast, b != 0)]; fh = hit; }
        ast = cb_step(ast, arpk, hit ? kGate : 0u, hit && b ? aaddpk : 0u);
        dirty |= hit;
      }
      if constexpr (BITS) acc += fh ? fc : 0u;
      // (only a model that coded a bin: the others may be another wave's.  update == 0 -- the 64x64 candidate's blocks -- counts on the
      // registers and writes nothing back: no copy of the models is made)
      if (dirty && update) m[amodel] = ast;
    }
    if constexpr (!BITS) {
      CTU_SYNC();
      RQ_T(31);
      return 0.0;
    }
  }
  // ---- bypass-coded parts: remainders, bypass positions, signs (the level and the Rice parameters are in the position's record) ----
  for (int sp = lane; sp <= last; sp += 64) {
    if (!((coded >> (sp >> 4)) & 1)) continue;
    const uint32_t rec = recs[sp];
    const unsigned a = rec & 0xffffu;
    if (sp > sw) { if (a >= 4) ibits += coeff_remain_bits((a - 4) >> 1, (rec >> 25) & 3, 5); }
    else {
      const unsigned rice = (rec >> 27) & 3, pos0 = 1u << rice;
      ibits += coeff_remain_bits(a == 0 ? pos0 : (a <= pos0 ? a - 1 : a), rice, 5);
    }
    ibits += a != 0;
  }
  unsigned long long q15 = acc;       // sum of bit costs in units of 2^-15
  for (int o = 32; o >= 1; o >>= 1) {
    q15 += __shfl_xor(q15, o, 64);
    ibits += __shfl_xor(ibits, o, 64);
  }
  CTU_SYNC();
  RQ_T(31);
  return (double)q15 / 32768.0 + (double)ibits;
#endif
}

// the transform-tree part of the RD cost of one <= 32 block whose levels are in S->lv (cu_rd_cost_tr_split_accurate, search.c:724-986);
// red[0..2]: SSD of y, u, v.  lane 0.  update: state->search_cabac.update.
template <typename PX> CTU_NOINLINE CTU_DEV double tr_cost(lds<PX> *S, const params &P, int update, int n, int cbf, int has_chroma, int cn)
{
  wctx *const V = wv_of(S);
  // called by all lanes of the first wave; the flag bins are lane 0's, the coefficient costs the wave's
  double coeff_bits_ = 0, luma_bits = 0, chroma_bits = 0;
  const int cb_y = cbf & 1, cb_u = (cbf >> 1) & 1, cb_v = (cbf >> 2) & 1;
  SERIAL {
    CTU_LDS uint32_t *const m = LDSP(uint32_t, V->cur);
    if (has_chroma) {
      m_code(m, update, M_CBF_CB + 0, cb_u, chroma_bits);
      m_code(m, update, M_CBF_CR + cb_u, cb_v, chroma_bits);
    }
    m_code(m, update, M_CBF_LUMA + 0, cb_y, luma_bits);
  }
  CTU_SYNC();
  const unsigned luma_ssd = (unsigned)V->red[0];
  // uvg_get_coeff_cost counts on a copy of the models that is kept only when update is set (rdo.c:322-356)
  if (cb_y) coeff_bits_ += coeff_bits(S, V->cur, update, lv_of(V, 0), n, 0);
  unsigned chroma_ssd = 0;
  if (has_chroma) {
    const unsigned ssd_u = (unsigned)((unsigned)V->red[1] * P.chroma_weight_u), ssd_v = (unsigned)((unsigned)V->red[2] * P.chroma_weight_v);
    chroma_ssd = ssd_u + ssd_v;
    chroma_bits += coeff_bits(S, V->cur, update, lv_of(V, 1), cn, 1);
    chroma_bits += coeff_bits(S, V->cur, update, lv_of(V, 2), cn, 2);
  }
  const double bits = luma_bits + coeff_bits_;
  return luma_ssd * 1.0 + chroma_ssd * 1.0 + (bits + chroma_bits) * P.lambda;
}

// cur_cu->mode_type_tree: the tree's bits plus the parent's type at the CU's own depth (search.c:1387-1388)
CTU_DEV uint32_t cu_mtt(uint32_t tree_mtt, int L) { return tree_mtt | ((tree_mtt >> ((L - 1 > 0 ? L - 1 : 0) * 2)) & 3u) << (L * 2); }

// lcu_fill_cu_info (search.c:314-353) for an n x n intra CU; lane 0
template <typename PX> CTU_NOINLINE CTU_DEV void fill_cu(lds<PX> *S, int lx, int ly, int n, int mode, int mode_chroma, int log2_c, uint32_t split_tree, uint32_t mtt)
{
  const int l2 = ilog2_dev(n);
  for (int yy = ly; yy < ly + n; yy += 4)
    for (int xx = lx; xx < lx + n; xx += 4) {
      cu4 *c = cu_at(S, xx, yy);
      c->type = CU_INTRA; c->log2 = (uint8_t)l2; c->log2_c = (uint8_t)log2_c; c->mode = (int8_t)mode; c->mode_chroma = (int8_t)mode_chroma;
#if defined(CTU_PB)
      { const int u = ((yy >> 2) + 1) * 17 + (xx >> 2) + 1; S->pb.mot[u].type = CU_INTRA; S->pb.fl[u][0] = 0; S->pb.fl[u][1] = 0; }   // (skipped / merged: what the neighbours' contexts read)
#endif
      S->scr->tree[(yy >> 2) * 16 + (xx >> 2)] = (uint16_t)split_tree;
      S->scr->mtt[(yy >> 2) * 16 + (xx >> 2)] = (uint16_t)mtt;
    }
}

#if defined(CTU_PB)
template <typename PX> CTU_DEV void pb_intra_flag_bits(lds<PX> *S, const job<PX> &J, uint32_t *m_, int update, int x, int y, int lx, int ly, int n, double &bits);
#endif
// search + reconstruction + RD cost of the n x n CU at depth L as ONE coding unit (the part of search_cu before the split loop,
// search.c:1395-1774), by the calling wave.  to_cand = 0 (a CU that cannot be split): straight into the decided planes / side
// information / coefficient array, on the walk's models.  to_cand = 1 (its split is tried as well, by another wave at the same
// time): into the depth's candidate buffers, on the depth's own copy of the entry models -- nothing another wave reads is touched.
// Cost / mode / cbf go to S->lvl[L].
#if defined(__HIPCC__)
CTU_DEV int mb_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); }
CTU_DEV void mb_store(int32_t *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
#endif

template <typename PX> CTU_NOINLINE CTU_DEV void eval_cu(lds<PX> *S, const job<PX> &J, int L, int to_cand
#if defined(CTU_PB)
                                                         , int forced_mode = -1      // P / B: the rough search already ran (ctu_pb.h); >= 0: its mode
#endif
                                                         )
{
  wctx *const V = wv_of(S);
  const params &P = J.P;
  level_state &N = S->lvl[L];
  const int n = 64 >> L, x = N.x, y = N.y, lx = x & 63, ly = y & 63;
  const int sep = n == 4;                                 // a 4x4 CU: its chroma belongs to the 8x8 area, carried by the fourth one
  const int has_chroma = N.has_chroma;
  if (to_cand) {
    SERIAL V->cur = S->work[L - 1];             // (the walk put the CU's entry models there before posting the request)
  } else {
    SERIAL {
      V->cur = S->cur;
      cu4 *c = cu_at(S, lx, ly);                           // the CU's own entry is reset (search.c:1371-1388)
      c->type = CU_NOTSET; c->cbf = 0; c->luma_edges = 0; c->chroma_edges = 0; c->mode = 0; c->mode_chroma = 0; c->log2 = (uint8_t)ilog2_dev(n);
      c->log2_c = (uint8_t)(sep ? 2 : ilog2_dev(n) - 1);
#if defined(CTU_PB)
      { const int u = ((ly >> 2) + 1) * 17 + (lx >> 2) + 1; S->pb.mot[u].type = CU_NOTSET; S->pb.fl[u][0] = 0; S->pb.fl[u][1] = 0; }
#endif
    }
  }
  CTU_SYNC();
#if defined(CTU_PB)
  if (forced_mode < 0)
#endif
  { CTU_T0();
  build_refs(S, P, 0, x, y, lx, ly, n, n);
  search_intra_rough(S, J, x, y, lx, ly, n);
  CTU_T1(J.W, 0); }
#if defined(CTU_PB)
  const int mode = forced_mode < 0 ? V->u_mode : forced_mode;
#else
  const int mode = V->u_mode;
#endif
  if (!to_cand) { SERIAL fill_cu(S, lx, ly, n, mode, mode, sep ? 2 : ilog2_dev(n) - 1, N.split_tree, cu_mtt(N.mode_type_tree, L)); CTU_SYNC(); }
#if defined(__HIPCC__) && !defined(CTU_PB)
  if (n == 8 && !to_cand) leaf_load_area(S, J, lx, ly);          // (an 8x8 leaf: the walk's own wave)
#endif
  // where the three blocks are reconstructed and where their levels go
  int cn = n >> 1, cx = x, cy = y;                        // the chroma area (luma coordinates) and its block size
  if (sep) { cn = 4; cx = x & ~7; cy = y & ~7; }
  const int area = sep ? 8 : n;
  PX *ry, *ru, *rv;
  int16_t *ky, *ku, *kv;
  int rpy, rpc, kpy, kpc;
  if (to_cand) {
    ry = cand_px_of(S, J, L, 0); ru = cand_px_of(S, J, L, 1); rv = cand_px_of(S, J, L, 2);
    int16_t *const kb = J.W->cand_co;
    ky = kb + cand_px_off(L, 0); ku = kb + cand_px_off(L, 1); kv = kb + cand_px_off(L, 2);
    rpy = kpy = n; rpc = kpc = cn;
  } else {
    ry = S->Dy + (ly + 1) * PY + lx + 1;
    ru = S->Du + (((cy & 63) >> 1) + 1) * PC + ((cx & 63) >> 1) + 1; rv = S->Dv + (((cy & 63) >> 1) + 1) * PC + ((cx & 63) >> 1) + 1;
    ky = J.coeff + ly * LCU + lx;
    ku = J.coeff + 4096 + ((cy & 63) >> 1) * LCU_C + ((cx & 63) >> 1); kv = J.coeff + 5120 + ((cy & 63) >> 1) * LCU_C + ((cx & 63) >> 1);
    rpy = PY; rpc = PC; kpy = LCU; kpc = LCU_C;
  }
  int cbf = 0;
#if defined(__HIPCC__)
#pragma nounroll
#endif
  for (int color = 0; color < (has_chroma ? 3 : 1); ++color) {
    const bool c = color != 0;
#if defined(__HIPCC__) && !defined(CTU_PB)
    if (c && n == 8) {
      // the 4x4 chroma blocks of an 8x8 CU: the register-resident blocks of ctu_leaf4.h, Cb and Cr in one pass (the area's source
      // samples are in S->lf_src; the luma block's reference rows are no longer needed)
      CTU_T0();
      const lf_blocks B = leaf_recon_uv(S, J, V, mode, x, y, lx, ly, ru, rv, rpc, ku, kv, kpc);
      SERIAL { V->red[1] = B.ssd_u; V->red[2] = B.ssd_v; }
      cbf |= B.cbf;
      CTU_T1(J.W, 3);
      break;
    }
#endif
    const int has = recon_tu_inl(S, J, color, c ? cx : x, c ? cy : y, c ? cx & 63 : lx, c ? cy & 63 : ly, c ? area : n, mode, color == 2 ? (cbf >> 1) & 1 : 0,
                                 color == 0 ? ry : (color == 1 ? ru : rv), c ? rpc : rpy, color == 0 ? ky : (color == 1 ? ku : kv), c ? kpc : kpy, c ? area : n);
    cbf |= has << color;
  }
#if defined(__HIPCC__) && !defined(CTU_PB)
  if (has_chroma && n != 8)          // (an 8x8 CU's chroma blocks: their SSDs came with the blocks, above)
#else
  if (has_chroma)
#endif
  {
    { CTU_T0();
    ssd_block(S, J, 1, cx & 63, cy & 63, area, 1, ru, rpc);
    ssd_block(S, J, 2, cx & 63, cy & 63, area, 2, rv, rpc);
    CTU_T1(J.W, 4); }
  }
  { CTU_T0();
  ssd_block(S, J, 0, lx, ly, n, 0, ry, rpy);
  CTU_T1(J.W, 4); }
  CTU_T0();
  {
    double bits = 0;
    SERIAL {
      if (!to_cand) {
        cu4 *c = cu_at(S, lx, ly);
        c->cbf = (uint8_t)(cbf & 1);
        if (has_chroma) {
          if (!sep) c->cbf = (uint8_t)cbf;
          else {
            // the area's chroma flags sit at its first entry and are copied to all four (lcu_fill_chroma_cbfs), with the chroma mode and
            // chroma size of this, the last, CU (lcu_fill_chroma_cu_info, search.c:355-400)
            for (int k = 0; k < 4; ++k) {
              cu4 *q = cu_at(S, (cx & 63) + (k & 1) * 4, (cy & 63) + (k >> 1) * 4);
              q->cbf = (uint8_t)((q->cbf & 1) | (cbf & 6));
              q->mode_chroma = (int8_t)mode;
              q->log2_c = 2;
            }
          }
        }
      }
      // uvg_mock_encode_coding_unit with search_cabac.update = 1 (search.c:1700-1716)
      split_flag_bits(S, P, V->cur, 1, x, y, lx, ly, n, 0, bits);
#if defined(CTU_PB)
      pb_intra_flag_bits(S, J, V->cur, 1, x, y, lx, ly, n, bits);       // a P / B slice: skip flag 0, prediction mode "intra"
#endif
      luma_mode_bits(S, V->cur, 1, x, y, lx, ly, n, mode, bits);
      if (has_chroma) chroma_mode_bits(V->cur, 1, mode, mode, bits);
    }
    CTU_SYNC();
    const double trc = tr_cost(S, P, 1, n, cbf, has_chroma, cn);       // cu_rd_cost_tr_split_accurate (:1718)
    SERIAL {
      double cost = bits * P.lambda;
      cost += trc;
      if (!to_cand) mark_deblocking(S, x, y, lx, ly, n, sep, has_chroma);
      N.cost = cost; N.type = CU_INTRA; N.mode = mode; N.cbf = cbf;
    }
  }
  CTU_SYNC();
  CTU_T1(J.W, 5);
}

#if defined(__HIPCC__)
// eval_cu(S, J, 4, 0) for the 4x4 CU described by lvl[4] on the register-resident formulation of ctu_leaf4.h: same decisions, same
// models, same reconstruction; the walk's wave, on wv[0].
template <typename PX> CTU_NOINLINE CTU_DEV void eval_cu4(lds<PX> *S, const job<PX> &J)
{
  wctx *const V = wv_of(S);
  const params &P = J.P;
  level_state &N = S->lvl[4];
  const int x = N.x, y = N.y, lx = x & 63, ly = y & 63;
  const int has_chroma = N.has_chroma;
  SERIAL {
    V->cur = S->cur;
    cu4 *c = cu_at(S, lx, ly);                           // the CU's own entry is reset (search.c:1371-1388)
    c->type = CU_NOTSET; c->cbf = 0; c->luma_edges = 0; c->chroma_edges = 0; c->mode = 0; c->mode_chroma = 0; c->log2 = 2; c->log2_c = 2;
#if defined(CTU_PB)
    { const int u = ((ly >> 2) + 1) * 17 + (lx >> 2) + 1; S->pb.mot[u].type = CU_NOTSET; S->pb.fl[u][0] = 0; S->pb.fl[u][1] = 0; }
#endif
  }
  LF_T0();
  leaf_load_area(S, J, lx, ly);
  CTU_SYNC();
  LF_T(0);
  int mode, mpm[6];
  { CTU_T0();
  leaf_refs(S, P, V, 0, x, y, lx, ly, 4);
  LF_T(1);
  mode = leaf_rough(S, J, V, x, y, lx, ly, leaf_src(S, 0, lx, ly), mpm);
  CTU_T1(J.W, 0); }
  LF_TR();          // (the rough search and the block passes time themselves: slot 9 is what lies between the named steps)
  SERIAL {          // lcu_fill_cu_info (search.c:314-353) for the one entry of a 4x4 CU
    cu4 *c = cu_at(S, lx, ly);
    c->type = CU_INTRA; c->log2 = 2; c->log2_c = 2; c->mode = (int8_t)mode; c->mode_chroma = (int8_t)mode;
#if defined(CTU_PB)
    { const int u = ((ly >> 2) + 1) * 17 + (lx >> 2) + 1; S->pb.mot[u].type = CU_INTRA; S->pb.fl[u][0] = 0; S->pb.fl[u][1] = 0; }   // (as fill_cu: what the neighbours' contexts read)
#endif
    scratch *const W = S->scr;
    W->tree[(ly >> 2) * 16 + (lx >> 2)] = (uint16_t)N.split_tree;
    W->mtt[(ly >> 2) * 16 + (lx >> 2)] = (uint16_t)cu_mtt(N.mode_type_tree, 4);
  }
  CTU_SYNC();
  const int cx = x & ~7, cy = y & ~7, clx = cx & 63, cly = cy & 63;          // the chroma area
  PX *const ry = S->Dy + (ly + 1) * PY + lx + 1;
  PX *const ru = S->Du + ((cly >> 1) + 1) * PC + (clx >> 1) + 1, *const rv = S->Dv + ((cly >> 1) + 1) * PC + (clx >> 1) + 1;
  int16_t *const ky = J.coeff + ly * LCU + lx;
  int16_t *const ku = J.coeff + 4096 + (cly >> 1) * LCU_C + (clx >> 1), *const kv = J.coeff + 5120 + (cly >> 1) * LCU_C + (clx >> 1);
  // the first three CUs of an area: the luma block; the fourth: its luma block and the area's two chroma blocks in one pass, a row of
  // 16 lanes each (Cb's reference rows in the unused smoothed rows, Cr's in the luma rows once the luma prediction is taken)
  int ssd_y = 0, ssd_u = 0, ssd_v = 0, cbf = 0, lev_y = 0, lev_u = 0, lev_v = 0;
  LF_T(9);
  { CTU_T0();
  if (has_chroma) {
    const lf_blocks B = leaf_recon_rows<PX, true>(S, J, V, mode, x, y, lx, ly, cx, cy, clx, cly, V->ftop, V->fleft, V->top, V->left, ry, ru, rv, PY, PC, ky, ku, kv, LCU, LCU_C);
    cbf = B.cbf; ssd_y = B.ssd_y; ssd_u = B.ssd_u; ssd_v = B.ssd_v; lev_y = B.lev_y; lev_u = B.lev_u; lev_v = B.lev_v;
  } else {
    const lf_block B = leaf_recon_inl(S, J, V, 0, mode, 0, x, y, lx, ly, 4, 1, ry, PY, ky, LCU);
    cbf = B.has; ssd_y = B.ssd; lev_y = B.level;
  }
  CTU_T1(J.W, 3); }
  CTU_T0();
  LF_TR();
  // ---- the CU's side information and RD cost (search.c:1700-1774) ----
  double bits = 0;
  SERIAL {
    cu4 *c = cu_at(S, lx, ly);
    c->cbf = (uint8_t)(cbf & 1);
    // mark_deblocking (search.c:1075-1174) for a 4x4 CU: its own luma edges; the area's chroma edges with the CU that carries the chroma
    c->luma_edges = (uint8_t)((x ? 1 : 0) | (y ? 2 : 0));
    if (has_chroma) {
      // the area's chroma flags sit at its first entry and are copied to all four (lcu_fill_chroma_cbfs), with the chroma mode and
      // chroma size of this, the last, CU (lcu_fill_chroma_cu_info, search.c:355-400)
      for (int k = 0; k < 4; ++k) {
        cu4 *q = cu_at(S, clx + (k & 1) * 4, cly + (k >> 1) * 4);
        q->cbf = (uint8_t)((q->cbf & 1) | (cbf & 6));
        q->mode_chroma = (int8_t)mode;
        q->log2_c = 2;
        if ((cx & ~7) && !(k & 1)) q->chroma_edges |= 1;
        if ((cy & ~7) && !(k >> 1)) q->chroma_edges |= 2;
      }
    }
    // uvg_mock_encode_coding_unit with search_cabac.update = 1 (search.c:1700-1716); a 4x4 CU has no split flag
    lf_luma_mode_bits(V->cur, mpm, mode, bits);
    if (has_chroma) chroma_mode_bits(V->cur, 1, mode, mode, bits);
  }
  LF_T(11);
  // cu_rd_cost_tr_split_accurate (search.c:724-986): the three coded block flags, a lane each (their models are distinct) ...
  double tbits;
  {
    CTU_LDS uint32_t *const m = LDSP(uint32_t, V->cur);
    const int lane = CTU_TID;
    const int fmodel = lane == 0 ? M_CBF_LUMA : (lane == 1 ? M_CBF_CB : M_CBF_CR + ((cbf >> 1) & 1));
    const int fbin = lane == 0 ? cbf & 1 : (lane == 1 ? (cbf >> 1) & 1 : (cbf >> 2) & 1);
    int fq = 0;
    if (lane == 0 || (lane < 3 && has_chroma)) {
      const uint32_t st = m[fmodel];
      const int rw = LDSP(const uint8_t, kRate)[fmodel], r0 = rw >> 4, r1 = rw & 15;
      uint32_t s0 = st & 0xffffu, s1 = st >> 16;
      fq = (int)LDSP(const uint32_t, tab_ebits())[(((s0 + s1) >> 8) << 1) ^ (uint32_t)fbin];
      s0 -= (s0 >> r0) & 0x7fe0u;
      s1 -= (s1 >> r1) & 0x7ffeu;
      if (fbin) { s0 += (0x7fffu >> r0) & 0x7fe0u; s1 += (0x7fffu >> r1) & 0x7ffeu; }
      m[fmodel] = (s0 & 0xffffu) | (s1 << 16);
    }
    const int fsum = __builtin_amdgcn_readlane(fq, 0) + __builtin_amdgcn_readlane(fq, 1) + __builtin_amdgcn_readlane(fq, 2);
    CTU_SYNC();
    // ... and the levels' bits (every term a multiple of 2^-15: the order of the sum is immaterial)
    tbits = (double)fsum / 32768.0;
    if (cbf & 1) tbits += coeff_bits4r(S, m, 1, lev_y, 0);
    if (has_chroma) { tbits += coeff_bits4r(S, m, 1, lev_u, 1); tbits += coeff_bits4r(S, m, 1, lev_v, 2); }
  }
  LF_T(12);
  SERIAL {
    const unsigned chroma_ssd = has_chroma ? (unsigned)((unsigned)ssd_u * P.chroma_weight_u) + (unsigned)((unsigned)ssd_v * P.chroma_weight_v) : 0u;
    const double trc = (unsigned)ssd_y * 1.0 + chroma_ssd * 1.0 + tbits * P.lambda;
    double cost = bits * P.lambda;
    cost += trc;
    N.cost = cost; N.type = CU_INTRA; N.mode = mode; N.cbf = cbf;
  }
  CTU_SYNC();
  LF_T(13);
  CTU_T1(J.W, 5);
}
#endif

// the depth's unsplit candidate becomes the decision: the split lost (work_tree_copy_up in reverse)
template <typename PX> CTU_NOINLINE CTU_DEV void unpark(lds<PX> *S, const job<PX> &J, int L)
{
  const level_state &N = S->lvl[L];
  const int n = 64 >> L, lx = N.x & 63, ly = N.y & 63;
  for (int color = 0; color < 3; ++color) {
    const int c = color != 0, w = n >> c, l2 = ilog2_dev(w), pit = pitch_of(color), spit = c ? LCU_C : LCU;
    PX *D = plane(S, color) + ((ly >> c) + 1) * pit + (lx >> c) + 1;
    int16_t *co = J.coeff + co_off(color) + (ly >> c) * spit + (lx >> c);
    const int off = cand_px_off(L, color);
    if (lds_cfg<PX>::slim && L == 1) {
      const PX *const from = (const PX *)J.W->cand_px32 + off;
      PAR_FOR(e, w * w) { const int r = e >> l2, q = e & (w - 1); D[r * pit + q] = CTU_GLOAD(&from[e]); co[r * spit + q] = CTU_GLOAD(&J.W->cand_co[off + e]); }
      continue;
    }
    const PX *const from = cand_px_of(S, J, L, color);
    PAR_FOR(e, w * w) { const int r = e >> l2, q = e & (w - 1); D[r * pit + q] = from[e]; co[r * spit + q] = CTU_GLOAD(&J.W->cand_co[off + e]); }
  }
  SERIAL {
    for (int yy = ly; yy < ly + n; yy += 4)
      for (int xx = lx; xx < lx + n; xx += 4) { cu4 *c = cu_at(S, xx, yy); c->cbf = 0; c->luma_edges = 0; c->chroma_edges = 0; }
    fill_cu(S, lx, ly, n, N.mode, N.mode, ilog2_dev(n) - 1, N.split_tree, cu_mtt(N.mode_type_tree, L));
    cu_at(S, lx, ly)->cbf = (uint8_t)N.cbf;
    mark_deblocking(S, N.x, N.y, lx, ly, n, 0, 1);
  }
  CTU_SYNC();
}

CTU_NOINLINE CTU_DEV void copy_models(uint32_t *dst_, const uint32_t *src_)
{
  CTU_LDS uint32_t *const dst = LDSP(uint32_t, dst_);
  CTU_LDS const uint32_t *const src = LDSP(const uint32_t, src_);
  PAR_FOR(i, NMX) dst[i] = src[i];
  CTU_SYNC();
}

#if !defined(CTU_PB)
// ---- the 64x64 CU tried with the mode of the first 32x32 CU (combine_intra_cus, search.c:2082-2143) ------------------------------
// The reference tries it after the four 32x32 areas are decided, in place, on the CTU's entry models without adaptation.  Nothing it
// computes depends on the split's outcome but the two modes, and those are the first area's: so the candidate is POSTED when the first
// area is decided (post64) and built beside the walk -- its four luma transform blocks by depth 1's wave, its chroma blocks by depth 2's,
// each between the evaluations that wave is asked for (worker_loop) -- into the workgroup's global scratch (save_px / save_co, laid
// out like the decided planes / the coefficient array), never into D.  A block's references come from the CTU's border (D's row and
// column -1, fixed for the CTU) and from the candidate's own earlier blocks (build_refs64).  At the end of the walk finish64 waits for
// the two chains, prices the CU in the reference's order of summation and, if it wins, brings it into D (unpark64); if the split wins
// there is nothing to undo.  (Rounds 3-5 built it on the walk's wave after the split, saving and restoring the whole CTU around it:
// 4.7 M of a CTU's 25.4 M cycles, profiles/r05_ctu_intra_phases_1080p8.txt.)

// uvg_intra_build_reference for transform block i (raster order) of the candidate: what build_refs computes when the side information says
// "one 64x64 intra CU" -- the counts of uvg_count_available_edge_cus (cu.c:516-537) are those of that state, whatever the split left
// in S->cu -- with the samples inside the CTU taken from the candidate's own planes.
template <typename PX> CTU_NOINLINE CTU_DEV void build_refs64(lds<PX> *S, const job<PX> &J, int color, int i)
{
  wctx *const V = wv_of(S);
  const params &P = J.P;
  const int c = color != 0, w = 32 >> c, pw = 64 >> c;
  const int lx = (i & 1) * 32, ly = (i >> 1) * 32, x = J.x + lx, y = J.y + ly;
  const int px_x = lx >> c, px_y = ly >> c;
  const int pit = pitch_of(color);
  const PX *const Dp = plane(S, color);
  const uint16_t *const C = J.W->save_px + co_off(color);
  // a sample at (row, column) of the plane relative to the CTU's origin
  auto at_ = [&](int r, int q) -> int { return (r < 0 || q < 0) ? (int)Dp[(r + 1) * pit + q + 1] : (int)CTU_GLOAD(&C[r * pw + q]); };
  SERIAL {
    const int lcnt = x == 0 ? 0 : (lx == 0 ? (LCU - ly) / 4 : 8);
    const int tcnt = y == 0 ? 0 : ((ly == 0 || lx == 0) ? 16 : 8);
    int al = lcnt * (c ? 2 : 4);
    if (al > 2 * w) al = 2 * w;
    if (al > ((P.pic_h - y) >> c)) al = (P.pic_h - y) >> c;
    int at = tcnt * (c ? 2 : 4);
    if (at > 2 * w) at = 2 * w;
    if (at > ((P.pic_w - x) >> c)) at = (P.pic_w - x) >> c;
    if (x > 0 && y > 0 && P.wpp && px_y == 0 && at > (LCU >> c) - px_x) at = (LCU >> c) - px_x;
    V->u_avail_left = al; V->u_avail_top = at;
  }
  CTU_SYNC();
  const int al = V->u_avail_left, at = V->u_avail_top;
  const int dc = 1 << (px_info<PX>::depth - 1);
  CTU_LDS uint16_t *const r_top = LDSP(uint16_t, V->top), *const r_left = LDSP(uint16_t, V->left);
  CTU_LDS uint16_t *const r_ftop = LDSP(uint16_t, V->ftop), *const r_fleft = LDSP(uint16_t, V->fleft);
  PAR_FOR(k, V->refn - 1) {
    int lv, tv;
    if (x > 0) lv = at_(px_y + (k < al ? k : al - 1), px_x - 1);
    else lv = y > 0 ? at_(px_y - 1, px_x) : dc;
    if (y > 0) tv = at_(px_y - 1, px_x + (k < at ? k : at - 1));
    else tv = x > 0 ? at_(px_y, px_x - 1) : dc;
    r_left[k + 1] = (uint16_t)lv;
    r_top[k + 1] = (uint16_t)tv;
  }
  SERIAL {
    int corner;
    if (x > 0 && y > 0) corner = at_(px_y - 1, px_x - 1);
    else corner = x > 0 ? at_(px_y, px_x - 1) : (y > 0 ? at_(px_y - 1, px_x) : dc);
    r_left[0] = r_top[0] = (uint16_t)corner;
  }
  CTU_SYNC();
  const int flim = 2 * (64 >> c) < V->refn - 1 ? 2 * (64 >> c) : V->refn - 1;
  PAR_FOR(k, V->refn) {
    int fl, ft;
    if (k == 0) fl = ft = (r_left[1] + 2 * r_left[0] + r_top[1] + 2) >> 2;
    else {
      fl = k < flim ? (r_left[k - 1] + 2 * r_left[k] + r_left[k + 1] + 2) >> 2 : r_left[k];
      ft = k < flim ? (r_top[k - 1] + 2 * r_top[k] + r_top[k + 1] + 2) >> 2 : r_top[k];
    }
    r_fleft[k] = (uint16_t)fl;
    r_ftop[k] = (uint16_t)ft;
  }
  CTU_SYNC();
}

// predict + quantise (RDOQ) + reconstruct transform block i of the candidate, colour `color`, on the calling wave's scratch: the
// prediction is staged in the transform's second buffer and made AGAIN after the inverse transform (it is the cheap part, and the
// image has no room for another tile); samples and levels go to the scratch planes, the levels stay in lv, the SSD lands in
// V->red[color].  -> has_coeffs
template <typename PX> CTU_NOINLINE CTU_DEV int recon_tu64(lds<PX> *S, const job<PX> &J, int color, int i, int mode, int cbf_u, int16_t *lv_)
{
  wctx *const V = wv_of(S);
  scratch *const W = J.W;
  const int c = color != 0, w = 32 >> c, l2 = c ? 4 : 5, pw = 64 >> c;
  const int lx = (i & 1) * 32, ly = (i >> 1) * 32;
  CTU_LDS int16_t *const t0 = LDSP(int16_t, V->t0);
  PX *const pred_ = (PX *)V->t1;
  typename mg_ptr<PX, PX>::type const pred = MGP(PX, PX, pred_);
  typename mg_ptr<PX, int16_t>::type const lv = MGP(PX, int16_t, lv_);
  int sps;
  CTU_GLB const PX *Sp = src_block(J, color, lx >> c, ly >> c, &sps);
  const int depth = (int)px_info<PX>::depth;
  { CTU_T0();
  build_refs64(S, J, color, i);
  predict_block(S, mode, color, w, pred_, w);
  CTU_T1(J.W, 1); }
  { CTU_T0();
  PAR_FOR(e, w * w) { const int r = e >> l2, q = e & (w - 1); t0[e] = (int16_t)((int)Sp[r * sps + q] - (int)pred[e]); }
  CTU_SYNC();
  fwd_pass(w, V->t0, V->t1, l2 - 1 + depth - 8);
  fwd_pass(w, V->t1, V->t0, l2 + 6);
  CTU_T1(J.W, 2); }
  const int qps = scaled_qp<PX>(J.P, color);
  { CTU_T0();
  const double lambda = c ? J.P.c_lambda_tu : J.P.lambda;
  rdoq_wave_ool(S, W, V->t0, lv_, w, color, cbf_u, qps, lambda, depth);
  CTU_SYNC();
  CTU_T1(J.W, 3); }
  const int has = V->rq_i[1];
  uint16_t *const px64 = W->save_px + co_off(color) + (ly >> c) * pw + (lx >> c);
  int16_t *const co64 = W->save_co + co_off(color) + (ly >> c) * pw + (lx >> c);
  PAR_FOR(e, w * w) { const int r = e >> l2, q = e & (w - 1); co64[r * pw + q] = lv[e]; }
  if (has) {
    const int transform_shift = 15 - depth - l2;
    const int shift = 20 - 14 - transform_shift;
    const int32_t scale = (int32_t)kInvQuantScales[qps % 6] << (qps / 6);
    const int32_t add = 1 << (shift - 1);
    PAR_FOR(e, w * w) t0[e] = (int16_t)clampi((lv[e] * scale + add) >> shift, -32768, 32767);
    CTU_SYNC();
    inv_pass(w, V->t0, V->t1, 7);
    inv_pass(w, V->t1, V->t0, 12 - (depth - 8));
  }
  predict_block(S, mode, color, w, pred_, w);
  int acc = 0;
  PAR_FOR(e, w * w) {
    const int r = e >> l2, q = e & (w - 1);
    int v = (int)pred[e];
    if (has) v = clampi((int16_t)(t0[e] + v), 0, (int)px_info<PX>::maxv);
    px64[r * pw + q] = (uint16_t)v;
    const int d = (int)Sp[r * sps + q] - v;
    acc += d * d;
  }
#if defined(__HIPCC__)
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
#endif
  SERIAL V->red[color] = acc >> (2 * (depth - 8));
  CTU_SYNC();
  return has;
}

// luma transform block i of the candidate (depth 1's wave, its own scratch)
template <typename PX> CTU_NOINLINE CTU_DEV void luma64_step(lds<PX> *S, const job<PX> &J, int i)
{
  wctx *const V = wv_of(S);
  const int cy = recon_tu64(S, J, 0, i, S->m64[0], 0, V->lv0);
  double by = 0;
  SERIAL m_code(LDSP(uint32_t, S->coder), 0, M_CBF_LUMA + 0, cy, by);
  CTU_SYNC();
  if (cy) by += coeff_bits(S, S->coder, 0, V->lv0, 32, 0);
  SERIAL { S->h64[i].cy = cy; S->h64[i].ssd_y = V->red[0]; S->h64[i].bits_y = by; }
  CTU_SYNC();
}
// a chroma block of transform unit i (depth 2's wave: a 16x16 block is that depth's luma size, so the levels of Cb and Cr take turns
// in its luma level array)
template <typename PX> CTU_NOINLINE CTU_DEV void chroma64_step(lds<PX> *S, const job<PX> &J, int i, int color)
{
  wctx *const V = wv_of(S);
  const int cu = color == 2 ? S->h64[i].cu : 0;
  const int has = recon_tu64(S, J, color, i, S->m64[1], cu, V->lv0);
  const double cb = coeff_bits(S, S->coder, 0, V->lv0, 16, color);
  SERIAL {
    if (color == 1) { S->h64[i].cu = has; S->h64[i].ssd_u = V->red[1]; S->h64[i].bits = cb; }
    else {
      double fb = 0;
      m_code(LDSP(uint32_t, S->coder), 0, M_CBF_CB + 0, cu, fb);
      m_code(LDSP(uint32_t, S->coder), 0, M_CBF_CR + cu, has, fb);
      double both = S->h64[i].bits;
      both += cb;
      S->h64[i].cv = has; S->h64[i].ssd_v = V->red[2]; S->h64[i].bits = fb + both;
    }
  }
  CTU_SYNC();
}

// the walk: the first 32x32 area is decided and is one intra CU -- ask for the candidate
template <typename PX> CTU_DEV void post64(lds<PX> *S, const job<PX> &J)
{
  SERIAL { S->m64[0] = cu_at(S, 0, 0)->mode; S->m64[1] = cu_at(S, 0, 0)->mode_chroma; }
  CTU_SYNC();
#if defined(__HIPCC__)
  SERIAL mb_store(&S->req64, 1);
#else
  S->req64 = 1;
  emul_on_wave(3, [&] { for (int i = 0; i < 4; ++i) luma64_step(S, J, i); });
  emul_on_wave(2, [&] { for (int i = 0; i < 4; ++i) { chroma64_step(S, J, i, 1); chroma64_step(S, J, i, 2); } });
  S->done64[0] = S->done64[1] = 1;
#endif
}

// the candidate won: into the decided planes, the coefficient array and the side information (the walk's wave)
template <typename PX> CTU_NOINLINE CTU_DEV void unpark64(lds<PX> *S, const job<PX> &J)
{
  scratch *W = J.W;
  level_state &N = S->lvl[0];
  for (int color = 0; color < 3; ++color) {
    const int w = color ? 32 : 64, l2 = color ? 5 : 6, pit = pitch_of(color);
    PX *D = plane(S, color) + pit + 1;
    PAR_FOR(e, w * w) { D[(e >> l2) * pit + (e & (w - 1))] = (PX)CTU_GLOAD(&W->save_px[co_off(color) + e]); J.coeff[co_off(color) + e] = CTU_GLOAD(&W->save_co[co_off(color) + e]); }
  }
  SERIAL {
    for (int e = 0; e < 256; ++e) { cu4 *c = cu_at(S, (e & 15) * 4, (e >> 4) * 4); c->cbf = 0; c->luma_edges = 0; c->chroma_edges = 0; }
    fill_cu(S, 0, 0, 64, S->m64[0], S->m64[1], 5, N.split_tree, cu_mtt(N.mode_type_tree, 0));
    for (int i = 0; i < 4; ++i) cu_at(S, (i & 1) * 32, (i >> 1) * 32)->cbf = (uint8_t)(S->h64[i].cy | S->h64[i].cu << 1 | S->h64[i].cv << 2);
    mark_deblocking(S, N.x, N.y, 0, 0, 64, 0, 1);
    N.type = CU_INTRA;
  }
  CTU_SYNC();
}

// the walk, after the four 32x32 areas: the candidate's cost into lvl[0].cost; -> the split wins
template <typename PX> CTU_DEV bool finish64(lds<PX> *S, const job<PX> &J)
{
  const params &P = J.P;
  level_state &N = S->lvl[0];
#if defined(__HIPCC__)
  { CTU_T0();
  while (mb_load(&S->done64[0]) == 0 || mb_load(&S->done64[1]) == 0) __builtin_amdgcn_s_sleep(2);
  CTU_T1(J.W, 12); }        // (profile slots 12 / 13 of the walk's wave: the wait for the two chains, unpark64)
#endif
  CTU_SYNC();
  SERIAL {
    // the models are the CTU's entry models (the coder's, untouched until its pass after the search) and do not adapt
    // (search_cabac.update is 0 on this path): bits only
    const int mode = S->m64[0], mode_chroma = S->m64[1];
    double bits = 0;
    split_flag_bits(S, P, S->coder, 0, N.x, N.y, 0, 0, 64, 0, bits);
    double mode_bits = 0;
    {   // calc_mode_bits (search.c:988-1003): the luma mode on a copy of the models, the chroma mode without adaptation
      for (int k = 0; k < NMODELS; ++k) S->work[2][k] = S->coder[k];          // (depth 3's entry models: nobody's after the walk)
      luma_mode_bits(S, S->work[2], 0, N.x, N.y, 0, 0, 64, mode, mode_bits);
      if (mode_chroma == mode) mode_bits += m_fbits(S->coder, M_CHROMA_PRED, 0);
      else mode_bits += 2.0 + m_fbits(S->coder, M_CHROMA_PRED, 1);
    }
    mode_bits += bits;
    const double d0 = mode_bits * P.lambda;
    double d1 = 0;
    for (int i = 0; i < 4; ++i) {
      // cu_rd_cost_tr_split_accurate of the unit (tr_cost): SSDs + (luma bits + chroma bits) * lambda
      const unsigned chroma_ssd = (unsigned)((unsigned)S->h64[i].ssd_u * P.chroma_weight_u) + (unsigned)((unsigned)S->h64[i].ssd_v * P.chroma_weight_v);
      d1 += (unsigned)S->h64[i].ssd_y * 1.0 + chroma_ssd * 1.0 + (S->h64[i].bits_y + S->h64[i].bits) * P.lambda;
    }
    double c2 = 0;
    c2 += d0;
    c2 += d1 + 0 * P.lambda;          // the sum of the four blocks + luma_bits (0) * lambda (search.c:779)
    N.cost = c2;
  }
  CTU_SYNC();
  const bool split_wins = N.split_cost < N.cost;
  CTU_SYNC();
  // post_search_cabac = the unadapted entry models; search_cabac = temp_cabac, the models after the split (:2140-2141): S->cur as it is
  if (split_wins) { SERIAL N.cost = N.split_cost; CTU_SYNC(); }
  else { CTU_T0(); unpark64(S, J); CTU_T1(J.W, 13); }
  return split_wins;
}
#endif

#define V_flag(S) (wv_of(S)->u_flag)

// ---- the depth pipeline ---------------------------------------------------------------------------------------------------
// A CU whose split is tried as well is evaluated unsplit by the wave of ITS depth while the walk goes on into its children: the
// evaluation needs only what is decided before the CU (samples, side information, the entry models) and writes only its own
// candidate buffers.  The reference evaluates the CU first and uses its cost to cut the children short (search.c:1952-1956,
// 2002-2005); evaluating children it would have skipped changes nothing: every cut decides "not split", and so does the final
// comparison whenever a cut would have applied (costs only grow child by child; the pruning test is re-applied when the cost is known).

// the pruning test (search.c:1952-1956): with the CU's own cost N.cost known, the reference would not try its split
CTU_INLINE CTU_DEV bool split_pruned(const params &P, const level_state &N)
{
  const double factor = P.qp > 30 ? 1.1 : 1.075;
  return N.split_bits * P.lambda + N.cost / factor > N.cost;
}

// ask the wave of depth L (1..3) to evaluate the CU described by lvl[L] / pre[L] (walk's wave, lane 0 has written both)
template <typename PX> CTU_DEV void post_eval(lds<PX> *S, const job<PX> &J, int L)
{
#if defined(__HIPCC__)
  CTU_SYNC();
  SERIAL mb_store(&S->req[L], S->req[L] + 1);
#else
  emul_on_wave(4 - L, [&] { eval_cu(S, J, L, 1); });
  S->done[L] = ++S->req[L];
#endif
}
template <typename PX> CTU_DEV bool eval_ready(lds<PX> *S, int L)
{
#if defined(__HIPCC__)
  return __builtin_amdgcn_readfirstlane(mb_load(&S->done[L]) == S->req[L]) != 0;      // lane 0's view, for every lane
#else
  return !g_emul_lazy;
#endif
}
template <typename PX> CTU_DEV void wait_eval(lds<PX> *S, int L)
{
#if defined(__HIPCC__)
  while (mb_load(&S->done[L]) != S->req[L]) __builtin_amdgcn_s_sleep(2);
  CTU_SYNC();
#endif
}
enum { CODER_FLAGS = 1, CODER_LUMA = 2, CODER_CHROMA = 4, CODER_ALL = 7 };      // the coder's pass by model (below, at coder_pass)
template <typename PX> CTU_DEV void coder_pass(lds<PX> *S, const job<PX> &J, int parts);
#if defined(__HIPCC__)
// waves 1..3: evaluate depth 4 - wave whenever asked, until told to stop (req < 0)
template <typename PX> CTU_DEV void worker_loop(lds<PX> *S, const job<PX> &J)
{
  const int L = 4 - CTU_WAVE;
  int seen = 0;
  // the 64x64 candidate (post64): depth 1's wave owes it four luma blocks, depth 2's eight chroma blocks, one at a time whenever the
  // wave has no evaluation to do
  const int steps64 = L == 1 ? 4 : (L == 2 ? 8 : 0);
  int n64 = 0;
  bool coded = false;
  for (;;) {
    int r;
    bool step = false;
    for (;;) {
      r = mb_load(&S->req[L]);
      if (r != seen) break;
      if (n64 < steps64 && mb_load(&S->req64)) { step = true; break; }
      if (L >= 2 && !coded && mb_load(&S->creq)) {
        // the search is over: this wave's part of the coder's pass (depth 3: the flags, depth 2: the chroma coefficients)
        { CTU_T0();
        coder_pass(S, J, L == 3 ? CODER_FLAGS : CODER_CHROMA);
        CTU_T1(J.W, 8); }
        CTU_SYNC();
        SERIAL mb_store(&S->cdone[3 - L], 1);
        coded = true;
        continue;
      }
      if (L == 3) __builtin_amdgcn_s_sleep(1); else __builtin_amdgcn_s_sleep(4);
    }
    if (r != seen) {
      if (r < 0) break;
      seen = r;
      eval_cu(S, J, L, 1);
      CTU_SYNC();
      SERIAL mb_store(&S->done[L], r);
    } else if (step) {
      if (L == 1) luma64_step(S, J, n64); else chroma64_step(S, J, n64 >> 1, 1 + (n64 & 1));
      if (++n64 == steps64) { CTU_SYNC(); SERIAL mb_store(&S->done64[L - 1], 1); }
    }
  }
}
#endif

// search_cu (search.c:1299-2221) as a depth-first loop over the quad tree of one CTU, run by the first wave
template <typename PX> CTU_DEV void search_ctu(lds<PX> *S, const job<PX> &J)
{
  const params &P = J.P;
  SERIAL {
    level_state &R = S->lvl[0];
    R.x = J.x; R.y = J.y; R.split_tree = 0; R.mode_type_tree = 0; R.has_chroma = 1; R.child = 0;
  }
  CTU_SYNC();
  int L = 0;
  int entering = 1;
  double ret = 0;            // the cost a finished node hands to its parent (uniform: read from LDS after a fence)
  for (;;) {
    level_state &N = S->lvl[L];
    const int n = 64 >> L;
    if (entering) {
      const int x = N.x, y = N.y;
      CTU_SYNC();            // every lane holds its copy before lane 0 may reach the parent's bookkeeping and rewrite this entry
      if (x >= P.pic_w || y >= P.pic_h) { ret = 0; entering = 0; if (L == 0) break; --L; continue; }     // outside: nothing to code (search.c:1350)
      const int inside = x + n <= P.pic_w && y + n <= P.pic_h;
      // check_can_use_intra (search.c:1257-1287)
      const int min_w = 64 >> P.depth_max;
      const int can_intra = inside && ((L >= P.depth_min && L <= P.depth_max) || (x & ~(min_w - 1)) + min_w > P.pic_w || (y & ~(min_w - 1)) + min_w > P.pic_h);
      const int can_split = (!can_intra || L < P.depth_max) && n > 4;
      if (!can_split) {
        // a leaf: evaluated here, straight into the decided state
        if (can_intra) {
          CTU_T0();
          SERIAL S->vsel[CTU_WAVE] = 4 - L;          // the scratch sized for this depth (its own wave has nothing to do for a leaf)
          CTU_SYNC();
#if defined(__HIPCC__)
          if (L == 4) eval_cu4(S, J); else
#endif
          eval_cu(S, J, L, 0);
          SERIAL S->vsel[CTU_WAVE] = 0;
          CTU_SYNC();
          CTU_T1(J.W, 19 + L);
        }
        else { SERIAL { N.cost = CTU_MAX_DOUBLE; N.type = CU_NOTSET; } CTU_SYNC(); }
        ret = N.cost; entering = 0; if (L == 0) break; --L; continue;
      }
      SERIAL { N.type = can_intra ? CU_INTRA : CU_NOTSET; N.cost = CTU_MAX_DOUBLE; N.pending = can_intra; }
#if defined(__HIPCC__)
      if (n == 8) leaf_load_area(S, J, x & 63, y & 63);          // (the 8x8 CU's chroma blocks and the four 4x4 CUs below it read the source from there)
#endif
      if (can_intra) { copy_models(S->work[L - 1], S->cur); post_eval(S, J, L); }          // its own wave evaluates the CU unsplit from these models ...
      // ... while the walk tries the split: its flag first (models from the CU's entry: cur still holds them)
      SERIAL {
        double split_bits = 0;
        split_flag_bits(S, P, S->cur, 1, x, y, x & 63, y & 63, n, 1, split_bits);
        N.split_bits = split_bits;
        N.split_cost = split_bits * P.lambda;
        N.child = 0;
        level_state &C = S->lvl[L + 1];
        const int cond_infer = (N.mode_type_tree >> ((L - 1 > 0 ? L - 1 : 0) * 2) & 3) == 0 && n == 8;      // uvg_derive_mode_type_cond: MODE_TYPE_INFER
        const uint32_t mode_type = cond_infer ? 2u : (N.mode_type_tree >> ((L - 1 > 0 ? L - 1 : 0) * 2) & 3);
        C.split_tree = N.split_tree | 1u << (L * 3);
        C.mode_type_tree = N.mode_type_tree | mode_type << (L * 2);
        C.x = N.x; C.y = N.y; C.has_chroma = (n >> 1) == 4 ? 0 : 1;
      }
      CTU_SYNC();
      ++L;
      continue;
    }
    // a child of N came back with `ret`
    const bool known = !N.pending || eval_ready(S, L);      // is the CU's own cost there yet?  (only to stop early; never changes the outcome)
    if (known && N.pending) WAIT_EVAL(S, L);
    SERIAL {
      N.split_cost += ret;
      const int k = N.child;
      const int last = k == 3;
      V_flag(S) = (known && N.split_cost > N.cost) || last;       // (best_split_cost is still MAX_DOUBLE: one split type)
      N.child = k + 1;
      if (!V_flag(S)) {
        level_state &C = S->lvl[L + 1];
        const int h = n >> 1, k1 = k + 1;
        C.x = N.x + (k1 & 1) * h; C.y = N.y + (k1 >> 1) * h;
        C.has_chroma = h == 4 ? (k1 == 3) : 1;
      }
    }
    CTU_SYNC();
#if !defined(CTU_PB)
    // the first 32x32 area is decided: if it is one intra CU the 64x64 candidate will be tried with its modes (combine_intra_cus) -- ask
    // for it now, the depth waves build it beside the walk (post64).  Only when no leaf can borrow those waves' scratch (vsel).
    if (L == 0 && N.child == 1 && N.type == CU_NOTSET && P.combine_intra_cus && P.depth_max >= 3 && N.x + 64 <= P.pic_w && N.y + 64 <= P.pic_h &&
        cu_at(S, 0, 0)->type == CU_INTRA && cu_at(S, 0, 0)->log2 == 5) post64(S, J);
#endif
    if (!V_flag(S)) { ++L; entering = 1; continue; }
    // the split is complete (or was cut short): the CU's own cost is needed now
    if (N.pending) WAIT_EVAL(S, L);
    // The comparison is taken by every lane BEFORE lane 0 may overwrite a cost.
    const bool pruned = N.type != CU_NOTSET && split_pruned(P, N);      // the reference would not have tried the split
    const bool split_wins = !pruned && N.split_cost < N.cost;
    const int ntype = N.type;
    CTU_SYNC();
#if !defined(CTU_PB)
    if (L == 0 && ntype == CU_NOTSET && P.combine_intra_cus && N.x + 64 <= P.pic_w && N.y + 64 <= P.pic_h &&
        cu_at(S, 0, 0)->type == CU_INTRA && cu_at(S, 0, 0)->log2 == 5) {
      CTU_T0();
      if (!S->req64) post64(S, J);                       // (leaves above depth 3 borrow the depth waves' scratch: nothing was posted beside them)
      (void)finish64(S, J);
      CTU_T1(J.W, 7);
      ret = N.cost;
      break;
    }
#endif
    if (split_wins) {
      SERIAL N.cost = N.split_cost;
      CTU_SYNC();
    } else {
      CTU_T0();
      if (L > 0) copy_models(S->cur, S->work[L - 1]);      // post_search_cabac: the models as the unsplit CU leaves them
      if (ntype != CU_NOTSET) unpark(S, J, L);
      CTU_T1(J.W, 6);
    }
    ret = N.cost;
    if (L == 0) break;
    --L;
  }
}

// ====================================================================== the real coder's model adaptation + CTU in / out ======
CTU_DEV int z_to_x(int z) { return (z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4) | ((z >> 3) & 8); }
// A context model is a state machine of its own: what it becomes depends on the bins coded with IT, in coding order, and on nothing
// else; which model a bin uses depends on the syntax (levels, modes, flags, neighbours), never on another model's state.  So the pass
// over the decided CTU splits by MODEL into three passes that each walk the CUs in coding order and touch disjoint entries of
// S->coder: the flags (split, prediction modes, the three cbf), the luma coefficients (significance / greater-than / parity /
// last position / group flags of colour type 0) and the chroma coefficients (the same of colour type 1, Cb before Cr).  Three waves
// run them side by side (run_ctu); the host emulation runs them one after the other.  (enum CODER_*: above worker_loop)

#if defined(__HIPCC__)
// the real coder's walk over an 8x8 area of four 4x4 CUs (the shape most of a detailed CTU consists of): the area's 64 + 32 levels are
// fetched once, a lane each; every block's bins go through coeff_bits4r from registers.  Same bins in the same order as coder_pass.
template <typename PX> CTU_DEV void coder_area4(lds<PX> *S, const job<PX> &J, int lx, int ly, int parts)
{
  const params &P = J.P;
  const int lane = CTU_TID, r = lane & 15;
  int lev_all = 0, clev = 0;
  {
    const int k = lane >> 4;
    if (parts & CODER_LUMA) lev_all = CTU_GLOAD(&J.coeff[(ly + (k >> 1) * 4 + (r >> 2)) * LCU + lx + (k & 1) * 4 + (r & 3)]);
    if ((parts & CODER_CHROMA) && lane < 32) clev = CTU_GLOAD(&J.coeff[4096 + k * 1024 + ((ly >> 1) + (r >> 2)) * LCU_C + (lx >> 1) + (r & 3)]);
  }
  CTU_LDS uint32_t *const m = LDSP(uint32_t, S->coder);
  for (int k = 0; k < 4; ++k) {
    const int clx = lx + (k & 1) * 4, cly = ly + (k >> 1) * 4, x = J.x + clx, y = J.y + cly;
    const cu4 *c = cu_at(S, clx, cly);
    const int mode = __builtin_amdgcn_readfirstlane((int)c->mode), cb_y = __builtin_amdgcn_readfirstlane((int)c->cbf) & 1;
    if (parts & CODER_FLAGS) {
      int mpm[6];
      {
        const cu4 *l, *a;
        mpm_neighbours(S, x, y, clx, cly, 4, &l, &a);
        int left_dir = 0, above_dir = 0;
        if (l && l->type == CU_INTRA) left_dir = l->mode;
        if (a && a->type == CU_INTRA && y % LCU != 0) above_dir = a->mode;
        lf_mpm(__builtin_amdgcn_readfirstlane(left_dir), __builtin_amdgcn_readfirstlane(above_dir), mpm);
      }
      SERIAL {
        double dummy = 0;
        if (k == 0)          // split flags of the enclosing quad-tree nodes that begin here (a 4x4 CU has none of its own)
          for (int d = 0; (64 >> d) > 4; ++d) {
            const int sz = 64 >> d;
            if (!(lx & (sz - 1)) && !(ly & (sz - 1))) split_flag_bits(S, P, S->coder, 1, x, y, lx, ly, sz, 1, dummy);
          }
        lf_luma_mode_bits(S->coder, mpm, mode, dummy);
        m_code(m, 1, M_CBF_LUMA + 0, cb_y, dummy);
      }
      CTU_SYNC();
    }
    if ((parts & CODER_LUMA) && cb_y) (void)coeff_bits4r<PX, false>(S, m, 1, lf_shfl(lev_all, k * 16 + r), 0);
    if (k == 3) {
      // the area's chroma after its last luma CU: mode (the co-located luma CU is this one), cbfs of the area's first entry, levels
      const cu4 *a = cu_at(S, lx, ly);
      const int acbf = __builtin_amdgcn_readfirstlane((int)a->cbf), au = (acbf >> 1) & 1, av = (acbf >> 2) & 1;
      if (parts & CODER_FLAGS) {
        SERIAL {
          double dummy = 0;
          chroma_mode_bits(S->coder, 1, c->mode_chroma, c->mode, dummy);
          m_code(m, 1, M_CBF_CB + 0, au, dummy);
          m_code(m, 1, M_CBF_CR + au, av, dummy);
        }
        CTU_SYNC();
      }
      if (parts & CODER_CHROMA) {
        if (au) (void)coeff_bits4r<PX, false>(S, m, 1, lf_shfl(clev, r), 1);
        if (av) (void)coeff_bits4r<PX, false>(S, m, 1, lf_shfl(clev, 16 + r), 2);
      }
    }
  }
  CTU_SYNC();
}
#endif

template <typename PX> CTU_NOINLINE CTU_DEV void coder_pass(lds<PX> *S, const job<PX> &J, int parts)
{
  wctx *const V = wv_of(S);
  const params &P = J.P;
  // the chroma pass runs on depth 2's scratch: a 16x16 block is that depth's luma size, Cb and Cr take turns in its luma level array
  int16_t *const lvu = parts == CODER_CHROMA ? V->lv0 : lv_of(V, 1), *const lvv = parts == CODER_CHROMA ? V->lv0 : lv_of(V, 2);
  for (int z = 0; z < 256; ++z) {
    const int lx = z_to_x(z) * 4, ly = z_to_x(z >> 1) * 4;
    const int x = J.x + lx, y = J.y + ly;
    if (x >= P.pic_w || y >= P.pic_h) continue;
    const cu4 *c = cu_at(S, lx, ly);
    const int n = 1 << c->log2;
    if ((lx & (n - 1)) || (ly & (n - 1))) continue;
#if defined(__HIPCC__)
    if (n == 4) {              // (4x4 CUs come as whole 8x8 areas, the first of the four at the area's origin)
      if (!(lx & 4) && !(ly & 4)) coder_area4(S, J, lx, ly, parts);
      continue;
    }
#endif
    const int sep = n == 4, last4 = sep && (lx & 4) && (ly & 4);
    const int tus = n == 64 ? 4 : 1, tn = n == 64 ? 32 : n;
    for (int tu = 0; tu < tus; ++tu) {
      const int tlx = lx + (tu & 1) * 32, tly = ly + (tu >> 1) * 32;
      const cu4 *t = cu_at(S, tlx, tly);
      const int cb_y = t->cbf & 1, cb_u = (t->cbf >> 1) & 1, cb_v = (t->cbf >> 2) & 1;
      // the chroma blocks of this transform unit (for the last 4x4 CU of an 8x8 area: the area's)
      const int has_c = !sep || last4;
      const int cw = sep ? 4 : tn >> 1, cl2 = ilog2_dev(cw);
      const int cbx = (sep ? (tlx & ~7) : tlx) >> 1, cby = (sep ? (tly & ~7) : tly) >> 1;
      const cu4 *a = sep ? cu_at(S, lx & ~7, ly & ~7) : t;       // (4x4 CUs: the flags of the area's first entry)
      const int au = sep ? (a->cbf >> 1) & 1 : cb_u, av = sep ? (a->cbf >> 2) & 1 : cb_v;
      uint32_t *m = S->coder;
      if (parts & CODER_FLAGS) {
        SERIAL {
          double dummy = 0;
          if (tu == 0) {
            // split flags of the enclosing quad-tree nodes that begin here, then this CU's own
            for (int d = 0; (64 >> d) > n; ++d) {
              const int s = 64 >> d;
              if (!(lx & (s - 1)) && !(ly & (s - 1))) split_flag_bits(S, P, m, 1, x, y, lx, ly, s, 1, dummy);
            }
            split_flag_bits(S, P, m, 1, x, y, lx, ly, n, 0, dummy);
            luma_mode_bits(S, m, 1, x, y, lx, ly, n, c->mode, dummy);
            if (!sep) chroma_mode_bits(m, 1, c->mode_chroma, c->mode, dummy);
          }
          if (!sep) {
            m_code(m, 1, M_CBF_CB + 0, cb_u, dummy);
            m_code(m, 1, M_CBF_CR + cb_u, cb_v, dummy);
          }
          m_code(m, 1, M_CBF_LUMA + 0, cb_y, dummy);      // luma_cbf_ctx stays 0: one transform unit per CU, or a CU that is not a TU
          if (last4) {
            // the area's chroma after its last luma CU: mode (the co-located luma CU is this one), cbfs of the area's first entry
            chroma_mode_bits(m, 1, c->mode_chroma, c->mode, dummy);
            m_code(m, 1, M_CBF_CB + 0, au, dummy);
            m_code(m, 1, M_CBF_CR + au, av, dummy);
          }
        }
        CTU_SYNC();
      }
      if ((parts & CODER_LUMA) && cb_y) {
        const int16_t *co = J.coeff + tly * LCU + tlx;
        const int l2 = ilog2_dev(tn);
        PAR_FOR(e, tn * tn) lv_of(V, 0)[e] = CTU_GLOAD(&co[(e >> l2) * LCU + (e & (tn - 1))]);
        CTU_SYNC();
        (void)coeff_bits<PX, false>(S, m, 1, lv_of(V, 0), tn, 0);
      }
      if ((parts & CODER_CHROMA) && has_c) {
        if (au) {
          PAR_FOR(e, cw * cw) lvu[e] = CTU_GLOAD(&J.coeff[4096 + (cby + (e >> cl2)) * LCU_C + cbx + (e & (cw - 1))]);
          CTU_SYNC();
          (void)coeff_bits<PX, false>(S, m, 1, lvu, cw, 1);
        }
        if (av) {
          PAR_FOR(e, cw * cw) lvv[e] = CTU_GLOAD(&J.coeff[5120 + (cby + (e >> cl2)) * LCU_C + cbx + (e & (cw - 1))]);
          CTU_SYNC();
          (void)coeff_bits<PX, false>(S, m, 1, lvv, cw, 2);
        }
      }
      CTU_SYNC();
    }
  }
}

template <typename PX> CTU_NOINLINE CTU_DEV void load_ctu(lds<PX> *S, const job<PX> &J)
{
  const params &P = J.P;
  const int x = J.x, y = J.y, W = P.pic_w, H = P.pic_h;
  BLK_FOR(i, 17 * 17) { cu4 z = {0, 0, 0, 0, 0, 0, 0, 0}; S->cu[i] = z; }
  BLK_FOR(i, 256) { J.W->tree[i] = 0; J.W->mtt[i] = 0; }
  if (BLK_TID == 0) S->scr = J.W;
  BLK_SYNC();
  BLK_FOR(i, 33) {
    // i = 0: the corner, 1..16 the row above, 17..32 the column to the left
    int ax, ay, ok;
    if (i == 0) { ax = x - 4; ay = y - 4; ok = x > 0 && y > 0; }
    else if (i <= 16) { ax = x + (i - 1) * 4; ay = y - 4; ok = y > 0 && ax < W; }
    else { ax = x - 4; ay = y + (i - 17) * 4; ok = x > 0 && ay < H; }
    if (ok) {
      const uvghip_scu_t *s = &J.cu_tab[(ay >> 2) * J.cu_stride + (ax >> 2)];
      cu4 *c = cu_at(S, ax - x, ay - y);
      c->type = s->type; c->log2 = s->log2_width; c->cbf = s->cbf; c->log2_c = s->log2_chroma_width;
      c->mode = (int8_t)(s->mv[0][0] & 0xff); c->mode_chroma = (int8_t)((s->mv[0][0] >> 8) & 0xff);
    }
  }
  for (int color = 0; color < 3; ++color) {
    const int c = color != 0, w = 64 >> c, pit = pitch_of(color);
    PX *D = plane(S, color);
    const PX *rec = color == 0 ? J.rec_y : (color == 1 ? J.rec_u : J.rec_v);
    const int rs = c ? J.rec_stride_c : J.rec_stride;
    const int px = x >> c, py = y >> c, pw = W >> c, ph = H >> c;
    BLK_FOR(i, 2 * w + 1) {
      // i = 0 corner, 1..w the row above, w + 1..2w the column to the left
      if (i == 0) { if (px > 0 && py > 0) D[0] = rec[(py - 1) * rs + px - 1]; }
      else if (i <= w) { const int q = px + i - 1; if (py > 0 && q < pw) D[i] = rec[(py - 1) * rs + q]; }
      else { const int r = py + i - w - 1; if (px > 0 && r < ph) D[(i - w) * pit] = rec[r * rs + px - 1]; }
    }
  }
  BLK_FOR(i, 512) tab_ebits()[i] = kEntropyBits[i];
  BLK_FOR(i, NMODELS) {
    tab_rate()[i] = k_ctx_init[3][i];
    if (J.models_in) S->coder[i] = J.models_in[i];
#if defined(CTU_PB)
    else models_init_one(S->coder, i, J.init_qp, J.slice_type);
#else
    else models_init_one(S->coder, i, P.qp, 2);
#endif
  }
#if defined(CTU_PB)
  BLK_FOR(i, NMX - NMODELS) {
    tab_rate()[NMODELS + i] = k_ctx_init_inter[3][i];
    if (J.models_in) S->coder[NMODELS + i] = J.pbm_in[i];
    else {
      const int v = k_ctx_init_inter[J.slice_type][i];
      const int slope = (v >> 3) - 4, offset = ((v & 7) * 18) + 1;
      int st = ((slope * (J.init_qp - 16)) >> 1) + offset;
      st = st < 1 ? 1 : (st > 127 ? 127 : st);
      S->coder[NMODELS + i] = (uint32_t)((st << 8) & 0x7fe0) | ((uint32_t)((st << 8) & 0x7ffe) << 16);
    }
  }
#endif
  BLK_SYNC();
#if defined(CTU_PB)
  BLK_FOR(i, NMX - NMODELS) { const uint32_t v = S->coder[NMODELS + i]; S->cur[NMODELS + i] = v; J.pbm_out[i] = v; }
#endif
  BLK_FOR(i, NMODELS) {
    const uint32_t v = S->coder[i];
    S->cur[i] = v;
    J.models_out[i] = v;
    if (i < 244) {
      const int st = m_state(S->coder, i);
      S->rdoq_state[i] = (uint8_t)st;
      tab_rdoq_bits()[2 * i] = kEntropyBits[st << 1];
      tab_rdoq_bits()[2 * i + 1] = kEntropyBits[(st << 1) ^ 1];
    }
  }
  BLK_SYNC();
  BLK_FOR(cfg, 16) {            // calc_last_bits (rdo.c:664-700) for every shape once: the models uvg_rdoq prices with are the CTU's
    const int t = cfg >> 3, l2 = 2 + ((cfg >> 1) & 3), xy = cfg & 1, n = 1 << l2;
    const int prefix_ctx[8] = {0, 0, 0, 3, 6, 10, 15, 21};
    const int off = t ? 0 : prefix_ctx[l2];
    const int sh = t ? clampi(n >> 3, 0, 2) : ((l2 + 1) >> 2);
    const int base = (xy ? M_LASTY : M_LASTX) + (t ? 20 : 0) + off;
    int32_t b = 0;
    int ctx;
    if (t && l2 == 5) continue;                 // (no 32x32 chroma block)
    int32_t *const lb = S->last_bits + last_bits_off(t, l2, xy);
    for (ctx = 0; ctx < group_idx(n - 1); ctx++) {
      const int mdl = base + (ctx >> sh);
      lb[ctx] = b + (int32_t)tab_rdoq_bits()[2 * mdl];
      b += (int32_t)tab_rdoq_bits()[2 * mdl + 1];
    }
    lb[ctx] = b;
  }
  BLK_SYNC();
}

// copy_lcu_to_cu_data (search.c:2331-2377) + the models of the three checkpoints
template <typename PX> CTU_NOINLINE CTU_DEV void store_ctu(lds<PX> *S, const job<PX> &J)
{
  const params &P = J.P;
  const int x = J.x, y = J.y, W = P.pic_w, H = P.pic_h;
  for (int color = 0; color < 3; ++color) {
    const int c = color != 0, w = 64 >> c, pit = pitch_of(color);
    const PX *D = plane(S, color) + pit + 1;
    PX *rec = color == 0 ? J.rec_y : (color == 1 ? J.rec_u : J.rec_v);
    const int rs = c ? J.rec_stride_c : J.rec_stride;
    const int px = x >> c, py = y >> c, pw = W >> c, ph = H >> c;
    BLK_FOR(e, w * w) {
      const int r = e / w, q = e - r * w;
      if (py + r < ph && px + q < pw) rec[(py + r) * rs + px + q] = D[r * pit + q];
    }
  }
  BLK_FOR(e, 256) {
    const int lx = (e & 15) * 4, ly = (e >> 4) * 4;
    if (x + lx < W && y + ly < H) {
      const cu4 *c = cu_at(S, lx, ly);
      uvghip_scu_t s;
      memset(&s, 0, sizeof s);
      s.luma_edges = c->luma_edges; s.chroma_edges = c->chroma_edges; s.type = c->type; s.cbf = c->cbf; s.qp = (int8_t)P.qp;
      s.log2_width = s.log2_height = c->log2; s.log2_chroma_width = s.log2_chroma_height = c->log2_c;
      s.mv[0][0] = (int32_t)((uint32_t)(uint8_t)c->mode | (uint32_t)(uint8_t)c->mode_chroma << 8);
      s.mv[0][1] = (int32_t)CTU_GLOAD(&J.W->tree[e]);
      s.mv[1][0] = (int32_t)CTU_GLOAD(&J.W->mtt[e]);
      J.cu_tab[((y + ly) >> 2) * J.cu_stride + ((x + lx) >> 2)] = s;
    }
  }
}

// carve the arena: wv[k] serves depth 4 - k (blocks of 4 << k)
template <typename PX> CTU_DEV void setup_waves(lds<PX> *S, scratch *W = nullptr)
{
  if (lds_cfg<PX>::slim_scan) { if (BLK_TID == 0) S->scr = W; }      // (scan_of reads it before load_ctu sets it again)
  BLK_FOR(k, 4) {
    const int n = 4 << k, nn = n * n, c2 = (n / 2) * (n / 2) < 16 ? 16 : (n / 2) * (n / 2), tiles = n >= 8 ? (n / 8) * (n / 8) : 1;
    int off = 0;
#if !defined(CTU_PB)
    for (int j = 0; j < k; ++j) off += arena_bytes(4 << j);          // (the slim depth-1 share is the last one)
#else
    if (k == 0) off = arena_bytes(32);
#endif
    unsigned char *a = S->arena + off;
#if defined(CTU_PB)
    if (k == 1 && BLK_NT > 128) a = S->arena8;             // (three waves: the walk evaluates 8x8 CUs while the depth wave is in the big region)
    if (k == 2 && BLK_NT > 192) a = S->arena16;            // (four waves: 16x16 and 32x32 CUs on a wave each)
#endif
    unsigned char *const a0 = a;
    wctx *V = &S->wv[k];
    const int rn = 4 * n + 8;
    V->refn = (int16_t)rn;
    V->top = (uint16_t *)a; V->left = V->top + rn; V->ftop = V->left + rn; V->fleft = V->ftop + rn; a += 4 * rn * 2;
    V->t0 = (int16_t *)a; V->t1 = V->t0 + nn; a += 2 * nn * 2;
    if (lds_cfg<PX>::slim && n == 32) { V->lv0 = W->lv32; V->lv1 = V->lv0 + nn; V->lv2 = V->lv1 + c2; }
    else { V->lv0 = (int16_t *)a; V->lv1 = V->lv0 + nn; V->lv2 = V->lv1 + c2; a += (nn + 2 * c2) * 2; }
    // the rough search's (satd, sad) per (mode, tile) -- 2 * 18 * tiles words -- fit the three transform buffers from 8x8 on, which
    // idle until the mode is chosen
#if defined(__HIPCC__)
    if (n == 4) { V->part = nullptr; V->rq_cc = V->rq_cs = nullptr; }       // (the general evaluation never runs on this scratch: eval_cu4)
    else
#endif
    {
    if (n >= 8) V->part = (uint32_t *)V->t0;
    else { V->part = (uint32_t *)a; a += 2 * 18 * tiles * 4; }
    a = a0 + ((a - a0 + 7) & ~7);
    if (n <= 8) { V->rq_cc = (double *)a; V->rq_cs = V->rq_cc + nn; }
    else V->rq_cc = V->rq_cs = nullptr;
    }
    V->cur = S->cur;
    S->vsel[k] = k;
    S->req[k] = 0; S->done[k] = 0;
#if !defined(CTU_PB)
    if (k == 0) { S->req64 = 0; S->done64[0] = 0; S->done64[1] = 0; S->creq = 0; S->cdone[0] = 0; S->cdone[1] = 0; }
#endif
  }
  BLK_SYNC();
}

// one CTU, start to finish (all four waves)
template <typename PX> CTU_DEV void run_ctu(lds<PX> *S, const job<PX> &J)
{
  CTU_PROF_RESET(S, J)
  CTU_T0();
  { CTU_T0();
  setup_waves(S, J.W);
#if defined(__HIPCC__)
  leaf_tables(S, J.P);
#endif
  if (CTU_WAVE == 0) build_scans(S);
  BLK_SYNC();
  load_ctu(S, J);
  // the CTU's coefficient array starts empty (lcu->coeff = calloc, encoderstate.c:752)
  BLK_FOR(e, 6144) J.coeff[e] = 0;
  BLK_SYNC();
  CTU_T1(J.W, 9); }
#if defined(__HIPCC__)
  if (CTU_WAVE == 0) {
    __builtin_amdgcn_s_setprio(3);        // the walker is the CTU's critical path: it wins the issue slot against the depth waves sharing its SIMD
#endif
    search_ctu(S, J);
    PAR_FOR(i, NMODELS) J.models_out[NMODELS + i] = S->cur[i];
    { CTU_T0();
    SERIAL S->vsel[CTU_WAVE] = 3;          // the depth-1 scratch for the coder's 32x32 blocks: the other waves are idle now
    CTU_SYNC();
#if defined(__HIPCC__)
    // the coder's pass, split by model (CODER_*): the flags on depth 3's wave, the chroma coefficients on depth 2's, the luma
    // coefficients here
    SERIAL mb_store(&S->creq, 1);
    { CTU_T0();
    coder_pass(S, J, CODER_LUMA);
    CTU_T1(J.W, 14); }        // (profile slot 14 of the walk's wave: its own part; slot 8: with the wait for the other two)
    while (mb_load(&S->cdone[0]) == 0 || mb_load(&S->cdone[1]) == 0) __builtin_amdgcn_s_sleep(1);
    CTU_SYNC();
#else
    coder_pass(S, J, CODER_LUMA);
    SERIAL S->vsel[CTU_WAVE] = 0;
    emul_on_wave(1, [&] { coder_pass(S, J, CODER_FLAGS); });
    emul_on_wave(2, [&] { coder_pass(S, J, CODER_CHROMA); });
#endif
    CTU_T1(J.W, 8); }
#if defined(__HIPCC__)
    SERIAL { for (int L = 1; L <= 3; ++L) mb_store(&S->req[L], -1); }
  } else {
    worker_loop(S, J);
  }
#endif
  BLK_SYNC();
  { CTU_T0();
  BLK_FOR(i, NMODELS) J.models_out[2 * NMODELS + i] = S->coder[i];
  store_ctu(S, J);
  BLK_SYNC();
  CTU_T1(J.W, 10); }
  CTU_T1(J.W, 11);
}

}  // namespace ctu
