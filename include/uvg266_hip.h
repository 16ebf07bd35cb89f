/*
 * uvg266_hip.h -- C ABI of libuvg266hip.so, the MI355X (gfx950) "hip"
 * strategy backend for uvg266's per-CTU block-processing hot path.
 *
 * Two layers are exported:
 *
 *  (1) Drop-in registrars, one per strategy group, with the reference's
 *      registrar signature (src/strategies/generic/picture-generic.c:1445,
 *      src/strategyselector.h:99):
 *          int uvg_strategy_register_<group>_hip(void *opaque, uint8_t bitdepth);
 *      Each calls the host's uvg_strategyselector_register(opaque, type,
 *      "hip", 50, fptr) for every function of the group this backend
 *      implements (priority 50 > avx2's 40, src/strategyselector.c:283-348).
 *      The registered function pointers have exactly the reference typedefs
 *      (src/strategies/strategies-*.h) and take HOST buffers: one call = one
 *      upload + launch + download.  This is the parity path, not the
 *      throughput path (hard part 1).
 *
 *  (2) A batched ABI over planes that are already resident in HBM
 *      (uvghip_* below).  Every pointer argument is a DEVICE pointer unless
 *      its name ends in _host; `stream` is a hipStream_t passed as void*
 *      (NULL = the default stream).  Calls enqueue work and return without
 *      synchronising.  Return value: 0 on success, otherwise a hipError_t
 *      value (uvghip_last_error() gives text).  `bitdepth` selects the pixel
 *      type the reference fixes at compile time (src/uvg266.h:89-99):
 *      8 -> uint8_t planes, 10 -> uint16_t planes.
 *
 * No type from PyTorch, HIP or the reference appears in any signature.
 */
#ifndef UVG266_HIP_H_
#define UVG266_HIP_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* exported symbol marker (the library is built with -fvisibility=hidden) */
#define UVGHIP_API __attribute__((visibility("default")))

#define UVGHIP_STRATEGY_NAME     "hip"
#define UVGHIP_STRATEGY_PRIORITY 50

/* ------------------------------------------------------------------ core */

/* Select the device and create the per-process context.  Returns 0 or a
 * hipError_t.  Must succeed before any other call; there is NO CPU fallback:
 * without a usable gfx950 device every entry point fails. */
UVGHIP_API int uvghip_init(int device);
/* Text for the last failing call on this thread ("" if none). */
UVGHIP_API const char *uvghip_last_error(void);
/* ABI version of this header (bumped on any signature change). */
UVGHIP_API int uvghip_abi_version(void);

/* A picture's kernel sequence is fixed once its descriptor tables exist, so the host captures it into a hipGraph and
 * replays it with one call per picture (the per-launch host cost of 40 small kernels exceeds their GPU time):
 *   uvghip_graph_begin(stream);  ...any uvghip_*_batch / _frame / _band calls on `stream`...;  uvghip_graph_end(stream, &g);
 *   uvghip_graph_launch(g, any_stream);  ...;  uvghip_graph_destroy(g);
 * Capture is thread-local (hipStreamCaptureModeThreadLocal).  uvghip_comm_* calls are not captured: issue them
 * between graph segments. */
UVGHIP_API int uvghip_graph_begin(void *stream);
UVGHIP_API int uvghip_graph_end(void *stream, void **graph_exec_out);
UVGHIP_API int uvghip_graph_launch(void *graph_exec, void *stream);
UVGHIP_API int uvghip_graph_destroy(void *graph_exec);

/* ---------------------------------------------- (1) drop-in registrars -- */
/* replaces: the line a maintainer adds after
 *   src/strategies/strategies-picture.c:106-108 (avx2 registration), etc.
 * The host's uvg_strategyselector_register symbol is resolved at load time;
 * when the library is loaded stand-alone (tests), uvghip_set_register_fn()
 * must supply it. */
typedef int (*uvghip_register_fn)(void *opaque, const char *type, const char *strategy_name,
                                  int priority, void *fptr);
UVGHIP_API void uvghip_set_register_fn(uvghip_register_fn fn);

UVGHIP_API int uvg_strategy_register_picture_hip(void *opaque, uint8_t bitdepth); /* strategies-picture.h:160-232 */
UVGHIP_API int uvg_strategy_register_dct_hip(void *opaque, uint8_t bitdepth);     /* strategies-dct.h:77-110   */
UVGHIP_API int uvg_strategy_register_intra_hip(void *opaque, uint8_t bitdepth);   /* strategies-intra.h:81-103 */
UVGHIP_API int uvg_strategy_register_sao_hip(void *opaque, uint8_t bitdepth);     /* strategies-sao.h:66-82    */
UVGHIP_API int uvg_strategy_register_quant_hip(void *opaque, uint8_t bitdepth);   /* strategies-quant.h:93-111 (state-free functions only) */
UVGHIP_API int uvg_strategy_register_ipol_hip(void *opaque, uint8_t bitdepth);    /* strategies-ipol.h:116-139 (all ten) */

/* -------------------------------------------- (2) batched ABI: picture -- */

/* One block pair: top-left of the block in the current plane and in the
 * reference plane (integer pel).  The reference position may lie partly or
 * wholly outside the reference frame; samples are then edge-replicated,
 * which is what uvg_image_calc_sad / uvg_image_calc_satd compute
 * (src/image.c:310-428,438-473,482-557). */
typedef struct uvghip_blk {
  int32_t cur_x, cur_y;
  int32_t ref_x, ref_y;
} uvghip_blk_t;

/* replaces: uvg_image_calc_sad -> uvg_reg_sad / uvg_hor_sad / uvg_ver_sad
 * (src/image.c:438; src/strategies/generic/picture-generic.c:99,1266,1308).
 * out[i] = SAD(block i) >> (bitdepth-8).  bw,bh: multiples of 4, 4..64 (any
 * w,h >= 1 accepted).  ref_w/ref_h: visible size of the reference frame. */
UVGHIP_API int uvghip_sad_batch(int bitdepth, const void *cur, int cur_stride, const void *ref, int ref_stride,
                     int ref_w, int ref_h, int bw, int bh,
                     const uvghip_blk_t *blks, int n, uint32_t *out, void *stream);

/* replaces: uvg_image_calc_satd -> uvg_satd_any_size
 * (src/image.c:482; src/strategies/strategies-picture.h:76-109).  Tiling
 * rule: first 4 columns by 4x4 tiles if bw%8, first 4 rows by 4x4 if bh%8,
 * the rest by 8x8; out[i] = sum >> (bitdepth-8). */
UVGHIP_API int uvghip_satd_batch(int bitdepth, const void *cur, int cur_stride, const void *ref, int ref_stride,
                      int ref_w, int ref_h, int bw, int bh,
                      const uvghip_blk_t *blks, int n, uint32_t *out, void *stream);

/* replaces: uvg_pixels_calc_ssd (picture-generic.c:1115); out[i] = SSD >> 2*(bitdepth-8).
 * No clamping: both blocks must be inside their planes. */
UVGHIP_API int uvghip_ssd_batch(int bitdepth, const void *a, int a_stride, const void *b, int b_stride,
                     int bw, int bh, const uvghip_blk_t *blks, int n, uint32_t *out, void *stream);

/* Full-search SAD surface for integer motion estimation: for every bw x bh
 * block of the grid covering the frame (blocks_x = cur_w/bw, blocks_y =
 * cur_h/bh, row-major) and every displacement (dx,dy) in [-range,range]^2,
 *   out[(blk*(2r+1) + (dy+r))*(2r+1) + (dx+r)] = uvg_image_calc_sad(cur, ref,
 *        bx, by, bx+dx, by+dy, bw, bh)
 * i.e. the value check_mv_cost (src/search_inter.c:204) obtains per
 * candidate, for all candidates at once.  The search window of each block is
 * staged once in LDS. */
UVGHIP_API int uvghip_sad_surface(int bitdepth, const void *cur, int cur_stride, const void *ref, int ref_stride,
                       int w, int h, int bw, int bh, int range, uint32_t *out, void *stream);

/* replaces: uvg_generate_residual (picture-generic.c:1360) over whole planes:
 * res[y*res_stride+x] = (int16)(a - b). */
UVGHIP_API int uvghip_residual_plane(int bitdepth, const void *a, int a_stride, const void *b, int b_stride,
                          int16_t *res, int res_stride, int w, int h, void *stream);

/* ------------------------------------------ (2) batched ABI: transforms -- */

/* transform kernel types, values of tr_type_t (src/uvg266.h:235-237) */
#define UVGHIP_TR_DCT2 0
#define UVGHIP_TR_DCT8 1
#define UVGHIP_TR_DST7 2

/* replaces: uvg_dct_NxN / uvg_idct_NxN / uvg_mts_dct / uvg_mts_idct
 * (src/strategies/generic/dct-generic.c:720-750,2560-2678) for n blocks of
 * one shape.  in/out: n contiguous blocks of width*height int16 (row-major,
 * stride = width), exactly the coeff_t buffers the reference passes.
 * width,height in {4,8,16,32}, or "thin" blocks with a dimension of 1 or 2 and at most 64 coefficients (ISP sub-partitions,
 * 2xN chroma of multi-type trees: 2-point DCT-2 and the single-pass 1xN / Nx1 cases, dct-generic.c:1030-1090,2608-2612);
 * type_*: UVGHIP_TR_*; skip_width/skip_height:
 * the reference's zero-out counts (0 for plain DCT-2; use uvghip_mts_select).
 * Forward truncates to int16, inverse clips, as the reference does. */
UVGHIP_API int uvghip_transform_batch(int bitdepth, int inverse, int type_hor, int type_ver, int width, int height,
                           int skip_width, int skip_height, const int16_t *in, int16_t *out, int n,
                           void *stream);

/* Host helper, no device work: uvg_get_tr_type (dct-generic.c:2501-2557) and
 * the skip rules of mts_dct_generic (:2582-2600) on plain arguments.
 * color: 0 luma / 1,2 chroma; cu_type: cu_type_t value (1 intra, 2 inter);
 * mts_type: enum uvg_mts (src/uvg266.h:225-229). */
UVGHIP_API int uvghip_mts_select(int width, int height, int color, int cu_type, int isp_mode, int lfnst_idx,
                      int cr_lfnst_idx, int tr_idx, int mts_type, int *type_hor, int *type_ver,
                      int *skip_width, int *skip_height);

/* ------------------------------------- (2) batched ABI: quantisation / TU -- */

/* replaces: uvg_quant (src/strategies/generic/quant-generic.c:51-121) with the
 * values it reads from encoder_state_t passed explicitly:
 *   qp_scaled      = uvg_get_scaled_qp(color, state->qp, (bitdepth-8)*6, qp_map[0])  (src/transform.c:150)
 *   slice_is_intra = state->frame->slicetype == UVG_SLICE_I  (rounding offset 171 vs 85, :77)
 * Scaling lists off, lfnst_idx 0, sign hiding off (signhide=0 in the presets of
 * the target configs).  coef/q_coef: n contiguous blocks of width*height int16. */
UVGHIP_API int uvghip_quant_batch(int bitdepth, const int16_t *coef, int16_t *q_coef, int width, int height, int n,
                       int qp_scaled, int transform_skip, int slice_is_intra, void *stream);

/* replaces: uvg_quant with lfnst_idx != 0 (quant-generic.c:101-120): only the first 8 (4x4 / 8x8 blocks) or 16 coefficients
 * of the diagonal scan are quantised, everything else is zero.  This branch takes its scale from the (flat) encoder
 * scaling-list array, which has no sqrt(2) variant for blocks with an odd log2 size sum (scalinglist.c:415-417) while
 * q_bits keeps that adjustment -- reproduced, so that levels equal the reference's. */
UVGHIP_API int uvghip_quant_lfnst_batch(int bitdepth, const int16_t *coef, int16_t *q_coef, int width, int height, int n,
                             int qp_scaled, int transform_skip, int slice_is_intra, void *stream);

/* replaces: uvg_quant with cfg.signhide_enable = 1 (quant-generic.c:51-232; presets slow and slower): the levels of
 * uvghip_quant_batch (lfnst_idx 0) or uvghip_quant_lfnst_batch, then sign-bit hiding per 4x4 coefficient group -- where the first
 * and last non-zero levels of a group are at least 4 scan positions apart and the parity of their sum disagrees with the sign of
 * the first one, the level with the smallest quantisation-error cost is moved by one.  width, height in {4,8,16,32}. */
UVGHIP_API int uvghip_quant_signhide_batch(int bitdepth, const int16_t *coef, int16_t *q_coef, int width, int height, int n,
                                int qp_scaled, int transform_skip, int slice_is_intra, int lfnst_idx, void *stream);

/* replaces: uvg_dequant (quant-generic.c:618-669), no scaling list / dep-quant. */
UVGHIP_API int uvghip_dequant_batch(int bitdepth, const int16_t *q_coef, int16_t *coef, int width, int height, int n,
                         int qp_scaled, int transform_skip, void *stream);

/* replaces: uvg_coeff_abs_sum (quant-generic.c:671): out[b] = sum |c| over `length` coefficients of block b. */
UVGHIP_API int uvghip_coeff_abs_sum_batch(const int16_t *coeffs, int length, int n, uint32_t *out, void *stream);

/* replaces: uvg_fast_coeff_cost (quant-generic.c:688): weights = four packed u16 for |c| = 0,1,2,>=3. */
UVGHIP_API int uvghip_fast_coeff_cost_batch(const int16_t *coeffs, int width, int height, int n, uint64_t weights,
                                 uint32_t *out, void *stream);

/* ---- rate-distortion optimised quantisation ---- */

/* Snapshot of the CABAC context models uvg_rdoq prices bins with (state->cabac.ctx, src/cabac.h:60-131), each reduced
 * to CTX_STATE(ctx) = (ctx->state[0] + ctx->state[1]) >> 8 (cabac.h:175-176) -- all CTX_ENTROPY_BITS (rdo.h:106)
 * looks at.  [0] = luma, [1] = chroma where the reference keeps separate models (unused tail entries zero).  The
 * models are read-only during a call, which is what makes the blocks of a batch independent. */
typedef struct uvghip_rdoq_ctx {
  uint8_t sig_group[2][2];    /* sig_coeff_group_model[0..1] | [2..3] */
  uint8_t sig[2][12];         /* cu_sig_model_luma[0][0..11] | cu_sig_model_chroma[0][0..7] */
  uint8_t par[2][21];         /* cu_parity_flag_model_luma[21] | _chroma[11] */
  uint8_t gt1[2][21];         /* cu_gtx_flag_model_luma[1][21] | _chroma[1][11] */
  uint8_t gt2[2][21];         /* cu_gtx_flag_model_luma[0][21] | _chroma[0][11] */
  uint8_t last_x[2][20];      /* cu_ctx_last_x_luma[20] | _chroma[3] */
  uint8_t last_y[2][20];      /* cu_ctx_last_y_luma[20] | _chroma[3] */
  uint8_t cbf_luma[4], cbf_cb[2], cbf_cr[3];   /* qt_cbf_model_luma / _cb / _cr */
  uint8_t root_cbf;           /* cu_qt_root_cbf_model */
} uvghip_rdoq_ctx_t;

/* replaces: uvg_rdoq (src/rdo.c:1449-1870; called from uvg_quantize_residual when cfg.rdoq_enable,
 * quant-generic.c:527-531) for n transformed blocks of one shape: q_coef[i] = the RD-optimal levels of coef[i]
 * (both n contiguous blocks of width*height int16).  width, height in {4,8,16,32}.  What the reference reads from
 * encoder_state_t is passed in:
 *   qp_scaled  = uvg_get_scaled_qp(color, state->qp, (bitdepth-8)*6, qp_map[0])          (src/transform.c:150)
 *   lambda     = color ? state->c_lambda : state->lambda
 *   ctx_host   = the context snapshot above (HOST pointer, copied into the launch)
 *   block_type = cu_type_t (1 intra), cbf_u = cbf_is_set(cbf, COLOR_U) (only read for color 2),
 *   lfnst_idx / mts_idx as the reference's arguments.
 * Scaling lists and sign-data hiding off (as in every preset of the target configs); diagonal scan.
 * workspace: device memory of at least uvghip_rdoq_workspace_bytes(width, height, n) bytes (the per-position cost
 * arrays the last-position search re-reads).  abs_sum_out[i] (may be NULL) = sum of |level|; has_coeffs[i] (may be
 * NULL) = any level != 0.  Costs are IEEE doubles in the reference's operation order: levels are bit-exact. */
UVGHIP_API size_t uvghip_rdoq_workspace_bytes(int width, int height, int n);
UVGHIP_API int uvghip_rdoq_batch(int bitdepth, const int16_t *coef, int16_t *q_coef, int width, int height, int n, int color,
                      int block_type, int cbf_u, int lfnst_idx, int mts_idx, int qp_scaled, double lambda,
                      const uvghip_rdoq_ctx_t *ctx_host, void *workspace, size_t workspace_bytes,
                      uint32_t *abs_sum_out, uint8_t *has_coeffs, void *stream);

/* uvg_rdoq with cfg.signhide_enable = 1 (presets slow and slower): the walk also records struct sh_rates_t (rdo.c:214-223,
 * 1660-1687) and uvg_rdoq_sign_hiding (:700-845) runs at the end.  Same arguments as uvghip_rdoq_batch; the workspace holds the
 * rate records too: >= uvghip_rdoq_signhide_workspace_bytes(width, height, n).  lambda must be > 0.  abs_sum_out / has_coeffs
 * are the values before the hiding step (what :1865 tests). */
UVGHIP_API size_t uvghip_rdoq_signhide_workspace_bytes(int width, int height, int n);
UVGHIP_API int uvghip_rdoq_signhide_batch(int bitdepth, const int16_t *coef, int16_t *q_coef, int width, int height, int n, int color,
                               int block_type, int cbf_u, int lfnst_idx, int mts_idx, int qp_scaled, double lambda,
                               const uvghip_rdoq_ctx_t *ctx_host, void *workspace, size_t workspace_bytes,
                               uint32_t *abs_sum_out, uint8_t *has_coeffs, void *stream);

/* ---- CABAC bit cost of coefficient blocks ---- */

/* The context models of the coefficient coder with their full state (cabac_ctx_t, src/cabac.h:47-51: two 16-bit probability
 * states and the rate byte), in the index space of uvghip_rdoq_ctx_t: model i of that struct is entry i here, and
 * CTX_STATE = (state0[i] + state1[i]) >> 8. */
typedef struct uvghip_cabac_models {
  uint16_t state0[244], state1[244];
  uint8_t rate[244];
} uvghip_cabac_models_t;

/* replaces: uvg_get_coeff_cost on its CABAC branch = get_coeff_cabac_cost (src/rdo.c:297-356, taken when the QP is not below
 * cfg.fast_residual_cost_limit; the other branch is uvghip_fast_coeff_cost_batch) -> uvg_encode_coeff_nxn in count mode
 * (encode_coding_tree-generic.c:53-323) for n blocks of one shape: bits_out[i] = the bits the coefficient coder would spend on
 * block i starting from the models in models_host (HOST pointer; every block starts from the same copy, as the reference copies
 * its search CABAC per call), with the models adapting bin by bin inside the block.  0.0 for an all-zero block.
 * flags_out[i] (may be NULL): what the coder records in cur_cu on the way -- bit 0 violates_lfnst_constrained_luma/_chroma,
 * bit 1 lfnst_last_scan_pos, bit 2 mts_last_scan_pos, bit 3 violates_mts_coeff_constraint (:113-121, :303-317).
 * width, height in {4,8,16,32}; diagonal scan; dependent quantisation and sign-data hiding off; not for transform-skip blocks
 * (uvg_encode_ts_residual). */
UVGHIP_API int uvghip_coeff_cost_batch(const int16_t *coeff, int width, int height, int n, int color,
                            const uvghip_cabac_models_t *models_host, double *bits_out, uint8_t *flags_out, void *stream);

/* top-left corner of a transform unit inside the planes */
typedef struct uvghip_tu {
  int32_t x, y;
} uvghip_tu_t;

/* replaces: uvg_quantize_residual (quant-generic.c:460-612) on its plain-quant
 * branch (no RDOQ / dep-quant / transform skip / LFNST / LMCS chroma scaling),
 * for n TUs of one shape lying at tus[i] in three co-located planes:
 *   residual = orig - pred -> forward transform -> quant -> coeff_out[i]
 *   -> dequant -> inverse transform -> rec = clip(pred + residual)
 * has_coeffs[i] (may be NULL) = any level != 0.  rec may alias pred only if no
 * two TUs overlap.  type_* / skip_* as for uvghip_transform_batch. */
UVGHIP_API int uvghip_tu_roundtrip_batch(int bitdepth, int type_hor, int type_ver, int skip_width, int skip_height,
                              int width, int height, int qp_scaled, int slice_is_intra,
                              const void *orig, int orig_stride, const void *pred, int pred_stride,
                              void *rec, int rec_stride, const uvghip_tu_t *tus, int n,
                              int16_t *coeff_out, uint8_t *has_coeffs, void *stream);

/* The two halves of uvg_quantize_residual around the quantiser, for hosts that run the quantiser over a larger batch than
 * the plane kernels (e.g. RDOQ over the TUs of several pictures in one launch):
 *   forward: residual = orig - pred (uvg_generate_residual) -> uvg_transform2d | uvg_transformskip -> coef_out[i]
 *            (quant-generic.c:483-502), n contiguous blocks of width*height int16, the reference's coeff_t buffer;
 *   inverse: coef_in[i] = DEQUANTISED coefficients -> uvg_itransform2d | uvg_itransformskip -> rec = clip(pred + residual)
 *            (:565-597).
 * type_* / skip_* from uvghip_mts_select. */
UVGHIP_API int uvghip_tu_forward_batch(int bitdepth, int type_hor, int type_ver, int skip_width, int skip_height, int width, int height,
                            int use_trskip, const void *orig, int orig_stride, const void *pred, int pred_stride,
                            const uvghip_tu_t *tus, int n, int16_t *coef_out, void *stream);
UVGHIP_API int uvghip_tu_inverse_batch(int bitdepth, int type_hor, int type_ver, int skip_width, int skip_height, int width, int height,
                            int use_trskip, const int16_t *coef_in, const void *pred, int pred_stride, void *rec, int rec_stride,
                            const uvghip_tu_t *tus, int n, void *stream);

/* uvghip_dequant_batch (uvg_dequant, quant-generic.c:618-669, no transform skip / scaling list) followed by
 * uvghip_tu_inverse_batch, in one launch: `levels` are dequantised as the inverse transform loads them.  Square blocks of
 * 4..32 without zero-out, levels 16-byte aligned; other shapes: hipErrorNotSupported (use the two entry points). */
UVGHIP_API int uvghip_tu_dequant_inverse_batch(int bitdepth, int type_hor, int type_ver, int width, int height, int qp_scaled,
                                    const int16_t *levels, const void *pred, int pred_stride, void *rec, int rec_stride,
                                    const uvghip_tu_t *tus, int n, void *stream);

/* Everything uvg_quantize_residual reads from its arguments, the CU and the encoder state (quant-generic.c:460-612). */
typedef struct uvghip_qr_params {
  int32_t width, height, color;                          /* TU shape; COLOR_Y/U/V = 0/1/2 */
  int32_t type_hor, type_ver, skip_width, skip_height;   /* uvghip_mts_select for this CU */
  int32_t qp_scaled, slice_is_intra, cu_type;            /* as uvghip_quant_batch; cu_type = cur_cu->type (1 intra, 2 inter) */
  int32_t use_trskip;                                    /* uvg_quantize_residual's use_trskip: identity transform; the quantiser's TS
                                                          * shifts only for luma (tr_idx == MTS_SKIP && color == COLOR_Y, :537-539) */
  int32_t rdoq_enable, rdoq_skip, dep_quant;             /* cfg.rdoq_enable / cfg.rdoq_skip / cfg.dep_quant (must be 0) */
  int32_t cbf_u;                                         /* cbf_is_set(cur_cu->cbf, COLOR_U): RDOQ of a V block reads it */
  int32_t mts_idx;                                       /* cur_cu->tr_idx (passed to RDOQ for luma) */
  int32_t lfnst_idx;                                     /* lfnst_index as uvg_quant / uvg_rdoq receive it (cur_cu->lfnst_idx, or
                                                          * cr_lfnst_idx for chroma of a chroma tree; :505): with it != 0 the
                                                          * quantiser keeps only the first 8 / 16 scan positions (:101-120) even
                                                          * where the transform itself does not apply */
  int32_t signhide_enable;                               /* cfg.signhide_enable: sign-data hiding in uvg_quant / uvg_rdoq */
  double lambda;                                         /* color ? state->c_lambda : state->lambda */
  uvghip_rdoq_ctx_t ctx;                                 /* state->cabac context snapshot (RDOQ only) */
} uvghip_qr_params_t;

/* replaces: uvg_quantize_residual (quant-generic.c:460-612) on EVERY branch but dependent quantisation, transform-skip
 * RDOQ, LMCS chroma scaling and scaling lists -- for n TUs of one shape at tus[i] in three co-located planes:
 *   residual -> uvg_transform2d or uvg_transformskip -> [uvg_fwd_lfnst] -> uvg_rdoq | uvg_quant -> coeff_out[i], has_coeffs[i]
 *   -> uvg_dequant -> [uvg_inv_lfnst] -> uvg_itransform2d | uvg_itransformskip -> rec = clip(pred + residual)
 * as a chain of launches through `workspace` (device, >= uvghip_quantize_residual_workspace_bytes(p, n)).
 * uvghip_tu_roundtrip_batch is the single-launch form of the plain-quant / no-LFNST branch.  lfnst_tus: device array of
 * n entries for uvghip_lfnst_batch, or NULL where the LFNST transform does not apply (cfg.lfnst off, inter CU, chroma of
 * a single tree: uvg_fwd_lfnst, transform.c:988).  p: HOST pointer. */
struct uvghip_lfnst_tu;   /* defined in the LFNST section below */
UVGHIP_API size_t uvghip_quantize_residual_workspace_bytes(const uvghip_qr_params_t *p, int n);
UVGHIP_API int uvghip_quantize_residual_batch(int bitdepth, const uvghip_qr_params_t *p, const void *orig, int orig_stride,
                                   const void *pred, int pred_stride, void *rec, int rec_stride, const uvghip_tu_t *tus,
                                   int n, const struct uvghip_lfnst_tu *lfnst_tus, int16_t *coeff_out, uint8_t *has_coeffs,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* replaces: uvg_quant_cbcr_residual (quant-generic.c:241-442; cfg.jccr): joint coding of the Cb and Cr residuals of n TUs of one
 * shape at tus[i] in the two chroma planes -- combined residual by joint_cb_cr (1..3) and the picture's jccr_sign ->
 * uvg_transform2d -> [uvg_fwd_lfnst] -> uvg_rdoq | uvg_quant (contexts / QP of V for joint_cb_cr == 1, else of U) ->
 * coeff_out[i] -> uvg_dequant -> [uvg_inv_lfnst] -> uvg_itransform2d -> both reconstructions.
 * ret_out[i] = the function's return value: joint_cb_cr if the block has coefficients, else 0.  early_skip as the reference's
 * argument (reconstruction = prediction).  p: as for uvghip_quantize_residual_batch (color is derived, use_trskip ignored;
 * qp_scaled = the chroma QP).  workspace >= uvghip_quant_cbcr_residual_workspace_bytes(p, n). */
UVGHIP_API size_t uvghip_quant_cbcr_residual_workspace_bytes(const uvghip_qr_params_t *p, int n);
UVGHIP_API int uvghip_quant_cbcr_residual_batch(int bitdepth, const uvghip_qr_params_t *p, int joint_cb_cr, int jccr_sign,
                                     const void *u_orig, const void *v_orig, int orig_stride, const void *u_pred,
                                     const void *v_pred, int pred_stride, void *u_rec, void *v_rec, int rec_stride,
                                     const uvghip_tu_t *tus, int n, const struct uvghip_lfnst_tu *lfnst_tus, int16_t *coeff_out,
                                     uint8_t *ret_out, int early_skip, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------ (2) batched ABI: intra -------- */

/* One intra block in a reconstructed plane.  avail_top / avail_left are the
 * numbers of already reconstructed samples to the top(-right) and left(-below)
 * of the block that may be used as references, i.e. px_available_top/left of
 * uvg_intra_build_reference after all its limits (coded-neighbour count * 4,
 * cu+pu size, picture size, WPP clamp; src/intra.c:850-852,1038-1039,1252-1318).
 * The caller knows the coding order; the kernels never guess it. */
typedef struct uvghip_intra_blk {
  int32_t x, y;
  int32_t avail_top, avail_left;
} uvghip_intra_blk_t;

/* replaces: uvg_intra_build_reference + uvg_intra_predict (src/intra.c:1344,1372:
 * reference rows incl. [1 2 1]/4 smoothing, planar / DC / angular with wide
 * angles, PDPC) for n blocks of one shape and a list of n_modes signalled modes
 * (0 planar, 1 DC, 2..66).  MRL 0, no ISP/MIP/CCLM.
 * preds_out: [n][n_modes][height*width] pixels. */
UVGHIP_API int uvghip_intra_pred_batch(int bitdepth, const void *rec, int rec_stride, int is_chroma, int width, int height,
                            const uvghip_intra_blk_t *blks, int n, const int8_t *modes, int n_modes,
                            void *preds_out, void *stream);

/* replaces: uvg_mip_predict = mip_predict_generic (src/strategies/generic/intra-generic.c:579-727) with the
 * reference rows built from the plane as in uvghip_intra_pred_batch (MRL 0): matrix-based intra prediction of n
 * blocks of one shape (4..64 per side).  mode_transp[i] = mip_mode | transpose << 7 (modes 0..15 for 4x4, 0..7 for
 * 4xN / Nx4 / 8x8, 0..5 otherwise).  preds_out: [n][height*width]. */
UVGHIP_API int uvghip_mip_pred_batch(int bitdepth, const void *rec, int rec_stride, int width, int height,
                          const uvghip_intra_blk_t *blks, int n, const uint8_t *mode_transp, void *preds_out,
                          void *stream);

/* replaces: the rough mode search loop of search_intra_rough (src/search_intra.c:986-1110)
 * = uvg_intra_predict + get_cost_dual (:133-158) per candidate, for n square luma
 * blocks of `size` (4..32) and all n_modes candidates at once:
 *   costs[i*n_modes + m] = min(SATD, 2*SAD)(pred of modes[m], orig block at (x,y)).
 * Predictions stay in registers; only costs are written. */
UVGHIP_API int uvghip_intra_search_batch(int bitdepth, const void *rec, int rec_stride, const void *orig, int orig_stride,
                              int size, const uvghip_intra_blk_t *blks, int n, const int8_t *modes, int n_modes,
                              uint32_t *costs, void *stream);

/* uvghip_intra_search_batch + uvghip_intra_select_best in one launch: the whole rough search of
 * search_intra_rough (src/search_intra.c:986-1110) down to its winner.  best_mode[i] = the candidate
 * with the smallest min(SATD, 2*SAD), ties to the earlier candidate (strict "<", :1089-1101);
 * best_cost (may be NULL) its cost; costs (may be NULL) the full [n][n_modes] matrix as above.
 * Without `costs` the kernel writes 5 bytes per block instead of 4*n_modes. */
UVGHIP_API int uvghip_intra_search_best_batch(int bitdepth, const void *rec, int rec_stride, const void *orig, int orig_stride,
                                   int size, const uvghip_intra_blk_t *blks, int n, const int8_t *modes,
                                   int n_modes, int8_t *best_mode, uint32_t *best_cost, uint32_t *costs,
                                   void *stream);

/* As uvghip_intra_pred_batch for square luma blocks, but every block has its own decided mode
 * (modes[i]) and the prediction is written into `pred_plane` at the block's position: the
 * predict step of uvg_intra_recon_cu (src/intra.c:1537-1580). */
UVGHIP_API int uvghip_intra_pred_plane_batch(int bitdepth, const void *rec, int rec_stride, int size,
                                  const uvghip_intra_blk_t *blks, int n, const int8_t *modes,
                                  void *pred_plane, int pred_stride, void *stream);

/* uvghip_intra_pred_plane_batch for a chroma plane (4:2:0): no reference smoothing, 2-tap interpolation, the chroma
 * PDPC rules (intra-generic.c:55-295 with channel_type != COLOR_Y; intra.c:690-726).  modes[i]: the final chroma mode
 * (0, 1, 2..66 -- for the derived mode that is the co-located luma mode, src/search_intra.c:1657). */
UVGHIP_API int uvghip_intra_pred_plane_chroma_batch(int bitdepth, const void *rec, int rec_stride, int size,
                                         const uvghip_intra_blk_t *blks, int n, const int8_t *modes,
                                         void *pred_plane, int pred_stride, void *stream);

/* The three entry points above for a STACK of pictures: `rec` / `orig` / `pred_plane` hold several pictures of pic_rows rows
 * each, one under the other with the same stride; blks[i].y is a row of the stack.  A block's neighbours are looked up in its
 * own picture (a block on row 0 of its picture has no row above, whatever lies above it in the stack), so one launch
 * serves the blocks of all pictures -- frame-parallel operation, where one picture alone does not fill the GPU.
 * pic_rows == 0: as the plain entry points.  uvghip_intra_pred_plane_stacked_batch: is_chroma selects the chroma rules of
 * uvghip_intra_pred_plane_chroma_batch. */
UVGHIP_API int uvghip_intra_search_best_stacked_batch(int bitdepth, const void *rec, int rec_stride, const void *orig,
                                           int orig_stride, int size, const uvghip_intra_blk_t *blks, int n,
                                           const int8_t *modes, int n_modes, int8_t *best_mode, uint32_t *best_cost,
                                           uint32_t *costs, int pic_rows, void *stream);
UVGHIP_API int uvghip_intra_pred_plane_stacked_batch(int bitdepth, const void *rec, int rec_stride, int size,
                                          const uvghip_intra_blk_t *blks, int n, const int8_t *modes,
                                          void *pred_plane, int pred_stride, int pic_rows, int is_chroma, void *stream);

/* Picks, per block, the candidate with the smallest cost; ties keep the earlier candidate, like
 * the strict "<" scans of search_intra_rough (src/search_intra.c:1089-1101).
 * best_mode[i] = modes[argmin_m costs[i*n_modes+m]], best_cost (may be NULL) the minimum. */
UVGHIP_API int uvghip_intra_select_best(const uint32_t *costs, int n, const int8_t *modes, int n_modes,
                             int8_t *best_mode, uint32_t *best_cost, void *stream);

/* ------------------------------------ (2) batched ABI: interpolation ------- */

/* One motion-compensated block: (x,y) = integer sample position of the block's
 * top-left in the reference plane (block position + (mv >> 4), may lie outside
 * the picture: edge replication as uvg_get_extended_block, ipol-generic.c:761),
 * fx,fy = fractional phase (luma: mv & 15, chroma: mv & 31). */
typedef struct uvghip_mc_blk {
  int32_t x, y;
  int32_t fx, fy;
} uvghip_mc_blk_t;

/* replaces: uvg_get_extended_block + uvg_sample_quarterpel_luma(_hi) /
 * uvg_sample_octpel_chroma(_hi) (src/strategies/generic/ipol-generic.c:134-211,
 * 681-758; callers src/inter.c:107-330).  dst: n contiguous blocks of
 * width*height; pixels when hi == 0, int16 14-bit intermediates when hi != 0. */
UVGHIP_API int uvghip_mc_batch(int bitdepth, const void *ref, int ref_stride, int pic_w, int pic_h, int is_chroma,
                    int width, int height, const uvghip_mc_blk_t *blks, int n, int hi, void *dst, void *stream);

/* replaces: uvg_get_extended_block / uvg_get_extended_block_wraparound (ipol-generic.c:761-883; callers inter.c:103-232,
 * search_inter.c:1106, image.c:541) for n blocks of one shape at pos[i] = (blk_x, blk_y): dst[i] = (pad_t + blk_h + pad_b +
 * pad_b_simd) rows of (pad_l + blk_w + pad_r) samples -- rows clamped to the picture, columns edge-replicated
 * (wraparound = 0) or taken modulo the picture width (wraparound = 1, 360-degree content), the pad_b_simd rows zero.
 * A device batch always copies; the "block is inside, hand out a pointer" shortcut belongs to the per-call pointer. */
UVGHIP_API int uvghip_extended_block_batch(int bitdepth, const void *src, int src_stride, int src_w, int src_h, int wraparound,
                                int blk_w, int blk_h, int pad_l, int pad_r, int pad_t, int pad_b, int pad_b_simd,
                                const uvghip_tu_t *pos, int n, void *dst, void *stream);

/* replaces: one or more steps of search_frac (src/search_inter.c:1029-1216):
 * uvg_filter_{hpel,qpel}_blocks_{hor_ver,diag}_luma + uvg_satd_any_size_quad.
 * For block i (cur position / integer-MV reference position in blks[i]) and
 * each of the n_cand displacements cand_mv[2c], cand_mv[2c+1] (1/16 sample
 * units, |mv| <= 15, shared by all blocks):
 *   costs[i*n_cand + c] = SATD(cur block, prediction at ref + mv)
 * which is what the reference obtains from filtered[j] of the step that owns
 * that displacement.  width,height: multiples of 4, <= 64. */
UVGHIP_API int uvghip_frac_satd_batch(int bitdepth, const void *cur, int cur_stride, const void *ref, int ref_stride,
                           int pic_w, int pic_h, int width, int height, const uvghip_blk_t *blks, int n,
                           const int16_t *cand_mv, int n_cand, uint32_t *costs, void *stream);

/* replaces: crc32c_4x4 / crc32c_8x8 (picture-generic.c:1371-1443; the IBC hash): CRC-32C of the size x size block at
 * blks[i] (bytes in raster order; 10-bit samples contribute low byte then high byte), init/final xor 0xFFFFFFFF. */
UVGHIP_API int uvghip_crc32c_batch(int bitdepth, const void *plane, int stride, int size, const uvghip_tu_t *blks, int n,
                        uint32_t *out, void *stream);

/* replaces: pixel_var (picture-generic.c:1334-1357; VAQ): out[i] = variance (double) of the len samples
 * arr[i*len ..].  Floating point: summation order differs from the reference, results agree to ~1e-13 relative. */
UVGHIP_API int uvghip_pixel_var_batch(int bitdepth, const void *arr, uint32_t len, int n, double *out, void *stream);

/* replaces: bipred_average_px_px / _im_im / _px_im (picture-generic.c:1132-1193)
 * on flat arrays of `total` samples.  mode bit0: l0 is int16 14-bit, bit1: l1 is. */
UVGHIP_API int uvghip_bipred_average_batch(int bitdepth, const void *l0, const void *l1, int mode, size_t total,
                                void *dst, void *stream);

/* ------------------------------------------ (2) batched ABI: SAO ----------- */

/* A rectangle of a plane (one CTU, or the part of it the reference hands to SAO). */
typedef struct uvghip_rect {
  int32_t x, y, w, h;
} uvghip_rect_t;

/* replaces: uvg_calc_sao_edge_dir for all four classes + calc_sao_bands
 * (src/strategies/generic/sao-generic.c:51-81, src/sao.c:268-285) for n rectangles:
 *   edge_stats[r][class][0][cat] = sum(orig - rec), [1][cat] = count   (40 int32 per rectangle)
 *   band_stats[r][0][band]       = sum(orig - rec), [1][band] = count  (64 int32 per rectangle)
 * over the rectangle's interior (edge) / whole area (band); neighbours are taken inside the
 * rectangle only, like the reference's packed CTU copies.  uvg_sao_edge_ddistortion and
 * uvg_sao_band_ddistortion are exact functions of these statistics
 * (sum_cat cnt*o^2 - 2*o*sum), so the offset/RD decision needs nothing else from the pixels. */
UVGHIP_API int uvghip_sao_stats_batch(int bitdepth, const void *orig, int orig_stride, const void *rec, int rec_stride,
                           const uvghip_rect_t *rects, int n, int32_t *edge_stats, int32_t *band_stats,
                           void *stream);

/* SAO parameters of one rectangle for ONE colour plane (the host picks the U or V
 * half of sao_info_t.offsets / band_position; src/sao.h:55-63).  type: 0 none, 1 band, 2 edge.
 * offsets[cat] for edge; offsets[1..4] = the four band offsets for band. */
typedef struct uvghip_sao_param {
  int32_t type, eo_class, band_position;
  int32_t offsets[5];
} uvghip_sao_param_t;

/* replaces: uvg_sao_reconstruct -> uvg_sao_reconstruct_color (src/sao.c:302-361,
 * sao-generic.c:84-124): out = SAO(rec) inside each rectangle with its parameters.  Samples SAO does not
 * modify -- type 0 rectangles and the picture's outermost row/column for edge classes (sao.c:321-348) -- are
 * copied from rec, so every sample of every rectangle is written (the reference filters a copy of the picture in
 * place and gets the same picture).  rec and out must be different planes.  The planes may hold several pictures of
 * pic_height rows one under the other (frame-parallel operation): a rectangle's position relative to the picture's top and
 * bottom edge is taken inside its own picture (y mod pic_height). */
UVGHIP_API int uvghip_sao_apply_batch(int bitdepth, const void *rec, int rec_stride, void *out, int out_stride,
                           int pic_w, int pic_h, const uvghip_rect_t *rects,
                           const uvghip_sao_param_t *params, int n, void *stream);

/* replaces: the arithmetic core of sao_search_edge_sao (src/sao.c:380-439): per rectangle and edge
 * class the offsets  (sum + (cnt >> 1)) / cnt  clipped to +-7 with the sign constraint of the
 * category (:400-411), the class's distortion change  sum_cat cnt*o^2 - 2*o*sum  (:421), and the
 * class with the smallest one (strict "<", first wins).  The CABAC rate term mode_bits*lambda
 * (:426-427) depends on the serial entropy-coder state and stays with the host: pass it per
 * (rectangle, class) in rate_cost[n][4] (already (int)(bits*lambda + 0.5)), or NULL for 0.
 * edge_stats as written by uvghip_sao_stats_batch; params_out[i] = {type 2, class, 0, offsets};
 * ddist_out[i] (optional) = the winning sum_ddistortion. */
UVGHIP_API int uvghip_sao_edge_offsets_batch(const int32_t *edge_stats, const int32_t *rate_cost, int n,
                                  uvghip_sao_param_t *params_out, int32_t *ddist_out, void *stream);

/* replaces: uvg_sao_search_lcu (src/sao.c:670-742) for every CTU of n_pictures all-intra pictures of one size -- the whole
 * decision: sao_search_best_mode (:490-603: edge classes, band position, "nothing", the merge candidates), the bit estimates
 * sao_mode_bits_* (:52-178) on the coder's two SAO context models, and those models' adaptation by encode_sao
 * (src/encoderstate.c:523-608) from CTU to CTU in coding order (WPP: a row starts from the models after the first CTU of the
 * row above).  Input: the statistics of uvghip_sao_stats_batch taken with one rectangle per CTU (raster order, pictures one
 * after the other: [picture][ctu]) on the picture uvghip_deblock_frame_sao_snapshot produced, per plane; every distortion the
 * reference measures on samples is an exact function of them.  qp / lambda: state->qp / state->lambda of the (intra) slice;
 * sao_type: cfg.sao_type (1 edge, 2 band, 3 both).
 * Output per CTU: info_out[34] = the reference's two sao_info_t (luma, chroma: type, eo_class, ddistortion, merge_left_flag,
 * merge_up_flag, band_position[2], offsets[10]; entries the reference leaves uninitialised are 0), models_out[6] = the two models
 * (sao_merge_flag, sao_type_idx: state[0], state[1], rate) after the CTU's SAO syntax, and the three uvghip_sao_param_t
 * uvghip_sao_apply_batch takes.  workspace: uvghip_sao_decide_workspace_bytes of device memory. */
UVGHIP_API size_t uvghip_sao_decide_workspace_bytes(int n_pictures, int pic_w, int pic_h);
UVGHIP_API int uvghip_sao_decide_pictures(int bitdepth, int n_pictures, int pic_w, int pic_h, int qp, double lambda, int sao_type,
                                          const int32_t *edge_y, const int32_t *band_y, const int32_t *edge_u, const int32_t *band_u,
                                          const int32_t *edge_v, const int32_t *band_v, void *workspace, int32_t *info_out,
                                          uint16_t *models_out, uvghip_sao_param_t *params_y, uvghip_sao_param_t *params_u,
                                          uvghip_sao_param_t *params_v, void *stream);

/* the same for the pictures of a P / B slice: slice_type 0 B, 1 P, 2 I selects the row of the context initialisation the two SAO models
 * start from (uvg_init_contexts, src/context.c:471-500); qp / lambda are the picture's */
UVGHIP_API int uvghip_sao_decide_pictures_slice(int bitdepth, int n_pictures, int pic_w, int pic_h, int qp, double lambda, int sao_type,
                                                int slice_type, const int32_t *edge_y, const int32_t *band_y, const int32_t *edge_u,
                                                const int32_t *band_u, const int32_t *edge_v, const int32_t *band_v, void *workspace,
                                                int32_t *info_out, uint16_t *models_out, uvghip_sao_param_t *params_y,
                                                uvghip_sao_param_t *params_u, uvghip_sao_param_t *params_v, void *stream);

/* ------------------------------------------ (2) batched ABI: deblocking ---- */

/* Side information of one 4x4 luma block ("SCU"), the subset of cu_info_t
 * (src/cu.h:134-198) that src/filter.c reads, in a fixed 32-byte device layout.
 * One entry per 4x4 block of the picture, row-major, scu_stride entries per row
 * (the reference's cu_array_t, src/cu.h:256-263).  The host-side conversion from
 * cu_info_t is shown in INTEGRATION.md. */
typedef struct uvghip_scu {
  uint8_t luma_edges;          /* cu_info_t.luma_deblocking: bit0 (EDGE_VER=1) left edge, bit1 (EDGE_HOR=2) top edge */
  uint8_t chroma_edges;        /* cu_info_t.chroma_deblocking, same bits; must be a subset of luma_edges (single tree: the
                                * reference only visits chroma where filter_deblock_unit runs for luma, filter.c:1284-1289;
                                * a dual tree's separate chroma cu_array, :1290-1292, is not modelled) */
  uint8_t type;                /* cu_type_t: 1 intra, 2 inter, 4 IBC */
  uint8_t cbf;                 /* bit0 Y, bit1 U, bit2 V (cbf_is_set, src/cu.h:581) */
  int8_t  qp;                  /* cu_info_t.qp */
  uint8_t log2_width, log2_height, log2_chroma_width, log2_chroma_height;
  uint8_t isp_mode;            /* 0 none, 1 horizontal, 2 vertical (src/intra.h:183-185) */
  uint8_t mv_dir;              /* bit0: L0 used, bit1: L1 used */
  uint8_t reserved;
  int16_t ref_id[2];           /* state->frame->ref_LX[l][mv_ref[l]] (filter.c:770-773): only compared for equality */
  int32_t mv[2][2];            /* 1/16-sample motion vectors */
} uvghip_scu_t;

/* replaces: uvg_filter_deblock_lcu called for every CTU of a picture
 * (src/filter.c:1372; caller src/encoderstate.c:842), luma and 4:2:0 chroma, in place.
 * u/v may be NULL (luma only).  width/height: multiples of 4.
 *   beta_offset_div2 / tc_offset_div2 = cfg.deblock_beta / cfg.deblock_tc
 *   slice_is_b  = state->frame->slicetype == UVG_SLICE_B
 *   frame_qp    = state->qp when per-CU QPs are off (max_qp_delta_depth < 0), else -1
 *   chroma_qp_map_host = encoder_control->qp_map[0] (64 entries, HOST pointer) or NULL */
UVGHIP_API int uvghip_deblock_frame(int bitdepth, void *y, int y_stride, void *u, void *v, int c_stride, int width, int height,
                         const uvghip_scu_t *scu, int scu_stride, int beta_offset_div2, int tc_offset_div2,
                         int slice_is_b, int frame_qp, const int8_t *chroma_qp_map_host, void *stream);

/* ------------------------------------------ (2) batched ABI: LFNST --------- */

/* Per-TU parameters of the low-frequency non-separable transform.  intra_mode: the mode the reference
 * resolves before the wide-angle correction (src/transform.c:978-1001: the luma mode; for chroma the
 * chroma mode, the co-located luma mode for CCLM, planar for MIP).  lfnst_idx: 0 = leave the TU alone,
 * 1..2 = kernel.  log2_cu_width/height: the dimensions uvg_wide_angle_correction is called with
 * (:1004-1009: the CU's for luma, the TU's for chroma). */
typedef struct uvghip_lfnst_tu {
  int8_t intra_mode, lfnst_idx, log2_cu_width, log2_cu_height;
} uvghip_lfnst_tu_t;

/* replaces: uvg_fwd_lfnst (inverse = 0, src/transform.c:965-1077) / uvg_inv_lfnst (inverse = 1,
 * :1104-1225) -- plain C in the reference, called between the primary transform and quantisation --
 * for n TUs of one shape, in place on coeffs[n][height][width]. */
UVGHIP_API int uvghip_lfnst_batch(int inverse, int16_t *coeffs, int width, int height, const uvghip_lfnst_tu_t *tus, int n,
                       void *stream);

/* ------------------------------------------ (2) batched ABI: ALF ----------- */

/* replaces: alf_derive_classification -> uvg_alf_derive_classification_blk over the whole luma plane
 * (src/alf.c:5138-5189, src/strategies/generic/alf-generic.c:49-288).  One byte per 4x4 block:
 *   cls[(y/4)*cls_stride + x/4] = class_idx (0..24) | transpose_idx (0..3) << 5
 * (the reference stores the same pair per pixel, alf.h:197-200).  shift = input_bitdepth + 4. */
UVGHIP_API int uvghip_alf_classify_frame(int bitdepth, const void *rec, int rec_stride, int width, int height, int shift,
                              uint8_t *cls, int cls_stride, void *stream);

/* replaces: the CTU loop of alf_reconstruct -> uvg_alf_filter_7x7_blk / uvg_alf_filter_5x5_blk
 * (src/alf.c:5075-5125, alf-generic.c:290-737).  For rectangle i (a CTU): set_idx[i] < 0 -> not filtered (dst
 * untouched), else the filter set to use:
 *   luma   (is_chroma 0): coef_sets/clip_sets = [n_sets][25 classes][13] int16, per-4x4 class/transpose from cls
 *   chroma (is_chroma 1): coef_sets/clip_sets = [n_alternatives][7] int16, cls unused
 * src and dst must be different planes (src = the pre-ALF copy alf_tmp_*).  Rectangles are CTUs or parts of CTUs: at most
 * 64 x 64 samples, x and y multiples of 4 (the classification grid). */
UVGHIP_API int uvghip_alf_filter_batch(int bitdepth, const void *src, int src_stride, void *dst, int dst_stride, int pic_w,
                            int pic_h, int is_chroma, const uvghip_rect_t *rects, const int32_t *set_idx, int n,
                            const int16_t *coef_sets, const int16_t *clip_sets, const uint8_t *cls, int cls_stride,
                            void *stream);

/* replaces: alf_get_blk_stats per CTU (src/alf.c:4227-4330, alf-generic.c:742-999).  For rectangle r (width <= 64,
 * x and width multiples of 4) and class c (luma: 25 classes from cls; chroma: c = 0):
 *   ee[r][c][k][l][b0][b1] (int64, full symmetric 13x13x4x4), y[r][c][k][b] (int32), pix_acc[r][c] (int64; the
 *   reference keeps this integer in a double) -- the fields of alf_covariance (alf.h:176-182).
 * Clipping values are the reference's defaults for the bit depth (alf.c:5248-5260).  Every entry of the three outputs is
 * written exactly once (zeros for classes without a block in the rectangle): the buffers need no initialisation. */
UVGHIP_API int uvghip_alf_stats_batch(int bitdepth, const void *org, int org_stride, const void *rec, int rec_stride, int pic_w,
                           int pic_h, int is_chroma, const uvghip_rect_t *rects, int n, const uint8_t *cls,
                           int cls_stride, int64_t *ee, int32_t *y, int64_t *pix_acc, void *stream);

/* uvghip_alf_stats_batch with a compact output: the covariances are symmetric (ee[k][l][b0][b1] == ee[l][k][b1][b0];
 * the reference symmetrises after the fact, alf-generic.c:984-997) and most of the 25 classes are absent from any one
 * CTU, so only the classes PRESENT in a rectangle are written, and of ee only the pairs k <= l:
 *   present[r]                       bit c set = class c occurs in rectangle r
 *   records[(r * ncls + s)]          the s-th present class of r (increasing class order); ncls = 25 luma / 1 chroma;
 *                                    slots s >= popcount(present[r]) are left untouched
 * one record = UVGHIP_ALF_REC_WORDS int64:
 *   [ (k*13 - k*(k-1)/2 + l-k) * 16 + b0*4 + b1 ]  ee[k][l][b0][b1], k <= l < 13      (91 * 16 words)
 *   [1456 .. 1481] as int32[52]                     y[k][b]
 *   [1482]                                          pix_acc;   [1483] zero
 * i.e. 11.9 KB per present class instead of 21.9 KB for each of the 25. */
#define UVGHIP_ALF_REC_WORDS 1484
UVGHIP_API int uvghip_alf_stats_compact_batch(int bitdepth, const void *org, int org_stride, const void *rec, int rec_stride,
                                   int pic_w, int pic_h, int is_chroma, const uvghip_rect_t *rects, int n,
                                   const uint8_t *cls, int cls_stride, int64_t *records, uint32_t *present, void *stream);

/* Compact records -> the full per-class layout uvghip_alf_stats_batch writes (zeros for absent classes). */
UVGHIP_API int uvghip_alf_cov_expand(const int64_t *records, const uint32_t *present, int n, int is_chroma, int64_t *ee,
                          int32_t *y, int64_t *pix_acc, void *stream);

/* replaces: the accumulation of the CTU covariances into the frame covariances the filters are derived from
 * (src/alf.c:792-835).  sums[c] = UVGHIP_ALF_SUM_WORDS int64 per class: the ee triangle as in a record (1456 words), then
 * y[52] widened to int64, then pix_acc.  In a multi-GPU run every rank reduces its own CTUs and the ranks' sums meet
 * in uvghip_comm_allreduce_i64. */
#define UVGHIP_ALF_SUM_WORDS 1509
UVGHIP_API int uvghip_alf_cov_reduce(const int64_t *records, const uint32_t *present, int n, int is_chroma, int64_t *sums,
                          void *stream);

/* replaces: apply_cc_alf_filter -> filter_blk_cc_alf over the CTUs of one chroma plane (src/alf.c:1726-1775, 1626-1725; 4:2:0).
 * rects: the CTUs' chroma rectangles; filter_idx[i] < 0 -> rectangle i untouched (cc_alf_filter_control 0), else the filter
 * control - 1 into coef[4][8] (int16, seven taps used).  luma: the picture BEFORE ALF (the reference reads alf_tmp_y), pic_w / pic_h
 * its size; chroma: the plane after the chroma ALF, filtered in place. */
UVGHIP_API int uvghip_cc_alf_filter_batch(int bitdepth, const void *luma, int luma_stride, void *chroma, int chroma_stride, int pic_w,
                               int pic_h, const uvghip_rect_t *rects, const int32_t *filter_idx, int n, const int16_t *coef,
                               void *stream);

/* replaces: get_blk_stats_cc_alf per CTU (src/alf.c:2613-2779, called from derive_stats_for_cc_alf_filtering :2780; 4:2:0) for one chroma
 * plane.  For rectangle r (a CTU's chroma rectangle: <= 32 x 32, y a multiple of 32): ee[r][7][7] (int64, full symmetric: the fields
 * ee[k][l][0][0] of alf_covariance), y[r][7] (int32: y[k][0]), pix_acc[r] (int64; the reference keeps this integer in a double).
 * org / rec: the source chroma plane and the chroma plane AFTER its ALF (alf_tmp_u / _v at that point); luma: the picture BEFORE ALF
 * (alf_tmp_y), pic_w / pic_h its size.  Every entry of the three outputs is written. */
UVGHIP_API int uvghip_cc_alf_stats_batch(int bitdepth, const void *org, int org_stride, const void *rec, int rec_stride, const void *luma,
                              int luma_stride, int pic_w, int pic_h, const uvghip_rect_t *rects, int n, int64_t *ee, int32_t *y,
                              int64_t *pix_acc, void *stream);

/* replaces: alf_reconstruct_coeff_aps / alf_reconstruct_coeff (src/alf.c:4332-4368, 2925-2986, is_rdo = 0) and the fixed filter
 * sets and clipping values uvg_alf_enc_process prepares (:5244-5279).  HOST function, no device involved.
 *   luma_aps[n_luma_aps][UVGHIP_ALF_LUMA_APS_WORDS] int16: luma_coeff[25][13], luma_clipp[25][13] (clip indices), filter_coeff_delta_idx[25],
 *     num_luma_filters, non_linear_flag -- the fields of alf_aps (alf.h:213-232) as coded;
 *   chroma_aps[UVGHIP_ALF_CHROMA_APS_WORDS] int16 (may be NULL with the chroma outputs): chroma_coeff[8][7], chroma_clipp[8][7], num_alternatives, non_linear_flag.
 * -> luma_coef / luma_clip [24][25][13]: sets 0..15 the fixed filter sets, 16 + i APS i (unused APSs zero); chroma_coef / chroma_clip [8][7]:
 *    what uvghip_alf_filter_batch takes as coef_sets / clip_sets. */
#define UVGHIP_ALF_LUMA_APS_WORDS 677
#define UVGHIP_ALF_CHROMA_APS_WORDS 114
UVGHIP_API int uvghip_alf_expand_tables(int bitdepth, int n_luma_aps, const int16_t *luma_aps, const int16_t *chroma_aps, int16_t *luma_coef,
                             int16_t *luma_clip, int16_t *chroma_coef, int16_t *chroma_clip);

/* replaces: alf_reconstruct + the CC-ALF tail of uvg_alf_enc_process (src/alf.c:5032-5137, 5363-5440) for one picture, given
 * the decisions the encoder's derivation took (alf_encoder, alf_encoder_ctb, derive_cc_alf_filter stay host work upstream):
 * out = the picture ALF leaves.  Planes are device memory, the decisions host memory (read before the call returns).
 *   slice_enabled[3]            tile_group_alf_enabled_flag (Y off: nothing is filtered, alf.c:5035)
 *   ctu_flags[7][n_ctus] u8     per CTU in raster order: ctu_enable_flag Y / Cb / Cr, ctu_alternative Cb / Cr, cc_alf_filter_control Cb / Cr
 *   filter_set_idx[n_ctus]      alf_ctb_filter_index: < 16 a fixed filter set, else 16 + index into the slice's luma APS list
 *   luma_aps / chroma_aps       as for uvghip_alf_expand_tables (the APSs the slice refers to, in tile_group_luma_aps_id order)
 *   alf_full, cc_alf_enabled[2], cc_coeff[2][4][8]   CC-ALF (cfg.alf_type == UVG_ALF_FULL): cc_alf_filter_enabled, cc_alf_coeff
 *   classification_shift        cfg.input_bitdepth + 4 (alf.c:5185: the depth of the INPUT, not the encoder's)
 * width / height multiples of 8.  CC-ALF without luma ALF is refused (the reference reads a buffer it never filled, alf.c:5066). */
typedef struct uvghip_alf_picture {
  const void *in_y, *in_u, *in_v; int32_t in_stride, in_stride_c;
  void *out_y, *out_u, *out_v; int32_t out_stride, out_stride_c;
  int32_t width, height;
  int32_t slice_enabled[3];
  int32_t n_luma_aps;
  const uint8_t *ctu_flags;
  const int16_t *filter_set_idx;
  const int16_t *luma_aps, *chroma_aps;
  int32_t alf_full, cc_alf_enabled[2];
  const int16_t *cc_coeff;
  int32_t classification_shift;
} uvghip_alf_picture_t;
UVGHIP_API size_t uvghip_alf_reconstruct_workspace_bytes(int pic_w, int pic_h);
UVGHIP_API int uvghip_alf_reconstruct_picture(int bitdepth, const uvghip_alf_picture_t *picture, void *workspace, void *stream);

/* ------------------------------- (2) batched ABI: CTU-row bands (multi-GPU) ---- */

/* One picture sharded over the GPUs of a node by contiguous CTU rows (the reference's own row
 * parallelism: one job per CTU row, src/encoderstate.c:1085-1189).  Every rank keeps full-size planes and fills / filters
 * only the rows it owns plus the halo rows it received, so every kernel keeps picture coordinates and its
 * picture-border behaviour.  Halo rows a band needs from its neighbours (luma rows; chroma = half):
 *   deblocking   a horizontal edge on a band boundary is filtered by BOTH neighbours, each into its own copy.  At a
 *                CTU boundary the P (upper) side reads 4 rows and the Q (lower) side 8 (src/filter.c:611-619,908-973
 *                with the CTB-boundary shortening :224-226), after the vertical-edge pass; plus one row of
 *                uvghip_scu_t on either side for Bs / QP / transform sizes.  The rows SAO reads across the boundary
 *                (+-1) come out of this redundant filtering already final.
 *   ALF          3 rows of SAO output either side (7x7 diamond and 8x8 Laplacian window, both clamped at the
 *                virtual boundary 4 rows above the CTU boundary, src/alf.h:32-33); 4 are exchanged. */
#define UVGHIP_HALO_DBK_P 4
#define UVGHIP_HALO_DBK_Q 8
#define UVGHIP_HALO_ALF   4

typedef struct uvghip_band_plan {
  int32_t rank, nranks;
  int32_t ctu_rows;             /* CTU rows of the picture */
  int32_t ctu_row0, ctu_row1;   /* this rank owns CTU rows [ctu_row0, ctu_row1): balanced, the first ctu_rows % nranks ranks get one more */
  int32_t y0, y1;               /* = luma rows [y0, y1) (y1 clipped to the picture) */
  int32_t up, down;             /* neighbour ranks, -1 at the picture border */
} uvghip_band_plan_t;

/* Host only, no device.  Fails when nranks exceeds the number of CTU rows. */
UVGHIP_API int uvghip_band_plan(int pic_h, int nranks, int rank, uvghip_band_plan_t *out);

/* uvghip_deblock_frame restricted to a band (rows multiples of 4).  passes bit 0: the vertical edges of rows
 * [row0, row1); bit 1: the horizontal edges at y = row0 .. row1, INCLUDING y = row1 when that is not the picture's
 * bottom -- both owners of a boundary edge filter it.  The horizontal pass of a band needs the vertical pass of the
 * rows [row0 - UVGHIP_HALO_DBK_P, row1 + UVGHIP_HALO_DBK_Q) to have completed (own rows + received halos). */
UVGHIP_API int uvghip_deblock_band(int bitdepth, void *y, int y_stride, void *u, void *v, int c_stride, int width, int height,
                        const uvghip_scu_t *scu, int scu_stride, int beta_offset_div2, int tc_offset_div2,
                        int slice_is_b, int frame_qp, const int8_t *chroma_qp_map_host, int row0, int row1, int passes,
                        void *stream);

/* The picture as uvg_sao_search_lcu sees it (src/sao.c:641-668, called at src/encoderstate.c:849 right after the CTU's own
 * uvg_filter_deblock_lcu): every CTU deblocked by its OWN edges only.  Same arguments and in-place operation as
 * uvghip_deblock_frame, but an edge on a CTU boundary does not write into the CTU before it (that CTU took its SAO statistics
 * before this edge was filtered, filter.c:1372-1380) and horizontal edges skip the last 8 luma columns of every CTU that is not
 * the last of its row (filter.c:1224-1238: they wait for the next CTU).  Every sample of the result is the value the
 * reference's SAO decision of the CTU containing it reads; run uvghip_sao_stats_batch on it, uvghip_sao_apply_batch on the
 * picture uvghip_deblock_frame produces from the same input. */
UVGHIP_API int uvghip_deblock_frame_sao_snapshot(int bitdepth, void *y, int y_stride, void *u, void *v, int c_stride, int width,
                                                 int height, const uvghip_scu_t *scu, int scu_stride, int beta_offset_div2,
                                                 int tc_offset_div2, int slice_is_b, int frame_qp, const int8_t *chroma_qp_map_host,
                                                 void *stream);

/* uvghip_alf_classify_frame for the 4x4 blocks of rows [row0, row1). */
UVGHIP_API int uvghip_alf_classify_band(int bitdepth, const void *rec, int rec_stride, int width, int height, int shift,
                             uint8_t *cls, int cls_stride, int row0, int row1, void *stream);

/* ---- data-path exchanges between the ranks: RCCL over xGMI, issued on the caller's stream ---- */
#define UVGHIP_COMM_ID_BYTES 128
/* rank 0: ncclGetUniqueId into a HOST buffer of UVGHIP_COMM_ID_BYTES; the host distributes it to the other ranks
 * (any out-of-band channel: the launcher's store, MPI, a file). */
UVGHIP_API int uvghip_comm_unique_id(void *id_host);
/* every rank, after uvghip_init on its own device: ncclCommInitRank. */
UVGHIP_API int uvghip_comm_create(const void *id_host, int nranks, int rank, void **comm_out);
UVGHIP_API int uvghip_comm_destroy(void *comm);

/* One pairwise transfer: send_bytes from `send` to `peer` and/or recv_bytes from `peer` into `recv` (device pointers). */
typedef struct uvghip_xfer {
  int32_t peer, reserved;
  const void *send; uint64_t send_bytes;
  void *recv;       uint64_t recv_bytes;
} uvghip_xfer_t;
/* ncclGroupStart; ncclSend / ncclRecv for every entry; ncclGroupEnd -- the halo exchange (two neighbours) and the
 * all-to-all distribution of reconstructed bands (uneven sizes) are both lists of these.  xfers_host: HOST array. */
UVGHIP_API int uvghip_comm_exchange(void *comm, const uvghip_xfer_t *xfers_host, int n, void *stream);
/* ncclAllReduce(sum, int64) in place: the frame-level ALF covariances (src/alf.c:792-835 sums them over the CTUs). */
UVGHIP_API int uvghip_comm_allreduce_i64(void *comm, int64_t *buf, size_t count, void *stream);
/* ncclAllGather of equal-sized contributions (bytes_per_rank each). */
UVGHIP_API int uvghip_comm_allgather(void *comm, const void *send, void *recv, size_t bytes_per_rank, void *stream);

/* ------------- (3) per-call entry points behind plain-value views (state-taking strategies) ------------- */

/* The reference typedefs of quant / dequant / quantize_residual (strategies-quant.h:48-86) and inter_recon_bipred
 * (strategies-picture.h:136-148) take encoder_state_t* / cu_info_t* / lcu_t*: encoder-private structs whose layout
 * depends on the encoder's compile options.  The typedef-exact functions therefore live in a shim compiled in the encoder
 * tree (uvg266_amd/csrc/shim/strategies-hip-state.c) that does nothing but copy the fields
 * below out of those structs; everything else is behind these functions.  HOST buffers in and out, synchronous,
 * re-entrant from any number of threads (each thread owns a stream and a staging arena). */
typedef struct uvghip_state_view {
  int32_t bitdepth;                 /* encoder_control->bitdepth */
  int32_t qp;                       /* state->qp */
  int32_t slice_is_intra;           /* state->frame->slicetype == UVG_SLICE_I */
  int32_t rdoq_enable, rdoq_skip;   /* cfg.rdoq_enable, cfg.rdoq_skip */
  int32_t dep_quant, signhide_enable, scaling_list_enabled;   /* cfg.dep_quant, cfg.signhide_enable, scaling_list.enable:
                                                               * dep_quant and scaling lists must be 0 (the shim checks) */
  int32_t lfnst, mts;               /* cfg.lfnst, cfg.mts (enum uvg_mts) */
  int32_t lmcs_chroma_adj_enabled;  /* lmcs_aps->m_sliceReshapeInfo.enableChromaAdj: must be 0 for chroma calls */
  int32_t collocated_luma_mode;     /* state->collocated_luma_mode (LFNST of a CCLM chroma block) */
  int32_t jccr_sign, reserved;      /* state->frame->jccr_sign (joint Cb-Cr coding) */
  double lambda, c_lambda;          /* state->lambda, state->c_lambda */
  int8_t qp_map[64];                /* encoder_control->qp_map[0] */
  uvghip_rdoq_ctx_t cabac;          /* CTX_STATE of state->cabac.ctx's models (RDOQ only) */
} uvghip_state_view_t;

typedef struct uvghip_cu_view {     /* cu_info_t (src/cu.h:134-198), the fields uvg_quantize_residual's callees read */
  int8_t type;                      /* cu_type_t: 1 intra, 2 inter */
  int8_t tr_idx, lfnst_idx, cr_lfnst_idx;
  int8_t log2_width, log2_height;
  int8_t intra_mode, intra_mode_chroma, mip_flag, isp_mode;   /* intra.* (read only when type == 1) */
  uint16_t cbf;
  int8_t joint_cb_cr, reserved[3];
} uvghip_cu_view_t;

/* uvg_quant (quant-generic.c:51-232) / uvg_dequant (:618-669) for one block. */
UVGHIP_API unsigned uvghip_quant_percall(const uvghip_state_view_t *sv, const int16_t *coef, int16_t *q_coef, int32_t width,
                                         int32_t height, int color, int scan_idx, int block_type, int transform_skip,
                                         int lfnst_idx);
UVGHIP_API unsigned uvghip_dequant_percall(const uvghip_state_view_t *sv, const int16_t *q_coef, int16_t *coef, int32_t width,
                                           int32_t height, int color, int block_type, int transform_skip);
/* uvg_quantize_residual (quant-generic.c:460-612) for one TU: returns has_coeffs, writes coeff_out (width*height) and
 * rec_out (reconstruction, or the prediction when nothing was coded / early_skip).  tree_type: enum uvg_tree_type. */
UVGHIP_API int uvghip_quantize_residual_percall(const uvghip_state_view_t *sv, const uvghip_cu_view_t *cu, int width, int height,
                                                int color, int scan_order, int use_trskip, int in_stride, int out_stride,
                                                const void *ref_in, const void *pred_in, void *rec_out, int16_t *coeff_out,
                                                int early_skip, int lmcs_chroma_adj, int tree_type);
/* uvg_quant_cbcr_residual (quant-generic.c:241-442) for one chroma TU pair: returns joint_cb_cr if coefficients were coded, else 0. */
UVGHIP_API int uvghip_quant_cbcr_residual_percall(const uvghip_state_view_t *sv, const uvghip_cu_view_t *cu, int width, int height,
                                                  int scan_order, int in_stride, int out_stride, const void *u_ref_in,
                                                  const void *v_ref_in, const void *u_pred_in, const void *v_pred_in, void *u_rec_out,
                                                  void *v_rec_out, int16_t *coeff_out, int early_skip, int lmcs_chroma_adj, int tree_type);
/* One plane of bipred_average_generic (picture-generic.c:1195-1262): dst rows of pu_w samples at dst_stride; l0 / l1 are
 * pu_w*pu_h contiguous samples -- pixels, or 14-bit int16 intermediates where *_is_im. */
/* The `alf` strategy group behind plain values (strategies-alf.h:48-109; csrc/alf_percall.hip): what the shim's four typedef-exact
 * functions call.  Host planes in (whole planes of pic_w x pic_h, stride in samples), host results out.
 *   classify: cls_out[h / 4][w / 4] = class_idx | transpose_idx << 5 of the 4x4 blocks of [x, x + w) x [y, y + h)
 *   filter:   one filter set (luma: coef / clip [25][13] + the plane's class bytes `cls`; chroma: [7], cls NULL) over the block -> dst_block[h][w]
 *   stats:    the block's own sums in uvghip_alf_stats_batch's layout, ee[ncls][13][13][4][4] / yv[ncls][13][4] / pix_acc[ncls] (ncls 25 / 1) */
UVGHIP_API int uvghip_alf_classify_percall(int bitdepth, const void *rec, int rec_stride, int pic_w, int pic_h, int shift, int x, int y, int w, int h, uint8_t *cls_out);
UVGHIP_API int uvghip_alf_filter_percall(int bitdepth, int is_chroma, const void *src, int src_stride, int pic_w, int pic_h, int x, int y, int w, int h,
                                         const int16_t *coef, const int16_t *clip, const uint8_t *cls, int cls_stride, void *dst_block);
UVGHIP_API int uvghip_alf_stats_percall(int bitdepth, int is_chroma, const void *org, int org_stride, const void *rec, int rec_stride, int pic_w, int pic_h, int x, int y,
                                        int w, int h, const uint8_t *cls, int cls_stride, int64_t *ee, int32_t *yv, int64_t *pix_acc);
UVGHIP_API void uvghip_bipred_average_percall(int bitdepth, void *dst, int dst_stride, const void *l0, int l0_is_im,
                                              const void *l1, int l1_is_im, unsigned pu_w, unsigned pu_h);

/* ------------------- (4) closed-loop intra search of whole pictures: the CALLER of the block kernels, on the device ---- */

/* replaces: encoder_state_worker_encode_lcu_search's uvg_search_lcu (src/encoderstate.c:808 -> src/search.c:2384-2479:
 * search_cu's split / mode RD decisions, uvg_search_cu_intra's rough search, uvg_intra_recon_cu, uvg_rdoq, the bit costs of
 * uvg_mock_encode_coding_unit / uvg_get_coeff_cost on state->search_cabac) for every CTU of n all-intra pictures, followed per CTU
 * by the model adaptation of the real coder (uvg_encode_coding_tree, src/encoderstate.c:888) so that the next CTU -- and, under
 * WPP, the first CTU of the next row (encoderstate.c:966-975) -- starts from the models the reference would hand it.
 * One workgroup per CTU; CTUs of a picture are released along the WPP wavefront (left and upper neighbour done,
 * encoderstate.c:1160-1167) through flags in device memory, pictures are independent (-p 1) and fill the device together.
 * Configuration: what --preset medium -p 1 enables (rd 0, rdoq, pu-depth-intra min..max, quad-tree splits only, WPP,
 * cu-split-termination zero, combine-intra-cus); anything else is refused.  Bit-exact with the reference: tests/golden/ref_ctu*.
 *
 * What the search reads from encoder_state_t / encoder_control_t: */
typedef struct uvghip_ctu_params {
  int32_t pic_w, pic_h;          /* multiples of 8 */
  int32_t qp;                    /* state->qp */
  int32_t qp_c;                  /* encoder_control->qp_map[0][qp] */
  int32_t depth_min, depth_max;  /* cfg.pu_depth_intra: 1 <= min <= max <= 4; min > 1 only with combine_intra_cus = 0 (the reference combines at every depth
                                  * without a search, search.c:2082-2143; the kernel at depth 0 only) */
  int32_t wpp;                   /* cfg.wpp: must be 1 */
  int32_t combine_intra_cus;     /* cfg.combine_intra_cus */
  int32_t rough_levels;          /* cfg.intra_rough_search_levels: 2 or 3 */
  int32_t rd;                    /* cfg.rdo: 0 (--preset medium and faster) or 1 (--preset slow).  The two differ in ONE decision: with rd 0 a CU of
                                  * a P / B picture whose inter cost per sample is below INTRA_THRESHOLD skips its intra search (search.c:1413-1419);
                                  * I pictures are searched the same way.  rd >= 2 (full RD of several intra modes, of the merge / AMVP candidates)
                                  * is refused by uvghip_ctu_search_pb. */
  double lambda, lambda_sqrt;    /* state->lambda, state->lambda_sqrt */
  double c_lambda;               /* state->c_lambda */
  double chroma_weight_u, chroma_weight_v;   /* state->chroma_weights[1], [2] */
  double c_lambda_tu;            /* uvg_calculate_chroma_lambda(state, 0, 0) (src/rate_control.c:1216): lambda / 2^((qp - qp_c) / 3) */
} uvghip_ctu_params_t;

/* One picture, everything in device memory.  src: the source planes.  rec: the reconstruction BEFORE the in-loop filters
 * (frame->rec as copy_lcu_to_cu_data leaves it, search.c:2331).  cu: the picture's side information, one uvghip_scu_t per 4x4
 * (frame->cu_array) with, for intra CUs, mv[0][0] = intra mode | chroma mode << 8, mv[0][1] = cu_info_t.split_tree,
 * mv[1][0] = cu_info_t.mode_type_tree; cu_stride = 16 * CTUs per row.  coeff: per CTU an lcu_coeff_t (src/cu.h: y[64*64],
 * u[32*32], v[32*32] levels, raster inside the CTU) -- with cu the hand-over to the bitstream coder (encoderstate.c:863-976).
 * models: per CTU three sets of UVGHIP_CTU_MODELS context models (state[0] | state[1] << 16) -- at the CTU's start, at the end of
 * its search (state->search_cabac), after the real coder (state->cabac); the model order is that of csrc/ctu_core.h. */
#define UVGHIP_CTU_MODELS 257
typedef struct uvghip_ctu_picture {
  const void *src_y, *src_u, *src_v;
  int32_t src_stride, src_stride_c;     /* in samples */
  void *rec_y, *rec_u, *rec_v;
  int32_t rec_stride, rec_stride_c;
  uvghip_scu_t *cu;
  int32_t cu_stride, reserved;
  int16_t *coeff;
  uint32_t *models;
} uvghip_ctu_picture_t;

UVGHIP_API size_t uvghip_ctu_search_workspace_bytes(int n_pictures, int pic_w, int pic_h);
/* A plan binds a configuration, n picture descriptors (HOST array) and a workspace (device memory of the size above, owned by
 * the caller, in use until the plan is destroyed): the release order of the CTUs and the picture table are uploaded once.
 * uvghip_ctu_plan_run enqueues the search of all n pictures on `stream` (a memset of the counters + one launch; the host does not
 * wait) -- this is what an encoder calls once per group of pictures where the reference queues its per-CTU search jobs
 * (encoderstate.c:1130-1200); plans on different streams run side by side.  A plan may be run any number of times (new source
 * samples in the same buffers), one run at a time. */
typedef struct uvghip_ctu_plan uvghip_ctu_plan_t;
UVGHIP_API int uvghip_ctu_plan_create(int bitdepth, const uvghip_ctu_params_t *params, const uvghip_ctu_picture_t *pictures,
                                      int n_pictures, void *workspace, uvghip_ctu_plan_t **plan_out);
/* The same for a band of CTU rows [ctu_row0, ctu_row1) of every picture -- one picture sharded over the GPUs of a node by CTU rows
 * (the reference's one job per CTU row with the dependency on the row above, src/encoderstate.c:1085-1189).  The row
 * above the band is taken as complete: before the run the caller puts what a CTU row reads of it into the pictures' buffers -- its last
 * line of rec_y / rec_u / rec_v (hor_buf_search), its last row of `cu` (4x4 units) and the third model set of its FIRST CTU (the WPP
 * context hand-over, encoderstate.c:966-975): the halo the band above sends down (uvg266_amd/bands.py::BandLayout.halo_search).  The
 * band's rows come out bit-identical to the same rows of a whole-picture run (tests/test_gpu_search_bands.py). */
UVGHIP_API int uvghip_ctu_plan_create_rows(int bitdepth, const uvghip_ctu_params_t *params, const uvghip_ctu_picture_t *pictures,
                                           int n_pictures, int ctu_row0, int ctu_row1, void *workspace, uvghip_ctu_plan_t **plan_out);
UVGHIP_API int uvghip_ctu_plan_run(uvghip_ctu_plan_t *plan, void *stream);
UVGHIP_API void uvghip_ctu_plan_destroy(uvghip_ctu_plan_t *plan);
/* One-shot form: plan + run + wait for the stream + destroy. */
UVGHIP_API int uvghip_ctu_search_intra(int bitdepth, const uvghip_ctu_params_t *params, const uvghip_ctu_picture_t *pictures,
                                       int n_pictures, void *workspace, void *stream);

/* ------------------- (5) the per-picture loop of the CTU worker as one call per group of pictures ---------------------- */

/* replaces, for all-intra pictures: encoder_state_worker_encode_lcu_search for every CTU (src/encoderstate.c:808-976 minus the
 * bitstream writer) and the frame's SAO reconstruction (:256-343) -- uvghip_ctu_plan_run, then ONE launch of the per-CTU filter stage
 * over all pictures (what encoder_state_worker_encode_lcu_search does after uvg_search_lcu, encoderstate.c:841-853: deblocking,
 * uvg_sao_search_lcu's statistics and decision, encoder_sao_reconstruct), then one launch of the arithmetic coder.
 * A picture: the search's descriptor (outputs as described there) + where the filtered picture goes.  search.rec_* stay unfiltered; the
 * deblocked pictures live in the workspace; out_* receive the picture uvg_encoder_encode returns (after SAO) / the next picture's
 * reference.  Everything on `stream`, nothing waits.
 * sao_type: cfg.sao_type.  workspace: uvghip_loop_workspace_bytes of device memory, in use until the plan is destroyed.
 * uvghip_loop_plan_results: device pointers to the decisions ([picture][ctu][34] int32, the reference's two sao_info_t) and the
 * two SAO context models after every CTU's SAO syntax ([picture][ctu][6] uint16) -- what encode_sao codes. */
typedef struct uvghip_loop_picture {
  uvghip_ctu_picture_t search;
  void *out_y, *out_u, *out_v;
  int32_t out_stride, out_stride_c;     /* in samples */
} uvghip_loop_picture_t;
typedef struct uvghip_loop_plan uvghip_loop_plan_t;
UVGHIP_API size_t uvghip_loop_workspace_bytes(int bitdepth, int n_pictures, int pic_w, int pic_h);
UVGHIP_API int uvghip_loop_plan_create(int bitdepth, const uvghip_ctu_params_t *params, const uvghip_loop_picture_t *pictures,
                                       int n_pictures, int sao_type, void *workspace, uvghip_loop_plan_t **plan_out);
UVGHIP_API int uvghip_loop_plan_run(uvghip_loop_plan_t *plan, void *stream);
/* The same results with the three launches BESIDE each other instead of one after the other (the latency of ONE group: a clip, a picture):
 * the search on `stream`, the filter stage on a stream of the plan's own behind the search's per-CTU "searched" flags, the coder on
 * another behind the filter stage's per-CTU "final" flags -- a CTU is
 * filtered when it is searched and coded when it is filtered, as encoder_state_worker_encode_lcu_search / _bitstream do CTU by CTU
 * (src/encoderstate.c:808-939), and the group's tail is one CTU's filter + its row's last bins instead of the whole filter and coder
 * launches.  Forked from and joined to `stream`.  What runs beside the search is capped (128 persistent filter workgroups, 256 persistent
 * coder waves that take row r of every picture, then row r + 1), because a waiting
 * workgroup holds LDS the search cannot use.  For the latency of ONE small group: when the pictures' wavefronts can have more than 512 CTUs in
 * progress (half the device's workgroup slots: more than 30 pictures of 1080p) the call IS uvghip_loop_plan_run -- beside a search that fills
 * the device the overlap costs more search slots than the tail it hides (measured), and with several groups in flight
 * (bench.py's judged line) launches overlap across groups anyway. */
UVGHIP_API int uvghip_loop_plan_run_overlapped(uvghip_loop_plan_t *plan, void *stream);
/* The two halves of uvghip_loop_plan_run on their own (a caller that wants events or other work between them). */
UVGHIP_API int uvghip_loop_plan_run_search(uvghip_loop_plan_t *plan, void *stream);
UVGHIP_API int uvghip_loop_plan_run_filters(uvghip_loop_plan_t *plan, void *stream);
UVGHIP_API int uvghip_loop_plan_results(const uvghip_loop_plan_t *plan, const int32_t **sao_info, const uint16_t **sao_models);
/* The plan also codes the slice data (uvghip_encode_slice_rows, section 6) as the last thing of a run: device pointers to the rows'
 * bytes (row r of picture p at rows + (p * n_rows + r) * row_cap) and their lengths ([picture][row]). */
UVGHIP_API int uvghip_loop_plan_slice_data(const uvghip_loop_plan_t *plan, const uint8_t **rows, const int32_t **row_bytes, int *row_cap,
                                           int *n_rows);

/* The loop plan of a BAND of CTU rows [ctu_row0, ctu_row1) of every picture: one picture sharded over the GPUs of a node by CTU rows
 * with the closed loop whole -- search (uvghip_ctu_plan_create_rows), filter stage and coder over the band's rows only.  The hand-over
 * goes ONE way: the per-CTU filter stage pulls (a CTU builds its tile from the unfiltered reconstruction of itself and its left, upper
 * and upper-left neighbour and writes only up and left of its lower right corner), the SAO decision chains from the left and from the
 * first CTU of the row above, and every WPP row's substream starts from the models behind the first CTU of the row above -- so a band
 * reads of the band ABOVE and of nothing below.  The band's rows of every output come out as the whole-picture plan gives them
 * (tests/test_gpu_loop_bands.py: against the reference encoder's records).
 * uvghip_loop_plan_create is the call with (0, CTU rows of the picture) and sao_type 1..3; this call also takes sao_type 0 (no SAO:
 * out = the deblocked picture, no SAO syntax in the rows).  Same workspace size, same accessors; uvghip_loop_plan_slice_data keeps
 * its layout (row r of a picture at its usual place; rows outside the band are not written).  uvghip_loop_plan_run, _run_search and
 * _run_filters work on a band plan; uvghip_loop_plan_run_overlapped on a band plan IS uvghip_loop_plan_run.  The filter launch knows
 * the band's first row: no CTU waits for a flag of a row outside the band.
 *
 * The hand-over.  Before a run of a band with ctu_row0 > 0 the caller puts into the plan's buffers what the band's three launches read
 * of the band above; after the run of a band with ctu_row1 < CTU rows it takes the same pieces out of that band's buffers.
 * uvghip_loop_plan_halo lists them for all pictures -- side 0: received from above, side 1: sent down -- as (device pointer, bytes per
 * row, rows, pitch in bytes); cap < the number of pieces is an error, *n reports the need either way.  The list goes kind after kind,
 * inside a kind picture after picture.  The kinds, with Y = 64 * the boundary's CTU row, b = bytes per sample, wc = CTUs per row:
 *   rec_y rows [Y - 16, Y), rec_u / rec_v rows [Y / 2 - 8, Y / 2): the unfiltered reconstruction the first row's tiles start in (the
 *     search's single line is the last of them);
 *   cu rows [Y / 4 - 4, Y / 4) of wc * 16 units: the tiles' edges and filter strengths, the search's and the coder's contexts;
 *   with SAO: the deblocked picture (in the workspace) luma rows [Y - 11, Y - 8), chroma rows [Y / 2 - 6, Y / 2 - 4): what the first
 *     row's part of the output picture reads above the band's own deblocked rows (10 rows of SAO delay, one more for the edge classes);
 *   with SAO: the decisions of the whole CTU row above (wc * 34 int32): merge candidates, and the offsets of the 10 output rows above;
 *   the third model set of the FIRST CTU of the row above (UVGHIP_CTU_MODELS uint32): the WPP hand-over of search and coder;
 *   with SAO: the SAO models behind that CTU (6 uint16).
 * uvghip_loop_plan_halo_bytes: the size of ONE packed message = n_pictures * (b * 24 * pic_w + 2048 * wc + 4 * UVGHIP_CTU_MODELS +
 * (sao_type ? b * 5 * pic_w + 136 * wc + 12 : 0)) -- the pieces' bytes, nothing else; 0 for a plan of the whole picture.  The message
 * holds piece kind after piece kind in the order above, inside a kind picture after picture, rows tightly packed: its layout depends on
 * (bitdepth, n_pictures, pic_w, sao_type) only, not on strides, so two bands whose planes are padded differently agree.
 * uvghip_loop_plan_halo_pack gathers the side 1 pieces of all pictures into `message` (device memory) in ONE launch,
 * uvghip_loop_plan_halo_unpack scatters a message into the side 0 pieces: a boundary costs one send and one receive per group.
 * uvghip_loop_plan_out_rows: the luma rows [*y0, *y1) of the output pictures the band writes: [ctu_row0 ? 64 ctu_row0 - delay : 0,
 * last band ? pic_h : 64 ctu_row1 - delay), delay = 10 (8 with sao_type 0).  The bands' rectangles tile the picture, so their
 * uvghip_picture_checksum_rect terms add up to the picture's checksum. */
typedef struct uvghip_halo_piece {
  void *ptr;                 /* DEVICE: the piece's first row */
  size_t row_bytes, pitch;   /* bytes of a row that belong to the piece; distance of two rows */
  int32_t rows, reserved;
} uvghip_halo_piece_t;
UVGHIP_API int uvghip_loop_plan_create_rows(int bitdepth, const uvghip_ctu_params_t *params, const uvghip_loop_picture_t *pictures,
                                            int n_pictures, int sao_type, int ctu_row0, int ctu_row1, void *workspace,
                                            uvghip_loop_plan_t **plan_out);
UVGHIP_API int uvghip_loop_plan_halo(const uvghip_loop_plan_t *plan, int side, uvghip_halo_piece_t *pieces, int cap, int *n);
UVGHIP_API size_t uvghip_loop_plan_halo_bytes(const uvghip_loop_plan_t *plan);
UVGHIP_API int uvghip_loop_plan_halo_pack(uvghip_loop_plan_t *plan, void *message, void *stream);
UVGHIP_API int uvghip_loop_plan_halo_unpack(uvghip_loop_plan_t *plan, const void *message, void *stream);
UVGHIP_API int uvghip_loop_plan_out_rows(const uvghip_loop_plan_t *plan, int *y0, int *y1);
UVGHIP_API void uvghip_loop_plan_destroy(uvghip_loop_plan_t *plan);

/* ------------------- (6) the slice data: the arithmetic coder on the device -------------------------------------------- */

/* replaces: encoder_state_worker_encode_lcu_bitstream for every CTU of n all-intra pictures (src/encoderstate.c:862-939):
 * encode_sao, uvg_encode_coding_tree with uvg_encode_coeff_nxn, through the arithmetic coder of src/cabac.c, one substream per
 * WPP row (uvg_cabac_start ... end_of_sub_stream_one_bit, uvg_cabac_finish, alignment), emulation prevention applied
 * (uvg_bitstream_put_byte).  pictures: HOST array of the descriptors the search ran on (cu, cu_stride, coeff, models are read --
 * the row's start models are the third model set of the first CTU of the row above); sao_info / sao_models: the decisions and
 * models of uvghip_sao_decide_pictures ([picture][ctu][34] / [6]; both NULL = SAO off: no SAO syntax).
 * out: device buffer, row r of picture p at out + (p * rows + r) * row_cap; row_bytes[p * rows + r] = its length (if larger than
 * row_cap the buffer was too small and the row is truncated: 2 * 64 * pic_w * 1.5 bytes per row is a safe capacity).
 * The slice data of picture p is its rows one after the other; entry points = the row lengths.  One wave per row.
 * workspace: uvghip_slice_rows_workspace_bytes(n_pictures) of device memory; it receives the picture table (a synchronous
 * upload).  A later uvghip_encode_slice_rows with pictures == NULL reuses the table in the workspace and just enqueues the kernel. */
UVGHIP_API size_t uvghip_slice_rows_workspace_bytes(int n_pictures);
UVGHIP_API int uvghip_encode_slice_rows(int bitdepth, const uvghip_ctu_params_t *params, const uvghip_ctu_picture_t *pictures,
                                        int n_pictures, const int32_t *sao_info, const uint16_t *sao_models, void *workspace,
                                        uint8_t *out, int row_cap, int32_t *row_bytes, void *stream);

/* P / B pictures.  Beside uvghip_scu_t (type, sizes, cbf, mv_dir, mv[2][2] in 1/16 units; an intra CU keeps its modes in mv[0][0] as an
 * all-intra picture does) a second table holds what only the coder reads of an inter CU (cu_info_t: skipped, merged, merge_idx, root_cbf,
 * inter.mv_cand0 / 1, inter.mv_ref[2]); same indexing as the scu table. */
typedef struct uvghip_inter4_t { uint8_t skipped, merged, merge_idx, root_cbf, mv_cand0, mv_cand1, mv_ref0, mv_ref1; } uvghip_inter4_t;
/* the picture's slice-level state (encoder_state_t::frame: slicetype, poc, ref, ref_LX, ref_LX_size; cfg: tmvp_enable, max_merge,
 * log2_parallel_merge_level) and its side tables */
typedef struct uvghip_slice_pb_t {
  int32_t slice_type;              /* 0 B, 1 P (2 = I: the plain entry point does that) */
  int32_t poc, n_refs, ref_pocs[16], l_size[2], l[2][16];
  int32_t tmvp, max_merge, merge_level;
  int32_t frame_qp;                /* state->frame->QP: the slice's context models are initialised with it (params->qp is the CTUs' QP) */
  const int32_t *col;              /* DEVICE: the collocated picture ref_LX[0][0] on its 8x8 grid (uvghip_merge_cand_batch's layout) */
  const uvghip_inter4_t *inter4;   /* DEVICE, cu_stride entries per row */
  const uint32_t *models_inter;    /* DEVICE: per CTU three sets of the 18 inter-syntax models (state0 | state1 << 16), as `models` holds the 257 */
  int32_t col_stride;              /* > 0: `col` is the collocated picture's per-4x4 motion table (uvghip_ctu_pb_picture_t.motion_out) with this many
                                    * units per row, read at its even positions; 0: `col` is already the 8x8 grid */
  int32_t second_pass;             /* uvghip_encode_slice_rows_pb_alf only (the plain entry point ignores it), != 0: the rows are the SECOND coding
                                    * pass of the picture, as in every --alf run of the encoder -- it codes the CTUs once behind their search to keep
                                    * its models going and for real after the picture's ALF (src/encoderstate.c:856-860, 1043-1052), and clears a
                                    * row's history table (HMVP) before the first pass only (:1021-1028).  The AMVP predictors of the bitstream's
                                    * pass are derived with the table the row's first pass left, so its mvd bins, and the models a row hands to
                                    * the row below, are not those of the first pass (which `models` / `models_inter` hold): every row derives
                                    * its start by coding, into nothing, the first CTU of each row above.  0: one pass, the table starts empty */
} uvghip_slice_pb_t;
/* uvghip_encode_slice_rows for P / B pictures: the skip flag, prediction mode, merge flag / index, inter direction, reference indices,
 * motion vector differences against the AMVP predictor the CU chose (uvg_inter_get_mv_cand_cua on the picture's side information with the
 * row's history table, which the coder feeds as uvg_encode_coding_tree does), the root cbf and the transform tree of inter CUs
 * (src/encode_coding_tree.c:1470-1640, 769-900, 1865-1910, 628-760), intra CUs as in an I slice; models initialised for the slice type.
 * pb: HOST array, one per picture.  workspace: uvghip_slice_rows_pb_workspace_bytes(n_pictures). */
UVGHIP_API size_t uvghip_slice_rows_pb_workspace_bytes(int n_pictures);
UVGHIP_API int uvghip_encode_slice_rows_pb(int bitdepth, const uvghip_ctu_params_t *params, const uvghip_ctu_picture_t *pictures,
                                           const uvghip_slice_pb_t *pb, int n_pictures, const int32_t *sao_info, const uint16_t *sao_models,
                                           void *workspace, uint8_t *out, int row_cap, int32_t *row_bytes, void *stream);

/* uvghip_encode_slice_rows for all-intra pictures of an --alf on / --alf full run: the CTU-level ALF syntax (uvg_encode_alf_bits,
 * src/alf.c:1365-1413, called at src/encoderstate.c:880) between a CTU's SAO syntax and its coding tree -- alf_ctb_flag per component by the
 * neighbours' flags, the APS / fixed filter set choice and its truncated-binary index, the chroma alternative, the CC-ALF control.  The 18
 * models of that syntax follow the WPP hand-over like the others; a row's coder derives its start from the first CTUs of the rows above.
 *   alf[n_pictures] (HOST array; ctu_flags / filter_set_idx are DEVICE memory in the layout of uvghip_alf_picture_t): alf_type = cfg.alf_type
 *   (1 / 2), enabled = tile_group_alf_enabled_flag, n_luma_aps = tile_group_num_aps, n_alternatives_chroma of the slice's chroma APS,
 *   cc_enabled / cc_filter_count = cc_filter_param->cc_alf_filter_enabled / _count.
 * workspace: uvghip_slice_rows_alf_workspace_bytes(n_pictures). */
typedef struct uvghip_slice_alf {
  int32_t alf_type, enabled[3], n_luma_aps, n_alternatives_chroma, cc_enabled[2], cc_filter_count[2];
  const uint8_t *ctu_flags;
  const int16_t *filter_set_idx;
} uvghip_slice_alf_t;
UVGHIP_API size_t uvghip_slice_rows_alf_workspace_bytes(int n_pictures);
UVGHIP_API int uvghip_encode_slice_rows_alf(int bitdepth, const uvghip_ctu_params_t *params, const uvghip_ctu_picture_t *pictures, const uvghip_slice_alf_t *alf,
                                            int n_pictures, const int32_t *sao_info, const uint16_t *sao_models, void *workspace, uint8_t *out, int row_cap,
                                            int32_t *row_bytes, void *stream);

/* uvghip_encode_slice_rows_pb for P / B pictures of an --alf on / --alf full run: both tables -- pb[n_pictures] and alf[n_pictures], HOST
 * arrays as in the two entry points above, uploaded in stream order -- and the CTU-level ALF syntax between a CTU's SAO syntax and its
 * coding tree, its models initialised for the slice type.  A picture whose enabled[] and cc_enabled[] are all zero codes no ALF bin: with
 * pb[i].second_pass == 0 its rows are uvghip_encode_slice_rows_pb's.  A picture of a real --alf run has second_pass = 1, ALF on or off in its
 * slice (uvghip_loop_pb_alf_stage sets it).  workspace: uvghip_slice_rows_pb_alf_workspace_bytes(n_pictures). */
UVGHIP_API size_t uvghip_slice_rows_pb_alf_workspace_bytes(int n_pictures);
UVGHIP_API int uvghip_encode_slice_rows_pb_alf(int bitdepth, const uvghip_ctu_params_t *params, const uvghip_ctu_picture_t *pictures, const uvghip_slice_pb_t *pb,
                                               const uvghip_slice_alf_t *alf, int n_pictures, const int32_t *sao_info, const uint16_t *sao_models, void *workspace,
                                               uint8_t *out, int row_cap, int32_t *row_bytes, void *stream);

/* The ALF stage of a picture group behind uvghip_loop_plan_run (BASELINE configs[3]: --alf full) -- where the encoder runs
 * uvg_alf_enc_process (src/alf.c:5193) on pictures whose search, deblocking and SAO the device did.  The derivation of the decisions
 * (alf_encoder :3994, alf_encoder_ctb :4369, derive_cc_alf_filter :2212) stays with the host behind `decide`:
 *   decide(user, i, picture, decision): picture->out_* = the picture ALF gets (device planes), picture->search.src_* = the source; the
 *     statistics of alf_derive_stats_for_filtering (:4227) are the callback's to gather from them (uvghip_alf_classify_frame,
 *     uvghip_alf_stats_compact_batch + uvghip_alf_cov_reduce, uvghip_alf_stats_batch for chroma, uvghip_cc_alf_stats_batch; it
 *     synchronises what it reads back).  It fills *decision with HOST arrays in the layouts of uvghip_alf_picture_t / uvghip_slice_alf_t,
 *     valid until it is called again or the stage returns; 0 = ok.
 * Per picture the stage then runs uvghip_alf_reconstruct_picture from the SAO output into alf_out[i] (a picture without any enabled
 * component is copied), and for the group uvghip_encode_slice_rows_alf: rows / row_bytes as in uvghip_encode_slice_rows_alf
 * ([picture][row][row_cap] bytes, [picture][row] lengths; device memory).  classification_shift: cfg.input_bitdepth + 4 (:5185).
 * workspace: uvghip_loop_plan_alf_workspace_bytes(plan) of device memory.  The call returns with the stream's work enqueued; it
 * synchronises the stream between pictures (the decisions are host data). */
typedef struct uvghip_alf_decision {
  int32_t alf_type;                  /* cfg.alf_type: 1 --alf no-cc, 2 --alf full */
  int32_t enabled[3];                /* slice->alf->tile_group_alf_enabled_flag[c] */
  int32_t n_luma_aps;                /* tile_group_num_aps */
  const int16_t *luma_aps;           /* [n_luma_aps][677] as uvghip_alf_picture_t.luma_aps */
  const int16_t *chroma_aps;         /* [114] as uvghip_alf_picture_t.chroma_aps ([112] = num_alternatives_chroma) */
  int32_t cc_enabled[2], cc_filter_count[2];
  const int16_t *cc_coeff;           /* [2][4][8] */
  const uint8_t *ctu_flags;          /* [7][ctus] as uvghip_alf_picture_t.ctu_flags */
  const int16_t *filter_set_idx;     /* [ctus] */
} uvghip_alf_decision_t;
typedef struct uvghip_alf_planes { void *y, *u, *v; int32_t stride, stride_c; } uvghip_alf_planes_t;      /* device planes, strides in samples */
typedef int (*uvghip_alf_decide_fn)(void *user, int picture, const uvghip_loop_picture_t *planes, uvghip_alf_decision_t *decision);
UVGHIP_API size_t uvghip_loop_plan_alf_workspace_bytes(const uvghip_loop_plan_t *plan);
UVGHIP_API int uvghip_loop_plan_alf_stage(uvghip_loop_plan_t *plan, uvghip_alf_decide_fn decide, void *user, int classification_shift, const uvghip_alf_planes_t *alf_out,
                                          void *workspace, uint8_t *rows, int row_cap, int32_t *row_bytes, void *stream);

/* ------------------- (7) the picture's NAL units behind the parameter sets -------------------------------------------- */

/* replaces: uvg_image_checksum / array_checksum_generic (src/nal.c:91-115, src/strategies/generic/nal-generic.c:68-92) on the
 * picture after the in-loop filters: per plane the sum of (low byte ^ m) [+ (high byte ^ m) above 8 bits], m = (x ^ y ^ x >> 8 ^
 * y >> 8) & 0xff, modulo 2^32.  sums: three uint32 in DEVICE memory (Y, U, V), zeroed and filled on the stream. */
UVGHIP_API int uvghip_picture_checksum(int bitdepth, const void *plane_y, int stride_y, const void *plane_u, const void *plane_v,
                                       int stride_c, int width, int height, uint32_t *sums, void *stream);
/* ... of the rectangle [x0, x0 + width) x [y0, y0 + height) (luma samples, even) of the picture whose planes are given, ADDED to sums (the
 * caller zeroes them): a sample's term depends on the sample and its position in the picture only, so the sums of rectangles that tile the
 * picture add up to uvghip_picture_checksum's -- tiles on several devices contribute with an all-reduce of three words. */
UVGHIP_API int uvghip_picture_checksum_rect(int bitdepth, const void *plane_y, int stride_y, const void *plane_u, const void *plane_v,
                                            int stride_c, int x0, int y0, int width, int height, uint32_t *sums, void *stream);

/* replaces: for an IDR picture of an all-intra (-p 1) stream in the configuration of uvghip_ctu_plan_create (WPP, one slice, picture
 * header in the slice header): uvg_nal_write + uvg_encoder_state_write_bitstream_slice_header with the entry points
 * (src/encoder_state-bitstream.c:993-1139, 1248-1411, src/nal.c:43-74), the rows' substreams appended as the encoder's
 * uvg_bitstream_move does, and add_checksum (:1420-1477), with the emulation prevention of src/bitstream.c:215-226.
 * A HOST function (works without a device): rows = the slice data of uvghip_encode_slice_rows copied to host memory (row r at rows +
 * r * row_pitch, row_bytes[r] bytes), checksum = the three sums of uvghip_picture_checksum (NULL: no SEI), sao != 0: the stream has
 * SAO on (two flags in the header).  poc = the picture's index in the stream: picture 0 follows the parameter sets (IDR_N_LP, short
 * start code), later pictures open their access unit (IDR_W_RADL, long start code; src/encoderstate.c:1965-1966).  Writes at most cap bytes to out, *len = the bytes needed (an error if that is more than cap).
 * Behind the encoder's parameter sets (SPS, PPS, version SEI -- control plane, independent of the picture) these bytes complete the
 * .266 of a one-picture encode, byte for byte (tests/test_picture_nal.py). */
UVGHIP_API int uvghip_write_picture_nals(int poc, int sao, const uint8_t *rows, size_t row_pitch, const int32_t *row_bytes, int n_rows,
                                         const uint32_t *checksum, uint8_t *out, size_t cap, size_t *len);
/* the same with a slice QP offset: sh_qp_delta = state->frame->QP - cfg.qp (the intra QP offset of the first picture of a low-delay stream) */
UVGHIP_API int uvghip_write_idr_nals(int poc, int qp_delta, int sao, const uint8_t *rows, size_t row_pitch, const int32_t *row_bytes, int n_rows,
                                     const uint32_t *checksum, uint8_t *out, size_t cap, size_t *len);
/* the same with the POC width of the stream's SPS: poc_lsb_bits = encoder_control->poc_lsb_bits = max(4, ceil_log2(2 gop_len + 1))
 * (src/encoder.c:242; ph_pic_order_cnt_lsb, src/encoder_state-bitstream.c:1041-1042).  The two functions above write 4 bits. */
UVGHIP_API int uvghip_write_idr_nals_ra(int poc, int poc_lsb_bits, int qp_delta, int sao, const uint8_t *rows, size_t row_pitch, const int32_t *row_bytes,
                                        int n_rows, const uint32_t *checksum, uint8_t *out, size_t cap, size_t *len);
/* ... and for a P / B picture of a low-delay stream (pictype TRAIL, one temporal layer, long start code).
 * replaces: uvg_encoder_state_write_bitstream_slice_header (src/encoder_state-bitstream.c:1248-1411) with _picture_header (:1009-1139)
 * and _ref_pic_list (:1141-1246): inter / intra slice allowed, ph_pic_temporal_mvp_enabled_flag, slice type, the reference picture
 * list syntax -- list 0's entries written twice when cfg.bipred (copy_rpl1: the low-delay list 1 is a copy, :1165), the active
 * override, the collocated picture -- and sh_qp_delta.  delta_neg[n_ref_neg]: poc - POC of every reference picture in the order of the
 * GOP structure's ref_neg[] (uvg_config_process_lp_gop, src/cfg.c:1640-1720: ascending distance); poc_lsb_bits: encoder_control->
 * poc_lsb_bits; slice_type 0 B, 1 P; tmvp: cfg.tmvp_enable; qp_delta: state->frame->QP - cfg.qp. */
UVGHIP_API int uvghip_write_picture_nals_pb(int poc, int poc_lsb_bits, int slice_type, int n_ref_neg, const int32_t *delta_neg, int copy_rpl1, int tmvp,
                                            int qp_delta, int sao, const uint8_t *rows, size_t row_pitch, const int32_t *row_bytes, int n_rows,
                                            const uint32_t *checksum, uint8_t *out, size_t cap, size_t *len);
/* ... and for a P / B picture of a random-access stream (--gop 8 / --gop 16, the hierarchical structures of src/gop.h; what --preset
 * medium and slower run with): the same syntax with list 1 holding the references in the FUTURE -- num_ref_entries[1] and its entries
 * with strp_entry_sign_flag 0 (:1200-1234), sh_num_ref_idx_active_minus1[1] when it has more than one (:1237-1241).  delta_pos[n_ref_pos]:
 * POC of the reference - poc, in the order of the GOP entry's ref_pos[] restricted to the pictures in the reference buffer (ascending);
 * delta_neg likewise from ref_neg[].  poc_lsb_bits: max(4, ceil_log2(2 gop_len + 1)) (src/encoder.c:242; 6 for --gop 16).  Pictures of
 * such a stream are written in CODING order. */
UVGHIP_API int uvghip_write_picture_nals_ra(int poc, int poc_lsb_bits, int slice_type, int n_ref_neg, const int32_t *delta_neg, int n_ref_pos,
                                            const int32_t *delta_pos, int tmvp, int qp_delta, int sao, const uint8_t *rows, size_t row_pitch,
                                            const int32_t *row_bytes, int n_rows, const uint32_t *checksum, uint8_t *out, size_t cap, size_t *len);

/* ... with the NAL unit type as a parameter, for a random-access stream with several intra periods and an open GOP (cfg.open_gop, the
 * default): nal_type 9 (CRA: the I picture opening a later period -- slice_type 2; its header still carries the reference picture lists
 * of the buffer, :1326-1329, and sh_no_output_of_prior_pics_flag, :1278), 3 (RASL: a picture before the CRA picture in display order
 * coded after it; pictype at src/encoderstate.c:1957-1972) or 0 (TRAIL = uvghip_write_picture_nals_ra). */
UVGHIP_API int uvghip_write_picture_nals_gop(int nal_type, int poc, int poc_lsb_bits, int slice_type, int n_ref_neg, const int32_t *delta_neg, int n_ref_pos,
                                             const int32_t *delta_pos, int tmvp, int qp_delta, int sao, const uint8_t *rows, size_t row_pitch,
                                             const int32_t *row_bytes, int n_rows, const uint32_t *checksum, uint8_t *out, size_t cap, size_t *len);

/* ... of a picture of an --alf on / --alf full all-intra stream: the ALF APS NAL units written in front of the slice
 * (uvg_encode_alf_adaptive_parameter_set, src/alf.c:1610 -> encode_alf_aps :1575, encoder_state_write_adaptation_parameter_set :1547,
 * encode_alf_aps_flags :1452, encode_alf_aps_filter :1415; called at src/encoder_state-bitstream.c:1562) and the slice header's ALF fields
 * (:1283-1330).  HOST function.  aps[n_aps]: the parameter sets the encoder's map marks as changed for this picture, in aps id order.
 *   uvghip_alf_slice_t: alf_type = cfg.alf_type (1 no CC-ALF, 2 full); enabled = tile_group_alf_enabled_flag; n_luma_aps / luma_aps_id =
 *     tile_group_num_aps / tile_group_luma_aps_id; chroma_aps_id; cc_enabled = cc_filter_param->cc_alf_filter_enabled; cc_aps_id =
 *     tile_group_cc_alf_cb_aps_id / _cr_aps_id
 *   uvghip_alf_aps_t: the fields of alf_aps (alf.h:213-232) as coded: luma = luma_coeff[25][13], luma_clipp[25][13], filter_coeff_delta_idx[25]
 *     (int16, 675 words); chroma = chroma_coeff[8][7], chroma_clipp[8][7] (112 words); cc = cc_alf_coeff[2][4][8] (64 words) */
typedef struct uvghip_alf_slice {
  int32_t alf_type, enabled[3], n_luma_aps, luma_aps_id[8], chroma_aps_id, cc_enabled[2], cc_aps_id[2];
} uvghip_alf_slice_t;
typedef struct uvghip_alf_aps {
  int32_t aps_id, new_filter[2], non_linear[2], num_luma_filters, num_alternatives_chroma, new_cc_filter[2], cc_filter_count[2];
  const int16_t *luma, *chroma, *cc;
} uvghip_alf_aps_t;
UVGHIP_API int uvghip_write_idr_nals_alf(int poc, int qp_delta, int sao, const uvghip_alf_slice_t *alf, const uvghip_alf_aps_t *aps, int n_aps, const uint8_t *rows,
                                         size_t row_pitch, const int32_t *row_bytes, int n_rows, const uint32_t *checksum, uint8_t *out, size_t cap, size_t *len);

/* ... of a picture of an --alf on / --alf full stream WITH a GOP structure (BASELINE configs[3]: --gop 16): uvghip_write_picture_nals_gop
 * plus the APS NAL units in front of the slice and the slice header's ALF fields, which stand behind sh_slice_type /
 * sh_no_output_of_prior_pics_flag and in front of the reference picture lists (src/encoder_state-bitstream.c:1283-1330).  The first NAL unit
 * of the access unit -- the first APS, or the slice when n_aps == 0 -- takes the long start code.  alf is required (the SPS of such a stream
 * has ALF on: a slice with everything off still carries slice_alf_enabled_flag = 0).
 * nal_type: 0 TRAIL, 3 RASL, 9 CRA as uvghip_write_picture_nals_gop, and 7 / 8 (IDR_W_RADL / IDR_N_LP: slice_type 2, no reference lists, the
 * POC in poc_lsb_bits bits; an IDR picture with poc 0 follows the stream's parameter sets and takes short start codes as in
 * uvghip_write_idr_nals_alf).  copy_rpl1: as in uvghip_write_picture_nals_pb (a low-delay structure with cfg.bipred: list 1 signalled as a
 * copy of list 0's entries, n_ref_pos = 0); 0 for a random-access stream.  HOST function. */
UVGHIP_API int uvghip_write_picture_nals_gop_alf(int nal_type, int poc, int poc_lsb_bits, int slice_type, int n_ref_neg, const int32_t *delta_neg, int n_ref_pos,
                                                 const int32_t *delta_pos, int copy_rpl1, int tmvp, int qp_delta, int sao, const uvghip_alf_slice_t *alf,
                                                 const uvghip_alf_aps_t *aps, int n_aps, const uint8_t *rows, size_t row_pitch, const int32_t *row_bytes, int n_rows,
                                                 const uint32_t *checksum, uint8_t *out, size_t cap, size_t *len);

/* After uvghip_loop_plan_run: the NAL units (slice + hash SEI) of picture `picture` of the plan's group as picture number `poc` of the
 * stream, into HOST memory -- uvghip_picture_checksum on its output picture, its rows brought to the host, uvghip_write_picture_nals.
 * Waits for the stream.  *len = bytes needed; an error if that exceeds cap. */
UVGHIP_API int uvghip_loop_plan_picture_nals(uvghip_loop_plan_t *plan, int picture, int poc, uint8_t *out, size_t cap, size_t *len, void *stream);
/* ... of ALL pictures of the group, as pictures first_poc, first_poc + 1, ... : what n calls of uvghip_loop_plan_picture_nals write, one
 * after the other into `out` (lens[i] = bytes of picture i; HOST memory, n entries).  The checksums of all pictures first, their sums
 * and row lengths in one copy, the rows gathered on the device and brought over in one copy: two waits for the stream instead of 2 n.
 * (The encoder's bitstream writer appends a frame's NAL units when the frame is done, src/encoder_state-bitstream.c:1513-1607; with a group
 * of frames in one launch they are all done together.) */
UVGHIP_API int uvghip_loop_plan_group_nals(uvghip_loop_plan_t *plan, int first_poc, uint8_t *out, size_t cap, size_t *lens, void *stream);

/* ------------------- (7a) one all-intra picture from HOST memory: the frame-level hand-over ------------------------------- */

/* replaces, for an all-intra frame under --preset medium -p 1 --wpp: encoder_state_encode(state) inside uvg_encode_one_frame
 * (src/encoderstate.c:2051-2091 -> :1221-1365 -> encoder_state_encode_leaf :1004-1190: the per-CTU search / bitstream jobs of every WPP row)
 * and the frame's SAO reconstruction.  The encoder keeps encoder_state_init_new_frame in front of it (slice type, QP, lambda: the
 * params below are what uvg_set_lcu_lambda_and_qp leaves in a leaf state, src/rate_control.c:1097-1188) and its own
 * uvg_encoder_state_worker_write_bitstream behind it: parameter sets, slice header with the entry points, the children's streams,
 * the hash SEI (src/encoder_state-bitstream.c:1513-1607).
 * One pool per encoder: n_slots = frames in flight (the reference has one main encoder_state_t per --owf slot: cfg.owf + 1), each slot
 * the device buffers of one picture.  Frames that are begun collect in a GROUP; a group becomes ONE uvghip_loop_plan launch on a stream of
 * its own when it holds group_max pictures, when a frame with other parameters arrives, or when one of its frames is asked for -- the
 * pictures of a group share the device as the pictures of bench.py's launch do (separate launches of single pictures do not: beyond a
 * handful of queues their waiting workgroups crowd each other out).
 *   begin:  slot = the frame's slot (free: never used or finished); src_* = frame->source planes (HOST memory, strides in samples);
 *           stages them, enqueues the upload and returns.  params may differ from picture to picture (QP, lambda); the size may not.
 *   finish: launches the slot's group if it still collects, waits for it; out_* (HOST, strides in samples) receive the picture the
 *           encoder returns (frame->rec after deblocking and SAO); rows / row_bytes / n_rows: the substreams of the WPP rows one after
 *           the other in HOST memory owned by the pool (valid until the slot's next begin), row_bytes[r] bytes each -- what leaf state r
 *           holds in `stream` after its last CTU, emulation prevention included (append with uvg_bitstream_writebyte, not
 *           uvg_bitstream_put_byte).  May be called from another thread than begin (the bitstream job) and beside it.
 * Refuses what uvghip_loop_plan_create refuses (anything but --preset medium / slow -p 1 with SAO, qp_c != qp).
 * Reference-side caller: uvg266_amd/csrc/shim/frame-hip.c, applied by tools/refcheck/patch_ref_hip.py. */
typedef struct uvghip_frame_pool uvghip_frame_pool_t;
UVGHIP_API int uvghip_frame_pool_create(int bitdepth, const uvghip_ctu_params_t *params, int sao_type, int n_slots, int group_max, uvghip_frame_pool_t **pool_out);
/* ... for frames cut into tiles (--tiles CxR --wpp, section 7b): col_ctus[cols] / row_ctus[rows] = encoder->tiles_col_width[] / tiles_row_height[] (in
 * CTUs; the uniform grid and --tiles-width-split / --tiles-height-split alike).  A group is then one uvghip_tiles_plan launch; finish hands out
 * the substreams of ALL tiles in the order of the bitstream (tile raster order, each tile's rows in order: the encoder's leaf states in the
 * order encoder_state_write_bitstream_children visits them), n_rows = their number. */
UVGHIP_API int uvghip_frame_pool_create_tiles(int bitdepth, const uvghip_ctu_params_t *params, int sao_type, int n_slots, int group_max, const int32_t *col_ctus, int cols,
                                              const int32_t *row_ctus, int rows, uvghip_frame_pool_t **pool_out);
UVGHIP_API int uvghip_frame_pool_begin(uvghip_frame_pool_t *pool, int slot, const uvghip_ctu_params_t *params, const void *src_y, const void *src_u,
                                       const void *src_v, int src_stride, int src_stride_c);
UVGHIP_API int uvghip_frame_pool_finish(uvghip_frame_pool_t *pool, int slot, void *out_y, void *out_u, void *out_v, int out_stride, int out_stride_c,
                                        const uint8_t **rows, const int32_t **row_bytes, int *n_rows);
UVGHIP_API void uvghip_frame_pool_destroy(uvghip_frame_pool_t *pool);

/* ------------------- (7b) tiles: the independent rectangles of a picture ---------------------------------------------------- */

/* replaces: the encoder's TILE states for all-intra pictures under --tiles <cols>x<rows> --wpp (encoder_state_t of type
 * ENCODER_STATE_TYPE_TILE, src/encoder_state-ctors_dtors.c: a sub-image of the frame, a cu_array view, a CABAC start and WPP rows per tile;
 * the uniform grid and the tile scan of src/encoder.c:445-451, 480-510; the tile loop of encoder_state_encode, src/encoderstate.c:1221).
 * In the reference a tile's edges are picture edges to the search AND to the in-loop filters (state->tile->frame everywhere;
 * pps_loop_filter_across_tiles_enabled_flag = 0, src/encoder_state-bitstream.c:788), every tile starts from initialised context models,
 * and the slice data is the tiles' substreams in tile raster order with all of them among the slice header's entry points (:977-1007).
 * So a tile is a picture of its own size whose planes are views into the frame's: a tiles plan is one uvghip_loop_plan per tile SIZE (a
 * uniform grid has at most four) that run beside each other -- the tiles of one picture are that many WPP wavefronts in flight.
 *
 * uvghip_tile_grid: HOST function.  tiles[cols * rows]: the grid in samples, raster order; first_ctu[cols * rows] (may be NULL): the
 * tile-scan address (tiles_ctb_addr_rs_to_ts) of each tile's first CTU.  Refuses what the encoder refuses (more tiles than CTUs in a
 * dimension, MAX_TILES_PER_DIM).
 * uvghip_tiles_plan_create: pictures = the WHOLE pictures as for uvghip_loop_plan_create, params = the whole picture's; coeff / models
 * hold a picture's CTUs in TILE-SCAN order (the order of the bitstream); cu in picture raster as ever (cu_stride >= 16 * CTUs per row).
 * workspace: uvghip_tiles_workspace_bytes of device memory, in use until the plan is destroyed.
 * uvghip_tiles_plan_run: search + filters + slice data of every tile of every picture; returns at once; the size classes run on the
 * plan's own streams, forked from and joined to `stream`.
 * uvghip_tiles_plan_tile: where tile `tile` (raster order) of picture `picture` lives -- its size class's loop plan and its picture index
 * there (for uvghip_loop_plan_results / _slice_data), its rectangle, its first CTU's tile-scan address; any output pointer may be NULL.
 * uvghip_tiles_plan_nals: after a run, the NAL units (slice NAL with the entry points of ALL substreams + hash SEI of the whole output
 * picture) of pictures [first, first + count) as pictures first_poc, ... of the stream, one after the other into HOST memory (lens[i]
 * bytes each); waits for the stream.  Behind the encoder's parameter sets (its PPS carries the grid, :768-791) they complete the .266 the
 * encoder writes under --tiles, byte for byte (tests/test_gpu_tiles.py against tests/golden/ref_tiles_*.npz). */
typedef struct uvghip_tiles_plan uvghip_tiles_plan_t;
UVGHIP_API int uvghip_tile_grid(int pic_w, int pic_h, int cols, int rows, uvghip_rect_t *tiles, int32_t *first_ctu);
UVGHIP_API size_t uvghip_tiles_workspace_bytes(int bitdepth, int n_pictures, int pic_w, int pic_h, int cols, int rows);
UVGHIP_API int uvghip_tiles_plan_create(int bitdepth, const uvghip_ctu_params_t *params, const uvghip_loop_picture_t *pictures, int n_pictures, int tile_cols, int tile_rows,
                                        int sao_type, void *workspace, uvghip_tiles_plan_t **plan_out);
UVGHIP_API int uvghip_tiles_plan_run(uvghip_tiles_plan_t *plan, void *stream);
UVGHIP_API int uvghip_tiles_plan_layout(const uvghip_tiles_plan_t *plan, int *n_tiles, int *n_classes, int *n_substreams);
UVGHIP_API int uvghip_tiles_plan_tile(const uvghip_tiles_plan_t *plan, int picture, int tile, uvghip_loop_plan_t **loop_plan, int *index, uvghip_rect_t *rect, int *first_ctu);
UVGHIP_API int uvghip_tiles_plan_nals(uvghip_tiles_plan_t *plan, int first, int count, int first_poc, uint8_t *out, size_t cap, size_t *lens, void *stream);
UVGHIP_API void uvghip_tiles_plan_destroy(uvghip_tiles_plan_t *plan);
/* The tiles of a picture over the devices of a node ("independent units exist at ... tiles").  Tiles share nothing -- no
 * neighbour in the search, no sample in the filters --, so under the closed loop they are the one partition of ONE picture whose parts run
 * side by side from the first CTU on (CTU-row bands wait for the band above), and the only exchange is at the picture's end: the substreams'
 * lengths and bytes and three words of checksum go to whoever writes the NAL units.
 * uvghip_tiles_plan_create_owned: owned[cols * rows] (raster order of the tiles; NULL = all): the tiles this device searches, filters and
 * codes.  Pictures, tables and the layout of coeff / models are the whole picture's on every device; a device writes its tiles' parts.
 * uvghip_tiles_plan_substreams: after a run, in HOST memory: lens[count][n_substreams] (uvghip_tiles_plan_layout) -- every substream's length
 * in the order of the bitstream, 0 for the tiles of other devices --, the owned substreams' bytes one after the other in that order
 * (*used bytes; an error beyond cap), sums[count][3] -- the owned tiles' terms of the output picture's checksum
 * (uvghip_picture_checksum_rect).  Over the devices lengths and sums ADD UP (an all-reduce / a gather); uvghip_write_picture_nals then
 * writes what uvghip_tiles_plan_nals writes on one device (tests/test_gpu_tiles.py with emulated ranks, tests/test_tiles.py with gloo). */
/* ... with the grid of --tiles-width-split / --tiles-height-split (src/encoder.c:452-478) instead of the uniform one: col_ctus[cols] / row_ctus[rows]
 * = the columns' widths and the rows' heights in CTUs (encoder->tiles_col_width[] / tiles_row_height[]: the options' sample positions divided by
 * 64, the last one the remainder); they must add up to the picture's CTU columns / rows.  owned as for _create_owned (NULL: all tiles). */
UVGHIP_API int uvghip_tile_grid_split(int pic_w, int pic_h, const int32_t *col_ctus, int cols, const int32_t *row_ctus, int rows, uvghip_rect_t *tiles, int32_t *first_ctu);
UVGHIP_API size_t uvghip_tiles_workspace_bytes_split(int bitdepth, int n_pictures, int pic_w, int pic_h, const int32_t *col_ctus, int cols, const int32_t *row_ctus, int rows,
                                                     const uint8_t *owned);
UVGHIP_API int uvghip_tiles_plan_create_split(int bitdepth, const uvghip_ctu_params_t *params, const uvghip_loop_picture_t *pictures, int n_pictures, const int32_t *col_ctus,
                                              int tile_cols, const int32_t *row_ctus, int tile_rows, const uint8_t *owned, int sao_type, void *workspace,
                                              uvghip_tiles_plan_t **plan_out);
UVGHIP_API size_t uvghip_tiles_workspace_bytes_owned(int bitdepth, int n_pictures, int pic_w, int pic_h, int cols, int rows, const uint8_t *owned);
UVGHIP_API int uvghip_tiles_plan_create_owned(int bitdepth, const uvghip_ctu_params_t *params, const uvghip_loop_picture_t *pictures, int n_pictures, int tile_cols,
                                              int tile_rows, const uint8_t *owned, int sao_type, void *workspace, uvghip_tiles_plan_t **plan_out);
UVGHIP_API int uvghip_tiles_plan_substreams(uvghip_tiles_plan_t *plan, int first, int count, int32_t *lens, uint8_t *bytes, size_t cap, size_t *used, uint32_t *sums,
                                            void *stream);

/* ------------------- (8) P / B pictures: candidate lists of the inter search ---------------------------------------------- */

/* replaces: uvg_inter_get_merge_cand (src/inter.c:1989-2192) for n calls at once, one lane per call: the spatial candidates A0 / A1 /
 * B0 / B1 / B2 with the coding-order and duplicate tests (get_spatial_merge_candidates :1368-1455, is_cand_coded :770-876), the
 * temporal candidate from the collocated picture with POC scaling and the stored-vector round trip (:1031-1165, 1547-1601), the history
 * table, the pairwise average, the zero vectors.  All arrays in DEVICE memory:
 *   ctx  [n][64]       the call: [1..4] x, y, width, height of the CU; [5] POC; [6] slice type (0 = B, 1 = P); [7..8] picture size;
 *                      [9] tmvp; [10] max merge candidates; [11] log2 parallel merge level; [12] wpp; [13] reference pictures in use,
 *                      [14..29] their POCs; [30..31] list sizes, [32..39] / [40..47] ref_LX[0] / [1]; [49] the CU's split_tree;
 *                      (uvghip_amvp_cand_batch: [50] the list, [51..52] the CU's mv_ref[0..1])
 *   lcu  [n][290][8]   lcu_t.cu at the moment of the call (17 x 17 + 1 entries: type, mv[2][2], mv_ref[2], mv_dir); MODIFIED like the
 *                      reference does (inter_clear_cu_unused on the neighbours it looks at, :749-758)
 *   col  [n] x col_stride ints: the collocated picture ref_LX[0][0] on its 8x8 grid ((pic_w + 7) / 8 positions per row), 8 ints per
 *                      position: type, mv[2][2], mv_dir, the POC the L0 / L1 vector points to (col_stride 0: one picture for all calls)
 *   hmvp [n][41]       [0] entries in the CTU row's history table, then its five entries (most recent first) in the lcu layout
 *   cands [n][6][7]    inter_merge_cand_t: dir, ref[2], mv[2][2];  counts [n]: the function's return value */
UVGHIP_API int uvghip_merge_cand_batch(const int32_t *ctx, int32_t *lcu, const int32_t *col, long col_stride, const int32_t *hmvp, int n,
                                       int32_t *cands, int32_t *counts, void *stream);
/* replaces: uvg_inter_get_mv_cand (src/inter.c:1606-1737): the two AMVP predictors of list ctx[50] for the reference index being
 * searched, rounded to quarter samples.  mv_cand [n][2][2]. */
UVGHIP_API int uvghip_amvp_cand_batch(const int32_t *ctx, int32_t *lcu, const int32_t *col, long col_stride, const int32_t *hmvp, int n,
                                      int32_t *mv_cand, void *stream);

/* replaces: for n prediction units at once, what search_pu_inter_ref and search_frac do for one reference picture once the predictors
 * are known (src/search_inter.c:1404-1500, 1029-1226): select_starting_point (:297-375), early_terminate (:491-539), hexagon_search
 * (:767-847), then the four fractional steps on SATD (:1133-1216), every point priced as SAD / SATD + bits * lambda_sqrt with the bits
 * of get_mvd_coding_cost against the cheaper of the two AMVP predictors (:378-488).  --preset medium: me = hexbs, subme = 4,
 * me-early-termination = on, mv-rdo = 0, no mv constraint.  One wave per unit; all units of a call have the same size. */
typedef struct uvghip_me_job_t {
  int32_t x, y;                /* the unit's position in the picture (luma samples) */
  int32_t ref;                 /* index into refs_dev */
  int32_t mv_cand[2][2];       /* uvg_inter_get_mv_cand's two predictors, 1/16 sample units */
  int32_t extra_mv[2];         /* the reference picture's own vector at the unit's centre, scaled (search_inter.c:1346-1402); (0, 0): none */
  int32_t n_start;             /* the uni-predicted merge candidates' vectors, in list order (dir != 3), 1/16 units;
                                  -1: no integer search -- search_frac alone around the integer vector extra_mv (a multiple of 16) */
  int32_t start[6][2];
} uvghip_me_job_t;
typedef struct uvghip_me_result_t {
  int32_t mv[2];               /* the vector after the fractional search (the integer vector if fme_level == 0), 1/16 units */
  int32_t int_mv[2];           /* after the integer search */
  double cost, bits;           /* search_frac's best_cost / best_bits (or the integer search's) */
  double int_cost, int_bits;
  int32_t mv_cand;             /* select_mv_cand for mv: which predictor codes it cheaper */
  int32_t skipped_hexagon;     /* early_terminate said stop */
} uvghip_me_result_t;
/* cur: the source luma plane; refs_dev: DEVICE array of pointers to the reference pictures' luma planes (pic_w x pic_h samples, stride
 * ref_stride; blocks reaching outside are edge-replicated as uvg_image_calc_sad / uvg_get_extended_block do); size: 8, 16, 32 or 64;
 * fme_level: 0 or 4; jobs / results: DEVICE arrays. */
UVGHIP_API int uvghip_me_search_batch(int bitdepth, const void *cur, int cur_stride, const void *const *refs_dev, int ref_stride, int pic_w,
                                      int pic_h, double lambda_sqrt, int fme_level, int size, const uvghip_me_job_t *jobs, int n,
                                      uvghip_me_result_t *results, void *stream);

/* replaces: uvg_inter_pred_pu (luma) + uvg_satd_any_size as the inter search uses them per candidate motion (src/search_inter.c:
 * 1758-1775 merge analysis, :2018-2031 the bi-prediction of the two best uni-predictions) and, with `pred` given, the luma of
 * uvg_inter_recon_cu (src/inter.c:400-748: integer copy or 8-tap interpolation per list with border replication, 14-bit intermediates and
 * uvg_bipred_average for two lists).  One wave per candidate; all candidates of a call have the same square size (8 .. 64). */
typedef struct uvghip_motion_t {
  int32_t x, y;                /* the unit's position in the picture */
  int32_t dir;                 /* 1: list 0, 2: list 1, 3: both */
  int32_t ref[2];              /* per list: index into refs_dev (the PICTURE, i.e. ref_LX[l][mv_ref[l]]) */
  int32_t mv[2][2];            /* 1/16 sample units */
} uvghip_motion_t;
/* satd[n]: uvg_satd_any_size(prediction, source) >> (bitdepth - 8);  pred (optional): n blocks of size x size samples */
UVGHIP_API int uvghip_inter_pred_satd_batch(int bitdepth, const void *cur, int cur_stride, const void *const *refs_dev, int ref_stride, int pic_w,
                                            int pic_h, int size, const uvghip_motion_t *cands, int n, uint32_t *satd, void *pred, void *stream);

/* ------------------- (9) P / B pictures: the closed-loop CTU search ------------------------------------------------------- */

/* replaces, for the CTUs of P / B pictures of a low-delay encode (BASELINE configs[2]: --gop lp-g4d3t1 --preset medium):
 * encoder_state_worker_encode_lcu_search (src/encoderstate.c:808-976) minus the bitstream writer -- uvg_search_lcu / search_cu
 * (src/search.c:1299-2479) with uvg_search_cu_inter (src/search_inter.c:2329-2406: merge analysis with SATD, the early skip test,
 * per reference picture the starting points + early termination + hexagon search + fractional search, bi-prediction of the two best)
 * competing with the intra search, 64x64 CUs, the history table (src/inter.c:1831-1905), RDOQ with the root cbf, the reconstruction of
 * inter CUs (src/inter.c:400-748), then the deblocking filter's side effect on the stored motion (src/filter.c:745-765) and the real
 * coder's model adaptation (uvg_encode_coding_tree) so that the next CTU starts from the reference's models and history table.
 * Configuration subset: rd = 0, me = hexbs, subme = 0 or 4, bipred, early-skip, me-early-termination on, mv-rdo off, max-merge <= 6,
 * pu-depth-inter 0-3, pu-depth-intra 1..4 / 2..4, WPP, owf = 0 (every vector inside the reference is legal), one slice per picture.
 * Bit-exact with the reference: tests/golden/ref_inter_* (tests/test_gpu_ctu_search_pb.py; the CPU tests run the same source on the
 * host, tests/test_ctu_pb_emulation.py).  Vectors and reference indices of the lists a 4x4 unit does NOT use may differ from the
 * reference's cu_array in units on the right / bottom edge of a CU (csrc/ctu_pb.h); nothing reads them.
 *
 * One picture: `params` are ITS QP and lambdas (the GOP layer's); `pic` as for an intra picture (an inter CU's entry of `cu` holds
 * mv_dir, mv[2][2] in 1/16 units and ref_id[] = the position of each used list's picture in the reference array; an intra CU's
 * mv[0][0] its modes); inter4 / models_inter / trees / motion_out: the outputs beside it -- the coder's second side table
 * (uvghip_encode_slice_rows_pb reads cu, inter4, coeff, models, models_inter as they are), three sets of the 18 inter-syntax models
 * per CTU, split_tree | mode_type_tree << 16 per 4x4 (optional), and this picture's motion in the layout of ref_motion (optional;
 * what later pictures that refer to this one are given).
 * ref_y/u/v[i], ref_motion[i]: reference picture i of state->frame->ref (planes AFTER its in-loop filters; motion [per 4x4][8] int32:
 * cu type, mv[2][2], mv_dir, the POC the L0 / L1 vector points to or -1; rows of ref_motion_stride units; an intra picture: type 1
 * everywhere).  ref_pocs / l_size / l: state->frame->ref->pocs, ref_LX_size, ref_LX.  All pointers DEVICE memory. */
typedef struct uvghip_ctu_pb_picture {
  uvghip_ctu_params_t params;
  uvghip_ctu_picture_t pic;
  int32_t slice_type;              /* 0 B, 1 P */
  int32_t poc, n_refs, ref_pocs[16], l_size[2], l[2][16];
  int32_t tmvp, max_merge, merge_level;      /* cfg.tmvp_enable, cfg.max_merge (5 or 6: below 5 the reference's own list construction
                                              * overruns its array, src/inter.c:2028-2176), cfg.log2_parallel_merge_level */
  int32_t frame_qp;                /* state->frame->QP: the slice's context models are initialised with it */
  int32_t bipred, fme_level, early_skip;     /* cfg.bipred, cfg.fme_level, cfg.early_skip */
  int32_t depth_inter_min, depth_inter_max;  /* cfg.pu_depth_inter: 0, 3 */
  int32_t ref_stride, ref_stride_c, ref_motion_stride;
  int32_t inflight_margin;         /* 0: cfg.owf == 0, every vector inside the reference picture is legal (the pictures of a call and their references
                                    * are complete).  Else 1 + the in-loop filters' delay in samples (11 = 1 + SAO_DELAY_PX with cfg.sao_type, 9 with
                                    * deblocking only, 1 without filters; global.h:240-252): the search of an encoder with frames in flight, whose
                                    * vectors may not reach beyond what is final in a reference picture still being coded -- one CTU row below the
                                    * block's own, two CTUs down-right (fracmv_within_tile, src/search_inter.c:94-149; encoder.c:244-245) */
  const void *ref_y[16], *ref_u[16], *ref_v[16];
  const int32_t *ref_motion[16];
  uvghip_inter4_t *inter4;
  uint32_t *models_inter;
  uint32_t *trees;
  int32_t *motion_out;
} uvghip_ctu_pb_picture_t;
/* pictures: HOST array of n pictures that do not depend on each other (each one's references are complete: the pictures of several
 * sequences, or of one sequence's reference DAG at the same depth -- slice types, QPs and reference lists may differ).  workspace:
 * uvghip_ctu_search_pb_workspace_bytes of device memory, in use until the work enqueued on `stream` is done.  The call does not wait for
 * the stream: the picture table is written in stream order, then one launch of persistent one-wave workgroups (a few per CTU of a
 * picture's widest wavefront diagonal) that take CTU after CTU in an order that respects the left / upper / upper-right dependencies,
 * pictures interleaved.  params.rd: 0 or 1 (uvghip_ctu_params_t). */
UVGHIP_API size_t uvghip_ctu_search_pb_workspace_bytes(int n_pictures, int pic_w, int pic_h);
UVGHIP_API int uvghip_ctu_search_pb(int bitdepth, const uvghip_ctu_pb_picture_t *pictures, int n_pictures, void *workspace, void *stream);

/* replaces, for a group of independent P / B pictures: the whole per-picture loop of the CTU worker (src/encoderstate.c:808-976) --
 * uvghip_ctu_search_pb, then per picture uvghip_deblock_frame_sao_snapshot on a copy of the reconstruction + uvghip_sao_stats_batch,
 * uvghip_sao_decide_pictures_slice (the picture's QP, lambda and slice type), uvghip_deblock_frame in place on rec (boundary strengths
 * from the motion the search stored) + uvghip_sao_apply_batch into `out` -- the picture uvg_encoder_encode returns and the next pictures'
 * reference -- and uvghip_encode_slice_rows_pb.  sao_type: cfg.sao_type (0: no SAO, out = the deblocked picture).
 * uvghip_loop_pb_results: device pointers into the workspace -- SAO decisions [picture][ctu][34] / models [picture][ctu][6], the rows'
 * bytes (row r of picture p at rows + (p * n_rows + r) * row_cap) and lengths [picture][row].  The run waits for the stream between
 * pictures (the coder's table upload); everything else is enqueued. */
typedef struct uvghip_loop_pb_picture {
  uvghip_ctu_pb_picture_t search;
  void *out_y, *out_u, *out_v;
  int32_t out_stride, out_stride_c;     /* in samples */
} uvghip_loop_pb_picture_t;
UVGHIP_API size_t uvghip_loop_pb_workspace_bytes(int bitdepth, int n_pictures, int pic_w, int pic_h);
UVGHIP_API int uvghip_loop_pb_run(int bitdepth, const uvghip_loop_pb_picture_t *pictures, int n_pictures, int sao_type, void *workspace, void *stream);
UVGHIP_API int uvghip_loop_pb_results(int bitdepth, int n_pictures, int pic_w, int pic_h, void *workspace, const int32_t **sao_info,
                                      const uint16_t **sao_models, const uint8_t **rows, const int32_t **row_bytes, int *row_cap, int *n_rows);

/* The ALF stage behind uvghip_loop_pb_run, on the same pictures[] and loop workspace (what uvghip_loop_plan_alf_stage is behind
 * uvghip_loop_plan_run): per picture `decide` -- the same callback type, handed a uvghip_loop_picture_t view of search.pic and out_* (the
 * picture ALF gets = the loop's SAO output) -- then uvghip_alf_reconstruct_picture from out_* into alf_out[i] (a picture with nothing enabled
 * is copied), and per run of pictures with equal QP, lambda and slice type (the runs of uvghip_loop_pb_run)
 * uvghip_encode_slice_rows_pb_alf with the loop's SAO decisions: rows / row_bytes ([picture][row][row_cap] bytes, [picture][row] lengths;
 * device memory) replace the rows uvghip_loop_pb_run coded, which carry no ALF syntax.  sao_type, classification_shift: as in
 * uvghip_loop_pb_run / uvghip_loop_plan_alf_stage.  workspace: uvghip_loop_pb_alf_workspace_bytes of device memory.
 * alf_out[i] is the picture the encoder returns, hashes AND predicts from: pictures that reference picture i must be given alf_out[i] as
 * ref_y / ref_u / ref_v, not out_*.  So the stage of a picture runs before any picture that references it is issued; the derivation needs the
 * whole picture's statistics, which is why the in-flight entry points below take no ALF argument.
 * The call returns with the stream's work enqueued; it synchronises the stream between pictures (the decisions are host data). */
UVGHIP_API size_t uvghip_loop_pb_alf_workspace_bytes(int bitdepth, int n_pictures, int pic_w, int pic_h);
UVGHIP_API int uvghip_loop_pb_alf_stage(int bitdepth, const uvghip_loop_pb_picture_t *pictures, int n_pictures, int sao_type, void *loop_workspace,
                                        uvghip_alf_decide_fn decide, void *user, int classification_shift, const uvghip_alf_planes_t *alf_out, void *workspace,
                                        uint8_t *rows, int row_cap, int32_t *row_bytes, void *stream);

/* uvghip_loop_pb_run for pictures IN FLIGHT behind their references -- the encoder's --owf schedule (src/encoderstate.c:1060-1116: with
 * cfg.owf != 0 the search of CTU (x, y) of a picture waits for CTU (x + 2, y + 1) of its reference, clamped to the picture;
 * encoder.c:244-245 max_inter_ref_lcu = {1, 1}; its vectors stay inside what is final there, fracmv_within_tile src/search_inter.c:94-149
 * = inflight_margin).  The pictures of ONE call may refer to each other: they are given in coding order, ref_in_call[i * 16 + k] = the
 * index (< i) of the picture of this call whose OUTPUT picture reference k of picture i is (its out_* planes and search.motion_out), or -1
 * for a reference that is complete before the call.  The device waits for less than the reference and for enough: CTU (x, y) starts when
 * CTU (x + 1, y + 1) of every reference inside the call is FINAL ((x + 2, y) in the last CTU row) -- under the vector restriction nothing
 * beyond the CTUs (x + 2 + j, y - j), j >= 0, and (x + 1, y + 1) can be read, and a CTU's "final" flag is raised after its left, upper and
 * upper-right neighbour's, so that one flag covers exactly that shape.  Same pictures, same stream, a shorter wait.
 * One persistent launch for the search of the whole reference DAG of the call, every CTU running its in-loop filters right behind its
 * search (what encoder_state_worker_encode_lcu_search does after uvg_search_lcu, encoderstate.c:841-853: deblocking, uvg_sao_search_lcu's
 * statistics and decision, encoder_sao_reconstruct), so that the output picture becomes final CTU by CTU and a per-CTU flag releases the
 * CTUs of the pictures behind; then one launch of the arithmetic coder over all its pictures.  pic.rec_* stay unfiltered; the deblocked
 * pictures live in the workspace; out_* receive the picture uvg_encoder_encode returns (after SAO; sao_type 0: the deblocked picture).
 * Requirements beyond uvghip_ctu_search_pb: params.qp == params.qp_c == frame_qp; a picture with a reference inside the call has
 * inflight_margin = 11 (sao_type != 0) or 9.  The search launch has four waves per CTU (the walk, the 4x4 CUs of 8x8 areas, the 16x16 and
 * the 32x32 CUs on a wave each, ahead of the walk: csrc/ctu_pb.h; UVGHIP_PB_WAVES=1..4 for development) -- a CTU's latency, not the
 * device's occupancy, sets the pace of dependent pictures.  Results as uvghip_loop_pb_results.  Nothing waits for the stream. */
UVGHIP_API size_t uvghip_loop_pb_inflight_workspace_bytes(int bitdepth, int n_pictures, int pic_w, int pic_h);
UVGHIP_API int uvghip_loop_pb_run_inflight(int bitdepth, const uvghip_loop_pb_picture_t *pictures, int n_pictures, int sao_type, const int32_t *ref_in_call,
                                           void *workspace, void *stream);
UVGHIP_API int uvghip_loop_pb_inflight_results(int bitdepth, int n_pictures, int pic_w, int pic_h, void *workspace, const int32_t **sao_info,
                                               const uint16_t **sao_models, const uint8_t **rows, const int32_t **row_bytes, int *row_cap, int *n_rows);
/* ... with the clip's I pictures IN the flight: the first entries of `pictures` are the pictures of the all-intra loop plans `intra_plans`,
 * plan after plan, picture after picture.  The library fills those entries from the plans (the search's picture, the output planes); the
 * caller's are ignored and may be zero.  Their search runs in the plans' own launches -- a few persistent workgroups, one per CTU a picture's
 * wavefront can have in progress -- BESIDE the in-flight launch, which runs their filter stage CTU by CTU as they are searched, so that the
 * P / B pictures that refer to an I picture follow it four diagonals behind, as behind any other picture.  A picture that refers to one
 * names it in ref_in_call; its ref_motion is the caller's table for an intra picture (type 1 inside the picture, no vectors).
 * Results: an I picture's SAO decisions and slice data are its plan's (uvghip_loop_plan_results / _slice_data; its entries of this call's
 * result arrays stay unwritten), a P / B picture's as uvghip_loop_pb_inflight_results.  workspace:
 * uvghip_loop_pb_inflight_workspace_bytes of ALL n_pictures.  The plans' searches and the flight run on streams of the first plan's own,
 * forked from and joined to `stream`: work enqueued on `stream` afterwards sees all of it; nothing waits for the stream.  One such call
 * per plan at a time.  Refused before anything is enqueued: a NULL plan, a plan whose size, bit depth or sao_type differs from the call's,
 * fewer pictures than the plans hold, a ref_in_call entry that is not an earlier picture. */
UVGHIP_API int uvghip_loop_pb_run_inflight_intra(int bitdepth, uvghip_loop_plan_t *const *intra_plans, int n_plans, const uvghip_loop_pb_picture_t *pictures,
                                                 int n_pictures, int sao_type, const int32_t *ref_in_call, void *workspace, void *stream);
/* The slice data of an all-intra plan alone, from the SAO decisions in the plan's arrays (uvghip_loop_plan_results). */
UVGHIP_API int uvghip_loop_plan_run_coder(uvghip_loop_plan_t *plan, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* UVG266_HIP_H_ */
