// uvghip_loop_pb_*: one call per group of independent P / B pictures for the whole per-picture loop of the encoder's CTU worker
// (src/encoderstate.c:808-976): the closed-loop CTU search (uvghip_ctu_search_pb), then per picture the in-loop filters on the
// reference's schedule -- every CTU deblocked by its own edges only (what uvg_sao_search_lcu reads), SAO statistics and decisions with
// the slice type's models, deblocking of the reconstruction, SAO apply into the output picture (the next pictures' reference) -- and
// the slice data (uvghip_encode_slice_rows_pb).  Host code only: it strings the library's own entry points together on the caller's
// stream inside one workspace.
#include "uvghip_common.h"
#include <vector>
#include <cstring>

namespace {

struct layout_t { size_t search, snap, rects_y, rects_c, edge[3], band[3], decide, params[3], total; uvgi_coder_tail tail; };

// inflight: the layout of uvghip_loop_pb_run_inflight (below) -- the filters run inside the search launch, so none of the chain's tables,
// and `snap` holds the deblocked pictures
layout_t layout_of(int bitdepth, int n, int w, int h, bool inflight = false)
{
  const size_t ctus = (size_t)((w + 63) / 64) * ((h + 63) / 64), b = bitdepth == 8 ? 1 : 2;
  layout_t L;
  uvgi_carver c;
  L.search = c.take(uvghip_ctu_search_pb_workspace_bytes(n, w, h));
  L.snap = c.take((size_t)n * ((size_t)w * h * 3 / 2) * b);
  if (!inflight) {
    L.rects_y = c.take(ctus * sizeof(uvghip_rect_t));
    L.rects_c = c.take(ctus * sizeof(uvghip_rect_t));
    for (int k = 0; k < 3; ++k) { L.edge[k] = c.take((size_t)n * ctus * 40 * 4); L.band[k] = c.take((size_t)n * ctus * 64 * 4); }
    L.decide = c.take(uvghip_sao_decide_workspace_bytes(n, w, h));
  }
  L.tail.carve_sao(c, n, ctus);
  for (int k = 0; k < 3 && !inflight; ++k) L.params[k] = c.take((size_t)n * ctus * sizeof(uvghip_sao_param_t));
  L.tail.carve_rows(c, bitdepth, n, w, (size_t)((h + 63) / 64), uvghip_slice_rows_pb_workspace_bytes(n));
  L.total = c.at;
  return L;
}

// one body behind the two *_results entry points
int results_of(int bitdepth, int n_pictures, int pic_w, int pic_h, bool inflight, void *workspace, const char *who, const int32_t **sao_info, const uint16_t **sao_models,
               const uint8_t **rows, const int32_t **row_bytes, int *row_cap, int *n_rows)
{
  if ((bitdepth != 8 && bitdepth != 10) || n_pictures <= 0 || pic_w <= 0 || pic_h <= 0 || !workspace) return uvghip_set_error(hipErrorInvalidValue, who);
  const uvgi_coder_tail t = layout_of(bitdepth, n_pictures, pic_w, pic_h, inflight).tail;
  const unsigned char *ws = static_cast<const unsigned char *>(workspace);
  if (sao_info) *sao_info = reinterpret_cast<const int32_t *>(ws + t.info);
  if (sao_models) *sao_models = reinterpret_cast<const uint16_t *>(ws + t.models);
  if (rows) *rows = ws + t.rows;
  if (row_bytes) *row_bytes = reinterpret_cast<const int32_t *>(ws + t.row_bytes);
  if (row_cap) *row_cap = t.row_cap;
  if (n_rows) *n_rows = (pic_h + 63) / 64;
  return 0;
}

}  // namespace

extern "C" size_t uvghip_loop_pb_workspace_bytes(int bitdepth, int n_pictures, int pic_w, int pic_h)
{
  if ((bitdepth != 8 && bitdepth != 10) || n_pictures <= 0 || pic_w <= 0 || pic_h <= 0) return 0;
  return layout_of(bitdepth, n_pictures, pic_w, pic_h).total;
}

extern "C" int uvghip_loop_pb_results(int bitdepth, int n_pictures, int pic_w, int pic_h, void *workspace, const int32_t **sao_info, const uint16_t **sao_models,
                                      const uint8_t **rows, const int32_t **row_bytes, int *row_cap, int *n_rows)
{
  return results_of(bitdepth, n_pictures, pic_w, pic_h, false, workspace, __func__, sao_info, sao_models, rows, row_bytes, row_cap, n_rows);
}

extern "C" int uvghip_loop_pb_run(int bitdepth, const uvghip_loop_pb_picture_t *pictures, int n_pictures, int sao_type, void *workspace, void *stream)
{
  UVGHIP_REQUIRE_READY();
  UVGHIP_REQUIRE_DEPTH(bitdepth);
  if (!pictures || n_pictures <= 0 || !workspace || sao_type < 0 || sao_type > 3) return uvghip_set_error(hipErrorInvalidValue, __func__);
  const int w = pictures[0].search.params.pic_w, h = pictures[0].search.params.pic_h;
  if (w <= 0 || h <= 0) return uvghip_set_error(hipErrorInvalidValue, __func__);
  std::vector<uvghip_ctu_pb_picture_t> sp(n_pictures);
  for (int i = 0; i < n_pictures; ++i) {
    const uvghip_loop_pb_picture_t &q = pictures[i];
    if (int rc = uvgi_check_out_planes(q, w, "uvghip_loop_pb_run: output planes")) return rc;
    // the filters run without a chroma QP table (deblock.hip: identity)
    if (q.search.params.qp_c != q.search.params.qp) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_pb_run: qp_c != qp needs a chroma QP table");
    // The slice's context models start from frame_qp everywhere (uvg_init_contexts with state->frame->QP: the search, the coder); the SAO
    // decision below takes ONE QP for its models and its CTUs.  A picture whose CTUs' QP differs from the frame's (per-CTU QP offsets) is not
    // something this loop implements: refuse it instead of deciding SAO on other models than the coder's.
    if (q.search.params.qp != q.search.frame_qp) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_pb_run: params.qp differs from frame_qp");
    sp[i] = q.search;
  }
  const layout_t L = layout_of(bitdepth, n_pictures, w, h);
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  hipStream_t st = uvghip_stream(stream);
  if (int rc = uvghip_ctu_search_pb(bitdepth, sp.data(), n_pictures, ws + L.search, stream)) return rc;
  const int wc = (w + 63) / 64, hc = (h + 63) / 64, ctus = wc * hc, cw = w / 2, ch = h / 2;
  const size_t b = bitdepth == 8 ? 1 : 2;
  uvghip_rect_t *rects_y = reinterpret_cast<uvghip_rect_t *>(ws + L.rects_y), *rects_c = reinterpret_cast<uvghip_rect_t *>(ws + L.rects_c);
  {
    std::vector<uvghip_rect_t> ry(ctus), rc(ctus);
    for (int cy = 0; cy < hc; ++cy)
      for (int cx = 0; cx < wc; ++cx) {
        const int x = cx * 64, y = cy * 64, bw = x + 64 > w ? w - x : 64, bh = y + 64 > h ? h - y : 64;
        ry[cy * wc + cx] = uvghip_rect_t{x, y, bw, bh};
        rc[cy * wc + cx] = uvghip_rect_t{x / 2, y / 2, bw / 2, bh / 2};
      }
    // (in stream order: an earlier run on this workspace may still read the tables)
    if (int e = uvghip_upload_ordered(rects_y, ry.data(), ry.size() * sizeof(uvghip_rect_t), st)) return e;
    if (int e = uvghip_upload_ordered(rects_c, rc.data(), rc.size() * sizeof(uvghip_rect_t), st)) return e;
  }
  int32_t *edge[3], *band[3];
  uvghip_sao_param_t *prm[3];
  for (int c = 0; c < 3; ++c) {
    edge[c] = reinterpret_cast<int32_t *>(ws + L.edge[c]); band[c] = reinterpret_cast<int32_t *>(ws + L.band[c]);
    prm[c] = reinterpret_cast<uvghip_sao_param_t *>(ws + L.params[c]);
  }
  int32_t *sao_info = reinterpret_cast<int32_t *>(ws + L.tail.info), *row_bytes = reinterpret_cast<int32_t *>(ws + L.tail.row_bytes);
  uint16_t *sao_models = reinterpret_cast<uint16_t *>(ws + L.tail.models);
  const size_t snap_bytes = (size_t)w * h * 3 / 2 * b;
  // pictures that share QP, lambda and slice type (the same temporal position of several sequences) go through the SAO decision and
  // the coder together: runs of such pictures
  for (int i0 = 0; i0 < n_pictures;) {
    const uvghip_ctu_pb_picture_t &s0 = pictures[i0].search;
    int i1 = i0 + 1;
    while (i1 < n_pictures && pictures[i1].search.params.qp == s0.params.qp && pictures[i1].search.params.lambda == s0.params.lambda &&
           pictures[i1].search.slice_type == s0.slice_type && pictures[i1].search.frame_qp == s0.frame_qp)
      ++i1;
    const int m = i1 - i0, is_b = s0.slice_type == 0, qp = s0.params.qp;
    const size_t o0 = (size_t)i0 * ctus;
    if (sao_type) {
      for (int i = i0; i < i1; ++i) {
        const uvghip_ctu_picture_t &p = pictures[i].search.pic;
        unsigned char *sy = ws + L.snap + (size_t)i * snap_bytes, *su = sy + (size_t)w * h * b, *sv = su + (size_t)cw * ch * b;
        UVGHIP_TRY(hipMemcpy2DAsync(sy, (size_t)w * b, p.rec_y, (size_t)p.rec_stride * b, (size_t)w * b, h, hipMemcpyDeviceToDevice, st));
        UVGHIP_TRY(hipMemcpy2DAsync(su, (size_t)cw * b, p.rec_u, (size_t)p.rec_stride_c * b, (size_t)cw * b, ch, hipMemcpyDeviceToDevice, st));
        UVGHIP_TRY(hipMemcpy2DAsync(sv, (size_t)cw * b, p.rec_v, (size_t)p.rec_stride_c * b, (size_t)cw * b, ch, hipMemcpyDeviceToDevice, st));
        if (int rc = uvghip_deblock_frame_sao_snapshot(bitdepth, sy, w, su, sv, cw, w, h, p.cu, p.cu_stride, 0, 0, is_b, qp, nullptr, stream)) return rc;
        const size_t o = (size_t)i * ctus;
        if (int rc = uvghip_sao_stats_batch(bitdepth, p.src_y, p.src_stride, sy, w, rects_y, ctus, edge[0] + o * 40, band[0] + o * 64, stream)) return rc;
        if (int rc = uvghip_sao_stats_batch(bitdepth, p.src_u, p.src_stride_c, su, cw, rects_c, ctus, edge[1] + o * 40, band[1] + o * 64, stream)) return rc;
        if (int rc = uvghip_sao_stats_batch(bitdepth, p.src_v, p.src_stride_c, sv, cw, rects_c, ctus, edge[2] + o * 40, band[2] + o * 64, stream)) return rc;
      }
      if (int rc = uvghip_sao_decide_pictures_slice(bitdepth, m, w, h, qp, s0.params.lambda, sao_type, s0.slice_type, edge[0] + o0 * 40, band[0] + o0 * 64,
                                                    edge[1] + o0 * 40, band[1] + o0 * 64, edge[2] + o0 * 40, band[2] + o0 * 64,
                                                    ws + L.decide, sao_info + o0 * 34, sao_models + o0 * 6, prm[0] + o0, prm[1] + o0, prm[2] + o0, stream))
        return rc;
    }
    std::vector<uvghip_ctu_picture_t> cp(m);
    std::vector<uvghip_slice_pb_t> sl(m);
    for (int i = i0; i < i1; ++i) {
      const uvghip_loop_pb_picture_t &q = pictures[i];
      const uvghip_ctu_pb_picture_t &s = q.search;
      const uvghip_ctu_picture_t &p = s.pic;
      const size_t o = (size_t)i * ctus;
      if (int rc = uvghip_deblock_frame(bitdepth, p.rec_y, p.rec_stride, p.rec_u, p.rec_v, p.rec_stride_c, w, h, p.cu, p.cu_stride, 0, 0, is_b, qp, nullptr, stream)) return rc;
      if (sao_type) {
        if (int rc = uvghip_sao_apply_batch(bitdepth, p.rec_y, p.rec_stride, q.out_y, q.out_stride, w, h, rects_y, prm[0] + o, ctus, stream)) return rc;
        if (int rc = uvghip_sao_apply_batch(bitdepth, p.rec_u, p.rec_stride_c, q.out_u, q.out_stride_c, cw, ch, rects_c, prm[1] + o, ctus, stream)) return rc;
        if (int rc = uvghip_sao_apply_batch(bitdepth, p.rec_v, p.rec_stride_c, q.out_v, q.out_stride_c, cw, ch, rects_c, prm[2] + o, ctus, stream)) return rc;
      } else {
        UVGHIP_TRY(hipMemcpy2DAsync(q.out_y, (size_t)q.out_stride * b, p.rec_y, (size_t)p.rec_stride * b, (size_t)w * b, h, hipMemcpyDeviceToDevice, st));
        UVGHIP_TRY(hipMemcpy2DAsync(q.out_u, (size_t)q.out_stride_c * b, p.rec_u, (size_t)p.rec_stride_c * b, (size_t)cw * b, ch, hipMemcpyDeviceToDevice, st));
        UVGHIP_TRY(hipMemcpy2DAsync(q.out_v, (size_t)q.out_stride_c * b, p.rec_v, (size_t)p.rec_stride_c * b, (size_t)cw * b, ch, hipMemcpyDeviceToDevice, st));
      }
      cp[i - i0] = p;
      sl[i - i0] = uvgi_slice_pb_of(s);
    }
    // the slice data of the run's pictures: the search's hand-over and the SAO decisions through the arithmetic coder (its tables are
    // uploaded in stream order: a later run's upload comes after the earlier run's coder on the stream)
    if (int rc = uvghip_encode_slice_rows_pb(bitdepth, &s0.params, cp.data(), sl.data(), m, sao_type ? sao_info + o0 * 34 : nullptr, sao_type ? sao_models + o0 * 6 : nullptr,
                                             ws + L.tail.coder, ws + L.tail.rows + (size_t)i0 * hc * L.tail.row_cap, L.tail.row_cap, row_bytes + (size_t)i0 * hc, stream))
      return rc;
    i0 = i1;
  }
  return 0;
}

// ---- the ALF stage behind uvghip_loop_pb_run (BASELINE configs[3]: --gop 16 --alf full), on the same pictures and loop workspace: where the
// encoder runs uvg_alf_enc_process (src/alf.c:5193) on a P / B picture and then codes its CTUs for real (src/encoderstate.c:1043-1052).  The
// decisions come from the caller's `decide` as in uvghip_loop_plan_alf_stage; alf_out[i] is what later pictures predict from. ----
namespace {
struct alf_layout_t { size_t rec, coder, flags, per, total; };
alf_layout_t alf_layout_of(int n, int w, int h)
{
  const size_t ctus = (size_t)((w + 63) / 64) * ((h + 63) / 64);
  alf_layout_t A;
  uvgi_carver c;
  A.rec = c.take(uvghip_alf_reconstruct_workspace_bytes(w, h));
  A.coder = c.take(uvghip_slice_rows_pb_alf_workspace_bytes(n));
  A.per = uvgi_align_up(ctus * 7 + (ctus & 1) + ctus * sizeof(int16_t), 256);          // per picture: ctu_flags [7][ctus], filter_set_idx [ctus]
  A.flags = c.take((size_t)n * A.per);
  A.total = c.at;
  return A;
}
}  // namespace

extern "C" size_t uvghip_loop_pb_alf_workspace_bytes(int bitdepth, int n_pictures, int pic_w, int pic_h)
{
  if ((bitdepth != 8 && bitdepth != 10) || n_pictures <= 0 || pic_w <= 0 || pic_h <= 0) return 0;
  return alf_layout_of(n_pictures, pic_w, pic_h).total;
}

extern "C" int uvghip_loop_pb_alf_stage(int bitdepth, const uvghip_loop_pb_picture_t *pictures, int n_pictures, int sao_type, void *loop_workspace, uvghip_alf_decide_fn decide,
                                        void *user, int classification_shift, const uvghip_alf_planes_t *alf_out, void *workspace, uint8_t *rows, int row_cap, int32_t *row_bytes,
                                        void *stream)
{
  UVGHIP_REQUIRE_READY();
  UVGHIP_REQUIRE_DEPTH(bitdepth);
  if (!pictures || n_pictures <= 0 || sao_type < 0 || sao_type > 3 || !loop_workspace || !decide || !alf_out || !workspace || !rows || row_cap <= 0 || !row_bytes ||
      classification_shift < 8 || classification_shift > 20)
    return uvghip_set_error(hipErrorInvalidValue, __func__);
  const int w = pictures[0].search.params.pic_w, h = pictures[0].search.params.pic_h;
  if (w <= 0 || h <= 0) return uvghip_set_error(hipErrorInvalidValue, __func__);
  const layout_t L = layout_of(bitdepth, n_pictures, w, h);
  const alf_layout_t A = alf_layout_of(n_pictures, w, h);
  const unsigned char *lws = static_cast<const unsigned char *>(loop_workspace);
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  hipStream_t st = uvghip_stream(stream);
  const int wc = (w + 63) / 64, hc = (h + 63) / 64, ctus = wc * hc;
  const size_t b = bitdepth == 8 ? 1 : 2;
  const int32_t *sao_info = reinterpret_cast<const int32_t *>(lws + L.tail.info);
  const uint16_t *sao_models = reinterpret_cast<const uint16_t *>(lws + L.tail.models);
  std::vector<uvghip_slice_alf_t> sa(n_pictures);
  for (int i = 0; i < n_pictures; ++i) {
    const uvghip_loop_pb_picture_t &q = pictures[i];
    const uvghip_alf_planes_t &o = alf_out[i];
    if (q.search.params.pic_w != w || q.search.params.pic_h != h) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_pb_alf_stage: a picture's size differs from the first one's");
    if (int rc = uvgi_check_out_planes(q, w, "uvghip_loop_pb_alf_stage: the loop's output planes")) return rc;
    if (!o.y || !o.u || !o.v || o.stride < w || o.stride_c < w / 2) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_pb_alf_stage: output planes");
    uvghip_loop_picture_t view;
    memset(&view, 0, sizeof view);
    view.search = q.search.pic;
    view.out_y = q.out_y; view.out_u = q.out_u; view.out_v = q.out_v; view.out_stride = q.out_stride; view.out_stride_c = q.out_stride_c;
    uvghip_alf_decision_t d;
    memset(&d, 0, sizeof d);
    if (int rc = decide(user, i, &view, &d)) return uvghip_set_error(hipErrorInvalidValue, rc > 0 ? "uvghip_loop_pb_alf_stage: decide() failed" : "uvghip_loop_pb_alf_stage: decide() refused");
    const bool any = d.enabled[0] || d.enabled[1] || d.enabled[2] || d.cc_enabled[0] || d.cc_enabled[1];
    if ((d.alf_type != 1 && d.alf_type != 2) || d.n_luma_aps < 0 || d.n_luma_aps > 8 || (any && (!d.ctu_flags || !d.filter_set_idx)) || (d.n_luma_aps && !d.luma_aps) ||
        ((d.enabled[1] || d.enabled[2]) && !d.chroma_aps) || ((d.cc_enabled[0] || d.cc_enabled[1]) && !d.cc_coeff))
      return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_pb_alf_stage: the decision decide() returned");
    if (any) {
      uvghip_alf_picture_t a;
      memset(&a, 0, sizeof a);
      a.in_y = q.out_y; a.in_u = q.out_u; a.in_v = q.out_v; a.in_stride = q.out_stride; a.in_stride_c = q.out_stride_c;
      a.out_y = o.y; a.out_u = o.u; a.out_v = o.v; a.out_stride = o.stride; a.out_stride_c = o.stride_c;
      a.width = w; a.height = h;
      for (int c = 0; c < 3; ++c) a.slice_enabled[c] = d.enabled[c];
      a.n_luma_aps = d.n_luma_aps; a.ctu_flags = d.ctu_flags; a.filter_set_idx = d.filter_set_idx; a.luma_aps = d.luma_aps; a.chroma_aps = d.chroma_aps;
      a.alf_full = d.alf_type == 2; a.cc_alf_enabled[0] = d.cc_enabled[0]; a.cc_alf_enabled[1] = d.cc_enabled[1]; a.cc_coeff = d.cc_coeff;
      a.classification_shift = classification_shift;
      if (int rc = uvghip_alf_reconstruct_picture(bitdepth, &a, ws + A.rec, stream)) return rc;
    } else {          // a picture ALF leaves alone
      UVGHIP_TRY(hipMemcpy2DAsync(o.y, (size_t)o.stride * b, q.out_y, (size_t)q.out_stride * b, (size_t)w * b, h, hipMemcpyDeviceToDevice, st));
      UVGHIP_TRY(hipMemcpy2DAsync(o.u, (size_t)o.stride_c * b, q.out_u, (size_t)q.out_stride_c * b, (size_t)(w / 2) * b, h / 2, hipMemcpyDeviceToDevice, st));
      UVGHIP_TRY(hipMemcpy2DAsync(o.v, (size_t)o.stride_c * b, q.out_v, (size_t)q.out_stride_c * b, (size_t)(w / 2) * b, h / 2, hipMemcpyDeviceToDevice, st));
    }
    // the slice's side of the decision: the flags and set indices on the device, where the coder reads them
    uvghip_slice_alf_t &s = sa[i];
    memset(&s, 0, sizeof s);
    s.alf_type = d.alf_type; s.n_luma_aps = d.n_luma_aps; s.n_alternatives_chroma = d.chroma_aps ? d.chroma_aps[112] : 0;
    for (int c = 0; c < 3; ++c) s.enabled[c] = d.enabled[c];
    for (int c = 0; c < 2; ++c) { s.cc_enabled[c] = d.cc_enabled[c]; s.cc_filter_count[c] = d.cc_filter_count[c]; }
    if (any) {
      unsigned char *fl = ws + A.flags + (size_t)i * A.per, *si = fl + (size_t)ctus * 7 + ((size_t)ctus & 1);
      UVGHIP_TRY(hipMemcpyAsync(fl, d.ctu_flags, (size_t)ctus * 7, hipMemcpyHostToDevice, st));
      UVGHIP_TRY(hipMemcpyAsync(si, d.filter_set_idx, (size_t)ctus * sizeof(int16_t), hipMemcpyHostToDevice, st));
      UVGHIP_TRY(hipStreamSynchronize(st));          // (decide()'s arrays need not outlive the next call)
      s.ctu_flags = fl; s.filter_set_idx = reinterpret_cast<const int16_t *>(si);
    }
  }
  // the slice data, run by run as uvghip_loop_pb_run codes it (pictures that share QP, lambda and slice type)
  for (int i0 = 0; i0 < n_pictures;) {
    const uvghip_ctu_pb_picture_t &s0 = pictures[i0].search;
    int i1 = i0 + 1;
    while (i1 < n_pictures && pictures[i1].search.params.qp == s0.params.qp && pictures[i1].search.params.lambda == s0.params.lambda &&
           pictures[i1].search.slice_type == s0.slice_type && pictures[i1].search.frame_qp == s0.frame_qp)
      ++i1;
    const int m = i1 - i0;
    const size_t o0 = (size_t)i0 * ctus;
    std::vector<uvghip_ctu_picture_t> cp(m);
    std::vector<uvghip_slice_pb_t> sl(m);
    for (int i = i0; i < i1; ++i) {
      cp[i - i0] = pictures[i].search.pic; sl[i - i0] = uvgi_slice_pb_of(pictures[i].search);
      sl[i - i0].second_pass = 1;          // the encoder's real coding pass behind ALF follows a simulated one (uvghip_slice_pb_t)
    }
    if (int rc = uvghip_encode_slice_rows_pb_alf(bitdepth, &s0.params, cp.data(), sl.data(), sa.data() + i0, m, sao_type ? sao_info + o0 * 34 : nullptr,
                                                 sao_type ? sao_models + o0 * 6 : nullptr, ws + A.coder, rows + (size_t)i0 * hc * row_cap, row_cap, row_bytes + (size_t)i0 * hc, stream))
      return rc;
    i0 = i1;
  }
  return 0;
}

// ---- pictures in flight behind their references: one call = one persistent launch for the whole DAG (uvgi_search_pb_inflight: the
// search with the per-CTU filters inside), then ONE coder launch over all pictures -- their QPs, lambdas and slice types may differ ----
extern "C" size_t uvghip_loop_pb_inflight_workspace_bytes(int bitdepth, int n_pictures, int pic_w, int pic_h)
{
  if ((bitdepth != 8 && bitdepth != 10) || n_pictures <= 0 || pic_w <= 0 || pic_h <= 0) return 0;
  return layout_of(bitdepth, n_pictures, pic_w, pic_h, true).total;
}

extern "C" int uvghip_loop_pb_inflight_results(int bitdepth, int n_pictures, int pic_w, int pic_h, void *workspace, const int32_t **sao_info, const uint16_t **sao_models,
                                               const uint8_t **rows, const int32_t **row_bytes, int *row_cap, int *n_rows)
{
  return results_of(bitdepth, n_pictures, pic_w, pic_h, true, workspace, __func__, sao_info, sao_models, rows, row_bytes, row_cap, n_rows);
}

namespace {
// A picture of the flight whose SEARCH runs in another launch beside it (an I picture of an all-intra plan, uvgi_ctu_plan_launch on another
// stream): that launch's per-CTU "searched" flags [ctus] and where the picture's SAO decisions go ([ctus][34] / [ctus][6], the plan's arrays,
// which its coder reads).
struct external_t { const int32_t *searched_flags; int32_t *sao_info; uint16_t *sao_models; };

// The flight on `stream`: the in-flight launch, then the coder over the pictures it searched.  The first n_ext pictures are searched
// elsewhere (ext[0 .. n_ext)): the launch filters them CTU by CTU as that launch finishes their CTUs, so that the P / B pictures behind them
// are in flight behind an I picture as behind any other; they get no slice data here.  The caller's duties (uvgi_search_pb_inflight): that
// launch is already LAUNCHED, its flags were zeroed in stream order before this stream's position, and other_workgroups is its grid.
int run_flight(int bitdepth, const uvghip_loop_pb_picture_t *pictures, int n_pictures, int sao_type, const int32_t *ref_in_call, const external_t *ext, int n_ext,
               int other_workgroups, void *workspace, void *stream)
{
  UVGHIP_REQUIRE_READY();
  UVGHIP_REQUIRE_DEPTH(bitdepth);
  if (!pictures || n_pictures <= 0 || !workspace || !ref_in_call || sao_type < 0 || sao_type > 3) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_pb_run_inflight");
  const int w = pictures[0].search.params.pic_w, h = pictures[0].search.params.pic_h;
  if (w <= 0 || h <= 0) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_pb_run_inflight");
  const layout_t L = layout_of(bitdepth, n_pictures, w, h, true);
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  const int wc = (w + 63) / 64, hc = (h + 63) / 64, ctus = wc * hc;
  const size_t planes = (size_t)w * h * (bitdepth == 8 ? 1 : 2) * 3 / 2;
  int32_t *sao_info = reinterpret_cast<int32_t *>(ws + L.tail.info), *row_bytes = reinterpret_cast<int32_t *>(ws + L.tail.row_bytes);
  uint16_t *sao_models = reinterpret_cast<uint16_t *>(ws + L.tail.models);
  std::vector<uvghip_ctu_pb_picture_t> sp(n_pictures);
  std::vector<uvgi_pb_filter> fl(n_pictures);
  std::vector<uvghip_ctu_picture_t> cp(n_pictures);
  std::vector<uvghip_slice_pb_t> sl(n_pictures);
  std::vector<const int32_t *> flags(n_pictures, nullptr);
  for (int i = 0; i < n_pictures; ++i) {
    const uvghip_loop_pb_picture_t &q = pictures[i];
    const uvghip_ctu_pb_picture_t &s = q.search;
    if (int rc = uvgi_check_out_planes(q, w, "uvghip_loop_pb_run_inflight: output planes")) return rc;
    sp[i] = s;
    if (i < n_ext) flags[i] = ext[i].searched_flags;
    fl[i] = uvgi_pb_filter_of(q, ws + L.snap + (size_t)i * planes, bitdepth, w, h, i < n_ext ? ext[i].sao_info : sao_info + (size_t)i * ctus * 34,
                              i < n_ext ? ext[i].sao_models : sao_models + (size_t)i * ctus * 6, sao_type);
    cp[i] = s.pic;
    if (i >= n_ext) sl[i] = uvgi_slice_pb_of(s);          // (the others are not coded here)
  }
  if (int rc = uvgi_search_pb_inflight(bitdepth, sp.data(), fl.data(), ref_in_call, n_ext ? flags.data() : nullptr, other_workgroups, n_pictures, ws + L.search, stream))
    return rc;
  if (n_ext == n_pictures) return 0;
  // the slice data of every picture it searched in one launch (a P / B picture's models start from its own frame_qp and slice type: `params`
  // only names the size); they keep their place in the results' arrays
  return uvghip_encode_slice_rows_pb(bitdepth, &pictures[n_ext].search.params, cp.data() + n_ext, sl.data() + n_ext, n_pictures - n_ext,
                                     sao_type ? sao_info + (size_t)n_ext * ctus * 34 : nullptr, sao_type ? sao_models + (size_t)n_ext * ctus * 6 : nullptr, ws + L.tail.coder,
                                     ws + L.tail.rows + (size_t)n_ext * hc * L.tail.row_cap, L.tail.row_cap, row_bytes + (size_t)n_ext * hc, stream);
}
}  // namespace

extern "C" int uvghip_loop_pb_run_inflight(int bitdepth, const uvghip_loop_pb_picture_t *pictures, int n_pictures, int sao_type, const int32_t *ref_in_call, void *workspace,
                                           void *stream)
{
  return run_flight(bitdepth, pictures, n_pictures, sao_type, ref_in_call, nullptr, 0, 0, workspace, stream);
}

// ---- ... with the I pictures of the clip IN the flight: searched by their all-intra plans on one stream of the first plan's own BESIDE the
// flight on the other, which filters them CTU by CTU as they are searched; their slice data behind their search, beside the flight.  The
// whole stream order is here; the order of the steps below is what keeps a kernel from waiting for flags that are not zero yet, or for a
// launch that is not in the queue.
extern "C" int uvghip_loop_pb_run_inflight_intra(int bitdepth, uvghip_loop_plan_t *const *intra_plans, int n_plans, const uvghip_loop_pb_picture_t *pictures, int n_pictures,
                                                 int sao_type, const int32_t *ref_in_call, void *workspace, void *stream)
{
  UVGHIP_REQUIRE_READY();
  UVGHIP_REQUIRE_DEPTH(bitdepth);
  if (!intra_plans || n_plans <= 0 || !intra_plans[0] || !pictures || n_pictures <= 0 || !workspace || !ref_in_call) return uvghip_set_error(hipErrorInvalidValue, __func__);
  uvghip_loop_plan *const p0 = intra_plans[0];
  const int w = p0->w, h = p0->h, ctus = p0->ctus, wc = (w + 63) / 64, per = wc < p0->hc ? wc : p0->hc;
  // everything that can be refused is refused before anything is enqueued
  int n_intra = 0, other_workgroups = 0;
  for (int k = 0; k < n_plans; ++k) {
    const uvghip_loop_plan *pl = intra_plans[k];
    if (!pl || pl->bitdepth != bitdepth || pl->w != w || pl->h != h || pl->sao_type != sao_type)
      return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_pb_run_inflight_intra: a plan's size, bit depth or sao_type differs from the call's");
    if (pl->row0 > 0 || pl->row1 < pl->hc) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_pb_run_inflight_intra: a band plan (uvghip_loop_plan_create_rows) holds a part of its pictures");
    n_intra += pl->n;
    // the plan's launch beside the flight, whose workgroups take whole CUs: one workgroup per CTU the pictures' wavefronts can have in progress
    // (more only wait and take CUs from the flight), which the flight leaves the CUs for
    other_workgroups += pl->n * (per < ctus ? per : ctus);
  }
  if (n_pictures < n_intra) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_pb_run_inflight_intra: fewer pictures than the plans hold");
  if (other_workgroups > uvgi_flight_other_max) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_pb_run_inflight_intra: the plans' launches need more than 512 workgroups");
  for (int i = n_intra; i < n_pictures; ++i) {
    if (pictures[i].search.params.pic_w != w || pictures[i].search.params.pic_h != h)
      return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_pb_run_inflight_intra: a picture's size differs from the plans'");
    for (int k = 0; k < 16 && k < pictures[i].search.n_refs; ++k)
      if (ref_in_call[(size_t)i * 16 + k] >= i) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_pb_run_inflight_intra: a reference inside the call must be an earlier picture of it");
  }
  // the I entries from the plans: the search's picture, the output planes, the SAO arrays, the searched flags
  std::vector<uvghip_loop_pb_picture_t> pics(pictures, pictures + n_pictures);
  std::vector<external_t> ext(n_intra);
  for (int k = 0, at = 0; k < n_plans; ++k) {
    uvghip_loop_plan *pl = intra_plans[k];
    if (ctus > per)          // (else the plan keeps its workgroup per CTU)
      if (int rc = uvgi_ctu_plan_set_grid(pl->search, per * pl->n)) return rc;
    for (int j = 0; j < pl->n; ++j, ++at) {
      const uvghip_loop_picture_t &p = pl->pics[j];
      uvghip_loop_pb_picture_t &q = pics[at];
      memset(&q, 0, sizeof q);
      q.search.params = pl->ctu_params; q.search.pic = p.search; q.search.slice_type = 2;
      q.out_y = p.out_y; q.out_u = p.out_u; q.out_v = p.out_v; q.out_stride = p.out_stride; q.out_stride_c = p.out_stride_c;
      ext[at] = external_t{uvgi_ctu_plan_done_flags(pl->search) + (size_t)j * ctus, pl->sao_info + (size_t)j * ctus * 34, pl->sao_models + (size_t)j * ctus * 6};
    }
  }
  if (int rc = uvgi_loop_plan_side_streams(p0)) return rc;
  hipStream_t st = uvghip_stream(stream), intra = p0->side[0], flight = p0->side[1];
  // 1. both sides behind the caller's stream
  UVGHIP_TRY(hipEventRecord(p0->ev_fork, st));
  UVGHIP_TRY(hipStreamWaitEvent(intra, p0->ev_fork, 0));
  UVGHIP_TRY(hipStreamWaitEvent(flight, p0->ev_fork, 0));
  // 2. the I pictures' "final" flags (which their coder waits for, behind the search on the I side) and the plans' "searched" flags to zero;
  //    the flight behind that: its kernel must not look at them before
  const layout_t L = layout_of(bitdepth, n_pictures, w, h, true);
  int32_t *final_flags = const_cast<int32_t *>(uvgi_search_pb_inflight_final_flags(n_pictures, w, h, static_cast<unsigned char *>(workspace) + L.search));
  UVGHIP_TRY(hipMemsetAsync(final_flags, 0, (size_t)n_intra * ctus * sizeof(int32_t), intra));
  for (int k = 0; k < n_plans; ++k)
    if (int rc = uvgi_ctu_plan_reset(intra_plans[k]->search, intra)) return rc;
  UVGHIP_TRY(hipEventRecord(p0->ev_side[0], intra));
  UVGHIP_TRY(hipStreamWaitEvent(flight, p0->ev_side[0], 0));
  // 3. the searches, in the queue BEFORE the flight that waits for them
  for (int k = 0; k < n_plans; ++k)
    if (int rc = uvgi_ctu_plan_launch(intra_plans[k]->search, intra)) return rc;
  // 4. the flight: the I pictures' filters, the P / B pictures and their slice data
  int rc = run_flight(bitdepth, pics.data(), n_pictures, sao_type, ref_in_call, ext.data(), n_intra, other_workgroups, workspace, flight);
  // 5. the I pictures' slice data behind their search, BESIDE the flight: a row waits, CTU by CTU, for the flight's filter stage
  //    (not when the flight was refused: nothing would raise the flags)
  for (int k = 0, first = 0; k < n_plans && !rc; first += intra_plans[k++]->n) {
    const uvghip_loop_plan *pl = intra_plans[k];
    rc = uvgi_encode_slice_rows_behind(bitdepth, &pl->ctu_params, pl->n, pl->sao_info, pl->sao_models, final_flags + (size_t)first * ctus, nullptr, 0, pl->coder_ws, pl->rows,
                                       pl->row_cap, pl->row_bytes, intra);
  }
  // 6. the flight waits for the I side, the caller's stream for the flight
  UVGHIP_TRY(hipEventRecord(p0->ev_side[1], intra));
  UVGHIP_TRY(hipStreamWaitEvent(flight, p0->ev_side[1], 0));
  UVGHIP_TRY(hipEventRecord(p0->ev_fork, flight));
  UVGHIP_TRY(hipStreamWaitEvent(st, p0->ev_fork, 0));
  return rc;
}
