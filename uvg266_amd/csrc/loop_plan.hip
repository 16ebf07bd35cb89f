// uvghip_loop_plan_*: one call per group of all-intra pictures for the whole per-picture loop of the encoder's CTU worker
// (src/encoderstate.c:808-976 without the bitstream writer): the closed-loop CTU search, then the in-loop filters on the
// reference's own schedule -- every CTU deblocked by its own edges only (what uvg_sao_search_lcu reads), SAO statistics, the
// SAO decision of every CTU of every picture, deblocking of the reconstruction, SAO apply.  Host code only: a plan strings the
// library's own entry points together on the caller's stream and owns the tables they need.
#include "uvghip_common.h"
#include <new>
#include <vector>
#include <cstring>

namespace {

struct layout_t { size_t search, snap, sums, filt, tick, total; uvgi_coder_tail tail; };

layout_t layout_of(int bitdepth, int n, int w, int h)
{
  layout_t L;
  uvgi_carver c;
  L.search = c.take(uvghip_ctu_search_workspace_bytes(n, w, h));
  L.snap = c.take((size_t)n * ((size_t)w * h * 3 / 2) * (bitdepth == 8 ? 1 : 2));
  const size_t hc = (size_t)((h + 63) / 64);
  L.tail.carve_sao(c, n, (size_t)((w + 63) / 64) * hc);
  L.tail.carve_rows(c, bitdepth, n, w, hc, uvghip_slice_rows_workspace_bytes(n));
  L.sums = c.take((size_t)n * 3 * sizeof(uint32_t));
  L.filt = c.take(uvgi_filter_workspace_bytes(n, w, h));
  L.tick = c.take(256);
  L.total = c.at;
  return L;
}

}  // namespace

extern "C" size_t uvghip_loop_workspace_bytes(int bitdepth, int n_pictures, int pic_w, int pic_h)
{
  if ((bitdepth != 8 && bitdepth != 10) || n_pictures <= 0 || pic_w <= 0 || pic_h <= 0) return 0;
  return layout_of(bitdepth, n_pictures, pic_w, pic_h).total;
}

extern "C" int uvghip_loop_plan_create(int bitdepth, const uvghip_ctu_params_t *params, const uvghip_loop_picture_t *pictures, int n_pictures,
                                       int sao_type, void *workspace, uvghip_loop_plan_t **plan_out)
{
  UVGHIP_REQUIRE_READY();
  UVGHIP_REQUIRE_DEPTH(bitdepth);
  if (!params || !pictures || n_pictures <= 0 || !workspace || !plan_out || sao_type < 1 || sao_type > 3)
    return uvghip_set_error(hipErrorInvalidValue, __func__);
  return uvghip_loop_plan_create_rows(bitdepth, params, pictures, n_pictures, sao_type, 0, (params->pic_h + 63) / 64, workspace, plan_out);
}

namespace {
// The hand-over of a band plan at the boundary above CTU row `b` (side 0: b = row0, the plan receives; side 1: b = row1, it sends): kind
// after kind, inside a kind picture after picture -- the order of the packed message.  Every extent is what the three launches read of
// the row above: ctu_filter.h (tile from 64 cy - 16; F from 64 cy - delay with the edge classes' row above it, D from 64 cy - 8;
// sao_region's decisions of the CTU row the rows lie in; the merge candidates and the models of the chain), slice_coder.hip (one unit row
// of border, the row's start models, its SAO models), ctu_search.hip (the last line, the last unit row, the models).
void halo_list(const uvghip_loop_plan *pl, const unsigned char *snap, int b, std::vector<uvghip_halo_piece_t> &out, std::vector<size_t> &at, size_t &total)
{
  const size_t bps = pl->bitdepth == 8 ? 1 : 2;
  const int w = pl->w, wc = (w + 63) / 64, Y = 64 * b;
  const size_t plane = (size_t)w * pl->h * bps, planes = plane * 3 / 2;
  total = 0;
  auto add = [&](void *base, size_t pitch, size_t first_row, int rows, size_t row_bytes) {
    out.push_back(uvghip_halo_piece_t{static_cast<unsigned char *>(base) + first_row * pitch, row_bytes, pitch, rows, 0});
    at.push_back(total);
    total += row_bytes * rows;
  };
  const int n = pl->n;
  for (int i = 0; i < n; ++i) { const uvghip_ctu_picture_t &q = pl->pics[i].search; add(q.rec_y, q.rec_stride * bps, Y - 16, 16, w * bps); }
  for (int i = 0; i < n; ++i) { const uvghip_ctu_picture_t &q = pl->pics[i].search; add(q.rec_u, q.rec_stride_c * bps, Y / 2 - 8, 8, w / 2 * bps); }
  for (int i = 0; i < n; ++i) { const uvghip_ctu_picture_t &q = pl->pics[i].search; add(q.rec_v, q.rec_stride_c * bps, Y / 2 - 8, 8, w / 2 * bps); }
  for (int i = 0; i < n; ++i) { const uvghip_ctu_picture_t &q = pl->pics[i].search; add(q.cu, (size_t)q.cu_stride * sizeof(uvghip_scu_t), Y / 4 - 4, 4, (size_t)wc * 16 * sizeof(uvghip_scu_t)); }
  if (pl->sao_type) {
    for (int i = 0; i < n; ++i) add(const_cast<unsigned char *>(snap) + (size_t)i * planes, w * bps, Y - 11, 3, w * bps);
    for (int i = 0; i < n; ++i) add(const_cast<unsigned char *>(snap) + (size_t)i * planes + plane, w / 2 * bps, Y / 2 - 6, 2, w / 2 * bps);
    for (int i = 0; i < n; ++i) add(const_cast<unsigned char *>(snap) + (size_t)i * planes + plane + plane / 4, w / 2 * bps, Y / 2 - 6, 2, w / 2 * bps);
    for (int i = 0; i < n; ++i) add(pl->sao_info + (size_t)i * pl->ctus * 34, (size_t)wc * 34 * 4, b - 1, 1, (size_t)wc * 34 * 4);
  }
  const size_t mrow = (size_t)UVGHIP_CTU_MODELS * 4;          // a model set; the third set of CTU k is row 3 k + 2
  for (int i = 0; i < n; ++i) add(pl->pics[i].search.models, mrow, (size_t)(b - 1) * wc * 3 + 2, 1, mrow);
  if (pl->sao_type)
    for (int i = 0; i < n; ++i) add(pl->sao_models + (size_t)i * pl->ctus * 6, 12, (size_t)(b - 1) * wc, 1, 12);
}

// The pack / unpack kernels: plain copies, one workgroup per (piece, row) -- grid.x the piece, grid.y the row (a piece has at most 16) --
// between a piece's row and its place in the message.  16 bytes per lane where both addresses allow (planes and the side information of
// the usual sizes: every lane of a wave in one 1 KB stretch), else 4 bytes, else bytes; the remainder of a row byte by byte.
struct halo_dev_piece { unsigned char *ptr; unsigned long long pitch, row_bytes, at; int rows, pad; };

template <bool PACK>
__global__ void __launch_bounds__(256) halo_copy_kernel(const halo_dev_piece *__restrict__ pieces, unsigned char *__restrict__ message)
{
  const halo_dev_piece P = pieces[blockIdx.x];
  const int r = blockIdx.y;
  if (r >= P.rows) return;
  unsigned char *plane = P.ptr + (size_t)r * P.pitch, *msg = message + P.at + (size_t)r * P.row_bytes;
  const unsigned char *src = PACK ? plane : msg;
  unsigned char *dst = PACK ? msg : plane;
  const size_t nb = P.row_bytes;
  const unsigned long long both = (unsigned long long)(uintptr_t)src | (unsigned long long)(uintptr_t)dst;
  size_t done = 0;
  if (!(both & 15)) {
    const size_t nv = nb >> 4;
    for (size_t i = threadIdx.x; i < nv; i += blockDim.x) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src)[i];
    done = nv << 4;
  } else if (!(both & 3)) {
    const size_t nv = nb >> 2;
    for (size_t i = threadIdx.x; i < nv; i += blockDim.x) reinterpret_cast<uint32_t *>(dst)[i] = reinterpret_cast<const uint32_t *>(src)[i];
    done = nv << 2;
  }
  for (size_t i = done + threadIdx.x; i < nb; i += blockDim.x) dst[i] = src[i];
}
}  // namespace

extern "C" int uvghip_loop_plan_create_rows(int bitdepth, const uvghip_ctu_params_t *params, const uvghip_loop_picture_t *pictures, int n_pictures,
                                            int sao_type, int ctu_row0, int ctu_row1, void *workspace, uvghip_loop_plan_t **plan_out)
{
  UVGHIP_REQUIRE_READY();
  UVGHIP_REQUIRE_DEPTH(bitdepth);
  if (!params || !pictures || n_pictures <= 0 || !workspace || !plan_out || sao_type < 0 || sao_type > 3)
    return uvghip_set_error(hipErrorInvalidValue, __func__);
  const int w = params->pic_w, h = params->pic_h;
  if (w <= 0 || h <= 0 || ctu_row0 < 0 || ctu_row1 > (h + 63) / 64 || ctu_row0 >= ctu_row1)
    return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_plan_create_rows: CTU row range");
  // the filters run without a chroma QP table (deblock.hip: identity), so a search that quantises chroma at another QP than luma
  // would be filtered with the wrong tc: refused rather than silently different (the reference's default table is the identity)
  if (params->qp_c != params->qp) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_plan_create: qp_c != qp needs a chroma QP table, which the loop plan does not take");
  std::vector<uvghip_ctu_picture_t> sp(n_pictures);
  for (int i = 0; i < n_pictures; ++i) {
    if (int rc = uvgi_check_out_planes(pictures[i], w, "uvghip_loop_plan_create: output planes", "uvghip_loop_plan_create: output strides")) return rc;
    sp[i] = pictures[i].search;
  }
  const layout_t L = layout_of(bitdepth, n_pictures, w, h);
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  uvghip_loop_plan *pl = new (std::nothrow) uvghip_loop_plan;
  if (!pl) return uvghip_set_error(hipErrorOutOfMemory, __func__);
  pl->search = nullptr;
  if (int rc = uvghip_ctu_plan_create_rows(bitdepth, params, sp.data(), n_pictures, ctu_row0, ctu_row1, ws + L.search, &pl->search)) { delete pl; return rc; }
  const int wc = (w + 63) / 64, hc = (h + 63) / 64;
  pl->row0 = ctu_row0; pl->row1 = ctu_row1;
  pl->bitdepth = bitdepth; pl->n = n_pictures; pl->w = w; pl->h = h; pl->sao_type = sao_type;
  pl->ctus = wc * hc;
  pl->pics.assign(pictures, pictures + n_pictures);
  pl->sao_info = reinterpret_cast<int32_t *>(ws + L.tail.info);
  pl->sao_models = reinterpret_cast<uint16_t *>(ws + L.tail.models);
  pl->coder_ws = ws + L.tail.coder;
  pl->rows = ws + L.tail.rows;
  pl->row_bytes = reinterpret_cast<int32_t *>(ws + L.tail.row_bytes);
  pl->row_cap = L.tail.row_cap; pl->hc = hc;
  pl->sums = reinterpret_cast<uint32_t *>(ws + L.sums);
  pl->ctu_params = *params;
  pl->filt_ws = ws + L.filt;
  pl->coder_ticket = reinterpret_cast<int32_t *>(ws + L.tick);
  if (int rc = uvgi_slice_rows_prepare(params, sp.data(), n_pictures, pl->coder_ws, false, nullptr)) { uvghip_ctu_plan_destroy(pl->search); delete pl; return rc; }
  // The in-loop filters are ONE launch behind the search, a workgroup per CTU (filters.hip, ctu_filter.h); the deblocked pictures go to
  // the workspace (per picture Y, U, V, tightly packed)
  std::vector<uvgi_pb_filter> fl(n_pictures);
  const size_t planes = (size_t)w * h * (bitdepth == 8 ? 1 : 2) * 3 / 2;
  for (int i = 0; i < n_pictures; ++i)
    fl[i] = uvgi_pb_filter_of(pictures[i], ws + L.snap + (size_t)i * planes, bitdepth, w, h, pl->sao_info + (size_t)i * pl->ctus * 34, pl->sao_models + (size_t)i * pl->ctus * 6, sao_type);
  if (int rc = uvgi_filter_prepare(bitdepth, params, sp.data(), fl.data(), n_pictures, 2, pl->filt_ws)) { uvghip_ctu_plan_destroy(pl->search); delete pl; return rc; }
  // a band's hand-over: the piece lists, and their tables for the pack / unpack kernels on the device (synchronous, once, as the tables above)
  for (int side = 0; side < 2; ++side) {
    if (side == 0 ? ctu_row0 == 0 : ctu_row1 == hc) continue;
    halo_list(pl, ws + L.snap, side == 0 ? ctu_row0 : ctu_row1, pl->halo[side], pl->halo_at[side], pl->halo_bytes);
    const size_t np = pl->halo[side].size();
    std::vector<halo_dev_piece> hd(np);
    for (size_t i = 0; i < np; ++i) {
      const uvghip_halo_piece_t &q = pl->halo[side][i];
      hd[i] = halo_dev_piece{static_cast<unsigned char *>(q.ptr), q.pitch, q.row_bytes, pl->halo_at[side][i], q.rows, 0};
    }
    hipError_t e = hipMalloc(&pl->halo_dev[side], np * sizeof(halo_dev_piece));
    if (e == hipSuccess) e = hipMemcpy(pl->halo_dev[side], hd.data(), np * sizeof(halo_dev_piece), hipMemcpyHostToDevice);
    if (e != hipSuccess) { uvghip_loop_plan_destroy(pl); return uvghip_set_error(e, __func__); }
  }
  *plan_out = pl;
  return 0;
}

extern "C" int uvghip_loop_plan_halo(const uvghip_loop_plan_t *pl, int side, uvghip_halo_piece_t *pieces, int cap, int *n)
{
  if (!pl || !n || cap < 0 || (cap && !pieces)) return uvghip_set_error(hipErrorInvalidValue, __func__);
  if (side != 0 && side != 1) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_plan_halo: side is 0 (received from the band above) or 1 (sent to the band below)");
  const std::vector<uvghip_halo_piece_t> &h = pl->halo[side];
  *n = (int)h.size();
  if ((size_t)cap < h.size()) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_plan_halo: cap is smaller than the number of pieces (*n)");
  for (size_t i = 0; i < h.size(); ++i) pieces[i] = h[i];
  return 0;
}

extern "C" size_t uvghip_loop_plan_halo_bytes(const uvghip_loop_plan_t *pl) { return pl ? pl->halo_bytes : 0; }

namespace {
int halo_copy(uvghip_loop_plan *pl, int side, void *message, void *stream, const char *none)
{
  if (pl->halo[side].empty()) return uvghip_set_error(hipErrorInvalidValue, none);
  const dim3 grid((unsigned)pl->halo[side].size(), 16);
  const halo_dev_piece *tab = static_cast<const halo_dev_piece *>(pl->halo_dev[side]);
  if (side) hipLaunchKernelGGL(halo_copy_kernel<true>, grid, dim3(256), 0, uvghip_stream(stream), tab, static_cast<unsigned char *>(message));
  else hipLaunchKernelGGL(halo_copy_kernel<false>, grid, dim3(256), 0, uvghip_stream(stream), tab, static_cast<unsigned char *>(message));
  UVGHIP_CHECK_LAUNCH();
}
}  // namespace

extern "C" int uvghip_loop_plan_halo_pack(uvghip_loop_plan_t *pl, void *message, void *stream)
{
  UVGHIP_REQUIRE_READY();
  if (!pl || !message) return uvghip_set_error(hipErrorInvalidValue, __func__);
  return halo_copy(pl, 1, message, stream, "uvghip_loop_plan_halo_pack: the plan holds the picture's last CTU row: nothing goes down");
}

extern "C" int uvghip_loop_plan_halo_unpack(uvghip_loop_plan_t *pl, const void *message, void *stream)
{
  UVGHIP_REQUIRE_READY();
  if (!pl || !message) return uvghip_set_error(hipErrorInvalidValue, __func__);
  return halo_copy(pl, 0, const_cast<void *>(message), stream, "uvghip_loop_plan_halo_unpack: the plan holds the picture's first CTU row: nothing comes from above");
}

extern "C" int uvghip_loop_plan_out_rows(const uvghip_loop_plan_t *pl, int *y0, int *y1)
{
  if (!pl || !y0 || !y1) return uvghip_set_error(hipErrorInvalidValue, __func__);
  const int delay = pl->sao_type ? 10 : 8;
  *y0 = pl->row0 ? 64 * pl->row0 - delay : 0;
  *y1 = pl->row1 == pl->hc ? pl->h : 64 * pl->row1 - delay;
  return 0;
}

extern "C" int uvghip_loop_plan_run(uvghip_loop_plan_t *pl, void *stream)
{
  UVGHIP_REQUIRE_READY();
  if (!pl) return uvghip_set_error(hipErrorInvalidValue, __func__);
  if (int rc = uvghip_ctu_plan_run(pl->search, stream)) return rc;
  return uvghip_loop_plan_run_filters(pl, stream);
}

// The plan's two streams and three events, created on first use (uvghip_loop_plan_run_overlapped; uvghip_loop_pb_run_inflight_intra).
int uvgi_loop_plan_side_streams(uvghip_loop_plan *pl)
{
  if (pl->side[0]) return 0;
  for (int i = 0; i < 2; ++i) {
    UVGHIP_TRY(hipStreamCreateWithFlags(&pl->side[i], hipStreamNonBlocking));
    UVGHIP_TRY(hipEventCreateWithFlags(&pl->ev_side[i], hipEventDisableTiming));
  }
  UVGHIP_TRY(hipEventCreateWithFlags(&pl->ev_fork, hipEventDisableTiming));
  return 0;
}

extern "C" int uvghip_loop_plan_run_overlapped(uvghip_loop_plan_t *pl, void *stream)
{
  UVGHIP_REQUIRE_READY();
  if (!pl) return uvghip_set_error(hipErrorInvalidValue, __func__);
  // only while the pictures' wavefronts leave half the device free, and what runs beside the search capped (internal.h: the measurements)
  const int wc = (pl->w + 63) / 64, per = wc < pl->hc ? wc : pl->hc;
  if ((long long)pl->n * per > uvgi_overlap_max_ctus || pl->row0 > 0 || pl->row1 < pl->hc) return uvghip_loop_plan_run(pl, stream);          // (no side-stream schedule for bands)
  hipStream_t st = uvghip_stream(stream);
  if (int rc = uvgi_loop_plan_side_streams(pl)) return rc;
  // all flags to zero in `stream`, the side streams behind that; then the search, so that it is in the queue before anything waits for it
  if (int rc = uvgi_ctu_plan_reset(pl->search, stream)) return rc;
  if (int rc = uvgi_filter_reset(pl->n, pl->w, pl->h, pl->filt_ws, stream)) return rc;
  UVGHIP_TRY(hipMemsetAsync(pl->coder_ticket, 0, sizeof(int32_t), st));
  UVGHIP_TRY(hipEventRecord(pl->ev_fork, st));
  if (int rc = uvgi_ctu_plan_launch(pl->search, stream)) return rc;
  for (int i = 0; i < 2; ++i) UVGHIP_TRY(hipStreamWaitEvent(pl->side[i], pl->ev_fork, 0));
  // the filter stage: as many persistent workgroups as the pictures' wavefronts can have CTUs in progress, at most an eighth of the device
  long long g = (long long)per * pl->n;
  if (g > uvgi_overlap_filter_cap) g = uvgi_overlap_filter_cap;
  if (int rc = uvgi_filter_run(pl->bitdepth, pl->n, pl->w, pl->h, pl->filt_ws, uvgi_ctu_plan_done_flags(pl->search), (int)g, pl->side[0])) return rc;
  if (int rc = uvgi_encode_slice_rows_behind(pl->bitdepth, &pl->ctu_params, pl->n, pl->sao_info, pl->sao_models, uvgi_filter_final_flags(pl->n, pl->w, pl->h, pl->filt_ws),
                                             pl->coder_ticket, uvgi_overlap_coder_cap, pl->coder_ws, pl->rows, pl->row_cap, pl->row_bytes, pl->side[1]))
    return rc;
  for (int i = 0; i < 2; ++i) {
    UVGHIP_TRY(hipEventRecord(pl->ev_side[i], pl->side[i]));
    UVGHIP_TRY(hipStreamWaitEvent(st, pl->ev_side[i], 0));
  }
  return 0;
}

extern "C" int uvghip_loop_plan_run_search(uvghip_loop_plan_t *pl, void *stream)
{
  UVGHIP_REQUIRE_READY();
  if (!pl) return uvghip_set_error(hipErrorInvalidValue, __func__);
  return uvghip_ctu_plan_run(pl->search, stream);
}

// one launch for the filters of every picture, one for the slice data: every WPP row's substream from the levels, the side information and
// the SAO decisions
extern "C" int uvghip_loop_plan_run_filters(uvghip_loop_plan_t *pl, void *stream)
{
  UVGHIP_REQUIRE_READY();
  if (!pl) return uvghip_set_error(hipErrorInvalidValue, __func__);
  if (int rc = uvgi_filter_run_rows(pl->bitdepth, pl->n, pl->w, pl->h, pl->row0, pl->row1, pl->filt_ws, nullptr, 0, stream)) return rc;
  return uvghip_loop_plan_run_coder(pl, stream);
}

// the slice data alone (the pictures' SAO decisions are in the plan's arrays: uvghip_loop_plan_results)
extern "C" int uvghip_loop_plan_run_coder(uvghip_loop_plan_t *pl, void *stream)
{
  UVGHIP_REQUIRE_READY();
  if (!pl) return uvghip_set_error(hipErrorInvalidValue, __func__);
  return uvgi_encode_slice_rows_band(pl->bitdepth, &pl->ctu_params, pl->n, pl->sao_type ? pl->sao_info : nullptr, pl->sao_type ? pl->sao_models : nullptr, pl->row0, pl->row1,
                                     pl->coder_ws, pl->rows, pl->row_cap, pl->row_bytes, stream);
}

extern "C" int uvghip_loop_plan_slice_data(const uvghip_loop_plan_t *pl, const uint8_t **rows, const int32_t **row_bytes, int *row_cap, int *n_rows)
{
  if (!pl) return uvghip_set_error(hipErrorInvalidValue, __func__);
  if (rows) *rows = pl->rows;
  if (row_bytes) *row_bytes = pl->row_bytes;
  if (row_cap) *row_cap = pl->row_cap;
  if (n_rows) *n_rows = pl->hc;
  return 0;
}

// The NAL units of one picture of the group after a run: the checksum of its output picture on the device, its rows and their
// lengths brought to the host, uvghip_write_picture_nals.  Waits for the stream (the bytes are host memory).
extern "C" int uvghip_loop_plan_picture_nals(uvghip_loop_plan_t *pl, int picture, int poc, uint8_t *out, size_t cap, size_t *len, void *stream)
{
  UVGHIP_REQUIRE_READY();
  if (!pl || picture < 0 || picture >= pl->n || poc < 0 || !len || (!out && cap)) return uvghip_set_error(hipErrorInvalidValue, __func__);
  if (pl->row0 > 0 || pl->row1 < pl->hc) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_plan_picture_nals: a band plan holds a part of the picture (gather the bands' rows and checksum terms)");
  hipStream_t st = uvghip_stream(stream);
  const uvghip_loop_picture_t &q = pl->pics[picture];
  uint32_t *d_sums = pl->sums + 3 * (size_t)picture;
  if (int rc = uvghip_picture_checksum(pl->bitdepth, q.out_y, q.out_stride, q.out_u, q.out_v, q.out_stride_c, pl->w, pl->h, d_sums, stream)) return rc;
  uint32_t sums[3];
  std::vector<int32_t> nb(pl->hc);
  UVGHIP_TRY(hipMemcpyAsync(sums, d_sums, sizeof sums, hipMemcpyDeviceToHost, st));
  UVGHIP_TRY(hipMemcpyAsync(nb.data(), pl->row_bytes + (size_t)picture * pl->hc, (size_t)pl->hc * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  UVGHIP_TRY(hipStreamSynchronize(st));
  size_t pitch = 1;
  for (int r = 0; r < pl->hc; ++r) {
    if (nb[r] <= 0 || nb[r] > pl->row_cap) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_plan_picture_nals: a row overflowed its slot (or the plan has not run)");
    if ((size_t)nb[r] > pitch) pitch = (size_t)nb[r];
  }
  std::vector<uint8_t> rows(pitch * pl->hc);
  for (int r = 0; r < pl->hc; ++r)
    UVGHIP_TRY(hipMemcpyAsync(rows.data() + (size_t)r * pitch, pl->rows + ((size_t)picture * pl->hc + r) * pl->row_cap, (size_t)nb[r], hipMemcpyDeviceToHost, st));
  UVGHIP_TRY(hipStreamSynchronize(st));
  return uvghip_write_picture_nals(poc, pl->sao_type != 0, rows.data(), pitch, nb.data(), pl->hc, sums, out, cap, len);
}

// The NAL units of ALL pictures of the group after a run, as pictures first_poc, first_poc + 1, ... : what n calls of
// uvghip_loop_plan_picture_nals write, one after the other into `out`, with two waits for the stream instead of 2 n and one download of the
// rows instead of n * rows: the checksums of all pictures, then their sums and row lengths in one copy; the rows gathered on the device
// (picture p at a 16-byte-aligned base, its rows at the picture's own pitch) into one buffer that comes over in one copy to pinned memory.
namespace {
__global__ void nal_layout_kernel(const int32_t *__restrict__ row_bytes, int n, int hc, unsigned long long *__restrict__ base)
{
  if (threadIdx.x || blockIdx.x) return;
  unsigned long long at = 0;
  unsigned long long *pitch = base + n + 1;
  for (int p = 0; p < n; ++p) {
    int m = 1;
    for (int r = 0; r < hc; ++r) { const int b = row_bytes[(size_t)p * hc + r]; m = b > m ? b : m; }
    const unsigned long long pt = ((unsigned long long)m + 15) & ~15ull;
    base[p] = at; pitch[p] = pt;
    at += pt * hc;
  }
  base[n] = at;
}
__global__ void __launch_bounds__(256) nal_gather_kernel(const uint8_t *__restrict__ rows, int row_cap, const int32_t *__restrict__ row_bytes, int n, int hc,
                                                         const unsigned long long *__restrict__ base, uint8_t *__restrict__ packed)
{
  const int p = blockIdx.x / hc, r = blockIdx.x - p * hc;
  const int nb = row_bytes[blockIdx.x];
  if (nb <= 0 || nb > row_cap) return;
  const uint4 *src = reinterpret_cast<const uint4 *>(rows + (size_t)blockIdx.x * row_cap);
  uint4 *dst = reinterpret_cast<uint4 *>(packed + base[p] + (size_t)r * base[n + 1 + p]);
  for (int i = threadIdx.x; i < (nb + 15) / 16; i += blockDim.x) dst[i] = src[i];
}
}  // namespace

extern "C" int uvghip_loop_plan_group_nals(uvghip_loop_plan_t *pl, int first_poc, uint8_t *out, size_t cap, size_t *lens, void *stream)
{
  UVGHIP_REQUIRE_READY();
  if (!pl || first_poc < 0 || !lens || (!out && cap)) return uvghip_set_error(hipErrorInvalidValue, __func__);
  if (pl->row0 > 0 || pl->row1 < pl->hc) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_plan_group_nals: a band plan holds a part of the picture (gather the bands' rows and checksum terms)");
  if (pl->row_cap & 15) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_plan_group_nals: the plan's row slots are not 16-byte multiples");
  hipStream_t st = uvghip_stream(stream);
  const int n = pl->n, hc = pl->hc;
  for (int i = 0; i < n; ++i) {
    const uvghip_loop_picture_t &q = pl->pics[i];
    if (int rc = uvghip_picture_checksum(pl->bitdepth, q.out_y, q.out_stride, q.out_u, q.out_v, q.out_stride_c, pl->w, pl->h, pl->sums + 3 * (size_t)i, stream)) return rc;
  }
  if (!pl->pack_base) UVGHIP_TRY(hipMalloc(reinterpret_cast<void **>(&pl->pack_base), (size_t)(2 * n + 1) * sizeof(unsigned long long)));
  hipLaunchKernelGGL(nal_layout_kernel, dim3(1), dim3(1), 0, st, pl->row_bytes, n, hc, pl->pack_base);
  std::vector<uint32_t> sums((size_t)3 * n);
  std::vector<int32_t> nb((size_t)n * hc);
  UVGHIP_TRY(hipMemcpyAsync(sums.data(), pl->sums, sums.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  UVGHIP_TRY(hipMemcpyAsync(nb.data(), pl->row_bytes, nb.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  UVGHIP_TRY(hipStreamSynchronize(st));
  // the same layout on the host
  std::vector<size_t> base((size_t)n + 1), pitch(n);
  size_t at = 0;
  for (int p = 0; p < n; ++p) {
    int m = 1;
    for (int r = 0; r < hc; ++r) {
      const int b = nb[(size_t)p * hc + r];
      if (b <= 0 || b > pl->row_cap) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_plan_group_nals: a row overflowed its slot (or the plan has not run)");
      m = b > m ? b : m;
    }
    base[p] = at; pitch[p] = ((size_t)m + 15) & ~(size_t)15;
    at += pitch[p] * hc;
  }
  base[n] = at;
  if (at > pl->pack_cap) {
    if (pl->pack_dev) { UVGHIP_TRY(hipFree(pl->pack_dev)); pl->pack_dev = nullptr; }
    if (pl->pack_host) { UVGHIP_TRY(hipHostFree(pl->pack_host)); pl->pack_host = nullptr; }
    pl->pack_cap = 0;
    const size_t want = at + at / 4 + 4096;
    UVGHIP_TRY(hipMalloc(reinterpret_cast<void **>(&pl->pack_dev), want));
    UVGHIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&pl->pack_host), want, hipHostMallocDefault));
    pl->pack_cap = want;
  }
  hipLaunchKernelGGL(nal_gather_kernel, dim3(n * hc), dim3(256), 0, st, pl->rows, pl->row_cap, pl->row_bytes, n, hc, pl->pack_base, pl->pack_dev);
  UVGHIP_TRY(hipGetLastError());
  UVGHIP_TRY(hipMemcpyAsync(pl->pack_host, pl->pack_dev, at, hipMemcpyDeviceToHost, st));
  UVGHIP_TRY(hipStreamSynchronize(st));
  size_t used = 0;
  for (int p = 0; p < n; ++p) {
    size_t len = 0;
    if (int rc = uvghip_write_picture_nals(first_poc + p, pl->sao_type != 0, pl->pack_host + base[p], pitch[p], nb.data() + (size_t)p * hc, hc, sums.data() + 3 * (size_t)p,
                                           out ? out + used : nullptr, cap > used ? cap - used : 0, &len)) return rc;
    lens[p] = len;
    used += len;
  }
  return 0;
}

extern "C" int uvghip_loop_plan_results(const uvghip_loop_plan_t *pl, const int32_t **sao_info, const uint16_t **sao_models)
{
  if (!pl) return uvghip_set_error(hipErrorInvalidValue, __func__);
  if (sao_info) *sao_info = pl->sao_info;
  if (sao_models) *sao_models = pl->sao_models;
  return 0;
}

// The ALF stage of the group (BASELINE configs[3]: --alf full), after uvghip_loop_plan_run: where the encoder runs uvg_alf_enc_process
// (src/alf.c:5193) on a picture whose search and SAO the device did.  Per picture the caller's `decide` is called with the picture's planes
// -- what ALF gets (the plan's SAO output) and the source -- and returns the decisions; the derivation itself (alf_encoder :3994,
// alf_encoder_ctb :4369, derive_cc_alf_filter :2212 on the statistics of alf_derive_stats_for_filtering :4227, which `decide` gathers with
// uvghip_alf_classify_frame / uvghip_alf_stats_compact_batch / uvghip_alf_cov_reduce / uvghip_cc_alf_stats_batch on the given planes and
// stream) stays host code.  Then uvghip_alf_reconstruct_picture into the caller's output planes and, for the whole group,
// uvghip_encode_slice_rows_alf: the slice data with the CTU-level ALF syntax.
extern "C" size_t uvghip_loop_plan_alf_workspace_bytes(const uvghip_loop_plan_t *pl)
{
  if (!pl) return 0;
  return uvgi_align_up(uvghip_alf_reconstruct_workspace_bytes(pl->w, pl->h), 256) + uvgi_align_up(uvghip_slice_rows_alf_workspace_bytes(pl->n), 256) +
         (size_t)pl->n * uvgi_align_up((size_t)pl->ctus * 7 + (size_t)pl->ctus * sizeof(int16_t), 256);
}

extern "C" int uvghip_loop_plan_alf_stage(uvghip_loop_plan_t *pl, uvghip_alf_decide_fn decide, void *user, int classification_shift, const uvghip_alf_planes_t *alf_out,
                                          void *workspace, uint8_t *rows, int row_cap, int32_t *row_bytes, void *stream)
{
  UVGHIP_REQUIRE_READY();
  if (!pl || !decide || !alf_out || !workspace || !rows || row_cap <= 0 || !row_bytes || classification_shift < 8 || classification_shift > 20)
    return uvghip_set_error(hipErrorInvalidValue, __func__);
  hipStream_t st = uvghip_stream(stream);
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  unsigned char *ws_rec = ws, *ws_coder = ws_rec + uvgi_align_up(uvghip_alf_reconstruct_workspace_bytes(pl->w, pl->h), 256);
  unsigned char *ws_flags = ws_coder + uvgi_align_up(uvghip_slice_rows_alf_workspace_bytes(pl->n), 256);
  const size_t per = uvgi_align_up((size_t)pl->ctus * 7 + (size_t)pl->ctus * sizeof(int16_t), 256), b = pl->bitdepth == 8 ? 1 : 2;
  std::vector<uvghip_slice_alf_t> sl(pl->n);
  std::vector<uvghip_ctu_picture_t> cp(pl->n);
  for (int i = 0; i < pl->n; ++i) {
    const uvghip_loop_picture_t &q = pl->pics[i];
    const uvghip_alf_planes_t &o = alf_out[i];
    if (!o.y || !o.u || !o.v || o.stride < pl->w || o.stride_c < pl->w / 2) return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_plan_alf_stage: output planes");
    uvghip_alf_decision_t d;
    memset(&d, 0, sizeof d);
    if (int rc = decide(user, i, &q, &d)) return uvghip_set_error(hipErrorInvalidValue, rc > 0 ? "uvghip_loop_plan_alf_stage: decide() failed" : "uvghip_loop_plan_alf_stage: decide() refused");
    const bool any = d.enabled[0] || d.enabled[1] || d.enabled[2] || d.cc_enabled[0] || d.cc_enabled[1];
    if ((d.alf_type != 1 && d.alf_type != 2) || d.n_luma_aps < 0 || d.n_luma_aps > 8 || (any && (!d.ctu_flags || !d.filter_set_idx)) || (d.n_luma_aps && !d.luma_aps) ||
        ((d.enabled[1] || d.enabled[2]) && !d.chroma_aps) || ((d.cc_enabled[0] || d.cc_enabled[1]) && !d.cc_coeff))
      return uvghip_set_error(hipErrorInvalidValue, "uvghip_loop_plan_alf_stage: the decision decide() returned");
    if (any) {
      uvghip_alf_picture_t a;
      memset(&a, 0, sizeof a);
      a.in_y = q.out_y; a.in_u = q.out_u; a.in_v = q.out_v; a.in_stride = q.out_stride; a.in_stride_c = q.out_stride_c;
      a.out_y = o.y; a.out_u = o.u; a.out_v = o.v; a.out_stride = o.stride; a.out_stride_c = o.stride_c;
      a.width = pl->w; a.height = pl->h;
      for (int c = 0; c < 3; ++c) a.slice_enabled[c] = d.enabled[c];
      a.n_luma_aps = d.n_luma_aps; a.ctu_flags = d.ctu_flags; a.filter_set_idx = d.filter_set_idx; a.luma_aps = d.luma_aps; a.chroma_aps = d.chroma_aps;
      a.alf_full = d.alf_type == 2; a.cc_alf_enabled[0] = d.cc_enabled[0]; a.cc_alf_enabled[1] = d.cc_enabled[1]; a.cc_coeff = d.cc_coeff;
      a.classification_shift = classification_shift;
      if (int rc = uvghip_alf_reconstruct_picture(pl->bitdepth, &a, ws_rec, stream)) return rc;
    } else {          // a picture ALF leaves alone
      UVGHIP_TRY(hipMemcpy2DAsync(o.y, (size_t)o.stride * b, q.out_y, (size_t)q.out_stride * b, (size_t)pl->w * b, pl->h, hipMemcpyDeviceToDevice, st));
      UVGHIP_TRY(hipMemcpy2DAsync(o.u, (size_t)o.stride_c * b, q.out_u, (size_t)q.out_stride_c * b, (size_t)(pl->w / 2) * b, pl->h / 2, hipMemcpyDeviceToDevice, st));
      UVGHIP_TRY(hipMemcpy2DAsync(o.v, (size_t)o.stride_c * b, q.out_v, (size_t)q.out_stride_c * b, (size_t)(pl->w / 2) * b, pl->h / 2, hipMemcpyDeviceToDevice, st));
    }
    // the slice's side of the decision: the flags and set indices on the device, where the coder reads them
    uvghip_slice_alf_t &s = sl[i];
    memset(&s, 0, sizeof s);
    s.alf_type = d.alf_type; s.n_luma_aps = d.n_luma_aps; s.n_alternatives_chroma = d.chroma_aps ? d.chroma_aps[112] : 0;
    for (int c = 0; c < 3; ++c) s.enabled[c] = d.enabled[c];
    for (int c = 0; c < 2; ++c) { s.cc_enabled[c] = d.cc_enabled[c]; s.cc_filter_count[c] = d.cc_filter_count[c]; }
    unsigned char *fl = ws_flags + (size_t)i * per;
    if (d.ctu_flags && d.filter_set_idx) {
      UVGHIP_TRY(hipMemcpyAsync(fl, d.ctu_flags, (size_t)pl->ctus * 7, hipMemcpyHostToDevice, st));
      UVGHIP_TRY(hipMemcpyAsync(fl + (size_t)pl->ctus * 7 + ((size_t)pl->ctus & 1), d.filter_set_idx, (size_t)pl->ctus * sizeof(int16_t), hipMemcpyHostToDevice, st));
      UVGHIP_TRY(hipStreamSynchronize(st));          // (decide()'s arrays need not outlive the next call)
      s.ctu_flags = fl; s.filter_set_idx = reinterpret_cast<const int16_t *>(fl + (size_t)pl->ctus * 7 + ((size_t)pl->ctus & 1));
    }
    cp[i] = q.search;
  }
  return uvghip_encode_slice_rows_alf(pl->bitdepth, &pl->ctu_params, cp.data(), sl.data(), pl->n, pl->sao_info, pl->sao_models, ws_coder, rows, row_cap, row_bytes, stream);
}

extern "C" void uvghip_loop_plan_destroy(uvghip_loop_plan_t *pl)
{
  if (!pl) return;
  uvghip_ctu_plan_destroy(pl->search);
  if (pl->pack_dev) (void)hipFree(pl->pack_dev);
  if (pl->pack_host) (void)hipHostFree(pl->pack_host);
  if (pl->pack_base) (void)hipFree(pl->pack_base);
  for (int i = 0; i < 2; ++i) {
    if (pl->halo_dev[i]) (void)hipFree(pl->halo_dev[i]);
    if (pl->side[i]) (void)hipStreamDestroy(pl->side[i]);
    if (pl->ev_side[i]) (void)hipEventDestroy(pl->ev_side[i]);
  }
  if (pl->ev_fork) (void)hipEventDestroy(pl->ev_fork);
  delete pl;
}
