// uvgi_filter_*: the in-loop filters of a whole group of searched pictures in ONE launch -- a workgroup per CTU runs the per-CTU
// filter stage of ctu_filter.h (deblocking of what the CTU completes, its SAO statistics and decision, SAO into the output picture: what
// encoder_state_worker_encode_lcu_search does after uvg_search_lcu, src/encoderstate.c:841-853, with the pictures' reconstruction left
// unfiltered).  It replaces the chain of whole-picture kernels the loop plans strung behind the search (per picture: three snapshot
// copies, two snapshot deblocking passes, three SAO statistics launches, two deblocking passes, three SAO apply launches; per group the
// two decision kernels: ~9 000 launches for 224 pictures, each taking turns with the other group's search on a full device) -- the
// same pictures, decisions and models (tests/test_gpu_sao_decide.py, the whole-picture goldens).
//
// The stage is the P / B kernel's (where it runs inside the persistent search kernel, pictures in flight); here it is a kernel of its
// own because the I-picture search kernel is built for four workgroups per CU at 128 registers, under which the deblocking segment
// functions spill (3.8 M cycles per CTU inside that kernel against 0.17 M here).  CTUs are handed out in wavefront order (a ticket per
// workgroup), so the SAO decision's chain -- a CTU reads the models its left neighbour left, the first CTU of a row those of the first
// CTU of the row above, and both neighbours' decisions as merge candidates -- only ever waits for CTUs that are running or done.
#include "uvghip_common.h"
#define CTUF_CALL __attribute__((always_inline))
#include "ctu_filter.h"
#include "ctu_ticket.h"
#include <vector>

namespace {

struct fpic_dev {
  ctuf::filt_pic F;
  const void *rec_y, *rec_u, *rec_v, *src_y, *src_u, *src_v;
  const uvghip_scu_t *scu;
  int32_t rec_stride, rec_stride_c, src_stride, src_stride_c, scu_stride, pad;
};

struct filter_args {
  const fpic_dev *pics;
  int32_t *ticket, *sao_done, *final_done;
  int wc, hc, n_pictures, W, H;
  int row0, row1;               // the CTU rows of this launch (a band of every picture; the whole picture: 0, hc)
  const int32_t *searched;      // BEHIND: [picture][ctu], the search's "done" flags (uvgi_ctu_plan_done_flags)
};

// BEHIND: a small grid of persistent workgroups that take CTU after CTU and wait for the SEARCH's flag of each -- the filters of a group
// BESIDE its search launch (uvghip_loop_plan_run_overlapped), a CTU filtered as soon as it is searched instead of after the last CTU of the
// launch.  The grid is capped by the caller so that the search, launched first, keeps the device: a waiting workgroup holds its slot.
template <typename PX, bool BEHIND>
__global__ void __launch_bounds__(256) ctu_filter_kernel(filter_args A)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int s_ticket;
  for (;;) {
  if (threadIdx.x == 0) s_ticket = atomicAdd(A.ticket, 1);
  __syncthreads();
  // ticket -> (picture, row, column) in the band's wavefront order (ctu_ticket.h): every CTU comes after its left, upper and upper right
  // neighbour; pictures interleaved
  const int wc = A.wc, hc = A.hc, ctus = wc * hc;
  if (s_ticket >= wc * (A.row1 - A.row0) * A.n_pictures) break;
  const uvgi_ticket_ctu T = uvgi_filter_ticket(s_ticket, wc, A.row0, A.row1, A.n_pictures);
  const int pic = T.pic, cy = T.cy, cx = T.cx;
  const fpic_dev &D = A.pics[pic];
  ctuf::filt_ctu F;
  F.rec_y = D.rec_y; F.rec_u = D.rec_u; F.rec_v = D.rec_v; F.src_y = D.src_y; F.src_u = D.src_u; F.src_v = D.src_v;
  F.rec_stride = D.rec_stride; F.rec_stride_c = D.rec_stride_c; F.src_stride = D.src_stride; F.src_stride_c = D.src_stride_c;
  F.scu = D.scu; F.scu_stride = D.scu_stride;
  F.W = A.W; F.H = A.H; F.cx = cx; F.cy = cy; F.wc = wc; F.hc = hc; F.row0 = A.row0;
  F.sao_done = A.sao_done + (size_t)pic * ctus; F.final_done = A.final_done + (size_t)pic * ctus;
  if (BEHIND) {
    // the CTU's own flag: its left / upper / upper-left neighbours, whose samples and side information the stage reads too, were searched before it
    if (threadIdx.x == 0) { ctuf::wait_set(&A.searched[(size_t)pic * ctus + cy * wc + cx]); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); }
    __syncthreads();
  }
  ctuf::filter_ctu<PX>(smem, D.F, F);
  if (!BEHIND) break;
  __syncthreads();          // the LDS image and s_ticket are free again
  }
}

// (bitdepth, BEHIND) -> the instantiation: the one launch site's kernel
const void *filter_kernel(int bitdepth, bool behind)
{
  const void *const fn[2][2] = {{reinterpret_cast<const void *>(&ctu_filter_kernel<uint8_t, true>), reinterpret_cast<const void *>(&ctu_filter_kernel<uint16_t, true>)},
                                {reinterpret_cast<const void *>(&ctu_filter_kernel<uint8_t, false>), reinterpret_cast<const void *>(&ctu_filter_kernel<uint16_t, false>)}};
  return fn[!behind][bitdepth != 8];
}
struct fl_layout { size_t ticket, sao_done, final_done, pics, total; };
fl_layout layout(int n, int w, int h)
{
  const size_t ctus = (size_t)((w + 63) / 64) * ((h + 63) / 64), total = ctus * n;
  fl_layout L;
  uvgi_carver c;
  L.ticket = c.take(256);
  L.sao_done = c.take(2 * total * 4);          // one piece: the two flag arrays
  L.final_done = L.sao_done + total * 4;
  L.pics = c.take((size_t)n * sizeof(fpic_dev));          // [0, pics): zeroed before every run
  L.total = c.end;
  return L;
}

}  // namespace

size_t uvgi_filter_workspace_bytes(int n_pictures, int pic_w, int pic_h)
{
  if (n_pictures <= 0 || pic_w <= 0 || pic_h <= 0) return 0;
  return layout(n_pictures, pic_w, pic_h).total;
}

// The picture table is written once per workspace (prepare: synchronous copy, as the slice coder's table), a run is a memset of the
// flags and one launch.
int uvgi_filter_prepare(int bitdepth, const uvghip_ctu_params_t *params, const uvghip_ctu_picture_t *pictures, const uvgi_pb_filter *filters, int n_pictures,
                        int slice_type, void *workspace)
{
  UVGHIP_REQUIRE_READY();
  UVGHIP_REQUIRE_DEPTH(bitdepth);
  if (!params || !pictures || !filters || n_pictures <= 0 || !workspace || slice_type < 0 || slice_type > 2) return uvghip_set_error(hipErrorInvalidValue, __func__);
  const int w = params->pic_w, h = params->pic_h;
  if (w <= 0 || h <= 0 || (w & 7) || (h & 7)) return uvghip_set_error(hipErrorInvalidValue, "uvgi_filter_prepare: picture size");
  if (params->qp_c != params->qp) return uvghip_set_error(hipErrorInvalidValue, "uvgi_filter_prepare: qp_c != qp needs a chroma QP table");
  const int wc = (w + 63) / 64;
  std::vector<fpic_dev> pd(n_pictures);
  for (int i = 0; i < n_pictures; ++i) {
    const uvghip_ctu_picture_t &p = pictures[i];
    if (int rc = uvgi_check_picture(p, w, wc, false, "uvgi_filter_prepare: picture descriptor")) return rc;
    if (int rc = uvgi_check_filter(filters[i], w, "uvgi_filter_prepare: filter stage")) return rc;
    fpic_dev &d = pd[i];
    d.F = uvgi_filt_pic_of(filters[i], params->lambda, params->qp, slice_type);
    d.rec_y = p.rec_y; d.rec_u = p.rec_u; d.rec_v = p.rec_v; d.src_y = p.src_y; d.src_u = p.src_u; d.src_v = p.src_v; d.scu = p.cu;
    d.rec_stride = p.rec_stride; d.rec_stride_c = p.rec_stride_c; d.src_stride = p.src_stride; d.src_stride_c = p.src_stride_c; d.scu_stride = p.cu_stride; d.pad = 0;
  }
  const fl_layout L = layout(n_pictures, w, h);
  UVGHIP_TRY(hipMemcpy(static_cast<unsigned char *>(workspace) + L.pics, pd.data(), pd.size() * sizeof(fpic_dev), hipMemcpyHostToDevice));
  return 0;
}

int uvgi_filter_reset(int n_pictures, int pic_w, int pic_h, void *workspace, void *stream)
{
  UVGHIP_REQUIRE_READY();
  if (n_pictures <= 0 || pic_w <= 0 || pic_h <= 0 || !workspace) return uvghip_set_error(hipErrorInvalidValue, __func__);
  UVGHIP_TRY(hipMemsetAsync(workspace, 0, layout(n_pictures, pic_w, pic_h).pics, uvghip_stream(stream)));
  return 0;
}
const int32_t *uvgi_filter_final_flags(int n_pictures, int pic_w, int pic_h, const void *workspace)
{
  if (n_pictures <= 0 || pic_w <= 0 || pic_h <= 0 || !workspace) return nullptr;
  return reinterpret_cast<const int32_t *>(static_cast<const unsigned char *>(workspace) + layout(n_pictures, pic_w, pic_h).final_done);
}

// searched == NULL: the flags to zero here and a workgroup per CTU; else at most max_workgroups persistent workgroups behind the search's
// flags, the flags zeroed beforehand by uvgi_filter_reset
int uvgi_filter_run(int bitdepth, int n_pictures, int pic_w, int pic_h, void *workspace, const int32_t *searched, int max_workgroups, void *stream)
{
  return uvgi_filter_run_rows(bitdepth, n_pictures, pic_w, pic_h, 0, (pic_h + 63) / 64, workspace, searched, max_workgroups, stream);
}

// ... over the CTU rows [row0, row1) of every picture.  The kernel KNOWS row0: a CTU of row row0 waits for no flag of row row0 - 1 (the flags
// of rows outside the band are never set by this launch; what the row reads of the row above is in the buffers before the launch).
int uvgi_filter_run_rows(int bitdepth, int n_pictures, int pic_w, int pic_h, int row0, int row1, void *workspace, const int32_t *searched, int max_workgroups,
                         void *stream)
{
  UVGHIP_REQUIRE_READY();
  UVGHIP_REQUIRE_DEPTH(bitdepth);
  if (n_pictures <= 0 || pic_w <= 0 || pic_h <= 0 || !workspace || (searched && max_workgroups < 1) || row0 < 0 || row0 >= row1 || row1 > (pic_h + 63) / 64)
    return uvghip_set_error(hipErrorInvalidValue, __func__);
  const fl_layout L = layout(n_pictures, pic_w, pic_h);
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  hipStream_t st = uvghip_stream(stream);
  if (!searched) UVGHIP_TRY(hipMemsetAsync(ws, 0, L.pics, st));
  filter_args A;
  A.pics = reinterpret_cast<const fpic_dev *>(ws + L.pics);
  A.ticket = reinterpret_cast<int32_t *>(ws + L.ticket);
  A.sao_done = reinterpret_cast<int32_t *>(ws + L.sao_done);
  A.final_done = reinterpret_cast<int32_t *>(ws + L.final_done);
  A.wc = (pic_w + 63) / 64; A.hc = (pic_h + 63) / 64; A.n_pictures = n_pictures; A.W = pic_w; A.H = pic_h;
  A.row0 = row0; A.row1 = row1;
  A.searched = searched;
  const int total = A.wc * (row1 - row0) * n_pictures, grid = searched && max_workgroups < total ? max_workgroups : total;
  void *args[] = {&A};
  (void)hipLaunchKernel(filter_kernel(bitdepth, searched != nullptr), dim3(grid), dim3(256), args, bitdepth == 8 ? sizeof(ctuf::filt_lds<uint8_t>) : sizeof(ctuf::filt_lds<uint16_t>), st);
  UVGHIP_CHECK_LAUNCH();
}
