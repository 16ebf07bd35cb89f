// The steps that one .hip file of the library calls in another: the launch halves and flags of the loop plans' search, filter and
// coder launches.  Not part of the C ABI -- plain C++ linkage and no UVGHIP_API, so -fvisibility=hidden keeps them out of
// libuvg266hip.so.  Their contracts (what must be zeroed in stream order first, what must already be LAUNCHED) are the callers' duty:
// loop_plan.hip, loop_pb.hip and the public entry points of the files that define them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <vector>
#include "../../include/uvg266_hip.h"

int uvghip_set_error(hipError_t e, const char *where);          // context.hip

// ---- what the device is assumed to hold (MI355X) and the launch caps that follow: constants, not hipDeviceProp -- the measurements
// beside them were taken with these values ------------------------------------------------------------------------------------------------
constexpr int uvgi_cus = 256, uvgi_lds_per_cu = 160 * 1024;          // 8 XCDs x 32 CUs; a CU's LDS
// Search workgroups per CU: ctu_search_kernel's __launch_bounds__(256, 4) (four waves each, one per SIMD) and the one-wave P / B kernel,
// whose registers allow one wave per SIMD.  A workgroup's LDS -- dynamic image plus the function-scope tables the build's .usage file
// reports -- must fit this share: one more word and the device holds three workgroups per CU instead of four (-25 %).
constexpr int uvgi_search_wgs_per_cu = 4, uvgi_search_lds_share = uvgi_lds_per_cu / uvgi_search_wgs_per_cu;
constexpr int uvgi_wg_slots = uvgi_cus * uvgi_search_wgs_per_cu;          // search workgroups the device holds at once
// Scratch slots of a search workspace: a workgroup claims one while it runs.  Twice what the device can hold of the kernel, so a free
// bit always exists; small jobs take one slot per CTU, rounded up to whole bitmap words.
constexpr int uvgi_max_slots = 2 * uvgi_wg_slots;
// ctu_search_kernel's walkers-per-SIMD counters, indexed by what the hardware reports: [XCC_ID (3 bits)][HW_ID's SE, SH, CU (8 bits)][SIMD]
constexpr int uvgi_simd_counters = 8 * 256 * 4;
// uvghip_loop_plan_run_overlapped.  Beside a search that fills the device the stage's workgroups and the coder's waves displace search
// workgroups (a CU's 160 KB of LDS are four search workgroups exactly: one coder wave of 10 KB costs the CU a whole one) and the group gets
// SLOWER -- measured: 60 pictures of 1080p, up to 1020 CTUs in progress on 1024 slots, 543 -> 621 ms; 16 pictures 484 -> 415 ms, one
// picture 461 -> 396 ms.  So: only while the pictures' wavefronts leave half the device free ...
constexpr int uvgi_overlap_max_ctus = uvgi_wg_slots / 2;
// ... and what runs beside the search is capped: a waiting filter workgroup or coder wave holds LDS a search workgroup cannot use.  The
// filter stage gets an eighth of the slots, the coder a wave per CU.
constexpr int uvgi_overlap_filter_cap = uvgi_wg_slots / 8, uvgi_overlap_coder_cap = uvgi_cus;
// The in-flight P / B launch (uvgi_search_pb_inflight).  Its workgroups of three or four waves take a CU each, of one or two waves a
// share of the slots.  A launch BESIDE it that it waits for (the I pictures' search, other_workgroups of four per CU) is left its CUs --
// at most half the slots, so that the flight keeps half the device; a flight cut down to its room keeps a sixteenth of the CUs at least.
constexpr int uvgi_flight_other_max = uvgi_wg_slots / 2, uvgi_flight_min_grid = uvgi_cus / 16;
inline int uvgi_flight_grid_cap(int waves) { return waves >= 3 ? uvgi_cus : uvgi_wg_slots / waves; }
inline int uvgi_flight_room(int other_workgroups) { return uvgi_cus - (other_workgroups + uvgi_search_wgs_per_cu - 1) / uvgi_search_wgs_per_cu; }
static_assert(uvgi_search_lds_share == 40960 && uvgi_wg_slots == 1024 && uvgi_max_slots == 2048 && uvgi_simd_counters == 8192 && uvgi_overlap_max_ctus == 512 &&
              uvgi_overlap_filter_cap == 128 && uvgi_overlap_coder_cap == 256 && uvgi_flight_other_max == 512 && uvgi_flight_min_grid == 16,
              "the launch caps the goldens and the recorded timings were taken with");

// ---- carving a workspace: offsets in the order they are taken, every one 256-byte aligned -----------------------------------------------
constexpr size_t uvgi_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
struct uvgi_carver {
  size_t at = 0, end = 0;          // the next offset; where the last piece really ends (a layout whose size is not rounded up)
  size_t take(size_t bytes) { const size_t o = at; end = at + bytes; at = uvgi_align_up(end, 256); return o; }
};
// the slice data's tail of the three loop layouts (loop_plan.hip, loop_pb.hip): SAO decisions, the coder's table, the rows and their lengths
struct uvgi_coder_tail {
  size_t info, models, coder, row_bytes, rows;
  int row_cap;          // twice the raw storage of a CTU row of 4:2:0 samples: no row of real content comes near
  void carve_sao(uvgi_carver &c, size_t n, size_t ctus) { info = c.take(n * ctus * 34 * 4); models = c.take(n * ctus * 6 * 2); }
  void carve_rows(uvgi_carver &c, int bitdepth, size_t n, int w, size_t hc, size_t coder_bytes)
  {
    row_cap = 3 * 64 * w * (bitdepth == 8 ? 1 : 2);
    coder = c.take(coder_bytes); row_bytes = c.take(n * hc * 4); rows = c.take(n * hc * row_cap);
  }
};

// ---- descriptor checks: one copy of every pointer and stride rule.  `text` is the caller's own error text, reported as it always was ------
inline int uvgi_refuse_if(bool bad, const char *text) { return bad ? uvghip_set_error(hipErrorInvalidValue, text) : 0; }
// params: the range every search takes.  depth_max_least: the all-intra kernel walks any pu-depth-intra range up to 4 (4 > depth_max is
// tested, tests/test_ctu_emulation.py); the P / B search is only pinned against the reference with 4x4 intra leaves and asks for 4.
inline int uvgi_check_params(const uvghip_ctu_params_t &p, int depth_max_least, bool needs_lambda_sqrt, const char *text)
{
  return uvgi_refuse_if(p.wpp != 1 || p.depth_min < 1 || p.depth_max < depth_max_least || p.depth_max > 4 || p.depth_min > p.depth_max || p.rough_levels < 2 ||
                        p.rough_levels > 3 || p.qp < 0 || p.qp > 63 || p.qp_c < 0 || p.qp_c > 63 || !(p.lambda > 0) || (needs_lambda_sqrt && !(p.lambda_sqrt > 0)) ||
                        p.rd < 0 || p.rd > 1, text);
}
// a searched picture of width w, wc CTUs a row (coeff / models: not for a caller that only filters it); text_strides: where the caller has
// a text of its own for a stride smaller than the picture
inline int uvgi_check_picture(const uvghip_ctu_picture_t &c, int w, int wc, bool needs_coeff_models, const char *text, const char *text_strides = nullptr)
{
  if (int rc = uvgi_refuse_if(!c.src_y || !c.src_u || !c.src_v || !c.rec_y || !c.rec_u || !c.rec_v || !c.cu || (needs_coeff_models && (!c.coeff || !c.models)) ||
                              c.cu_stride < wc * 16, text)) return rc;
  return uvgi_refuse_if(c.src_stride < w || c.rec_stride < w || c.src_stride_c < w / 2 || c.rec_stride_c < w / 2, text_strides ? text_strides : text);
}
template <typename OUT>          // uvghip_loop_picture_t / uvghip_loop_pb_picture_t: out_y .. out_stride_c
inline int uvgi_check_out_planes(const OUT &q, int w, const char *text, const char *text_strides = nullptr)
{
  if (int rc = uvgi_refuse_if(!q.out_y || !q.out_u || !q.out_v, text)) return rc;
  return uvgi_refuse_if(q.out_stride < w || q.out_stride_c < w / 2, text_strides ? text_strides : text);
}

// ---- ctu_search.hip: an all-intra search plan's run in two halves ------------------------------------------------------------------
// For a caller that lets ANOTHER stream's kernel wait for this plan's per-CTU flags (pictures in flight behind an I picture,
// uvghip_loop_pb_run_inflight_intra): reset -- the counters and flags back to zero, in stream order; the other stream waits for an event
// recorded behind it -- then launch.  uvghip_ctu_plan_run is the two in a row.
int uvgi_ctu_plan_reset(uvghip_ctu_plan_t *pl, void *stream);
int uvgi_ctu_plan_launch(uvghip_ctu_plan_t *pl, void *stream);
// ... max_workgroups > 0: the launch is that many persistent workgroups (0: one per CTU, the default)
int uvgi_ctu_plan_set_grid(uvghip_ctu_plan_t *pl, int max_workgroups);
// ... the per-CTU "searched" flags [picture][ctu] (DEVICE memory; zero after the reset, 1 when the CTU's outputs are published)
const int32_t *uvgi_ctu_plan_done_flags(const uvghip_ctu_plan_t *pl);

// ---- the per-CTU in-loop filter stage (ctu_filter.h): where a picture's filtered planes and SAO decisions go ---------------------------
// dbk_*: the deblocked picture; out_*: the picture uvg_encoder_encode returns (after SAO; sao_type 0: the deblocked picture); sao_info
// [ctu][34] / sao_models [ctu][6]: the decisions in uvghip_sao_decide_pictures_slice's layout.  The search's pic.rec_* stay unfiltered.
struct uvgi_pb_filter {
  void *dbk_y, *dbk_u, *dbk_v;          // DEVICE, pic_w x pic_h (+ chroma)
  void *out_y, *out_u, *out_v;
  int32_t dbk_stride, dbk_stride_c, out_stride, out_stride_c;     // in samples
  int32_t *sao_info;
  uint16_t *sao_models;
  int32_t sao_type, reserved;           // cfg.sao_type: 0 off, 1 edge, 2 band, 3 both
};

inline int uvgi_check_filter(const uvgi_pb_filter &f, int w, const char *text)
{
  return uvgi_refuse_if(!f.dbk_y || !f.dbk_u || !f.dbk_v || !f.out_y || !f.out_u || !f.out_v || f.dbk_stride < w || f.dbk_stride_c < w / 2 || f.out_stride < w ||
                        f.out_stride_c < w / 2 || f.sao_type < 0 || f.sao_type > 3 || (f.sao_type && (!f.sao_info || !f.sao_models)), text);
}
// the stage of a w x h picture: deblocked into `dbk` (Y, U, V tightly packed), SAO into the caller's output planes, the decisions into the given arrays
template <typename OUT>
inline uvgi_pb_filter uvgi_pb_filter_of(const OUT &q, void *dbk, int bitdepth, int w, int h, int32_t *sao_info, uint16_t *sao_models, int sao_type)
{
  unsigned char *d = static_cast<unsigned char *>(dbk);
  const size_t plane = (size_t)w * h * (bitdepth == 8 ? 1 : 2);
  return uvgi_pb_filter{d, d + plane, d + plane + plane / 4, q.out_y, q.out_u, q.out_v, w, w / 2, q.out_stride, q.out_stride_c, sao_info, sao_models, sao_type, 0};
}

// ---- filters.hip: the filter stage as ONE launch over a group of searched pictures, a workgroup per CTU -------------------------------
// What the all-intra loop plan runs behind its search instead of the chain of whole-picture kernels (snapshot deblocking, SAO statistics,
// decision, deblocking, SAO apply: the same pictures, decisions and models).  pictures[i].rec_* / cu / src_*: the search's outputs,
// filters[i] as above; slice_type 0 B / 1 P / 2 I (the SAO models' initialisation) and params->qp / lambda of the whole group.
// prepare: the picture table into the workspace (synchronous, once).
size_t uvgi_filter_workspace_bytes(int n_pictures, int pic_w, int pic_h);
int uvgi_filter_prepare(int bitdepth, const uvghip_ctu_params_t *params, const uvghip_ctu_picture_t *pictures, const uvgi_pb_filter *filters, int n_pictures,
                        int slice_type, void *workspace);
// run, searched == NULL: BEHIND the search -- a memset of the ticket and flags, then a workgroup per CTU; nothing waits.
// run, searched != NULL: BESIDE the search that feeds it -- uvgi_filter_reset (ticket and flags to zero, in stream order) first, then this on
// a stream that waits for the reset: at most max_workgroups persistent workgroups that take CTU after CTU in wavefront order and wait for
// searched[picture][ctu] (the search plan's flags, uvgi_ctu_plan_done_flags) of each -- a CTU is filtered as soon as it is searched (the
// order of encoder_state_worker_encode_lcu_search, src/encoderstate.c:808-853).  The search must have been LAUNCHED before this kernel
// (a waiting workgroup holds its slot; the cap keeps the device for the search).
int uvgi_filter_run(int bitdepth, int n_pictures, int pic_w, int pic_h, void *workspace, const int32_t *searched, int max_workgroups, void *stream);
int uvgi_filter_reset(int n_pictures, int pic_w, int pic_h, void *workspace, void *stream);
// ... the same launch over the CTU rows [row0, row1) of every picture (a band of a picture sharded by CTU rows): the band's CTUs only, in
// wavefront order within the band (ctu_ticket.h).  The kernel knows row0: a CTU of the band's first row waits for no flag of the row above,
// whose unfiltered samples, side information, deblocked rows, SAO decisions and models the caller has put into the buffers.
int uvgi_filter_run_rows(int bitdepth, int n_pictures, int pic_w, int pic_h, int row0, int row1, void *workspace, const int32_t *searched, int max_workgroups,
                         void *stream);
// ... the stage's own per-CTU "final" flags [picture][ctu] (DEVICE memory): 1 when the CTU's SAO decision and its part of the output picture
// are published -- what uvgi_encode_slice_rows_behind waits for
const int32_t *uvgi_filter_final_flags(int n_pictures, int pic_w, int pic_h, const void *workspace);

// ---- ctu_search_pb.hip: P / B pictures IN FLIGHT behind their references, the filter stage inside the persistent search kernel -------
// uvghip_ctu_search_pb with, per CTU, the in-loop filters right behind its search (what encoder_state_worker_encode_lcu_search does after
// uvg_search_lcu, encoderstate.c:841-853), so that an output picture becomes final CTU by CTU and a per-CTU flag releases the CTUs of the
// pictures behind.  ref_in_call[i * 16 + k]: the index (< i) of the picture of this call whose OUTPUT (filters[].out_*, pictures[].motion_out)
// is reference k of picture i, or -1 for a reference complete before the call.  Requirements beyond uvghip_ctu_search_pb: params.qp ==
// params.qp_c == frame_qp; a picture with a reference inside the call has inflight_margin = 11 (sao_type != 0) or 9.  Workspace:
// uvghip_ctu_search_pb_workspace_bytes.  Everything is enqueued on `stream` in stream order; nothing waits for the device.
// searched_flags (may be NULL): [n_pictures], non-NULL for a picture whose SEARCH runs in another launch beside this one (an I picture in
// uvgi_ctu_plan_launch; slice_type 2, its filters only, CTU by CTU behind that launch's flags).  That launch must already be LAUNCHED and its
// flags zeroed in stream order before this call's kernel; other_workgroups (0..512, and 0 when searched_flags is NULL) is its grid, which this
// launch leaves the CUs for.
int uvgi_search_pb_inflight(int bitdepth, const uvghip_ctu_pb_picture_t *pictures, const uvgi_pb_filter *filters, const int32_t *ref_in_call,
                            const int32_t *const *searched_flags, int other_workgroups, int n_pictures, void *workspace, void *stream);
// where the in-flight launch raises a picture's per-CTU "final" flags (picture i at [i * ctus]): a consumer of the finished pictures that
// runs beside the launch waits on them (uvgi_encode_slice_rows_behind).  The launch zeroes them in stream order before its kernel.
const int32_t *uvgi_search_pb_inflight_final_flags(int n_pictures, int pic_w, int pic_h, const void *workspace);

// ---- slice_coder.hip ------------------------------------------------------------------------------------------------------------------
// The coder's picture table in `workspace` (uvghip_slice_rows_workspace_bytes): ordered == false uploads it synchronously (once, for a
// table that later runs reuse: uvghip_encode_slice_rows with pictures == NULL); ordered == true in stream order on `st` (callers that take
// a stream: nothing waits for it).
int uvgi_slice_rows_prepare(const uvghip_ctu_params_t *params, const uvghip_ctu_picture_t *pictures, int n_pictures, void *workspace, bool ordered, hipStream_t st);
// uvghip_encode_slice_rows with the table already prepared, over the CTU rows [row0, row1) of every picture: one wave per row of the band; a
// row's start models and its SAO models come from the buffers (the first CTU of the row above: of the band above for row0).
int uvgi_encode_slice_rows_band(int bitdepth, const uvghip_ctu_params_t *params, int n_pictures, const int32_t *sao_info, const uint16_t *sao_models, int row0, int row1,
                                void *workspace, uint8_t *out, int row_cap, int32_t *row_bytes, void *stream);
// uvghip_encode_slice_rows with the table already prepared, for pictures whose search is complete but whose in-loop filters (the SAO
// decisions the slice data carries) are finished by ANOTHER launch beside this one: a row waits for each of its CTUs' final_flags
// ([picture][ctu]) and for the first CTU of the row above (its SAO models).  The caller orders the flags' zeroing before this call's
// stream position.
// ticket == NULL: one wave per row (I pictures in the flight, uvgi_search_pb_inflight_final_flags).
// ticket != NULL: at most max_waves rows in progress -- persistent waves take row r of every picture, then row r + 1, from `ticket` (one
// int32 of DEVICE memory the caller zeroes in stream order before the launch): behind a search that is still RUNNING a waiting row must not
// hold what the search needs, and a wave per row of a whole clip does (uvghip_loop_plan_run_overlapped, uvgi_filter_final_flags).
int uvgi_encode_slice_rows_behind(int bitdepth, const uvghip_ctu_params_t *params, int n_pictures, const int32_t *sao_info, const uint16_t *sao_models,
                                  const int32_t *final_flags, int32_t *ticket, int max_waves, void *workspace, uint8_t *out, int row_cap,
                                  int32_t *row_bytes, void *stream);

// ---- loop_plan.hip: the all-intra loop plan, for loop_pb.hip (I pictures in the flight: uvghip_loop_pb_run_inflight_intra) -------------
struct uvghip_loop_plan {
  int bitdepth, n, w, h, sao_type, ctus;
  int row0 = 0, row1 = 0;                 // the CTU rows the plan runs (uvghip_loop_plan_create_rows; the whole picture: 0, hc)
  uvghip_ctu_plan_t *search;
  std::vector<uvghip_loop_picture_t> pics;
  // carved out of the caller's workspace
  int32_t *sao_info;
  uint16_t *sao_models;
  void *coder_ws;                         // the slice coder's picture table
  uint8_t *rows;                          // the slice data: row r of picture p at rows + (p * hc + r) * row_cap
  int32_t *row_bytes;
  int row_cap, hc;
  uint32_t *sums;                         // per picture: the three plane checksums of the hash SEI (filled on demand)
  uvghip_ctu_params_t ctu_params;
  void *filt_ws;                          // the filter stage (uvgi_filter_run)
  int32_t *coder_ticket;                  // uvghip_loop_plan_run_overlapped: the persistent coder's row counter
  // two streams and three events of the plan's own for what runs BESIDE the search (uvgi_loop_plan_side_streams)
  hipStream_t side[2] = {nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_side[2] = {nullptr, nullptr};
  // uvghip_loop_plan_group_nals: the rows of the whole group gathered on the device and brought over in one copy (grown on demand)
  uint8_t *pack_dev = nullptr, *pack_host = nullptr;
  size_t pack_cap = 0;
  unsigned long long *pack_base = nullptr;    // device: [n + 1] byte offsets of the pictures in the packed buffer, then [n] row pitches
  // a band plan's hand-over (uvghip_loop_plan_halo*): what it receives from the band above [0] / sends to the band below [1], all pictures
  std::vector<uvghip_halo_piece_t> halo[2];
  std::vector<size_t> halo_at[2];         // each piece's offset in the packed message
  size_t halo_bytes = 0;
  void *halo_dev[2] = {nullptr, nullptr}; // device: the two piece tables of the pack / unpack kernels
};
int uvgi_loop_plan_side_streams(uvghip_loop_plan *pl);

// ---- the P / B slice descriptor the coder takes, from the picture's search descriptor (loop_pb.hip) -----------------------------------
inline uvghip_slice_pb_t uvgi_slice_pb_of(const uvghip_ctu_pb_picture_t &s)
{
  uvghip_slice_pb_t d;
  memset(&d, 0, sizeof d);
  d.slice_type = s.slice_type; d.poc = s.poc; d.n_refs = s.n_refs;
  for (int k = 0; k < 16; ++k) { d.ref_pocs[k] = s.ref_pocs[k]; d.l[0][k] = s.l[0][k]; d.l[1][k] = s.l[1][k]; }
  d.l_size[0] = s.l_size[0]; d.l_size[1] = s.l_size[1];
  d.tmvp = s.tmvp; d.max_merge = s.max_merge; d.merge_level = s.merge_level; d.frame_qp = s.frame_qp;
  d.col = s.ref_motion[s.l[0][0]]; d.col_stride = s.ref_motion_stride;
  d.inter4 = s.inter4; d.models_inter = s.models_inter;
  return d;
}
