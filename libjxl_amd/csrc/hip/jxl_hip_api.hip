// libjxl_amd — implementation of the thin extern "C" HIP layer declared in include/jxl_amd_hip.h.
// One context = one HIP stream + the device buffers of one frame. Launch functions never allocate or synchronise
// (jxlhip_frame_upload does the allocation), so a caller may capture jxlhip_run_* into a hipGraph.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <unistd.h>
#include <mutex>
#include <new>
#include <chrono>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/jxl_amd_hip.h"
#include "../host/jxh_enc_shared.h"
#include "../host/jxh_filter_plan.h"
#include "../host/jxh_lane_plan.h"
#include "../host/jxh_modular_launch_plan.h"
#include "../host/jxh_modular_upload_plan.h"
#include "../host/jxh_reduced_plan.h"
#include "../host/jxh_window_plan.h"
#include "../host/jxh_resample_plan.h"
#include "../host/jxh_set_memo.h"
#include "../host/jxh_tensor_out.h"
#include "../host/jxh_transform_plan.h"
#include "../host/jxh_upload_plan.h"
#include "jxl_hip_kernels.h"
#include "jxl_hip_entropy_lanes.h"
#include "jxl_hip_filter_fused.h"
#include "jxl_hip_modular.h"
#include "jxl_hip_enc.h"
#include "jxl_hip_canvas.h"
#include "jxl_hip_dc.h"
#include "jxl_hip_resample.h"
#include "jxl_hip_reduced.h"
#include "jxl_hip_dc_window.h"

namespace reduced = jxlhip::reduced;
namespace upload = jxlhip::upload;
namespace tensor_out = jxlhip::tensor_out;
namespace resample = jxlhip::resample;
namespace lane_plan = jxh::lane_plan;
namespace modular_launch = jxh::modular_launch;
namespace filter_plan = jxh::filter_plan;
namespace transform_plan = jxh::transform_plan;
struct JxlHipContext;
using SetMemo = jxh::SetMemo<JxlHipContext>;  // the set a batched launch's description was built for (jxh_set_memo.h)

namespace {
#include "../host/afv_basis.inc"
#include "../host/dither.inc"

#define HIP_TRY(expr)                          \
  do {                                         \
    hipError_t e_ = (expr);                    \
    if (e_ != hipSuccess) return -int(e_);     \
  } while (0)

// "blocking_sync" option: waits of this library poll + sleep (hipStreamSynchronize / hipEventSynchronize spin).
std::atomic<bool> g_yield_waits{false};
inline hipError_t WaitStream(hipStream_t st) {
  if (!g_yield_waits.load(std::memory_order_relaxed)) return hipStreamSynchronize(st);
  for (;;) {
    const hipError_t q = hipStreamQuery(st);
    if (q != hipErrorNotReady) return q;
    usleep(200);
  }
}
inline hipError_t WaitEvent(hipEvent_t ev) {
  if (!g_yield_waits.load(std::memory_order_relaxed)) return hipEventSynchronize(ev);
  for (;;) {
    const hipError_t q = hipEventQuery(ev);
    if (q != hipErrorNotReady) return q;
    usleep(100);
  }
}

// JXLHIP_GUARD=1 (debug aid, read at every allocation): every device buffer gets a guard band either side, filled with a
// pattern that jxlhip_check_guards() verifies: stray WRITES of a kernel next to its buffers show up in a test instead of
// silently landing in a neighbour. Stray READS: the pattern is JXLHIP_GUARD_BYTE (default 0xA5), and a fresh allocation is
// filled with it as a whole; a decode whose result changes with the pattern has read a guard band or memory nothing wrote
// (tests/test_gpu_parity.py::test_no_result_depends_on_bytes_outside_the_buffers runs the kernels under three patterns).
constexpr size_t kGuardBytes = 4096;
inline bool GuardOn() {
  const char* e = getenv("JXLHIP_GUARD");
  return e && *e && atoi(e) != 0;
}
inline int GuardByte() {
  const char* e = getenv("JXLHIP_GUARD_BYTE");
  return e && *e ? (int(strtol(e, nullptr, 0)) & 0xFF) : 0xA5;
}

struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  bool view = false;  // p points into another allocation (a frame's table blob): nothing to free
  void* base = nullptr;  // the allocation when it has guard bands (p = base + kGuardBytes), else NULL
  int guard_byte = 0xA5;  // the pattern its bands were filled with
  int Ensure(size_t n) {
    if (view) {
      p = nullptr;
      cap = 0;
      view = false;
    }
    if (n <= cap && p) return 0;
    if (p) {
      hipError_t e = hipFree(base ? base : p);
      p = base = nullptr;
      cap = 0;
      if (e != hipSuccess) return -int(e);
    }
    size_t want = n < 256 ? 256 : n;
    if (GuardOn()) {
      want = (want + 255) & ~size_t(255);
      hipError_t e = hipMalloc(&base, want + 2 * kGuardBytes);
      guard_byte = GuardByte();
      if (e == hipSuccess) e = hipMemset(base, guard_byte, want + 2 * kGuardBytes);  // (bands and body: see GuardByte)
      // (hipMemset returns before the fill has run, and the contexts' non-blocking streams do not wait for the null
      // stream: without this the fill can land on top of a table copy that was enqueued after it)
      if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
      if (e != hipSuccess) {
        if (base) (void)hipFree(base);
        base = nullptr;
        return -int(e);
      }
      p = static_cast<uint8_t*>(base) + kGuardBytes;
      cap = want;
      return 0;
    }
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
      p = nullptr;
      return -int(e);
    }
    cap = want;
    return 0;
  }
  void Free() {
    if (p && !view) (void)hipFree(base ? base : p);
    p = base = nullptr;
    cap = 0;
    view = false;
  }
  // 0 = both guard bands intact (or none), 1 = the band before, 2 = the band after, 3 = both were written to
  int GuardsTouched() const {
    if (!base || view) return 0;
    std::vector<uint8_t> h(2 * kGuardBytes);
    if (hipMemcpy(h.data(), base, kGuardBytes, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    if (hipMemcpy(h.data() + kGuardBytes, static_cast<uint8_t*>(base) + kGuardBytes + cap, kGuardBytes, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    int r = 0;
    for (size_t i = 0; i < kGuardBytes; i++) {
      if (h[i] != guard_byte) r |= 1;
      if (h[kGuardBytes + i] != guard_byte) r |= 2;
    }
    return r;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};

struct PassBufs {
  Buf ctx_map, alias, cfg, orders, ptable, poffset, alias_packed;
};

using ModLaunch = upload::ModLaunch;  // one launch of the Modular transform / output kernels over the frames of a set

// Pinned host staging block of a context: every table of a frame is assembled in it and leaves through asynchronous
// copies on the context's stream, so that an upload neither blocks on pageable-memory copies nor synchronises per table.
// The block is reused by the next upload once `done` (recorded after the upload's last copy) has passed.
struct Stage {
  uint8_t* p = nullptr;
  size_t cap = 0, used = 0;
  hipEvent_t done = nullptr;
  bool recorded = false;
};

constexpr int kEntropyWPG = 4;  // waves (= AC sections) per workgroup of the scalar-form entropy kernel
// The LDS a frame's lane-kernel workgroup may need at most, in waves of 64 lanes: the test that admits a frame to the lane
// kernel (jxlhip_frame_upload) still budgets four, though every launch now runs one wave per workgroup.
constexpr int kLanesAdmitWaves = 4;
constexpr size_t kLdsBudget = 150 * 1024;

}  // namespace

struct JxlHipContext {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[6] = {};
  bool ev_valid[3] = {false, false, false};
  Buf basis;
  Stage stage;
  // jxlhip_frame_upload: every table of the frame lives in one device allocation laid out like the staging block, filled
  // by ONE host-to-device copy at the end of the upload (HIP serialises API calls of all host threads: twenty small
  // copies per frame capped a multi-threaded uploader at ~0.6 ms per frame); the tables' Bufs are views into it.
  Buf frame_blob;
  bool have_frame = false;
  // geometry
  uint32_t xs = 0, ys = 0, xb = 0, yb = 0, xg = 0, ng = 0, np = 0, xp = 0, yp = 0, coef_bits = 16;
  int gab = 0, epf_iters = 0;
  float epf_pass0 = 0.9f, epf_pass2 = 6.5f, epf_border = 2.0f / 3;
  // buffers
  Buf sections, sec_word, sec_size, blocks, gbb, bctx_lut, dequant, dc, inv_sigma, ytox, ytob, passes_dev, coeffs, errors;
  Buf dc_q, dc_ep;    // coded DC integers and the DC groups' extra-precision bytes (DequantDC on the device)
  Buf dc_raw, sharp;  // inputs of the DC-path kernels (jxl_hip_dc.h) when the upload smooths the DC image / computes 1 / sigma
  Buf plane[3], rgb, tlist, scratch, sec_end, lz_window;
  bool generic_codec = false;  // a pass is prefix-coded or uses LZ77 (k_entropy_generic decodes the frame unless lane_prefix)
  bool lane_prefix = false;    // every pass is prefix-coded without LZ77: the lane kernel's prefix form decodes the frame
  // ---- Modular frame (jxlhip_modular_upload): channel pool, tables, stream descriptors, inverse-transform operations
  struct Modular {
    bool have = false;
    Buf pool, sections, blob, streams, rects, status, end_bits, scratch, windows, batch_streams;
    std::vector<size_t> buf_off;            // per channel buffer: first int32 of the pool
    std::vector<uint32_t> buf_w, buf_h;
    std::vector<JxlHipModOp> ops;
    std::vector<jxlhip::ModStream> streams_host;  // device pointers filled in
    std::vector<uint32_t> stream_samples;
    uint32_t out_buffer[4] = {0, 0, 0, 0};
    uint32_t num_color = 3, has_alpha = 0, bits = 8, alpha_bits = 8, xs = 0, ys = 0, nstreams = 0;
    bool xyb = false;  // XYB Modular frame: integer Y, X, B - Y channels, the colour stage's parameters in `xyb_color`
    float xyb_factor[3] = {0, 0, 0};
    jxlhip::FilterParams xyb_color;
    JxlHipColorTarget xyb_target;
    std::vector<uint32_t> code_table_words;  // per entropy code: words of its symbol tables (ModCode::table_words)
    // jxlhip_modular_run_batch (PrepareModBatch): the set batch_plan was made for, under batch_lanes_override;
    // batch_streams holds the set's stream descriptors in launch order
    SetMemo batch_set;
    int batch_lanes_override = 0;  // JXLHIP_MOD_LANES (measurement aid) as the plan was made under it
    modular_launch::ModBatchPlan batch_plan;
    Buf batch_ops;  // parameter blocks of the set's transform / output launches
  } mod;
  size_t plane_bytes = 0;  // bytes of plane[0] the current frame needs
  Buf ep_dev;                         // device copy of `ep` (the entropy kernel reads it through the scalar cache)
  Buf batch_params, batch_map, batch_lanes;  // jxlhip_run_entropy_batch: parameter blocks, workgroup map, lane map
  lane_plan::LanePlan batch_plan;            // ... and what the launch reads of them (PrepareBatch; jxh_lane_plan.h)
  lane_plan::LaneOverrides batch_overrides;  // the measurement aids the batch was planned under
  int batch_kernel = -1;
  // JXLHIP_LANES_PROF=2 (measurement aid): the per-wave records of the last kTimelineKeep lane-kernel launches
  Buf lanes_timeline;
  size_t timeline_launches = 0, timeline_stride = 0, timeline_wgs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<uint32_t> sec_size_host, sec_sel_host, pass_clusters, pass_log_alpha;
  // Coefficient layout of this frame (see TransformParams::scan_order); scan order is produced by k_entropy_lanes.
  // band decode: groups this context decodes (band + one group row either side), pixel rows it produces
  std::vector<uint32_t> group_list;
  std::vector<uint32_t> absent_groups;  // JxlHipFrameDesc::group_absent: drawn from the DC image alone
  std::vector<uint32_t> absent_blocks;  // per absent group: first block, block count
  std::vector<uint32_t> absent_sections;  // (partial frames) passes of present groups that have not arrived: pass, first block, block count
  uint32_t band_y0 = 0, band_y1 = 0;
  uint32_t ext_y0 = 0, ext_y1 = 0;  // the pixel rows the transforms produce (the band and the group rows decoded around it)
  // upsampled frames: factor (1 = none), image size, kernels
  uint32_t ups = 1, oxs = 0, oys = 0;
  Buf ups_kernel;
  bool scan_order = false;
  // lanes: the frame's entropy stage runs on k_entropy_lanes. Single-pass frames hand the scan-order layout to the
  // transforms (scan_order); progressive frames (lane_multi) decode every pass into its own scan-order buffer and
  // k_merge_passes sums them into the natural layout.
  bool lanes = false, lane_multi = false;
  uint32_t nblocks = 0;
  bool keep_filtered = false;  // jxlhip_set_option("keep_filtered"): also write the filtered XYB planes (tests)
  bool keep_upsampled = false;  // jxlhip_set_option("keep_upsampled"): an upsampled frame's X, Y, B at the image's size stay (tests)
  bool ups_kept = false;        // ... and the uploaded frame was set up for it (ups_planes holds them after the filter launch)
  bool transform_dense = false;  // jxlhip_set_option("transform_dense"): TransformParams::dense at the next upload (tests)
  bool band_halo = false;      // jxlhip_set_option("band_halo"): a band decodes ONLY its own group rows; the rows of the
                               // neighbouring bands that its filters read arrive through jxlhip_halo_unpack
  // output pixel format (jxlhip_set_output_format; JxlDataType numbering): RGB8 by default
  uint32_t out_type = 2, out_nc = 3, out_bits = 8, out_swap = 0;
  // jxlhip_set_output_tensor: the pixels go to the caller's memory in `tensor`'s layout and type instead of `rgb`, which
  // is then not allocated (OutType / OutChannels / OutBits / OutSwap say what the writers make). tensor_fused (set at
  // upload): from k_filter_rows2's tensor form. tensor_event orders the writers against tensor.consumer_stream.
  bool tensor_bound = false, tensor_fused = false;
  JxlHipTensorOut tensor{};
  hipEvent_t tensor_event = nullptr;
  // forward (encoder) path, jxlhip_enc_forward: device buffers and the kernel time of the last call
  Buf enc_rgb, enc_planes[3], enc_act, enc_acs, enc_qf, enc_off, enc_dc, enc_coef, enc_lut, enc_dq, enc_ytox, enc_ytob;
  hipEvent_t enc_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // whole sequence; the transform kernel of its last pass; the two adaptive-quant kernels of its last pass (quant_field_mode 1)
  bool enc_timed = false;
  jxlhip::EncTok enc_tok;      // jxlhip_enc_token_counts -> jxlhip_enc_tokens
  bool enc_tok_ready = false;
  std::vector<uint32_t> enc_tok_totals;
  Buf enc_tok_orders, enc_tok_blk, enc_tok_info, enc_tok_off, enc_tok_nzmap, enc_tok_small, enc_tok_out, enc_tok_base;
  // entropy coding of the resident tokens (jxlhip_enc_histograms, jxlhip_enc_ans_sizes -> jxlhip_enc_ans_write): the groups
  // the tokens in enc_tok_out belong to, the bit lengths of the last sizes call, kernel times
  std::vector<uint32_t> ent_base, ent_count, ent_bits;
  bool ent_resident = false, ent_sized = false, ent_timed[3] = {false, false, false};
  jxlhip::EncAns ent;
  Buf ent_counts, ent_status, ent_grp, ent_tab, ent_rec, ent_fl, ent_small, ent_out, ent_obase;
  hipEvent_t ent_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // histograms; records + chain; scatter
  jxlhip::EncFwd enc_last;     // the parameters of the last jxlhip_enc_forward (its input stays resident): jxlhip_enc_forward_rerun
  jxlhip::EncAq enc_last_aq;   // ... and of its adaptive quant field (quant_field_mode 1)
  Buf enc_aq_cells, enc_aq_map, enc_aq_mask, enc_aq_in;  // cell image, field, masking; the planes of jxlhip_enc_initial_quant_field
  Buf enc_mask1x1;                                        // the per-pixel masking of jxlhip_enc_masking_1x1 (its Y plane goes through enc_aq_in)
  hipEvent_t mask_ev[2] = {nullptr, nullptr};             // ... and its kernel's time
  bool mask_timed = false;
  // jxlhip_enc_estimate_entropy: its inputs (planes, quant field, mask1x1, factors, tables), the sorted candidates with
  // their places and `scaled` offsets, and its outputs; its kernels' time
  Buf est_planes, est_qf, est_mask, est_ytox, est_ytob, est_dq, est_cand, est_index, est_at, est_out, est_scaled;
  hipEvent_t est_ev[2] = {nullptr, nullptr};
  bool est_timed = false;
  bool enc_last_gaborish = false;
  uint32_t out_orient = 0;  // jxlhip_set_output_orientation: PixelOut::orient bits (0 = the image as coded)
  bool out_unpremul = false;  // jxlhip_set_output_unpremultiply (PixelOut::orient bit 3 for outputs that carry alpha)
  // splines (JxlHipSplines): the draw cache on the device; for a Modular frame also the float planes they are drawn over
  Buf spl_seg, spl_row_start, spl_row_seg, spl_planes;
  uint32_t spl_segments = 0;
  // patches (JxlHipPatches): records and row lists on the device, the reference planes they read
  Buf pat_rec, pat_row_start, pat_row_list;
  uint32_t pat_positions = 0;
  const float* pat_src[4] = {nullptr, nullptr, nullptr, nullptr};
  const float* pat_src_alpha[4] = {nullptr, nullptr, nullptr, nullptr};
  bool pat_uses_alpha = false, pat_premultiplied = false;
  // the alpha plane the patch stage blended into (a copy: the plane that was set stays as it is, the stages can run again);
  // valid from the filter stage of such a frame on
  Buf alpha_patched;
  bool alpha_patched_valid = false;
  uint32_t pat_src_w[4] = {0, 0, 0, 0}, pat_src_h[4] = {0, 0, 0, 0};
  bool keep_xyb = false;  // option "keep_xyb_planes": a Modular frame also leaves its colour as float planes (spl_planes)
  // noise synthesis (JxlHipFrameDesc::has_noise): raw random planes [3][ys][xs], LUT, seeds, base colour correlation
  Buf noise;
  bool has_noise = false;
  float noise_lut[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t noise_seed[2] = {0, 0};
  float noise_ytox = 0.0f, noise_ytob = 1.0f;
  Buf alpha;                // f32 plane of the image size (jxlhip_set_alpha), used by 2- and 4-channel output
  bool have_alpha = false;
  bool color_out = false;   // the pixels come from k_color_out / k_upsample_color's generic writer (set at upload)
  bool gray8_fast = false;  // one 8-bit sRGB channel from k_filter_rows2's one-channel form: fp.rgb has 1 byte per pixel (set at upload)
  JxlHipColorTarget ct{};   // JxlHipFrameDesc::color_target of the frame: its output encoding (tf != 0: the generic writer)
  Buf kend, block_recs, dequant_scan;
  Buf trecs;     // the transform work lists as 16-byte varblock records (TransformParams::trecs)
  Buf ec_stage;  // jxlhip_upsample_plane: a coded extra channel, its kernels and (unless it becomes the alpha plane) the result
  std::vector<JxlHipVarBlock> blocks_host;  // for jxlhip_download("coeffs") of a scan-order frame
  std::vector<uint32_t> gbb_host;
  std::vector<uint16_t> orders_host;
  uint32_t order_offset_host[39] = {};
  SetMemo batch_set;  // jxlhip_run_entropy_batch: the set batch_plan was made for, under batch_kernel and batch_overrides
  hipEvent_t batch_done = nullptr;
  // Set by jxlhip_run_entropy_batch on the contexts whose coefficients a launch on ANOTHER context's stream produces;
  // applied (hipStreamWaitEvent on this context's stream) by the next call that touches those results. Enqueuing the
  // wait only then keeps barrier packets of a long entropy launch out of the hardware queues other streams share.
  hipEvent_t pending_wait = nullptr;
  // jxlhip_share_planes: this context's inverse-transform output lives in `plane_lender`'s plane buffer (NULL: its own).
  // planes_event (on the context that owns the buffer): end of the last filter launch that read the buffer, recorded on
  // planes_stream; a transform launch from another stream waits for it before overwriting the planes.
  // Option "filter_async": batched filter + colour launches from this context go to its SECOND stream, ordered after
  // what the first stream holds at that moment; the first stream is then free for the next entropy launch (which touches
  // neither the planes nor the pixels) while the filter still runs. filter_wait (on every context of such a launch):
  // the launch's end event; waited for by whatever touches the planes or the pixels next (transform, download, sync,
  // upload), never by an entropy launch.
  bool filter_async = false;
  bool entropy_gate = false;  // option "entropy_gate" (see EntropyGate)
  hipEvent_t halo_event = nullptr;  // jxlhip_halo_*_batch: orders the halo copies against the transport's stream
  Buf ups_planes;                   // upsampled X, Y, B planes of a frame with noise ([3][oys][oxs padded to 8])
  bool pooled_once = false;         // the object has been through the context pool (RecycleContext frees it for good)
  bool owns_stream = false;   // `stream` is this context's own (it heads batched launches), not one of the shared pool
  hipStream_t stream2 = nullptr;
  hipStream_t fstream = nullptr;  // stream of the filter launch in progress (set by BeginDownstreamBatch)
  hipEvent_t fork_event = nullptr, filter_done = nullptr, filter_wait = nullptr;
  hipEvent_t transform_done = nullptr;  // filter_async: end of the set's last batched transform launch on `stream`
  bool transform_done_valid = false;
  JxlHipContext* plane_lender = nullptr;
  hipEvent_t planes_event = nullptr;
  hipStream_t planes_stream = nullptr;
  // jxlhip_run_transform_batch / jxlhip_run_filter_color_batch: description of the frame set launched from this context
  // (tlaunches: the transform launches, jxh_transform_plan.h, over tb_desc; tblocks: the frames' transform blocks as
  // resolved for the set, i.e. with the plane holder's buffer, the host copy of tb_params; fgroups: the filter launches,
  // jxh_filter_plan.h; fb_params holds the frames' blocks in the plan's order). down_set: the set all of it was built for,
  // with each frame's plane buffer, which a lender's upload may have reallocated without the borrower's generation moving.
  Buf tb_params, tb_desc, fb_params;
  SetMemo down_set;
  std::vector<jxlhip::TransformParams> tblocks;
  std::vector<transform_plan::TransformLaunch> tlaunches;
  uint32_t cs = 0;  // chroma-subsampled frame: hshift of channel c in bit 2 * c, vshift in bit 2 * c + 1 (0 = 4:4:4)
  std::vector<filter_plan::FilterGroup> fgroups;
  hipEvent_t down_done = nullptr;
  uint64_t generation = 0;            // bumped by every jxlhip_frame_upload
  std::vector<PassBufs> pass_bufs;
  uint32_t list_begin[27] = {}, list_count[27] = {};
  jxlhip::EntropyParams ep;
  jxlhip::TransformParams tp;
  jxlhip::FilterParams fp;
  size_t lds_entropy = 0;
  bool alias_lds = false;
  int final_plane = 0;  // which plane set holds the filtered XYB after jxlhip_run_filter_color
  // the AC-strategy search of the forward path (strategy_mode 2, 3): its own mask1x1, zero chroma-from-luma factors, the
  // candidate list of the frame size it was last built for (srch_xb x srch_yb blocks, srch_floating; kind k is
  // srch_first[k] .. srch_first[k + 1]) with the index array k_enc_estimate writes through, and the walk's table; the times
  // of mask1x1, the estimate launches and the walk in the last pass. jxlhip_enc_acs_walk has buffers of its own.
  // (Behind everything else, so that no member the decode stages read moves.)
  Buf srch_mask, srch_zero, srch_cand, srch_index, srch_table, walk_table, walk_acs, walk_entropy;
  uint32_t srch_xb = 0, srch_yb = 0, srch_floating = 0;
  size_t srch_first[jxh::kAcsWalkKinds + 1] = {};
  hipEvent_t srch_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // jxlhip_set_output_resized: the context renders f32 pixels of resized.tensor.num_channels channels into `rgb` as for
  // jxlhip_set_output_format(0, nc, 0, 0), and the resample passes (jxl_hip_resample.h) take a box of them to the caller's
  // tensor. rs_block (placed at upload): the descriptor and the two tap tables; rs_dev: the descriptor's host copy, from
  // which a batched launch builds its array (rs_batch on the launch's first context, kept while the set stays the same);
  // rs_tmp: the rows between the passes; rs_src: jxlhip_debug_resample's source.
  bool resized_bound = false;
  JxlHipResizedOut resized{};
  resample::ResampleDev rs_dev{};
  Buf rs_block, rs_tmp, rs_src, rs_batch;
  SetMemo rs_batch_set;
  // jxlhip_reduced_upload: the context holds the inputs of a reduced image instead of a frame (have_frame and mod.have are
  // then both false). red_block (placed at upload, one staged copy): the kernel's descriptor, the DC groups' precision bytes
  // and the coded integers (jxh_reduced_plan.h BlockLayout); red.dev: the descriptor's host copy, from which a batched launch
  // builds its array (red_batch on the launch's first context, kept while the set stays the same). The pixels go to `rgb`
  // or the bound tensor, the kept DC planes (option "keep_dc") to `dc`.
  bool keep_dc = false;
  struct Reduced {
    bool have = false, ran = false, dc_kept = false;
    uint64_t generation = 0;  // the context's, as the upload left it: output settings changed since ask for another upload
    jxlhip::ReducedDev dev{};
    SetMemo batch_set;
    uint32_t batch_tiles = 0;
  } red;
  Buf red_block, red_batch;
  // jxlhip_dc_window: the apron's integers with the frame's precision bytes behind them (one staged copy), and the window's
  // three float planes, which the window's frame upload takes as its dc_device (`dc` is then a view of dcw_out).
  Buf dcw_in, dcw_out;
};

// JXLHIP_ENTROPY=1 (a test hook): no frame takes the lane-parallel k_entropy_lanes, every frame the wave-per-section
// fallback (k_entropy_uni, or k_entropy_ans for tables beyond the LDS budget) that multi-pass frames and large tables take.
static bool SectionEntropyForced() {
  static const bool v = [] {
    const char* e = getenv("JXLHIP_ENTROPY");
    return e && e[0] == '1';
  }();
  return v;
}
static JxlHipContext* PlaneHolder(JxlHipContext* c) { return c->plane_lender ? c->plane_lender : c; }
static const JxlHipContext* PlaneHolder(const JxlHipContext* c) { return c->plane_lender ? c->plane_lender : c; }

// The sample format the writers make: the bound tensor's, else jxlhip_set_output_format's.
// (a resized binding: what jxlhip_set_output_format(ctx, 0, num_channels, 0, 0) would have set, into the context's own buffer)
static uint32_t OutType(const JxlHipContext* c) { return c->tensor_bound ? c->tensor.dtype : (c->resized_bound ? 0u : c->out_type); }
static uint32_t OutChannels(const JxlHipContext* c) {
  return c->tensor_bound ? c->tensor.num_channels : (c->resized_bound ? c->resized.tensor.num_channels : c->out_nc);
}
static uint32_t OutBits(const JxlHipContext* c) { return c->tensor_bound ? 8u : (c->resized_bound ? 16u : c->out_bits); }
static uint32_t OutSwap(const JxlHipContext* c) { return c->tensor_bound || c->resized_bound ? 0u : c->out_swap; }
static size_t OutSampleBytes(const JxlHipContext* c) { return c->resized_bound ? 4 : (c->out_type == 2 ? 1 : (c->out_type == 0 ? 4 : 2)); }
static size_t OutPixelBytes(const JxlHipContext* c) { return OutSampleBytes(c) * (c->resized_bound ? c->resized.tensor.num_channels : c->out_nc); }
// (the context's own RGB8 rows: never a tensor, whatever its type)
static bool OutIsRgb8(const JxlHipContext* c) {
  return !c->tensor_bound && !c->resized_bound && upload::OutIsRgb8(c->out_type, c->out_nc, c->out_bits);
}
// The pixels are the caller's (a bound tensor) or feed the caller's tensor (a resized binding): downloads, bands and
// canvases are refused alike. The tensor whose consumer stream the writes are ordered against.
static bool CallerOwnsPixels(const JxlHipContext* c) { return c->tensor_bound || c->resized_bound; }
static const JxlHipTensorOut* CallerTensor(const JxlHipContext* c) {
  return c->tensor_bound ? &c->tensor : (c->resized_bound ? &c->resized.tensor : nullptr);
}
// Room of the context's own pixel buffer for the frame: none while a tensor is bound.
static size_t OwnPixelBytes(const JxlHipContext* c) { return c->tensor_bound ? 0 : size_t(c->oxs) * c->oys * OutPixelBytes(c); }

// The generic writers' block for an image of xsize x ysize: orientation and un-premultiplication, then where and how they
// store: the context's interleaved rows, or the bound tensor.
static void FillPixelOut(const JxlHipContext* c, uint32_t xsize, uint32_t ysize, float* alpha, jxlhip::PixelOut* po) {
  po->alpha = alpha; po->xsize = xsize; po->ysize = ysize;
  po->orient = c->out_orient | (c->out_unpremul ? 8u : 0u);
  po->type = OutType(c);
  po->nc = OutChannels(c);
  po->bits = OutBits(c);
  po->swap = OutSwap(c);
  if (c->tensor_bound) {
    const JxlHipTensorOut& t = c->tensor;
    po->dst = t.data;
    po->stride_c = t.stride_c;
    po->stride_y = t.stride_y;
    po->stride_x = t.stride_x;
    po->tensor = 1;
    po->clamp01 = t.clamp01 ? 1 : 0;
    memcpy(po->scale, t.scale, sizeof(po->scale));
    memcpy(po->bias, t.bias, sizeof(po->bias));
    return;
  }
  po->dst = c->rgb.p;
  jxlhip::SetInterleaved(po, (po->orient & 4) ? po->ysize : po->xsize);
}

static int EnvInt(const char* name, int def) {
  const char* e = getenv(name);
  return e && *e ? atoi(e) : def;
}
// The measurement aids of the lane launch plan (jxh_lane_plan.h LaneOverrides). JXLHIP_WG_ORDER = 0 emits the lane kernel's
// workgroups in frame order, 2 in frame order dealt over the XCDs (jxh_launch_order.h kDealt); 1, the default and what
// any other value means: longest estimated unit first.
static lane_plan::LaneOverrides LaneOverridesFromEnv() {
  lane_plan::LaneOverrides o;
  o.lanes_per_wave = EnvInt("JXLHIP_LANES", 0);
  o.table_form = EnvInt("JXLHIP_GALIAS", -1);
  o.a6 = EnvInt("JXLHIP_A6", 1);
  o.wg_order = EnvInt("JXLHIP_WG_ORDER", 1);
  if (o.wg_order < 0 || o.wg_order > 2) o.wg_order = 1;
  o.wait_shift = uint32_t(EnvInt("JXLHIP_WAIT_SHIFT", 1));
  return o;
}

extern "C" {

const char* jxlhip_version(void) { return "libjxl_amd 0.1 (gfx950)"; }

int jxlhip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// Streams. A context does NOT get a HIP stream of its own: with more than ~16 streams alive in a process (used or not) the
// runtime time-slices its hardware queues, and a long kernel is then preempted and resumed several times over (rocprofv3
// counts each resumption as a wave: SQ_WAVES 251 for a 32-wave launch); scripts/r03_streams_probe2.py: the same 8-frame
// entropy launch takes 79 ms with up to 16 streams in the process, 114 ms with 32, 125 ms with 64. Contexts share a small
// pool per device (JXLHIP_STREAMS, default 4); a context that heads batched launches over several contexts gets a
// dedicated stream the first time it does (EnsureOwnStream), so that the batched stages of different frame sets overlap.
static hipStream_t PoolStream(int device) {
  static std::mutex mu;
  static std::vector<hipStream_t> pool[64];
  static size_t next[64] = {};
  std::lock_guard<std::mutex> lock(mu);
  if (device < 0 || device >= 64) return nullptr;
  if (pool[device].empty()) {
    int n = 4;
    if (const char* e = getenv("JXLHIP_STREAMS")) n = atoi(e);
    n = n < 1 ? 1 : (n > 16 ? 16 : n);
    for (int i = 0; i < n; i++) {
      hipStream_t st = nullptr;
      if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) break;
      pool[device].push_back(st);
    }
    if (pool[device].empty()) return nullptr;
  }
  return pool[device][next[device]++ % pool[device].size()];
}

// The head context of a batched launch runs the batch on a stream of its own (created on first use).
static int EnsureOwnStream(JxlHipContext* c);

// Contexts that callers have destroyed are kept, a few per process, with their device buffers, pinned staging block and
// events: a caller that creates a decoder per image (JxlDecoderCreate .. JxlDecoderDestroy, what djxl does) otherwise pays
// for the basis tables, a dozen hipMalloc of up to 100 MB and as many hipFree (each a device synchronisation) on every
// image: 5 - 9 ms of a 27 ms 4K decode. A recycled context is a NEW JxlHipContext object (every option and per-frame field
// at its default) that takes over the old one's allocations. Off with JXLHIP_CTX_POOL=0 and in guard mode (whose tests
// want fresh, pattern-filled allocations).
static std::mutex g_ctx_pool_mu;
static std::vector<JxlHipContext*> g_ctx_pool;
constexpr size_t kCtxPoolMax = 4, kCtxPoolBytes = size_t(1) << 30;
static std::vector<Buf*> AllBufs(JxlHipContext* c);
static JxlHipContext* RecycleContext(int device) {
  if (GuardOn() || !EnvInt("JXLHIP_CTX_POOL", 1)) return nullptr;
  JxlHipContext* o = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_ctx_pool_mu);
    for (size_t i = 0; i < g_ctx_pool.size(); i++)
      if (g_ctx_pool[i]->device == device) {
        o = g_ctx_pool[i];
        g_ctx_pool.erase(g_ctx_pool.begin() + long(i));
        break;
      }
  }
  if (!o) return nullptr;
  JxlHipContext* c = new (std::nothrow) JxlHipContext;
  if (!c) {
    jxlhip_ctx_destroy(o);
    return nullptr;
  }
  c->device = device;
  c->stream = PoolStream(device);
  std::vector<Buf*> to = AllBufs(c), from = AllBufs(o);  // (the new object has no per-pass buffers yet: the common prefix)
  for (size_t i = 0; i < to.size(); i++) {
    *to[i] = *from[i];
    if (to[i]->view) *to[i] = Buf();  // (a view into the old frame's table blob means nothing here)
    *from[i] = Buf();
  }
  c->pass_bufs = std::move(o->pass_bufs);
  o->pass_bufs.clear();
  for (size_t i = 0; i < sizeof(c->ev) / sizeof(c->ev[0]); i++) std::swap(c->ev[i], o->ev[i]);
  for (size_t i = 0; i < sizeof(c->enc_ev) / sizeof(c->enc_ev[0]); i++) std::swap(c->enc_ev[i], o->enc_ev[i]);
  for (size_t i = 0; i < sizeof(c->ent_ev) / sizeof(c->ent_ev[0]); i++) std::swap(c->ent_ev[i], o->ent_ev[i]);
  for (size_t i = 0; i < sizeof(c->mask_ev) / sizeof(c->mask_ev[0]); i++) std::swap(c->mask_ev[i], o->mask_ev[i]);
  for (size_t i = 0; i < sizeof(c->est_ev) / sizeof(c->est_ev[0]); i++) std::swap(c->est_ev[i], o->est_ev[i]);
  for (size_t i = 0; i < sizeof(c->srch_ev) / sizeof(c->srch_ev[0]); i++) std::swap(c->srch_ev[i], o->srch_ev[i]);
  std::swap(c->stage, o->stage);
  jxlhip_ctx_destroy(o);  // (what is left of it: lazily created events, a stream of its own)
  return c;
}

// The DCT basis every context uploads (jxlhip_ctx_create): the [k][n] matrices of N = 1, 2 .. 256, matrix N at float
// (N * N - 1) / 3, and behind them, 16-byte aligned, the transposed [n][k] ones.
constexpr size_t kBasisFloats = 87381;  // (4^9 - 1) / 3
constexpr size_t kBasisTransposed = kBasisFloats + 3;

int jxlhip_ctx_create(int device, JxlHipContext** out) {
  if (!out) return JXLHIP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  HIP_TRY(hipSetDevice(device));
  if (JxlHipContext* recycled = RecycleContext(device)) {
    *out = recycled;
    return 0;
  }
  JxlHipContext* c = new (std::nothrow) JxlHipContext;
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  c->device = device;
  hipError_t e = hipSuccess;
  c->stream = PoolStream(device);
  if (!c->stream) {
    delete c;
    return JXLHIP_ERR_INVALID_ARGUMENT;
  }
  for (auto& ev : c->ev) {
    e = hipEventCreate(&ev);
    if (e != hipSuccess) {
      delete c;
      return -int(e);
    }
  }
  // static tables
  std::vector<float> bt(2 * kBasisFloats + 4);
  for (int l = 0; l <= 8; l++) {
    const int N = 1 << l;
    float* dst = bt.data() + (size_t(N) * N - 1) / 3;
    float* dst_t = dst + kBasisTransposed;
    for (int k = 0; k < N; k++)
      for (int n = 0; n < N; n++) {
        const float v = float((k ? std::sqrt(2.0) : 1.0) * std::cos((n + 0.5) * k * M_PI / N));
        dst[size_t(k) * N + n] = v;
        dst_t[size_t(n) * N + k] = v;
      }
  }
  int r = c->basis.Ensure(bt.size() * sizeof(float));
  if (r) {
    jxlhip_ctx_destroy(c);
    return r;
  }
  float resample[63];
  for (int n = 1; n <= 32; n *= 2)
    for (int i = 0; i < n; i++) {
      const double N = 8.0 * n;
      resample[n - 1 + i] = float(1.0 / (std::cos(i / (2 * N) * M_PI) * std::cos(i / N * M_PI) * std::cos(i / (N / 2) * M_PI)));
    }
  e = hipMemcpy(c->basis.p, bt.data(), bt.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(jxlhip::c_afv_basis), kAfvBasis, sizeof(kAfvBasis));
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(jxlhip::c_dither), kDither32, sizeof(kDither32));
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(jxlhip::c_resample), resample, sizeof(resample));
  if (e != hipSuccess) {
    jxlhip_ctx_destroy(c);
    return -int(e);
  }
  *out = c;
  return 0;
}

static std::vector<Buf*> AllBufs(JxlHipContext* c) {
  std::vector<Buf*> all = {&c->basis, &c->sections, &c->sec_word, &c->sec_size, &c->blocks, &c->gbb, &c->bctx_lut, &c->dequant, &c->dc, &c->dc_raw, &c->dc_q, &c->dc_ep, &c->sharp,
                &c->inv_sigma, &c->ytox, &c->ytob, &c->passes_dev, &c->coeffs, &c->errors, &c->plane[0], &c->plane[1],
                &c->plane[2], &c->rgb, &c->tlist, &c->scratch, &c->ep_dev, &c->batch_params, &c->batch_map, &c->batch_lanes, &c->lanes_timeline, &c->ups_kernel, &c->kend, &c->block_recs, &c->dequant_scan, &c->ec_stage, &c->alpha_patched, &c->trecs, &c->enc_tok_orders, &c->enc_tok_blk, &c->enc_tok_info,
                &c->enc_tok_off, &c->enc_tok_nzmap, &c->enc_tok_small, &c->enc_tok_out, &c->enc_tok_base, &c->tb_params, &c->tb_desc, &c->fb_params, &c->alpha, &c->sec_end, &c->lz_window, &c->mod.pool, &c->mod.sections, &c->mod.blob, &c->mod.streams,
                &c->mod.rects, &c->mod.status, &c->mod.end_bits, &c->mod.scratch, &c->mod.windows, &c->mod.batch_streams, &c->mod.batch_ops, &c->frame_blob, &c->noise, &c->spl_seg, &c->spl_row_start, &c->spl_row_seg, &c->spl_planes, &c->pat_rec, &c->pat_row_start, &c->pat_row_list,
                &c->enc_rgb, &c->enc_planes[0], &c->enc_planes[1], &c->enc_planes[2], &c->enc_act, &c->enc_acs, &c->enc_qf, &c->enc_off, &c->enc_dc, &c->enc_coef, &c->enc_lut, &c->enc_dq, &c->enc_ytox, &c->enc_ytob, &c->ups_planes, &c->enc_aq_cells, &c->enc_aq_map, &c->enc_aq_mask, &c->enc_aq_in, &c->enc_mask1x1,
                &c->est_planes, &c->est_qf, &c->est_mask, &c->est_ytox, &c->est_ytob, &c->est_dq, &c->est_cand, &c->est_index, &c->est_at, &c->est_out, &c->est_scaled,
                &c->srch_mask, &c->srch_zero, &c->srch_cand, &c->srch_index, &c->srch_table, &c->walk_table, &c->walk_acs, &c->walk_entropy,
                &c->rs_block, &c->rs_tmp, &c->rs_src, &c->rs_batch, &c->red_block, &c->red_batch, &c->dcw_in, &c->dcw_out, &c->ent_counts, &c->ent_status, &c->ent_grp, &c->ent_tab, &c->ent_rec, &c->ent_fl, &c->ent_small, &c->ent_out, &c->ent_obase};
  for (auto& pb : c->pass_bufs)
    for (Buf* b : {&pb.ctx_map, &pb.alias, &pb.cfg, &pb.orders, &pb.ptable, &pb.poffset, &pb.alias_packed}) all.push_back(b);
  return all;
}

void jxlhip_ctx_destroy(JxlHipContext* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->stream2) (void)hipStreamSynchronize(c->stream2);
  // (the caller's tensor is the caller's to free from here on: whoever takes this context from the pool starts unbound)
  c->tensor_bound = c->tensor_fused = false;
  c->tensor = JxlHipTensorOut{};
  c->resized_bound = false;
  c->resized = JxlHipResizedOut{};
  if (c->basis.p && !c->pooled_once && !GuardOn() && EnvInt("JXLHIP_CTX_POOL", 1)) {  // keep it for the next jxlhip_ctx_create (see RecycleContext)
    size_t bytes = 0;
    for (Buf* b : AllBufs(c))
      if (!b->view) bytes += b->cap;
    std::lock_guard<std::mutex> lk(g_ctx_pool_mu);
    if (bytes <= kCtxPoolBytes && g_ctx_pool.size() < kCtxPoolMax) {
      c->pooled_once = true;  // (a context leaves the pool through RecycleContext, which destroys the shell for good)
      g_ctx_pool.push_back(c);
      return;
    }
  }
  std::vector<Buf*> all = AllBufs(c);
  for (Buf* b : all) b->Free();
  for (auto& ev : c->ev)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : c->enc_ev)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : c->ent_ev)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : c->mask_ev)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : c->est_ev)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : c->srch_ev)
    if (ev) (void)hipEventDestroy(ev);
  if (c->stage.done) (void)hipEventDestroy(c->stage.done);
  if (c->stage.p) (void)hipHostFree(c->stage.p);
  if (c->batch_done) (void)hipEventDestroy(c->batch_done);
  if (c->down_done) (void)hipEventDestroy(c->down_done);
  if (c->fork_event) (void)hipEventDestroy(c->fork_event);
  if (c->transform_done) (void)hipEventDestroy(c->transform_done);
  if (c->filter_done) (void)hipEventDestroy(c->filter_done);
  if (c->halo_event) (void)hipEventDestroy(c->halo_event);
  if (c->tensor_event) (void)hipEventDestroy(c->tensor_event);
  if (c->stream2) (void)hipStreamDestroy(c->stream2);
  if (c->stream && c->owns_stream) (void)hipStreamDestroy(c->stream);
  delete c;
}
}  // extern "C"

// Bound tensors against their consumers' streams, with no host wait (the pattern of jxlhip_halo_unpack_batch / _pack_batch).
// Before the first launch of a call that writes them: the launch stream `ls` waits for what every consumer stream holds
// now (the consumer's earlier fill or read of the tensor). After the last one: every consumer stream waits for `ls`.
// Contexts without a tensor cost nothing; consecutive contexts on one consumer stream cost one event.
static int TensorsBeforeWriters(JxlHipContext* const* ctxs, size_t n, hipStream_t ls) {
  bool any = false;
  hipStream_t waited = nullptr;
  for (size_t i = 0; i < n; i++) {
    JxlHipContext* c = ctxs[i];
    const JxlHipTensorOut* t = CallerTensor(c);
    if (!t) continue;
    const hipStream_t cs = static_cast<hipStream_t>(t->consumer_stream);
    if (any && cs == waited) continue;
    if (!c->tensor_event) HIP_TRY(hipEventCreateWithFlags(&c->tensor_event, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->tensor_event, cs));
    HIP_TRY(hipStreamWaitEvent(ls, c->tensor_event, 0));
    any = true;
    waited = cs;
  }
  return 0;
}
static int TensorsAfterWriters(JxlHipContext* const* ctxs, size_t n, hipStream_t ls) {
  hipEvent_t done = nullptr;
  hipStream_t told = nullptr;
  for (size_t i = 0; i < n; i++) {
    JxlHipContext* c = ctxs[i];
    const JxlHipTensorOut* t = CallerTensor(c);
    if (!t) continue;
    const hipStream_t cs = static_cast<hipStream_t>(t->consumer_stream);
    if (done && cs == told) continue;
    if (!done) {  // (one record behind the last writer serves every consumer stream)
      if (!c->tensor_event) HIP_TRY(hipEventCreateWithFlags(&c->tensor_event, hipEventDisableTiming));
      HIP_TRY(hipEventRecord(c->tensor_event, ls));
      done = c->tensor_event;
    }
    HIP_TRY(hipStreamWaitEvent(cs, done, 0));
    told = cs;
  }
  return 0;
}

static int ApplyPendingWait(JxlHipContext* c) {
  if (c->pending_wait) {
    HIP_TRY(hipStreamWaitEvent(c->stream, c->pending_wait, 0));
    c->pending_wait = nullptr;
  }
  if (c->filter_wait) {
    HIP_TRY(hipStreamWaitEvent(c->stream, c->filter_wait, 0));
    c->filter_wait = nullptr;
  }
  return 0;
}
// The two ends of a batched launch that runs on the first context's stream (the Modular and the reduced batch). Before it:
// the pending waits of the set, then the first stream waits for what the others still have in flight.
static int JoinSetOnFirstStream(JxlHipContext* const* ctxs, size_t n) {
  int r;
  for (size_t i = 0; i < n; i++)
    if ((r = ApplyPendingWait(ctxs[i]))) return r;
  for (size_t i = 1; i < n; i++) {
    if (!ctxs[i]->down_done) HIP_TRY(hipEventCreateWithFlags(&ctxs[i]->down_done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ctxs[i]->down_done, ctxs[i]->stream));
    HIP_TRY(hipStreamWaitEvent(ctxs[0]->stream, ctxs[i]->down_done, 0));
  }
  return 0;
}
// Behind it: the next call on one of the other contexts waits for the launch.
static int PublishBatchDone(JxlHipContext* const* ctxs, size_t n) {
  if (n < 2) return 0;
  JxlHipContext* c0 = ctxs[0];
  if (!c0->batch_done) HIP_TRY(hipEventCreateWithFlags(&c0->batch_done, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(c0->batch_done, c0->stream));
  for (size_t i = 1; i < n; i++) ctxs[i]->pending_wait = c0->batch_done;
  return 0;
}

// Table uploads go through one high-priority stream per device, not through the contexts' own streams: streams share a
// few hardware queues, and a copy queued behind another context's 100 ms entropy launch on the same queue waits for it
// (6.6 ms per upload in the end-to-end pipeline against 0.7 ms alone). A priority stream gets a queue of its own.
static hipStream_t CopyStream(int device) {
  static std::mutex mu;
  static hipStream_t streams[64] = {};
  std::lock_guard<std::mutex> lock(mu);
  if (device < 0 || device >= 64) return nullptr;
  if (!streams[device]) {
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) return nullptr;
    if (hipStreamCreateWithPriority(&streams[device], hipStreamNonBlocking, hi) != hipSuccess) streams[device] = nullptr;
  }
  return streams[device];
}

// Start of an upload: the previous upload's copies have left the staging block.
static int StageReset(JxlHipContext* c) {
  Stage& s = c->stage;
  if (!s.done) HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  if (s.recorded) HIP_TRY(hipEventSynchronize(s.done));
  else if (s.used) HIP_TRY(hipStreamSynchronize(c->stream));  // (an upload that failed half way)
  s.recorded = false;
  s.used = 0;
  return 0;
}
static int StageAlloc(JxlHipContext* c, size_t bytes, void** out) {
  Stage& s = c->stage;
  const size_t need = upload::StagedBytes(bytes);
  if (s.used + need > s.cap) {  // a larger block: copies out of the current one may still be in flight
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (hipStream_t cs = CopyStream(c->device)) HIP_TRY(hipStreamSynchronize(cs));
    size_t want = s.cap * 2 > need ? s.cap * 2 : need;
    if (want < (size_t(1) << 22)) want = size_t(1) << 22;
    if (s.p) HIP_TRY(hipHostFree(s.p));
    s.p = nullptr;
    s.cap = 0;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&s.p), want, hipHostMallocDefault));
    s.cap = want;
    s.used = 0;
  }
  *out = s.p + s.used;
  s.used += need;
  return 0;
}
// A table to a buffer of its own: through the staging block, by an asynchronous copy on the context's stream (an empty
// table still gets a valid address).
static int Upload(JxlHipContext* c, Buf& b, const void* src, size_t bytes) {
  void* st = nullptr;
  int r = StageAlloc(c, bytes, &st);
  if (r) return r;
  if ((r = b.Ensure(bytes ? bytes : 16))) return r;
  if (!bytes) return 0;
  memcpy(st, src, bytes);
  HIP_TRY(hipMemcpyAsync(b.p, st, bytes, hipMemcpyHostToDevice, c->stream));
  return 0;
}
// (the visitor of upload::Visit...Tables that does so for every table of a list; the first failure stays)
struct PlainUploader {
  JxlHipContext* c;
  int r = 0;
  void copy(Buf& b, size_t bytes, const void* src) {
    if (!r) r = Upload(c, b, src, bytes);
  }
};
// Small host-to-device copies of launch descriptions (parameter blocks, work lists): through the context's staging block
// and the copy stream like the tables, complete when End() returns.
struct ParamCopy {
  JxlHipContext* c = nullptr;
  hipStream_t cs = nullptr;
  int Begin(JxlHipContext* ctx) {
    c = ctx;
    cs = CopyStream(c->device);
    if (!cs) cs = c->stream;
    return StageReset(c);
  }
  int Add(void* dst, const void* src, size_t bytes) {
    if (!bytes) return 0;
    void* st = nullptr;
    int r = StageAlloc(c, bytes, &st);
    if (r) return r;
    memcpy(st, src, bytes);
    HIP_TRY(hipMemcpyAsync(dst, st, bytes, hipMemcpyHostToDevice, cs));
    return 0;
  }
  int End() {
    HIP_TRY(hipEventRecord(c->stage.done, cs));
    c->stage.recorded = true;
    HIP_TRY(WaitEvent(c->stage.done));
    return 0;
  }
};

// A frame's tables live in ONE device allocation laid out like the staging block (JxlHipContext::frame_blob). BlobBegin
// sizes both for the bytes the frame's table list takes; BlobPlacer, walking the same list, assembles each table at the
// next staging offset and makes its Buf a view of the blob there; BlobEnd copies everything at once.
static int BlobBegin(JxlHipContext* c, size_t bytes) {
  Stage& s = c->stage;
  if (s.cap < bytes) {
    void* dummy = nullptr;
    int r = StageAlloc(c, bytes, &dummy);  // grows the block (the stream is idle here: StageReset ran)
    if (r) return r;
    s.used = 0;
  }
  return c->frame_blob.Ensure(s.cap);
}
// JXLHIP_UPLOAD_PROF=1 (a measurement aid) prints where the host time of an upload goes: microseconds per phase.
struct UploadProf {
  const bool on = EnvInt("JXLHIP_UPLOAD_PROF", 0) != 0;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  std::string line;
  void lap(const char* what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    line += std::string(what) + " " + std::to_string(std::chrono::duration_cast<std::chrono::microseconds>(now - t0).count()) + "  ";
    t0 = now;
  }
};
struct BlobPlacer {
  JxlHipContext* c;
  UploadProf* prof;
  void* place(Buf& b, size_t bytes) {
    Stage& s = c->stage;
    void* st = s.p + s.used;
    if (!b.view) b.Free();
    b.p = c->frame_blob.as<uint8_t>() + s.used;
    b.cap = bytes ? bytes : 16;
    b.view = true;
    s.used += upload::StagedBytes(bytes);
    return st;
  }
  void copy(Buf& b, size_t bytes, const void* src) {
    void* st = place(b, bytes);
    if (bytes) memcpy(st, src, bytes);
  }
  template <typename F>
  void build(Buf& b, size_t bytes, F&& fill) { fill(place(b, bytes)); }
  void phase(const char* what) { prof->lap(what); }
};
// Where a placed table is being assembled (the parameter blocks are filled once every buffer has its address).
template <typename T>
static T* Staged(JxlHipContext* c, const Buf& b) {
  return reinterpret_cast<T*>(c->stage.p + (b.as<uint8_t>() - c->frame_blob.as<uint8_t>()));
}
// `smooth` / `sigma` / `dequant`: the DC-path kernels of this frame (NULL = not asked for), launched on the copy stream
// behind the copy they read, so that the event the upload waits for covers them too.
static int BlobEnd(JxlHipContext* c, const jxlhip::DcSmoothParams* smooth = nullptr, const jxlhip::SigmaParams* sigma = nullptr,
                   const jxlhip::DcDequantParams* dequant = nullptr) {
  hipStream_t cs = CopyStream(c->device);
  if (!cs) cs = c->stream;
  if (c->stage.used) HIP_TRY(hipMemcpyAsync(c->frame_blob.p, c->stage.p, c->stage.used, hipMemcpyHostToDevice, cs));
  if (dequant) {
    hipLaunchKernelGGL(jxlhip::k_dc_dequant, dim3((dequant->xs + 63) / 64, (dequant->ys + 3) / 4), dim3(256), 0, cs, *dequant);
    HIP_TRY(hipGetLastError());
  }
  if (smooth) {
    hipLaunchKernelGGL(jxlhip::k_dc_smooth, dim3((smooth->xs + 63) / 64, (smooth->ys + 3) / 4), dim3(256), 0, cs, *smooth);
    HIP_TRY(hipGetLastError());
  }
  if (sigma && sigma->num_blocks) {
    hipLaunchKernelGGL(jxlhip::k_epf_sigma, dim3((sigma->num_blocks + 255) / 256), dim3(256), 0, cs, *sigma);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(c->stage.done, cs));
  c->stage.recorded = true;
  return 0;
}

// What the context remembers of a frame's splines and patches (the tables themselves: upload::Visit...Tables).
static void AdoptSplines(JxlHipContext* c, const JxlHipSplines& sp) { c->spl_segments = sp.num_segments; }
static void AdoptPatches(JxlHipContext* c, const JxlHipPatches& pt) {
  c->pat_positions = pt.num_positions;
  c->pat_uses_alpha = pt.num_positions && pt.uses_alpha != 0;
  c->alpha_patched_valid = false;
  if (!pt.num_positions) return;
  c->pat_premultiplied = pt.premultiplied != 0;
  for (int i = 0; i < 4; i++) {
    c->pat_src_alpha[i] = pt.slot_alpha[i];
    c->pat_src[i] = pt.slot_planes[i];
    c->pat_src_w[i] = pt.slot_w[i];
    c->pat_src_h[i] = pt.slot_h[i];
  }
}
// ------------------------------------------------------------------------------------- resized binding (jxh_resample_plan.h)
// The descriptor and the tap tables of `d` (which CheckResizedOut took for an image of w x h whose f32 pixels are `src`, rows
// of w pixels) into the context's block: built in the staging block, one copy on the context's stream, complete on return.
// The caller has made sure that nothing reads the block or the staging block any more.
static int PlaceResample(JxlHipContext* c, const JxlHipResizedOut& d, uint32_t w, uint32_t h, const float* src) {
  const resample::Box b = resample::BoxOf(d, w, h);
  const resample::BlockLayout l = resample::LayoutOf(b, d.out_xsize, d.out_ysize);
  int r;
  if ((r = c->rs_block.Ensure(l.bytes))) return r;
  if ((r = c->rs_tmp.Ensure(resample::TmpBytes(b, d.tensor.num_channels, d.out_ysize)))) return r;
  if ((r = StageReset(c))) return r;
  void* st = nullptr;
  if ((r = StageAlloc(c, l.bytes, &st))) return r;
  if ((r = resample::PlaceBlock(d, b, src, w, c->rs_tmp.as<float>(), st, uintptr_t(c->rs_block.p)))) return r;
  memcpy(&c->rs_dev, static_cast<uint8_t*>(st) + l.desc, sizeof(c->rs_dev));
  HIP_TRY(hipMemcpyAsync(c->rs_block.p, st, l.bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipEventRecord(c->stage.done, c->stream));
  c->stage.recorded = true;
  HIP_TRY(WaitEvent(c->stage.done));
  return 0;
}
// ... of the frame the context has just adopted: the source is its own pixel buffer at the oriented output size.
static int PlaceResampleOfFrame(JxlHipContext* c) {
  const bool transposed = (c->out_orient & 4) != 0;
  return PlaceResample(c, c->resized, transposed ? c->oys : c->oxs, transposed ? c->oxs : c->oys, c->rgb.as<float>());
}
static int LaunchResamplePasses(const resample::ResampleDev* descs, uint32_t n, uint32_t v_tiles, uint32_t h_tiles, hipStream_t ls) {
  hipLaunchKernelGGL(jxlhip::k_resample_rows, dim3(v_tiles), dim3(256), 0, ls, descs, n);
  hipLaunchKernelGGL(jxlhip::k_resample_columns, dim3(h_tiles), dim3(256), 0, ls, descs, n);
  HIP_TRY(hipGetLastError());
  return 0;
}
// The tail of a filter + colour or Modular launch: the two passes, once for every context of the set that has a resized
// binding, behind the writers on `ls`. One such context: its own block is the launch's descriptor array. Several: their
// descriptors side by side with running tile origins, on the set's first context, rebuilt only when the set changed.
static int LaunchResample(JxlHipContext* const* ctxs, size_t n, hipStream_t ls) {
  std::vector<const JxlHipContext*> set;
  for (size_t i = 0; i < n; i++)
    if (ctxs[i]->resized_bound) set.push_back(ctxs[i]);
  if (set.empty()) return 0;
  if (set.size() == 1) {
    const JxlHipContext* c = set[0];
    return LaunchResamplePasses(c->rs_block.as<resample::ResampleDev>(), 1, c->rs_dev.v_tiles, c->rs_dev.h_tiles, ls);
  }
  JxlHipContext* c0 = ctxs[0];
  std::vector<resample::ResampleDev> descs(set.size());
  uint64_t v = 0, h = 0;
  for (size_t i = 0; i < set.size(); i++) {
    descs[i] = set[i]->rs_dev;
    descs[i].v_tile0 = uint32_t(v);
    descs[i].h_tile0 = uint32_t(h);
    v += descs[i].v_tiles;
    h += descs[i].h_tiles;
  }
  if (v > 0x7FFFFFFFu || h > 0x7FFFFFFFu) return JXLHIP_ERR_UNSUPPORTED;
  if (!c0->rs_batch_set.Matches(set.data(), set.size())) {
    c0->rs_batch_set.Forget();
    const size_t bytes = descs.size() * sizeof(resample::ResampleDev);
    int r = c0->rs_batch.Ensure(bytes);
    if (r) return r;
    // (on the launch stream itself: behind an earlier launch that still reads the array, and without a host wait)
    void* st = nullptr;
    if ((r = StageReset(c0)) || (r = StageAlloc(c0, bytes, &st))) return r;
    memcpy(st, descs.data(), bytes);
    HIP_TRY(hipMemcpyAsync(c0->rs_batch.p, st, bytes, hipMemcpyHostToDevice, ls));
    HIP_TRY(hipEventRecord(c0->stage.done, ls));
    c0->stage.recorded = true;
    c0->rs_batch_set.Remember(set.data(), set.size());
  }
  return LaunchResamplePasses(c0->rs_batch.as<resample::ResampleDev>(), uint32_t(set.size()), uint32_t(v), uint32_t(h), ls);
}

// -------------------------------------------------------------------------------------------------- frame upload
// The bound tensor against the frame: whole frames only, and the descriptor's rules (jxh_tensor_out.h) at the size of the
// output image, which a transposing orientation turns. *reach: bytes from the tensor's first element to behind the last one.
static int CheckBoundTensor(const JxlHipContext* c, const upload::Geometry& g, uint32_t group_rows, uint64_t* reach) {
  if (g.band_row0 != 0 || g.band_row1 != group_rows) return JXLHIP_ERR_UNSUPPORTED;
  const bool transposed = (c->out_orient & 4) != 0;
  const uint32_t w = transposed ? g.oys : g.oxs, h = transposed ? g.oxs : g.oys;
  const int r = tensor_out::CheckTensorOut(c->tensor, w, h);
  if (r) return r;
  uint64_t max_offset = 0;
  tensor_out::MaxOffset(c->tensor, w, h, &max_offset);
  *reach = (max_offset + 1) * tensor_out::ElemBytes(c->tensor.dtype);
  return 0;
}
// The resized binding against the frame: whole frames only, and the descriptor's rules (jxh_resample_plan.h) at the size
// of the oriented output image.
static int CheckBoundResized(const JxlHipContext* c, const upload::Geometry& g, uint32_t group_rows) {
  if (g.band_row0 != 0 || g.band_row1 != group_rows) return JXLHIP_ERR_UNSUPPORTED;
  const bool transposed = (c->out_orient & 4) != 0;
  return resample::CheckResizedOut(c->resized, transposed ? g.oys : g.oxs, transposed ? g.oxs : g.oys);
}
static upload::UploadOptions OptionsOf(const JxlHipContext* c) {
  upload::UploadOptions o;
  o.band_halo = c->band_halo;
  o.keep_filtered = c->keep_filtered;
  o.keep_upsampled = c->keep_upsampled;
  o.out_type = OutType(c);
  o.out_nc = OutChannels(c);
  o.out_bits = OutBits(c);
  o.out_swap = OutSwap(c);
  o.out_orient = c->out_orient;
  o.tensor = c->tensor_bound;
  o.tensor_rows = c->tensor_bound && c->tensor.stride_x == 1;
  o.have_alpha = c->have_alpha;
  o.alpha_capacity = c->alpha.cap;
  o.section_entropy = SectionEntropyForced();
  o.no_lane_prefix = EnvInt("JXLHIP_NO_LANE_PREFIX", 0) != 0;
  return o;
}

// Which kernel decodes the frame's AC sections (stays beside the kernels: LanesLdsLayout is the lane kernel's own).
// Frames whose tables fit LDS are decoded by the lane-parallel kernel into scan order (its packed block records hold the
// block contexts in 4 bits each): single-pass frames hand that layout to the transforms (scan_order), progressive frames
// decode every pass into its own buffer and k_merge_passes sums them (lane_multi).
struct EntropyRoute {
  bool generic, any_lz77, lane_prefix, lanes, scan_order, lane_multi, alias_lds;
  uint32_t lds_ctx_bytes, lds_alias_bytes;
};
static EntropyRoute EntropyRouteOf(const JxlHipFrameDesc& d, const upload::UploadOptions& o) {
  EntropyRoute e = {};
  const uint32_t nctx = d.num_block_ctxs * 495;
  size_t alias_bytes_max = 0;
  bool all_prefix = true;
  for (uint32_t p = 0; p < d.num_passes; p++) {
    const JxlHipPassDesc& s = d.passes[p];
    e.generic = e.generic || s.use_prefix || s.lz77;
    e.any_lz77 = e.any_lz77 || s.lz77;
    all_prefix = all_prefix && s.use_prefix;
    alias_bytes_max = std::max(alias_bytes_max, upload::AliasBytes(s));
  }
  e.lds_ctx_bytes = (nctx + 16 + 15) & ~15u;
  e.alias_lds = e.lds_ctx_bytes + alias_bytes_max + 1024 + 4 * 5120 <= kLdsBudget;
  e.lds_alias_bytes = e.alias_lds ? uint32_t((alias_bytes_max + 15) & ~size_t(15)) : 0;
  e.lane_prefix = all_prefix && !e.any_lz77 && !o.no_lane_prefix;
  e.lanes = !o.section_entropy && d.num_block_ctxs <= 16 && d.num_passes <= 8 && (!e.generic || e.lane_prefix);
  for (uint32_t p = 0; e.lanes && p < d.num_passes; p++)  // (alias tables that do not fit LDS are read in place)
    e.lanes = jxlhip::LanesLdsLayout(1, nctx, d.passes[p].num_clusters, d.passes[p].log_alpha, kLanesAdmitWaves, 64, false, e.lane_prefix).total <= kLdsBudget;
  if (!e.lanes) e.lane_prefix = false;
  e.scan_order = e.lanes && d.num_passes == 1;
  e.lane_multi = e.lanes && d.num_passes > 1;
  return e;
}

// The frame's table list: what the descriptor gives (upload::VisitFrameTables) and the two parameter tables the entropy
// kernels read from device memory, which hold device addresses and are filled once every buffer has one.
template <typename V>
static void VisitTables(JxlHipContext* c, const JxlHipFrameDesc& d, const upload::Plan& P, V& v) {
  upload::VisitFrameTables(*c, d, P, v);
  v.build(c->passes_dev, size_t(d.num_passes) * sizeof(jxlhip::PassDev), [](void*) {});
  v.build(c->ep_dev, sizeof(jxlhip::EntropyParams), [](void*) {});
}

// What the context remembers of the frame beside its tables.
static void AdoptFrame(JxlHipContext* c, const JxlHipFrameDesc& d, const upload::Plan& P, const EntropyRoute& E) {
  const upload::Geometry& g = P.g;
  c->cs = g.cs;
  c->xs = d.xsize; c->ys = d.ysize; c->xb = d.xsize_blocks; c->yb = d.ysize_blocks;
  c->xg = d.xsize_groups; c->ng = d.num_groups; c->np = d.num_passes;
  c->nblocks = d.num_blocks;
  c->xp = c->xb * 8; c->yp = c->yb * 8;
  c->ups = g.ups; c->oxs = g.oxs; c->oys = g.oys;
  c->band_y0 = g.band_y0; c->band_y1 = g.band_y1; c->ext_y0 = g.ext_y0; c->ext_y1 = g.ext_y1;
  upload::BuildGroupLists(d, g, &c->group_list, &c->absent_groups, &c->absent_blocks, &c->absent_sections);
  c->coef_bits = d.coef_bits;
  c->gab = d.gab; c->epf_iters = d.epf_iters;
  c->epf_pass0 = d.epf_pass0_sigma_scale;
  c->epf_pass2 = d.epf_pass2_sigma_scale;
  c->epf_border = d.epf_border_sad_mul;
  c->sec_size_host.assign(d.section_size, d.section_size + g.nsec);
  c->sec_sel_host.resize(g.nsec);
  upload::BuildSelectors(d, c->sec_sel_host.data());
  c->pass_clusters.resize(d.num_passes);
  c->pass_log_alpha.resize(d.num_passes);
  for (uint32_t p = 0; p < d.num_passes; p++) {
    c->pass_clusters[p] = d.passes[p].num_clusters;
    c->pass_log_alpha[p] = d.passes[p].log_alpha;
  }
  if (c->pass_bufs.size() < d.num_passes) c->pass_bufs.resize(d.num_passes);
  memcpy(c->list_begin, P.list_begin, sizeof(c->list_begin));
  memcpy(c->list_count, P.list_count, sizeof(c->list_count));
  c->plane_bytes = size_t(c->xp) * c->yp * 3 * 4;
  c->color_out = P.px.color_out;
  c->gray8_fast = P.px.gray8_fast;
  c->tensor_fused = P.px.tensor_fused;
  c->ups_kept = P.px.ups_kept;
  c->ct = d.color_target ? *d.color_target : JxlHipColorTarget{};
  c->has_noise = d.has_noise != 0;
  if (c->has_noise) {
    memcpy(c->noise_lut, d.noise_lut, sizeof(c->noise_lut));
    c->noise_seed[0] = d.noise_frame_index[0];
    c->noise_seed[1] = d.noise_frame_index[1];
    c->noise_ytox = d.base_corr_x;
    c->noise_ytob = d.base_corr_b;
  }
  AdoptSplines(c, d.splines);
  AdoptPatches(c, d.patches);
  c->generic_codec = E.generic;
  c->lane_prefix = E.lane_prefix;
  c->lanes = E.lanes;
  c->scan_order = E.scan_order;
  c->lane_multi = E.lane_multi;
  c->alias_lds = E.alias_lds;
  c->lds_entropy = E.lds_ctx_bytes + E.lds_alias_bytes + 3072;
  if (c->lanes || c->scan_order)  // (PrepareBatch's cost estimate; jxlhip_download("coeffs"))
    c->gbb_host.assign(d.group_block_begin, d.group_block_begin + d.num_groups + 1);
  if (c->scan_order) {  // for jxlhip_download("coeffs")
    c->blocks_host.assign(d.blocks, d.blocks + d.num_blocks);
    c->orders_host.assign(d.passes[0].orders, d.passes[0].orders + d.passes[0].orders_size);
    memcpy(c->order_offset_host, d.passes[0].order_offset, sizeof(c->order_offset_host));
  }
  c->ev_valid[0] = c->ev_valid[1] = c->ev_valid[2] = false;
  c->generation++;
}

// The buffers the kernels write: allocated here (launch functions never allocate), cleared where a launch may leave them.
static int EnsureWorkBuffers(JxlHipContext* c, const JxlHipFrameDesc& d, const upload::Plan& P, const EntropyRoute& E) {
  int r;
  const size_t nblk = P.g.nblk;
  if (d.dc_device) {  // the planes of a DC frame decoded earlier (kUseDcFrame): used where they are
    if (!c->dc.view) c->dc.Free();
    c->dc.p = const_cast<float*>(d.dc_device);
    c->dc.cap = nblk * 3 * 4;
    c->dc.view = true;
  } else {  // (the DC kernels' outputs are allocations of their own, not views of the blob)
    if (P.dc.smooth && P.dc.dequant && (r = c->dc_raw.Ensure(nblk * 3 * 4))) return r;
    if ((P.dc.smooth || P.dc.dequant) && (r = c->dc.Ensure(nblk * 3 * 4))) return r;
  }
  if (!d.inv_sigma && (r = c->inv_sigma.Ensure(nblk * 4))) return r;  // (computed here, or no EPF: never read)
  // (progressive frames: the natural-layout buffer + one scan-order buffer per pass for the lane kernel)
  const size_t coef_bytes = size_t(d.num_groups) * 3 * 65536 * (d.coef_bits / 8);
  // (+ 64 bytes: a lane of the entropy kernel that decodes a CORRUPT section may write up to three coefficients past the
  // last scan position of a block before it is stopped, jxl_hip_lanes_trip.inc: past the buffer for the very last block)
  if ((r = c->coeffs.Ensure(coef_bytes * (d.num_passes > 1 ? d.num_passes + 1 : 1) + 64))) return r;
  if ((r = c->errors.Ensure(size_t(d.num_groups) * 4))) return r;
  HIP_TRY(hipMemsetAsync(c->errors.p, 0, size_t(d.num_groups) * 4, c->stream));  // groups outside a band stay clean
  if (!c->plane_lender && (r = c->plane[0].Ensure(c->plane_bytes))) return r;
  // (an upsampled frame's noise is generated and added at the IMAGE's resolution, behind the upsampling:
  // dec_cache.cc:206-216, dec_group.cc PrepareNoiseInput: one generator per 256 x 256 square of the image)
  if (c->has_noise && (r = c->noise.Ensure(size_t(c->oxs) * c->oys * 3 * 4))) return r;
  if (((c->has_noise && c->ups != 1) || c->ups_kept) && (r = c->ups_planes.Ensure(size_t((c->oxs + 7) & ~7u) * c->oys * 3 * 4))) return r;
  if (P.px.plane1 && (r = c->plane[1].Ensure(c->plane_bytes))) return r;
  if (!c->tensor_bound && (r = c->rgb.Ensure(OwnPixelBytes(c)))) return r;
  uint32_t big = 0;  // the largest transforms go through scratch planes, a launch's varblocks at a time
  for (uint32_t s = 0; s < jxlhip::kTransformStrategies; s++)
    if (jxlhip::TransformClassOf(s) == jxlhip::kBigClass) big = std::max(big, P.list_count[s]);
  if (big && (r = c->scratch.Ensure(jxlhip::BigScratchBytes(big)))) return r;
  if (E.any_lz77 && (r = c->lz_window.Ensure(size_t(d.num_groups) * jxlhip::kLzWindow * 4))) return r;
  if ((r = c->sec_end.Ensure(P.g.nsec * 4))) return r;
  HIP_TRY(hipMemsetAsync(c->sec_end.p, 0, P.g.nsec * 4, c->stream));
  if ((r = c->kend.Ensure(size_t(d.num_blocks ? d.num_blocks : 1) * 3 * 4 * d.num_passes))) return r;
  return 0;
}

// The entropy kernels' parameters: c->ep, its device copy and the per-pass table, assembled where they were placed.
static void FillEntropyParams(JxlHipContext* c, const JxlHipFrameDesc& d, const upload::Plan& P, const EntropyRoute& E) {
  jxlhip::PassDev* pd = Staged<jxlhip::PassDev>(c, c->passes_dev);
  memset(pd, 0, size_t(d.num_passes) * sizeof(jxlhip::PassDev));
  for (uint32_t p = 0; p < d.num_passes; p++) {
    const JxlHipPassDesc& s = d.passes[p];
    const PassBufs& pb = c->pass_bufs[p];
    pd[p].ctx_map = pb.ctx_map.as<uint8_t>();
    pd[p].alias = pb.alias.as<uint2>();
    pd[p].alias_packed = pb.alias_packed.as<uint2>();
    pd[p].cfg = pb.cfg.as<uint32_t>();
    pd[p].orders = pb.orders.as<uint16_t>();
    memcpy(pd[p].order_offset, s.order_offset, sizeof(s.order_offset));
    pd[p].use_prefix = s.use_prefix ? 1 : 0;
    pd[p].lz77 = s.lz77 ? 1 : 0;
    pd[p].lz_min_symbol = s.lz_min_symbol;
    pd[p].lz_min_length = s.lz_min_length;
    pd[p].lz_len_cfg = s.lz_len_cfg;
    pd[p].lz_dist_ctx = s.lz_dist_ctx;
    pd[p].prefix_table = pb.ptable.as<uint32_t>();
    pd[p].prefix_offset = pb.poffset.as<uint32_t>();
    pd[p].log_alpha = s.log_alpha;
    pd[p].num_clusters = s.num_clusters;
    pd[p].shift = s.shift;
    pd[p].alias_lds = 0;
  }
  jxlhip::EntropyParams& ep = c->ep;
  memset(&ep, 0, sizeof(ep));
  ep.sections = c->sections.as<uint32_t>();
  ep.sec_word = c->sec_word.as<uint32_t>();
  ep.sec_size = c->sec_size.as<uint32_t>();
  ep.first_bit_offset = d.first_section_bit_offset;
  ep.blocks = c->blocks.as<JxlHipVarBlock>();
  ep.gbb = c->gbb.as<uint32_t>();
  ep.bctx_lut = c->bctx_lut.as<uint8_t>();
  ep.nq = d.num_qf_thresholds + 1;
  ep.ndc = d.num_dc_ctxs;
  ep.num_bctx = d.num_block_ctxs;
  for (uint32_t i = 0; i < d.num_qf_thresholds; i++) ep.qf_thr[i] = d.qf_thresholds[i];
  ep.num_hist = d.num_histograms;
  ep.nctx = P.g.nctx;
  ep.cs = P.g.cs;
  ep.passes = c->passes_dev.as<jxlhip::PassDev>();
  ep.num_passes = d.num_passes;
  ep.num_groups = d.num_groups;
  ep.coeffs = c->coeffs.p;
  ep.errors = c->errors.as<uint32_t>();
  ep.lz_window = E.any_lz77 ? c->lz_window.as<uint32_t>() : nullptr;
  ep.sec_end_bits = c->sec_end.as<uint32_t>();
  ep.lds_ctx_bytes = E.lds_ctx_bytes;
  ep.lds_alias_bytes = E.lds_alias_bytes;
  const size_t kend_per_pass = size_t(d.num_blocks ? d.num_blocks : 1) * 3;
  ep.kend = c->kend.as<uint32_t>();
  ep.coef_pass_base = E.lane_multi ? uint64_t(d.num_groups) * 3 * 65536 : 0;
  ep.coef_pass_stride = uint64_t(d.num_groups) * 3 * 65536;
  ep.kend_pass_stride = uint32_t(kend_per_pass);
  ep.block_recs = c->block_recs.as<uint32_t>();
  memcpy(Staged<jxlhip::EntropyParams>(c, c->ep_dev), &ep, sizeof(ep));
}

static void FillTransformParams(JxlHipContext* c, const JxlHipFrameDesc& d) {
  jxlhip::TransformParams& tp = c->tp;
  memset(&tp, 0, sizeof(tp));
  tp.coeffs = c->coeffs.p;
  tp.coef_bits = d.coef_bits;
  tp.blocks = c->blocks.as<JxlHipVarBlock>();
  tp.dequant = c->dequant.as<float>();
  memcpy(tp.dq_offset, d.dequant_offset, sizeof(tp.dq_offset));
  memcpy(tp.dq_size, d.dequant_size, sizeof(tp.dq_size));
  tp.dense = c->transform_dense ? 1 : 0;
  tp.cs = c->cs;
  tp.cs_out = c->plane[1].as<float>();  // (a YCbCr frame's colour stage is the generic writer: the second plane set exists)
  tp.dc = c->dc.as<float>();
  tp.ytox = c->ytox.as<int8_t>();
  tp.ytob = c->ytob.as<int8_t>();
  tp.basis_t = c->basis.as<float>();
  tp.basis_n = c->basis.as<float>() + kBasisTransposed;
  tp.inv_global_scale = d.inv_global_scale;
  tp.x_dm = d.x_dm;
  tp.b_dm = d.b_dm;
  tp.color_scale = d.color_scale;
  tp.base_x = d.base_corr_x;
  tp.base_b = d.base_corr_b;
  memcpy(tp.biases, d.quant_biases, sizeof(tp.biases));
  tp.xb = c->xb; tp.yb = c->yb; tp.xg = c->xg; tp.xp = c->xp; tp.yp = c->yp;
  // (the planes as they stand now: every launch takes `out` and `cs_out` from the block ResolveTransformBlocks makes for
  // its set, where a lender's buffer is checked)
  tp.out = PlaneHolder(c)->plane[0].as<float>();
  tp.scratch = c->scratch.as<float>();
  tp.tlist = c->tlist.as<uint32_t>();
  tp.trecs = c->trecs.as<uint4>();
  memcpy(tp.list_begin, c->list_begin, sizeof(tp.list_begin));
  memcpy(tp.list_count, c->list_count, sizeof(tp.list_count));
  tp.scan_order = c->scan_order ? 1 : 0;
  tp.kend = c->kend.as<uint32_t>();
  tp.orders = c->pass_bufs[0].orders.as<uint16_t>();
  tp.dequant_scan = c->scan_order ? c->dequant_scan.as<float>() : nullptr;
  memcpy(tp.order_offset, d.passes[0].order_offset, sizeof(tp.order_offset));
}

static void FillFilterParams(JxlHipContext* c, const JxlHipFrameDesc& d) {
  jxlhip::FilterParams& fp = c->fp;
  memset(&fp, 0, sizeof(fp));
  fp.xs = c->xs; fp.ys = c->ys; fp.xp = c->xp; fp.yp = c->yp; fp.xb = c->xb;
  fp.y_begin = c->band_y0; fp.y_end = c->band_y1;
  fp.inv_sigma = c->inv_sigma.as<float>();
  upload::FoldGaborish(d.gab_w, fp.gab_w);
  for (int ch = 0; ch < 3; ch++) {
    fp.ch_scale[ch] = d.epf_channel_scale[ch];
    fp.opsin_bias[ch] = d.opsin_bias[ch];
    fp.opsin_bias_cbrt[ch] = cbrtf(d.opsin_bias[ch]);
  }
  memcpy(fp.opsin_inv, d.opsin_inv, sizeof(fp.opsin_inv));
  fp.linear_output = d.linear_output;
  if (c->tensor_bound) return;  // (no pixel buffer of the context's own: the tensor form reads FusedFilterParams' t_ fields)
  fp.rgb = OutIsRgb8(c) || c->gray8_fast ? c->rgb.as<uint8_t>() : nullptr;
  fp.rgbf = !OutIsRgb8(c) && !c->gray8_fast && !c->color_out ? c->rgb.as<float>() : nullptr;
}

// The DC-path kernels' parameters (jxl_hip_dc.h): DequantDC, adaptive smoothing, 1 / sigma, as the frame asks for them.
struct DcParams {
  jxlhip::DcDequantParams dequant;
  jxlhip::DcSmoothParams smooth;
  jxlhip::SigmaParams sigma;
};
static void FillDcParams(JxlHipContext* c, const JxlHipFrameDesc& d, const upload::Plan& P, DcParams* dp) {
  if (P.dc.dequant) {
    jxlhip::DcDequantParams& q = dp->dequant;
    q.q = c->dc_q.as<int32_t>();
    q.out = P.dc.smooth ? c->dc_raw.as<float>() : c->dc.as<float>();
    q.xs = c->xb;
    q.ys = c->yb;
    q.xgroups = (c->xb + 255) / 256;
    q.extra_precision = d.dc_extra_precision ? c->dc_ep.as<uint8_t>() : nullptr;
    for (int ch = 0; ch < 3; ch++) q.step[ch] = d.dc_step[ch];
    q.cfl_x = d.dc_cfl_x;
    q.cfl_b = d.dc_cfl_b;
    q.cs = c->cs;
  }
  if (P.dc.smooth) {
    jxlhip::DcSmoothParams& s = dp->smooth;
    s.in = c->dc_raw.as<float>();
    s.out = c->dc.as<float>();
    s.xs = c->xb;
    s.ys = c->yb;
    for (int ch = 0; ch < 3; ch++) s.step[ch] = d.dc_step[ch];
  }
  if (P.dc.sigma) {
    jxlhip::SigmaParams& s = dp->sigma;
    s.blocks = c->blocks.as<JxlHipVarBlock>();
    s.num_blocks = d.num_blocks;
    s.xb = c->xb;
    s.sharpness = c->sharp.as<uint8_t>();
    s.inv_sigma = c->inv_sigma.as<float>();
    s.quant_scale = d.quant_scale;
    s.epf_quant_mul = d.epf_quant_mul;
    memcpy(s.sharp_lut, d.epf_sharp_lut, sizeof(s.sharp_lut));
  }
}

extern "C" int jxlhip_frame_upload(JxlHipContext* c, const JxlHipFrameDesc* d) {
  if (!c || !d) return JXLHIP_ERR_INVALID_ARGUMENT;
  UploadProf prof;
  // 1. whether the descriptor is taken: decided on the host alone, so that a refused one costs no device call and
  // leaves the context's tables as they were (but no frame to run: the caller meant to replace it)
  upload::UploadOptions opt = OptionsOf(c);
  int r = upload::CheckFrameDesc(*d, opt);
  if (!r && c->tensor_bound) r = CheckBoundTensor(c, upload::MakeGeometry(*d, opt), d->num_groups / d->xsize_groups, &opt.tensor_reach);
  if (!r && c->resized_bound) r = CheckBoundResized(c, upload::MakeGeometry(*d, opt), d->num_groups / d->xsize_groups);
  upload::Plan P;
  EntropyRoute E = {};
  if (!r) {
    P = upload::MakePlan(*d, opt);
    E = EntropyRouteOf(*d, opt);
    P.scan_order = E.scan_order;
    r = upload::CheckOrders(*d, P.list_count, E.lanes ? d->num_passes : 0);
  }
  if (r) {
    c->have_frame = false;
    c->red.have = c->red.ran = false;
    return r;
  }
  prof.lap("validate");
  // 2. the tables are overwritten from the copy stream: whatever still reads the old ones has to be finished
  HIP_TRY(hipSetDevice(c->device));
  if ((r = ApplyPendingWait(c))) return r;
  if ((r = StageReset(c))) return r;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->stream2) HIP_TRY(hipStreamSynchronize(c->stream2));
  c->have_frame = false;
  c->red.have = c->red.ran = false;  // (an ordinary context again)
  AdoptFrame(c, *d, P, E);
  // 3. the tables: one list, walked once for the size of the blob and once to place them
  upload::TableBound bound;
  VisitTables(c, *d, P, bound);
  if ((r = BlobBegin(c, bound.bytes))) return r;
  BlobPlacer placer{c, &prof};
  VisitTables(c, *d, P, placer);
  // 4. work buffers, then the parameter blocks, which hold their addresses
  if ((r = EnsureWorkBuffers(c, *d, P, E))) return r;
  prof.lap("buffers");
  DcParams dc;
  FillDcParams(c, *d, P, &dc);
  FillEntropyParams(c, *d, P, E);
  FillTransformParams(c, *d);
  FillFilterParams(c, *d);
  if ((r = BlobEnd(c, P.dc.smooth ? &dc.smooth : nullptr, P.dc.sigma ? &dc.sigma : nullptr, P.dc.dequant ? &dc.dequant : nullptr))) return r;
  // The tables are resident when the call returns (batch launches over this context run on other contexts' streams).
  // (Leaving the copies of many contexts in flight at once instead, ordered by events, made every later kernel of the
  // process ~1.35x slower on this runtime: scripts/async_probe.py.)
  HIP_TRY(WaitEvent(c->stage.done));
  if (c->resized_bound && (r = PlaceResampleOfFrame(c))) return r;
  prof.lap("rest");
  if (prof.on) fprintf(stderr, "[upload] %s\n", prof.line.c_str());
  c->have_frame = true;
  c->mod.have = false;  // (the context now holds a VarDCT frame, not the Modular one it may have held before)
  return 0;
}

template <typename CoefT>
static int LaunchEntropy(JxlHipContext* c) {
  const dim3 grid(c->ng), block(64);
  if (c->generic_codec) {
    hipLaunchKernelGGL(jxlhip::k_entropy_generic<CoefT>, grid, block, 3072, c->stream, c->ep);
  } else if (c->alias_lds) {
    // scalar-form kernel: alias tables, context map and uint configs shared in LDS by the waves of a workgroup
    const size_t shared = size_t(c->ep.lds_ctx_bytes) + c->ep.lds_alias_bytes + 1024;
    jxlhip::EntropyBatch b{c->ep_dev.as<jxlhip::EntropyParams>(), nullptr};
    if (c->ep.num_hist == 1) {
      constexpr int WPG = kEntropyWPG;
      auto k = jxlhip::k_entropy_uni<CoefT, WPG>;
      const size_t lds = shared + WPG * 5120;
      if (lds > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
      hipLaunchKernelGGL(k, dim3((c->ng + WPG - 1) / WPG), dim3(64 * WPG), lds, c->stream, b);
    } else {
      auto k = jxlhip::k_entropy_uni<CoefT, 1>;
      const size_t lds = shared + 5120;
      if (lds > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
      hipLaunchKernelGGL(k, grid, block, lds, c->stream, b);
    }
  } else {  // alias tables beyond the LDS budget: read in place
    hipLaunchKernelGGL(jxlhip::k_entropy_ans<CoefT>, grid, block, c->lds_entropy, c->stream, c->ep);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

static int RunEntropySingle(JxlHipContext* c) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->red.have) return JXLHIP_ERR_UNSUPPORTED;  // (a reduced upload has no AC stage: jxlhip_reduced_run)
  if (!c->have_frame) return JXLHIP_ERR_NO_FRAME;
  HIP_TRY(hipSetDevice(c->device));
  {
    int pw = ApplyPendingWait(c);
    if (pw) return pw;
  }
  HIP_TRY(hipEventRecord(c->ev[0], c->stream));
  HIP_TRY(hipMemsetAsync(c->errors.p, 0, size_t(c->ng) * 4, c->stream));
  int r = c->coef_bits == 16 ? LaunchEntropy<int16_t>(c) : LaunchEntropy<int32_t>(c);
  if (r) return r;
  HIP_TRY(hipEventRecord(c->ev[1], c->stream));
  c->ev_valid[0] = true;
  return 0;
}

// ---- transform + filter launches, batched over the frames of a set ---------------------------------------------------
// The kernel of a descriptor list (jxl_hip_transform_abi.h): the strategy's class and covered blocks pick it, and the list
// of chroma-subsampled frames takes the 8x8 DCT's CS form.
typedef void (*ListKernel)(const jxlhip::TransformParams*, const uint2*, uint32_t);
template <typename CoefT, uint32_t S>
constexpr ListKernel KernelOfStrategy() {
  if constexpr (jxlhip::TransformClassOf(S) == jxlhip::kFastClass)
    return jxlhip::k_idct_fast<CoefT, jxlhip::kCoveredX[S], jxlhip::kCoveredY[S]>;
  else
    return jxlhip::k_special<CoefT>;
}
template <typename CoefT, size_t... S>
static ListKernel ListKernelOf(uint32_t list, std::index_sequence<S...>) {
  static const ListKernel kTable[] = {KernelOfStrategy<CoefT, uint32_t(S)>()..., jxlhip::k_idct_fast<CoefT, 1, 1, true>};
  static_assert(sizeof...(S) == jxlhip::kSubsampledList && sizeof(kTable) / sizeof(kTable[0]) == jxlhip::kTransformLists, "a kernel per list");
  return kTable[list];
}

// A launch per entry of the set's plan (jxh_transform_plan.h), in the plan's order. Every address comes from the frame's
// resolved block (ResolveTransformBlocks).
template <typename CoefT>
static int LaunchTransforms(JxlHipContext* c0) {
  for (const transform_plan::TransformLaunch& L : c0->tlaunches) {
    const dim3 grid(L.grid_x, L.grid_y), block(L.block);
    switch (L.kind) {
      case transform_plan::kListLaunch:
        hipLaunchKernelGGL(ListKernelOf<CoefT>(L.list, std::make_index_sequence<jxlhip::kSubsampledList>()), grid, block, L.lds, c0->stream,
                           c0->tb_params.as<jxlhip::TransformParams>(), c0->tb_desc.as<uint2>() + L.first, L.strategy);
        break;
      case transform_plan::kChromaUpLaunch: {  // a subsampled channel back to the frame's resolution, in front of the filters
        const JxlHipContext* c = c0->down_set[L.frame];
        const jxlhip::TransformParams& tp = c0->tblocks[L.frame];
        const size_t plane = size_t(tp.xp) * tp.yp;
        jxlhip::ChromaUpParams up;
        up.src = tp.cs_out + L.channel * plane;
        up.dst = tp.out + L.channel * plane;
        up.xs = c->xs;
        up.ys = c->ys;
        up.xp = tp.xp;
        up.y0 = c->ext_y0;
        up.y1 = c->ext_y1;
        up.hs = (tp.cs >> (2 * L.channel)) & 1u;
        up.vs = (tp.cs >> (2 * L.channel + 1)) & 1u;
        hipLaunchKernelGGL(jxlhip::k_chroma_upsample, grid, block, 0, c0->stream, up);
        break;
      }
      case transform_plan::kBigLaunch: {  // through the frame's global scratch: one frame at a time (rare)
        const jxlhip::TransformParams& tp = c0->tblocks[L.frame];
        hipLaunchKernelGGL((jxlhip::k_dct_big<CoefT>), grid, block, 0, c0->stream, tp, tp.tlist + tp.list_begin[L.strategy] + L.first, L.count, L.strategy);
        break;
      }
    }
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

static void FillFusedParams(const JxlHipContext* c, jxlhip::FusedFilterParams* p) {
  p->debug = uint32_t(EnvInt("JXLHIP_FILTER_DEBUG", 0));
  p->f = c->fp;
  p->f.in = PlaneHolder(c)->plane[0].as<float>();
  p->f.out = nullptr;
  for (int stage = 0; stage < 3; stage++) {
    const float scale = stage == 0 ? c->epf_pass0 : stage == 2 ? c->epf_pass2 : 1.0f;
    p->sm[stage] = stage == 1 ? 1.65f : float(scale * 1.65);
    p->bsm[stage] = p->sm[stage] * c->epf_border;
  }
  p->filtered = (c->keep_filtered || c->ups != 1 || c->color_out) ? c->plane[1].as<float>() : nullptr;
  if (c->ups != 1 || c->color_out) {
    p->f.rgb = nullptr;
    p->f.rgbf = nullptr;
  }  // the upsampling / colour kernel produces the pixels
  if (c->tensor_fused) {  // (PixelRouteOf: three float planes with adjacent columns, every byte offset below 2^31)
    const JxlHipTensorOut& t = c->tensor;
    const size_t elem = tensor_out::ElemBytes(t.dtype);
    p->t_dtype = t.dtype;
    p->t_data = t.data;
    p->t_stride_c = uint32_t(uint64_t(t.stride_c) * elem);
    p->t_stride_y = uint32_t(uint64_t(t.stride_y) * elem);
    p->t_parity = uint32_t((uintptr_t(t.data) / elem) & 1);
    p->t_clamp01 = t.clamp01 ? 1 : 0;
    for (int ch = 0; ch < 3; ch++) {
      p->t_scale[ch] = t.scale[ch];
      p->t_bias[ch] = t.bias[ch];
    }
  }
}
// Plans the filter launches of a set (jxh_filter_plan.h) into c0->fgroups; `fparams`: the frames' blocks in launch order.
static int PlanFilterLaunches(JxlHipContext* c0, JxlHipContext* const* ctxs, size_t n, std::vector<jxlhip::FusedFilterParams>* fparams) {
  std::vector<jxlhip::FusedFilterParams> blocks(n);
  std::vector<filter_plan::FilterFrame> frames(n);
  for (size_t i = 0; i < n; i++) {
    const JxlHipContext* c = ctxs[i];
    const jxlhip::FusedFilterParams& b = blocks[i];
    FillFusedParams(c, &blocks[i]);
    frames[i] = {filter_plan::FormOf(c->epf_iters, c->gab, c->gray8_fast, c->tensor_fused), c->xs, c->band_y1 - c->band_y0,
                 b.f.rgb != nullptr, b.f.rgbf != nullptr, b.filtered != nullptr, b.f.linear_output != 0};
  }
  filter_plan::FilterPlan plan;
  const int r = filter_plan::PlanFilterGroups(frames.data(), n, &plan);
  if (r) return r;
  c0->fgroups = std::move(plan.groups);
  fparams->resize(n);
  for (size_t j = 0; j < n; j++) (*fparams)[j] = blocks[plan.order[j]];
  return 0;
}
// Each frame's transform block as the set's launches take it: the frame's own, with the planes of whoever holds them now.
static int ResolveTransformBlocks(JxlHipContext* const* ctxs, size_t n, std::vector<jxlhip::TransformParams>* blocks) {
  blocks->resize(n);
  for (size_t i = 0; i < n; i++) {
    const JxlHipContext* c = ctxs[i];
    jxlhip::TransformParams& tp = (*blocks)[i];
    tp = c->tp;
    const JxlHipContext* h = PlaneHolder(c);
    if (!h->plane[0].p || h->plane[0].cap < c->plane_bytes) return JXLHIP_ERR_INVALID_ARGUMENT;  // lender too small
    tp.out = h->plane[0].as<float>();
    if (c->cs && (!c->plane[1].p || c->plane[1].cap < c->plane_bytes)) return JXLHIP_ERR_INVALID_ARGUMENT;
    tp.cs_out = c->plane[1].as<float>();
  }
  return 0;
}
static void PlanTransforms(JxlHipContext* const* ctxs, size_t n, transform_plan::TransformPlan* plan) {
  std::vector<transform_plan::TransformFrame> frames(n);
  for (size_t i = 0; i < n; i++) {
    const JxlHipContext* c = ctxs[i];
    memcpy(frames[i].list_count, c->list_count, sizeof(frames[i].list_count));
    frames[i].cs = c->cs;
    frames[i].xs = c->xs;
    frames[i].ext_y0 = c->ext_y0;
    frames[i].ext_y1 = c->ext_y1;
  }
  transform_plan::PlanTransformLaunches(frames.data(), n, plan);
}
// Builds (or re-uses) the description of a set of frames for the batched transform and filter launches: resolve the
// frames' blocks, plan the transforms, plan the filters, ensure the buffers, copy.
static int PrepareDownstream(JxlHipContext* c0, JxlHipContext* const* ctxs, size_t n) {
  std::vector<uintptr_t> planes(n);  // (what a block's `out` will be)
  for (size_t i = 0; i < n; i++) planes[i] = uintptr_t(PlaneHolder(ctxs[i])->plane[0].p);
  if (c0->down_set.Matches(ctxs, n, planes.data())) return 0;
  c0->down_set.Forget();
  int r;
  if ((r = ResolveTransformBlocks(ctxs, n, &c0->tblocks))) return r;
  transform_plan::TransformPlan tplan;
  PlanTransforms(ctxs, n, &tplan);
  std::vector<jxlhip::FusedFilterParams> fparams;
  if ((r = PlanFilterLaunches(c0, ctxs, n, &fparams))) return r;
  const std::vector<jxlhip::TransformParams>& tparams = c0->tblocks;
  static_assert(sizeof(transform_plan::WorkgroupDesc) == sizeof(uint2), "the kernels read a descriptor as a uint2");
  if ((r = c0->tb_params.Ensure(n * sizeof(tparams[0])))) return r;
  if ((r = c0->tb_desc.Ensure((tplan.desc.size() + 1) * sizeof(uint2)))) return r;
  if ((r = c0->fb_params.Ensure(n * sizeof(fparams[0])))) return r;
  {
    ParamCopy pc;
    if ((r = pc.Begin(c0))) return r;
    if ((r = pc.Add(c0->tb_params.p, tparams.data(), n * sizeof(tparams[0])))) return r;
    if ((r = pc.Add(c0->tb_desc.p, tplan.desc.data(), tplan.desc.size() * sizeof(uint2)))) return r;
    if ((r = pc.Add(c0->fb_params.p, fparams.data(), n * sizeof(fparams[0])))) return r;
    if ((r = pc.End())) return r;
  }
  c0->tlaunches = std::move(tplan.launches);
  c0->down_set.Remember(ctxs, n, planes.data());
  return 0;
}

typedef void (*FusedKernel)(const jxlhip::FusedFilterParams*);
typedef void (*RowsKernel)(const jxlhip::FusedFilterParams*, int);
// The tile kernel of a form with 0 or 3 EPF iterations.
static FusedKernel FusedKernelOf(const filter_plan::FilterForm& f) {
  static const FusedKernel kTable[2][2] = {  // [3 iterations][Gaborish]
      {jxlhip::k_filter_fused<false, 0>, jxlhip::k_filter_fused<true, 0>},
      {jxlhip::k_filter_fused<false, 3>, jxlhip::k_filter_fused<true, 3>}};
  return kTable[f.epf == 3][f.gab];
}
// The row-streaming kernel of a form with 1 or 2 EPF iterations. The tensor writer has one form whatever the group writes;
// the one-channel writer is an 8-bit sRGB form (PlanFilterGroups refuses a grey group that is not).
static RowsKernel RowsKernelOf(const filter_plan::FilterForm& f, bool u8srgb) {
  static const RowsKernel kTable[4][2][2] = {  // [writer][2 iterations][Gaborish]
      {{jxlhip::k_filter_rows2<false, 1, false>, jxlhip::k_filter_rows2<false, 1>},
       {jxlhip::k_filter_rows2<false, 2, false>, jxlhip::k_filter_rows2<false, 2>}},
      {{jxlhip::k_filter_rows2<true, 1, false>, jxlhip::k_filter_rows2<true, 1>},
       {jxlhip::k_filter_rows2<true, 2, false>, jxlhip::k_filter_rows2<true, 2>}},
      {{jxlhip::k_filter_rows2<true, 1, false, true>, jxlhip::k_filter_rows2<true, 1, true, true>},
       {jxlhip::k_filter_rows2<true, 2, false, true>, jxlhip::k_filter_rows2<true, 2, true, true>}},
      {{jxlhip::k_filter_rows2<false, 1, false, false, true>, jxlhip::k_filter_rows2<false, 1, true, false, true>},
       {jxlhip::k_filter_rows2<false, 2, false, false, true>, jxlhip::k_filter_rows2<false, 2, true, false, true>}}};
  return kTable[f.tensor ? 3 : f.grey ? 2 : u8srgb ? 1 : 0][f.epf == 2][f.gab];
}

static int LaunchFused(JxlHipContext* c0, const filter_plan::FilterGroup& g) {
  const FusedKernel k = FusedKernelOf(g.form);
  const size_t lds = jxlhip::FusedLdsBytes(g.form.gab, g.form.epf);
  if (lds > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
  for (uint32_t z = 0; z < g.count; z += 65535) {  // grid z limit
    const uint32_t zn = g.count - z < 65535 ? g.count - z : 65535;
    hipLaunchKernelGGL(k, dim3(g.tiles_x, g.tiles_y, zn), dim3(jxlhip::kFusedThreads), lds, c0->fstream,
                       c0->fb_params.as<jxlhip::FusedFilterParams>() + g.first + z);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// (Gaborish +) EPF1 (the d1.0 configuration) or EPF1 + EPF2: the row-streaming kernel, no LDS.
static int LaunchFilterRows(JxlHipContext* c0, const filter_plan::FilterGroup& g) {
  const filter_plan::RowsGridDims d = filter_plan::RowsGrid(g.tiles_x, g.tiles_y, g.count);
  const RowsKernel k = RowsKernelOf(g.form, g.u8srgb);
  for (uint32_t z = 0; z < g.count; z += 65535) {  // grid z limit
    const uint32_t zn = g.count - z < 65535 ? g.count - z : 65535;
    const jxlhip::FusedFilterParams* fp = c0->fb_params.as<jxlhip::FusedFilterParams>() + g.first + z;
    hipLaunchKernelGGL(k, dim3(d.gx, d.gy, zn), dim3(64 * jxlhip::kRowsWaves), 0, c0->fstream, fp, int(d.strip));
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// A launch per group of the set's plan, in the plan's order.
static int LaunchFilterGroups(JxlHipContext* c0) {
  for (const filter_plan::FilterGroup& g : c0->fgroups) {
    int r;
    switch (filter_plan::KernelOf(g.form)) {
      case filter_plan::kFusedKernel: r = LaunchFused(c0, g); break;
      case filter_plan::kRowsKernel: r = LaunchFilterRows(c0, g); break;
      default: r = JXLHIP_ERR_INVALID_ARGUMENT;
    }
    if (r) return r;
  }
  return 0;
}

// Validates a set for a batched downstream call and orders the launch stream after everything its frames wait for.
static int EnsureOwnStream(JxlHipContext* c) {
  if (c->owns_stream) return 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));  // (what the context queued on the shared stream so far)
  hipStream_t st = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  c->stream = st;
  c->owns_stream = true;
  return 0;
}

// A batched entropy launch must get the machine FIRST. Its workgroups are few (one per frame), long-lived and large in LDS
// (37 - 54 KB: 640 of them take 84 % of the chip's LDS); when a transform launch of another frame set is already streaming
// its small workgroups through the CUs, the entropy workgroups find no CU with that much LDS free and trickle in only as the
// other launch drains: 133 ms per launch instead of 62 ms (scripts/r03_interference.py; 80 ms behind a filter launch,
// which holds registers, not LDS). Arriving first it loses nothing to the same neighbours (62 ms). So: every workgroup of a
// batched entropy launch counts itself in when it starts, and the batched transform / filter launches enqueued after it,
// on whatever stream, wait (hipStreamWaitValue64, a wait packet in their own queue) until that count says the whole
// entropy launch is resident. The counter only grows: a launch's target is the running total after it.
struct EntropyGate {
  unsigned long long* counter = nullptr;  // device memory (hipMallocSignalMemory)
  unsigned long long total = 0;           // workgroups of every launch so far
  unsigned long long target = 0;          // count at which the latest launch is resident
  unsigned cus = 256;                     // compute units and LDS bytes per unit of the device (read with the counter)
  size_t lds_per_cu = 160 * 1024;
  bool tried = false;
};
static std::mutex g_gate_mu;
static EntropyGate g_gate[16];
// True when this process's kernels may be run one at a time (runtime debug switches, a single hardware queue, counter
// collection by a profiler): a device-side wait for ANOTHER launch's workgroups could then wait for a kernel that is not
// allowed to start, so the gate is never used there. Read once.
static bool RuntimeMaySerialise() {
  static const bool v = [] {
    auto on = [](const char* n) {
      const char* e = getenv(n);
      return e && *e && !(e[0] == '0' && !e[1]);
    };
    if (on("AMD_SERIALIZE_KERNEL") || on("AMD_SERIALIZE_COPY") || on("HIP_LAUNCH_BLOCKING") || on("ROCPROF_COUNTER_COLLECTION") ||
        on("HSA_ENABLE_DEBUG") || on("ROCM_DEBUG_AGENT") || on("HIP_ENABLE_DEFERRED_LOADING_DEBUG"))
      return true;
    if (const char* q = getenv("GPU_MAX_HW_QUEUES"))
      if (*q && atoi(q) < 2) return true;
    if (const char* t = getenv("HSA_TOOLS_LIB"))  // a debugger / tracer intercepting the queues (rocgdb, roctracer)
      if (*t && (strstr(t, "debug") || strstr(t, "rocgdb"))) return true;
    return false;
  }();
  return v;
}
// the counter the next batched entropy launch of `device` counts into (NULL: gating unavailable, not asked for by the
// caller -- option "entropy_gate" of the launch's first context, off by default -- or unsafe in this process)
static unsigned long long* GateCounter(const JxlHipContext* c0) {
  const int device = c0->device;
  if (device < 0 || device >= 16 || !c0->entropy_gate || !EnvInt("JXLHIP_ENTROPY_GATE", 1) || RuntimeMaySerialise()) return nullptr;
  std::lock_guard<std::mutex> lk(g_gate_mu);
  EntropyGate& g = g_gate[device];
  if (!g.tried) {
    g.tried = true;
    int can = 0;
    if (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, device) == hipSuccess && can) {
      void* p = nullptr;
      if (hipExtMallocWithFlags(&p, 8, hipMallocSignalMemory) == hipSuccess && hipMemset(p, 0, 8) == hipSuccess)
        g.counter = static_cast<unsigned long long*>(p);
    }
    (void)hipGetLastError();
    int cus = 0, lds = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) g.cus = unsigned(cus);
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, device) == hipSuccess && lds > 0) g.lds_per_cu = size_t(lds);
    (void)hipGetLastError();
  }
  return g.counter;
}
static void GateAdvance(int device, unsigned long long workgroups, unsigned long long resident_cap) {
  std::lock_guard<std::mutex> lk(g_gate_mu);
  EntropyGate& g = g_gate[device];
  g.target = g.total + (workgroups < resident_cap ? workgroups : resident_cap);
  g.total += workgroups;
}
static int GateWait(int device, hipStream_t stream) {
  if (device < 0 || device >= 16) return 0;
  unsigned long long* counter;
  unsigned long long target;
  {
    std::lock_guard<std::mutex> lk(g_gate_mu);
    counter = g_gate[device].counter;
    target = g_gate[device].target;
  }
  if (!counter || !target) return 0;
  HIP_TRY(hipStreamWaitValue64(stream, counter, target, hipStreamWaitValueGte, ~0ull));
  return 0;
}

static int BeginDownstreamBatch(JxlHipContext* const* ctxs, size_t n, bool filter_stage = false) {
  if (!ctxs || !n) return JXLHIP_ERR_INVALID_ARGUMENT;
  JxlHipContext* c0 = ctxs[0];
  for (size_t i = 0; i < n; i++) {
    if (!ctxs[i]) return JXLHIP_ERR_INVALID_ARGUMENT;
    if (ctxs[i]->red.have) return JXLHIP_ERR_UNSUPPORTED;  // (a reduced upload has neither transforms nor filters)
    if (!ctxs[i]->have_frame) return JXLHIP_ERR_NO_FRAME;
    if (ctxs[i]->device != c0->device || ctxs[i]->coef_bits != c0->coef_bits) return JXLHIP_ERR_INVALID_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(c0->device));
  if (n > 1) {
    const int r = EnsureOwnStream(c0);
    if (r) return r;
  }
  hipStream_t ls = c0->stream;  // launch stream
  if (filter_stage && c0->filter_async) {
    if (!c0->stream2) {
      HIP_TRY(hipStreamCreateWithFlags(&c0->stream2, hipStreamNonBlocking));
      if (!c0->fork_event) HIP_TRY(hipEventCreateWithFlags(&c0->fork_event, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&c0->filter_done, hipEventDisableTiming));
    }
    ls = c0->stream2;
    if (c0->transform_done_valid) {
      // after the set's transform launch, NOT after whatever the first stream has been given since: the caller may
      // already have queued the set's next entropy launch there (which must reach the machine before this launch does:
      // see EntropyGate), and the filter stage has nothing to do with it
      HIP_TRY(hipStreamWaitEvent(ls, c0->transform_done, 0));
    } else {
      HIP_TRY(hipEventRecord(c0->fork_event, c0->stream));  // after everything the first stream holds
      HIP_TRY(hipStreamWaitEvent(ls, c0->fork_event, 0));
    }
  }
  c0->fstream = ls;
  if (n > 1 && c0->entropy_gate && !RuntimeMaySerialise()) {  // (see EntropyGate)
    const int r = GateWait(c0->device, ls);
    if (r) return r;
  }
  hipEvent_t waited = nullptr;
  for (size_t i = 0; i < n; i++)
    if (ctxs[i]->pending_wait) {
      if (ctxs[i]->pending_wait != waited) HIP_TRY(hipStreamWaitEvent(ls, ctxs[i]->pending_wait, 0));
      waited = ctxs[i]->pending_wait;
      ctxs[i]->pending_wait = nullptr;
    }
  // planes / pixels still in use by an asynchronous filter launch: wait for it, once per event
  waited = nullptr;
  for (size_t i = 0; i < n; i++)
    if (ctxs[i]->filter_wait) {
      if (ctxs[i]->filter_wait != waited) HIP_TRY(hipStreamWaitEvent(ls, ctxs[i]->filter_wait, 0));
      waited = ctxs[i]->filter_wait;
      ctxs[i]->filter_wait = nullptr;
    }
  // plane buffers last read by a filter launch on another stream (shared planes): wait for that launch, once per event
  waited = nullptr;
  for (size_t i = 0; i < n; i++) {
    JxlHipContext* h = PlaneHolder(ctxs[i]);
    if (h->planes_event && h->planes_stream != ls && h->planes_event != waited) {
      HIP_TRY(hipStreamWaitEvent(ls, h->planes_event, 0));
      waited = h->planes_event;
    }
  }
  return PrepareDownstream(c0, ctxs, n);
}
static int EndDownstreamBatch(JxlHipContext* const* ctxs, size_t n, bool filter_stage = false) {
  JxlHipContext* c0 = ctxs[0];
  bool shared = false;
  for (size_t i = 0; i < n && !shared; i++) shared = ctxs[i]->plane_lender != nullptr || ctxs[i]->planes_event != nullptr;
  hipEvent_t done = nullptr;
  if (filter_stage && c0->fstream != c0->stream) {  // asynchronous filter launch: every context of it remembers its end
    HIP_TRY(hipEventRecord(c0->filter_done, c0->fstream));
    done = c0->filter_done;
    for (size_t i = 0; i < n; i++) ctxs[i]->filter_wait = done;
  } else if (n > 1 || shared) {
    if (!c0->down_done) HIP_TRY(hipEventCreateWithFlags(&c0->down_done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c0->down_done, c0->stream));
    done = c0->down_done;
    for (size_t i = 1; i < n; i++) ctxs[i]->pending_wait = done;
  }
  if (!filter_stage && c0->filter_async) {
    if (!c0->transform_done) HIP_TRY(hipEventCreateWithFlags(&c0->transform_done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c0->transform_done, c0->stream));
    c0->transform_done_valid = true;
  }
  if (shared && filter_stage)
    for (size_t i = 0; i < n; i++) {
      JxlHipContext* h = PlaneHolder(ctxs[i]);
      h->planes_event = done;
      h->planes_stream = c0->fstream;
    }
  return 0;
}

template <typename CoefT, bool AIDS, bool GALIAS, bool PREFIX = false, bool A6 = false>
static int LaunchEntropyLanesW(JxlHipContext* c0) {
  auto k = jxlhip::k_entropy_lanes<CoefT, AIDS, GALIAS, PREFIX, A6>;
  const lane_plan::LanePlan& P = c0->batch_plan;
  if (P.lds > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, int(P.lds)));
  jxlhip::EntropyLaneBatch b;
  b.params = c0->batch_params.as<jxlhip::EntropyParams>();
  uint8_t* blob = c0->batch_lanes.as<uint8_t>();
  b.wg_unit = c0->batch_map.as<uint32_t>();
  b.list = reinterpret_cast<const uint32_t*>(blob);
  b.units = reinterpret_cast<const uint4*>(blob + P.off_units);
  b.queue = reinterpret_cast<uint32_t*>(blob + P.off_queue);
  b.wave_lanes = blob + P.off_wave_lanes;
  HIP_TRY(hipMemsetAsync(b.queue, 0, P.units * 4, c0->stream));
  b.wait_shift = P.wait_shift;
  b.refill_mask = jxlhip::kLanesAsmTrip<CoefT, GALIAS, PREFIX> ? 0u : jxlhip::kLanesRefillEvery - 1;
  b.extra_pass_min = jxlhip::kLanesExtraPassMin;
  b.debug = uint32_t(EnvInt("JXLHIP_LANES_DEBUG", 0));
  b.prof = nullptr;
  b.started = c0->batch_set.size() > 1 ? GateCounter(c0) : nullptr;
  // debugging aid: per-wave cycle split, printed to stderr (1); 2: per-wave start and end on the clock all XCDs share, kept
  // for jxlhip_debug_entropy_timeline and not waited for, so that the launches around this one overlap it as they do unprofiled
  const int prof_mode = EnvInt("JXLHIP_LANES_PROF", 0);
  const bool prof = prof_mode != 0 && prof_mode != 2;
  const size_t nwaves = P.wg_unit.size();
  if (AIDS && prof_mode == 2) {
    constexpr size_t kTimelineKeep = sizeof(c0->timeline_wgs) / sizeof(c0->timeline_wgs[0]);
    if (nwaves * 64 > c0->timeline_stride) {  // (the first launch, or a larger one: earlier records are dropped)
      HIP_TRY(hipStreamSynchronize(c0->stream));
      int r = c0->lanes_timeline.Ensure(nwaves * 64 * kTimelineKeep);
      if (r) return r;
      c0->timeline_stride = nwaves * 64;
      for (size_t& w : c0->timeline_wgs) w = 0;
    }
    const size_t slot = c0->timeline_launches++ % kTimelineKeep;
    c0->timeline_wgs[slot] = nwaves;
    b.prof = reinterpret_cast<unsigned long long*>(c0->lanes_timeline.as<uint8_t>() + slot * c0->timeline_stride);
    b.debug |= 64;
    HIP_TRY(hipMemsetAsync(b.prof, 0, nwaves * 64, c0->stream));
  }
  if (prof) {
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&b.prof), nwaves * 64));
    HIP_TRY(hipMemsetAsync(b.prof, 0, nwaves * 64, c0->stream));
  }
  hipLaunchKernelGGL(k, dim3(uint32_t(P.wg_unit.size())), dim3(64), P.lds, c0->stream, b);
  HIP_TRY(hipGetLastError());
  if (b.started) {
    // "resident" = as many of its workgroups as the chip's LDS holds at once, less a margin (the rest start as the first
    // ones end, and are not waited for)
    unsigned long long cus, lds_cu;
    {
      std::lock_guard<std::mutex> lk(g_gate_mu);
      cus = g_gate[c0->device].cus;
      lds_cu = g_gate[c0->device].lds_per_cu;
    }
    const unsigned long long per_cu = P.lds ? lds_cu / P.lds : 8, cap = cus * (per_cu ? per_cu : 1) * 3 / 4;
    GateAdvance(c0->device, P.wg_unit.size(), cap);
  }
  if (prof) {
    std::vector<unsigned long long> h(nwaves * 8);
    HIP_TRY(hipStreamSynchronize(c0->stream));
    HIP_TRY(hipMemcpy(h.data(), b.prof, nwaves * 64, hipMemcpyDeviceToHost));
    (void)hipFree(b.prof);
    // per wave: {cycles total, cycles in service, service calls, hot trips, lane-trips taken, service: waiting for the
    // previous phase's DMA / flush + DMA requests / transitions}; one JSON line: the longest wave and the mean over waves
    unsigned long long mx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    size_t used = 0;
    for (size_t w = 0; w < nwaves; w++) {
      if (!h[w * 8 + 3] && !h[w * 8 + 2]) continue;
      used++;
      if (h[w * 8] > mx[0]) for (int j = 0; j < 8; j++) mx[j] = h[w * 8 + j];
      for (int j = 0; j < 8; j++) sum[j] += double(h[w * 8 + j]);
    }
    const char* names[8] = {"cycles", "refill_cycles", "passes", "trips", "lane_trips", "trip_cycles", "pass_lanes_served", "pass_cycles"};
    std::string line = "{\"waves\": " + std::to_string(used) + ", \"longest\": {";
    for (int j = 0; j < 8; j++) line += std::string(j ? ", " : "") + "\"" + names[j] + "\": " + std::to_string(mx[j]);
    line += "}, \"mean\": {";
    for (int j = 0; j < 8; j++) line += std::string(j ? ", " : "") + "\"" + names[j] + "\": " + std::to_string((unsigned long long)(sum[j] / (used ? used : 1)));
    line += "}}";
    fprintf(stderr, "[lanes prof] %s\n", line.c_str());
    if (b.debug & 16)  // (measurement aid: per wave: cycles, trips, HW_ID fields wave / simd / cu / sh / se, XCC)
      for (size_t w = 0; w < nwaves && w < 64; w++) {
        const unsigned long long hw = h[w * 8 + 6];
        fprintf(stderr, "[lanes wave] %zu cycles %llu trips %llu trip_cycles %llu pass_cycles %llu passes %llu refill_cycles %llu simd %llu cu %llu sh %llu se %llu xcc %llu\n", w, h[w * 8], h[w * 8 + 3], h[w * 8 + 5], h[w * 8 + 7], h[w * 8 + 2], h[w * 8 + 1], (hw >> 4) & 3,
                (hw >> 8) & 15, (hw >> 12) & 1, (hw >> 13) & 7, (hw >> 32) & 15);
      }
  }
  return 0;
}

// The lane kernel's forms: prefix codes, six-byte LDS tables (int16 coefficients), or alias tables in LDS / in global
// memory; the last two also as the instrumented build (JXLHIP_LANES_DEBUG / JXLHIP_LANES_PROF, measurement aids).
template <typename CoefT>
static int LaunchEntropyLanes(JxlHipContext* c0) {
  const lane_plan::LanePlan::Form form = c0->batch_plan.form;
  if (form == lane_plan::LanePlan::kPrefix) return LaunchEntropyLanesW<CoefT, false, true, true>(c0);
  if constexpr (sizeof(CoefT) == 2) {
    if (form == lane_plan::LanePlan::kLds6) return LaunchEntropyLanesW<CoefT, false, false, false, true>(c0);
  }
  const bool galias = form == lane_plan::LanePlan::kGlobal;
  if (EnvInt("JXLHIP_LANES_DEBUG", 0) || EnvInt("JXLHIP_LANES_PROF", 0))
    return galias ? LaunchEntropyLanesW<CoefT, true, true>(c0) : LaunchEntropyLanesW<CoefT, true, false>(c0);
  return galias ? LaunchEntropyLanesW<CoefT, false, true>(c0) : LaunchEntropyLanesW<CoefT, false, false>(c0);
}

template <typename CoefT>
static int LaunchEntropyUniBatch(JxlHipContext* c0) {
  auto k = jxlhip::k_entropy_uni<CoefT, kEntropyWPG>;
  const lane_plan::LanePlan& P = c0->batch_plan;
  if (P.lds > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, int(P.lds)));
  jxlhip::EntropyBatch b{c0->batch_params.as<jxlhip::EntropyParams>(), c0->batch_map.as<uint32_t>()};
  hipLaunchKernelGGL(k, dim3(uint32_t(P.wg_unit.size())), dim3(64 * kEntropyWPG), P.lds, c0->stream, b);
  HIP_TRY(hipGetLastError());
  return 0;
}

// Builds (or re-uses) the description of a batch in four steps: key, plan, place, remember. The plan (jxh_lane_plan.h) is
// a function of the set, the device and the measurement aids, so these are the key; it holds the workgroup map and, for
// the lane-parallel kernel, the lane -> section assignment, and stays in the context for the launch to read.
static int PrepareBatch(JxlHipContext* c0, JxlHipContext* const* ctxs, size_t n, int kernel) {
  const lane_plan::LaneOverrides overrides = LaneOverridesFromEnv();
  if (c0->batch_set.Matches(ctxs, n) && c0->batch_kernel == kernel && c0->batch_overrides == overrides) return 0;

  lane_plan::LanePlan plan;
  if (kernel == 2) {
    std::vector<lane_plan::LaneFrame> frames(n);
    for (size_t i = 0; i < n; i++) {
      const JxlHipContext* c = ctxs[i];
      frames[i] = {c->ng, c->np, c->ep.num_hist, c->ep.nctx, c->sec_size_host.data(), c->sec_sel_host.data(), c->group_list.data(),
                   c->group_list.size(), !c->absent_sections.empty(), c->gbb_host.data(), c->gbb_host.size(), c->pass_clusters.data(),
                   c->pass_log_alpha.data()};
    }
    lane_plan::LaneBatchTraits traits;
    traits.prefix = c0->lane_prefix;
    traits.coef_bits = c0->coef_bits;
    traits.lds_budget = kLdsBudget;
    int dev_cus = int(traits.device_cus);  // (what a failing query leaves)
    (void)hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, c0->device);
    traits.device_cus = uint32_t(dev_cus);
    plan = lane_plan::PlanLaneBatch(frames.data(), n, traits, overrides);
    if (EnvInt("JXLHIP_PACK_DEBUG", 0))
      fprintf(stderr, "[pack] units %zu sections %zu lanes(min) %zu lanes/wave %u waves/wg 1 workgroups %zu lds %zu tables %s\n", plan.units,
              plan.total_sections, plan.min_lanes_total, plan.lanes_per_wave, plan.wg_unit.size(), plan.lds, lane_plan::FormName(plan.form));
  } else {
    std::vector<uint32_t> groups(n);
    std::vector<size_t> table_bytes(n);
    for (size_t i = 0; i < n; i++) {
      groups[i] = ctxs[i]->ng;
      table_bytes[i] = size_t(ctxs[i]->ep.lds_ctx_bytes) + ctxs[i]->ep.lds_alias_bytes;
    }
    plan = lane_plan::PlanUniBatch(groups.data(), table_bytes.data(), n, kEntropyWPG);
  }

  std::vector<jxlhip::EntropyParams> params(n);
  for (size_t i = 0; i < n; i++) params[i] = ctxs[i]->ep;
  int r;
  if ((r = c0->batch_params.Ensure(params.size() * sizeof(params[0])))) return r;
  if ((r = c0->batch_map.Ensure(plan.wg_unit.size() * 4))) return r;
  ParamCopy pc;
  if ((r = pc.Begin(c0))) return r;
  if ((r = pc.Add(c0->batch_params.p, params.data(), params.size() * sizeof(params[0])))) return r;
  if ((r = pc.Add(c0->batch_map.p, plan.wg_unit.data(), plan.wg_unit.size() * 4))) return r;
  if (!plan.list.empty()) {
    std::vector<uint8_t> blob(plan.blob_bytes);
    lane_plan::PackLaneBlob(plan, blob.data());
    if ((r = c0->batch_lanes.Ensure(blob.size()))) return r;
    if ((r = pc.Add(c0->batch_lanes.p, blob.data(), blob.size()))) return r;
  }
  if ((r = pc.End())) return r;

  c0->batch_set.Remember(ctxs, n);
  c0->batch_kernel = kernel;
  c0->batch_overrides = overrides;
  c0->batch_plan = std::move(plan);
  return 0;
}

extern "C" int jxlhip_run_entropy_batch(JxlHipContext* const* ctxs, size_t n) {
  if (!ctxs || !n || n > 0xFFFF) return JXLHIP_ERR_INVALID_ARGUMENT;
  JxlHipContext* c0 = ctxs[0];
  // One launch needs one kernel: every frame in scan-order layout (lane kernel), or every frame in natural layout with
  // tables that the scalar-form kernel can share in LDS; anything else is decoded frame by frame.
  bool all_scan = true, all_uni = true;
  for (size_t i = 0; i < n; i++) {
    const JxlHipContext* c = ctxs[i];
    if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
    if (c->red.have) return JXLHIP_ERR_UNSUPPORTED;
    if (!c->have_frame) return JXLHIP_ERR_NO_FRAME;
    if (c->device != c0->device) return JXLHIP_ERR_INVALID_ARGUMENT;
    if (n > 1 && !c->absent_groups.empty()) return JXLHIP_ERR_INVALID_ARGUMENT;  // (partial frames go one at a time: jxlhip_run_entropy)
    if (!c->lanes || c->coef_bits != c0->coef_bits || c->lane_prefix != c0->lane_prefix) all_scan = false;
    if (c->lanes || c->generic_codec || !c->alias_lds || c->ep.num_hist != 1 || c->np != 1 || c->coef_bits != c0->coef_bits ||
        c->ng > 0xFFFF * kEntropyWPG)
      all_uni = false;
  }
  if (!all_scan && !all_uni) {
    for (size_t i = 0; i < n; i++) {
      int r = ctxs[i]->lanes ? jxlhip_run_entropy_batch(&ctxs[i], 1) : RunEntropySingle(ctxs[i]);
      if (r) return r;
    }
    return 0;
  }
  const int kernel = all_scan ? 2 : 1;
  HIP_TRY(hipSetDevice(c0->device));
  if (n > 1) {
    const int r = EnsureOwnStream(c0);
    if (r) return r;
  }
  // measurement aid: JXLHIP_BATCH_PROF=1 prints the host time of the phases of this call (microseconds)
  const bool prof = EnvInt("JXLHIP_BATCH_PROF", 0) != 0;
  std::chrono::steady_clock::time_point tp0 = std::chrono::steady_clock::now();
  std::string prof_line;
  auto lap = [&](const char* what) {
    if (!prof) return;
    const auto now = std::chrono::steady_clock::now();
    prof_line += std::string(what) + " " + std::to_string(std::chrono::duration_cast<std::chrono::microseconds>(now - tp0).count()) + "  ";
    tp0 = now;
  };
  if (!c0->batch_done) HIP_TRY(hipEventCreateWithFlags(&c0->batch_done, hipEventDisableTiming));
  int r = PrepareBatch(c0, ctxs, n, kernel);
  if (r) return r;
  lap("prepare");
  // the batch kernel runs on the first context's stream, after whatever the other contexts still have in flight
  for (size_t i = 1; i < n; i++) {
    if (ctxs[i]->ev_valid[2]) HIP_TRY(hipStreamWaitEvent(c0->stream, ctxs[i]->ev[5], 0));
  }
  hipEvent_t waited = nullptr;
  for (size_t i = 0; i < n; i++)
    if (ctxs[i]->pending_wait) {  // results of an earlier batch launch that nobody consumed: order after that launch
      if (ctxs[i]->pending_wait != waited) HIP_TRY(hipStreamWaitEvent(c0->stream, ctxs[i]->pending_wait, 0));
      waited = ctxs[i]->pending_wait;
      ctxs[i]->pending_wait = nullptr;
    }
  lap("waits");
  HIP_TRY(hipEventRecord(c0->ev[0], c0->stream));
  for (size_t i = 0; i < n; i++)  // (the lane kernel writes every section's flag word itself, unless passes share it)
    if (kernel != 2 || ctxs[i]->np > 1) HIP_TRY(hipMemsetAsync(ctxs[i]->errors.p, 0, size_t(ctxs[i]->ng) * 4, c0->stream));
  if (kernel == 2) r = c0->coef_bits == 16 ? LaunchEntropyLanes<int16_t>(c0) : LaunchEntropyLanes<int32_t>(c0);
  else r = c0->coef_bits == 16 ? LaunchEntropyUniBatch<int16_t>(c0) : LaunchEntropyUniBatch<int32_t>(c0);
  if (r) return r;
  if (kernel == 2)
    for (size_t i = 0; i < n; i++) {  // progressive frames: sum the passes into the natural layout
      const JxlHipContext* c = ctxs[i];
      if (!c->lane_multi) continue;
      jxlhip::MergeParams m;
      m.coeffs = c->coeffs.p;
      m.blocks = c->blocks.as<JxlHipVarBlock>();
      m.passes = c->passes_dev.as<jxlhip::PassDev>();
      m.kend = c->kend.as<uint32_t>();
      m.pass_stride = c->ep.coef_pass_stride;
      m.num_blocks = c->nblocks;
      m.num_passes = c->np;
      m.xg = c->xg;
      m.kend_stride = c->ep.kend_pass_stride;
      if (!m.num_blocks) continue;
      if (c->coef_bits == 16) hipLaunchKernelGGL(jxlhip::k_merge_passes<int16_t>, dim3(m.num_blocks), dim3(64), 0, c0->stream, m);
      else hipLaunchKernelGGL(jxlhip::k_merge_passes<int32_t>, dim3(m.num_blocks), dim3(64), 0, c0->stream, m);
      HIP_TRY(hipGetLastError());
    }
  lap("launch");
  if (prof) fprintf(stderr, "[entropy batch] %s\n", prof_line.c_str());
  HIP_TRY(hipEventRecord(c0->ev[1], c0->stream));
  c0->ev_valid[0] = true;
  if (n > 1) {
    HIP_TRY(hipEventRecord(c0->batch_done, c0->stream));
    for (size_t i = 1; i < n; i++) {
      ctxs[i]->pending_wait = c0->batch_done;
      ctxs[i]->ev_valid[0] = false;
    }
  }
  return 0;
}

// Groups whose AC sections have not arrived (JxlHipFrameDesc::group_absent): no coefficients at all, so that the transform
// stage draws their blocks from the lowest frequencies (the DC image) alone. Queued in front of the entropy launch.
static int ZeroAbsentGroups(JxlHipContext* c) {
  if (c->absent_groups.empty() && c->absent_sections.empty()) return 0;
  HIP_TRY(hipSetDevice(c->device));
  const size_t coef_group_bytes = size_t(3) * 65536 * (c->coef_bits / 8);
  for (size_t i = 0; i < c->absent_groups.size(); i++) {
    const uint32_t g = c->absent_groups[i], b0 = c->absent_blocks[2 * i], nb = c->absent_blocks[2 * i + 1];
    HIP_TRY(hipMemsetAsync(c->coeffs.as<uint8_t>() + size_t(g) * coef_group_bytes, 0, coef_group_bytes, c->stream));
    for (uint32_t p = 0; p < c->np && nb && c->lanes; p++)  // (the scan-order layout's counts; the other kernels zero-fill natural layout)
      HIP_TRY(hipMemsetAsync(c->kend.as<uint32_t>() + size_t(p) * c->ep.kend_pass_stride + size_t(b0) * 3, 0, size_t(nb) * 12, c->stream));
  }
  for (size_t i = 0; c->lanes && i + 2 < c->absent_sections.size(); i += 3) {  // passes that have not arrived add nothing (k_merge_passes)
    const uint32_t p = c->absent_sections[i], b0 = c->absent_sections[i + 1], nb = c->absent_sections[i + 2];
    if (nb) HIP_TRY(hipMemsetAsync(c->kend.as<uint32_t>() + size_t(p) * c->ep.kend_pass_stride + size_t(b0) * 3, 0, size_t(nb) * 12, c->stream));
  }
  return 0;
}

extern "C" int jxlhip_run_entropy(JxlHipContext* c) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->red.have) return JXLHIP_ERR_UNSUPPORTED;
  if (!c->have_frame) return JXLHIP_ERR_NO_FRAME;
  const int r = ZeroAbsentGroups(c);
  if (r) return r;
  if (c->group_list.empty()) {  // (nothing but the DC image has arrived)
    HIP_TRY(hipMemsetAsync(c->errors.p, 0, size_t(c->ng) * 4, c->stream));
    return 0;
  }
  return c->lanes ? jxlhip_run_entropy_batch(&c, 1) : RunEntropySingle(c);
}


// ------------------------------------------------------------------------------------------------ Modular frames
// What the context remembers of a Modular frame beside its tables.
static void AdoptModFrame(JxlHipContext* c, const JxlHipModFrameDesc& d, const upload::ModPlan& P) {
  JxlHipContext::Modular& M = c->mod;
  M.buf_off = P.buf_off;
  M.buf_w.resize(d.num_buffers);
  M.buf_h.resize(d.num_buffers);
  for (uint32_t i = 0; i < d.num_buffers; i++) {
    M.buf_w[i] = d.buffers[i].w;
    M.buf_h[i] = d.buffers[i].h;
  }
  M.code_table_words = P.table_words;
  M.nstreams = d.num_streams;
  M.stream_samples.resize(d.num_streams);
  for (uint32_t i = 0; i < d.num_streams; i++) M.stream_samples[i] = d.streams[i].num_samples;
  M.ops.assign(d.ops, d.ops + d.num_ops);
  for (uint32_t j = 0; j < d.num_color + (d.has_alpha ? 1 : 0); j++) M.out_buffer[j] = d.out_buffer[j];
  M.num_color = d.num_color;
  M.has_alpha = d.has_alpha;
  M.bits = d.bits;
  M.alpha_bits = d.alpha_bits;
  M.xs = d.xsize;
  M.ys = d.ysize;
  c->oxs = c->xs = d.xsize;
  c->oys = c->ys = d.ysize;
  M.xyb = d.xyb != 0;
  if (M.xyb) {
    memset(&M.xyb_color, 0, sizeof(M.xyb_color));
    for (int ch = 0; ch < 3; ch++) {
      M.xyb_factor[ch] = d.xyb_factor[ch];
      M.xyb_color.opsin_bias[ch] = d.opsin_bias[ch];
      M.xyb_color.opsin_bias_cbrt[ch] = cbrtf(d.opsin_bias[ch]);
    }
    memcpy(M.xyb_color.opsin_inv, d.opsin_inv, sizeof(M.xyb_color.opsin_inv));
    M.xyb_color.linear_output = d.linear_output;
  }
  M.xyb_target = d.color_target ? *d.color_target : JxlHipColorTarget{};
  AdoptSplines(c, d.splines);
  AdoptPatches(c, d.patches);
}

// The buffers of a Modular frame: those its tables go to and those the kernels write (launch functions never allocate).
// The order of the first allocations decides the buffers' addresses: with `streams` in front of `status` the lossless
// benchmark ran 0.6 % slower on identical kernels (profiles/modular_upload_compare.txt).
static int EnsureModBuffers(JxlHipContext* c, const JxlHipModFrameDesc& d, const upload::ModPlan& P) {
  JxlHipContext::Modular& M = c->mod;
  int r;
  if ((r = M.pool.Ensure((P.pool_ints + 4) * 4))) return r;
  // (a channel buffer that no stream covers must read as zeros, not as the previous frame's samples)
  HIP_TRY(hipMemsetAsync(M.pool.p, 0, (P.pool_ints + 4) * 4, c->stream));
  if ((r = M.sections.Ensure(P.section_bytes))) return r;
  if ((r = M.blob.Ensure(P.blob_bytes + 16))) return r;
  if ((r = M.rects.Ensure(upload::ModChannelEntries(d) * sizeof(jxlhip::ModChannel)))) return r;
  if ((r = M.status.Ensure((size_t(d.num_streams) + 1) * 4))) return r;
  if ((r = M.end_bits.Ensure((size_t(d.num_streams) + 1) * 4))) return r;
  if ((r = M.scratch.Ensure((P.scratch_ints + 4) * 4))) return r;
  if ((r = M.windows.Ensure((P.window_words + 4) * 4))) return r;
  if ((r = M.streams.Ensure(std::max<size_t>(16, size_t(d.num_streams) * sizeof(jxlhip::ModStream))))) return r;
  if (!c->tensor_bound && (r = c->rgb.Ensure(OwnPixelBytes(c)))) return r;
  if (P.float_planes && (r = c->spl_planes.Ensure(size_t(d.xsize) * d.ysize * 3 * 4))) return r;
  return 0;
}

// Every table of the frame, built in the staging block with the device addresses it will hold, and sent from there on
// the context's stream. The stream descriptors also stay on the host: jxlhip_modular_run_batch sorts those of a set.
static int SendModTables(JxlHipContext* c, const JxlHipModFrameDesc& d, const upload::ModPlan& P) {
  JxlHipContext::Modular& M = c->mod;
  auto send = [c](Buf& dst, size_t bytes, auto&& fill) -> int {
    void* st = nullptr;
    const int r = StageAlloc(c, bytes, &st);
    if (r || !bytes) return r;
    fill(st);
    HIP_TRY(hipMemcpyAsync(dst.p, st, bytes, hipMemcpyHostToDevice, c->stream));
    return 0;
  };
  upload::ModBases b;
  b.pool = uintptr_t(M.pool.p);
  b.sections = uintptr_t(M.sections.p);
  b.blob = uintptr_t(M.blob.p);
  b.rects = uintptr_t(M.rects.p);
  b.scratch = uintptr_t(M.scratch.p);
  b.windows = uintptr_t(M.windows.p);
  b.status = uintptr_t(M.status.p);
  b.end_bits = uintptr_t(M.end_bits.p);
  int r;
  if ((r = send(M.sections, P.section_bytes, [&](void* p) { upload::PackModSections(d, P, static_cast<uint8_t*>(p)); }))) return r;
  if ((r = send(M.blob, P.blob_bytes, [&](void* p) { upload::BuildModBlob(d, P, static_cast<uint8_t*>(p), b.blob); }))) return r;
  if ((r = send(M.rects, upload::ModChannelEntries(d) * sizeof(jxlhip::ModChannel),
                [&](void* p) { upload::BuildModChannels(d, P, static_cast<jxlhip::ModChannel*>(p), b.pool); })))
    return r;
  if ((r = send(M.streams, size_t(d.num_streams) * sizeof(jxlhip::ModStream), [&](void* p) {
         jxlhip::ModStream* s = static_cast<jxlhip::ModStream*>(p);
         upload::BuildModStreams(d, P, s, b);
         M.streams_host.assign(s, s + d.num_streams);
       })))
    return r;
  if (!d.num_streams) M.streams_host.clear();
  PlainUploader up{c};
  upload::VisitSplineTables(*c, d.splines, d.ysize, up);
  upload::VisitPatchTables(*c, d.patches, d.ysize, up);
  return up.r;
}

extern "C" int jxlhip_modular_upload(JxlHipContext* c, const JxlHipModFrameDesc* d) {
  if (!c || !d) return JXLHIP_ERR_INVALID_ARGUMENT;
  // 1. whether the descriptor is taken: decided on the host alone (upload::ModRule), so that a refused one costs no
  // device call and leaves the context's tables as they were (but no frame to run: the caller meant to replace it)
  upload::ModUploadOptions opt;
  opt.keep_xyb = c->keep_xyb;
  int r = upload::CheckModFrameDesc(*d, opt);
  c->mod.have = false;
  c->have_frame = false;
  c->red.have = c->red.ran = false;
  if (!r && c->tensor_bound) {  // (the bound tensor against the image's size, which a transposing orientation turns)
    const bool transposed = (c->out_orient & 4) != 0;
    r = tensor_out::CheckTensorOut(c->tensor, transposed ? d->ysize : d->xsize, transposed ? d->xsize : d->ysize);
  }
  if (!r && c->resized_bound) {
    const bool transposed = (c->out_orient & 4) != 0;
    r = resample::CheckResizedOut(c->resized, transposed ? d->ysize : d->xsize, transposed ? d->xsize : d->ysize);
  }
  if (r) return r;
  const upload::ModPlan P = upload::MakeModPlan(*d, opt);
  // 2. the tables are overwritten on the context's stream, behind whatever still reads the old ones
  HIP_TRY(hipSetDevice(c->device));
  if ((r = ApplyPendingWait(c))) return r;
  if ((r = StageReset(c))) return r;
  // 3. - 5. what the context remembers, the buffers, then the tables, which hold the buffers' addresses
  AdoptModFrame(c, *d, P);
  if ((r = EnsureModBuffers(c, *d, P))) return r;
  if ((r = SendModTables(c, *d, P))) return r;
  // The tables are resident and the descriptor's arrays free when the call returns, as for a VarDCT frame: batch launches
  // over this context run on other contexts' streams, and copies left in flight slow later kernels (jxlhip_frame_upload).
  HIP_TRY(hipEventRecord(c->stage.done, c->stream));
  c->stage.recorded = true;
  HIP_TRY(WaitEvent(c->stage.done));
  if (c->resized_bound && (r = PlaceResampleOfFrame(c))) return r;
  c->mod.have = true;
  c->mod.batch_set.Forget();
  c->generation++;
  return 0;
}

// ---- The parameter blocks of the kernels behind the filters, each stated once: the VarDCT filter stage, the Modular passes
// and the test entries fill them through these. The blocks come zeroed (memset: padding included).
// Three dense or padded planes, `plane_stride` floats apart, and the rows the patch and spline kernels take (a test entry
// builds one from its arguments).
struct PlaneView {
  float* planes;
  uint32_t stride;
  size_t plane_stride;
  uint32_t xsize, y_begin, y_end;
};
static PlaneView FrameView(const JxlHipContext* c) {  // the filtered planes of a VarDCT frame, its band
  return {c->plane[1].as<float>(), c->xp, size_t(c->xp) * c->yp, c->xs, c->band_y0, c->band_y1};
}
static PlaneView ModularView(const JxlHipContext* c) {  // the float planes of a Modular frame
  return {c->spl_planes.as<float>(), c->mod.xs, size_t(c->mod.xs) * c->mod.ys, c->mod.xs, 0, c->mod.ys};
}
// The tables of the patches / splines / noise on the device: a context's (upload) or what a test entry staged.
struct PatchTables {
  const uint32_t *records, *row_start, *row_list;
  const float* const* slot_planes;  // [4], as slot_w, slot_h
  const uint32_t *slot_w, *slot_h;
};
struct PatchAlpha {  // the alpha plane the patches blend into (dense rows), and the reference frames' ([4])
  float* plane;
  size_t stride;
  uint32_t premultiplied;
  const float* const* slot;
};
struct SplineTables {
  const float* segments;
  const uint32_t *row_start, *row_segments;
};
struct NoiseTables {
  float* raw;
  uint32_t seed0, seed1;
  const float* lut;  // [8]
  float ytox, ytob;
};
static PatchTables PatchTablesOf(const JxlHipContext* c) {
  return {c->pat_rec.as<uint32_t>(), c->pat_row_start.as<uint32_t>(), c->pat_row_list.as<uint32_t>(), c->pat_src, c->pat_src_w, c->pat_src_h};
}
static SplineTables SplineTablesOf(const JxlHipContext* c) {
  return {c->spl_seg.as<float>(), c->spl_row_start.as<uint32_t>(), c->spl_row_seg.as<uint32_t>()};
}
static NoiseTables NoiseTablesOf(const JxlHipContext* c) {
  return {c->noise.as<float>(), c->noise_seed[0], c->noise_seed[1], c->noise_lut, c->noise_ytox, c->noise_ytob};
}
// `alpha` NULL: the image has no alpha channel, or the patches leave it alone.
static void FillPatchParams(const PlaneView& v, const PatchTables& t, const PatchAlpha* alpha, jxlhip::PatchParams* pp) {
  pp->planes = v.planes; pp->stride = v.stride; pp->plane_stride = v.plane_stride;
  pp->xsize = v.xsize; pp->y_begin = v.y_begin; pp->y_end = v.y_end;
  pp->records = t.records; pp->row_start = t.row_start; pp->row_list = t.row_list;
  for (int k = 0; k < 4; k++) {
    pp->slot_planes[k] = t.slot_planes[k]; pp->slot_w[k] = t.slot_w[k]; pp->slot_h[k] = t.slot_h[k];
    if (alpha) pp->slot_alpha[k] = alpha->slot[k];
  }
  if (!alpha) return;
  pp->alpha = alpha->plane; pp->alpha_stride = alpha->stride; pp->premultiplied = alpha->premultiplied;
}
static void FillSplineParams(const PlaneView& v, const SplineTables& t, jxlhip::SplineParams* sp) {
  sp->planes = v.planes; sp->stride = v.stride; sp->plane_stride = v.plane_stride;
  sp->xsize = v.xsize; sp->y_begin = v.y_begin; sp->y_end = v.y_end;
  sp->segments = t.segments; sp->row_start = t.row_start; sp->row_segments = t.row_segments;
}
// Three planes [3][yp][xp] of an image of xs x ys, and the rows the noise and colour kernels take.
struct PaddedPlanes {
  float* planes;
  uint32_t xs, ys, xp, yp, y_begin, y_end;
};
static PaddedPlanes FilteredPlanes(const JxlHipContext* c) {  // the frame's resolution (what c->fp describes)
  return {c->plane[1].as<float>(), c->xs, c->ys, c->xp, c->yp, c->band_y0, c->band_y1};
}
static PaddedPlanes UpsampledPlanes(const JxlHipContext* c) {  // the image's resolution, behind the upsampling
  return {c->ups_planes.as<float>(), c->oxs, c->oys, (c->oxs + 7) & ~7u, c->oys, 0, c->oys};
}
// `xgroups`, `ngroups`: the 256 x 256 generator groups across and in all.
static void FillNoiseParams(const PaddedPlanes& v, const NoiseTables& t, uint32_t xgroups, uint32_t ngroups, jxlhip::NoiseParams* np) {
  np->raw = t.raw; np->planes = v.planes;
  np->xsize = v.xs; np->ysize = v.ys; np->xp = v.xp; np->yp = v.yp;
  np->xgroups = xgroups; np->ngroups = ngroups; np->seed[0] = t.seed0; np->seed[1] = t.seed1;
  memcpy(np->lut, t.lut, sizeof(np->lut));
  np->ytox = t.ytox; np->ytob = t.ytob;
  np->y_begin = v.y_begin; np->y_end = v.y_end;
}
// The random planes of every group, then their high-pass onto `rows` rows of `columns` samples.
static void LaunchNoise(const jxlhip::NoiseParams& np, uint32_t columns, uint32_t rows, hipStream_t st) {
  hipLaunchKernelGGL(jxlhip::k_noise_random, dim3((np.ngroups * 8 + 63) / 64), dim3(64), 0, st, np);
  hipLaunchKernelGGL(jxlhip::k_noise_add, dim3((columns + 63) / 64, (rows + 3) / 4), dim3(256), 0, st, np);
}
// The colour stage on `v`: the frame's constants (`fp`) with the geometry of the planes it reads.
static void FillColorOutParams(const jxlhip::FilterParams& fp, const PaddedPlanes& v, const jxlhip::PixelOut& po, const JxlHipColorTarget& t,
                               jxlhip::ColorOutParams* cp) {
  cp->f = fp;  // (the frame's constants)
  cp->f.in = v.planes;
  cp->f.xs = v.xs; cp->f.ys = v.ys; cp->f.xp = v.xp; cp->f.yp = v.yp;
  cp->f.y_begin = v.y_begin; cp->f.y_end = v.y_end;
  cp->po = po; cp->t = t;
}
static void LaunchColorOut(const jxlhip::ColorOutParams& cp, hipStream_t st) {
  hipLaunchKernelGGL(jxlhip::k_color_out, dim3((cp.f.xs + 63) / 64, (cp.f.y_end - cp.f.y_begin + 3) / 4), dim3(256), 0, st, cp);
}

// The parameter blocks of the passes behind the inverse transforms, one fill function per pass (false: the frame does not
// take the pass); they live with the kernels' structs. Frames with patches / splines / kept XYB planes: colour samples to
// float planes (kind 4), the patches (kind 6), then the splines (kind 5) over them (dec_cache.cc:193-201), then the output
// (kind 3) reads them.
static bool ModFloatPlanes(const JxlHipContext* c) { return c->spl_segments || c->keep_xyb || c->pat_positions; }
static bool FillModPlanes(const JxlHipContext* c, jxlhip::ModOutput* o) {
  if (!ModFloatPlanes(c)) return false;
  const JxlHipContext::Modular& M = c->mod;
  for (uint32_t j = 0; j < 3; j++) {
    o->ch[j] = M.pool.as<int32_t>() + M.buf_off[M.out_buffer[j]];
    o->stride[j] = M.xs;
  }
  o->num_color = 3;
  o->bits = M.bits;
  o->w = M.xs;
  o->h = M.ys;
  o->fplanes = c->spl_planes.as<float>();
  o->fmode = 1;
  o->xyb = M.xyb ? 1 : 0;  // (the planes then hold XYB; the final pass converts what it reads back)
  memcpy(o->xyb_factor, M.xyb_factor, sizeof(o->xyb_factor));
  return true;
}
static bool FillModPatches(const JxlHipContext* c, jxlhip::PatchParams* pp) {  // (no alpha: upload refuses patches that use it)
  if (c->pat_positions) FillPatchParams(ModularView(c), PatchTablesOf(c), nullptr, pp);
  return c->pat_positions != 0;
}
static bool FillModSplines(const JxlHipContext* c, jxlhip::SplineParams* sp) {
  if (c->spl_segments) FillSplineParams(ModularView(c), SplineTablesOf(c), sp);
  return c->spl_segments != 0;
}
static bool FillModOutput(const JxlHipContext* c, jxlhip::ModOutput* o) {  // (every frame: a set has at least one, so this launch always exists)
  const JxlHipContext::Modular& M = c->mod;
  if (ModFloatPlanes(c)) {
    o->fplanes = c->spl_planes.as<float>();
    o->fmode = 2;
  }
  o->xyb = M.xyb ? 1 : 0;
  memcpy(o->xyb_factor, M.xyb_factor, sizeof(o->xyb_factor));
  o->color = M.xyb_color;
  o->target = M.xyb_target;
  for (uint32_t j = 0; j < M.num_color + (M.has_alpha ? 1 : 0); j++) {
    o->ch[j] = M.pool.as<int32_t>() + M.buf_off[M.out_buffer[j]];
    o->stride[j] = M.xs;
  }
  o->num_color = M.num_color;
  o->has_alpha = M.has_alpha;
  o->bits = M.bits;
  o->alpha_bits = M.alpha_bits;
  o->w = M.xs;
  o->h = M.ys;
  FillPixelOut(c, M.xs, M.ys, nullptr, &o->po);
  return true;
}
// One pass over the frames of a set that take it: a zeroed block each, one launch. `rows`: one workgroup per row (the
// spline and patch kernels) instead of 256 columns per workgroup.
template <typename Block>
static void ModAppendPass(JxlHipContext* const* ctxs, size_t n, uint32_t kind, bool rows, bool (*fill)(const JxlHipContext*, Block*),
                          std::vector<uint8_t>* blob, std::vector<ModLaunch>* launches) {
  upload::ModBlobAlign(blob);
  ModLaunch L{kind, blob->size(), 0, 0, 0};
  for (size_t i = 0; i < n; i++) {
    Block b;
    memset(&b, 0, sizeof(b));
    if (!fill(ctxs[i], &b)) continue;
    upload::ModBlobAppend(blob, &b, sizeof(b));
    modular_launch::ModPassAdd(&L, rows, ctxs[i]->mod.xs, ctxs[i]->mod.ys);
  }
  if (L.count) launches->push_back(L);
}
// The inverse transforms (upload::BuildModSchedule) and the pixel writer of a set of frames, as launches over
// parameter-block arrays. Built once per set (cached with the stream list), blocks in `blob` (host), launches in `launches`.
static void ModularBuildOps(JxlHipContext* const* ctxs, size_t n, std::vector<uint8_t>* blob, std::vector<ModLaunch>* launches) {
  blob->clear();
  launches->clear();
  std::vector<upload::ModFrameOps> frames(n);
  for (size_t i = 0; i < n; i++) {
    const JxlHipContext::Modular& M = ctxs[i]->mod;
    frames[i] = {uintptr_t(M.pool.p), M.buf_off.data(), M.buf_w.data(), M.ops.data(), M.ops.size()};
  }
  upload::BuildModSchedule(frames.data(), n, blob, launches);
  ModAppendPass(ctxs, n, 4, false, FillModPlanes, blob, launches);
  ModAppendPass(ctxs, n, 6, true, FillModPatches, blob, launches);
  ModAppendPass(ctxs, n, 5, true, FillModSplines, blob, launches);
  ModAppendPass(ctxs, n, 3, false, FillModOutput, blob, launches);
}
// Builds (or re-uses) the description of a set in four steps: key, plan, place, remember. The plan
// (jxh_modular_launch_plan.h) is a function of the set and of JXLHIP_MOD_LANES (measurement aid), so these are the key.
// A changed variable over an unchanged set therefore describes the set anew, its two copies included (it used to change
// the lanes of the next launch without a copy): the price of one key for everything the plan holds.
static int PrepareModBatch(JxlHipContext* c0, JxlHipContext* const* ctxs, size_t n) {
  JxlHipContext::Modular& M0 = c0->mod;
  const int lanes_override = EnvInt("JXLHIP_MOD_LANES", 0);
  if (M0.batch_set.Matches(ctxs, n) && M0.batch_lanes_override == lanes_override) return 0;
  M0.batch_set.Forget();  // (what is on the device is no set's until both copies below have been made)

  std::vector<modular_launch::ModStreamFrame> frames(n);
  for (size_t i = 0; i < n; i++) {
    const JxlHipContext::Modular& M = ctxs[i]->mod;
    frames[i] = {M.streams_host.data(), M.stream_samples.data(), M.streams_host.size(), M.code_table_words.data(), M.code_table_words.size()};
  }
  std::vector<jxlhip::ModStream> flat;
  modular_launch::ModBatchPlan plan = modular_launch::PlanModStreams(frames.data(), n, lanes_override, &flat);
  std::vector<uint8_t> ops_blob;
  std::vector<ModLaunch> launches;
  ModularBuildOps(ctxs, n, &ops_blob, &launches);
  plan.grids = modular_launch::ExpandModLaunches(launches);
  if (EnvInt("JXLHIP_PACK_DEBUG", 0))
    fprintf(stderr, "[modular pack] streams %u lanes %u workgroups %u lds %u tree_cap %u table_cap %u form %s\n", plan.n, plan.lanes, plan.workgroups,
            plan.lds, plan.tree_cap, plan.table_cap, modular_launch::FormName(plan));

  int r;
  if ((r = M0.batch_streams.Ensure(flat.size() * sizeof(jxlhip::ModStream)))) return r;
  HIP_TRY(hipMemcpy(M0.batch_streams.p, flat.data(), flat.size() * sizeof(jxlhip::ModStream), hipMemcpyHostToDevice));
  if ((r = M0.batch_ops.Ensure(ops_blob.size() + 16))) return r;
  if (!ops_blob.empty()) HIP_TRY(hipMemcpy(M0.batch_ops.p, ops_blob.data(), ops_blob.size(), hipMemcpyHostToDevice));

  M0.batch_set.Remember(ctxs, n);
  M0.batch_lanes_override = lanes_override;
  M0.batch_plan = std::move(plan);
  return 0;
}
static int LaunchModStreams(const JxlHipContext* c0) {
  const modular_launch::ModBatchPlan& P = c0->mod.batch_plan;
  if (!P.n) return 0;
  auto kernel = P.wp ? (P.refs ? jxlhip::k_modular_streams<true, true> : jxlhip::k_modular_streams<true, false>)
                     : (P.refs ? jxlhip::k_modular_streams<false, true> : jxlhip::k_modular_streams<false, false>);
  if (P.lds > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(P.lds)));
  hipLaunchKernelGGL(kernel, dim3(P.workgroups), dim3(64), P.lds, c0->stream, c0->mod.batch_streams.as<jxlhip::ModStream>(), P.n, P.lanes,
                     P.tree_cap, P.table_cap);
  HIP_TRY(hipGetLastError());
  return 0;
}
static int ModularLaunchOps(const std::vector<modular_launch::ModGrid>& grids, const uint8_t* dev, hipStream_t st) {
  for (const modular_launch::ModGrid& g : grids) {
    const dim3 grid(g.grid[0], g.grid[1], g.grid[2]), block(g.block);
    const uint8_t* at = dev + g.offset;
    if (g.kind == 0)
      hipLaunchKernelGGL(jxlhip::k_modular_rct, grid, block, 0, st, reinterpret_cast<const jxlhip::ModRct*>(at) + g.first);
    else if (g.kind == 1)
      hipLaunchKernelGGL(jxlhip::k_modular_palette, grid, block, 0, st, reinterpret_cast<const jxlhip::ModPalette*>(at) + g.first);
    else if (g.kind == 2)
      hipLaunchKernelGGL(jxlhip::k_modular_unsqueeze, grid, block, 0, st, reinterpret_cast<const jxlhip::ModUnsqueeze*>(at) + g.first);
    else if (g.kind == 5)
      hipLaunchKernelGGL(jxlhip::k_splines_add_batch, grid, block, 0, st, reinterpret_cast<const jxlhip::SplineParams*>(at) + g.first);
    else if (g.kind == 6)
      hipLaunchKernelGGL(jxlhip::k_patches_add_batch, grid, block, 0, st, reinterpret_cast<const jxlhip::PatchParams*>(at) + g.first);
    else  // (3 the output, 4 the float planes)
      hipLaunchKernelGGL(jxlhip::k_modular_output, grid, block, 0, st, reinterpret_cast<const jxlhip::ModOutput*>(at) + g.first);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

extern "C" int jxlhip_modular_run_batch(JxlHipContext* const* ctxs, size_t n) {
  if (!ctxs || !n) return JXLHIP_ERR_INVALID_ARGUMENT;
  JxlHipContext* c0 = ctxs[0];
  for (size_t i = 0; i < n; i++) {
    if (!ctxs[i] || ctxs[i]->device != c0->device) return JXLHIP_ERR_INVALID_ARGUMENT;
    if (!ctxs[i]->mod.have) return JXLHIP_ERR_NO_FRAME;
    if (OwnPixelBytes(ctxs[i]) > ctxs[i]->rgb.cap) return JXLHIP_ERR_INVALID_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(c0->device));
  int r;
  if (n > 1 && (r = EnsureOwnStream(c0))) return r;
  if ((r = PrepareModBatch(c0, ctxs, n))) return r;
  if ((r = JoinSetOnFirstStream(ctxs, n))) return r;
  if ((r = TensorsBeforeWriters(ctxs, n, c0->stream))) return r;
  HIP_TRY(hipEventRecord(c0->ev[0], c0->stream));
  if ((r = LaunchModStreams(c0))) return r;
  if ((r = ModularLaunchOps(c0->mod.batch_plan.grids, c0->mod.batch_ops.as<uint8_t>(), c0->stream))) return r;
  if ((r = LaunchResample(ctxs, n, c0->stream))) return r;
  HIP_TRY(hipEventRecord(c0->ev[1], c0->stream));
  if ((r = TensorsAfterWriters(ctxs, n, c0->stream))) return r;
  c0->ev_valid[0] = true;  // (the other contexts' ev_valid[0] stay as they are, unlike the reduced batch, which clears them)
  if ((r = PublishBatchDone(ctxs, n))) return r;
  for (size_t i = 0; i < n; i++) ctxs[i]->have_frame = true;  // (the pixel download entry points need it)
  return 0;
}
extern "C" int jxlhip_modular_run(JxlHipContext* c) { return jxlhip_modular_run_batch(&c, 1); }

extern "C" int jxlhip_modular_status(JxlHipContext* c, uint32_t* status, uint32_t* end_bits, size_t n) {
  if (!c || !status) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->mod.have) return JXLHIP_ERR_NO_FRAME;
  if (n < c->mod.nstreams) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  {
    int pw = ApplyPendingWait(c);
    if (pw) return pw;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->mod.nstreams) {
    HIP_TRY(hipMemcpy(status, c->mod.status.p, size_t(c->mod.nstreams) * 4, hipMemcpyDeviceToHost));
    if (end_bits) HIP_TRY(hipMemcpy(end_bits, c->mod.end_bits.p, size_t(c->mod.nstreams) * 4, hipMemcpyDeviceToHost));
  }
  for (uint32_t i = 0; i < c->mod.nstreams; i++)
    if (status[i]) return JXLHIP_ERR_STREAM;
  return 0;
}

extern "C" int jxlhip_modular_download_buffer(JxlHipContext* c, uint32_t buffer, int32_t* dst, size_t n) {
  if (!c || !dst) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->mod.have) return JXLHIP_ERR_NO_FRAME;
  if (buffer >= c->mod.buf_off.size() || n < size_t(c->mod.buf_w[buffer]) * c->mod.buf_h[buffer]) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  {
    int pw = ApplyPendingWait(c);
    if (pw) return pw;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(dst, c->mod.pool.as<int32_t>() + c->mod.buf_off[buffer], size_t(c->mod.buf_w[buffer]) * c->mod.buf_h[buffer] * 4,
                    hipMemcpyDeviceToHost));
  return 0;
}

// ------------------------------------------------------------------------------------- reduced output (jxl_hip_reduced.h)
// The colour stage's and the writer's blocks of a reduced image, as FillFilterParams and FillPixelOut make a frame's.
static void FillReducedDev(const JxlHipContext* c, const JxlHipReducedDesc& d, const reduced::ReducedHead& head, jxlhip::ReducedDev* dev) {
  memset(dev, 0, sizeof(*dev));
  dev->h = head;
  jxlhip::FilterParams& fp = dev->f;
  for (int ch = 0; ch < 3; ch++) {
    fp.opsin_bias[ch] = d.opsin_bias[ch];
    fp.opsin_bias_cbrt[ch] = cbrtf(d.opsin_bias[ch]);
  }
  memcpy(fp.opsin_inv, d.opsin_inv, sizeof(fp.opsin_inv));
  fp.linear_output = d.linear_output;
  FillPixelOut(c, d.xsize_blocks, d.ysize_blocks, nullptr, &dev->po);
  dev->t = d.color_target ? *d.color_target : JxlHipColorTarget{};
}

extern "C" int jxlhip_reduced_upload(JxlHipContext* c, const JxlHipReducedDesc* d) {
  if (!c || !d) return JXLHIP_ERR_INVALID_ARGUMENT;
  // 1. whether the descriptor and the bindings are taken at the reduced size: on the host alone, before any device call
  int r = reduced::CheckReducedDesc(*d);
  if (!r && (OutChannels(c) == 2 || OutChannels(c) == 4)) r = JXLHIP_ERR_UNSUPPORTED;  // (the reduced image is opaque colour)
  const bool transposed = (c->out_orient & 4) != 0;
  const uint32_t w = transposed ? d->ysize_blocks : d->xsize_blocks, h = transposed ? d->xsize_blocks : d->ysize_blocks;
  if (!r && c->tensor_bound) r = tensor_out::CheckTensorOut(c->tensor, w, h);
  if (!r && c->resized_bound) r = resample::CheckResizedOut(c->resized, w, h);
  c->have_frame = false;  // (the caller meant to replace whatever the context held)
  c->mod.have = false;
  c->red.have = c->red.ran = false;
  if (r) return r;
  // 2. the block is overwritten: whatever still reads the old one has to be finished
  HIP_TRY(hipSetDevice(c->device));
  if ((r = ApplyPendingWait(c))) return r;
  if ((r = StageReset(c))) return r;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->stream2) HIP_TRY(hipStreamSynchronize(c->stream2));
  c->xb = d->xsize_blocks; c->yb = d->ysize_blocks;
  c->xs = c->oxs = d->xsize_blocks; c->ys = c->oys = d->ysize_blocks;
  c->ups = 1;
  c->generation++;
  // 3. the buffers the kernel writes, then the block, which holds their addresses: one staged copy
  const reduced::BlockLayout l = reduced::LayoutOf(*d, sizeof(jxlhip::ReducedDev));
  if ((r = c->red_block.Ensure(l.bytes))) return r;
  if (!c->tensor_bound && (r = c->rgb.Ensure(OwnPixelBytes(c)))) return r;
  c->red.dc_kept = c->keep_dc;
  if (c->keep_dc && (r = c->dc.Ensure(l.q_bytes))) return r;
  void* st = nullptr;
  if ((r = StageAlloc(c, l.bytes, &st))) return r;
  reduced::ReducedHead head;
  if ((r = reduced::PlaceBlock(*d, l, c->keep_dc ? c->dc.as<float>() : nullptr, st, uintptr_t(c->red_block.p), &head))) return r;
  FillReducedDev(c, *d, head, &c->red.dev);
  memcpy(static_cast<uint8_t*>(st) + l.desc, &c->red.dev, sizeof(c->red.dev));
  hipStream_t cs = CopyStream(c->device);
  if (!cs) cs = c->stream;
  HIP_TRY(hipMemcpyAsync(c->red_block.p, st, l.bytes, hipMemcpyHostToDevice, cs));
  HIP_TRY(hipEventRecord(c->stage.done, cs));
  c->stage.recorded = true;
  // (resident when the call returns: a batched launch over this context runs on another context's stream)
  HIP_TRY(WaitEvent(c->stage.done));
  if (c->resized_bound && (r = PlaceResampleOfFrame(c))) return r;
  c->red.generation = c->generation;
  c->red.have = true;
  return 0;
}

extern "C" int jxlhip_reduced_run_batch(JxlHipContext* const* ctxs, size_t n) {
  if (!ctxs || !n) return JXLHIP_ERR_INVALID_ARGUMENT;
  JxlHipContext* c0 = ctxs[0];
  for (size_t i = 0; i < n; i++) {
    JxlHipContext* c = ctxs[i];
    if (!c || c->device != c0->device) return JXLHIP_ERR_INVALID_ARGUMENT;
    if (!c->red.have) return c->have_frame || c->mod.have ? JXLHIP_ERR_INVALID_ARGUMENT : JXLHIP_ERR_NO_FRAME;
    if (c->red.generation != c->generation) return JXLHIP_ERR_INVALID_ARGUMENT;  // (output settings changed since the upload)
  }
  HIP_TRY(hipSetDevice(c0->device));
  int r;
  if (n > 1 && (r = EnsureOwnStream(c0))) return r;
  const hipStream_t ls = c0->stream;
  if ((r = JoinSetOnFirstStream(ctxs, n))) return r;
  // One context: its own block begins with the launch's descriptor. Several: their descriptors side by side with running
  // tile origins, on the set's first context, rebuilt only when the set changed.
  const jxlhip::ReducedDev* descs = c0->red_block.as<jxlhip::ReducedDev>();
  uint32_t tiles = c0->red.dev.h.tiles;
  if (n > 1) {
    JxlHipContext::Reduced& R = c0->red;
    if (!R.batch_set.Matches(ctxs, n)) {
      R.batch_set.Forget();
      const size_t bytes = reduced::BatchBytes(n, sizeof(jxlhip::ReducedDev));
      if ((r = c0->red_batch.Ensure(bytes))) return r;
      std::vector<const void*> each(n);
      for (size_t i = 0; i < n; i++) each[i] = &ctxs[i]->red.dev;
      // (on the launch stream itself: behind an earlier launch that still reads the array, and without a host wait)
      void* st = nullptr;
      if ((r = StageReset(c0)) || (r = StageAlloc(c0, bytes, &st))) return r;
      if ((r = reduced::PlaceBatch(each.data(), n, sizeof(jxlhip::ReducedDev), st, bytes, &R.batch_tiles))) return r;
      HIP_TRY(hipMemcpyAsync(c0->red_batch.p, st, bytes, hipMemcpyHostToDevice, ls));
      HIP_TRY(hipEventRecord(c0->stage.done, ls));
      c0->stage.recorded = true;
      R.batch_set.Remember(ctxs, n);
    }
    descs = c0->red_batch.as<jxlhip::ReducedDev>();
    tiles = R.batch_tiles;
  }
  if ((r = TensorsBeforeWriters(ctxs, n, ls))) return r;
  HIP_TRY(hipEventRecord(c0->ev[0], ls));
  hipLaunchKernelGGL(jxlhip::k_reduced_pixels, dim3(tiles), dim3(256), 0, ls, descs, uint32_t(n));
  HIP_TRY(hipGetLastError());
  if ((r = LaunchResample(ctxs, n, ls))) return r;
  HIP_TRY(hipEventRecord(c0->ev[1], ls));
  if ((r = TensorsAfterWriters(ctxs, n, ls))) return r;
  c0->ev_valid[0] = true;
  for (size_t i = 1; i < n; i++) ctxs[i]->ev_valid[0] = false;  // (the Modular batch leaves them as they are)
  if ((r = PublishBatchDone(ctxs, n))) return r;
  for (size_t i = 0; i < n; i++) ctxs[i]->red.ran = true;  // (the pixel download entry points need it)
  return 0;
}
extern "C" int jxlhip_reduced_run(JxlHipContext* c) { return jxlhip_reduced_run_batch(&c, 1); }

// ------------------------------------------------------------------------------- DC image of a window (jxl_hip_dc_window.h)
// The descriptor is checked on the host; then the apron and the precision bytes leave in one staged copy on the copy
// stream, the kernel follows them there, and the call waits for both (the planes are read by launches on other streams).
extern "C" int jxlhip_dc_window(JxlHipContext* c, const JxlHipDcWindow* d) {
  namespace window = jxlhip::window;
  if (!c || !d) return JXLHIP_ERR_INVALID_ARGUMENT;
  int r = window::CheckDcWindow(*d);
  if (r) return r;
  // whatever still reads the planes of an earlier window (a transform launch) has to be finished
  HIP_TRY(hipSetDevice(c->device));
  if ((r = ApplyPendingWait(c))) return r;
  if ((r = StageReset(c))) return r;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->stream2) HIP_TRY(hipStreamSynchronize(c->stream2));
  const size_t q_bytes = size_t(d->apron_xsize) * d->apron_ysize * 12;
  const size_t ep_bytes = d->dc_extra_precision ? size_t(d->num_dc_groups) : 0;
  const size_t out_bytes = size_t(d->win_xsize) * d->win_ysize * 12;
  if ((r = c->dcw_in.Ensure(q_bytes + ep_bytes))) return r;
  if ((r = c->dcw_out.Ensure(out_bytes))) return r;
  void* st = nullptr;
  if ((r = StageAlloc(c, q_bytes + ep_bytes, &st))) return r;
  memcpy(st, d->apron, q_bytes);
  if (ep_bytes) memcpy(static_cast<uint8_t*>(st) + q_bytes, d->dc_extra_precision, ep_bytes);
  jxlhip::DcWindowParams P;
  memset(&P, 0, sizeof(P));
  P.q = c->dcw_in.as<int32_t>();
  P.ep = ep_bytes ? c->dcw_in.as<uint8_t>() + q_bytes : nullptr;
  P.out = c->dcw_out.as<float>();
  P.ax0 = int(d->apron_x0); P.ay0 = int(d->apron_y0); P.axs = int(d->apron_xsize); P.ays = int(d->apron_ysize);
  P.wx0 = int(d->win_x0); P.wy0 = int(d->win_y0); P.wxs = int(d->win_xsize); P.wys = int(d->win_ysize);
  P.fxs = int(d->frame_xsize_blocks); P.fys = int(d->frame_ysize_blocks);
  P.xgroups = (d->frame_xsize_blocks + window::kDcGroupBlocks - 1) / window::kDcGroupBlocks;
  P.smoothing = d->dc_smoothing ? 1 : 0;
  for (int ch = 0; ch < 3; ch++) P.step[ch] = d->dc_step[ch];
  P.cfl_x = d->dc_cfl_x;
  P.cfl_b = d->dc_cfl_b;
  hipStream_t cs = CopyStream(c->device);
  if (!cs) cs = c->stream;
  HIP_TRY(hipMemcpyAsync(c->dcw_in.p, st, q_bytes + ep_bytes, hipMemcpyHostToDevice, cs));
  hipLaunchKernelGGL(jxlhip::k_dc_window, dim3(window::TilesX(d->win_xsize), window::TilesY(d->win_ysize)), dim3(256), 0, cs, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->stage.done, cs));
  c->stage.recorded = true;
  HIP_TRY(WaitEvent(c->stage.done));
  return 0;
}
extern "C" const float* jxlhip_dc_window_planes(JxlHipContext* c) { return c ? c->dcw_out.as<float>() : nullptr; }
extern "C" int jxlhip_debug_dc_window(JxlHipContext* c, const JxlHipDcWindow* d, float* host_out) {
  if (!c || !d || !host_out) return JXLHIP_ERR_INVALID_ARGUMENT;
  int r = jxlhip::window::CheckDcWindow(*d);
  if (r) return r;
  // the output buffer with a kilobyte of room behind the planes, all of it filled with a sentinel first
  constexpr size_t kTail = 1024;
  constexpr int kSentinel = 0x7B;
  const size_t out_bytes = size_t(d->win_xsize) * d->win_ysize * 12;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if ((r = c->dcw_out.Ensure(out_bytes + kTail))) return r;
  HIP_TRY(hipMemset(c->dcw_out.p, kSentinel, out_bytes + kTail));
  HIP_TRY(hipDeviceSynchronize());
  if ((r = jxlhip_dc_window(c, d))) return r;
  uint8_t tail[kTail];
  HIP_TRY(hipMemcpy(host_out, c->dcw_out.p, out_bytes, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(tail, c->dcw_out.as<uint8_t>() + out_bytes, kTail, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < kTail; i++)
    if (tail[i] != kSentinel) return JXLHIP_ERR_GUARD;
  return 0;
}

extern "C" {

int jxlhip_run_transform_batch(JxlHipContext* const* ctxs, size_t n) {
  int r = BeginDownstreamBatch(ctxs, n);
  if (r) return r;
  JxlHipContext* c0 = ctxs[0];
  HIP_TRY(hipEventRecord(c0->ev[2], c0->stream));
  r = c0->coef_bits == 16 ? LaunchTransforms<int16_t>(c0) : LaunchTransforms<int32_t>(c0);
  if (r) return r;
  HIP_TRY(hipEventRecord(c0->ev[3], c0->stream));
  c0->ev_valid[1] = true;
  for (size_t i = 1; i < n; i++) ctxs[i]->ev_valid[1] = false;
  return EndDownstreamBatch(ctxs, n);
}

// ---- The steps of jxlhip_run_filter_color_batch behind the filters, each over the frames in the order given, on `ls`.
// The patches, onto the filtered planes; where they blend the alpha channel, into a copy of the frame's alpha plane.
static int LaunchPatches(JxlHipContext* const* ctxs, size_t n, hipStream_t ls) {
  for (size_t i = 0; i < n; i++) {
    JxlHipContext* c = ctxs[i];
    c->alpha_patched_valid = false;
    if (!c->pat_positions) continue;
    PatchAlpha alpha = {};
    if (c->pat_uses_alpha) {  // the frame's alpha plane must be there by now (jxlhip_set_alpha); blended into a copy of it
      const size_t bytes = size_t(c->xs) * c->ys * 4;
      if (!c->have_alpha || c->alpha.cap < bytes) return JXLHIP_ERR_INVALID_ARGUMENT;
      int ar = c->alpha_patched.Ensure(bytes);
      if (ar) return ar;
      HIP_TRY(hipMemcpyAsync(c->alpha_patched.p, c->alpha.p, bytes, hipMemcpyDeviceToDevice, ls));
      alpha = {c->alpha_patched.as<float>(), c->xs, c->pat_premultiplied ? 1u : 0u, c->pat_src_alpha};
      c->alpha_patched_valid = true;
    }
    jxlhip::PatchParams pp;
    memset(&pp, 0, sizeof(pp));
    FillPatchParams(FrameView(c), PatchTablesOf(c), c->pat_uses_alpha ? &alpha : nullptr, &pp);
    hipLaunchKernelGGL(jxlhip::k_patches_add, dim3(c->band_y1 - c->band_y0), dim3(256), 0, ls, pp);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}
static int LaunchSplines(JxlHipContext* const* ctxs, size_t n, hipStream_t ls) {
  for (size_t i = 0; i < n; i++) {
    const JxlHipContext* c = ctxs[i];
    if (!c->spl_segments) continue;
    jxlhip::SplineParams sp;
    memset(&sp, 0, sizeof(sp));
    FillSplineParams(FrameView(c), SplineTablesOf(c), &sp);
    hipLaunchKernelGGL(jxlhip::k_splines_add, dim3(c->band_y1 - c->band_y0), dim3(256), 0, ls, sp);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}
// Noise onto the filtered planes of the frames coded at the image's resolution (upsampled frames: LaunchUpsampledWriter).
static int LaunchFrameNoise(JxlHipContext* const* ctxs, size_t n, hipStream_t ls) {
  for (size_t i = 0; i < n; i++) {
    const JxlHipContext* c = ctxs[i];
    if (!c->has_noise || c->ups != 1) continue;
    jxlhip::NoiseParams np;
    memset(&np, 0, sizeof(np));
    FillNoiseParams(FilteredPlanes(c), NoiseTablesOf(c), c->xg, c->ng, &np);
    LaunchNoise(np, c->xs, c->band_y1 - c->band_y0, ls);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}
// An upsampled frame: straight to pixels, or (noise, kept planes) to planes at the image's resolution, the noise onto
// them, then the colour stage.
static int LaunchUpsampledWriter(const JxlHipContext* c, const jxlhip::PixelOut& po, hipStream_t ls) {
  const bool to_planes = c->has_noise || c->ups_kept;
  const PaddedPlanes big = UpsampledPlanes(c);
  jxlhip::UpsampleParams up;
  up.f = c->fp;
  up.f.in = c->plane[1].as<float>();
  up.f.rgb = c->rgb.as<uint8_t>();
  up.kernel = c->ups_kernel.as<float>();
  up.n = c->ups;
  up.oxs = c->oxs;
  up.oys = c->oys;
  up.po = po;
  up.xyb_out = to_planes ? big.planes : nullptr;
  up.oxp = to_planes ? big.xp : 0;
  up.t = c->ct;
  hipLaunchKernelGGL(jxlhip::k_upsample_color, dim3((c->xs + 63) / 64, (c->ys + 3) / 4), dim3(256), 0, ls, up);
  HIP_TRY(hipGetLastError());
  if (c->has_noise) {
    jxlhip::NoiseParams np;
    memset(&np, 0, sizeof(np));
    const uint32_t xgroups = (c->oxs + 255) / 256;
    FillNoiseParams(big, NoiseTablesOf(c), xgroups, xgroups * ((c->oys + 255) / 256), &np);
    LaunchNoise(np, c->oxs, c->oys, ls);
  }
  if (to_planes) {
    jxlhip::ColorOutParams cp;
    FillColorOutParams(c->fp, big, po, c->ct, &cp);
    LaunchColorOut(cp, ls);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}
// The frames whose pixels the filter kernel did not write: the colour stage, or the upsampling in front of it.
static int LaunchPixelWriters(JxlHipContext* const* ctxs, size_t n, hipStream_t ls) {
  for (size_t i = 0; i < n; i++) {
    const JxlHipContext* c = ctxs[i];
    if (c->ups == 1 && !c->color_out) continue;
    jxlhip::PixelOut po;
    memset(&po, 0, sizeof(po));
    if (c->color_out)
      FillPixelOut(c, c->oxs, c->oys, c->have_alpha ? (c->alpha_patched_valid ? c->alpha_patched.as<float>() : c->alpha.as<float>()) : nullptr, &po);
    if (c->ups != 1) {
      const int r = LaunchUpsampledWriter(c, po, ls);
      if (r) return r;
      continue;
    }
    jxlhip::ColorOutParams cp;
    FillColorOutParams(c->fp, FilteredPlanes(c), po, c->ct, &cp);
    LaunchColorOut(cp, ls);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

int jxlhip_run_filter_color_batch(JxlHipContext* const* ctxs, size_t n) {
  int r = BeginDownstreamBatch(ctxs, n, true);
  if (r) return r;
  JxlHipContext* c0 = ctxs[0];
  const hipStream_t ls = c0->fstream;
  if ((r = TensorsBeforeWriters(ctxs, n, ls))) return r;
  HIP_TRY(hipEventRecord(c0->ev[4], ls));
  if ((r = LaunchFilterGroups(c0))) return r;
  if ((r = LaunchPatches(ctxs, n, ls))) return r;
  if ((r = LaunchSplines(ctxs, n, ls))) return r;
  if ((r = LaunchFrameNoise(ctxs, n, ls))) return r;
  if ((r = LaunchPixelWriters(ctxs, n, ls))) return r;
  if ((r = LaunchResample(ctxs, n, ls))) return r;
  HIP_TRY(hipEventRecord(c0->ev[5], ls));
  if ((r = TensorsAfterWriters(ctxs, n, ls))) return r;
  c0->ev_valid[2] = true;
  for (size_t i = 0; i < n; i++) ctxs[i]->final_plane = 1;
  for (size_t i = 1; i < n; i++) ctxs[i]->ev_valid[2] = false;
  return EndDownstreamBatch(ctxs, n, true);
}

int jxlhip_run_transform(JxlHipContext* c) { return jxlhip_run_transform_batch(&c, 1); }
int jxlhip_run_filter_color(JxlHipContext* c) { return jxlhip_run_filter_color_batch(&c, 1); }

int jxlhip_share_planes(JxlHipContext* c, JxlHipContext* lender) {
  if (!c || c == lender || (lender && (lender->plane_lender || lender->device != c->device))) return JXLHIP_ERR_INVALID_ARGUMENT;
  c->plane_lender = lender;
  if (lender && !lender->planes_event) {  // marks the lender as shared from now on (its launches record the event)
    HIP_TRY(hipSetDevice(lender->device));
    if (!lender->down_done) HIP_TRY(hipEventCreateWithFlags(&lender->down_done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(lender->down_done, lender->stream));
    lender->planes_event = lender->down_done;
    lender->planes_stream = lender->stream;
  }
  c->generation++;  // cached batch descriptions hold plane pointers
  return 0;
}

// ---- halo exchange between the bands of one frame: the filters of a band read up to `rows` rows of the
// inverse-transform output above and below it; with "band_halo" those rows are not decoded a second time but copied from
// the neighbouring band's planes (another context: another GPU's, through any device-to-device transport).
int jxlhip_halo_rows(JxlHipContext* c, uint32_t* rows) {
  if (!c || !rows) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->red.have) return JXLHIP_ERR_UNSUPPORTED;
  if (!c->have_frame) return JXLHIP_ERR_NO_FRAME;
  *rows = uint32_t(jxlhip::FusedHalo(c->gab != 0, int(c->epf_iters)));
  return 0;
}
namespace {
// rows [y0, y0 + rows) of the three planes <-> a dense [3][rows][xp] f32 block, enqueued on `st`
int HaloCopy(JxlHipContext* c, uint32_t y0, uint32_t rows, void* block, bool to_block, hipStream_t st) {
  const size_t row_bytes = size_t(c->xp) * 4, plane = size_t(c->xp) * c->yp;
  float* planes = PlaneHolder(c)->plane[0].as<float>();
  for (int ch = 0; ch < 3; ch++) {
    float* in_plane = planes + ch * plane + size_t(y0) * c->xp;
    float* in_block = static_cast<float*>(block) + size_t(ch) * rows * c->xp;
    HIP_TRY(hipMemcpyAsync(to_block ? in_block : in_plane, to_block ? in_plane : in_block, row_bytes * rows, hipMemcpyDeviceToDevice, st));
  }
  return 0;
}
int HaloCheck(JxlHipContext* c, int side, const void* p, size_t bytes, bool pack, uint32_t* rows) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  int r = jxlhip_halo_rows(c, rows);
  if (r) return r;
  if (!p || (side != 0 && side != 1) || bytes < size_t(3) * *rows * c->xp * 4) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (pack ? c->band_y1 - c->band_y0 < *rows : (side == 0 ? c->band_y0 < *rows : c->band_y1 + *rows > c->ys)) return JXLHIP_ERR_INVALID_ARGUMENT;
  return 0;
}
// the stream on which the halo copies of a frame set led by c0 run: the one its batched transform launch ran on
hipStream_t HaloStream(JxlHipContext* c0) { return c0->stream; }
}  // namespace
// side 0: the first rows of this band (what the band ABOVE needs), side 1: its last rows (what the band BELOW needs);
// `dst` = device memory of at least 3 * rows * xp floats. Runs behind the context's transform; complete on return.
int jxlhip_halo_pack(JxlHipContext* c, int side, void* dst, size_t dst_bytes) {
  uint32_t rows = 0;
  int r = HaloCheck(c, side, dst, dst_bytes, true, &rows);
  if (r) return r;
  HIP_TRY(hipSetDevice(c->device));
  if (!rows) return 0;
  if ((r = ApplyPendingWait(c))) return r;  // (behind the batched transform launch that produced the planes)
  if ((r = HaloCopy(c, side == 0 ? c->band_y0 : c->band_y1 - rows, rows, dst, true, c->stream))) return r;
  HIP_TRY(hipStreamSynchronize(c->stream));  // the block is handed to a transport this library knows nothing about
  return 0;
}
// side 0: the rows just above this band (the band above packed them with side 1), side 1: the rows just below it.
int jxlhip_halo_unpack(JxlHipContext* c, int side, const void* src, size_t src_bytes) {
  uint32_t rows = 0;
  int r = HaloCheck(c, side, src, src_bytes, false, &rows);
  if (r) return r;
  HIP_TRY(hipSetDevice(c->device));
  if (!rows) return 0;
  if ((r = ApplyPendingWait(c))) return r;
  if ((r = HaloCopy(c, side == 0 ? c->band_y0 - rows : c->band_y1, rows, const_cast<void*>(src), false, c->stream))) return r;
  HIP_TRY(hipStreamSynchronize(c->stream));  // the planes go to a filter launch on another stream
  return 0;
}
// The set forms: every frame of a set (the contexts of one batched transform launch, same order) in one call, block i at
// `dst + i * block_bytes`, ordered against the TRANSPORT's stream by events instead of host synchronisation.
int jxlhip_halo_pack_batch(JxlHipContext* const* ctxs, size_t n, int side, void* dst, size_t block_bytes, void* transport_stream) {
  if (!ctxs || !n || !ctxs[0]) return JXLHIP_ERR_INVALID_ARGUMENT;
  JxlHipContext* c0 = ctxs[0];
  HIP_TRY(hipSetDevice(c0->device));
  hipStream_t st = HaloStream(c0);
  uint32_t rows = 0;
  for (size_t i = 0; i < n; i++) {
    int r = HaloCheck(ctxs[i], side, dst, block_bytes, true, &rows);
    if (r) return r;
    if (ctxs[i]->device != c0->device) return JXLHIP_ERR_INVALID_ARGUMENT;
    if (!rows) continue;
    // (the set's transform launch ran on this very stream: a frame's `pending_wait`, which names that launch, stays for its filter stage)
    if ((r = HaloCopy(ctxs[i], side == 0 ? ctxs[i]->band_y0 : ctxs[i]->band_y1 - rows, rows, static_cast<uint8_t*>(dst) + i * block_bytes, true, st))) return r;
  }
  if (!c0->halo_event) HIP_TRY(hipEventCreateWithFlags(&c0->halo_event, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(c0->halo_event, st));
  HIP_TRY(hipStreamWaitEvent(static_cast<hipStream_t>(transport_stream), c0->halo_event, 0));  // the transport reads the blocks after the copies
  return 0;
}
int jxlhip_halo_unpack_batch(JxlHipContext* const* ctxs, size_t n, int side, const void* src, size_t block_bytes, void* transport_stream) {
  if (!ctxs || !n || !ctxs[0]) return JXLHIP_ERR_INVALID_ARGUMENT;
  JxlHipContext* c0 = ctxs[0];
  HIP_TRY(hipSetDevice(c0->device));
  hipStream_t st = HaloStream(c0);
  // the copies read the blocks after whatever the transport's stream holds NOW (the receive the caller enqueued there)
  if (!c0->halo_event) HIP_TRY(hipEventCreateWithFlags(&c0->halo_event, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(c0->halo_event, static_cast<hipStream_t>(transport_stream)));
  HIP_TRY(hipStreamWaitEvent(st, c0->halo_event, 0));
  uint32_t rows = 0;
  for (size_t i = 0; i < n; i++) {
    int r = HaloCheck(ctxs[i], side, src, block_bytes, false, &rows);
    if (r) return r;
    if (ctxs[i]->device != c0->device) return JXLHIP_ERR_INVALID_ARGUMENT;
    if (!rows) continue;
    if ((r = HaloCopy(ctxs[i], side == 0 ? ctxs[i]->band_y0 - rows : ctxs[i]->band_y1, rows,
                      const_cast<uint8_t*>(static_cast<const uint8_t*>(src)) + i * block_bytes, false, st)))
      return r;
  }
  // the set's filter launch follows the copies: on this stream by stream order; on the second stream (option
  // "filter_async") it waits for `transform_done`, which is moved behind the copies here. The transport's stream must not
  // recycle the blocks before the copies have read them either.
  if (c0->filter_async && c0->transform_done_valid) HIP_TRY(hipEventRecord(c0->transform_done, st));
  HIP_TRY(hipEventRecord(c0->halo_event, st));
  HIP_TRY(hipStreamWaitEvent(static_cast<hipStream_t>(transport_stream), c0->halo_event, 0));
  return 0;
}

int jxlhip_set_option(JxlHipContext* c, const char* name, int value) {
  if (!c || !name) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (std::string(name) == "keep_filtered") {
    c->keep_filtered = value != 0;
    return 0;
  }
  if (std::string(name) == "keep_upsampled") {  // (takes effect at the next upload)
    c->keep_upsampled = value != 0;
    return 0;
  }
  if (std::string(name) == "transform_dense") {  // (takes effect at the next upload)
    c->transform_dense = value != 0;
    return 0;
  }
  if (std::string(name) == "band_halo") {  // (takes effect at the next upload of a band)
    c->band_halo = value != 0;
    return 0;
  }
  if (std::string(name) == "filter_async") {
    c->filter_async = value != 0;
    return 0;
  }
  if (std::string(name) == "entropy_gate") {
    // Set on the FIRST context of a frame set by callers that keep several batched launches in flight (bench.py's
    // pipeline): the set's batched entropy launches then count their workgroups in, and batched transform / filter
    // launches enqueued after one wait (a device-side wait packet) until it is resident: see EntropyGate. Off by default:
    // the wait has no bound, so it is only for callers that know every launch they enqueue can start.
    c->entropy_gate = value != 0;
    return 0;
  }
  if (std::string(name) == "keep_dc") {  // (takes effect at the next reduced upload)
    c->keep_dc = value != 0;
    return 0;
  }
  if (std::string(name) == "keep_xyb_planes") {  // (takes effect at the next Modular upload)
    c->keep_xyb = value != 0;
    c->generation++;
    return 0;
  }
  if (std::string(name) == "blocking_sync") {
    // Host threads waiting for the device in this library's calls poll and sleep instead of spinning inside the runtime
    // (the whole process, not only this context): for hosts that pipeline many frames over more threads than they have
    // CPUs to spare.
    g_yield_waits.store(value != 0);
    return 0;
  }
  return JXLHIP_ERR_INVALID_ARGUMENT;
}

int jxlhip_set_output_format(JxlHipContext* c, uint32_t data_type, uint32_t num_channels, uint32_t bits_per_sample, int big_endian) {
  if (!c || num_channels < 1 || num_channels > 4) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (data_type != 0 && data_type != 2 && data_type != 3 && data_type != 5) return JXLHIP_ERR_INVALID_ARGUMENT;
  const uint32_t max_bits = data_type == 2 ? 8 : 16;
  if (bits_per_sample == 0) bits_per_sample = max_bits;
  if ((data_type == 2 || data_type == 3) && bits_per_sample > max_bits) return JXLHIP_ERR_INVALID_ARGUMENT;
  c->out_type = data_type;
  c->out_nc = num_channels;
  c->out_bits = bits_per_sample;
  c->out_swap = big_endian && data_type != 2 ? 1 : 0;
  c->generation++;  // cached batch descriptions hold the pixel pointers
  return 0;
}

int jxlhip_set_output_tensor(JxlHipContext* c, const JxlHipTensorOut* t) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (t) {  // what can be said without an image (one pixel); the upload checks again at the image's size
    const int r = tensor_out::CheckTensorOut(*t, 1, 1);
    if (r) return r;
    c->tensor = *t;
  } else {
    c->tensor = JxlHipTensorOut{};
  }
  c->tensor_bound = t != nullptr;
  c->tensor_fused = false;
  c->resized_bound = false;  // (one destination at a time)
  c->resized = JxlHipResizedOut{};
  c->have_frame = false;  // (a frame uploaded for the other destination has no writer for this one: upload again)
  c->mod.have = false;
  c->red.have = c->red.ran = false;
  c->generation++;  // cached batch descriptions hold the pixel pointers
  return 0;
}

int jxlhip_set_output_resized(JxlHipContext* c, const JxlHipResizedOut* d) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (d) {  // what can be said without an image (any box that fits 32 bits is inside); the upload checks again
    const int r = resample::CheckResizedOut(*d, resample::kAnyImageExtent, resample::kAnyImageExtent);
    if (r) return r;
    c->resized = *d;
  } else {
    c->resized = JxlHipResizedOut{};
  }
  c->resized_bound = d != nullptr;
  c->tensor_bound = c->tensor_fused = false;  // (one destination at a time)
  c->tensor = JxlHipTensorOut{};
  c->have_frame = false;  // (a frame uploaded for another destination has neither the pixel buffer nor the tables: upload again)
  c->mod.have = false;
  c->red.have = c->red.ran = false;
  c->generation++;
  return 0;
}

int jxlhip_debug_resample(JxlHipContext* c, const float* src, uint32_t xsize, uint32_t ysize, uint32_t nc, const JxlHipResizedOut* d) {
  if (!c || !src || !d) return JXLHIP_ERR_INVALID_ARGUMENT;
  int r = resample::CheckResizedOut(*d, xsize, ysize);
  if (r) return r;
  if (nc != d->tensor.num_channels || uint64_t(xsize) * ysize * nc > (uint64_t(1) << 26)) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  if ((r = ApplyPendingWait(c))) return r;
  HIP_TRY(hipStreamSynchronize(c->stream));  // (whatever still reads the context's block or its source)
  if (c->resized_bound) c->have_frame = c->mod.have = c->red.have = c->red.ran = false;  // (an uploaded frame's tables are overwritten: upload again)
  const size_t bytes = size_t(xsize) * ysize * nc * 4;
  if ((r = c->rs_src.Ensure(bytes))) return r;
  HIP_TRY(hipMemcpy(c->rs_src.p, src, bytes, hipMemcpyHostToDevice));
  if ((r = PlaceResample(c, *d, xsize, ysize, c->rs_src.as<float>()))) return r;
  const hipStream_t cs = static_cast<hipStream_t>(d->tensor.consumer_stream);
  if (!c->tensor_event) HIP_TRY(hipEventCreateWithFlags(&c->tensor_event, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(c->tensor_event, cs));
  HIP_TRY(hipStreamWaitEvent(c->stream, c->tensor_event, 0));
  if ((r = LaunchResamplePasses(c->rs_block.as<resample::ResampleDev>(), 1, c->rs_dev.v_tiles, c->rs_dev.h_tiles, c->stream))) return r;
  HIP_TRY(hipEventRecord(c->tensor_event, c->stream));
  HIP_TRY(hipStreamWaitEvent(cs, c->tensor_event, 0));
  HIP_TRY(WaitStream(c->stream));
  return 0;
}

int jxlhip_set_output_orientation(JxlHipContext* c, uint32_t orientation) {
  if (!c || orientation < 1 || orientation > 8) return JXLHIP_ERR_INVALID_ARGUMENT;
  // EXIF numbering -> mirror x (1) | mirror y (2) | transpose (4): stage_write.cc:441-458
  c->out_orient = jxlhip::window::OrientBits(orientation);
  c->generation++;
  return 0;
}

int jxlhip_set_output_unpremultiply(JxlHipContext* c, int on) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  c->out_unpremul = on != 0;
  c->generation++;
  return 0;
}

int jxlhip_set_alpha(JxlHipContext* c, const float* alpha, uint32_t xsize, uint32_t ysize) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  c->alpha_patched_valid = false;
  if (!alpha) {
    c->have_alpha = false;
    return 0;
  }
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = size_t(xsize) * ysize * 4;
  int r = c->alpha.Ensure(bytes);
  if (r) return r;
  HIP_TRY(hipMemcpy(c->alpha.p, alpha, bytes, hipMemcpyHostToDevice));
  c->have_alpha = true;
  return 0;
}

int jxlhip_download_alpha(JxlHipContext* c, float* dst) {
  if (!c || !dst) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->have_alpha) return JXLHIP_ERR_NO_FRAME;
  HIP_TRY(hipSetDevice(c->device));
  {
    int pw = ApplyPendingWait(c);
    if (pw) return pw;
  }
  const Buf& a = c->alpha_patched_valid ? c->alpha_patched : c->alpha;
  HIP_TRY(hipMemcpyAsync(dst, a.p, size_t(c->oxs) * c->oys * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int jxlhip_upsample_plane(JxlHipContext* c, const float* plane, uint32_t xsize, uint32_t ysize, uint32_t factor, const float* kernels,
                          uint32_t out_xsize, uint32_t out_ysize, int as_alpha, float* host_out) {
  if (!c || !plane || !kernels || !xsize || !ysize || (factor != 2 && factor != 4 && factor != 8)) return JXLHIP_ERR_INVALID_ARGUMENT;
  if ((uint64_t(out_xsize) + factor - 1) / factor != xsize || (uint64_t(out_ysize) + factor - 1) / factor != ysize || !out_xsize || !out_ysize)
    return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  {
    int pw = ApplyPendingWait(c);
    if (pw) return pw;
  }
  const size_t in_bytes = size_t(xsize) * ysize * 4, k_bytes = size_t(factor) * factor * 25 * 4, out_bytes = size_t(out_xsize) * out_ysize * 4;
  int r;
  // (the staging buffer: the coded plane, then the kernels; the result goes to the alpha plane or behind them)
  const size_t k_at = (in_bytes + 255) & ~size_t(255), out_at = (k_at + k_bytes + 255) & ~size_t(255);
  if ((r = c->ec_stage.Ensure(out_at + (as_alpha ? 0 : out_bytes)))) return r;
  if (as_alpha && (r = c->alpha.Ensure(out_bytes))) return r;
  uint8_t* base = static_cast<uint8_t*>(c->ec_stage.p);
  HIP_TRY(hipMemcpyAsync(base, plane, in_bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(base + k_at, kernels, k_bytes, hipMemcpyHostToDevice, c->stream));
  jxlhip::UpsamplePlaneParams up;
  up.in = reinterpret_cast<const float*>(base);
  up.kernel = reinterpret_cast<const float*>(base + k_at);
  up.out = as_alpha ? c->alpha.as<float>() : reinterpret_cast<float*>(base + out_at);
  up.xs = xsize;
  up.ys = ysize;
  up.n = factor;
  up.oxs = out_xsize;
  up.oys = out_ysize;
  hipLaunchKernelGGL(jxlhip::k_upsample_plane, dim3((xsize + 63) / 64, (ysize + 3) / 4), dim3(256), 0, c->stream, up);
  HIP_TRY(hipGetLastError());
  if (host_out) HIP_TRY(hipMemcpyAsync(host_out, up.out, out_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // (the host buffers are the caller's; pageable copies are staged by the runtime)
  if (as_alpha) c->have_alpha = true;
  return 0;
}

int jxlhip_download_pixels(JxlHipContext* c, void* dst, size_t stride) {
  if (!c || !dst || CallerOwnsPixels(c)) return JXLHIP_ERR_INVALID_ARGUMENT;  // (a bound tensor holds the pixels, not the context)
  if (!c->have_frame && !c->red.ran) return JXLHIP_ERR_NO_FRAME;  // (a reduced upload that has run: the reduced image)
  const bool transposed = (c->out_orient & 4) != 0;  // rows of the output are columns of the image
  const size_t row = size_t(transposed ? c->oys : c->oxs) * OutPixelBytes(c), rows = transposed ? c->oxs : c->oys;
  if (stride < row) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  {
    int pw = ApplyPendingWait(c);
    if (pw) return pw;
  }
  HIP_TRY(hipMemcpy2DAsync(dst, stride, c->rgb.p, row, row, rows, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int jxlhip_run_all(JxlHipContext* c) {
  int r = jxlhip_run_entropy(c);
  if (!r) r = jxlhip_run_transform(c);
  if (!r) r = jxlhip_run_filter_color(c);
  return r;
}

// The colour stage alone (k_color_out: XYB -> linear RGB -> transfer function) on `n` caller-supplied XYB triples, planar
// [3][n], with the opsin biases of the frame the context last uploaded; f32 RGB out, interleaved. t == NULL: the frame's
// own matrix and linear_output; else t's matrix and the generic writer's colour target.
static int DebugColor(JxlHipContext* c, const float* xyb, size_t n, int linear_output, const JxlHipColorTarget* t, float* rgb) {
  if (!c || !xyb || !rgb || !n || n > (1u << 24)) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (t && (t->tf > JXLHIP_TF_GAMMA || t->tone > JXLHIP_TONE_HLG_OOTF)) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->have_frame) return JXLHIP_ERR_NO_FRAME;
  HIP_TRY(hipSetDevice(c->device));
  Buf in, out;
  int r;
  if ((r = in.Ensure(n * 12)) || (r = out.Ensure(n * 12))) {
    in.Free();
    out.Free();
    return r;
  }
  hipError_t e = hipMemcpy(in.p, xyb, n * 12, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    jxlhip::PixelOut po;
    memset(&po, 0, sizeof(po));
    po.dst = out.p;
    po.xsize = uint32_t(n);
    po.ysize = 1;
    po.type = 0;
    po.nc = 3;
    po.bits = 32;
    jxlhip::SetInterleaved(&po, po.xsize);
    jxlhip::ColorOutParams cp;
    memset(&cp, 0, sizeof(cp));
    FillColorOutParams(c->fp, {in.as<float>(), uint32_t(n), 1, uint32_t(n), 1, 0, 1}, po, t ? *t : JxlHipColorTarget{}, &cp);
    cp.f.linear_output = t ? 1 : linear_output;
    if (t) memcpy(cp.f.opsin_inv, t->matrix, sizeof(cp.f.opsin_inv));
    LaunchColorOut(cp, c->stream);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(rgb, out.p, n * 12, hipMemcpyDeviceToHost);
  }
  in.Free();
  out.Free();
  return e == hipSuccess ? 0 : -int(e);
}
// Test entries: for the closed-form colour tests of the reference (opsin_image_test.cc) against the kernel itself, and for
// the output encodings of tagged XYB images (jxl_hip_color.h) against a float64 reading.
int jxlhip_debug_color(JxlHipContext* c, const float* xyb, size_t n, int linear_output, float* rgb) {
  return DebugColor(c, xyb, n, linear_output, nullptr, rgb);
}
int jxlhip_debug_color_target(JxlHipContext* c, const float* xyb, size_t n, const JxlHipColorTarget* t, float* rgb) {
  if (!t) return JXLHIP_ERR_INVALID_ARGUMENT;
  return DebugColor(c, xyb, n, 1, t, rgb);
}

// Test entry: noise synthesis alone (k_noise_random, k_noise_add) on caller-supplied dense planes, for a float64 reading.
int jxlhip_debug_noise(JxlHipContext* c, const float* xyb, uint32_t xsize, uint32_t ysize, uint32_t seed0, uint32_t seed1, const float* lut,
                       float ytox, float ytob, uint32_t y_begin, uint32_t y_end, float* raw_out, float* xyb_out) {
  if (!c || !xyb || !lut || !xyb_out || !xsize || !ysize || xsize > (1u << 16) || ysize > (1u << 16)) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (uint64_t(xsize) * ysize > (1u << 24) || y_begin >= y_end || y_end > ysize) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!std::isfinite(ytox) || !std::isfinite(ytob)) return JXLHIP_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < 8; i++)
    if (!std::isfinite(lut[i])) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  {
    int pw = ApplyPendingWait(c);
    if (pw) return pw;
  }
  const size_t bytes = size_t(xsize) * ysize * 12;
  Buf raw, planes;
  int r;
  if ((r = raw.Ensure(bytes)) || (r = planes.Ensure(bytes))) {
    raw.Free();
    planes.Free();
    return r;
  }
  hipError_t e = hipMemcpyAsync(planes.p, xyb, bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    jxlhip::NoiseParams np;
    memset(&np, 0, sizeof(np));
    const uint32_t xgroups = (xsize + 255) / 256;
    FillNoiseParams({planes.as<float>(), xsize, ysize, xsize, ysize, y_begin, y_end}, {raw.as<float>(), seed0, seed1, lut, ytox, ytob}, xgroups,
                    xgroups * ((ysize + 255) / 256), &np);
    LaunchNoise(np, xsize, y_end - y_begin, c->stream);
    e = hipGetLastError();
    if (e == hipSuccess && raw_out) e = hipMemcpyAsync(raw_out, raw.p, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(xyb_out, planes.p, bytes, hipMemcpyDeviceToHost, c->stream);
  }
  const hipError_t es = hipStreamSynchronize(c->stream);  // (before the buffers go, whatever was enqueued)
  raw.Free();
  planes.Free();
  if (e == hipSuccess) e = es;
  return e == hipSuccess ? 0 : -int(e);
}

int jxlhip_debug_pixel_route(JxlHipContext* c, uint32_t* route) {
  if (!c || !route) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->have_frame) return JXLHIP_ERR_NO_FRAME;
  *route = c->color_out || c->ups != 1 ? 0u : (c->tensor_fused ? 3u : (c->gray8_fast ? 2u : 1u));
  return 0;
}

// Test access: the workgroup -> unit map of the lane-kernel batch last prepared on `ctx0` (the first context of a
// jxlhip_run_entropy_batch call) and the estimated length of every workgroup's unit, in dispatch order. `n` is the room
// in both arrays; entries past the batch's workgroups are set to 0xFFFFFFFF / 0.
int jxlhip_debug_entropy_order(JxlHipContext* ctx0, uint32_t* wg_unit, uint64_t* est, size_t n) {
  if (!ctx0 || !wg_unit || !est) return JXLHIP_ERR_INVALID_ARGUMENT;
  const lane_plan::LanePlan& P = ctx0->batch_plan;
  const size_t have = P.wg_est.size();  // (a scalar-form batch has no estimates and reports nothing)
  if (have > n) return JXLHIP_ERR_INVALID_ARGUMENT;
  for (size_t i = 0; i < n; i++) {
    wg_unit[i] = i < have ? P.wg_unit[i] : 0xFFFFFFFFu;
    est[i] = i < have ? P.wg_est[i] : 0;
  }
  return 0;
}
int jxlhip_debug_entropy_timeline(JxlHipContext* ctx0, uint32_t back, uint64_t* records, size_t n, size_t* workgroups) {
  if (!ctx0 || !workgroups) return JXLHIP_ERR_INVALID_ARGUMENT;
  constexpr size_t kKeep = sizeof(ctx0->timeline_wgs) / sizeof(ctx0->timeline_wgs[0]);
  if (back >= kKeep || back >= ctx0->timeline_launches) return JXLHIP_ERR_INVALID_ARGUMENT;
  const size_t slot = (ctx0->timeline_launches - 1 - back) % kKeep, wgs = ctx0->timeline_wgs[slot];
  *workgroups = wgs;
  if (!records) return 0;
  if (n < wgs || !wgs) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(ctx0->device));
  HIP_TRY(hipStreamSynchronize(ctx0->stream));
  HIP_TRY(hipMemcpy(records, ctx0->lanes_timeline.as<uint8_t>() + slot * ctx0->timeline_stride, wgs * 64, hipMemcpyDeviceToHost));
  return 0;
}
int jxlhip_debug_entropy_route(JxlHipContext* c, uint32_t* route) {
  if (!c || !route) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->have_frame) return JXLHIP_ERR_NO_FRAME;
  *route = c->lanes ? 0u : (c->generic_codec ? 3u : (c->alias_lds ? 1u : 2u));  // (LaunchEntropy's own order of choices)
  return 0;
}

int jxlhip_check_guards(JxlHipContext* c, uint32_t* touched) {
  if (!c || !touched) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  *touched = 0;
  uint32_t index = 0;
  for (Buf* b : AllBufs(c)) {
    index++;
    const int t = b->GuardsTouched();
    if (t && !*touched) *touched = index << 2 | uint32_t(t);  // which buffer (1-based position in AllBufs), which side
  }
  return 0;
}

int jxlhip_sync(JxlHipContext* c) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  {
    int pw = ApplyPendingWait(c);
    if (pw) return pw;
  }
  HIP_TRY(WaitStream(c->stream));
  return 0;
}

int jxlhip_download_rgb8(JxlHipContext* c, uint8_t* dst, size_t stride) {
  if (!c || !dst || CallerOwnsPixels(c)) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->have_frame && !c->red.ran) return JXLHIP_ERR_NO_FRAME;
  if (c->red.ran && (c->out_orient & 4)) return JXLHIP_ERR_INVALID_ARGUMENT;  // (transposed rows: jxlhip_download_pixels)
  if (stride < size_t(c->oxs) * 3 || !OutIsRgb8(c)) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  {
    int pw = ApplyPendingWait(c);
    if (pw) return pw;
  }
  HIP_TRY(hipMemcpy2DAsync(dst, stride, c->rgb.p, size_t(c->oxs) * 3, size_t(c->oxs) * 3, c->oys, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(WaitStream(c->stream));
  return 0;
}

int jxlhip_download_rgb8_rows(JxlHipContext* c, uint8_t* dst, size_t stride, uint32_t y_begin, uint32_t y_end) {
  if (!c || !dst || CallerOwnsPixels(c)) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->have_frame) return JXLHIP_ERR_NO_FRAME;
  if (stride < size_t(c->oxs) * 3 || y_begin >= y_end || y_end > c->oys || !OutIsRgb8(c)) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->out_orient & 4) return JXLHIP_ERR_INVALID_ARGUMENT;  // a transposed output has other rows: jxlhip_download_pixels
  HIP_TRY(hipSetDevice(c->device));
  {
    int pw = ApplyPendingWait(c);
    if (pw) return pw;
  }
  HIP_TRY(hipMemcpy2DAsync(dst, stride, c->rgb.as<uint8_t>() + size_t(y_begin) * c->oxs * 3, size_t(c->oxs) * 3, size_t(c->oxs) * 3,
                           y_end - y_begin, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

const uint8_t* jxlhip_rgb8_device_ptr(JxlHipContext* c) { return c && c->have_frame && !CallerOwnsPixels(c) ? c->rgb.as<uint8_t>() : nullptr; }

int jxlhip_get_errors(JxlHipContext* c, uint32_t* flags, size_t n) {
  if (!c || !flags) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->have_frame) return JXLHIP_ERR_NO_FRAME;
  if (n < c->ng) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  {
    int pw = ApplyPendingWait(c);
    if (pw) return pw;
  }
  HIP_TRY(hipMemcpyAsync(flags, c->errors.p, size_t(c->ng) * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (uint32_t g = 0; g < c->ng; g++)
    if (flags[g]) return JXLHIP_ERR_STREAM;
  return 0;
}

int jxlhip_get_section_end_bits(JxlHipContext* c, uint32_t* bits, size_t n) {
  if (!c || !bits) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->have_frame) return JXLHIP_ERR_NO_FRAME;
  if (n < size_t(c->ng) * c->np) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  {
    int pw = ApplyPendingWait(c);
    if (pw) return pw;
  }
  HIP_TRY(hipMemcpyAsync(bits, c->sec_end.p, size_t(c->ng) * c->np * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int jxlhip_download(JxlHipContext* c, const char* name, void* dst, size_t dst_size, size_t* needed) {
  if (!c || !name) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (c->red.have) {  // a reduced upload: the kept DC planes of its run, and nothing of the AC stages
    if (std::string(name) != "dc") return JXLHIP_ERR_UNSUPPORTED;
    if (!c->red.dc_kept || !c->red.ran) return JXLHIP_ERR_INVALID_ARGUMENT;  // needs jxlhip_set_option("keep_dc", 1) and a run
    const size_t dc_bytes = size_t(c->xb) * c->yb * 12;
    if (needed) *needed = dc_bytes;
    if (!dst) return 0;
    if (dst_size < dc_bytes) return JXLHIP_ERR_INVALID_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    {
      int pw = ApplyPendingWait(c);
      if (pw) return pw;
    }
    HIP_TRY(hipMemcpyAsync(dst, c->dc.p, dc_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
  }
  if (!c->have_frame) return JXLHIP_ERR_NO_FRAME;
  const void* src = nullptr;
  size_t bytes = 0;
  const std::string n(name);
  const size_t plane_bytes = size_t(c->xp) * c->yp * 3 * 4;
  if (n == "coeffs") {
    src = c->coeffs.p;
    bytes = size_t(c->ng) * 3 * 65536 * (c->coef_bits / 8);
  } else if (n == "xyb_idct") {
    src = PlaneHolder(c)->plane[0].p;
    bytes = plane_bytes;
  } else if (n == "dc") {  // the DC image the transform stage reads (after smoothing): [3][yb][xb]
    src = c->dc.p;
    bytes = size_t(c->xb) * c->yb * 12;
  } else if (n == "inv_sigma") {
    src = c->inv_sigma.p;
    bytes = size_t(c->xb) * c->yb * 4;
  } else if (n == "kend") {  // uint32 [varblock][3]: scan position after the last non-zero coefficient (scan-order frames)
    if (!c->scan_order) return JXLHIP_ERR_INVALID_ARGUMENT;
    src = c->kend.p;
    bytes = c->blocks_host.size() * 12;
  } else if (n == "transform_lists") {  // uint32 [entry][2] = {strategy, varblock}: the transform work lists in launch order
    if (!c->scan_order) return JXLHIP_ERR_INVALID_ARGUMENT;
    bytes = size_t(c->list_begin[26] + c->list_count[26]) * 8;
  } else if (n == "xyb_filtered") {
    if (!c->keep_filtered || !c->plane[1].p) return JXLHIP_ERR_INVALID_ARGUMENT;  // needs jxlhip_set_option("keep_filtered", 1)
    src = c->plane[1].p;
    bytes = plane_bytes;
  } else if (n == "xyb_upsampled") {  // [3][out_ysize][out_xsize padded to 8]: behind the upsampling (and the noise, if any)
    if (!c->ups_kept || !c->ups_planes.p) return JXLHIP_ERR_INVALID_ARGUMENT;  // needs jxlhip_set_option("keep_upsampled", 1)
    src = c->ups_planes.p;
    bytes = size_t((c->oxs + 7) & ~7u) * c->oys * 3 * 4;
  } else {
    return JXLHIP_ERR_INVALID_ARGUMENT;
  }
  if (needed) *needed = bytes;
  if (!dst) return 0;
  if (dst_size < bytes) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  {
    int pw = ApplyPendingWait(c);
    if (pw) return pw;
  }
  if (n == "transform_lists") {
    uint32_t* out = static_cast<uint32_t*>(dst);
    std::vector<uint32_t> list(bytes / 8);
    HIP_TRY(hipMemcpyAsync(list.data(), c->tlist.p, list.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int s = 0; s < 27; s++)
      for (uint32_t j = 0; j < c->list_count[s]; j++) {
        out[2 * size_t(c->list_begin[s] + j)] = uint32_t(s);
        out[2 * size_t(c->list_begin[s] + j) + 1] = list[c->list_begin[s] + j];
      }
    return 0;
  }
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (n == "coeffs" && c->scan_order) {
    // the device holds scan-order entries [covered, kend) per (block, channel): present them in the natural layout
    std::vector<uint32_t> kend(c->blocks_host.size() * 3);
    HIP_TRY(hipMemcpy(kend.data(), c->kend.p, kend.size() * 4, hipMemcpyDeviceToHost));
    const size_t esz = c->coef_bits / 8;
    std::vector<uint8_t> tmp(65536 * esz);
    for (uint32_t g = 0; g < c->ng; g++)
      for (uint32_t b = c->gbb_host[g]; b < c->gbb_host[g + 1]; b++) {
        const JxlHipVarBlock& v = c->blocks_host[b];
        const uint32_t covered = jxlhip::CoveredBlocks(v.strategy), size = covered * 64;
        for (int ch = 0; ch < 3; ch++) {
          uint8_t* base = static_cast<uint8_t*>(dst) + ((size_t(g) * 3 + ch) * 65536 + v.coef_offset) * esz;
          const uint16_t* order = c->orders_host.data() + c->order_offset_host[jxlhip::kStrategyOrder[v.strategy] * 3 + ch];
          uint32_t ke = kend[size_t(b) * 3 + ch];
          ke = ke > size ? size : ke;
          memcpy(tmp.data(), base, size * esz);
          memset(base, 0, size * esz);
          for (uint32_t k = covered; k < ke; k++) memcpy(base + size_t(order[k]) * esz, tmp.data() + size_t(k) * esz, esz);
        }
      }
  }
  return 0;
}

// ---- canvas (jxl_hip_canvas.h)
struct JxlHipCanvas {
  int device = 0;
  uint32_t xs = 0, ys = 0;
  bool has_alpha = false, premultiplied = false, unpremul_out = false;
  Buf cur, slot[4], pixels;
  bool slot_valid[4] = {false, false, false, false};
  // frames kept before the colour transform, [3][xyb_h][xyb_w]: 0..3 the reference slots (patch sources), 4..7 the DC
  // frames of level 1..4 (passes_state.h:90 dc_frames: the DC image of a later frame with kUseDcFrame)
  Buf xyb[8];
  uint32_t xyb_w[8] = {0, 0, 0, 0, 0, 0, 0, 0}, xyb_h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool xyb_alpha[8] = {false, false, false, false, false, false, false, false};  // a fourth plane: the frame's alpha
  hipStream_t last_stream = nullptr;  // the stream of the last blend: later work on the canvas is ordered behind it
};

int jxlhip_canvas_set_unpremultiply(JxlHipCanvas* v, int on) {
  if (!v) return JXLHIP_ERR_INVALID_ARGUMENT;
  v->unpremul_out = on != 0;
  return 0;
}

int jxlhip_canvas_create(int device, uint32_t xsize, uint32_t ysize, uint32_t has_alpha, uint32_t premultiplied, JxlHipCanvas** out) {
  if (!out || !xsize || !ysize || xsize > (1u << 18) || ysize > (1u << 18)) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(device));
  JxlHipCanvas* v = new (std::nothrow) JxlHipCanvas;
  if (!v) return JXLHIP_ERR_INVALID_ARGUMENT;
  v->device = device;
  v->xs = xsize;
  v->ys = ysize;
  v->has_alpha = has_alpha != 0;
  v->premultiplied = premultiplied != 0;
  int r = v->cur.Ensure(size_t(xsize) * ysize * 16);
  if (r) {
    delete v;
    return r;
  }
  *out = v;
  return 0;
}

void jxlhip_canvas_destroy(JxlHipCanvas* v) {
  if (!v) return;
  (void)hipSetDevice(v->device);
  if (v->last_stream) (void)hipStreamSynchronize(v->last_stream);
  v->cur.Free();
  v->pixels.Free();
  for (Buf& b : v->slot) b.Free();
  for (Buf& b : v->xyb) b.Free();
  delete v;
}

int jxlhip_canvas_save_xyb(JxlHipCanvas* v, JxlHipContext* c, uint32_t slot) {
  if (!v || !c || slot > 7 || c->device != v->device) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (CallerOwnsPixels(c)) return JXLHIP_ERR_UNSUPPORTED;  // (composed frames keep the context's own buffers)
  if (c->red.have) return JXLHIP_ERR_UNSUPPORTED;          // (a reduced image is no frame of the canvas's size)
  HIP_TRY(hipSetDevice(v->device));
  {
    int pw = ApplyPendingWait(c);
    if (pw) return pw;
  }
  const float* src;
  size_t src_stride, src_plane;
  uint32_t w, h;
  if (c->mod.have) {  // a Modular frame (a later VarDCT upload clears the flag): the float planes of the "keep_xyb_planes" pass
    if (!c->keep_xyb || !c->spl_planes.p) return JXLHIP_ERR_INVALID_ARGUMENT;
    w = c->mod.xs;
    h = c->mod.ys;
    src = c->spl_planes.as<float>();
    src_stride = w;
    src_plane = size_t(w) * h;
  } else if (c->have_frame) {  // a VarDCT frame: the filtered planes (patches, splines, noise already on them)
    if (c->ups != 1 || !c->color_out || !c->plane[1].p) return JXLHIP_ERR_UNSUPPORTED;
    w = c->xs;
    h = c->ys;
    src = c->plane[1].as<float>();
    src_stride = c->xp;
    src_plane = size_t(c->xp) * c->yp;
  } else {
    return JXLHIP_ERR_NO_FRAME;
  }
  // (the frame's extra channels are kept with it, for patches that blend through alpha: dec_patch_dictionary.cc:342-347)
  const bool mod_alpha = c->mod.have && c->mod.has_alpha;
  const bool with_alpha = mod_alpha || (!c->mod.have && c->have_alpha && c->alpha.cap >= size_t(w) * h * 4);
  int r = v->xyb[slot].Ensure(size_t(w) * h * (with_alpha ? 16 : 12));
  if (r) return r;
  if (v->last_stream && v->last_stream != c->stream) HIP_TRY(hipStreamSynchronize(v->last_stream));
  hipLaunchKernelGGL(jxlhip::k_copy_planes, dim3((w + 255) / 256, h, 3), dim3(256), 0, c->stream, src, src_stride, src_plane,
                     v->xyb[slot].as<float>(), w, h);
  HIP_TRY(hipGetLastError());
  if (mod_alpha) {
    const JxlHipContext::Modular& M = c->mod;
    const size_t n = size_t(w) * h;
    hipLaunchKernelGGL(jxlhip::k_int_plane_to_float, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, c->stream,
                       M.pool.as<int32_t>() + M.buf_off[M.out_buffer[M.num_color]], v->xyb[slot].as<float>() + n * 3, n,
                       1.0f / float((uint64_t(1) << M.alpha_bits) - 1));
    HIP_TRY(hipGetLastError());
  } else if (with_alpha)
    HIP_TRY(hipMemcpyAsync(v->xyb[slot].as<float>() + size_t(w) * h * 3, (c->alpha_patched_valid ? c->alpha_patched : c->alpha).p,
                           size_t(w) * h * 4, hipMemcpyDeviceToDevice, c->stream));
  v->xyb_alpha[slot] = with_alpha;
  HIP_TRY(hipStreamSynchronize(c->stream));  // (later frames read the slot from other streams of other contexts)
  v->xyb_w[slot] = w;
  v->xyb_h[slot] = h;
  if (slot < 4) v->slot_valid[slot] = false;  // (the slot now holds a frame saved BEFORE the colour transform: not a blending source)
  v->last_stream = c->stream;
  return 0;
}

int jxlhip_canvas_xyb_source(JxlHipCanvas* v, uint32_t slot, const float** planes, uint32_t* xsize, uint32_t* ysize) {
  if (!v || slot > 7 || !planes || !xsize || !ysize) return JXLHIP_ERR_INVALID_ARGUMENT;
  *planes = v->xyb_w[slot] ? v->xyb[slot].as<float>() : nullptr;
  *xsize = v->xyb_w[slot];
  *ysize = v->xyb_h[slot];
  return 0;
}

int jxlhip_canvas_xyb_alpha(JxlHipCanvas* v, uint32_t slot, const float** alpha) {
  if (!v || slot > 7 || !alpha) return JXLHIP_ERR_INVALID_ARGUMENT;
  *alpha = (v->xyb_w[slot] && v->xyb_alpha[slot]) ? v->xyb[slot].as<float>() + size_t(v->xyb_w[slot]) * v->xyb_h[slot] * 3 : nullptr;
  return 0;
}

int jxlhip_canvas_blend(JxlHipCanvas* v, JxlHipContext* c, const JxlHipBlend* b) {
  if (!v || !c || !b || c->device != v->device) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (b->mode > 4 || b->alpha_mode > 4 || b->source > 3 || b->alpha_source > 3 || b->save_slot > 3) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (CallerOwnsPixels(c)) return JXLHIP_ERR_UNSUPPORTED;  // (the frame's pixels are in the caller's tensor, not in c->rgb)
  if (c->red.have) return JXLHIP_ERR_UNSUPPORTED;
  if (!c->have_frame && !c->mod.have) return JXLHIP_ERR_NO_FRAME;
  if (c->out_type != 0 || c->out_nc != 4 || c->out_swap || c->out_orient) return JXLHIP_ERR_INVALID_ARGUMENT;  // f32 x 4 as coded
  if (size_t(c->oxs) * c->oys * 16 > c->rgb.cap) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(v->device));
  {
    int pw = ApplyPendingWait(c);
    if (pw) return pw;
  }
  const size_t bytes = size_t(v->xs) * v->ys * 16;
  jxlhip::BlendParams P;
  memset(&P, 0, sizeof(P));
  P.out = v->cur.as<float>();
  P.bg_color = v->slot_valid[b->source] ? v->slot[b->source].as<float>() : nullptr;
  P.bg_alpha = v->slot_valid[b->alpha_source] ? v->slot[b->alpha_source].as<float>() : nullptr;
  P.fg = c->rgb.as<float>();
  P.w = v->xs;
  P.h = v->ys;
  P.fw = c->oxs;
  P.fh = c->oys;
  P.x0 = b->x0;
  P.y0 = b->y0;
  P.mode = b->mode;
  P.alpha_mode = b->alpha_mode;
  P.clamp = b->clamp;
  P.alpha_clamp = b->alpha_clamp;
  P.has_alpha = v->has_alpha;
  P.premultiplied = v->premultiplied;
  if (v->last_stream && v->last_stream != c->stream) HIP_TRY(hipStreamSynchronize(v->last_stream));
  hipLaunchKernelGGL(jxlhip::k_canvas_blend, dim3((v->xs + 255) / 256, v->ys), dim3(256), 0, c->stream, P);
  HIP_TRY(hipGetLastError());
  if (b->save_slot >= 0) {
    int r = v->slot[b->save_slot].Ensure(bytes);
    if (r) return r;
    HIP_TRY(hipMemcpyAsync(v->slot[b->save_slot].p, v->cur.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    v->slot_valid[b->save_slot] = true;
    // the slot now holds a frame saved AFTER the colour transform: patches cannot take it (dec_patch_dictionary.cc:66-73)
    v->xyb_w[b->save_slot] = v->xyb_h[b->save_slot] = 0;
  }
  v->last_stream = c->stream;
  return 0;
}

int jxlhip_debug_blend(int device, const float* bg, const float* fg, size_t n, const JxlHipBlend* b, uint32_t has_alpha, uint32_t premultiplied,
                       float* out) {
  if (!bg || !fg || !b || !out || !n || n > (1u << 20) || b->mode > 4 || b->alpha_mode > 4) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(device));
  Buf dbg, dfg, dout;
  int r;
  if ((r = dbg.Ensure(n * 16)) || (r = dfg.Ensure(n * 16)) || (r = dout.Ensure(n * 16))) {
    dbg.Free();
    dfg.Free();
    dout.Free();
    return r;
  }
  hipError_t e = hipMemcpy(dbg.p, bg, n * 16, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dfg.p, fg, n * 16, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    jxlhip::BlendParams P;
    memset(&P, 0, sizeof(P));
    P.out = dout.as<float>();
    P.bg_color = dbg.as<float>();
    P.bg_alpha = dbg.as<float>();
    P.fg = dfg.as<float>();
    P.w = P.fw = uint32_t(n);
    P.h = P.fh = 1;
    P.mode = b->mode;
    P.alpha_mode = b->alpha_mode;
    P.clamp = b->clamp;
    P.alpha_clamp = b->alpha_clamp;
    P.has_alpha = has_alpha;
    P.premultiplied = premultiplied;
    hipLaunchKernelGGL(jxlhip::k_canvas_blend, dim3((uint32_t(n) + 255) / 256, 1), dim3(256), 0, nullptr, P);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, n * 16, hipMemcpyDeviceToHost);
  }
  dbg.Free();
  dfg.Free();
  dout.Free();
  return e == hipSuccess ? 0 : -int(e);
}

// Device buffers of one test entry: freed together, whichever way the entry leaves.
namespace {
struct DebugBufs {
  Buf b[12];
  ~DebugBufs() {
    for (Buf& x : b) x.Free();
  }
  // `bytes` of host memory into buffer k (NULL: the buffer stays empty)
  int Put(int k, const void* host, size_t bytes) {
    if (!host) return 0;
    int r = b[k].Ensure(bytes);
    if (r) return r;
    HIP_TRY(hipMemcpy(b[k].p, host, bytes, hipMemcpyHostToDevice));
    return 0;
  }
};
}  // namespace

// Test entry: k_canvas_blend as jxlhip_canvas_blend launches it, on a caller's canvas, backgrounds and frame.
int jxlhip_debug_blend_rect(int device, uint32_t xsize, uint32_t ysize, const float* bg_color, const float* bg_alpha, const float* fg,
                            uint32_t fxsize, uint32_t fysize, const JxlHipBlend* b, uint32_t has_alpha, uint32_t premultiplied, float* out) {
  if (!fg || !b || !out || !xsize || !ysize || !fxsize || !fysize) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (xsize > (1u << 14) || ysize > (1u << 14) || fxsize > (1u << 14) || fysize > (1u << 14)) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (b->mode > 4 || b->alpha_mode > 4 || b->x0 < -(1 << 20) || b->x0 > (1 << 20) || b->y0 < -(1 << 20) || b->y0 > (1 << 20))
    return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(device));
  const size_t bytes = size_t(xsize) * ysize * 16, fbytes = size_t(fxsize) * fysize * 16;
  DebugBufs d;
  int r;
  if ((r = d.Put(0, bg_color, bytes)) || (r = d.Put(1, bg_alpha, bytes)) || (r = d.Put(2, fg, fbytes)) || (r = d.b[3].Ensure(bytes))) return r;
  jxlhip::BlendParams P;
  memset(&P, 0, sizeof(P));
  P.out = d.b[3].as<float>();
  P.bg_color = d.b[0].as<float>();
  P.bg_alpha = d.b[1].as<float>();
  P.fg = d.b[2].as<float>();
  P.w = xsize;
  P.h = ysize;
  P.fw = fxsize;
  P.fh = fysize;
  P.x0 = b->x0;
  P.y0 = b->y0;
  P.mode = b->mode;
  P.alpha_mode = b->alpha_mode;
  P.clamp = b->clamp;
  P.alpha_clamp = b->alpha_clamp;
  P.has_alpha = has_alpha;
  P.premultiplied = premultiplied;
  hipLaunchKernelGGL(jxlhip::k_canvas_blend, dim3((xsize + 255) / 256, ysize), dim3(256), 0, nullptr, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, d.b[3].p, bytes, hipMemcpyDeviceToHost));
  return 0;
}

// Test entry: k_patches_add as the filter stage launches it, on a caller's dense planes; the reference frames and every
// table come from host memory and are checked like an upload's (upload::CheckPatches) before anything is launched.
int jxlhip_debug_patches(JxlHipContext* c, const float* planes_in, const float* alpha_in, uint32_t xsize, uint32_t ysize, const JxlHipPatches* pt,
                         uint32_t y_begin, uint32_t y_end, float* planes_out, float* alpha_out) {
  if (!c || !planes_in || !planes_out || !pt || !xsize || !ysize || xsize > (1u << 14) || ysize > (1u << 14)) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (y_begin >= y_end || y_end > ysize || !pt->num_positions) return JXLHIP_ERR_INVALID_ARGUMENT;
  if ((alpha_in != nullptr) != (pt->uses_alpha != 0) || (alpha_in != nullptr) != (alpha_out != nullptr)) return JXLHIP_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < 4; k++)
    if (pt->slot_planes[k] && (!pt->slot_w[k] || !pt->slot_h[k] || pt->slot_w[k] > (1u << 14) || pt->slot_h[k] > (1u << 14)))
      return JXLHIP_ERR_INVALID_ARGUMENT;
  // (a rectangle may reach past xsize, as on a VarDCT frame it may reach into the padding: the kernel clips its columns at
  // xsize, which a test must be able to show; rows come from the row lists alone, and those are checked)
  int r = upload::CheckPatches(*pt, ysize, 1u << 15, ysize);
  if (r) return r;
  HIP_TRY(hipSetDevice(c->device));
  if ((r = ApplyPendingWait(c))) return r;
  HIP_TRY(hipStreamSynchronize(c->stream));
  const size_t n = size_t(xsize) * ysize;
  DebugBufs d;
  if ((r = d.Put(0, planes_in, n * 12)) || (r = d.Put(1, alpha_in, n * 4)) || (r = d.Put(2, pt->records, size_t(pt->num_positions) * 32)) ||
      (r = d.Put(3, pt->row_start, (size_t(ysize) + 1) * 4)) || (r = d.Put(4, pt->row_list, size_t(pt->num_row_entries) * 4)))
    return r;
  const float *slot_planes[4] = {}, *slot_alpha[4] = {};
  uint32_t slot_w[4] = {}, slot_h[4] = {};
  for (int k = 0; k < 4; k++) {
    if (!pt->slot_planes[k]) continue;
    const size_t sn = size_t(pt->slot_w[k]) * pt->slot_h[k];
    if ((r = d.Put(5 + k, pt->slot_planes[k], sn * 12))) return r;
    if (alpha_in && (r = d.Put(9 + k, pt->slot_alpha[k], sn * 4))) return r;
    slot_planes[k] = d.b[5 + k].as<float>();
    slot_alpha[k] = d.b[9 + k].as<float>();
    slot_w[k] = pt->slot_w[k];
    slot_h[k] = pt->slot_h[k];
  }
  const PatchAlpha alpha = {d.b[1].as<float>(), xsize, pt->premultiplied ? 1u : 0u, slot_alpha};  // (a null plane without alpha_in)
  jxlhip::PatchParams pp;
  memset(&pp, 0, sizeof(pp));
  FillPatchParams({d.b[0].as<float>(), xsize, n, xsize, y_begin, y_end},
                  {d.b[2].as<uint32_t>(), d.b[3].as<uint32_t>(), d.b[4].as<uint32_t>(), slot_planes, slot_w, slot_h}, &alpha, &pp);
  hipLaunchKernelGGL(jxlhip::k_patches_add, dim3(y_end - y_begin), dim3(256), 0, c->stream, pp);
  hipError_t e = hipGetLastError();
  const hipError_t es = hipStreamSynchronize(c->stream);  // (before the buffers go, whatever was enqueued)
  if (e == hipSuccess) e = es;
  if (e == hipSuccess) e = hipMemcpy(planes_out, d.b[0].p, n * 12, hipMemcpyDeviceToHost);
  if (e == hipSuccess && alpha_out) e = hipMemcpy(alpha_out, d.b[1].p, n * 4, hipMemcpyDeviceToHost);
  return e == hipSuccess ? 0 : -int(e);
}

// Test entry: k_splines_add as the filter stage launches it, on a caller's dense planes and a draw cache from host memory,
// checked like an upload's (upload::CheckSplines); segments the kernel's llroundf could not take are refused as well.
int jxlhip_debug_splines(JxlHipContext* c, const float* planes_in, uint32_t xsize, uint32_t ysize, const JxlHipSplines* sp, uint32_t y_begin,
                         uint32_t y_end, float* planes_out) {
  if (!c || !planes_in || !planes_out || !sp || !xsize || !ysize || xsize > (1u << 14) || ysize > (1u << 14)) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (y_begin >= y_end || y_end > ysize || !sp->num_segments) return JXLHIP_ERR_INVALID_ARGUMENT;
  int r = upload::CheckSplines(*sp, ysize);
  if (r) return r;
  for (size_t i = 0; i < size_t(sp->num_segments) * 8; i++) {
    const float v = sp->segments[i];
    if (!std::isfinite(v) || ((i & 7) < 3 && std::fabs(v) > float(1 << 30))) return JXLHIP_ERR_INVALID_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(c->device));
  if ((r = ApplyPendingWait(c))) return r;
  HIP_TRY(hipStreamSynchronize(c->stream));
  const size_t n = size_t(xsize) * ysize;
  DebugBufs d;
  if ((r = d.Put(0, planes_in, n * 12)) || (r = d.Put(1, sp->segments, size_t(sp->num_segments) * 32)) ||
      (r = d.Put(2, sp->row_start, (size_t(ysize) + 1) * 4)) || (r = d.Put(3, sp->row_segments, size_t(sp->num_row_segments) * 4)))
    return r;
  jxlhip::SplineParams P;
  memset(&P, 0, sizeof(P));
  FillSplineParams({d.b[0].as<float>(), xsize, n, xsize, y_begin, y_end}, {d.b[1].as<float>(), d.b[2].as<uint32_t>(), d.b[3].as<uint32_t>()}, &P);
  hipLaunchKernelGGL(jxlhip::k_splines_add, dim3(y_end - y_begin), dim3(256), 0, c->stream, P);
  hipError_t e = hipGetLastError();
  const hipError_t es = hipStreamSynchronize(c->stream);  // (before the buffers go, whatever was enqueued)
  if (e == hipSuccess) e = es;
  if (e == hipSuccess) e = hipMemcpy(planes_out, d.b[0].p, n * 12, hipMemcpyDeviceToHost);
  return e == hipSuccess ? 0 : -int(e);
}

int jxlhip_canvas_download(JxlHipCanvas* v, uint32_t data_type, uint32_t num_channels, uint32_t bits, int big_endian, uint32_t orientation,
                           void* dst, size_t stride) {
  if (!v || !dst || num_channels < 1 || num_channels > 4 || orientation < 1 || orientation > 8) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (data_type != 0 && data_type != 2 && data_type != 3 && data_type != 5) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(v->device));
  static const uint8_t kBits[9] = {0, 0, 1, 3, 2, 4, 6, 7, 5};
  const uint32_t sample = data_type == 2 ? 1 : (data_type == 0 ? 4 : 2), full = sample * 8;
  jxlhip::PixelOut po;
  memset(&po, 0, sizeof(po));
  int r = v->pixels.Ensure(size_t(v->xs) * v->ys * num_channels * sample);
  if (r) return r;
  po.dst = v->pixels.p;
  po.alpha = v->has_alpha ? v->cur.as<float>() + size_t(3) * v->xs * v->ys : nullptr;
  po.xsize = v->xs;
  po.ysize = v->ys;
  po.orient = kBits[orientation] | ((v->unpremul_out && v->has_alpha) ? 8u : 0u);
  po.type = data_type;
  po.nc = num_channels;
  po.bits = (data_type == 2 || data_type == 3) ? (bits && bits < full ? bits : full) : 0;
  po.swap = big_endian && sample > 1;
  jxlhip::SetInterleaved(&po, (po.orient & 4) ? po.ysize : po.xsize);
  hipStream_t st = v->last_stream;
  hipLaunchKernelGGL(jxlhip::k_canvas_out, dim3((v->xs + 255) / 256, v->ys), dim3(256), 0, st, static_cast<const float*>(v->cur.as<float>()), po);
  HIP_TRY(hipGetLastError());
  const bool transposed = (po.orient & 4) != 0;
  const size_t row = size_t(transposed ? v->ys : v->xs) * num_channels * sample, rows = transposed ? v->xs : v->ys;
  if (stride < row) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipMemcpy2DAsync(dst, stride, v->pixels.p, row, row, rows, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

int jxlhip_canvas_download_alpha(JxlHipCanvas* v, float* dst, size_t n) {
  if (!v || !dst || n < size_t(v->xs) * v->ys) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(v->device));
  HIP_TRY(hipMemcpyAsync(dst, v->cur.as<float>() + size_t(3) * v->xs * v->ys, size_t(v->xs) * v->ys * 4, hipMemcpyDeviceToHost, v->last_stream));
  HIP_TRY(hipStreamSynchronize(v->last_stream));
  return 0;
}

// ---- forward path: see jxl_hip_enc.h
// The two kernels of the adaptive quant field (jxl_hip_enc.h) on the context's stream.
static void EncAqLaunch(JxlHipContext* c, const jxlhip::EncAq& A) {
  const uint32_t strips = (A.xp + jxlhip::kAqCols - 1) / jxlhip::kAqCols;
  hipLaunchKernelGGL(jxlhip::k_enc_aq_cells, dim3((strips + 3) / 4, (A.yp + jxlhip::kAqRows - 1) / jxlhip::kAqRows), dim3(256), 0, c->stream, A);
  hipLaunchKernelGGL(jxlhip::k_enc_aq_blocks, dim3((A.xb + 7) / 8, A.yb), dim3(64), 0, c->stream, A);
}
static int EncAqEnsure(JxlHipContext* c, uint32_t xp, uint32_t yp, jxlhip::EncAq* A) {
  const size_t nb = size_t(xp / 8) * (yp / 8);
  int r;
  if ((r = c->enc_aq_cells.Ensure(nb * 4 * 4)) || (r = c->enc_aq_map.Ensure(nb * 4)) || (r = c->enc_aq_mask.Ensure(nb * 4))) return r;
  A->cells = c->enc_aq_cells.as<float>();
  A->aq = c->enc_aq_map.as<float>();
  A->mask = c->enc_aq_mask.as<float>();
  A->xp = xp;
  A->yp = yp;
  A->xb = xp / 8;
  A->yb = yp / 8;
  return 0;
}

// What the search of strategy_mode 2 / 3 needs besides the forward path's own buffers: the candidate list of the frame size
// (built on the host and uploaded once per (xb, yb, floating): a second frame of the same size and jxlhip_enc_forward_rerun
// upload nothing), the walk's table with the entries nothing writes at zero, the masking plane, the zero factors, the events.
static int EncSearchPrepare(JxlHipContext* c, const jxlhip::EncFwd& P, uint32_t floating) {
  const size_t tiles = size_t((P.xb + 7) / 8) * ((P.yb + 7) / 8);
  int r;
  if ((r = c->srch_mask.Ensure(size_t(P.xp) * P.yp * 4)) || (r = c->srch_zero.Ensure(tiles)) || (r = c->srch_table.Ensure(tiles * jxh::kAcsWalkTileFloats * 4)))
    return r;
  for (auto& ev : c->srch_ev)
    if (!ev) HIP_TRY(hipEventCreate(&ev));
  HIP_TRY(hipMemsetAsync(c->srch_zero.p, 0, tiles, c->stream));
  if (c->srch_xb == P.xb && c->srch_yb == P.yb && c->srch_floating == floating && c->srch_cand.p) return 0;
  c->srch_xb = c->srch_yb = 0;
  jxh::AcsWalkList list;
  if (!jxh::AcsWalkCandidates(P.xb, P.yb, floating, &list)) return JXLHIP_ERR_INVALID_ARGUMENT;
  const size_t n = list.cand.size();
  if ((r = c->srch_cand.Ensure(n * sizeof(JxlHipEncAcsCandidate))) || (r = c->srch_index.Ensure(n * 4))) return r;
  HIP_TRY(hipMemcpyAsync(c->srch_cand.p, list.cand.data(), n * sizeof(JxlHipEncAcsCandidate), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->srch_index.p, list.index.data(), n * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->srch_table.p, 0, tiles * jxh::kAcsWalkTileFloats * 4, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // (the list is a local)
  memcpy(c->srch_first, list.first, sizeof(c->srch_first));
  c->srch_xb = P.xb;
  c->srch_yb = P.yb;
  c->srch_floating = floating;
  return 0;
}

// The kernel sequence of the forward path on the context's stream (P.planes is set on the way).
static int EncLaunch(JxlHipContext* c, jxlhip::EncFwd& P, bool gaborish) {
  const size_t nb = size_t(P.xb) * P.yb, ng = size_t(P.xg) * P.yg;
  // colour: into planes[0] when there is no sharpening, else into the `orig` set
  float* sets[3] = {c->enc_planes[0].as<float>(), c->enc_planes[1].as<float>(), c->enc_planes[2].as<float>()};
  const dim3 px_grid((P.xp + 255) / 256, P.yp);
  P.planes = gaborish ? sets[2] : sets[0];
  hipLaunchKernelGGL(jxlhip::k_enc_xyb, px_grid, dim3(256), 0, c->stream, P);
  if (P.quant_field_mode) {  // the adaptive quant field, from the planes before the sharpening (enc_heuristics.cc:1118-1143)
    jxlhip::EncAq& A = c->enc_last_aq;
    int r = EncAqEnsure(c, P.xp, P.yp, &A);  // (jxlhip_enc_initial_quant_field shares the buffers and may have grown them since)
    if (r) return r;
    P.aq_map = A.aq;
    A.planes = P.planes;
    HIP_TRY(hipEventRecord(c->enc_ev[4], c->stream));
    EncAqLaunch(c, A);
    HIP_TRY(hipEventRecord(c->enc_ev[5], c->stream));
  }
  const bool search = P.strategy_mode >= 2;  // (jxlhip_enc_forward has prepared the list and the buffers: EncSearchPrepare)
  if (search) {  // the per-pixel masking, like the field from the planes before the sharpening
    jxlhip::EncMask1x1 M;
    M.y = P.planes + size_t(P.xp) * P.yp;
    M.out = c->srch_mask.as<float>();
    M.xp = P.xp;
    M.yp = P.yp;
    jxh::EncMask1x1Weights(M.w);
    HIP_TRY(hipEventRecord(c->srch_ev[0], c->stream));
    hipLaunchKernelGGL(jxlhip::k_enc_mask1x1, dim3((P.xp + jxlhip::kMaskCols - 1) / jxlhip::kMaskCols, (P.yp + jxlhip::kMaskRows - 1) / jxlhip::kMaskRows),
                       dim3(256), 0, c->stream, M);
    HIP_TRY(hipEventRecord(c->srch_ev[1], c->stream));
  }
  if (gaborish) {
    if (getenv("JXLHIP_ENC_SHARPEN_ROUNDS")) {  // the one-round-per-launch form: orig = sets[2]; 2 -> 0 -> 1 -> 0 -> 1
      const dim3 g3(px_grid.x, px_grid.y, 3);
      const float* in = sets[2];
      float* out = sets[0];
      for (int it = 0; it < 4; it++) {
        hipLaunchKernelGGL(jxlhip::k_enc_sharpen, g3, dim3(256), 0, c->stream, static_cast<const float*>(sets[2]), in, out, P.xp, P.yp);
        in = out;
        out = out == sets[0] ? sets[1] : sets[0];
      }
      P.planes = const_cast<float*>(in);
    } else {
      const uint32_t strips = (P.xp + jxlhip::kSharpenCols - 1) / jxlhip::kSharpenCols;
      hipLaunchKernelGGL(jxlhip::k_enc_sharpen_rows, dim3((strips + 3) / 4, (P.yp + jxlhip::kSharpenRows - 1) / jxlhip::kSharpenRows, 3), dim3(256), 0,
                         c->stream, static_cast<const float*>(sets[2]), sets[0], P.xp, P.yp);
      P.planes = sets[0];
    }
  }
  const uint32_t tiles = ((P.xb + 7) / 8) * ((P.yb + 7) / 8);
  if (search) {
    // the reference's search in place of the activity rule: every candidate's estimate on the resident planes (the field
    // and the masking from before the sharpening, chroma-from-luma factors 0, the frame's own distance) into the walk's
    // table, one launch per kind, then the walk, which also writes the quant field
    jxlhip::EncEstimate E;
    memset(&E, 0, sizeof(E));
    E.planes = P.planes;
    E.quant = P.aq_map;
    E.mask = c->srch_mask.as<float>();
    E.ytox = E.ytob = c->srch_zero.as<int8_t>();
    E.basis_t = P.basis_t;
    E.estimates = c->srch_table.as<float>();
    E.xp = P.xp;
    E.yp = P.yp;
    E.xb = P.xb;
    E.tiles_x = (P.xb + 7) / 8;
    jxh::EncEstimateWeights(P.distance, E.weights);
    jxh::EncEstimateChannelMul(E.channel_mul);
    HIP_TRY(hipEventRecord(c->srch_ev[2], c->stream));
    for (uint32_t k = 0; k < jxh::kAcsWalkKinds; k++) {
      const size_t first = c->srch_first[k], n = c->srch_first[k + 1] - first;
      if (!n) continue;
      uint32_t dq_kind = 0;
      jxh::EncEstimateShape(jxh::AcsWalkStrategy(k), &E.cx, &E.cy, &dq_kind);
      E.dequant = P.dequant + P.dq_offset[dq_kind];
      E.cand = c->srch_cand.as<JxlHipEncAcsCandidate>() + first;
      E.index = c->srch_index.as<uint32_t>() + first;
      E.n = uint32_t(n);
      E.x_weight = E.cx * E.cy >= 2 ? jxh::EncEstimateXWeight(E.cx * E.cy) : 1.0f;
      const uint32_t area = E.cx * E.cy * 64;
      if (area < 1024) hipLaunchKernelGGL((jxlhip::k_enc_estimate<64, 1>), dim3((E.n + 3) / 4), dim3(256), 0, c->stream, E);
      else if (area == 1024) hipLaunchKernelGGL((jxlhip::k_enc_estimate<256, 4>), dim3(E.n), dim3(256), 0, c->stream, E);
      else hipLaunchKernelGGL((jxlhip::k_enc_estimate<256, 8>), dim3(E.n), dim3(256), 0, c->stream, E);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(c->srch_ev[3], c->stream));
    jxlhip::EncAcsWalk W;
    memset(&W, 0, sizeof(W));
    W.table = c->srch_table.as<float>();
    W.acs = P.acs;
    W.qf = P.qf;
    W.aq_map = P.aq_map;
    W.xb = P.xb;
    W.yb = P.yb;
    W.floating = P.strategy_mode - 2;
    W.mul8x8 = jxh::AcsWalkMul8x8(P.distance);
    W.mean_max_mixer = P.mean_max_mixer;
    W.inv_gs = P.inv_gs;
    hipLaunchKernelGGL(jxlhip::k_enc_acs_walk, dim3(tiles), dim3(64), 0, c->stream, W);
    HIP_TRY(hipEventRecord(c->srch_ev[4], c->stream));
  } else {
    hipLaunchKernelGGL(jxlhip::k_enc_activity, dim3((P.xb + 7) / 8, P.yb), dim3(64), 0, c->stream, P);
    if (P.quant_field_mode) hipLaunchKernelGGL(jxlhip::k_enc_select<true>, dim3(tiles), dim3(64), 0, c->stream, P);
    else hipLaunchKernelGGL(jxlhip::k_enc_select<false>, dim3(tiles), dim3(64), 0, c->stream, P);
  }
  hipLaunchKernelGGL(jxlhip::k_enc_offsets, dim3(uint32_t(ng)), dim3(64), 0, c->stream, P);
  HIP_TRY(hipMemsetAsync(c->enc_coef.p, 0, ng * 3 * 65536 * 4, c->stream));
  HIP_TRY(hipEventRecord(c->enc_ev[2], c->stream));
  if (getenv("JXLHIP_ENC_BLOCK_KERNEL"))  // the one-workgroup-per-transform form (kept as the simple statement of the algorithm)
    hipLaunchKernelGGL(jxlhip::k_enc_transform<256>, dim3(uint32_t(nb)), dim3(256), 0, c->stream, P);
  else
    hipLaunchKernelGGL(jxlhip::k_enc_transform_tile, dim3(tiles), dim3(256), 0, c->stream, P);
  HIP_TRY(hipEventRecord(c->enc_ev[3], c->stream));
  HIP_TRY(hipGetLastError());
  return 0;
}

int jxlhip_enc_forward(JxlHipContext* c, const uint8_t* rgb, size_t stride, const JxlHipEncDesc* d, uint8_t* acs, int32_t* qf, int32_t* dc,
                       int32_t* coeffs) {
  if (!c || !rgb || !d || !acs || !qf || !dc) return JXLHIP_ERR_INVALID_ARGUMENT;  // (coeffs may be NULL: they stay on the device)
  if (!d->xsize || !d->ysize || d->xsize > (1u << 18) || d->ysize > (1u << 18) || stride < size_t(d->xsize) * 3) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!(d->distance > 0) || !d->global_scale || !d->quant_dc || !d->dequant || d->strategy_mode > 3 || d->quant_field_mode > 1)
    return JXLHIP_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < 17; k++)
    if (size_t(d->dequant_offset[k]) + 3 * size_t(d->dequant_size[k]) > d->dequant_floats) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (d->strategy_mode >= 2) {  // the search: the adaptive field, a size the walk takes, a table of the right size for every kind it estimates
    if (d->quant_field_mode != 1 || !std::isfinite(d->distance) || !jxh::AcsWalkSizeOk((d->xsize + 7) / 8, (d->ysize + 7) / 8)) return JXLHIP_ERR_INVALID_ARGUMENT;
    for (uint32_t k = 0; k < jxh::kAcsWalkKinds; k++) {
      uint32_t cx = 0, cy = 0, dq_kind = 0;
      jxh::EncEstimateShape(jxh::AcsWalkStrategy(k), &cx, &cy, &dq_kind);
      if (d->dequant_size[dq_kind] != cx * cy * 64) return JXLHIP_ERR_INVALID_ARGUMENT;
    }
  }
  HIP_TRY(hipSetDevice(c->device));
  jxlhip::EncFwd P;
  memset(&P, 0, sizeof(P));
  P.xs = d->xsize;
  P.ys = d->ysize;
  P.xb = (P.xs + 7) / 8;
  P.yb = (P.ys + 7) / 8;
  P.xp = P.xb * 8;
  P.yp = P.yb * 8;
  P.xg = (P.xs + 255) / 256;
  P.yg = (P.ys + 255) / 256;
  const size_t nb = size_t(P.xb) * P.yb, plane = size_t(P.xp) * P.yp, ng = size_t(P.xg) * P.yg;
  int r;
  if ((r = c->enc_rgb.Ensure(stride * P.ys)) || (r = c->enc_act.Ensure(nb * 4)) || (r = c->enc_acs.Ensure(nb)) || (r = c->enc_qf.Ensure(nb * 4)) ||
      (r = c->enc_off.Ensure(nb * 4)) || (r = c->enc_dc.Ensure(3 * nb * 4)) || (r = c->enc_coef.Ensure(ng * 3 * 65536 * 4)) ||
      (r = c->enc_lut.Ensure(256 * 4)) || (r = c->enc_dq.Ensure(size_t(d->dequant_floats) * 4)))
    return r;
  const size_t ntiles = size_t((P.xb + 7) / 8) * ((P.yb + 7) / 8);
  if ((r = c->enc_ytox.Ensure(ntiles)) || (r = c->enc_ytob.Ensure(ntiles))) return r;
  if (d->cfl_fit && getenv("JXLHIP_ENC_BLOCK_KERNEL")) return JXLHIP_ERR_UNSUPPORTED;  // (the tile kernel makes the fit)
  for (auto& b : c->enc_planes)
    if ((r = b.Ensure(3 * plane * 4))) return r;
  for (auto& ev : c->enc_ev)
    if (!ev) HIP_TRY(hipEventCreate(&ev));
  float lut[256];
  for (int i = 0; i < 256; i++) lut[i] = jxh::SrgbEotf8(i);
  HIP_TRY(hipMemcpyAsync(c->enc_lut.p, lut, sizeof(lut), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->enc_dq.p, d->dequant, size_t(d->dequant_floats) * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->enc_rgb.p, rgb, stride * P.ys, hipMemcpyHostToDevice, c->stream));
  P.rgb = c->enc_rgb.as<uint8_t>();
  P.rgb_stride = stride;
  P.srgb_lut = c->enc_lut.as<float>();
  P.act = c->enc_act.as<float>();
  P.acs = c->enc_acs.as<uint8_t>();
  P.qf = c->enc_qf.as<int32_t>();
  P.coef_off = c->enc_off.as<uint32_t>();
  P.basis_t = c->basis.as<float>() + kBasisTransposed;
  P.dequant = c->enc_dq.as<float>();
  memcpy(P.dq_offset, d->dequant_offset, sizeof(P.dq_offset));
  memcpy(P.dq_size, d->dequant_size, sizeof(P.dq_size));
  P.dc = c->enc_dc.as<int32_t>();
  P.coeffs = c->enc_coef.as<int32_t>();
  P.distance = d->distance;
  P.quant_ac = d->quant_ac;
  P.inv_gs = 65536.0f / float(d->global_scale);
  P.x_dm = jxh::EncXDm();
  P.b_dm = jxh::EncBDm();
  const float inv_quant_dc = P.inv_gs / float(d->quant_dc);
  P.dc_step[0] = inv_quant_dc / 4096.0f;
  P.dc_step[1] = inv_quant_dc / 512.0f;
  P.dc_step[2] = inv_quant_dc / 256.0f;
  P.strategy_mode = d->strategy_mode;
  P.cfl_fit = d->cfl_fit ? 1 : 0;
  P.scale = float(d->global_scale) / 65536.0f;
  P.ytox = c->enc_ytox.as<int8_t>();
  P.ytob = c->enc_ytob.as<int8_t>();
  P.quant_field_mode = d->quant_field_mode;
  if (P.quant_field_mode) {
    jxlhip::EncAq& A = c->enc_last_aq;
    // enc_heuristics.cc:1119-1122: the field's distance is 0.62 of the frame's without Gaborish; rescale 1
    jxh::EncAqDistanceParams(d->gaborish ? d->distance : d->distance * 0.62f, 1.0f, &A);
    P.mean_max_mixer = jxh::EncMeanMaxMixer(d->distance);
  }
  HIP_TRY(hipMemsetAsync(c->enc_ytox.p, 0, ntiles, c->stream));
  HIP_TRY(hipMemsetAsync(c->enc_ytob.p, 0, ntiles, c->stream));
  if (P.strategy_mode >= 2 && (r = EncSearchPrepare(c, P, P.strategy_mode - 2))) return r;
  HIP_TRY(hipEventRecord(c->enc_ev[0], c->stream));
  if ((r = EncLaunch(c, P, d->gaborish != 0))) return r;
  c->enc_last = P;
  c->enc_last_gaborish = d->gaborish != 0;
  HIP_TRY(hipEventRecord(c->enc_ev[1], c->stream));
  c->enc_timed = true;
  if (d->ytox) HIP_TRY(hipMemcpyAsync(d->ytox, c->enc_ytox.p, ntiles, hipMemcpyDeviceToHost, c->stream));
  if (d->ytob) HIP_TRY(hipMemcpyAsync(d->ytob, c->enc_ytob.p, ntiles, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(acs, c->enc_acs.p, nb, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(qf, c->enc_qf.p, nb * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(dc, c->enc_dc.p, 3 * nb * 4, hipMemcpyDeviceToHost, c->stream));
  if (coeffs) HIP_TRY(hipMemcpyAsync(coeffs, c->enc_coef.p, ng * 3 * 65536 * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->enc_tok_ready = false;
  c->ent_resident = c->ent_sized = false;
  return 0;
}

// ---- tokenisation of the last forward call's coefficients (jxl_hip_enc.h)
int jxlhip_enc_token_counts(JxlHipContext* c, const JxlHipEncTokDesc* d, uint32_t* totals) {
  if (!c || !d || !totals || !d->orders || !d->num_ctxs || !d->num_hist || d->num_ctxs > 16) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->enc_timed) return JXLHIP_ERR_NO_FRAME;
  // every index the kernels form from the tables must stay inside them: the order buckets of the transforms the forward
  // path selects (up to 64x64), complete and with entries below their size; block contexts below num_ctxs
  static const uint32_t kBucketSize[9] = {64, 64, 256, 1024, 128, 256, 512, 4096, 2048};
  for (int b = 0; b < 9; b++) {
    if (uint64_t(d->order_offset[b]) + kBucketSize[b] > d->orders_size) return JXLHIP_ERR_INVALID_ARGUMENT;
    for (uint32_t k = 0; k < kBucketSize[b]; k++)
      if (d->orders[d->order_offset[b] + k] >= kBucketSize[b]) return JXLHIP_ERR_INVALID_ARGUMENT;
  }
  for (int i = 0; i < 39; i++)
    if (d->ctx_map[i] >= d->num_ctxs) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  const jxlhip::EncFwd& F = c->enc_last;
  const size_t ng = size_t(F.xg) * F.yg;
  int r;
  if ((r = c->enc_tok_orders.Ensure(size_t(d->orders_size) * 2 + 16)) || (r = c->enc_tok_blk.Ensure(ng * 1024 * 2)) ||
      (r = c->enc_tok_info.Ensure(ng * jxlhip::kTokPerGroup * 4)) || (r = c->enc_tok_off.Ensure(ng * jxlhip::kTokPerGroup * 4)) ||
      (r = c->enc_tok_nzmap.Ensure(ng * 3 * 1024)) || (r = c->enc_tok_small.Ensure(ng * 12)))
    return r;
  HIP_TRY(hipMemcpyAsync(c->enc_tok_orders.p, d->orders, size_t(d->orders_size) * 2, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->enc_tok_nzmap.p, 0, ng * 3 * 1024, c->stream));
  jxlhip::EncTok& T = c->enc_tok;
  memset(&T, 0, sizeof(T));
  T.acs = F.acs;
  T.coef_off = F.coef_off;
  T.coeffs = F.coeffs;
  T.xb = F.xb;
  T.yb = F.yb;
  T.xg = F.xg;
  T.orders = c->enc_tok_orders.as<uint16_t>();
  memcpy(T.order_offset, d->order_offset, sizeof(T.order_offset));
  memcpy(T.ctx_map, d->ctx_map, sizeof(T.ctx_map));
  T.num_ctxs = d->num_ctxs;
  T.num_hist = d->num_hist;
  T.nctx = d->num_ctxs * 495;
  T.blk = c->enc_tok_blk.as<uint16_t>();
  T.info = c->enc_tok_info.as<uint32_t>();
  T.off = c->enc_tok_off.as<uint32_t>();
  T.nzmap = c->enc_tok_nzmap.as<uint8_t>();
  T.nblk = c->enc_tok_small.as<uint32_t>();
  T.total = c->enc_tok_small.as<uint32_t>() + ng;
  hipLaunchKernelGGL(jxlhip::k_enc_tok_count, dim3(uint32_t(ng)), dim3(jxlhip::kTokThreads), 0, c->stream, T);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(totals, T.total, ng * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->enc_tok_totals.assign(totals, totals + ng);
  c->enc_tok_ready = true;
  return 0;
}

int jxlhip_enc_tokens(JxlHipContext* c, const uint32_t* bases, uint32_t* tokens, size_t capacity) {
  if (!c || !bases) return JXLHIP_ERR_INVALID_ARGUMENT;  // (tokens == NULL: they stay on the device, for the entropy calls)
  if (!c->enc_tok_ready) return JXLHIP_ERR_NO_FRAME;
  const size_t ng = c->enc_tok_totals.size();
  uint64_t need = 0;
  for (size_t g = 0; g < ng; g++) {  // every group's range inside the caller's buffer (ranges may not overlap: they are a prefix sum)
    if (uint64_t(bases[g]) + c->enc_tok_totals[g] > capacity) return JXLHIP_ERR_INVALID_ARGUMENT;
    need = std::max<uint64_t>(need, uint64_t(bases[g]) + c->enc_tok_totals[g]);
  }
  HIP_TRY(hipSetDevice(c->device));
  int r;
  if ((r = c->enc_tok_out.Ensure(size_t(need ? need : 1) * 8)) || (r = c->enc_tok_base.Ensure(ng * 4))) return r;
  HIP_TRY(hipMemcpyAsync(c->enc_tok_base.p, bases, ng * 4, hipMemcpyHostToDevice, c->stream));
  jxlhip::EncTok T = c->enc_tok;
  T.base = c->enc_tok_base.as<uint32_t>();
  T.tokens = c->enc_tok_out.as<uint2>();
  hipLaunchKernelGGL(jxlhip::k_enc_tok_emit, dim3(uint32_t(ng)), dim3(jxlhip::kTokThreads), 0, c->stream, T);
  HIP_TRY(hipGetLastError());
  if (tokens) HIP_TRY(hipMemcpyAsync(tokens, c->enc_tok_out.p, size_t(need) * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->ent_base.assign(bases, bases + ng);
  c->ent_count = c->enc_tok_totals;
  c->ent_resident = true;
  c->ent_sized = false;
  return 0;
}

// ---- entropy coding of the resident tokens (jxl_hip_enc.h)
namespace {
// What both passes start with: the groups' token counts on the device, the events, the token side of the parameters.
int EntBegin(JxlHipContext* c, jxlhip::EncAns* A, uint32_t* blocks) {
  const size_t ng = c->ent_base.size();
  int r;
  if ((r = c->ent_grp.Ensure(ng * 4))) return r;
  for (auto& ev : c->ent_ev)
    if (!ev) HIP_TRY(hipEventCreate(&ev));
  HIP_TRY(hipMemcpyAsync(c->ent_grp.p, c->ent_count.data(), ng * 4, hipMemcpyHostToDevice, c->stream));
  memset(A, 0, sizeof(*A));
  A->tokens = c->enc_tok_out.as<uint2>();
  A->base = c->enc_tok_base.as<uint32_t>();
  A->count = c->ent_grp.as<uint32_t>();
  uint32_t most = 0;
  for (uint32_t n : c->ent_count) most = std::max(most, n);
  // (per-token kernels: blocks per group so that a thread takes about sixteen tokens)
  *blocks = std::max(1u, std::min(32u, (most + jxlhip::kAnsThreads * 16 - 1) / (jxlhip::kAnsThreads * 16)));
  return 0;
}
bool HybridOk(uint32_t split_exp, uint32_t msb, uint32_t lsb) { return split_exp <= 8 && msb + lsb <= split_exp; }
}  // namespace

int jxlhip_enc_histograms(JxlHipContext* c, const JxlHipEncHistDesc* d, uint32_t* counts, uint32_t* max_token) {
  if (!c || !d || !counts || !max_token || !d->num_ctx || d->num_ctx > (1u << 20) || !HybridOk(d->split_exp, d->msb_in_token, d->lsb_in_token))
    return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->ent_resident) return JXLHIP_ERR_NO_FRAME;
  HIP_TRY(hipSetDevice(c->device));
  const size_t ng = c->ent_base.size(), bytes = size_t(d->num_ctx) * 256 * 4;
  jxlhip::EncAns A;
  uint32_t blocks;
  int r;
  if ((r = EntBegin(c, &A, &blocks)) || (r = c->ent_counts.Ensure(bytes)) || (r = c->ent_status.Ensure(8))) return r;
  HIP_TRY(hipMemsetAsync(c->ent_counts.p, 0, bytes, c->stream));
  HIP_TRY(hipMemsetAsync(c->ent_status.p, 0, 8, c->stream));
  A.split_exp = d->split_exp;
  A.msb = d->msb_in_token;
  A.lsb = d->lsb_in_token;
  A.num_ctx = d->num_ctx;
  A.counts = c->ent_counts.as<uint32_t>();
  A.status = c->ent_status.as<uint32_t>();
  HIP_TRY(hipEventRecord(c->ent_ev[0], c->stream));
  hipLaunchKernelGGL(jxlhip::k_enc_hist, dim3(blocks, uint32_t(ng)), dim3(jxlhip::kAnsThreads), 0, c->stream, A);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ent_ev[1], c->stream));
  c->ent_timed[0] = true;
  uint32_t status[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(counts, c->ent_counts.p, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(status, c->ent_status.p, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *max_token = status[0];
  return (status[1] || status[0] >= 256) ? JXLHIP_ERR_INVALID_ARGUMENT : 0;
}

int jxlhip_enc_ans_sizes(JxlHipContext* c, const JxlHipEncAnsDesc* d, uint32_t* bit_counts) {
  if (!c || !d || !bit_counts || !d->ctx_map || !d->freq || !d->rev_start || !d->rev || !d->prefix_count || !d->prefix_value || !d->num_ctx ||
      d->num_ctx > (1u << 20) || !d->num_clusters || d->num_clusters > 256 || d->log_alpha < 5 || d->log_alpha > 8 ||
      !HybridOk(d->split_exp, d->msb_in_token, d->lsb_in_token))
    return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->ent_resident) return JXLHIP_ERR_NO_FRAME;
  c->ent_sized = false;
  // (every index the kernels form from the tables stays inside them)
  if (!jxh::AnsTablesInBounds(*d)) return JXLHIP_ERR_INVALID_ARGUMENT;
  const size_t ng = c->ent_base.size(), K = d->num_clusters;
  uint64_t need = 0;
  for (size_t g = 0; g < ng; g++) {
    if (d->prefix_count[g] > 8) return JXLHIP_ERR_INVALID_ARGUMENT;
    need = std::max<uint64_t>(need, uint64_t(c->ent_base[g]) + c->ent_count[g]);
  }
  HIP_TRY(hipSetDevice(c->device));
  // the tables in one block: ctx_map | freq | rev_start | rev | prefix_count | prefix_value, each 16-byte aligned
  auto up16 = [](size_t v) { return (v + 15) & ~size_t(15); };
  const size_t o_freq = up16(d->num_ctx), o_start = o_freq + K * 512, o_rev = o_start + K * 512, o_pc = o_rev + K * 8192, o_pv = o_pc + up16(ng),
               tab_bytes = o_pv + up16(ng);
  jxlhip::EncAns& A = c->ent;
  uint32_t blocks;
  int r;
  if ((r = EntBegin(c, &A, &blocks)) || (r = c->ent_tab.Ensure(tab_bytes)) || (r = c->ent_rec.Ensure(size_t(need ? need : 1) * 4)) ||
      (r = c->ent_fl.Ensure(size_t(need ? need : 1) * 4)) || (r = c->ent_small.Ensure(ng * 12)))
    return r;
  uint8_t* tab = c->ent_tab.as<uint8_t>();
  HIP_TRY(hipMemcpyAsync(tab, d->ctx_map, d->num_ctx, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(tab + o_freq, d->freq, K * 512, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(tab + o_start, d->rev_start, K * 512, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(tab + o_rev, d->rev, K * 8192, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(tab + o_pc, d->prefix_count, ng, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(tab + o_pv, d->prefix_value, ng, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->ent_small.p, 0, ng * 12, c->stream));
  A.split_exp = d->split_exp;
  A.msb = d->msb_in_token;
  A.lsb = d->lsb_in_token;
  A.num_ctx = d->num_ctx;
  A.ctx_map = tab;
  A.freq = reinterpret_cast<const uint16_t*>(tab + o_freq);
  A.rev_start = reinterpret_cast<const uint16_t*>(tab + o_start);
  A.rev = reinterpret_cast<const uint16_t*>(tab + o_rev);
  A.prefix_count = tab + o_pc;
  A.prefix_value = tab + o_pv;
  A.rec = c->ent_rec.as<uint32_t>();
  A.fl = c->ent_fl.as<uint32_t>();
  A.state = c->ent_small.as<uint32_t>();
  A.bits = A.state + ng;
  A.err = A.state + 2 * ng;
  HIP_TRY(hipEventRecord(c->ent_ev[2], c->stream));
  hipLaunchKernelGGL(jxlhip::k_enc_ans_records, dim3(blocks, uint32_t(ng)), dim3(jxlhip::kAnsThreads), 0, c->stream, A);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(jxlhip::k_enc_ans_chain, dim3(uint32_t(ng)), dim3(64), 0, c->stream, A);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ent_ev[3], c->stream));
  c->ent_timed[1] = true;
  c->ent_timed[2] = false;
  std::vector<uint32_t> back(2 * ng);
  HIP_TRY(hipMemcpyAsync(back.data(), A.bits, ng * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t g = 0; g < ng; g++)
    if (back[ng + g]) return JXLHIP_ERR_INVALID_ARGUMENT;  // a token this code cannot code (context, alphabet or a zero frequency)
  c->ent_bits.assign(back.begin(), back.begin() + ng);
  memcpy(bit_counts, back.data(), ng * 4);
  c->ent_sized = true;
  return 0;
}

int jxlhip_enc_ans_write(JxlHipContext* c, const uint64_t* byte_bases, uint8_t* out, size_t capacity) {
  if (!c || !byte_bases || !out) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->ent_resident || !c->ent_sized) return JXLHIP_ERR_NO_FRAME;
  const size_t ng = c->ent_base.size();
  uint64_t end = 0;
  for (size_t g = 0; g < ng; g++) {  // every group's range inside the caller's buffer (they may not overlap: a prefix sum)
    const uint64_t bytes = (uint64_t(c->ent_bits[g]) + 7) / 8;
    if (byte_bases[g] > capacity || bytes > capacity - byte_bases[g]) return JXLHIP_ERR_INVALID_ARGUMENT;
    end = std::max(end, byte_bases[g] + bytes);
  }
  HIP_TRY(hipSetDevice(c->device));
  const size_t words = size_t((end + 3) / 4) + 2;  // (a token's bits reach into at most the word its last bit is in)
  int r;
  if ((r = c->ent_out.Ensure(words * 4)) || (r = c->ent_obase.Ensure(ng * 8))) return r;
  HIP_TRY(hipMemsetAsync(c->ent_out.p, 0, words * 4, c->stream));
  HIP_TRY(hipMemcpyAsync(c->ent_obase.p, byte_bases, ng * 8, hipMemcpyHostToDevice, c->stream));
  jxlhip::EncAns A = c->ent;
  A.out_base = c->ent_obase.as<uint64_t>();
  A.out = c->ent_out.as<uint32_t>();
  HIP_TRY(hipEventRecord(c->ent_ev[4], c->stream));
  hipLaunchKernelGGL(jxlhip::k_enc_ans_scatter, dim3(uint32_t(ng)), dim3(jxlhip::kAnsThreads), 0, c->stream, A);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ent_ev[5], c->stream));
  c->ent_timed[2] = true;
  if (end) HIP_TRY(hipMemcpyAsync(out, c->ent_out.p, size_t(end), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int jxlhip_debug_ans_write(JxlHipContext* c, const uint32_t* tokens, size_t n, const JxlHipEncAnsDesc* d, uint8_t* out, size_t capacity,
                           uint64_t* bits) {
  if (!c || (!tokens && n) || !d || !out || !bits || n >= (size_t(1) << 28)) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  int r;
  if ((r = c->enc_tok_out.Ensure((n ? n : 1) * 8)) || (r = c->enc_tok_base.Ensure(4))) return r;
  if (n) HIP_TRY(hipMemcpyAsync(c->enc_tok_out.p, tokens, n * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->enc_tok_base.p, 0, 4, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->enc_tok_ready = false;  // (the resident tokens are no longer those of the last jxlhip_enc_token_counts)
  c->ent_base.assign(1, 0);
  c->ent_count.assign(1, uint32_t(n));
  c->ent_resident = true;
  c->ent_sized = false;
  uint32_t nbits = 0;
  if ((r = jxlhip_enc_ans_sizes(c, d, &nbits))) return r;
  *bits = nbits;
  const uint64_t base = 0;
  return jxlhip_enc_ans_write(c, &base, out, capacity);
}

int jxlhip_enc_entropy_last_ms(JxlHipContext* c, float* ms) {
  if (!c || !ms) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  float t[3] = {0, 0, 0};
  for (int i = 0; i < 3; i++)
    if (c->ent_timed[i]) {
      HIP_TRY(hipEventSynchronize(c->ent_ev[2 * i + 1]));
      HIP_TRY(hipEventElapsedTime(&t[i], c->ent_ev[2 * i], c->ent_ev[2 * i + 1]));
    }
  ms[0] = t[0];
  ms[1] = t[1] + t[2];
  return 0;
}

int jxlhip_enc_initial_quant_field(JxlHipContext* c, const float* xyb, uint32_t xsize, uint32_t ysize, float butteraugli_target, float rescale,
                                   float* aq_map, float* mask) {
  if (!c || !xyb || !aq_map || !xsize || !ysize || (xsize & 7) || (ysize & 7) || xsize > (1u << 18) || ysize > (1u << 18))
    return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!(butteraugli_target > 0) || !(rescale > 0) || !std::isfinite(butteraugli_target) || !std::isfinite(rescale)) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  jxlhip::EncAq A;  // (its own planes and parameters: the last forward call's stay what jxlhip_enc_forward_rerun replays)
  memset(&A, 0, sizeof(A));
  const size_t plane = size_t(xsize) * ysize, nb = plane / 64;
  int r;
  if ((r = c->enc_aq_in.Ensure(3 * plane * 4)) || (r = EncAqEnsure(c, xsize, ysize, &A))) return r;
  jxh::EncAqDistanceParams(butteraugli_target, rescale, &A);
  A.planes = c->enc_aq_in.as<float>();
  HIP_TRY(hipMemcpyAsync(c->enc_aq_in.p, xyb, 3 * plane * 4, hipMemcpyHostToDevice, c->stream));
  EncAqLaunch(c, A);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(aq_map, A.aq, nb * 4, hipMemcpyDeviceToHost, c->stream));
  if (mask) HIP_TRY(hipMemcpyAsync(mask, A.mask, nb * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int jxlhip_enc_masking_1x1(JxlHipContext* c, const float* xyb, uint32_t xsize, uint32_t ysize, float* out) {
  if (!c || !xyb || !out || !xsize || !ysize || (xsize & 7) || (ysize & 7) || xsize > (1u << 18) || ysize > (1u << 18))
    return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  const size_t plane = size_t(xsize) * ysize;
  int r;
  if ((r = c->enc_aq_in.Ensure(plane * 4)) || (r = c->enc_mask1x1.Ensure(plane * 4))) return r;
  for (auto& ev : c->mask_ev)
    if (!ev) HIP_TRY(hipEventCreate(&ev));
  jxlhip::EncMask1x1 M;
  M.y = c->enc_aq_in.as<float>();
  M.out = c->enc_mask1x1.as<float>();
  M.xp = xsize;
  M.yp = ysize;
  jxh::EncMask1x1Weights(M.w);
  HIP_TRY(hipMemcpyAsync(c->enc_aq_in.p, xyb + plane, plane * 4, hipMemcpyHostToDevice, c->stream));  // (the Y plane is all it reads)
  HIP_TRY(hipEventRecord(c->mask_ev[0], c->stream));
  hipLaunchKernelGGL(jxlhip::k_enc_mask1x1, dim3((xsize + jxlhip::kMaskCols - 1) / jxlhip::kMaskCols, (ysize + jxlhip::kMaskRows - 1) / jxlhip::kMaskRows),
                     dim3(256), 0, c->stream, M);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->mask_ev[1], c->stream));
  c->mask_timed = true;
  HIP_TRY(hipMemcpyAsync(out, M.out, plane * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int jxlhip_enc_masking_last_ms(JxlHipContext* c, float* ms) {
  if (!c || !ms) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->mask_timed) return JXLHIP_ERR_NO_FRAME;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->mask_ev[1]));
  HIP_TRY(hipEventElapsedTime(ms, c->mask_ev[0], c->mask_ev[1]));
  return 0;
}

// The cost estimate of the AC-strategy search (k_enc_estimate, jxl_hip_enc.h). Everything is checked here, on the host
// (jxh::EncEstimateArgsOk: every candidate inside the planes and one tile, every table of the right size); the candidates are
// sorted by strategy (stable) and each strategy present is one launch of the form its size asks for.
int jxlhip_enc_estimate_entropy(JxlHipContext* c, const JxlHipEncEstimateDesc* d, const JxlHipEncAcsCandidate* cand, size_t n, float* estimates,
                                float* scaled) {
  size_t total_area = 0;
  if (!c || !jxh::EncEstimateArgsOk(d, cand, n, estimates, &total_area) || n > (size_t(1) << 30)) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  for (auto& ev : c->est_ev)
    if (!ev) HIP_TRY(hipEventCreate(&ev));
  if (!n) {
    HIP_TRY(hipEventRecord(c->est_ev[0], c->stream));
    HIP_TRY(hipEventRecord(c->est_ev[1], c->stream));
    c->est_timed = true;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
  }
  const uint32_t xb = d->xsize / 8, yb = d->ysize / 8, tiles_x = (xb + 7) / 8, tiles_y = (yb + 7) / 8;
  const size_t plane = size_t(d->xsize) * d->ysize, nb = size_t(xb) * yb, ntiles = size_t(tiles_x) * tiles_y;
  // the candidates in launch order: by strategy, the caller's order inside one
  std::vector<uint32_t> index(n);
  for (size_t i = 0; i < n; i++) index[i] = uint32_t(i);
  std::stable_sort(index.begin(), index.end(), [&](uint32_t a, uint32_t b) { return cand[a].strategy < cand[b].strategy; });
  std::vector<JxlHipEncAcsCandidate> sorted(n);
  std::vector<unsigned long long> start(n + 1, 0), at(n);
  for (size_t i = 0; i < n; i++) {
    uint32_t cx = 0, cy = 0, kind = 0;
    jxh::EncEstimateShape(cand[i].strategy, &cx, &cy, &kind);
    start[i + 1] = start[i] + 3ull * cx * cy * 64;
  }
  for (size_t i = 0; i < n; i++) {
    sorted[i] = cand[index[i]];
    at[i] = start[index[i]];
  }
  int r;
  if ((r = c->est_planes.Ensure(3 * plane * 4)) || (r = c->est_qf.Ensure(nb * 4)) || (r = c->est_mask.Ensure(plane * 4)) ||
      (r = c->est_ytox.Ensure(ntiles)) || (r = c->est_ytob.Ensure(ntiles)) || (r = c->est_dq.Ensure(size_t(d->dequant_floats) * 4)) ||
      (r = c->est_cand.Ensure(n * sizeof(JxlHipEncAcsCandidate))) || (r = c->est_index.Ensure(n * 4)) || (r = c->est_at.Ensure(n * 8)) ||
      (r = c->est_out.Ensure(n * 4)) || (scaled && (r = c->est_scaled.Ensure(3 * total_area * 4))))
    return r;
  HIP_TRY(hipMemcpyAsync(c->est_planes.p, d->xyb, 3 * plane * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->est_qf.p, d->quant_field, nb * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->est_mask.p, d->mask1x1, plane * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->est_ytox.p, d->ytox, ntiles, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->est_ytob.p, d->ytob, ntiles, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->est_dq.p, d->dequant, size_t(d->dequant_floats) * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->est_cand.p, sorted.data(), n * sizeof(JxlHipEncAcsCandidate), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->est_index.p, index.data(), n * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->est_at.p, at.data(), n * 8, hipMemcpyHostToDevice, c->stream));
  jxlhip::EncEstimate P;
  memset(&P, 0, sizeof(P));
  P.planes = c->est_planes.as<float>();
  P.quant = c->est_qf.as<float>();
  P.mask = c->est_mask.as<float>();
  P.ytox = c->est_ytox.as<int8_t>();
  P.ytob = c->est_ytob.as<int8_t>();
  P.basis_t = c->basis.as<float>() + kBasisTransposed;
  P.estimates = c->est_out.as<float>();
  P.scaled = scaled ? c->est_scaled.as<float>() : nullptr;
  P.xp = d->xsize;
  P.yp = d->ysize;
  P.xb = xb;
  P.tiles_x = tiles_x;
  jxh::EncEstimateWeights(d->distance, P.weights);
  jxh::EncEstimateChannelMul(P.channel_mul);
  HIP_TRY(hipEventRecord(c->est_ev[0], c->stream));
  for (size_t first = 0; first < n;) {
    size_t last = first;
    while (last < n && sorted[last].strategy == sorted[first].strategy) last++;
    uint32_t kind = 0;
    jxh::EncEstimateShape(sorted[first].strategy, &P.cx, &P.cy, &kind);
    P.dequant = c->est_dq.as<float>() + d->dequant_offset[kind];
    P.cand = c->est_cand.as<JxlHipEncAcsCandidate>() + first;
    P.index = c->est_index.as<uint32_t>() + first;
    P.scaled_at = c->est_at.as<unsigned long long>() + first;
    P.n = uint32_t(last - first);
    P.x_weight = P.cx * P.cy >= 2 ? jxh::EncEstimateXWeight(P.cx * P.cy) : 1.0f;
    const uint32_t area = P.cx * P.cy * 64;
    if (area < 1024) hipLaunchKernelGGL((jxlhip::k_enc_estimate<64, 1>), dim3((P.n + 3) / 4), dim3(256), 0, c->stream, P);
    else if (area == 1024) hipLaunchKernelGGL((jxlhip::k_enc_estimate<256, 4>), dim3(P.n), dim3(256), 0, c->stream, P);
    else hipLaunchKernelGGL((jxlhip::k_enc_estimate<256, 8>), dim3(P.n), dim3(256), 0, c->stream, P);
    HIP_TRY(hipGetLastError());
    first = last;
  }
  HIP_TRY(hipEventRecord(c->est_ev[1], c->stream));
  c->est_timed = true;
  HIP_TRY(hipMemcpyAsync(estimates, c->est_out.p, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (scaled) HIP_TRY(hipMemcpyAsync(scaled, c->est_scaled.p, 3 * total_area * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int jxlhip_enc_estimate_last_ms(JxlHipContext* c, float* ms) {
  if (!c || !ms) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->est_timed) return JXLHIP_ERR_NO_FRAME;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->est_ev[1]));
  HIP_TRY(hipEventElapsedTime(ms, c->est_ev[0], c->est_ev[1]));
  return 0;
}

// The merge walk alone (k_enc_acs_walk, jxl_hip_enc.h) on a caller's table; buffers of its own, so that the last forward
// call's search data and state stay what they were.
int jxlhip_enc_acs_walk(JxlHipContext* c, const JxlHipEncAcsWalkDesc* d, const float* estimates, uint8_t* acs, float* entropy) {
  if (!c || !jxh::AcsWalkArgsOk(d, estimates, acs)) return JXLHIP_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(c->device));
  const size_t nb = size_t(d->xb) * d->yb, tiles = size_t((d->xb + 7) / 8) * ((d->yb + 7) / 8);
  int r;
  if ((r = c->walk_table.Ensure(tiles * jxh::kAcsWalkTileFloats * 4)) || (r = c->walk_acs.Ensure(nb)) || (entropy && (r = c->walk_entropy.Ensure(nb * 4))))
    return r;
  HIP_TRY(hipMemcpyAsync(c->walk_table.p, estimates, tiles * jxh::kAcsWalkTileFloats * 4, hipMemcpyHostToDevice, c->stream));
  jxlhip::EncAcsWalk W;
  memset(&W, 0, sizeof(W));
  W.table = c->walk_table.as<float>();
  W.acs = c->walk_acs.as<uint8_t>();
  W.entropy = entropy ? c->walk_entropy.as<float>() : nullptr;
  W.xb = d->xb;
  W.yb = d->yb;
  W.floating = d->floating;
  W.mul8x8 = jxh::AcsWalkMul8x8(d->distance);
  hipLaunchKernelGGL(jxlhip::k_enc_acs_walk, dim3(uint32_t(tiles)), dim3(64), 0, c->stream, W);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(acs, c->walk_acs.p, nb, hipMemcpyDeviceToHost, c->stream));
  if (entropy) HIP_TRY(hipMemcpyAsync(entropy, c->walk_entropy.p, nb * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int jxlhip_enc_search_last_ms(JxlHipContext* c, float* ms) {
  if (!c || !ms) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->enc_timed || c->enc_last.strategy_mode < 2) return JXLHIP_ERR_NO_FRAME;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->srch_ev[4]));
  HIP_TRY(hipEventElapsedTime(&ms[0], c->srch_ev[0], c->srch_ev[1]));
  HIP_TRY(hipEventElapsedTime(&ms[1], c->srch_ev[2], c->srch_ev[3]));
  HIP_TRY(hipEventElapsedTime(&ms[2], c->srch_ev[3], c->srch_ev[4]));
  return 0;
}

int jxlhip_debug_enc_search(JxlHipContext* c, float* planes_before, float* planes_after, float* aq_map, float* mask1x1, float* estimates) {
  if (!c) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->enc_timed || c->enc_last.strategy_mode < 2) return JXLHIP_ERR_NO_FRAME;
  HIP_TRY(hipSetDevice(c->device));
  const jxlhip::EncFwd& F = c->enc_last;
  const size_t plane = size_t(F.xp) * F.yp, nb = size_t(F.xb) * F.yb, tiles = size_t((F.xb + 7) / 8) * ((F.yb + 7) / 8);
  const float* before = c->enc_last_gaborish ? c->enc_planes[2].as<float>() : c->enc_planes[0].as<float>();
  if (planes_before) HIP_TRY(hipMemcpyAsync(planes_before, before, 3 * plane * 4, hipMemcpyDeviceToHost, c->stream));
  if (planes_after) HIP_TRY(hipMemcpyAsync(planes_after, F.planes, 3 * plane * 4, hipMemcpyDeviceToHost, c->stream));
  if (aq_map) HIP_TRY(hipMemcpyAsync(aq_map, F.aq_map, nb * 4, hipMemcpyDeviceToHost, c->stream));
  if (mask1x1) HIP_TRY(hipMemcpyAsync(mask1x1, c->srch_mask.p, plane * 4, hipMemcpyDeviceToHost, c->stream));
  if (estimates) HIP_TRY(hipMemcpyAsync(estimates, c->srch_table.p, tiles * jxh::kAcsWalkTileFloats * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int jxlhip_enc_aq_last_ms(JxlHipContext* c, float* ms) {
  if (!c || !ms) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->enc_timed || !c->enc_last.quant_field_mode) return JXLHIP_ERR_NO_FRAME;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->enc_ev[5]));
  HIP_TRY(hipEventElapsedTime(ms, c->enc_ev[4], c->enc_ev[5]));
  return 0;
}

int jxlhip_enc_forward_rerun(JxlHipContext* c, uint32_t times) {
  if (!c || !times || times > 4096) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->enc_timed) return JXLHIP_ERR_NO_FRAME;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventRecord(c->enc_ev[0], c->stream));
  for (uint32_t i = 0; i < times; i++) {
    int r = EncLaunch(c, c->enc_last, c->enc_last_gaborish);
    if (r) return r;
  }
  HIP_TRY(hipEventRecord(c->enc_ev[1], c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int jxlhip_enc_last_ms(JxlHipContext* c, float* ms) {
  if (!c || !ms) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->enc_timed) return JXLHIP_ERR_NO_FRAME;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->enc_ev[1]));
  HIP_TRY(hipEventElapsedTime(ms, c->enc_ev[0], c->enc_ev[1]));
  return 0;
}

int jxlhip_enc_last_transform_ms(JxlHipContext* c, float* ms) {
  if (!c || !ms) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->enc_timed) return JXLHIP_ERR_NO_FRAME;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->enc_ev[3]));
  HIP_TRY(hipEventElapsedTime(ms, c->enc_ev[2], c->enc_ev[3]));
  return 0;
}

int jxlhip_last_stage_ms(JxlHipContext* c, int which, float* ms) {
  if (!c || !ms || which < 0 || which > 2) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!c->ev_valid[which]) return JXLHIP_ERR_NO_FRAME;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->ev[which * 2 + 1]));
  HIP_TRY(hipEventElapsedTime(ms, c->ev[which * 2], c->ev[which * 2 + 1]));
  return 0;
}

}  // extern "C"
