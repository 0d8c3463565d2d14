// libjxl_amd — the frame-level entry points of a region decode (include/jxl_amd.h "Region decode"): the window a box of the
// output needs, and its upload as a frame of its own. A file of its own like jxl_api_reduced.cc: it is the one caller of
// jxlhip_dc_window on the host side, so the CPU programs that build jxl_api.cc around "no device" doubles of the HIP layer
// need none for it. The plan is csrc/host/jxh_window_plan.h; the whole frame's descriptor comes from jxl_api.cc
// (jxlamd_internal::FillFrameDesc), where jxlamd_frame_upload_band fills it too.
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/jxl_amd.h"
#include "../host/jxh_window_plan.h"
#include "jxl_amd_frame.h"

extern "C" {

namespace {
namespace window = jxlhip::window;
// (the counts of the frame's size: a chroma-subsampled frame's blocks are whole MCUs, but its window is the whole frame)
window::FrameGeom GeomOfFrame(const jxh::FramePlan& P) { return window::GeomOf(uint32_t(P.dim.xsize), uint32_t(P.dim.ysize)); }
// What the parsed frame itself says of the whole-frame reasons (the descriptor's fields are derived from the same plan).
window::FrameTraits TraitsOfFrame(const jxh::FramePlan& P, uint32_t num_channels) {
  window::FrameTraits t;
  memset(&t, 0, sizeof(t));
  t.partial = P.reduced || !P.group_absent.empty();
  t.upsampling = P.fh.upsampling;
  for (int c = 0; c < 3; c++) t.subsampled = t.subsampled || P.fh.hshift[c] || P.fh.vshift[c];
  t.noise = P.has_noise;
  t.patches = P.has_patches && !P.patches.pos.empty();
  t.splines = P.has_splines;
  t.dc_frame = P.use_dc_frame;
  t.single_section = P.first_section_bit_offset != 0 || (P.dim.num_groups == 1 && P.fh.num_passes == 1);
  t.num_channels = num_channels;
  return t;
}
}  // namespace

size_t jxlamd_sizeof_window(void) { return sizeof(JxlAmdWindow); }

int jxlamd_frame_plan_window(const JxlAmdFrame* f, const uint32_t box[4], uint32_t num_channels, JxlAmdWindow* out) {
  jxlamd_internal::SetLastError("");
  if (!f || !box || !out || out->orientation > 8) {
    jxlamd_internal::SetLastError("invalid argument");
    return 1;
  }
  const jxh::FramePlan& P = f->plan;
  const window::FrameGeom g = GeomOfFrame(P);
  const uint32_t orientation = out->orientation ? out->orientation : 1;
  window::WindowPlan w;
  int rule = -1;
  // (an upsampled frame's image is larger than the frame: its box is no box of the frame, and its window the whole frame)
  const bool frame_is_image = P.fh.upsampling == 1;
  const window::Rect whole{0, 0, 0, 0};
  if (!frame_is_image) {  // (its box is held to the image's size all the same)
    window::WindowPlan unused;
    if (window::PlanWindow(window::GeomOf(uint32_t(P.ih.xsize), uint32_t(P.ih.ysize)), 0, 0, window::OrientBits(orientation),
                           window::Rect{box[0], box[1], box[2], box[3]}, &unused, &rule)) {
      jxlamd_internal::SetLastError("region decode: the box is refused (jxh_window_plan.h WindowRule " + std::to_string(rule) + ")");
      return 1;
    }
  }
  if (window::PlanWindow(g, P.fh.lf.gab, int(P.fh.lf.epf_iters), window::OrientBits(orientation),
                         frame_is_image ? window::Rect{box[0], box[1], box[2], box[3]} : whole, &w, &rule)) {
    jxlamd_internal::SetLastError("region decode: the box is refused (jxh_window_plan.h WindowRule " + std::to_string(rule) + ")");
    return 1;
  }
  const window::WholeFrameReason reason = window::WholeFrameReasonOf(TraitsOfFrame(P, num_channels), w);
  if (reason != window::kWindowed) {  // the whole frame, and the caller's own box
    window::PlanWindow(g, P.fh.lf.gab, int(P.fh.lf.epf_iters), window::OrientBits(orientation), whole, &w);
    w.box = window::Rect{box[0], box[1], box[2], box[3]};
  }
  memset(out, 0, sizeof(*out));
  out->orientation = orientation;
  out->x0 = w.pixels.x0; out->y0 = w.pixels.y0; out->xsize = w.pixels.xsize; out->ysize = w.pixels.ysize;
  out->gx0 = w.gx0; out->gy0 = w.gy0; out->gxs = w.gxs; out->gys = w.gys;
  out->box[0] = w.box.x0; out->box[1] = w.box.y0; out->box[2] = w.box.xsize; out->box[3] = w.box.ysize;
  out->groups_taken = w.groups_taken;
  out->groups_in_frame = w.groups_in_frame;
  out->reason = uint32_t(reason);
  return 0;
}

int jxlamd_frame_upload_window(const JxlAmdFrame* f, JxlHipContext* ctx, const JxlAmdWindow* win) {
  jxlamd_internal::SetLastError("");
  if (!f || !ctx || !win) {
    jxlamd_internal::SetLastError("invalid argument");
    return 1;
  }
  if (win->reason) return jxlamd_frame_upload(f, ctx);
  const jxh::FramePlan& P = f->plan;
  // the window again from its own rectangle: whole groups of this frame, fewer than all of them, of a frame that has windows
  const window::FrameGeom g = GeomOfFrame(P);
  window::WindowPlan w;
  memset(&w, 0, sizeof(w));
  const window::Rect r{win->x0, win->y0, win->xsize, win->ysize};
  const bool inside = r.xsize && r.ysize && uint64_t(r.x0) + r.xsize <= g.xsize && uint64_t(r.y0) + r.ysize <= g.ysize;
  if (inside) window::CoverWithGroups(g, r, &w);
  w.groups_taken = w.gxs * w.gys;
  w.groups_in_frame = g.xsize_groups * g.ysize_groups;
  if (!inside || !(w.pixels == r) || w.gx0 != win->gx0 || w.gy0 != win->gy0 || w.gxs != win->gxs || w.gys != win->gys ||
      window::WholeFrameReasonOf(TraitsOfFrame(P, 3), w) != window::kWindowed) {
    jxlamd_internal::SetLastError("region decode: the window is not one jxlamd_frame_plan_window made for this frame");
    return 1;
  }
  JxlHipFrameDesc whole;
  jxlamd_internal::FrameDescHold hold;
  if (jxlamd_internal::FillFrameDesc(f, &whole, &hold)) return 1;
  // 1. the window's DC image, from the apron of coded integers
  const window::Rect apron = window::PlanDcApron(w.blocks, g.xsize_blocks, g.ysize_blocks);
  std::vector<int32_t> apron_q(size_t(apron.xsize) * apron.ysize * 3);
  window::PackDcApron(P.dc_q.data(), g.xsize_blocks, g.ysize_blocks, apron, apron_q.data());
  JxlHipDcWindow dw;
  memset(&dw, 0, sizeof(dw));
  dw.frame_xsize_blocks = g.xsize_blocks; dw.frame_ysize_blocks = g.ysize_blocks;
  dw.win_x0 = w.blocks.x0; dw.win_y0 = w.blocks.y0; dw.win_xsize = w.blocks.xsize; dw.win_ysize = w.blocks.ysize;
  dw.apron_x0 = apron.x0; dw.apron_y0 = apron.y0; dw.apron_xsize = apron.xsize; dw.apron_ysize = apron.ysize;
  dw.apron = apron_q.data();
  dw.dc_extra_precision = P.dc_extra_precision.empty() ? nullptr : P.dc_extra_precision.data();
  dw.num_dc_groups = uint32_t(P.dc_extra_precision.size());
  memcpy(dw.dc_step, P.dc_step, sizeof(dw.dc_step));
  dw.dc_cfl_x = P.dc_cfl_x;
  dw.dc_cfl_b = P.dc_cfl_b;
  dw.dc_smoothing = P.dc_smoothing ? 1 : 0;
  int rc = jxlhip_dc_window(ctx, &dw);
  if (rc) {
    jxlamd_internal::SetLastError("jxlhip_dc_window failed (" + std::to_string(rc) + ")");
    return rc;
  }
  // 2. the window as a frame of its own
  window::WindowTables tables;
  JxlHipFrameDesc d;
  window::BuildWindowDesc(whole, w, jxlhip_dc_window_planes(ctx), &tables, &d);
  rc = jxlhip_frame_upload(ctx, &d);
  if (rc) jxlamd_internal::SetLastError("jxlhip_frame_upload failed (" + std::to_string(rc) + ")");
  return rc;
}

}  // extern "C"
