// libjxl_amd — the frame-level entry point that hands a frame's DC image to the HIP layer as a reduced image
// (include/jxl_amd.h "Reduced decode"). A file of its own: it is the one caller of jxlhip_reduced_upload on the host side,
// so the CPU programs that build jxl_api.cc around "no device" doubles of the HIP layer need none for it. The parse
// (jxlamd_frame_dc_extent, jxlamd_frame_parse_reduced) is a mode of the one frame parser and lives with it in jxl_api.cc.
#include <cstring>
#include <string>

#include "../../../include/jxl_amd.h"
#include "../host/jxh_color.h"
#include "jxl_amd_frame.h"

extern "C" {

// The frame's DC image to a context as a reduced image: a frame parsed for it, or a whole frame (which holds the same DC).
int jxlamd_frame_upload_reduced(const JxlAmdFrame* f, JxlHipContext* ctx) {
  jxlamd_internal::SetLastError("");
  if (!f || !ctx) {
    jxlamd_internal::SetLastError("invalid argument");
    return 1;
  }
  const jxh::FramePlan& P = f->plan;
  // (a whole frame was not held to the reduced parse's rules when it was parsed: the same rules here)
  const jxh::FrameHeader& fh = P.fh;
  const char* why = nullptr;
  if (fh.frame_type != 0 || fh.custom_size || !fh.is_last || fh.blend.mode != 0) why = "it is not a regular, full-canvas, last frame that replaces the canvas";
  else if (P.use_dc_frame || P.dc_q.empty()) why = "it takes its DC image from a DC frame (kUseDcFrame)";
  else if (P.has_patches) why = "it has patches";
  else if (P.has_splines) why = "it has splines";
  else if (fh.upsampling != 1) why = "it is upsampled";
  else if (!fh.Is444()) why = "it is chroma-subsampled";
  else if (!P.ih.xyb_encoded) why = "the image is not XYB-encoded";
  else if (P.ih.have_preview) why = "it is a preview";
  if (why) {
    jxlamd_internal::SetLastError(std::string("reduced decode of a whole frame: ") + why);
    return 1;
  }
  JxlHipReducedDesc d;
  memset(&d, 0, sizeof(d));
  d.xsize_blocks = uint32_t(P.dim.xsize_blocks);
  d.ysize_blocks = uint32_t(P.dim.ysize_blocks);
  d.dc_quantised = P.dc_q.data();
  d.dc_extra_precision = P.dc_extra_precision.data();
  memcpy(d.dc_step, P.dc_step, sizeof(d.dc_step));
  d.dc_cfl_x = P.dc_cfl_x;
  d.dc_cfl_b = P.dc_cfl_b;
  d.dc_smoothing = P.dc_smoothing ? 1 : 0;
  // (the colour description of jxlamd_frame_upload_band)
  const jxh::ColorOutput& co = f->color;
  float own_matrix[9];
  jxh::OwnMatrix(P.ih, own_matrix);
  for (int i = 0; i < 9; i++) d.opsin_inv[i] = co.active ? co.matrix[i] : own_matrix[i];
  for (int c = 0; c < 3; c++) d.opsin_bias[c] = P.ih.opsin_bias[c];
  d.linear_output = (co.active ? co.linear : P.ih.linear_tf) ? 1 : 0;
  d.color_target = co.active && co.target.tf ? &co.target : nullptr;
  const int r = jxlhip_reduced_upload(ctx, &d);
  if (r) jxlamd_internal::SetLastError("jxlhip_reduced_upload failed (" + std::to_string(r) + ")");
  return r;
}

}  // extern "C"
