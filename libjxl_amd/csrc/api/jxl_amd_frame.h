// libjxl_amd — what a JxlAmdFrame (include/jxl_amd.h) holds, for the files of csrc/api that implement its entry points.
#ifndef JXL_AMD_FRAME_H_
#define JXL_AMD_FRAME_H_

#include <string>
#include <vector>

#include "../../../include/jxl_amd.h"
#include "../host/jxh_color.h"
#include "../host/jxh_frame.h"

struct JxlAmdFrame {
  jxh::FramePlan plan;
  jxh::ColorOutput color;  // the output encoding the decoder asks of an XYB frame (PrepareColorOutput)
  const uint8_t* data = nullptr;
  size_t size = 0;
  uint32_t coef_bits = 16;
  std::vector<JxlHipPassDesc> pass_desc;
};

namespace jxlamd_internal {
// jxlamd_last_error's text of the calling thread (it lives in jxl_api.cc).
void SetLastError(const std::string& text);
// The JxlHipFrameDesc of the whole frame (jxl_api.cc; the band fields stay 0). `hold` keeps what the descriptor points at
// beside the frame's own arrays. 0, or 1 with the thread's error text set.
struct FrameDescHold {
  std::vector<JxlHipPassDesc> pd;
  std::vector<float> ups_kernel;
};
int FillFrameDesc(const JxlAmdFrame* f, JxlHipFrameDesc* out, FrameDescHold* hold);
}  // namespace jxlamd_internal

#endif  // JXL_AMD_FRAME_H_
