// The launch plan of the filter stage (jxlhip_run_filter_color_batch): host only, no HIP types.
//
// A frame's filter form (EPF iterations, Gaborish, the one-channel 8-bit writer, the tensor writer) picks its kernel. The
// frames of a set are grouped by form, a launch per group with one grid z slice per frame, sized for the group's largest
// frame. The tile kernel (k_filter_fused) takes 0 or 3 EPF iterations, the row-streaming kernel (k_filter_rows2) 1 or 2;
// the tile and strip sizes are the kernels' own (jxl_hip_filter_abi.h).
#ifndef JXH_FILTER_PLAN_H_
#define JXH_FILTER_PLAN_H_

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../../include/jxl_amd_hip.h"
#include "../hip/jxl_hip_filter_abi.h"

namespace jxh {
namespace filter_plan {

struct FilterForm {
  int epf;      // EPF iterations, 0..3
  bool gab;     // Gaborish
  bool grey;    // the one-channel 8-bit writer
  bool tensor;  // the writer into a caller's tensor
  // Groups are launched in ascending key order.
  int Key() const { return (tensor ? 16 : 0) + (grey ? 8 : 0) + (gab ? 4 : 0) + epf; }
};
inline FilterForm FormOf(int epf_iters, bool gab, bool grey, bool tensor) {
  return {epf_iters < 0 ? 0 : (epf_iters > 3 ? 3 : epf_iters), gab, grey, tensor};
}

enum FilterKernel : int { kNoKernel = 0, kFusedKernel, kRowsKernel };
// The row-streaming kernel has 1 or 2 EPF iterations, the tile kernel 0 or 3. Only the row-streaming kernel has the grey
// and the tensor writers: such a frame with 0 or 3 iterations has no kernel.
inline FilterKernel KernelOf(const FilterForm& f) {
  if (f.epf == 1 || f.epf == 2) return kRowsKernel;
  return f.grey || f.tensor ? kNoKernel : kFusedKernel;
}

struct FilterFrame {
  FilterForm form;
  uint32_t xs, band_rows;                      // columns, rows of the band to filter
  bool rgb, rgbf, filtered, linear_output;     // the frame writes 8-bit sRGB only: rgb && !rgbf && !filtered && !linear_output
};
struct FilterGroup {
  FilterForm form;
  uint32_t first, count;      // frames order[first .. first + count)
  uint32_t tiles_x, tiles_y;  // of the group's widest / tallest frame
  bool u8srgb;                // every frame of the group writes 8-bit sRGB only (k_filter_rows2<true>)
};
struct FilterPlan {
  std::vector<uint32_t> order;  // frames by form, frames of one form in the order given
  std::vector<FilterGroup> groups;
};

// 0, or JXLHIP_ERR_INVALID_ARGUMENT for a grey frame in a group that does not write 8-bit sRGB only: a one-channel frame
// has no other form to fall back to, every other writer would put three bytes per pixel into its rows.
inline int PlanFilterGroups(const FilterFrame* frames, size_t n, FilterPlan* plan) {
  plan->order.resize(n);
  std::iota(plan->order.begin(), plan->order.end(), 0u);
  std::stable_sort(plan->order.begin(), plan->order.end(), [frames](uint32_t a, uint32_t b) { return frames[a].form.Key() < frames[b].form.Key(); });
  plan->groups.clear();
  for (size_t j = 0; j < n; j++) {
    const FilterFrame& f = frames[plan->order[j]];
    if (plan->groups.empty() || plan->groups.back().form.Key() != f.form.Key()) plan->groups.push_back({f.form, uint32_t(j), 0, 0, 0, true});
    FilterGroup& g = plan->groups.back();
    g.count++;
    g.u8srgb = g.u8srgb && f.rgb && !f.rgbf && !f.filtered && !f.linear_output;
    if (f.form.grey && !g.u8srgb) return JXLHIP_ERR_INVALID_ARGUMENT;
    g.tiles_x = std::max(g.tiles_x, (f.xs + jxlhip::kFusedTW - 1) / jxlhip::kFusedTW);
    g.tiles_y = std::max(g.tiles_y, (f.band_rows + jxlhip::kFusedTH - 1) / jxlhip::kFusedTH);
  }
  return 0;
}

// Grid of the row-streaming kernel over `count` frames of at most tiles_x x tiles_y tiles: gx workgroups of kRowsWaves
// waves across, gy strips of `strip` rows down.
struct RowsGridDims {
  uint32_t gx, gy, strip;
};
inline RowsGridDims RowsGrid(uint32_t tiles_x, uint32_t tiles_y, uint32_t count) {
  const uint32_t cols = tiles_x * jxlhip::kFusedTW, rows = tiles_y * jxlhip::kFusedTH;  // upper bounds of the group
  RowsGridDims d;
  d.gx = ((cols + jxlhip::kRows2Cols - 1) / jxlhip::kRows2Cols + jxlhip::kRowsWaves - 1) / jxlhip::kRowsWaves;
  // strip height: every strip re-reads and re-filters 6 halo rows, so the taller the better as long as the launch still
  // has several waves for each of the chip's 1024 SIMDs (256 measured no better than 64: 0.0374 / 0.0361 / 0.0374 ms per 4K frame)
  d.strip = jxlhip::kRowsStrip;
  if (uint64_t(d.gx) * jxlhip::kRowsWaves * ((rows + 2 * d.strip - 1) / (2 * d.strip)) * count >= 6 * 1024) d.strip *= 2;
  d.gy = (rows + d.strip - 1) / d.strip;
  return d;
}

}  // namespace filter_plan
}  // namespace jxh

#endif  // JXH_FILTER_PLAN_H_
