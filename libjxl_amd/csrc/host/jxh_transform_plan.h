// The launch plan of the transform stage (jxlhip_run_transform_batch): host only, no HIP types.
//
// The varblocks of a set's frames are bucketed by strategy at upload (TransformParams::list_count). The strategies of
// the fast and special classes are launched once for the whole set: a workgroup reads a descriptor (frame, first varblock
// of the frame's list) and takes as many varblocks from there as its kernel handles. The 8x8 DCT varblocks of
// chroma-subsampled frames have a list of their own; such a frame's subsampled channels then go back to the frame's
// resolution; and the big class goes frame by frame through the frame's scratch. The kernels' sizes are their own
// (jxl_hip_transform_abi.h).
#ifndef JXH_TRANSFORM_PLAN_H_
#define JXH_TRANSFORM_PLAN_H_

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../hip/jxl_hip_transform_abi.h"

namespace jxh {
namespace transform_plan {

// What the plan needs of a frame.
struct TransformFrame {
  uint32_t list_count[jxlhip::kTransformStrategies];  // varblocks per strategy
  uint32_t cs;                                        // TransformParams::cs (0 = 4:4:4)
  uint32_t xs, ext_y0, ext_y1;                        // columns; the pixel rows the transforms produce
};

// One workgroup of a descriptor-list launch (the kernels read it as a uint2).
struct WorkgroupDesc {
  uint32_t frame, first;
};

enum LaunchKind : int { kListLaunch = 0, kChromaUpLaunch, kBigLaunch };
struct TransformLaunch {
  LaunchKind kind;
  uint32_t strategy;      // list and big launches
  uint32_t list;          // list launches: the descriptor list (the strategy, or kSubsampledList for strategy 0)
  uint32_t frame;         // chroma and big launches
  uint32_t first, count;  // list launches: descriptors [first, first + count); big: varblocks of the frame's list `strategy`
  uint32_t channel;       // chroma launches
  uint32_t grid_x, grid_y, block;
  size_t lds;
};
struct TransformPlan {
  std::vector<WorkgroupDesc> desc;
  std::vector<TransformLaunch> launches;
};

// Whether channel `ch` of a frame goes through k_chroma_upsample.
inline bool ChannelUpsamples(uint32_t cs, uint32_t ch) { return ((cs >> (2 * ch)) & 3u) != 0; }
// Whether descriptor list `list` holds varblocks of this frame: list 0 the 4:4:4 frames', kSubsampledList the others'.
inline bool ListTakesFrame(uint32_t list, uint32_t cs) { return list == jxlhip::kSubsampledList ? cs != 0 : (list != 0 || cs == 0); }
inline uint32_t StrategyOfList(uint32_t list) { return list == jxlhip::kSubsampledList ? 0 : list; }
inline uint32_t DivUp(uint32_t a, uint32_t b) { return a / b + (a % b != 0); }

// The launches in their order: the lists that have work; per subsampled frame, the channels to upsample (no rows, no
// launch); per frame and big strategy, chunks of kBigBlocksPerLaunch.
inline void PlanTransformLaunches(const TransformFrame* frames, size_t n, TransformPlan* plan) {
  using namespace jxlhip;
  size_t ndesc = 0, nlaunch = 0;
  for (uint32_t list = 0; list < kTransformLists; list++) {
    const uint32_t s = StrategyOfList(list), bpw = TransformBlocksPerWG(s);
    const size_t before = ndesc;
    for (size_t i = 0; i < n; i++)
      if (ListTakesFrame(list, frames[i].cs)) ndesc += DivUp(frames[i].list_count[s], bpw);
    nlaunch += ndesc != before;
  }
  for (size_t i = 0; i < n; i++) {
    if (frames[i].cs) nlaunch += 3;
    for (uint32_t s = kSubsampledList; s < kTransformStrategies; s++) nlaunch += DivUp(frames[i].list_count[s], kBigBlocksPerLaunch);
  }
  plan->desc.clear();
  plan->launches.clear();
  plan->desc.reserve(ndesc);
  plan->launches.reserve(nlaunch);

  for (uint32_t list = 0; list < kTransformLists; list++) {
    const uint32_t s = StrategyOfList(list), bpw = TransformBlocksPerWG(s);
    const uint32_t first = uint32_t(plan->desc.size());
    for (size_t i = 0; i < n; i++) {
      if (!ListTakesFrame(list, frames[i].cs)) continue;
      for (uint32_t j = 0; j < frames[i].list_count[s]; j += bpw) plan->desc.push_back({uint32_t(i), j});
    }
    const uint32_t count = uint32_t(plan->desc.size()) - first;
    if (!count) continue;
    const bool fast = TransformClassOf(s) == kFastClass;
    const int cx = kCoveredX[s], cy = kCoveredY[s];
    plan->launches.push_back({kListLaunch, s, list, 0, first, count, 0, count, 1, uint32_t(fast ? IdctFastThreads(cx, cy) : kSpecialThreads),
                              fast ? IdctFastLdsBytes(cx, cy) : 0});
  }
  for (size_t i = 0; i < n; i++) {
    const TransformFrame& f = frames[i];
    if (!f.cs || f.ext_y1 <= f.ext_y0) continue;
    for (uint32_t ch = 0; ch < 3; ch++)
      if (ChannelUpsamples(f.cs, ch))
        plan->launches.push_back({kChromaUpLaunch, 0, 0, uint32_t(i), 0, 0, ch, DivUp(f.xs, kChromaUpCols), DivUp(f.ext_y1 - f.ext_y0, kChromaUpRows),
                                  uint32_t(kChromaUpThreads), 0});
  }
  for (size_t i = 0; i < n; i++)
    for (uint32_t s = kSubsampledList; s < kTransformStrategies; s++)
      for (uint32_t j = 0; j < frames[i].list_count[s]; j += kBigBlocksPerLaunch) {
        const uint32_t m = frames[i].list_count[s] - j < kBigBlocksPerLaunch ? frames[i].list_count[s] - j : kBigBlocksPerLaunch;
        plan->launches.push_back({kBigLaunch, s, 0, uint32_t(i), j, m, 0, m * kBigWGsPerBlock, 1, uint32_t(kBigThreads), 0});
      }
}

}  // namespace transform_plan
}  // namespace jxh

#endif  // JXH_TRANSFORM_PLAN_H_
