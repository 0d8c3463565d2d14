// The launch plan of a batched Modular decode (jxlhip_modular_run_batch; jxl_hip_api.hip PrepareModBatch): host only, no
// HIP types. Pure functions of what the frames of the set say and of the one measurement aid: in what order the streams
// of the set go to the stream kernel, how many share a wave, how much LDS a workgroup asks for and which form of the
// kernel runs; and the grids of the transform / output launches behind it (upload::ModLaunch), cut to the grid limits.
#ifndef JXH_MODULAR_LAUNCH_PLAN_H_
#define JXH_MODULAR_LAUNCH_PLAN_H_

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../hip/jxl_hip_modular_abi.h"
#include "jxh_modular_upload_plan.h"

namespace jxh {
namespace modular_launch {

using jxlhip::ModStream;
using jxlhip::upload::ModLaunch;

// What the plan reads of a frame: views into what the context holds.
struct ModStreamFrame {
  const ModStream* streams;          // the host copy of the frame's descriptors, device addresses filled in
  const uint32_t* stream_samples;    // [num_streams]
  size_t num_streams;
  const uint32_t* code_table_words;  // per entropy code: ModCode::table_words
  size_t num_codes;
};

// One launch as plain integers: blocks [first, first + count) of the parameter-block array at `offset` of the blob.
struct ModGrid {
  uint32_t kind;  // ModLaunch::kind
  size_t offset;
  uint32_t first, count;
  uint32_t grid[3], block;
};

struct ModBatchPlan {
  uint32_t n = 0;                               // streams of the set
  uint32_t tree_cap = 0, table_cap = 0;         // LDS room: tree nodes, words of symbol tables
  bool wp = false, refs = false;                // the form k_modular_streams<WP, REFS>
  uint32_t lanes = 1, lds = 0, workgroups = 0;  // streams per wave, dynamic LDS of a workgroup, the grid (none without a stream)
  std::vector<ModGrid> grids;                   // the transform / output launches in their order (ExpandModLaunches)
};
inline const char* FormName(const ModBatchPlan& p) { return p.wp ? (p.refs ? "wp+refs" : "wp") : (p.refs ? "refs" : "plain"); }

inline bool LanesOverrideTaken(int v) { return v >= 1 && v <= 64 && (v & (v - 1)) == 0; }

// The stream launch of a set. `flat`: the descriptors in launch order (one zeroed entry when the set has no stream, so
// that the copy to the device is never empty).
inline ModBatchPlan PlanModStreams(const ModStreamFrame* frames, size_t n, int lanes_override, std::vector<ModStream>* flat) {
  ModBatchPlan p;
  // every stream of every frame, largest first (ties in frame, then stream order): the lanes of a wave then carry
  // streams of similar length
  struct Ref {
    uint32_t samples;
    const ModStream* s;
  };
  std::vector<Ref> all;
  for (size_t i = 0; i < n; i++)
    for (size_t j = 0; j < frames[i].num_streams; j++) all.push_back({frames[i].stream_samples[j], &frames[i].streams[j]});
  std::stable_sort(all.begin(), all.end(), [](const Ref& a, const Ref& b) { return a.samples > b.samples; });
  flat->assign(all.size() ? all.size() : 1, ModStream());
  for (size_t i = 0; i < all.size(); i++) (*flat)[i] = *all[i].s;
  p.n = uint32_t(all.size());
  for (const Ref& q : all) {
    // LDS room for the largest tree of the batch that fits (waves whose streams share a tree stage it)
    if (q.s->tree_nodes <= jxlhip::kModTreeLdsNodes && q.s->tree_nodes > p.tree_cap) p.tree_cap = q.s->tree_nodes;
    // the kernel form: what some stream of the launch needs
    p.wp = p.wp || q.s->uses_wp != 0;
    p.refs = p.refs || q.s->num_props > 16;
  }
  for (size_t i = 0; i < n; i++)  // likewise for the largest set of symbol tables that fits
    for (size_t k = 0; k < frames[i].num_codes; k++) {
      const uint32_t w = frames[i].code_table_words[k];
      if (w <= jxlhip::kModTableLdsWords && w > p.table_cap) p.table_cap = w;
    }
  // A stream is a chain of dependent latencies: as few streams per wave as still leaves every SIMD of the device a
  // few waves (the override: measurement aid). 384 lossless 4K frames = 53 760 streams: 32 lanes per wave
  // 2 219 MP/s, 16 lanes 2 360, 8 lanes 1 864, 4 lanes 1 166: up to four waves per SIMD.
  while (p.lanes < 64 && p.n / p.lanes > 4096) p.lanes *= 2;
  if (LanesOverrideTaken(lanes_override)) p.lanes = uint32_t(lanes_override);
  p.lds = jxlhip::ModLdsBytes(p.lanes, p.tree_cap, p.table_cap);
  p.workgroups = (p.n + p.lanes - 1) / p.lanes;
  return p;
}

// One more block of a pass over whole frames (float planes, patches, splines, output), for a frame of xs x ys. `rows`:
// one workgroup per row (the spline and patch kernels) instead of 256 columns per workgroup.
inline void ModPassAdd(ModLaunch* L, bool rows, uint32_t xs, uint32_t ys) {
  L->count++;
  L->gx = rows ? 1 : std::max(L->gx, (xs + 255) / 256);
  L->gy = std::max(L->gy, ys);
}

constexpr uint32_t kModGridZ = 65535;      // grid z / y limit: the blocks of a launch beyond it go to further launches
constexpr uint32_t kModSampleRows = 4096;  // grid y of the sample kernels (their row loops stride by the grid)

// The grids of the launches, in their order.
inline std::vector<ModGrid> ExpandModLaunches(const std::vector<ModLaunch>& launches) {
  std::vector<ModGrid> grids;
  for (const ModLaunch& L : launches)
    for (uint32_t z = 0; z < L.count; z += kModGridZ) {
      const uint32_t zn = std::min<uint32_t>(L.count - z, kModGridZ);
      ModGrid g{L.kind, L.offset, z, zn, {1, 1, 1}, 256};
      if (L.kind == 2) {  // unsqueeze: 64 lines per workgroup, the blocks along y
        g.grid[0] = L.gx;
        g.grid[1] = zn;
        g.block = 64;
      } else if (L.kind == 5 || L.kind == 6) {  // splines, patches: one workgroup per row, so the full height and not
        g.grid[0] = L.gy;                       // the strided grid of the sample kernels; the blocks along y
        g.grid[1] = zn;
      } else {  // RCT, palette, float planes, output: 256 columns per workgroup, the blocks along z
        g.grid[0] = L.gx;
        g.grid[1] = std::min<uint32_t>(L.gy, kModSampleRows);
        g.grid[2] = zn;
      }
      grids.push_back(g);
    }
  return grids;
}

}  // namespace modular_launch
}  // namespace jxh

#endif  // JXH_MODULAR_LAUNCH_PLAN_H_
