// libjxl_amd — the tile and strip sizes of the filter kernels (jxl_hip_filter_fused.h), free of HIP constructs: the kernels
// walk their tiles by them, and a plain C++ compile (csrc/host/jxh_filter_plan.h, the CPU tests) sizes the launches by the
// very same statement.
#ifndef JXL_HIP_FILTER_ABI_H_
#define JXL_HIP_FILTER_ABI_H_

namespace jxlhip {

constexpr int kFusedTW = 64, kFusedTH = 16;  // 37 KB of LDS with a 3-pixel halo: two tiles fit beside an entropy workgroup
constexpr int kRowsStrip = 64;               // output rows per wave
constexpr int kRowsWaves = 4;                // waves (adjacent column groups) per workgroup
constexpr int kRows2Cols = 120;  // output columns per wave: 128 - 2 * 4 (left halo rounded up to a whole pair)

}  // namespace jxlhip

#endif  // JXL_HIP_FILTER_ABI_H_
