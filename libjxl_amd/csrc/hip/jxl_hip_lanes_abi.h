// libjxl_amd — the LDS layout of a k_entropy_lanes workgroup (jxl_hip_entropy_lanes.h), free of HIP constructs: the kernel
// carves its LDS by it, and a plain C++ compile (csrc/host/jxh_lane_plan.h, the CPU tests) sizes the launch by the very
// same statement. The static_asserts pin the offsets that jxl_hip_lanes_trip.inc carries as immediates.
#ifndef JXL_HIP_LANES_ABI_H_
#define JXL_HIP_LANES_ABI_H_

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define JXL_HIP_LANES_HD __host__ __device__
#else
#define JXL_HIP_LANES_HD
#endif

namespace jxlhip {

// LDS layout of one workgroup (byte offsets, every region 16-byte aligned); the host sizes the launch with it.
struct LanesLds {
  uint32_t f2, alias, ctx, ctx2, cfg, poff, wave0, per_wave, total;
};
constexpr uint32_t kLanesF2Bytes = 128;  // 2 * kCoeffFreqContext[b], b < 128, at LDS offset 0 (jxl_hip_lanes_trip.inc reads it with no base)
// Per-wave LDS, all [row][lane] with a row of 64 entries (conflict-free):
constexpr uint32_t kLanesNzRows = 96;               // nzeros line buffer [channel * 32 + column], u8
constexpr uint32_t kLanesRingWords = 16;            // stream ring, u32; + 2 mirror rows (a 3-word read at slot 15 needs no wrap)
constexpr uint32_t kLanesBlockRing = 8;             // packed block records, u32
constexpr uint32_t kLanesPerLaneBytes = kLanesNzRows + (kLanesRingWords + 2) * 4 + kLanesBlockRing * 4;
// alias_lds = false: the alias tables stay in global memory (k_entropy_lanes<..., GALIAS = true>); prefix = true: prefix
// codes (no alias tables at all; the per-cluster table offsets get a 1 KB region).
// a6 = true: the six-byte form of the alias tables (jxl_hip_lanes_trip.inc, variant 6: log_alpha <= 7, at most 128 clusters
// and 8192 slots; fixed regions of 16 KB + 32 KB + 256 B whatever the table size, so that the trip's offsets are immediates).
constexpr uint32_t kLanesA6Clusters = 128, kLanesA6Slots = 8192, kLanesA6B = 128, kLanesA6A = kLanesA6B + kLanesA6Slots * 2,
                   kLanesA6Cfg = kLanesA6A + kLanesA6Slots * 4, kLanesA6End = kLanesA6Cfg + kLanesA6Clusters * 2;
static_assert(kLanesA6A == 16512 && kLanesA6Cfg == 49280, "jxl_hip_lanes_trip.inc LT_EREAD_6 has these as immediates");
JXL_HIP_LANES_HD inline LanesLds LanesLdsLayout(uint32_t num_hist, uint32_t nctx, uint32_t num_clusters, uint32_t log_alpha,
                                                uint32_t waves, uint32_t lanes, bool alias_lds = true, bool prefix = false, bool a6 = false) {
  LanesLds l;
  l.f2 = 0;
  l.alias = kLanesF2Bytes;  // (jxl_hip_lanes_trip.inc: ds_read_b64 ... offset:128)
  l.ctx = a6 ? kLanesA6End : l.alias + (alias_lds ? (num_clusters << log_alpha) * 8 : 0);
  l.ctx2 = l.ctx + ((num_hist * nctx + 16 + 15) & ~15u);
  l.cfg = l.ctx2 + 64 * 2;
  l.poff = l.cfg + (prefix ? 256 * 2 : 0);  // (the rANS forms carry a cluster's uint config in its alias entries)
  l.wave0 = l.poff + (prefix ? 256 * 4 : 0);
  l.per_wave = kLanesPerLaneBytes * lanes;
  l.total = l.wave0 + waves * l.per_wave;
  return l;
}

}  // namespace jxlhip

#endif  // JXL_HIP_LANES_ABI_H_
