// libjxl_amd — the reduced output (jxlhip_reduced_upload / jxlhip_reduced_run): a VarDCT frame's 1/8-scale image from its
// DC image alone, one sample per 8x8 block.
//   k_reduced_pixels  per tile of kTileCols x kTileRows samples (jxh_reduced_plan.h) and a one-sample halo: loads the three
//                     coded integer planes, lanes along x (a wave's load of a plane row is one 256-byte line; the two halo
//                     columns come from a few lanes of the first wave), dequantises every sample once into an LDS tile
//                     (DcDequantSample: the DC group's precision shift, chroma from luma), smooths from LDS (DcSmoothSample;
//                     the frame's border samples are copied, so a frame narrower or lower than 3 blocks has no interior),
//                     then XybToRgb, ApplyColorTarget and StorePixel as k_color_out runs them.
// The arithmetic of the first two steps is that of k_dc_dequant and k_dc_smooth (jxl_hip_dc.h): the same device functions.
// One launch serves every context of a batch: a workgroup finds its context by bisection over the tile origins.
#ifndef JXL_HIP_REDUCED_H_
#define JXL_HIP_REDUCED_H_

#include <hip/hip_runtime.h>

#include "../host/jxh_reduced_plan.h"
#include "jxl_hip_color.h"
#include "jxl_hip_dc.h"
#include "jxl_hip_filter_fused.h"
#include "jxl_hip_kernels.h"

namespace jxlhip {

// What the kernel reads of one context: the plan's head, then the colour stage's and the writer's blocks as k_color_out
// takes them (of `f` the colour fields alone are read).
struct ReducedDev {
  reduced::ReducedHead h;
  FilterParams f;
  PixelOut po;
  JxlHipColorTarget t;
};

// The context whose tiles hold tile `t` of a launch: the last one that starts at or before it (tile origins ascend, and
// every context has at least one tile).
__device__ __forceinline__ uint32_t ReducedDescOf(const ReducedDev* descs, uint32_t n, uint32_t t) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (descs[mid].h.tile0 <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

constexpr uint32_t kReducedPitch = reduced::kTileCols + 2, kReducedHaloRows = reduced::kTileRows + 2;
constexpr uint32_t kReducedPlane = kReducedPitch * kReducedHaloRows;

// Sample (x, y) of the frame, dequantised, to the tile's three planes at `at`; a position outside the frame (the halo of a
// tile at the frame's edge, which no interior sample's stencil reaches) gets zeros.
__device__ __forceinline__ void ReducedLoadSample(const reduced::ReducedHead& H, int x, int y, float* tile, uint32_t at) {
  float vx = 0.0f, vy = 0.0f, vb = 0.0f;
  if (x >= 0 && y >= 0 && x < int(H.xs) && y < int(H.ys)) {
    const size_t plane = size_t(H.xs) * H.ys, gi = size_t(y) * H.xs + size_t(x);
    const uint32_t ep = H.ep ? H.ep[(uint32_t(y) >> 8) * H.xgroups + (uint32_t(x) >> 8)] : 0u;
    DcDequantSample(H.q[gi], H.q[plane + gi], H.q[2 * plane + gi], ep, H.step, H.cfl_x, H.cfl_b, &vx, &vy, &vb);
  }
  tile[at] = vx;
  tile[kReducedPlane + at] = vy;
  tile[2 * kReducedPlane + at] = vb;
}

__global__ __launch_bounds__(256) void k_reduced_pixels(const ReducedDev* __restrict__ descs, uint32_t n) {
  __shared__ float tile[3 * kReducedPlane];
  const ReducedDev& D = descs[ReducedDescOf(descs, n, blockIdx.x)];
  const reduced::ReducedHead& H = D.h;
  const uint32_t t = blockIdx.x - H.tile0;
  if (t >= H.tiles) return;
  const uint32_t ty = t / H.tiles_x, tx = t - ty * H.tiles_x;
  const int x0 = int(tx * reduced::kTileCols), y0 = int(ty * reduced::kTileRows);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t r = wave; r < kReducedHaloRows; r += 4) ReducedLoadSample(H, x0 + int(lane), y0 - 1 + int(r), tile, r * kReducedPitch + lane + 1);
  if (threadIdx.x < 2 * kReducedHaloRows) {  // the columns left and right of the tile
    const uint32_t r = threadIdx.x >> 1, right = threadIdx.x & 1;
    ReducedLoadSample(H, right ? x0 + int(reduced::kTileCols) : x0 - 1, y0 - 1 + int(r), tile, r * kReducedPitch + (right ? reduced::kTileCols + 1 : 0));
  }
  __syncthreads();
  const int x = x0 + int(lane);
  if (x >= int(H.xs)) return;
  const size_t plane = size_t(H.xs) * H.ys;
  for (uint32_t r = wave; r < reduced::kTileRows; r += 4) {
    const int y = y0 + int(r);
    if (y >= int(H.ys)) break;
    const float* m = tile + (r + 1) * kReducedPitch + lane + 1;
    float v[3];
    // (compressed_dc.cc:141-147, 171-175: the frame's borders are copied; a frame that asks for no smoothing keeps every sample)
    if (!H.smoothing || x == 0 || y == 0 || x + 1 == int(H.xs) || y + 1 == int(H.ys)) {
      v[0] = m[0];
      v[1] = m[kReducedPlane];
      v[2] = m[2 * kReducedPlane];
    } else {
      DcSmoothSample(m, kReducedPlane, kReducedPitch, H.step, v);
    }
    if (H.dc_out) {
      const size_t gi = size_t(y) * H.xs + size_t(x);
      H.dc_out[gi] = v[0];
      H.dc_out[plane + gi] = v[1];
      H.dc_out[2 * plane + gi] = v[2];
    }
    float rr, gg, bb;
    XybToRgb(D.f, v[0], v[1], v[2], &rr, &gg, &bb);
    if (D.t.tf) ApplyColorTarget(D.t, &rr, &gg, &bb);
    StorePixel(D.po, x, y, rr, gg, bb);
  }
}

}  // namespace jxlhip
#endif  // JXL_HIP_REDUCED_H_
