// libjxl_amd — the DC image of a window of a frame (jxlhip_dc_window; region decode, csrc/host/jxh_window_plan.h).
//   k_dc_window  per tile of kTileCols x kTileRows samples of the window and a one-sample halo: loads the three coded integer
//                planes of the apron (the window grown by one block, clipped to the frame), lanes along x (a wave's load of
//                a plane row is one 256-byte line; the two halo columns come from a few lanes of the first wave),
//                dequantises every sample once into an LDS tile (DcDequantSample; the DC group's precision shift is looked
//                up at the sample's ABSOLUTE block position in the frame), smooths from LDS (DcSmoothSample) and stores
//                the window's dense planes. A sample on the FRAME's border is copied (compressed_dc.cc:141-147,171-175); a
//                sample on the window's edge that is not on the frame's border is smoothed from the apron.
// The arithmetic is that of k_dc_dequant and k_dc_smooth (jxl_hip_dc.h): the same device functions, so the planes equal
// the window's rectangle of the whole frame's DC image bit for bit. The tiling is k_reduced_pixels' (jxl_hip_reduced.h).
#ifndef JXL_HIP_DC_WINDOW_H_
#define JXL_HIP_DC_WINDOW_H_

#include <hip/hip_runtime.h>

#include "../host/jxh_window_plan.h"
#include "jxl_hip_dc.h"

namespace jxlhip {

struct DcWindowParams {
  const int32_t* q;    // [3][ays][axs]: the apron's coded integers of X, Y, B
  const uint8_t* ep;   // the frame's precision shifts per DC group, or NULL (all 0)
  float* out;          // [3][wys][wxs]
  int ax0, ay0, axs, ays;  // the apron, in blocks of the frame
  int wx0, wy0, wxs, wys;  // the window
  int fxs, fys;            // the frame
  uint32_t xgroups;        // DC groups per row of the frame
  uint32_t smoothing;
  float step[3], cfl_x, cfl_b;
};

constexpr uint32_t kDcWinPitch = window::kTileCols + 2, kDcWinHaloRows = window::kTileRows + 2;
constexpr uint32_t kDcWinPlane = kDcWinPitch * kDcWinHaloRows;

// Sample (x, y) of the FRAME, dequantised, to the tile's three planes at `at`; a position outside the apron (outside the
// frame, or beyond the ring no sample of the window's stencil reaches) gets zeros.
__device__ __forceinline__ void DcWindowLoadSample(const DcWindowParams& P, int x, int y, float* tile, uint32_t at) {
  float vx = 0.0f, vy = 0.0f, vb = 0.0f;
  const int rx = x - P.ax0, ry = y - P.ay0;
  if (rx >= 0 && ry >= 0 && rx < P.axs && ry < P.ays) {
    const size_t plane = size_t(P.axs) * size_t(P.ays), gi = size_t(ry) * size_t(P.axs) + size_t(rx);
    const uint32_t ep = P.ep ? P.ep[(uint32_t(y) >> 8) * P.xgroups + (uint32_t(x) >> 8)] : 0u;
    DcDequantSample(P.q[gi], P.q[plane + gi], P.q[2 * plane + gi], ep, P.step, P.cfl_x, P.cfl_b, &vx, &vy, &vb);
  }
  tile[at] = vx;
  tile[kDcWinPlane + at] = vy;
  tile[2 * kDcWinPlane + at] = vb;
}

__global__ __launch_bounds__(256) void k_dc_window(DcWindowParams P) {
  __shared__ float tile[3 * kDcWinPlane];
  // (the tile's origin in the window, and in the frame)
  const int tx0 = int(blockIdx.x * window::kTileCols), ty0 = int(blockIdx.y * window::kTileRows);
  const int x0 = P.wx0 + tx0, y0 = P.wy0 + ty0;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t r = wave; r < kDcWinHaloRows; r += 4) DcWindowLoadSample(P, x0 + int(lane), y0 - 1 + int(r), tile, r * kDcWinPitch + lane + 1);
  if (threadIdx.x < 2 * kDcWinHaloRows) {  // the columns left and right of the tile
    const uint32_t r = threadIdx.x >> 1, right = threadIdx.x & 1;
    DcWindowLoadSample(P, right ? x0 + int(window::kTileCols) : x0 - 1, y0 - 1 + int(r), tile, r * kDcWinPitch + (right ? window::kTileCols + 1 : 0));
  }
  __syncthreads();
  const int wx = tx0 + int(lane), x = x0 + int(lane);
  if (wx >= P.wxs) return;
  const size_t plane = size_t(P.wxs) * size_t(P.wys);
  for (uint32_t r = wave; r < window::kTileRows; r += 4) {
    const int wy = ty0 + int(r), y = y0 + int(r);
    if (wy >= P.wys) break;
    const float* m = tile + (r + 1) * kDcWinPitch + lane + 1;
    float v[3];
    // (the frame's borders are copied; a frame that asks for no smoothing keeps every sample)
    if (!P.smoothing || x == 0 || y == 0 || x + 1 == P.fxs || y + 1 == P.fys) {
      v[0] = m[0];
      v[1] = m[kDcWinPlane];
      v[2] = m[2 * kDcWinPlane];
    } else {
      DcSmoothSample(m, kDcWinPlane, kDcWinPitch, P.step, v);
    }
    const size_t gi = size_t(wy) * size_t(P.wxs) + size_t(wx);
    P.out[gi] = v[0];
    P.out[plane + gi] = v[1];
    P.out[2 * plane + gi] = v[2];
  }
}

}  // namespace jxlhip
#endif  // JXL_HIP_DC_WINDOW_H_
