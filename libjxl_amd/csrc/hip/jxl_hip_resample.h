// libjxl_amd — the two passes of a resized binding (jxlhip_set_output_resized): the separable antialiased triangle filter
// over a box of the context's f32 pixels, into the caller's tensor. The weights come from the host's tables
// (jxh_resample_plan.h); the kernels multiply and add in float32.
//   k_resample_rows     the vertical pass first: the source's interleaved rows are read as they lie (a wave takes 64
//                       adjacent floats of a row, so every load is one 256-byte line) and only the box's rows and columns
//                       are touched; out_ysize rows of the box's width stay (ResampleDev::tmp).
//   k_resample_columns  the horizontal pass: a workgroup stages the piece of an intermediate row that its 64 output columns
//                       read in LDS, once, and walks a window that is longer than the tile piece by piece; it stores through
//                       the tensor's strides with the writer's own conversion (TensorAffine, StoreFloatSample, ToU8D: jxl_hip_kernels.h).
// One launch per pass serves every context of a batch: a workgroup finds its context by its tile number.
#ifndef JXL_HIP_RESAMPLE_H_
#define JXL_HIP_RESAMPLE_H_

#include <hip/hip_runtime.h>

#include "../host/jxh_resample_plan.h"
#include "jxl_hip_kernels.h"

namespace jxlhip {

using resample::ResampleDev;

// The context whose tiles hold tile `t` of a launch: the last one that starts at or before it (tile origins ascend, and
// every context has at least one tile).
template <bool kVertical>
__device__ __forceinline__ uint32_t ResampleDescOf(const ResampleDev* descs, uint32_t n, uint32_t t) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    const uint32_t t0 = kVertical ? descs[mid].v_tile0 : descs[mid].h_tile0;
    if (t0 <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_resample_rows(const ResampleDev* __restrict__ descs, uint32_t n) {
  const ResampleDev& D = descs[ResampleDescOf<true>(descs, n, blockIdx.x)];
  const uint32_t tile = blockIdx.x - D.v_tile0;
  if (tile >= D.v_tiles) return;
  const uint32_t row_floats = D.box_xsize * D.nc;
  const uint32_t col_tiles = (row_floats + resample::kVTileCols - 1) / resample::kVTileCols;
  const uint32_t ty = tile / col_tiles, tx = tile - ty * col_tiles;
  const uint32_t k = tx * resample::kVTileCols + (threadIdx.x & 63);
  const uint32_t oy = ty * resample::kVTileRows + (threadIdx.x >> 6);  // (one output row per wave: its taps are scalar loads)
  if (k >= row_floats || oy >= D.out_ysize) return;
  const uint32_t first = D.y.first[oy], count = D.y.count[oy];
  const float* __restrict__ w = D.y.weights + D.y.offset[oy];
  const size_t pitch = size_t(D.src_row) * D.nc;
  const float* __restrict__ s = D.src + (size_t(D.box_y0) + first) * pitch + size_t(D.box_x0) * D.nc + k;
  float acc = 0.0f;
#pragma unroll 4
  for (uint32_t j = 0; j < count; j++) acc = fmaf(w[j], s[size_t(j) * pitch], acc);
  D.tmp[size_t(oy) * row_floats + k] = acc;
}

// Pixels of an intermediate row a workgroup holds in LDS at a time (4 KiB at 4 channels). 64 columns of a 3840 -> 224
// tile read 1100 pixels: five pieces; a single window of 600 -> 7 (172 taps) already spans two or three.
constexpr uint32_t kResamplePiece = 256;

__global__ __launch_bounds__(256) void k_resample_columns(const ResampleDev* __restrict__ descs, uint32_t n) {
  __shared__ float piece[kResamplePiece * 4];
  const ResampleDev& D = descs[ResampleDescOf<false>(descs, n, blockIdx.x)];
  const uint32_t tile = blockIdx.x - D.h_tile0;
  if (tile >= D.h_tiles) return;
  const uint32_t nc = D.nc;
  const uint32_t col_tiles = (D.out_xsize + resample::kHTileCols - 1) / resample::kHTileCols;
  const uint32_t oy = tile / col_tiles, tx = tile - oy * col_tiles;
  const uint32_t ox0 = tx * resample::kHTileCols;
  const uint32_t ox1 = min(ox0 + resample::kHTileCols, D.out_xsize);
  const uint32_t ox = ox0 + (threadIdx.x >> 2), c = threadIdx.x & 3;
  const bool live = ox < ox1 && c < nc;
  const uint32_t first = live ? D.x.first[ox] : 0, count = live ? D.x.count[ox] : 0;
  const float* __restrict__ w = D.x.weights + (live ? D.x.offset[ox] : 0);
  // what the tile's columns read of the row: windows start and end in ascending order
  const uint32_t span_begin = D.x.first[ox0], span_end = D.x.first[ox1 - 1] + D.x.count[ox1 - 1];
  const float* __restrict__ row = D.tmp + size_t(oy) * D.box_xsize * nc;
  float acc = 0.0f;
  for (uint32_t p0 = span_begin; p0 < span_end; p0 += kResamplePiece) {
    const uint32_t p1 = min(p0 + kResamplePiece, span_end);
    const uint32_t floats = (p1 - p0) * nc;
    for (uint32_t i = threadIdx.x; i < floats; i += 256) piece[i] = row[size_t(p0) * nc + i];
    __syncthreads();
    const uint32_t a = max(first, p0), b = min(first + count, p1);
    for (uint32_t j = a; j < b; j++) acc = fmaf(w[j - first], piece[(j - p0) * nc + c], acc);
    __syncthreads();
  }
  if (!live) return;
  const size_t index = size_t(c) * size_t(D.stride_c) + size_t(oy) * size_t(D.stride_y) + size_t(ox) * size_t(D.stride_x);
  if (D.dtype == 2) {  // v * 255 rounded, clamped, to nearest even: the writer's 8-bit conversion without a dither cell
    static_cast<uint8_t*>(D.dst)[index] = ToU8D(acc, 0.0f);
    return;
  }
  // (the writer's own tensor arithmetic and float conversion: TensorAffine, StoreFloatSample)
  const float scale = c == 0 ? D.scale[0] : (c == 1 ? D.scale[1] : (c == 2 ? D.scale[2] : D.scale[3]));
  const float bias = c == 0 ? D.bias[0] : (c == 1 ? D.bias[1] : (c == 2 ? D.bias[2] : D.bias[3]));
  StoreFloatSample(D.dst, D.dtype, 0, index, TensorAffine(acc, scale, bias, D.clamp01));
}

}  // namespace jxlhip
#endif  // JXL_HIP_RESAMPLE_H_
