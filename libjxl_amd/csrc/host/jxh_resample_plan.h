// libjxl_amd — the host plan of a resized binding (jxlhip_set_output_resized): whether a JxlHipResizedOut is taken, the tap
// tables of the separable antialiased triangle filter, and the layout of what the resample kernels (jxl_hip_resample.h)
// read from device memory. Free of HIP, so that tests/c/resample_kats.cc holds every line of it on the CPU. The HIP layer
// checks when the binding is set (no image yet), again at upload with the image's size, and in jxlhip_debug_resample.
#ifndef JXH_RESAMPLE_PLAN_H_
#define JXH_RESAMPLE_PLAN_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "jxh_tensor_out.h"

namespace jxlhip {
namespace resample {

// Every reason to refuse a descriptor, each stated once in CheckResizedOut. tests/c/resample_kats.cc breaks each rule in
// turn; tests/test_resample_host.py fails when a rule here has no row there.
enum ResampleRule : int {
  kResampleRuleOutput,     // out_xsize and out_ysize > 0
  kResampleRuleFilter,     // JXLHIP_RESAMPLE_TRIANGLE
  kResampleRuleOutLimit,   // out_xsize and out_ysize <= kMaxOutExtent
  kResampleRuleBoxExtents, // both box extents zero (then the origin too: the whole image) or both non-zero
  kResampleRuleBoxInside,  // x0 + xsize <= image xsize, y0 + ysize <= image ysize
  kResampleRuleTensor,     // the embedded tensor, by jxh_tensor_out.h at out_xsize x out_ysize
  kResampleRuleCount
};

// The largest output extent: what a tap table's 32-bit offsets and the launch grids are sized for.
constexpr uint32_t kMaxOutExtent = 16384;
// "No image yet" for CheckResizedOut: every box that fits 32 bits is inside.
constexpr uint32_t kAnyImageExtent = 0xFFFFFFFFu;

// The box the descriptor means in an image of xsize x ysize: all zero is the whole image.
struct Box {
  uint32_t x0, y0, xsize, ysize;
};
inline Box BoxOf(const JxlHipResizedOut& d, uint32_t image_xsize, uint32_t image_ysize) {
  if (!d.box_xsize && !d.box_ysize) return Box{0, 0, image_xsize, image_ysize};
  return Box{d.box_x0, d.box_y0, d.box_xsize, d.box_ysize};
}

// 0 when the descriptor is taken for an oriented output image of image_xsize x image_ysize, else
// JXLHIP_ERR_INVALID_ARGUMENT with the rule that refused it in *rule (may be NULL; when the tensor refuses, *tensor_rule,
// may be NULL, gets jxh_tensor_out.h's rule).
inline int CheckResizedOut(const JxlHipResizedOut& d, uint32_t image_xsize, uint32_t image_ysize, int* rule = nullptr,
                           int* tensor_rule = nullptr) {
#define JXH_RESAMPLE_REFUSE(cond, r)        \
  do {                                      \
    if (cond) {                             \
      if (rule) *rule = (r);                \
      return JXLHIP_ERR_INVALID_ARGUMENT;   \
    }                                       \
  } while (0)
  JXH_RESAMPLE_REFUSE(!d.out_xsize || !d.out_ysize, kResampleRuleOutput);
  JXH_RESAMPLE_REFUSE(d.filter != JXLHIP_RESAMPLE_TRIANGLE, kResampleRuleFilter);
  JXH_RESAMPLE_REFUSE(d.out_xsize > kMaxOutExtent || d.out_ysize > kMaxOutExtent, kResampleRuleOutLimit);
  JXH_RESAMPLE_REFUSE((d.box_xsize == 0) != (d.box_ysize == 0), kResampleRuleBoxExtents);
  JXH_RESAMPLE_REFUSE(!d.box_xsize && !d.box_ysize && (d.box_x0 || d.box_y0), kResampleRuleBoxExtents);
  // (64-bit sums: an origin and an extent near 2^32 do not wrap; an image of no pixels holds no box)
  JXH_RESAMPLE_REFUSE(!image_xsize || !image_ysize, kResampleRuleBoxInside);
  JXH_RESAMPLE_REFUSE(uint64_t(d.box_x0) + d.box_xsize > image_xsize || uint64_t(d.box_y0) + d.box_ysize > image_ysize, kResampleRuleBoxInside);
  int tr = -1;
  const int r = tensor_out::CheckTensorOut(d.tensor, d.out_xsize, d.out_ysize, &tr);
  if (r && tensor_rule) *tensor_rule = tr;
  JXH_RESAMPLE_REFUSE(r != 0, kResampleRuleTensor);
#undef JXH_RESAMPLE_REFUSE
  return 0;
}

// Room for the weights of one axis, n_in source samples to n_out output samples: 2 * n_in + 2 * n_out + 2.
// Why it holds. With scale = n_in / n_out and support = max(scale, 1), row i has hi - lo taps, where lo and hi are the
// truncations of two doubles that lie 2 * support apart before their own roundings, both clamped to [0, n_in].
//   n_out >= n_in (support is exactly 1): the two ends lie exactly 2 apart, so a row has 2 taps, unless center + 1.5 rounds
//     up to an integer that the exact sum stays below (9 -> 33, row 5: center = 1.5 - 2^-52, hi = 3, a third tap of weight
//     ~0). That needs the exact end within a few ulp of an integer; the ends of different rows lie scale >= 2^-14 apart
//     (n_out <= kMaxOutExtent), so each integer 2 .. n_in + 1 is met by at most one row: 2 * n_out + n_in taps at most.
//   n_out < n_in: floor(a + 2 s) - floor(a) <= ceil(2 s) <= 2 s + 1, and the roundings of the two ends can move each
//     truncation across at most one integer, which the clamp or the other end does not always absorb: at most 2 s + 2 taps
//     per row, n_out * (2 * n_in / n_out + 2) = 2 * n_in + 2 * n_out over the axis.
// Both are inside the bound (the + 2 is slack); MakeAxisTaps also refuses to write past the room it is given.
inline uint64_t AxisWeightBound(uint32_t n_in, uint32_t n_out) { return 2 * uint64_t(n_in) + 2 * uint64_t(n_out) + 2; }

// The table of one axis: row i reads source samples first[i] .. first[i] + count[i] - 1 (relative to the box) with the
// weights that follow those of row i - 1 in `weights` (room: `room` floats). Everything in double, each weight rounded to
// float at the end: what torch's interpolate(mode="bilinear", antialias=True, align_corners=False) computes in float64,
// and Pillow's rule. Returns the number of weights, or -1 when `room` is too small (nothing past it is written).
inline int64_t MakeAxisTaps(uint32_t n_in, uint32_t n_out, uint32_t* first, uint32_t* count, float* weights, uint64_t room) {
  if (!n_in || !n_out) return -1;
  const double scale = double(n_in) / double(n_out);
  const double support = scale > 1.0 ? scale : 1.0;
  const double inv = 1.0 / support;
  uint64_t total = 0;
  for (uint32_t i = 0; i < n_out; i++) {
    const double center = scale * (double(i) + 0.5);
    double lo_d = trunc(center - support + 0.5), hi_d = trunc(center + support + 0.5);
    if (lo_d < 0.0) lo_d = 0.0;
    if (hi_d > double(n_in)) hi_d = double(n_in);
    const uint32_t lo = uint32_t(lo_d), hi = uint32_t(hi_d);
    const uint32_t n = hi > lo ? hi - lo : 0;
    if (total + n > room) return -1;
    double sum = 0.0;
    for (uint32_t k = 0; k < n; k++) {
      const double w = 1.0 - fabs((double(lo + k) - center + 0.5) * inv);
      sum += w > 0.0 ? w : 0.0;
    }
    for (uint32_t k = 0; k < n; k++) {
      const double w = 1.0 - fabs((double(lo + k) - center + 0.5) * inv);
      weights[total + k] = float((w > 0.0 ? w : 0.0) / sum);
    }
    first[i] = lo;
    count[i] = n;
    total += n;
  }
  return int64_t(total);
}

// ---- what is placed on the device. Per context: one ResampleDev and the tables of the two axes, in one block; a batched
// launch reads an array of ResampleDev (the contexts' own, copied side by side). An axis table is four arrays, one after
// the other: first[n_out], count[n_out], offset[n_out] (of the row's first weight), weights[AxisWeightBound].
struct AxisDev {
  const uint32_t* first;
  const uint32_t* count;
  const uint32_t* offset;
  const float* weights;
};
struct ResampleDev {
  const float* src;  // interleaved f32 rows of src_row pixels of nc samples: the context's own pixel buffer
  float* tmp;        // [out_ysize][box_xsize * nc] f32: the box behind the vertical pass
  void* dst;         // the tensor
  AxisDev x, y;
  int64_t stride_c, stride_y, stride_x;
  uint32_t src_row, nc;
  uint32_t box_x0, box_y0, box_xsize, box_ysize;
  uint32_t out_xsize, out_ysize;
  uint32_t dtype, clamp01;
  float scale[4], bias[4];
  // the context's workgroups in the two launches: v_tiles from v_tile0 on (vertical pass), h_tiles from h_tile0 on
  uint32_t v_tile0, v_tiles, h_tile0, h_tiles;
};
// Tiles of the two passes (the kernels' own shapes): the vertical pass takes kVTileCols floats of a box row by kVTileRows
// output rows per workgroup, the horizontal pass kHTileCols output columns of one output row.
constexpr uint32_t kVTileCols = 64, kVTileRows = 4, kHTileCols = 64;
inline uint32_t VerticalTiles(uint32_t box_xsize, uint32_t nc, uint32_t out_ysize) {
  const uint64_t row = uint64_t(box_xsize) * nc;
  return uint32_t(((row + kVTileCols - 1) / kVTileCols) * ((out_ysize + kVTileRows - 1) / kVTileRows));
}
inline uint32_t HorizontalTiles(uint32_t out_xsize, uint32_t out_ysize) { return ((out_xsize + kHTileCols - 1) / kHTileCols) * out_ysize; }

inline size_t AxisTableBytes(uint32_t n_in, uint32_t n_out) { return (3 * size_t(n_out) + size_t(AxisWeightBound(n_in, n_out))) * 4; }
// Builds the axis table into `block` (AxisTableBytes(n_in, n_out) bytes, 4-aligned), which will live at `device_base`;
// *dev gets the device addresses. Returns the number of weights or -1.
inline int64_t PlaceAxisTable(uint32_t n_in, uint32_t n_out, void* block, uintptr_t device_base, AxisDev* dev) {
  uint32_t* first = static_cast<uint32_t*>(block);
  uint32_t* count = first + n_out;
  uint32_t* offset = count + n_out;
  float* weights = reinterpret_cast<float*>(offset + n_out);
  const int64_t total = MakeAxisTaps(n_in, n_out, first, count, weights, AxisWeightBound(n_in, n_out));
  if (total < 0) return total;
  uint32_t at = 0;
  for (uint32_t i = 0; i < n_out; i++) {
    offset[i] = at;
    at += count[i];
  }
  dev->first = reinterpret_cast<const uint32_t*>(device_base);
  dev->count = dev->first + n_out;
  dev->offset = dev->count + n_out;
  dev->weights = reinterpret_cast<const float*>(dev->offset + n_out);
  return total;
}

// The block of one context: the descriptor, then the x table, then the y table.
struct BlockLayout {
  size_t desc, x, y, bytes;
};
inline BlockLayout LayoutOf(const Box& b, uint32_t out_xsize, uint32_t out_ysize) {
  BlockLayout l;
  l.desc = 0;
  l.x = (sizeof(ResampleDev) + 15) & ~size_t(15);
  l.y = l.x + ((AxisTableBytes(b.xsize, out_xsize) + 15) & ~size_t(15));
  l.bytes = l.y + ((AxisTableBytes(b.ysize, out_ysize) + 15) & ~size_t(15));
  return l;
}
inline size_t TmpBytes(const Box& b, uint32_t nc, uint32_t out_ysize) { return size_t(out_ysize) * b.xsize * nc * 4; }

// Fills `block` (LayoutOf(...).bytes bytes, to live at device_base) for a descriptor that CheckResizedOut took at the
// size of an image whose pixels are `src` (rows of src_row pixels). The tile origins stay 0: the launch sets them.
inline int PlaceBlock(const JxlHipResizedOut& d, const Box& b, const float* src, uint32_t src_row, float* tmp, void* block, uintptr_t device_base) {
  const BlockLayout l = LayoutOf(b, d.out_xsize, d.out_ysize);
  uint8_t* p = static_cast<uint8_t*>(block);
  ResampleDev r;
  memset(&r, 0, sizeof(r));
  if (PlaceAxisTable(b.xsize, d.out_xsize, p + l.x, device_base + l.x, &r.x) < 0) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (PlaceAxisTable(b.ysize, d.out_ysize, p + l.y, device_base + l.y, &r.y) < 0) return JXLHIP_ERR_INVALID_ARGUMENT;
  r.src = src;
  r.tmp = tmp;
  r.dst = d.tensor.data;
  r.stride_c = d.tensor.stride_c;
  r.stride_y = d.tensor.stride_y;
  r.stride_x = d.tensor.stride_x;
  r.src_row = src_row;
  r.nc = d.tensor.num_channels;
  r.box_x0 = b.x0;
  r.box_y0 = b.y0;
  r.box_xsize = b.xsize;
  r.box_ysize = b.ysize;
  r.out_xsize = d.out_xsize;
  r.out_ysize = d.out_ysize;
  r.dtype = d.tensor.dtype;
  r.clamp01 = d.tensor.clamp01 ? 1 : 0;
  memcpy(r.scale, d.tensor.scale, sizeof(r.scale));
  memcpy(r.bias, d.tensor.bias, sizeof(r.bias));
  r.v_tiles = VerticalTiles(b.xsize, r.nc, d.out_ysize);
  r.h_tiles = HorizontalTiles(d.out_xsize, d.out_ysize);
  memcpy(p + l.desc, &r, sizeof(r));
  return 0;
}

}  // namespace resample
}  // namespace jxlhip
#endif  // JXH_RESAMPLE_PLAN_H_
