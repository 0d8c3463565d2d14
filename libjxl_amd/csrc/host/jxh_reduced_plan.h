// libjxl_amd — the host plan of a reduced upload (jxlhip_reduced_upload): whether a JxlHipReducedDesc is taken, the tiles
// k_reduced_pixels (jxl_hip_reduced.h) cuts a reduced image into, the layout of what one context places on the device, and
// the descriptor array of a batched launch with its running tile origins. Free of HIP, so that tests/c/reduced_kats.cc
// holds every line of it on the CPU.
#ifndef JXH_REDUCED_PLAN_H_
#define JXH_REDUCED_PLAN_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../../include/jxl_amd_hip.h"

namespace jxlhip {
namespace reduced {

// Every reason to refuse a descriptor, each stated once in CheckReducedDesc. tests/c/reduced_kats.cc breaks each rule in
// turn; tests/test_reduced_host.py fails when a rule here has no row there.
enum ReducedRule : int {
  kReducedRuleExtents,    // xsize_blocks and ysize_blocks > 0
  kReducedRulePlaneSize,  // 12 * xsize_blocks * ysize_blocks (the three planes in bytes) fits 64 bits and size_t
  kReducedRuleLimit,      // xsize_blocks and ysize_blocks <= kMaxExtentBlocks
  kReducedRulePlanes,     // dc_quantised != NULL
  kReducedRuleSteps,      // the three dc_step finite and > 0
  kReducedRuleLinear,     // linear_output 0 or 1
  kReducedRulePrecision,  // dc_extra_precision != NULL for a frame of several DC groups
  kReducedRuleLaunch,     // the image's tiles <= kMaxLaunchTiles: one launch holds them
  kReducedRuleCount
};

// The format's limit: an image side is at most 2^30 pixels (headers: SizeHeader), 2^27 blocks.
constexpr uint32_t kMaxExtentBlocks = 1u << 27;
// A DC group covers 256 x 256 blocks (2048 x 2048 pixels).
constexpr uint32_t kDcGroupBlocks = 256;
inline uint64_t DcGroups(uint32_t xsize_blocks, uint32_t ysize_blocks) {
  return uint64_t((xsize_blocks + kDcGroupBlocks - 1) / kDcGroupBlocks) * ((ysize_blocks + kDcGroupBlocks - 1) / kDcGroupBlocks);
}

// ---- tiles. A workgroup of 256 threads takes kTileCols x kTileRows samples: lanes run along x, so that a wave's load of a
// plane row is one 256-byte line, and every thread makes kTileRows / 4 samples. With the one-sample halo the smoothing reads,
// a tile loads (kTileCols + 2) * (kTileRows + 2) samples of each plane: 1.29 per sample it makes, in 7.9 KB of LDS.
// (The shape is a guess between the halo's share, 1.55 at 4 rows and 1.16 at 16, and the number of workgroups a small image
// gives the device: a 480 x 270 image is 272 tiles; it has not been measured against other shapes.)
constexpr uint32_t kTileCols = 64, kTileRows = 8;
inline uint32_t TilesX(uint32_t xsize_blocks) { return (xsize_blocks + kTileCols - 1) / kTileCols; }
inline uint32_t TilesY(uint32_t ysize_blocks) { return (ysize_blocks + kTileRows - 1) / kTileRows; }
inline uint64_t Tiles(uint32_t xsize_blocks, uint32_t ysize_blocks) { return uint64_t(TilesX(xsize_blocks)) * TilesY(ysize_blocks); }
// The launch grid is one-dimensional over the tiles of all the contexts of a set: at most 2^32 - 1 threads in the grid's
// x dimension (the runtime's limit on blocks times threads), 256 per tile.
constexpr uint64_t kMaxLaunchTiles = 0xFFFFFFFFull / 256;

// 0 when the descriptor is taken, else JXLHIP_ERR_INVALID_ARGUMENT with the rule that refused it in *rule (may be NULL).
inline int CheckReducedDesc(const JxlHipReducedDesc& d, int* rule = nullptr) {
#define JXH_REDUCED_REFUSE(cond, r)         \
  do {                                      \
    if (cond) {                             \
      if (rule) *rule = (r);                \
      return JXLHIP_ERR_INVALID_ARGUMENT;   \
    }                                       \
  } while (0)
  JXH_REDUCED_REFUSE(!d.xsize_blocks || !d.ysize_blocks, kReducedRuleExtents);
  // (before the limit, so that the product is never formed unchecked: two 32-bit extents times 12 can pass 2^64)
  unsigned long long samples = 0, bytes = 0;
  const bool wraps = __builtin_mul_overflow((unsigned long long)d.xsize_blocks, (unsigned long long)d.ysize_blocks, &samples) ||
                     __builtin_mul_overflow(samples, 12ull, &bytes);
  JXH_REDUCED_REFUSE(wraps || bytes > (unsigned long long)SIZE_MAX, kReducedRulePlaneSize);
  JXH_REDUCED_REFUSE(d.xsize_blocks > kMaxExtentBlocks || d.ysize_blocks > kMaxExtentBlocks, kReducedRuleLimit);
  JXH_REDUCED_REFUSE(!d.dc_quantised, kReducedRulePlanes);
  for (int c = 0; c < 3; c++) JXH_REDUCED_REFUSE(!isfinite(d.dc_step[c]) || !(d.dc_step[c] > 0.0f), kReducedRuleSteps);
  JXH_REDUCED_REFUSE(d.linear_output != 0 && d.linear_output != 1, kReducedRuleLinear);
  JXH_REDUCED_REFUSE(!d.dc_extra_precision && DcGroups(d.xsize_blocks, d.ysize_blocks) > 1, kReducedRulePrecision);
  JXH_REDUCED_REFUSE(Tiles(d.xsize_blocks, d.ysize_blocks) > kMaxLaunchTiles, kReducedRuleLaunch);
#undef JXH_REDUCED_REFUSE
  return 0;
}

// ---- what is placed on the device. The head of a context's descriptor (the kernel's descriptor, jxl_hip_reduced.h
// ReducedDev, begins with it and goes on with the colour stage's and the pixel writer's blocks).
struct ReducedHead {
  const int32_t* q;     // [3][ys][xs]
  const uint8_t* ep;    // per DC group, or NULL (all 0)
  float* dc_out;        // [3][ys][xs], or NULL: option "keep_dc"
  uint32_t xs, ys, xgroups, smoothing;
  float step[3], cfl_x, cfl_b;
  // the context's workgroups in the launch: `tiles` from tile0 on, tiles_x per tile row
  uint32_t tile0, tiles, tiles_x;
};

// The block of one context: the descriptor (desc_bytes: sizeof the kernel's descriptor), then the precision bytes, then the
// integers; one staged copy.
struct BlockLayout {
  size_t desc, ep, q, bytes;
  size_t ep_bytes, q_bytes;
};
inline BlockLayout LayoutOf(const JxlHipReducedDesc& d, size_t desc_bytes) {
  BlockLayout l;
  l.desc = 0;
  l.ep = (desc_bytes + 15) & ~size_t(15);
  l.ep_bytes = d.dc_extra_precision ? size_t(DcGroups(d.xsize_blocks, d.ysize_blocks)) : 0;
  l.q = (l.ep + l.ep_bytes + 255) & ~size_t(255);  // (the planes start on a 256-byte line of the block)
  l.q_bytes = size_t(d.xsize_blocks) * d.ysize_blocks * 12;
  l.bytes = l.q + l.q_bytes;
  return l;
}
// Fills the head and copies the arrays into `block` (LayoutOf(...).bytes bytes, to live at device_base) for a descriptor
// that CheckReducedDesc took (its tiles fit a launch). tile0 stays 0: a batched launch sets it in its own copy.
inline int PlaceBlock(const JxlHipReducedDesc& d, const BlockLayout& l, float* dc_out, void* block, uintptr_t device_base, ReducedHead* head) {
  const uint64_t tiles = Tiles(d.xsize_blocks, d.ysize_blocks);
  uint8_t* p = static_cast<uint8_t*>(block);
  if (l.ep_bytes) memcpy(p + l.ep, d.dc_extra_precision, l.ep_bytes);
  memcpy(p + l.q, d.dc_quantised, l.q_bytes);
  ReducedHead h;
  memset(&h, 0, sizeof(h));
  h.q = reinterpret_cast<const int32_t*>(device_base + l.q);
  h.ep = l.ep_bytes ? reinterpret_cast<const uint8_t*>(device_base + l.ep) : nullptr;
  h.dc_out = dc_out;
  h.xs = d.xsize_blocks;
  h.ys = d.ysize_blocks;
  h.xgroups = (d.xsize_blocks + kDcGroupBlocks - 1) / kDcGroupBlocks;
  h.smoothing = d.dc_smoothing ? 1 : 0;
  for (int c = 0; c < 3; c++) h.step[c] = d.dc_step[c];
  h.cfl_x = d.dc_cfl_x;
  h.cfl_b = d.dc_cfl_b;
  h.tile0 = 0;
  h.tiles = uint32_t(tiles);
  h.tiles_x = TilesX(d.xsize_blocks);
  *head = h;
  return 0;
}

// ---- the descriptor array of a batched launch: the contexts' descriptors side by side (desc_bytes each, every one
// beginning with its ReducedHead), tile origins running. BatchBytes bounds the block.
inline size_t BatchBytes(size_t n, size_t desc_bytes) { return n * desc_bytes; }
// Copies descriptor i from descs[i] into `block` (BatchBytes(n, desc_bytes) bytes of room in `room`) and sets its tile0;
// *total = the launch's tiles. JXLHIP_ERR_INVALID_ARGUMENT when the room is too small or a descriptor has no tiles,
// JXLHIP_ERR_UNSUPPORTED when the tiles pass kMaxLaunchTiles; nothing past the room is written.
inline int PlaceBatch(const void* const* descs, size_t n, size_t desc_bytes, void* block, size_t room, uint32_t* total) {
  if (!n || desc_bytes < sizeof(ReducedHead) || n > room / desc_bytes) return JXLHIP_ERR_INVALID_ARGUMENT;
  uint64_t at = 0;
  uint8_t* p = static_cast<uint8_t*>(block);
  for (size_t i = 0; i < n; i++) {
    ReducedHead h;
    memcpy(&h, descs[i], sizeof(h));
    if (!h.tiles) return JXLHIP_ERR_INVALID_ARGUMENT;
    h.tile0 = uint32_t(at);
    at += h.tiles;
    if (at > kMaxLaunchTiles) return JXLHIP_ERR_UNSUPPORTED;
    memcpy(p + i * desc_bytes, descs[i], desc_bytes);
    memcpy(p + i * desc_bytes, &h, sizeof(h));
  }
  *total = uint32_t(at);
  return 0;
}

}  // namespace reduced
}  // namespace jxlhip
#endif  // JXH_REDUCED_PLAN_H_
