// libjxl_amd — the sizes the transform kernels (jxl_hip_kernels.h: k_idct_fast, k_special, k_dct_big, k_chroma_upsample)
// and their launches share, free of HIP constructs: the kernels walk their work by them, and a plain C++ compile
// (csrc/host/jxh_transform_plan.h, the CPU tests) sizes the launches by the very same statement.
#ifndef JXL_HIP_TRANSFORM_ABI_H_
#define JXL_HIP_TRANSFORM_ABI_H_

#include <stddef.h>
#include <stdint.h>

#include "jxl_hip_block_ctx.h"

namespace jxlhip {

constexpr uint32_t kTransformStrategies = 27;

// Which kernel a strategy takes, from the blocks it covers: more than 64 points a side go through global scratch
// (k_dct_big); of the one-block strategies only the DCT is a plain transform, the others are k_special's (IDENTITY,
// DCT2X2, DCT4X4, DCT4X8, DCT8X4, AFV0-3); everything else is k_idct_fast<CX, CY>.
enum TransformClass : int { kFastClass = 0, kSpecialClass, kBigClass };
constexpr TransformClass TransformClassOf(uint32_t s) {
  return (kCoveredX[s] > 8 || kCoveredY[s] > 8) ? kBigClass : ((s != 0 && CoveredBlocks(s) == 1) ? kSpecialClass : kFastClass);
}

// The batched launches of a set take their workgroups from descriptor lists: one per strategy of the fast and special
// classes, and one more for the 8x8 DCT varblocks of chroma-subsampled frames (k_idct_fast<1, 1, CS>), which list 0 leaves out.
constexpr uint32_t kSubsampledList = 21;
constexpr uint32_t kTransformLists = 22;
constexpr bool ListsAreTheSmallClasses() {
  for (uint32_t s = 0; s < kTransformStrategies; s++)
    if ((TransformClassOf(s) == kBigClass) != (s >= kSubsampledList)) return false;
  return true;
}
static_assert(ListsAreTheSmallClasses(), "strategies 0..20 have a descriptor list each, 21..26 are the big class");

// k_idct_fast. Threads per workgroup: one wave (e.g. two 32x32 varblocks, 8.4 KB of LDS; eight 8x8 ones), so that a
// workgroup fits into the LDS the resident entropy workgroups leave free and a barrier stalls one wave only. A varblock
// takes max(rows, columns) threads and an LDS tile of R rows of C + 1 floats.
constexpr int IdctFastThreads(int cx, int cy) { return (void(cx), void(cy), 64); }
constexpr int IdctFastBlockThreads(int cx, int cy) { return (cx > cy ? cx : cy) * 8; }
constexpr int IdctFastBlocksPerWG(int cx, int cy) { return IdctFastThreads(cx, cy) / IdctFastBlockThreads(cx, cy); }
constexpr int IdctFastTileFloats(int cx, int cy) { return (cy * 8) * (cx * 8 + 1); }
constexpr size_t IdctFastLdsBytes(int cx, int cy) { return size_t(IdctFastBlocksPerWG(cx, cy)) * IdctFastTileFloats(cx, cy) * sizeof(float); }

// k_special: 64 threads per varblock (one per pixel).
constexpr int kSpecialBlocksPerWG = 4;
constexpr int kSpecialThreads = 64 * kSpecialBlocksPerWG;

// Varblocks a workgroup of a descriptor-list strategy's kernel handles.
constexpr uint32_t TransformBlocksPerWG(uint32_t s) {
  return TransformClassOf(s) == kFastClass ? uint32_t(IdctFastBlocksPerWG(kCoveredX[s], kCoveredY[s])) : uint32_t(kSpecialBlocksPerWG);
}

// k_chroma_upsample: one thread per output pixel, a workgroup takes this many columns of this many rows.
constexpr int kChromaUpCols = 64, kChromaUpRows = 4;
constexpr int kChromaUpThreads = kChromaUpCols * kChromaUpRows;

// k_dct_big: one workgroup per (varblock, channel), each with two scratch planes of the largest transform's size; a
// launch takes at most as many varblocks as the frame's scratch is sized for.
constexpr uint32_t kBigBlocksPerLaunch = 32, kBigWGsPerBlock = 3;
constexpr int kBigThreads = 256;
constexpr size_t kBigScratchFloatsPerWG = 2 * 65536;
constexpr size_t BigScratchBytes(uint32_t blocks) {
  return size_t(blocks < kBigBlocksPerLaunch ? blocks : kBigBlocksPerLaunch) * kBigWGsPerBlock * kBigScratchFloatsPerWG * sizeof(float);
}

}  // namespace jxlhip

#endif  // JXL_HIP_TRANSFORM_ABI_H_
