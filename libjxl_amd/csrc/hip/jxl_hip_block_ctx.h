// libjxl_amd — the HIP layer's one statement of the per-strategy tables and of the block-context rules of the AC
// coefficient walk (lib/jxl/dec_group.cc:470-639, ac_context.h, entropy_coder.h). The section-per-workgroup entropy
// kernels, the tokeniser of the encode path and jxlhip_frame_upload's block records all read these; the lane kernel
// (jxl_hip_entropy_lanes.h) keeps its own fused forms. A plain C++ compile (csrc/host/jxh_upload_plan.h, the CPU tests) sees
// the constexpr tables and the rules as inline functions; the __constant__ copies exist under hipcc only.
#ifndef JXL_HIP_BLOCK_CTX_H_
#define JXL_HIP_BLOCK_CTX_H_

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

namespace jxlhip {

// ---------------------------------------------------------------------------------------------- per-strategy tables
// One value per AcStrategy::Type. The k... objects are for host code and constant expressions; device code indexes the
// __constant__ copies below, which are initialised from them (k_epf_sigma alone indexes the constant objects).
template <typename T>
struct PerStrategy {
  T v[27];
  constexpr T operator[](uint32_t s) const { return v[s]; }
};
// ac_strategy.h:130-167 covered_blocks_x / covered_blocks_y
constexpr PerStrategy<uint8_t> kCoveredX = {{1, 1, 1, 1, 2, 4, 1, 2, 1, 4, 2, 4, 1, 1, 1, 1, 1, 1, 8, 4, 8, 16, 8, 16, 32, 16, 32}};
constexpr PerStrategy<uint8_t> kCoveredY = {{1, 1, 1, 1, 2, 4, 2, 1, 4, 1, 4, 2, 1, 1, 1, 1, 1, 1, 8, 8, 4, 16, 16, 8, 32, 32, 16}};
// coeff_order.h:44-46 kStrategyOrder: the coefficient-order bucket
constexpr PerStrategy<uint8_t> kStrategyOrder = {{0, 1, 1, 1, 2, 3, 4, 4, 5, 5, 6, 6, 1, 1, 1, 1, 1, 1, 7, 8, 8, 9, 10, 10, 11, 12, 12}};
// quant_weights.h:352-382 kQuantTable: the kind of dequantisation matrix
constexpr PerStrategy<uint8_t> kStrategyQuantTable = {{0, 1, 2, 3, 4, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 10, 10, 11, 12, 12, 13, 14, 14, 15, 16, 16}};

constexpr uint32_t Log2OfPow2(uint32_t v) { return v <= 1 ? 0 : 1 + Log2OfPow2(v >> 1); }
constexpr uint32_t Log2CoveredX(uint32_t s) { return Log2OfPow2(kCoveredX[s]); }
constexpr uint32_t Log2CoveredY(uint32_t s) { return Log2OfPow2(kCoveredY[s]); }
constexpr uint32_t CoveredBlocks(uint32_t s) { return uint32_t(kCoveredX[s]) * kCoveredY[s]; }
constexpr PerStrategy<uint8_t> MakeLog2Covered() {
  PerStrategy<uint8_t> r = {};
  for (uint32_t s = 0; s < 27; s++) r.v[s] = uint8_t(Log2CoveredX(s) + Log2CoveredY(s));
  return r;
}
constexpr PerStrategy<uint8_t> kLog2Covered = MakeLog2Covered();
// covered_x | covered_y << 8 | log2_covered << 16 | order bucket << 24: one scalar load per varblock (k_entropy_uni)
constexpr PerStrategy<uint32_t> MakeStrategyInfo() {
  PerStrategy<uint32_t> r = {};
  for (uint32_t s = 0; s < 27; s++)
    r.v[s] = uint32_t(kCoveredX[s]) | uint32_t(kCoveredY[s]) << 8 | uint32_t(kLog2Covered[s]) << 16 | uint32_t(kStrategyOrder[s]) << 24;
  return r;
}
constexpr PerStrategy<uint32_t> kStrategyInfo = MakeStrategyInfo();
static_assert(kStrategyInfo[0] == 0x00000101 && kStrategyInfo[18] == 0x07060808 && kStrategyInfo[26] == 0x0C091020, "the packing");
static_assert(kLog2Covered[5] == 4 && kLog2Covered[25] == 9 && (1u << kLog2Covered[23]) == CoveredBlocks(23), "log2 covered");

#ifdef __HIPCC__
__constant__ PerStrategy<uint8_t> c_covered_x = kCoveredX;
__constant__ PerStrategy<uint8_t> c_covered_y = kCoveredY;
__constant__ PerStrategy<uint8_t> c_log2_covered = kLog2Covered;
__constant__ PerStrategy<uint8_t> c_strategy_order = kStrategyOrder;
__constant__ PerStrategy<uint8_t> c_strategy_qtable = kStrategyQuantTable;
__constant__ PerStrategy<uint32_t> c_strategy_info = kStrategyInfo;
#define JXLHIP_RULE __host__ __device__ __forceinline__
#else
#define JXLHIP_RULE inline
#endif

// ---------------------------------------------------------------------------------------------- block-context rules

// ac_context.h:116-121 BlockCtxMap::Context: the bucket of a quant-field value among `nq` buckets (nq - 1 thresholds).
template <typename Thresholds>
JXLHIP_RULE uint32_t QfBucket(uint32_t qf, Thresholds thr, uint32_t nq) {
  uint32_t b = 0;
  for (uint32_t t = 0; t + 1 < nq; t++) b += qf > thr[t];
  return b;
}

// EntropyParams::cs (frame_header.h YCbCrChromaSubsampling): whether channel c has half the frame's columns (bit 2c; rows: 2c + 1).
JXLHIP_RULE uint32_t ChannelHShift(uint32_t cs, uint32_t c) { return (cs >> (2 * c)) & 1u; }
// dec_group.cc:485-491: block (fbx, fby) of the group carries channel c only when it lies on the channel's own grid;
// (lbx, lby) is its cell there, where the channel's non-zero counts live.
JXLHIP_RULE bool ChannelCell(uint32_t cs, uint32_t c, uint32_t fbx, uint32_t fby, uint32_t& lbx, uint32_t& lby) {
  const uint32_t hs = ChannelHShift(cs, c), vs = (cs >> (2 * c + 1)) & 1u;
  lbx = fbx >> hs;
  lby = fby >> vs;
  return ((fbx & hs) | (fby & vs)) == 0;
}
// dec_group.cc:492, 583-588 (qf_row[sbx]): the block context takes the quant field at the channel's own column of the
// frame's row. A subsampled frame has one block per varblock in raster order (jxlhip_frame_upload checks it), so that
// block lies this many entries back in the row.
JXLHIP_RULE uint32_t QfColumnBack(uint32_t fbx, uint32_t lbx) { return fbx - lbx; }

// ac_context.h:116-128 BlockCtxMap::Context: index into the block-context lut.
JXLHIP_RULE uint32_t BctxLutIndex(uint32_t c, uint32_t ord, uint32_t nq, uint32_t qfc, uint32_t ndc, uint32_t dcctx) {
  return ((c * 13 + ord) * nq + qfc) * ndc + dcctx;
}

// entropy_coder.h:25-35 PredictFromTopAndLeft over a channel's 32-wide map of counts: 32, top, left, or their rounded
// mean. `cell(i)` reads entry i of the map.
template <typename Cell>
JXLHIP_RULE uint32_t PredictNonZeros(const Cell& cell, uint32_t lbx, uint32_t lby) {
  if (lbx == 0) return lby ? cell((lby - 1) * 32) : 32u;
  if (lby == 0) return cell(lbx - 1);
  return (cell((lby - 1) * 32 + lbx) + cell(lby * 32 + lbx - 1) + 1) >> 1;
}
// ac_context.h:131-143 NonZeroContext: the bucket of a predicted count (times num_bctx, plus the block context).
JXLHIP_RULE uint32_t NonZeroBucket(uint32_t pred) {
  const uint32_t nzb = pred >= 64 ? 64 : pred;
  return nzb < 8 ? nzb : 4 + nzb / 2;
}
// dec_group.cc:517-521: a count as the map of counts and the zero-density context hold it: per covered block, rounded up.
JXLHIP_RULE uint32_t NonZerosPerBlock(uint32_t nzeros, uint32_t covered, uint32_t log2c) { return (nzeros + covered - 1) >> log2c; }

// ac_context.h:145-149 ZeroDensityContextsOffset, and ac_context.h:63-83 ZeroDensityContext inside it from the tables'
// values for the non-zeros left and the scan position.
JXLHIP_RULE uint32_t ZeroDensityBase(uint32_t num_bctx, uint32_t bctx) { return num_bctx * 37 + 458 * bctx; }
JXLHIP_RULE uint32_t ZeroDensityContext(uint32_t base, uint32_t nnz_ctx, uint32_t freq_ctx, uint32_t prev) {
  return base + (nnz_ctx + freq_ctx) * 2 + prev;
}

// dec_group.cc:536-538: the value a token adds to its coefficient (UnpackSigned, then the pass's shift).
JXLHIP_RULE uint32_t TokenValue(uint32_t u, uint32_t shift) {
  const uint32_t mag = u >> 1, neg = (~u) & 1;
  return (mag ^ (neg - 1)) << shift;
}

// dec_group.cc:716-718: bits of a section's histogram selector, CeilLog2Nonzero(num_histograms).
JXLHIP_RULE uint32_t SelectorBits(uint32_t num_hist) {
  uint32_t hb = 0;
  while ((1u << hb) < num_hist) hb++;
  return hb;
}

}  // namespace jxlhip
#endif  // JXL_HIP_BLOCK_CTX_H_
