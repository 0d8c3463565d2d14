// What the host stream writer (csrc/enc/jxl_enc.cc) and the host side of the device forward path (csrc/hip/jxl_hip_api.hip)
// must state identically: float32 arithmetic whose results the two are compared on bit for bit, and the walk over a
// caller's ANS tables that keeps every index formed from them in bounds. Host code, one text for two compilers; the merge
// walk of the AC-strategy search (JXH_HD below) is compiled as device code as well.
#ifndef JXH_ENC_SHARED_H_
#define JXH_ENC_SHARED_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../../include/jxl_amd_hip.h"  // JxlHipEncAnsDesc, JxlHipEncEstimateDesc, JxlHipEncAcsCandidate, JxlHipEncAcsWalkDesc

namespace jxh {

// The parameters of the adaptive quant field that depend on the distance alone (enc_adaptive_quantization.cc:319-331
// dampen, :397-412 erosion weights, :1268-1270 scale), into any A with w[4] (erosion weights of the four smallest of a
// 3x3 neighbourhood, normalised), mul (scale * dampen) and add ((1 - dampen) * 0.48 * scale).
template <class A>
inline void EncAqDistanceParams(float target, float rescale, A* a) {
  const float scale = 0.765f / target * rescale;
  const float base_level = 0.48f * scale;
  float dampen = 1.0f;
  if (target >= 2.0f) {
    dampen = 1.0f - ((target - 2.0f) / (14.0f - 2.0f));
    if (dampen < 0) dampen = 0;
  }
  a->mul = scale * dampen;
  a->add = (1.0f - dampen) * base_level;
  const float kMulBase[4] = {0.125f, 0.1f, 0.09f, 0.06f}, kMulAdd[4] = {0.0f, -0.1f, -0.09f, -0.06f};
  const float mul = target < 2.0f ? (2.0f - target) * (1.0f / 2.0f) : 0.0f;
  float norm_sum = 0.0f;
  for (int i = 0; i < 4; i++) {
    a->w[i] = kMulBase[i] + mul * kMulAdd[i];
    norm_sum += a->w[i];
  }
  for (int i = 0; i < 4; i++) a->w[i] *= 0.29959705784054957f / norm_sum;
}

// The six distinct weights of the 5x5 blur of the per-pixel masking (Blur1x1Masking, enc_adaptive_quantization.cc:639-655,
// with the member order of WeightsSymmetric5, convolve.h:30-40), the lower-right quadrant of the kernel being
//   c r R
//   r d L
//   R L D
// into w = {c, r, R, d, L, D}. The sum of the filter is float arithmetic up to the factor 4, double from the 1.0 on.
inline void EncMask1x1Weights(float w[6]) {
  const float k[5] = {0.364911248f, 0.05f, 0.1688888021f, 0.221069183f, 0.306563504f};
  double sum = 1.0 + 4 * (k[0] + k[1] + k[2] + k[4] + 2 * k[3]);
  if (sum < 1e-5) sum = 1e-5;
  const float normalize = static_cast<float>(1.0 / sum);
  w[0] = normalize;
  w[1] = normalize * k[0];
  w[2] = normalize * k[2];
  w[3] = normalize * k[1];
  w[4] = normalize * k[3];
  w[5] = normalize * k[4];
}

// AdjustQuantField (enc_adaptive_quantization.cc:1207-1218) with the frame's own distance: how much of the largest field
// value under a transform of four blocks or more is kept, the rest being the mean.
inline float EncMeanMaxMixer(float distance) {
  float mean_max_mixer = 1.0f;
  if (distance > 1.54138f) mean_max_mixer = std::max(0.0f, 1.0f - (distance - 1.54138f) * 0.56391f);
  return mean_max_mixer;
}

// ---- the cost estimate of the AC-strategy search (jxlhip_enc_estimate_entropy and its CPU double)
// The three weights of EstimateEntropy that depend on the distance alone (AcStrategyHeuristics::Init,
// enc_ac_strategy.cc:1107-1123), float32 as ACSConfig holds them: {info_loss_multiplier, zeros_mul, cost_delta}.
inline void EncEstimateWeights(float distance, float w[3]) {
  const float kBias = 0.13731742964354549f;
  const float ratio = (distance + kBias) / (1.0f + kBias);
  w[0] = 1.2f;
  w[1] = 9.3089059022677905f;
  w[2] = 10.833273317067883f;
  w[0] *= std::pow(ratio, 0.33677806662454718f);
  w[1] *= std::pow(ratio, 0.50990926717963703f);
  w[2] *= std::pow(ratio, 0.36702940662370243f);
}
// The weight of X's share for a transform of num_blocks >= 2 blocks (:499), and the weights of the channels' eighth-power
// losses (:480-485: doubles rounded to float)
inline float EncEstimateXWeight(uint32_t num_blocks) { return float(1.0 + std::min(3.0, num_blocks / 8.0)); }
inline void EncEstimateChannelMul(float m[3]) {
  m[0] = float(std::pow(8.2, 8.0));
  m[1] = float(std::pow(1.0, 8.0));
  m[2] = float(std::pow(1.03, 8.0));
}
// Blocks covered (x, y) and dequantisation-table kind of the pure-DCT strategies the estimate takes (ac_strategy.h:130-167,
// quant_weights.h:352-382); false for any other strategy.
inline bool EncEstimateShape(uint32_t strategy, uint32_t* cx, uint32_t* cy, uint32_t* kind) {
  switch (strategy) {
    case 0: *cx = 1, *cy = 1, *kind = 0; return true;    // 8x8
    case 4: *cx = 2, *cy = 2, *kind = 4; return true;    // 16x16
    case 5: *cx = 4, *cy = 4, *kind = 5; return true;    // 32x32
    case 6: *cx = 1, *cy = 2, *kind = 6; return true;    // 16x8 (rows x columns)
    case 7: *cx = 2, *cy = 1, *kind = 6; return true;    // 8x16
    case 8: *cx = 1, *cy = 4, *kind = 7; return true;    // 32x8
    case 9: *cx = 4, *cy = 1, *kind = 7; return true;    // 8x32
    case 10: *cx = 2, *cy = 4, *kind = 8; return true;   // 32x16
    case 11: *cx = 4, *cy = 2, *kind = 8; return true;   // 16x32
    case 18: *cx = 8, *cy = 8, *kind = 11; return true;  // 64x64
    case 19: *cx = 4, *cy = 8, *kind = 12; return true;  // 64x32
    case 20: *cx = 8, *cy = 4, *kind = 12; return true;  // 32x64
    default: return false;
  }
}
// Everything both forms check before they touch a plane: pointers, sizes, the tables of every kind a candidate uses, and
// each candidate inside the planes and inside one 64x64 tile. *total_area: the samples of all candidates together.
inline bool EncEstimateArgsOk(const JxlHipEncEstimateDesc* d, const JxlHipEncAcsCandidate* cand, size_t n, const float* estimates, size_t* total_area) {
  if (!d || (n && (!cand || !estimates))) return false;
  if (!d->xyb || !d->quant_field || !d->mask1x1 || !d->ytox || !d->ytob || !d->dequant) return false;
  if (!d->xsize || !d->ysize || (d->xsize & 7) || (d->ysize & 7) || d->xsize > (1u << 18) || d->ysize > (1u << 18)) return false;
  if (!(d->distance > 0) || !std::isfinite(d->distance)) return false;
  for (int k = 0; k < 17; k++)
    if (size_t(d->dequant_offset[k]) + 3 * size_t(d->dequant_size[k]) > d->dequant_floats) return false;
  const uint32_t xb = d->xsize / 8, yb = d->ysize / 8;
  size_t area = 0;
  for (size_t i = 0; i < n; i++) {
    uint32_t cx, cy, kind;
    if (!EncEstimateShape(cand[i].strategy, &cx, &cy, &kind)) return false;
    if (d->dequant_size[kind] != cx * cy * 64) return false;
    if (cand[i].bx >= xb || cand[i].by >= yb || cx > xb - cand[i].bx || cy > yb - cand[i].by) return false;
    if ((cand[i].bx & 7) + cx > 8 || (cand[i].by & 7) + cy > 8) return false;
    if (!std::isfinite(cand[i].entropy_mul)) return false;
    area += size_t(cx) * cy * 64;
  }
  if (total_area) *total_area = area;
  return true;
}

// ---- the merge walk of the AC-strategy search (ProcessRectACS, enc_ac_strategy.cc:827-1059, with TryMergeAcs :618-653,
// SetEntropyForTransform :655-665, FindBestFirstLevelDivisionForSquare :703-825 and the two crossing tests :302-362), for
// decoding_speed_tier 0 and DCT as the only 8x8 kind. Every estimate the walk could ask for is in a table before it starts
// (an estimate depends on the candidate alone; the walk's state only decides whether it is asked for), so the walk is
// float32 additions in the reference's raster orders, std::min and <. One text for the CPU double (csrc/enc/jxl_enc.cc), the
// launch layer and the kernel (k_enc_acs_walk, csrc/hip/jxl_hip_enc.h): JXH_HD makes it device code there as well, and every
// function that adds floats turns contraction off for itself.
#if defined(__HIPCC__)
#define JXH_HD __host__ __device__ __forceinline__
#else
#define JXH_HD inline
#endif

// The ten kinds the walk places, in the order of the table: 8x8, 16x8, 8x16, 16x16, 32x16, 16x32, 32x32, 64x32, 32x64, 64x64
// (rows x columns, as the reference names them). Blocks covered are 1 << log2; the multipliers are the reference's
// entropy_mul16X8 .. entropy_mul64X64 (:892-897), both rectangles of a square taking the rectangle's; 1 (0.8 / 0.8) for the 8x8.
constexpr uint32_t kAcsWalkKinds = 10, kAcsWalkTileFloats = kAcsWalkKinds * 64;
JXH_HD uint32_t AcsWalkLog2X(uint32_t kind) { return uint32_t(0x3322211100ull >> (4 * kind)) & 15u; }
JXH_HD uint32_t AcsWalkLog2Y(uint32_t kind) { return uint32_t(0x3232121010ull >> (4 * kind)) & 15u; }
JXH_HD uint32_t AcsWalkStrategy(uint32_t kind) {
  return kind == 0 ? 0u : kind == 1 ? 6u : kind == 2 ? 7u : kind == 3 ? 4u : kind == 4 ? 10u : kind == 5 ? 11u : kind == 6 ? 5u : kind == 7 ? 19u : kind == 8 ? 20u : 18u;
}
inline float AcsWalkEntropyMul(uint32_t kind) {
  const float m[kAcsWalkKinds] = {1.0f, 1.21f, 1.21f, 1.34f, 1.49f, 1.49f, 1.48f, 2.25f, 2.25f, 2.25f};
  return m[kind];
}
// What the 8x8 estimate, loss included, is multiplied by (:863-866: the three constants are floats)
inline float AcsWalkMul8x8(float distance) { return 1.0f + (-0.4f) / (distance + 1.4f); }

// The table the walk reads: per 64x64 tile (raster order) [kind][cy][cx] floats, (cx, cy) the candidate's top-left block
// inside the tile; the estimate already carries the kind's multiplier. Entries nothing asks for are never read.
inline size_t AcsWalkTableIndex(size_t tile, uint32_t kind, uint32_t cx, uint32_t cy) { return tile * kAcsWalkTileFloats + kind * 64 + cy * 8 + cx; }

// The candidates a walk over a tile of w x h blocks can ask for, one bit (cy * 8 + cx) per kind. The aligned walk: every
// candidate aligned to its own size in both directions that fits (the squares' halves, and the odd last rows' and columns'
// TryMergeAcs, come to exactly that). The floating passes (:1033-1057, step 1) add the 16-level square and its four halves
// at every position not even in both coordinates, the 32-level one at every position not a multiple of four in both.
inline void AcsWalkTileAsks(uint32_t w, uint32_t h, uint32_t floating, uint64_t asked[kAcsWalkKinds]) {
  for (uint32_t k = 0; k < kAcsWalkKinds; k++) {
    asked[k] = 0;
    const uint32_t kx = 1u << AcsWalkLog2X(k), ky = 1u << AcsWalkLog2Y(k);
    for (uint32_t cy = 0; cy + ky <= h; cy += ky)
      for (uint32_t cx = 0; cx + kx <= w; cx += kx) asked[k] |= uint64_t(1) << (cy * 8 + cx);
  }
  if (!floating) return;
  auto square = [&](uint32_t blocks, uint32_t jxk, uint32_t cx, uint32_t cy) {  // kinds jxk, jxk + 1 (KXJ), jxk + 2 (JXJ)
    const uint32_t half = blocks / 2;
    asked[jxk] |= (uint64_t(1) << (cy * 8 + cx)) | (uint64_t(1) << (cy * 8 + cx + half));
    asked[jxk + 1] |= (uint64_t(1) << (cy * 8 + cx)) | (uint64_t(1) << ((cy + half) * 8 + cx));
    asked[jxk + 2] |= uint64_t(1) << (cy * 8 + cx);
  };
  for (uint32_t cy = 0; cy + 1 < h; cy++)
    for (uint32_t cx = 0; cx + 1 < w; cx++)
      if ((cy | cx) % 2 != 0) square(2, 1, cx, cy);
  for (uint32_t cy = 0; cy + 3 < h; cy++)
    for (uint32_t cx = 0; cx + 3 < w; cx++)
      if ((cy | cx) % 4 != 0) square(4, 4, cx, cy);
}

// The sizes a walk is defined for: blocks per side as the forward path has them, and a table whose indices fit 32 bits.
inline bool AcsWalkSizeOk(uint32_t xb, uint32_t yb) {
  if (!xb || !yb || xb > (1u << 15) || yb > (1u << 15)) return false;
  return uint64_t((xb + 7) / 8) * ((yb + 7) / 8) * kAcsWalkTileFloats < (uint64_t(1) << 31);
}
// The candidate list of a frame of xb x yb blocks, grouped by kind (kind k is cand[first[k]] .. cand[first[k + 1]]), tiles in
// raster order inside a kind and positions in raster order inside a tile; index[i] is the table entry of cand[i].
struct AcsWalkList {
  std::vector<JxlHipEncAcsCandidate> cand;
  std::vector<uint32_t> index;
  size_t first[kAcsWalkKinds + 1];
};
inline bool AcsWalkCandidates(uint32_t xb, uint32_t yb, uint32_t floating, AcsWalkList* out) {
  if (!out || !AcsWalkSizeOk(xb, yb) || floating > 1) return false;
  out->cand.clear();
  out->index.clear();
  const uint32_t tiles_x = (xb + 7) / 8, tiles_y = (yb + 7) / 8;
  for (uint32_t k = 0; k < kAcsWalkKinds; k++) {
    out->first[k] = out->cand.size();
    for (uint32_t ty = 0; ty < tiles_y; ty++)
      for (uint32_t tx = 0; tx < tiles_x; tx++) {
        uint64_t asked[kAcsWalkKinds];
        AcsWalkTileAsks(std::min(8u, xb - tx * 8), std::min(8u, yb - ty * 8), floating, asked);
        for (uint32_t i = 0; i < 64; i++)
          if (asked[k] >> i & 1) {
            out->cand.push_back({AcsWalkStrategy(k), tx * 8 + (i & 7), ty * 8 + (i >> 3), AcsWalkEntropyMul(k)});
            out->index.push_back(uint32_t(AcsWalkTableIndex(size_t(ty) * tiles_x + tx, k, i & 7, i >> 3)));
          }
      }
  }
  out->first[kAcsWalkKinds] = out->cand.size();
  return true;
}
// What both forms of the stand-alone walk check before anything else
inline bool AcsWalkArgsOk(const JxlHipEncAcsWalkDesc* d, const float* estimates, const uint8_t* acs) {
  if (!d || !estimates || !acs || !AcsWalkSizeOk(d->xb, d->yb) || d->floating > 1) return false;
  return d->distance > 0 && std::isfinite(d->distance);
}

// The state of one tile's walk: the tile's table, entropy_estimate[64], the strategy image of the tile as (kind << 1) | first
// on an 8 x 8 grid, priority[64], and the tile's size in blocks (smaller than 8 at the right and bottom frame edges).
// Coordinates are the tile's own: the reference's bx, by are multiples of 8, so `x % 8`, `x & ~7` and the image-size tests
// read the same on them (a coordinate of 8 is either beyond the image or a multiple of 8: both return false).
struct AcsWalkState {
  const float* est;
  float* entropy;
  uint8_t* acs;
  uint8_t* priority;
  uint32_t w, h;
};
JXH_HD bool AcsWalkCrossesH(const AcsWalkState& s, uint32_t start_x, uint32_t y, uint32_t end_x) {  // :302-330
  if (start_x >= s.w || y >= s.h) return false;
  if (y % 8 == 0) return false;
  end_x = end_x < s.w ? end_x : s.w;
  while (start_x != 0 && !(s.acs[y * 8 + start_x] & 1)) --start_x;
  for (uint32_t x = start_x; x < end_x;) {
    const uint32_t a = s.acs[y * 8 + x];
    if (a & 1) x += 1u << AcsWalkLog2X(a >> 1);
    else return true;
  }
  return false;
}
JXH_HD bool AcsWalkCrossesV(const AcsWalkState& s, uint32_t x, uint32_t start_y, uint32_t end_y) {  // :332-362
  if (x >= s.w || start_y >= s.h) return false;
  if (x % 8 == 0) return false;
  end_y = end_y < s.h ? end_y : s.h;
  while (start_y != 0 && !(s.acs[start_y * 8 + x] & 1)) --start_y;
  for (uint32_t y = start_y; y < end_y;) {
    const uint32_t a = s.acs[y * 8 + x];
    if (a & 1) y += 1u << AcsWalkLog2Y(a >> 1);
    else return true;
  }
  return false;
}
// The four tests at the head of the square function (:725-732): does a transform placed earlier reach across the outline
// of the blocks x blocks_y rectangle at (cx, cy)?
JXH_HD bool AcsWalkLeaks(const AcsWalkState& s, uint32_t cx, uint32_t cy, uint32_t bx, uint32_t by) {
  return AcsWalkCrossesH(s, cx, cy, cx + bx) || AcsWalkCrossesH(s, cx, cy + by, cx + bx) || AcsWalkCrossesV(s, cx, cy, cy + by) ||
         AcsWalkCrossesV(s, cx + bx, cy, cy + by);
}
JXH_HD void AcsWalkSet(const AcsWalkState& s, uint32_t cx, uint32_t cy, uint32_t kind) {  // AcStrategyImage::Set
  const uint32_t kx = 1u << AcsWalkLog2X(kind), ky = 1u << AcsWalkLog2Y(kind);
  for (uint32_t iy = 0; iy < ky; iy++)
    for (uint32_t ix = 0; ix < kx; ix++) s.acs[(cy + iy) * 8 + cx + ix] = uint8_t((kind << 1) | ((iy | ix) == 0 ? 1 : 0));
}
JXH_HD void AcsWalkSetEntropy(const AcsWalkState& s, uint32_t cx, uint32_t cy, uint32_t kind, float entropy) {  // :655-665
  const uint32_t kx = 1u << AcsWalkLog2X(kind), ky = 1u << AcsWalkLog2Y(kind);
  for (uint32_t dy = 0; dy < ky; dy++)
    for (uint32_t dx = 0; dx < kx; dx++) s.entropy[(cy + dy) * 8 + cx + dx] = 0.0f;
  s.entropy[cy * 8 + cx] = entropy;
}
// Two guards are not the reference's. They make every placement cover whole earlier transforms only, whatever the table
// holds, so that the strategy image is a valid tiling by construction (the kernels after the walk index by it); on a table of
// finite estimates above zero neither can refuse anything (tests/test_acs_walk.py holds them to that):
//   - TryMergeAcs makes the four tests of AcsWalkLeaks before it accepts. In a full tile the reference tries DCT32X64 at
//     (0, 4) after the 64-level square, whose halves carry no priority; over a DCT64X32 placed by that square it would leave
//     an orphaned half. With finite positive estimates TryMergeAcs has placed that DCT64X32 itself, with its priority.
//   - the square function places a half only if it took its estimate: the reference's FLT_MAX stand-in for "not taken" is
//     below an infinite sum.
// TryMergeAcs (:618-653)
JXH_HD void AcsWalkTryMerge(const AcsWalkState& s, uint32_t kind, uint32_t cx, uint32_t cy, uint8_t candidate_priority) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const uint32_t kx = 1u << AcsWalkLog2X(kind), ky = 1u << AcsWalkLog2Y(kind);
  float entropy_current = 0;
  for (uint32_t iy = 0; iy < ky; ++iy)
    for (uint32_t ix = 0; ix < kx; ++ix) {
      if (s.priority[(cy + iy) * 8 + (cx + ix)] >= candidate_priority) return;
      entropy_current += s.entropy[(cy + iy) * 8 + (cx + ix)];
    }
  const float entropy_candidate = s.est[kind * 64 + cy * 8 + cx];
  if (entropy_candidate >= entropy_current) return;
  if (AcsWalkLeaks(s, cx, cy, kx, ky)) return;
  for (uint32_t iy = 0; iy < ky; iy++)
    for (uint32_t ix = 0; ix < kx; ix++) {
      s.entropy[(cy + iy) * 8 + cx + ix] = 0;
      s.priority[(cy + iy) * 8 + cx + ix] = candidate_priority;
    }
  AcsWalkSet(s, cx, cy, kind);
  s.entropy[cy * 8 + cx] = entropy_candidate;
}
// FindBestFirstLevelDivisionForSquare (:703-825) with allow_square_transform true; jxk is the kind of the tall half, jxk + 1
// the wide one's, jxk + 2 the square's.
JXH_HD void AcsWalkSquare(const AcsWalkState& s, uint32_t blocks, uint32_t jxk, uint32_t cx, uint32_t cy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const uint32_t half = blocks / 2, kxj = jxk + 1, jxj = jxk + 2;
  if (AcsWalkLeaks(s, cx, cy, blocks, blocks)) return;
  const bool allow_JXK = !AcsWalkCrossesV(s, cx + half, cy, cy + blocks);
  const bool allow_KXJ = !AcsWalkCrossesH(s, cx, cy + half, cx + blocks);
  float entropy[2][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
  for (uint32_t dy = 0; dy < blocks; ++dy)
    for (uint32_t dx = 0; dx < blocks; ++dx) entropy[dy / half][dx / half] += s.entropy[(cy + dy) * 8 + (cx + dx)];
  const float kMax = 3.402823466e+38f;
  float entropy_JXK_left = kMax, entropy_JXK_right = kMax, entropy_KXJ_top = kMax, entropy_KXJ_bottom = kMax;
  const bool take_left = allow_JXK && uint32_t(s.acs[cy * 8 + cx] >> 1) != jxk, take_right = allow_JXK && uint32_t(s.acs[cy * 8 + cx + half] >> 1) != jxk;
  const bool take_top = allow_KXJ && uint32_t(s.acs[cy * 8 + cx] >> 1) != kxj, take_bottom = allow_KXJ && uint32_t(s.acs[(cy + half) * 8 + cx] >> 1) != kxj;
  if (take_left) entropy_JXK_left = s.est[jxk * 64 + cy * 8 + cx];
  if (take_right) entropy_JXK_right = s.est[jxk * 64 + cy * 8 + cx + half];
  if (take_top) entropy_KXJ_top = s.est[kxj * 64 + cy * 8 + cx];
  if (take_bottom) entropy_KXJ_bottom = s.est[kxj * 64 + (cy + half) * 8 + cx];
  const float entropy_JXJ = s.est[jxj * 64 + cy * 8 + cx];
  const float left = entropy[0][0] + entropy[1][0], right = entropy[0][1] + entropy[1][1];
  const float top = entropy[0][0] + entropy[0][1], bottom = entropy[1][0] + entropy[1][1];
  // (std::min(a, b) is b < a ? b : a)
  const float costJxN = (left < entropy_JXK_left ? left : entropy_JXK_left) + (right < entropy_JXK_right ? right : entropy_JXK_right);
  const float costNxJ = (top < entropy_KXJ_top ? top : entropy_KXJ_top) + (bottom < entropy_KXJ_bottom ? bottom : entropy_KXJ_bottom);
  if (entropy_JXJ < costJxN && entropy_JXJ < costNxJ) {
    AcsWalkSet(s, cx, cy, jxj);
    AcsWalkSetEntropy(s, cx, cy, jxj, entropy_JXJ);
  } else if (costJxN < costNxJ) {
    if (take_left && entropy_JXK_left < left) {
      AcsWalkSet(s, cx, cy, jxk);
      AcsWalkSetEntropy(s, cx, cy, jxk, entropy_JXK_left);
    }
    if (take_right && entropy_JXK_right < right) {
      AcsWalkSet(s, cx + half, cy, jxk);
      AcsWalkSetEntropy(s, cx + half, cy, jxk, entropy_JXK_right);
    }
  } else {
    if (take_top && entropy_KXJ_top < top) {
      AcsWalkSet(s, cx, cy, kxj);
      AcsWalkSetEntropy(s, cx, cy, kxj, entropy_KXJ_top);
    }
    if (take_bottom && entropy_KXJ_bottom < bottom) {
      AcsWalkSet(s, cx, cy + half, kxj);
      AcsWalkSetEntropy(s, cx, cy + half, kxj, entropy_KXJ_bottom);
    }
  }
}
// ProcessRectACS (:860-1058) from the 8x8 estimates on. The merge table is kTransformsForMerge (:907-920) as kinds of this
// header: {16X8, 2}, {8X16, 2}, {16X32, 4}, {32X16, 4}, {64X32, 6}, {32X64, 6}; the loop body is the reference's, test by test.
JXH_HD void AcsWalkTile(const AcsWalkState& s, float mul8x8, uint32_t floating) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (uint32_t i = 0; i < 64; i++) {
    s.entropy[i] = 0.0f;
    s.priority[i] = 0;
    s.acs[i] = 1;  // (written for the whole grid: the blocks outside a partial tile are never read)
  }
  for (uint32_t iy = 0; iy < s.h; iy++)
    for (uint32_t ix = 0; ix < s.w; ix++) s.entropy[iy * 8 + ix] = s.est[iy * 8 + ix] * mul8x8;
  const uint32_t w = s.w, h = s.h;
  for (uint32_t m = 0; m < 6; m++) {
    const uint32_t kind = m == 0 ? 1u : m == 1 ? 2u : m == 2 ? 5u : m == 3 ? 4u : m == 4 ? 7u : 8u;
    const uint8_t priority = m < 2 ? 2 : m < 4 ? 4 : 6;
    const uint32_t kx = 1u << AcsWalkLog2X(kind), ky = 1u << AcsWalkLog2Y(kind);
    for (uint32_t cy = 0; cy + ky - 1 < h; cy += ky)
      for (uint32_t cx = 0; cx + kx - 1 < w; cx += kx) {
        if (cy + 7 < h && cx + 7 < w) {
          if (kind == 8) {
            if ((cy | cx) % 8 == 0) AcsWalkSquare(s, 8, 7, cx, cy);
            continue;
          } else if (kind == 4) {
            continue;
          }
        }
        if ((kind == 5 && cy % 4 != 0) || (kind == 4 && cx % 4 != 0)) continue;
        if (cy + 3 < h && cx + 3 < w) {
          if (kind == 5) {
            if ((cy | cx) % 4 == 0) AcsWalkSquare(s, 4, 4, cx, cy);
            continue;
          } else if (kind == 4) {
            continue;
          }
        }
        if ((kind == 5 && cy % 4 != 0) || (kind == 4 && cx % 4 != 0)) continue;
        if (cy + 1 < h && cx + 1 < w) {
          if (kind == 2) {
            if ((cy | cx) % 2 == 0) AcsWalkSquare(s, 2, 1, cx, cy);
            continue;
          } else if (kind == 1) {
            continue;
          }
        }
        if ((kind == 2 && cy % 2 == 1) || (kind == 1 && cx % 2 == 1)) continue;
        AcsWalkTryMerge(s, kind, cx, cy, priority);
      }
  }
  if (!floating) return;
  for (uint32_t cy = 0; cy + 1 < h; ++cy)
    for (uint32_t cx = 0; cx + 1 < w; ++cx)
      if ((cy | cx) % 2 != 0) AcsWalkSquare(s, 2, 1, cx, cy);
  for (uint32_t cy = 0; cy + 3 < h; ++cy)
    for (uint32_t cx = 0; cx + 3 < w; ++cx) {
      if ((cy | cx) % 4 == 0) continue;
      AcsWalkSquare(s, 4, 4, cx, cy);
    }
}

// sRGB EOTF of one 8-bit code (transfer_functions-inl.h TF_SRGB)
inline float SrgbEotf8(int code) {
  const float v = float(code) / 255.0f;
  return v <= 0.04045f ? v / 12.92f : std::pow((v + 0.055f) / 1.055f, 2.4f);
}

// The dequantisation multipliers of X and B for x_qm_scale 3 and b_qm_scale 2, what the frame header codes (dec_cache.h:161-162).
inline float EncXDm() { return std::pow(1.25f, 2.0f - 3.0f); }
inline float EncBDm() { return std::pow(1.25f, 2.0f - 2.0f); }

// The tables of an ANS descriptor whose pointers, cluster count (1..256) and log_alpha (5..8) the caller has checked: every
// index an entropy coder forms from them stays inside them. Clusters below num_clusters; per cluster the frequencies sum
// to 4096 with rev_start their running sum (so rev_start + freq <= 4096) and no symbol beyond the alphabet; reverse-map
// entries below 4096. The scalar preconditions (num_ctx, the hybrid-uint configuration) differ by caller and stay there.
inline bool AnsTablesInBounds(const JxlHipEncAnsDesc& d) {
  for (uint32_t i = 0; i < d.num_ctx; i++)
    if (d.ctx_map[i] >= d.num_clusters) return false;
  for (uint32_t k = 0; k < d.num_clusters; k++) {
    uint32_t sum = 0;
    for (uint32_t s = 0; s < 256; s++) {
      const uint32_t fr = d.freq[k * 256 + s];
      if (fr && ((s >> d.log_alpha) || d.rev_start[k * 256 + s] != sum)) return false;
      sum += fr;
      if (sum > 4096) return false;
    }
    if (sum != 4096) return false;
    for (uint32_t i = 0; i < 4096; i++)
      if (d.rev[k * 4096 + i] >= 4096) return false;
  }
  return true;
}

}  // namespace jxh

#endif  // JXH_ENC_SHARED_H_
