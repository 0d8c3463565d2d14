// What the host stream writer (csrc/enc/jxl_enc.cc) and the host side of the device forward path (csrc/hip/jxl_hip_api.hip)
// must state identically: float32 arithmetic whose results the two are compared on bit for bit, and the walk over a
// caller's ANS tables that keeps every index formed from them in bounds. Host code only; one text, two compilers.
#ifndef JXH_ENC_SHARED_H_
#define JXH_ENC_SHARED_H_

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../../include/jxl_amd_hip.h"  // JxlHipEncAnsDesc, JxlHipEncEstimateDesc, JxlHipEncAcsCandidate

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
