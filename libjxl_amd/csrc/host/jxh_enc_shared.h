// What the host stream writer (csrc/enc/jxl_enc.cc) and the host side of the device forward path (csrc/hip/jxl_hip_api.hip)
// must state identically: float32 arithmetic whose results the two are compared on bit for bit, and the walk over a
// caller's ANS tables that keeps every index formed from them in bounds. Host code only; one text, two compilers.
#ifndef JXH_ENC_SHARED_H_
#define JXH_ENC_SHARED_H_

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../../include/jxl_amd_hip.h"  // JxlHipEncAnsDesc

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
