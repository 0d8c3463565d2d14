// libjxl_amd — the colour stage of XYB images whose output encoding is not (linear) sRGB, for gfx950 (MI355X).
// Applied by the generic pixel writers (k_color_out, k_upsample_color, k_modular_output) to the linear RGB that the
// frame's inverse opsin matrix (towards the target primaries, JxlHipColorTarget::matrix) produced:
//   tone mapping (render_pipeline/stage_tone_mapping.cc:30-120; cms/tone_mapping.h:23-175, tone_mapping-inl.h:30-215)
//   -> transfer function (render_pipeline/stage_from_linear.cc:37-99,146-168; cms/transfer_functions-inl.h).
// The curves are the closed forms of the standards (SMPTE ST 2084, BT.2100 HLG, BT.709) with the hardware exp2 / log2,
// where the reference evaluates rational-polynomial fits of them. Every branch on JxlHipColorTarget is wave-uniform.
#ifndef JXL_HIP_COLOR_H_
#define JXL_HIP_COLOR_H_

#include "jxl_hip_kernels.h"

namespace jxlhip {

// x^e for x > 0 (v_log_f32, v_exp_f32)
__device__ __forceinline__ float PowPos(float x, float e) { return exp2f(e * log2f(x)); }

// SMPTE ST 2084 constants
constexpr float kPqM1 = 2610.0f / 16384.0f, kPqM2 = 2523.0f / 4096.0f * 128.0f;
constexpr float kPqC1 = 3424.0f / 4096.0f, kPqC2 = 2413.0f / 4096.0f * 32.0f, kPqC3 = 2392.0f / 4096.0f * 32.0f;

// TF_PQ::EncodedFromDisplay: `scale` maps the value to units of 10000 cd/m2; odd symmetry as the reference.
__device__ __forceinline__ float PqEncode(float v, float scale) {
  const float a = fabsf(v) * scale;
  const float y = a > 0.0f ? PowPos(a, kPqM1) : 0.0f;
  const float r = PowPos(fmaf(kPqC2, y, kPqC1) / fmaf(kPqC3, y, 1.0f), kPqM2);
  return copysignf(r, v);
}
// TF_PQ(1.0)::DisplayFromEncoded: cd/m2
__device__ __forceinline__ float PqDecodeNits(float e) {
  const float a = fabsf(e);
  const float p = a > 0.0f ? PowPos(a, 1.0f / kPqM2) : 0.0f;
  const float num = fmaxf(p - kPqC1, 0.0f), den = fmaf(-kPqC3, p, kPqC2);
  const float r = num > 0.0f ? PowPos(num / den, 1.0f / kPqM1) * 10000.0f : 0.0f;
  return copysignf(r, e);
}
// TF_HLG::EncodedFromDisplay (BT.2100): sqrt(3 x) up to 1/12, a ln(12 x - b) + c above; odd symmetry
__device__ __forceinline__ float HlgEncode(float v) {
  constexpr float kA = 0.17883277f, kB = 0.28466892f, kC = 0.55991073f, kLn2 = 0.69314718055994531f;
  const float x = fabsf(v);
  const float r = x <= 1.0f / 12 ? __builtin_amdgcn_sqrtf(3.0f * x) : fmaf(kA * kLn2, log2f(fmaf(12.0f, x, -kB)), kC);
  return copysignf(r, v);
}
// TF_709::EncodedFromDisplay
__device__ __forceinline__ float Rec709Encode(float v) {
  return v <= 0.018f ? 4.5f * v : fmaf(1.099f, PowPos(v, 0.45f), -0.099f);
}

__device__ __forceinline__ float TargetLuminance(const JxlHipColorTarget& t, float r, float g, float b) {
  return fmaf(t.luminances[0], r, fmaf(t.luminances[1], g, t.luminances[2] * b));
}
// HlgOOTF::Apply: multiply by luminance^exponent, at most 1e9. A pixel whose luminance is not positive (black, or out of
// gamut) is left as it is: the reference's power of such a luminance is undefined (NaN, or the cap times rounding noise).
__device__ __forceinline__ void HlgOotf(const JxlHipColorTarget& t, float exponent, float* r, float* g, float* b) {
  const float lum = TargetLuminance(t, *r, *g, *b);
  const float ratio = lum > 0.0f ? fminf(PowPos(lum, exponent), 1e9f) : 1.0f;
  *r *= ratio;
  *g *= ratio;
  *b *= ratio;
}
// Rec2408ToneMapper::ToneMap (tone_mapping-inl.h:36-75)
__device__ __forceinline__ void Rec2408ToneMap(const JxlHipColorTarget& t, float* r, float* g, float* b) {
  const float lum = t.tm_source_peak * TargetLuminance(t, *r, *g, *b);
  const float npq = fminf(1.0f, (PqEncode(lum, 1.0f / 10000.0f) - t.tm_pq_min) * t.tm_inv_pq_range);
  float e2 = npq;
  if (npq >= t.tm_ks) {
    const float tb = (npq - t.tm_ks) * t.tm_inv_one_minus_ks, tb2 = tb * tb, tb3 = tb2 * tb;
    e2 = fmaf(fmaf(2.0f, tb3, fmaf(-3.0f, tb2, 1.0f)), t.tm_ks,
              fmaf(tb3 + fmaf(-2.0f, tb2, tb), 1.0f - t.tm_ks, fmaf(-2.0f, tb3, 3.0f * tb2) * t.tm_max_lum));
  }
  const float om = 1.0f - e2, om2 = om * om;
  const float e3 = fmaf(t.tm_min_lum, om2 * om2, e2);
  const float e4 = fmaf(e3, t.tm_pq_range, t.tm_pq_min);
  const float new_lum = fminf(t.tm_target_peak, fmaxf(PqDecodeNits(e4), 0.0f));
  const bool use_cap = lum <= 1e-6f;
  const float mul = new_lum / fmaxf(lum, 1e-6f) * t.tm_normalizer, cap = new_lum * t.tm_inv_target_peak;
  *r = use_cap ? cap : *r * mul;
  *g = use_cap ? cap : *g * mul;
  *b = use_cap ? cap : *b * mul;
}
// GamutMap with preserve_saturation 0.1 (tone_mapping-inl.h:170-215)
__device__ __forceinline__ void GamutMap(const JxlHipColorTarget& t, float* r, float* g, float* b) {
  const float lum = TargetLuminance(t, *r, *g, *b);
  float* ch[3] = {r, g, b};
  float mix_sat = 0.0f, mix_lum = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float v = *ch[c], d = v - lum;
    const float inv = 1.0f / (d == 0.0f ? 1.0f : d), over = v * inv;
    mix_sat = d >= 0.0f ? mix_sat : fmaxf(mix_sat, over);
    mix_lum = fmaxf(mix_lum, d <= 0.0f ? mix_sat : over - inv);
  }
  const float mix = __builtin_amdgcn_fmed3f(fmaf(0.1f, mix_sat - mix_lum, mix_lum), 0.0f, 1.0f);
#pragma unroll
  for (int c = 0; c < 3; c++) *ch[c] = fmaf(mix, lum - *ch[c], *ch[c]);
  const float norm = 1.0f / fmaxf(fmaxf(1.0f, *r), fmaxf(*g, *b));
  *r *= norm;
  *g *= norm;
  *b *= norm;
}

__device__ __forceinline__ float TargetTf(const JxlHipColorTarget& t, float v) {
  switch (t.tf) {
    case JXLHIP_TF_SRGB: return LinearToSrgb(v);
    case JXLHIP_TF_PQ: return PqEncode(v, t.pq_display_scale);
    case JXLHIP_TF_HLG: return HlgEncode(v);
    case JXLHIP_TF_709: return Rec709Encode(v);
    case JXLHIP_TF_GAMMA: return v <= 1e-5f ? 0.0f : PowPos(v, t.inv_gamma);
    default: return v;
  }
}

// Linear RGB in the target primaries (1.0 = the image's intensity target) -> the target encoding.
__device__ __forceinline__ void ApplyColorTarget(const JxlHipColorTarget& t, float* r, float* g, float* b) {
  if (t.tone) {
    *r *= t.pre_scale;
    *g *= t.pre_scale;
    *b *= t.pre_scale;
    if (t.tone == JXLHIP_TONE_REC2408) {
      Rec2408ToneMap(t, r, g, b);
    } else if (t.tone_exponent != 0.0f) {
      HlgOotf(t, t.tone_exponent, r, g, b);
    }
    if (t.gamut_map) GamutMap(t, r, g, b);
    *r *= t.post_scale;
    *g *= t.post_scale;
    *b *= t.post_scale;
  }
  if (t.tf == JXLHIP_TF_HLG && t.hlg_exponent != 0.0f) HlgOotf(t, t.hlg_exponent, r, g, b);
  *r = TargetTf(t, *r);
  *g = TargetTf(t, *g);
  *b = TargetTf(t, *b);
}

}  // namespace jxlhip
#endif  // JXL_HIP_COLOR_H_
