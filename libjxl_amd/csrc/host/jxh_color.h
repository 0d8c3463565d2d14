// libjxl_amd host front-end: the output description of the XYB colour stage for an enum colour encoding (no CMS).
// Follows: reference lib/jxl/dec_xyb.cc:127-250 (CanOutputToColorEncoding, SetColorEncoding: the inverse opsin matrix
// towards the target primaries and white point, luminances, inverse gamma), lib/jxl/cms/jxl_cms_internal.h:43-126
// (PrimariesToXYZ, Bradford AdaptToXYZD50, PrimariesToXYZD50), render_pipeline/stage_tone_mapping.cc:30-76 (which tone
// mapper), cms/tone_mapping.h:23-113 (Rec2408ToneMapperBase constants, HlgOOTF_Base), tone_mapping-inl.h:115-140
// (HlgOOTF::ToSceneLight), stage_from_linear.cc:146-168 (which transfer function).
#ifndef JXH_COLOR_H_
#define JXH_COLOR_H_

#include <jxl/color_encoding.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "jxh_headers.h"
#include "../../../include/jxl_amd_hip.h"

namespace jxh {

// Chromaticities of the enum white points and primaries (color_encoding_cms.h)
static const double kSrgbPrimariesXy[6] = {0.639998686, 0.330010138, 0.300003784, 0.600003357, 0.150002046, 0.059997204};
static const double k2100PrimariesXy[6] = {0.708, 0.292, 0.170, 0.797, 0.131, 0.046};
static const double kP3PrimariesXy[6] = {0.680, 0.320, 0.265, 0.690, 0.150, 0.060};

// The colour encoding an image header codes, in the form of the public API (custom values in full precision).
static inline void EncodingFromHeader(const ImageHeader& ih, JxlColorEncoding* ce) {
  memset(ce, 0, sizeof(*ce));
  ce->color_space = ih.gray ? JXL_COLOR_SPACE_GRAY : JXL_COLOR_SPACE_RGB;
  ce->white_point = JxlWhitePoint(ih.white_point);
  switch (ih.white_point) {
    case 2: ce->white_point_xy[0] = ih.white_xy[0] * 1e-6; ce->white_point_xy[1] = ih.white_xy[1] * 1e-6; break;
    case 10: ce->white_point_xy[0] = ce->white_point_xy[1] = 1.0 / 3; break;
    case 11: ce->white_point_xy[0] = 0.314; ce->white_point_xy[1] = 0.351; break;
    default: ce->white_point_xy[0] = 0.3127; ce->white_point_xy[1] = 0.3290; break;
  }
  ce->primaries = JxlPrimaries(ih.primaries);
  double xy[6];
  for (int i = 0; i < 6; i++)
    xy[i] = ih.primaries == 2 ? ih.primaries_xy[i] * 1e-6
                              : (ih.primaries == 9 ? k2100PrimariesXy[i] : (ih.primaries == 11 ? kP3PrimariesXy[i] : kSrgbPrimariesXy[i]));
  ce->primaries_red_xy[0] = xy[0]; ce->primaries_red_xy[1] = xy[1];
  ce->primaries_green_xy[0] = xy[2]; ce->primaries_green_xy[1] = xy[3];
  ce->primaries_blue_xy[0] = xy[4]; ce->primaries_blue_xy[1] = xy[5];
  if (ih.have_gamma) {
    ce->transfer_function = JXL_TRANSFER_FUNCTION_GAMMA;
    ce->gamma = ih.gamma * 1e-7;
  } else {
    ce->transfer_function = JxlTransferFunction(ih.transfer_function);
  }
  ce->rendering_intent = JxlRenderingIntent(ih.rendering_intent);
}

// The same encoding (ColorEncoding::SameColorEncoding without the rendering intent, which has no effect without a CMS).
static inline bool SameEncoding(const JxlColorEncoding& a, const JxlColorEncoding& b) {
  if (a.color_space != b.color_space || a.white_point != b.white_point || a.transfer_function != b.transfer_function) return false;
  if (a.white_point == JXL_WHITE_POINT_CUSTOM && (a.white_point_xy[0] != b.white_point_xy[0] || a.white_point_xy[1] != b.white_point_xy[1]))
    return false;
  if (a.color_space == JXL_COLOR_SPACE_RGB) {
    if (a.primaries != b.primaries) return false;
    if (a.primaries == JXL_PRIMARIES_CUSTOM &&
        (a.primaries_red_xy[0] != b.primaries_red_xy[0] || a.primaries_red_xy[1] != b.primaries_red_xy[1] ||
         a.primaries_green_xy[0] != b.primaries_green_xy[0] || a.primaries_green_xy[1] != b.primaries_green_xy[1] ||
         a.primaries_blue_xy[0] != b.primaries_blue_xy[0] || a.primaries_blue_xy[1] != b.primaries_blue_xy[1]))
      return false;
  }
  return a.transfer_function != JXL_TRANSFER_FUNCTION_GAMMA || std::fabs(a.gamma - b.gamma) < 1e-7;
}

typedef double Mat3[3][3];
static inline void Mul3(const Mat3 a, const Mat3 b, Mat3 out) {
  Mat3 t;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) t[i][j] = a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j];
  memcpy(out, t, sizeof(t));
}
static inline bool Inv3(Mat3 m) {
  const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                     m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
  if (!std::isfinite(det) || std::fabs(det) < 1e-300) return false;
  Mat3 t;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const int i1 = (j + 1) % 3, i2 = (j + 2) % 3, j1 = (i + 1) % 3, j2 = (i + 2) % 3;
      t[i][j] = (m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1]) / det;
    }
  memcpy(m, t, sizeof(t));
  return true;
}
// jxl_cms_internal.h:43-69: the RGB -> XYZ matrix of primaries r, g, b (xy) whose white (1, 1, 1) is (wx, wy)
static inline bool PrimariesToXYZ(const double* p, double wx, double wy, Mat3 out) {
  if (!(wx >= 0 && wx <= 1 && wy > 0 && wy <= 1)) return false;
  Mat3 prim = {{p[0], p[2], p[4]}, {p[1], p[3], p[5]}, {1 - p[0] - p[1], 1 - p[2] - p[3], 1 - p[4] - p[5]}};
  Mat3 inv;
  memcpy(inv, prim, sizeof(inv));
  if (!Inv3(inv)) return false;
  const double w[3] = {wx / wy, 1.0, (1 - wx - wy) / wy};
  if (!std::isfinite(w[0]) || !std::isfinite(w[2])) return false;
  for (int i = 0; i < 3; i++) {
    const double s = inv[i][0] * w[0] + inv[i][1] * w[1] + inv[i][2] * w[2];
    for (int r = 0; r < 3; r++) out[r][i] = prim[r][i] * s;
  }
  return true;
}
// jxl_cms_internal.h:71-113: Bradford adaptation of white (wx, wy) to D50
static inline bool AdaptToXYZD50(double wx, double wy, Mat3 out) {
  static const Mat3 kBradford = {{0.8951, 0.2664, -0.1614}, {-0.7502, 1.7135, 0.0367}, {0.0389, -0.0685, 1.0296}};
  static const Mat3 kBradfordInv = {{0.9869929, -0.1470543, 0.1599627}, {0.4323053, 0.5183603, 0.0492912}, {-0.0085287, 0.0400428, 0.9684867}};
  if (!(wx >= 0 && wx <= 1 && wy > 0 && wy <= 1)) return false;
  const double w[3] = {wx / wy, 1.0, (1 - wx - wy) / wy}, w50[3] = {0.96422, 1.0, 0.82521};
  double lms[3], lms50[3];
  for (int i = 0; i < 3; i++) {
    lms[i] = kBradford[i][0] * w[0] + kBradford[i][1] * w[1] + kBradford[i][2] * w[2];
    lms50[i] = kBradford[i][0] * w50[0] + kBradford[i][1] * w50[1] + kBradford[i][2] * w50[2];
    if (lms[i] == 0 || !std::isfinite(lms50[i] / lms[i])) return false;
  }
  Mat3 a = {{lms50[0] / lms[0], 0, 0}, {0, lms50[1] / lms[1], 0}, {0, 0, lms50[2] / lms[2]}};
  Mul3(a, kBradford, a);
  Mul3(kBradfordInv, a, out);
  return true;
}

// ST 2084 inverse EOTF of `nits` cd/m2 (TF_PQ(1.0)::EncodedFromDisplay), in double
static inline double PqEncodeNits(double nits) {
  const double m1 = 2610.0 / 16384, m2 = 2523.0 / 4096 * 128, c1 = 3424.0 / 4096, c2 = 2413.0 / 4096 * 32, c3 = 2392.0 / 4096 * 32;
  const double y = std::pow(std::fabs(nits) / 10000.0, m1);
  return std::pow((c1 + c2 * y) / (1 + c3 * y), m2);
}

// The output description of an XYB image coded in `src` (intensity target `src_intensity`) rendered to `dst` with the
// desired intensity target `desired` (0 = the image's). inv_opsin: the image's OpsinInverseMatrix (row-major). The
// description's tf is the target's transfer function even when the filter kernels can render it themselves (sRGB or
// linear without tone mapping; NeedsGenericWriter tells). Returns false with *err for what cannot be rendered.
static inline bool MakeColorOutput(const JxlColorEncoding& src, float src_intensity, const JxlColorEncoding& dst, float desired,
                                   const float* inv_opsin, JxlHipColorTarget* t, std::string* err) {
  memset(t, 0, sizeof(*t));
  // dec_xyb.cc:127-135,228-232: a grey image renders to grey (D65 here, see ReadColorEncoding), a colour image to RGB
  const bool grey = src.color_space == JXL_COLOR_SPACE_GRAY;
  if (grey ? (dst.color_space != JXL_COLOR_SPACE_GRAY || src.white_point != JXL_WHITE_POINT_D65 || dst.white_point != JXL_WHITE_POINT_D65)
           : (dst.color_space != JXL_COLOR_SPACE_RGB || src.color_space != JXL_COLOR_SPACE_RGB)) {
    *err = grey ? "unsupported: grey XYB output to a colour space other than D65 grey" : "unsupported: XYB output to a colour space other than RGB";
    return false;
  }
  if (!(src_intensity > 0)) {
    *err = "invalid intensity target";
    return false;
  }
  if (!(desired > 0)) desired = src_intensity;
  Mat3 m;
  for (int i = 0; i < 9; i++) m[i / 3][i % 3] = inv_opsin[i];
  double lum[3] = {0.2126, 0.7152, 0.0722};
  if (!grey && (dst.primaries != JXL_PRIMARIES_SRGB || dst.white_point != JXL_WHITE_POINT_D65)) {  // dec_xyb.cc:195-226
    Mat3 srgb_to_xyz, adapt, to_xyz, xyzd50_to_dst;
    const double p[6] = {dst.primaries_red_xy[0], dst.primaries_red_xy[1], dst.primaries_green_xy[0],
                         dst.primaries_green_xy[1], dst.primaries_blue_xy[0], dst.primaries_blue_xy[1]};
    if (!PrimariesToXYZ(kSrgbPrimariesXy, 0.3127, 0.3290, srgb_to_xyz) || !AdaptToXYZD50(0.3127, 0.3290, adapt)) {
      *err = "sRGB primaries";
      return false;
    }
    Mul3(adapt, srgb_to_xyz, srgb_to_xyz);
    if (!PrimariesToXYZ(p, dst.white_point_xy[0], dst.white_point_xy[1], to_xyz) ||
        !AdaptToXYZD50(dst.white_point_xy[0], dst.white_point_xy[1], adapt)) {
      *err = "invalid primaries or white point";
      return false;
    }
    for (int i = 0; i < 3; i++) lum[i] = to_xyz[1][i];
    Mul3(adapt, to_xyz, xyzd50_to_dst);
    if (!Inv3(xyzd50_to_dst)) {
      *err = "invalid primaries or white point";
      return false;
    }
    Mul3(xyzd50_to_dst, srgb_to_xyz, xyzd50_to_dst);
    Mul3(xyzd50_to_dst, m, m);
  }
  if (grey) {  // dec_xyb.cc:228-232: [lum; lum; lum] * inverse matrix: three equal channels, the writer hands out the first
    Mat3 l;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) l[i][j] = lum[j];
    Mul3(l, m, m);
  }
  // InitSIMDInverseMatrix: relative luminance, 1.0 = the image's intensity target (as the sRGB path: jxl_api.cc)
  for (int i = 0; i < 9; i++) t->matrix[i] = float(m[i / 3][i % 3]) * (255.0f / src_intensity);
  for (int i = 0; i < 3; i++) t->luminances[i] = float(lum[i]);
  t->pre_scale = t->post_scale = 1.0f;
  switch (dst.transfer_function) {  // stage_from_linear.cc:146-168
    case JXL_TRANSFER_FUNCTION_LINEAR: t->tf = JXLHIP_TF_LINEAR; break;
    case JXL_TRANSFER_FUNCTION_SRGB: t->tf = JXLHIP_TF_SRGB; break;
    case JXL_TRANSFER_FUNCTION_PQ: t->tf = JXLHIP_TF_PQ; t->pq_display_scale = src_intensity / 10000.0f; break;
    case JXL_TRANSFER_FUNCTION_709: t->tf = JXLHIP_TF_709; break;
    case JXL_TRANSFER_FUNCTION_DCI: t->tf = JXLHIP_TF_GAMMA; t->inv_gamma = float(1.0 / 2.6); break;
    case JXL_TRANSFER_FUNCTION_GAMMA:
      if (!(dst.gamma > 0 && dst.gamma <= 1)) {
        *err = "invalid gamma";
        return false;
      }
      t->tf = JXLHIP_TF_GAMMA;
      t->inv_gamma = float(dst.gamma);
      break;
    case JXL_TRANSFER_FUNCTION_HLG: {  // HlgOOTF::ToSceneLight(desired) ahead of the curve
      const double e = (1 / 1.2) * std::pow(1.111, -std::log2(double(desired) / 1000.0)) - 1;
      t->tf = JXLHIP_TF_HLG;
      t->hlg_exponent = (e < -0.01 || e > 0.01) ? float(e) : 0.0f;
      break;
    }
    default:
      *err = "unsupported: transfer function";
      return false;
  }
  if (desired != src_intensity) {  // stage_tone_mapping.cc:35-70
    if (src.transfer_function == JXL_TRANSFER_FUNCTION_PQ && desired < src_intensity) {
      const double pq_min = PqEncodeNits(0), pq_range = PqEncodeNits(src_intensity) - pq_min;
      const double max_lum = (PqEncodeNits(desired) - pq_min) / pq_range, ks = 1.5 * max_lum - 0.5;
      t->tone = JXLHIP_TONE_REC2408;
      t->gamut_map = 1;
      t->tm_source_peak = src_intensity;
      t->tm_target_peak = desired;
      t->tm_pq_min = float(pq_min);
      t->tm_pq_range = float(pq_range);
      t->tm_inv_pq_range = float(1 / pq_range);
      t->tm_min_lum = float((PqEncodeNits(0) - pq_min) / pq_range);
      t->tm_max_lum = float(max_lum);
      t->tm_ks = float(ks);
      t->tm_inv_one_minus_ks = float(1 / std::max(1e-6, 1 - ks));
      t->tm_normalizer = src_intensity / desired;
      t->tm_inv_target_peak = 1.0f / desired;
    } else if (src.transfer_function == JXL_TRANSFER_FUNCTION_HLG && dst.transfer_function != JXL_TRANSFER_FUNCTION_HLG) {
      const double e = std::pow(1.111, std::log2(double(desired) / src_intensity)) - 1;
      const bool apply = e < -0.01 || e > 0.01;
      t->tone = JXLHIP_TONE_HLG_OOTF;
      t->tone_exponent = apply ? float(e) : 0.0f;
      t->gamut_map = apply && e < 0 ? 1 : 0;
    }
    if (t->tone && dst.transfer_function == JXL_TRANSFER_FUNCTION_PQ) {
      t->pre_scale = 10000.0f / src_intensity;
      t->post_scale = desired / 10000.0f;
    }
  }
  return true;
}
// The matrix of a frame whose colour stage nobody described (ColorOutput inactive): the image's own inverse opsin matrix
// scaled to relative luminance, for a grey image behind the luminance rows of MakeColorOutput.
static inline void OwnMatrix(const ImageHeader& ih, float* out) {
  const float scale = 255.0f / ih.intensity_target;
  for (int i = 0; i < 9; i++) out[i] = ih.inv_opsin[i] * scale;
  if (!ih.gray || !ih.xyb_encoded) return;
  const double lum[3] = {0.2126, 0.7152, 0.0722};
  for (int j = 0; j < 3; j++) {
    const double v = lum[0] * ih.inv_opsin[j] + lum[1] * ih.inv_opsin[3 + j] + lum[2] * ih.inv_opsin[6 + j];
    out[j] = out[3 + j] = out[6 + j] = float(v) * scale;
  }
}
// What the decoder hands a frame's upload: the matrix towards the output primaries (scaled by 255 / intensity target),
// whether the filter kernels end linear, and the generic writer's target (target.tf != 0) when they cannot render it.
// Inactive: the image's own inverse opsin matrix and transfer-function flag, as for ICC-tagged and non-XYB images.
struct ColorOutput {
  bool active = false;
  bool linear = false;
  float matrix[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  JxlHipColorTarget target = {};
};
// A target the filter kernels cannot render themselves: the frame takes the generic writer.
static inline bool NeedsGenericWriter(const JxlHipColorTarget& t) {
  return t.tone != JXLHIP_TONE_NONE || (t.tf != JXLHIP_TF_LINEAR && t.tf != JXLHIP_TF_SRGB);
}

}  // namespace jxh
#endif  // JXH_COLOR_H_
