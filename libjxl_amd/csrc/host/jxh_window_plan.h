// libjxl_amd — the host plan of a region decode (jxlamd_frame_upload_window): which rectangle of whole 256 x 256 groups a
// box of the output image needs (PlanWindow), for which frames the window is the whole frame (WholeFrameReasonOf), the
// descriptor of the window as a frame of its own (BuildWindowDesc), and the apron of coded DC integers that k_dc_window
// (csrc/hip/jxl_hip_dc_window.h) turns into the window's DC image (PlanDcApron / PackDcApron / CheckDcWindow). Free of HIP,
// one function per rule, so that tests/c/window_kats.cc holds every line of it on the CPU.
#ifndef JXH_WINDOW_PLAN_H_
#define JXH_WINDOW_PLAN_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../../include/jxl_amd_hip.h"
#include "jxh_filter_halo.h"

namespace jxlhip {
namespace window {

constexpr uint32_t kGroupDim = 256;                // pixels of a group's side
constexpr uint32_t kGroupBlocks = kGroupDim / 8;   // blocks
constexpr uint32_t kCflTileBlocks = 8;             // a chroma-from-luma tile is 64 pixels: 4 tiles per group side
constexpr uint32_t kDcGroupBlocks = 256;           // a DC group covers 256 x 256 blocks
constexpr uint64_t kMaxDcWindowSamples = uint64_t(1) << 24;

struct Rect {
  uint32_t x0, y0, xsize, ysize;
};
inline bool operator==(const Rect& a, const Rect& b) { return a.x0 == b.x0 && a.y0 == b.y0 && a.xsize == b.xsize && a.ysize == b.ysize; }

// ---------------------------------------------------------------------------------------------------- orientation
// EXIF numbering 1..8 -> mirror x (1) | mirror y (2) | transpose (4), the bits of PixelOut::orient
// (jxlhip_set_output_orientation; stage_write.cc:441-458). 0 counts as 1.
inline uint32_t OrientBits(uint32_t orientation) {
  static const uint8_t kBits[9] = {0, 0, 1, 3, 2, 4, 6, 7, 5};
  return orientation <= 8 ? kBits[orientation] : 0;
}
// The writer sends pixel (x, y) of an image of xs x ys to column u, row v of the oriented image (PixelOutIndex):
// ox = mirror x ? xs - 1 - x : x, oy likewise; (u, v) = transposed ? (oy, ox) : (ox, oy). The two maps below are that rule
// and its inverse on rectangles.
inline Rect ToOriented(const Rect& r, uint32_t xs, uint32_t ys, uint32_t bits) {
  const uint32_t ox0 = (bits & 1) ? xs - (r.x0 + r.xsize) : r.x0, oy0 = (bits & 2) ? ys - (r.y0 + r.ysize) : r.y0;
  return (bits & 4) ? Rect{oy0, ox0, r.ysize, r.xsize} : Rect{ox0, oy0, r.xsize, r.ysize};
}
inline Rect FromOriented(const Rect& b, uint32_t xs, uint32_t ys, uint32_t bits) {
  const Rect o = (bits & 4) ? Rect{b.y0, b.x0, b.ysize, b.xsize} : b;  // (ox, oy) ranges
  return Rect{(bits & 1) ? xs - (o.x0 + o.xsize) : o.x0, (bits & 2) ? ys - (o.y0 + o.ysize) : o.y0, o.xsize, o.ysize};
}

// ---------------------------------------------------------------------------------------------------- the window
struct FrameGeom {
  uint32_t xsize, ysize;                // pixels
  uint32_t xsize_blocks, ysize_blocks;  // ceil(size / 8)
  uint32_t xsize_groups, ysize_groups;  // ceil(size / 256)
};
inline FrameGeom GeomOf(uint32_t xsize, uint32_t ysize) {
  return FrameGeom{xsize, ysize, (xsize + 7) / 8, (ysize + 7) / 8, (xsize + kGroupDim - 1) / kGroupDim, (ysize + kGroupDim - 1) / kGroupDim};
}

// Every reason PlanWindow refuses for, each stated once there; tests/c/window_kats.cc breaks each.
enum WindowRule : int {
  kWindowRuleFrame,       // a frame of pixels whose block and group counts are those of its size
  kWindowRuleBoxExtents,  // both box extents zero (then the origin too: the whole image) or both non-zero (CheckResizedOut)
  kWindowRuleBoxInside,   // x0 + xsize <= oriented image xsize, y0 + ysize <= ysize, in 64 bits (CheckResizedOut)
  kWindowRuleCount
};

struct WindowPlan {
  Rect need;     // the box in frame pixels, grown by the filters' halo and clipped to the frame
  Rect pixels;   // the window in frame pixels: whole groups (the last column / row ends at the frame's edge)
  Rect blocks;   // the same in 8x8 blocks
  uint32_t gx0, gy0, gxs, gys;  // and in groups
  Rect box;      // the caller's box in the oriented coordinates of the window image: what gets bound
  uint32_t groups_taken, groups_in_frame;
};

// Step 2: the box of the oriented output image as a rectangle of the frame.
inline Rect BoxInFrame(const FrameGeom& g, uint32_t orient_bits, const Rect& box) { return FromOriented(box, g.xsize, g.ysize, orient_bits); }
// Step 3: grown by `halo` pixels on every side, clipped to the frame.
inline Rect GrowAndClip(const FrameGeom& g, const Rect& r, uint32_t halo) {
  const uint32_t x0 = r.x0 > halo ? r.x0 - halo : 0, y0 = r.y0 > halo ? r.y0 - halo : 0;
  const uint64_t x1 = uint64_t(r.x0) + r.xsize + halo, y1 = uint64_t(r.y0) + r.ysize + halo;
  return Rect{x0, y0, uint32_t(x1 < g.xsize ? x1 : g.xsize) - x0, uint32_t(y1 < g.ysize ? y1 : g.ysize) - y0};
}
// Step 4: the smallest rectangle of whole groups that covers a non-empty rectangle of the frame, into `w`.
inline void CoverWithGroups(const FrameGeom& g, const Rect& r, WindowPlan* w) {
  w->gx0 = r.x0 / kGroupDim;
  w->gy0 = r.y0 / kGroupDim;
  const uint32_t gx1 = (r.x0 + r.xsize - 1) / kGroupDim + 1, gy1 = (r.y0 + r.ysize - 1) / kGroupDim + 1;
  w->gxs = gx1 - w->gx0;
  w->gys = gy1 - w->gy0;
  const uint32_t px1 = gx1 == g.xsize_groups ? g.xsize : gx1 * kGroupDim, py1 = gy1 == g.ysize_groups ? g.ysize : gy1 * kGroupDim;
  w->pixels = Rect{w->gx0 * kGroupDim, w->gy0 * kGroupDim, px1 - w->gx0 * kGroupDim, py1 - w->gy0 * kGroupDim};
  const uint32_t bx1 = gx1 == g.xsize_groups ? g.xsize_blocks : gx1 * kGroupBlocks, by1 = gy1 == g.ysize_groups ? g.ysize_blocks : gy1 * kGroupBlocks;
  w->blocks = Rect{w->gx0 * kGroupBlocks, w->gy0 * kGroupBlocks, bx1 - w->gx0 * kGroupBlocks, by1 - w->gy0 * kGroupBlocks};
}

// The window of `box` (oriented output coordinates; all zero: the whole image) for a frame whose filters are gab /
// epf_iters and whose output undoes orientation bits `orient_bits`. 0, or JXLHIP_ERR_INVALID_ARGUMENT with the rule.
inline int PlanWindow(const FrameGeom& g, int gab, int epf_iters, uint32_t orient_bits, const Rect& box_in, WindowPlan* out, int* rule = nullptr) {
#define JXH_WINDOW_REFUSE(cond, r)          \
  do {                                      \
    if (cond) {                             \
      if (rule) *rule = (r);                \
      return JXLHIP_ERR_INVALID_ARGUMENT;   \
    }                                       \
  } while (0)
  JXH_WINDOW_REFUSE(!g.xsize || !g.ysize || g.xsize > (1u << 30) || g.ysize > (1u << 30), kWindowRuleFrame);
  const FrameGeom want = GeomOf(g.xsize, g.ysize);
  JXH_WINDOW_REFUSE(g.xsize_blocks != want.xsize_blocks || g.ysize_blocks != want.ysize_blocks || g.xsize_groups != want.xsize_groups ||
                        g.ysize_groups != want.ysize_groups,
                    kWindowRuleFrame);
  // 1. what CheckResizedOut refuses of a box, with its arithmetic
  JXH_WINDOW_REFUSE((box_in.xsize == 0) != (box_in.ysize == 0), kWindowRuleBoxExtents);
  JXH_WINDOW_REFUSE(!box_in.xsize && !box_in.ysize && (box_in.x0 || box_in.y0), kWindowRuleBoxExtents);
  const bool transposed = (orient_bits & 4) != 0;
  const uint32_t image_xsize = transposed ? g.ysize : g.xsize, image_ysize = transposed ? g.xsize : g.ysize;
  JXH_WINDOW_REFUSE(uint64_t(box_in.x0) + box_in.xsize > image_xsize || uint64_t(box_in.y0) + box_in.ysize > image_ysize, kWindowRuleBoxInside);
#undef JXH_WINDOW_REFUSE
  const Rect box = box_in.xsize ? box_in : Rect{0, 0, image_xsize, image_ysize};
  WindowPlan w;
  memset(&w, 0, sizeof(w));
  const Rect in_frame = BoxInFrame(g, orient_bits, box);                                      // 2
  w.need = GrowAndClip(g, in_frame, uint32_t(FusedHalo(gab != 0, epf_iters)));                // 3
  CoverWithGroups(g, w.need, &w);                                                             // 4
  // 5. the box where the window image has it: relative to the window, then through the orientation at the window's size
  w.box = ToOriented(Rect{in_frame.x0 - w.pixels.x0, in_frame.y0 - w.pixels.y0, in_frame.xsize, in_frame.ysize}, w.pixels.xsize,
                     w.pixels.ysize, orient_bits);
  w.groups_taken = w.gxs * w.gys;
  w.groups_in_frame = g.xsize_groups * g.ysize_groups;
  *out = w;
  return 0;
}

// ------------------------------------------------------------------------------------------ whole-frame reasons
// Why the window of a frame is the whole frame (the caller then takes jxlamd_frame_upload, the route it had). A reason is
// a report, not an error: nothing is refused that decodes today. Each is stated once, in WholeFrameReasonOf; the first
// that holds in the order of the enum is reported.
enum WholeFrameReason : int {
  kWindowed = 0,            // a true window
  kWholePartial,            // the frame was parsed as reduced or partial (group_absent)
  kWholeUpsampling,         // upsampling above 1
  kWholeSubsampling,        // chroma subsampling
  kWholeNoise,              // noise: its generators are seeded with each group's origin in the frame
  kWholePatches,            // patches
  kWholeSplines,            // splines
  kWholeDcFrame,            // kUseDcFrame
  kWholeAlpha,              // an output that needs the alpha plane (2 or 4 channels; the plane is finished at image size)
  kWholeSingleSection,      // a single-section frame (first_section_bit_offset)
  kWholeOneGroup,           // a frame of one group
  kWholeWindowIsFrame,      // a window that equals the frame
  kWholeReasonCount
};
// (filled by the caller from the parsed frame: csrc/api/jxl_api.cc TraitsOfFrame)
struct FrameTraits {
  bool partial, subsampled, noise, patches, splines, dc_frame, single_section;
  uint32_t upsampling;    // 0 or 1: none
  uint32_t num_channels;  // of the output
};
inline WholeFrameReason WholeFrameReasonOf(const FrameTraits& t, const WindowPlan& w) {
  if (t.partial) return kWholePartial;
  if (t.upsampling > 1) return kWholeUpsampling;
  if (t.subsampled) return kWholeSubsampling;
  if (t.noise) return kWholeNoise;
  if (t.patches) return kWholePatches;
  if (t.splines) return kWholeSplines;
  if (t.dc_frame) return kWholeDcFrame;
  if (t.num_channels == 2 || t.num_channels == 4) return kWholeAlpha;
  if (t.single_section) return kWholeSingleSection;
  if (w.groups_in_frame == 1) return kWholeOneGroup;
  if (w.groups_taken == w.groups_in_frame) return kWholeWindowIsFrame;
  return kWindowed;
}

// ------------------------------------------------------------------------------------- the window as a frame
// What a window's descriptor owns: the arrays that are gathered or cropped. Everything per-frame is shared by pointer with
// the whole frame's descriptor.
struct WindowTables {
  std::vector<uint64_t> section_offset;
  std::vector<uint32_t> section_size, group_block_begin;
  std::vector<JxlHipVarBlock> blocks;
  std::vector<uint8_t> sharpness;
  std::vector<float> inv_sigma;
  std::vector<int8_t> ytox, ytob;
};
// Group `i` of the window, row-major, as a group of the frame.
inline uint32_t FrameGroupOf(const WindowPlan& w, uint32_t frame_xsize_groups, uint32_t i) {
  return (w.gy0 + i / w.gxs) * frame_xsize_groups + w.gx0 + i % w.gxs;
}
template <typename T>
inline void CropPlane(const T* src, uint32_t src_row, const Rect& r, std::vector<T>* dst) {
  dst->resize(size_t(r.xsize) * r.ysize);
  for (uint32_t y = 0; y < r.ysize; y++) memcpy(dst->data() + size_t(y) * r.xsize, src + size_t(r.y0 + y) * src_row + r.x0, size_t(r.xsize) * sizeof(T));
}
// Fills *out with the descriptor of window `w` of the frame `whole` describes (a frame for which WholeFrameReasonOf gave
// kWindowed), with the window's DC planes `dc_device` (jxlhip_dc_window); `t` holds its arrays and must outlive its use.
inline void BuildWindowDesc(const JxlHipFrameDesc& whole, const WindowPlan& w, const float* dc_device, WindowTables* t, JxlHipFrameDesc* out) {
  JxlHipFrameDesc d = whole;  // passes, dequant tables, block-context LUT, loop filter, colour, scalars: shared
  d.xsize = w.pixels.xsize;
  d.ysize = w.pixels.ysize;
  d.xsize_blocks = w.blocks.xsize;
  d.ysize_blocks = w.blocks.ysize;
  d.xsize_groups = w.gxs;
  d.num_groups = w.groups_taken;
  d.band_group_row_begin = d.band_group_row_end = 0;
  d.group_absent = nullptr;
  // sections: per pass, the chosen groups' in the window's row-major order
  t->section_offset.resize(size_t(d.num_passes) * d.num_groups);
  t->section_size.resize(t->section_offset.size());
  for (uint32_t p = 0; p < d.num_passes; p++)
    for (uint32_t i = 0; i < d.num_groups; i++) {
      const size_t from = size_t(p) * whole.num_groups + FrameGroupOf(w, whole.xsize_groups, i);
      t->section_offset[size_t(p) * d.num_groups + i] = whole.section_offset[from];
      t->section_size[size_t(p) * d.num_groups + i] = whole.section_size[from];
    }
  d.section_offset = t->section_offset.data();
  d.section_size = t->section_size.data();
  // varblocks: the chosen groups' in that order, positions relative to the window; coef_offset, qf, strategy and
  // quant_dc_ctx are the group's own
  t->blocks.clear();
  t->group_block_begin.assign(1, 0);
  for (uint32_t i = 0; i < d.num_groups; i++) {
    const uint32_t grp = FrameGroupOf(w, whole.xsize_groups, i);
    for (uint32_t b = whole.group_block_begin[grp]; b < whole.group_block_begin[grp + 1]; b++) {
      JxlHipVarBlock v = whole.blocks[b];
      v.bx = uint16_t(v.bx - w.blocks.x0);
      v.by = uint16_t(v.by - w.blocks.y0);
      t->blocks.push_back(v);
    }
    t->group_block_begin.push_back(uint32_t(t->blocks.size()));
  }
  d.blocks = t->blocks.data();
  d.num_blocks = uint32_t(t->blocks.size());
  d.group_block_begin = t->group_block_begin.data();
  // block-resolution planes: the 8- and 64-pixel grids divide 256
  if (whole.sharpness) {
    CropPlane(whole.sharpness, whole.xsize_blocks, w.blocks, &t->sharpness);
    d.sharpness = t->sharpness.data();
  }
  if (whole.inv_sigma) {
    CropPlane(whole.inv_sigma, whole.xsize_blocks, w.blocks, &t->inv_sigma);
    d.inv_sigma = t->inv_sigma.data();
  }
  const uint32_t per_group = kGroupBlocks / kCflTileBlocks;
  const Rect tiles{w.gx0 * per_group, w.gy0 * per_group, (w.blocks.xsize + kCflTileBlocks - 1) / kCflTileBlocks,
                   (w.blocks.ysize + kCflTileBlocks - 1) / kCflTileBlocks};
  const uint32_t tile_row = (whole.xsize_blocks + kCflTileBlocks - 1) / kCflTileBlocks;
  CropPlane(whole.ytox, tile_row, tiles, &t->ytox);
  CropPlane(whole.ytob, tile_row, tiles, &t->ytob);
  d.ytox = t->ytox.data();
  d.ytob = t->ytob.data();
  // the DC image: the planes k_dc_window made, used where they are
  d.dc = nullptr;
  d.dc_quantised = nullptr;
  d.dc_extra_precision = nullptr;
  d.dc_smoothing = 0;
  d.dc_device = dc_device;
  *out = d;
}

// ---------------------------------------------------------------------------------------------- the DC apron
// The window in blocks, grown by one block on each side and clipped to the frame: what the smoothing of the window reads.
inline Rect PlanDcApron(const Rect& window_blocks, uint32_t frame_xsize_blocks, uint32_t frame_ysize_blocks) {
  const uint32_t x0 = window_blocks.x0 ? window_blocks.x0 - 1 : 0, y0 = window_blocks.y0 ? window_blocks.y0 - 1 : 0;
  const uint64_t x1 = uint64_t(window_blocks.x0) + window_blocks.xsize + 1, y1 = uint64_t(window_blocks.y0) + window_blocks.ysize + 1;
  return Rect{x0, y0, uint32_t(x1 < frame_xsize_blocks ? x1 : frame_xsize_blocks) - x0, uint32_t(y1 < frame_ysize_blocks ? y1 : frame_ysize_blocks) - y0};
}
// The three integer planes of `apron` out of the frame's ([3][frame_ys][frame_xs], FramePlan::dc_q) into `dst`
// (3 * apron.xsize * apron.ysize integers).
inline void PackDcApron(const int32_t* frame_q, uint32_t frame_xs, uint32_t frame_ys, const Rect& apron, int32_t* dst) {
  const size_t plane = size_t(frame_xs) * frame_ys, out_plane = size_t(apron.xsize) * apron.ysize;
  for (int c = 0; c < 3; c++)
    for (uint32_t y = 0; y < apron.ysize; y++)
      memcpy(dst + c * out_plane + size_t(y) * apron.xsize, frame_q + c * plane + size_t(apron.y0 + y) * frame_xs + apron.x0, size_t(apron.xsize) * 4);
}

// Every reason to refuse a JxlHipDcWindow, each stated once in CheckDcWindow. tests/c/window_kats.cc breaks each rule in turn
// and fails when a rule here has no row there.
enum DcWindowRule : int {
  kDcWindowRuleWindow,     // a non-empty window inside a frame of at most 2^27 blocks a side
  kDcWindowRuleApron,      // the apron is the window grown by one block and clipped to the frame (so: inside the frame)
  kDcWindowRulePlanes,     // apron != NULL
  kDcWindowRuleSteps,      // the three dc_step finite and > 0
  kDcWindowRuleSize,       // the apron's planes (and so the window's) at most 2^24 samples
  kDcWindowRulePrecision,  // a precision byte for every DC group the apron touches (NULL: a frame of one DC group)
  kDcWindowRuleCount
};
inline int CheckDcWindow(const JxlHipDcWindow& d, int* rule = nullptr) {
#define JXH_DCWIN_REFUSE(cond, r)           \
  do {                                      \
    if (cond) {                             \
      if (rule) *rule = (r);                \
      return JXLHIP_ERR_INVALID_ARGUMENT;   \
    }                                       \
  } while (0)
  const uint32_t kMaxExtentBlocks = 1u << 27;
  JXH_DCWIN_REFUSE(!d.win_xsize || !d.win_ysize || !d.frame_xsize_blocks || !d.frame_ysize_blocks || d.frame_xsize_blocks > kMaxExtentBlocks ||
                       d.frame_ysize_blocks > kMaxExtentBlocks,
                   kDcWindowRuleWindow);
  JXH_DCWIN_REFUSE(uint64_t(d.win_x0) + d.win_xsize > d.frame_xsize_blocks || uint64_t(d.win_y0) + d.win_ysize > d.frame_ysize_blocks,
                   kDcWindowRuleWindow);
  const Rect apron = PlanDcApron(Rect{d.win_x0, d.win_y0, d.win_xsize, d.win_ysize}, d.frame_xsize_blocks, d.frame_ysize_blocks);
  JXH_DCWIN_REFUSE(!(apron == Rect{d.apron_x0, d.apron_y0, d.apron_xsize, d.apron_ysize}), kDcWindowRuleApron);
  JXH_DCWIN_REFUSE(!d.apron, kDcWindowRulePlanes);
  for (int c = 0; c < 3; c++) JXH_DCWIN_REFUSE(!isfinite(d.dc_step[c]) || !(d.dc_step[c] > 0.0f), kDcWindowRuleSteps);
  JXH_DCWIN_REFUSE(uint64_t(apron.xsize) * apron.ysize > kMaxDcWindowSamples, kDcWindowRuleSize);
  const uint32_t xgroups = (d.frame_xsize_blocks + kDcGroupBlocks - 1) / kDcGroupBlocks;
  const uint64_t last_group = uint64_t((apron.y0 + apron.ysize - 1) / kDcGroupBlocks) * xgroups + (apron.x0 + apron.xsize - 1) / kDcGroupBlocks;
  const uint64_t frame_groups = uint64_t(xgroups) * ((d.frame_ysize_blocks + kDcGroupBlocks - 1) / kDcGroupBlocks);
  JXH_DCWIN_REFUSE(d.dc_extra_precision ? last_group >= d.num_dc_groups : frame_groups > 1, kDcWindowRulePrecision);
#undef JXH_DCWIN_REFUSE
  return 0;
}

// ---- tiles of k_dc_window: a workgroup of 256 threads takes kTileCols x kTileRows samples of the window, lanes along x
// (k_reduced_pixels' shape, jxh_reduced_plan.h).
constexpr uint32_t kTileCols = 64, kTileRows = 8;
inline uint32_t TilesX(uint32_t xsize_blocks) { return (xsize_blocks + kTileCols - 1) / kTileCols; }
inline uint32_t TilesY(uint32_t ysize_blocks) { return (ysize_blocks + kTileRows - 1) / kTileRows; }

}  // namespace window
}  // namespace jxlhip
#endif  // JXH_WINDOW_PLAN_H_
