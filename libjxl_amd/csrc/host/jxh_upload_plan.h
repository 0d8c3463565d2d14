// libjxl_amd — what jxlhip_frame_upload computes from a frame descriptor, apart from where it puts it: the checks that
// admit a JxlHipFrameDesc, the tables derived from it on the host, the pixel route, and the ONE list of the tables a
// frame's blob holds. Pure functions: no context, no device call, no getenv; plain C++17, so tests/c/upload_plan_kats.cc
// holds every one of them on the CPU. The HIP layer (csrc/hip/jxl_hip_api.hip) decides where the bytes go.
#ifndef JXH_UPLOAD_PLAN_H_
#define JXH_UPLOAD_PLAN_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../../include/jxl_amd_hip.h"
#include "../hip/jxl_hip_block_ctx.h"

namespace jxlhip {
namespace upload {

// The context state the checks and the routes read (jxlhip_set_option, jxlhip_set_output_*, jxlhip_set_alpha) and the two
// environment switches, which the HIP layer reads once.
struct UploadOptions {
  bool band_halo = false, keep_filtered = false, keep_upsampled = false;
  uint32_t out_type = 2, out_nc = 3, out_bits = 8, out_swap = 0;  // jxlhip_set_output_format (JxlDataType numbering)
  uint32_t out_orient = 0;
  bool have_alpha = false;
  size_t alpha_capacity = 0;     // bytes of the alpha plane that was set
  bool section_entropy = false;  // JXLHIP_ENTROPY=1: no frame takes the lane kernel
  bool no_lane_prefix = false;   // JXLHIP_NO_LANE_PREFIX
  // jxlhip_set_output_tensor: the pixels go to a caller's tensor (out_type / out_nc then describe it; out_type may be
  // JXLHIP_TENSOR_BF16). tensor_rows: its columns are adjacent elements (stride_x 1); tensor_reach: bytes from its first
  // element to behind the last one the frame's image reaches. The defaults mean "no tensor".
  bool tensor = false, tensor_rows = false;
  uint64_t tensor_reach = 0;
};
inline bool OutIsRgb8(uint32_t type, uint32_t nc, uint32_t bits) { return type == 2 && nc == 3 && bits == 8; }
inline bool OutIsGray8(uint32_t type, uint32_t nc, uint32_t bits) { return type == 2 && nc == 1 && bits == 8; }
inline bool OutIsRgbF32(uint32_t type, uint32_t nc, uint32_t swap) { return type == 0 && nc == 3 && !swap; }

// ------------------------------------------------------------------------------------------------------ geometry
// Of a descriptor whose sizes CheckFrameDesc has accepted (it divides by them).
struct Geometry {
  uint32_t cs = 0;  // chroma shifts: hshift of channel c in bit 2 * c, vshift in bit 2 * c + 1 (0 = 4:4:4)
  uint32_t ups = 1, oxs = 0, oys = 0;  // upsampling factor (1 = none) and the image's size
  uint32_t band_row0 = 0, band_row1 = 0;  // group rows whose pixels the context produces
  uint32_t ext_row0 = 0, ext_row1 = 0;    // group rows to entropy-decode and transform (the band and one row either side)
  uint32_t band_y0 = 0, band_y1 = 0, ext_y0 = 0, ext_y1 = 0;  // the same in pixel rows
  uint32_t nctx = 0;                                          // AC contexts of one histogram set
  size_t nsec = 0, nblk = 0, ntiles = 0;
};
inline uint32_t ChromaShifts(const JxlHipFrameDesc& d) {
  uint32_t cs = 0;
  for (int ch = 0; ch < 3; ch++) cs |= uint32_t(d.chroma_hshift[ch]) << (2 * ch) | uint32_t(d.chroma_vshift[ch]) << (2 * ch + 1);
  return cs;
}
inline Geometry MakeGeometry(const JxlHipFrameDesc& d, const UploadOptions& o) {
  Geometry g;
  g.cs = ChromaShifts(d);
  g.ups = d.upsampling > 1 ? d.upsampling : 1;
  g.oxs = g.ups == 1 ? d.xsize : d.out_xsize;
  g.oys = g.ups == 1 ? d.ysize : d.out_ysize;
  const uint32_t yg = d.num_groups / d.xsize_groups;
  g.band_row0 = d.band_group_row_begin;
  g.band_row1 = d.band_group_row_end;
  if (g.band_row0 == 0 && g.band_row1 == 0) g.band_row1 = yg;
  g.ext_row0 = (g.band_row0 && !o.band_halo) ? g.band_row0 - 1 : g.band_row0;
  g.ext_row1 = (g.band_row1 < yg && !o.band_halo) ? g.band_row1 + 1 : g.band_row1;
  g.band_y0 = g.band_row0 * 256;
  g.ext_y0 = g.ext_row0 * 256;
  g.ext_y1 = uint64_t(g.ext_row1) * 256 < d.ysize ? g.ext_row1 * 256 : d.ysize;
  g.band_y1 = uint64_t(g.band_row1) * 256 < d.ysize ? g.band_row1 * 256 : d.ysize;
  g.nctx = d.num_block_ctxs * 495;
  g.nsec = size_t(d.num_groups) * d.num_passes;
  g.nblk = size_t(d.xsize_blocks) * d.ysize_blocks;
  g.ntiles = size_t((d.xsize_blocks + 7) / 8) * ((d.ysize_blocks + 7) / 8);
  return g;
}
inline bool InBand(const JxlHipVarBlock& v, const Geometry& g) { return uint32_t(v.by >> 5) >= g.ext_row0 && uint32_t(v.by >> 5) < g.ext_row1; }

// The DC image and 1 / sigma: final as handed over, or finished on the device (jxl_hip_dc.h) behind the table copy.
struct DcRoute {
  bool dequant, smooth, sigma;
};
inline DcRoute DcRouteOf(const JxlHipFrameDesc& d) {
  DcRoute r;
  r.dequant = d.dc_quantised != nullptr && !d.dc_device;
  // (compressed_dc.cc:134: smaller images are left alone; a DC frame's planes are used where they are, never smoothed)
  r.smooth = d.dc_smoothing != 0 && d.xsize_blocks > 2 && d.ysize_blocks > 2 && !d.dc_device;
  r.sigma = !d.inv_sigma && d.epf_iters > 0;
  return r;
}

// --------------------------------------------------------------------------------------------------------- checks
// Every reason to refuse a descriptor, each stated once below. tests/c/upload_plan_kats.cc breaks each rule in turn and
// fails when a rule here has no row in its table.
enum Rule : int {
  kRuleSizes,                  // no pixels, groups or passes; more than 11 passes
  kRuleCoefBits,               // 16 or 32
  kRuleChromaShift,            // shifts are 0 or 1
  kRuleWholeMcus,              // the block counts of the frame's size
  kRuleSubsampledFrame,        // a subsampled frame is YCbCr, unsmoothed, without a DC frame
  kRuleSubsampledHaloBand,     // (unsupported) ... and not a band whose neighbours' rows arrive as halos
  kRuleGroupCounts,            // the group counts of the frame's size
  kRuleBlockCtxCounts,         // thresholds, block contexts, DC contexts
  kRuleUpsampling,             // factor, kernel, image size, no band
  kRuleBandRows,               // a non-empty range of the frame's group rows
  kRuleAbsentGroupSections,    // an absent group has no sections
  kRulePartialPassOrder,       // once a pass of a group is missing, all later ones are
  kRuleGroupBlockRanges,       // the groups' block ranges tile [0, num_blocks)
  kRuleVarblockFields,         // strategy, quant field, DC context
  kRuleVarblockInsideGroup,    // inside its group and the frame
  kRuleVarblockCoefOffset,     // coefficients packed in decode order, at most 65536 per channel and group
  kRuleSubsampledOneBlock,     // a subsampled frame's varblocks cover one block
  kRuleSubsampledRaster,       // ... and are the group's blocks in raster order
  kRulePassLimits,             // clusters 1..256, log_alpha 5..8 for rANS
  kRulePrefixTables,           // every index a prefix lookup can form is inside the table
  kRuleLz77,                   // distance context, minimum length
  kRuleCtxMapSize,             // one entry per histogram set and context (+ 16)
  kRuleCtxMapEntries,          // every entry names a cluster
  kRuleUintConfig,             // hybrid-uint configs within their token width
  kRuleDcSource,               // some form of the DC image
  kRuleSharpness,              // 1 / sigma on the device needs the sharpness bytes
  kRuleDcStep,                 // DC steps positive where the device dequantises or smooths
  kRuleQuantScale,             // positive where the device computes 1 / sigma
  kRuleLinearOutput,           // 0..3
  kRuleColorTarget,            // transfer function and tone mapping known
  kRuleColorTargetLinear,      // a colour target takes linear RGB
  kRuleSplineTables,           // pointers and counts
  kRuleSplineRows,             // row lists consistent, every entry a segment
  kRulePatchTables,            // pointers and counts
  kRulePatchRows,              // row lists consistent, every entry one of its patch's rows
  kRulePatchRecords,           // rectangles inside the frame and their reference frame, modes known
  kRulePatchAlphaUpsampled,    // (unsupported) alpha patches on an upsampled frame
  kRuleAlphaCapacity,          // the alpha plane that was set covers the image
  kRuleBlockCtxLutSize,        // [channel][order bucket][qf bucket][DC bucket]
  kRuleDequantExtents,         // the tables of the strategies in use have their size and lie inside `dequant`
  kRuleOrdersInBucket,         // (CheckOrders) the orders of the strategies in use are permutations inside their bucket
  kNumRules
};

#define JXH_REFUSE(cond, which, code) \
  do {                                \
    if (cond) {                       \
      if (rule) *rule = which;        \
      return code;                    \
    }                                 \
  } while (0)
#define JXH_INVALID(cond, which) JXH_REFUSE(cond, which, JXLHIP_ERR_INVALID_ARGUMENT)

// Every index PrefixLookup (jxl_hip_kernels.h) can form from a cluster's two-level tables stays inside `table`, and
// every code length it can return is at most 15 bits.
inline bool ValidPrefixTables(uint32_t offset_word, const uint32_t* table, size_t table_size) {
  const size_t first = offset_word & 0xFFFFFFu, root_bits = offset_word >> 24;
  if (root_bits > 15 || first + (size_t(1) << root_bits) > table_size) return false;
  for (size_t r = 0; r < (size_t(1) << root_bits); r++) {
    const uint32_t e = table[first + r];
    if (!(e & 0x80u)) {
      if ((e & 0xFFu) > 15) return false;
      continue;
    }
    const size_t sub_bits = e & 0x7Fu, sub = first + (e >> 8);
    if (sub_bits == 0 || root_bits + sub_bits > 15 || sub + (size_t(1) << sub_bits) > table_size) return false;
    for (size_t j = 0; j < (size_t(1) << sub_bits); j++)
      if ((table[sub + j] & 0x80u) || (table[sub + j] & 0xFFu) > 15) return false;
  }
  return true;
}

// The draw cache of a frame's splines: every index a kernel forms from it is in range.
inline int CheckSplines(const JxlHipSplines& sp, uint32_t ysize, Rule* rule = nullptr) {
  if (!sp.num_segments) return 0;
  JXH_INVALID(!sp.segments || !sp.row_start || !sp.row_segments || sp.num_segments > (1u << 26) || sp.num_row_segments > (1u << 30), kRuleSplineTables);
  JXH_INVALID(sp.row_start[0] != 0 || sp.row_start[ysize] != sp.num_row_segments, kRuleSplineRows);
  for (uint32_t y = 0; y < ysize; y++) JXH_INVALID(sp.row_start[y] > sp.row_start[y + 1], kRuleSplineRows);
  for (uint32_t i = 0; i < sp.num_row_segments; i++) JXH_INVALID(sp.row_segments[i] >= sp.num_segments, kRuleSplineRows);
  return 0;
}

// The patch dictionary of a frame, validated like every table a kernel indexes with (rectangles inside the frame and
// inside their reference frame, row lists consistent). ysize rows; positions may reach xlimit x ylimit.
inline int CheckPatches(const JxlHipPatches& pt, uint32_t ysize, uint32_t xlimit, uint32_t ylimit, Rule* rule = nullptr) {
  if (!pt.num_positions) return 0;
  JXH_INVALID(!pt.records || !pt.row_start || !pt.row_list || pt.num_positions > (1u << 24) || pt.num_row_entries > (1u << 26), kRulePatchTables);
  JXH_INVALID(pt.row_start[0] != 0 || pt.row_start[ysize] != pt.num_row_entries, kRulePatchRows);
  for (uint32_t y = 0; y < ysize; y++) JXH_INVALID(pt.row_start[y] > pt.row_start[y + 1], kRulePatchRows);
  for (uint32_t i = 0; i < pt.num_positions; i++) {
    const uint32_t* q = pt.records + size_t(i) * 8;
    const uint32_t slot = q[6];
    JXH_INVALID(slot > 3 || !pt.slot_planes[slot] || (q[7] & 255) > 7 || ((q[7] >> 16) & 255) > 7 || !q[2] || !q[3], kRulePatchRecords);
    JXH_INVALID(pt.uses_alpha && !pt.slot_alpha[slot], kRulePatchRecords);  // (the reference frame kept no alpha plane)
    JXH_INVALID(uint64_t(q[4]) + q[2] > pt.slot_w[slot] || uint64_t(q[5]) + q[3] > pt.slot_h[slot], kRulePatchRecords);
    JXH_INVALID(uint64_t(q[0]) + q[2] > xlimit || uint64_t(q[1]) + q[3] > ylimit, kRulePatchRecords);
  }
  for (uint32_t y = 0; y < ysize; y++)
    for (uint32_t i = pt.row_start[y]; i < pt.row_start[y + 1]; i++) {
      JXH_INVALID(pt.row_list[i] >= pt.num_positions, kRulePatchRows);
      const uint32_t* q = pt.records + size_t(pt.row_list[i]) * 8;
      JXH_INVALID(y < q[1] || y >= q[1] + q[3], kRulePatchRows);  // (the row is one of the patch's rows)
    }
  return 0;
}

// Whether jxlhip_frame_upload takes the descriptor: 0, or the code it returns (`rule`: which rule refused). The kernels
// index with these tables unchecked, so every table index they can form is checked here.
inline int CheckFrameDesc(const JxlHipFrameDesc& d, const UploadOptions& o, Rule* rule = nullptr) {
  JXH_INVALID(!d.xsize || !d.ysize || !d.num_groups || !d.num_passes || d.num_passes > 11, kRuleSizes);
  JXH_INVALID(d.coef_bits != 16 && d.coef_bits != 32, kRuleCoefBits);
  uint32_t cs_maxh = 0, cs_maxv = 0;
  for (int ch = 0; ch < 3; ch++) {
    JXH_INVALID(d.chroma_hshift[ch] > 1 || d.chroma_vshift[ch] > 1, kRuleChromaShift);
    cs_maxh |= d.chroma_hshift[ch];
    cs_maxv |= d.chroma_vshift[ch];
  }
  const uint32_t cs = ChromaShifts(d);
  // (frame_dimensions.h:43-44: whole MCUs of a chroma-subsampled frame)
  JXH_INVALID(d.xsize_blocks != ((d.xsize + (8u << cs_maxh) - 1) / (8u << cs_maxh)) << cs_maxh ||
                  d.ysize_blocks != ((d.ysize + (8u << cs_maxv) - 1) / (8u << cs_maxv)) << cs_maxv,
              kRuleWholeMcus);
  if (cs) {
    // no adaptive DC smoothing (dec_frame.cc:206-212), no DC frame behind it, every varblock one block (checked below);
    // a band whose neighbours' rows arrive as halos cannot upsample its edge rows: the other band form works
    JXH_INVALID(d.dc_smoothing || d.dc_device || d.linear_output != 2, kRuleSubsampledFrame);
    JXH_REFUSE(o.band_halo && (d.band_group_row_begin | d.band_group_row_end), kRuleSubsampledHaloBand, JXLHIP_ERR_UNSUPPORTED);
  }
  JXH_INVALID(d.num_groups != d.xsize_groups * ((d.ysize + 255) / 256) || d.xsize_groups != (d.xsize + 255) / 256, kRuleGroupCounts);
  JXH_INVALID(d.num_qf_thresholds > 15 || d.num_block_ctxs == 0 || d.num_block_ctxs > 16 || d.num_dc_ctxs == 0, kRuleBlockCtxCounts);
  const Geometry g = MakeGeometry(d, o);
  if (g.ups != 1) {
    JXH_INVALID((g.ups != 2 && g.ups != 4 && g.ups != 8) || !d.upsampling_kernel || (d.band_group_row_begin | d.band_group_row_end) ||
                    (g.oxs + g.ups - 1) / g.ups != d.xsize || (g.oys + g.ups - 1) / g.ups != d.ysize,
                kRuleUpsampling);
  }
  JXH_INVALID(g.band_row0 >= g.band_row1 || g.band_row1 > d.num_groups / d.xsize_groups, kRuleBandRows);
  for (uint32_t grp = g.ext_row0 * d.xsize_groups; d.group_absent && grp < g.ext_row1 * d.xsize_groups; grp++) {
    if (d.group_absent[grp]) {
      for (uint32_t p = 0; p < d.num_passes; p++) JXH_INVALID(d.section_size[size_t(p) * d.num_groups + grp], kRuleAbsentGroupSections);
      continue;
    }
    // a partial frame's group is drawn from its leading passes (dec_frame.cc:620-680): the missing ones have size 0,
    // and once one is missing all later ones are
    bool missing = false;
    for (uint32_t p = 1; p < d.num_passes; p++) {
      const bool empty = d.section_size[size_t(p) * d.num_groups + grp] == 0;
      JXH_INVALID(missing && !empty, kRulePartialPassOrder);
      missing = missing || empty;
    }
  }
  // ---- varblocks against the geometry (the kernels index with these)
  uint32_t used = 0;  // strategies of the varblocks the context transforms
  {
    uint32_t prev_end = 0;
    for (uint32_t grp = 0; grp < d.num_groups; grp++) {
      const uint32_t b0 = d.group_block_begin[grp], b1 = d.group_block_begin[grp + 1];
      JXH_INVALID(b0 != prev_end || b1 < b0 || b1 > d.num_blocks, kRuleGroupBlockRanges);
      prev_end = b1;
      uint32_t off = 0;
      const uint32_t gx0 = (grp % d.xsize_groups) * 32, gy0 = (grp / d.xsize_groups) * 32;
      for (uint32_t i = b0; i < b1; i++) {
        const JxlHipVarBlock& v = d.blocks[i];
        JXH_INVALID(v.strategy >= 27 || v.qf == 0 || v.qf > 256 || v.quant_dc_ctx >= d.num_dc_ctxs, kRuleVarblockFields);
        const uint32_t cx = kCoveredX[v.strategy], cy = kCoveredY[v.strategy];
        JXH_INVALID(v.bx < gx0 || v.by < gy0 || v.bx + cx > gx0 + 32 || v.by + cy > gy0 + 32 || v.bx + cx > d.xsize_blocks || v.by + cy > d.ysize_blocks,
                    kRuleVarblockInsideGroup);
        JXH_INVALID(v.coef_offset != off, kRuleVarblockCoefOffset);
        JXH_INVALID(cs && cx * cy != 1, kRuleSubsampledOneBlock);  // (dec_modular.cc:534-538)
        // (so a subsampled group's varblocks are its blocks in raster order: the entropy stage finds the block at a
        // channel's own column, whose quant field its block context takes, that many entries back in the row)
        if (cs) {
          const uint32_t gw = std::min<uint32_t>(32, d.xsize_blocks - gx0);
          JXH_INVALID(v.bx != gx0 + (i - b0) % gw || v.by != gy0 + (i - b0) / gw, kRuleSubsampledRaster);
        }
        off += 64u * cx * cy;
        JXH_INVALID(off > 65536, kRuleVarblockCoefOffset);
        if (InBand(v, g)) used |= 1u << v.strategy;
      }
    }
    JXH_INVALID(prev_end != d.num_blocks, kRuleGroupBlockRanges);
  }
  // ---- per-pass tables: every table index the kernel can form must be inside the table
  for (uint32_t p = 0; p < d.num_passes; p++) {
    const JxlHipPassDesc& s = d.passes[p];
    JXH_INVALID(s.num_clusters == 0 || s.num_clusters > 256 || (!s.use_prefix && (s.log_alpha < 5 || s.log_alpha > 8)), kRulePassLimits);
    if (s.use_prefix) {
      JXH_INVALID(!s.prefix_offset || !s.prefix_table, kRulePrefixTables);
      for (uint32_t i = 0; i < s.num_clusters; i++)
        JXH_INVALID(!ValidPrefixTables(s.prefix_offset[i], s.prefix_table, s.prefix_table_size), kRulePrefixTables);
    }
    JXH_INVALID(s.lz77 && (s.lz_dist_ctx >= s.num_clusters || s.lz_min_length == 0), kRuleLz77);
    JXH_INVALID(s.ctx_map_size < size_t(d.num_histograms) * g.nctx + 16, kRuleCtxMapSize);
    for (uint32_t i = 0; i < s.ctx_map_size; i++) JXH_INVALID(s.ctx_map[i] >= s.num_clusters, kRuleCtxMapEntries);
    for (uint32_t i = 0; i < s.num_clusters; i++) {  // hybrid-uint configs: split_exponent, msb_in_token, lsb_in_token
      const uint32_t se = s.uint_cfg[i] & 0xFF, msb = (s.uint_cfg[i] >> 8) & 0xFF, lsb = (s.uint_cfg[i] >> 16) & 0xFF;
      JXH_INVALID(se > (s.use_prefix ? 15u : s.log_alpha) || msb > se || lsb > se - msb, kRuleUintConfig);
    }
  }
  // ---- the DC image and 1 / sigma
  const DcRoute dc = DcRouteOf(d);
  JXH_INVALID(!d.dc && !d.dc_device && !d.dc_quantised, kRuleDcSource);
  JXH_INVALID(dc.sigma && !d.sharpness, kRuleSharpness);
  if (dc.dequant || dc.smooth)
    for (int ch = 0; ch < 3; ch++) JXH_INVALID(!(d.dc_step[ch] > 0.0f), kRuleDcStep);
  JXH_INVALID(dc.sigma && !(d.quant_scale > 0.0f), kRuleQuantScale);
  // ---- colour: frames of images that are not XYB encoded (linear_output 2 = YCbCr, 3 = no colour transform) take
  // XybToRgb's other branches; an output encoding other than (linear) sRGB (jxl_hip_color.h) starts from linear RGB
  JXH_INVALID(d.linear_output < 0 || d.linear_output > 3, kRuleLinearOutput);
  if (d.color_target) {
    JXH_INVALID(d.color_target->tf > JXLHIP_TF_GAMMA || d.color_target->tone > JXLHIP_TONE_HLG_OOTF, kRuleColorTarget);
    JXH_INVALID(d.color_target->tf && d.linear_output != 1, kRuleColorTargetLinear);
  }
  // ---- splines and patches (an upsampled frame's are drawn at its own resolution: dec_cache.cc:193-212)
  int r;
  if ((r = CheckSplines(d.splines, d.ysize, rule))) return r;
  if ((r = CheckPatches(d.patches, d.ysize, d.xsize_blocks * 8, d.ysize_blocks * 8, rule))) return r;
  JXH_REFUSE(d.patches.num_positions && d.patches.uses_alpha && g.ups != 1, kRulePatchAlphaUpsampled, JXLHIP_ERR_UNSUPPORTED);
  JXH_INVALID(o.have_alpha && o.alpha_capacity < size_t(g.oxs) * g.oys * 4, kRuleAlphaCapacity);
  // ---- block contexts and dequantisation tables
  JXH_INVALID(size_t(d.block_ctx_lut_size) < size_t(3) * 13 * (d.num_qf_thresholds + 1) * d.num_dc_ctxs, kRuleBlockCtxLutSize);
  for (int s = 0; s < 27; s++) {
    if (!(used >> s & 1)) continue;
    const uint32_t k = kStrategyQuantTable[s];
    JXH_INVALID(d.dequant_size[k] != 64u * CoveredBlocks(s) || size_t(d.dequant_offset[k]) + 3 * size_t(d.dequant_size[k]) > d.dequant_floats,
                kRuleDequantExtents);
  }
  return 0;
}

// The coefficient orders of passes [0, num_passes) for the strategies in use (list_count): inside `orders` and a
// permutation's entries inside their bucket. k_merge_passes and the scan-order dequant tables index through them, so
// the lane routes ask for every pass they decode; the section-per-workgroup kernels bound their own reads.
inline int CheckOrders(const JxlHipFrameDesc& d, const uint32_t* list_count, uint32_t num_passes, Rule* rule = nullptr) {
  for (uint32_t p = 0; p < num_passes; p++)
    for (int st = 0; st < 27; st++) {
      if (!list_count[st]) continue;
      const uint32_t size = d.dequant_size[kStrategyQuantTable[st]];
      for (int ch = 0; ch < 3; ch++) {
        const uint32_t oo = d.passes[p].order_offset[kStrategyOrder[st] * 3 + ch];
        JXH_INVALID(size_t(oo) + size > d.passes[p].orders_size, kRuleOrdersInBucket);
        for (uint32_t k = 0; k < size; k++) JXH_INVALID(d.passes[p].orders[oo + k] >= size, kRuleOrdersInBucket);
      }
    }
  return 0;
}
#undef JXH_INVALID
#undef JXH_REFUSE

// ----------------------------------------------------------------------------------------------------- pixel route
// Where the pixels come from: RGB8 from every filter kernel, RGB f32 and one 8-bit sRGB channel from the row-streaming
// one; any other format, orientation, colour transform, noise, splines, patches or kept planes from the generic writer
// (k_color_out on the filtered planes, or k_upsample_color).
struct PixelRoute {
  bool color_out;   // the pixels come from the generic writer
  bool gray8_fast;  // one 8-bit sRGB channel from k_filter_rows2's one-channel form (the filtered planes are not kept beside it)
  bool ups_kept;    // (tests) the upsampled planes are kept: the route of a noisy upsampled frame without the noise
  bool plane1;      // the second plane set is needed
  bool tensor_fused = false;  // a caller's planar float tensor from k_filter_rows2's tensor form
};
inline PixelRoute PixelRouteOf(const JxlHipFrameDesc& d, const UploadOptions& o) {
  const uint32_t ups = d.upsampling > 1 ? d.upsampling : 1;
  // (a tensor is never the context's own RGB8 / one-channel rows, whatever its type)
  const bool rgb8 = !o.tensor && OutIsRgb8(o.out_type, o.out_nc, o.out_bits), g8 = !o.tensor && OutIsGray8(o.out_type, o.out_nc, o.out_bits);
  const bool rows_kernel = ups == 1 && (d.epf_iters == 1 || d.epf_iters == 2);
#ifdef JXLHIP_NO_GRAY8_ROWS  // (scripts/measure_grey_xyb.py: the comparison build, one 8-bit channel from the generic writer)
  const bool gray8 = false;
#else
  const bool gray8 = g8 && rows_kernel && d.linear_output == 0 && !o.keep_filtered;
#endif
  // The frame would get RGB f32 from the row-streaming kernel, and the tensor is three planes of a float type whose rows
  // the kernel's 32-bit offsets reach (that form writes nothing else: kept filtered planes go through the generic writer).
  const bool float_type = o.out_type == JXLHIP_TENSOR_F32 || o.out_type == JXLHIP_TENSOR_F16 || o.out_type == JXLHIP_TENSOR_BF16;
  const bool tensor_rows = o.tensor && float_type && o.out_nc == 3 && o.tensor_rows && o.tensor_reach < (uint64_t(1) << 31) &&
                           rows_kernel && !o.keep_filtered;
  const bool rgbf32 = !o.tensor && OutIsRgbF32(o.out_type, o.out_nc, o.out_swap) && rows_kernel;
  PixelRoute r;
  r.ups_kept = o.keep_upsampled && ups != 1;
  r.color_out = (!rgb8 && !gray8 && !rgbf32 && !tensor_rows) ||
                o.out_orient ||                               // the oriented layout
                d.linear_output >= 2 ||                       // XybToRgb's other branches
                (d.color_target && d.color_target->tf) ||     // the frame's matrix gives linear RGB, the generic writer the rest
                d.has_noise ||                                // added between the filter launch and the colour conversion
                r.ups_kept || d.splines.num_segments || d.patches.num_positions;  // drawn over the filtered planes
  r.gray8_fast = g8 && !r.color_out;
  r.tensor_fused = tensor_rows && !r.color_out;
  r.plane1 = o.keep_filtered || ups != 1 || r.color_out;
  return r;
}

// -------------------------------------------------------------------------------------------------------- builders
// Each writes into memory the caller gives it (the staging block), sized by the function beside it.

// AC sections at 16-byte aligned offsets (the lane kernel's LDS-DMA), 4 spare bytes behind each, and a 256-byte tail: the
// lane kernel prefetches up to 64 bytes past a section.
inline size_t SectionStride(uint32_t size) { return (size_t(size) + 15 + 4) & ~size_t(15); }
constexpr size_t kSectionTail = 256;
inline size_t PackedSectionBytes(const JxlHipFrameDesc& d) {
  size_t total = 0;
  for (size_t i = 0, n = size_t(d.num_groups) * d.num_passes; i < n; i++) total += SectionStride(d.section_size[i]);
  return total + kSectionTail;
}
inline void BuildSectionWords(const JxlHipFrameDesc& d, uint32_t* sec_word) {  // first 32-bit word of every section
  size_t total = 0;
  for (size_t i = 0, n = size_t(d.num_groups) * d.num_passes; i < n; i++) {
    sec_word[i] = uint32_t(total / 4);
    total += SectionStride(d.section_size[i]);
  }
}
inline void PackSections(const JxlHipFrameDesc& d, const uint32_t* sec_word, uint8_t* packed, size_t bytes) {
  size_t end = 0;
  for (size_t i = 0, n = size_t(d.num_groups) * d.num_passes; i < n; i++) {
    const size_t at = size_t(sec_word[i]) * 4;
    memset(packed + end, 0, at - end);
    memcpy(packed + at, d.codestream + d.section_offset[i], d.section_size[i]);
    end = at + d.section_size[i];
  }
  memset(packed + end, 0, bytes - end);
}
// Histogram selector of every section [pass * num_groups + group]: its first SelectorBits bits (dec_group.cc:594-610).
inline void BuildSelectors(const JxlHipFrameDesc& d, uint32_t* sel) {
  const uint32_t hb = SelectorBits(d.num_histograms);
  for (size_t i = 0, n = size_t(d.num_groups) * d.num_passes; i < n; i++) {
    const uint8_t* p = d.codestream + d.section_offset[i];
    const uint32_t bit0 = i == 0 ? d.first_section_bit_offset : 0;
    uint64_t v = 0;
    for (uint32_t b = 0; hb && b < 8 && b < d.section_size[i]; b++) v |= uint64_t(p[b]) << (8 * b);
    sel[i] = uint32_t((v >> bit0) & ((1u << hb) - 1));
  }
}

// A pass's alias tables in the lane kernel's form (none for a prefix-coded pass).
//   alias entry {cutoff u8, right u8, freq0 u16 | offsets1 u16, freq1 u16} ->
//   x = (freq0 - 1) & 0xFFF | uint config << 12 | cutoff << 24   taken when pos <  cutoff: symbol = slot, offset = pos
//   y = (freq1 - 1) & 0xFFF | offsets1 << 12 | right << 24        taken when pos >= cutoff
// (uint config of the entry's cluster: split_exponent | msb_in_token << 4 | lsb_in_token << 8)
inline size_t AliasBytes(const JxlHipPassDesc& s) { return s.use_prefix ? 0 : (size_t(s.num_clusters) << s.log_alpha) * 8; }
inline void PackAlias(const JxlHipPassDesc& s, uint32_t* dst) {
  const uint32_t* src = static_cast<const uint32_t*>(s.alias);
  for (size_t i = 0, n = AliasBytes(s) / 8; i < n; i++) {
    const uint32_t ex = src[2 * i], ey = src[2 * i + 1];
    const uint32_t cutoff = ex & 0xFF, right = (ex >> 8) & 0xFF, freq0 = ex >> 16, offs1 = ey & 0xFFFF, freq1 = ey >> 16;
    const uint32_t uc = s.uint_cfg[i >> s.log_alpha];
    const uint32_t cfg12 = (uc & 15u) | (((uc >> 8) & 15u) << 4) | (((uc >> 16) & 15u) << 8);
    dst[2 * i] = ((freq0 - 1) & 0xFFFu) | (cfg12 << 12) | (cutoff << 24);
    dst[2 * i + 1] = ((freq1 - 1) & 0xFFFu) | ((offs1 & 0xFFFu) << 12) | (right << 24);
  }
}

// Transform work lists: the indices of the varblocks the context transforms, bucketed by strategy (tlist), and in the same
// order everything k_idct_fast needs to know of a varblock in ONE 16-byte load (trecs: the kernel's waves live for a
// handful of dependent memory round trips, and list entry -> block -> coefficients was three of them):
// {bx | by << 16, raw quant field, element offset of its coefficients (group * 3 * 65536 + offset in the group's planes),
// index of the varblock (for its coefficient counts)}. Entries behind the last list are zero.
inline size_t WorkListEntries(const JxlHipFrameDesc& d) { return d.num_blocks ? d.num_blocks : 1; }
inline void CountWorkLists(const JxlHipFrameDesc& d, const Geometry& g, uint32_t* list_begin, uint32_t* list_count) {
  for (int s = 0; s < 27; s++) list_count[s] = 0;
  for (uint32_t i = 0; i < d.num_blocks; i++)
    if (InBand(d.blocks[i], g)) list_count[d.blocks[i].strategy]++;
  uint32_t acc = 0;
  for (int s = 0; s < 27; s++) {
    list_begin[s] = acc;
    acc += list_count[s];
  }
}
inline void BuildWorkList(const JxlHipFrameDesc& d, const Geometry& g, const uint32_t* list_begin, uint32_t* tlist) {
  uint32_t fill[27] = {};
  for (uint32_t i = 0; i < d.num_blocks; i++) {
    if (!InBand(d.blocks[i], g)) continue;
    const int s = d.blocks[i].strategy;
    tlist[list_begin[s] + fill[s]++] = i;
  }
  uint32_t acc = 0;
  for (int s = 0; s < 27; s++) acc += fill[s];
  for (size_t j = acc, n = WorkListEntries(d); j < n; j++) tlist[j] = 0;
}
inline void BuildWorkRecords(const JxlHipFrameDesc& d, const uint32_t* tlist, uint32_t listed, uint32_t* trecs) {
  for (size_t j = 0, n = WorkListEntries(d); j < n; j++) {
    uint32_t* rec = trecs + 4 * j;
    if (j >= listed) {
      rec[0] = rec[1] = rec[2] = rec[3] = 0;
      continue;
    }
    const uint32_t i = tlist[j];
    const JxlHipVarBlock& v = d.blocks[i];
    const uint32_t grp = uint32_t(v.by >> 5) * d.xsize_groups + (v.bx >> 5);
    rec[0] = uint32_t(v.bx) | uint32_t(v.by) << 16;
    rec[1] = v.qf;
    rec[2] = grp * (3u * 65536u) + v.coef_offset;
    rec[3] = i;
  }
}

// Per varblock, everything the lane kernel's block transition needs in one word, so that it does no dependent table
// lookups: column in the group (5 bits) | not in the group's first row (1) | log2 covered_x (3) | log2 covered_y (3) |
// block context of X, Y, B (4 bits each: ac_context.h:101-143 BlockCtxMap::Context, from the strategy's order bucket, the
// quant-field bucket and the DC bucket; the codestream allows at most 16) | chroma-subsampled frames: bit 24 + channel =
// the block is off the channel's grid and carries nothing for it, bit 27 + channel = the channel's columns are half the
// frame's. 16 zero entries of padding (the kernel reads records in aligned groups of four).
inline size_t BlockRecEntries(const JxlHipFrameDesc& d) { return size_t(d.num_blocks) + 16; }
inline void BuildBlockRecs(const JxlHipFrameDesc& d, uint32_t* recs) {
  const uint32_t cs = ChromaShifts(d), nq = d.num_qf_thresholds + 1, ndc = d.num_dc_ctxs;
  for (uint32_t i = 0; i < d.num_blocks; i++) {
    const JxlHipVarBlock& v = d.blocks[i];
    const uint32_t qfi = QfBucket(v.qf, d.qf_thresholds, nq);
    const uint32_t fbx = v.bx & 31u, fby = v.by & 31u;
    uint32_t rec = fbx | (fby ? 32u : 0u) | Log2CoveredX(v.strategy) << 6 | Log2CoveredY(v.strategy) << 9;
    for (uint32_t ch = 0; ch < 3; ch++) {
      const uint32_t hs = ChannelHShift(cs, ch);
      uint32_t lbx, lby;
      const bool carried = ChannelCell(cs, ch, fbx, fby, lbx, lby);
      // (the quant field at the channel's own column: a subsampled group's varblocks are its blocks in raster order)
      const uint32_t qfc = hs ? QfBucket(d.blocks[i - QfColumnBack(fbx, lbx)].qf, d.qf_thresholds, nq) : qfi;
      const uint32_t bctx = d.block_ctx_lut[BctxLutIndex(ch, kStrategyOrder[v.strategy], nq, qfc, ndc, v.quant_dc_ctx)];
      rec |= (bctx & 15u) << (12 + 4 * ch);
      if (!carried) rec |= 1u << (24 + ch);
      rec |= hs << (27 + ch);
    }
    recs[i] = rec;
  }
  for (size_t i = d.num_blocks, n = BlockRecEntries(d); i < n; i++) recs[i] = 0;
}

// The dequantisation tables in the scan order of pass 0 for the kinds in use, zero elsewhere (single-pass lane frames:
// the transforms read coefficients in scan order). d.dequant_floats entries; CheckOrders has held the orders.
inline void BuildDequantScan(const JxlHipFrameDesc& d, const uint32_t* list_count, float* scan) {
  for (uint32_t i = 0; i < d.dequant_floats; i++) scan[i] = 0.0f;
  for (int st = 0; st < 27; st++) {
    if (!list_count[st]) continue;
    const uint32_t kind = kStrategyQuantTable[st], size = d.dequant_size[kind];
    for (int ch = 0; ch < 3; ch++) {
      const uint16_t* order = d.passes[0].orders + d.passes[0].order_offset[kStrategyOrder[st] * 3 + ch];
      const float* m = d.dequant + d.dequant_offset[kind] + size_t(ch) * size;
      float* o = scan + d.dequant_offset[kind] + size_t(ch) * size;
      for (uint32_t k = 0; k < size; k++) o[k] = m[order[k]];
    }
  }
}

// Gaborish weights per channel {w1, w2} folded with their normalisation: {mul, w1 * mul, w2 * mul}.
inline void FoldGaborish(const float* gab_w, float* folded) {
  for (int ch = 0; ch < 3; ch++) {
    const float w1 = gab_w[ch * 2], w2 = gab_w[ch * 2 + 1];
    const float mul = 1.0f / (1.0f + 4 * (w1 + w2));
    folded[ch * 3] = mul;
    folded[ch * 3 + 1] = w1 * mul;
    folded[ch * 3 + 2] = w2 * mul;
  }
}

// The groups the context decodes (the lane kernel takes a list of the sections that have arrived), and for a partial
// frame what has not arrived: groups drawn from the DC image alone (absent_blocks: first block and block count of each),
// and the missing passes of present groups as {pass, first block, block count}.
inline void BuildGroupLists(const JxlHipFrameDesc& d, const Geometry& g, std::vector<uint32_t>* group_list, std::vector<uint32_t>* absent_groups,
                            std::vector<uint32_t>* absent_blocks, std::vector<uint32_t>* absent_sections) {
  group_list->clear();
  absent_groups->clear();
  absent_blocks->clear();
  absent_sections->clear();
  for (uint32_t grp = g.ext_row0 * d.xsize_groups; grp < g.ext_row1 * d.xsize_groups; grp++) {
    const uint32_t b0 = d.group_block_begin[grp], nb = d.group_block_begin[grp + 1] - b0;
    if (d.group_absent && d.group_absent[grp]) {
      absent_groups->push_back(grp);
      absent_blocks->push_back(b0);
      absent_blocks->push_back(nb);
      continue;
    }
    group_list->push_back(grp);
    for (uint32_t p = 1; d.group_absent && p < d.num_passes; p++)
      if (d.section_size[size_t(p) * d.num_groups + grp] == 0) {
        absent_sections->push_back(p);
        absent_sections->push_back(b0);
        absent_sections->push_back(nb);
      }
  }
}

// ------------------------------------------------------------------------------------------------ the table list
// Everything about an accepted descriptor that decides which tables exist and what they hold.
struct Plan {
  Geometry g;
  DcRoute dc;
  PixelRoute px;
  uint32_t list_begin[27], list_count[27], listed;  // transform work lists (listed = their sum)
  size_t section_bytes;
  bool scan_order = false;  // the entropy route (set by the caller): a single-pass lane frame needs dequant_scan
};
inline Plan MakePlan(const JxlHipFrameDesc& d, const UploadOptions& o) {
  Plan p;
  p.g = MakeGeometry(d, o);
  p.dc = DcRouteOf(d);
  p.px = PixelRouteOf(d, o);
  CountWorkLists(d, p.g, p.list_begin, p.list_count);
  p.listed = p.list_begin[26] + p.list_count[26];
  p.section_bytes = PackedSectionBytes(d);
  return p;
}

// A table takes its bytes (an empty one 16, so that it still has an address) rounded up to the staging granule.
inline size_t StagedBytes(size_t bytes) { return ((bytes ? bytes : 16) + 63) & ~size_t(63); }

template <typename Dest, typename V>
void VisitSplineTables(Dest& c, const JxlHipSplines& sp, uint32_t ysize, V& v) {
  if (!sp.num_segments) return;
  v.copy(c.spl_seg, size_t(sp.num_segments) * 32, sp.segments);
  v.copy(c.spl_row_start, (size_t(ysize) + 1) * 4, sp.row_start);
  v.copy(c.spl_row_seg, std::max<size_t>(4, size_t(sp.num_row_segments) * 4), sp.row_segments);
}
template <typename Dest, typename V>
void VisitPatchTables(Dest& c, const JxlHipPatches& pt, uint32_t ysize, V& v) {
  if (!pt.num_positions) return;
  v.copy(c.pat_rec, size_t(pt.num_positions) * 32, pt.records);
  v.copy(c.pat_row_start, (size_t(ysize) + 1) * 4, pt.row_start);
  v.copy(c.pat_row_list, std::max<size_t>(4, size_t(pt.num_row_entries) * 4), pt.row_list);
}

// THE list of the tables a frame's blob holds that come from the descriptor: each named once, with its destination (a
// member of `c`: the context, or a test's double with members of the same names), its size, and its bytes: a copy of a
// descriptor array, or a builder that writes them in place. The upload walks it twice: with TableBound to size the blob,
// then with a visitor that places. v.phase(name) marks the phases that JXLHIP_UPLOAD_PROF reports.
// c.pass_bufs has at least d.num_passes entries.
template <typename Dest, typename V>
void VisitFrameTables(Dest& c, const JxlHipFrameDesc& d, const Plan& P, V& v) {
  const Geometry& g = P.g;
  const uint32_t* sec_word = nullptr;
  v.build(c.sec_word, g.nsec * 4, [&](void* p) { BuildSectionWords(d, static_cast<uint32_t*>(p)); sec_word = static_cast<uint32_t*>(p); });
  v.build(c.sections, P.section_bytes, [&](void* p) { PackSections(d, sec_word, static_cast<uint8_t*>(p), P.section_bytes); });
  v.copy(c.sec_size, g.nsec * 4, d.section_size);
  v.phase("sections");
  v.copy(c.blocks, size_t(d.num_blocks) * sizeof(JxlHipVarBlock), d.blocks);
  v.copy(c.gbb, (size_t(d.num_groups) + 1) * 4, d.group_block_begin);
  v.copy(c.bctx_lut, d.block_ctx_lut_size, d.block_ctx_lut);
  v.copy(c.dequant, size_t(d.dequant_floats) * 4, d.dequant);
  if (P.dc.dequant) {  // the coded integers; one extra-precision byte per group of 256 x 256 blocks
    v.copy(c.dc_q, g.nblk * 3 * 4, d.dc_quantised);
    if (d.dc_extra_precision) v.copy(c.dc_ep, size_t((d.xsize_blocks + 255) / 256) * ((d.ysize_blocks + 255) / 256), d.dc_extra_precision);
  } else if (!d.dc_device) {  // the dequantised image: the smoothing kernel's input, or final
    v.copy(P.dc.smooth ? c.dc_raw : c.dc, g.nblk * 3 * 4, d.dc);
  }
  if (P.dc.sigma) v.copy(c.sharp, g.nblk, d.sharpness);
  else if (d.inv_sigma) v.copy(c.inv_sigma, g.nblk * 4, d.inv_sigma);
  v.copy(c.ytox, g.ntiles, d.ytox);
  v.copy(c.ytob, g.ntiles, d.ytob);
  v.phase("planes");
  for (uint32_t p = 0; p < d.num_passes; p++) {
    const JxlHipPassDesc& s = d.passes[p];
    auto& pb = c.pass_bufs[p];
    v.copy(pb.ctx_map, s.ctx_map_size, s.ctx_map);
    v.copy(pb.alias, AliasBytes(s), s.alias);
    v.build(pb.alias_packed, AliasBytes(s), [&](void* q) { PackAlias(s, static_cast<uint32_t*>(q)); });
    v.copy(pb.cfg, size_t(s.num_clusters) * 4, s.uint_cfg);
    v.copy(pb.orders, size_t(s.orders_size) * 2, s.orders);
    v.copy(pb.ptable, s.use_prefix ? size_t(s.prefix_table_size) * 4 : 0, s.prefix_table);
    v.copy(pb.poffset, s.use_prefix ? size_t(s.num_clusters) * 4 : 0, s.prefix_offset);
  }
  v.phase("tables");
  VisitSplineTables(c, d.splines, d.ysize, v);
  VisitPatchTables(c, d.patches, d.ysize, v);
  if (g.ups != 1) v.copy(c.ups_kernel, size_t(g.ups) * g.ups * 25 * 4, d.upsampling_kernel);
  const uint32_t* tlist = nullptr;
  v.build(c.tlist, WorkListEntries(d) * 4, [&](void* p) { BuildWorkList(d, g, P.list_begin, static_cast<uint32_t*>(p)); tlist = static_cast<uint32_t*>(p); });
  v.build(c.trecs, WorkListEntries(d) * 16, [&](void* p) { BuildWorkRecords(d, tlist, P.listed, static_cast<uint32_t*>(p)); });
  v.phase("lists");
  v.build(c.block_recs, BlockRecEntries(d) * 4, [&](void* p) { BuildBlockRecs(d, static_cast<uint32_t*>(p)); });
  if (P.scan_order) v.build(c.dequant_scan, size_t(d.dequant_floats) * 4, [&](void* p) { BuildDequantScan(d, P.list_count, static_cast<float*>(p)); });
  v.phase("records");
}

// The first walk: the bytes of staging block and blob the list takes.
struct TableBound {
  size_t bytes = 0;
  template <typename B>
  void copy(B&, size_t n, const void*) { bytes += StagedBytes(n); }
  template <typename B, typename F>
  void build(B&, size_t n, F&&) { bytes += StagedBytes(n); }
  void phase(const char*) {}
};

}  // namespace upload
}  // namespace jxlhip
#endif  // JXH_UPLOAD_PLAN_H_
