// libjxl_amd — what jxlhip_modular_upload computes from a Modular frame descriptor, apart from where it puts it: the
// checks that admit a JxlHipModFrameDesc, the layout of everything the upload sends (channel pool, sections, tree / code
// blob, per-stream scratch and LZ77 windows), the builders of those tables, and the schedule of the inverse transforms.
// Pure functions: no context, no device call, no getenv; plain C++17, so tests/c/modular_upload_kats.cc holds every one of
// them on the CPU. The HIP layer (csrc/hip/jxl_hip_api.hip) decides where the bytes go and hands in the device addresses.
#ifndef JXH_MODULAR_UPLOAD_PLAN_H_
#define JXH_MODULAR_UPLOAD_PLAN_H_

#include <array>

#include "../hip/jxl_hip_modular_abi.h"
#include "jxh_upload_plan.h"

namespace jxlhip {
namespace upload {

// The only context state the checks read: jxlhip_set_option("keep_xyb_planes") makes float planes necessary.
struct ModUploadOptions {
  bool keep_xyb = false;
};

// --------------------------------------------------------------------------------------------------------- checks
// Every reason to refuse a descriptor, each stated once below. tests/c/modular_upload_kats.cc breaks each rule in turn
// and fails when a rule here has no row in its table. These are device-safety rules: the kernels index with the tables
// unchecked, the stream kernel's tree walk follows child indices unchecked, and the transform kernels write wherever
// their rectangles say.
enum ModRule : int {
  kModRuleSizes,              // no pixels, sections, trees or codes; a code per tree
  kModRuleNumColor,           // 1 or 3 colour channels
  kModRuleNullTable,          // (own) a table with a non-zero count has an address
  kModRuleSizeWrap,           // (own) the pool's bytes fit size_t, a code's table words 32 bits
  kModRuleTreeProperty,       // (unsupported) a property beyond 15 + four previous channels
  kModRuleTreeChildren,       // children exist and lie behind their parent, or the kernel's tree walk spins forever
  kModRuleTreeLeaf,           // predictor known, context inside the code's context map
  kModRuleCodeLimits,         // clusters 1..256, a context map, log_alpha 5..8 for rANS
  kModRuleCtxMapEntries,      // every entry names a cluster
  kModRulePrefixTables,       // every index a prefix lookup can form is inside the table
  kModRuleLz77,               // distance context, minimum length
  kModRuleRectInsideBuffer,   // a stream's channel lies inside its buffer
  kModRuleStreamIndices,      // section, tree (a present one), code and rectangles exist
  kModRuleStreamBitOffset,    // inside its section
  kModRuleStreamProps,        // 16 .. kModMaxProps properties
  kModRuleOpFields,           // kind, buffer count, local flag, level
  kModRuleOpBuffers,          // every buffer of an operation exists
  kModRuleOpRectangles,       // every rectangle of an operation lies inside its buffer
  kModRuleRctType,            // below 42
  kModRulePaletteShape,       // 1..4 channels, the palette a whole buffer of that many rows and `param` columns
  kModRuleUnsqueezeAlias,     // an unsqueeze output is not one of its inputs (a line is read while it is written)
  kModRuleOutBuffers,         // the output buffers exist and have the frame's size
  kModRuleSampleDepth,        // integer or float sample types the writer knows; integer alpha of at most 24 bits
  kModRuleSplinesGrey,        // (unsupported) splines over a grey frame
  kModRuleXybGrey,            // (unsupported) an XYB frame has three channels
  kModRuleColorTarget,        // transfer function and tone mapping known
  kModRuleColorTargetLinear,  // a colour target takes the linear RGB of an XYB frame
  kModRuleSplineTables,       // pointers and counts
  kModRuleSplineRows,         // row lists consistent, every entry a segment
  kModRulePatchAlpha,         // (unsupported) patches that blend through alpha: the frame's alpha is an integer channel
  kModRulePatchTables,        // pointers and counts
  kModRulePatchRows,          // row lists consistent, every entry one of its patch's rows
  kModRulePatchRecords,       // rectangles inside the frame and their reference frame, modes known
  kModRuleFloatPlanesGrey,    // (unsupported) patches or kept XYB planes of a grey frame
  kNumModRules
};

#define JXH_REFUSE(cond, which, code) \
  do {                                \
    if (cond) {                       \
      if (rule) *rule = which;        \
      return code;                    \
    }                                 \
  } while (0)
#define JXH_INVALID(cond, which) JXH_REFUSE(cond, which, JXLHIP_ERR_INVALID_ARGUMENT)

// Sample depths: low byte = bits, bits 8..15 = exponent bits of a float type (image_metadata.cc BitDepth: 2..8, mantissa 2..23)
inline bool ModDepthOk(uint32_t d) {
  const uint32_t bits = d & 0xFF, e = (d >> 8) & 0xFF;
  if (d >> 16) return false;
  if (e == 0) return bits >= 1 && bits <= 31;
  return e >= 2 && e <= 8 && bits >= e + 3 && bits <= e + 24 && bits <= 32;
}
// The LZ77 window of a stream: as large as the stream can fill, at most the format's 2^20 (32-bit words).
inline uint32_t ModWindowWords(uint32_t num_samples) {
  uint32_t w = 256;
  while (w < num_samples && w < (1u << 20)) w <<= 1;
  return w;
}
inline size_t ModBufferInts(const JxlHipModBuffer& b) { return (size_t(b.w) * b.h + 3) & ~size_t(3); }
inline bool ModFloatPlanes(const JxlHipModFrameDesc& d, const ModUploadOptions& o) {
  return d.splines.num_segments || o.keep_xyb || d.patches.num_positions;
}

// Whether jxlhip_modular_upload takes the descriptor: 0, or the code it returns (`rule`: which rule refused).
inline int CheckModFrameDesc(const JxlHipModFrameDesc& d, const ModUploadOptions& o, ModRule* rule = nullptr) {
  JXH_INVALID(!d.xsize || !d.ysize || !d.num_sections || !d.num_trees || !d.num_codes || d.num_trees != d.num_codes, kModRuleSizes);
  JXH_INVALID(d.num_color != 1 && d.num_color != 3, kModRuleNumColor);
  JXH_INVALID(!d.codestream || !d.section_offset || !d.section_size || !d.trees || !d.tree_size || !d.codes || (d.num_buffers && !d.buffers) ||
                  (d.num_rects && !d.rects) || (d.num_streams && !d.streams) || (d.num_ops && !d.ops),
              kModRuleNullTable);
  {  // (the pool's byte size, with its 4 spare ints, fits size_t)
    size_t pool = 0;
    for (uint32_t i = 0; i < d.num_buffers; i++) {
      const size_t ints = ModBufferInts(d.buffers[i]);
      JXH_INVALID(ints > SIZE_MAX / 8 - pool, kModRuleSizeWrap);
      pool += ints;
    }
  }
  // ---- trees and codes: every index the stream kernel can form from them
  for (uint32_t i = 0; i < d.num_trees; i++) {
    const JxlHipModCode& k = d.codes[i];
    if (!d.tree_size[i]) continue;  // (an absent global tree: neither it nor its code is read)
    // (a context map without an address is the leaf rule's: every tree ends in a leaf)
    JXH_INVALID(!d.trees[i] || !k.uint_cfg || (k.use_prefix ? !k.prefix_table || !k.prefix_offset : !k.alias), kModRuleNullTable);
    for (uint32_t n = 0; n < d.tree_size[i]; n++) {
      const JxlHipModTreeNode& nd = d.trees[i][n];
      JXH_REFUSE(nd.property >= int32_t(kModMaxProps), kModRuleTreeProperty, JXLHIP_ERR_UNSUPPORTED);
      // children behind their parent (the breadth-first order dec_ma.cc:107-159 produces): a back edge would make the
      // kernel's tree walk spin forever
      JXH_INVALID(nd.property >= 0 && (nd.lchild >= d.tree_size[i] || nd.rchild >= d.tree_size[i] || nd.lchild <= n || nd.rchild <= n),
                  kModRuleTreeChildren);
      JXH_INVALID(nd.property < 0 && (nd.predictor > 13 || nd.lchild >= k.ctx_map_size || !k.ctx_map), kModRuleTreeLeaf);
    }
    JXH_INVALID(!k.num_clusters || k.num_clusters > 256 || !k.ctx_map_size || (!k.use_prefix && (k.log_alpha < 5 || k.log_alpha > 8)), kModRuleCodeLimits);
    for (uint32_t j = 0; j < k.ctx_map_size; j++) JXH_INVALID(k.ctx_map[j] >= k.num_clusters, kModRuleCtxMapEntries);
    if (k.use_prefix) {
      JXH_INVALID(k.prefix_table_size > 0xFFFFFFFFu - 2 * k.num_clusters, kModRuleSizeWrap);
      for (uint32_t j = 0; j < k.num_clusters; j++)
        JXH_INVALID(!ValidPrefixTables(k.prefix_offset[j], k.prefix_table, k.prefix_table_size), kModRulePrefixTables);
    }
    JXH_INVALID(k.lz77 && (k.lz_dist_ctx >= k.num_clusters || !k.lz_min_length), kModRuleLz77);
  }
  // ---- rectangles and streams
  auto inside = [&](uint32_t buffer, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
    return uint64_t(x0) + w <= d.buffers[buffer].w && uint64_t(y0) + h <= d.buffers[buffer].h;
  };
  for (uint32_t i = 0; i < d.num_rects; i++) {
    const JxlHipModRect& q = d.rects[i];
    JXH_INVALID(q.buffer >= d.num_buffers || !inside(q.buffer, q.x0, q.y0, q.w, q.h), kModRuleRectInsideBuffer);
  }
  for (uint32_t i = 0; i < d.num_streams; i++) {
    const JxlHipModStream& q = d.streams[i];
    // (the tree must be a present one; the CODE is not asked to be: a stream that names the code slot of an absent tree,
    // which no code rule above has seen, is taken as it always was. The front-end gives a stream its tree's own code.)
    JXH_INVALID(q.section >= d.num_sections || q.tree >= d.num_trees || q.code >= d.num_codes || !d.tree_size[q.tree] ||
                    uint64_t(q.first_rect) + q.num_rects > d.num_rects,
                kModRuleStreamIndices);
    JXH_INVALID(q.bit_offset > uint64_t(d.section_size[q.section]) * 8, kModRuleStreamBitOffset);
    JXH_INVALID(q.num_props < 16 || q.num_props > uint32_t(kModMaxProps), kModRuleStreamProps);
  }
  // ---- operations: no kernel reads or writes outside the pool
  for (uint32_t i = 0; i < d.num_ops; i++) {
    const JxlHipModOp& op = d.ops[i];
    const uint32_t nbuf = op.kind == 0 ? 3 : (op.kind == 1 ? 2 + op.nb : 3);
    JXH_INVALID(op.kind > 3 || nbuf > 6 || op.local > 1 || op.level >= d.num_ops, kModRuleOpFields);
    for (uint32_t j = 0; j < nbuf; j++) JXH_INVALID(op.buf[j] >= d.num_buffers, kModRuleOpBuffers);
    // the w x h rectangle of buffer j at that buffer's origin lies inside it
    auto in = [&](uint32_t j, uint32_t w, uint32_t h) { return inside(op.buf[j], op.ox[j], op.oy[j], w, h); };
    if (op.kind == 0) {
      for (uint32_t j = 0; j < 3; j++) JXH_INVALID(!in(j, op.w, op.h), kModRuleOpRectangles);
      JXH_INVALID(op.param >= 42, kModRuleRctType);
    } else if (op.kind == 1) {  // the palette is a whole buffer; index and outputs are rectangles
      JXH_INVALID(op.nb < 1 || op.nb > 4 || d.buffers[op.buf[0]].h < op.nb || op.param != d.buffers[op.buf[0]].w || op.ox[0] || op.oy[0],
                  kModRulePaletteShape);
      for (uint32_t j = 1; j < 2 + op.nb; j++) JXH_INVALID(!in(j, op.w, op.h), kModRuleOpRectangles);
    } else {  // averages and residuals follow from the output's size: they add up by construction, each must lie in its buffer
      const bool hz = op.kind == 2;
      const uint32_t n = hz ? op.w : op.h, na = n - n / 2, nr = n / 2;
      JXH_INVALID(!in(0, hz ? na : op.w, hz ? op.h : na) || !in(1, hz ? nr : op.w, hz ? op.h : nr) || !in(2, op.w, op.h), kModRuleOpRectangles);
      JXH_INVALID(op.buf[2] == op.buf[0] || op.buf[2] == op.buf[1], kModRuleUnsqueezeAlias);
    }
  }
  // ---- output
  for (uint32_t j = 0; j < d.num_color + (d.has_alpha ? 1 : 0); j++)
    JXH_INVALID(d.out_buffer[j] >= d.num_buffers || d.buffers[d.out_buffer[j]].w != d.xsize || d.buffers[d.out_buffer[j]].h != d.ysize, kModRuleOutBuffers);
  JXH_INVALID(!ModDepthOk(d.bits) || !ModDepthOk(d.alpha_bits) || (d.alpha_bits >> 8) || (d.alpha_bits & 0xFF) > 24, kModRuleSampleDepth);
  JXH_REFUSE(d.splines.num_segments && d.num_color != 3, kModRuleSplinesGrey, JXLHIP_ERR_UNSUPPORTED);
  JXH_REFUSE(d.xyb && d.num_color != 3, kModRuleXybGrey, JXLHIP_ERR_UNSUPPORTED);
  if (d.color_target) {
    JXH_INVALID(d.color_target->tf > JXLHIP_TF_GAMMA || d.color_target->tone > JXLHIP_TONE_HLG_OOTF, kModRuleColorTarget);
    JXH_INVALID(d.color_target->tf && (!d.xyb || d.linear_output != 1), kModRuleColorTargetLinear);
  }
  // ---- splines and patches, checked like a VarDCT frame's
  Rule sub = kNumRules;
  int r;
  if ((r = CheckSplines(d.splines, d.ysize, &sub))) JXH_REFUSE(true, sub == kRuleSplineTables ? kModRuleSplineTables : kModRuleSplineRows, r);
  JXH_REFUSE(d.patches.num_positions && d.patches.uses_alpha, kModRulePatchAlpha, JXLHIP_ERR_UNSUPPORTED);
  if ((r = CheckPatches(d.patches, d.ysize, d.xsize, d.ysize, &sub)))
    JXH_REFUSE(true, sub == kRulePatchTables ? kModRulePatchTables : (sub == kRulePatchRows ? kModRulePatchRows : kModRulePatchRecords), r);
  JXH_REFUSE(ModFloatPlanes(d, o) && d.num_color != 3, kModRuleFloatPlanesGrey, JXLHIP_ERR_UNSUPPORTED);
  return 0;
}
#undef JXH_INVALID
#undef JXH_REFUSE

// ----------------------------------------------------------------------------------------------------------- plan
// Where everything an accepted descriptor sends lies, relative to the bases the HIP layer allocates.
struct ModPlan {
  // channel pool: first int32 of every buffer (each a multiple of 4 ints, so that every buffer starts 16-byte aligned)
  std::vector<size_t> buf_off;
  size_t pool_ints = 0;
  // sections: 4-byte aligned starts, at least 8 zero bytes behind each (the bit reader's word loaded ahead), 16 at the end
  std::vector<size_t> sec_off;
  size_t section_bytes = 0;
  // tree / code blob, every item 16-byte aligned: the trees' packed nodes, per present code {ctx_map, alias, cfg,
  // prefix_table, prefix_offset}, then the ModCode array
  std::vector<size_t> tree_at;
  std::vector<std::array<size_t, 5>> code_parts;
  size_t codes_at = 0, blob_bytes = 0;
  std::vector<uint32_t> table_words;  // ModCode::table_words per code (0 for an absent one)
  // per stream: weighted-predictor scratch (ints) and LZ77 window (words); mask = window size - 1
  std::vector<size_t> scratch_at, window_at;
  std::vector<uint32_t> window_mask;
  size_t scratch_ints = 0, window_words = 0;
  bool float_planes = false;
};
inline std::array<size_t, 5> ModCodePartBytes(const JxlHipModCode& k) {
  return {size_t(k.ctx_map_size), k.use_prefix ? 0 : (size_t(k.num_clusters) << k.log_alpha) * 8, size_t(k.num_clusters) * 4,
          k.use_prefix ? size_t(k.prefix_table_size) * 4 : 0, k.use_prefix ? size_t(k.num_clusters) * 4 : 0};
}
inline ModPlan MakeModPlan(const JxlHipModFrameDesc& d, const ModUploadOptions& o) {
  ModPlan P;
  P.buf_off.resize(d.num_buffers);
  for (uint32_t i = 0; i < d.num_buffers; i++) {
    P.buf_off[i] = P.pool_ints;
    P.pool_ints += ModBufferInts(d.buffers[i]);
  }
  P.sec_off.resize(d.num_sections);
  for (uint32_t i = 0; i < d.num_sections; i++) {
    P.sec_off[i] = P.section_bytes;
    P.section_bytes += (size_t(d.section_size[i]) + 3 + 8) & ~size_t(3);
  }
  P.section_bytes += 16;
  size_t cursor = 0;
  auto put = [&](size_t bytes) {
    const size_t at = (cursor + 15) & ~size_t(15);
    cursor = at + bytes;
    return at;
  };
  P.tree_at.resize(d.num_trees);
  for (uint32_t i = 0; i < d.num_trees; i++) P.tree_at[i] = put(size_t(d.tree_size[i]) * sizeof(ModTreeNode));
  P.code_parts.assign(d.num_codes, {0, 0, 0, 0, 0});
  P.table_words.assign(d.num_codes, 0);
  for (uint32_t i = 0; i < d.num_codes; i++) {
    if (!d.tree_size[i]) continue;  // (an absent global tree)
    const JxlHipModCode& k = d.codes[i];
    const std::array<size_t, 5> bytes = ModCodePartBytes(k);
    for (int j = 0; j < 5; j++) P.code_parts[i][j] = put(bytes[j]);
    P.table_words[i] = k.use_prefix ? k.prefix_table_size + 2 * k.num_clusters : ((k.num_clusters << k.log_alpha) * 2 + k.num_clusters);
  }
  P.codes_at = put(size_t(d.num_codes) * sizeof(ModCode));
  P.blob_bytes = cursor;
  P.scratch_at.assign(d.num_streams, 0);
  P.window_at.assign(d.num_streams, 0);
  P.window_mask.assign(d.num_streams, 0);
  for (uint32_t i = 0; i < d.num_streams; i++) {
    const JxlHipModStream& q = d.streams[i];
    if (q.uses_wp) {
      P.scratch_at[i] = P.scratch_ints;
      P.scratch_ints += (size_t(q.max_width) + 2) * 2 * kModWpEntry;
    }
    if (d.codes[q.code].lz77) {
      const uint32_t w = ModWindowWords(q.num_samples);
      P.window_at[i] = P.window_words;
      P.window_mask[i] = w - 1;
      P.window_words += w;
    }
  }
  P.float_planes = ModFloatPlanes(d, o);
  return P;
}

// -------------------------------------------------------------------------------------------------------- builders
// Each writes into memory the caller gives it (the staging block), with the device addresses the tables will have.
struct ModBases {
  uintptr_t pool = 0, sections = 0, blob = 0, rects = 0, scratch = 0, windows = 0, status = 0, end_bits = 0;
};
template <typename T>
inline T* ModAddr(uintptr_t base, size_t bytes) { return reinterpret_cast<T*>(base + bytes); }

inline void PackModSections(const JxlHipModFrameDesc& d, const ModPlan& P, uint8_t* packed) {  // P.section_bytes
  size_t end = 0;
  for (uint32_t i = 0; i < d.num_sections; i++) {
    memset(packed + end, 0, P.sec_off[i] - end);
    if (d.section_size[i]) memcpy(packed + P.sec_off[i], d.codestream + d.section_offset[i], d.section_size[i]);
    end = P.sec_off[i] + d.section_size[i];
  }
  memset(packed + end, 0, P.section_bytes - end);
}

// The kernel's 16-byte nodes: leaves carry -1 - predictor, the offset, the histogram their context maps to, the multiplier.
inline ModTreeNode PackModTreeNode(const JxlHipModTreeNode& nd, const JxlHipModCode& k) {
  ModTreeNode o;
  if (nd.property >= 0) {
    o.property = nd.property;
    o.splitval = nd.splitval;
    o.lchild = nd.lchild;
    o.rchild = nd.rchild;
  } else {
    o.property = -1 - int32_t(nd.predictor);
    o.splitval = nd.offset;
    o.lchild = k.ctx_map[nd.lchild];
    o.rchild = nd.multiplier;
  }
  return o;
}
inline void BuildModBlob(const JxlHipModFrameDesc& d, const ModPlan& P, uint8_t* blob, uintptr_t dev) {  // P.blob_bytes; gaps zero
  memset(blob, 0, P.blob_bytes);
  for (uint32_t i = 0; i < d.num_trees; i++) {
    ModTreeNode* t = reinterpret_cast<ModTreeNode*>(blob + P.tree_at[i]);
    for (uint32_t n = 0; n < d.tree_size[i]; n++) t[n] = PackModTreeNode(d.trees[i][n], d.codes[i]);
  }
  ModCode* codes = reinterpret_cast<ModCode*>(blob + P.codes_at);
  for (uint32_t i = 0; i < d.num_codes; i++) {
    const JxlHipModCode& k = d.codes[i];
    const std::array<size_t, 5>& at = P.code_parts[i];
    if (d.tree_size[i]) {
      const void* src[5] = {k.ctx_map, k.alias, k.uint_cfg, k.prefix_table, k.prefix_offset};
      const std::array<size_t, 5> bytes = ModCodePartBytes(k);
      for (int j = 0; j < 5; j++)
        if (bytes[j]) memcpy(blob + at[j], src[j], bytes[j]);
    }
    ModCode& mc = codes[i];
    mc.ctx_map = ModAddr<const uint8_t>(dev, at[0]);
    mc.alias = ModAddr<const ModAliasEntry>(dev, at[1]);
    mc.cfg = ModAddr<const uint32_t>(dev, at[2]);
    mc.prefix_table = ModAddr<const uint32_t>(dev, at[3]);
    mc.prefix_offset = ModAddr<const uint32_t>(dev, at[4]);
    mc.log_alpha = k.log_alpha;
    mc.use_prefix = k.use_prefix;
    mc.lz77 = k.lz77;
    mc.lz_min_symbol = k.lz_min_symbol;
    mc.lz_min_length = k.lz_min_length;
    mc.lz_len_cfg = k.lz_len_cfg;
    mc.lz_dist_ctx = k.lz_dist_ctx;
    mc.table_words = P.table_words[i];
    mc.num_clusters = k.num_clusters;
  }
}

inline size_t ModChannelEntries(const JxlHipModFrameDesc& d) { return d.num_rects ? d.num_rects : 1; }
inline void BuildModChannels(const JxlHipModFrameDesc& d, const ModPlan& P, ModChannel* rects, uintptr_t pool) {
  memset(rects, 0, ModChannelEntries(d) * sizeof(ModChannel));
  for (uint32_t i = 0; i < d.num_rects; i++) {
    const JxlHipModRect& q = d.rects[i];
    const uint32_t stride = d.buffers[q.buffer].w;
    rects[i].data = ModAddr<int32_t>(pool, (P.buf_off[q.buffer] + size_t(q.y0) * stride + q.x0) * 4);
    rects[i].stride = stride;
    rects[i].w = q.w;
    rects[i].h = q.h;
    rects[i].sig = q.sig;
  }
}

inline void BuildModStreams(const JxlHipModFrameDesc& d, const ModPlan& P, ModStream* streams, const ModBases& b) {
  if (d.num_streams) memset(streams, 0, size_t(d.num_streams) * sizeof(ModStream));
  for (uint32_t i = 0; i < d.num_streams; i++) {
    const JxlHipModStream& q = d.streams[i];
    ModStream& o = streams[i];
    o.words = ModAddr<const uint32_t>(b.sections, P.sec_off[q.section]);
    o.bit_offset = q.bit_offset;
    o.size_bytes = d.section_size[q.section];
    o.tree = ModAddr<const ModTreeNode>(b.blob, P.tree_at[q.tree]);
    o.tree_nodes = d.tree_size[q.tree];
    o.code = ModAddr<const ModCode>(b.blob, P.codes_at + size_t(q.code) * sizeof(ModCode));
    o.channels = ModAddr<const ModChannel>(b.rects, size_t(q.first_rect) * sizeof(ModChannel));
    o.num_channels = q.num_rects;
    o.stream_id = q.stream_id;
    o.first_channel_index = q.first_channel_index;
    memcpy(o.wp, q.wp, sizeof(o.wp));
    o.uses_wp = q.uses_wp;
    o.num_props = q.num_props;
    o.dist_multiplier = q.dist_multiplier;
    o.wp_scratch = q.uses_wp ? ModAddr<int32_t>(b.scratch, P.scratch_at[i] * 4) : nullptr;
    o.lz_window = d.codes[q.code].lz77 ? ModAddr<uint32_t>(b.windows, P.window_at[i] * 4) : nullptr;
    o.lz_window_mask = P.window_mask[i];
    o.status = ModAddr<uint32_t>(b.status, size_t(i) * 4);
    o.end_bit = ModAddr<uint32_t>(b.end_bits, size_t(i) * 4);
  }
}

// ------------------------------------------------------------------------------------- the operation schedule
// One launch of the Modular transform / output kernels over the frames of a set.
struct ModLaunch {
  uint32_t kind;  // 0 RCT, 1 palette, 2 unsqueeze, 3 output, 4 / 5 / 6 float planes, splines, patches
  size_t offset;  // of the first parameter block in the blob
  uint32_t count, gx, gy;
};
// What the schedule reads of a frame: its pool's device address and layout, and its operations.
struct ModFrameOps {
  uintptr_t pool;
  const size_t* buf_off;
  const uint32_t* buf_w;
  const JxlHipModOp* ops;
  size_t num_ops;
};
inline void ModBlobAlign(std::vector<uint8_t>* blob) { blob->resize((blob->size() + 15) & ~size_t(15)); }
inline void ModBlobAppend(std::vector<uint8_t>* blob, const void* p, size_t bytes) {
  const size_t at = blob->size();
  blob->resize(at + bytes);
  memcpy(blob->data() + at, p, bytes);
}
// The inverse transforms of a set of frames (kinds 0..2), as launches over parameter-block arrays. First the local
// phase: the operations that undo the transforms of single group streams. They are group-sized, those of different
// groups touch disjoint rectangles and private buffers, and inside a group `level` orders them; so ALL operations of one
// level and kind, of every group of every frame, are one launch (a frame with an RCT in each of its 135 groups: one RCT
// launch). Then the frames' own transforms on whole channels, level k of every frame that has one in one launch per kind.
// The two never share a launch: its grid is sized for its largest block, and one 4K channel beside thousands of group
// blocks would start mostly empty workgroups. Blocks are appended to `blob`, launches to `launches`.
inline void BuildModSchedule(const ModFrameOps* frames, size_t n, std::vector<uint8_t>* blob, std::vector<ModLaunch>* launches) {
  struct Ref {
    uint32_t phase, level, kind;  // kind: the ModLaunch kind
    uint32_t frame, op;
  };
  std::vector<Ref> refs;
  for (size_t i = 0; i < n; i++)
    for (size_t k = 0; k < frames[i].num_ops; k++) {
      const JxlHipModOp& op = frames[i].ops[k];
      refs.push_back({op.local ? 0u : 1u, op.level, op.kind >= 2 ? 2u : op.kind, uint32_t(i), uint32_t(k)});
    }
  std::stable_sort(refs.begin(), refs.end(), [](const Ref& a, const Ref& b) {
    return a.phase != b.phase ? a.phase < b.phase : (a.level != b.level ? a.level < b.level : a.kind < b.kind);
  });
  for (size_t first = 0; first < refs.size();) {
    size_t end = first;
    while (end < refs.size() && refs[end].phase == refs[first].phase && refs[end].level == refs[first].level && refs[end].kind == refs[first].kind) end++;
    const uint32_t kind = refs[first].kind;
    ModBlobAlign(blob);
    ModLaunch L{kind, blob->size(), 0, 0, 0};
    for (size_t q = first; q < end; q++) {
      const ModFrameOps& F = frames[refs[q].frame];
      const JxlHipModOp& op = F.ops[refs[q].op];
      auto at = [&](uint32_t j) { return ModAddr<int32_t>(F.pool, (F.buf_off[op.buf[j]] + size_t(op.oy[j]) * F.buf_w[op.buf[j]] + op.ox[j]) * 4); };
      if (!op.w || !op.h) continue;
      if (kind == 0) {
        ModRct p;
        memset(&p, 0, sizeof(p));
        for (uint32_t j = 0; j < 3; j++) {
          p.stride[j] = F.buf_w[op.buf[j]];
          p.c[j] = at(j);
        }
        p.w = op.w;
        p.h = op.h;
        p.type = op.param;
        ModBlobAppend(blob, &p, sizeof(p));
        L.gx = std::max(L.gx, (op.w + 255) / 256);
        L.gy = std::max(L.gy, op.h);
      } else if (kind == 1) {
        ModPalette p;
        memset(&p, 0, sizeof(p));
        p.palette = ModAddr<int32_t>(F.pool, F.buf_off[op.buf[0]] * 4);
        p.index = at(1);
        p.index_stride = F.buf_w[op.buf[1]];
        for (uint32_t j = 0; j < op.nb; j++) {
          p.out[j] = at(2 + j);
          p.out_stride[j] = F.buf_w[op.buf[2 + j]];
        }
        p.palette_w = op.param;
        p.nb = op.nb;
        p.w = op.w;
        p.h = op.h;
        p.bit_depth = op.bit_depth;
        ModBlobAppend(blob, &p, sizeof(p));
        L.gx = std::max(L.gx, (op.w + 255) / 256);
        L.gy = std::max(L.gy, op.h);
      } else {
        const bool hz = op.kind == 2;
        const uint32_t len = hz ? op.w : op.h;
        ModUnsqueeze p;
        memset(&p, 0, sizeof(p));
        p.avg = at(0);
        p.res = at(1);
        p.out = at(2);
        p.lines = hz ? op.h : op.w;
        p.na = len - len / 2;
        p.nr = len / 2;
        const uint32_t wa = F.buf_w[op.buf[0]], wr = F.buf_w[op.buf[1]], wo = F.buf_w[op.buf[2]];
        p.avg_line = hz ? wa : 1;
        p.avg_step = hz ? 1 : wa;
        p.res_line = hz ? wr : 1;
        p.res_step = hz ? 1 : wr;
        p.out_line = hz ? wo : 1;
        p.out_step = hz ? 1 : wo;
        ModBlobAppend(blob, &p, sizeof(p));
        L.gx = std::max(L.gx, (p.lines + 63) / 64);
        L.gy = 1;
      }
      L.count++;
    }
    if (L.count) launches->push_back(L);
    first = end;
  }
}

}  // namespace upload
}  // namespace jxlhip
#endif  // JXH_MODULAR_UPLOAD_PLAN_H_
