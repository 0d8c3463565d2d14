// What jxlhip_modular_upload computes on the host (libjxl_amd/csrc/host/jxh_modular_upload_plan.h), held on the CPU over
// the descriptors of real streams. Built by tests/test_kats.py with -fsanitize=address,undefined around
// libjxl_amd/csrc/api/jxl_api.cc like upload_plan_kats.cc; the HIP entry points are no-device doubles, except
// jxlhip_modular_upload: this program's double receives the descriptor jxlamd_modframe_upload built and runs the checks
// below on it.
//   refusals  the descriptor is accepted as parsed; for every rule of CheckModFrameDesc a copy in which one field, table
//             entry or pointer breaks that rule and nothing else is refused by that rule, with the code the table states
//   layout    against fake base addresses: channel buffers disjoint and 4-int aligned; sections 4-byte aligned, their
//             bytes, at least 8 zero bytes behind each; blob items 16-byte aligned and disjoint; every pointer of every
//             ModCode, ModChannel and ModStream inside its region with its full extent; leaves carry -1 - predictor, the
//             mapped cluster, the multiplier; LZ77 windows powers of two in 256..2^20 and disjoint; WP scratch disjoint
//   schedule  every non-empty operation in exactly one launch of its own phase, level and kind; launches local before
//             global, then by level; grids cover their largest block; each block addresses its operation's rectangles
// usage: modular_upload_kats file [second]     (second: the frame behind the first, whose patches read the first)
// prints "exercised: <rules>" for the caller to add up
#include "../../libjxl_amd/csrc/api/jxl_api.cc"
#define KATS_OWN_MODULAR_UPLOAD
#include "no_device_doubles.inc"
#include "../../libjxl_amd/csrc/host/jxh_modular_upload_plan.h"

#include <functional>

namespace up = jxlhip::upload;

#define EXPECT(cond, ...)                                        \
  do {                                                           \
    if (!(cond)) {                                               \
      fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                              \
      fprintf(stderr, "\n");                                     \
      return 1;                                                  \
    }                                                            \
  } while (0)

static const char* const kRuleNames[] = {
    "Sizes", "NumColor", "NullTable", "SizeWrap", "TreeProperty", "TreeChildren", "TreeLeaf", "CodeLimits", "CtxMapEntries", "PrefixTables", "Lz77",
    "RectInsideBuffer", "StreamIndices", "StreamBitOffset", "StreamProps", "OpFields", "OpBuffers", "OpRectangles", "RctType", "PaletteShape",
    "UnsqueezeAlias", "OutBuffers", "SampleDepth", "SplinesGrey", "XybGrey", "ColorTarget", "ColorTargetLinear", "SplineTables", "SplineRows",
    "PatchAlpha", "PatchTables", "PatchRows", "PatchRecords", "FloatPlanesGrey"};
static_assert(sizeof(kRuleNames) / sizeof(kRuleNames[0]) == up::kNumModRules, "a name for every rule of jxh_modular_upload_plan.h");

// A descriptor with copies of the arrays the mutations write to, and room for the spline / patch tables some rows add.
struct Mut {
  JxlHipModFrameDesc d;
  up::ModUploadOptions o;
  std::vector<std::vector<JxlHipModTreeNode>> trees;
  std::vector<const JxlHipModTreeNode*> tree_ptr;
  std::vector<JxlHipModCode> codes;
  std::vector<std::vector<uint8_t>> ctx_map;
  std::vector<JxlHipModBuffer> buffers;
  std::vector<JxlHipModRect> rects;
  std::vector<JxlHipModStream> streams;
  std::vector<JxlHipModOp> ops;
  JxlHipColorTarget ct;
  std::vector<uint32_t> rows, one, record;
  float segment[8], plane[1];
  uint32_t t = 0;  // the first tree that is there
  explicit Mut(const JxlHipModFrameDesc& src) : d(src) {
    trees.resize(d.num_trees);
    tree_ptr.resize(d.num_trees);
    codes.assign(d.codes, d.codes + d.num_codes);
    ctx_map.resize(d.num_codes);
    for (uint32_t i = 0; i < d.num_trees; i++) {
      trees[i].assign(d.trees[i], d.trees[i] + d.tree_size[i]);
      tree_ptr[i] = trees[i].data();
      if (!d.tree_size[i]) continue;
      ctx_map[i].assign(codes[i].ctx_map, codes[i].ctx_map + codes[i].ctx_map_size);
      codes[i].ctx_map = ctx_map[i].data();
    }
    while (t + 1 < d.num_trees && !d.tree_size[t]) t++;
    buffers.assign(d.buffers, d.buffers + d.num_buffers);
    rects.assign(d.rects, d.rects + d.num_rects);
    streams.assign(d.streams, d.streams + d.num_streams);
    ops.assign(d.ops, d.ops + d.num_ops);
    d.trees = tree_ptr.data();
    d.codes = codes.data();
    d.buffers = buffers.data();
    d.rects = rects.data();
    d.streams = streams.data();
    d.ops = ops.data();
    memset(&ct, 0, sizeof(ct));
    // one spline segment / one patch of one pixel, drawn in row 0
    rows.assign(size_t(d.ysize) + 1, 1);
    rows[0] = 0;
    one.assign(1, 0);
    record = {0, 0, 1, 1, 0, 0, 0, 1};
    memset(segment, 0, sizeof(segment));
  }
  void AddSplines() {
    memset(&d.splines, 0, sizeof(d.splines));
    d.splines.num_segments = d.splines.num_row_segments = 1;
    d.splines.segments = segment;
    d.splines.row_start = rows.data();
    d.splines.row_segments = one.data();
  }
  void AddPatches() {
    memset(&d.patches, 0, sizeof(d.patches));
    d.patches.num_positions = d.patches.num_row_entries = 1;
    d.patches.records = record.data();
    d.patches.row_start = rows.data();
    d.patches.row_list = one.data();
    d.patches.slot_planes[0] = plane;  // (a device address to the upload: never read on the host)
    d.patches.slot_w[0] = d.patches.slot_h[0] = 1;
  }
  int FirstOp(uint32_t kind_lo, uint32_t kind_hi) const {
    for (size_t i = 0; i < ops.size(); i++)
      if (ops[i].kind >= kind_lo && ops[i].kind <= kind_hi && ops[i].w && ops[i].h) return int(i);
    return -1;
  }
  JxlHipModTreeNode& FirstLeaf() {
    for (JxlHipModTreeNode& n : trees[t])
      if (n.property < 0) return n;
    return trees[t][0];
  }
};

// At least one row per rule: when the stream can reach it, a set-up that the checks still take (tables the stream does not have),
// and the one change that breaks the rule. The codes are those jxlhip_modular_upload returned for the same change before
// its checks moved to the header: "unsupported" for tree properties beyond the kernel's, grey frames with splines, XYB,
// patches or kept planes, and alpha patches; "invalid argument" for everything else, as for the two rules that refuse
// what used to be read out of bounds (NullTable, SizeWrap).
struct Row {
  up::ModRule rule;
  int code;
  std::function<bool(const Mut&)> applies;
  std::function<void(Mut&)> setup;
  std::function<void(Mut&)> mutate;
};
static bool Always(const Mut&) { return true; }
static void Nothing(Mut&) {}
static bool Colour(const Mut& m) { return m.d.num_color == 3; }
static bool HasStreams(const Mut& m) { return m.d.num_streams != 0; }
static const int kInv = JXLHIP_ERR_INVALID_ARGUMENT, kUns = JXLHIP_ERR_UNSUPPORTED;

static std::vector<Row> Rows() {
  using M = Mut&;
  using C = const Mut&;
  return {
      {up::kModRuleSizes, kInv, Always, Nothing, [](M m) { m.d.num_sections = 0; }},
      {up::kModRuleNumColor, kInv, Always, Nothing, [](M m) { m.d.num_color = 2; }},
      // (the two rules of the header's own are several conditions each: a row for each kind of condition)
      {up::kModRuleNullTable, kInv, Always, Nothing, [](M m) { m.d.section_offset = nullptr; }},
      {up::kModRuleNullTable, kInv, HasStreams, Nothing, [](M m) { m.d.streams = nullptr; }},
      {up::kModRuleNullTable, kInv, Always, Nothing, [](M m) { m.tree_ptr[m.t] = nullptr; }},
      {up::kModRuleNullTable, kInv, Always, Nothing, [](M m) { m.codes[m.t].uint_cfg = nullptr; }},
      {up::kModRuleNullTable, kInv, [](C m) { return !m.codes[m.t].use_prefix; }, Nothing, [](M m) { m.codes[m.t].alias = nullptr; }},
      {up::kModRuleNullTable, kInv, [](C m) { return m.codes[m.t].use_prefix != 0; }, Nothing, [](M m) { m.codes[m.t].prefix_offset = nullptr; }},
      {up::kModRuleSizeWrap, kInv, Always, Nothing, [](M m) { m.buffers[0].w = m.buffers[0].h = 0xFFFFFFFFu; }},
      {up::kModRuleSizeWrap, kInv, [](C m) { return m.codes[m.t].use_prefix != 0; }, Nothing, [](M m) { m.codes[m.t].prefix_table_size = 0xFFFFFFFFu; }},
      {up::kModRuleTreeProperty, kUns, Always, Nothing, [](M m) { m.trees[m.t][0].property = jxlhip::kModMaxProps; }},
      {up::kModRuleTreeChildren, kInv, [](C m) { return m.trees[m.t][0].property >= 0; }, Nothing, [](M m) { m.trees[m.t][0].lchild = 0; }},
      {up::kModRuleTreeLeaf, kInv, Always, Nothing, [](M m) { m.FirstLeaf().predictor = 14; }},
      {up::kModRuleCodeLimits, kInv, Always, Nothing, [](M m) { m.codes[m.t].num_clusters = 257; }},
      {up::kModRuleCtxMapEntries, kInv, [](C m) { return m.codes[m.t].num_clusters < 256; }, Nothing,
       [](M m) { m.ctx_map[m.t][0] = uint8_t(m.codes[m.t].num_clusters); }},
      {up::kModRulePrefixTables, kInv, [](C m) { return m.codes[m.t].use_prefix != 0; }, Nothing, [](M m) { m.codes[m.t].prefix_table_size = 0; }},
      {up::kModRuleLz77, kInv, [](C m) { return m.codes[m.t].lz77 != 0; }, Nothing, [](M m) { m.codes[m.t].lz_min_length = 0; }},
      {up::kModRuleRectInsideBuffer, kInv, [](C m) { return m.d.num_rects != 0; }, Nothing,
       [](M m) { m.rects[0].x0 = m.d.buffers[m.rects[0].buffer].w - m.rects[0].w + 1; }},
      {up::kModRuleStreamIndices, kInv, HasStreams, Nothing, [](M m) { m.streams[0].section = m.d.num_sections; }},
      {up::kModRuleStreamBitOffset, kInv, HasStreams, Nothing, [](M m) { m.streams[0].bit_offset = m.d.section_size[m.streams[0].section] * 8 + 1; }},
      {up::kModRuleStreamProps, kInv, HasStreams, Nothing, [](M m) { m.streams[0].num_props = 15; }},
      {up::kModRuleOpFields, kInv, [](C m) { return !m.ops.empty(); }, Nothing, [](M m) { m.ops[0].local = 2; }},
      {up::kModRuleOpBuffers, kInv, [](C m) { return !m.ops.empty(); }, Nothing, [](M m) { m.ops[0].buf[1] = m.d.num_buffers; }},
      {up::kModRuleOpRectangles, kInv, [](C m) { return m.FirstOp(0, 3) >= 0; }, Nothing,
       [](M m) {  // (one column outside; not the palette itself, which is a whole buffer)
         JxlHipModOp& op = m.ops[m.FirstOp(0, 3)];
         op.ox[1] = m.d.buffers[op.buf[1]].w + 1;
       }},
      {up::kModRuleRctType, kInv, [](C m) { return m.FirstOp(0, 0) >= 0; }, Nothing, [](M m) { m.ops[m.FirstOp(0, 0)].param = 42; }},
      {up::kModRulePaletteShape, kInv, [](C m) { return m.FirstOp(1, 1) >= 0; }, Nothing, [](M m) { m.ops[m.FirstOp(1, 1)].nb = 0; }},
      {up::kModRuleUnsqueezeAlias, kInv, [](C m) { return m.FirstOp(2, 3) >= 0; }, Nothing,
       [](M m) {  // the averages read from the output's own buffer, at the output's origin (where they fit)
         JxlHipModOp& op = m.ops[m.FirstOp(2, 3)];
         op.buf[0] = op.buf[2];
         op.ox[0] = op.ox[2];
         op.oy[0] = op.oy[2];
       }},
      {up::kModRuleOutBuffers, kInv, Always, Nothing, [](M m) { m.d.out_buffer[0] = m.d.num_buffers; }},
      {up::kModRuleSampleDepth, kInv, Always, Nothing, [](M m) { m.d.bits = 0; }},
      {up::kModRuleSplinesGrey, kUns, Colour, [](M m) { m.AddSplines(); }, [](M m) { m.d.num_color = 1; }},
      {up::kModRuleXybGrey, kUns, [](C m) { return Colour(m) && !m.d.splines.num_segments; }, [](M m) { m.d.xyb = 1; }, [](M m) { m.d.num_color = 1; }},
      // (the target is filled in beside the descriptor; the one change hands it over)
      {up::kModRuleColorTarget, kInv, [](C m) { return !m.d.color_target; }, [](M m) { m.ct.tone = JXLHIP_TONE_HLG_OOTF + 1; },
       [](M m) { m.d.color_target = &m.ct; }},
      {up::kModRuleColorTargetLinear, kInv, [](C m) { return !m.d.color_target && (!m.d.xyb || m.d.linear_output != 1); },
       [](M m) { m.ct.tf = JXLHIP_TF_GAMMA; }, [](M m) { m.d.color_target = &m.ct; }},
      {up::kModRuleSplineTables, kInv, Colour, [](M m) { m.AddSplines(); }, [](M m) { m.d.splines.segments = nullptr; }},
      {up::kModRuleSplineRows, kInv, Colour, [](M m) { m.AddSplines(); }, [](M m) { m.one[0] = 1; }},
      {up::kModRulePatchAlpha, kUns, Colour, [](M m) { m.AddPatches(); }, [](M m) { m.d.patches.uses_alpha = 1; }},
      {up::kModRulePatchTables, kInv, Colour, [](M m) { m.AddPatches(); }, [](M m) { m.d.patches.records = nullptr; }},
      {up::kModRulePatchRows, kInv, Colour, [](M m) { m.AddPatches(); }, [](M m) { m.rows[1] = 0; }},
      {up::kModRulePatchRecords, kInv, Colour, [](M m) { m.AddPatches(); }, [](M m) { m.record[6] = 4; }},
      // (a grey frame: the option alone; a colour one that keeps its planes: losing two channels)
      {up::kModRuleFloatPlanesGrey, kUns, [](C m) { return !Colour(m) || (!m.d.xyb && !m.d.splines.num_segments); },
       [](M m) { m.o.keep_xyb = Colour(m); },
       [](M m) {
         if (Colour(m)) m.d.num_color = 1;
         else m.o.keep_xyb = true;
       }},
  };
}

static int CheckRefusals(const JxlHipModFrameDesc& d, std::vector<bool>* exercised) {
  const std::vector<Row> rows = Rows();
  std::vector<int> have(up::kNumModRules, 0);
  for (const Row& r : rows) have[r.rule]++;
  for (int i = 0; i < up::kNumModRules; i++) EXPECT(have[i] >= 1, "rule %s has no row", kRuleNames[i]);
  up::ModRule rule = up::kNumModRules;
  {
    Mut m(d);
    EXPECT(up::CheckModFrameDesc(m.d, m.o, &rule) == 0, "the descriptor as parsed is refused by %s", kRuleNames[rule]);
  }
  for (const Row& r : rows) {
    Mut m(d);
    if (!r.applies(m)) continue;
    r.setup(m);
    rule = up::kNumModRules;
    EXPECT(up::CheckModFrameDesc(m.d, m.o, &rule) == 0, "%s: the set-up is refused by %s", kRuleNames[r.rule], kRuleNames[rule]);
    r.mutate(m);
    const int code = up::CheckModFrameDesc(m.d, m.o, &rule);
    EXPECT(code == r.code && rule == r.rule, "%s: code %d (want %d) from rule %s", kRuleNames[r.rule], code, r.code,
           rule < up::kNumModRules ? kRuleNames[rule] : "none");
    (*exercised)[r.rule] = true;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------------- the layout
// Half-open byte ranges that must not overlap.
struct Range {
  uint64_t lo, hi;
};
static bool Disjoint(std::vector<Range> r) {
  std::sort(r.begin(), r.end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
  for (size_t i = 1; i < r.size(); i++)
    if (r[i].lo < r[i - 1].hi) return false;
  return true;
}
static uint64_t A(const void* p) { return uint64_t(reinterpret_cast<uintptr_t>(p)); }

static int CheckTables(const JxlHipModFrameDesc& d) {
  const up::ModPlan P = up::MakeModPlan(d, up::ModUploadOptions());
  up::ModBases b;  // 64 GiB apart: no extent of one region reaches the next
  b.pool = uint64_t(1) << 36;
  b.sections = uint64_t(2) << 36;
  b.blob = uint64_t(3) << 36;
  b.rects = uint64_t(4) << 36;
  b.scratch = uint64_t(5) << 36;
  b.windows = uint64_t(6) << 36;
  b.status = uint64_t(7) << 36;
  b.end_bits = uint64_t(8) << 36;
  EXPECT(P.float_planes == (d.splines.num_segments || d.patches.num_positions), "float planes");

  // ---- channel pool
  EXPECT(P.buf_off.size() == d.num_buffers, "buf_off");
  uint64_t pool_end = 0;
  for (uint32_t i = 0; i < d.num_buffers; i++) {
    EXPECT(P.buf_off[i] % 4 == 0 && P.buf_off[i] >= pool_end, "buffer %u at %zu, the one before ends at %llu", i, P.buf_off[i], (unsigned long long)pool_end);
    pool_end = P.buf_off[i] + uint64_t(d.buffers[i].w) * d.buffers[i].h;
  }
  EXPECT(P.pool_ints >= pool_end, "pool of %zu ints, buffers end at %llu", P.pool_ints, (unsigned long long)pool_end);

  // ---- sections (into a block of exactly the planned size, so that a short plan is a sanitizer report)
  std::vector<uint8_t> packed(P.section_bytes, 0xEE);
  up::PackModSections(d, P, packed.data());
  {
    std::vector<uint8_t> covered(P.section_bytes, 0);
    uint64_t prev_end = 0;
    for (uint32_t i = 0; i < d.num_sections; i++) {
      const size_t at = P.sec_off[i];
      EXPECT(at % 4 == 0 && at >= prev_end + (i ? 8 : 0) && at + d.section_size[i] + 8 <= P.section_bytes, "section %u at %zu", i, at);
      EXPECT(memcmp(packed.data() + at, d.codestream + d.section_offset[i], d.section_size[i]) == 0, "section %u bytes", i);
      for (size_t k = 0; k < d.section_size[i]; k++) covered[at + k] = 1;
      prev_end = at + d.section_size[i];
    }
    for (size_t k = 0; k < covered.size(); k++) EXPECT(covered[k] || packed[k] == 0, "byte %zu between the sections is %d", k, packed[k]);
  }

  // ---- blob: trees, the parts of the codes, the code array
  std::vector<uint8_t> blob(P.blob_bytes, 0xEE);
  up::BuildModBlob(d, P, blob.data(), b.blob);
  std::vector<Range> items;
  auto item = [&](size_t at, size_t bytes) {
    if (bytes) items.push_back({at, at + bytes});
    return at % 16 == 0 && at + bytes <= P.blob_bytes;
  };
  EXPECT(item(P.codes_at, size_t(d.num_codes) * sizeof(jxlhip::ModCode)), "code array at %zu", P.codes_at);
  const jxlhip::ModCode* mcodes = reinterpret_cast<const jxlhip::ModCode*>(blob.data() + P.codes_at);
  for (uint32_t i = 0; i < d.num_trees; i++) {
    EXPECT(item(P.tree_at[i], size_t(d.tree_size[i]) * 16), "tree %u at %zu", i, P.tree_at[i]);
    const JxlHipModCode& k = d.codes[i];
    const jxlhip::ModCode& mc = mcodes[i];
    if (!d.tree_size[i]) {
      EXPECT(mc.table_words == 0 && P.table_words[i] == 0, "absent code %u", i);
      continue;
    }
    const jxlhip::ModTreeNode* t = reinterpret_cast<const jxlhip::ModTreeNode*>(blob.data() + P.tree_at[i]);
    for (uint32_t n = 0; n < d.tree_size[i]; n++) {
      const JxlHipModTreeNode& nd = d.trees[i][n];
      if (nd.property >= 0)
        EXPECT(t[n].property == nd.property && t[n].splitval == nd.splitval && t[n].lchild == nd.lchild && t[n].rchild == nd.rchild, "tree %u node %u", i, n);
      else
        EXPECT(t[n].property == -1 - int32_t(nd.predictor) && t[n].splitval == nd.offset && t[n].lchild == k.ctx_map[nd.lchild] &&
                   t[n].rchild == nd.multiplier,
               "tree %u leaf %u", i, n);
    }
    // every pointer of the code: inside the blob with its full extent, the descriptor's bytes behind it
    const size_t slots = k.use_prefix ? 0 : size_t(k.num_clusters) << k.log_alpha;
    const struct {
      const void* dev;
      const void* src;
      size_t bytes;
    } parts[5] = {{mc.ctx_map, k.ctx_map, k.ctx_map_size},
                  {mc.alias, k.alias, slots * 8},
                  {mc.cfg, k.uint_cfg, size_t(k.num_clusters) * 4},
                  {mc.prefix_table, k.prefix_table, k.use_prefix ? size_t(k.prefix_table_size) * 4 : 0},
                  {mc.prefix_offset, k.prefix_offset, k.use_prefix ? size_t(k.num_clusters) * 4 : 0}};
    for (int j = 0; j < 5; j++) {
      const uint64_t at = A(parts[j].dev) - b.blob;
      EXPECT(A(parts[j].dev) >= b.blob && item(at, parts[j].bytes), "code %u part %d at %llu", i, j, (unsigned long long)at);
      EXPECT(!parts[j].bytes || memcmp(blob.data() + at, parts[j].src, parts[j].bytes) == 0, "code %u part %d bytes", i, j);
    }
    EXPECT(mc.log_alpha == k.log_alpha && mc.use_prefix == k.use_prefix && mc.lz77 == k.lz77 && mc.lz_min_symbol == k.lz_min_symbol &&
               mc.lz_min_length == k.lz_min_length && mc.lz_len_cfg == k.lz_len_cfg && mc.lz_dist_ctx == k.lz_dist_ctx && mc.num_clusters == k.num_clusters,
           "code %u fields", i);
    // (what a wave stages in LDS: the symbol table, a config word per cluster, for prefix codes an offset word too)
    const uint64_t words = k.use_prefix ? uint64_t(k.prefix_table_size) + 2 * k.num_clusters : slots * 2 + k.num_clusters;
    EXPECT(mc.table_words == words && P.table_words[i] == words, "code %u: %u table words, read %llu", i, mc.table_words, (unsigned long long)words);
  }
  EXPECT(Disjoint(items), "blob items overlap");

  // ---- channels: each rectangle inside its buffer of the pool
  const size_t nrects = up::ModChannelEntries(d);
  std::vector<jxlhip::ModChannel> rects(nrects);
  memset(rects.data(), 0xEE, nrects * sizeof(jxlhip::ModChannel));
  up::BuildModChannels(d, P, rects.data(), b.pool);
  for (uint32_t i = 0; i < d.num_rects; i++) {
    const JxlHipModRect& q = d.rects[i];
    const jxlhip::ModChannel& c = rects[i];
    const uint64_t buf_lo = b.pool + 4 * uint64_t(P.buf_off[q.buffer]), buf_hi = buf_lo + 4 * uint64_t(d.buffers[q.buffer].w) * d.buffers[q.buffer].h;
    EXPECT(c.stride == d.buffers[q.buffer].w && c.w == q.w && c.h == q.h && c.sig == q.sig, "rect %u fields", i);
    EXPECT(A(c.data) == buf_lo + 4 * (uint64_t(q.y0) * c.stride + q.x0), "rect %u origin", i);
    const uint64_t last = q.w && q.h ? A(c.data) + 4 * (uint64_t(q.h - 1) * c.stride + q.w) : A(c.data);
    EXPECT(A(c.data) >= buf_lo && last <= buf_hi, "rect %u leaves its buffer", i);
  }

  // ---- streams
  std::vector<jxlhip::ModStream> streams(d.num_streams ? d.num_streams : 1);
  up::BuildModStreams(d, P, streams.data(), b);
  std::vector<Range> scratch, windows;
  for (uint32_t i = 0; i < d.num_streams; i++) {
    const JxlHipModStream& q = d.streams[i];
    const jxlhip::ModStream& s = streams[i];
    EXPECT(A(s.words) == b.sections + P.sec_off[q.section] && s.size_bytes == d.section_size[q.section] && s.bit_offset == q.bit_offset, "stream %u section", i);
    EXPECT(A(s.tree) == b.blob + P.tree_at[q.tree] && s.tree_nodes == d.tree_size[q.tree] && P.tree_at[q.tree] + size_t(s.tree_nodes) * 16 <= P.blob_bytes,
           "stream %u tree", i);
    EXPECT(A(s.code) == b.blob + P.codes_at + uint64_t(q.code) * sizeof(jxlhip::ModCode) && q.code < d.num_codes, "stream %u code", i);
    EXPECT(A(s.channels) == b.rects + uint64_t(q.first_rect) * sizeof(jxlhip::ModChannel) && s.num_channels == q.num_rects &&
               uint64_t(q.first_rect) + q.num_rects <= nrects,
           "stream %u channels", i);
    EXPECT(s.stream_id == q.stream_id && s.first_channel_index == q.first_channel_index && memcmp(s.wp, q.wp, sizeof(s.wp)) == 0 &&
               s.uses_wp == q.uses_wp && s.num_props == q.num_props && s.dist_multiplier == q.dist_multiplier,
           "stream %u fields", i);
    EXPECT(A(s.status) == b.status + 4 * uint64_t(i) && A(s.end_bit) == b.end_bits + 4 * uint64_t(i), "stream %u status words", i);
    EXPECT((s.wp_scratch != nullptr) == (q.uses_wp != 0), "stream %u scratch", i);
    if (q.uses_wp) {  // two rows of max_width + 2 entries of kModWpEntry ints
      const uint64_t lo = A(s.wp_scratch), hi = lo + 4 * (uint64_t(q.max_width) + 2) * 2 * jxlhip::kModWpEntry;
      EXPECT(lo >= b.scratch && lo % 16 == 0 && hi <= b.scratch + 4 * uint64_t(P.scratch_ints), "stream %u scratch extent", i);
      scratch.push_back({lo, hi});
    }
    const bool lz = d.codes[q.code].lz77 != 0;
    EXPECT((s.lz_window != nullptr) == lz && (lz || s.lz_window_mask == 0), "stream %u window", i);
    if (lz) {
      const uint64_t w = uint64_t(s.lz_window_mask) + 1, lo = A(s.lz_window), hi = lo + 4 * w;
      EXPECT((w & (w - 1)) == 0 && w >= 256 && w <= (1u << 20), "stream %u: window of %llu words", i, (unsigned long long)w);
      EXPECT(w >= std::min<uint64_t>(q.num_samples, 1u << 20) && (w == 256 || w / 2 < q.num_samples), "stream %u: window of %llu words for %u samples", i,
             (unsigned long long)w, q.num_samples);
      EXPECT(lo >= b.windows && hi <= b.windows + 4 * uint64_t(P.window_words), "stream %u window extent", i);
      windows.push_back({lo, hi});
    }
  }
  EXPECT(Disjoint(scratch) && Disjoint(windows), "scratch regions or windows overlap");
  return 0;
}

// ----------------------------------------------------------------------------------------------------- the schedule
static int CheckSchedule(const JxlHipModFrameDesc& d) {
  const up::ModPlan P = up::MakeModPlan(d, up::ModUploadOptions());
  const uint64_t pool = uint64_t(1) << 36;
  std::vector<uint32_t> buf_w(d.num_buffers);
  for (uint32_t i = 0; i < d.num_buffers; i++) buf_w[i] = d.buffers[i].w;
  const up::ModFrameOps frame = {uintptr_t(pool), P.buf_off.data(), buf_w.data(), d.ops, d.num_ops};
  std::vector<uint8_t> blob;
  std::vector<up::ModLaunch> launches;
  up::BuildModSchedule(&frame, 1, &blob, &launches);
  // where buffer j of an operation starts, and whether a w x h rectangle of samples `step` apart and rows `line` apart,
  // starting at `addr`, stays inside that buffer
  auto origin = [&](const JxlHipModOp& op, uint32_t j) {
    return pool + 4 * (uint64_t(P.buf_off[op.buf[j]]) + uint64_t(op.oy[j]) * buf_w[op.buf[j]] + op.ox[j]);
  };
  auto inside = [&](const JxlHipModOp& op, uint32_t j, uint64_t addr, uint64_t w, uint64_t step, uint64_t h, uint64_t line) {
    const uint64_t lo = pool + 4 * uint64_t(P.buf_off[op.buf[j]]), hi = lo + 4 * uint64_t(d.buffers[op.buf[j]].w) * d.buffers[op.buf[j]].h;
    return addr >= lo && (!w || !h || addr + 4 * ((w - 1) * step + (h - 1) * line) < hi);
  };
  // whether the block at `at` is the one operation `op` asks for: every address, stride and count, read from the
  // operation's documentation (include/jxl_amd_hip.h) and the kernels' (jxl_hip_modular.h)
  auto matches = [&](const JxlHipModOp& op, const uint8_t* at) {
    if (op.kind == 0) {
      jxlhip::ModRct p;
      memcpy(&p, at, sizeof(p));
      for (uint32_t j = 0; j < 3; j++)
        if (A(p.c[j]) != origin(op, j) || p.stride[j] != buf_w[op.buf[j]] || !inside(op, j, A(p.c[j]), p.w, 1, p.h, p.stride[j])) return false;
      return p.w == op.w && p.h == op.h && p.type == op.param;
    }
    if (op.kind == 1) {
      jxlhip::ModPalette p;
      memcpy(&p, at, sizeof(p));
      if (A(p.palette) != pool + 4 * uint64_t(P.buf_off[op.buf[0]]) || p.palette_w != buf_w[op.buf[0]] || p.nb != op.nb || p.nb < 1 || p.nb > 4 ||
          !inside(op, 0, A(p.palette), p.palette_w, 1, p.nb, p.palette_w))
        return false;
      if (A(p.index) != origin(op, 1) || p.index_stride != buf_w[op.buf[1]] || !inside(op, 1, A(p.index), p.w, 1, p.h, p.index_stride)) return false;
      for (uint32_t j = 0; j < 4; j++) {
        if (j >= p.nb && (p.out[j] || p.out_stride[j])) return false;
        if (j < p.nb && (A(p.out[j]) != origin(op, 2 + j) || p.out_stride[j] != buf_w[op.buf[2 + j]] ||
                         !inside(op, 2 + j, A(p.out[j]), p.w, 1, p.h, p.out_stride[j])))
          return false;
      }
      return p.w == op.w && p.h == op.h && p.bit_depth == op.bit_depth;
    }
    jxlhip::ModUnsqueeze p;  // a line is a row of the output (horizontal) or a column (vertical): (n + 1) / 2 averages, n / 2 residuals
    memcpy(&p, at, sizeof(p));
    const bool hz = op.kind == 2;
    const uint32_t n = hz ? op.w : op.h, lines = hz ? op.h : op.w;
    const uint32_t wa = buf_w[op.buf[0]], wr = buf_w[op.buf[1]], wo = buf_w[op.buf[2]];
    if (p.lines != lines || p.na != (n + 1) / 2 || p.nr != n / 2) return false;
    if (A(p.avg) != origin(op, 0) || A(p.res) != origin(op, 1) || A(p.out) != origin(op, 2)) return false;
    if (p.avg_line != (hz ? wa : 1) || p.avg_step != (hz ? 1 : wa) || p.res_line != (hz ? wr : 1) || p.res_step != (hz ? 1 : wr) ||
        p.out_line != (hz ? wo : 1) || p.out_step != (hz ? 1 : wo))
      return false;
    return inside(op, 0, A(p.avg), p.na, p.avg_step, p.lines, p.avg_line) && inside(op, 1, A(p.res), p.nr, p.res_step, p.lines, p.res_line) &&
           inside(op, 2, A(p.out), n, p.out_step, p.lines, p.out_line);
  };
  std::vector<int> launch_of(d.num_ops, -1);
  for (size_t li = 0; li < launches.size(); li++) {
    const up::ModLaunch& L = launches[li];
    EXPECT(L.kind <= 2 && L.count && L.offset % 16 == 0, "launch %zu", li);
    const size_t block = L.kind == 0 ? sizeof(jxlhip::ModRct) : (L.kind == 1 ? sizeof(jxlhip::ModPalette) : sizeof(jxlhip::ModUnsqueeze));
    EXPECT(L.offset + size_t(L.count) * block <= blob.size(), "launch %zu leaves the blob", li);
    uint32_t need_gx = 0, need_gy = 1;
    for (uint32_t z = 0; z < L.count; z++) {
      int found = -1;
      for (uint32_t k = 0; k < d.num_ops && found < 0; k++) {
        const JxlHipModOp& op = d.ops[k];
        if (launch_of[k] < 0 && op.w && op.h && (op.kind >= 2 ? 2u : op.kind) == L.kind && matches(op, blob.data() + L.offset + size_t(z) * block)) found = int(k);
      }
      EXPECT(found >= 0, "launch %zu block %u is no operation's", li, z);
      launch_of[found] = int(li);
      // the kernels: 256 columns per workgroup and a workgroup row per sample row; the unsqueeze 64 lines per workgroup
      const JxlHipModOp& op = d.ops[found];
      need_gx = std::max(need_gx, L.kind == 2 ? ((op.kind == 2 ? op.h : op.w) + 63) / 64 : (op.w + 255) / 256);
      if (L.kind != 2) need_gy = std::max(need_gy, op.h);
    }
    EXPECT(L.gx >= need_gx && L.gy >= need_gy, "launch %zu: grid %u x %u, its largest block needs %u x %u", li, L.gx, L.gy, need_gx, need_gy);
  }
  // every non-empty operation once; a launch holds one phase, level and kind; launches local first, then by level, then by kind
  struct Key {
    uint32_t phase, level, kind;
    bool operator<(const Key& o) const { return phase != o.phase ? phase < o.phase : (level != o.level ? level < o.level : kind < o.kind); }
  };
  std::vector<Key> key(launches.size(), Key{9, 0, 0});
  for (uint32_t k = 0; k < d.num_ops; k++) {
    const JxlHipModOp& op = d.ops[k];
    if (!op.w || !op.h) continue;
    EXPECT(launch_of[k] >= 0, "operation %u is in no launch", k);
    const Key mine = {op.local ? 0u : 1u, op.level, op.kind >= 2 ? 2u : op.kind};
    Key& have = key[launch_of[k]];
    if (have.phase == 9) have = mine;
    EXPECT(!(have < mine) && !(mine < have), "operation %u (phase %u level %u kind %u) shares a launch with phase %u level %u kind %u", k, mine.phase,
           mine.level, mine.kind, have.phase, have.level, have.kind);
  }
  for (size_t li = 1; li < launches.size(); li++) EXPECT(key[li - 1] < key[li], "launch %zu is not behind launch %zu", li, li - 1);
  return 0;
}

// ------------------------------------------------------------------------------------------------------- the double
struct Kats {
  int result = -1;
  std::vector<bool> exercised = std::vector<bool>(up::kNumModRules, false);
};
extern "C" int jxlhip_modular_upload(JxlHipContext* ctx, const JxlHipModFrameDesc* d) {
  Kats* k = reinterpret_cast<Kats*>(ctx);
  k->result = CheckRefusals(*d, &k->exercised);
  if (!k->result) k->result = CheckTables(*d);
  if (!k->result) k->result = CheckSchedule(*d);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const bool second = argc >= 3 && std::string(argv[2]) == "second";
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> data;
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + n);
  fclose(f);
  JxlAmdModFrame* frame = nullptr;
  int r = jxlamd_modframe_parse(data.data(), data.size(), &frame);
  float plane[1];
  if (!r && second) {  // the first frame is what the second one's patches read: only its size matters here
    uint32_t info[16];
    jxlamd_modframe_info(frame, info);
    const size_t end = jxlamd_modframe_end(frame, nullptr);
    jxlamd_modframe_free(frame);
    frame = nullptr;
    r = jxlamd_modframe_parse_at(data.data(), data.size(), end, 1, &frame);
    const float* planes[4] = {plane, plane, plane, plane};
    const uint32_t xs[4] = {info[0], info[0], info[0], info[0]}, ys[4] = {info[1], info[1], info[1], info[1]};
    if (!r) r = jxlamd_modframe_set_patch_sources(frame, planes, xs, ys);
  }
  if (r || !frame) {
    fprintf(stderr, "FAIL: %s does not parse (%s)\n", argv[1], jxlamd_last_error());
    return 1;
  }
  Kats k;
  r = jxlamd_modframe_upload(frame, reinterpret_cast<JxlHipContext*>(&k));
  jxlamd_modframe_free(frame);
  if (r || k.result) {
    fprintf(stderr, "FAIL: upload %d, checks %d\n", r, k.result);
    return 1;
  }
  printf("exercised:");
  for (int i = 0; i < up::kNumModRules; i++)
    if (k.exercised[i]) printf(" %s", kRuleNames[i]);
  printf("\n");
  return 0;
}
