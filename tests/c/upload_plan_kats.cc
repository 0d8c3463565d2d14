// What jxlhip_frame_upload computes on the host (libjxl_amd/csrc/host/jxh_upload_plan.h), held on the CPU over the
// descriptors of real streams. Built by tests/test_kats.py with -fsanitize=address,undefined around
// libjxl_amd/csrc/api/jxl_api.cc like api_fuzz.cc; the HIP entry points are no-device doubles, except jxlhip_frame_upload:
// this program's double receives the descriptor jxlamd_frame_upload_band built and runs the checks below on it.
//   refusals     the descriptor is accepted as parsed; for every rule of CheckFrameDesc a copy in which one field, table
//                entry or pointer breaks that rule and nothing else is refused by that rule, with its code
//   block_recs   every field of every word against a reading written here from the layout and ac_context.h's rule
//   alias_packed every entry unpacked by the documented layout against the descriptor's alias entry and uint config
//   work lists   every in-band varblock once, under its own strategy; trecs agree with tlist; padding zero
//   sections     16-byte aligned, the codestream's bytes, gaps and tail zero; selectors read bit by bit
//   dequant_scan entry k = dequant[order[k]] for every kind in use, zero elsewhere
//   table list   placing (into a block of exactly the bound, so that a short bound is a sanitizer report) consumes no
//                more than the bound computed from the same list
// usage: upload_plan_kats whole|band B0 B1|partial|partial_late file       prints "exercised: <rules>" for the caller to add up
#include "../../libjxl_amd/csrc/api/jxl_api.cc"
#define KATS_OWN_FRAME_UPLOAD
#include "no_device_doubles.inc"
#include "../../libjxl_amd/csrc/host/jxh_upload_plan.h"

#include <functional>
#include <map>

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
    "Sizes", "CoefBits", "ChromaShift", "WholeMcus", "SubsampledFrame", "SubsampledHaloBand", "GroupCounts", "BlockCtxCounts", "Upsampling",
    "BandRows", "AbsentGroupSections", "PartialPassOrder", "GroupBlockRanges", "VarblockFields", "VarblockInsideGroup", "VarblockCoefOffset",
    "SubsampledOneBlock", "SubsampledRaster", "PassLimits", "PrefixTables", "Lz77", "CtxMapSize", "CtxMapEntries", "UintConfig", "DcSource",
    "Sharpness", "DcStep", "QuantScale", "LinearOutput", "ColorTarget", "ColorTargetLinear", "SplineTables", "SplineRows", "PatchTables",
    "PatchRows", "PatchRecords", "PatchAlphaUpsampled", "AlphaCapacity", "BlockCtxLutSize", "DequantExtents", "OrdersInBucket"};
static_assert(sizeof(kRuleNames) / sizeof(kRuleNames[0]) == up::kNumRules, "a name for every rule of jxh_upload_plan.h");

// A descriptor with copies of the arrays the mutations write to, and room for the spline / patch tables some rows add.
struct Mut {
  JxlHipFrameDesc d;
  up::UploadOptions o;
  std::vector<JxlHipVarBlock> blocks;
  std::vector<uint32_t> gbb, section_size;
  std::vector<uint8_t> group_absent;
  std::vector<JxlHipPassDesc> passes;
  std::vector<std::vector<uint8_t>> ctx_map;
  std::vector<std::vector<uint32_t>> uint_cfg;
  std::vector<std::vector<uint16_t>> orders;
  JxlHipColorTarget ct;
  std::vector<uint32_t> rows, one, record;
  float segment[8], plane[1];
  explicit Mut(const JxlHipFrameDesc& src) : d(src) {
    const size_t nsec = size_t(d.num_groups) * d.num_passes;
    blocks.assign(d.blocks, d.blocks + d.num_blocks);
    gbb.assign(d.group_block_begin, d.group_block_begin + d.num_groups + 1);
    section_size.assign(d.section_size, d.section_size + nsec);
    if (d.group_absent) group_absent.assign(d.group_absent, d.group_absent + d.num_groups);
    passes.assign(d.passes, d.passes + d.num_passes);
    ctx_map.resize(d.num_passes);
    uint_cfg.resize(d.num_passes);
    for (uint32_t p = 0; p < d.num_passes; p++) {
      ctx_map[p].assign(passes[p].ctx_map, passes[p].ctx_map + passes[p].ctx_map_size);
      uint_cfg[p].assign(passes[p].uint_cfg, passes[p].uint_cfg + passes[p].num_clusters);
      passes[p].ctx_map = ctx_map[p].data();
      passes[p].uint_cfg = uint_cfg[p].data();
    }
    d.blocks = blocks.data();
    d.group_block_begin = gbb.data();
    d.section_size = section_size.data();
    if (d.group_absent) d.group_absent = group_absent.data();
    d.passes = passes.data();
    memset(&ct, 0, sizeof(ct));
    // one spline segment / one patch of one pixel, drawn in row 0
    rows.assign(size_t(d.ysize) + 1, 1);
    rows[0] = 0;
    one.assign(1, 0);
    record = {0, 0, 1, 1, 0, 0, 0, 1};
    memset(segment, 0, sizeof(segment));
  }
  void OwnOrders() {  // (megabytes for a frame with the largest transforms: copied for the one row that writes to them)
    orders.resize(d.num_passes);
    for (uint32_t p = 0; p < d.num_passes; p++) {
      orders[p].assign(passes[p].orders, passes[p].orders + passes[p].orders_size);
      passes[p].orders = orders[p].data();
    }
  }
  void AddSplines() {
    d.splines.num_segments = d.splines.num_row_segments = 1;
    d.splines.segments = segment;
    d.splines.row_start = rows.data();
    d.splines.row_segments = one.data();
  }
  void AddPatches(bool alpha) {
    d.patches.num_positions = d.patches.num_row_entries = 1;
    d.patches.records = record.data();
    d.patches.row_start = rows.data();
    d.patches.row_list = one.data();
    d.patches.slot_planes[0] = plane;  // (a device address to the upload: never read on the host)
    d.patches.slot_w[0] = d.patches.slot_h[0] = 1;
    if (alpha) {
      d.patches.uses_alpha = 1;
      d.patches.slot_alpha[0] = plane;
    }
  }
  uint32_t FirstInBand() const {  // a varblock the context transforms
    const up::Geometry g = up::MakeGeometry(d, o);
    for (uint32_t i = 0; i < d.num_blocks; i++)
      if (up::InBand(d.blocks[i], g)) return i;
    return 0;
  }
};

// One row per rule: when the stream can reach it, a set-up that the checks still take (tables the stream does not have),
// and the one change that breaks the rule.
struct Row {
  up::Rule rule;
  int code;
  std::function<bool(const Mut&)> applies;
  std::function<void(Mut&)> setup;
  std::function<void(Mut&)> mutate;
};
static bool Always(const Mut&) { return true; }
static void Nothing(Mut&) {}
static bool Subsampled(const Mut& m) { return up::ChromaShifts(m.d) != 0; }
static bool Banded(const Mut& m) { return (m.d.band_group_row_begin | m.d.band_group_row_end) != 0; }
static const int kInv = JXLHIP_ERR_INVALID_ARGUMENT, kUns = JXLHIP_ERR_UNSUPPORTED;

static std::vector<Row> Rows() {
  using M = Mut&;
  using C = const Mut&;
  return {
      {up::kRuleSizes, kInv, Always, Nothing, [](M m) { m.d.num_passes = 12; }},
      {up::kRuleCoefBits, kInv, Always, Nothing, [](M m) { m.d.coef_bits = 24; }},
      {up::kRuleChromaShift, kInv, Always, Nothing, [](M m) { m.d.chroma_hshift[0] = 2; }},
      {up::kRuleWholeMcus, kInv, Always, Nothing, [](M m) { m.d.xsize_blocks += 1; }},
      {up::kRuleSubsampledFrame, kInv, Subsampled, Nothing, [](M m) { m.d.dc_smoothing = 1; }},
      {up::kRuleSubsampledHaloBand, kUns, [](C m) { return Subsampled(m) && !Banded(m); }, [](M m) { m.o.band_halo = true; },
       [](M m) { m.d.band_group_row_end = 1; }},
      {up::kRuleGroupCounts, kInv, Always, Nothing, [](M m) { m.d.xsize_groups += 1; }},
      {up::kRuleBlockCtxCounts, kInv, Always, Nothing, [](M m) { m.d.num_dc_ctxs = 0; }},
      {up::kRuleUpsampling, kInv, Always, Nothing, [](M m) { m.d.upsampling = 3; }},
      {up::kRuleBandRows, kInv, Always, Nothing, [](M m) { m.d.band_group_row_end = m.d.num_groups / m.d.xsize_groups + 1; }},
      {up::kRuleAbsentGroupSections, kInv,
       [](C m) {  // a partial frame with a group that is there
         for (uint32_t g = 0; m.d.group_absent && g < m.d.num_groups; g++)
           if (!m.d.group_absent[g] && m.d.section_size[g]) return true;
         return false;
       },
       Nothing,
       [](M m) {
         for (uint32_t g = 0; g < m.d.num_groups; g++)
           if (!m.group_absent[g] && m.section_size[g]) {
             m.group_absent[g] = 1;
             return;
           }
       }},
      {up::kRulePartialPassOrder, kInv,
       [](C m) {  // a partial frame of three passes with a group that has all of them
         for (uint32_t g = 0; m.d.group_absent && m.d.num_passes >= 3 && g < m.d.num_groups; g++)
           if (!m.d.group_absent[g] && m.d.section_size[m.d.num_groups + g] && m.d.section_size[2 * m.d.num_groups + g]) return true;
         return false;
       },
       Nothing,
       [](M m) {
         for (uint32_t g = 0; g < m.d.num_groups; g++)
           if (!m.group_absent[g] && m.section_size[m.d.num_groups + g] && m.section_size[2 * m.d.num_groups + g]) {
             m.section_size[m.d.num_groups + g] = 0;
             return;
           }
       }},
      {up::kRuleGroupBlockRanges, kInv, Always, Nothing, [](M m) { m.gbb[m.d.num_groups] += 1; }},
      {up::kRuleVarblockFields, kInv, Always, Nothing, [](M m) { m.blocks[0].qf = 0; }},
      {up::kRuleVarblockInsideGroup, kInv, Always, Nothing, [](M m) { m.blocks[0].bx = uint16_t(m.d.xsize_blocks); }},
      {up::kRuleVarblockCoefOffset, kInv, Always, Nothing, [](M m) { m.blocks[0].coef_offset = 64; }},
      {up::kRuleSubsampledOneBlock, kInv, Subsampled, Nothing, [](M m) { m.blocks[0].strategy = 4; }},
      {up::kRuleSubsampledRaster, kInv, Subsampled, Nothing, [](M m) { m.blocks[0].bx = 1; }},
      {up::kRulePassLimits, kInv, Always, Nothing, [](M m) { m.passes[0].num_clusters = 257; }},
      {up::kRulePrefixTables, kInv, [](C m) { return m.d.passes[0].use_prefix != 0; }, Nothing, [](M m) { m.passes[0].prefix_table_size = 0; }},
      {up::kRuleLz77, kInv, [](C m) { return m.d.passes[0].lz77 != 0; }, Nothing, [](M m) { m.passes[0].lz_min_length = 0; }},
      {up::kRuleCtxMapSize, kInv, Always, Nothing, [](M m) { m.passes[0].ctx_map_size = 15; }},
      {up::kRuleCtxMapEntries, kInv, [](C m) { return m.d.passes[0].num_clusters < 256; }, Nothing,
       [](M m) { m.ctx_map[0][0] = uint8_t(m.passes[0].num_clusters); }},
      {up::kRuleUintConfig, kInv, Always, Nothing, [](M m) { m.uint_cfg[0][0] = 16; }},
      {up::kRuleDcSource, kInv, [](C m) { return !m.d.dc && !m.d.dc_device; }, Nothing, [](M m) { m.d.dc_quantised = nullptr; }},
      {up::kRuleSharpness, kInv, [](C m) { return up::DcRouteOf(m.d).sigma; }, Nothing, [](M m) { m.d.sharpness = nullptr; }},
      {up::kRuleDcStep, kInv, [](C m) { return up::DcRouteOf(m.d).dequant; }, Nothing, [](M m) { m.d.dc_step[1] = 0.0f; }},
      {up::kRuleQuantScale, kInv, [](C m) { return up::DcRouteOf(m.d).sigma; }, Nothing, [](M m) { m.d.quant_scale = 0.0f; }},
      {up::kRuleLinearOutput, kInv, [](C m) { return !Subsampled(m); }, Nothing, [](M m) { m.d.linear_output = 4; }},
      // (the target is filled in beside the descriptor; the one change hands it over)
      {up::kRuleColorTarget, kInv, [](C m) { return !m.d.color_target; }, [](M m) { m.ct.tone = JXLHIP_TONE_HLG_OOTF + 1; },
       [](M m) { m.d.color_target = &m.ct; }},
      {up::kRuleColorTargetLinear, kInv, [](C m) { return !m.d.color_target && m.d.linear_output != 1; }, [](M m) { m.ct.tf = JXLHIP_TF_GAMMA; },
       [](M m) { m.d.color_target = &m.ct; }},
      {up::kRuleSplineTables, kInv, Always, [](M m) { m.AddSplines(); }, [](M m) { m.d.splines.segments = nullptr; }},
      {up::kRuleSplineRows, kInv, Always, [](M m) { m.AddSplines(); }, [](M m) { m.one[0] = 1; }},
      {up::kRulePatchTables, kInv, Always, [](M m) { m.AddPatches(false); }, [](M m) { m.d.patches.records = nullptr; }},
      {up::kRulePatchRows, kInv, Always, [](M m) { m.AddPatches(false); }, [](M m) { m.rows[1] = 0; }},
      {up::kRulePatchRecords, kInv, Always, [](M m) { m.AddPatches(false); }, [](M m) { m.record[6] = 4; }},
      {up::kRulePatchAlphaUpsampled, kUns, [](C m) { return !Banded(m) && m.d.upsampling <= 1; },
       [](M m) {  // (everything an upsampled frame needs but the factor)
         m.AddPatches(true);
         m.d.upsampling_kernel = m.plane;
         m.d.out_xsize = 2 * m.d.xsize;
         m.d.out_ysize = 2 * m.d.ysize;
       },
       [](M m) { m.d.upsampling = 2; }},
      {up::kRuleAlphaCapacity, kInv, Always, Nothing, [](M m) { m.o.have_alpha = true; }},
      {up::kRuleBlockCtxLutSize, kInv, Always, Nothing, [](M m) { m.d.block_ctx_lut_size = 0; }},
      {up::kRuleDequantExtents, kInv, Always, Nothing,
       [](M m) { m.d.dequant_size[jxlhip::kStrategyQuantTable[m.blocks[m.FirstInBand()].strategy]] += 1; }},
      {up::kRuleOrdersInBucket, kInv, Always, Nothing,
       [](M m) {
         const uint32_t st = m.blocks[m.FirstInBand()].strategy;
         m.OwnOrders();
         m.orders[0][m.passes[0].order_offset[jxlhip::kStrategyOrder[st] * 3 + 1]] = uint16_t(m.d.dequant_size[jxlhip::kStrategyQuantTable[st]]);
       }},
  };
}
// Rules that no parsed stream reaches by one change (at most five; none at present).
static const std::vector<up::Rule> kUnreachable = {};

// Both halves of the upload's admission: the descriptor's checks, then (`orders`: the walk over every coefficient order
// is the slow half, and only its own row changes what it reads) the orders of every pass.
static int Admit(const Mut& m, bool orders, up::Rule* rule) {
  int r = up::CheckFrameDesc(m.d, m.o, rule);
  if (r || !orders) return r;
  uint32_t begin[27], count[27];
  up::CountWorkLists(m.d, up::MakeGeometry(m.d, m.o), begin, count);
  return up::CheckOrders(m.d, count, m.d.num_passes, rule);
}

static int CheckRefusals(const JxlHipFrameDesc& d, std::vector<bool>* exercised) {
  const std::vector<Row> rows = Rows();
  std::vector<int> have(up::kNumRules, 0);
  for (const Row& r : rows) have[r.rule]++;
  for (up::Rule u : kUnreachable) have[u]++;
  EXPECT(kUnreachable.size() <= 5, "%zu rules listed as unreachable", kUnreachable.size());
  for (int i = 0; i < up::kNumRules; i++) EXPECT(have[i] == 1, "rule %s has %d rows", kRuleNames[i], have[i]);
  EXPECT(rows.size() + kUnreachable.size() == size_t(up::kNumRules), "%zu rows for %d rules", rows.size(), int(up::kNumRules));
  up::Rule rule = up::kNumRules;
  {
    Mut m(d);
    EXPECT(Admit(m, true, &rule) == 0, "the descriptor as parsed is refused by %s", kRuleNames[rule]);
  }
  for (const Row& r : rows) {
    Mut m(d);
    if (!r.applies(m)) continue;
    r.setup(m);
    rule = up::kNumRules;
    const bool orders = r.rule == up::kRuleOrdersInBucket;
    EXPECT(Admit(m, orders, &rule) == 0, "%s: the set-up is refused by %s", kRuleNames[r.rule], kRuleNames[rule]);
    r.mutate(m);
    const int code = Admit(m, orders, &rule);
    EXPECT(code == r.code && rule == r.rule, "%s: code %d (want %d) from rule %s", kRuleNames[r.rule], code, r.code,
           rule < up::kNumRules ? kRuleNames[rule] : "none");
    (*exercised)[r.rule] = true;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------ the table list, placed
// The context's double: the members upload::VisitFrameTables names. A table is where it was placed in the block.
struct Tab {
  size_t at = 0, bytes = 0;
  bool placed = false;
};
struct PassTabs {
  Tab ctx_map, alias, alias_packed, cfg, orders, ptable, poffset;
};
struct Ctx {
  Tab sec_word, sections, sec_size, blocks, gbb, bctx_lut, dequant, dc_q, dc_ep, dc_raw, dc, sharp, inv_sigma, ytox, ytob, spl_seg, spl_row_start,
      spl_row_seg, pat_rec, pat_row_start, pat_row_list, ups_kernel, tlist, trecs, block_recs, dequant_scan;
  std::vector<PassTabs> pass_bufs;
};
struct Placer {  // only advances an offset; the bytes go to a block of exactly the bound
  std::vector<uint8_t>* block;
  size_t used = 0;
  bool overrun = false;
  void* place(Tab& t, size_t n) {
    t.at = used;
    t.bytes = n;
    t.placed = true;
    used += up::StagedBytes(n);
    if (used > block->size()) overrun = true;
    return overrun ? nullptr : block->data() + t.at;
  }
  void copy(Tab& t, size_t n, const void* src) {
    void* p = place(t, n);
    if (p && n) memcpy(p, src, n);
  }
  template <typename F>
  void build(Tab& t, size_t n, F&& fill) {
    void* p = place(t, n);
    if (p) fill(p);
  }
  void phase(const char*) {}
};

// n bits from bit `bit` of a section of `size` bytes, least significant first (a section that ends before them reads zeros)
static uint32_t BitsAt(const uint8_t* p, size_t size, size_t bit, uint32_t n) {
  uint32_t v = 0;
  for (uint32_t i = 0; i < n; i++)
    if ((bit + i) / 8 < size) v |= uint32_t((p[(bit + i) / 8] >> ((bit + i) % 8)) & 1) << i;
  return v;
}
static uint32_t Log2(uint32_t v) {
  uint32_t l = 0;
  while ((1u << l) < v) l++;
  return l;
}

static int CheckTables(const JxlHipFrameDesc& d, const up::UploadOptions& o) {
  up::Plan P = up::MakePlan(d, o);
  P.scan_order = d.num_passes == 1;  // (what the lane route of a single-pass frame asks for)
  const up::Geometry& g = P.g;
  Ctx c;
  c.pass_bufs.resize(d.num_passes);
  up::TableBound bound;
  up::VisitFrameTables(c, d, P, bound);
  std::vector<uint8_t> block(bound.bytes, 0xEE);
  Placer placer{&block};
  up::VisitFrameTables(c, d, P, placer);
  EXPECT(!placer.overrun && placer.used <= bound.bytes, "placing takes %zu bytes, the bound is %zu", placer.used, bound.bytes);
  const uint8_t* B = block.data();
  const size_t nsec = g.nsec;

  // ---- sections
  const uint32_t* sec_word = reinterpret_cast<const uint32_t*>(B + c.sec_word.at);
  const uint8_t* packed = B + c.sections.at;
  EXPECT(c.sec_word.bytes == nsec * 4 && c.sec_size.bytes == nsec * 4 && c.sections.bytes == P.section_bytes, "section table sizes");
  EXPECT(memcmp(B + c.sec_size.at, d.section_size, nsec * 4) == 0, "sec_size");
  std::vector<uint8_t> covered(c.sections.bytes, 0);
  size_t prev_end = 0;
  for (size_t i = 0; i < nsec; i++) {
    const size_t at = size_t(sec_word[i]) * 4;
    EXPECT(at % 16 == 0 && at >= prev_end && at + d.section_size[i] + 256 <= c.sections.bytes, "section %zu at %zu", i, at);
    EXPECT(memcmp(packed + at, d.codestream + d.section_offset[i], d.section_size[i]) == 0, "section %zu bytes", i);
    for (size_t k = 0; k < d.section_size[i]; k++) covered[at + k] = 1;
    prev_end = at + d.section_size[i];
  }
  for (size_t k = 0; k < covered.size(); k++) EXPECT(covered[k] || packed[k] == 0, "byte %zu between the sections is %d", k, packed[k]);
  EXPECT(c.sections.bytes - prev_end >= 256, "tail");
  std::vector<uint32_t> sel(nsec, 99);
  up::BuildSelectors(d, sel.data());
  const uint32_t hb = Log2(d.num_histograms);
  for (size_t i = 0; i < nsec; i++) {
    const size_t bit0 = i == 0 ? d.first_section_bit_offset : 0;
    const uint32_t want = BitsAt(d.codestream + d.section_offset[i], d.section_size[i], bit0, hb);
    EXPECT(sel[i] == want, "selector %zu: %u, read %u", i, sel[i], want);
  }

  // ---- block records: the layout's fields from a reading of ac_context.h written here
  const uint32_t* recs = reinterpret_cast<const uint32_t*>(B + c.block_recs.at);
  EXPECT(c.block_recs.bytes == (size_t(d.num_blocks) + 16) * 4, "block_recs size");
  std::vector<uint16_t> qf_at(g.nblk, 0);  // the raw quant field of the varblock whose top-left block is there
  for (uint32_t i = 0; i < d.num_blocks; i++) qf_at[size_t(d.blocks[i].by) * d.xsize_blocks + d.blocks[i].bx] = d.blocks[i].qf;
  const uint32_t nq = d.num_qf_thresholds + 1;
  for (uint32_t i = 0; i < d.num_blocks; i++) {
    const JxlHipVarBlock& v = d.blocks[i];
    const uint32_t w = recs[i], col = v.bx % 32, row = v.by % 32;
    EXPECT((w & 31) == col && ((w >> 5) & 1) == (row != 0), "block %u: position bits %x", i, w);
    EXPECT((1u << ((w >> 6) & 7)) == jxlhip::kCoveredX[v.strategy] && (1u << ((w >> 9) & 7)) == jxlhip::kCoveredY[v.strategy], "block %u: covered", i);
    for (uint32_t ch = 0; ch < 3; ch++) {
      const uint32_t hs = d.chroma_hshift[ch], vs = d.chroma_vshift[ch];
      const bool off_grid = (hs && col % 2) || (vs && row % 2);
      // dec_group.cc:492: the quant field at column (bx >> hshift) of the group, in the block's own row
      const uint32_t qx = v.bx - col + (col >> hs);
      const uint32_t qf = qf_at[size_t(v.by) * d.xsize_blocks + qx];
      EXPECT(qf != 0, "block %u channel %u: no varblock starts at the channel's column", i, ch);
      uint32_t bucket = 0;
      for (uint32_t t = 0; t < d.num_qf_thresholds; t++) bucket += qf > d.qf_thresholds[t] ? 1 : 0;
      const size_t idx = ((size_t(ch) * 13 + jxlhip::kStrategyOrder[v.strategy]) * nq + bucket) * d.num_dc_ctxs + v.quant_dc_ctx;
      EXPECT(((w >> (12 + 4 * ch)) & 15) == d.block_ctx_lut[idx], "block %u channel %u: context %u, the lut has %u", i, ch,
             (w >> (12 + 4 * ch)) & 15, d.block_ctx_lut[idx]);
      EXPECT(((w >> (24 + ch)) & 1) == uint32_t(off_grid) && ((w >> (27 + ch)) & 1) == hs, "block %u channel %u: grid bits", i, ch);
    }
    EXPECT((w >> 30) == 0, "block %u: spare bits", i);
  }
  for (uint32_t i = 0; i < 16; i++) EXPECT(recs[d.num_blocks + i] == 0, "block_recs padding");

  // ---- alias tables in the lane kernel's form
  for (uint32_t p = 0; p < d.num_passes; p++) {
    const JxlHipPassDesc& s = d.passes[p];
    const size_t n = s.use_prefix ? 0 : size_t(s.num_clusters) << s.log_alpha;
    EXPECT(c.pass_bufs[p].alias_packed.bytes == n * 8 && c.pass_bufs[p].alias.bytes == n * 8, "pass %u: alias sizes", p);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(B + c.pass_bufs[p].alias_packed.at);
    const uint8_t* a = static_cast<const uint8_t*>(s.alias);
    for (size_t i = 0; i < n; i++) {
      const uint32_t cutoff = a[8 * i], right = a[8 * i + 1], freq0 = a[8 * i + 2] | a[8 * i + 3] << 8, offs1 = a[8 * i + 4] | a[8 * i + 5] << 8,
                     freq1 = a[8 * i + 6] | a[8 * i + 7] << 8;
      const uint32_t cfg = s.uint_cfg[i >> s.log_alpha], x = q[2 * i], y = q[2 * i + 1];
      EXPECT((x & 0xFFF) == ((freq0 - 1) & 0xFFF) && (x >> 24) == cutoff, "pass %u entry %zu: x", p, i);
      EXPECT(((x >> 12) & 15) == (cfg & 0xFF) && ((x >> 16) & 15) == ((cfg >> 8) & 0xFF) && ((x >> 20) & 15) == ((cfg >> 16) & 0xFF), "pass %u entry %zu: config", p, i);
      EXPECT((y & 0xFFF) == ((freq1 - 1) & 0xFFF) && ((y >> 12) & 0xFFF) == offs1 && (y >> 24) == right, "pass %u entry %zu: y", p, i);
    }
  }

  // ---- work lists
  const uint32_t* tlist = reinterpret_cast<const uint32_t*>(B + c.tlist.at);
  const uint32_t* trecs = reinterpret_cast<const uint32_t*>(B + c.trecs.at);
  const size_t entries = d.num_blocks ? d.num_blocks : 1;
  EXPECT(c.tlist.bytes == entries * 4 && c.trecs.bytes == entries * 16, "work list sizes");
  std::vector<int> seen(d.num_blocks, 0);
  uint32_t listed = 0;
  for (int s = 0; s < 27; s++) {
    EXPECT(P.list_begin[s] == listed, "list %d begins at %u, not %u", s, P.list_begin[s], listed);
    for (uint32_t j = listed; j < listed + P.list_count[s]; j++) {
      EXPECT(tlist[j] < d.num_blocks && d.blocks[tlist[j]].strategy == s, "entry %u of list %d", j, s);
      seen[tlist[j]]++;
    }
    listed += P.list_count[s];
  }
  EXPECT(listed == P.listed, "listed");
  for (uint32_t i = 0; i < d.num_blocks; i++) {
    const uint32_t group_row = d.blocks[i].by / 32;
    const bool in_band = group_row >= g.ext_row0 && group_row < g.ext_row1;
    EXPECT(seen[i] == (in_band ? 1 : 0), "block %u (group row %u) is listed %d times", i, group_row, seen[i]);
  }
  for (size_t j = 0; j < entries; j++) {
    const uint32_t* r = trecs + 4 * j;
    if (j >= listed) {
      EXPECT(tlist[j] == 0 && !r[0] && !r[1] && !r[2] && !r[3], "padding entry %zu", j);
      continue;
    }
    const JxlHipVarBlock& v = d.blocks[tlist[j]];
    const uint32_t group = (v.by / 32) * d.xsize_groups + v.bx / 32;
    EXPECT(r[0] == (uint32_t(v.bx) | uint32_t(v.by) << 16) && r[1] == v.qf && r[2] == group * 3 * 65536 + v.coef_offset && r[3] == tlist[j], "record %zu", j);
  }
  {  // the same rows, as the group lists and the pixel rows have them
    const uint32_t yg = d.num_groups / d.xsize_groups;
    const uint32_t b0 = d.band_group_row_begin, b1 = d.band_group_row_end ? d.band_group_row_end : yg;
    EXPECT(g.ext_row0 == (b0 ? b0 - 1 : 0) && g.ext_row1 == std::min(yg, b1 + 1) && g.band_y0 == b0 * 256 && g.band_y1 == std::min(d.ysize, b1 * 256), "band rows");
    std::vector<uint32_t> gl, ag, ab, as;
    up::BuildGroupLists(d, g, &gl, &ag, &ab, &as);
    EXPECT(gl.size() + ag.size() == size_t(g.ext_row1 - g.ext_row0) * d.xsize_groups && ab.size() == 2 * ag.size() && as.size() % 3 == 0, "group lists");
    for (uint32_t grp : gl) EXPECT(grp / d.xsize_groups >= g.ext_row0 && grp / d.xsize_groups < g.ext_row1 && !(d.group_absent && d.group_absent[grp]), "group %u", grp);
    for (uint32_t grp : ag) EXPECT(d.group_absent && d.group_absent[grp], "absent group %u", grp);
    size_t missing = 0;
    for (uint32_t grp : gl)
      for (uint32_t p = 1; d.group_absent && p < d.num_passes; p++) missing += d.section_size[size_t(p) * d.num_groups + grp] == 0;
    EXPECT(as.size() == 3 * missing, "%zu missing sections listed, %zu are", as.size() / 3, missing);
  }

  // ---- dequantisation tables in scan order (single-pass frames)
  if (P.scan_order) {
    const float* scan = reinterpret_cast<const float*>(B + c.dequant_scan.at);
    EXPECT(c.dequant_scan.bytes == size_t(d.dequant_floats) * 4, "dequant_scan size");
    std::vector<float> want(d.dequant_floats, 0.0f);
    for (uint32_t i = 0; i < d.num_blocks; i++) {
      if (!seen[i]) continue;
      const uint32_t st = d.blocks[i].strategy, kind = jxlhip::kStrategyQuantTable[st], size = d.dequant_size[kind];
      for (uint32_t ch = 0; ch < 3; ch++) {
        const uint16_t* order = d.passes[0].orders + d.passes[0].order_offset[jxlhip::kStrategyOrder[st] * 3 + ch];
        for (uint32_t k = 0; k < size; k++) want[d.dequant_offset[kind] + ch * size + k] = d.dequant[d.dequant_offset[kind] + ch * size + order[k]];
      }
    }
    EXPECT(memcmp(scan, want.data(), want.size() * 4) == 0, "dequant_scan");
  } else {
    EXPECT(!c.dequant_scan.placed, "dequant_scan of a progressive frame");
  }
  float folded[9];
  up::FoldGaborish(d.gab_w, folded);
  for (int ch = 0; ch < 3; ch++) {
    const float mul = 1.0f / (1.0f + 4 * (d.gab_w[2 * ch] + d.gab_w[2 * ch + 1]));
    EXPECT(folded[3 * ch] == mul && folded[3 * ch + 1] == d.gab_w[2 * ch] * mul && folded[3 * ch + 2] == d.gab_w[2 * ch + 1] * mul, "gaborish %d", ch);
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------------- the double
struct Kats {
  int result = -1;
  std::vector<bool> exercised = std::vector<bool>(up::kNumRules, false);
};
extern "C" int jxlhip_frame_upload(JxlHipContext* ctx, const JxlHipFrameDesc* d) {
  Kats* k = reinterpret_cast<Kats*>(ctx);
  k->result = CheckRefusals(*d, &k->exercised);
  if (!k->result) k->result = CheckTables(*d, up::UploadOptions());
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string kind = argv[1];
  const uint32_t b0 = kind == "band" && argc >= 5 ? uint32_t(atoi(argv[2])) : 0, b1 = kind == "band" && argc >= 5 ? uint32_t(atoi(argv[3])) : 0;
  FILE* f = fopen(argv[argc - 1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> data;
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + n);
  fclose(f);
  JxlAmdFrame* frame = nullptr;
  if (kind == "partial") {  // the shortest prefix, in steps of a twentieth, that has some groups and lacks others
    for (int step = 4; step < 20 && !frame; step++) {
      uint32_t present = 0, info[16];
      if (jxlamd_frame_parse_partial_at(data.data(), data.size() * step / 20, 0, 0, nullptr, nullptr, &frame, &present)) continue;
      jxlamd_frame_info(frame, info);
      if (present == 0 || present == info[4]) {
        jxlamd_frame_free(frame);
        frame = nullptr;
      }
    }
  } else if (kind == "partial_late") {
    // the longest such prefix. Sections come pass by pass, so only here do some groups have every pass while others lack
    // the last ones
    for (int step = 19; step >= 4 && !frame; step--)
      if (jxlamd_frame_parse_partial_at(data.data(), data.size() * step / 20, 0, 0, nullptr, nullptr, &frame, nullptr)) frame = nullptr;
  } else if (jxlamd_frame_parse(data.data(), data.size(), nullptr, nullptr, &frame)) {
    frame = nullptr;
  }
  if (!frame) {
    fprintf(stderr, "FAIL: %s does not parse (%s)\n", argv[argc - 1], jxlamd_last_error());
    return 1;
  }
  Kats k;
  const int r = jxlamd_frame_upload_band(frame, reinterpret_cast<JxlHipContext*>(&k), b0, b1);
  jxlamd_frame_free(frame);
  if (r || k.result) {
    fprintf(stderr, "FAIL: upload %d, checks %d\n", r, k.result);
    return 1;
  }
  printf("exercised:");
  for (int i = 0; i < up::kNumRules; i++)
    if (k.exercised[i]) printf(" %s", kRuleNames[i]);
  printf("\n");
  return 0;
}
