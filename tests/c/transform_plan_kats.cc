// Known-answer tests of libjxl_amd/csrc/host/jxh_transform_plan.h, the launch plan of jxlhip_run_transform_batch, and of
// libjxl_amd/csrc/host/jxh_set_memo.h, the memo of a batched launch's set. Built by tests/test_transform_plan.py as a
// stand-alone program with -fsanitize=address,undefined; its arguments are the covered blocks of the 27 strategies across
// and down, from tests/golden/ref_constant_tables.json, and TransformParams::cs of the five subsampled layouts of the GPU
// tests (test_inverse_f64.SUBSAMPLED_KW). The expected reading is the descriptor loop and the launch loops as they stood
// in the HIP layer (jxl_hip_api.hip PrepareDownstream / BlocksPerWG / LaunchIdctFast / LaunchTransforms) before the
// header existed, recording each launch instead of making it, with the kernels' sizes written out here: nothing expected
// comes from the headers.
#include "../../libjxl_amd/csrc/host/jxh_transform_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../libjxl_amd/csrc/host/jxh_set_memo.h"

namespace tp = jxh::transform_plan;

#define EXPECT(cond, ...)                                             \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                                   \
      fprintf(stderr, "\n");                                          \
      return 1;                                                       \
    }                                                                 \
  } while (0)
#define RUN(call)       \
  do {                  \
    if (call) return 1; \
  } while (0)

static uint32_t g_covered_x[27], g_covered_y[27];  // the golden file's
static uint32_t g_layout_cs[27];                   // SUBSAMPLED_KW's (five), as hshift of channel c in bit 2c, vshift in bit 2c + 1

// ------------------------------------------------------------------------------------------------- the earlier reading
namespace before {
// What the loops read of a context.
struct Context {
  uint32_t list_count[27];
  uint32_t cs, xs, ext_y0, ext_y1;
};
struct uint2 {
  uint32_t x, y;
};
enum Kernel { k_idct_fast, k_special, k_chroma_upsample, k_dct_big };
// A launch as the loops made it: the kernel and its template arguments, grid, block, dynamic LDS, and what the arguments
// said (the descriptor offset; the frame, its channel's shifts and rows; the frame, the offset into its list and the count).
struct Launch {
  Kernel kernel;
  int CX, CY;
  bool CS;
  uint32_t grid_x, grid_y, block;
  size_t lds;
  uint32_t strategy, desc_first, frame, ch, hs, vs, y0, y1, list_first, m;
};
struct Set {
  std::vector<uint2> desc;
  uint32_t desc_begin[27] = {}, desc_count[27] = {};
  std::vector<Launch> launches;
};

constexpr int IdctFastThreads(int cx, int cy) { return (void(cx), void(cy), 64); }
// Varblocks a workgroup of the strategy's kernel handles.
static uint32_t BlocksPerWG(int s) {
  const uint32_t cx = g_covered_x[s], cy = g_covered_y[s];
  if (s == 0 || (s >= 4 && s <= 11) || (s >= 18 && s <= 20))  // k_idct_fast: max(rows, columns) threads per varblock
    return IdctFastThreads(cx, cy) / ((cx > cy ? cx : cy) * 8);
  return 4;  // k_special
}

template <int CX, int CY, bool CS = false>
static void LaunchIdctFast(Set* c0, int s) {
  constexpr int C = CX * 8, R = CY * 8, TB = R > C ? R : C, GROUPS = IdctFastThreads(CX, CY) / TB;
  constexpr size_t lds = size_t(GROUPS) * R * (C + 1) * sizeof(float);
  const int li = CS ? 21 : s;  // (the work list; the strategy stays s)
  c0->launches.push_back({k_idct_fast, CX, CY, CS, c0->desc_count[li], 1, uint32_t(IdctFastThreads(CX, CY)), lds, uint32_t(s), c0->desc_begin[li], 0, 0, 0,
                          0, 0, 0, 0, 0});
}

static void PrepareDownstream(Set* c0, const Context* ctxs, size_t n) {
  std::vector<uint2>& desc = c0->desc;
  for (int s = 0; s < 22; s++) {  // (21: the 8x8 DCT varblocks of chroma-subsampled frames, which list 0 leaves out)
    c0->desc_begin[s] = uint32_t(desc.size());
    const int st = s == 21 ? 0 : s;
    const uint32_t bpw = BlocksPerWG(st);
    for (size_t i = 0; i < n; i++) {
      if (st == 0 && (ctxs[i].cs != 0) != (s == 21)) continue;
      for (uint32_t j = 0; j < ctxs[i].list_count[st]; j += bpw) desc.push_back({uint32_t(i), j});
    }
    c0->desc_count[s] = uint32_t(desc.size()) - c0->desc_begin[s];
  }
}

static void LaunchTransforms(Set* c0, const Context* ctxs, size_t nctx) {
  for (int s = 0; s < 21; s++) {
    if (!c0->desc_count[s]) continue;
    switch (s) {
      case 0: LaunchIdctFast<1, 1>(c0, s); break;
      case 4: LaunchIdctFast<2, 2>(c0, s); break;
      case 5: LaunchIdctFast<4, 4>(c0, s); break;
      case 6: LaunchIdctFast<1, 2>(c0, s); break;
      case 7: LaunchIdctFast<2, 1>(c0, s); break;
      case 8: LaunchIdctFast<1, 4>(c0, s); break;
      case 9: LaunchIdctFast<4, 1>(c0, s); break;
      case 10: LaunchIdctFast<2, 4>(c0, s); break;
      case 11: LaunchIdctFast<4, 2>(c0, s); break;
      case 18: LaunchIdctFast<8, 8>(c0, s); break;  // (the 64-class: one varblock per wave)
      case 19: LaunchIdctFast<4, 8>(c0, s); break;
      case 20: LaunchIdctFast<8, 4>(c0, s); break;
      default:
        c0->launches.push_back({k_special, 0, 0, false, c0->desc_count[s], 1, 256, 0, uint32_t(s), c0->desc_begin[s], 0, 0, 0, 0, 0, 0, 0, 0});
    }
  }
  if (c0->desc_count[21]) {  // the 8x8 DCT varblocks of chroma-subsampled frames
    LaunchIdctFast<1, 1, true>(c0, 0);
  }
  // ... whose subsampled channels then go back to the frame's resolution, in front of the filters
  for (size_t f = 0; f < nctx; f++) {
    const Context* c = &ctxs[f];
    if (!c->cs) continue;
    for (uint32_t ch = 0; ch < 3; ch++) {
      const uint32_t hs = (c->cs >> (2 * ch)) & 1u;
      const uint32_t vs = (c->cs >> (2 * ch + 1)) & 1u;
      if (!(hs | vs)) continue;
      const uint32_t xs = c->xs, y0 = c->ext_y0, y1 = c->ext_y1;
      if (y1 <= y0) continue;
      c0->launches.push_back({k_chroma_upsample, 0, 0, false, (xs + 63) / 64, (y1 - y0 + 3) / 4, 256, 0, 0, 0, uint32_t(f), ch, hs, vs, y0, y1, 0, 0});
    }
  }
  // 128/256-class transforms go through per-frame global scratch: one frame at a time (rare)
  for (size_t f = 0; f < nctx; f++) {
    const Context* c = &ctxs[f];
    for (int s = 21; s < 27; s++) {
      const uint32_t n = c->list_count[s];
      if (!n) continue;
      for (uint32_t i = 0; i < n; i += 32) {
        const uint32_t m = n - i < 32 ? n - i : 32;
        c0->launches.push_back({k_dct_big, 0, 0, false, m * 3, 1, 256, 0, uint32_t(s), 0, uint32_t(f), 0, 0, 0, 0, 0, i, m});
      }
    }
  }
}
}  // namespace before

// ------------------------------------------------------------------------------------------------- the comparison
typedef before::Context Frame;

static Frame Frame444(uint32_t xs = 520, uint32_t ys = 392) {
  Frame f;
  memset(&f, 0, sizeof(f));
  f.xs = xs;
  f.ext_y1 = ys;
  return f;
}

// Both readings of `frames`: the same descriptors and the same launches. What the HIP layer derives from a planned launch
// (the kernel and its template arguments from the list, the chroma shifts from cs) is derived here in the same way.
static int Compare(const char* what, const std::vector<Frame>& frames, tp::TransformPlan* plan_out = nullptr) {
  std::vector<tp::TransformFrame> in(frames.size());
  for (size_t i = 0; i < frames.size(); i++) {
    memcpy(in[i].list_count, frames[i].list_count, sizeof(in[i].list_count));
    in[i].cs = frames[i].cs;
    in[i].xs = frames[i].xs;
    in[i].ext_y0 = frames[i].ext_y0;
    in[i].ext_y1 = frames[i].ext_y1;
  }
  before::Set want;
  before::PrepareDownstream(&want, frames.data(), frames.size());
  before::LaunchTransforms(&want, frames.data(), frames.size());
  tp::TransformPlan plan;
  tp::PlanTransformLaunches(in.data(), in.size(), &plan);
  EXPECT(plan.desc.size() == want.desc.size(), "%s: %zu descriptors, were %zu", what, plan.desc.size(), want.desc.size());
  EXPECT(plan.desc.capacity() == plan.desc.size(), "%s: the descriptor array was reserved for %zu, holds %zu", what, plan.desc.capacity(), plan.desc.size());
  for (size_t i = 0; i < want.desc.size(); i++)
    EXPECT(plan.desc[i].frame == want.desc[i].x && plan.desc[i].first == want.desc[i].y, "%s: descriptor %zu is (%u, %u), was (%u, %u)", what, i,
           plan.desc[i].frame, plan.desc[i].first, want.desc[i].x, want.desc[i].y);
  EXPECT(plan.launches.size() == want.launches.size(), "%s: %zu launches, were %zu", what, plan.launches.size(), want.launches.size());
  for (size_t i = 0; i < want.launches.size(); i++) {
    const tp::TransformLaunch& L = plan.launches[i];
    const before::Launch& w = want.launches[i];
    EXPECT(L.grid_x == w.grid_x && L.grid_y == w.grid_y && L.block == w.block && L.lds == w.lds, "%s: launch %zu is %u x %u of %u with %zu bytes, was %u x %u of %u with %zu",
           what, i, L.grid_x, L.grid_y, L.block, L.lds, w.grid_x, w.grid_y, w.block, w.lds);
    switch (w.kernel) {
      case before::k_idct_fast:
      case before::k_special: {
        EXPECT(L.kind == tp::kListLaunch && L.strategy == w.strategy && L.first == w.desc_first && L.count == w.grid_x, "%s: launch %zu: kind %d strategy %u first %u count %u, was strategy %u first %u count %u",
               what, i, int(L.kind), L.strategy, L.first, L.count, w.strategy, w.desc_first, w.grid_x);
        EXPECT(L.list == (w.CS ? 21u : w.strategy) && L.list < jxlhip::kTransformLists, "%s: launch %zu: list %u", what, i, L.list);
        const bool fast = jxlhip::TransformClassOf(L.strategy) == jxlhip::kFastClass;
        EXPECT(fast == (w.kernel == before::k_idct_fast), "%s: launch %zu: strategy %u is of class %d", what, i, L.strategy, int(jxlhip::TransformClassOf(L.strategy)));
        if (fast)
          EXPECT(int(jxlhip::kCoveredX[L.strategy]) == w.CX && int(jxlhip::kCoveredY[L.strategy]) == w.CY && (L.list == jxlhip::kSubsampledList) == w.CS,
                 "%s: launch %zu: k_idct_fast<%d, %d, %d>", what, i, w.CX, w.CY, int(w.CS));
        break;
      }
      case before::k_chroma_upsample:
        EXPECT(L.kind == tp::kChromaUpLaunch && L.frame == w.frame && L.channel == w.ch, "%s: launch %zu: kind %d frame %u channel %u, was frame %u channel %u", what, i,
               int(L.kind), L.frame, L.channel, w.frame, w.ch);
        EXPECT(((frames[L.frame].cs >> (2 * L.channel)) & 1u) == w.hs && ((frames[L.frame].cs >> (2 * L.channel + 1)) & 1u) == w.vs &&
                   frames[L.frame].ext_y0 == w.y0 && frames[L.frame].ext_y1 == w.y1,
               "%s: launch %zu: the channel's shifts and rows", what, i);
        break;
      case before::k_dct_big:
        EXPECT(L.kind == tp::kBigLaunch && L.strategy == w.strategy && L.frame == w.frame && L.first == w.list_first && L.count == w.m,
               "%s: launch %zu: kind %d strategy %u frame %u first %u count %u, was strategy %u frame %u first %u count %u", what, i, int(L.kind), L.strategy, L.frame,
               L.first, L.count, w.strategy, w.frame, w.list_first, w.m);
        break;
    }
  }
  if (plan_out) *plan_out = std::move(plan);
  return 0;
}

static size_t CountKind(const tp::TransformPlan& plan, tp::LaunchKind kind) {
  size_t k = 0;
  for (const tp::TransformLaunch& L : plan.launches) k += L.kind == kind;
  return k;
}

// One frame with all 27 lists non-zero (and unequal), alone and between two others.
static int TestAllLists() {
  Frame f = Frame444();
  for (int s = 0; s < 27; s++) f.list_count[s] = uint32_t(3 + 5 * s);
  tp::TransformPlan plan;
  RUN(Compare("all 27 lists", {f}, &plan));
  EXPECT(CountKind(plan, tp::kListLaunch) == 21 && CountKind(plan, tp::kChromaUpLaunch) == 0, "all 27 lists: %zu list launches", CountKind(plan, tp::kListLaunch));
  for (size_t i = 0; i < 21; i++) EXPECT(plan.launches[i].strategy == i && plan.launches[i].list == i, "all 27 lists: launch %zu", i);
  // by hand: 8x8 takes eight varblocks per wave and 8 * 8 * 9 floats; 32x32 two and 2 * 32 * 33; 64x64 one and 64 * 65
  EXPECT(plan.launches[0].count == 1 && plan.launches[0].lds == 8 * 8 * 9 * 4 && plan.launches[0].block == 64, "all 27 lists: the 8x8 launch");
  EXPECT(plan.launches[5].count == (3 + 25 + 1) / 2 && plan.launches[5].lds == 2 * 32 * 33 * 4, "all 27 lists: the 32x32 launch");
  EXPECT(plan.launches[18].count == 3 + 90 && plan.launches[18].lds == 64 * 65 * 4, "all 27 lists: the 64x64 launch");
  EXPECT(plan.launches[1].count == (3 + 5 + 3) / 4 && plan.launches[1].lds == 0 && plan.launches[1].block == 256, "all 27 lists: the IDENTITY launch");
  Frame g = Frame444(264, 136), h = Frame444(331, 245);
  for (int s = 0; s < 27; s += 2) g.list_count[s] = uint32_t(40 - s);
  for (int s = 1; s < 27; s += 3) h.list_count[s] = uint32_t(7 * s);
  RUN(Compare("three frames", {g, f, h}));
  return 0;
}

// Counts of 0, 1, exactly one workgroup, and one more than that, for each class; frames beside each other so that a
// frame's last workgroup is ragged in the middle of a list.
static int TestWorkgroupEdges() {
  for (int s = 0; s < 21; s++) {
    const uint32_t cx = g_covered_x[s], cy = g_covered_y[s];
    const bool fast = s == 0 || (s >= 4 && s <= 11) || (s >= 18 && s <= 20);
    const uint32_t bpw = fast ? 64 / ((cx > cy ? cx : cy) * 8) : 4;
    const uint32_t counts[] = {0, 1, bpw, bpw + 1};
    std::vector<Frame> all;
    for (uint32_t n : counts) {
      Frame f = Frame444();
      f.list_count[s] = n;
      tp::TransformPlan plan;
      RUN(Compare(("strategy " + std::to_string(s) + ", " + std::to_string(n) + " varblocks").c_str(), {f}, &plan));
      EXPECT(plan.launches.size() == (n ? 1u : 0u) && plan.desc.size() == (n + bpw - 1) / bpw, "strategy %d, %u varblocks: %zu launches, %zu descriptors", s, n,
             plan.launches.size(), plan.desc.size());
      all.push_back(f);
    }
    RUN(Compare(("strategy " + std::to_string(s) + ", four frames").c_str(), all));
  }
  return 0;
}

// A 4:4:4 and a 4:2:0 frame together: list 0 against list 21, with neither in the other's.
static int TestSubsampledBeside444() {
  Frame a = Frame444(), b = Frame444(264, 200);
  a.list_count[0] = 100;
  a.list_count[4] = 9;
  b.cs = 0x33;  // channels 0 and 2 at half size both ways
  b.list_count[0] = 37;
  b.list_count[2] = 6;
  for (int order = 0; order < 2; order++) {
    const uint32_t ia = order ? 1 : 0, ib = 1 - ia;
    tp::TransformPlan plan;
    RUN(Compare("4:4:4 beside 4:2:0", order ? std::vector<Frame>{b, a} : std::vector<Frame>{a, b}, &plan));
    const tp::TransformLaunch& l0 = plan.launches[0];
    EXPECT(l0.list == 0 && l0.count == 13, "4:4:4 beside 4:2:0: list 0 has %u workgroups", l0.count);
    for (uint32_t i = 0; i < l0.count; i++) EXPECT(plan.desc[l0.first + i].frame == ia, "4:4:4 beside 4:2:0: list 0 names frame %u", plan.desc[l0.first + i].frame);
    const tp::TransformLaunch* l21 = nullptr;
    for (const tp::TransformLaunch& L : plan.launches)
      if (L.kind == tp::kListLaunch && L.list == 21) l21 = &L;
    EXPECT(l21 && l21->strategy == 0 && l21->count == 5, "4:4:4 beside 4:2:0: list 21");
    for (uint32_t i = 0; i < l21->count; i++) EXPECT(plan.desc[l21->first + i].frame == ib, "4:4:4 beside 4:2:0: list 21 names frame %u", plan.desc[l21->first + i].frame);
    EXPECT(CountKind(plan, tp::kChromaUpLaunch) == 2, "4:4:4 beside 4:2:0: %zu channels upsample", CountKind(plan, tp::kChromaUpLaunch));
    // (by hand: 264 columns in 5 workgroups of 64, 200 rows in 50 of 4)
    for (const tp::TransformLaunch& L : plan.launches)
      if (L.kind == tp::kChromaUpLaunch) EXPECT(L.frame == ib && L.grid_x == 5 && L.grid_y == 50 && L.block == 256, "4:4:4 beside 4:2:0: the upsampling grid");
  }
  return 0;
}

// The subsampled streams of the GPU tests (4:2:0, 4:2:2, 4:4:0: Cb and Cr at half size both ways / across / down; Cb 1x2,
// Y 2x1, Cr 2x2: Cb halved across, Y halved down; 4:2:0 again) and two more: which channels upsample; and no rows, no launch.
static int TestSubsampledLayouts() {
  const struct {
    const char* name;
    uint32_t cs, channels, mask;  // (mask: bit c for channel c)
  } kLayouts[] = {{"4:2:0", g_layout_cs[0], 2, 5}, {"4:2:2", g_layout_cs[1], 2, 5}, {"4:4:0", g_layout_cs[2], 2, 5}, {"luma subsampled too", g_layout_cs[3], 2, 3},
                  {"4:2:0, custom cmap", g_layout_cs[4], 2, 5}, {"every channel, mixed", 0x27, 3, 7}, {"one channel across", 0x04, 1, 2}};
  EXPECT(g_layout_cs[0] == 0x33 && g_layout_cs[1] == 0x11 && g_layout_cs[2] == 0x22 && g_layout_cs[3] == 0x09 && g_layout_cs[4] == 0x33, "the layouts' cs");
  for (const auto& l : kLayouts) {
    Frame f = Frame444(265, 201);
    f.cs = l.cs;
    f.list_count[0] = 50;
    f.list_count[13] = 3;
    tp::TransformPlan plan;
    RUN(Compare(l.name, {f}, &plan));
    EXPECT(CountKind(plan, tp::kChromaUpLaunch) == l.channels, "%s: %zu channels upsample", l.name, CountKind(plan, tp::kChromaUpLaunch));
    for (const tp::TransformLaunch& L : plan.launches)
      if (L.kind == tp::kChromaUpLaunch) EXPECT(((l.mask >> L.channel) & 1u) != 0 && L.grid_x == 5 && L.grid_y == 51, "%s: channel %u", l.name, L.channel);
    // a band: rows 64 .. 130; then ext_y1 == ext_y0 and ext_y1 < ext_y0
    f.ext_y0 = 64;
    f.ext_y1 = 130;
    RUN(Compare(l.name, {f}, &plan));
    for (const tp::TransformLaunch& L : plan.launches)
      if (L.kind == tp::kChromaUpLaunch) EXPECT(L.grid_y == 17, "%s: a band of 66 rows in %u workgroups", l.name, L.grid_y);
    f.ext_y1 = 64;
    RUN(Compare(l.name, {f, Frame444()}, &plan));
    EXPECT(CountKind(plan, tp::kChromaUpLaunch) == 0 && CountKind(plan, tp::kListLaunch) == 2, "%s: no rows, %zu upsampling launches", l.name,
           CountKind(plan, tp::kChromaUpLaunch));
    f.ext_y1 = 8;
    RUN(Compare(l.name, {f}, &plan));
    EXPECT(CountKind(plan, tp::kChromaUpLaunch) == 0, "%s: rows 64 .. 8", l.name);
  }
  return 0;
}

// Big lists of 31, 32, 33 and 65 varblocks: chunks of 32, three workgroups per varblock.
static int TestBig() {
  const uint32_t counts[] = {31, 32, 33, 65};
  const size_t chunks[] = {1, 1, 2, 3};
  std::vector<Frame> all;
  for (int k = 0; k < 4; k++) {
    Frame f = Frame444();
    f.list_count[21 + k] = counts[k];
    tp::TransformPlan plan;
    RUN(Compare("a big list", {f}, &plan));
    EXPECT(plan.desc.empty() && plan.launches.size() == chunks[k], "a big list of %u: %zu launches", counts[k], plan.launches.size());
    uint32_t at = 0;
    for (const tp::TransformLaunch& L : plan.launches) {
      EXPECT(L.first == at && L.count <= 32 && L.grid_x == 3 * L.count && L.block == 256, "a big list of %u: chunk at %u of %u", counts[k], L.first, L.count);
      at += L.count;
    }
    EXPECT(at == counts[k], "a big list of %u: %u varblocks launched", counts[k], at);
    f.list_count[26] = 1;
    f.list_count[0] = 11;
    all.push_back(f);
  }
  RUN(Compare("big lists of four frames", all));
  return 0;
}

static int TestEmpty() {
  tp::TransformPlan plan;
  plan.launches.resize(3);  // (what an earlier plan left)
  plan.desc.resize(5);
  RUN(Compare("no frames", {}, &plan));
  EXPECT(plan.desc.empty() && plan.launches.empty(), "no frames");
  RUN(Compare("frames without varblocks", {Frame444(), Frame444(8, 8)}, &plan));
  EXPECT(plan.desc.empty() && plan.launches.empty(), "frames without varblocks");
  return 0;
}

// 640 frames of 129 600 8x8 varblocks (3840 x 2160): 16 200 workgroups a frame, 10 368 000 descriptors, one launch.
static int Test640() {
  Frame f = Frame444(3840, 2160);
  f.list_count[0] = 129600;
  tp::TransformPlan plan;
  RUN(Compare("640 4K frames", std::vector<Frame>(640, f), &plan));
  EXPECT(plan.launches.size() == 1 && plan.desc.size() == 10368000u, "640 4K frames: %zu launches, %zu descriptors", plan.launches.size(), plan.desc.size());
  const tp::TransformLaunch& L = plan.launches[0];
  EXPECT(L.first == 0 && L.count == 10368000u && L.grid_x == 10368000u && uint64_t(L.grid_x) * L.block < (uint64_t(1) << 32), "640 4K frames: the launch");
  EXPECT(plan.desc.back().frame == 639 && plan.desc.back().first == 129592, "640 4K frames: the last descriptor");
  EXPECT(plan.desc.size() * sizeof(tp::WorkgroupDesc) < (uint64_t(1) << 32), "640 4K frames: the array's bytes");
  return 0;
}

// The class of each strategy, and the fast class's template arguments, against the golden file's covered sizes.
static int TestClasses() {
  for (uint32_t s = 0; s < 27; s++) {
    const uint32_t cx = g_covered_x[s], cy = g_covered_y[s];
    EXPECT(jxlhip::kCoveredX[s] == cx && jxlhip::kCoveredY[s] == cy, "strategy %u covers %u x %u", s, cx, cy);
    const bool fast = s == 0 || (s >= 4 && s <= 11) || (s >= 18 && s <= 20), big = s >= 21;  // as the switch and the loops had it
    const jxlhip::TransformClass want = fast ? jxlhip::kFastClass : (big ? jxlhip::kBigClass : jxlhip::kSpecialClass);
    EXPECT(jxlhip::TransformClassOf(s) == want, "strategy %u: class %d, was %d", s, int(jxlhip::TransformClassOf(s)), int(want));
    EXPECT(big == (cx * 8 > 64 || cy * 8 > 64), "strategy %u: %u x %u blocks", s, cx, cy);
    if (!big) EXPECT(jxlhip::TransformBlocksPerWG(s) == before::BlocksPerWG(int(s)), "strategy %u: %u varblocks per workgroup", s, jxlhip::TransformBlocksPerWG(s));
  }
  static_assert(jxlhip::kSubsampledList == 21 && jxlhip::kTransformLists == 22 && jxlhip::kSpecialBlocksPerWG == 4 && jxlhip::kSpecialThreads == 256 &&
                    jxlhip::kChromaUpCols == 64 && jxlhip::kChromaUpRows == 4 && jxlhip::kBigBlocksPerLaunch == 32 && jxlhip::kBigWGsPerBlock == 3,
                "the kernels' sizes");
  // the scratch of a frame: min(largest big list, 32) varblocks x 3 channels x 2 planes of 65536 floats
  const uint32_t bigs[] = {1, 31, 32, 33, 1000};
  for (uint32_t big : bigs)
    EXPECT(jxlhip::BigScratchBytes(big) == size_t(big < 32u ? big : 32u) * 3 * 2 * 65536 * 4, "scratch for %u varblocks: %zu bytes", big, jxlhip::BigScratchBytes(big));
  return 0;
}

// ------------------------------------------------------------------------------------------------- the set memo
struct Ctx {
  uint64_t generation;
};
static int TestMemo() {
  Ctx a{1}, b{1}, c{7};
  const Ctx* set[] = {&a, &b, &c};
  const Ctx* swapped[] = {&b, &a, &c};
  uintptr_t planes[] = {0x1000, 0x2000, 0x1000};
  jxh::SetMemo<Ctx> memo;
  EXPECT(!memo.Matches(set, 3) && memo.size() == 0, "a fresh memo");
  memo.Remember(set, 3);
  EXPECT(memo.Matches(set, 3) && memo.size() == 3 && memo[1] == &b, "the same set");
  EXPECT(!memo.Matches(swapped, 3), "the same contexts in another order");
  EXPECT(!memo.Matches(set, 2) && !memo.Matches(set + 1, 2) && !memo.Matches(set, 0), "a shorter set");
  EXPECT(!memo.Matches(set, 3, planes), "a set with extra words against one remembered without");
  b.generation++;
  EXPECT(!memo.Matches(set, 3), "another generation");
  b.generation--;
  EXPECT(memo.Matches(set, 3), "the generation back");
  // with an extra word per context: the plane buffer of a lender that an upload reallocated
  memo.Remember(set, 3, planes);
  EXPECT(memo.Matches(set, 3, planes) && !memo.Matches(set, 3), "the same set with its words");
  planes[2] = 0x3000;
  EXPECT(!memo.Matches(set, 3, planes), "another extra word");
  memo.Remember(set, 3, planes);
  EXPECT(memo.Matches(set, 3, planes), "remembered again");
  memo.Remember(set, 2);
  EXPECT(memo.Matches(set, 2) && !memo.Matches(set, 2, planes) && !memo.Matches(set, 3, planes) && memo.size() == 2, "a shorter set remembered");
  memo.Forget();
  EXPECT(!memo.Matches(set, 2) && !memo.Matches(set, 3, planes) && memo.size() == 0, "forgotten");
  return 0;
}

static int ParseList(const char* arg, uint32_t* out) {
  int n = 0;
  for (const char* p = arg; *p && n < 27; n++) {
    char* end = nullptr;
    out[n] = uint32_t(strtoul(p, &end, 10));
    if (end == p) return -1;
    p = *end == ',' ? end + 1 : end;
  }
  return n;
}

int main(int argc, char** argv) {
  if (argc != 4 || ParseList(argv[1], g_covered_x) != 27 || ParseList(argv[2], g_covered_y) != 27 || ParseList(argv[3], g_layout_cs) != 5) {
    fprintf(stderr, "usage: transform_plan_kats covered_blocks_x covered_blocks_y (27 comma-separated values each) layouts_cs (5)\n");
    return 2;
  }
  RUN(TestClasses());
  RUN(TestAllLists());
  RUN(TestWorkgroupEdges());
  RUN(TestSubsampledBeside444());
  RUN(TestSubsampledLayouts());
  RUN(TestBig());
  RUN(TestEmpty());
  RUN(Test640());
  RUN(TestMemo());
  printf("transform plan kats passed\n");
  return 0;
}
