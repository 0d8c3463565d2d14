// Known-answer tests of libjxl_amd/csrc/host/jxh_filter_plan.h: the grouping of a set's frames into filter launches and the
// grid of the row-streaming kernel. Built by tests/test_filter_plan.py as a stand-alone program with
// -fsanitize=address,undefined. The expected reading is the grouping loop and the grid lines as they stood in the HIP
// layer (jxl_hip_api.hip PrepareDownstream / LaunchFilterRows) before the header existed, with the tile and strip sizes
// written out here: nothing expected comes from the header.
#include "../../libjxl_amd/csrc/host/jxh_filter_plan.h"

#include <stdio.h>

#include <string>

namespace fp = jxh::filter_plan;

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

// ------------------------------------------------------------------------------------------------- the earlier reading
namespace before {
namespace jxlhip {
constexpr int kFusedTW = 64, kFusedTH = 16;
constexpr int kRowsStrip = 64;
constexpr int kRowsWaves = 4;
constexpr int kRows2Cols = 120;
}  // namespace jxlhip
constexpr int JXLHIP_ERR_INVALID_ARGUMENT_ = 1;  // (include/jxl_amd_hip.h)

// What the loop read of a context and of its filter block.
struct Context {
  int epf_iters;
  bool gab, gray8_fast, tensor_fused;
  uint32_t xs, band_y0, band_y1;
};
struct Block {
  struct {
    bool rgb, rgbf;
    int linear_output;
  } f;
  bool filtered;
};
struct FilterGroup {
  int key;
  uint32_t first, count, tiles_x, tiles_y;
  bool u8srgb;
};

static int FilterKey(const Context* c) {
  const int epf = c->epf_iters < 0 ? 0 : (c->epf_iters > 3 ? 3 : c->epf_iters);
  return (c->tensor_fused ? 16 : 0) + (c->gray8_fast ? 8 : 0) + (c->gab ? 4 : 0) + epf;
}
// `blocks`: per context, in the order given (the loop filled block j from context order[j]).
static int Group(const Context* ctxs, const Block* blocks, size_t n, std::vector<size_t>* order_out, std::vector<FilterGroup>* fgroups) {
  std::vector<size_t> order(n);
  for (size_t i = 0; i < n; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return FilterKey(&ctxs[a]) < FilterKey(&ctxs[b]); });
  std::vector<Block> fparams(n);
  fgroups->clear();
  for (size_t j = 0; j < n; j++) {
    const Context* c = &ctxs[order[j]];
    fparams[j] = blocks[order[j]];
    const int key = FilterKey(c);
    const uint32_t tx = (c->xs + jxlhip::kFusedTW - 1) / jxlhip::kFusedTW;
    const uint32_t ty = (c->band_y1 - c->band_y0 + jxlhip::kFusedTH - 1) / jxlhip::kFusedTH;
    if (fgroups->empty() || fgroups->back().key != key) fgroups->push_back({key, uint32_t(j), 0, 0, 0, true});
    FilterGroup& g = fgroups->back();
    g.count++;
    g.u8srgb = g.u8srgb && fparams[j].f.rgb && !fparams[j].f.rgbf && !fparams[j].filtered && !fparams[j].f.linear_output;
    // (a one-channel frame has no other form to fall back to: every other writer would put three bytes per pixel into its rows)
    if (c->gray8_fast && !g.u8srgb) return JXLHIP_ERR_INVALID_ARGUMENT_;
    g.tiles_x = tx > g.tiles_x ? tx : g.tiles_x;
    g.tiles_y = ty > g.tiles_y ? ty : g.tiles_y;
  }
  *order_out = order;
  return 0;
}
static void Grid(const FilterGroup& g, uint32_t* gx_out, uint32_t* gy_out, uint32_t* strip_out) {
  const uint32_t cols = g.tiles_x * jxlhip::kFusedTW, rows = g.tiles_y * jxlhip::kFusedTH;  // upper bounds of the group
  const uint32_t gx = ((cols + jxlhip::kRows2Cols - 1) / jxlhip::kRows2Cols + jxlhip::kRowsWaves - 1) / jxlhip::kRowsWaves;
  uint32_t strip = jxlhip::kRowsStrip;
  if (uint64_t(gx) * jxlhip::kRowsWaves * ((rows + 2 * strip - 1) / (2 * strip)) * g.count >= 6 * 1024) strip *= 2;
  const uint32_t gy = (rows + strip - 1) / strip;
  *gx_out = gx;
  *gy_out = gy;
  *strip_out = strip;
}
}  // namespace before

static_assert(JXLHIP_ERR_INVALID_ARGUMENT == before::JXLHIP_ERR_INVALID_ARGUMENT_, "the refusal's code");
static_assert(jxlhip::kFusedTW == 64 && jxlhip::kFusedTH == 16 && jxlhip::kRowsStrip == 64 && jxlhip::kRowsWaves == 4 && jxlhip::kRows2Cols == 120,
              "the kernels' tile and strip sizes");

// ------------------------------------------------------------------------------------------------- the comparison
struct Frame {
  before::Context c;
  before::Block b;
};
// A frame of the 8-bit sRGB writer, whole height.
static Frame Rgb8(uint32_t xs, uint32_t ys, int epf = 1, bool gab = true) { return {{epf, gab, false, false, xs, 0, ys}, {{true, false, 0}, false}}; }

// Both readings of `frames`: the same verdict, and when it is 0 the same order, groups and row-kernel grids.
static int Compare(const char* what, const std::vector<Frame>& frames, int want_code, fp::FilterPlan* plan_out = nullptr) {
  std::vector<before::Context> ctxs;
  std::vector<before::Block> blocks;
  std::vector<fp::FilterFrame> in;
  for (const Frame& f : frames) {
    ctxs.push_back(f.c);
    blocks.push_back(f.b);
    in.push_back({fp::FormOf(f.c.epf_iters, f.c.gab, f.c.gray8_fast, f.c.tensor_fused), f.c.xs, f.c.band_y1 - f.c.band_y0, f.b.f.rgb, f.b.f.rgbf,
                  f.b.filtered, f.b.f.linear_output != 0});
    EXPECT(in.back().form.Key() == before::FilterKey(&f.c), "%s: key %d, was %d", what, in.back().form.Key(), before::FilterKey(&f.c));
  }
  std::vector<size_t> order;
  std::vector<before::FilterGroup> groups;
  const int want = before::Group(ctxs.data(), blocks.data(), frames.size(), &order, &groups);
  fp::FilterPlan plan;
  const int got = fp::PlanFilterGroups(in.data(), in.size(), &plan);
  EXPECT(want == want_code, "%s: the earlier reading gives %d, the case expects %d", what, want, want_code);
  EXPECT(got == want, "%s: code %d, was %d", what, got, want);
  if (want) return 0;
  EXPECT(plan.order.size() == order.size() && plan.groups.size() == groups.size(), "%s: %zu frames in %zu groups, were %zu in %zu", what,
         plan.order.size(), plan.groups.size(), order.size(), groups.size());
  for (size_t j = 0; j < order.size(); j++) EXPECT(plan.order[j] == order[j], "%s: place %zu holds frame %u, held %zu", what, j, plan.order[j], order[j]);
  for (size_t i = 0; i < groups.size(); i++) {
    const fp::FilterGroup& g = plan.groups[i];
    const before::FilterGroup& w = groups[i];
    EXPECT(g.form.Key() == w.key && g.first == w.first && g.count == w.count && g.tiles_x == w.tiles_x && g.tiles_y == w.tiles_y && g.u8srgb == w.u8srgb,
           "%s: group %zu is key %d first %u count %u tiles %u x %u u8srgb %d, was key %d first %u count %u tiles %u x %u u8srgb %d", what, i,
           g.form.Key(), g.first, g.count, g.tiles_x, g.tiles_y, int(g.u8srgb), w.key, w.first, w.count, w.tiles_x, w.tiles_y, int(w.u8srgb));
    // (the grid of every group, whichever kernel it takes: the arithmetic is the same)
    uint32_t gx, gy, strip;
    before::Grid(w, &gx, &gy, &strip);
    const fp::RowsGridDims d = fp::RowsGrid(g.tiles_x, g.tiles_y, g.count);
    EXPECT(d.gx == gx && d.gy == gy && d.strip == strip, "%s: group %zu grid %u x %u strip %u, was %u x %u strip %u", what, i, d.gx, d.gy, d.strip, gx,
           gy, strip);
  }
  if (plan_out) *plan_out = plan;
  return 0;
}

static int Test4K() {
  fp::FilterPlan plan;
  // one frame, by hand: 60 x 135 tiles; 3840 columns in 32 waves of 120 = 8 workgroups; 2160 rows in 34 strips of 64
  RUN(Compare("one 4K frame", {Rgb8(3840, 2160)}, 0, &plan));
  EXPECT(plan.groups.size() == 1 && plan.groups[0].tiles_x == 60 && plan.groups[0].tiles_y == 135 && plan.groups[0].u8srgb, "one 4K frame: the group");
  fp::RowsGridDims d = fp::RowsGrid(60, 135, 1);
  EXPECT(d.gx == 8 && d.strip == 64 && d.gy == 34, "one 4K frame: grid %u x %u, strip %u", d.gx, d.gy, d.strip);
  // the strip doubles where the launch with doubled strips still has 6 * 1024 waves: 8 * 4 * 17 = 544 per frame,
  // 544 * 11 = 5984 < 6144 <= 6528 = 544 * 12
  RUN(Compare("eleven 4K frames", std::vector<Frame>(11, Rgb8(3840, 2160)), 0));
  d = fp::RowsGrid(60, 135, 11);
  EXPECT(d.gx == 8 && d.strip == 64 && d.gy == 34, "eleven 4K frames: grid %u x %u, strip %u", d.gx, d.gy, d.strip);
  RUN(Compare("twelve 4K frames", std::vector<Frame>(12, Rgb8(3840, 2160)), 0));
  d = fp::RowsGrid(60, 135, 12);
  EXPECT(d.gx == 8 && d.strip == 128 && d.gy == 17, "twelve 4K frames: grid %u x %u, strip %u", d.gx, d.gy, d.strip);
  RUN(Compare("640 4K frames", std::vector<Frame>(640, Rgb8(3840, 2160)), 0, &plan));
  EXPECT(plan.groups.size() == 1 && plan.groups[0].first == 0 && plan.groups[0].count == 640, "640 4K frames: one group");
  d = fp::RowsGrid(60, 135, 640);
  EXPECT(d.gx == 8 && d.strip == 128 && d.gy == 17, "640 4K frames: grid %u x %u, strip %u", d.gx, d.gy, d.strip);
  return 0;
}

// All eight (gab, epf) forms, twice over and out of order, with grey and tensor frames between them; unequal sizes, a
// 1 x 1 frame, a band of one row, an epf count beyond 3 and one below 0.
static int TestMixed() {
  std::vector<Frame> frames;
  const uint32_t xs[] = {520, 1, 64, 65, 3840, 121, 480, 1000}, ys[] = {300, 1, 16, 17, 2160, 33, 481, 7};
  for (int round = 0; round < 2; round++)
    for (int k = 0; k < 8; k++) {
      const int form = round ? k : 7 - k;  // (descending first: the sort has work to do, and equal keys must keep their order)
      Frame f = Rgb8(xs[(k + 3 * round) % 8], ys[(k + 5 * round) % 8], form & 3, (form & 4) != 0);
      if (round && k == 2) f.c.epf_iters = 7;   // counts as 3
      if (round && k == 5) f.c.epf_iters = -2;  // counts as 0
      frames.push_back(f);
      if (k % 3 == 1) {  // a grey frame of the row kernel's forms
        Frame g = Rgb8(200 + 7 * k, 90 + k, 1 + (k & 1), (k & 2) != 0);
        g.c.gray8_fast = true;
        frames.push_back(g);
      }
      if (k % 3 == 2) {  // a tensor frame: no pixel buffer of the context's own
        Frame t = Rgb8(300 + 11 * k, 50 + 3 * k, 1 + (k & 1), (k & 4) != 0);
        t.c.tensor_fused = true;
        t.b.f.rgb = false;
        frames.push_back(t);
      }
    }
  Frame band = Rgb8(777, 500, 2, true);  // a band of one row in the middle of a frame
  band.c.band_y0 = 250;
  band.c.band_y1 = 251;
  frames.push_back(band);
  fp::FilterPlan plan;
  RUN(Compare("mixed forms", frames, 0, &plan));
  EXPECT(plan.groups.size() > 8, "mixed forms: %zu groups", plan.groups.size());
  for (size_t i = 1; i < plan.groups.size(); i++)
    EXPECT(plan.groups[i - 1].form.Key() < plan.groups[i].form.Key() && plan.groups[i].first == plan.groups[i - 1].first + plan.groups[i - 1].count,
           "mixed forms: group %zu follows group %zu", i, i - 1);
  RUN(Compare("a 1 x 1 frame", {Rgb8(1, 1, 0, false)}, 0, &plan));
  EXPECT(plan.groups[0].tiles_x == 1 && plan.groups[0].tiles_y == 1, "a 1 x 1 frame: tiles");
  return 0;
}

static int TestU8Srgb() {
  // every way a single frame clears the group's u8srgb, in the middle of the group
  for (int way = 0; way < 4; way++) {
    std::vector<Frame> frames(5, Rgb8(520, 300));
    before::Block& b = frames[2].b;
    if (way == 0) b.f.rgb = false;
    if (way == 1) b.f.rgbf = true;
    if (way == 2) b.filtered = true;
    if (way == 3) b.f.linear_output = 1;
    frames.push_back(Rgb8(520, 300, 2));  // (another group keeps its own)
    fp::FilterPlan plan;
    RUN(Compare(("u8srgb cleared, way " + std::to_string(way)).c_str(), frames, 0, &plan));
    EXPECT(plan.groups.size() == 2 && !plan.groups[0].u8srgb && plan.groups[1].u8srgb, "u8srgb cleared, way %d", way);
  }
  // a grey group that one frame clears is refused, wherever the frame stands; a grey group that none clears is not
  for (size_t at = 0; at < 3; at++) {
    std::vector<Frame> grey(3, Rgb8(520, 300));
    for (Frame& f : grey) f.c.gray8_fast = true;
    RUN(Compare("grey frames", grey, 0));
    grey[at].b.f.linear_output = 1;
    grey.insert(grey.begin(), Rgb8(64, 64));
    RUN(Compare("a grey frame in a group without u8srgb", grey, JXLHIP_ERR_INVALID_ARGUMENT));
  }
  return 0;
}

static int TestEmpty() {
  fp::FilterPlan plan;
  RUN(Compare("no frames", {}, 0, &plan));
  EXPECT(plan.order.empty() && plan.groups.empty(), "no frames");
  Frame f = Rgb8(520, 300);
  f.c.band_y0 = f.c.band_y1 = 120;  // an empty band: no tiles down, no strips
  RUN(Compare("an empty band", {f, Rgb8(520, 300, 3)}, 0, &plan));
  EXPECT(plan.groups.size() == 2 && plan.groups[0].tiles_x == 9 && plan.groups[0].tiles_y == 0, "an empty band: tiles %u x %u", plan.groups[0].tiles_x,
         plan.groups[0].tiles_y);
  const fp::RowsGridDims d = fp::RowsGrid(9, 0, 1);
  EXPECT(d.gx == 2 && d.gy == 0 && d.strip == 64, "an empty band: grid %u x %u, strip %u", d.gx, d.gy, d.strip);
  return 0;
}

// The kernel of every form: the row kernel takes 1 and 2 iterations, the tile kernel 0 and 3 without the grey and tensor writers.
static int TestKernelOf() {
  for (int key = 0; key < 32; key++) {
    const fp::FilterForm f = fp::FormOf(key & 3, (key & 4) != 0, (key & 8) != 0, (key & 16) != 0);
    EXPECT(f.Key() == key, "key %d", key);
    const int epf = key & 3;
    const fp::FilterKernel want = (epf == 1 || epf == 2) ? fp::kRowsKernel : ((key & 24) ? fp::kNoKernel : fp::kFusedKernel);
    EXPECT(fp::KernelOf(f) == want, "key %d: kernel %d", key, int(fp::KernelOf(f)));
  }
  return 0;
}

int main() {
  RUN(Test4K());
  RUN(TestMixed());
  RUN(TestU8Srgb());
  RUN(TestEmpty());
  RUN(TestKernelOf());
  printf("filter plan kats passed\n");
  return 0;
}
