// Known-answer tests of libjxl_amd/csrc/host/jxh_window_plan.h (the host plan of a region decode), built with
// AddressSanitizer + UBSan and run as a child process by tests/test_region_host.py:
//  * every WholeFrameReason is raised once, by the one trait that raises it;
//  * every DcWindowRule and every WindowRule refuses the one change that breaks it, and names itself;
//  * PlanWindow on a 1000 x 700 frame (4 x 3 groups, ragged last column and row): the filters' halo decides at the pixel
//    which group columns and rows a box takes, on both sides; H = 0; a one-pixel box; the ragged corner; the whole image;
//    all eight orientations on this non-square frame (the box mapped into the frame and back is the box, and a marked
//    pixel lands where the writer's rule puts it); sums near 2^32;
//  * BuildWindowDesc on a synthetic descriptor of that frame: the result passes CheckFrameDesc (jxh_upload_plan.h) as it
//    is, block ranges tile, every varblock lies inside its window group, and the gathered sections are the chosen groups'
//    for every pass; cropped planes are the frame's;
//  * PlanDcApron / PackDcApron into a heap block of exactly the apron's size (ASan watches).
// Prints "reasons: ...", "dc_rules: ..." and "window_rules: ..." for the Python side to hold against the header's enums.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "../../libjxl_amd/csrc/host/jxh_upload_plan.h"
#include "../../libjxl_amd/csrc/host/jxh_window_plan.h"

using namespace jxlhip::window;
namespace up = jxlhip::upload;

static int g_failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      g_failures++;                                                    \
    }                                                                  \
  } while (0)

// ------------------------------------------------------------------------------------------------ reasons
static const char* const kReasonNames[] = {"Windowed", "Partial",        "Upsampling", "Subsampling", "Noise",         "Patches",
                                           "Splines",  "DcFrame",        "Alpha",      "SingleSection", "OneGroup", "WindowIsFrame"};
static_assert(sizeof(kReasonNames) / sizeof(kReasonNames[0]) == kWholeReasonCount, "a name for every reason");

static void Reasons() {
  const FrameGeom g = GeomOf(1000, 700);
  WindowPlan inner, all, one;
  EXPECT(PlanWindow(g, 1, 1, 0, Rect{300, 300, 100, 100}, &inner) == 0);
  EXPECT(PlanWindow(g, 1, 1, 0, Rect{0, 0, 0, 0}, &all) == 0);
  EXPECT(PlanWindow(GeomOf(200, 100), 1, 1, 0, Rect{3, 3, 10, 10}, &one) == 0);
  FrameTraits none;
  memset(&none, 0, sizeof(none));
  none.upsampling = 1;
  none.num_channels = 3;
  std::set<std::string> raised;
  auto raise = [&](FrameTraits t, const WindowPlan& w, WholeFrameReason want) {
    const WholeFrameReason got = WholeFrameReasonOf(t, w);
    if (got != want) {
      printf("FAILED: reason %s, expected %s\n", kReasonNames[got], kReasonNames[want]);
      g_failures++;
    }
    raised.insert(kReasonNames[want]);
  };
  raise(none, inner, kWindowed);
  FrameTraits t = none;
  t.partial = true;
  raise(t, inner, kWholePartial);
  t = none;
  t.upsampling = 2;
  raise(t, inner, kWholeUpsampling);
  t = none;
  t.subsampled = true;
  raise(t, inner, kWholeSubsampling);
  t = none;
  t.noise = true;
  raise(t, inner, kWholeNoise);
  t = none;
  t.patches = true;
  raise(t, inner, kWholePatches);
  t = none;
  t.splines = true;
  raise(t, inner, kWholeSplines);
  t = none;
  t.dc_frame = true;
  raise(t, inner, kWholeDcFrame);
  for (uint32_t nc : {2u, 4u}) {
    t = none;
    t.num_channels = nc;
    raise(t, inner, kWholeAlpha);
  }
  t = none;
  t.num_channels = 1;
  raise(t, inner, kWindowed);
  t = none;
  t.single_section = true;
  raise(t, one, kWholeSingleSection);
  raise(none, one, kWholeOneGroup);
  raise(none, all, kWholeWindowIsFrame);
  printf("reasons:");
  for (const std::string& s : raised) printf(" %s", s.c_str());
  printf("\n");
}

// ------------------------------------------------------------------------------------------------ PlanWindow
static WindowPlan Plan(const FrameGeom& g, int gab, int epf, uint32_t bits, Rect box) {
  WindowPlan w;
  memset(&w, 0xEE, sizeof(w));
  const int r = PlanWindow(g, gab, epf, bits, box, &w);
  if (r) {
    printf("FAILED: PlanWindow refused a good box\n");
    g_failures++;
  }
  return w;
}
static const char* const kWindowRuleNames[] = {"Frame", "BoxExtents", "BoxInside"};
static_assert(sizeof(kWindowRuleNames) / sizeof(kWindowRuleNames[0]) == kWindowRuleCount, "a name for every rule");
static std::set<std::string> g_window_rules;
static void BoxRefused(const FrameGeom& g, uint32_t bits, Rect box, int want, int line) {
  WindowPlan w;
  int rule = -1;
  const int r = PlanWindow(g, 1, 3, bits, box, &w, &rule);
  if (r != JXLHIP_ERR_INVALID_ARGUMENT || rule != want) {
    printf("FAILED line %d: code %d rule %d, expected %s\n", line, r, rule, kWindowRuleNames[want]);
    g_failures++;
  }
  EXPECT(PlanWindow(g, 1, 3, bits, box, &w) == r);
  g_window_rules.insert(kWindowRuleNames[want]);
}

static void Windows() {
  const FrameGeom g = GeomOf(1000, 700);
  EXPECT(g.xsize_groups == 4 && g.ysize_groups == 3 && g.xsize_blocks == 125 && g.ysize_blocks == 88);
  EXPECT(jxlhip::FusedHalo(true, 3) == 7 && jxlhip::FusedHalo(false, 0) == 0 && jxlhip::FusedHalo(false, 1) == 2 &&
         jxlhip::FusedHalo(true, 2) == 4);
  // H = 7: the near side, columns then rows
  WindowPlan w = Plan(g, 1, 3, 0, Rect{256 + 6, 300, 100, 100});
  EXPECT(w.gx0 == 0 && w.gxs == 2 && w.gy0 == 1 && w.gys == 1);
  EXPECT((w.pixels == Rect{0, 256, 512, 256}) && (w.blocks == Rect{0, 32, 64, 32}) && (w.box == Rect{262, 44, 100, 100}));
  EXPECT(w.groups_taken == 2 && w.groups_in_frame == 12);
  w = Plan(g, 1, 3, 0, Rect{256 + 7, 300, 100, 100});
  EXPECT(w.gx0 == 1 && w.gxs == 1 && (w.box == Rect{7, 44, 100, 100}) && w.groups_taken == 1);
  w = Plan(g, 1, 3, 0, Rect{300, 256 + 6, 100, 100});
  EXPECT(w.gy0 == 0 && w.gys == 2 && w.gx0 == 1 && w.gxs == 1);
  w = Plan(g, 1, 3, 0, Rect{300, 256 + 7, 100, 100});
  EXPECT(w.gy0 == 1 && w.gys == 1);
  // ... and the far side: a box that ends at 512 - 7 stays in column 1, one that ends at 512 - 6 takes column 2
  w = Plan(g, 1, 3, 0, Rect{300, 300, 512 - 7 - 300, 50});
  EXPECT(w.gx0 == 1 && w.gxs == 1);
  w = Plan(g, 1, 3, 0, Rect{300, 300, 512 - 6 - 300, 50});
  EXPECT(w.gx0 == 1 && w.gxs == 2 && (w.pixels == Rect{256, 256, 512, 256}));
  w = Plan(g, 1, 3, 0, Rect{300, 300, 50, 512 - 7 - 300});
  EXPECT(w.gy0 == 1 && w.gys == 1);
  w = Plan(g, 1, 3, 0, Rect{300, 300, 50, 512 - 6 - 300});
  EXPECT(w.gy0 == 1 && w.gys == 2 && (w.pixels == Rect{256, 256, 256, 444}) && (w.blocks == Rect{32, 32, 32, 56}));
  // epf 1 without Gaborish: H = 2
  w = Plan(g, 0, 1, 0, Rect{256 + 1, 300, 10, 10});
  EXPECT(w.gx0 == 0 && w.gxs == 2);
  w = Plan(g, 0, 1, 0, Rect{256 + 2, 300, 10, 10});
  EXPECT(w.gx0 == 1 && w.gxs == 1);
  // H = 0: exactly the groups the box touches
  w = Plan(g, 0, 0, 0, Rect{256, 256, 256, 256});
  EXPECT(w.groups_taken == 1 && (w.pixels == Rect{256, 256, 256, 256}) && (w.box == Rect{0, 0, 256, 256}));
  w = Plan(g, 0, 0, 0, Rect{255, 256, 258, 256});
  EXPECT(w.gx0 == 0 && w.gxs == 3 && w.gys == 1);
  // one pixel
  w = Plan(g, 1, 3, 0, Rect{600, 400, 1, 1});
  EXPECT(w.groups_taken == 1 && w.gx0 == 2 && w.gy0 == 1 && (w.box == Rect{88, 144, 1, 1}));
  w = Plan(g, 1, 3, 0, Rect{0, 0, 1, 1});
  EXPECT(w.groups_taken == 1 && (w.need == Rect{0, 0, 8, 8}));
  // the ragged corner: the last column ends at 1000, the last row at 700
  w = Plan(g, 1, 3, 0, Rect{990, 690, 10, 10});
  EXPECT(w.gx0 == 3 && w.gy0 == 2 && (w.pixels == Rect{768, 512, 232, 188}) && (w.blocks == Rect{96, 64, 29, 24}) && (w.box == Rect{222, 178, 10, 10}));
  EXPECT((w.need == Rect{983, 683, 17, 17}));
  // the whole image, stated or all zero
  for (Rect box : {Rect{0, 0, 1000, 700}, Rect{0, 0, 0, 0}}) {
    w = Plan(g, 1, 3, 0, box);
    EXPECT(w.groups_taken == 12 && (w.pixels == Rect{0, 0, 1000, 700}) && (w.blocks == Rect{0, 0, 125, 88}) && (w.box == Rect{0, 0, 1000, 700}));
  }
  // all eight orientations: the box mapped into the frame and back is the box; a marked pixel goes where the writer's rule
  // (PixelOutIndex) sends it, in the frame and in the window image alike
  for (uint32_t orientation = 1; orientation <= 8; orientation++) {
    const uint32_t bits = OrientBits(orientation);
    const bool tr = (bits & 4) != 0;
    const uint32_t iw = tr ? 700 : 1000, ih = tr ? 1000 : 700;
    for (Rect box : {Rect{40, 300, 100, 37}, Rect{0, 0, 1, 1}, Rect{iw - 3, ih - 2, 3, 2}, Rect{0, 0, iw, ih}}) {
      const Rect f = FromOriented(box, 1000, 700, bits);
      EXPECT(f.x0 + f.xsize <= 1000 && f.y0 + f.ysize <= 700);
      EXPECT(ToOriented(f, 1000, 700, bits) == box);
      w = Plan(g, 1, 3, bits, box);
      // the first pixel of the box in the oriented window image is the pixel of the frame that the writer sends there
      const uint32_t wx = w.pixels.xsize, wy = w.pixels.ysize;
      const uint32_t u = w.box.x0, v = w.box.y0;                       // column, row in the window image
      const uint32_t ox = tr ? v : u, oy = tr ? u : v;
      const uint32_t x = (bits & 1) ? wx - 1 - ox : ox, y = (bits & 2) ? wy - 1 - oy : oy;  // in the window
      const uint32_t fu = box.x0, fv = box.y0;
      const uint32_t fox = tr ? fv : fu, foy = tr ? fu : fv;
      const uint32_t fx = (bits & 1) ? 1000 - 1 - fox : fox, fy = (bits & 2) ? 700 - 1 - foy : foy;  // in the frame
      EXPECT(x + w.pixels.x0 == fx && y + w.pixels.y0 == fy);
      EXPECT(w.box.xsize == box.xsize && w.box.ysize == box.ysize);
      EXPECT(w.box.x0 + w.box.xsize <= (tr ? wy : wx) && w.box.y0 + w.box.ysize <= (tr ? wx : wy));
    }
  }
  EXPECT(OrientBits(1) == 0 && OrientBits(2) == 1 && OrientBits(3) == 3 && OrientBits(4) == 2 && OrientBits(5) == 4 && OrientBits(6) == 6 &&
         OrientBits(7) == 7 && OrientBits(8) == 5 && OrientBits(0) == 0);
  // a 3840 x 2160 frame: any 224 x 224 box takes at most 4 of 135 groups (224 + 2 * 7 <= 256)
  const FrameGeom k4 = GeomOf(3840, 2160);
  uint32_t most = 0;
  for (uint32_t y = 0; y + 224 <= 2160; y += 7)
    for (uint32_t x = 0; x + 224 <= 3840; x += 5) {
      PlanWindow(k4, 1, 3, 0, Rect{x, y, 224, 224}, &w);
      most = most > w.groups_taken ? most : w.groups_taken;
    }
  EXPECT(most == 4 && w.groups_in_frame == 135);
  // refusals: CheckResizedOut's, with its 64-bit sums
  BoxRefused(g, 0, Rect{0, 0, 10, 0}, kWindowRuleBoxExtents, __LINE__);
  BoxRefused(g, 0, Rect{0, 0, 0, 10}, kWindowRuleBoxExtents, __LINE__);
  BoxRefused(g, 0, Rect{1, 0, 0, 0}, kWindowRuleBoxExtents, __LINE__);
  BoxRefused(g, 0, Rect{991, 0, 10, 10}, kWindowRuleBoxInside, __LINE__);
  BoxRefused(g, 0, Rect{0, 691, 10, 10}, kWindowRuleBoxInside, __LINE__);
  BoxRefused(g, 6, Rect{691, 0, 10, 10}, kWindowRuleBoxInside, __LINE__);  // (transposed: the image is 700 wide)
  EXPECT(PlanWindow(g, 1, 3, 6, Rect{690, 990, 10, 10}, &w) == 0);
  BoxRefused(g, 0, Rect{0xFFFFFFF0u, 0, 0x20, 10}, kWindowRuleBoxInside, __LINE__);  // (the 32-bit sum would be 0x10)
  BoxRefused(g, 0, Rect{0, 0xFFFFFFFFu, 10, 1}, kWindowRuleBoxInside, __LINE__);
  BoxRefused(g, 0, Rect{0x80000000u, 0, 0x80000000u, 1}, kWindowRuleBoxInside, __LINE__);
  FrameGeom bad = g;
  bad.xsize_groups = 5;
  BoxRefused(bad, 0, Rect{0, 0, 10, 10}, kWindowRuleFrame, __LINE__);
  bad = g;
  bad.ysize = 0;
  BoxRefused(bad, 0, Rect{0, 0, 10, 10}, kWindowRuleFrame, __LINE__);
  printf("window_rules:");
  for (const std::string& s : g_window_rules) printf(" %s", s.c_str());
  printf("\n");
}

// ------------------------------------------------------------------------------------------------ CheckDcWindow
static const char* const kDcRuleNames[] = {"Window", "Apron", "Planes", "Steps", "Size", "Precision"};
static_assert(sizeof(kDcRuleNames) / sizeof(kDcRuleNames[0]) == kDcWindowRuleCount, "a name for every rule");
static std::set<std::string> g_dc_rules;

static JxlHipDcWindow GoodDc(uint32_t fxs, uint32_t fys, Rect win) {
  JxlHipDcWindow d;
  memset(&d, 0, sizeof(d));
  d.frame_xsize_blocks = fxs;
  d.frame_ysize_blocks = fys;
  d.win_x0 = win.x0; d.win_y0 = win.y0; d.win_xsize = win.xsize; d.win_ysize = win.ysize;
  const Rect a = PlanDcApron(win, fxs, fys);
  d.apron_x0 = a.x0; d.apron_y0 = a.y0; d.apron_xsize = a.xsize; d.apron_ysize = a.ysize;
  d.apron = reinterpret_cast<const int32_t*>(uintptr_t(0x10000));               // (never dereferenced: the check is pure)
  d.dc_extra_precision = reinterpret_cast<const uint8_t*>(uintptr_t(0x20000));
  d.num_dc_groups = ((fxs + 255) / 256) * ((fys + 255) / 256);
  d.dc_step[0] = 0.001f; d.dc_step[1] = 0.002f; d.dc_step[2] = 0.004f;
  d.dc_cfl_b = 1.0f;
  d.dc_smoothing = 1;
  return d;
}
static void DcRefused(const JxlHipDcWindow& d, int want, int line) {
  int rule = -1;
  const int r = CheckDcWindow(d, &rule);
  if (r != JXLHIP_ERR_INVALID_ARGUMENT || rule != want) {
    printf("FAILED line %d: code %d rule %d, expected %s\n", line, r, rule, kDcRuleNames[want]);
    g_failures++;
  }
  EXPECT(CheckDcWindow(d) == r);
  g_dc_rules.insert(kDcRuleNames[want]);
}
#define DC_REFUSED(d, rule) DcRefused(d, rule, __LINE__)

static void DcRules() {
  EXPECT((PlanDcApron(Rect{32, 32, 32, 32}, 125, 88) == Rect{31, 31, 34, 34}));
  EXPECT((PlanDcApron(Rect{0, 0, 32, 32}, 125, 88) == Rect{0, 0, 33, 33}));
  EXPECT((PlanDcApron(Rect{96, 64, 29, 24}, 125, 88) == Rect{95, 63, 30, 25}));
  EXPECT((PlanDcApron(Rect{0, 0, 125, 88}, 125, 88) == Rect{0, 0, 125, 88}));
  EXPECT((PlanDcApron(Rect{0, 0, 1, 1}, 1, 1) == Rect{0, 0, 1, 1}));
  for (Rect win : {Rect{32, 2, 32, 8}, Rect{0, 0, 1, 1}, Rect{259, 11, 1, 1}, Rect{250, 2, 10, 9}, Rect{0, 0, 260, 12}})
    EXPECT(CheckDcWindow(GoodDc(260, 12, win)) == 0);
  JxlHipDcWindow d = GoodDc(260, 12, Rect{10, 2, 3, 3});
  d.win_xsize = 0;
  DC_REFUSED(d, kDcWindowRuleWindow);
  d = GoodDc(260, 12, Rect{10, 2, 3, 3});
  d.win_ysize = 0;
  DC_REFUSED(d, kDcWindowRuleWindow);
  d = GoodDc(260, 12, Rect{10, 2, 3, 3});
  d.win_x0 = 258;  // 258 + 3 > 260
  DC_REFUSED(d, kDcWindowRuleWindow);
  d.win_x0 = 0xFFFFFFFEu;  // (the 32-bit sum would be 1)
  DC_REFUSED(d, kDcWindowRuleWindow);
  d = GoodDc(260, 12, Rect{10, 2, 3, 3});
  d.win_y0 = 10;
  DC_REFUSED(d, kDcWindowRuleWindow);
  d = GoodDc(260, 12, Rect{10, 2, 3, 3});
  d.frame_xsize_blocks = (1u << 27) + 1;
  DC_REFUSED(d, kDcWindowRuleWindow);
  // the apron: each of its four numbers off by one, and one that leaves the frame
  for (int field = 0; field < 4; field++)
    for (int delta : {-1, 1}) {
      d = GoodDc(260, 12, Rect{10, 2, 3, 3});
      uint32_t* p[4] = {&d.apron_x0, &d.apron_y0, &d.apron_xsize, &d.apron_ysize};
      *p[field] += uint32_t(delta);
      DC_REFUSED(d, kDcWindowRuleApron);
    }
  d = GoodDc(260, 12, Rect{250, 2, 10, 10});
  d.apron_xsize += 1;  // (one column beyond the frame)
  DC_REFUSED(d, kDcWindowRuleApron);
  d = GoodDc(260, 12, Rect{10, 2, 3, 3});
  d.apron = nullptr;
  DC_REFUSED(d, kDcWindowRulePlanes);
  for (int c = 0; c < 3; c++)
    for (float v : {0.0f, -1.0f, float(NAN), float(INFINITY)}) {
      d = GoodDc(260, 12, Rect{10, 2, 3, 3});
      d.dc_step[c] = v;
      DC_REFUSED(d, kDcWindowRuleSteps);
    }
  // precision bytes: a window in the second DC group needs two entries; one in the first needs one; none at all serves a
  // frame of one DC group only
  d = GoodDc(260, 12, Rect{257, 2, 3, 3});
  d.num_dc_groups = 1;
  DC_REFUSED(d, kDcWindowRulePrecision);
  d = GoodDc(260, 12, Rect{254, 2, 2, 3});  // (its apron reaches column 256)
  d.num_dc_groups = 1;
  DC_REFUSED(d, kDcWindowRulePrecision);
  d = GoodDc(260, 12, Rect{10, 2, 3, 3});
  d.num_dc_groups = 1;
  EXPECT(CheckDcWindow(d) == 0);
  d.num_dc_groups = 0;
  DC_REFUSED(d, kDcWindowRulePrecision);
  d.dc_extra_precision = nullptr;
  DC_REFUSED(d, kDcWindowRulePrecision);
  d = GoodDc(256, 256, Rect{10, 2, 3, 3});
  d.dc_extra_precision = nullptr;
  d.num_dc_groups = 0;
  EXPECT(CheckDcWindow(d) == 0);
  d = GoodDc(520, 300, Rect{515, 280, 3, 3});  // the last of 3 x 2 DC groups
  EXPECT(CheckDcWindow(d) == 0);
  d.num_dc_groups = 5;
  DC_REFUSED(d, kDcWindowRulePrecision);
  // size: 4094 x 4094 + apron = 4096 x 4096 = 2^24 passes, one more row does not
  d = GoodDc(8000, 8000, Rect{1, 1, 4094, 4094});
  EXPECT(CheckDcWindow(d) == 0);
  d = GoodDc(8000, 8000, Rect{1, 1, 4094, 4095});
  DC_REFUSED(d, kDcWindowRuleSize);
  d = GoodDc(1u << 27, 1u << 27, Rect{0, 0, 1u << 27, 1u << 27});
  DC_REFUSED(d, kDcWindowRuleSize);
  printf("dc_rules:");
  for (const std::string& s : g_dc_rules) printf(" %s", s.c_str());
  printf("\n");
  // the pack, into a block of exactly the apron's size
  const uint32_t fxs = 125, fys = 88;
  std::vector<int32_t> q(size_t(3) * fxs * fys);
  for (size_t i = 0; i < q.size(); i++) q[i] = int32_t((uint32_t(i) * 2654435761u) >> 8) - (1 << 22);
  for (Rect win : {Rect{32, 32, 32, 32}, Rect{0, 0, 32, 32}, Rect{96, 64, 29, 24}, Rect{0, 0, 125, 88}, Rect{124, 87, 1, 1}}) {
    const Rect a = PlanDcApron(win, fxs, fys);
    int32_t* block = static_cast<int32_t*>(malloc(size_t(3) * a.xsize * a.ysize * 4));
    PackDcApron(q.data(), fxs, fys, a, block);
    bool same = true;
    for (uint32_t c = 0; c < 3; c++)
      for (uint32_t y = 0; y < a.ysize; y++)
        for (uint32_t x = 0; x < a.xsize; x++)
          same = same && block[(size_t(c) * a.ysize + y) * a.xsize + x] == q[(size_t(c) * fys + a.y0 + y) * fxs + a.x0 + x];
    EXPECT(same);
    free(block);
  }
}

// ------------------------------------------------------------------------------------------------ BuildWindowDesc
// A descriptor of a 1000 x 700 frame that CheckFrameDesc takes: two passes, every group filled with 2 x 2-block DCT16
// varblocks where they fit and single blocks elsewhere, tables of the smallest legal size.
struct Synth {
  JxlHipFrameDesc d;
  std::vector<JxlHipVarBlock> blocks;
  std::vector<uint32_t> gbb, section_size;
  std::vector<uint64_t> section_offset;
  std::vector<uint8_t> ctx_map, lut, sharpness;
  std::vector<int8_t> ytox, ytob;
  std::vector<uint32_t> cfg;
  std::vector<JxlHipPassDesc> passes;
  std::vector<float> dequant;
};
static void MakeSynth(Synth* s) {
  JxlHipFrameDesc& d = s->d;
  memset(&d, 0, sizeof(d));
  const FrameGeom g = GeomOf(1000, 700);
  d.xsize = g.xsize; d.ysize = g.ysize; d.xsize_blocks = g.xsize_blocks; d.ysize_blocks = g.ysize_blocks;
  d.xsize_groups = g.xsize_groups; d.num_groups = g.xsize_groups * g.ysize_groups;
  d.num_passes = 2;
  d.coef_bits = 16;
  d.codestream = reinterpret_cast<const uint8_t*>(uintptr_t(0x100000));
  for (uint32_t p = 0; p < d.num_passes; p++)
    for (uint32_t grp = 0; grp < d.num_groups; grp++) {
      s->section_offset.push_back(1000 + 5000ull * (p * d.num_groups + grp));
      s->section_size.push_back(100 + 7 * grp + 1000 * p);
    }
  d.section_offset = s->section_offset.data();
  d.section_size = s->section_size.data();
  s->gbb.push_back(0);
  for (uint32_t grp = 0; grp < d.num_groups; grp++) {
    const uint32_t gx0 = (grp % d.xsize_groups) * 32, gy0 = (grp / d.xsize_groups) * 32;
    const uint32_t gw = std::min(32u, d.xsize_blocks - gx0), gh = std::min(32u, d.ysize_blocks - gy0);
    std::vector<uint8_t> taken(size_t(gw) * gh, 0);
    uint32_t off = 0;
    for (uint32_t y = 0; y < gh; y++)
      for (uint32_t x = 0; x < gw; x++) {
        if (taken[y * gw + x]) continue;
        const bool big = x % 4 == 0 && y % 4 == 0 && x + 2 <= gw && y + 2 <= gh;
        JxlHipVarBlock v;
        v.bx = uint16_t(gx0 + x);
        v.by = uint16_t(gy0 + y);
        v.strategy = big ? 4 : 0;
        v.quant_dc_ctx = 0;
        v.qf = uint16_t(1 + (grp * 31 + x + 32 * y) % 256);
        v.coef_offset = off;
        const uint32_t n = big ? 2 : 1;
        for (uint32_t iy = 0; iy < n; iy++)
          for (uint32_t ix = 0; ix < n; ix++) taken[(y + iy) * gw + x + ix] = 1;
        off += 64 * n * n;
        s->blocks.push_back(v);
      }
    s->gbb.push_back(uint32_t(s->blocks.size()));
  }
  d.blocks = s->blocks.data();
  d.num_blocks = uint32_t(s->blocks.size());
  d.group_block_begin = s->gbb.data();
  d.num_block_ctxs = 1;
  d.num_dc_ctxs = 1;
  d.num_histograms = 1;
  s->lut.assign(3 * 13, 0);
  d.block_ctx_lut = s->lut.data();
  d.block_ctx_lut_size = uint32_t(s->lut.size());
  s->ctx_map.assign(495 + 16, 0);
  s->cfg.assign(1, 0);
  s->passes.resize(d.num_passes);
  for (JxlHipPassDesc& p : s->passes) {
    memset(&p, 0, sizeof(p));
    p.log_alpha = 5;
    p.num_clusters = 1;
    p.ctx_map = s->ctx_map.data();
    p.ctx_map_size = uint32_t(s->ctx_map.size());
    p.uint_cfg = s->cfg.data();
  }
  d.passes = s->passes.data();
  uint32_t at = 0;
  for (uint32_t st = 0; st < 27; st++) {
    const uint32_t k = jxlhip::kStrategyQuantTable[st];
    if (d.dequant_size[k]) continue;
    d.dequant_size[k] = 64 * jxlhip::CoveredBlocks(st);
    d.dequant_offset[k] = at;
    at += 3 * d.dequant_size[k];
  }
  s->dequant.assign(at, 1.0f);
  d.dequant = s->dequant.data();
  d.dequant_floats = at;
  s->sharpness.resize(size_t(d.xsize_blocks) * d.ysize_blocks);
  for (size_t i = 0; i < s->sharpness.size(); i++) s->sharpness[i] = uint8_t((i * 7 + i / d.xsize_blocks) & 7);
  d.sharpness = s->sharpness.data();
  const uint32_t tx = (d.xsize_blocks + 7) / 8, ty = (d.ysize_blocks + 7) / 8;
  s->ytox.resize(size_t(tx) * ty);
  s->ytob.resize(size_t(tx) * ty);
  for (size_t i = 0; i < s->ytox.size(); i++) {
    s->ytox[i] = int8_t(i * 5 - 60);
    s->ytob[i] = int8_t(90 - i * 3);
  }
  d.ytox = s->ytox.data();
  d.ytob = s->ytob.data();
  d.dc_quantised = reinterpret_cast<const int32_t*>(uintptr_t(0x200000));
  d.dc_smoothing = 1;
  d.dc_step[0] = d.dc_step[1] = d.dc_step[2] = 0.01f;
  d.quant_scale = 0.5f;
  d.epf_quant_mul = 0.46f;
  d.gab = 1;
  d.epf_iters = 3;
  d.inv_global_scale = 1.0f;
}

static void WindowDescs() {
  Synth s;
  MakeSynth(&s);
  const JxlHipFrameDesc& whole = s.d;
  up::UploadOptions opt;
  up::Rule rule = up::kNumRules;
  EXPECT(up::CheckFrameDesc(whole, opt, &rule) == 0);
  if (rule != up::kNumRules) printf("  (the synthetic frame itself is refused by rule %d)\n", int(rule));
  const FrameGeom g = GeomOf(whole.xsize, whole.ysize);
  const float* planes = reinterpret_cast<const float*>(uintptr_t(0x300000));
  for (Rect box : {Rect{300, 300, 100, 100}, Rect{256 + 6, 300, 100, 100}, Rect{990, 690, 10, 10}, Rect{200, 200, 400, 400}, Rect{0, 0, 1, 1},
                   Rect{700, 10, 290, 300}}) {
    const WindowPlan w = Plan(g, whole.gab, whole.epf_iters, 0, box);
    WindowTables t;
    JxlHipFrameDesc d;
    BuildWindowDesc(whole, w, planes, &t, &d);
    rule = up::kNumRules;
    const int r = up::CheckFrameDesc(d, opt, &rule);
    if (r) {
      printf("FAILED: the window of box %u %u is refused by rule %d\n", box.x0, box.y0, int(rule));
      g_failures++;
      continue;
    }
    EXPECT(d.xsize == w.pixels.xsize && d.ysize == w.pixels.ysize && d.xsize_blocks == w.blocks.xsize && d.ysize_blocks == w.blocks.ysize);
    EXPECT(d.xsize_groups == w.gxs && d.num_groups == w.groups_taken && d.num_passes == whole.num_passes);
    EXPECT(d.dc_device == planes && !d.dc_quantised && !d.dc && d.dc_smoothing == 0 && !d.group_absent);
    EXPECT(d.passes == whole.passes && d.dequant == whole.dequant && d.block_ctx_lut == whole.block_ctx_lut && d.codestream == whole.codestream);
    EXPECT(d.gab == whole.gab && d.epf_iters == whole.epf_iters);
    // block ranges tile; every varblock inside its window group; fields but the position unchanged
    EXPECT(d.group_block_begin[0] == 0 && d.group_block_begin[d.num_groups] == d.num_blocks);
    for (uint32_t i = 0; i < d.num_groups; i++) {
      const uint32_t grp = FrameGroupOf(w, whole.xsize_groups, i);
      EXPECT(grp == (w.gy0 + i / w.gxs) * 4 + w.gx0 + i % w.gxs);
      const uint32_t n = whole.group_block_begin[grp + 1] - whole.group_block_begin[grp];
      EXPECT(d.group_block_begin[i + 1] - d.group_block_begin[i] == n);
      const uint32_t gx0 = (i % d.xsize_groups) * 32, gy0 = (i / d.xsize_groups) * 32;
      for (uint32_t k = 0; k < n; k++) {
        const JxlHipVarBlock& a = d.blocks[d.group_block_begin[i] + k];
        const JxlHipVarBlock& b = whole.blocks[whole.group_block_begin[grp] + k];
        const uint32_t cx = jxlhip::kCoveredX[a.strategy], cy = jxlhip::kCoveredY[a.strategy];
        EXPECT(a.bx >= gx0 && a.by >= gy0 && a.bx + cx <= gx0 + 32 && a.by + cy <= gy0 + 32 && a.bx + cx <= d.xsize_blocks && a.by + cy <= d.ysize_blocks);
        EXPECT(a.bx + w.blocks.x0 == b.bx && a.by + w.blocks.y0 == b.by);
        EXPECT(a.strategy == b.strategy && a.qf == b.qf && a.quant_dc_ctx == b.quant_dc_ctx && a.coef_offset == b.coef_offset);
      }
      for (uint32_t p = 0; p < d.num_passes; p++) {
        EXPECT(d.section_offset[p * d.num_groups + i] == whole.section_offset[p * whole.num_groups + grp]);
        EXPECT(d.section_size[p * d.num_groups + i] == whole.section_size[p * whole.num_groups + grp]);
      }
    }
    // cropped planes
    bool same = true;
    for (uint32_t y = 0; y < d.ysize_blocks; y++)
      for (uint32_t x = 0; x < d.xsize_blocks; x++)
        same = same && d.sharpness[size_t(y) * d.xsize_blocks + x] == whole.sharpness[size_t(y + w.blocks.y0) * whole.xsize_blocks + x + w.blocks.x0];
    const uint32_t tx = (d.xsize_blocks + 7) / 8, ty = (d.ysize_blocks + 7) / 8, ftx = (whole.xsize_blocks + 7) / 8;
    EXPECT(t.ytox.size() == size_t(tx) * ty && t.ytob.size() == t.ytox.size() && t.sharpness.size() == size_t(d.xsize_blocks) * d.ysize_blocks);
    for (uint32_t y = 0; y < ty; y++)
      for (uint32_t x = 0; x < tx; x++) {
        same = same && d.ytox[y * tx + x] == whole.ytox[(y + w.blocks.y0 / 8) * ftx + x + w.blocks.x0 / 8];
        same = same && d.ytob[y * tx + x] == whole.ytob[(y + w.blocks.y0 / 8) * ftx + x + w.blocks.x0 / 8];
      }
    EXPECT(same);
  }
}

int main() {
  Reasons();
  Windows();
  DcRules();
  WindowDescs();
  if (g_failures) {
    printf("%d check(s) failed\n", g_failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
