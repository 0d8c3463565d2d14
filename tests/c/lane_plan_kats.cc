// The launch plan of the batched lane kernel (libjxl_amd/csrc/host/jxh_lane_plan.h), held on the CPU. Built by
// tests/test_lane_plan.py as a stand-alone program with -fsanitize=address,undefined around libjxl_amd/csrc/api/jxl_api.cc
// (mode plan reads real streams through its parser; the HIP entry points are no-device doubles).
//   kats                          hand-made section tables: the rules of the header, each against a reading written here
//   plan FILE... --cus N [--lanes L] [--order O] [--galias G] [--a6 A]
//                                 what jxlhip_run_entropy_batch plans for these streams on a device of N CUs, as text
#include "../../libjxl_amd/csrc/api/jxl_api.cc"
#define KATS_OWN_FRAME_UPLOAD
#include "no_device_doubles.inc"
#include "../../libjxl_amd/csrc/host/jxh_lane_plan.h"
#include "../../libjxl_amd/csrc/host/jxh_upload_plan.h"

#include <map>
#include <memory>
#include <tuple>

namespace lp = jxh::lane_plan;
namespace up = jxlhip::upload;
using lp::LanePlan;

#define EXPECT(cond, ...)                                        \
  do {                                                           \
    if (!(cond)) {                                               \
      fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                              \
      fprintf(stderr, "\n");                                     \
      return 1;                                                  \
    }                                                            \
  } while (0)
#define RUN(call)       \
  do {                  \
    if (call) return 1; \
  } while (0)

// The layout the hand-written trip has as immediates, through the plain header.
static_assert(jxlhip::kLanesF2Bytes == 128 && jxlhip::kLanesA6B == 128 && jxlhip::kLanesA6A == 16512 && jxlhip::kLanesA6Cfg == 49280 &&
                  jxlhip::kLanesA6End == 49536 && jxlhip::kLanesPerLaneBytes == 200,
              "jxl_hip_lanes_trip.inc reads the tables at these offsets");

// ------------------------------------------------------------------------------------------------- hand-made frames
struct Hand {
  uint32_t ng = 0, np = 1, nh = 1, nctx = 495;
  std::vector<uint32_t> size, sel, groups, gbb, clusters = {8}, log_alpha = {5};
  bool partial = false;
  // one pass, one histogram set, every group listed, 10 blocks per group
  static Hand Of(std::vector<uint32_t> sizes) {
    Hand h;
    h.ng = uint32_t(sizes.size());
    h.size = std::move(sizes);
    h.sel.assign(h.ng, 0);
    for (uint32_t g = 0; g < h.ng; g++) h.groups.push_back(g);
    for (uint32_t g = 0; g <= h.ng; g++) h.gbb.push_back(10 * g);
    return h;
  }
  lp::LaneFrame View() const {
    return {ng, np, nh, nctx, size.data(), sel.data(), groups.data(), groups.size(), partial, gbb.data(), gbb.size(), clusters.data(), log_alpha.data()};
  }
};
// (views: the frames must outlive them)
static std::vector<lp::LaneFrame> Views(std::vector<Hand>&&, size_t = 1) = delete;
static std::vector<lp::LaneFrame> Views(const std::vector<Hand>& hands, size_t repeat = 1) {
  std::vector<lp::LaneFrame> v;
  for (size_t r = 0; r < repeat; r++)
    for (const Hand& h : hands) v.push_back(h.View());
  return v;
}

// What holds of every plan, from the rules and the frames alone. `unit_lanes`: the lanes of every unit, in unit order.
static int CheckPlan(const std::vector<lp::LaneFrame>& frames, const lp::LaneOverrides& o, const LanePlan& P, std::vector<uint32_t>* unit_lanes = nullptr) {
  const size_t units = P.unit_desc.size() / 4;
  EXPECT(P.units == units && P.unit_desc.size() % 4 == 0, "unit count");
  // every listed section in exactly one unit, once; inside a unit largest first, equal sizes as the frame lists them
  std::map<std::tuple<uint32_t, uint32_t, uint32_t>, int> seen;
  size_t min_total = 0, sections = 0, next = 0;
  std::vector<uint32_t> min_lanes(units);
  for (size_t u = 0; u < units; u++) {
    const uint32_t fi = P.unit_desc[4 * u] & 0xFFFF, sel = P.unit_desc[4 * u] >> 16, begin = P.unit_desc[4 * u + 1], count = P.unit_desc[4 * u + 2],
                   pass = P.unit_desc[4 * u + 3];
    EXPECT(fi < frames.size() && count >= 1 && begin == next && size_t(begin) + count <= P.list.size(), "unit %zu: frame %u, entries %u + %u", u, fi, begin, count);
    next = begin + count;
    const lp::LaneFrame& f = frames[fi];
    EXPECT(pass < f.num_passes && sel < f.num_hist, "unit %zu: pass %u set %u", u, pass, sel);
    const uint32_t* sz = f.sec_size + size_t(pass) * f.num_groups;
    std::map<uint32_t, size_t> listed_at;
    for (size_t k = 0; k < f.group_count; k++) listed_at[f.group_list[k]] = k;
    uint64_t total = 0, longest = 0;
    for (uint32_t j = 0; j < count; j++) {
      const uint32_t g = P.list[begin + j];
      EXPECT(listed_at.count(g), "unit %zu: group %u is not in the frame's list", u, g);
      const uint32_t s = f.sec_sel[size_t(pass) * f.num_groups + g];
      EXPECT(s == sel || (sel == 0 && s >= f.num_hist), "unit %zu: group %u has set %u", u, g, s);
      seen[std::make_tuple(fi, pass, g)]++;
      if (j) {
        const uint32_t prev = P.list[begin + j - 1];
        EXPECT(sz[prev] > sz[g] || (sz[prev] == sz[g] && listed_at[prev] < listed_at[g]), "unit %zu: entry %u out of order", u, j);
      }
      total += uint64_t(sz[g]) + 4000;
      longest = std::max<uint64_t>(longest, uint64_t(sz[g]) + 4000);
    }
    const uint64_t ceil_rule = (total + longest - 1) / longest;
    min_lanes[u] = uint32_t(std::min<uint64_t>(std::max<uint64_t>(ceil_rule, 1), count));
    min_total += min_lanes[u];
    sections += count;
  }
  EXPECT(next == P.list.size(), "the list holds %zu entries, the units %zu", P.list.size(), next);
  size_t want_sections = 0;
  for (size_t fi = 0; fi < frames.size(); fi++) {
    const lp::LaneFrame& f = frames[fi];
    for (uint32_t pass = 0; pass < f.num_passes; pass++)
      for (size_t k = 0; k < f.group_count; k++) {
        const uint32_t g = f.group_list[k];
        if (pass && f.partial && f.sec_size[size_t(pass) * f.num_groups + g] == 0) continue;
        want_sections++;
        EXPECT(seen[std::make_tuple(uint32_t(fi), pass, g)] == 1, "frame %zu pass %u group %u is in %d units", fi, pass, g, seen[std::make_tuple(uint32_t(fi), pass, g)]);
      }
  }
  EXPECT(sections == want_sections && P.total_sections == sections, "%zu sections in units, %zu listed, the plan says %zu", sections, want_sections, P.total_sections);
  EXPECT(P.min_lanes_total == min_total, "min lanes %zu, the ceiling rule gives %zu", P.min_lanes_total, min_total);

  // the workgroups: a permutation of the units, the waves of each adjacent; lanes split evenly to within one
  const size_t wgs = P.wg_unit.size();
  EXPECT(P.wave_lanes.size() == wgs && P.wg_est.size() == wgs, "per-workgroup arrays");
  const uint32_t lpw = P.lanes_per_wave;
  EXPECT(lpw >= 1 && lpw <= 64 && (lpw & (lpw - 1)) == 0, "lanes per wave %u", lpw);
  std::vector<int> runs(units, 0);
  std::vector<uint32_t> lanes(units, 0), waves(units, 0), lo(units, 255), hi(units, 0);
  for (size_t p = 0; p < wgs; p++) {
    const uint32_t u = P.wg_unit[p];
    EXPECT(u < units, "workgroup %zu: unit %u", p, u);
    if (p == 0 || P.wg_unit[p - 1] != u) runs[u]++;
    else EXPECT(P.wg_est[p] == P.wg_est[p - 1], "workgroup %zu: another estimate for the same unit", p);
    lanes[u] += P.wave_lanes[p];
    waves[u]++;
    lo[u] = std::min<uint32_t>(lo[u], P.wave_lanes[p]);
    hi[u] = std::max<uint32_t>(hi[u], P.wave_lanes[p]);
  }
  for (size_t u = 0; u < units; u++) {
    const uint32_t count = P.unit_desc[4 * u + 2];
    EXPECT(runs[u] == 1, "unit %zu is emitted in %d runs", u, runs[u]);
    EXPECT(lo[u] >= 1 && hi[u] - lo[u] <= 1 && hi[u] <= lpw, "unit %zu: waves of %u to %u lanes", u, lo[u], hi[u]);
    EXPECT(lanes[u] >= min_lanes[u] && lanes[u] <= std::max(count, min_lanes[u]) && waves[u] == (lanes[u] + lpw - 1) / lpw, "unit %zu: %u lanes in %u waves", u,
           lanes[u], waves[u]);
    if (lpw > 1 && lpw < 32) EXPECT(lanes[u] == min_lanes[u], "unit %zu: %u lanes, the ceiling rule gives %u", u, lanes[u], min_lanes[u]);
  }
  if (o.wg_order == 1)
    for (size_t p = 1; p < wgs; p++) EXPECT(P.wg_est[p] <= P.wg_est[p - 1], "workgroup %zu: a longer unit behind a shorter one", p);
  if (unit_lanes) *unit_lanes = lanes;

  // the device buffer: uint4 reads of the descriptors, uint32 reads of the counters; packed into exactly blob_bytes
  EXPECT(P.off_units % 16 == 0 && P.off_units >= P.list.size() * 4 && P.off_units < P.list.size() * 4 + 16, "off_units %zu", P.off_units);
  EXPECT(P.off_queue == P.off_units + units * 16 && P.off_wave_lanes == P.off_queue + units * 4 && P.blob_bytes == P.off_wave_lanes + wgs, "blob layout");
  std::unique_ptr<uint8_t[]> blob(new uint8_t[P.blob_bytes ? P.blob_bytes : 1]);  // (exactly that many: a byte more is a sanitizer report)
  memset(blob.get(), 0xEE, P.blob_bytes);
  lp::PackLaneBlob(P, blob.get());
  EXPECT(P.list.empty() || memcmp(blob.get(), P.list.data(), P.list.size() * 4) == 0, "blob: list");
  for (size_t i = P.list.size() * 4; i < P.off_units; i++) EXPECT(blob[i] == 0, "blob: padding byte %zu", i);
  EXPECT(units == 0 || memcmp(blob.get() + P.off_units, P.unit_desc.data(), units * 16) == 0, "blob: descriptors");
  for (size_t i = P.off_queue; i < P.off_wave_lanes; i++) EXPECT(blob[i] == 0, "blob: queue counter byte %zu", i);
  EXPECT(wgs == 0 || memcmp(blob.get() + P.off_wave_lanes, P.wave_lanes.data(), wgs) == 0, "blob: wave lanes");
  return 0;
}

static int Units() {
  // two frames; the second with two passes, two histogram sets (a selector past the sets counts as set 0), a list that
  // leaves group 1 out, equal sizes, and a short group_block_begin
  Hand a = Hand::Of({500, 9000, 500, 0, 700});
  Hand b;
  b.ng = 6; b.np = 2; b.nh = 2;
  b.size = {100, 5, 300, 300, 300, 0, /* pass 1 */ 40, 40, 0, 40, 7, 40};
  b.sel = {0, 1, 1, 0, 7, 1, /* pass 1 */ 1, 1, 1, 1, 0, 0};
  b.groups = {5, 0, 2, 3, 4};
  b.gbb = {0, 10, 20, 30};
  b.clusters = {8, 9};
  b.log_alpha = {5, 6};
  const std::vector<Hand> hands = {a, b};
  for (int order = 0; order < 3; order++)
    for (int lanes : {0, 2, 64}) {
      lp::LaneOverrides o;
      o.wg_order = order;
      o.lanes_per_wave = lanes;
      const std::vector<lp::LaneFrame> frames = Views(hands);
      const LanePlan P = lp::PlanLaneBatch(frames.data(), frames.size(), lp::LaneBatchTraits(), o);
      RUN(CheckPlan(frames, o, P));
      // frame 0; frame 1 pass 0 set 0 (groups 0, 3 and 4, whose selector is past the sets), set 1 (5, 2); pass 1 set 0, set 1
      EXPECT(P.units == 5, "%zu units", P.units);
      const std::vector<uint32_t> want = {1, 4, 0, 2, 3, /**/ 3, 4, 0, /**/ 2, 5, /**/ 5, 4, /**/ 0, 3, 2};
      EXPECT(P.list == want, "the section list");
      const std::vector<uint32_t> desc = {0, 0, 5, 0, /**/ 1, 5, 3, 0, /**/ 1 | 1 << 16, 8, 2, 0, /**/ 1, 10, 2, 1, /**/ 1 | 1 << 16, 12, 3, 1};
      EXPECT(P.unit_desc == desc, "the unit descriptors");
    }
  return 0;
}

// The three regimes of lanes per wave, the numbers worked out here from the rule.
static int Regimes() {
  const lp::LaneBatchTraits traits;
  const lp::LaneOverrides none;
  std::vector<uint32_t> lanes;
  {  // room to spare, one section cost far above the rest: 100000 + 20 * 4000 = 180000 -> ceil(1.8) = 2 lanes at least per unit;
     // 200 frames: 400 < 1024 -> one lane per wave, and every unit grows by 1024 / 400 = 2.56: floor(5.12) = 5 lanes, 5 waves
    std::vector<uint32_t> sizes(21, 0);
    sizes[7] = 96000;
    const std::vector<Hand> hands = {Hand::Of(sizes)};
    const std::vector<lp::LaneFrame> frames = Views(hands, 200);
    const LanePlan P = lp::PlanLaneBatch(frames.data(), frames.size(), traits, none);
    RUN(CheckPlan(frames, none, P, &lanes));
    EXPECT(P.min_lanes_total == 400 && P.lanes_per_wave == 1 && P.wg_unit.size() == 1000, "grow: %zu lanes, %u per wave, %zu workgroups", P.min_lanes_total,
           P.lanes_per_wave, P.wg_unit.size());
    for (uint32_t l : lanes) EXPECT(l == 5, "grow: %u lanes", l);
    for (uint8_t l : P.wave_lanes) EXPECT(l == 1, "grow: a wave of %u lanes", l);
  }
  {  // ... and growth stops at a lane per section: 10000 + 6000 + 5000 + 4000 = 25000 -> ceil(2.5) = 3; x 341.3 -> 4 sections, 4 lanes
    const std::vector<Hand> hands = {Hand::Of({6000, 2000, 1000, 0})};
    const std::vector<lp::LaneFrame> frames = Views(hands);
    const LanePlan P = lp::PlanLaneBatch(frames.data(), 1, traits, none);
    RUN(CheckPlan(frames, none, P, &lanes));
    EXPECT(P.min_lanes_total == 3 && P.lanes_per_wave == 1 && lanes[0] == 4 && P.wg_unit.size() == 4, "grow to a lane per section");
  }
  {  // between: 2 * 100000 + 13 * 4000 = 252000 -> ceil(2.52) = 3 lanes; 400 frames: 1200 > 1024, 600 <= 1024 -> two lanes per wave;
     // a unit keeps its 3 lanes: two waves, of 2 lanes and of 1
    std::vector<uint32_t> sizes(15, 0);
    sizes[0] = sizes[9] = 96000;
    const std::vector<Hand> hands = {Hand::Of(sizes)};
    const std::vector<lp::LaneFrame> frames = Views(hands, 400);
    const LanePlan P = lp::PlanLaneBatch(frames.data(), frames.size(), traits, none);
    RUN(CheckPlan(frames, none, P, &lanes));
    EXPECT(P.min_lanes_total == 1200 && P.lanes_per_wave == 2 && P.wg_unit.size() == 800, "between: %zu lanes, %u per wave, %zu workgroups", P.min_lanes_total,
           P.lanes_per_wave, P.wg_unit.size());
    for (size_t p = 0; p < 800; p++) EXPECT(P.wave_lanes[p] == (p % 2 ? 1 : 2), "between: wave %zu has %u lanes", p, P.wave_lanes[p]);
    // ... 700 frames: 2100 -> 1050 waves of two are too many, 525 of four fit: one wave of 3 lanes per unit
    const std::vector<lp::LaneFrame> more = Views(hands, 700);
    const LanePlan Q = lp::PlanLaneBatch(more.data(), more.size(), traits, none);
    RUN(CheckPlan(more, none, Q, &lanes));
    EXPECT(Q.lanes_per_wave == 4 && Q.wg_unit.size() == 700 && Q.wave_lanes[0] == 3, "between: %u per wave", Q.lanes_per_wave);
  }
  {  // dense: 5500 such frames: 16500 lanes; 1032 waves of 16 are too many -> 32 or more means 64 per wave, one wave per unit with
     // a lane per section (15)
    std::vector<uint32_t> sizes(15, 0);
    sizes[0] = sizes[9] = 96000;
    const std::vector<Hand> hands = {Hand::Of(sizes)};
    const std::vector<lp::LaneFrame> frames = Views(hands, 5500);
    const LanePlan P = lp::PlanLaneBatch(frames.data(), frames.size(), traits, none);
    RUN(CheckPlan(frames, none, P, &lanes));
    EXPECT(P.min_lanes_total == 16500 && P.lanes_per_wave == 64 && P.wg_unit.size() == 5500, "dense: %zu lanes, %u per wave, %zu workgroups", P.min_lanes_total,
           P.lanes_per_wave, P.wg_unit.size());
    for (uint8_t l : P.wave_lanes) EXPECT(l == 15, "dense: a wave of %u lanes", l);
  }
  {  // dense when forced (32 counts as 64): 70 equal sections need 70 lanes, two waves of 35; 10 sections that need 3 get 10
    lp::LaneOverrides o;
    o.lanes_per_wave = 32;
    const std::vector<Hand> hands = {Hand::Of(std::vector<uint32_t>(70, 100)), Hand::Of({96000, 96000, 0, 0, 0, 0, 0, 0, 0, 0})};
    const std::vector<lp::LaneFrame> frames = Views(hands);
    const LanePlan P = lp::PlanLaneBatch(frames.data(), frames.size(), traits, o);
    RUN(CheckPlan(frames, o, P, &lanes));
    EXPECT(P.lanes_per_wave == 64 && P.min_lanes_total == 73 && lanes[0] == 70 && lanes[1] == 10 && P.wg_unit.size() == 3, "forced dense");
    o.lanes_per_wave = 3;  // (not a power of two: ignored)
    EXPECT(lp::PlanLaneBatch(frames.data(), frames.size(), traits, o).lanes_per_wave == 1, "a forced 3");
    o.lanes_per_wave = 8;
    EXPECT(lp::PlanLaneBatch(frames.data(), frames.size(), traits, o).lanes_per_wave == 8, "a forced 8");
  }
  return 0;
}

// The form of the tables: `n` frames of one section each are n workgroups.
static int FormOf(const Hand& h, size_t n, lp::LaneBatchTraits t, lp::LaneOverrides o, LanePlan::Form want, size_t want_lds, const char* what) {
  const std::vector<Hand> hands = {h};
  const std::vector<lp::LaneFrame> frames = Views(hands, n);
  const LanePlan P = lp::PlanLaneBatch(frames.data(), n, t, o);
  RUN(CheckPlan(frames, o, P));
  EXPECT(P.wg_unit.size() == n, "%s: %zu workgroups", what, P.wg_unit.size());
  EXPECT(P.form == want && P.lds == want_lds, "%s: tables %s, lds %zu; want %s, %zu", what, lp::FormName(P.form), P.lds, lp::FormName(want), want_lds);
  return 0;
}
static int Forms() {
  {  // the layout, by hand: 128 clusters x 2^6 slots, 8 block contexts (3960 contexts -> 3984 bytes of map)
    const jxlhip::LanesLds l8 = jxlhip::LanesLdsLayout(1, 3960, 128, 6, 1, 64, true, false, false);
    EXPECT(l8.f2 == 0 && l8.alias == 128 && l8.ctx == 128 + 65536 && l8.ctx2 == 65664 + 3984 && l8.cfg == 69648 + 128 && l8.poff == l8.cfg && l8.wave0 == 69776 &&
               l8.per_wave == 12800 && l8.total == 82576, "eight-byte layout");
    const jxlhip::LanesLds lg = jxlhip::LanesLdsLayout(1, 3960, 128, 6, 1, 64, false, false, false);
    EXPECT(lg.ctx == 128 && lg.wave0 == 128 + 3984 + 128 && lg.total == 4240 + 12800, "global layout");
    const jxlhip::LanesLds l6 = jxlhip::LanesLdsLayout(1, 3960, 128, 6, 1, 64, false, false, true);
    EXPECT(l6.ctx == 49536 && l6.wave0 == 49536 + 3984 + 128 && l6.total == 66448, "six-byte layout");
    const jxlhip::LanesLds lp_ = jxlhip::LanesLdsLayout(1, 3960, 128, 6, 1, 64, false, true, false);
    EXPECT(lp_.ctx == 128 && lp_.cfg == 4240 && lp_.poff == 4240 + 512 && lp_.wave0 == 4752 + 1024 && lp_.total == 5776 + 12800, "prefix layout");
  }
  const lp::LaneOverrides none;
  lp::LaneBatchTraits one_cu;
  one_cu.device_cus = 1;
  // small tables: 64 clusters x 2^6 slots = 32 KB, 495 contexts: 128 + 32768 + 512 + 128 + 12800 = 46336 bytes, three to a CU's 160 KB;
  // six-byte 49536 + 512 + 128 + 12800 = 62976; global 128 + 512 + 128 + 12800 = 13568
  Hand small = Hand::Of({1000});
  small.clusters = {64};
  small.log_alpha = {6};
  // libjxl-sized tables, 3960 contexts: 82576 bytes, one to a CU; six-byte 66448, two to a CU; global 17040
  Hand big = small;
  big.clusters = {128};
  big.nctx = 3960;
  RUN(FormOf(small, 3, one_cu, none, LanePlan::kLds8, 46336, "fits and resident"));
  RUN(FormOf(small, 4, one_cu, none, LanePlan::kGlobal, 13568, "not resident, nor in six bytes (two to a CU)"));
  RUN(FormOf(big, 1, one_cu, none, LanePlan::kLds8, 82576, "one workgroup, one CU"));
  RUN(FormOf(big, 2, one_cu, none, LanePlan::kLds6, 66448, "not resident, six-byte eligible and resident"));
  RUN(FormOf(big, 3, one_cu, none, LanePlan::kGlobal, 17040, "not resident in six bytes either"));
  lp::LaneBatchTraits t = one_cu;
  t.coef_bits = 32;
  RUN(FormOf(big, 2, t, none, LanePlan::kGlobal, 17040, "int32 coefficients have no six-byte form"));
  t = one_cu;
  t.prefix = true;
  RUN(FormOf(big, 2, t, none, LanePlan::kPrefix, 18576, "prefix"));
  t = one_cu;
  t.lds_budget = 66447;
  RUN(FormOf(big, 2, t, none, LanePlan::kGlobal, 17040, "six bytes over the budget"));
  t.lds_budget = 66448;
  RUN(FormOf(big, 2, t, none, LanePlan::kLds6, 66448, "six bytes at the budget"));
  // the aids
  lp::LaneOverrides o;
  o.table_form = 1;
  RUN(FormOf(small, 3, one_cu, o, LanePlan::kGlobal, 13568, "GALIAS=1"));
  RUN(FormOf(big, 2, one_cu, o, LanePlan::kGlobal, 17040, "GALIAS=1 rules six bytes out"));
  o.a6 = 2;
  RUN(FormOf(big, 2, one_cu, o, LanePlan::kLds6, 66448, "A6=2 whenever eligible, whatever GALIAS says"));
  o = none;
  o.table_form = 0;
  RUN(FormOf(big, 2, one_cu, o, LanePlan::kLds8, 82576, "GALIAS=0 where eight bytes fit the budget"));
  t = one_cu;
  t.lds_budget = 82575;
  RUN(FormOf(big, 1, t, o, LanePlan::kLds6, 66448, "GALIAS=0 only where eight bytes fit the budget"));
  o = none;
  o.a6 = 0;
  RUN(FormOf(big, 2, one_cu, o, LanePlan::kGlobal, 17040, "A6=0"));
  o.a6 = 2;
  RUN(FormOf(small, 3, one_cu, o, LanePlan::kLds6, 62976, "A6=2 though eight bytes are resident"));
  t = one_cu;
  t.prefix = true;
  RUN(FormOf(small, 3, t, o, LanePlan::kPrefix, 128 + 512 + 128 + 512 + 1024 + 12800, "A6=2, prefix"));
  // the bounds of the six-byte form, one at a time (A6=2: eligible is chosen): log_alpha 7 / 8, 128 / 129 clusters, 8192 slots and
  // the first count above that the other two bounds allow (65 << 7); 8193 clusters of one slot are 8193 slots
  struct Edge {
    uint32_t clusters, log_alpha;
    bool eligible;
  };
  for (const Edge& e : {Edge{64, 7, true}, Edge{32, 8, false}, Edge{128, 6, true}, Edge{129, 5, false}, Edge{65, 7, false}, Edge{8192, 0, false},
                        Edge{8193, 0, false}, Edge{128, 0, true}}) {
    Hand h = Hand::Of({1000});
    h.clusters = {e.clusters};
    h.log_alpha = {e.log_alpha};
    const size_t lds8 = 128 + (size_t(e.clusters) << e.log_alpha) * 8 + 512 + 128 + 12800;
    char what[64];
    snprintf(what, sizeof(what), "%u clusters, log_alpha %u", e.clusters, e.log_alpha);
    RUN(FormOf(h, 1, one_cu, o, e.eligible ? LanePlan::kLds6 : LanePlan::kLds8, e.eligible ? 62976 : lds8, what));
  }
  return 0;
}

static int Extremes() {
  const lp::LaneBatchTraits traits;
  const lp::LaneOverrides none;
  {  // nothing listed: no units, no workgroups, an empty buffer
    Hand h = Hand::Of({100, 200});
    h.groups.clear();
    const std::vector<lp::LaneFrame> frames = {h.View()};
    const LanePlan P = lp::PlanLaneBatch(frames.data(), 1, traits, none);
    RUN(CheckPlan(frames, none, P));
    EXPECT(P.units == 0 && P.wg_unit.empty() && P.blob_bytes == 0 && P.lds == 0, "an empty group list");
    const LanePlan Q = lp::PlanLaneBatch(nullptr, 0, traits, none);
    EXPECT(Q.units == 0 && Q.blob_bytes == 0, "no frames");
  }
  {  // a partial frame whose second pass has not arrived at all, and one where it has for one group
    Hand h = Hand::Of({100, 200, 0});
    h.np = 2;
    h.size = {100, 200, 0, /* pass 1 */ 0, 0, 0};
    h.sel.assign(6, 0);
    h.clusters = {8, 8};
    h.log_alpha = {5, 5};
    h.partial = true;
    std::vector<lp::LaneFrame> frames = {h.View()};
    LanePlan P = lp::PlanLaneBatch(frames.data(), 1, traits, none);
    RUN(CheckPlan(frames, none, P));
    EXPECT(P.units == 1 && P.total_sections == 3, "a pass that is absent: %zu units", P.units);  // (pass 0 keeps its empty section)
    h.size[4] = 50;
    frames = {h.View()};
    P = lp::PlanLaneBatch(frames.data(), 1, traits, none);
    RUN(CheckPlan(frames, none, P));
    EXPECT(P.units == 2 && P.total_sections == 4 && P.list.back() == 1, "a pass with one section");
    h.partial = false;  // (a whole frame's empty sections are sections)
    frames = {h.View()};
    P = lp::PlanLaneBatch(frames.data(), 1, traits, none);
    RUN(CheckPlan(frames, none, P));
    EXPECT(P.units == 2 && P.total_sections == 6, "empty sections of a whole frame");
  }
  {  // one section, and one of the largest size
    for (uint32_t size : {0u, 1u, 0xFFFFFFFFu}) {
      const Hand h = Hand::Of({size});
      const std::vector<lp::LaneFrame> frames = {h.View()};
      const LanePlan P = lp::PlanLaneBatch(frames.data(), 1, traits, none);
      RUN(CheckPlan(frames, none, P));
      EXPECT(P.units == 1 && P.wg_unit.size() == 1 && P.wave_lanes[0] == 1 && P.blob_bytes == 16 + 16 + 4 + 1, "one section");
    }
  }
  {  // 65 535 frames of one section
    const std::vector<Hand> hands = {Hand::Of({300}), Hand::Of({0xFFFFFFFFu})};
    std::vector<lp::LaneFrame> frames = Views(hands, 32768);
    frames.pop_back();
    for (int order = 0; order < 3; order++) {
      lp::LaneOverrides o;
      o.wg_order = order;
      const LanePlan P = lp::PlanLaneBatch(frames.data(), frames.size(), traits, o);
      RUN(CheckPlan(frames, o, P));
      EXPECT(P.units == 65535 && P.lanes_per_wave == 64 && P.wg_unit.size() == 65535 && (P.unit_desc[4 * 65534] & 0xFFFF) == 65534, "65 535 frames");
    }
  }
  {  // the scalar-form batch: a workgroup per four sections, the largest frame's tables + 1 KB + 5 KB per wave
    const uint32_t groups[3] = {9, 4, 1};
    const size_t tables[3] = {1000, 3000, 2000};
    const LanePlan P = lp::PlanUniBatch(groups, tables, 3, 4);
    const std::vector<uint32_t> want = {0, 1, 2, 1 << 16, 2 << 16};
    EXPECT(P.wg_unit == want && P.lds == 3000 + 1024 + 4 * 5120 && P.list.empty() && P.wg_est.empty(), "the scalar-form batch");
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------- real streams
// What jxlhip_frame_upload keeps of a descriptor for the planner (jxl_hip_api.hip AdoptFrame).
struct Kept {
  uint32_t ng, np, nh, nctx, coef_bits;
  bool prefix;
  std::vector<uint32_t> size, sel, groups, absent_groups, absent_blocks, absent_sections, gbb, clusters, log_alpha;
  lp::LaneFrame View() const {
    return {ng, np, nh, nctx, size.data(), sel.data(), groups.data(), groups.size(), !absent_sections.empty(), gbb.data(), gbb.size(), clusters.data(),
            log_alpha.data()};
  }
};
extern "C" int jxlhip_frame_upload(JxlHipContext* ctx, const JxlHipFrameDesc* dp) {
  Kept* k = reinterpret_cast<Kept*>(ctx);
  const JxlHipFrameDesc& d = *dp;
  const up::Geometry g = up::MakeGeometry(d, up::UploadOptions());
  k->ng = d.num_groups;
  k->np = d.num_passes;
  k->nh = d.num_histograms;
  k->nctx = g.nctx;
  k->coef_bits = d.coef_bits;
  k->prefix = true;
  up::BuildGroupLists(d, g, &k->groups, &k->absent_groups, &k->absent_blocks, &k->absent_sections);
  k->size.assign(d.section_size, d.section_size + g.nsec);
  k->sel.resize(g.nsec);
  up::BuildSelectors(d, k->sel.data());
  k->gbb.assign(d.group_block_begin, d.group_block_begin + d.num_groups + 1);
  for (uint32_t p = 0; p < d.num_passes; p++) {
    k->clusters.push_back(d.passes[p].num_clusters);
    k->log_alpha.push_back(d.passes[p].log_alpha);
    k->prefix = k->prefix && d.passes[p].use_prefix && !d.passes[p].lz77;
  }
  return 0;
}

static int PlanFiles(int argc, char** argv) {
  lp::LaneOverrides o;
  lp::LaneBatchTraits traits;
  std::vector<std::unique_ptr<Kept>> kept;
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a.rfind("--", 0) == 0) {
      if (i + 1 >= argc) return 2;
      const int v = atoi(argv[++i]);
      if (a == "--cus") traits.device_cus = uint32_t(v);
      else if (a == "--lanes") o.lanes_per_wave = v;
      else if (a == "--order") o.wg_order = v;
      else if (a == "--galias") o.table_form = v;
      else if (a == "--a6") o.a6 = v;
      else return 2;
      continue;
    }
    FILE* f = fopen(argv[i], "rb");
    if (!f) return 2;
    std::vector<uint8_t> data;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + n);
    fclose(f);
    JxlAmdFrame* frame = nullptr;
    if (jxlamd_frame_parse(data.data(), data.size(), nullptr, nullptr, &frame)) {
      fprintf(stderr, "FAIL: %s does not parse (%s)\n", argv[i], jxlamd_last_error());
      return 1;
    }
    kept.emplace_back(new Kept());
    const int r = jxlamd_frame_upload_band(frame, reinterpret_cast<JxlHipContext*>(kept.back().get()), 0, 0);
    jxlamd_frame_free(frame);
    EXPECT(r == 0, "upload of %s: %d", argv[i], r);
  }
  if (kept.empty()) return 2;
  std::vector<lp::LaneFrame> frames;
  for (const auto& k : kept) frames.push_back(k->View());
  traits.prefix = kept[0]->prefix;
  traits.coef_bits = kept[0]->coef_bits;
  const LanePlan P = lp::PlanLaneBatch(frames.data(), frames.size(), traits, o);
  RUN(CheckPlan(frames, o, P));
  printf("pack units %zu sections %zu lanes(min) %zu lanes/wave %u workgroups %zu lds %zu tables %s\n", P.units, P.total_sections, P.min_lanes_total,
         P.lanes_per_wave, P.wg_unit.size(), P.lds, lp::FormName(P.form));
  printf("wg_unit");
  for (uint32_t u : P.wg_unit) printf(" %u", u);
  printf("\nwg_est");
  for (uint64_t e : P.wg_est) printf(" %llu", (unsigned long long)e);
  printf("\nwave_lanes");
  for (uint8_t l : P.wave_lanes) printf(" %u", l);
  printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "plan") return PlanFiles(argc, argv);
  if (mode != "kats") return 2;
  if (Units() || Regimes() || Forms() || Extremes()) return 1;
  printf("lane plan kats passed\n");
  return 0;
}
