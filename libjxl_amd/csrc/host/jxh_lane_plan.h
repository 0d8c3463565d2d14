// The launch plan of a batched k_entropy_lanes launch (jxl_hip_api.hip PrepareBatch): host only, no HIP types. A pure
// function of what the frames of the set say, of the device and of the measurement aids: which sections form a unit, how
// many lanes and waves a unit gets, in what order the workgroups are emitted, which form of the tables the launch uses
// and how much LDS it asks for; and the layout of the one device buffer the kernel reads all of that from.
//
// unit = the sections of one frame and pass that share a histogram set (a workgroup stages ONE set's slice of the context
// map; the selector is read from the first bits of every section at upload). The lanes of a unit take its sections
// from a queue, largest first, so the split by lanes below only fixes HOW MANY lanes serve a unit:
//   * a launch lasts as long as its busiest lane, which cannot beat the unit's longest section, so a unit gets
//     about (its total cost) / (cost of its longest section) lanes: more would idle (typical 4K d1.0 frame: 135
//     sections of 12k-100k tokens, 60 lanes). The cost of a section is estimated as bytes + kSectionBytes (token
//     counts are unknown before decoding; a constant term dominates in sparse sections);
//   * small batches that leave SIMDs empty spread over up to one lane per section;
//   * the lanes of a unit are split evenly over its waves.
// One wave per workgroup: the waves of a workgroup slow each other down (a lone 4K frame, one lane per wave: 832
// cycles per trip with four waves per workgroup, 517 with two, 417 with one; 29.6 / 24.1 / 19.6 ms for the frame:
// profiles/r04_single_frame.txt), and a workgroup of its own per wave costs only another copy of the tables in LDS.
#ifndef JXH_LANE_PLAN_H_
#define JXH_LANE_PLAN_H_

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../hip/jxl_hip_lanes_abi.h"
#include "jxh_launch_order.h"

namespace jxh {
namespace lane_plan {

constexpr uint32_t kSectionBytes = 4000;
constexpr size_t kTargetWaves = 1024;

struct LaneFrame {  // one frame of the set: views into what the context holds
  uint32_t num_groups, num_passes, num_hist, nctx;
  const uint32_t* sec_size;  // [pass * num_groups + group]
  const uint32_t* sec_sel;   // same indexing: the section's histogram set
  const uint32_t* group_list;  // the groups this context decodes
  size_t group_count;
  bool partial;  // a later pass of some group has not arrived: such a section has size 0 and is left out
  const uint32_t* group_block_begin;  // [group]: first block; a group's last entry + 1 may be missing (gbb_count)
  size_t gbb_count;
  const uint32_t* pass_clusters;   // [pass]
  const uint32_t* pass_log_alpha;  // [pass]
};

struct LaneBatchTraits {
  bool prefix = false;      // every frame of the set is prefix-coded: the kernel's prefix form
  uint32_t coef_bits = 16;  // of every frame of the set
  uint32_t device_cus = 256;
  size_t lds_per_cu = 160 * 1024, lds_budget = 150 * 1024;  // of a CU; of one workgroup
};

// The measurement aids, as the environment gives them (jxl_hip_api.hip LaneOverridesFromEnv). Part of the plan's key.
struct LaneOverrides {
  int lanes_per_wave = 0;  // JXLHIP_LANES: a power of two up to 64 forces that many lanes per wave
  int table_form = -1;     // JXLHIP_GALIAS: 0 = alias tables in LDS where the 8-byte form fits the budget, 1 = in global memory
  int a6 = 1;              // JXLHIP_A6: 0 = never the six-byte form, 2 = whenever eligible
  int wg_order = 1;        // JXLHIP_WG_ORDER: jxh::launch_order::Mode
  uint32_t wait_shift = 1;  // JXLHIP_WAIT_SHIFT: EntropyLaneBatch::wait_shift, handed through
  bool operator==(const LaneOverrides& o) const {
    return lanes_per_wave == o.lanes_per_wave && table_form == o.table_form && a6 == o.a6 && wg_order == o.wg_order && wait_shift == o.wait_shift;
  }
};

struct LanePlan {
  std::vector<uint32_t> list;       // group indices of every unit, largest compressed size first
  std::vector<uint32_t> unit_desc;  // per unit: {frame | histogram set << 16, first entry in `list`, entries, pass}
  std::vector<uint32_t> wg_unit;    // per workgroup (one wave), in dispatch order: its unit
  std::vector<uint8_t> wave_lanes;  // per workgroup: populated lanes
  std::vector<uint64_t> wg_est;     // per workgroup: the estimated length of its unit (jxh_launch_order.h)
  enum Form { kLds8, kGlobal, kLds6, kPrefix } form = kLds8;  // where the kernel reads its tables
  size_t lds = 0;                   // dynamic LDS of the launch
  uint32_t lanes_per_wave = 0, wait_shift = 1;
  size_t units = 0, min_lanes_total = 0, total_sections = 0;
  // one device buffer: section list | unit descriptors (16-byte aligned) | queue counters | populated lanes per wave
  size_t off_units = 0, off_queue = 0, off_wave_lanes = 0, blob_bytes = 0;
};
inline const char* FormName(LanePlan::Form f) {
  return f == LanePlan::kPrefix ? "prefix" : (f == LanePlan::kLds6 ? "lds6" : (f == LanePlan::kGlobal ? "global" : "lds8"));
}

struct Unit {
  uint32_t frame, sel, pass, begin, count, min_lanes, lanes;
};

// Units: per frame, pass and histogram set (a selector past the frame's sets counts as set 0) the listed sections, sorted
// stably by size, largest first, appended to `list`. min_lanes = ceil(total cost / longest cost), in [1, count].
inline std::vector<Unit> BuildUnits(const LaneFrame* frames, size_t n, std::vector<uint32_t>* list) {
  std::vector<Unit> units;
  std::vector<uint32_t> order;
  for (size_t i = 0; i < n; i++) {
    const LaneFrame& f = frames[i];
    for (uint32_t pass = 0; pass < f.num_passes; pass++)
    for (uint32_t sel = 0; sel < f.num_hist; sel++) {
      const uint32_t* sz = f.sec_size + size_t(pass) * f.num_groups;
      const uint32_t* ssel = f.sec_sel + size_t(pass) * f.num_groups;
      order.clear();
      for (size_t k = 0; k < f.group_count; k++) {
        const uint32_t g = f.group_list[k];
        if (pass && sz[g] == 0 && f.partial) continue;  // (a partial frame: this pass of the group has not arrived)
        if (ssel[g] == sel || (sel == 0 && ssel[g] >= f.num_hist)) order.push_back(g);
      }
      if (order.empty()) continue;
      std::stable_sort(order.begin(), order.end(), [sz](uint32_t a, uint32_t b) { return sz[a] > sz[b]; });
      uint64_t total = 0;
      for (uint32_t g : order) total += uint64_t(sz[g]) + kSectionBytes;
      const uint64_t longest = uint64_t(sz[order[0]]) + kSectionBytes;
      Unit u;
      u.frame = uint32_t(i);
      u.sel = sel;
      u.pass = pass;
      u.begin = uint32_t(list->size());
      u.count = uint32_t(order.size());
      u.min_lanes = uint32_t((total + longest - 1) / longest);
      u.min_lanes = u.min_lanes > u.count ? u.count : (u.min_lanes ? u.min_lanes : 1);
      u.lanes = u.min_lanes;
      list->insert(list->end(), order.begin(), order.end());
      units.push_back(u);
    }
  }
  return units;
}

// Lanes per wave: the fewest (a power of two) that fit all lanes into kTargetWaves waves (a trip costs ~900 + 20 * lanes
// cycles), unless forced. Then the lanes of every unit:
//   dense regime, 32 or more: all of a unit's lanes in one wave of 64 (a trip costs about the same for 14 or 55 lanes),
//     and the wave's spare lanes are free: a lane per section, up to 64;
//   1, with room to spare: more lanes per unit by kTargetWaves / min_total, up to one per section;
//   otherwise min_lanes.
inline uint32_t ChooseLanes(std::vector<Unit>* units, size_t min_total, int forced) {
  uint32_t lanes_per_wave = 1;
  while (lanes_per_wave < 64 && (min_total + lanes_per_wave - 1) / lanes_per_wave > kTargetWaves) lanes_per_wave *= 2;
  if (forced >= 1 && forced <= 64 && (forced & (forced - 1)) == 0) lanes_per_wave = uint32_t(forced);
  if (lanes_per_wave >= 32) {
    lanes_per_wave = 64;
    for (Unit& u : *units)
      if (u.lanes < 64) u.lanes = u.count < 64 ? u.count : 64;
  }
  if (lanes_per_wave == 1 && min_total < kTargetWaves) {
    const double grow = double(kTargetWaves) / double(min_total);
    for (Unit& u : *units) {
      const uint32_t want = uint32_t(double(u.min_lanes) * grow);
      u.lanes = want > u.count ? u.count : (want < u.min_lanes ? u.min_lanes : want);
    }
  }
  return lanes_per_wave;
}

// The lanes of a unit split evenly over its waves: wave w of `waves` gets the w-th share, the first (lanes % waves) one more.
inline uint32_t WaveShare(uint32_t lanes, uint32_t waves, uint32_t w) { return lanes / waves + (w < lanes % waves ? 1u : 0u); }

// How long a unit will take: its queue replayed with the sections' estimated costs (bytes, and the blocks of the group,
// 0 where group_block_begin does not reach). `bytes` and `blocks` are scratch.
inline uint64_t EstimateUnit(const LaneFrame& f, const Unit& u, const uint32_t* list, std::vector<uint32_t>* bytes, std::vector<uint32_t>* blocks) {
  const uint32_t* sz = f.sec_size + size_t(u.pass) * f.num_groups;
  bytes->resize(u.count);
  blocks->resize(u.count);
  for (uint32_t j = 0; j < u.count; j++) {
    const uint32_t g = list[u.begin + j];
    (*bytes)[j] = sz[g];
    (*blocks)[j] = size_t(g) + 1 < f.gbb_count ? f.group_block_begin[g + 1] - f.group_block_begin[g] : 0;
  }
  return launch_order::UnitEstimate(bytes->data(), blocks->data(), u.count, u.lanes);
}

// LDS of the launch under each form of the tables (LanePlan::Form kLds8, kGlobal, kLds6; prefix codes have no alias tables:
// all three the same) = the largest workgroup: its unit's tables and one wave of 64 lanes. `a6_ok`: every unit's tables
// are within the six-byte form's bounds (log_alpha <= 7, kLanesA6Clusters, kLanesA6Slots).
inline void SizeLds(const LaneFrame* frames, const std::vector<Unit>& units, bool prefix, size_t lds_by_form[3], bool* a6_ok) {
  lds_by_form[0] = lds_by_form[1] = lds_by_form[2] = 0;
  *a6_ok = true;
  for (const Unit& u : units) {
    const LaneFrame& f = frames[u.frame];
    const uint32_t clusters = f.pass_clusters[u.pass], log_alpha = f.pass_log_alpha[u.pass];
    if (log_alpha > 7 || clusters > jxlhip::kLanesA6Clusters || (size_t(clusters) << log_alpha) > jxlhip::kLanesA6Slots) *a6_ok = false;
    for (int form = 0; form < 3; form++) {
      const size_t l = jxlhip::LanesLdsLayout(1, f.nctx, clusters, log_alpha, 0, 0, form == 0 && !prefix, prefix, form == 2).wave0 +
                       size_t(jxlhip::kLanesPerLaneBytes) * 64;
      lds_by_form[form] = std::max(lds_by_form[form], l);
    }
  }
}

// The form of the tables. With the alias tables in LDS a CU holds lds_per_cu / (LDS of a workgroup) workgroups; when that
// leaves part of the launch waiting for a second round (libjxl-sized tables: 128 clusters x 2^6 slots are 64 KB), the
// tables stay in global memory instead: a cached global round trip on every token's serial chain, but every frame
// resident. Between the two, for tables within the six-byte form's bounds and int16 coefficients: the six-byte form in LDS
// (70 KB per frame: two frames per CU instead of one), when THAT leaves the launch resident.
// The aids: table_form 0 / 1 forces LDS (only where the 8-byte form fits the budget) / global memory, and 1 also rules
// the six-byte form out; a6 0 rules it out, 2 takes it whenever eligible, whatever table_form says.
inline LanePlan::Form ChooseForm(const size_t lds_by_form[3], bool a6_ok, size_t num_wgs, const LaneBatchTraits& t, const LaneOverrides& o) {
  const size_t resident = lds_by_form[0] ? size_t(t.device_cus) * (t.lds_per_cu / lds_by_form[0]) : num_wgs;
  bool galias = lds_by_form[0] > t.lds_budget || resident < num_wgs;
  if (o.table_form == 0 && lds_by_form[0] <= t.lds_budget) galias = false;
  if (o.table_form == 1) galias = true;
  if (t.prefix) galias = true;  // (prefix codes have no alias tables: the two forms are the same)
  const size_t resident6 = lds_by_form[2] ? size_t(t.device_cus) * (t.lds_per_cu / lds_by_form[2]) : num_wgs;
  const bool eligible = a6_ok && !t.prefix && t.coef_bits == 16 && o.a6 != 0 && lds_by_form[2] <= t.lds_budget;
  if (eligible && ((galias && o.table_form != 1 && resident6 >= num_wgs) || o.a6 == 2)) return LanePlan::kLds6;
  return t.prefix ? LanePlan::kPrefix : (galias ? LanePlan::kGlobal : LanePlan::kLds8);
}

inline LanePlan PlanLaneBatch(const LaneFrame* frames, size_t n, const LaneBatchTraits& traits, const LaneOverrides& o) {
  LanePlan P;
  std::vector<Unit> units = BuildUnits(frames, n, &P.list);
  for (const Unit& u : units) {
    P.min_lanes_total += u.min_lanes;
    P.total_sections += u.count;
  }
  P.units = units.size();
  P.lanes_per_wave = ChooseLanes(&units, P.min_lanes_total, o.lanes_per_wave);
  P.wait_shift = o.wait_shift;

  // descriptors, estimates, and the workgroups in frame order: unit after unit, a workgroup per wave of the unit
  std::vector<uint64_t> unit_est(units.size());
  std::vector<uint32_t> unit_waves(units.size()), bytes, blocks, map;
  std::vector<uint8_t> lanes;
  P.unit_desc.reserve(units.size() * 4);
  for (size_t i = 0; i < units.size(); i++) {
    const Unit& u = units[i];
    unit_waves[i] = (u.lanes + P.lanes_per_wave - 1) / P.lanes_per_wave;
    unit_est[i] = EstimateUnit(frames[u.frame], u, P.list.data(), &bytes, &blocks);
    P.unit_desc.push_back(u.frame | u.sel << 16);
    P.unit_desc.push_back(u.begin);
    P.unit_desc.push_back(u.count);
    P.unit_desc.push_back(u.pass);
    for (uint32_t w = 0; w < unit_waves[i]; w++) {
      map.push_back(uint32_t(i));
      lanes.push_back(uint8_t(WaveShare(u.lanes, unit_waves[i], w)));
    }
  }
  // The hardware starts workgroups in index order, and those of the next launch in the LDS slots that ending ones free:
  // the longest units go first, so that what starts last is short (jxh_launch_order.h). Only the workgroup -> unit map
  // is permuted; the waves of a unit stay adjacent.
  const size_t num_wgs = map.size();
  const std::vector<uint32_t> from = launch_order::OrderWorkgroups(unit_est.data(), unit_waves.data(), units.size(), o.wg_order);
  P.wg_unit.resize(num_wgs);
  P.wave_lanes.resize(num_wgs);
  P.wg_est.resize(num_wgs);
  for (size_t p = 0; p < num_wgs; p++) {
    P.wg_unit[p] = map[from[p]];
    P.wave_lanes[p] = lanes[from[p]];
    P.wg_est[p] = unit_est[P.wg_unit[p]];
  }

  size_t lds_by_form[3];
  bool a6_ok;
  SizeLds(frames, units, traits.prefix, lds_by_form, &a6_ok);
  P.form = ChooseForm(lds_by_form, a6_ok, num_wgs, traits, o);
  P.lds = lds_by_form[P.form == LanePlan::kLds6 ? 2 : (P.form == LanePlan::kLds8 ? 0 : 1)];

  P.off_units = (P.list.size() * 4 + 15) & ~size_t(15);
  P.off_queue = P.off_units + P.unit_desc.size() * 4;
  P.off_wave_lanes = P.off_queue + P.units * 4;
  P.blob_bytes = P.off_wave_lanes + P.wave_lanes.size();
  return P;
}

// The device buffer of a lane plan: exactly blob_bytes at `dst`; padding and the queue counters are zero.
inline void PackLaneBlob(const LanePlan& P, uint8_t* dst) {
  memset(dst, 0, P.blob_bytes);
  if (!P.list.empty()) memcpy(dst, P.list.data(), P.list.size() * 4);
  if (!P.unit_desc.empty()) memcpy(dst + P.off_units, P.unit_desc.data(), P.unit_desc.size() * 4);
  if (!P.wave_lanes.empty()) memcpy(dst + P.off_wave_lanes, P.wave_lanes.data(), P.wave_lanes.size());
}

// The scalar-form batch (k_entropy_uni): a workgroup per waves_per_wg sections of a frame, frame << 16 | index in
// wg_unit; LDS = the largest frame's tables (lds_table_bytes[i]: context map + alias tables) + 1 KB + 5 KB per wave.
inline LanePlan PlanUniBatch(const uint32_t* num_groups, const size_t* lds_table_bytes, size_t n, uint32_t waves_per_wg) {
  LanePlan P;
  for (size_t i = 0; i < n; i++) {
    const uint32_t wgs = (num_groups[i] + waves_per_wg - 1) / waves_per_wg;
    for (uint32_t j = 0; j < wgs; j++) P.wg_unit.push_back(uint32_t(i) << 16 | j);
    P.lds = std::max(P.lds, lds_table_bytes[i] + 1024 + size_t(waves_per_wg) * 5120);
  }
  return P;
}

}  // namespace lane_plan
}  // namespace jxh

#endif  // JXH_LANE_PLAN_H_
