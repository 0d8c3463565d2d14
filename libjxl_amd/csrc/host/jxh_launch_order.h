// Order of the workgroups of a batched k_entropy_lanes launch (jxh_lane_plan.h PlanLaneBatch): host only, no HIP types.
//
// A unit (the sections of one frame that share a histogram set) lasts as long as its busiest lane. A launch ends with its
// last unit, and the workgroups of the NEXT launch start in the LDS slots the ending ones free, in dispatch order: what
// starts last should be short. So the workgroups are emitted by estimated unit length, longest first.
//
// The estimate replays the kernel's queue (sections in list order, each to the lane that is free first) with a section
// cost of a * bytes + b * blocks + c, fitted against the stream writer's token counts over the benchmark's eight streams
// (scripts/fit_entropy_cost.py; DESIGN.md section 8.1 has the fit and the rank agreement it reaches). Nothing here is
// learnt from a decode: a frame is decoded once.
#ifndef JXH_LAUNCH_ORDER_H_
#define JXH_LAUNCH_ORDER_H_

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <numeric>
#include <queue>
#include <utility>
#include <vector>

namespace jxh {
namespace launch_order {

// tokens of a section ~ 3.21 * bytes - 23.4 * blocks + 27823, in 1/16 token (1024 x 768, d1.0, seeds 177-184: r = 0.948)
constexpr int64_t kCostPerByte = 51, kCostPerBlock = -374, kCostPerSection = 445170;

enum Mode : int {
  kFrameOrder = 0,    // unit after unit as planned
  kLongestFirst = 1,  // by estimate, largest first; equal estimates keep frame order
  kDealt = 2,         // frame order with every run of kDealRun units rotated by the run's index: unit i no longer meets
                      // the same XCD as units i + 8, i + 16, ... but nothing is sorted (measurement aid)
};
constexpr size_t kDealRun = 8;  // XCDs of an MI355X: the hardware deals workgroups to them in turn

inline uint64_t SectionCost(uint32_t bytes, uint32_t blocks) {
  const int64_t c = kCostPerByte * int64_t(bytes) + kCostPerBlock * int64_t(blocks) + kCostPerSection;
  return c > 16 ? uint64_t(c) : 16u;  // (a section costs a token at least: never zero, never negative)
}

// The queue replay: `cost[i]` in list order, each to the lane that is free first (the lowest lane among equals); the
// finishing time of the busiest lane. No sections: 0. No lanes counts as one.
inline uint64_t ReplayQueue(const uint64_t* cost, size_t n, uint32_t lanes) {
  if (n == 0) return 0;
  if (lanes == 0) lanes = 1;
  if (size_t(lanes) >= n) return *std::max_element(cost, cost + n);  // a lane each
  typedef std::pair<uint64_t, uint32_t> Lane;  // (free at, index)
  std::priority_queue<Lane, std::vector<Lane>, std::greater<Lane>> free_at;
  for (uint32_t l = 0; l < lanes; l++) free_at.push(Lane(0, l));
  uint64_t end = 0;
  for (size_t i = 0; i < n; i++) {
    Lane l = free_at.top();
    free_at.pop();
    l.first += cost[i];
    end = std::max(end, l.first);
    free_at.push(l);
  }
  return end;
}

// Estimated length of a unit: its sections' byte sizes and block counts in list order (largest bytes first), `lanes`
// lanes over all of its waves.
inline uint64_t UnitEstimate(const uint32_t* bytes, const uint32_t* blocks, size_t n, uint32_t lanes) {
  std::vector<uint64_t> cost(n);
  for (size_t i = 0; i < n; i++) cost[i] = SectionCost(bytes[i], blocks[i]);
  return ReplayQueue(cost.data(), n, lanes);
}

// units in dispatch order
inline std::vector<uint32_t> OrderUnits(const uint64_t* est, size_t units, int mode) {
  std::vector<uint32_t> order(units);
  std::iota(order.begin(), order.end(), 0u);
  if (mode == kLongestFirst) {
    std::stable_sort(order.begin(), order.end(), [est](uint32_t a, uint32_t b) { return est[a] > est[b]; });
  } else if (mode == kDealt) {
    for (size_t r0 = 0, run = 0; r0 < units; r0 += kDealRun, run++) {
      const size_t len = std::min(kDealRun, units - r0);
      std::rotate(order.begin() + r0, order.begin() + r0 + run % len, order.begin() + r0 + len);
    }
  }
  return order;
}

// Workgroups in dispatch order: entry p = the workgroup, counted in frame order (unit after unit, `waves[u]` each), that
// is emitted p-th. The waves of a unit stay adjacent and ascending.
inline std::vector<uint32_t> OrderWorkgroups(const uint64_t* est, const uint32_t* waves, size_t units, int mode) {
  std::vector<size_t> first(units + 1, 0);
  for (size_t u = 0; u < units; u++) first[u + 1] = first[u] + waves[u];
  std::vector<uint32_t> from;
  from.reserve(first[units]);
  for (uint32_t u : OrderUnits(est, units, mode))
    for (uint32_t w = 0; w < waves[u]; w++) from.push_back(uint32_t(first[u] + w));
  return from;
}

}  // namespace launch_order
}  // namespace jxh

#endif  // JXH_LAUNCH_ORDER_H_
