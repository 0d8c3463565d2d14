// Known-answer tests of libjxl_amd/csrc/host/jxh_launch_order.h: the order in which jxlhip_run_entropy_batch emits the lane
// kernel's workgroups, and the cost estimate behind it. Built by tests/test_launch_order.py with
// -fsanitize=address,undefined (CPU only).
//
// usage: launch_order_kats kats          the properties of the order and the queue replay
//        launch_order_kats slots FILE    FILE: per stream a line "stream N" and N lines "bytes blocks tokens" (its sections);
//                                        the slot check below on the frames these streams make
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../libjxl_amd/csrc/host/jxh_launch_order.h"

namespace lo = jxh::launch_order;

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                    \
    }                                                                \
  } while (0)

// The properties every order has: a permutation of the workgroups; the waves of a unit adjacent and ascending.
static void CheckOrder(const std::vector<uint32_t>& from, const std::vector<uint64_t>& est, const std::vector<uint32_t>& waves, int mode) {
  std::vector<uint32_t> unit_of;  // frame order: workgroup -> unit
  std::vector<uint32_t> first(waves.size());
  for (size_t u = 0; u < waves.size(); u++) {
    first[u] = uint32_t(unit_of.size());
    for (uint32_t w = 0; w < waves[u]; w++) unit_of.push_back(uint32_t(u));
  }
  CHECK(from.size() == unit_of.size());
  std::vector<uint8_t> seen(unit_of.size(), 0);
  for (uint32_t f : from) {
    CHECK(f < seen.size());
    if (f >= seen.size()) return;
    CHECK(!seen[f]);
    seen[f] = 1;
  }
  for (size_t p = 0; p < from.size();) {
    const uint32_t u = unit_of[from[p]];
    CHECK(from[p] == first[u]);  // a unit begins with its first wave ...
    for (uint32_t w = 0; w < waves[u]; w++) CHECK(p + w < from.size() && from[p + w] == first[u] + w);  // ... and goes on to its last
    if (p + waves[u] < from.size()) {
      const uint32_t next = unit_of[from[p + waves[u]]];
      if (mode == lo::kLongestFirst) {
        CHECK(est[u] >= est[next]);                // estimates are non-increasing along the order
        if (est[u] == est[next]) CHECK(u < next);  // equal estimates keep frame order
      }
      if (mode == lo::kFrameOrder) CHECK(next == u + 1);
    }
    p += waves[u];
  }
}

static uint64_t Rng(uint64_t* s) {
  *s = *s * 6364136223846793005ull + 1442695040888963407ull;
  return *s >> 33;
}

static void Kats() {
  // the queue replay by hand: costs 9 7 6 5 4 on two lanes. 9 -> lane 0 (9), 7 -> lane 1 (7), 6 -> lane 1 (13),
  // 5 -> lane 0 (14), 4 -> lane 1 (17): the busiest lane ends at 17
  {
    const uint64_t cost[5] = {9, 7, 6, 5, 4};
    CHECK(lo::ReplayQueue(cost, 5, 2) == 17);
    CHECK(lo::ReplayQueue(cost, 5, 1) == 31);
    CHECK(lo::ReplayQueue(cost, 5, 5) == 9);
    CHECK(lo::ReplayQueue(cost, 5, 64) == 9);
    CHECK(lo::ReplayQueue(cost, 5, 0) == 31);  // (no lanes counts as one)
    CHECK(lo::ReplayQueue(cost, 0, 2) == 0);
    CHECK(lo::ReplayQueue(cost, 1, 2) == 9);
    // the same through the section costs: five sections on two lanes, list order
    const uint32_t bytes[5] = {9000, 7000, 6000, 5000, 4000}, blocks[5] = {100, 90, 1024, 0, 50};
    uint64_t c[5];
    for (int i = 0; i < 5; i++) {
      c[i] = lo::SectionCost(bytes[i], blocks[i]);
      CHECK(int64_t(c[i]) == lo::kCostPerByte * bytes[i] + lo::kCostPerBlock * blocks[i] + lo::kCostPerSection);
    }
    CHECK(c[0] > c[1] && c[1] > c[3] && c[3] > c[4] && c[4] > c[2]);
    // c0 -> lane 0, c1 -> lane 1, c2 -> lane 1 (free first), then c3 to whichever is free first, c4 likewise
    uint64_t l0 = c[0], l1 = c[1] + c[2];
    (l0 <= l1 ? l0 : l1) += c[3];
    (l0 <= l1 ? l0 : l1) += c[4];
    CHECK(lo::UnitEstimate(bytes, blocks, 5, 2) == std::max(l0, l1));
  }
  // a section's cost is never zero or negative, and does not overflow at the largest inputs
  {
    CHECK(lo::SectionCost(0, 0) == uint64_t(lo::kCostPerSection));
    CHECK(lo::SectionCost(0, 1024) >= 16);
    CHECK(lo::SectionCost(0, 0xFFFFFFFFu) == 16);
    CHECK(lo::SectionCost(0xFFFFFFFFu, 0) == uint64_t(lo::kCostPerByte) * 0xFFFFFFFFull + uint64_t(lo::kCostPerSection));
    const uint32_t zero[3] = {0, 0, 0}, blocks[3] = {1024, 0, 7};
    CHECK(lo::UnitEstimate(zero, blocks, 3, 1) == lo::SectionCost(0, 1024) + lo::SectionCost(0, 0) + lo::SectionCost(0, 7));
    const uint32_t big[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
    CHECK(lo::UnitEstimate(big, zero, 2, 1) == 2 * lo::SectionCost(0xFFFFFFFFu, 0));
    CHECK(lo::UnitEstimate(big, zero, 0, 4) == 0);
  }
  // one unit, one section
  for (int mode = 0; mode < 3; mode++) {
    const uint32_t b = 0, k = 0;
    std::vector<uint64_t> est = {lo::UnitEstimate(&b, &k, 1, 1)};
    std::vector<uint32_t> waves = {1};
    std::vector<uint32_t> from = lo::OrderWorkgroups(est.data(), waves.data(), 1, mode);
    CHECK(from.size() == 1 && from[0] == 0);
    CHECK(lo::OrderWorkgroups(est.data(), waves.data(), 0, mode).empty());
  }
  // 65 535 frames (a batch's limit), some with several units and waves, many equal estimates; and small counts round the
  // dealt order's run length
  uint64_t seed = 12345;
  for (size_t units : {size_t(1), size_t(2), size_t(7), size_t(8), size_t(9), size_t(17), size_t(640), size_t(65535), size_t(70000)})
    for (int mode = 0; mode < 3; mode++) {
      std::vector<uint64_t> est(units);
      std::vector<uint32_t> waves(units);
      for (size_t u = 0; u < units; u++) {
        est[u] = (Rng(&seed) % 5 == 0) ? 0xFFFFFFFFFFFFFFF0ull + Rng(&seed) % 3 : Rng(&seed) % 8;
        waves[u] = 1 + uint32_t(Rng(&seed) % 20 == 0 ? Rng(&seed) % 16 : 0);
      }
      const std::vector<uint32_t> from = lo::OrderWorkgroups(est.data(), waves.data(), units, mode);
      CheckOrder(from, est, waves, mode);
      if (mode == lo::kDealt && units >= 16) {  // unit i and unit i + 8 no longer meet the same position modulo 8
        std::vector<uint32_t> order = lo::OrderUnits(est.data(), units, mode);
        CHECK(order[0] == 0 && order[7] == 7 && order[8] == 9 && order[15] == 8);
        if (units >= 24) CHECK(order[16] == 18 && order[22] == 16 && order[23] == 17);
      }
    }
  // the benchmark's shape: eight streams cycled over 640 frames, one wave each: the longest stream's 80 frames come first
  {
    const uint64_t stream_est[8] = {50, 80, 30, 30, 70, 10, 60, 20};
    std::vector<uint64_t> est(640);
    std::vector<uint32_t> waves(640, 1);
    for (size_t u = 0; u < 640; u++) est[u] = stream_est[u % 8];
    const std::vector<uint32_t> from = lo::OrderWorkgroups(est.data(), waves.data(), 640, lo::kLongestFirst);
    CheckOrder(from, est, waves, lo::kLongestFirst);
    for (size_t p = 0; p < 80; p++) CHECK(from[p] == 8 * p + 1);
    for (size_t p = 0; p < 160; p++) CHECK(from[320 + p] == (p % 2 ? 8 * (p / 2) + 3 : 8 * (p / 2) + 2));  // the tie: frame order
    for (size_t p = 0; p < 80; p++) CHECK(from[560 + p] == 8 * p + 5);
  }
}

// Two launches of `wgs` workgroups on `slots` LDS slots, both enqueued at time 0: the hardware starts workgroups in dispatch
// order, the first launch's before the second's, each in the slot that is free first. `len[p]` = length of the p-th
// dispatched workgroup of either launch (the two frame sets hold the same frames). Returns when the second launch ends.
static uint64_t TwoLaunches(const std::vector<uint64_t>& len, size_t slots) {
  std::vector<uint64_t> free_at(slots, 0);
  uint64_t end = 0;
  for (int launch = 0; launch < 2; launch++)
    for (uint64_t l : len) {
      auto slot = std::min_element(free_at.begin(), free_at.end());
      *slot += l;
      if (launch == 1) end = std::max(end, *slot);
    }
  return end;
}

static int Slots(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) return 2;
  std::vector<uint64_t> est, truth;
  char word[16];
  unsigned n;
  while (fscanf(f, "%15s %u", word, &n) == 2 && !strcmp(word, "stream")) {
    std::vector<uint32_t> bytes(n), blocks(n), tokens(n), order(n);
    for (unsigned i = 0; i < n; i++)
      if (fscanf(f, "%u %u %u", &bytes[i], &blocks[i], &tokens[i]) != 3) return 2;
    for (unsigned i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return bytes[a] > bytes[b]; });  // the section list
    std::vector<uint32_t> lb(n), lk(n);
    std::vector<uint64_t> lt(n);
    for (unsigned i = 0; i < n; i++) {
      lb[i] = bytes[order[i]];
      lk[i] = blocks[order[i]];
      lt[i] = uint64_t(tokens[order[i]]) * 16;
    }
    const uint32_t lanes = n < 64 ? n : 64;  // (the dense regime: one wave per unit, a lane per section up to 64)
    est.push_back(lo::UnitEstimate(lb.data(), lk.data(), n, lanes));
    truth.push_back(lo::ReplayQueue(lt.data(), n, lanes));
    printf("stream %zu: sections %u estimate %llu true %llu (1/16 token)\n", est.size() - 1, n, (unsigned long long)est.back(),
           (unsigned long long)truth.back());
  }
  fclose(f);
  if (est.size() != 8) return 2;
  const size_t kSlots = 24, kWgs = 20;
  std::vector<uint64_t> unit_est(kWgs);
  std::vector<uint32_t> waves(kWgs, 1);
  for (size_t u = 0; u < kWgs; u++) unit_est[u] = est[u % 8];  // the frames cycle through the streams
  uint64_t ends[3];
  for (int mode = 0; mode < 3; mode++) {
    const std::vector<uint32_t> from = lo::OrderWorkgroups(unit_est.data(), waves.data(), kWgs, mode);
    CheckOrder(from, unit_est, waves, mode);
    std::vector<uint64_t> len(kWgs);
    for (size_t p = 0; p < kWgs; p++) len[p] = truth[from[p] % 8];
    ends[mode] = TwoLaunches(len, kSlots);
    printf("order %d: the second launch ends at %llu\n", mode, (unsigned long long)ends[mode]);
  }
  CHECK(ends[lo::kLongestFirst] <= ends[lo::kFrameOrder]);  // the estimated order ends no later than frame order
  return g_failed ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "kats")) {
    Kats();
    if (!g_failed) printf("launch order kats passed\n");
    return g_failed ? 1 : 0;
  }
  if (argc == 3 && !strcmp(argv[1], "slots")) return Slots(argv[2]);
  fprintf(stderr, "usage: launch_order_kats kats | slots FILE\n");
  return 2;
}
