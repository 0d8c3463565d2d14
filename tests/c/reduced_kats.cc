// Known-answer tests of libjxl_amd/csrc/host/jxh_reduced_plan.h (what jxlhip_reduced_upload checks of a JxlHipReducedDesc,
// the block it places and the descriptor array of a batched launch), built with AddressSanitizer + UBSan and run as a
// child process by tests/test_reduced_host.py:
//  * every rule refuses the one change that breaks it, and names itself; extents near 2^32 are refused without overflow;
//  * a context's block placed into a heap block of exactly its size stays inside it (ASan watches) and says what the
//    descriptor said;
//  * for sets of 1, 2 and 7 frames, a 1x1-block frame among them, the tile origins are strictly increasing, every tile of
//    the launch belongs to exactly one frame, and the array stays inside BatchBytes; a room one descriptor short is
//    refused without a write past it.
// Prints "exercised: <rule names>" for the Python side to hold against the header's enum.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "../../libjxl_amd/csrc/host/jxh_reduced_plan.h"

using namespace jxlhip::reduced;

static int g_failures = 0;
static std::set<std::string> g_exercised;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      g_failures++;                                                    \
    }                                                                  \
  } while (0)

static const char* RuleName(int r) {
  switch (r) {
    case kReducedRuleExtents: return "Extents";
    case kReducedRulePlaneSize: return "PlaneSize";
    case kReducedRuleLimit: return "Limit";
    case kReducedRulePlanes: return "Planes";
    case kReducedRuleSteps: return "Steps";
    case kReducedRuleLinear: return "Linear";
    case kReducedRulePrecision: return "Precision";
    case kReducedRuleLaunch: return "Launch";
    default: return "?";
  }
}

static const int32_t* FakeQ() { return reinterpret_cast<const int32_t*>(uintptr_t(0x10000)); }  // (never dereferenced: the check is pure)
static const uint8_t* FakeEp() { return reinterpret_cast<const uint8_t*>(uintptr_t(0x20000)); }

static JxlHipReducedDesc Good(uint32_t xs, uint32_t ys) {
  JxlHipReducedDesc d;
  memset(&d, 0, sizeof(d));
  d.xsize_blocks = xs;
  d.ysize_blocks = ys;
  d.dc_quantised = FakeQ();
  d.dc_extra_precision = FakeEp();
  d.dc_step[0] = 0.001f;
  d.dc_step[1] = 0.002f;
  d.dc_step[2] = 0.004f;
  d.dc_cfl_x = 0.0f;
  d.dc_cfl_b = 1.0f;
  d.dc_smoothing = 1;
  d.linear_output = 0;
  return d;
}

static void Refused(const JxlHipReducedDesc& d, int want, int line) {
  int rule = -1;
  const int r = CheckReducedDesc(d, &rule);
  if (r != JXLHIP_ERR_INVALID_ARGUMENT || rule != want) {
    printf("FAILED line %d: code %d rule %s, expected %s\n", line, r, RuleName(rule), RuleName(want));
    g_failures++;
  }
  EXPECT(CheckReducedDesc(d) == r);  // (the rule pointer is optional)
  g_exercised.insert(RuleName(want));
}
#define REFUSED(d, rule) Refused(d, rule, __LINE__)

static void Rules() {
  for (uint32_t xs : {1u, 3u, 51u, 256u, 257u, 480u, kMaxExtentBlocks}) EXPECT(CheckReducedDesc(Good(xs, 35)) == 0);
  EXPECT(CheckReducedDesc(Good(35, kMaxExtentBlocks / 2)) == 0);
  // an image of more tiles than one launch's grid holds (blocks times 256 threads below 2^32), either way round
  EXPECT(Tiles(64, kMaxExtentBlocks - 8) == kMaxLaunchTiles && CheckReducedDesc(Good(64, kMaxExtentBlocks - 8)) == 0);
  JxlHipReducedDesc big = Good(64, kMaxExtentBlocks);
  REFUSED(big, kReducedRuleLaunch);
  big = Good(kMaxExtentBlocks, kMaxExtentBlocks);
  REFUSED(big, kReducedRuleLaunch);
  big = Good(kMaxExtentBlocks, 64);
  REFUSED(big, kReducedRuleLaunch);
  JxlHipReducedDesc d = Good(51, 35);
  d.xsize_blocks = 0;
  REFUSED(d, kReducedRuleExtents);
  d = Good(51, 35);
  d.ysize_blocks = 0;
  REFUSED(d, kReducedRuleExtents);
  // (two 32-bit extents whose plane bytes pass 2^64: refused by the checked product, before the limit is asked)
  d = Good(0xFFFFFFFFu, 0xFFFFFFFFu);
  REFUSED(d, kReducedRulePlaneSize);
  d = Good(0x80000000u, 0xC0000000u);
  REFUSED(d, kReducedRulePlaneSize);
  d = Good(kMaxExtentBlocks + 1, 1);
  REFUSED(d, kReducedRuleLimit);
  d = Good(1, kMaxExtentBlocks + 1);
  REFUSED(d, kReducedRuleLimit);
  d = Good(0xFFFFFFFFu, 1);
  REFUSED(d, kReducedRuleLimit);
  d = Good(51, 35);
  d.dc_quantised = nullptr;
  REFUSED(d, kReducedRulePlanes);
  for (int c = 0; c < 3; c++)
    for (float bad : {0.0f, -0.001f, float(INFINITY), float(NAN), -float(INFINITY)}) {
      d = Good(51, 35);
      d.dc_step[c] = bad;
      REFUSED(d, kReducedRuleSteps);
    }
  for (int32_t bad : {2, 3, -1, INT32_MIN, INT32_MAX}) {
    d = Good(51, 35);
    d.linear_output = bad;
    REFUSED(d, kReducedRuleLinear);
  }
  d = Good(51, 35);
  d.linear_output = 1;
  EXPECT(CheckReducedDesc(d) == 0);
  // one DC group: the precision bytes may be missing (all 0); several: they may not
  d = Good(256, 256);
  d.dc_extra_precision = nullptr;
  EXPECT(CheckReducedDesc(d) == 0);
  d = Good(257, 35);
  d.dc_extra_precision = nullptr;
  REFUSED(d, kReducedRulePrecision);
  d = Good(35, 257);
  d.dc_extra_precision = nullptr;
  REFUSED(d, kReducedRulePrecision);
  EXPECT(DcGroups(256, 256) == 1 && DcGroups(257, 256) == 2 && DcGroups(288, 38) == 2 && DcGroups(513, 513) == 9);
}

// A stand-in for the kernel's descriptor: the head, then bytes the plan never looks into.
struct FakeDev {
  ReducedHead h;
  uint8_t rest[331];
};

static void Blocks() {
  const uint32_t shapes[][2] = {{1, 1}, {2, 3}, {3, 3}, {65, 1}, {51, 35}, {288, 38}, {64, 8}, {65, 9}, {480, 270}};
  for (const auto& s : shapes) {
    const uint32_t xs = s[0], ys = s[1];
    std::vector<int32_t> q(size_t(3) * xs * ys);
    for (size_t i = 0; i < q.size(); i++) q[i] = int32_t(i * 2654435761u) >> 12;
    std::vector<uint8_t> ep(DcGroups(xs, ys));
    for (size_t i = 0; i < ep.size(); i++) ep[i] = uint8_t(1 + i);
    for (int with_ep = 0; with_ep < 2; with_ep++) {
      JxlHipReducedDesc d = Good(xs, ys);
      d.dc_quantised = q.data();
      d.dc_extra_precision = with_ep ? ep.data() : nullptr;
      if (CheckReducedDesc(d) != 0) continue;  // (several groups without their bytes)
      const BlockLayout l = LayoutOf(d, sizeof(FakeDev));
      EXPECT(l.desc == 0 && l.ep >= sizeof(FakeDev) && l.q >= l.ep + l.ep_bytes && l.bytes == l.q + l.q_bytes && l.q % 256 == 0);
      EXPECT(l.q_bytes == q.size() * 4 && l.ep_bytes == (with_ep ? ep.size() : 0));
      uint8_t* block = static_cast<uint8_t*>(malloc(l.bytes));  // (exactly its size: ASan sees a write past it)
      ReducedHead h;
      float* const dc_out = reinterpret_cast<float*>(uintptr_t(0x30000));
      const uintptr_t base = 0x7000000;
      EXPECT(PlaceBlock(d, l, dc_out, block, base, &h) == 0);
      EXPECT(!memcmp(block + l.q, q.data(), l.q_bytes));
      if (with_ep) EXPECT(!memcmp(block + l.ep, ep.data(), l.ep_bytes));
      EXPECT(uintptr_t(h.q) == base + l.q && (with_ep ? uintptr_t(h.ep) == base + l.ep : h.ep == nullptr) && h.dc_out == dc_out);
      EXPECT(h.xs == xs && h.ys == ys && h.xgroups == (xs + 255) / 256 && h.smoothing == 1);
      EXPECT(h.step[0] == 0.001f && h.step[1] == 0.002f && h.step[2] == 0.004f && h.cfl_x == 0.0f && h.cfl_b == 1.0f);
      EXPECT(h.tile0 == 0 && h.tiles == Tiles(xs, ys) && h.tiles_x == TilesX(xs) && h.tiles == h.tiles_x * TilesY(ys));
      // the tiles cover the image: the last tile's first sample is inside, the one behind it is not
      EXPECT((h.tiles_x - 1) * kTileCols < xs && h.tiles_x * kTileCols >= xs);
      EXPECT((TilesY(ys) - 1) * kTileRows < ys && TilesY(ys) * kTileRows >= ys);
      free(block);
    }
  }
}

static FakeDev DevOf(uint32_t xs, uint32_t ys, uint8_t mark) {
  FakeDev v;
  memset(&v, 0, sizeof(v));
  v.h.xs = xs;
  v.h.ys = ys;
  v.h.tiles = uint32_t(Tiles(xs, ys));
  v.h.tiles_x = TilesX(xs);
  memset(v.rest, mark, sizeof(v.rest));
  return v;
}

static void Batches() {
  const uint32_t all[7][2] = {{1, 1}, {2, 3}, {3, 3}, {65, 1}, {51, 35}, {288, 38}, {1, 1}};
  for (size_t n : {size_t(1), size_t(2), size_t(7)}) {
    std::vector<FakeDev> devs;
    for (size_t i = 0; i < n; i++) devs.push_back(DevOf(all[i][0], all[i][1], uint8_t(0x40 + i)));
    std::vector<const void*> each;
    for (const FakeDev& v : devs) each.push_back(&v);
    const size_t bytes = BatchBytes(n, sizeof(FakeDev));
    EXPECT(bytes == n * sizeof(FakeDev));
    uint8_t* block = static_cast<uint8_t*>(malloc(bytes));
    uint32_t total = 0;
    EXPECT(PlaceBatch(each.data(), n, sizeof(FakeDev), block, bytes, &total) == 0);
    std::vector<uint32_t> owner(total, 0xFFFFFFFFu);
    uint32_t prev = 0;
    for (size_t i = 0; i < n; i++) {
      FakeDev v;
      memcpy(&v, block + i * sizeof(FakeDev), sizeof(v));
      EXPECT(i == 0 ? v.h.tile0 == 0 : v.h.tile0 > prev);  // strictly increasing
      prev = v.h.tile0;
      EXPECT(v.h.tiles == devs[i].h.tiles && v.h.tiles >= 1 && v.h.xs == devs[i].h.xs && v.h.ys == devs[i].h.ys);
      EXPECT(!memcmp(v.rest, devs[i].rest, sizeof(v.rest)));  // (the rest of the descriptor travels as it is)
      for (uint32_t t = 0; t < v.h.tiles; t++) {
        EXPECT(uint64_t(v.h.tile0) + t < total);
        if (uint64_t(v.h.tile0) + t < total) {
          EXPECT(owner[v.h.tile0 + t] == 0xFFFFFFFFu);  // no tile twice
          owner[v.h.tile0 + t] = uint32_t(i);
        }
      }
    }
    for (uint32_t t = 0; t < total; t++) EXPECT(owner[t] != 0xFFFFFFFFu);  // every tile once
    // the kernel's bisection (the last descriptor that starts at or before the tile) finds the owner
    for (uint32_t t = 0; t < total; t++) {
      uint32_t lo = 0, hi = uint32_t(n);
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        FakeDev v;
        memcpy(&v, block + size_t(mid) * sizeof(FakeDev), sizeof(v));
        if (v.h.tile0 <= t) lo = mid;
        else hi = mid;
      }
      EXPECT(lo == owner[t]);
    }
    // a room one descriptor short: refused, nothing written (the block of exactly that size is ASan's to watch)
    if (n > 1) {
      uint8_t* small = static_cast<uint8_t*>(malloc(bytes - sizeof(FakeDev)));
      EXPECT(PlaceBatch(each.data(), n, sizeof(FakeDev), small, bytes - sizeof(FakeDev), &total) == JXLHIP_ERR_INVALID_ARGUMENT);
      free(small);
    }
    free(block);
  }
  // a set whose tiles pass the launch's bound, and a descriptor without tiles
  FakeDev big = DevOf(1, 1, 0);
  big.h.tiles = uint32_t(kMaxLaunchTiles);
  FakeDev one = DevOf(1, 1, 0);
  const void* two[2] = {&big, &one};
  std::vector<uint8_t> room(2 * sizeof(FakeDev));
  uint32_t total = 0;
  EXPECT(PlaceBatch(two, 2, sizeof(FakeDev), room.data(), room.size(), &total) == JXLHIP_ERR_UNSUPPORTED);
  EXPECT(PlaceBatch(two, 1, sizeof(FakeDev), room.data(), room.size(), &total) == 0 && total == kMaxLaunchTiles);
  one.h.tiles = 0;
  EXPECT(PlaceBatch(two + 1, 1, sizeof(FakeDev), room.data(), room.size(), &total) == JXLHIP_ERR_INVALID_ARGUMENT);
  EXPECT(PlaceBatch(two, 0, sizeof(FakeDev), room.data(), room.size(), &total) == JXLHIP_ERR_INVALID_ARGUMENT);
  EXPECT(PlaceBatch(two, 1, sizeof(ReducedHead) - 1, room.data(), room.size(), &total) == JXLHIP_ERR_INVALID_ARGUMENT);
}

int main() {
  Rules();
  Blocks();
  Batches();
  printf("exercised:");
  for (const std::string& r : g_exercised) printf(" %s", r.c_str());
  printf("\nsets: 1 2 7\n");
  if (g_failures) {
    printf("%d failures\n", g_failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
