// Known-answer tests of libjxl_amd/csrc/host/jxh_tensor_out.h (what jxlhip_set_output_tensor and the uploads check of a
// JxlHipTensorOut), built with AddressSanitizer + UBSan and run as a child process by tests/test_tensor_out_host.py:
//  * every rule refuses the one change that breaks it, and names itself;
//  * the layouts callers use are taken: contiguous CHW and HWC, a padded pitch, one image of an NCHW batch, odd data offsets;
//  * strides near 2^62 and a room one element short are refused without overflow;
//  * the largest offset the check works with equals a brute-force maximum over small extents, and the check accepts
//    exactly the room that holds it.
// Prints "exercised: <rule names>" for the Python side to hold against the header's enum.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "../../libjxl_amd/csrc/host/jxh_tensor_out.h"

using namespace jxlhip::tensor_out;

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
    case kTensorRuleData: return "Data";
    case kTensorRuleDtype: return "Dtype";
    case kTensorRuleChannels: return "Channels";
    case kTensorRuleAlignment: return "Alignment";
    case kTensorRuleStridesPositive: return "StridesPositive";
    case kTensorRuleFinite: return "Finite";
    case kTensorRuleU8Identity: return "U8Identity";
    case kTensorRuleInjective: return "Injective";
    case kTensorRuleBytes: return "Bytes";
    default: return "?";
  }
}

static void* Fake(uintptr_t address) { return reinterpret_cast<void*>(address); }  // (never dereferenced: the check is pure)

// A contiguous CHW tensor of `nc` channels over w x h with exactly the room it needs.
static JxlHipTensorOut Chw(uint32_t dtype, uint32_t nc, uint32_t w, uint32_t h) {
  JxlHipTensorOut t;
  memset(&t, 0, sizeof(t));
  t.data = Fake(0x10000);
  t.dtype = dtype;
  t.num_channels = nc;
  t.stride_x = 1;
  t.stride_y = w;
  t.stride_c = int64_t(w) * h;
  t.bytes = size_t(nc) * w * h * ElemBytes(dtype);
  for (int c = 0; c < 4; c++) {
    t.scale[c] = 1.0f;
    t.bias[c] = 0.0f;
  }
  return t;
}

// The descriptor is taken at w x h; after `breaker` it is refused with `rule` and nothing else.
template <typename F>
static void Refuses(const JxlHipTensorOut& good, uint32_t w, uint32_t h, int rule, F breaker) {
  int got = -1;
  EXPECT(CheckTensorOut(good, w, h, &got) == 0);
  EXPECT(got == -1);
  JxlHipTensorOut bad = good;
  breaker(bad);
  EXPECT(CheckTensorOut(bad, w, h, &got) == JXLHIP_ERR_INVALID_ARGUMENT);
  if (got != rule) {
    printf("FAILED: expected rule %s, refused by %s\n", RuleName(rule), RuleName(got));
    g_failures++;
  }
  EXPECT(CheckTensorOut(bad, w, h) == JXLHIP_ERR_INVALID_ARGUMENT);  // (without the out-parameter)
  g_exercised.insert(RuleName(rule));
}

static uint64_t BruteMaxOffset(const JxlHipTensorOut& t, uint32_t w, uint32_t h) {
  uint64_t best = 0;
  for (uint32_t c = 0; c < t.num_channels; c++)
    for (uint32_t y = 0; y < h; y++)
      for (uint32_t x = 0; x < w; x++) {
        const uint64_t o = uint64_t(c) * uint64_t(t.stride_c) + uint64_t(y) * uint64_t(t.stride_y) + uint64_t(x) * uint64_t(t.stride_x);
        if (o > best) best = o;
      }
  return best;
}
// Whether two elements of the image share an address (small extents only).
static bool BruteOverlaps(const JxlHipTensorOut& t, uint32_t w, uint32_t h) {
  std::set<uint64_t> seen;
  for (uint32_t c = 0; c < t.num_channels; c++)
    for (uint32_t y = 0; y < h; y++)
      for (uint32_t x = 0; x < w; x++)
        if (!seen.insert(uint64_t(c) * uint64_t(t.stride_c) + uint64_t(y) * uint64_t(t.stride_y) + uint64_t(x) * uint64_t(t.stride_x)).second) return true;
  return false;
}

int main() {
  const uint32_t W = 121, H = 37;
  const JxlHipTensorOut f16 = Chw(JXLHIP_TENSOR_F16, 3, W, H);
  // ---- every rule, broken alone
  Refuses(f16, W, H, kTensorRuleData, [](JxlHipTensorOut& t) { t.data = nullptr; });
  Refuses(f16, W, H, kTensorRuleDtype, [](JxlHipTensorOut& t) { t.dtype = 3; });  // (u16 is an interleaved format only)
  Refuses(f16, W, H, kTensorRuleDtype, [](JxlHipTensorOut& t) { t.dtype = 7; });
  Refuses(f16, W, H, kTensorRuleChannels, [](JxlHipTensorOut& t) { t.num_channels = 0; });
  Refuses(f16, W, H, kTensorRuleChannels, [](JxlHipTensorOut& t) { t.num_channels = 5; });
  Refuses(f16, W, H, kTensorRuleAlignment, [](JxlHipTensorOut& t) { t.data = Fake(0x10001); });
  Refuses(Chw(JXLHIP_TENSOR_F32, 3, W, H), W, H, kTensorRuleAlignment, [](JxlHipTensorOut& t) { t.data = Fake(0x10002); });
  Refuses(f16, W, H, kTensorRuleStridesPositive, [](JxlHipTensorOut& t) { t.stride_x = 0; });
  Refuses(f16, W, H, kTensorRuleStridesPositive, [](JxlHipTensorOut& t) { t.stride_y = -int64_t(W); });
  Refuses(f16, W, H, kTensorRuleStridesPositive, [](JxlHipTensorOut& t) { t.stride_c = INT64_MIN; });
  Refuses(f16, W, H, kTensorRuleFinite, [](JxlHipTensorOut& t) { t.scale[1] = INFINITY; });
  Refuses(f16, W, H, kTensorRuleFinite, [](JxlHipTensorOut& t) { t.bias[2] = NAN; });
  {
    JxlHipTensorOut t = f16;  // (a channel the tensor does not have is not read)
    t.scale[3] = NAN;
    EXPECT(CheckTensorOut(t, W, H) == 0);
  }
  const JxlHipTensorOut u8 = Chw(JXLHIP_TENSOR_U8, 3, W, H);
  Refuses(u8, W, H, kTensorRuleU8Identity, [](JxlHipTensorOut& t) { t.scale[0] = 2.0f; });
  Refuses(u8, W, H, kTensorRuleU8Identity, [](JxlHipTensorOut& t) { t.bias[1] = 0.5f; });
  Refuses(u8, W, H, kTensorRuleU8Identity, [](JxlHipTensorOut& t) { t.clamp01 = 1; });
  Refuses(f16, W, H, kTensorRuleInjective, [](JxlHipTensorOut& t) { t.stride_y = W - 1; });            // rows overlap by one column
  Refuses(f16, W, H, kTensorRuleInjective, [](JxlHipTensorOut& t) { t.stride_c = int64_t(W) * (H - 1); });  // planes overlap by a row
  Refuses(f16, W, H, kTensorRuleInjective, [](JxlHipTensorOut& t) { t.stride_c = t.stride_y; });       // equal strides
  Refuses(f16, W, H, kTensorRuleInjective, [](JxlHipTensorOut& t) { t.stride_x = 2; });                // columns run into the next row
  Refuses(f16, W, H, kTensorRuleBytes, [](JxlHipTensorOut& t) { t.bytes -= 1; });                      // one byte short
  Refuses(f16, W, H, kTensorRuleBytes, [](JxlHipTensorOut& t) { t.bytes -= ElemBytes(t.dtype); });     // one element short
  Refuses(f16, W, H, kTensorRuleBytes, [](JxlHipTensorOut& t) { t.bytes = 0; });
  // (an image larger than the one the room was made for)
  {
    int got = -1;
    EXPECT(CheckTensorOut(f16, W, H + 1, &got) == JXLHIP_ERR_INVALID_ARGUMENT && got == kTensorRuleInjective);  // (planes one row apart too little)
    JxlHipTensorOut one = Chw(JXLHIP_TENSOR_F16, 1, W, H);
    EXPECT(CheckTensorOut(one, W, H + 1, &got) == JXLHIP_ERR_INVALID_ARGUMENT && got == kTensorRuleBytes);
    EXPECT(CheckTensorOut(f16, 0, H, &got) == JXLHIP_ERR_INVALID_ARGUMENT && got == kTensorRuleData);  // (no image)
  }
  // ---- layouts callers use
  for (uint32_t dtype : {JXLHIP_TENSOR_U8, JXLHIP_TENSOR_F16, JXLHIP_TENSOR_BF16, JXLHIP_TENSOR_F32})
    for (uint32_t nc = 1; nc <= 4; nc++) {
      const size_t e = ElemBytes(dtype);
      EXPECT(e == (dtype == JXLHIP_TENSOR_U8 ? 1u : dtype == JXLHIP_TENSOR_F32 ? 4u : 2u));
      EXPECT(CheckTensorOut(Chw(dtype, nc, W, H), W, H) == 0);  // contiguous CHW
      JxlHipTensorOut hwc = Chw(dtype, nc, W, H);               // contiguous HWC
      hwc.stride_c = 1;
      hwc.stride_x = nc;
      hwc.stride_y = int64_t(W) * nc;
      EXPECT(CheckTensorOut(hwc, W, H) == 0);
      EXPECT(CheckTensorOut(hwc, H, W) != 0 || W == H);  // (the transposed image needs other strides)
      JxlHipTensorOut padded = Chw(dtype, nc, W, H);  // pitch W + 3, five spare rows between planes, data one element in
      padded.stride_y = W + 3;
      padded.stride_c = int64_t(W + 3) * (H + 5);
      padded.data = Fake(0x10000 + e);
      padded.bytes = (size_t(nc - 1) * size_t(padded.stride_c) + size_t(H - 1) * (W + 3) + W) * e;
      EXPECT(CheckTensorOut(padded, W, H) == 0);
      padded.bytes -= e;
      EXPECT(CheckTensorOut(padded, W, H) != 0);
      JxlHipTensorOut slice = Chw(dtype, nc, W, H);  // image 2 of an (N, C, H, W) batch of 4: the room is what is left of the batch
      slice.data = Fake(0x10000 + size_t(2) * nc * W * H * e);
      slice.bytes = size_t(2) * nc * W * H * e;
      EXPECT(CheckTensorOut(slice, W, H) == 0);
      JxlHipTensorOut nhwc = hwc;  // channels-last storage seen as CHW: the same map
      EXPECT(CheckTensorOut(nhwc, W, H) == 0);
    }
  {
    JxlHipTensorOut t = Chw(JXLHIP_TENSOR_F16, 1, W, H);  // one channel: its stride addresses nothing, whatever it is
    t.stride_c = 1;
    EXPECT(CheckTensorOut(t, W, H) == 0);
    t = Chw(JXLHIP_TENSOR_F32, 3, 1, 1);  // the 1 x 1 image of the binding call: only the channels count
    t.stride_c = 1;
    t.stride_y = t.stride_x = 1;
    EXPECT(CheckTensorOut(t, 1, 1) == 0);
  }
  // ---- no overflow: strides near 2^62
  {
    const int64_t big = int64_t(1) << 62;
    int got = -1;
    JxlHipTensorOut t = Chw(JXLHIP_TENSOR_F32, 3, W, H);
    t.bytes = SIZE_MAX;
    t.stride_c = big;  // 2 * 2^62 * 4 bytes: past 2^64
    EXPECT(CheckTensorOut(t, W, H, &got) == JXLHIP_ERR_INVALID_ARGUMENT && got == kTensorRuleBytes);
    t.stride_c = big - 1;
    EXPECT(CheckTensorOut(t, W, H, &got) == JXLHIP_ERR_INVALID_ARGUMENT && got == kTensorRuleBytes);
    t = Chw(JXLHIP_TENSOR_U8, 3, W, H);
    t.bytes = SIZE_MAX;
    t.stride_c = big;  // 2 * 2^62 + ... : fits 64 bits as an offset, one byte each
    EXPECT(CheckTensorOut(t, W, H, &got) == 0);
    uint64_t mo = 0;
    EXPECT(MaxOffset(t, W, H, &mo) && mo == 2 * uint64_t(big) + uint64_t(H - 1) * W + (W - 1));
    t.bytes = size_t(mo);  // one element short
    EXPECT(CheckTensorOut(t, W, H, &got) == JXLHIP_ERR_INVALID_ARGUMENT && got == kTensorRuleBytes);
    t.bytes = size_t(mo) + 1;
    EXPECT(CheckTensorOut(t, W, H) == 0);
    t.num_channels = 4;
    t.stride_c = INT64_MAX;  // 3 * (2^63 - 1): the offset itself does not fit
    EXPECT(!MaxOffset(t, W, H, &mo));
    EXPECT(CheckTensorOut(t, W, H, &got) == JXLHIP_ERR_INVALID_ARGUMENT && got == kTensorRuleBytes);
    t = Chw(JXLHIP_TENSOR_F16, 3, 16384, 16384);
    t.bytes = SIZE_MAX;
    t.stride_x = big;  // the smallest stride times its extent overflows: nothing can follow it
    t.stride_y = INT64_MAX - 1;
    t.stride_c = INT64_MAX;
    EXPECT(CheckTensorOut(t, 16384, 16384, &got) == JXLHIP_ERR_INVALID_ARGUMENT && got == kTensorRuleInjective);
    g_exercised.insert(RuleName(kTensorRuleInjective));
    g_exercised.insert(RuleName(kTensorRuleBytes));
  }
  // ---- against brute force over small extents: the largest offset, the exact room, and no accepted map overlaps
  {
    size_t accepted = 0, refused_injective = 0;
    const int64_t strides[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 16, 20, 35};
    for (uint32_t nc = 1; nc <= 4; nc++)
      for (uint32_t w = 1; w <= 5; w += 2)
        for (uint32_t h = 1; h <= 4; h += 3)
          for (int64_t sc : strides)
            for (int64_t sy : strides)
              for (int64_t sx : strides) {
                JxlHipTensorOut t = Chw(JXLHIP_TENSOR_F16, nc, w, h);
                t.stride_c = sc;
                t.stride_y = sy;
                t.stride_x = sx;
                const uint64_t want = BruteMaxOffset(t, w, h);
                uint64_t got = 0;
                EXPECT(MaxOffset(t, w, h, &got) && got == want);
                t.bytes = size_t(want + 1) * 2;
                int rule = -1;
                const int r = CheckTensorOut(t, w, h, &rule);
                if (r == 0) {
                  accepted++;
                  EXPECT(!BruteOverlaps(t, w, h));
                  t.bytes -= 1;  // the exact room: one byte less is refused by the byte rule
                  EXPECT(CheckTensorOut(t, w, h, &rule) == JXLHIP_ERR_INVALID_ARGUMENT && rule == kTensorRuleBytes);
                } else {
                  EXPECT(rule == kTensorRuleInjective);
                  refused_injective++;
                }
              }
    EXPECT(accepted > 1000 && refused_injective > 1000);
    printf("brute force: %zu maps accepted, %zu refused as overlapping\n", accepted, refused_injective);
  }
  printf("exercised:");
  for (const std::string& s : g_exercised) printf(" %s", s.c_str());
  printf("\n");
  if (g_failures) {
    printf("%d check(s) failed\n", g_failures);
    return 1;
  }
  printf("tensor_out_kats: ok\n");
  return 0;
}
