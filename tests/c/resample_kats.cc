// Known-answer tests of libjxl_amd/csrc/host/jxh_resample_plan.h (what jxlhip_set_output_resized, the uploads and
// jxlhip_debug_resample check of a JxlHipResizedOut, and the tap tables the resample kernels read), built with
// AddressSanitizer + UBSan and run as a child process by tests/test_resample_host.py:
//  * every rule refuses the one change that breaks it, and names itself;
//  * boxes and sizes near 2^32 are refused without overflow;
//  * every row of every table sums to 1 within 2^-23 * its tap count, windows ascend and stay inside the axis;
//  * the number of weights stays inside AxisWeightBound, MakeAxisTaps refuses a room one float short without writing past
//    it, and a table or a context's block placed into a heap block of exactly its size stays inside it (ASan watches);
//  * the placed descriptor says what the binding said.
// Prints "exercised: <rule names>" for the Python side to hold against the header's enum, and writes the tables of the
// axes named on the command line ("n_in:n_out" ...) to the file given first, for the Python side to hold against its own
// float64 reading: per axis n_in, n_out, total as uint32, then first[], count[], then the weights as float32.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "../../libjxl_amd/csrc/host/jxh_resample_plan.h"

using namespace jxlhip::resample;

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
    case kResampleRuleOutput: return "Output";
    case kResampleRuleFilter: return "Filter";
    case kResampleRuleOutLimit: return "OutLimit";
    case kResampleRuleBoxExtents: return "BoxExtents";
    case kResampleRuleBoxInside: return "BoxInside";
    case kResampleRuleTensor: return "Tensor";
    default: return "?";
  }
}

static void* Fake(uintptr_t address) { return reinterpret_cast<void*>(address); }  // (never dereferenced: the check is pure)

// A contiguous CHW f32 tensor of three channels over out_w x out_h with exactly the room it needs, the whole image.
static JxlHipResizedOut Good(uint32_t out_w, uint32_t out_h) {
  JxlHipResizedOut d;
  memset(&d, 0, sizeof(d));
  d.tensor.data = Fake(0x10000);
  d.tensor.dtype = JXLHIP_TENSOR_F32;
  d.tensor.num_channels = 3;
  d.tensor.stride_x = 1;
  d.tensor.stride_y = out_w;
  d.tensor.stride_c = int64_t(out_w) * out_h;
  d.tensor.bytes = size_t(3) * out_w * out_h * 4;
  for (int c = 0; c < 4; c++) {
    d.tensor.scale[c] = 1.0f;
    d.tensor.bias[c] = 0.0f;
  }
  d.out_xsize = out_w;
  d.out_ysize = out_h;
  d.filter = JXLHIP_RESAMPLE_TRIANGLE;
  return d;
}

template <typename F>
static void Refuses(const JxlHipResizedOut& good, uint32_t w, uint32_t h, int rule, F breaker) {
  int got = -1;
  EXPECT(CheckResizedOut(good, w, h, &got) == 0);
  EXPECT(got == -1);
  JxlHipResizedOut bad = good;
  breaker(bad);
  EXPECT(CheckResizedOut(bad, w, h, &got) == JXLHIP_ERR_INVALID_ARGUMENT);
  if (got != rule) {
    printf("FAILED: expected rule %s, refused by %s\n", RuleName(rule), RuleName(got));
    g_failures++;
  }
  EXPECT(CheckResizedOut(bad, w, h) == JXLHIP_ERR_INVALID_ARGUMENT);  // (without the out-parameter)
  g_exercised.insert(RuleName(rule));
}

static void Rules() {
  const JxlHipResizedOut g = Good(224, 200);
  Refuses(g, 520, 300, kResampleRuleOutput, [](JxlHipResizedOut& d) { d.out_xsize = 0; });
  Refuses(g, 520, 300, kResampleRuleOutput, [](JxlHipResizedOut& d) { d.out_ysize = 0; });
  Refuses(g, 520, 300, kResampleRuleFilter, [](JxlHipResizedOut& d) { d.filter = 1; });
  Refuses(g, 520, 300, kResampleRuleFilter, [](JxlHipResizedOut& d) { d.filter = 0xFFFFFFFFu; });
  Refuses(g, 520, 300, kResampleRuleOutLimit, [](JxlHipResizedOut& d) { d.out_xsize = kMaxOutExtent + 1; });
  Refuses(g, 520, 300, kResampleRuleOutLimit, [](JxlHipResizedOut& d) { d.out_ysize = 0xFFFFFFFFu; });
  Refuses(g, 520, 300, kResampleRuleBoxExtents, [](JxlHipResizedOut& d) { d.box_xsize = 10; });
  Refuses(g, 520, 300, kResampleRuleBoxExtents, [](JxlHipResizedOut& d) { d.box_ysize = 10; });
  Refuses(g, 520, 300, kResampleRuleBoxExtents, [](JxlHipResizedOut& d) { d.box_x0 = 1; });  // (an origin without extents)
  JxlHipResizedOut b = g;
  b.box_x0 = 20; b.box_y0 = 30; b.box_xsize = 500; b.box_ysize = 270;  // touches the right and the bottom edge
  Refuses(b, 520, 300, kResampleRuleBoxInside, [](JxlHipResizedOut& d) { d.box_x0 = 21; });
  Refuses(b, 520, 300, kResampleRuleBoxInside, [](JxlHipResizedOut& d) { d.box_ysize = 271; });
  // near 2^32: the sums are taken in 64 bits (a 32-bit sum wraps to a small number and would be taken)
  Refuses(b, 520, 300, kResampleRuleBoxInside, [](JxlHipResizedOut& d) { d.box_x0 = 0xFFFFFFFFu; d.box_xsize = 2; });
  Refuses(b, 520, 300, kResampleRuleBoxInside, [](JxlHipResizedOut& d) { d.box_y0 = 0x80000000u; d.box_ysize = 0x80000000u; });
  Refuses(b, 520, 300, kResampleRuleBoxInside, [](JxlHipResizedOut& d) { d.box_x0 = 1; d.box_xsize = 0xFFFFFFFFu; });
  Refuses(b, kAnyImageExtent, kAnyImageExtent, kResampleRuleBoxInside, [](JxlHipResizedOut& d) { d.box_x0 = 0xFFFFFFFFu; d.box_xsize = 2; });
  EXPECT(CheckResizedOut(b, 0, 300) == JXLHIP_ERR_INVALID_ARGUMENT);  // (no image)
  {  // without an image every box that fits 32 bits is taken
    JxlHipResizedOut big = b;
    big.box_x0 = 0xFFFFFFF0u; big.box_xsize = 15; big.box_y0 = 0; big.box_ysize = 0xFFFFFFFFu;
    EXPECT(CheckResizedOut(big, kAnyImageExtent, kAnyImageExtent) == 0);
    EXPECT(CheckResizedOut(big, 0xFFFFFFFEu, kAnyImageExtent) == JXLHIP_ERR_INVALID_ARGUMENT);
  }
  // the embedded tensor is held at the OUTPUT size: one row more than the tensor has room for; and its own rules
  Refuses(g, 520, 300, kResampleRuleTensor, [](JxlHipResizedOut& d) { d.tensor.bytes -= 4; });
  Refuses(g, 520, 300, kResampleRuleTensor, [](JxlHipResizedOut& d) { d.out_ysize = 201; });
  Refuses(g, 520, 300, kResampleRuleTensor, [](JxlHipResizedOut& d) { d.tensor.data = nullptr; });
  Refuses(g, 520, 300, kResampleRuleTensor, [](JxlHipResizedOut& d) { d.tensor.num_channels = 5; });
  {
    JxlHipResizedOut bad = g;
    bad.tensor.dtype = JXLHIP_TENSOR_U8;
    bad.tensor.scale[1] = 2.0f;
    int rule = -1, trule = -1;
    EXPECT(CheckResizedOut(bad, 520, 300, &rule, &trule) == JXLHIP_ERR_INVALID_ARGUMENT);
    EXPECT(rule == kResampleRuleTensor && trule == jxlhip::tensor_out::kTensorRuleU8Identity);
  }
  {  // the image's own size plays no part in the tensor's room: a tensor far smaller than the image is taken
    const JxlHipResizedOut tiny = Good(1, 1);
    EXPECT(CheckResizedOut(tiny, 16384, 16384) == 0);
    const Box whole = BoxOf(tiny, 16384, 9000);
    EXPECT(whole.x0 == 0 && whole.y0 == 0 && whole.xsize == 16384 && whole.ysize == 9000);
    const Box part = BoxOf(b, 520, 300);
    EXPECT(part.x0 == 20 && part.y0 == 30 && part.xsize == 500 && part.ysize == 270);
  }
  EXPECT(int(g_exercised.size()) == kResampleRuleCount);
}

struct Axis {
  uint32_t n_in, n_out;
};

// One axis: the table in heap blocks of exactly the sizes the header states.
static void CheckAxis(const Axis& a, FILE* dump) {
  const uint64_t bound = AxisWeightBound(a.n_in, a.n_out);
  std::vector<uint32_t> first(a.n_out), count(a.n_out);
  float* weights = static_cast<float*>(malloc(bound * sizeof(float)));  // (exactly the bound: ASan sees a write behind it)
  const int64_t total = MakeAxisTaps(a.n_in, a.n_out, first.data(), count.data(), weights, bound);
  EXPECT(total > 0 && uint64_t(total) <= bound);
  if (total <= 0) {
    free(weights);
    return;
  }
  uint64_t at = 0;
  uint32_t longest = 0;
  for (uint32_t i = 0; i < a.n_out; i++) {
    EXPECT(count[i] >= 1 && uint64_t(first[i]) + count[i] <= a.n_in);
    if (i) EXPECT(first[i] >= first[i - 1] && first[i] + count[i] >= first[i - 1] + count[i - 1]);  // (the kernels' tile spans rely on it)
    double sum = 0.0;
    for (uint32_t k = 0; k < count[i]; k++) {
      EXPECT(weights[at + k] >= 0.0f && weights[at + k] <= 1.0f);
      sum += double(weights[at + k]);
    }
    if (!(fabs(sum - 1.0) <= ldexp(1.0, -23) * count[i])) {
      printf("FAILED: %u -> %u row %u sums to %.17g over %u taps\n", a.n_in, a.n_out, i, sum, count[i]);
      g_failures++;
    }
    if (count[i] > longest) longest = count[i];
    at += count[i];
  }
  EXPECT(at == uint64_t(total));
  // (the header's argument for its bound: when upscaling 2 taps per row, a third in at most n_in rows; when downscaling at
  // most 2 * support + 2 per row)
  const double support = a.n_in > a.n_out ? double(a.n_in) / a.n_out : 1.0;
  EXPECT(a.n_in > a.n_out ? double(longest) <= 2.0 * support + 2.0 : (longest <= 3 && at <= 2 * uint64_t(a.n_out) + a.n_in));
  {  // a room one float short is refused, and the block of exactly that room is not written past
    float* small = static_cast<float*>(malloc((total - 1 + (total == 1)) * sizeof(float)));
    std::vector<uint32_t> f2(a.n_out), c2(a.n_out);
    EXPECT(MakeAxisTaps(a.n_in, a.n_out, f2.data(), c2.data(), small, uint64_t(total) - 1) == -1);
    free(small);
  }
  {  // the placed table: a heap block of exactly AxisTableBytes, offsets = running sum, device addresses relative to the base
    const size_t bytes = AxisTableBytes(a.n_in, a.n_out);
    uint8_t* block = static_cast<uint8_t*>(malloc(bytes));
    AxisDev dev;
    const uintptr_t base = 0x7000000;
    EXPECT(PlaceAxisTable(a.n_in, a.n_out, block, base, &dev) == total);
    const uint32_t* pf = reinterpret_cast<const uint32_t*>(block);
    EXPECT(memcmp(pf, first.data(), a.n_out * 4) == 0 && memcmp(pf + a.n_out, count.data(), a.n_out * 4) == 0);
    uint32_t run = 0;
    for (uint32_t i = 0; i < a.n_out; i++) {
      EXPECT(pf[2 * a.n_out + i] == run);
      run += count[i];
    }
    EXPECT(memcmp(pf + 3 * a.n_out, weights, size_t(total) * 4) == 0);
    EXPECT(uintptr_t(dev.first) == base && uintptr_t(dev.count) == base + 4 * a.n_out && uintptr_t(dev.offset) == base + 8 * a.n_out &&
           uintptr_t(dev.weights) == base + 12 * a.n_out);
    EXPECT(uintptr_t(dev.weights) + size_t(total) * 4 <= base + bytes);
    free(block);
  }
  if (dump) {
    const uint32_t head[3] = {a.n_in, a.n_out, uint32_t(total)};
    fwrite(head, 4, 3, dump);
    fwrite(first.data(), 4, a.n_out, dump);
    fwrite(count.data(), 4, a.n_out, dump);
    fwrite(weights, 4, size_t(total), dump);
  }
  free(weights);
}

// A context's block: descriptor and both tables in a heap block of exactly LayoutOf(...).bytes.
static void Blocks() {
  JxlHipResizedOut d = Good(7, 224);
  d.tensor.clamp01 = 1;
  d.tensor.scale[2] = 0.5f;
  d.tensor.bias[1] = -2.0f;
  d.box_x0 = 3; d.box_y0 = 5; d.box_xsize = 600; d.box_ysize = 290;
  EXPECT(CheckResizedOut(d, 640, 300) == 0);
  const Box b = BoxOf(d, 640, 300);
  const BlockLayout l = LayoutOf(b, d.out_xsize, d.out_ysize);
  EXPECT(l.desc == 0 && l.x >= sizeof(ResampleDev) && l.x % 16 == 0 && l.y % 16 == 0 && l.y >= l.x + AxisTableBytes(600, 7) &&
         l.bytes >= l.y + AxisTableBytes(290, 224));
  uint8_t* block = static_cast<uint8_t*>(malloc(l.bytes));
  const uintptr_t base = 0x9000000;
  const float* src = static_cast<const float*>(Fake(0x100000));
  float* tmp = static_cast<float*>(Fake(0x200000));
  EXPECT(PlaceBlock(d, b, src, 640, tmp, block, base) == 0);
  ResampleDev r;
  memcpy(&r, block, sizeof(r));
  EXPECT(r.src == src && r.tmp == tmp && r.dst == d.tensor.data && r.src_row == 640 && r.nc == 3);
  EXPECT(r.box_x0 == 3 && r.box_y0 == 5 && r.box_xsize == 600 && r.box_ysize == 290 && r.out_xsize == 7 && r.out_ysize == 224);
  EXPECT(r.stride_c == d.tensor.stride_c && r.stride_y == 7 && r.stride_x == 1 && r.dtype == JXLHIP_TENSOR_F32 && r.clamp01 == 1);
  EXPECT(r.scale[2] == 0.5f && r.bias[1] == -2.0f && r.scale[0] == 1.0f);
  EXPECT(uintptr_t(r.x.first) == base + l.x && uintptr_t(r.y.first) == base + l.y);
  EXPECT(r.v_tile0 == 0 && r.h_tile0 == 0);
  EXPECT(r.v_tiles == ((600 * 3 + kVTileCols - 1) / kVTileCols) * ((224 + kVTileRows - 1) / kVTileRows));
  EXPECT(r.h_tiles == 224 * ((7 + kHTileCols - 1) / kHTileCols));
  EXPECT(TmpBytes(b, 3, 224) == size_t(224) * 600 * 3 * 4);
  free(block);
}

int main(int argc, char** argv) {
  Rules();
  FILE* dump = argc > 1 ? fopen(argv[1], "wb") : nullptr;
  if (argc > 1 && !dump) {
    printf("cannot write %s\n", argv[1]);
    return 2;
  }
  int axes = 0;
  for (int i = 2; i < argc; i++) {
    Axis a;
    if (sscanf(argv[i], "%u:%u", &a.n_in, &a.n_out) != 2) {
      printf("not an axis: %s\n", argv[i]);
      return 2;
    }
    CheckAxis(a, dump);
    axes++;
  }
  if (dump) fclose(dump);
  // every pair of small extents, for the bound and the sums (no dump)
  for (uint32_t n_in = 1; n_in <= 40; n_in++)
    for (uint32_t n_out = 1; n_out <= 40; n_out++) CheckAxis(Axis{n_in, n_out}, nullptr);
  Blocks();
  {
    uint32_t f, c;
    float w;
    EXPECT(MakeAxisTaps(0, 4, &f, &c, &w, 1) == -1 && MakeAxisTaps(4, 0, &f, &c, &w, 1) == -1);
  }
  std::string names;
  for (const std::string& n : g_exercised) names += " " + n;
  printf("exercised:%s\n", names.c_str());
  printf("axes: %d\n", axes);
  printf(g_failures ? "%d failures\n" : "ok\n", g_failures);
  return g_failures ? 1 : 0;
}
