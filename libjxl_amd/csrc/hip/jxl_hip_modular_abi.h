// libjxl_amd — the plain-data structs the Modular kernels (jxl_hip_modular.h) read from device memory, free of HIP
// constructs: a plain C++ compile (csrc/host/jxh_modular_upload_plan.h, the CPU tests) fills the very blocks the kernels
// take. The static_asserts below pin sizes and field offsets, so that neither side can drift from the other.
#ifndef JXL_HIP_MODULAR_ABI_H_
#define JXL_HIP_MODULAR_ABI_H_

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <stddef.h>
#include <stdint.h>

namespace jxlhip {

#ifdef __HIPCC__
typedef uint2 ModAliasEntry;
#else
struct ModAliasEntry {  // the host spelling of uint2: two 32-bit words, 8-byte aligned
  alignas(8) uint32_t x;
  uint32_t y;
};
#endif

struct ModTreeNode {  // 16 bytes (BuildModBlob packs the boundary's nodes): one load per step of the walk
  int32_t property;   // decision: the property tested (>= 0); leaf: -1 - predictor
  int32_t splitval;   // leaf: offset
  uint32_t lchild;    // leaf: histogram (the context already mapped through the code's context map)
  uint32_t rchild;    // leaf: multiplier
};

struct ModCode {  // one entropy code (global or local to a stream); pointers into device memory
  const uint8_t* ctx_map;      // context -> cluster
  const ModAliasEntry* alias;  // cluster << log_alpha (ANS)
  const uint32_t* cfg;         // per cluster: split_exp | msb << 8 | lsb << 16
  const uint32_t* prefix_table;
  const uint32_t* prefix_offset;
  uint32_t log_alpha, use_prefix, lz77, lz_min_symbol, lz_min_length, lz_len_cfg, lz_dist_ctx;
  uint32_t table_words;     // 32-bit words of the symbol tables a wave may stage in LDS: the alias table (ANS) or the prefix
                            // table, then one word per cluster (cfg), then for prefix codes one more per cluster (offsets)
  uint32_t num_clusters, pad[3];
};

struct ModChannel {  // one channel of a stream: a rectangle of a frame channel buffer
  int32_t* data;     // top-left sample of the rectangle
  uint32_t stride;   // samples per row of the underlying buffer
  uint32_t w, h;
  uint32_t sig;      // channels of a stream with equal `sig` have identical size and shifts ("previous channel" properties)
};

struct ModStream {
  const uint32_t* words;   // section bytes (4-byte aligned start)
  uint32_t bit_offset;     // where the stream's sample data begins
  uint32_t size_bytes;     // section size: reads beyond it are zero, consuming beyond it is an error
  const ModTreeNode* tree;
  uint32_t tree_nodes;
  const ModCode* code;
  const ModChannel* channels;
  uint32_t num_channels;
  uint32_t stream_id;      // MA property 1
  uint32_t first_channel_index;  // MA property 0 of channels[0] (the following count up)
  int32_t wp[11];          // weighted predictor header: p1C p2C p3Ca..p3Ce, w0..w3
  uint32_t uses_wp;        // the tree tests property 15 or predicts with predictor 6
  uint32_t num_props;      // 16 + 4 * referenced previous channels
  uint32_t dist_multiplier;
  int32_t* wp_scratch;     // 5 arrays of 2 * (max width + 2) ints (uses_wp only)
  uint32_t* lz_window;     // lz_window_mask + 1 entries (code->lz77 only)
  uint32_t lz_window_mask;
  uint32_t* status;        // out: 0 ok, bit 0 = ANS final state, bit 1 = over-read, bit 2 = LZ77 length overflow
  uint32_t* end_bit;       // out: bit position after the last sample
};

constexpr uint32_t kModWpEntry = 8;       // ints per row entry of the weighted predictor's scratch
constexpr int kModMaxProps = 16 + 4 * 4;  // property 15 + up to four referenced previous channels (host refuses trees beyond)

// k_modular_streams and its launch (csrc/host/jxh_modular_launch_plan.h) share these.
constexpr uint32_t kModTreeLdsNodes = 2048;   // largest tree kept in LDS (32 KB)
constexpr uint32_t kModTableLdsWords = 8192;  // largest symbol-table set kept in LDS (32 KB)
// Dynamic LDS of a workgroup (one wave, `lanes` streams): the properties [property][lane], then `tree_cap` tree nodes,
// then `table_cap` words of symbol tables.
constexpr uint32_t ModLdsBytes(uint32_t lanes, uint32_t tree_cap, uint32_t table_cap) {
  return kModMaxProps * lanes * 4 + tree_cap * 16 + table_cap * 4 + 64 * 4;  // (+ the weighted predictor's division table)
}

// ---- inverse transforms on channel rectangles: whole channels for the frame's own transforms, a group's rectangle of the
// frame's buffers (or a private buffer) for the transforms of a group stream. The blocks carry pointers to the first
// sample of each rectangle and the strides of the buffers they lie in.
struct ModRct {
  int32_t* c[3];  // the three channels in stored order
  uint32_t stride[3];
  uint32_t w, h, type;
};
struct ModUnsqueeze {
  const int32_t* avg;
  const int32_t* res;
  int32_t* out;
  uint32_t lines, na, nr;             // lines to do; averages / residuals per line
  uint32_t avg_line, avg_step, res_line, res_step, out_line, out_step;  // strides between lines / between samples of a line
};
struct ModPalette {  // palette.cc:26-202, the form without delta entries and predictor (nb_deltas == 0, predictor 0)
  const int32_t* palette;  // [nb_channels][palette_w]
  const int32_t* index;    // the index channel's rectangle
  int32_t* out[4];         // the output rectangles; out[0] may be the index rectangle itself
  uint32_t palette_w, nb, w, h, bit_depth, index_stride, out_stride[4];
};

static_assert(sizeof(void*) == 8, "device pointers are 64-bit");
static_assert(sizeof(ModAliasEntry) == 8 && alignof(ModAliasEntry) == 8, "uint2");
static_assert(sizeof(ModTreeNode) == 16 && offsetof(ModTreeNode, lchild) == 8, "ModTreeNode");
static_assert(sizeof(ModCode) == 88 && offsetof(ModCode, prefix_offset) == 32 && offsetof(ModCode, log_alpha) == 40 &&
                  offsetof(ModCode, table_words) == 68 && offsetof(ModCode, num_clusters) == 72,
              "ModCode");
static_assert(sizeof(ModChannel) == 24 && offsetof(ModChannel, stride) == 8 && offsetof(ModChannel, sig) == 20, "ModChannel");
static_assert(sizeof(ModStream) == 160 && offsetof(ModStream, tree) == 16 && offsetof(ModStream, code) == 32 && offsetof(ModStream, channels) == 40 &&
                  offsetof(ModStream, num_channels) == 48 && offsetof(ModStream, wp) == 60 && offsetof(ModStream, uses_wp) == 104 &&
                  offsetof(ModStream, wp_scratch) == 120 && offsetof(ModStream, lz_window_mask) == 136 && offsetof(ModStream, status) == 144 &&
                  offsetof(ModStream, end_bit) == 152,
              "ModStream");
static_assert(sizeof(ModRct) == 48 && offsetof(ModRct, stride) == 24 && offsetof(ModRct, type) == 44, "ModRct");
static_assert(sizeof(ModUnsqueeze) == 64 && offsetof(ModUnsqueeze, lines) == 24 && offsetof(ModUnsqueeze, out_step) == 56, "ModUnsqueeze");
static_assert(sizeof(ModPalette) == 88 && offsetof(ModPalette, out) == 16 && offsetof(ModPalette, palette_w) == 48 && offsetof(ModPalette, out_stride) == 72,
              "ModPalette");

}  // namespace jxlhip
#endif  // JXL_HIP_MODULAR_ABI_H_
