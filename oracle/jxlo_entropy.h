// ORACLE (test infrastructure): entropy decoding — histograms, rANS with alias tables, prefix codes,
// hybrid integers, LZ77, context maps.
// Follows: reference lib/jxl/dec_ans.{h,cc} (ReadHistogram :58-191, DecodeANSCodes :195-271,
// DecodeUintConfig :272-295, DecodeHistograms :341-376, symbol reader dec_ans.h:170-353),
// lib/jxl/ans_common.{h,cc} (alias table construction/lookup), lib/jxl/dec_huffman.cc and
// lib/jxl/huffman_table.cc (Brotli-style prefix codes), lib/jxl/dec_context_map.cc:48-95,
// lib/jxl/inverse_mtf-inl.h:55-72.
#ifndef JXLO_ENTROPY_H_
#define JXLO_ENTROPY_H_

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "jxlo_bits.h"

namespace jxlo {

static const int kAnsLogTab = 12;
static const int kAnsTab = 1 << kAnsLogTab;
static const uint32_t kAnsSignature = 0x13;
static const size_t kLzWindow = 1 << 20;

struct HybridCfg {
  uint32_t split_exp = 4, split_token = 16, msb = 2, lsb = 0;
};

struct AliasEntry {  // one per table bucket
  uint8_t cutoff;
  uint8_t right_value;
  uint16_t freq0;
  uint16_t offsets1;
  uint16_t freq1;
};

// Prefix code decoding table: index by the next `max_len` bits (LSB first).
struct PrefixCode {
  int max_len = 0;
  std::vector<uint16_t> sym;  // size 1<<max_len
  std::vector<uint8_t> len;
};

struct EntropyCode {
  bool use_prefix = false;
  int log_alpha = 8;
  std::vector<HybridCfg> cfg;           // per cluster
  std::vector<AliasEntry> alias;        // cluster << log_alpha
  std::vector<PrefixCode> prefix;       // per cluster
  std::vector<int> degenerate;          // per cluster (-1 if not single-symbol)
  // per cluster as parsed, kept for the tests' export of the tables: symbol frequencies (rANS) or code lengths (prefix; a
  // single non-zero length is the zero-bit code of that symbol)
  std::vector<std::vector<int32_t>> parsed;
  bool lz77 = false;
  uint32_t lz_min_symbol = 224, lz_min_length = 3;
  HybridCfg lz_len_cfg;
  uint32_t lz_dist_ctx = 0;  // clustered
  size_t max_num_bits = 0;
  std::vector<uint8_t> ctx_map;  // context -> cluster
  size_t num_clusters = 1;
};

// ---- alias table (must reproduce the reference construction exactly: it defines the symbol<->slot map)
static inline void InitAliasTable(std::vector<int32_t> dist, int log_alpha, AliasEntry* a) {
  const uint32_t range = kAnsTab;
  const size_t table_size = size_t(1) << log_alpha;
  while (!dist.empty() && dist.back() == 0) dist.pop_back();
  if (dist.empty()) dist.push_back(range);
  JXLO_CHECK(dist.size() <= table_size, "alphabet too large for alias table");
  const uint32_t entry_size = range >> log_alpha;
  int single = -1;
  int64_t sum = 0;
  for (size_t s = 0; s < dist.size(); s++) {
    sum += dist[s];
    if (dist[s] == (int32_t)range) single = int(s);
  }
  JXLO_CHECK(sum == range, "histogram does not sum to 4096");
  if (single >= 0) {
    for (size_t i = 0; i < table_size; i++) {
      a[i].right_value = uint8_t(single);
      a[i].cutoff = 0;
      a[i].offsets1 = uint16_t(entry_size * i);
      a[i].freq0 = 0;
      a[i].freq1 = uint16_t(range);  // stored as 4096 -> wraps to 4096 in 16 bits (fits)
    }
    return;
  }
  std::vector<uint32_t> underfull, overfull, cutoffs(table_size);
  for (size_t i = 0; i < dist.size(); i++) {
    cutoffs[i] = dist[i];
    if (cutoffs[i] > entry_size) overfull.push_back(i);
    else if (cutoffs[i] < entry_size) underfull.push_back(i);
  }
  for (size_t i = dist.size(); i < table_size; i++) {
    cutoffs[i] = 0;
    underfull.push_back(i);
  }
  std::vector<uint32_t> offs1(table_size, 0), right(table_size, 0);
  while (!overfull.empty()) {
    uint32_t o = overfull.back();
    overfull.pop_back();
    JXLO_CHECK(!underfull.empty(), "alias table construction failed");
    uint32_t u = underfull.back();
    underfull.pop_back();
    uint32_t by = entry_size - cutoffs[u];
    cutoffs[o] -= by;
    right[u] = o;
    offs1[u] = cutoffs[o];
    if (cutoffs[o] < entry_size) underfull.push_back(o);
    else if (cutoffs[o] > entry_size) overfull.push_back(o);
  }
  for (size_t i = 0; i < table_size; i++) {
    if (cutoffs[i] == entry_size) {
      right[i] = i;
      offs1[i] = 0;
      a[i].cutoff = 0;
    } else {
      offs1[i] -= cutoffs[i];
      a[i].cutoff = uint8_t(cutoffs[i]);
    }
    a[i].right_value = uint8_t(right[i]);
    a[i].offsets1 = uint16_t(offs1[i]);
    a[i].freq0 = uint16_t(i < dist.size() ? dist[i] : 0);
    a[i].freq1 = uint16_t(right[i] < dist.size() ? dist[right[i]] : 0);
  }
}

// ---- prefix codes
static inline void BuildPrefixFromLengths(const std::vector<uint8_t>& lens, PrefixCode* pc) {
  int max_len = 0, nonzero = 0, last = 0;
  for (size_t i = 0; i < lens.size(); i++)
    if (lens[i]) {
      max_len = std::max<int>(max_len, lens[i]);
      nonzero++;
      last = int(i);
    }
  if (nonzero <= 1) {  // zero-bit code
    pc->max_len = 0;
    pc->sym.assign(1, uint16_t(last));
    pc->len.assign(1, 0);
    return;
  }
  pc->max_len = max_len;
  pc->sym.assign(size_t(1) << max_len, 0);
  pc->len.assign(size_t(1) << max_len, 0);
  uint32_t code = 0;
  size_t filled = 0;
  for (int l = 1; l <= max_len; l++) {
    for (size_t s = 0; s < lens.size(); s++) {
      if (lens[s] != l) continue;
      // canonical code `code` of length l, transmitted MSB first => reverse for LSB-first lookup
      uint32_t rev = 0;
      for (int b = 0; b < l; b++) rev |= ((code >> b) & 1) << (l - 1 - b);
      for (size_t k = rev; k < pc->sym.size(); k += size_t(1) << l) {
        pc->sym[k] = uint16_t(s);
        pc->len[k] = uint8_t(l);
      }
      filled += size_t(1) << (max_len - l);
      code++;
    }
    code <<= 1;
  }
  JXLO_CHECK(filled == pc->sym.size(), "prefix code is not complete");
}

static inline void ReadPrefixCode(BitReader& br, size_t alphabet_size, PrefixCode* pc, std::vector<uint8_t>* lens_out = nullptr) {
  JXLO_CHECK(alphabet_size <= (1u << 15), "prefix alphabet too large");
  std::vector<uint8_t> lens_local(alphabet_size, 0);
  if (lens_out) lens_out->assign(alphabet_size, 0);
  std::vector<uint8_t>& lens = lens_out ? *lens_out : lens_local;
  uint32_t hskip = uint32_t(br.Read(2));
  if (hskip == 1) {  // simple code: 1..4 explicit symbols
    int max_bits = alphabet_size > 1 ? FloorLog2(alphabet_size - 1) + 1 : 0;
    int n = int(br.Read(2)) + 1;
    uint16_t s[4] = {0, 0, 0, 0};
    for (int i = 0; i < n; i++) {
      s[i] = uint16_t(br.Read(max_bits));
      JXLO_CHECK(s[i] < alphabet_size, "simple prefix symbol out of range");
    }
    for (int i = 0; i < n; i++)
      for (int j = i + 1; j < n; j++) JXLO_CHECK(s[i] != s[j], "duplicate simple prefix symbol");
    if (n == 1) {
      lens[s[0]] = 1;  // single symbol => zero-bit code (handled by builder)
      pc->max_len = 0;
      pc->sym.assign(1, s[0]);
      pc->len.assign(1, 0);
      return;
    } else if (n == 2) {
      lens[s[0]] = lens[s[1]] = 1;
    } else if (n == 3) {
      lens[s[0]] = 1;
      lens[s[1]] = lens[s[2]] = 2;
    } else {
      bool tree_select = br.Read(1) != 0;
      if (!tree_select) {
        lens[s[0]] = lens[s[1]] = lens[s[2]] = lens[s[3]] = 2;
      } else {
        lens[s[0]] = 1;
        lens[s[1]] = 2;
        lens[s[2]] = lens[s[3]] = 3;
      }
    }
    BuildPrefixFromLengths(lens, pc);
    return;
  }
  // complex code: code-length code first
  static const uint8_t kOrder[18] = {1, 2, 3, 4, 0, 5, 17, 6, 16, 7, 8, 9, 10, 11, 12, 13, 14, 15};
  uint8_t cl_lens[18] = {0};
  int space = 32, num_codes = 0;
  for (size_t i = hskip; i < 18 && space > 0; i++) {
    // fixed code for the code-length-code lengths (values 0..5)
    uint32_t v4 = uint32_t(br.Peek(4));
    int val, nb;
    if ((v4 & 3) == 0) { val = 0; nb = 2; }
    else if ((v4 & 3) == 1) { val = 4; nb = 2; }
    else if ((v4 & 3) == 2) { val = 3; nb = 2; }
    else if ((v4 & 7) == 3) { val = 2; nb = 3; }
    else if ((v4 & 15) == 7) { val = 1; nb = 4; }
    else { val = 5; nb = 4; }
    br.Skip(nb);
    cl_lens[kOrder[i]] = uint8_t(val);
    if (val) {
      space -= 32 >> val;
      num_codes++;
    }
  }
  JXLO_CHECK(num_codes == 1 || space == 0, "invalid code length code");
  PrefixCode clc;
  BuildPrefixFromLengths(std::vector<uint8_t>(cl_lens, cl_lens + 18), &clc);
  size_t symbol = 0;
  uint8_t prev_len = 8, repeat_len = 0;
  int repeat = 0;
  int sp = 32768;
  while (symbol < alphabet_size && sp > 0) {
    uint32_t idx = clc.max_len ? uint32_t(br.Peek(clc.max_len)) : 0;
    br.Skip(clc.len[idx]);
    uint8_t code_len = uint8_t(clc.sym[idx]);
    if (code_len < 16) {
      repeat = 0;
      lens[symbol++] = code_len;
      if (code_len) {
        prev_len = code_len;
        sp -= 32768 >> code_len;
      }
    } else {
      int extra = code_len - 14;
      uint8_t new_len = code_len == 16 ? prev_len : 0;
      if (repeat_len != new_len) {
        repeat = 0;
        repeat_len = new_len;
      }
      int old = repeat;
      if (repeat > 0) {
        repeat -= 2;
        repeat <<= extra;
      }
      repeat += int(br.Read(extra)) + 3;
      int delta = repeat - old;
      JXLO_CHECK(symbol + delta <= alphabet_size, "prefix code length repeat overflow");
      for (int k = 0; k < delta; k++) lens[symbol++] = repeat_len;
      if (repeat_len) sp -= delta << (15 - repeat_len);
    }
  }
  JXLO_CHECK(sp == 0, "prefix code lengths do not fill the code space");
  BuildPrefixFromLengths(lens, pc);
}

// ---- histogram for rANS
static inline int VarLenU8(BitReader& br) {
  if (!br.Read(1)) return 0;
  int n = int(br.Read(3));
  return n == 0 ? 1 : int(br.Read(n)) + (1 << n);
}
static inline int VarLenU16(BitReader& br) {
  if (!br.Read(1)) return 0;
  int n = int(br.Read(4));
  return n == 0 ? 1 : int(br.Read(n)) + (1 << n);
}
static inline uint32_t PopCountPrecision(uint32_t logcount, uint32_t shift) {
  int r = std::min<int>(int(logcount), int(shift) - int((kAnsLogTab - logcount) >> 1));
  return r < 0 ? 0 : uint32_t(r);
}

static inline void ReadHistogram(BitReader& br, std::vector<int32_t>* counts) {
  const int range = kAnsTab;
  if (br.Read(1)) {  // one or two symbols
    int n = int(br.Read(1)) + 1;
    int sym[2] = {0, 0}, mx = 0;
    for (int i = 0; i < n; i++) {
      sym[i] = VarLenU8(br);
      mx = std::max(mx, sym[i]);
    }
    counts->assign(mx + 1, 0);
    if (n == 1) {
      (*counts)[sym[0]] = range;
    } else {
      JXLO_CHECK(sym[0] != sym[1], "histogram: repeated symbol");
      (*counts)[sym[0]] = int32_t(br.Read(kAnsLogTab));
      (*counts)[sym[1]] = range - (*counts)[sym[0]];
    }
    return;
  }
  if (br.Read(1)) {  // flat
    int alpha = VarLenU8(br) + 1;
    JXLO_CHECK(alpha <= range, "flat histogram too large");
    counts->assign(alpha, range / alpha);
    for (int i = 0; i < range % alpha; i++) (*counts)[i]++;
    return;
  }
  uint32_t shift;
  {
    int ub = FloorLog2(kAnsLogTab + 1), log = 0;
    for (; log < ub; log++)
      if (!br.Read(1)) break;
    shift = (uint32_t(br.Read(log)) | (1u << log)) - 1;
    JXLO_CHECK(shift <= kAnsLogTab + 1, "histogram: invalid shift");
  }
  const size_t length = VarLenU8(br) + 3;
  counts->assign(length, 0);
  // fixed prefix code for log-counts: {bit pattern (LSB first), length, value}
  static const uint8_t kLC[14][3] = {{0, 3, 10}, {1, 7, 12}, {2, 3, 7},  {3, 4, 3},  {4, 3, 6},
                                     {5, 3, 8},  {6, 3, 9},  {7, 4, 5},  {9, 4, 4},  {11, 4, 1},
                                     {15, 4, 2}, {17, 5, 0}, {33, 6, 11}, {65, 7, 13}};
  std::vector<int> logcounts(length), same(length, 0);
  int omit_log = -1, omit_pos = -1;
  for (size_t i = 0; i < length; ++i) {
    uint32_t v = uint32_t(br.Peek(7));
    int val = -1;
    for (int k = 0; k < 14; k++) {
      if ((v & ((1u << kLC[k][1]) - 1)) == kLC[k][0]) {
        val = kLC[k][2];
        br.Skip(kLC[k][1]);
        break;
      }
    }
    JXLO_CHECK(val >= 0, "histogram: bad log-count code");
    logcounts[i] = val - 1;
    if (logcounts[i] == kAnsLogTab) {  // RLE marker
      int rle = VarLenU8(br);
      same[i] = rle + 5;
      i += rle + 3;
      continue;
    }
    if (logcounts[i] > omit_log) {
      omit_log = logcounts[i];
      omit_pos = int(i);
    }
  }
  JXLO_CHECK(omit_pos >= 0, "histogram: nothing to omit");
  JXLO_CHECK(!(size_t(omit_pos) + 1 < length && logcounts[omit_pos + 1] == kAnsLogTab),
             "histogram: RLE after omitted symbol");
  int prev = 0, numsame = 0, total = 0;
  for (size_t i = 0; i < length; ++i) {
    if (same[i]) {
      numsame = same[i] - 1;
      prev = i > 0 ? (*counts)[i - 1] : 0;
    }
    if (numsame > 0) {
      (*counts)[i] = prev;
      numsame--;
    } else {
      int code = logcounts[i];
      if (int(i) == omit_pos || code < 0) {
        continue;
      } else if (shift == 0 || code == 0) {
        (*counts)[i] = 1 << code;
      } else {
        int bitcount = int(PopCountPrecision(code, shift));
        (*counts)[i] = (1 << code) + (int(br.Read(bitcount)) << (code - bitcount));
      }
    }
    total += (*counts)[i];
  }
  (*counts)[omit_pos] = range - total;
  JXLO_CHECK((*counts)[omit_pos] > 0, "histogram: counts exceed 4096");
}

static inline void ReadHybridCfg(BitReader& br, int log_alpha, HybridCfg* c) {
  c->split_exp = uint32_t(br.Read(CeilLog2(log_alpha + 1)));
  c->msb = c->lsb = 0;
  if (c->split_exp != uint32_t(log_alpha)) {
    c->msb = uint32_t(br.Read(CeilLog2(c->split_exp + 1)));
    JXLO_CHECK(c->msb <= c->split_exp, "invalid hybrid uint config");
    c->lsb = uint32_t(br.Read(CeilLog2(c->split_exp - c->msb + 1)));
  }
  JXLO_CHECK(c->lsb + c->msb <= c->split_exp, "invalid hybrid uint config");
  c->split_token = 1u << c->split_exp;
}

static inline void UpdateMaxBits(EntropyCode* code, size_t cluster, size_t symbol) {
  const HybridCfg* cfg = &code->cfg[cluster];
  if (code->lz77 && code->lz_dist_ctx != cluster && symbol >= code->lz_min_symbol) {
    symbol -= code->lz_min_symbol;
    cfg = &code->lz_len_cfg;
  }
  if (symbol < cfg->split_token) {
    code->max_num_bits = std::max<size_t>(code->max_num_bits, cfg->split_exp);
    return;
  }
  uint32_t extra = cfg->split_exp - (cfg->msb + cfg->lsb) + uint32_t((symbol - cfg->split_token) >> (cfg->msb + cfg->lsb));
  code->max_num_bits = std::max<size_t>(code->max_num_bits, cfg->msb + cfg->lsb + extra + 1);
}

class SymbolReader;
static inline void DecodeHistograms(BitReader& br, size_t num_contexts, EntropyCode* code, bool disallow_lz77 = false);

// ---- symbol reader
class SymbolReader {
 public:
  SymbolReader(const EntropyCode* code, BitReader* br, size_t dist_multiplier = 0) : c_(code), br_(br) {
    if (!c_->use_prefix) {
      state_ = uint32_t(br->Read(32));
    } else {
      state_ = kAnsSignature << 16;
    }
    if (c_->lz77) {
      window_.reset(new uint32_t[kLzWindow]);
      num_special_ = dist_multiplier == 0 ? 0 : 120;
      dist_multiplier_ = int(dist_multiplier);
    }
  }
  uint32_t ReadSymbol(size_t cluster) {
    if (c_->use_prefix) {
      const PrefixCode& pc = c_->prefix[cluster];
      if (pc.max_len == 0) return pc.sym[0];
      uint32_t idx = uint32_t(br_->Peek(pc.max_len));
      br_->Skip(pc.len[idx]);
      return pc.sym[idx];
    }
    const uint32_t res = state_ & (kAnsTab - 1);
    const int log_entry = kAnsLogTab - c_->log_alpha;
    const AliasEntry& e = c_->alias[(cluster << c_->log_alpha) + (res >> log_entry)];
    const uint32_t pos = res & ((1u << log_entry) - 1);
    uint32_t sym, off, freq;
    if (pos >= e.cutoff) {
      sym = e.right_value;
      off = e.offsets1 + pos;
      freq = e.freq1;
    } else {
      sym = res >> log_entry;
      off = pos;
      freq = e.freq0;
    }
    state_ = freq * (state_ >> kAnsLogTab) + off;
    if (state_ < (1u << 16)) {
      state_ = (state_ << 16) | uint32_t(br_->Read(16));
    }
    return sym;
  }
  static uint32_t ReadHybrid(const HybridCfg& cfg, uint32_t token, BitReader* br) {
    if (token < cfg.split_token) return token;
    uint32_t nbits = cfg.split_exp - (cfg.msb + cfg.lsb) + ((token - cfg.split_token) >> (cfg.msb + cfg.lsb));
    nbits &= 31;
    uint32_t low = token & ((1u << cfg.lsb) - 1);
    token >>= cfg.lsb;
    uint64_t bits = br->Read(nbits);
    uint64_t ret = (((((uint64_t(1) << cfg.msb) | (token & ((1u << cfg.msb) - 1))) << nbits) | bits) << cfg.lsb) | low;
    return uint32_t(ret);
  }
  // `cluster` is the clustered context.
  uint32_t ReadClustered(size_t cluster) {
    if (c_->lz77) {
      if (num_to_copy_ > 0) {
        uint32_t r = window_[(copy_pos_++) & (kLzWindow - 1)];
        num_to_copy_--;
        window_[(num_decoded_++) & (kLzWindow - 1)] = r;
        return r;
      }
    }
    uint32_t token = ReadSymbol(cluster);
    if (c_->lz77 && token >= c_->lz_min_symbol) {
      num_to_copy_ = ReadHybrid(c_->lz_len_cfg, token - c_->lz_min_symbol, br_) + c_->lz_min_length;
      uint32_t dtok = ReadSymbol(c_->lz_dist_ctx);
      uint32_t distance = ReadHybrid(c_->cfg[c_->lz_dist_ctx], dtok, br_);
      if (distance < num_special_) {
        distance = SpecialDistance(distance, dist_multiplier_);
      } else {
        distance = distance + 1 - num_special_;
      }
      if (distance > num_decoded_) distance = num_decoded_;
      if (distance > kLzWindow) distance = uint32_t(kLzWindow);
      copy_pos_ = num_decoded_ - distance;
      if (distance == 0) {
        size_t fill = std::min<size_t>(num_to_copy_, kLzWindow);
        memset(window_.get(), 0, fill * sizeof(uint32_t));
      }
      if (num_to_copy_ < c_->lz_min_length) {  // wrapped
        num_to_copy_ = 0;
        throw Error("lz77 copy length overflow");
      }
      uint32_t r = window_[(copy_pos_++) & (kLzWindow - 1)];
      num_to_copy_--;
      window_[(num_decoded_++) & (kLzWindow - 1)] = r;
      return r;
    }
    uint32_t r = ReadHybrid(c_->cfg[cluster], token, br_);
    if (c_->lz77) window_[(num_decoded_++) & (kLzWindow - 1)] = r;
    return r;
  }
  uint32_t Read(size_t ctx) { return ReadClustered(c_->ctx_map[ctx]); }
  bool FinalStateOk() const { return state_ == (kAnsSignature << 16); }

 private:
  static uint32_t SpecialDistance(uint32_t index, int mult) {
    static const int8_t kSD[120][2] = {
        {0, 1},  {1, 0},  {1, 1},  {-1, 1}, {0, 2},  {2, 0},  {1, 2},  {-1, 2}, {2, 1},  {-2, 1}, {2, 2},  {-2, 2},
        {0, 3},  {3, 0},  {1, 3},  {-1, 3}, {3, 1},  {-3, 1}, {2, 3},  {-2, 3}, {3, 2},  {-3, 2}, {0, 4},  {4, 0},
        {1, 4},  {-1, 4}, {4, 1},  {-4, 1}, {3, 3},  {-3, 3}, {2, 4},  {-2, 4}, {4, 2},  {-4, 2}, {0, 5},  {3, 4},
        {-3, 4}, {4, 3},  {-4, 3}, {5, 0},  {1, 5},  {-1, 5}, {5, 1},  {-5, 1}, {2, 5},  {-2, 5}, {5, 2},  {-5, 2},
        {4, 4},  {-4, 4}, {3, 5},  {-3, 5}, {5, 3},  {-5, 3}, {0, 6},  {6, 0},  {1, 6},  {-1, 6}, {6, 1},  {-6, 1},
        {2, 6},  {-2, 6}, {6, 2},  {-6, 2}, {4, 5},  {-4, 5}, {5, 4},  {-5, 4}, {3, 6},  {-3, 6}, {6, 3},  {-6, 3},
        {0, 7},  {7, 0},  {1, 7},  {-1, 7}, {5, 5},  {-5, 5}, {7, 1},  {-7, 1}, {4, 6},  {-4, 6}, {6, 4},  {-6, 4},
        {2, 7},  {-2, 7}, {7, 2},  {-7, 2}, {3, 7},  {-3, 7}, {7, 3},  {-7, 3}, {5, 6},  {-5, 6}, {6, 5},  {-6, 5},
        {8, 0},  {4, 7},  {-4, 7}, {7, 4},  {-7, 4}, {8, 1},  {8, 2},  {6, 6},  {-6, 6}, {8, 3},  {5, 7},  {-5, 7},
        {7, 5},  {-7, 5}, {8, 4},  {6, 7},  {-6, 7}, {7, 6},  {-7, 6}, {8, 5},  {7, 7},  {-7, 7}, {8, 6},  {8, 7}};
    int d = kSD[index][0] + mult * kSD[index][1];
    return d > 1 ? uint32_t(d) : 1u;
  }
  const EntropyCode* c_;
  BitReader* br_;
  uint32_t state_;
  std::unique_ptr<uint32_t[]> window_;
  uint32_t num_decoded_ = 0, num_to_copy_ = 0, copy_pos_ = 0, num_special_ = 0;
  int dist_multiplier_ = 0;
};

static inline void InverseMtf(uint8_t* v, size_t n) {
  uint8_t mtf[256];
  for (int i = 0; i < 256; i++) mtf[i] = uint8_t(i);
  for (size_t i = 0; i < n; i++) {
    uint8_t idx = v[i];
    uint8_t val = mtf[idx];
    v[i] = val;
    for (int k = idx; k > 0; k--) mtf[k] = mtf[k - 1];
    mtf[0] = val;
  }
}

static inline void DecodeContextMap(BitReader& br, std::vector<uint8_t>* map, size_t* num_clusters) {
  if (br.Read(1)) {  // simple
    int bits = int(br.Read(2));
    for (auto& e : *map) e = bits ? uint8_t(br.Read(bits)) : 0;
  } else {
    bool use_mtf = br.Read(1) != 0;
    EntropyCode code;
    DecodeHistograms(br, 1, &code, /*disallow_lz77=*/map->size() <= 2);
    SymbolReader rd(&code, &br);
    uint32_t maxsym = 0;
    for (size_t i = 0; i < map->size(); i++) {
      uint32_t s = rd.Read(0);
      maxsym = std::max(maxsym, s);
      (*map)[i] = uint8_t(s);
    }
    JXLO_CHECK(maxsym < 256, "context map: invalid cluster id");
    JXLO_CHECK(rd.FinalStateOk(), "context map: bad ANS final state");
    if (use_mtf) InverseMtf(map->data(), map->size());
  }
  *num_clusters = size_t(*std::max_element(map->begin(), map->end())) + 1;
  std::vector<bool> seen(*num_clusters, false);
  for (uint8_t c : *map) seen[c] = true;
  for (bool s : seen) JXLO_CHECK(s, "context map: unused cluster id");
}

static inline void DecodeHistograms(BitReader& br, size_t num_contexts, EntropyCode* code, bool disallow_lz77) {
  // LZ77Params bundle
  code->lz77 = br.Read(1) != 0;
  if (code->lz77) {
    code->lz_min_symbol = ReadU32(br, Val(224), Val(512), Val(4096), BitsOffset(15, 8));
    code->lz_min_length = ReadU32(br, Val(3), Val(4), BitsOffset(2, 5), BitsOffset(8, 9));
    num_contexts++;
    ReadHybridCfg(br, 8, &code->lz_len_cfg);
  }
  JXLO_CHECK(!(code->lz77 && disallow_lz77), "lz77 not allowed here");
  code->ctx_map.assign(num_contexts, 0);
  code->num_clusters = 1;
  if (num_contexts > 1) DecodeContextMap(br, &code->ctx_map, &code->num_clusters);
  code->lz_dist_ctx = code->ctx_map.back();
  code->use_prefix = br.Read(1) != 0;
  code->log_alpha = code->use_prefix ? 15 : int(br.Read(2)) + 5;
  code->cfg.resize(code->num_clusters);
  for (auto& c : code->cfg) ReadHybridCfg(br, code->log_alpha, &c);
  const size_t max_alpha = size_t(1) << code->log_alpha;
  code->degenerate.assign(code->num_clusters, -1);
  code->parsed.assign(code->num_clusters, std::vector<int32_t>());
  if (code->use_prefix) {
    code->prefix.resize(code->num_clusters);
    std::vector<uint32_t> sizes(code->num_clusters);
    for (auto& s : sizes) {
      s = VarLenU16(br) + 1;
      JXLO_CHECK(s <= max_alpha, "prefix alphabet too large");
    }
    for (size_t c = 0; c < code->num_clusters; c++) {
      if (sizes[c] > 1) {
        std::vector<uint8_t> lens;
        ReadPrefixCode(br, sizes[c], &code->prefix[c], &lens);
        code->parsed[c].assign(lens.begin(), lens.end());
      } else {
        code->parsed[c].assign(1, 1);
        code->prefix[c].max_len = 0;
        code->prefix[c].sym.assign(1, 0);
        code->prefix[c].len.assign(1, 0);
      }
      const PrefixCode& pc = code->prefix[c];
      for (size_t k = 0; k < pc.sym.size(); k++) UpdateMaxBits(code, c, pc.sym[k]);
    }
  } else {
    code->alias.resize(code->num_clusters << code->log_alpha);
    for (size_t c = 0; c < code->num_clusters; c++) {
      std::vector<int32_t> counts;
      ReadHistogram(br, &counts);
      JXLO_CHECK(counts.size() <= max_alpha, "ANS alphabet too large");
      while (!counts.empty() && counts.back() == 0) counts.pop_back();
      code->parsed[c] = counts;
      for (size_t s = 0; s < counts.size(); s++)
        if (counts[s]) UpdateMaxBits(code, c, s);
      int deg = counts.empty() ? 0 : int(counts.size()) - 1;
      for (int s = 0; s < deg; s++)
        if (counts[s]) {
          deg = -1;
          break;
        }
      code->degenerate[c] = deg;
      InitAliasTable(counts, code->log_alpha, &code->alias[c << code->log_alpha]);
    }
  }
}

}  // namespace jxlo
#endif  // JXLO_ENTROPY_H_
