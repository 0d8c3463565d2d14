// The launch plan of jxlhip_modular_run_batch (libjxl_amd/csrc/host/jxh_modular_launch_plan.h), held on the CPU. Built by
// tests/test_modular_launch_plan.py with -fsanitize=address,undefined around libjxl_amd/csrc/api/jxl_api.cc like
// modular_upload_kats.cc: the HIP entry points are no-device doubles, except jxlhip_modular_upload, whose double here keeps
// what the context would keep of the descriptor (the stream descriptors against fake bases, the sample counts, the codes'
// table words).
// The program holds the loops as the HIP layer had them before the header (Old*: the stream order, the caps, the form,
// the lanes, LDS and grid of jxlhip_modular_run_batch; the pass geometry of ModAppendPass; the grids of ModularLaunchOps,
// recording each launch) and compares field for field.
//   kats              synthetic descriptors: stream counts around every change of the lanes, every override, equal sample
//                     counts across frames, trees and tables around the LDS limits, WP / REFS set by one stream; the
//                     expansion at the grid limits, where the grids must cover every block once and exceed no limit
//   real FILE...      the plan of each stream's frame alone and of all as one set, under no override, 4 and 64
//   plan [--lanes N] FILE...   prints the plan of the set as the words of the HIP layer's "[modular pack]" line
// FILE: a path, or path:second for the frame behind the first, whose patches read the first.
#include "../../libjxl_amd/csrc/api/jxl_api.cc"
#define KATS_OWN_MODULAR_UPLOAD
#include "no_device_doubles.inc"
#include "../../libjxl_amd/csrc/host/jxh_modular_launch_plan.h"

namespace up = jxlhip::upload;
namespace ml = jxh::modular_launch;
using jxlhip::ModStream;

#define EXPECT(cond, ...)                                             \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                                   \
      fprintf(stderr, "\n");                                          \
      return 1;                                                       \
    }                                                                 \
  } while (0)

// What a context keeps of a frame for the batch (JxlHipContext::Modular).
struct Frame {
  std::vector<ModStream> streams_host;
  std::vector<uint32_t> stream_samples, code_table_words;
};
static std::vector<ml::ModStreamFrame> Views(const std::vector<Frame>& frames) {
  std::vector<ml::ModStreamFrame> v(frames.size());
  for (size_t i = 0; i < frames.size(); i++)
    v[i] = {frames[i].streams_host.data(), frames[i].stream_samples.data(), frames[i].streams_host.size(), frames[i].code_table_words.data(),
            frames[i].code_table_words.size()};
  return v;
}

// ------------------------------------------------------------------------- the HIP layer's loops before the header
struct OldPlan {
  std::vector<ModStream> flat;
  uint32_t batch_n = 0, batch_tree_cap = 0, batch_table_cap = 0;
  bool batch_wp = true, batch_refs = true;
  uint32_t lanes = 0, lds = 0, grid = 0;  // (of the launch; none without a stream)
};
static OldPlan OldStreams(const std::vector<Frame>& ctxs, int forced) {
  OldPlan M0;
  const size_t n = ctxs.size();
  struct Ref {
    uint32_t samples;
    const ModStream* s;
  };
  std::vector<Ref> all;
  for (size_t i = 0; i < n; i++)
    for (size_t j = 0; j < ctxs[i].streams_host.size(); j++) all.push_back({ctxs[i].stream_samples[j], &ctxs[i].streams_host[j]});
  std::stable_sort(all.begin(), all.end(), [](const Ref& a, const Ref& b) { return a.samples > b.samples; });
  std::vector<ModStream> flat(all.size() ? all.size() : 1);
  for (size_t i = 0; i < all.size(); i++) flat[i] = *all[i].s;
  M0.flat = flat;
  M0.batch_n = uint32_t(all.size());
  uint32_t cap = 0;
  for (const Ref& q : all)
    if (q.s->tree_nodes <= 2048 && q.s->tree_nodes > cap) cap = q.s->tree_nodes;
  M0.batch_tree_cap = cap;
  M0.batch_wp = M0.batch_refs = false;
  for (const Ref& q : all) {
    M0.batch_wp = M0.batch_wp || q.s->uses_wp != 0;
    M0.batch_refs = M0.batch_refs || q.s->num_props > 16;
  }
  uint32_t tcap = 0;
  for (size_t i = 0; i < n; i++)
    for (uint32_t w : ctxs[i].code_table_words)
      if (w <= 8192 && w > tcap) tcap = w;
  M0.batch_table_cap = tcap;
  if (M0.batch_n) {
    uint32_t lanes = 1;
    while (lanes < 64 && M0.batch_n / lanes > 4096) lanes *= 2;
    if (forced == 1 || forced == 2 || forced == 4 || forced == 8 || forced == 16 || forced == 32 || forced == 64) lanes = uint32_t(forced);
    M0.lanes = lanes;
    M0.lds = 32 * lanes * 4 + M0.batch_tree_cap * 16 + M0.batch_table_cap * 4 + 64 * 4;
    M0.grid = (M0.batch_n + lanes - 1) / lanes;
  }
  return M0;
}
struct OldGrid {
  uint32_t kind;
  size_t offset;
  uint32_t z, gx, gy, gz, block;
};
static std::vector<OldGrid> OldLaunchOps(const std::vector<up::ModLaunch>& launches) {
  std::vector<OldGrid> out;
  for (const up::ModLaunch& L : launches)
    for (uint32_t z = 0; z < L.count; z += 65535) {
      const uint32_t zn = std::min<uint32_t>(L.count - z, 65535);
      const uint32_t gy = std::min<uint32_t>(L.gy, 4096);
      if (L.kind == 0) out.push_back({0, L.offset, z, L.gx, gy, zn, 256});
      else if (L.kind == 1) out.push_back({1, L.offset, z, L.gx, gy, zn, 256});
      else if (L.kind == 2) out.push_back({2, L.offset, z, L.gx, zn, 1, 64});
      else if (L.kind == 5) out.push_back({5, L.offset, z, L.gy, zn, 1, 256});
      else if (L.kind == 6) out.push_back({6, L.offset, z, L.gy, zn, 1, 256});
      else out.push_back({L.kind, L.offset, z, L.gx, gy, zn, 256});
    }
  return out;
}
struct Size {
  uint32_t xs, ys;
};
static up::ModLaunch OldPass(uint32_t kind, bool rows, const std::vector<Size>& frames) {
  up::ModLaunch L{kind, 0, 0, 0, 0};
  for (size_t i = 0; i < frames.size(); i++) {
    L.count++;
    L.gx = rows ? 1 : std::max(L.gx, (frames[i].xs + 255) / 256);
    L.gy = std::max(L.gy, frames[i].ys);
  }
  return L;
}

// ------------------------------------------------------------------------------------------------ the comparisons
static bool SameStream(const ModStream& a, const ModStream& b) {
  return a.words == b.words && a.bit_offset == b.bit_offset && a.size_bytes == b.size_bytes && a.tree == b.tree && a.tree_nodes == b.tree_nodes &&
         a.code == b.code && a.channels == b.channels && a.num_channels == b.num_channels && a.stream_id == b.stream_id &&
         a.first_channel_index == b.first_channel_index && memcmp(a.wp, b.wp, sizeof(a.wp)) == 0 && a.uses_wp == b.uses_wp && a.num_props == b.num_props &&
         a.dist_multiplier == b.dist_multiplier && a.wp_scratch == b.wp_scratch && a.lz_window == b.lz_window && a.lz_window_mask == b.lz_window_mask &&
         a.status == b.status && a.end_bit == b.end_bit;
}
// The header's plan of `frames` under `forced` against the loops above; `got`: the plan, for the caller's own checks.
static int ComparePlan(const std::vector<Frame>& frames, int forced, ml::ModBatchPlan* got = nullptr) {
  const OldPlan old = OldStreams(frames, forced);
  const std::vector<ml::ModStreamFrame> views = Views(frames);
  std::vector<ModStream> flat(3);  // (what it held is gone afterwards)
  const ml::ModBatchPlan p = ml::PlanModStreams(views.data(), views.size(), forced, &flat);
  EXPECT(flat.size() == old.flat.size(), "%zu descriptors, the loops give %zu", flat.size(), old.flat.size());
  for (size_t i = 0; i < flat.size(); i++) EXPECT(SameStream(flat[i], old.flat[i]), "descriptor %zu (override %d)", i, forced);
  EXPECT(p.n == old.batch_n && p.tree_cap == old.batch_tree_cap && p.table_cap == old.batch_table_cap && p.wp == old.batch_wp && p.refs == old.batch_refs,
         "n %u/%u tree_cap %u/%u table_cap %u/%u wp %d/%d refs %d/%d", p.n, old.batch_n, p.tree_cap, old.batch_tree_cap, p.table_cap, old.batch_table_cap,
         p.wp, old.batch_wp, p.refs, old.batch_refs);
  if (old.batch_n)
    EXPECT(p.lanes == old.lanes && p.lds == old.lds && p.workgroups == old.grid, "override %d, %u streams: lanes %u/%u lds %u/%u workgroups %u/%u", forced,
           p.n, p.lanes, old.lanes, p.lds, old.lds, p.workgroups, old.grid);
  else
    EXPECT(p.workgroups == 0, "%u workgroups without a stream", p.workgroups);
  // (the kernel's own bounds: a lane per stream of the wave, every stream in a wave)
  EXPECT(p.lanes >= 1 && p.lanes <= 64 && (p.lanes & (p.lanes - 1)) == 0 && uint64_t(p.workgroups) * p.lanes >= p.n, "lanes %u workgroups %u", p.lanes,
         p.workgroups);
  EXPECT(p.grids.empty(), "PlanModStreams made grids");
  if (got) *got = p;
  return 0;
}
static int CompareGrids(const std::vector<up::ModLaunch>& launches) {
  const std::vector<OldGrid> old = OldLaunchOps(launches);
  const std::vector<ml::ModGrid> g = ml::ExpandModLaunches(launches);
  EXPECT(g.size() == old.size(), "%zu grids, the loops launch %zu", g.size(), old.size());
  for (size_t i = 0; i < g.size(); i++)
    EXPECT(g[i].kind == old[i].kind && g[i].offset == old[i].offset && g[i].first == old[i].z && g[i].grid[0] == old[i].gx && g[i].grid[1] == old[i].gy &&
               g[i].grid[2] == old[i].gz && g[i].block == old[i].block,
           "grid %zu: kind %u first %u (%u, %u, %u) x %u", i, g[i].kind, g[i].first, g[i].grid[0], g[i].grid[1], g[i].grid[2], g[i].block);
  // every block of every launch once, in order; no grid beyond the limits of the device (x 2^31 - 1, y and z 65535) or
  // with an empty dimension; the blocks along z for the sample kernels, along y for the others
  size_t at = 0;
  for (const up::ModLaunch& L : launches) {
    uint32_t next = 0;
    while (next < L.count) {
      EXPECT(at < g.size(), "launch of %u blocks ends at %u", L.count, next);
      const ml::ModGrid& q = g[at++];
      EXPECT(q.kind == L.kind && q.offset == L.offset && q.first == next && q.count >= 1 && q.count <= L.count - next, "chunk at %u of %u", next, L.count);
      EXPECT(q.grid[0] >= 1 && q.grid[0] <= 0x7FFFFFFFu && q.grid[1] >= 1 && q.grid[1] <= 65535 && q.grid[2] >= 1 && q.grid[2] <= 65535, "(%u, %u, %u)",
             q.grid[0], q.grid[1], q.grid[2]);
      const bool rows = L.kind == 5 || L.kind == 6;
      if (L.kind == 2 || rows) {
        EXPECT(q.grid[1] == q.count && q.grid[2] == 1 && q.grid[0] == (rows ? L.gy : L.gx) && q.block == (rows ? 256u : 64u), "kind %u grid", L.kind);
      } else {  // (a row loop that strides by the grid covers any height from a grid of at least one row)
        EXPECT(q.grid[2] == q.count && q.grid[0] == L.gx && q.grid[1] == std::min<uint32_t>(L.gy, 4096) && q.block == 256, "kind %u grid", L.kind);
      }
      next += q.count;
    }
  }
  EXPECT(at == g.size(), "%zu grids beyond the launches", g.size() - at);
  return 0;
}

// -------------------------------------------------------------------------------------------------------- kats
static const int kOverrides[] = {0, 1, 2, 4, 8, 16, 32, 64, -1, 3, 5, 12, 63, 65, 128, 4096};
static ModStream Synth(uint32_t id, uint32_t tree_nodes = 7, uint32_t uses_wp = 0, uint32_t num_props = 16) {
  ModStream s;
  memset(&s, 0, sizeof(s));
  s.stream_id = id;
  s.tree_nodes = tree_nodes;
  s.uses_wp = uses_wp;
  s.num_props = num_props;
  s.bit_offset = id * 3 + 1;
  s.status = reinterpret_cast<uint32_t*>(uintptr_t(0x1000) + 4 * uintptr_t(id));
  return s;
}
static int Kats() {
  // ---- stream counts: 0, 1, the last count at one lane and the first at two, likewise at four, the first at 64; over
  // three frames of uneven size (one without a stream), sample counts from a handful of values so that equal ones meet
  // across frames; every legal override and several that are not taken
  for (uint32_t total : {0u, 1u, 4096u, 4097u, 8193u, 8194u, 131104u}) {
    std::vector<Frame> frames(3);
    const uint32_t share[3] = {total / 3, 0, total - total / 3};
    for (uint32_t f = 0; f < 3; f++)
      for (uint32_t j = 0; j < share[f]; j++) {
        frames[f].streams_host.push_back(Synth(f << 20 | j));
        frames[f].stream_samples.push_back((j * 7 + f * 3) % 5 * 1000);
      }
    frames[0].code_table_words = {10, 300};
    for (int forced : kOverrides) {
      ml::ModBatchPlan p;
      if (ComparePlan(frames, forced, &p)) return 1;
      const bool taken = forced == 1 || forced == 2 || forced == 4 || forced == 8 || forced == 16 || forced == 32 || forced == 64;
      const uint32_t own = total <= 4096 ? 1 : (total <= 8193 ? 2 : (total <= 16387 ? 4 : 64));
      EXPECT(p.lanes == (taken ? uint32_t(forced) : own), "%u streams, override %d: %u lanes", total, forced, p.lanes);
      EXPECT(p.lds == 32 * 4 * p.lanes + 7 * 16 * (total ? 1 : 0) + 300 * 4 + 256, "lds %u", p.lds);
    }
    // the order on its own: largest first, equal sizes in frame then stream order, every stream once
    const std::vector<ml::ModStreamFrame> views = Views(frames);
    std::vector<ModStream> flat;
    ml::PlanModStreams(views.data(), views.size(), 0, &flat);
    EXPECT(flat.size() == std::max(total, 1u), "%zu descriptors of %u streams", flat.size(), total);
    auto samples_of = [&](const ModStream& s) { return frames[s.stream_id >> 20].stream_samples[s.stream_id & 0xFFFFF]; };
    for (uint32_t i = 1; i < total; i++) {
      const uint32_t a = samples_of(flat[i - 1]), b = samples_of(flat[i]);
      EXPECT(a > b || (a == b && flat[i - 1].stream_id < flat[i].stream_id), "descriptor %u: %u samples (stream %x) behind %u (stream %x)", i, b,
             flat[i].stream_id, a, flat[i - 1].stream_id);
    }
    if (!total) {
      ModStream zero;
      memset(&zero, 0, sizeof(zero));
      EXPECT(SameStream(flat[0], zero), "the entry of an empty set is not zero");
    }
  }
  // ---- trees of 0, 1, 2048 and 2049 nodes, tables of 8192 and 8193 words, alone and mixed: the largest that fits
  {
    const struct {
      std::vector<uint32_t> trees, tables;
      uint32_t tree_cap, table_cap;
    } rows[] = {{{0}, {8192}, 0, 8192},          {{1}, {8193}, 1, 0},           {{2048}, {8192, 8193}, 2048, 8192}, {{2049}, {8193, 100}, 0, 100},
                {{2048, 2049}, {0}, 2048, 0},    {{2049, 1, 0}, {}, 1, 0},      {{2049, 2048, 1}, {8193, 8192, 1}, 2048, 8192},
                {{5, 2047, 4000}, {9000, 8191, 7}, 2047, 8191}};
    for (const auto& row : rows)
      for (int split = 0; split < 2; split++) {  // all in one frame; a frame per tree and per table
        std::vector<Frame> frames(split ? std::max(row.trees.size(), row.tables.size()) : 1);
        for (size_t k = 0; k < row.trees.size(); k++) {
          Frame& f = frames[split ? k : 0];
          f.streams_host.push_back(Synth(uint32_t(k), row.trees[k]));
          f.stream_samples.push_back(100);
        }
        for (size_t k = 0; k < row.tables.size(); k++) frames[split ? k : 0].code_table_words.push_back(row.tables[k]);
        ml::ModBatchPlan p;
        if (ComparePlan(frames, 0, &p)) return 1;
        EXPECT(p.tree_cap == row.tree_cap && p.table_cap == row.table_cap, "caps %u %u, want %u %u", p.tree_cap, p.table_cap, row.tree_cap, row.table_cap);
        EXPECT(p.lds == 128 + row.tree_cap * 16 + row.table_cap * 4 + 256 && p.lds <= 128 + 32768 + 32768 + 256, "lds %u", p.lds);
      }
  }
  // ---- the form: WP and REFS each set by one stream of the last frame only
  for (int wp = 0; wp < 2; wp++)
    for (int refs = 0; refs < 2; refs++) {
      std::vector<Frame> frames(3);
      for (uint32_t f = 0; f < 3; f++)
        for (uint32_t j = 0; j < 5; j++) {
          frames[f].streams_host.push_back(Synth(f << 20 | j));
          frames[f].stream_samples.push_back(50 + j);  // (the two below are neither first nor last of the sorted list)
        }
      if (wp) frames[2].streams_host[1].uses_wp = 1;
      if (refs) frames[2].streams_host[3].num_props = 20;
      ml::ModBatchPlan p;
      if (ComparePlan(frames, 0, &p)) return 1;
      EXPECT(p.wp == (wp != 0) && p.refs == (refs != 0), "form %s for wp %d refs %d", ml::FormName(p), wp, refs);
      const char* const names[4] = {"plain", "refs", "wp", "wp+refs"};
      EXPECT(std::string(ml::FormName(p)) == names[wp * 2 + refs], "form name %s", ml::FormName(p));
    }
  // ---- the pass geometry
  {
    const std::vector<std::vector<Size>> sets = {{{1, 1}}, {{256, 10}, {257, 4097}}, {{3840, 2160}, {40, 5000}, {300, 280}}, {{40, 5000}}, {{4096, 4096}, {255, 7}}};
    for (const auto& set : sets)
      for (int rows = 0; rows < 2; rows++) {
        const up::ModLaunch want = OldPass(rows ? 5 : 3, rows != 0, set);
        up::ModLaunch L{rows ? 5u : 3u, 0, 0, 0, 0};
        uint32_t widest = 0, tallest = 0;
        for (const Size& s : set) {
          ml::ModPassAdd(&L, rows != 0, s.xs, s.ys);
          widest = std::max(widest, (s.xs + 255) / 256);
          tallest = std::max(tallest, s.ys);
        }
        EXPECT(L.kind == want.kind && L.offset == want.offset && L.count == want.count && L.gx == want.gx && L.gy == want.gy, "pass of %zu frames", set.size());
        EXPECT(L.count == set.size() && L.gx == (rows ? 1 : widest) && L.gy == tallest, "pass grid %u x %u", L.gx, L.gy);
      }
  }
  // ---- the expansion: block counts of 65535, 65536 and 131071, heights of 4096 and 4097, a row pass 5000 high, an
  // unsqueeze launch, an empty list
  {
    if (CompareGrids({})) return 1;
    EXPECT(ml::ExpandModLaunches({}).empty(), "grids of no launch");
    std::vector<up::ModLaunch> all;
    size_t offset = 0;
    for (uint32_t kind : {0u, 1u, 3u, 4u})
      for (uint32_t count : {1u, 65535u, 65536u, 131071u})
        for (uint32_t gy : {1u, 4096u, 4097u}) {
          all.push_back({kind, offset, count, 3, gy});
          offset += size_t(count) * 96 + 16;
        }
    for (uint32_t kind : {5u, 6u})
      for (uint32_t count : {1u, 65536u}) {
        up::ModLaunch L{kind, offset, 0, 0, 0};
        for (uint32_t i = 0; i < count; i++) ml::ModPassAdd(&L, true, 40, i == 0 ? 5000 : 30);
        all.push_back(L);
        offset += size_t(count) * 128;
      }
    for (uint32_t count : {1u, 65535u, 65536u, 131071u}) {
      all.push_back({2, offset, count, 7, 1});
      offset += size_t(count) * 64;
    }
    for (const up::ModLaunch& L : all)
      if (CompareGrids({L})) return 1;
    if (CompareGrids(all)) return 1;
    const std::vector<ml::ModGrid> g = ml::ExpandModLaunches({{5, 0, 2, 1, 5000}, {3, 64, 131071, 3, 4097}, {2, 128, 65536, 7, 1}});
    EXPECT(g.size() == 1 + 3 + 2, "%zu grids", g.size());
    EXPECT(g[0].grid[0] == 5000 && g[0].grid[1] == 2 && g[0].grid[2] == 1, "the row pass is cut");
    EXPECT(g[1].grid[1] == 4096 && g[1].grid[2] == 65535 && g[2].first == 65535 && g[3].first == 131070 && g[3].count == 1 && g[3].grid[2] == 1, "sample chunks");
    EXPECT(g[4].grid[0] == 7 && g[4].grid[1] == 65535 && g[4].block == 64 && g[5].first == 65535 && g[5].grid[1] == 1, "unsqueeze chunks");
  }
  printf("modular launch plan kats passed\n");
  return 0;
}

// ------------------------------------------------------------------------------------------------- real streams
// The double: what AdoptModFrame and SendModTables keep for the batch, against bases of the frame's own.
struct Collected {
  std::vector<Frame>* frames;
  int result = -1;
};
extern "C" int jxlhip_modular_upload(JxlHipContext* ctx, const JxlHipModFrameDesc* d) {
  Collected* k = reinterpret_cast<Collected*>(ctx);
  const up::ModUploadOptions opt;
  if ((k->result = up::CheckModFrameDesc(*d, opt))) return k->result;
  const up::ModPlan P = up::MakeModPlan(*d, opt);
  const uint64_t frame = (uint64_t(k->frames->size()) + 1) << 44;  // 64 GiB per region, sixteen regions per frame
  up::ModBases b;
  b.pool = frame + (uint64_t(1) << 36);
  b.sections = frame + (uint64_t(2) << 36);
  b.blob = frame + (uint64_t(3) << 36);
  b.rects = frame + (uint64_t(4) << 36);
  b.scratch = frame + (uint64_t(5) << 36);
  b.windows = frame + (uint64_t(6) << 36);
  b.status = frame + (uint64_t(7) << 36);
  b.end_bits = frame + (uint64_t(8) << 36);
  Frame f;
  f.streams_host.resize(d->num_streams);
  up::BuildModStreams(*d, P, f.streams_host.data(), b);
  f.code_table_words = P.table_words;
  for (uint32_t i = 0; i < d->num_streams; i++) f.stream_samples.push_back(d->streams[i].num_samples);
  k->frames->push_back(f);
  return 0;
}
static int Collect(const char* arg, std::vector<Frame>* frames) {
  std::string path(arg);
  const bool second = path.size() > 7 && path.compare(path.size() - 7, 7, ":second") == 0;
  if (second) path.resize(path.size() - 7);
  FILE* f = fopen(path.c_str(), "rb");
  EXPECT(f, "%s does not open", path.c_str());
  std::vector<uint8_t> data;
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + n);
  fclose(f);
  JxlAmdModFrame* frame = nullptr;
  int r = jxlamd_modframe_parse(data.data(), data.size(), &frame);
  float plane[1];
  if (!r && second) {  // the first frame is what the second one's patches read: only its size matters here
    uint32_t info[16];
    jxlamd_modframe_info(frame, info);
    const size_t end = jxlamd_modframe_end(frame, nullptr);
    jxlamd_modframe_free(frame);
    frame = nullptr;
    r = jxlamd_modframe_parse_at(data.data(), data.size(), end, 1, &frame);
    const float* planes[4] = {plane, plane, plane, plane};
    const uint32_t xs[4] = {info[0], info[0], info[0], info[0]}, ys[4] = {info[1], info[1], info[1], info[1]};
    if (!r) r = jxlamd_modframe_set_patch_sources(frame, planes, xs, ys);
  }
  EXPECT(!r && frame, "%s does not parse (%s)", path.c_str(), jxlamd_last_error());
  Collected k;
  k.frames = frames;
  r = jxlamd_modframe_upload(frame, reinterpret_cast<JxlHipContext*>(&k));
  jxlamd_modframe_free(frame);
  EXPECT(!r && !k.result, "%s: upload %d, checks %d", path.c_str(), r, k.result);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode(argv[1]);
  if (mode == "kats") return Kats();
  int lanes = 0;
  std::vector<Frame> frames;
  for (int i = 2; i < argc; i++) {
    if (std::string(argv[i]) == "--lanes" && i + 1 < argc) lanes = atoi(argv[++i]);
    else if (Collect(argv[i], &frames)) return 1;
  }
  if (mode == "real") {
    size_t streams = 0;
    for (int forced : {0, 4, 64}) {
      for (const Frame& f : frames)
        if (ComparePlan({f}, forced)) return 1;
      ml::ModBatchPlan p;
      if (ComparePlan(frames, forced, &p)) return 1;
      streams = p.n;
    }
    printf("modular launch plan real passed: %zu frames, %zu streams\n", frames.size(), streams);
    return 0;
  }
  if (mode == "plan") {
    const std::vector<ml::ModStreamFrame> views = Views(frames);
    std::vector<ModStream> flat;
    const ml::ModBatchPlan p = ml::PlanModStreams(views.data(), views.size(), lanes, &flat);
    printf("modular pack streams %u lanes %u workgroups %u lds %u tree_cap %u table_cap %u form %s\n", p.n, p.lanes, p.workgroups, p.lds, p.tree_cap,
           p.table_cap, ml::FormName(p));
    return 0;
  }
  return 2;
}
