// One Modular sub-bitstream through a front-end's ModularDecode, for tests/test_modular_np.py: the bytes come from the
// writer of tests/modular_np.py, the channels this program prints are compared with that reading's. Built twice like
// host_kats.cc: over the product's front-end (libjxl_amd/csrc/host) and, with -DKAT_ORACLE, over the oracle's; built with
// AddressSanitizer + UBSan and run as a program of its own.
//
// usage: modular_model_kats CASE            decodes twice, undo_transforms false then true, and prints both channel lists
//        modular_model_kats CASE flip B...  for every bit B: the bytes with that bit flipped, decoded with undo_transforms
//                                           true; prints "B ok" or "B error <what>" (an error is an answer, a crash is not)
// CASE is a text file: "num_channels nb_meta stream_id bit_depth num_bytes", a line "w h hshift vshift" per channel, then
// the bytes in hex on one line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#ifdef KAT_ORACLE
#include "../../oracle/jxlo_bits.h"
#include "../../oracle/jxlo_entropy.h"
#include "../../oracle/jxlo_modular.h"
namespace H = jxlo;
#else
#include "../../libjxl_amd/csrc/host/jxh_bits.h"
#include "../../libjxl_amd/csrc/host/jxh_entropy.h"
#include "../../libjxl_amd/csrc/host/jxh_modular.h"
namespace H = jxh;
#endif

struct Case {
  std::vector<H::MChannel> ch;
  size_t nb_meta = 0;
  int stream_id = 0, bit_depth = 8;
  std::vector<uint8_t> bytes;
};

static bool ReadCase(const char* path, Case* c) {
  FILE* f = fopen(path, "r");
  if (!f) return false;
  size_t nch = 0, nbytes = 0;
  bool ok = fscanf(f, "%zu %zu %d %d %zu", &nch, &c->nb_meta, &c->stream_id, &c->bit_depth, &nbytes) == 5 && nch <= 64 && nbytes <= (1u << 24);
  for (size_t i = 0; ok && i < nch; i++) {
    size_t w, h;
    int hs, vs;
    ok = fscanf(f, "%zu %zu %d %d", &w, &h, &hs, &vs) == 4 && w <= 4096 && h <= 4096;
    if (ok) c->ch.push_back(H::MChannel(w, h, hs, vs));
  }
  c->bytes.resize(ok ? nbytes : 0);
  for (size_t i = 0; ok && i < nbytes; i++) {
    unsigned v;
    ok = fscanf(f, "%2x", &v) == 1;
    c->bytes[i] = uint8_t(v);
  }
  fclose(f);
  return ok;
}

static void Decode(const Case& c, const std::vector<uint8_t>& bytes, bool undo, H::MImage* img) {
  img->ch = c.ch;
  img->nb_meta = c.nb_meta;
  img->bitdepth = c.bit_depth;
  H::BitReader br(bytes.data(), bytes.size());
  H::ModularDecode(br, img, c.stream_id, nullptr, size_t(1) << 30, undo);
  printf("end_bit %zu\n", br.BitPos());
}

static void Print(const char* name, const H::MImage& img) {
  printf("%s %zu %zu\n", name, img.ch.size(), img.nb_meta);
  for (const H::MChannel& ch : img.ch) {
    printf("%zu %zu %d %d", ch.w, ch.h, ch.hshift, ch.vshift);
    for (int32_t v : ch.d) printf(" %d", v);
    printf("\n");
  }
}

int main(int argc, char** argv) {
  Case c;
  if (argc < 2 || !ReadCase(argv[1], &c)) {
    fprintf(stderr, "usage: %s CASE [flip BIT...]\n", argv[0]);
    return 2;
  }
  if (argc >= 3 && !strcmp(argv[2], "flip")) {
    for (int i = 3; i < argc; i++) {
      const size_t bit = size_t(atol(argv[i]));
      if (bit >= c.bytes.size() * 8) return 2;
      std::vector<uint8_t> bytes = c.bytes;
      bytes[bit >> 3] ^= uint8_t(1u << (bit & 7));
      try {
        H::MImage img;
        Decode(c, bytes, true, &img);
        printf("%zu ok\n", bit);
      } catch (const std::exception& e) {
        printf("%zu error %s\n", bit, e.what());
      }
    }
    return 0;
  }
  try {
    H::MImage pre, fin;
    Decode(c, c.bytes, false, &pre);
    Print("pre", pre);
    Decode(c, c.bytes, true, &fin);
    Print("final", fin);
  } catch (const std::exception& e) {
    printf("error %s\n", e.what());
    return 1;
  }
  return 0;
}
