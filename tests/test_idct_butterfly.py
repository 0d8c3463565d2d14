"""The pruned 1-D inverse DCT butterfly of the transform kernels (FastIdctPruned<N, K>, jxl_idct_butterfly.h) against the full
one (FastIdct<N>) on the zero-padded input, on the CPU: the header is plain C++ templates a host compiler reads.

Both are built in one translation unit with the same flags and -ffp-contract=off, and every output element must compare
equal with `==`: the two forms may differ in the sign of an exact zero and in nothing else."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "libjxl_amd", "csrc", "hip")

DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
namespace jxlhip {
@WC_TABLES@
}  // namespace jxlhip
#include "jxl_idct_butterfly.h"

static uint32_t rng_state;
static uint32_t Next() {  // xorshift32
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}
// coefficient-like values of mixed magnitude, exact zeros and negative zeros among them
static float Value() {
  const uint32_t r = Next();
  const uint32_t kind = r & 15u;
  if (kind == 0) return 0.0f;
  if (kind == 1) return -0.0f;
  const float unit = float(int32_t(Next() >> 8) - (1 << 23)) / float(1 << 23);  // [-1, 1)
  const float scales[4] = {1e-4f, 0.03f, 1.0f, 37.0f};
  return unit * scales[(r >> 4) & 3u];
}

template <int N, int K>
static int Check(int trials) {
  int bad = 0;
  rng_state = 0x9E3779B9u ^ uint32_t(N * 131 + K);
  for (int trial = 0; trial < trials; trial++) {
    float full[N], pruned[N];
    for (int k = 0; k < N; k++) {
      const float x = Value();
      full[k] = k < K ? x : 0.0f;
      pruned[k] = k < K ? x : 1e30f;  // must not be read
    }
    if (trial == 0)
      for (int k = 0; k < K; k++) full[k] = pruned[k] = 0.0f;  // everything zero
    if (trial == 1)
      for (int k = 0; k < K; k++) full[k] = pruned[k] = -0.0f;
    jxlhip::FastIdct<N>(full);
    jxlhip::FastIdctPruned<N, K>(pruned);
    for (int n = 0; n < N; n++)
      if (!(full[n] == pruned[n])) {
        if (bad < 5) printf("N=%d K=%d trial %d out[%d]: full %.9g pruned %.9g\n", N, K, trial, n, full[n], pruned[n]);
        bad++;
      }
  }
  printf("N=%d K=%d: %d trials, %d differing outputs\n", N, K, trials, bad);
  return bad;
}

template <int N>
static int CheckN(int trials) {
  int bad = 0;
  if constexpr (1 < N) bad += Check<N, 1>(trials);
  if constexpr (2 < N) bad += Check<N, 2>(trials);
  if constexpr (4 < N) bad += Check<N, 4>(trials);
  if constexpr (8 < N) bad += Check<N, 8>(trials);
  return bad;
}

int main() {
  const int trials = 2000;
  int bad = CheckN<8>(trials) + CheckN<16>(trials) + CheckN<32>(trials) + CheckN<64>(trials);
  // (the sizes the kernels' recursion also reaches, and K = N, which is the full butterfly itself)
  bad += CheckN<2>(trials) + CheckN<4>(trials) + Check<8, 8>(trials) + Check<16, 3>(trials) + Check<32, 7>(trials);
  return bad ? 1 : 0;
}
"""


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_pruned_butterfly_equals_full_on_zero_padded_input(tmp_path, opt):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    # the multiplier tables as the kernels' header spells them: its WcTable<N> specialisations, each a complete declaration
    # (they stay in jxl_hip_kernels.h, where tests/test_kats.py holds their literals to the reference's)
    text = open(os.path.join(HEADER_DIR, "jxl_hip_kernels.h")).read()
    specs = re.findall(r"template <>\s*struct WcTable<\d+>\s*\{[^{}]*\{[^{}]*\};\s*\};", text)
    assert len(specs) == 6
    tables = "template <int N>\nstruct WcTable;\n" + "\n".join(specs)
    src = tmp_path / "butterfly_check.cc"
    src.write_text(DRIVER.replace("@WC_TABLES@", tables))
    exe = tmp_path / "butterfly_check"
    subprocess.run([cxx, "-std=c++17", opt, "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", HEADER_DIR, "-o", str(exe), str(src)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    # every (N, K) of the issue was run
    for n in (8, 16, 32, 64):
        for k in (1, 2, 4, 8):
            if k < n:
                assert "N=%d K=%d: 2000 trials, 0 differing outputs" % (n, k) in r.stdout
