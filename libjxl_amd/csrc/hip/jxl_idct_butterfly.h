// The 1-D inverse DCT of the fast transform kernels (k_idct_fast) as plain C++ templates: included by the HIP kernels and,
// for the CPU test of the pruned form, by a host compiler (tests/test_idct_butterfly.py).
//
// The algorithm is the recursive even / odd decomposition of lib/jxl/dct-inl.h:191-232 (IDCT1DImpl<N>): N/2-point IDCT of
// the even coefficients; N/2-point IDCT of the odd ones after d[j] = c[2j+1] + c[2j-1], d[0] = sqrt(2) c[1]; odd half scaled
// by WcMultipliers<N>[n] = 1 / (2 cos((n + 1/2) pi / N)), dct_scales.h:234-236; out[n], out[N-1-n] = even +- odd.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JXL_BFLY_FN __device__ __forceinline__
#else
#define JXL_BFLY_FN inline
#endif

namespace jxlhip {

// WcTable<N>::v[n] = WcMultipliers<N>[n], n < N / 2: the literals are in jxl_hip_kernels.h, which defines them before it
// includes this file (a host build supplies the same specialisations first).
template <int N>
struct WcTable;

template <int N>
JXL_BFLY_FN void FastIdct(float (&v)[N]) {
  if constexpr (N == 2) {
    const float a = v[0] + v[1], b = v[0] - v[1];
    v[0] = a;
    v[1] = b;
  } else if constexpr (N > 2) {
    float e[N / 2], o[N / 2];
#pragma unroll
    for (int j = 0; j < N / 2; j++) {
      e[j] = v[2 * j];
      o[j] = v[2 * j + 1];
    }
#pragma unroll
    for (int j = N / 2 - 1; j > 0; j--) o[j] += o[j - 1];
    o[0] *= 1.41421356237309504880f;
    FastIdct<N / 2>(e);
    FastIdct<N / 2>(o);
#pragma unroll
    for (int n = 0; n < N / 2; n++) {
      const float t = o[n] * WcTable<N>::v[n];
      v[n] = e[n] + t;
      v[N - 1 - n] = e[n] - t;
    }
  }
}

// The same butterfly for an input whose entries k >= K are zero, known at compile time: v[K..N) is not read, all N outputs
// are written. It is FastIdct<N>'s recursion with the operations on known zeros left out (x + 0, 0 * w, e +- 0) and every
// other operation in its place and form, so the result equals FastIdct<N> of the zero-padded input except, possibly, for
// the sign of an exact zero (x + 0 turns -0 into +0, the elided form keeps it).
//   * Even half: entries 2j < K, i.e. KE = ceil(K / 2) of them. Odd half: KO = floor(K / 2) entries, and after the running
//     sum o[j] += o[j-1] one more (o[KO] = 0 + o[KO-1]): KP of them.
//   * Device code is compiled with floating-point contraction, so a product whose only consumers are sums with a known
//     zero would, once those sums are elided, fuse into the NEXT sum instead and round differently from the full form. There
//     is one such product: sqrt(2) * o[0], which the recursion hands down as element 0 of the even halves to the 2-point
//     step, where it meets o[N/4]. Where that partner is a known zero the product is written as fma(o[0], sqrt(2), 0):
//     the rounded product, which no later sum can absorb.
//     How the device compiler contracts the two forms is not something this file can fix for good: the guard is
//     tests/test_gpu_sparse_transform.py::test_zero_ac_every_channel_from_its_corner, which runs every (CX, CY) of the kernel
//     through the pruned form in all three channels and asserts (it covers every fast strategy) planes equal to the full
//     form's under ==. A compiler that re-aims a contraction fails there.
template <int N, int K>
JXL_BFLY_FN void FastIdctPruned(float (&v)[N]) {
  static_assert(K >= 1 && K <= N, "at least the constant term, at most everything");
  if constexpr (K == N) {
    FastIdct<N>(v);
  } else if constexpr (N == 2) {  // K == 1: a = v[0] + 0, b = v[0] - 0
    v[1] = v[0];
  } else {
    constexpr int H = N / 2, KE = (K + 1) / 2, KO = K / 2, KP = KO == 0 ? 0 : (KO + 1 < H ? KO + 1 : H);
    float e[H];
#pragma unroll
    for (int j = 0; j < H; j++) e[j] = j < KE ? v[2 * j] : 0.0f;
    FastIdctPruned<H, KE>(e);
    if constexpr (KO == 0) {  // no odd half: t = 0 * w, v[n] = e[n] + 0, v[N-1-n] = e[n] - 0
#pragma unroll
      for (int n = 0; n < H; n++) {
        v[n] = e[n];
        v[N - 1 - n] = e[n];
      }
    } else {
      float o[H];
#pragma unroll
      for (int j = 0; j < H; j++) o[j] = j < KO ? v[2 * j + 1] : 0.0f;
#pragma unroll
      for (int j = KP - 1; j > 0; j--) {
        if (j < KO) o[j] += o[j - 1];
        else o[j] = o[j - 1];  // 0 + o[j-1]
      }
      if constexpr (H / 2 >= KP) o[0] = __builtin_fmaf(o[0], 1.41421356237309504880f, 0.0f);
      else o[0] *= 1.41421356237309504880f;
      FastIdctPruned<H, KP>(o);
#pragma unroll
      for (int n = 0; n < H; n++) {
        const float t = o[n] * WcTable<N>::v[n];
        v[n] = e[n] + t;
        v[N - 1 - n] = e[n] - t;
      }
    }
  }
}

}  // namespace jxlhip
