// Forward VarDCT path on the device (first slice): sRGB8 -> XYB, inverse-Gaborish sharpening, block
// activity, transform selection + quant field, forward DCT + DC extraction + quantisation with chroma-from-luma.
// What the reference does in enc_xyb.cc:83-174 (SRGBToXYB), enc_gaborish.cc:21-70, enc_group.cc:380-533
// (ComputeCoefficients: TransformFromPixels, DCFromLowestFrequencies, QuantizeBlockAC / QuantizeRoundtripYBlockAC) and
// enc_transforms-inl.h. By default the transform selection is the one of this repo's CPU stream writer (csrc/enc), not the
// reference's AC-strategy search (enc_ac_strategy.cc:827-1068; opt-in, below), and there is no Butteraugli loop
// (enc_adaptive_quantization.cc:707-1115). The quant field is the writer's own activity rule by default;
// with quant_field_mode 1 it is the reference's initial adaptive quant field (enc_adaptive_quantization.cc:88-449,
// 466-628, 1198-1247: k_enc_aq_cells, k_enc_aq_blocks and the tail of k_enc_select<true>). With strategy_mode 2 / 3 (and
// that quant field) the transforms are chosen by the reference's search restricted to the pure-DCT kinds instead: the
// per-pixel masking (k_enc_mask1x1), the cost estimate of every candidate (k_enc_estimate: EstimateEntropy,
// enc_ac_strategy.cc:364-511) and the merge walk (k_enc_acs_walk: ProcessRectACS :827-1059), each also a stand-alone entry;
// k_enc_activity and k_enc_select are then not launched. Every float expression keeps the
// operation order of the CPU writer with contraction off, so that the two agree except where cbrtf / log2f / exp2f differ
// in the last place.
#ifndef JXL_HIP_ENC_H_
#define JXL_HIP_ENC_H_

namespace jxlhip {

struct EncFwd {
  const uint8_t* rgb;     // interleaved RGB8, `rgb_stride` bytes per row
  const float* srgb_lut;  // 256 floats: sRGB byte -> linear
  float* planes;          // [3][yp][xp] XYB (X, Y, B), padded to whole blocks by edge replication
  float* planes_in;       // ping-pong partners of the sharpening iterations
  float* planes_orig;
  float* act;             // [yb][xb] mean absolute deviation of Y
  uint8_t* acs;           // [yb][xb] (strategy << 1) | first
  int32_t* qf;            // [yb][xb] quant field at first blocks
  uint32_t* coef_off;     // [yb][xb] coefficient offset of a first block inside its group
  const float* basis_t;   // [n][k] DCT matrices of 1..256 points (level l at (4^l - 1) / 3)
  const float* dequant;
  uint32_t dq_offset[17], dq_size[17];
  int32_t* dc;      // [3][yb][xb] quantised DC, stored X, Y, B
  int32_t* coeffs;  // [group][3][65536]
  uint32_t xs, ys, xb, yb, xp, yp, xg, yg;
  size_t rgb_stride;
  float distance, quant_ac, inv_gs, x_dm, b_dm;
  float dc_step[3];
  uint32_t strategy_mode;
  // chroma-from-luma fit per 64x64 tile (enc_chroma_from_luma.cc:128-151, 204-352): factors out, one int8 per tile
  uint32_t cfl_fit;
  float scale;  // Quantizer::Scale() = global_scale / 65536
  int8_t* ytox;
  int8_t* ytob;
  // quant_field_mode 1 (k_enc_select<true>): the adaptive quant field per block before aggregation (k_enc_aq_blocks, from
  // an EncAq over the planes before the sharpening) and the max / mean mix of AdjustQuantField
  uint32_t quant_field_mode;
  const float* aq_map;  // [yb][xb]
  float mean_max_mixer;
};

// enc_xyb.cc:50-104: opsin absorbance matrix + bias, cube root, X = (L - M) / 2, Y = (L + M) / 2, B = S.
__global__ void k_enc_xyb(EncFwd P) {
#pragma clang fp contract(off)
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= P.xp) return;
  const uint32_t sx = min(x, P.xs - 1), sy = min(y, P.ys - 1);
  const uint8_t* p = P.rgb + size_t(sy) * P.rgb_stride + size_t(sx) * 3;
  const float r = P.srgb_lut[p[0]], g = P.srgb_lut[p[1]], b = P.srgb_lut[p[2]];
  const float bias = 0.0037930732552754493f, cb = cbrtf(bias);
  const float mr = 0.30f * r + (1.0f - 0.078f - 0.30f) * g + 0.078f * b + bias;
  const float mg = 0.23f * r + (1.0f - 0.078f - 0.23f) * g + 0.078f * b + bias;
  const float mb = 0.24342268924547819f * r + 0.20476744424496821f * g + (1.0f - 0.24342268924547819f - 0.20476744424496821f) * b + bias;
  const float gr = cbrtf(mr) - cb, gg = cbrtf(mg) - cb, gb = cbrtf(mb) - cb;
  const size_t plane = size_t(P.xp) * P.yp, i = size_t(y) * P.xp + x;
  P.planes[i] = 0.5f * (gr - gg);
  P.planes[plane + i] = 0.5f * (gr + gg);
  P.planes[2 * plane + i] = gb;
}

// One round of y <- y + (x - K * y), K the decoder's 3x3 Gaborish with the default weights (the encoder-side sharpening
// enc_gaborish.cc:21-70 obtains with one tuned 5x5 kernel).
__global__ void k_enc_sharpen(const float* __restrict__ orig, const float* __restrict__ in, float* __restrict__ out, uint32_t xp, uint32_t yp) {
#pragma clang fp contract(off)
  const uint32_t xx = blockIdx.x * blockDim.x + threadIdx.x, yy = blockIdx.y, c = blockIdx.z;
  if (xx >= xp) return;
  const size_t plane = size_t(xp) * yp * c;
  const float* y = in + plane;
  const uint32_t y0 = yy ? yy - 1 : 0, y1 = yy + 1 < yp ? yy + 1 : yp - 1, x0 = xx ? xx - 1 : 0, x1 = xx + 1 < xp ? xx + 1 : xp - 1;
  const float w1 = 1.1f * 0.104699568f, w2 = 1.1f * 0.055680538f, nrm = 1.0f / (1.0f + 4 * (w1 + w2));
  const float side = y[size_t(yy) * xp + x0] + y[size_t(yy) * xp + x1] + y[size_t(y0) * xp + xx] + y[size_t(y1) * xp + xx];
  const float corner = y[size_t(y0) * xp + x0] + y[size_t(y0) * xp + x1] + y[size_t(y1) * xp + x0] + y[size_t(y1) * xp + x1];
  const float centre = y[size_t(yy) * xp + xx];
  const float blur = (centre + w1 * side + w2 * corner) * nrm;
  out[plane + size_t(yy) * xp + xx] = centre + (orig[plane + size_t(yy) * xp + xx] - blur);
}

// The four rounds without LDS: a wave owns 64 adjacent columns (the middle 56 are written, four of halo either side) and
// walks down a strip of rows. Round k of row r needs rows r - 1 .. r + 1 of round k - 1, so when source row s arrives
// round 1 forms row s - 1, round 2 row s - 2, round 3 row s - 3 and round 4, the output, row s - 4: per round a window of
// three rows x (left, centre, right) lives in registers, the horizontal neighbours come from the adjacent lanes
// (wave_shr / wave_shl). Rows and columns outside the image are replaced as k_enc_sharpen does it (the neighbour index is
// clamped in image coordinates: the sample itself at an image edge); every sample sees the same operands in the same
// order as there. Lanes / rows of the halo that lack a neighbour hold garbage that never reaches a written sample.
constexpr int kSharpenCols = 56, kSharpenRows = 64;
__device__ __forceinline__ float EncFromLeft(float v) {  // the value of the lane of column x - 1
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xF, 0xF, true));
}
__device__ __forceinline__ float EncFromRight(float v) {  // ... of column x + 1
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xF, 0xF, true));
}
struct SharpenRow {  // one row of each level j (0 = the source, j = after round j): left / centre / right neighbours
  float L[4], C[4], R[4];
};
// One step: source row s enters; `c` (the oldest row's storage) receives the entering row of every level, `a` and `b` hold
// rows r - 1 and r of the level. The three row sets take the roles in turn, so nothing is copied from step to step.
// EDGE = false: no sample of the step lies on an image edge (no clamped neighbour to substitute).
template <bool EDGE>
__device__ __forceinline__ void SharpenStep(SharpenRow& a, SharpenRow& b, SharpenRow& c, float v0, const float (&osrc)[4], int s, int last,
                                            bool left_edge, bool right_edge, bool writes, int Y0, int Y1, float* dst, uint32_t xp) {
#pragma clang fp contract(off)
  const float w1 = 1.1f * 0.104699568f, w2 = 1.1f * 0.055680538f, nrm = 1.0f / (1.0f + 4 * (w1 + w2));
  float nC = v0;  // the new row of level j as it enters level j's window
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const float nL = EncFromLeft(nC), nR = EncFromRight(nC);
    c.L[j] = (EDGE && left_edge) ? nC : nL;
    c.C[j] = nC;
    c.R[j] = (EDGE && right_edge) ? nC : nR;
    // round j + 1 forms row r = s - j - 1
    const int r = s - j - 1;
    if (EDGE && r == 0) {  // no row above: the row itself
      a.L[j] = b.L[j]; a.C[j] = b.C[j]; a.R[j] = b.R[j];
    }
    if (EDGE && r == last) {  // no row below
      c.L[j] = b.L[j]; c.C[j] = b.C[j]; c.R[j] = b.R[j];
    }
    const float side = b.L[j] + b.R[j] + a.C[j] + c.C[j];
    const float corner = a.L[j] + a.R[j] + c.L[j] + c.R[j];
    const float centre = b.C[j];
    const float blur = (centre + w1 * side + w2 * corner) * nrm;
    nC = centre + (osrc[j] - blur);  // row r of level j + 1
    if (j == 3 && writes && r >= Y0 && r < Y1) dst[size_t(r) * xp] = nC;
  }
}
__global__ __launch_bounds__(256) void k_enc_sharpen_rows(const float* __restrict__ orig, float* __restrict__ out, uint32_t xp, uint32_t yp) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int strip_x0 = (int(blockIdx.x) * 4 + wave) * kSharpenCols - 4, gx = strip_x0 + lane;
  const int Y0 = int(blockIdx.y) * kSharpenRows, Y1 = min(Y0 + kSharpenRows, int(yp));
  if (strip_x0 + 4 >= int(xp)) return;  // (a wave beyond the last column strip)
  const size_t plane = size_t(xp) * yp * blockIdx.z;
  const bool in_x = gx >= 0 && gx < int(xp), left_edge = gx == 0, right_edge = gx == int(xp) - 1;
  const bool x_edge = strip_x0 <= 0 || strip_x0 + 63 >= int(xp) - 1;  // (wave-uniform: the strip holds an image edge column)
  const bool writes = lane >= 4 && lane < 4 + kSharpenCols && in_x;
  const float* src = orig + plane + (in_x ? gx : 0);
  float* dst = out + plane + (in_x ? gx : 0);
  SharpenRow P, Q, R;
#pragma unroll
  for (int j = 0; j < 4; j++)
    P.L[j] = P.C[j] = P.R[j] = Q.L[j] = Q.C[j] = Q.R[j] = R.L[j] = R.C[j] = R.R[j] = 0.0f;
  float osrc[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // the source's centre values of rows s - 1 .. s - 4
  const int s_begin = max(Y0 - 4, 0), s_end = Y1 - 1 + 4, last = int(yp) - 1;
  float next = in_x ? src[size_t(s_begin) * xp] : 0.0f;
  // (the row sets rotate through the roles in a fixed order of three steps; up to two steps beyond s_end write nothing)
  auto step = [&](SharpenRow& a, SharpenRow& b, SharpenRow& c, int s) {
    const float v0 = next;  // source row s (stale beyond the image: replaced by the edge rule before anything reads it)
    if (s + 1 <= last) next = in_x ? src[size_t(s + 1) * xp] : 0.0f;
    // rounds 1..4 form rows s - 1 .. s - 4: one of them is the image's first or last row
    if (x_edge || s <= 4 || s > last) SharpenStep<true>(a, b, c, v0, osrc, s, last, left_edge, right_edge, writes, Y0, Y1, dst, xp);
    else SharpenStep<false>(a, b, c, v0, osrc, s, last, left_edge, right_edge, writes, Y0, Y1, dst, xp);
    osrc[3] = osrc[2]; osrc[2] = osrc[1]; osrc[1] = osrc[0]; osrc[0] = v0;
  };
  for (int s = s_begin; s <= s_end; s += 3) {
    step(Q, R, P, s);
    step(R, P, Q, s + 1);
    step(P, Q, R, s + 2);
  }
}

// Mean absolute deviation of Y from the block mean, per 8x8 block: a wave per 8 blocks (lane = block * 8 + row).
__global__ void k_enc_activity(EncFwd P) {
#pragma clang fp contract(off)
  const uint32_t lane = threadIdx.x, row = lane & 7;
  const uint32_t bx = blockIdx.x * 8 + (lane >> 3), by = blockIdx.y;
  const bool live = bx < P.xb;
  const float* s = P.planes + size_t(P.xp) * P.yp + size_t(by * 8 + row) * P.xp + size_t(live ? bx : 0) * 8;
  float v[8];
  for (int x = 0; x < 8; x++) v[x] = s[x];
  // the CPU writer sums the 64 samples in raster order: row sums cannot be combined without changing the rounding, so
  // lane (block, 0) walks the rows of its block through cross-lane reads
  float mean = 0.0f;
  for (int y = 0; y < 8; y++)
    for (int x = 0; x < 8; x++) mean += __shfl(v[x], (lane & ~7u) + y, 64);
  mean /= 64;
  float a = 0.0f;
  for (int y = 0; y < 8; y++)
    for (int x = 0; x < 8; x++) a += fabsf(__shfl(v[x], (lane & ~7u) + y, 64) - mean);
  if (live && row == 0) P.act[size_t(by) * P.xb + bx] = a / 64;
}

// ---------------------------------------------------------------- adaptive quant field (quant_field_mode 1)
// The reference's initial quant field (lib/jxl/enc_adaptive_quantization.cc: ComputeTile :528-628, FuzzyErosion :389-449,
// PerBlockModulations :315-348 with ComputeMask :95-117, GammaModulation :179-211, HfModulation :260-313, BlueModulation
// :221-256) over the XYB planes before the sharpening, as csrc/enc/jxl_enc.cc InitialQuantField states it in float32:
//   k_enc_aq_cells   per 4x4 pixels: the masked, gamma-weighted Laplacian of Y, summed down the four rows of each column
//                    (row 0 first) and averaged over the four columns (c0 + c1 + c2 + c3, left to right, times 0.25)
//   k_enc_aq_blocks  per 8x8 block: the four smallest of each cell's 3x3 neighbourhood weighted and summed over the
//                    block's 2x2 cells (raster order), the masking output 1 / (e + 0.001), and the modulations
// Sums over the 64 samples of a block: per row left to right (where a sample adds two terms, in the order written), then
// the eight row sums as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)). log2f / exp2f are the exact functions where the
// reference has rational approximations (base/fast_math-inl.h). One global cell image: the reference's 64x64 tiles carry
// a border cell of their neighbours, so its tiling leaves no seam either.
struct EncAq {
  const float* planes;  // [3][yp][xp] X, Y, B; a neighbour outside the plane is the nearest sample of the plane
  float* cells;         // [yp / 4][xp / 4]
  float* aq;            // [yb][xb] the field, before the aggregation over transforms
  float* mask;          // [yb][xb] masking for the AC-strategy search (ComputeMaskForAcStrategyUse)
  uint32_t xp, yp, xb, yb;
  float w[4];           // erosion weights of the four smallest, normalised (they depend on the distance below 2)
  float mul, add;       // scale * dampen, (1 - dampen) * 0.48 * scale
};

// RatioOfDerivativesOfCubicRootToSimpleGamma (:127-145): den / num, or num / den when INVERT
template <bool INVERT>
__device__ __forceinline__ float EncGammaRatio(float v) {
#pragma clang fp contract(off)
  const float kInvLog2e = 0.6931471805599453f, kSGmul = 226.77216153508914f, kSGmul2 = 1.0f / 73.377132366608819f;
  const float kSGRetMul = kSGmul2 * 18.6580932135f * kInvLog2e, kSGVOffset = 7.7825991679894591f, kEpsilon = 1e-2f;
  const float kNumMul = kSGRetMul * 3 * kSGmul, kVOffset = kSGVOffset * kInvLog2e + kEpsilon, kDenMul = kInvLog2e * kSGmul;
  v = v < 0.0f ? 0.0f : v;
  const float v2 = v * v;
  const float num = kNumMul * v2 + kEpsilon, den = (kDenMul * v) * v2 + kVOffset;
  return INVERT ? num / den : den / num;
}

constexpr int kAqCols = 56, kAqRows = 32;
template <int CTRL>
__device__ __forceinline__ float EncDpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// A wave owns 64 adjacent columns (the middle 56 = 14 cells are written, four of halo either side so that cells start at a
// multiple of four lanes) and walks down a strip of rows, a cell row (four rows) per step, with the rows above and at in
// registers; the horizontal neighbours come from the adjacent lanes, the four column sums of a cell from the lanes of its quad.
__global__ __launch_bounds__(256) void k_enc_aq_cells(EncAq P) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int strip_x0 = (int(blockIdx.x) * 4 + wave) * kAqCols - 4, gx = strip_x0 + lane;
  if (strip_x0 + 4 >= int(P.xp)) return;  // (a wave beyond the last column strip)
  const int Y0 = int(blockIdx.y) * kAqRows, Y1 = min(Y0 + kAqRows, int(P.yp)), last = int(P.yp) - 1;
  const bool in_x = gx >= 0 && gx < int(P.xp), left_edge = gx == 0, right_edge = gx == int(P.xp) - 1;
  const bool writes = lane >= 4 && lane < 4 + kAqCols && in_x && (lane & 3) == 0;
  const float* src = P.planes + size_t(P.xp) * P.yp + (in_x ? gx : 0);
  float* dst = P.cells + (in_x ? gx >> 2 : 0);
  const float kSqrtMul = sqrtf(float(211.66567973503678f * 1e8)), kLogOffset = 27.505837037000106f;
  float up = src[size_t(max(Y0 - 1, 0)) * P.xp], cur = src[size_t(Y0) * P.xp];
  for (int y = Y0; y < Y1; y += 4) {  // (Y0 and Y1 are multiples of four: a cell row per step)
    // the four rows below in flight together: with one load per step the kernel waits out a memory latency per row
    float next[4];
#pragma unroll
    for (int k = 0; k < 4; k++) next[k] = src[size_t(min(y + 1 + k, last)) * P.xp];
    float col = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float down = next[k];
      const float l = EncFromLeft(cur), r = EncFromRight(cur);
      const float left = left_edge ? cur : l, right = right_edge ? cur : r;
      const float base = 0.25f * (down + up + left + right);
      float d = EncGammaRatio<false>(cur + 0.019f) * (cur - base);
      d *= d;
      d = d >= 0.2f ? 0.2f : d;
      const float p = 0.25f * sqrtf(d * kSqrtMul + kLogOffset);  // MaskingSqrt
      col = k ? col + p : p;
      up = cur;
      cur = down;
    }
    const float c0 = EncDpp<0x00>(col), c1 = EncDpp<0x55>(col), c2 = EncDpp<0xAA>(col), c3 = EncDpp<0xFF>(col);  // quad_perm broadcasts
    if (writes) dst[size_t(y >> 2) * (P.xp >> 2)] = (c0 + c1 + c2 + c3) * 0.25f;
  }
}

// A wave per 8 blocks (lane = block * 8 + row), each lane holding its row of X, Y and B; the row below comes from the next
// lane. Lanes 0..3 of a block erode its four cells, reading the 3x3 neighbourhoods from the cell image.
__global__ __launch_bounds__(64) void k_enc_aq_blocks(EncAq P) {
#pragma clang fp contract(off)
  const uint32_t lane = threadIdx.x, row = lane & 7, first = lane & ~7u;
  const uint32_t bx = blockIdx.x * 8 + (lane >> 3), by = blockIdx.y;
  const bool live = bx < P.xb;
  const uint32_t lbx = live ? bx : 0;
  const size_t plane = size_t(P.xp) * P.yp;
  const float* s = P.planes + size_t(by * 8 + row) * P.xp + size_t(lbx) * 8;
  float X[8], Y[8], B[8], N[8];
  {
    const float4 x0 = *reinterpret_cast<const float4*>(s), x1 = *reinterpret_cast<const float4*>(s + 4);
    const float4 y0 = *reinterpret_cast<const float4*>(s + plane), y1 = *reinterpret_cast<const float4*>(s + plane + 4);
    const float4 b0 = *reinterpret_cast<const float4*>(s + 2 * plane), b1 = *reinterpret_cast<const float4*>(s + 2 * plane + 4);
    X[0] = x0.x; X[1] = x0.y; X[2] = x0.z; X[3] = x0.w; X[4] = x1.x; X[5] = x1.y; X[6] = x1.z; X[7] = x1.w;
    Y[0] = y0.x; Y[1] = y0.y; Y[2] = y0.z; Y[3] = y0.w; Y[4] = y1.x; Y[5] = y1.y; Y[6] = y1.z; Y[7] = y1.w;
    B[0] = b0.x; B[1] = b0.y; B[2] = b0.z; B[3] = b0.w; B[4] = b1.x; B[5] = b1.y; B[6] = b1.z; B[7] = b1.w;
  }
#pragma unroll
  for (int x = 0; x < 8; x++) {
    const float n = EncFromRight(Y[x]);  // the next lane: the row below
    N[x] = row == 7 ? Y[x] : n;          // (row 7 pairs with itself)
  }
  // ---- fuzzy erosion: cell (row >> 1, row & 1) of the block in lanes 0..3 (the other four repeat them)
  float v;
  {
    const uint32_t cw = P.xp >> 2, ch = P.yp >> 2;
    const uint32_t cy = by * 2 + ((row >> 1) & 1), cx = lbx * 2 + (row & 1);
    const uint32_t ya = cy ? cy - 1 : cy, yc = cy + 1 < ch ? cy + 1 : cy, xa = cx ? cx - 1 : cx, xc = cx + 1 < cw ? cx + 1 : cx;
    const float* ra = P.cells + size_t(ya) * cw;
    const float* rb = P.cells + size_t(cy) * cw;
    const float* rc = P.cells + size_t(yc) * cw;
    const float nb[9] = {ra[xa], ra[cx], ra[xc], rb[xa], rb[cx], rb[xc], rc[xa], rc[cx], rc[xc]};
    float m0 = nb[0], m1 = INFINITY, m2 = INFINITY, m3 = INFINITY;  // the four smallest, ascending
#pragma unroll
    for (int i = 1; i < 9; i++) {
      const float a0 = fminf(m0, nb[i]), b0 = fmaxf(m0, nb[i]);
      const float a1 = fminf(m1, b0), b1 = fmaxf(m1, b0);
      const float a2 = fminf(m2, b1), b2 = fmaxf(m2, b1);
      m3 = fminf(m3, b2);
      m0 = a0; m1 = a1; m2 = a2;
    }
    v = P.w[0] * m0 + P.w[1] * m1 + P.w[2] * m2 + P.w[3] * m3;
  }
  const float e = ((__shfl(v, first, 64) + __shfl(v, first + 1, 64)) + __shfl(v, first + 2, 64)) + __shfl(v, first + 3, 64);
  // ---- ComputeMask
  float m;
  {
    const float kOffset3 = 3.7179635626140772f, kOffset4 = 0.25f * kOffset3;
    const float v1 = fmaxf(e * 0.80061762862741759f, 1e-3f);
    const float v2 = 1.0f / (v1 + 302.59587815579727f);
    const float v3 = 1.0f / (v1 * v1 + kOffset3);
    const float v4 = 1.0f / (v1 * v1 + kOffset4);
    m = -0.7647f + (9.4708735624378946f * v4 + (17.35036561631863f * v2 + 6.7943250517376494f * v3));
  }
  // ---- the row's terms of the three sums
  float sg = 0.0f, sh = 0.0f, sb = 0.0f;
#pragma unroll
  for (int x = 0; x < 8; x++) {
    const float iny = Y[x] + 0.16f;
    sg += EncGammaRatio<true>(iny - X[x]);
    sg += EncGammaRatio<true>(iny + X[x]);
    if (x < 7) sh += fminf(0.0206f, fabsf(Y[x] - Y[x + 1]));
    sh += fminf(0.0206f, fabsf(Y[x] - N[x]));
    const float pye = (Y[x] + 0.0031994768654636393f) + fabsf(X[x]);
    sb += B[x] > pye ? fminf(B[x] - pye, 0.010474084867598155f) : 0.0f;
  }
#pragma unroll
  for (int d = 1; d < 8; d <<= 1) {  // (r0 + r1) + (r2 + r3) ... : addition commutes, every lane of the block holds the same sum
    sg += __shfl_xor(sg, d, 64);
    sh += __shfl_xor(sh, d, 64);
    sb += __shfl_xor(sb, d, 64);
  }
  m = 0.1005613337192697f * log2f(sg * (0.5f / 64)) + m;  // GammaModulation
  const float hf = (sh * -0.38f + 0.42f) + m;              // HfModulation
  const float kLimit = 0.010474084867598155f, kMaxLimit = 15.463398341612438f;
  if (sb >= 32 * kLimit) sb = 64 * kLimit - sb;            // BlueModulation: all blue is no reason to spend bits
  if (sb >= kMaxLimit * kLimit) sb = kMaxLimit * kLimit;
  sb *= 0.90590804735610064f;
  const float blue = sb + m;
  const float out = fminf(hf, blue);
  if (live && row == 0) {
    const size_t bi = size_t(by) * P.xb + bx;
    P.aq[bi] = exp2f(out * 1.442695041f) * P.mul + P.add;
    P.mask[bi] = 1.0f / (e + 0.001f);
  }
}

// ---------------------------------------------------------------- per-pixel masking (mask1x1)
// What the reference's AC-strategy search reads per pixel (enc_adaptive_quantization.cc ComputeTile :498-526, Blur1x1Masking
// :634-662 with the border rule of convolve_symmetric5.cc:35-97), from the Y plane before the sharpening, as csrc/enc/jxl_enc.cc
// Masking1x1 states it in float32: v = 1 / (log1p(|ratio<false>(Y + 0.019) (Y - base)|) + 0.01) with the Laplacian's
// neighbours clamped to the plane, then the symmetric 5x5 blur of v with rows and columns outside the plane mirrored.
// A workgroup owns kMaskCols x kMaskRows outputs: it forms v over them and two samples of halo either side in LDS (a halo
// sample outside the plane is v at its mirror image, formed from Y like any other), then every lane blurs four rows of one
// column out of a register window of 8 x 5 samples.
struct EncMask1x1 {
  const float* y;  // [yp][xp] the Y plane
  float* out;      // [yp][xp]
  uint32_t xp, yp;
  float w[6];      // c, r, R, d, L, D of the blur: jxh::EncMask1x1Weights
};
constexpr int kMaskCols = 64, kMaskRows = 16;
__global__ __launch_bounds__(256) void k_enc_mask1x1(EncMask1x1 P) {
#pragma clang fp contract(off)
  constexpr int W = kMaskCols + 4, H = kMaskRows + 4;
  __shared__ float s[H][W];
  const int xp = int(P.xp), yp = int(P.yp);
  const int X0 = int(blockIdx.x) * kMaskCols, Y0 = int(blockIdx.y) * kMaskRows;
  for (int i = threadIdx.x; i < W * H; i += 256) {
    const int ly = i / W, lx = i - ly * W;
    const int gx = X0 - 2 + lx, gy = Y0 - 2 + ly;  // -2 .. : at most two beyond either edge where an output reads it
    float v = 0.0f;
    if (gx <= xp + 1 && gy <= yp + 1) {  // (further out only the dead outputs of a partial tile would read)
      // Mirror (image_ops.h:184-196); xp, yp >= 8, so one reflection brings -2 .. n + 1 inside
      const int x = gx < 0 ? -gx - 1 : gx >= xp ? 2 * xp - 1 - gx : gx;
      const int y = gy < 0 ? -gy - 1 : gy >= yp ? 2 * yp - 1 - gy : gy;
      const float* row = P.y + size_t(y) * xp;
      const float cur = row[x];
      const float up = P.y[size_t(y ? y - 1 : y) * xp + x], down = P.y[size_t(y + 1 < yp ? y + 1 : y) * xp + x];
      const float left = row[x ? x - 1 : x], right = row[x + 1 < xp ? x + 1 : x];
      const float base = 0.25f * (down + up + left + right);
      const float d = fabsf(EncGammaRatio<false>(cur + 0.019f) * (cur - base));
      v = 1.0f / (log1pf(d) + 0.01f);
    }
    s[ly][lx] = v;
  }
  __syncthreads();
  const int lx = threadIdx.x & 63, r0 = int(threadIdx.x >> 6) * 4;  // rows r0 .. r0 + 3 of column lx
  float win[8][5];
#pragma unroll
  for (int j = 0; j < 8; j++)
#pragma unroll
    for (int k = 0; k < 5; k++) win[j][k] = s[r0 + j][lx + k];
  const int gx = X0 + lx;
  if (gx >= xp) return;
  auto row_sum = [](const float (&r)[5], float w0, float w1, float w2) {
    const float s2 = w2 * (r[0] + r[4]), s1 = w1 * (r[1] + r[3]), s0 = w0 * r[2];
    return s2 + (s1 + s0);
  };
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int gy = Y0 + r0 + j;
    float sum0 = row_sum(win[j + 2], P.w[0], P.w[1], P.w[2]);
    sum0 += row_sum(win[j], P.w[2], P.w[4], P.w[5]);
    float sum1 = row_sum(win[j + 4], P.w[2], P.w[4], P.w[5]);
    sum0 += row_sum(win[j + 1], P.w[1], P.w[3], P.w[4]);
    sum1 += row_sum(win[j + 3], P.w[1], P.w[3], P.w[4]);
    if (gy < yp) P.out[size_t(gy) * xp + gx] = sum0 + sum1;
  }
}

// Transform selection and quant field of one 64x64 tile (8x8 blocks) per wave: every candidate is aligned to its own
// size, so the greedy raster scan of the CPU writer never looks outside the tile it is in. The activity tests of every
// (position, candidate) pair are evaluated by the lanes in parallel; only the occupancy bookkeeping of the scan is serial.
// AQ = true (quant_field_mode 1): the quant field is the aggregation of the adaptive field P.aq_map over each transform
// (AdjustQuantField, enc_adaptive_quantization.cc:1198-1247, and Quantizer::SetQuantFieldRect, quantizer.cc:78-88);
// AQ = false is the writer's activity rule, compiled as it was before the other form existed.
template <bool AQ>
__global__ __launch_bounds__(64) void k_enc_select(EncFwd P) {
#pragma clang fp contract(off)
  const uint32_t tiles_x = (P.xb + 7) / 8;
  const uint32_t t = blockIdx.x, lane = threadIdx.x, x = lane & 7, y = lane >> 3;
  __shared__ float s_act[64];
  __shared__ uint32_t s_pass[64];
  __shared__ uint8_t s_acs[64];
  const uint32_t bx0 = (t % tiles_x) * 8, by0 = (t / tiles_x) * 8;
  const uint32_t w = min(8u, P.xb - bx0), h = min(8u, P.yb - by0);
  const bool inside = x < w && y < h;
  s_act[lane] = inside ? P.act[size_t(by0 + y) * P.xb + bx0 + x] : 0.0f;
  __shared__ float s_aq[64];  // (AQ only: the other form never names it and carries no LDS for it)
  if (AQ) s_aq[lane] = inside ? P.aq_map[size_t(by0 + y) * P.xb + bx0 + x] : 0.0f;
  s_acs[lane] = 0xFF;
  __syncthreads();
  const float T64 = 0.004f * P.distance, T32 = 0.008f * P.distance, T16 = 0.016f * P.distance, TR = 0.011f * P.distance;
  const uint8_t cand[11] = {18, 20, 19, 5, 11, 10, 4, 9, 8, 7, 6};  // in the order the scan tries them
  const float thr[11] = {T64, T64 * 1.3f, T64 * 1.3f, T32, TR, TR, T16, T16 * 0.8f, T16 * 0.8f, T16 * 1.5f, T16 * 1.5f};
  auto region_max = [&](uint32_t bx, uint32_t by, uint32_t cx, uint32_t cy) {
    float m = 0.0f;
    for (uint32_t yy = 0; yy < cy; yy++)
      for (uint32_t xx = 0; xx < cx; xx++) m = fmaxf(m, s_act[(by + yy) * 8 + bx + xx]);
    return m;
  };
  uint32_t pass = 0;
  if (inside && P.strategy_mode == 1)
    for (int s = 0; s < 11; s++) {
      const uint32_t cx = c_covered_x[cand[s]], cy = c_covered_y[cand[s]];
      if (x % cx || y % cy || x + cx > w || y + cy > h) continue;
      if (region_max(x, y, cx, cy) < thr[s]) pass |= 1u << s;
    }
  s_pass[lane] = pass;
  __syncthreads();
  if (lane == 0) {
    uint64_t occupied = 0;
    for (uint32_t by = 0; by < h; by++)
      for (uint32_t bx = 0; bx < w; bx++) {
        if (occupied >> (by * 8 + bx) & 1) continue;
        int st = 0;
        uint64_t mask = uint64_t(1) << (by * 8 + bx);
        for (uint32_t ps = s_pass[by * 8 + bx]; ps; ps &= ps - 1) {
          const int s = __builtin_ctz(ps);
          const uint32_t cx = c_covered_x[cand[s]], cy = c_covered_y[cand[s]];
          const uint64_t row = ((uint64_t(1) << cx) - 1) << bx;  // cx <= 8
          uint64_t m = 0;
          for (uint32_t yy = 0; yy < cy; yy++) m |= row << ((by + yy) * 8);
          if (occupied & m) continue;
          st = cand[s];
          mask = m;
          break;
        }
        occupied |= mask;
        const uint32_t cx = c_covered_x[st], cy = c_covered_y[st];
        for (uint32_t yy = 0; yy < cy; yy++)
          for (uint32_t xx = 0; xx < cx; xx++) s_acs[(by + yy) * 8 + bx + xx] = uint8_t((st << 1) | ((xx | yy) == 0));
      }
  }
  __syncthreads();
  if (!inside) return;
  const uint8_t a = s_acs[lane];
  const size_t bi = size_t(by0 + y) * P.xb + bx0 + x;
  P.acs[bi] = a;
  int32_t q = 0;
  if (AQ) {
    if (a & 1) {
      // the covered blocks in raster order: the largest, and the mean mixed in from four blocks on
      const int st = a >> 1;
      const uint32_t cx = c_covered_x[st], cy = c_covered_y[st];
      float mx = s_aq[lane], mean = 0.0f;
      for (uint32_t yy = 0; yy < cy; yy++)
        for (uint32_t xx = 0; xx < cx; xx++) {
          const float v = s_aq[(y + yy) * 8 + x + xx];
          mean += v;
          mx = fmaxf(v, mx);
        }
      mean /= float(cy * cx);
      if (cy * cx >= 4) {
        mx *= P.mean_max_mixer;
        mx += (1.0f - P.mean_max_mixer) * mean;
      }
      q = int(fmaxf(1.0f, fminf(mx * P.inv_gs + 0.5f, 256.0f)));
    }
  } else if (a & 1) {
    const int st = a >> 1;
    const float m = region_max(x, y, c_covered_x[st], c_covered_y[st]);
    float mul = 1.35f - 0.12f * log2f(1.0f + m * 400.0f);
    mul = fmaxf(0.8f, fminf(1.4f, mul));
    q = max(1, min(256, int(P.quant_ac * mul * P.inv_gs + 0.5f)));
  }
  P.qf[bi] = q;
}

// Coefficient offsets of the first blocks of one 256x256 group, in the raster order the bitstream uses: one wave per
// group, 16 consecutive raster positions per lane, exclusive scan across the lanes.
__global__ __launch_bounds__(64) void k_enc_offsets(EncFwd P) {
  const uint32_t g = blockIdx.x, lane = threadIdx.x;
  const uint32_t bx0 = (g % P.xg) * 32, by0 = (g / P.xg) * 32;
  const uint32_t gw = min(32u, P.xb - bx0), gh = min(32u, P.yb - by0), n = gw * gh;
  uint32_t sizes[16], sum = 0;
  for (uint32_t j = 0; j < 16; j++) {
    const uint32_t i = lane * 16 + j;
    uint32_t sz = 0;
    if (i < n) {
      const uint8_t a = P.acs[size_t(by0 + i / gw) * P.xb + bx0 + i % gw];
      if (a & 1) sz = 64u << c_log2_covered[a >> 1];
    }
    sizes[j] = sz;
    sum += sz;
  }
  uint32_t incl = sum;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 64);
    if (int(lane) >= d) incl += o;
  }
  uint32_t offset = incl - sum;
  for (uint32_t j = 0; j < 16; j++) {
    const uint32_t i = lane * 16 + j;
    if (i < n && sizes[j]) P.coef_off[size_t(by0 + i / gw) * P.xb + bx0 + i % gw] = offset;
    offset += sizes[j];
  }
}

__device__ __forceinline__ int32_t EncQuant(float v) {
  const float r = rintf(v);
  return fabsf(v) < 0.58f ? 0 : int32_t(r);
}

// One workgroup per transform: forward scaled DCT (matrix form, rows then columns), DC of the covered blocks from the
// lowest-frequency corner (the inverse of LowestFrequenciesFromDC, enc_transforms-inl.h DCFromLowestFrequencies), then
// quantisation: Y first, X and B as residuals of the chroma-from-luma prediction from the DEQUANTISED Y
// (enc_group.cc:455-520, QuantizeRoundtripYBlockAC :329-378).
template <int kThreads>
__global__ __launch_bounds__(kThreads) void k_enc_transform(EncFwd P) {
#pragma clang fp contract(off)
  const uint32_t bi = blockIdx.x, abx = bi % P.xb, aby = bi / P.xb, tid = threadIdx.x;
  const uint8_t a = P.acs[bi];
  if (!(a & 1)) return;
  const int st = a >> 1;
  const int cx = c_covered_x[st], cy = c_covered_y[st], R = cy * 8, C = cx * 8, size = R * C;
  const int cstride = max(cx, cy) * 8, lrows = min(cx, cy), lcols = max(cx, cy);
  __shared__ float s_a[4096], s_t[4096], s_yd[4096], s_ydc[64];
  const float* bc = P.basis_t + (size_t(C) * C - 1) / 3;
  const float* br = P.basis_t + (size_t(R) * R - 1) / 3;
  const float* bcc = P.basis_t + (size_t(cx) * cx - 1) / 3;
  const float* brr = P.basis_t + (size_t(cy) * cy - 1) / 3;
  const size_t plane = size_t(P.xp) * P.yp;
  const uint32_t g = (aby / 32) * P.xg + abx / 32, off = P.coef_off[bi];
  const float scaled = P.inv_gs / float(P.qf[bi]);
  const float norm = 1.0f / (float(R) * float(C));
  const int kind = c_strategy_qtable[st];
  const float biases1 = 1.0f - 0.07005449891748593f, biases3 = 0.145f;
  for (int ci = 0; ci < 3; ci++) {
    const int c = ci == 0 ? 1 : (ci == 1 ? 0 : 2);
    const float* src = P.planes + plane * c + size_t(aby) * 8 * P.xp + size_t(abx) * 8;
    for (int i = tid; i < size; i += kThreads) s_a[i] = src[size_t(i / C) * P.xp + i % C];
    __syncthreads();
    for (int o = tid; o < size; o += kThreads) {
      const int y = o / C, kx = o % C;
      float s = 0;
      for (int x = 0; x < C; x++) s += s_a[y * C + x] * bc[x * C + kx];
      s_t[o] = s;
    }
    __syncthreads();
    for (int o = tid; o < size; o += kThreads) {
      const int ky = o / C, kx = o % C;
      float s = 0;
      for (int y = 0; y < R; y++) s += s_t[y * C + kx] * br[y * R + ky];
      s *= norm;
      s_a[R < C ? ky * C + kx : kx * R + ky] = s;
    }
    __syncthreads();
    if (int(tid) < cx * cy) {
      const int y = tid / cx, x = tid % cx;
      float s = 0;
      for (int ky = 0; ky < cy; ky++)
        for (int kx = 0; kx < cx; kx++) {
          const float cf = (R < C) ? s_a[ky * cstride + kx] : s_a[kx * cstride + ky];
          const float llf = cf / (c_resample[cy - 1 + ky] * c_resample[cx - 1 + kx]);
          s += llf * brr[y * cy + ky] * bcc[x * cx + kx];
        }
      const size_t di = size_t(aby + y) * P.xb + abx + x;
      const size_t nb = size_t(P.xb) * P.yb;
      if (c == 1) {
        const int32_t qy = int32_t(lroundf(s / P.dc_step[1]));
        s_ydc[tid] = float(qy) * P.dc_step[1];
        P.dc[nb + di] = qy;
      } else if (c == 0) {
        P.dc[di] = int32_t(lroundf((s - 0.0f * s_ydc[tid]) / P.dc_step[0]));
      } else {
        P.dc[2 * nb + di] = int32_t(lroundf((s - 1.0f * s_ydc[tid]) / P.dc_step[2]));
      }
    }
    const float mulc = c == 0 ? scaled * P.x_dm : (c == 1 ? scaled : scaled * P.b_dm);
    const float cc = c == 0 ? 0.0f : 1.0f;  // chroma-from-luma factors of the default colour correlation (0 and 1)
    const float* m = P.dequant + P.dq_offset[kind] + size_t(c) * P.dq_size[kind];
    int32_t* dst = P.coeffs + (size_t(g) * 3 + c) * 65536 + off;
    for (int k = tid; k < size; k += kThreads) {
      const int row = k / cstride, col = k % cstride;
      int32_t q = 0;
      if (!(row < lrows && col < lcols)) {
        if (c == 1) {
          q = EncQuant(s_a[k] / (m[k] * mulc));
          const float ybias = q == 0 ? 0.0f : (q == 1 ? biases1 : (q == -1 ? -biases1 : float(q) - biases3 / float(q)));
          s_yd[k] = ybias * (m[k] * mulc);
        } else {
          q = EncQuant((s_a[k] - cc * s_yd[k]) / (m[k] * mulc));
        }
      }
      dst[k] = q;
    }
    __syncthreads();
  }
}

// The same work for one 64x64 tile (8x8 blocks) per workgroup, every transform of the tile at once: the tile's samples,
// the row-pass result and the DCT matrices of 1..64 points sit in LDS; thread (column, 16-row band) accumulates 8 rows
// against one matrix element at a time, so that a matrix read serves 8 multiply-adds and the sample reads are
// broadcasts. Sums run in the CPU writer's order (x = 0.., y = 0..), products are not contracted.
__global__ __launch_bounds__(256) void k_enc_transform_tile(EncFwd P) {
#pragma clang fp contract(off)
  // the DCT matrices of 1..32 points in LDS ((4^6 - 1) / 3 floats: levels 0..5); the 64-point one (16 KB, only the three
  // largest transforms use it) is read in place, which lets four workgroups share a CU instead of two
  constexpr int kBasisLds = 1365;
  // (the level of N points starts at (N * N - 1) / 3, which is 1 mod 4: shifted by 3 floats so that rows are 16-byte aligned)
  __shared__ __attribute__((aligned(16))) float s_px[64 * 64], s_t[64 * 64], s_basis_raw[kBasisLds + 3];
  __shared__ float s_ydc[64];
  float* const s_basis = s_basis_raw + 3;
  __shared__ uint32_t s_info[64], s_off[64];
  __shared__ int32_t s_qf[64];
  __shared__ float s_red[8], s_cc;
  __shared__ uint32_t s_cells;  // blocks of the tile that lie inside the frame
  const uint32_t tiles_x = (P.xb + 7) / 8;
  const uint32_t bx0 = (blockIdx.x % tiles_x) * 8, by0 = (blockIdx.x / tiles_x) * 8, tid = threadIdx.x;
  const uint32_t w = min(8u, P.xb - bx0), h = min(8u, P.yb - by0);
  for (int i = tid; i < kBasisLds; i += 256) s_basis[i] = P.basis_t[i];
  if (tid < 64) s_info[tid] = 0xFFFFFFFFu;
  __syncthreads();
  if (tid < 64) {
    const uint32_t x = tid & 7, y = tid >> 3;
    if (x < w && y < h) {
      const size_t bi = size_t(by0 + y) * P.xb + bx0 + x;
      const uint8_t a = P.acs[bi];
      if (a & 1) {
        const uint32_t st = a >> 1, cx = c_covered_x[st], cy = c_covered_y[st], off = P.coef_off[bi];
        const int32_t q = P.qf[bi];
        for (uint32_t dy = 0; dy < cy; dy++)
          for (uint32_t dx = 0; dx < cx; dx++) {
            const uint32_t cell = (y + dy) * 8 + x + dx;
            s_info[cell] = x | y << 3 | st << 6;
            s_off[cell] = off;
            s_qf[cell] = q;
          }
      }
    }
  }
  __syncthreads();
  if (tid < 64) {
    const unsigned long long m = __ballot(s_info[tid] != 0xFFFFFFFFu);
    if (tid == 0) s_cells = uint32_t(__popcll(m));
  }
  const uint32_t col = tid & 63, band = tid >> 6;  // this thread: tile column `col`, cell rows 2 * band and 2 * band + 1
  const uint32_t g = (by0 / 32) * P.xg + bx0 / 32;
  const size_t plane = size_t(P.xp) * P.yp, nb = size_t(P.xb) * P.yb;
  const float biases1 = 1.0f - 0.07005449891748593f, biases3 = 0.145f;
  float ydeq[2][8], ycoef[2][8];
  for (int ci = 0; ci < 3; ci++) {
    const int c = ci == 0 ? 1 : (ci == 1 ? 0 : 2);
    __syncthreads();
    {
      // (all sixteen loads of a thread in flight before the first one is used; requesting the next channel's during this
      // one's transform was measured slower: 0.208 -> 0.255 ms per 4K frame)
      const float* src = P.planes + plane * c + size_t(by0) * 8 * P.xp + size_t(bx0) * 8;
      float px[16];
#pragma unroll
      for (uint32_t u = 0; u < 16; u++) {
        const uint32_t i = tid + u * 256, y = i >> 6, x = i & 63;
        px[u] = (x < w * 8 && y < h * 8) ? src[size_t(y) * P.xp + x] : 0.0f;
      }
#pragma unroll
      for (uint32_t u = 0; u < 16; u++) s_px[tid + u * 256] = px[u];
    }
    __syncthreads();
    // rows: s_t[y][kx] = sum_x px[y][x0 + x] * B_C[x][kx]
    for (uint32_t half = 0; half < 2; half++) {
      const uint32_t cr = band * 2 + half, info = s_info[cr * 8 + (col >> 3)];
      if (info == 0xFFFFFFFFu) continue;
      const uint32_t ox = info & 7, C = uint32_t(c_covered_x[info >> 6]) * 8, kx = col - ox * 8;
      const float* px = s_px + cr * 8 * 64 + ox * 8;
      float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      auto rows = [&](const float* B) {
        for (uint32_t x = 0; x < C; x += 4) {  // four samples of each of the 8 rows per LDS read (a broadcast within a block)
          float4 v[8];
          for (int j = 0; j < 8; j++) v[j] = *reinterpret_cast<const float4*>(px + j * 64 + x);
          const float b0 = B[x * C], b1 = B[(x + 1) * C], b2 = B[(x + 2) * C], b3 = B[(x + 3) * C];
          for (int j = 0; j < 8; j++) {
            acc[j] += v[j].x * b0;
            acc[j] += v[j].y * b1;
            acc[j] += v[j].z * b2;
            acc[j] += v[j].w * b3;
          }
        }
      };
      if (C == 64) rows(P.basis_t + 1365 + kx);
      else rows(s_basis + (C * C - 1) / 3 + kx);
      for (int j = 0; j < 8; j++) s_t[(cr * 8 + j) * 64 + col] = acc[j];
    }
    __syncthreads();
    // columns: coefficient (ky, kx) at s_px[y0 + ky][col], natural layout
    for (uint32_t half = 0; half < 2; half++) {
      const uint32_t cr = band * 2 + half, info = s_info[cr * 8 + (col >> 3)];
      if (info == 0xFFFFFFFFu) continue;
      const uint32_t st = info >> 6, oy = (info >> 3) & 7, R = uint32_t(c_covered_y[st]) * 8, C = uint32_t(c_covered_x[st]) * 8;
      const uint32_t ky0 = (cr - oy) * 8;
      const float* tc = s_t + oy * 8 * 64 + col;
      float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (R == 64) {  // (the table in place: its rows are 4-byte aligned only)
        const float* B = P.basis_t + 1365 + ky0;
        for (uint32_t y = 0; y < R; y++) {
          const float v = tc[y * 64];
          for (int j = 0; j < 8; j++) acc[j] += v * B[y * R + j];
        }
      } else {
        const float* B = s_basis + (R * R - 1) / 3 + ky0;
        for (uint32_t y = 0; y < R; y++) {
          const float v = tc[y * 64];
          const float4 ba = *reinterpret_cast<const float4*>(B + y * R), bb = *reinterpret_cast<const float4*>(B + y * R + 4);
          acc[0] += v * ba.x;
          acc[1] += v * ba.y;
          acc[2] += v * ba.z;
          acc[3] += v * ba.w;
          acc[4] += v * bb.x;
          acc[5] += v * bb.y;
          acc[6] += v * bb.z;
          acc[7] += v * bb.w;
        }
      }
      const float norm = 1.0f / (float(R) * float(C));
      for (int j = 0; j < 8; j++) s_px[(cr * 8 + j) * 64 + col] = acc[j] * norm;
    }
    __syncthreads();
    // DC of every covered block from the lowest-frequency corner
    if (tid < 64 && s_info[tid] != 0xFFFFFFFFu) {
      const uint32_t info = s_info[tid], st = info >> 6, ox = info & 7, oy = (info >> 3) & 7;
      const int cx = c_covered_x[st], cy = c_covered_y[st], x = int(tid & 7) - int(ox), y = int(tid >> 3) - int(oy);
      const float* brr = s_basis + (cy * cy - 1) / 3;
      const float* bcc = s_basis + (cx * cx - 1) / 3;
      float s = 0;
      for (int ky = 0; ky < cy; ky++)
        for (int kx = 0; kx < cx; kx++) {
          const float llf = s_px[(oy * 8 + ky) * 64 + ox * 8 + kx] / (c_resample[cy - 1 + ky] * c_resample[cx - 1 + kx]);
          s += llf * brr[y * cy + ky] * bcc[x * cx + kx];
        }
      const size_t di = size_t(by0 + (tid >> 3)) * P.xb + bx0 + (tid & 7);
      if (c == 1) {
        const int32_t qy = int32_t(lroundf(s / P.dc_step[1]));
        s_ydc[tid] = float(qy) * P.dc_step[1];
        P.dc[nb + di] = qy;
      } else if (c == 0) {
        P.dc[di] = int32_t(lroundf((s - 0.0f * s_ydc[tid]) / P.dc_step[0]));
      } else {
        P.dc[2 * nb + di] = int32_t(lroundf((s - 1.0f * s_ydc[tid]) / P.dc_step[2]));
      }
    }
    // chroma-from-luma factor of the tile for this channel: the least squares of the reference's fast FindBestMultiplier
    // over the tile's AC coefficients (a = Y * w / 84, b = base * Y * w - chroma * w, w = Scale * 128 * qf / matrix)
    float cc = c == 0 ? 0.0f : 1.0f;  // (the default factors: 0 on X, the base correlation 1 on B)
    if (c == 1 || P.cfl_fit) {
      float sa2 = 0.0f, sab = 0.0f;
      for (uint32_t half = 0; half < 2; half++) {
        const uint32_t cr = band * 2 + half, cell = cr * 8 + (col >> 3), info = s_info[cell];
        if (info == 0xFFFFFFFFu) continue;
        const uint32_t st = info >> 6, ox = info & 7, oy = (info >> 3) & 7;
        const uint32_t cx = c_covered_x[st], cy = c_covered_y[st], R = cy * 8, C = cx * 8;
        const uint32_t kx = col - ox * 8, ky0 = (cr - oy) * 8;
        if (c == 1) {
          for (uint32_t j = 0; j < 8; j++) ycoef[half][j] = s_px[(cr * 8 + j) * 64 + col];
          continue;
        }
        const int kind = c_strategy_qtable[st];
        const float* m = P.dequant + P.dq_offset[kind] + size_t(c) * P.dq_size[kind];
        const float q = P.scale * 128.0f * float(s_qf[cell]);
        float mk[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) mk[j] = m[R < C ? (ky0 + j) * C + kx : kx * R + ky0 + j];
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
          const uint32_t ky = ky0 + j;
          if (ky < cy && kx < cx) continue;
          const float w = q / mk[j], yw = ycoef[half][j] * w;
          const float a = (1.0f / 84) * yw, b = cc * yw - s_px[(cr * 8 + j) * 64 + col] * w;
          sa2 += a * a;
          sab += a * b;
        }
      }
      if (c != 1) {
        for (int d = 32; d > 0; d >>= 1) {
          sa2 += __shfl_down(sa2, d, 64);
          sab += __shfl_down(sab, d, 64);
        }
        if ((tid & 63) == 0) {
          s_red[(tid >> 6) * 2] = sa2;
          s_red[(tid >> 6) * 2 + 1] = sab;
        }
        __syncthreads();
        if (tid == 0) {
          const float ta2 = (s_red[0] + s_red[2]) + (s_red[4] + s_red[6]), tab = (s_red[1] + s_red[3]) + (s_red[5] + s_red[7]);
          const uint32_t cells = s_cells;
          const float num = float(cells * 64);
          float x = cells ? -tab / (ta2 + num * 1e-9f * 0.5f) : 0.0f;
          x = x >= 2.6f ? x - 2.6f : (x <= -2.6f ? x + 2.6f : 0.0f);
          const float v = fmaxf(-128.0f, fminf(127.0f, roundf(x)));
          (c == 0 ? P.ytox : P.ytob)[blockIdx.x] = int8_t(v);
          s_cc = cc + v / 84.0f;
        }
        __syncthreads();
        cc = s_cc;
      }
    }
    // quantisation of this thread's 2 x 8 coefficients
    for (uint32_t half = 0; half < 2; half++) {
      const uint32_t cr = band * 2 + half, cell = cr * 8 + (col >> 3), info = s_info[cell];
      if (info == 0xFFFFFFFFu) continue;
      const uint32_t st = info >> 6, ox = info & 7, oy = (info >> 3) & 7;
      const uint32_t cx = c_covered_x[st], cy = c_covered_y[st], R = cy * 8, C = cx * 8;
      const uint32_t kx = col - ox * 8, ky0 = (cr - oy) * 8;
      const int kind = c_strategy_qtable[st];
      const float scaled = P.inv_gs / float(s_qf[cell]);
      const float mulc = c == 0 ? scaled * P.x_dm : (c == 1 ? scaled : scaled * P.b_dm);
      const float* m = P.dequant + P.dq_offset[kind] + size_t(c) * P.dq_size[kind];
      int32_t* dst = P.coeffs + (size_t(g) * 3 + c) * 65536 + s_off[cell];
      int32_t q[8];
      float mk[8];  // (the table entries first: eight independent loads)
#pragma unroll
      for (uint32_t j = 0; j < 8; j++) mk[j] = m[R < C ? (ky0 + j) * C + kx : kx * R + ky0 + j];
#pragma unroll
      for (uint32_t j = 0; j < 8; j++) {
        const uint32_t ky = ky0 + j;
        q[j] = 0;
        if (ky < cy && kx < cx) continue;  // lowest frequencies: carried by the DC image
        const float v = s_px[(cr * 8 + j) * 64 + col], step = mk[j] * mulc;
        if (c == 1) {
          q[j] = EncQuant(v / step);
          const float ybias = q[j] == 0 ? 0.0f : (q[j] == 1 ? biases1 : (q[j] == -1 ? -biases1 : float(q[j]) - biases3 / float(q[j])));
          ydeq[half][j] = ybias * step;
        } else {
          q[j] = EncQuant((v - cc * ydeq[half][j]) / step);
        }
      }
      if (R < C) {
        for (uint32_t j = 0; j < 8; j++) dst[(ky0 + j) * C + kx] = q[j];
      } else {  // 8 consecutive coefficients of column kx
        int4* d4 = reinterpret_cast<int4*>(dst + kx * R + ky0);
        d4[0] = make_int4(q[0], q[1], q[2], q[3]);
        d4[1] = make_int4(q[4], q[5], q[6], q[7]);
      }
    }
  }
}

// ---------------------------------------------------------------- cost estimate of the AC-strategy search
// EstimateEntropy of the reference (enc_ac_strategy.cc:364-511) for a list of candidate transforms of ONE pure-DCT kind
// (the launch layer sorts a caller's list by kind), as csrc/enc/jxl_enc.cc EstimateEntropy states it in float32: the three
// forward transforms, val = (coef - factor * coef_Y) * ((1 / m) * quant_norm16), its rounding, m * (val - round(val)) taken
// back to pixels, times mask1x1 + {12, 0, 4}, to the eighth power, and the sums of sqrt(|round|), of the non-zero roundings
// and of that loss. An estimate depends on its candidate alone, so the order of the list does not matter.
// Two forms, by the transform's size:
//   k_enc_estimate<64, 1>   a wave per candidate, four candidates per workgroup, for 64 .. 512 samples (8x8 .. 32x16): every
//                           lane forms one output of a pass at a time (an 8x8 has exactly one per lane)
//   k_enc_estimate<256, NB> a workgroup per candidate from 32x32 up: a thread accumulates NB outputs (4 at 32x32, else 8)
//                           against one matrix element at a time, as k_enc_transform_tile does
// Per group three LDS buffers of the transform's size (at most 16 KB each: 48 KB per workgroup, three workgroups per CU):
// a (samples, then X's / B's coefficients, then the error, then the loss terms), t (the pass between rows and columns) and
// y (Y's coefficients, which X and B are predicted from: Y is processed first, the three shares are kept apart and combined
// by one lane in the reference's order X, Y, B). The DCT matrices up to 32 points are in LDS (the wave form: all of 1 .. 32;
// the workgroup form: the 32-point one, which is all it needs besides the 64-point one); the 64-point one is read in place.
// The inverse's column pass stores its result transposed so that the row pass reads LDS conflict-free.
// Sums: the four matrix passes add in the CPU statement's order (index ascending, not contracted). The three reductions
// follow EstimateLaneSum of the CPU statement, which was written to their shape: lane l adds elements l, l + lanes, ..;
// within a wave pairwise at distances 32 .. 1 (shfl_xor: both partners form the same sum); the four waves of a workgroup
// through LDS as (s0 + s1) + (s2 + s3). No atomics: the result does not depend on scheduling. The quant field's 16-norm is
// summed by every lane alike in raster order, as the CPU statement does.
struct EncEstimate {
  const float* planes;  // [3][yp][xp]
  const float* quant;   // [yp / 8][xb] the quant field per block
  const float* mask;    // [yp][xp] mask1x1
  const int8_t* ytox;   // per 64x64 tile
  const int8_t* ytob;
  const float* basis_t;                // [n][k] DCT matrices, level of N points at (N * N - 1) / 3
  const float* dequant;                // this kind's weights: [3][R * C] in the codestream layout
  const JxlHipEncAcsCandidate* cand;   // this launch's candidates (all of one strategy)
  const uint32_t* index;               // ... their places in the caller's list
  const unsigned long long* scaled_at; // ... where their `scaled` values start (read only if scaled is set)
  float* estimates;                    // [the caller's n]
  float* scaled;                       // or NULL
  uint32_t n, xp, yp, xb, tiles_x;
  uint32_t cx, cy;                     // blocks covered by the launch's transform
  float weights[3];                    // info_loss_multiplier, zeros_mul, cost_delta
  float channel_mul[3];
  float x_weight;                      // (1 for a single block)
};
__device__ __forceinline__ uint32_t EncCeilLog2Nonzero(uint32_t v) { return v <= 1 ? 0u : 32u - uint32_t(__clz(int(v - 1))); }
template <int kLanes, int NB>
__global__ __launch_bounds__(256) void k_enc_estimate(EncEstimate P) {
#pragma clang fp contract(off)
  constexpr int kGroups = 256 / kLanes, kBuf = kLanes == 64 ? 512 : 4096, kWaves = kLanes / 64;
  constexpr int kBasisFirst = kLanes == 64 ? 0 : 341, kBasisFloats = kLanes == 64 ? 1365 : 1024;
  __shared__ __attribute__((aligned(16))) float s_buf[kGroups][3][kBuf];
  __shared__ __attribute__((aligned(16))) float s_basis[kBasisFloats];
  __shared__ float s_red[kGroups][3][kWaves], s_share[kGroups][3][3];
  const uint32_t tid = threadIdx.x, grp = tid / kLanes, lane = tid % kLanes;
  const uint32_t R = P.cy * 8, C = P.cx * 8, size = R * C, lc = 31u - uint32_t(__clz(int(C))), lr = 31u - uint32_t(__clz(int(R)));
  const uint32_t num_blocks = P.cx * P.cy, items = size / NB;
  for (int i = tid; i < kBasisFloats; i += 256) s_basis[i] = P.basis_t[kBasisFirst + i];
  const uint32_t slot = blockIdx.x * kGroups + grp;
  const bool live = slot < P.n;  // (a workgroup's last waves may have no candidate: they follow the last one and write nothing)
  const JxlHipEncAcsCandidate cand = P.cand[live ? slot : P.n - 1];
  const uint32_t x0 = cand.bx * 8, y0 = cand.by * 8;
  float* const a = s_buf[grp][0];
  float* const t = s_buf[grp][1];
  float* const yc = s_buf[grp][2];
  const float* bc = C == 64 ? P.basis_t + 1365 : s_basis + ((C * C - 1) / 3 - kBasisFirst);
  const float* br = R == 64 ? P.basis_t + 1365 : s_basis + ((R * R - 1) / 3 - kBasisFirst);
  // quant_norm16 (:384-414)
  const float* qf = P.quant + size_t(cand.by) * P.xb + cand.bx;
  float quant_norm16 = 0.0f;
  if (num_blocks == 1) {
    quant_norm16 = qf[0];
  } else if (num_blocks == 2) {
    quant_norm16 = fmaxf(qf[0], P.cy == 2 ? qf[P.xb] : qf[1]);
  } else {
    for (uint32_t iy = 0; iy < P.cy; iy++)
      for (uint32_t ix = 0; ix < P.cx; ix++) {
        float q = qf[iy * P.xb + ix];
        q *= q;
        q *= q;
        q *= q;
        quant_norm16 += q * q;
      }
    quant_norm16 /= float(num_blocks);
    quant_norm16 = powf(quant_norm16, 1.0f / 16.0f);
  }
  const uint32_t tile = (cand.by / 8) * P.tiles_x + cand.bx / 8;
  const float norm = 1.0f / (float(R) * float(C));
  const size_t plane = size_t(P.xp) * P.yp;
  __syncthreads();
  for (int ci = 0; ci < 3; ci++) {
    const int c = ci == 0 ? 1 : (ci == 1 ? 0 : 2);
    const float* src = P.planes + plane * c + size_t(y0) * P.xp + x0;
    for (uint32_t i = lane; i < size; i += kLanes) a[i] = src[size_t(i >> lc) * P.xp + (i & (C - 1))];
    __syncthreads();
    // forward rows: t[y][kx] = sum_x a[y][x] * B_C[x][kx]
    for (uint32_t w = lane; w < items; w += kLanes) {
      const uint32_t kx = w & (C - 1), r0 = (w >> lc) * NB;
      float acc[NB];
#pragma unroll
      for (int j = 0; j < NB; j++) acc[j] = 0.0f;
      for (uint32_t x = 0; x < C; x++) {
        const float b = bc[x * C + kx];
#pragma unroll
        for (int j = 0; j < NB; j++) acc[j] += a[(r0 + j) * C + x] * b;
      }
#pragma unroll
      for (int j = 0; j < NB; j++) t[(r0 + j) * C + kx] = acc[j];
    }
    __syncthreads();
    // forward columns: coef[ky][kx] = (sum_y t[y][kx] * B_R[y][ky]) * norm, natural layout; Y's stay in yc
    float* const coef = c == 1 ? yc : a;
    for (uint32_t w = lane; w < items; w += kLanes) {
      const uint32_t kx = w & (C - 1), k0 = (w >> lc) * NB;
      float acc[NB];
#pragma unroll
      for (int j = 0; j < NB; j++) acc[j] = 0.0f;
      for (uint32_t y = 0; y < R; y++) {
        const float v = t[y * C + kx];
#pragma unroll
        for (int j = 0; j < NB; j++) acc[j] += v * br[y * R + k0 + j];
      }
#pragma unroll
      for (int j = 0; j < NB; j++) coef[(k0 + j) * C + kx] = acc[j] * norm;
    }
    __syncthreads();
    // val, its rounding, the error times the weight (:428-444)
    const float factor = c == 0 ? 0.0f + float(P.ytox[tile]) / 84.0f : (c == 1 ? 0.0f : 1.0f + float(P.ytob[tile]) / 84.0f);
    const float* m = P.dequant + size_t(c) * size;
    float* const out = P.scaled && live ? P.scaled + P.scaled_at[slot] + size_t(c) * size : nullptr;
    float sum_sqrt = 0.0f, sum_nz = 0.0f, sum_loss = 0.0f;
    for (uint32_t k = lane; k < size; k += kLanes) {
      const uint32_t ky = k >> lc, kx = k & (C - 1);
      const float mk = m[R < C ? k : kx * R + ky];
      const float in_y = yc[k] * factor;
      const float val = (coef[k] - in_y) * ((1.0f / mk) * quant_norm16);
      const float r = rintf(val);
      if (out) out[k] = val;
      const float e = mk * (val - r);
      const float q = fabsf(r);
      sum_sqrt += sqrtf(q);
      sum_nz += q == 0.0f ? 0.0f : 1.0f;
      a[k] = e;  // (X's and B's coefficients are not needed again; Y's stay in yc)
    }
    __syncthreads();
    // inverse columns: u[y][kx] = sum_ky e[ky][kx] * B_R[y][ky], stored transposed: t[kx][y]
    for (uint32_t w = lane; w < items; w += kLanes) {
      const uint32_t kx = w & (C - 1), r0 = (w >> lc) * NB;
      float acc[NB];
#pragma unroll
      for (int j = 0; j < NB; j++) acc[j] = 0.0f;
      for (uint32_t ky = 0; ky < R; ky++) {
        const float v = a[ky * C + kx];
#pragma unroll
        for (int j = 0; j < NB; j++) acc[j] += v * br[(r0 + j) * R + ky];
      }
#pragma unroll
      for (int j = 0; j < NB; j++) t[kx * R + r0 + j] = acc[j];
    }
    __syncthreads();
    // inverse rows: p[y][x] = sum_kx u[y][kx] * B_C[x][kx]; the masked eighth power into a[y][x] (:457-479)
    const float mask_off = c == 0 ? 12.0f : (c == 1 ? 0.0f : 4.0f);
    const float* mask = P.mask + size_t(y0) * P.xp + x0;
    for (uint32_t w = lane; w < items; w += kLanes) {
      const uint32_t y = w & (R - 1), c0 = (w >> lr) * NB;
      float acc[NB];
#pragma unroll
      for (int j = 0; j < NB; j++) acc[j] = 0.0f;
      for (uint32_t kx = 0; kx < C; kx++) {
        const float v = t[kx * R + y];
#pragma unroll
        for (int j = 0; j < NB; j++) acc[j] += v * bc[(c0 + j) * C + kx];
      }
#pragma unroll
      for (int j = 0; j < NB; j++) {
        float v = (mask[size_t(y) * P.xp + c0 + j] + mask_off) * acc[j];
        v = v * v;
        v = v * v;
        v = v * v;
        a[y * C + c0 + j] = v;
      }
    }
    __syncthreads();
    for (uint32_t k = lane; k < size; k += kLanes) sum_loss += a[k];
    // the three sums of the group: within a wave, then across the waves
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      sum_sqrt = sum_sqrt + __shfl_xor(sum_sqrt, d, 64);
      sum_nz = sum_nz + __shfl_xor(sum_nz, d, 64);
      sum_loss = sum_loss + __shfl_xor(sum_loss, d, 64);
    }
    if (kWaves > 1) {
      if ((lane & 63) == 0) {
        s_red[grp][0][lane >> 6] = sum_sqrt;
        s_red[grp][1][lane >> 6] = sum_nz;
        s_red[grp][2][lane >> 6] = sum_loss;
      }
      __syncthreads();
      if (lane == 0) {
        sum_sqrt = (s_red[grp][0][0] + s_red[grp][0][1 % kWaves]) + (s_red[grp][0][2 % kWaves] + s_red[grp][0][3 % kWaves]);
        sum_nz = (s_red[grp][1][0] + s_red[grp][1][1 % kWaves]) + (s_red[grp][1][2 % kWaves] + s_red[grp][1][3 % kWaves]);
        sum_loss = (s_red[grp][2][0] + s_red[grp][2][1 % kWaves]) + (s_red[grp][2][2 % kWaves] + s_red[grp][2][3 % kWaves]);
      }
    }
    if (lane == 0) {
      s_share[grp][c][0] = sum_sqrt;
      s_share[grp][c][1] = sum_nz;
      s_share[grp][c][2] = sum_loss;
    }
    __syncthreads();  // (a, t and s_red are written again by the next channel)
  }
  if (lane == 0 && live) {
    // :488-509, in the reference's channel order
    float entropy = 0.0f, loss = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      entropy += P.weights[2] * s_share[grp][c][0];
      const uint32_t num_nzeros = uint32_t(s_share[grp][c][1]);
      const uint32_t nbits = EncCeilLog2Nonzero(num_nzeros + 1) + 1;
      entropy += P.weights[1] * float(EncCeilLog2Nonzero(nbits + 17) + nbits);
      loss += P.channel_mul[c] * s_share[grp][c][2];
      if (c == 0 && num_blocks >= 2) {
        entropy *= P.x_weight;
        loss *= P.x_weight;
      }
    }
    const float loss_scalar = powf(loss / float(size), 1.0f / 8.0f) * float(size) / quant_norm16;
    entropy *= cand.entropy_mul;
    entropy += P.weights[0] * loss_scalar;
    P.estimates[P.index[slot]] = entropy;
  }
}

// The merge walk of the reference's AC-strategy search (ProcessRectACS, enc_ac_strategy.cc:827-1059) over one 64x64 tile per
// wave, on a table that holds every estimate the walk can ask for (k_enc_estimate wrote it through the candidate list's
// index array, or a caller brought it: jxlhip_enc_acs_walk). The float32 statement is jxh::AcsWalkTile of
// csrc/host/jxh_enc_shared.h, the text the CPU double compiles, with contraction off in every function that adds. The tile's
// table (2 560 B), entropy_estimate[64], the strategy image and priority[64] are in LDS. The walk is serial by construction
// from the first floating square on (each reads what the one before wrote), and the aligned squares of one level, which
// are independent, are a small part of it: lane 0 walks, the wave's other lanes load the table before and write the results
// after. In the forward path (qf != NULL) every lane then aggregates the adaptive quant field over the transform its block
// starts, the arithmetic of k_enc_select<true>'s tail: AdjustQuantField and SetQuantFieldRect.
struct EncAcsWalk {
  const float* table;   // [tiles][10][8][8]
  uint8_t* acs;         // [yb][xb] (strategy << 1) | first
  float* entropy;       // [yb][xb] the walk's final entropy_estimate, or NULL
  int32_t* qf;          // [yb][xb] quant field at first blocks, or NULL
  const float* aq_map;  // [yb][xb], read with qf
  uint32_t xb, yb, floating;
  float mul8x8, mean_max_mixer, inv_gs;
};
__global__ __launch_bounds__(64) void k_enc_acs_walk(EncAcsWalk P) {
#pragma clang fp contract(off)
  __shared__ float s_est[jxh::kAcsWalkTileFloats];
  __shared__ float s_entropy[64], s_aq[64];
  __shared__ uint8_t s_acs[64], s_priority[64];
  const uint32_t tiles_x = (P.xb + 7) / 8;
  const uint32_t t = blockIdx.x, lane = threadIdx.x, x = lane & 7, y = lane >> 3;
  const uint32_t bx0 = (t % tiles_x) * 8, by0 = (t / tiles_x) * 8;
  const uint32_t w = min(8u, P.xb - bx0), h = min(8u, P.yb - by0);
  const bool inside = x < w && y < h;
  const size_t bi = size_t(by0 + y) * P.xb + bx0 + x;
  for (uint32_t i = lane; i < jxh::kAcsWalkTileFloats; i += 64) s_est[i] = P.table[size_t(t) * jxh::kAcsWalkTileFloats + i];
  s_aq[lane] = P.qf && inside ? P.aq_map[bi] : 0.0f;
  __syncthreads();
  if (lane == 0) {
    const jxh::AcsWalkState s = {s_est, s_entropy, s_acs, s_priority, w, h};
    jxh::AcsWalkTile(s, P.mul8x8, P.floating);
  }
  __syncthreads();
  if (!inside) return;
  const uint32_t a = s_acs[lane], kind = a >> 1;
  P.acs[bi] = uint8_t((jxh::AcsWalkStrategy(kind) << 1) | (a & 1));
  if (P.entropy) P.entropy[bi] = s_entropy[lane];
  if (!P.qf) return;
  int32_t q = 0;
  if (a & 1) {
    // the covered blocks in raster order: the largest, and the mean mixed in from four blocks on
    const uint32_t cx = 1u << jxh::AcsWalkLog2X(kind), cy = 1u << jxh::AcsWalkLog2Y(kind);
    float mx = s_aq[lane], mean = 0.0f;
    for (uint32_t yy = 0; yy < cy; yy++)
      for (uint32_t xx = 0; xx < cx; xx++) {
        const float v = s_aq[(y + yy) * 8 + x + xx];
        mean += v;
        mx = fmaxf(v, mx);
      }
    mean /= float(cy * cx);
    if (cy * cx >= 4) {
      mx *= P.mean_max_mixer;
      mx += (1.0f - P.mean_max_mixer) * mean;
    }
    q = int(fmaxf(1.0f, fminf(mx * P.inv_gs + 0.5f, 256.0f)));
  }
  P.qf[bi] = q;
}

// ---------------------------------------------------------------------------------------------- tokenisation
// The AC coefficient tokens of a frame on the device (reference lib/jxl/enc_entropy_coder.cc:153-255 TokenizeCoefficients;
// contexts lib/jxl/ac_context.h:63-143, entropy_coder.h:25-35): the quantised coefficients of the forward path never leave
// HBM, the host entropy coder receives (context, value) pairs in bitstream order. Unlike the decoder's walk nothing here
// is serial: a (varblock, channel)'s non-zero count is a popcount, the predicted count comes from the finished map of
// counts, the running "non-zeros left" of coefficient k is the count minus a prefix popcount, and a token's place in its
// group's stream is a prefix sum of the per-(varblock, channel) token counts.
// Two launches, one workgroup of sixteen waves per 256x256 group, a wave per (varblock, channel):
//   k_enc_tok_count  list of the group's varblocks in raster order, per (varblock, channel) the non-zero count and the last
//                    non-zero scan position, the map of counts per 8x8 block, token counts and their exclusive scan
//   k_enc_tok_emit   the tokens, at the group's base (a host-side prefix sum of the 135 group totals) + that offset
// Single pass, natural coefficient order, a block context map without thresholds (the default one): what the forward path's
// callers use; anything else is tokenised by the host as before.
struct EncTok {
  const uint8_t* acs;        // per block: strategy << 1 | first (k_enc_select)
  const uint32_t* coef_off;  // per first block: offset of its coefficients in the group's planes (k_enc_offsets)
  const int32_t* coeffs;     // [group][3][65536]
  uint32_t xb, yb, xg;
  const uint16_t* orders;    // natural coefficient orders of the 13 order buckets, concatenated
  uint32_t order_offset[13];
  uint8_t ctx_map[39];       // block context of (channel in stream order Y, X, B -> c < 2 ? c ^ 1 : 2; order bucket)
  uint32_t num_ctxs, num_hist, nctx;
  // per group (kTokPerGroup = 3072 entries: 1024 varblocks x 3 channels)
  uint16_t* blk;             // [group][1024] raster positions of the first blocks
  uint32_t* nblk;            // [group]
  uint32_t* info;            // [group][3072]: non-zero count | (last non-zero scan position + 1) << 16
  uint32_t* off;             // [group][3072]: first token of the (varblock, channel) in its group's stream
  uint8_t* nzmap;            // [group][3][1024]: ceil(count / covered blocks) per 8x8 block (the decoder's nzeros map)
  uint32_t* total;           // [group]
  const uint32_t* base;      // [group] (emit): first token of the group in `tokens`
  uint2* tokens;             // (emit) {context, value}
};
constexpr uint32_t kTokPerGroup = 3072;

constexpr uint32_t kTokThreads = 1024, kTokWaves = kTokThreads / 64;  // sixteen waves per group: the walk is latency-bound

__global__ __launch_bounds__(kTokThreads) void k_enc_tok_count(EncTok P) {
  __shared__ uint16_t l_blk[1024];
  __shared__ uint32_t l_cnt[kTokPerGroup];
  __shared__ uint32_t l_scan[256];
  const uint32_t g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool scanner = tid < 256;  // the two scans are the first four waves' work
  const uint32_t bx0 = (g % P.xg) * 32, by0 = (g / P.xg) * 32;
  const uint32_t gw = min(32u, P.xb - bx0), gh = min(32u, P.yb - by0), n = gw * gh;
  // ---- the group's first blocks in raster order: four consecutive raster positions per thread, exclusive scan
  uint32_t first[4] = {0, 0, 0, 0}, cnt = 0;
  if (scanner) {
    for (uint32_t j = 0; j < 4; j++) {
      const uint32_t i = tid * 4 + j;
      first[j] = (i < n && (P.acs[size_t(by0 + i / gw) * P.xb + bx0 + i % gw] & 1)) ? 1u : 0u;
      cnt += first[j];
    }
    l_scan[tid] = cnt;
  }
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint32_t v = (scanner && tid >= d) ? l_scan[tid - d] : 0u;
    __syncthreads();
    if (scanner) l_scan[tid] += v;
    __syncthreads();
  }
  const uint32_t nblk = l_scan[255];
  if (scanner) {
    uint32_t idx = l_scan[tid] - cnt;
    for (uint32_t j = 0; j < 4; j++)
      if (first[j]) {
        l_blk[idx] = uint16_t(tid * 4 + j);
        P.blk[size_t(g) * 1024 + idx] = uint16_t(tid * 4 + j);
        idx++;
      }
  }
  if (tid == 0) P.nblk[g] = nblk;
  __syncthreads();
  // ---- a wave per (varblock, channel): non-zero count beyond the lowest-frequency corner, last non-zero scan position
  for (uint32_t e = wave; e < nblk * 3; e += kTokWaves) {
    const uint32_t b = e / 3, ci = e % 3, c = ci == 0 ? 1u : (ci == 1 ? 0u : 2u);
    const uint32_t i = l_blk[b], lbx = i % gw, lby = i / gw;
    const size_t cell = size_t(by0 + lby) * P.xb + bx0 + lbx;
    const uint32_t st = P.acs[cell] >> 1, log2c = c_log2_covered[st], covered = 1u << log2c, size = covered * 64;
    const uint16_t* order = P.orders + P.order_offset[c_strategy_order[st]];
    const int32_t* co = P.coeffs + (size_t(g) * 3 + c) * 65536 + P.coef_off[cell];
    uint32_t nz = 0, last = 0;
    for (uint32_t k0 = 0; k0 < size; k0 += 64) {
      const uint32_t k = k0 + lane;
      const bool f = k >= covered && co[order[k]] != 0;
      const unsigned long long m = __ballot(f);
      nz += uint32_t(__popcll(m));
      if (m) last = k0 + 64 - uint32_t(__clzll(m));  // last non-zero scan position + 1
    }
    if (lane == 0) {
      P.info[size_t(g) * kTokPerGroup + e] = nz | last << 16;
      l_cnt[e] = 1 + (nz ? last - covered : 0u);
    }
    const uint32_t cx = c_covered_x[st], cy = c_covered_y[st];
    if (lane < cx * cy) P.nzmap[(size_t(g) * 3 + c) * 1024 + (lby + lane / cx) * 32 + lbx + lane % cx] = uint8_t((nz + covered - 1) >> log2c);
  }
  __syncthreads();
  // ---- exclusive scan of the token counts in stream order (twelve per thread)
  const uint32_t ne = nblk * 3;
  uint32_t sum = 0;
  if (scanner) {
    for (uint32_t j = 0; j < 12; j++) {
      const uint32_t e = tid * 12 + j;
      sum += e < ne ? l_cnt[e] : 0u;
    }
    l_scan[tid] = sum;
  }
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint32_t v = (scanner && tid >= d) ? l_scan[tid - d] : 0u;
    __syncthreads();
    if (scanner) l_scan[tid] += v;
    __syncthreads();
  }
  if (scanner) {
    uint32_t o = l_scan[tid] - sum;
    for (uint32_t j = 0; j < 12; j++) {
      const uint32_t e = tid * 12 + j;
      if (e < ne) {
        P.off[size_t(g) * kTokPerGroup + e] = o;
        o += l_cnt[e];
      }
    }
  }
  if (tid == 255) P.total[g] = l_scan[255];
}

__global__ __launch_bounds__(kTokThreads) void k_enc_tok_emit(EncTok P) {
  const uint32_t g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t bx0 = (g % P.xg) * 32, by0 = (g / P.xg) * 32;
  const uint32_t gw = min(32u, P.xb - bx0);
  const uint32_t nblk = P.nblk[g];
  const uint32_t hist_off = (g % P.num_hist) * P.nctx;
  uint2* const out = P.tokens + P.base[g];
  for (uint32_t e = wave; e < nblk * 3; e += kTokWaves) {
    const uint32_t b = e / 3, ci = e % 3, c = ci == 0 ? 1u : (ci == 1 ? 0u : 2u);
    const uint32_t i = P.blk[size_t(g) * 1024 + b], lbx = i % gw, lby = i / gw;
    const size_t cell = size_t(by0 + lby) * P.xb + bx0 + lbx;
    const uint32_t st = P.acs[cell] >> 1, log2c = c_log2_covered[st], covered = 1u << log2c, size = covered * 64;
    const uint32_t ord = c_strategy_order[st];
    const uint16_t* order = P.orders + P.order_offset[ord];
    const int32_t* co = P.coeffs + (size_t(g) * 3 + c) * 65536 + P.coef_off[cell];
    const uint32_t inf = P.info[size_t(g) * kTokPerGroup + e], nz = inf & 0xFFFFu, last = inf >> 16;
    const uint32_t o = P.off[size_t(g) * kTokPerGroup + e];
    const uint32_t bc = P.ctx_map[(c < 2 ? c ^ 1 : 2) * 13 + ord];
    if (lane == 0) {
      // entropy_coder.h:25-35 PredictFromTopAndLeft over the map of counts (every cell read here belongs to a varblock
      // that comes earlier in raster order), ac_context.h:131-143 NonZeroContext
      const uint8_t* m = P.nzmap + (size_t(g) * 3 + c) * 1024;
      const uint32_t pred = PredictNonZeros([m](uint32_t i) { return uint32_t(m[i]); }, lbx, lby);
      out[o] = make_uint2(hist_off + NonZeroBucket(pred) * P.num_ctxs + bc, nz);
    }
    if (!nz) continue;
    // ac_context.h:63-83 ZeroDensityContext for scan positions covered .. last - 1: non-zeros left = count - non-zeros before k
    const uint32_t hoff = hist_off + ZeroDensityBase(P.num_ctxs, bc);
    uint32_t before = 0;                            // non-zeros at scan positions [covered, k0)
    uint32_t carry = nz > size / 16 ? 0u : 1u;      // "previous coefficient was non-zero" for the chunk's first lane
    for (uint32_t k0 = covered & ~63u; k0 < last; k0 += 64) {
      const uint32_t k = k0 + lane;
      const bool in = k >= covered && k < last;
      const int32_t v = in ? co[order[k]] : 0;
      const unsigned long long mz = __ballot(in && v != 0);
      if (in) {
        const uint32_t left = nz - before - uint32_t(__popcll(mz & ((1ull << lane) - 1)));
        const uint32_t prev = (lane == 0 || k == covered) ? carry : uint32_t((mz >> (lane - 1)) & 1);
        const uint32_t nzl = (left + covered - 1) >> log2c;
        const uint32_t ctx = ZeroDensityContext(hoff, c_coeff_nnz_ctx[nzl & 63], c_coeff_freq_ctx[(k >> log2c) & 63], prev);
        const uint32_t val = v >= 0 ? uint32_t(v) * 2 : uint32_t(-(v + 1)) * 2 + 1;
        out[o + 1 + (k - covered)] = make_uint2(ctx, val);
      }
      before += uint32_t(__popcll(mz));
      carry = uint32_t((mz >> 63) & 1);
    }
  }
}

// ---------------------------------------------------------------- entropy coding of the tokens
// What the host coder does behind the tokens (csrc/enc/jxl_enc.cc CountSymbols and WriteTokens), on the tokens where they
// are: symbol counts per context go up, the host clusters and normalises them and sends the code's tables down, and every
// group's coded bit string goes up. The tokens themselves never leave the device.
//   k_enc_hist         per token: its hybrid-uint symbol, counted in counts[context][symbol] (integer sums: any order)
//   k_enc_ans_records  per token: the frequency of its symbol in its context's cluster and where the symbol's slots start
//                      in the cluster's reverse map, as one word; the number of extra bits
//   k_enc_ans_chain    per group, one wave: the coder state, backwards from the final state 0x13 << 16 (a token's state
//                      depends on the state behind it: this is the serial part). Per token whether it flushed 16 bits, and
//                      which; per group the state the stream starts with and the exact length in bits
//   k_enc_ans_scatter  per group, one workgroup: prefix sum of the bit lengths, every token's chunk and extra bits OR-ed
//                      into the words of the (zeroed) output it falls into
// Every index formed from a table is bounded by the checks jxlhip_enc_ans_sizes makes on the tables; a token the code cannot
// code (context out of range, symbol beyond the alphabet or without frequency) is coded as a symbol of frequency 1 at slot
// 0 - in bounds - and raises its group's error flag, which fails the call.
struct EncAns {
  const uint2* tokens;         // {context, value}; group g at tokens[base[g] .. base[g] + count[g])
  const uint32_t* base;        // [groups]
  const uint32_t* count;       // [groups]
  uint32_t split_exp, msb, lsb, num_ctx;
  uint32_t* counts;            // (hist) [num_ctx][256]
  uint32_t* status;            // (hist) [0] largest symbol, [1] non-zero: a token outside the table
  const uint8_t* ctx_map;      // [num_ctx], entries < clusters
  const uint16_t* freq;        // [clusters][256]
  const uint16_t* rev_start;   // [clusters][256]; rev_start + freq <= 4096
  const uint16_t* rev;         // [clusters][4096], entries < 4096
  const uint8_t* prefix_count; // [groups], <= 8
  const uint8_t* prefix_value; // [groups]
  uint32_t* rec;               // per token: frequency - 1 | (cluster * 4096 + rev_start) << 12
  uint32_t* fl;                // per token: chunk | flushed << 16 | extra bits << 17
  uint32_t* state;             // [groups] the state the stream starts with
  uint32_t* bits;              // [groups] length of the bit string
  uint32_t* err;               // [groups]
  const uint64_t* out_base;    // (scatter) [groups] first byte in out
  uint32_t* out;               // (scatter) words, zeroed
};
constexpr uint32_t kAnsThreads = 256, kAnsBlocksPerGroup = 8;

// (jxl_enc.cc HybridEncode; split_exp >= msb + lsb, so n - msb >= 0 for every value that gets here)
__device__ __forceinline__ void EncHybrid(uint32_t v, uint32_t split_exp, uint32_t msb, uint32_t lsb, uint32_t& tok, uint32_t& nbits, uint32_t& bits) {
  if (v < (1u << split_exp)) {
    tok = v;
    nbits = 0;
    bits = 0;
    return;
  }
  const uint32_t n = 31u - uint32_t(__clz(int(v))), m = v - (1u << n);
  tok = (1u << split_exp) + ((n - split_exp) << (msb + lsb)) + ((m >> (n - msb)) << lsb) + (m & ((1u << lsb) - 1u));
  nbits = n - msb - lsb;
  bits = (v >> lsb) & ((1u << nbits) - 1u);
}

__global__ __launch_bounds__(kAnsThreads) void k_enc_hist(EncAns P) {
  const uint32_t g = blockIdx.y, n = P.count[g];
  const uint2* tk = P.tokens + P.base[g];
  uint32_t mx = 0, bad = 0;
  for (uint32_t i = blockIdx.x * kAnsThreads + threadIdx.x; i < n; i += gridDim.x * kAnsThreads) {
    const uint2 t = tk[i];
    uint32_t tok, nb, bits;
    EncHybrid(t.y, P.split_exp, P.msb, P.lsb, tok, nb, bits);
    mx = max(mx, tok);
    if (t.x >= P.num_ctx || tok >= 256u) bad = 1;
    else atomicAdd(&P.counts[size_t(t.x) * 256 + tok], 1u);
  }
  for (int o = 32; o; o >>= 1) {
    mx = max(mx, uint32_t(__shfl_xor(int(mx), o)));
    bad |= uint32_t(__shfl_xor(int(bad), o));
  }
  if ((threadIdx.x & 63) == 0) {
    if (mx) atomicMax(&P.status[0], mx);
    if (bad) atomicOr(&P.status[1], 1u);
  }
}

__global__ __launch_bounds__(kAnsThreads) void k_enc_ans_records(EncAns P) {
  const uint32_t g = blockIdx.y, n = P.count[g], base = P.base[g];
  uint32_t bad = 0;
  for (uint32_t i = blockIdx.x * kAnsThreads + threadIdx.x; i < n; i += gridDim.x * kAnsThreads) {
    const uint2 t = P.tokens[base + i];
    uint32_t tok, nb, bits, rec = 0;
    EncHybrid(t.y, P.split_exp, P.msb, P.lsb, tok, nb, bits);
    if (t.x >= P.num_ctx || tok >= 256u) {
      bad |= 1;
    } else {
      const uint32_t k = P.ctx_map[t.x], f = P.freq[k * 256 + tok];
      if (!f) bad |= 2;
      else rec = (f - 1u) | (k * 4096u + P.rev_start[k * 256 + tok]) << 12;
    }
    P.rec[base + i] = rec;
    P.fl[base + i] = nb << 17;
  }
  if (bad) atomicOr(&P.err[g], bad);
}

// The state chain of one group on one wave. The wave loads 64 records at a time, coalesced, and every lane turns its own
// record's frequency into a double reciprocal; the 64 steps then run on wave-uniform values (a record comes out of its lane
// by v_readlane): state / freq as trunc(state * (1 / freq)) with one correction step - the product is within 2^-20 of the
// quotient, a non-integer quotient is at least 2^-12 from the next integer, so only an exact multiple can come out one low,
// and the remainder test catches it. The only load that depends on the state is rev[...].
__global__ __launch_bounds__(64) void k_enc_ans_chain(EncAns P) {
  const uint32_t g = blockIdx.x, lane = threadIdx.x, n = P.count[g], base = P.base[g];
  const uint16_t* __restrict__ rev = P.rev;
  uint32_t state = 0x13u << 16, total = 0;
  for (uint32_t t0 = ((n + 63u) & ~63u); t0 >= 64u;) {
    t0 -= 64u;
    const uint32_t i = t0 + lane;
    const bool in = i < n;
    const uint32_t rec = in ? P.rec[base + i] : 0u;
    uint32_t f = in ? P.fl[base + i] : 0u;
    const double rcp = 1.0 / double((rec & 0xFFFu) + 1u);
    const int rcp_lo = __double2loint(rcp), rcp_hi = __double2hiint(rcp);
    uint32_t mine = 0;
    for (int j = int(min(64u, n - t0)) - 1; j >= 0; j--) {
      const uint32_t r = uint32_t(__builtin_amdgcn_readlane(int(rec), j));
      const double rc = __hiloint2double(__builtin_amdgcn_readlane(rcp_hi, j), __builtin_amdgcn_readlane(rcp_lo, j));
      const uint32_t freq = (r & 0xFFFu) + 1u;
      const bool flush = (state >> 20) >= freq;
      const uint32_t chunk = state & 0xFFFFu;
      if (flush) state >>= 16;
      uint32_t q = uint32_t(double(state) * rc), rem = state - q * freq;
      if (rem >= freq) {
        q++;
        rem -= freq;
      }
      state = (q << 12) + rev[(r >> 12) + rem];
      if (int(lane) == j) mine = chunk | (flush ? 0x10000u : 0u);
    }
    if (in) {
      f |= mine;
      P.fl[base + i] = f;
      total += (f >> 17) + ((f >> 16) & 1u) * 16u;
    }
  }
  for (int o = 32; o; o >>= 1) total += uint32_t(__shfl_xor(int(total), o));
  if (lane == 0) {
    P.state[g] = state;
    P.bits[g] = uint32_t(P.prefix_count[g]) + 32u + total;
  }
}

// `len` (<= 47) bits of v at absolute bit position `pos` of the zeroed word array
__device__ __forceinline__ void AnsPut(uint32_t* out, uint64_t pos, uint64_t v, uint32_t len) {
  if (!len) return;
  const uint64_t w = pos >> 5;
  const uint32_t sh = uint32_t(pos & 31);
  const uint64_t lo = v << sh;
  const uint32_t w0 = uint32_t(lo), w1 = uint32_t(lo >> 32), w2 = sh ? uint32_t(v >> (64 - sh)) : 0u;
  if (w0) atomicOr(&out[w], w0);
  if (w1) atomicOr(&out[w + 1], w1);
  if (w2) atomicOr(&out[w + 2], w2);
}

__global__ __launch_bounds__(kAnsThreads) void k_enc_ans_scatter(EncAns P) {
  __shared__ uint32_t l_wave[kAnsThreads / 64];
  const uint32_t g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = P.count[g], base = P.base[g];
  if (P.err[g]) return;  // (uniform) nothing is written for a group the code cannot code
  const uint64_t bit0 = P.out_base[g] * 8;
  const uint32_t pc = P.prefix_count[g];
  if (tid == 0) {
    AnsPut(P.out, bit0, uint64_t(P.prefix_value[g]) & ((1u << pc) - 1u), pc);
    AnsPut(P.out, bit0 + pc, P.state[g], 32);
  }
  uint64_t running = pc + 32u;
  for (uint32_t t0 = 0; t0 < n; t0 += kAnsThreads) {
    const uint32_t i = t0 + tid;
    const bool in = i < n;
    const uint32_t f = in ? P.fl[base + i] : 0u;
    const uint32_t nb = (f >> 17) & 31u, flushed = (f >> 16) & 1u, len = nb + 16u * flushed;
    uint32_t incl = len;  // inclusive scan over the wave, then over the workgroup's four waves
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = uint32_t(__shfl_up(int(incl), o));
      if (int(lane) >= o) incl += v;
    }
    __syncthreads();  // (l_wave of the round before has been read)
    if (lane == 63) l_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < kAnsThreads / 64; w++) {
      if (w < wave) before += l_wave[w];
      all += l_wave[w];
    }
    if (len) {
      const uint32_t value = P.tokens[base + i].y;
      const uint64_t extra = (value >> P.lsb) & ((1u << nb) - 1u);
      const uint64_t v = flushed ? (uint64_t(f & 0xFFFFu) | extra << 16) : extra;
      AnsPut(P.out, bit0 + running + before + incl - len, v, len);
    }
    running += all;
  }
}

}  // namespace jxlhip
#endif  // JXL_HIP_ENC_H_
