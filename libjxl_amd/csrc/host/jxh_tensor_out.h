// libjxl_amd — whether a JxlHipTensorOut (jxlhip_set_output_tensor) is taken: a pure function of the descriptor and the
// size of the output image, free of HIP, so that tests/c/tensor_out_kats.cc holds every rule on the CPU. The HIP layer
// calls it when the tensor is bound (extents 1 x 1: what can be said without an image) and again at upload.
#ifndef JXH_TENSOR_OUT_H_
#define JXH_TENSOR_OUT_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/jxl_amd_hip.h"

namespace jxlhip {
namespace tensor_out {

// Every reason to refuse a descriptor, each stated once in CheckTensorOut. tests/c/tensor_out_kats.cc breaks each rule in
// turn; tests/test_tensor_out_host.py fails when a rule here has no row there.
enum TensorRule : int {
  kTensorRuleData,             // a device pointer
  kTensorRuleDtype,            // one of JXLHIP_TENSOR_*
  kTensorRuleChannels,         // 1..4
  kTensorRuleAlignment,        // data aligned to the element size
  kTensorRuleStridesPositive,  // every stride > 0
  kTensorRuleFinite,           // scale and bias finite (float types)
  kTensorRuleU8Identity,       // JXLHIP_TENSOR_U8: scale 1, bias 0, no clamp
  kTensorRuleInjective,        // sorted by stride, each stride >= the previous stride times its extent
  kTensorRuleBytes,            // (largest offset + 1) * element size <= bytes
  kTensorRuleCount
};

// Bytes of one element; 0 for a dtype that does not exist.
inline size_t ElemBytes(uint32_t dtype) {
  switch (dtype) {
    case JXLHIP_TENSOR_F32: return 4;
    case JXLHIP_TENSOR_U8: return 1;
    case JXLHIP_TENSOR_F16:
    case JXLHIP_TENSOR_BF16: return 2;
    default: return 0;
  }
}
inline bool IsFloatType(uint32_t dtype) { return dtype == JXLHIP_TENSOR_F32 || dtype == JXLHIP_TENSOR_F16 || dtype == JXLHIP_TENSOR_BF16; }

// The largest element offset the map reaches over an image of xsize x ysize (both > 0, strides > 0, channels 1..4);
// false when it does not fit 64 bits.
inline bool MaxOffset(const JxlHipTensorOut& t, uint32_t xsize, uint32_t ysize, uint64_t* max_offset) {
  const uint64_t stride[3] = {uint64_t(t.stride_c), uint64_t(t.stride_y), uint64_t(t.stride_x)};
  const uint64_t last[3] = {uint64_t(t.num_channels) - 1, uint64_t(ysize) - 1, uint64_t(xsize) - 1};
  uint64_t sum = 0;
  for (int i = 0; i < 3; i++) {
    uint64_t term;
    if (__builtin_mul_overflow(stride[i], last[i], &term) || __builtin_add_overflow(sum, term, &sum)) return false;
  }
  *max_offset = sum;
  return true;
}

// 0 when the descriptor is taken for an output image of xsize x ysize (after orientation), else JXLHIP_ERR_INVALID_ARGUMENT
// with the rule that refused it in *rule (may be NULL).
inline int CheckTensorOut(const JxlHipTensorOut& t, uint32_t xsize, uint32_t ysize, int* rule = nullptr) {
#define JXH_TENSOR_REFUSE(cond, r)          \
  do {                                      \
    if (cond) {                             \
      if (rule) *rule = (r);                \
      return JXLHIP_ERR_INVALID_ARGUMENT;   \
    }                                       \
  } while (0)
  JXH_TENSOR_REFUSE(!t.data || !xsize || !ysize, kTensorRuleData);
  const size_t elem = ElemBytes(t.dtype);
  JXH_TENSOR_REFUSE(!elem, kTensorRuleDtype);
  JXH_TENSOR_REFUSE(t.num_channels < 1 || t.num_channels > 4, kTensorRuleChannels);
  JXH_TENSOR_REFUSE(uintptr_t(t.data) % elem != 0, kTensorRuleAlignment);
  JXH_TENSOR_REFUSE(t.stride_c <= 0 || t.stride_y <= 0 || t.stride_x <= 0, kTensorRuleStridesPositive);
  if (IsFloatType(t.dtype)) {
    for (uint32_t c = 0; c < t.num_channels; c++) JXH_TENSOR_REFUSE(!isfinite(t.scale[c]) || !isfinite(t.bias[c]), kTensorRuleFinite);
  } else {
    for (uint32_t c = 0; c < t.num_channels; c++) JXH_TENSOR_REFUSE(t.scale[c] != 1.0f || t.bias[c] != 0.0f, kTensorRuleU8Identity);
    JXH_TENSOR_REFUSE(t.clamp01 != 0, kTensorRuleU8Identity);
  }
  // no two elements share an address: the dimensions that have more than one index, sorted by stride, nest
  uint64_t stride[3] = {uint64_t(t.stride_c), uint64_t(t.stride_y), uint64_t(t.stride_x)};
  uint64_t extent[3] = {t.num_channels, ysize, xsize};
  for (int i = 1; i < 3; i++)
    for (int j = i; j > 0 && (stride[j] < stride[j - 1] || (stride[j] == stride[j - 1] && extent[j] < extent[j - 1])); j--) {
      const uint64_t s = stride[j], e = extent[j];
      stride[j] = stride[j - 1];
      extent[j] = extent[j - 1];
      stride[j - 1] = s;
      extent[j - 1] = e;
    }
  uint64_t need = 1;  // (the stride the next dimension that counts has to reach)
  for (int i = 0; i < 3; i++) {
    if (extent[i] == 1) continue;  // (its one index is 0: the stride addresses nothing)
    JXH_TENSOR_REFUSE(stride[i] < need, kTensorRuleInjective);
    // (past 2^64 nothing larger can follow: the last dimension's own reach is the byte rule's to refuse)
    if (__builtin_mul_overflow(stride[i], extent[i], &need)) need = UINT64_MAX;
  }
  uint64_t max_offset = 0, count = 0, need_bytes = 0;
  JXH_TENSOR_REFUSE(!MaxOffset(t, xsize, ysize, &max_offset), kTensorRuleBytes);
  JXH_TENSOR_REFUSE(__builtin_add_overflow(max_offset, uint64_t(1), &count) || __builtin_mul_overflow(count, uint64_t(elem), &need_bytes),
                    kTensorRuleBytes);
  JXH_TENSOR_REFUSE(need_bytes > uint64_t(t.bytes), kTensorRuleBytes);
#undef JXH_TENSOR_REFUSE
  return 0;
}

}  // namespace tensor_out
}  // namespace jxlhip
#endif  // JXH_TENSOR_OUT_H_
