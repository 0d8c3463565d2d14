// libjxl_amd — how far the loop filters reach: the one statement of it, for the filter kernels (jxl_hip_filter_fused.h),
// the band exchange (jxlhip_halo_rows) and the host plan of a window (jxh_window_plan.h). Free of HIP: host code that is
// compiled without it includes this file alone.
#ifndef JXH_FILTER_HALO_H_
#define JXH_FILTER_HALO_H_

#if defined(__HIPCC__)
#define JXH_HOST_DEVICE __host__ __device__
#else
#define JXH_HOST_DEVICE
#endif

namespace jxlhip {

// Pixels of its neighbourhood a filtered pixel reads on every side: Gaborish 1, the EPF passes 3 (pass 0, epf_iters 3),
// 2 (pass 1, always) and 1 (pass 2, epf_iters >= 2). 0 to 7.
JXH_HOST_DEVICE constexpr int FusedHalo(bool gab, int epf) {
  return (gab ? 1 : 0) + (epf >= 3 ? 3 : 0) + (epf >= 1 ? 2 : 0) + (epf >= 2 ? 1 : 0);
}

}  // namespace jxlhip
#endif  // JXH_FILTER_HALO_H_
