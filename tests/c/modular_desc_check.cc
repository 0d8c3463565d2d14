// Whether jxlhip_modular_upload would take a descriptor, asked without a device: the host-only rules of
// libjxl_amd/csrc/host/jxh_modular_upload_plan.h as a shared library for tests/test_modular_np.py, which hands in the
// hand-made descriptors of tests/modular_desc.py before tests/test_gpu_modular_np.py sends them to a GPU.
// Returns 0, or 1000 + the rule that refused.
#include "../../libjxl_amd/csrc/host/jxh_modular_upload_plan.h"

extern "C" int modular_desc_check(const JxlHipModFrameDesc* d) {
  jxlhip::upload::ModUploadOptions opt;
  jxlhip::upload::ModRule rule = jxlhip::upload::kNumModRules;
  return jxlhip::upload::CheckModFrameDesc(*d, opt, &rule) ? 1000 + int(rule) : 0;
}
