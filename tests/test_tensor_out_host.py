"""Tensor output (jxlhip_set_output_tensor) on the CPU: the descriptor check of libjxl_amd/csrc/host/jxh_tensor_out.h under
AddressSanitizer + UBSan (tests/c/tensor_out_kats.cc, a stand-alone program), the pixel route decision, and what the Python
layer hands to the C ABI. Nothing here touches a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tensor_descriptor_check_under_sanitizers(tmp_path):
    """Every rule of jxh_tensor_out.h refuses the one change that breaks it; the layouts callers use are taken; strides near
    2^62 and a room one element short are refused without overflow; the largest offset equals a brute-force maximum. The
    rules the program exercised are the header's enum, all of it."""
    out = os.path.join(str(tmp_path), "tensor_out_kats")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                    "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "tensor_out_kats.cc"), "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("exercised:")]
    assert len(line) == 1, r.stdout
    header = open(os.path.join(ROOT, "libjxl_amd", "csrc", "host", "jxh_tensor_out.h")).read()
    rules = re.findall(r"^  kTensorRule(\w+),", header, re.M)
    assert len(rules) == 9 and set(line[0].split()[1:]) == set(rules), sorted(set(rules) ^ set(line[0].split()[1:]))
    # (and they stay out of the upload plan's enum, which tests/test_kats.py holds against its own program)
    plan = open(os.path.join(ROOT, "libjxl_amd", "csrc", "host", "jxh_upload_plan.h")).read()
    assert "kTensorRule" not in plan


def test_pixel_route_with_a_tensor(tmp_path):
    """PixelRouteOf (jxh_upload_plan.h): a three-plane float tensor with adjacent columns takes the row-streaming kernel's
    tensor form exactly where RGB f32 would come from that kernel; anything else the generic writer; and with the
    defaulted fields ("no tensor") every route is what the options without them give."""
    src = os.path.join(str(tmp_path), "route.cc")
    open(src, "w").write(r'''
#include <stdio.h>
#include "%s/libjxl_amd/csrc/host/jxh_upload_plan.h"
using namespace jxlhip::upload;
static int Route(const JxlHipFrameDesc& d, const UploadOptions& o) {
  const PixelRoute r = PixelRouteOf(d, o);
  return (r.color_out ? 1 : 0) | (r.gray8_fast ? 2 : 0) | (r.tensor_fused ? 4 : 0) | (r.plane1 ? 8 : 0);
}
int main() {
  int bad = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %%d: %%s\n", __LINE__, #c); bad++; } } while (0)
  JxlHipFrameDesc d;
  memset(&d, 0, sizeof(d));
  d.xsize = 520; d.ysize = 300;
  UploadOptions t;  // a contiguous CHW f16 tensor over the frame
  t.tensor = true; t.tensor_rows = true; t.out_type = JXLHIP_TENSOR_F16; t.out_nc = 3; t.tensor_reach = 520 * 300 * 3 * 2;
  for (int epf = 0; epf <= 3; epf++) {
    d.epf_iters = epf;
    const bool rows = epf == 1 || epf == 2;
    for (uint32_t type : {JXLHIP_TENSOR_F32, JXLHIP_TENSOR_F16, JXLHIP_TENSOR_BF16}) {
      UploadOptions o = t;
      o.out_type = type;
      EXPECT(Route(d, o) == (rows ? 4 : 9));
    }
    UploadOptions o = t;
    o.out_type = JXLHIP_TENSOR_U8;  // (never the context's own RGB8 rows, whatever the tensor's type)
    EXPECT(Route(d, o) == 9);
    o = t; o.out_nc = 4; EXPECT(Route(d, o) == 9);
    o = t; o.out_nc = 1; EXPECT(Route(d, o) == 9);
    o = t; o.tensor_rows = false; EXPECT(Route(d, o) == 9);        // HWC
    o = t; o.out_orient = 1; EXPECT(Route(d, o) == 9);
    o = t; o.keep_filtered = true; EXPECT(Route(d, o) == 9);
    o = t; o.tensor_reach = uint64_t(1) << 31; EXPECT(Route(d, o) == 9);  // beyond the kernel's 32-bit offsets
    o = t; o.tensor_reach = (uint64_t(1) << 31) - 1; EXPECT(Route(d, o) == (rows ? 4 : 9));
    JxlHipFrameDesc e = d;
    e.linear_output = 1; EXPECT(Route(e, t) == (rows ? 4 : 9));
    e.linear_output = 2; EXPECT(Route(e, t) == 9);
    e = d; e.has_noise = 1; EXPECT(Route(e, t) == 9);
    e = d; e.upsampling = 2; e.out_xsize = 1040; e.out_ysize = 600; EXPECT(Route(e, t) == 9);
    // no tensor: RGB8 from every filter kernel, RGB f32 and one 8-bit channel from the row-streaming one, as before
    UploadOptions p;
    EXPECT(Route(d, p) == 0);
    p.out_type = 0; EXPECT(Route(d, p) == (rows ? 0 : 9));
    p.out_type = 2; p.out_nc = 1; EXPECT(Route(d, p) == (rows ? 2 : 9));
    p.out_type = 5; p.out_nc = 3; EXPECT(Route(d, p) == 9);
  }
  printf(bad ? "failed\n" : "ok\n");
  return bad ? 1 : 0;
}
''' % ROOT)
    out = os.path.join(str(tmp_path), "route")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                    "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), src, "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]


def test_torch_io_descriptor_of_a_tensor():
    """torch_io.bind on CPU stand-ins: strides, channel count, room and the float32 scale / bias reach the raw binding as
    the tensor has them (a context double records the call); libjxl_amd itself imports without torch."""
    import libjxl_amd as J
    from libjxl_amd import torch_io

    src = open(os.path.join(ROOT, "libjxl_amd", "__init__.py")).read()
    assert "import torch" not in src

    class Ctx:
        def set_output_tensor(self, *a):
            self.call = a

    class Fake:  # a device tensor's face over a CPU one (bind refuses CPU tensors)
        is_cuda = True

        def __init__(self, t):
            self.t = t

        def __getattr__(self, name):
            return getattr(self.t, name)

    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    batch = torch.zeros((4, 3, 37, 121), dtype=torch.bfloat16)
    c = Ctx()
    torch_io.bind(c, Fake(batch[2]), "CHW", mean, std, True, stream=7)
    ptr, room, dtype, nc, strides, scale, bias, clamp, stream = c.call
    assert ptr == batch[2].data_ptr() and room == 2 * 3 * 37 * 121 * 2 and dtype == J.TENSOR_BF16 and nc == 3
    assert strides == (37 * 121, 121, 1) and clamp is True and stream == 7
    s32 = np.float32(1) / np.asarray(std, np.float32)
    assert scale.dtype == np.float32 and np.array_equal(scale, s32)
    assert np.array_equal(bias, -np.asarray(mean, np.float32) / np.asarray(std, np.float32)) and bias.dtype == np.float32
    hwc = torch.zeros((37, 121, 4), dtype=torch.float32)
    torch_io.bind(c, Fake(hwc), "HWC", mean, std, stream=0)
    assert c.call[3] == 4 and c.call[4] == (1, 121 * 4, 4)
    assert np.array_equal(c.call[5], np.append(s32, np.float32(1))) and c.call[6][3] == 0  # alpha: scale 1, bias 0
    padded = torch.zeros((3, 42, 124), dtype=torch.float16)[:, :37, 1:122]  # pitch 124, five spare rows, one element in
    torch_io.bind(c, Fake(padded), "CHW", stream=0)
    assert c.call[0] == padded.data_ptr() and c.call[4] == (42 * 124, 124, 1) and c.call[1] == (3 * 42 * 124 - 1) * 2
    # the structure the binding fills is the C one
    assert ctypes.sizeof(J.TensorOut) == 8 + 8 + 4 + 4 + 3 * 8 + 16 + 16 + 4 + 4 + 8
