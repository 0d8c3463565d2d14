"""libjxl_amd/csrc/host/jxh_filter_plan.h, the launch plan of jxlhip_run_filter_color_batch's filter kernels, on the CPU:
tests/c/filter_plan_kats.cc built as a stand-alone program with AddressSanitizer + UBSan. The program holds the grouping
loop and the row kernel's grid lines as the HIP layer had them before the header, and compares field for field: one 4K frame
(by hand: 8 workgroups across, 34 strips of 64 rows), eleven and twelve of them (either side of the strip doubling), 640;
all eight (Gaborish, EPF) forms with grey and tensor frames between them over unequal sizes, a 1 x 1 frame and a band of
one row; a frame that clears its group's u8srgb, in each of the four ways; a grey frame in such a group, refused with the
same code; an empty band and an empty set; and the kernel of each of the 32 forms."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("filter_plan")), "filter_plan_kats")
    subprocess.run(["g++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                    os.path.join(ROOT, "tests", "c", "filter_plan_kats.cc"), "-o", out], check=True)
    return out


def test_the_filter_plan_is_the_reading_the_hip_layer_had(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "filter plan kats passed" in r.stdout
