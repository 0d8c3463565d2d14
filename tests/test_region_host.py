"""Region decode on the CPU: the host plan of libjxl_amd/csrc/host/jxh_window_plan.h under AddressSanitizer + UBSan
(tests/c/window_kats.cc, a stand-alone program), Frame.plan_window on parsed streams, the whole-frame reasons on the streams
that raise them, and what the Python layer hands to the C ABI. Nothing here touches a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "libjxl_amd", "csrc", "host", "jxh_window_plan.h")


def test_window_plan_under_sanitizers(tmp_path):
    """Every WholeFrameReason raised once, every DcWindowRule and WindowRule broken once (the names the program exercised
    are the header's enums, all of them), PlanWindow's known answers on the 1000 x 700 frame, all eight orientations,
    sums near 2^32, and BuildWindowDesc through CheckFrameDesc: the program's own checks."""
    exe = os.path.join(str(tmp_path), "window_kats")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                    "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "window_kats.cc"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    header = open(HEADER).read()

    def exercised(tag):
        line = [l for l in r.stdout.splitlines() if l.startswith(tag + ":")]
        assert len(line) == 1, r.stdout
        return set(line[0].split()[1:])

    reasons = re.findall(r"^  kWhole(\w+),", header, re.M)
    assert len(reasons) == 11 and exercised("reasons") == set(reasons) | {"Windowed"}
    dc_rules = re.findall(r"^  kDcWindowRule(\w+),", header, re.M)
    assert len(dc_rules) == 6 and exercised("dc_rules") == set(dc_rules)
    window_rules = re.findall(r"^  kWindowRule(\w+),", header, re.M)
    assert len(window_rules) == 3 and exercised("window_rules") == set(window_rules)


def test_the_halo_is_stated_once():
    """FusedHalo lives in jxh_filter_halo.h alone; the filter kernels and the window plan include it."""
    found = []
    for base, _, files in os.walk(os.path.join(ROOT, "libjxl_amd", "csrc")):
        for name in files:
            if re.search(r"constexpr int FusedHalo\(", open(os.path.join(base, name), errors="replace").read()):
                found.append(name)
    assert found == ["jxh_filter_halo.h"]
    assert '#include "jxh_filter_halo.h"' in open(HEADER).read()
    assert "hip/hip_runtime.h" not in open(HEADER).read()  # the plan is free of HIP


def _halo(gab, epf):
    return (1 if gab else 0) + (3 if epf >= 3 else 0) + (2 if epf >= 1 else 0) + (1 if epf >= 2 else 0)


@pytest.mark.parametrize("epf,gab", [(0, 0), (1, 0), (1, 1), (3, 1), (3, 0)])
def test_plan_window_on_parsed_streams(built, epf, gab):
    """Frame.plan_window on a parsed 1000 x 700 stream (4 x 3 groups, ragged last column and row): the filters' reach H
    decides at the pixel which group columns and rows a box takes, on both sides of a boundary."""
    J = built
    f = J.Frame(J.encode_rgb8(J.synth_image(1000, 700, seed=31), epf_iters=epf, gab=gab))
    assert (f.info["epf_iters"], f.info["gab"], f.info["num_groups"]) == (epf, gab, 12)
    H = _halo(gab, epf)
    # near side: a box that starts H - 1 pixels behind x = 256 reads column 0 (when H > 0), one that starts H behind does not
    w = f.plan_window((256 + H, 300, 100, 100))
    assert (w["gx0"], w["gxs"], w["gy0"], w["gys"], w["reason"]) == (1, 1, 1, 1, 0)
    assert w["groups"] == [5] and w["groups_taken"] == 1 and w["groups_in_frame"] == 12
    assert (w["x0"], w["y0"], w["xsize"], w["ysize"]) == (256, 256, 256, 256) and w["box"] == (H, 44, 100, 100)
    if H:
        w = f.plan_window((256 + H - 1, 300, 100, 100))
        assert (w["gx0"], w["gxs"]) == (0, 2) and w["groups"] == [4, 5] and w["box"] == (256 + H - 1, 44, 100, 100)
        w = f.plan_window((300, 256 + H - 1, 100, 100))
        assert (w["gy0"], w["gys"]) == (0, 2) and w["groups"] == [1, 5]
    # far side: ending at 512 - H stays, ending one pixel later takes the next column / row
    w = f.plan_window((300, 300, 512 - H - 300, 50))
    assert (w["gx0"], w["gxs"]) == (1, 1)
    w = f.plan_window((300, 300, 512 - H - 300 + 1, 50))
    assert (w["gx0"], w["gxs"]) == (1, 2) and w["groups"] == [5, 6]
    w = f.plan_window((300, 300, 50, 512 - H - 300 + 1))
    assert (w["gy0"], w["gys"]) == (1, 2) and w["groups"] == [5, 9] and (w["ysize"], w["xsize"]) == (444, 256)
    # one pixel, the ragged corner, the whole image (stated and None)
    w = f.plan_window((600, 400, 1, 1))
    assert w["groups"] == [6] and w["box"] == (88, 144, 1, 1)
    w = f.plan_window((990, 690, 10, 10))
    assert w["groups"] == [11] and (w["x0"], w["y0"], w["xsize"], w["ysize"]) == (768, 512, 232, 188) and w["box"] == (222, 178, 10, 10)
    for box in ((0, 0, 1000, 700), None):
        w = f.plan_window(box)
        assert w["reason"] == J.WINDOW_REASONS.index("window_is_frame") and w["groups"] == list(range(12))
        assert (w["x0"], w["y0"], w["xsize"], w["ysize"]) == (0, 0, 1000, 700)
    # orientation 6 (the output is 700 wide): the box mapped into the frame decides the groups
    w = f.plan_window((20, 20, 100, 100), orientation=6)
    assert w["reason"] == 0 and w["orientation"] == 6
    for box in ((991, 0, 10, 10), (0, 0, 10, 0), (5, 0, 0, 0), (0xFFFFFFF0, 0, 0x20, 10)):
        with pytest.raises(J.JxlAmdError):
            f.plan_window(box)
    with pytest.raises(J.JxlAmdError):
        f.plan_window((691, 0, 10, 10), orientation=6)
    f.close()


def test_a_4k_frame_gives_a_training_crop_four_groups_at_most(built):
    """3840 x 2160, Gaborish and three EPF iterations (H = 7): any 224 x 224 box takes at most 4 of 135 groups, since
    224 + 2 * 7 <= 256. The plan of a parsed frame of that size (a flat image: the parse is what costs)."""
    J = built
    f = J.Frame(J.encode_rgb8(np.full((2160, 3840, 3), 90, np.uint8), epf_iters=3, gab=1))
    rng = np.random.default_rng(5)
    most = 0
    for _ in range(200):
        x, y = int(rng.integers(0, 3840 - 224 + 1)), int(rng.integers(0, 2160 - 224 + 1))
        w = f.plan_window((x, y, 224, 224))
        assert w["reason"] == 0 and w["groups_in_frame"] == 135
        most = max(most, w["groups_taken"])
    for x, y in ((250, 250), (256 * 14 - 3, 256 * 7 - 3), (3840 - 224, 2160 - 224), (0, 0)):
        most = max(most, f.plan_window((x, y, 224, 224))["groups_taken"])
    assert most == 4
    f.close()


def test_whole_frame_reasons_on_the_streams_that_raise_them(built):
    J = built
    R = J.WINDOW_REASONS
    assert len(R) == 12 and R[0] == "windowed"
    img = J.synth_image(600, 300, seed=77)
    box = (300, 40, 64, 64)

    def reason(data, channels=3, box=box, **kw):
        f = J.Frame(data, **kw)
        try:
            w = f.plan_window(box, channels)
            if w["reason"]:  # the whole frame, and the caller's own box
                assert w["groups"] == list(range(f.info["num_groups"])) and w["box"] == box
            return R[w["reason"]]
        finally:
            f.close()

    plain = J.encode_rgb8(img, epf_iters=1)
    assert reason(plain) == "windowed"
    assert reason(plain, channels=1) == "windowed"
    assert reason(plain, channels=4) == "alpha" and reason(plain, channels=2) == "alpha"
    assert reason(J.encode_rgb8(img, upsampling=2)) == "upsampling"
    assert reason(J.encode_rgb8(img, noise=60)) == "noise"
    assert reason(J.encode_rgb8(img, color_transform=2, chroma_subsampling=4, strategy_mode=0)) == "subsampling"
    J.set_splines([dict(points=[(20, 20), (200, 100), (500, 250)], color=[[30] + [0] * 31, [40] + [0] * 31, [10] + [0] * 31],
                        sigma=[20] + [0] * 31)])
    try:
        splined = J.encode_rgb8(img)
    finally:
        J.set_splines(None)
    assert reason(splined) == "splines"
    atlas = J.synth_image(64, 48, seed=3)
    patched = J.encode_patched(img, atlas, [dict(x0=4, y0=6, xsize=20, ysize=16, positions=[(250, 170, 2, 0)])], atlas_vardct=True)
    first = J.Frame(patched)
    assert reason(patched, frame_pos=first.end, frame_index=1) == "patches"
    first.close()
    small = J.synth_image(200, 100, seed=9)
    assert reason(J.encode_rgb8(small), box=(3, 3, 10, 10)) == "single_section"
    assert reason(J.encode_rgb8(small, num_passes=2), box=(3, 3, 10, 10)) == "one_group"
    with_dc = J.encode_with_dc_frame(img, dc_vardct=True)
    dc_frame = J.Frame(with_dc)
    assert reason(with_dc, frame_pos=dc_frame.end, frame_index=1) == "dc_frame"
    dc_frame.close()
    reduced = J.Frame(plain, reduced=True)
    assert R[reduced.plan_window(box)["reason"]] == "partial"
    reduced.close()


def test_the_window_structure_is_the_c_one(built):
    J = built
    src = os.path.join(ROOT, "include", "jxl_amd.h")
    exe = os.path.join(os.environ.get("TMPDIR", "/tmp"), "window_sizeof_%d" % os.getpid())
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n#include "%s"\nint main() { printf("%%zu %%zu %%zu %%zu %%zu %%zu\\n", ' \
           'sizeof(JxlAmdWindow), offsetof(JxlAmdWindow, box), offsetof(JxlAmdWindow, reason), sizeof(JxlHipDcWindow), ' \
           'offsetof(JxlHipDcWindow, apron), offsetof(JxlHipDcWindow, dc_smoothing)); return 0; }\n' % (src, os.path.join(ROOT, "include", "jxl_amd_hip.h"))
    try:
        subprocess.run(["g++", "-std=c++17", "-x", "c++", "-I" + os.path.join(ROOT, "include"), "-", "-o", exe], input=prog, text=True, check=True)
        sizes = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    finally:
        if os.path.exists(exe):
            os.remove(exe)
    assert sizes == [ctypes.sizeof(J.Window), J.Window.box.offset, J.Window.reason.offset, ctypes.sizeof(J.DcWindow), J.DcWindow.apron.offset,
                     J.DcWindow.dc_smoothing.offset]
    assert J.lib().jxlamd_sizeof_window() == ctypes.sizeof(J.Window)
    assert J.dc_apron((32, 32, 32, 32), (125, 88)) == (31, 31, 34, 34) and J.dc_apron((0, 0, 125, 88), (125, 88)) == (0, 0, 125, 88)
    assert J.dc_apron((96, 64, 29, 24), (125, 88)) == (95, 63, 30, 25)


def test_torch_io_routes_a_crop_through_the_window():
    """decode_to_tensor / decode_batch_to_tensor on CPU doubles: with size and box a VarDCT frame is planned, the TRANSLATED
    box is bound and upload_window takes the plan; region=False, no box, and Modular frames keep the former route; corrupt
    sections are named by frame group."""
    import torch
    import libjxl_amd as J
    from libjxl_amd import torch_io

    calls = []

    class Frame:
        info = dict(xsize=1000, ysize=700, out_xsize=1000, out_ysize=700, num_groups=12)

        def plan_window(self, box, channels=3):
            calls.append(("plan", tuple(box), channels))
            return dict(box=(7, 44, 100, 100), groups=[5, 6], reason=0)

    class Ctx:
        flags = [0, 0]

        def upload_window(self, f, w):
            calls.append(("upload_window", w["box"]))

        def upload(self, f):
            calls.append(("upload",))

        def errors(self):
            return (3 if any(self.flags) else 0), self.flags

    bound = []
    real = torch_io.bind_resized
    torch_io.bind_resized = lambda c, out, layout, box, *a, **k: bound.append(box)
    try:
        out = torch.zeros((3, 8, 8))
        assert torch_io._upload_crop(Ctx(), Frame(), out, "CHW", (263, 300, 100, 100), None, None, False, 3, True) == [5, 6]
        assert calls == [("plan", (263, 300, 100, 100), 3), ("upload_window", (7, 44, 100, 100))] and bound == [(7, 44, 100, 100)]
        del calls[:], bound[:]
        assert torch_io._upload_crop(Ctx(), Frame(), out, "CHW", (263, 300, 100, 100), None, None, False, 3, False) == list(range(12))
        assert calls == [("upload",)] and bound == [(263, 300, 100, 100)]
        del calls[:], bound[:]
        assert torch_io._upload_crop(Ctx(), Frame(), out, "CHW", None, None, None, False, 3, True) == list(range(12))
        assert calls == [("upload",)] and bound == [None]
    finally:
        torch_io.bind_resized = real
    import inspect
    for fn in (torch_io.decode_to_tensor, torch_io.decode_batch_to_tensor):
        assert inspect.signature(fn).parameters["region"].default is True
    assert "import torch" not in open(os.path.join(ROOT, "libjxl_amd", "__init__.py")).read()
