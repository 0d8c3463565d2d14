"""The resized binding (jxlhip_set_output_resized) on the CPU: the float64 reading of its semantics (tests/resample_f64.py)
against torch's own antialiased interpolation, the host plan of libjxl_amd/csrc/host/jxh_resample_plan.h under
AddressSanitizer + UBSan (tests/c/resample_kats.cc, a stand-alone program) against that reading, named misreadings of the
reading against the error bar, and what the Python layer hands to the C ABI. Nothing here touches a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import resample_f64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (in_h, in_w, out_h, out_w): up- and down-scaling, extents of 1, the identity, both axes different
SHAPES = [(37, 53, 8, 8), (8, 8, 21, 13), (300, 520, 224, 224), (17, 1, 5, 3), (1, 1, 4, 4), (64, 64, 64, 64), (100, 3, 7, 9), (5, 7, 5, 20)]
AXES = sorted({(s[0], s[2]) for s in SHAPES} | {(s[1], s[3]) for s in SHAPES} | {(600, 7), (7, 600), (16384, 1), (1, 16384)})


def _image(h, w, c=3, seed=0):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, (h, w, c))


def _torch_resize(img, out_h, out_w, box=None):
    x0, y0, bw, bh = box if box is not None else (0, 0, img.shape[1], img.shape[0])
    t = torch.from_numpy(np.ascontiguousarray(img[y0:y0 + bh, x0:x0 + bw])).permute(2, 0, 1)[None].to(torch.float64)
    o = torch.nn.functional.interpolate(t, size=(out_h, out_w), mode="bilinear", antialias=True, align_corners=False)
    return o[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_the_reading_is_torch_antialiased_bilinear_in_float64(shape):
    """The reading equals torch.nn.functional.interpolate(mode="bilinear", antialias=True, align_corners=False) on the CPU in
    float64 to 1e-12, whole image and a box (the crop comes first); 64 x 64 -> 64 x 64 is the identity exactly."""
    h, w, oh, ow = shape
    img = _image(h, w, 3, seed=h * 1000 + w)
    got = R.resize(img, oh, ow)
    assert np.abs(got - _torch_resize(img, oh, ow)).max() <= 1e-12
    if (h, w) == (oh, ow):
        assert np.array_equal(got, img)
    if h >= 5 and w >= 5:
        box = (1, 2, w - 3, h - 3)
        assert np.abs(R.resize(img, oh, ow, box) - _torch_resize(img, oh, ow, box)).max() <= 1e-12


def _build_kats(tmp_path):
    out = os.path.join(str(tmp_path), "resample_kats")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                    "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "resample_kats.cc"), "-o", out], check=True)
    return out


def test_resample_plan_under_sanitizers_against_the_reading(tmp_path):
    """Every ResampleRule refuses the one change that breaks it (the rules the program exercised are the header's enum, all of
    it), boxes near 2^32 included; MakeAxisTaps gives the reading's table for every axis of SHAPES and 600 -> 7, 7 -> 600,
    16384 -> 1, 1 -> 16384: the same first and count, and the reading's double weights rounded to float32, exactly; the
    sums, the bound and the placement into blocks of exactly their size are the program's own checks."""
    exe = _build_kats(tmp_path)
    dump = os.path.join(str(tmp_path), "tables.bin")
    r = subprocess.run([exe, dump] + ["%d:%d" % a for a in AXES], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("exercised:")]
    assert len(line) == 1, r.stdout
    header = open(os.path.join(ROOT, "libjxl_amd", "csrc", "host", "jxh_resample_plan.h")).read()
    rules = re.findall(r"^  kResampleRule(\w+),", header, re.M)
    assert "Count" not in rules and len(rules) >= 6 and set(line[0].split()[1:]) == set(rules), sorted(set(rules) ^ set(line[0].split()[1:]))
    # (and they stay out of the tensor descriptor's header, whose nine rules tests/test_tensor_out_host.py counts)
    assert "kResampleRule" not in open(os.path.join(ROOT, "libjxl_amd", "csrc", "host", "jxh_tensor_out.h")).read()
    assert "axes: %d" % len(AXES) in r.stdout
    raw = np.fromfile(dump, np.uint32)
    at = 0
    for n_in, n_out in AXES:
        assert (raw[at], raw[at + 1]) == (n_in, n_out)
        total = int(raw[at + 2])
        first = raw[at + 3:at + 3 + n_out]
        count = raw[at + 3 + n_out:at + 3 + 2 * n_out]
        weights = raw[at + 3 + 2 * n_out:at + 3 + 2 * n_out + total].view(np.float32)
        at += 3 + 2 * n_out + total
        rows = R.axis_taps(n_in, n_out)
        assert [lo for lo, _ in rows] == first.tolist() and [len(w) for _, w in rows] == count.tolist(), (n_in, n_out)
        want = np.concatenate([w for _, w in rows]).astype(np.float32)
        assert total == want.size and np.array_equal(weights, want), (n_in, n_out)
        assert total <= 2 * n_in + 2 * n_out + 2
    assert at == raw.size


# Each misreading against the listed case it must move by more than ten bars: (misreading, shape, box).
MISREAD_CASES = [
    ("align_corners", (8, 8, 21, 13), None),
    ("no_antialias", (300, 520, 224, 224), None),
    ("no_renormalise", (37, 53, 8, 8), None),
    ("crop_after", (300, 520, 224, 224), (100, 40, 300, 200)),
    ("origin_off_by_one", (300, 520, 224, 224), (100, 40, 300, 200)),
    ("scales_exchanged", (300, 520, 224, 224), None),
    ("floor_windows", (8, 8, 21, 13), None),
    ("normalise_after_f32", (300, 520, 224, 224), None),
]


def test_every_misreading_has_a_case():
    assert sorted(m for m, _, _ in MISREAD_CASES) == sorted(R.MISREADINGS)


@pytest.mark.parametrize("wrong,shape,box", MISREAD_CASES, ids=[m for m, _, _ in MISREAD_CASES])
def test_named_misreadings_are_far_outside_the_bar(wrong, shape, box):
    """A reading that takes one rule of the semantics wrongly moves its case by more than ten error bars: the bar of the GPU
    tests tells these apart."""
    h, w, oh, ow = shape
    # (the two ends of the value range at random: the largest contrast the range allows, so that a displaced weight shows
    # as much as it can; chosen before any misreading was measured on it)
    img = np.where(np.random.default_rng(7).integers(0, 2, (h, w, 3)) > 0, 1.1, -0.1)
    right = R.resize(img, oh, ow, box)
    moved = np.abs(R.resize(img, oh, ow, box, wrong=wrong) - right).max()
    bar = R.bar(img, oh, ow, box)
    print("%s: moved %.3g = %.1f bars" % (wrong, moved, moved / bar))
    assert moved > 10 * bar


def test_float32_emulation_stays_far_below_the_bar():
    """The bar is a priori; a float32 two-pass evaluation with the table's float32 weights uses a small part of it."""
    worst = 0.0
    for h, w, oh, ow in [(37, 53, 8, 8), (8, 8, 21, 13), (100, 3, 7, 9), (5, 600, 3, 7), (257, 263, 31, 29)]:
        img = _image(h, w, 2, seed=3).astype(np.float32)
        d = np.abs(R.emulate_f32(img, oh, ow).astype(np.float64) - R.resize(img, oh, ow)).max()
        worst = max(worst, d / R.bar(img, oh, ow))
    print("float32 emulation: %.3f of the bar at most" % worst)
    assert worst < 0.5


def test_torch_io_descriptor_of_a_resized_binding():
    """torch_io.bind_resized and decode_* on CPU stand-ins: the box, the output size, the strides of channels-last and padded
    tensors, and the float32 scale / bias reach the raw binding unchanged (a context double records the call); the ctypes
    structure is the C one; libjxl_amd itself imports without torch."""
    import libjxl_amd as J
    from libjxl_amd import torch_io

    assert "import torch" not in open(os.path.join(ROOT, "libjxl_amd", "__init__.py")).read()

    class Ctx:
        def set_output_resized(self, *a):
            self.call = a

    class Fake:  # a device tensor's face over a CPU one (bind_resized refuses CPU tensors)
        is_cuda = True

        def __init__(self, t):
            self.t = t

        def __getattr__(self, name):
            return getattr(self.t, name)

    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    batch = torch.zeros((4, 3, 33, 17), dtype=torch.float16)
    c = Ctx()
    torch_io.bind_resized(c, Fake(batch[1]), "CHW", (5, 6, 100, 80), mean, std, True, stream=9)
    ptr, room, dtype, nc, strides, out_size, box, scale, bias, clamp, stream = c.call
    assert ptr == batch[1].data_ptr() and room == 3 * 3 * 33 * 17 * 2 and dtype == J.TENSOR_F16 and nc == 3
    assert strides == (33 * 17, 17, 1) and out_size == (17, 33) and box == (5, 6, 100, 80) and clamp is True and stream == 9
    s32 = np.float32(1) / np.asarray(std, np.float32)
    assert scale.dtype == np.float32 and np.array_equal(scale, s32)
    assert bias.dtype == np.float32 and np.array_equal(bias, -np.asarray(mean, np.float32) / np.asarray(std, np.float32))
    hwc = torch.zeros((33, 17, 4), dtype=torch.float32)  # channels-last storage
    torch_io.bind_resized(c, Fake(hwc), "HWC", None, mean, std, stream=0)
    assert c.call[3] == 4 and c.call[4] == (1, 17 * 4, 4) and c.call[5] == (17, 33) and c.call[6] is None
    assert np.array_equal(c.call[7], np.append(s32, np.float32(1))) and c.call[8][3] == 0  # alpha: scale 1, bias 0
    padded = torch.zeros((3, 40, 24), dtype=torch.bfloat16)[:, :33, 1:18]  # pitch 24, seven spare rows, one element in
    torch_io.bind_resized(c, Fake(padded), "CHW", (0, 0, 1, 1), stream=0)
    assert c.call[0] == padded.data_ptr() and c.call[4] == (40 * 24, 24, 1) and c.call[1] == (3 * 40 * 24 - 1) * 2
    assert c.call[5] == (17, 33) and c.call[6] == (0, 0, 1, 1) and c.call[2] == J.TENSOR_BF16
    for bad in [(0, 0, 0, 5), (1, 2, 3), (-1, 0, 4, 4)]:
        with pytest.raises(ValueError):
            torch_io.bind_resized(c, Fake(hwc), "HWC", bad, stream=0)
    with pytest.raises(ValueError):
        torch_io.decode_to_tensor(b"", box=(0, 0, 4, 4))  # a box needs a size
    with pytest.raises(ValueError):
        torch_io.decode_batch_to_tensor([], boxes=[])
    # the raw binding: what HipContext.set_output_resized puts into the structure, and the structure is the C one
    d = J._resized_out(0x1000, 4096, J.TENSOR_F32, 3, (600, 20, 1), (20, 30), (1, 2, 3, 4), s32, [0.5], True, 11, J.RESAMPLE_TRIANGLE)
    assert (d.out_xsize, d.out_ysize, d.box_x0, d.box_y0, d.box_xsize, d.box_ysize, d.filter) == (20, 30, 1, 2, 3, 4, 0)
    assert (d.tensor.data, d.tensor.bytes, d.tensor.stride_c, d.tensor.stride_y, d.tensor.stride_x) == (0x1000, 4096, 600, 20, 1)
    assert list(d.tensor.scale) == [float(s32[0]), float(s32[1]), float(s32[2]), 1.0] and list(d.tensor.bias) == [0.5, 0, 0, 0]
    assert d.tensor.clamp01 == 1 and d.tensor.consumer_stream == 11
    whole = J._resized_out(0x1000, 4096, J.TENSOR_F32, 3, (600, 20, 1), (20, 30), None, None, None, False, 0, 0)
    assert (whole.box_x0, whole.box_y0, whole.box_xsize, whole.box_ysize) == (0, 0, 0, 0)
    src = os.path.join(ROOT, "include", "jxl_amd_hip.h")
    exe = os.path.join(os.environ.get("TMPDIR", "/tmp"), "resized_sizeof_%d" % os.getpid())
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main() { printf("%%zu %%zu %%zu\\n", sizeof(JxlHipResizedOut), ' \
           'offsetof(JxlHipResizedOut, out_xsize), offsetof(JxlHipResizedOut, filter)); return 0; }\n' % src
    try:
        subprocess.run(["g++", "-std=c++17", "-x", "c++", "-", "-o", exe], input=prog, text=True, check=True)
        sizes = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    finally:
        if os.path.exists(exe):
            os.remove(exe)
    assert [int(v) for v in sizes] == [ctypes.sizeof(J.ResizedOut), J.ResizedOut.out_xsize.offset, J.ResizedOut.filter.offset]
    assert ctypes.sizeof(J.ResizedOut) == ctypes.sizeof(J.TensorOut) + 7 * 4 + 4  # (seven uint32 and the tail's padding to 8)
