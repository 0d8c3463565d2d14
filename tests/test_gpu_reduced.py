"""GPU tests (-m gpu) of the reduced output (jxlhip_reduced_upload / jxlhip_reduced_run, libjxl_amd.decode_reduced,
torch_io's reduce=8): the image at 1/8 scale from the frame's DC image. Each link is held to something that is not the
code under test: the DC planes to the parent's k_dc_dequant / k_dc_smooth (bit for bit) and the oracle; the colour stage to
the float64 reading of tests/color_encoding_f64.py; the writer to tests/writer_np.py and the tensor formula, on the f32
output; the resized binding to tests/resample_f64.py; the definition to the 8x8 means of a source image."""
import ctypes
import os

import numpy as np
import pytest
import torch

import color_api as A
import color_encoding_f64 as C
import resample_f64 as R
import writer_np as W
from libjxl_amd import torch_io
from test_gpu_tensor_out import Canvas, _formula, _same

pytestmark = pytest.mark.gpu

# the smallest shapes that reach each branch: one block; all border; one interior block; one row of blocks over several
# tiles' worth of columns; several tiles both ways with ragged edges; two DC groups
SHAPES = [(8, 8), (16, 24), (24, 24), (520, 8), (403, 277), (2300, 300)]
SETTINGS = {"default": dict(), "d3_epf3": dict(distance=3.0, epf_iters=3), "no_smoothing_cmap": dict(skip_dc_smoothing=1, custom_cmap=1),
            "lf_cmap": dict(custom_lf=1, custom_cmap=1)}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
LUMA = np.array([0.2126, 0.7152, 0.0722])
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _stream(J, w, h, setting="default"):
    return _cached(("stream", w, h, setting), lambda: J.encode_rgb8(J.synth_image(w, h, seed=5), **SETTINGS[setting]))


def _reduced(J, data, fmt=(0, 3), orientation=1, keep_dc=False, bind=None, frame=None, whole=False):
    """One reduced decode on a fresh context -> (pixels or None when bound, DC planes [3, yb, xb] or None). frame(f): colour
    settings of the frame; whole: upload_reduced of a whole parse instead of the reduced one."""
    f = J.Frame(data) if whole else J.Frame(data, reduced=True)
    c = J.HipContext()
    try:
        if frame:
            frame(f)
        if keep_dc:
            c.set_option("keep_dc", 1)
        if orientation != 1:
            c.set_output_orientation(orientation)
        if bind:
            bind(c)
        else:
            c.set_output_format(*fmt)
        c.upload_reduced(f)
        c.run_reduced()
        xb, yb = f.reduced_size()
        dc = c.download("dc").reshape(3, yb, xb) if keep_dc else None
        return (None if bind else c.pixels()), dc
    finally:
        c.close()
        f.close()


def _f32(J, w, h, setting="default", nc=3):
    """The f32 reduced image of a stream: the writer tests' input, computed once."""
    return _cached(("f32", w, h, setting, nc), lambda: _reduced(J, _stream(J, w, h, setting), (0, nc))[0])


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_dc_planes_are_the_full_uploads_bit_for_bit(built, shape, setting):
    """With "keep_dc", download("dc") after run_reduced equals download("dc") after the whole upload of the same stream (the
    parent's k_dc_dequant and k_dc_smooth, which test_dc_path_kernels_against_the_oracle_and_a_float64_reading holds to
    the oracle), bit for bit, and stays within that test's 2e-6 of the oracle's dc. Without the option the download is
    refused: the planes exist nowhere."""
    import jxlo
    J = built
    data = _stream(J, *shape, setting)
    _, dc_r = _reduced(J, data, keep_dc=True)
    f = J.Frame(data)
    c = J.HipContext()
    try:
        c.upload(f)
        dc_f = c.download("dc").reshape(dc_r.shape)
    finally:
        c.close()
        f.close()
    assert np.array_equal(dc_r.view(np.uint32), dc_f.view(np.uint32)), np.abs(dc_r - dc_f).max()
    o = jxlo.Decoded(data)
    try:
        dc_o = o.buffer("dc").reshape(dc_r.shape)
        smoothed = o.buffer("dc_unsmoothed") is not None
    finally:
        o.close()
    if min(shape) >= 24:  # (the streams exercise what their names say; a frame without interior has nothing to smooth)
        assert smoothed == (setting != "no_smoothing_cmap")
    assert np.abs(dc_r - dc_o).max() < 2e-6
    if shape == (24, 24):
        f = J.Frame(data, reduced=True)
        c = J.HipContext()
        try:
            c.upload_reduced(f)
            c.run_reduced()
            with pytest.raises(J.JxlAmdError):
                c.download("dc")
        finally:
            c.close()
            f.close()


def test_precision_shift_of_each_dc_group(built):
    """The test encoders write precision shift 0 only: a descriptor handed to jxlhip_reduced_upload directly, 300 x 3 blocks
    in two DC groups with shifts 1 and 2 and no smoothing, against DequantDC in float32 NumPy (compressed_dc.cc:201-296:
    each product and each sum rounded once)."""
    J = built
    L = J.lib()

    class Desc(ctypes.Structure):  # JxlHipReducedDesc
        _fields_ = [("xsize_blocks", ctypes.c_uint32), ("ysize_blocks", ctypes.c_uint32), ("dc_quantised", ctypes.c_void_p),
                    ("dc_extra_precision", ctypes.c_void_p), ("dc_step", ctypes.c_float * 3), ("dc_cfl_x", ctypes.c_float),
                    ("dc_cfl_b", ctypes.c_float), ("dc_smoothing", ctypes.c_uint32), ("opsin_inv", ctypes.c_float * 9),
                    ("opsin_bias", ctypes.c_float * 3), ("linear_output", ctypes.c_int32), ("color_target", ctypes.c_void_p)]

    xb, yb = 300, 3
    rng = np.random.default_rng(11)
    q = np.ascontiguousarray(rng.integers(-900, 900, (3, yb, xb)), np.int32)
    ep = np.array([1, 2], np.uint8)
    step = np.array([0.00018154998, 0.0014523999, 0.0029047998], np.float32)
    cfl_x, cfl_b = np.float32(0.03125), np.float32(0.9375)
    d = Desc()
    d.xsize_blocks, d.ysize_blocks, d.dc_quantised, d.dc_extra_precision = xb, yb, q.ctypes.data, ep.ctypes.data
    d.dc_step[:] = [float(s) for s in step]
    d.dc_cfl_x, d.dc_cfl_b, d.dc_smoothing, d.linear_output = float(cfl_x), float(cfl_b), 0, 1
    d.opsin_inv[:] = [float(v) for v in C.INV_OPSIN.reshape(-1)]
    d.opsin_bias[:] = [C.BIAS] * 3
    L.jxlhip_reduced_upload.argtypes = [ctypes.c_void_p, ctypes.POINTER(Desc)]
    c = J.HipContext()
    try:
        c.set_option("keep_dc", 1)
        c.set_output_format(0, 3)
        assert L.jxlhip_reduced_upload(c._h, ctypes.byref(d)) == 0
        c.frame_info = dict(out_xsize=xb, out_ysize=yb)
        c.run_reduced()
        got = c.download("dc").reshape(3, yb, xb)
        # several DC groups without their precision bytes: refused, nothing to run
        d.dc_extra_precision = None
        assert L.jxlhip_reduced_upload(c._h, ctypes.byref(d)) == 1
        with pytest.raises(J.JxlAmdError):
            c.run_reduced()
    finally:
        c.close()
    mul = (np.float32(1) / np.exp2(np.where(np.arange(xb) < 256, 1, 2)).astype(np.float32))[None, :]
    in_x, in_y, in_b = [(q[k].astype(np.float32) * (step[k] * mul).astype(np.float32)).astype(np.float32) for k in range(3)]
    want = np.stack([((in_y * cfl_x).astype(np.float32) + in_x).astype(np.float32), in_y, ((in_y * cfl_b).astype(np.float32) + in_b).astype(np.float32)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _reading(dc, matrix):
    """Linear RGB [yb, xb, 3] of DC planes [3, yb, xb] by the float64 reading: matrix @ the opsin-mixed values."""
    lin = matrix @ C.xyb_to_mixed(dc.reshape(3, -1).astype(np.float64))
    return lin.T.reshape(dc.shape[1], dc.shape[2], 3)


def _ce_of(name):
    kw, p, w, tf, _ = A.ENCODINGS[name]
    ce = A.CE()
    ce.color_space, ce.white_point, ce.primaries = 0, kw["white_point"], kw["primaries"]
    ce.white_point_xy[:] = w
    ce.red[:], ce.green[:], ce.blue[:] = p[0:2], p[2:4], p[4:6]
    ce.transfer_function, ce.gamma, ce.rendering_intent = kw["transfer_function"], 0.0, 1
    return ce


def test_colour_stage_against_the_float64_reading(built):
    """The f32 reduced image against tests/color_encoding_f64.py applied to the downloaded DC planes, at the bars of
    test_gpu_grey_xyb.py / test_gpu_color_encoding.py: linear within 4e-6 of the largest sample, sRGB within 2e-4, a PQ
    BT.2100 stream rendered to its own encoding within 2e-4, and a grey stream whose one channel is the luminance (2e-4) and
    equals channel 0 of three. Each is also compared with the colour stage alone (jxlhip_debug_color[_target]) on the same
    planes after the whole upload, at the same bars; the largest difference is printed (0 is expected: the same device
    functions on the same inputs)."""
    J = built
    L = A.setup(J.lib())
    w, h = 403, 277
    data = _stream(J, w, h)
    img = J.synth_image(w, h, seed=5)

    def stage_alone(stream, xyb, linear=False, target=None, frame=None):
        f = J.Frame(stream)
        c = J.HipContext()
        try:
            if frame:
                frame(f)
            c.upload(f)
            if target is None:
                return c.debug_color(xyb, linear)
            out = np.empty((xyb.shape[1], 3), np.float32)
            assert L.jxlhip_debug_color_target(c._h, xyb.ctypes.data, xyb.shape[1], ctypes.byref(target), out.ctypes.data) == 0
            return out
        finally:
            c.close()
            f.close()

    # linear and sRGB of an untagged stream
    for linear in (True, False):
        px, dc = _reduced(J, data, keep_dc=True, frame=lambda f: f.set_linear_output(linear))
        lin = _reading(dc, C.output_matrix(C.SRGB, C.D65))
        want = lin if linear else C.srgb_encode(lin)
        err = np.abs(px - want).max()
        assert err <= (4e-6 * np.abs(want).max() if linear else 2e-4), (linear, err)
        alone = stage_alone(data, np.ascontiguousarray(dc.reshape(3, -1)), linear, frame=lambda f: f.set_linear_output(linear)).reshape(px.shape)
        print("%s: max |reduced - reading| = %.3g, max |reduced - stage alone| = %.3g" % ("linear" if linear else "sRGB", err, np.abs(px - alone).max()))
        assert np.abs(px - alone).max() <= (4e-6 * np.abs(want).max() if linear else 2e-4)
    # a PQ BT.2100 stream, rendered to its own encoding (the generic writer's colour target)
    name = "pq_10000"
    T = A.tagged(J, name, lambda: J.encode_rgb8(img))
    _, p, wp, tf, _ = A.ENCODINGS[name]
    it = A.intensity(name)
    px, dc = _reduced(J, T, keep_dc=True, frame=lambda f: f.set_color_output())
    want = C.render(C.output_matrix(p, wp, it) @ C.xyb_to_mixed(dc.reshape(3, -1).astype(np.float64)), tf, it, tf, p=p, w=wp).T.reshape(px.shape)
    err = np.abs(px - want).max()
    assert err <= 2e-4, err
    assert np.abs(px - _f32(J, w, h)).max() > 0.05  # (the target is applied: not the sRGB rendering)
    t = A.color_output(L, _ce_of(name), it, _ce_of(name))
    alone = stage_alone(T, np.ascontiguousarray(dc.reshape(3, -1)), target=t).reshape(px.shape)
    print("PQ: max |reduced - reading| = %.3g, max |reduced - stage alone| = %.3g" % (err, np.abs(px - alone).max()))
    assert np.abs(px - alone).max() <= 2e-4
    # a grey stream: luminance rows
    J.set_xyb_gray(True)
    try:
        G = J.encode_rgb8(img)
    finally:
        J.set_xyb_gray(False)
    px3, dc = _reduced(J, G, (0, 3), keep_dc=True, frame=lambda f: f.set_color_output())
    px1, _ = _reduced(J, G, (0, 1), frame=lambda f: f.set_color_output())
    assert px1.shape == (35, 51, 1) and np.array_equal(px1[..., 0].view(np.uint32), px3[..., 0].view(np.uint32))
    want = C.srgb_encode(_reading(dc, C.output_matrix(C.SRGB, C.D65)) @ LUMA)
    err = np.abs(px1[..., 0] - want).max()
    print("grey: max |reduced - reading| = %.3g" % err)
    assert err <= 2e-4
    assert np.abs(px3[..., 0] - px3[..., 1]).max() <= 1e-6 and np.abs(px3[..., 0] - px3[..., 2]).max() <= 1e-6


@pytest.mark.parametrize("case", [("u8", 2, 8, 1), ("u16", 3, 16, 1), ("f16", 5, 16, 1), ("u8", 2, 8, 5), ("u16", 3, 16, 6), ("f16", 5, 16, 6),
                                  ("u8", 2, 8, 6)], ids=lambda c: "%s-o%d" % (c[0], c[3]))
def test_writer_formats_and_orientations(built, case):
    """u8 (dithered at the reduced position), u16, f16 and orientations 5 and 6 against tests/writer_np.py on the f32 reduced
    image, exactly, as test_gpu_writer.py holds the full-size writer."""
    J = built
    name, dt, bits, orientation = case
    for (w, h) in ((403, 277), (24, 24)):
        v = _f32(J, w, h)
        got, _ = _reduced(J, _stream(J, w, h), (dt, 3), orientation)
        want = W.write(v, name, bits, orientation)
        assert got.shape == want.shape and got.dtype == want.dtype
        bad = got.view(np.uint16 if name == "f16" else got.dtype) != want.view(np.uint16 if name == "f16" else want.dtype)
        assert not bad.any(), "%s %dx%d o%d: %d samples differ" % (name, w, h, orientation, int(bad.sum()))
    # two and four channels: the reduced image is opaque colour
    f = J.Frame(_stream(J, 24, 24), reduced=True)
    c = J.HipContext()
    try:
        c.set_output_format(0, 4)
        with pytest.raises(J.JxlAmdError, match=r"failed \(4\)"):
            c.upload_reduced(f)
    finally:
        c.close()
        f.close()


@pytest.mark.parametrize("case", [(torch.float16, "CHW", False, True), (torch.bfloat16, "HWC", False, False), (torch.uint8, "CHW", False, False),
                                  (torch.float32, "CHW", True, True)], ids=lambda c: "%s-%s%s" % (str(c[0]).split(".")[1], c[1], "-padded" if c[2] else ""))
def test_tensor_bindings(built, case):
    """CHW f16 with mean / std, HWC bf16, u8 and a padded pitch against the NumPy line of test_gpu_tensor_out.py on the f32
    reduced image, bit for bit, the whole allocation: what lies outside the image keeps its sentinel."""
    J = built
    dtype, layout, padded, normalise = case
    w, h = 403, 277
    v = _f32(J, w, h)
    mean, std, clamp = (MEAN, STD, True) if normalise else (None, None, False)
    cv = Canvas(dtype, layout, 3, v.shape[0], v.shape[1], padded)
    _reduced(J, _stream(J, w, h), bind=lambda c: torch_io.bind(c, cv.tensor, layout, mean, std, clamp))
    if dtype == torch.uint8:
        want = W.write(v, "u8", 8, 1)
    else:
        want = _formula(v, torch_io.affine(mean, std, 3), clamp, dtype)
    _same(cv.got(), cv.expect(want), "reduced %s %s" % (dtype, layout))


@pytest.mark.parametrize("case", [((5, 7), None), ((13, 21), None), ((8, 8), (3, 2, 20, 11)), ((35, 51), None)], ids=lambda c: "%dx%d%s" % (c[0][1], c[0][0], "-box" if c[1] else ""))
def test_resized_binding(built, case):
    """The 403 x 277 stream's reduced image (51 x 35) to 7 x 5, to 21 x 13 and box (3, 2, 20, 11) -> 8 x 8 against
    tests/resample_f64.py's resize within its own bar, on the f32 reduced image; the identity size is bit-exact."""
    J = built
    (oh, ow), box = case
    v = _f32(J, 403, 277)
    assert v.shape == (35, 51, 3)
    out = torch.full((3, oh, ow), float("nan"), dtype=torch.float32, device="cuda")
    _reduced(J, _stream(J, 403, 277), bind=lambda c: torch_io.bind_resized(c, out, "CHW", box))
    torch.cuda.synchronize()
    got = out.cpu().numpy().transpose(1, 2, 0)
    if (oh, ow) == (35, 51):
        assert np.array_equal(got.view(np.uint32), v.view(np.uint32))
        return
    want, bar = R.resize(v, oh, ow, box), R.bar(v, oh, ow, box)
    err = np.abs(got - want).max()
    print("resized %dx%d: %.3f of the bar" % (ow, oh, err / bar))
    assert err <= bar
    if box is not None:  # (the box is in reduced-image coordinates: one sample off is far outside the bar)
        assert np.abs(R.resize(v, oh, ow, (box[0] + 1, box[1], box[2], box[3])) - want).max() > 10 * bar


def _batch_members(J):
    """Seven contexts' worth: the six shapes and a grey stream, with mixed output bindings."""
    J.set_xyb_gray(True)
    try:
        grey = _cached(("grey", 96, 64), lambda: J.encode_rgb8(J.synth_image(96, 64, seed=9)))
    finally:
        J.set_xyb_gray(False)
    datas = [_stream(J, w, h, "lf_cmap" if (w, h) == (2300, 300) else "default") for (w, h) in SHAPES] + [grey]
    kinds = ["f32", "u8", "f16_tensor", "resized", "f32", "resized_box", "grey1"]
    return datas, kinds


def _run_members(J, datas, kinds, together):
    """-> per member, its output as a NumPy array. together: one run_reduced_batch; else each alone."""
    frames, ctxs, outs, tensors = [], [], [], []
    try:
        for data, kind in zip(datas, kinds):
            f = J.Frame(data, reduced=True)
            frames.append(f)
            c = J.HipContext()
            ctxs.append(c)
            xb, yb = f.reduced_size()
            t = None
            if kind == "grey1":
                f.set_color_output()
                c.set_output_format(0, 1)
            elif kind == "f32":
                c.set_output_format(0, 3)
            elif kind == "u8":
                c.set_output_format(2, 3)
            elif kind == "f16_tensor":
                t = torch.zeros((3, yb, xb), dtype=torch.float16, device="cuda")
                torch_io.bind(c, t, "CHW", MEAN, STD, True)
            elif kind == "resized":
                t = torch.zeros((3, 2, 5), dtype=torch.float32, device="cuda")
                torch_io.bind_resized(c, t, "CHW", None)
            else:
                t = torch.zeros((3, 16, 16), dtype=torch.float32, device="cuda")
                torch_io.bind_resized(c, t, "CHW", (100, 3, 150, 30))
            tensors.append(t)
            c.upload_reduced(f)
            if not together:
                c.run_reduced()
        if together:
            J.run_reduced_batch(ctxs)
        torch.cuda.synchronize()
        for c, t in zip(ctxs, tensors):
            if t is None:
                outs.append(c.pixels())
            else:
                c.sync()
                outs.append(t.cpu().view(torch.int16 if t.dtype == torch.float16 else torch.int32).numpy())
        guards = [c.check_guards() for c in ctxs]
        return outs, guards
    finally:
        for c in ctxs:
            c.close()
        for f in frames:
            f.close()


def test_batch_of_seven_equals_each_alone(built, monkeypatch):
    """Seven contexts (the six shapes and a grey stream; f32, u8, an f16 tensor, two resized bindings, one channel) in one
    run_reduced_batch equal each alone, bit for bit; a batch of one equals run_reduced; under JXLHIP_GUARD=1 with two fill
    patterns no guard band of any context is touched and the results do not move."""
    J = built
    datas, kinds = _batch_members(J)
    alone, _ = _run_members(J, datas, kinds, False)
    both, _ = _run_members(J, datas, kinds, True)
    for kind, a, b in zip(kinds, alone, both):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), kind
    one, _ = _run_members(J, datas[4:5], ["f32"], True)
    assert np.array_equal(one[0].view(np.uint32), alone[4].view(np.uint32))
    assert np.array_equal(alone[0].view(np.uint32), _f32(J, 8, 8).view(np.uint32))
    monkeypatch.setenv("JXLHIP_GUARD", "1")
    for fill in ("0xA5", "0x00"):
        monkeypatch.setenv("JXLHIP_GUARD_BYTE", fill)
        guarded, touched = _run_members(J, datas, kinds, True)
        assert touched == [0] * len(kinds), (fill, touched)
        for kind, a, b in zip(kinds, alone, guarded):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (fill, kind)


def test_prefix_and_context_state(built):
    """The decode of data[:need] equals the decode of data; every stage of the full route answers with its code on a context
    that holds a reduced upload and leaves the reduced image as it was; run_reduced on a context that holds a whole frame is
    refused; a whole upload + run_all afterwards on the same context equals a fresh context's."""
    J = built
    L = J.lib()
    data = _stream(J, 403, 277)
    need = J.frame_dc_extent(data)
    assert need < len(data) // 4
    want = _f32(J, 403, 277)
    got, _ = _reduced(J, data[:need])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    got, _ = _reduced(J, data, whole=True)  # (a whole parse holds the same DC)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(J.decode_reduced(data[:need], 0, 3).view(np.uint32), want.view(np.uint32))
    L.jxlhip_halo_rows.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    L.jxlhip_canvas_create.argtypes = [ctypes.c_int] + [ctypes.c_uint32] * 4 + [ctypes.POINTER(ctypes.c_void_p)]
    L.jxlhip_canvas_destroy.argtypes = [ctypes.c_void_p]
    L.jxlhip_canvas_save_xyb.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    fr = J.Frame(data[:need], reduced=True)
    ff = J.Frame(data)
    c = J.HipContext()
    fresh = J.HipContext()
    canvas = ctypes.c_void_p()
    try:
        c.set_output_format(0, 3)
        c.upload_reduced(fr)
        c.run_reduced()
        arr = (ctypes.c_void_p * 1)(c._h)
        rows = ctypes.c_uint32()
        assert L.jxlhip_canvas_create(0, 51, 35, 0, 0, ctypes.byref(canvas)) == 0
        codes = {
            "run_entropy": L.jxlhip_run_entropy(c._h), "run_transform": L.jxlhip_run_transform(c._h),
            "run_filter_color": L.jxlhip_run_filter_color(c._h), "run_all": L.jxlhip_run_all(c._h),
            "run_entropy_batch": L.jxlhip_run_entropy_batch(arr, 1), "run_transform_batch": L.jxlhip_run_transform_batch(arr, 1),
            "run_filter_color_batch": L.jxlhip_run_filter_color_batch(arr, 1), "halo_rows": L.jxlhip_halo_rows(c._h, ctypes.byref(rows)),
            "canvas_save_xyb": L.jxlhip_canvas_save_xyb(canvas, c._h, 0),
            "download_coeffs": L.jxlhip_download(c._h, b"coeffs", None, 0, None),
            "download_xyb_idct": L.jxlhip_download(c._h, b"xyb_idct", None, 0, None),
            "upload_band": L.jxlamd_frame_upload_band(fr._h, c._h, 0, 1),
        }
        assert all(v in (1, 4) for v in codes.values()), codes  # JXLHIP_ERR_INVALID_ARGUMENT or _UNSUPPORTED
        assert np.array_equal(c.pixels().view(np.uint32), want.view(np.uint32))  # untouched
        # a whole frame on the same context: an ordinary context again
        c.upload(ff)
        L.jxlhip_reduced_run.argtypes = [ctypes.c_void_p]
        assert L.jxlhip_reduced_run(c._h) == 1
        c.run_all()
        fresh.set_output_format(0, 3)
        fresh.upload(ff)
        fresh.run_all()
        a, b = c.pixels(), fresh.pixels()
        assert a.shape == (277, 403, 3) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        # and back
        c.upload_reduced(ff)
        c.run_reduced()
        assert np.array_equal(c.pixels().view(np.uint32), want.view(np.uint32))
        # output settings changed after the upload: upload again
        c.set_output_format(2, 3)
        with pytest.raises(J.JxlAmdError):
            c.run_reduced()
    finally:
        if canvas:
            L.jxlhip_canvas_destroy(canvas)
        c.close()
        fresh.close()
        fr.close()
        ff.close()


def test_definition_against_block_means_of_the_source(built):
    """Guards against an offset or half-block shift, independently of every decoder: a smooth 200 x 120 image at d1.0; the
    linear-light reduced output against the 8x8 means of the linearised source over the blocks that lie wholly inside the
    image. Measured on the CPU with the oracle's DC and the float64 colour reading: rms 0.00164, max 0.00785; the source
    shifted by (1, 1) gives rms 0.0097, by 4 pixels 0.017. Condition: rms <= 0.004 (2.4x the reference's own value, 2.4x
    below the nearest wrong answer)."""
    J = built
    y, x = np.mgrid[0:120, 0:200].astype(np.float64)
    src = np.stack([0.5 + 0.4 * np.sin(x / 37) * np.cos(y / 23), 0.5 + 0.4 * np.cos(x / 51 + y / 40), 0.3 + 0.25 * np.sin((x + 2 * y) / 60)], -1)
    u8 = np.rint(src * 255).astype(np.uint8)
    data = J.encode_rgb8(u8, distance=1.0)
    got, _ = _reduced(J, data, frame=lambda f: f.set_linear_output(True))
    assert got.shape == (15, 25, 3)
    s = u8.astype(np.float64) / 255
    lin = np.where(s <= 0.04045, s / 12.92, ((s + 0.055) / 1.055) ** 2.4)
    means = lin.reshape(15, 8, 25, 8, 3).mean(axis=(1, 3))
    d = got.astype(np.float64) - means
    rms, worst = float(np.sqrt((d ** 2).mean())), float(np.abs(d).max())
    print("definition: rms %.5f, max %.5f" % (rms, worst))
    assert rms <= 0.004


def test_torch_io_reduce(built):
    """decode_to_tensor(data, reduce=8) has shape (3, 35, 51) and holds the tensor formula of the f32 reduced image;
    decode_batch_to_tensor(prefixes, size=(16, 16), reduce=8, boxes=...) on non-default streams equals the per-frame
    results; a stream the reduced parse refuses raises with the parser's text."""
    J = built
    data = _stream(J, 403, 277)
    v = _f32(J, 403, 277)
    t = torch_io.decode_to_tensor(data, dtype=torch.float16, mean=MEAN, std=STD, clamp=True, reduce=8)
    torch.cuda.synchronize()
    assert tuple(t.shape) == (3, 35, 51)
    want = _formula(v, torch_io.affine(MEAN, STD, 3), True, torch.float16)
    _same(t.cpu().view(torch.int16).numpy().transpose(1, 2, 0), want, "decode_to_tensor reduce=8")
    streams = [_stream(J, 403, 277, "d3_epf3"), _stream(J, 2300, 300, "lf_cmap"), _stream(J, 403, 277, "no_smoothing_cmap")]
    prefixes = [s[:J.frame_dc_extent(s)] for s in streams]
    boxes = [None, (0, 0, 8, 8), (3, 2, 20, 11)]
    batch = torch_io.decode_batch_to_tensor(prefixes, size=(16, 16), reduce=8, boxes=boxes, dtype=torch.float32)
    torch.cuda.synchronize()
    assert tuple(batch.shape) == (3, 3, 16, 16)
    for i, (s, box) in enumerate(zip(streams, boxes)):
        one = torch_io.decode_to_tensor(s, dtype=torch.float32, size=(16, 16), box=box, reduce=8)
        torch.cuda.synchronize()
        assert torch.equal(batch[i].view(torch.int32), one.view(torch.int32)), i
    same_size = torch_io.decode_batch_to_tensor([streams[0], streams[2]], reduce=8, dtype=torch.float32)
    torch.cuda.synchronize()
    assert tuple(same_size.shape) == (2, 3, 35, 51)
    ref, _ = _reduced(J, streams[2], (0, 3))
    assert np.array_equal(same_size[1].cpu().numpy().transpose(1, 2, 0).view(np.uint32), ref.view(np.uint32))
    with pytest.raises(J.JxlAmdError, match="reduced decode: the frame is upsampled"):
        torch_io.decode_to_tensor(J.encode_rgb8(J.synth_image(64, 64, seed=1), upsampling=2), reduce=8)
    with pytest.raises(ValueError):
        torch_io.decode_to_tensor(data, reduce=4)
