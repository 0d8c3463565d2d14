"""GPU tests (-m gpu) of cropping and resizing on the device while decoding into caller tensors (jxlhip_set_output_resized,
jxlhip_debug_resample, libjxl_amd.torch_io.bind_resized / decode_*(size=...)).

The expectation is tests/resample_f64.py, a float64 reading of the semantics that tests/test_resample_host.py holds to
torch's own float64 interpolation, applied to the float32 source: the seeded floats handed to jxlhip_debug_resample, or
pixels() as f32 with the same channel count from a second context decoding the same stream. The bar, for an f32 tensor
with scale 1 and bias 0, tx and ty the largest tap counts of the two axes and u = 2^-24:

    |got - reading| <= (tx + ty + 8) * u * max(1, max |v| over the box)

(n-term float32 sums of convex weights, weights good to u / 2, one rounding between the passes: a priori, not measured).
Other types and an affine: the documented arithmetic on the reading, within the bar times |scale[c]| plus one spacing of
the type there. uint8: rint(clamp(reading * 255)) exactly, except within 255 * bar of a half-integer (+-1 there; at most
0.5 % of a case's samples, checked on the CPU first). Every tensor lives inside a sentinel-filled allocation; what lies
outside the output must keep the sentinel."""
import os

import numpy as np
import pytest
import torch

import resample_f64 as R
from libjxl_amd import torch_io

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_INT = {torch.float16: (torch.int16, np.int16, 0x7B5A), torch.bfloat16: (torch.int16, np.int16, 0x7B5A),
        torch.float32: (torch.int32, np.int32, 0x7B5A7B5A), torch.uint8: (torch.uint8, np.uint8, 0x5A)}
_CACHE = {}
WORST = {}  # the kernels' largest distance in units of the bar, per test (printed; it does not set the bar)


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


class Canvas:
    """A tensor of the output inside a larger sentinel-filled allocation (the helper of tests/test_gpu_tensor_out.py, with a
    read-back that separates the image from what surrounds it)."""

    def __init__(self, dtype, layout, nc, h, w, padded, device="cuda"):
        self.dtype, self.layout = dtype, layout
        it, self.np_int, self.sentinel = _INT[dtype]
        ph, pw = (h + 5, w + 3) if padded else (h, w)
        self.offset = 1 if padded else 0
        self.shape = (nc, ph, pw) if layout == "CHW" else (ph, pw, nc)
        n = self.offset + nc * ph * pw + (2 if padded else 0)
        self.flat = torch.empty(n, dtype=dtype, device=device)
        self.flat.view(it).fill_(self.sentinel if dtype != torch.uint8 else 0x5A)
        self.cut = (slice(None), slice(0, h), slice(0, w)) if layout == "CHW" else (slice(0, h), slice(0, w), slice(None))
        self.tensor = self.flat[self.offset:self.offset + nc * ph * pw].view(self.shape)[self.cut]
        self.it = it

    def got(self):
        torch.cuda.synchronize()
        return self.flat.view(self.it).cpu().numpy()

    def untouched(self):
        return bool((self.got() == self.np_int(self.sentinel)).all())

    def image(self):
        """([H, W, C] integer view of the output, whether everything around it kept the sentinel)."""
        full = self.got().copy()
        n = int(np.prod(self.shape))
        view = full[self.offset:self.offset + n].reshape(self.shape)
        img = view[self.cut].copy()
        view[self.cut] = self.sentinel
        return (img.transpose(1, 2, 0) if self.layout == "CHW" else img), bool((full == self.np_int(self.sentinel)).all())


def _values(bits, dtype):
    """The integer view of a tensor -> its values in float64."""
    if dtype == torch.float32:
        return np.ascontiguousarray(bits).view(np.float32).astype(np.float64)
    if dtype == torch.float16:
        return np.ascontiguousarray(bits).view(np.float16).astype(np.float64)
    if dtype == torch.bfloat16:
        return (np.ascontiguousarray(bits).view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return bits.astype(np.float64)


def _spacing(e, dtype):
    """One spacing of the type at |e| (float64 array)."""
    a = np.abs(e)
    if dtype == torch.float32:
        return np.spacing(a.astype(np.float32)).astype(np.float64)
    if dtype == torch.float16:
        return np.spacing(np.minimum(a, 65000.0).astype(np.float16)).astype(np.float64)
    exp = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))  # bfloat16: 8 bits of significand
    return 2.0 ** (exp - 7)


def _check(cv, src, out_h, out_w, box, mean, std, clamp, what):
    """The canvas against the reading of src ([H, W, C] float32) by the rules of the module's docstring."""
    nc = src.shape[2]
    reading = R.resize(src, out_h, out_w, box)
    bar = R.bar(src, out_h, out_w, box)
    bits, clean = cv.image()
    assert clean, "%s: something outside the output was written" % what
    assert bits.shape == (out_h, out_w, nc), what
    if cv.dtype == torch.uint8:
        t = reading * 255.0
        want = np.rint(np.clip(t, 0.0, 255.0))
        near = np.abs(t - np.floor(t) - 0.5) <= 255.0 * bar
        assert near.mean() <= 0.005, "%s: %.3f %% of the samples lie within the bar of a half-integer" % (what, 100 * near.mean())
        d = np.abs(bits.astype(np.float64) - want)
        assert (d[~near] == 0).all() and (d <= 1).all(), "%s: %d samples differ away from a half-integer, max %g" % (
            what, int((d[~near] != 0).sum()), d.max())
        return
    scale, bias = torch_io.affine(mean, std, nc)
    e = np.clip(reading, 0.0, 1.0) if clamp else reading
    e = e * scale.astype(np.float64) + bias.astype(np.float64)
    got = _values(bits, cv.dtype)
    plain = cv.dtype == torch.float32 and mean is None and std is None and not clamp
    allowed = bar * np.abs(scale.astype(np.float64)) + (0.0 if plain else _spacing(e, cv.dtype))
    d = np.abs(got - e)
    assert not np.isnan(got).any(), "%s: NaN in the output" % what
    worst = float((d / allowed).max())
    if plain:
        WORST[what] = float(d.max() / bar)
        print("%s: %.3f of the bar" % (what, WORST[what]))
    assert worst <= 1.0, "%s: %.3g of the allowed distance (bar %.3g) at %s" % (what, worst, bar, np.unravel_index(np.argmax(d / allowed), d.shape))


def _debug(J, src, out_h, out_w, dtype=torch.float32, layout="CHW", padded=False, box=None, mean=None, std=None, clamp=False, what=""):
    nc = src.shape[2]
    cv = Canvas(dtype, layout, nc, out_h, out_w, padded)
    c = J.HipContext()
    try:
        class Rec:  # (records the descriptor torch_io.bind_resized makes of the tensor, for the raw entry)
            def set_output_resized(self, *a):
                self.a = a
        rec = Rec()
        torch_io.bind_resized(rec, cv.tensor, layout, box, mean, std, clamp)
        ptr, room, dt, _, strides, out_size, bx, scale, bias, cl, stream = rec.a
        c.debug_resample(src, ptr, room, dt, strides, out_size, bx, scale, bias, cl, stream)
    finally:
        c.close()
    _check(cv, src, out_h, out_w, box, mean, std, clamp, what or "%dx%d->%dx%d nc %d %s" % (src.shape[1], src.shape[0], out_w, out_h, nc, layout))
    return cv


def _floats(h, w, nc, seed):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, (h, w, nc)).astype(np.float32)


# (in_h, in_w, out_h, out_w, nc, layout, padded): every nc and both layouts appear; 600 -> 7 is a tap row of 172, longer
# than the 64-column tile; 5x600 -> 3x7 has it on the other axis; 300x520 -> 224x224 needs several tiles on both axes
PASSES = [
    (1, 1, 4, 4, 1, "CHW", False),
    (1, 17, 3, 5, 2, "HWC", True),
    (8, 8, 13, 21, 3, "CHW", True),
    (5, 600, 3, 7, 4, "HWC", False),
    (600, 5, 7, 3, 3, "CHW", False),
    (263, 257, 29, 31, 2, "CHW", True),
    (520, 300, 224, 224, 3, "HWC", True),
    (300, 520, 224, 224, 4, "CHW", False),
]


@pytest.mark.parametrize("case", PASSES, ids=lambda c: "%dx%d-%dx%d-nc%d-%s" % (c[1], c[0], c[3], c[2], c[4], c[5]))
def test_passes_alone(built, case):
    """jxlhip_debug_resample on seeded floats in [-0.1, 1.1], f32 with scale 1 and bias 0: inside the bar, sentinel intact."""
    h, w, oh, ow, nc, layout, padded = case
    _debug(built, _floats(h, w, nc, seed=h * 7 + w), oh, ow, torch.float32, layout, padded)


def test_identity_is_bit_exact(built):
    """64 x 64 -> 64 x 64: every row of both tables is the weights (1, 0), and the f32 output is the source bit for bit."""
    src = _floats(64, 64, 3, seed=64)
    for layout in ("CHW", "HWC"):
        cv = _debug(built, src, 64, 64, torch.float32, layout, True)
        bits, _ = cv.image()
        assert np.array_equal(bits, src.view(np.int32))


BOXES = [(0, 0, 200, 120), (320, 0, 200, 120), (0, 180, 200, 120), (320, 180, 200, 120), (519, 299, 1, 1), (77, 33, 1, 1)]


@pytest.mark.parametrize("box", BOXES, ids=lambda b: "%d_%d_%dx%d" % b)
def test_boxes_at_the_corners_and_of_one_pixel(built, box):
    """Boxes at each corner of a 520 x 300 source and boxes of a single pixel; outside the box the source is NaN, which must
    not reach the output (samples outside the box do not exist)."""
    src = _floats(300, 520, 3, seed=11)
    x0, y0, bw, bh = box
    poisoned = np.full_like(src, np.nan)
    poisoned[y0:y0 + bh, x0:x0 + bw] = src[y0:y0 + bh, x0:x0 + bw]
    clean = np.where(np.isnan(poisoned), np.float32(0), poisoned)  # (the reading never looks outside the box either)
    assert np.array_equal(R.resize(clean, 17, 33, box), R.resize(src, 17, 33, box))
    cv = Canvas(torch.float32, "CHW", 3, 17, 33, True)
    c = built.HipContext()
    try:
        c.debug_resample(poisoned, cv.tensor.data_ptr(), (cv.flat.numel() - cv.offset) * 4, built.TENSOR_F32, tuple(cv.tensor.stride()),
                         (33, 17), box)
    finally:
        c.close()
    _check(cv, clean, 17, 33, box, None, None, False, "box %r" % (box,))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.uint8], ids=lambda d: str(d).split(".")[1])
def test_every_dtype_with_mean_std_and_clamp(built, dtype):
    """257 x 263 -> 31 x 29 into each type: the float types with mean, std and clamp (and f16 also plain), uint8 undithered."""
    src = _floats(263, 257, 3, seed=5)
    if dtype == torch.uint8:
        t = R.resize(src, 29, 31) * 255.0  # (the seed keeps the reading itself away from half-integers: checked before the GPU run)
        assert (np.abs(t - np.floor(t) - 0.5) <= 255.0 * R.bar(src, 29, 31)).mean() <= 0.005
        for layout in ("CHW", "HWC"):
            _debug(built, src, 29, 31, dtype, layout, True, what="u8 " + layout)
        return
    _debug(built, src, 29, 31, dtype, "CHW", True, None, MEAN, STD, True, what="%s affine" % dtype)
    _debug(built, src, 29, 31, dtype, "HWC", False, (3, 5, 250, 255), MEAN, STD, False, what="%s affine box" % dtype)
    if dtype == torch.float16:
        _debug(built, src, 29, 31, dtype, "CHW", False, what="f16 plain")


def test_guard_bands_stay_clean(built, monkeypatch):
    """JXLHIP_GUARD=1: the two passes write next to none of the context's buffers (source, intermediate, tables)."""
    J = built
    monkeypatch.setenv("JXLHIP_GUARD", "1")
    src = _floats(263, 257, 2, seed=9)
    cv = Canvas(torch.float32, "CHW", 2, 29, 31, True)
    c = J.HipContext()
    try:
        c.debug_resample(src, cv.tensor.data_ptr(), (cv.flat.numel() - cv.offset) * 4, J.TENSOR_F32, tuple(cv.tensor.stride()), (31, 29),
                         (1, 2, 255, 260))
        assert c.check_guards() == 0
    finally:
        c.close()
    _check(cv, src, 29, 31, (1, 2, 255, 260), None, None, False, "guards")


# ------------------------------------------------------------------------------------------------ through the decoder
def _set_alpha(J, c, alpha):
    import ctypes
    L = J.lib()
    L.jxlhip_set_alpha.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
    a = np.ascontiguousarray(alpha, np.float32)
    assert L.jxlhip_set_alpha(c._h, a.ctypes.data, a.shape[1], a.shape[0]) == 0


def _decode(J, data, nc, modular, prepare=None, bind=None):
    """One decode on a fresh context: into what bind(ctx) bound, or pixels() as f32 with nc channels. -> (route, pixels)."""
    f = J.ModFrame(data) if modular else J.Frame(data)
    c = J.HipContext()
    try:
        if prepare:
            prepare(c, f)
        if bind:
            bind(c)
        else:
            c.set_output_format(0, nc)
        if modular:
            c.upload_modular(f)
            c.run_modular()
            r, status, _ = c.modular_status()
            assert r == 0 and not any(status)
            route = None
        else:
            c.upload(f)
            c.run_all()
            r, flags = c.errors()
            assert r == 0 and not any(flags)
            route = c.pixel_route()
        return route, (None if bind else c.pixels())
    finally:
        c.close()
        f.close()


def _rgba_case(J):
    xs, ys = 121, 37
    rgb = J.synth_image(xs, ys, seed=5)
    alpha = ((np.mgrid[0:ys, 0:xs][0] * 5 + np.mgrid[0:ys, 0:xs][1] * 3) & 255).astype(np.uint8)
    return J.encode_rgba8(np.dstack([rgb, alpha]), epf_iters=1), alpha.astype(np.float32) / np.float32(255)


def _decoder_cases(J):
    rgba, alpha = _cached("rgba", lambda: _rgba_case(J))
    return {
        # name: (stream, channels, Modular, prepare, the route of the f32 pixels or None)
        "rows_epf1": (lambda: J.encode_rgb8(J.synth_image(520, 300, seed=820), epf_iters=1), 3, False, None, 1),
        "rows_epf2": (lambda: J.encode_rgb8(J.synth_image(520, 300, seed=820), epf_iters=2), 3, False, None, 1),
        "generic_rgba": (lambda: rgba, 4, False, lambda c, f: _set_alpha(J, c, alpha), 0),
        "upsampling2": (lambda: J.encode_rgb8(J.synth_image(121, 37, seed=158), upsampling=2), 3, False, None, 0),
        "orientation6": (lambda: J.encode_rgb8(J.synth_image(71, 45, seed=116), epf_iters=1), 3, False, lambda c, f: c.set_output_orientation(6), 0),
        "modular_rgb": (lambda: J.encode_lossless(J.synth_image(264, 40, seed=11)), 3, True, None, None),
        "modular_rgba": (lambda: open(os.path.join(ROOT, "tests", "golden", "fjxl_d10_280x36_rgba_e2.jxl"), "rb").read(), 4, True, None, None),
    }


@pytest.mark.parametrize("name", ["rows_epf1", "rows_epf2", "generic_rgba", "upsampling2", "orientation6", "modular_rgb", "modular_rgba"])
def test_through_the_decoder(built, name):
    """Each pixel route, to 224 x 224 (whole image) and to 33 x 17 with a box: the f32 tensor is the reading of pixels() as
    f32 from a second context on the same stream, inside the bar; the context renders by the route that makes those pixels."""
    J = built
    make, nc, modular, prepare, want_route = _decoder_cases(J)[name]
    data = _cached(("stream", name), make)
    route_ref, v = _cached(("ref", name), lambda: _decode(J, data, nc, modular, prepare))
    h, w = v.shape[:2]
    if name == "orientation6":
        assert (h, w) == (71, 45)  # rows of the output are columns of the image: the box is in these coordinates
    assert route_ref == want_route
    for (oh, ow), box in (((224, 224), None), ((17, 33), (w // 5, h // 7, w // 2, h // 2))):
        for layout, padded in (("CHW", True), ("HWC", False)):
            cv = Canvas(torch.float32, layout, nc, oh, ow, padded)
            route, _ = _decode(J, data, nc, modular, prepare, bind=lambda c: torch_io.bind_resized(c, cv.tensor, layout, box))
            assert route == want_route, (route, want_route)
            _check(cv, v, oh, ow, box, None, None, False, "%s -> %dx%d %s" % (name, ow, oh, layout))


def test_one_shot_entry_with_a_size(built):
    """decode_to_tensor(size=...) finds the frame kind itself, allocates (C, h, w), takes a given `out` of that size and still
    refuses an `out` of another size; f16 with mean / std against the documented arithmetic on the reading."""
    J = built
    make, nc, modular, prepare, _ = _decoder_cases(J)["modular_rgb"]
    data = _cached(("stream", "modular_rgb"), make)
    _, v = _cached(("ref", "modular_rgb"), lambda: _decode(J, data, nc, modular, prepare))
    cv = Canvas(torch.float16, "CHW", 3, 20, 50, True)
    out = torch_io.decode_to_tensor(data, layout="CHW", mean=MEAN, std=STD, clamp=True, out=cv.tensor, size=(20, 50), box=(4, 2, 200, 30))
    assert out is cv.tensor
    _check(cv, v, 20, 50, (4, 2, 200, 30), MEAN, STD, True, "decode_to_tensor")
    t = torch_io.decode_to_tensor(data, dtype=torch.float32, layout="HWC", size=(20, 50))
    assert tuple(t.shape) == (20, 50, 3) and t.dtype == torch.float32
    with pytest.raises(ValueError):
        torch_io.decode_to_tensor(data, out=cv.tensor, size=(21, 50))
    with pytest.raises(ValueError):  # (without size: today's rule, the tensor must have the image's size)
        torch_io.decode_to_tensor(data, out=cv.tensor)


# -------------------------------------------------------------------------------------------------------------- batch
def test_batch_of_mixed_frames_on_a_side_stream(built):
    """decode_batch_to_tensor(size=(64, 64)) over three VarDCT sizes and two Modular sizes, boxes on two of them, on a
    non-default torch stream with a consumer (a clone) queued behind it and no synchronisation in between: the clone equals
    the five single decodes bit for bit, and the first of them is inside the bar."""
    J = built
    datas = _cached("batch", lambda: [J.encode_rgb8(J.synth_image(520, 300, seed=1), epf_iters=1),
                                      J.encode_rgb8(J.synth_image(264, 136, seed=2), epf_iters=2),
                                      J.encode_rgb8(J.synth_image(100, 100, seed=3), epf_iters=0),
                                      J.encode_lossless(J.synth_image(264, 40, seed=4)),
                                      J.encode_lossless(J.synth_image(121, 37, seed=5))])
    boxes = [None, (10, 20, 200, 100), None, (64, 0, 200, 40), None]
    singles = []
    for d, b in zip(datas, boxes):
        singles.append(torch_io.decode_to_tensor(d, dtype=torch.float16, mean=MEAN, std=STD, clamp=True, size=(64, 64), box=b))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = torch.full((5, 3, 64, 64), float("nan"), dtype=torch.float16, device="cuda")
        got = torch_io.decode_batch_to_tensor(datas, out=out, dtype=torch.float16, mean=MEAN, std=STD, clamp=True, size=(64, 64), boxes=boxes)
        copy = got.clone()  # the consumer, behind the decode on `side` with nothing in between
    torch.cuda.synchronize()
    assert got is out and not torch.isnan(copy).any()
    for i, one in enumerate(singles):
        a, b = copy[i].view(torch.int16).cpu().numpy(), one.view(torch.int16).cpu().numpy()
        assert np.array_equal(a, b), "frame %d: %d elements differ from the single decode" % (i, int((a != b).sum()))
    _, v = _decode(J, datas[1], 3, False)
    cv = Canvas(torch.float16, "CHW", 3, 64, 64, False)
    cv.flat.copy_(copy[1].reshape(-1))
    _check(cv, v, 64, 64, boxes[1], MEAN, STD, True, "batch frame 1")
    with pytest.raises(ValueError):
        torch_io.decode_batch_to_tensor(datas, size=(64, 64), boxes=boxes[:2])
    with pytest.raises(ValueError):  # (without size: frames of one size only, as before)
        torch_io.decode_batch_to_tensor(datas[:2])


# ----------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(built):
    """A refused binding, upload or call is an error code and no launch: the tensor keeps its sentinel."""
    J = built
    xs, ys = 121, 37
    data = _cached("small", lambda: J.encode_rgb8(J.synth_image(xs, ys, seed=158), epf_iters=1))
    cv = Canvas(torch.float32, "CHW", 3, 16, 24, False)
    ptr, room, chw = cv.tensor.data_ptr(), 3 * 16 * 24 * 4, (16 * 24, 24, 1)
    f = J.Frame(data)
    c = J.HipContext()
    try:
        # a box outside the image: taken when it is set (no image yet), found at upload
        c.set_output_resized(ptr, room, J.TENSOR_F32, 3, chw, (24, 16), (100, 0, 22, 37))
        with pytest.raises(J.JxlAmdError, match=r"\(1\)|code 1"):
            c.upload(f)
        with pytest.raises(J.JxlAmdError):  # (no frame to run)
            c.run_all()
        c.sync()
        assert cv.untouched()
        # an output larger than the tensor, an unknown filter, half a box: refused when set
        for kw in (dict(out_size=(25, 16)), dict(out_size=(24, 16), filter=1), dict(out_size=(24, 16), box=(0, 0, 5, 0)), dict(out_size=(0, 16))):
            with pytest.raises(J.JxlAmdError, match="code 1"):
                c.set_output_resized(ptr, room, J.TENSOR_F32, 3, chw, **kw)
        with pytest.raises(J.JxlAmdError, match="code 1"):
            c.debug_resample(np.zeros((8, 8, 3), np.float32), ptr, room, J.TENSOR_F32, chw, (24, 16), (4, 4, 5, 4))
        with pytest.raises(J.JxlAmdError, match="code 1"):  # (the source's channel count is not the tensor's)
            c.debug_resample(np.zeros((8, 8, 2), np.float32), ptr, room, J.TENSOR_F32, chw, (24, 16), num_channels=3)
        assert cv.untouched()
        # a band upload under a resized binding
        tall = J.Frame(_cached("tall", lambda: J.encode_rgb8(J.synth_image(8, 520, seed=4))))
        c.set_output_resized(ptr, room, J.TENSOR_F32, 3, chw, (24, 16))
        with pytest.raises(J.JxlAmdError, match=r"\(4\)"):  # JXLHIP_ERR_UNSUPPORTED
            c.upload(tall, band=(1, 2))
        tall.close()
        assert cv.untouched()
        # a good binding: the downloads of the context's own (private) pixels are refused while it lasts
        c.set_output_resized(ptr, room, J.TENSOR_F32, 3, chw, (24, 16))
        c.upload(f)
        c.run_all()
        for download in (c.rgb8, c.pixels, lambda: c.rgb8_rows(0, 8)):
            with pytest.raises(J.JxlAmdError, match="code 1"):
                download()
        assert J.lib().jxlhip_rgb8_device_ptr(c._h) is None
        c.sync()
        assert not cv.untouched()
        # the two bindings one after the other: the later one holds, the earlier one's memory is not written
        cv_t = Canvas(torch.float32, "CHW", 3, ys, xs, False)
        cv_r = Canvas(torch.float32, "CHW", 3, 16, 24, False)
        c.set_output_tensor(cv_t.tensor.data_ptr(), 3 * ys * xs * 4, J.TENSOR_F32, 3, (ys * xs, xs, 1))
        c.set_output_resized(cv_r.tensor.data_ptr(), room, J.TENSOR_F32, 3, chw, (24, 16))
        with pytest.raises(J.JxlAmdError):  # (the frame was uploaded for another destination: upload again)
            c.run_all()
        c.upload(f)
        c.run_all()
        c.sync()
        assert cv_t.untouched() and not cv_r.untouched()
        cv_r2 = Canvas(torch.float32, "CHW", 3, 16, 24, False)
        c.set_output_resized(cv_r2.tensor.data_ptr(), room, J.TENSOR_F32, 3, chw, (24, 16))
        c.set_output_tensor(cv_t.tensor.data_ptr(), 3 * ys * xs * 4, J.TENSOR_F32, 3, (ys * xs, xs, 1))
        c.upload(f)
        c.run_all()
        c.sync()
        assert cv_r2.untouched() and not cv_t.untouched()
        # unbound: the context's own buffer again, as a fresh context gives it
        c.set_output_resized(None)
        c.upload(f)
        c.run_all()
        fresh = _cached("small rgb8", lambda: J.decode_rgb8(data))
        assert np.array_equal(c.rgb8(), fresh)
        # closed while bound (the context goes to the pool): the next context starts unbound
        cv3 = Canvas(torch.float32, "CHW", 3, 16, 24, False)
        c.set_output_resized(cv3.tensor.data_ptr(), room, J.TENSOR_F32, 3, chw, (24, 16))
        c.close()
        c = J.HipContext()
        c.upload(f)
        c.run_all()
        assert np.array_equal(c.rgb8(), fresh) and cv3.untouched()
    finally:
        c.close()
        f.close()
