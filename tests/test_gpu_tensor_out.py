"""GPU tests (-m gpu) of decoding into caller-owned device tensors (jxlhip_set_output_tensor, libjxl_amd.torch_io).

Every comparison is on bit patterns. The writer's input v is always pixels() as f32, with the same channel count, of a
second context on the same stream data; the expectation is the documented formula applied to it in NumPy: clamp if asked,
v * scale rounded to float32, + bias rounded to float32, then round-to-nearest-even to the type (float16: NumPy's cast;
bfloat16: torch's CPU cast). -0.0f * 1 + 0 is +0.0f, so the formula is applied even for scale 1 / bias 0. Every tensor
lives inside a larger allocation filled with a sentinel pattern, and the whole allocation is compared: what lies outside
the image must keep the sentinel."""
import ctypes
import os

import numpy as np
import pytest
import torch

from libjxl_amd import torch_io

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_INT = {torch.float16: (torch.int16, np.int16, 0x7B5A), torch.bfloat16: (torch.int16, np.int16, 0x7B5A),
        torch.float32: (torch.int32, np.int32, 0x7B5A7B5A), torch.uint8: (torch.uint8, np.uint8, 0x5A)}
_CACHE = {}


def _stream(J, key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _rgb_stream(J, xs, ys, **kw):
    return _stream(J, ("rgb", xs, ys, tuple(sorted(kw.items()))), lambda: J.encode_rgb8(J.synth_image(xs, ys, seed=xs + ys), **kw))


def _bits(values_f32, dtype):
    """float32 array -> the integer view of its round-to-nearest-even conversion to `dtype`."""
    v = np.ascontiguousarray(values_f32, np.float32)
    if dtype == torch.float32:
        return v.view(np.int32)
    if dtype == torch.float16:
        return v.astype(np.float16).view(np.int16)
    return torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy()


def _formula(v, channels_last_scale_bias, clamp, dtype):
    """The documented arithmetic on v ([H, W, C] float32)."""
    scale, bias = channels_last_scale_bias
    v = np.asarray(v, np.float32)
    if clamp:
        v = np.minimum(np.maximum(v, np.float32(0)), np.float32(1))
    t = (v * scale.astype(np.float32)).astype(np.float32)
    t = (t + bias.astype(np.float32)).astype(np.float32)
    return _bits(t, dtype)


class Canvas:
    """A tensor of the image inside a larger sentinel-filled allocation, and the same view over a NumPy copy."""

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

    def expect(self, want_hwc_bits):
        """The whole allocation as integers, were only the image written, with `want` ([H, W, C] integer view) in it."""
        full = np.full(self.flat.numel(), self.sentinel, self.np_int)
        n = int(np.prod(self.shape))
        view = full[self.offset:self.offset + n].reshape(self.shape)
        view[self.cut] = want_hwc_bits.transpose(2, 0, 1) if self.layout == "CHW" else want_hwc_bits
        return full

    def got(self):
        torch.cuda.synchronize()
        return self.flat.view(self.it).cpu().numpy()

    def untouched(self):
        return bool((self.got() == self.np_int(self.sentinel)).all())


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = got != want
    assert not bad.any(), "%s: %d of %d elements differ, first at %s (got %r, want %r)" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), got[bad][0], want[bad][0])


def _set_alpha(J, c, alpha):
    L = J.lib()
    L.jxlhip_set_alpha.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
    a = np.ascontiguousarray(alpha, np.float32)
    assert L.jxlhip_set_alpha(c._h, a.ctypes.data, a.shape[1], a.shape[0]) == 0


def _vardct(J, data, nc=3, prepare=None, bind=None, fmt=(0, None)):
    """One VarDCT decode on a fresh context: into the bound tensor (bind(ctx)), or pixels() in format fmt. -> (route, pixels)."""
    f = J.Frame(data)
    c = J.HipContext()
    try:
        if prepare:
            prepare(c, f)
        if bind:
            bind(c)
        else:
            c.set_output_format(fmt[0], fmt[1] or nc)
        c.upload(f)
        c.run_all()
        r, flags = c.errors()
        assert r == 0 and not any(flags)
        return c.pixel_route(), (None if bind else c.pixels())
    finally:
        c.close()
        f.close()


def _reference(J, key, data, nc, prepare=None):
    return _stream(J, ("ref", key, nc), lambda: _vardct(J, data, nc, prepare))


def _check_vardct(J, key, data, dtype, layout, padded, normalise, nc=3, prepare=None, want_route=None, transposed=False):
    route_ref, v = _reference(J, key, data, nc, prepare)
    h, w = v.shape[:2]
    mean, std, clamp = (MEAN, STD, True) if normalise else (None, None, False)
    cv = Canvas(dtype, layout, nc, h, w, padded)
    route, _ = _vardct(J, data, nc, prepare, bind=lambda c: torch_io.bind(c, cv.tensor, layout, mean, std, clamp))
    if want_route is not None:
        assert route == want_route and route_ref == (1 if want_route == 3 else 0), (route, route_ref)
    else:
        assert route != 3
    _same(cv.got(), cv.expect(_formula(v, torch_io.affine(mean, std, nc), clamp, dtype)), "%s %s %s" % (key, dtype, layout))


# ------------------------------------------------------------------------------------------------------ fused route
@pytest.mark.parametrize("epf", [1, 2])
@pytest.mark.parametrize("size", [(8, 8), (121, 37), (257, 70), (520, 300)])
def test_fused_route(built, size, epf):
    """k_filter_rows2's tensor form: every dtype, contiguous CHW (an odd row pitch at the odd widths: every second row takes
    the element stores) and CHW inside a larger allocation (pitch xs + 3, planes five rows apart, data one element in:
    the parity starts odd), with and without mean / std / clamp. Route 3; every element the formula on the f32 output
    of the same kernel's float writer; everything around the image untouched."""
    J = built
    xs, ys = size
    data = _rgb_stream(J, xs, ys, epf_iters=epf)
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        for padded in (False, True):
            for normalise in (False, True):
                _check_vardct(J, ("fused", xs, ys, epf), data, dtype, "CHW", padded, normalise, want_route=3)


def test_fused_route_linear_target(built):
    """The frame's linear output (what the decoder API's linear target sets on the frame): no curve, the same stores."""
    J = built

    def linear(c, f):
        J.lib().jxlamd_frame_set_linear_output.argtypes = [ctypes.c_void_p, ctypes.c_int]
        J.lib().jxlamd_frame_set_linear_output(f._h, 1)

    data = _rgb_stream(J, 121, 37, epf_iters=1)
    for dtype in (torch.float16, torch.float32):
        _check_vardct(J, "linear", data, dtype, "CHW", True, True, prepare=linear, want_route=3)
    plain, lin = _reference(J, ("fused", 121, 37, 1), data, 3)[1], _reference(J, "linear", data, 3, linear)[1]
    assert np.abs(plain - lin).max() > 0.01  # (the target really changed the samples)


# ---------------------------------------------------------------------------------------------------- generic route
def _orient6(c, f):
    c.set_output_orientation(6)


_GENERIC = {
    "epf0": (lambda J: _rgb_stream(J, 121, 37, epf_iters=0), 3, None),
    "epf3": (lambda J: _rgb_stream(J, 121, 37, epf_iters=3), 3, None),
    "noise": (lambda J: _rgb_stream(J, 300, 270, noise=50), 3, None),
    "upsampling2": (lambda J: _rgb_stream(J, 121, 37, upsampling=2), 3, None),
    "orientation6": (lambda J: _rgb_stream(J, 71, 45, epf_iters=1), 3, _orient6),
}


@pytest.mark.parametrize("case", sorted(_GENERIC))
def test_generic_route_vardct(built, case):
    """k_color_out / k_upsample_color with a tensor: f16 CHW (padded, normalised) and f32 HWC (contiguous, plain)."""
    J = built
    make, nc, prepare = _GENERIC[case]
    data = make(J)
    _check_vardct(J, case, data, torch.float16, "CHW", True, True, nc, prepare)
    _check_vardct(J, case, data, torch.float32, "HWC", False, False, nc, prepare)
    _check_vardct(J, case, data, torch.bfloat16, "HWC", True, True, nc, prepare)
    if case == "orientation6":
        assert _reference(J, case, data, nc, prepare)[1].shape == (71, 45, 3)  # rows of the output are columns of the image


def test_generic_route_rgba(built):
    """Four channels: alpha is channel 3, with scale 1 / bias 0 behind the three normalised colour channels."""
    J = built
    xs, ys = 121, 37
    rgb = J.synth_image(xs, ys, seed=5)
    alpha = ((np.mgrid[0:ys, 0:xs][0] * 5 + np.mgrid[0:ys, 0:xs][1] * 3) & 255).astype(np.uint8)
    data = J.encode_rgba8(np.dstack([rgb, alpha]), epf_iters=1)

    def with_alpha(c, f):
        _set_alpha(J, c, alpha.astype(np.float32) / np.float32(255))

    _check_vardct(J, "rgba", data, torch.float16, "CHW", True, True, 4, with_alpha)
    _check_vardct(J, "rgba", data, torch.float32, "HWC", False, False, 4, with_alpha)
    v = _reference(J, "rgba", data, 4, with_alpha)[1]
    assert np.array_equal(v[..., 3], alpha.astype(np.float32) / np.float32(255))


@pytest.mark.parametrize("layout", ["CHW", "HWC"])
def test_u8_tensor_is_the_generic_writer_s_sample(built, layout):
    """uint8: StorePixel's dithered 8-bit sample, i.e. today's RGBA u8 output (the generic writer), not today's RGB u8
    (the fused kernel's own curve and contracted multiply-add)."""
    J = built
    data = _rgb_stream(J, 121, 37, epf_iters=1)
    want = _stream(J, "u8 rgba", lambda: _vardct(J, data, 4, fmt=(2, 4)))[1][..., :3]
    for padded in (False, True):
        cv = Canvas(torch.uint8, layout, 3, 37, 121, padded)
        route, _ = _vardct(J, data, 3, bind=lambda c: torch_io.bind(c, cv.tensor, layout))
        assert route == 0
        _same(cv.got(), cv.expect(want), "u8 %s" % layout)


# ---------------------------------------------------------------------------------------------------------- Modular
def _modular(J, data, nc, bind=None, fmt=0):
    f = J.ModFrame(data)
    c = J.HipContext()
    try:
        if bind:
            bind(c)
        else:
            c.set_output_format(fmt, nc)
        c.upload_modular(f)
        c.run_modular()
        r, status, _ = c.modular_status()
        assert r == 0 and not any(status)
        return None if bind else c.pixels()
    finally:
        c.close()
        f.close()


@pytest.mark.parametrize("name", ["lossless_rgb8", "fjxl_d10_280x36_rgba_e2"])
def test_modular_frames(built, name):
    """k_modular_output with a tensor: uint8 CHW equals pixels() u8, bf16 HWC (normalised) the formula on pixels() f32."""
    J = built
    if name == "lossless_rgb8":
        data, nc = J.encode_lossless(J.synth_image(121, 37, seed=11)), 3
    else:
        data, nc = open(os.path.join(ROOT, "tests", "golden", name + ".jxl"), "rb").read(), 4
    u8, f32 = _modular(J, data, nc, fmt=2), _modular(J, data, nc, fmt=0)
    h, w = u8.shape[:2]
    for padded in (False, True):
        cv = Canvas(torch.uint8, "CHW", nc, h, w, padded)
        _modular(J, data, nc, bind=lambda c: torch_io.bind(c, cv.tensor, "CHW"))
        _same(cv.got(), cv.expect(u8), name + " u8")
        cv = Canvas(torch.bfloat16, "HWC", nc, h, w, padded)
        _modular(J, data, nc, bind=lambda c: torch_io.bind(c, cv.tensor, "HWC", MEAN, STD, True))
        _same(cv.got(), cv.expect(_formula(f32, torch_io.affine(MEAN, STD, nc), True, torch.bfloat16)), name + " bf16")
    # the one-shot entry finds the frame kind itself
    t = torch_io.decode_to_tensor(data, dtype=torch.uint8, layout="HWC", channels=nc)
    torch.cuda.synchronize()
    _same(t.cpu().numpy(), u8, name + " decode_to_tensor")


# ------------------------------------------------------------------------------------------------------------ batch
def test_batch_into_one_nchw_tensor(built):
    """Three different 257 x 70 frames into one (3, 3, 70, 257) f16 tensor, one launch per stage: each slice equals its
    single-frame tensor decode bit for bit (which test_fused_route holds to the formula), and is the fused route's."""
    J = built
    datas = [J.encode_rgb8(J.synth_image(257, 70, seed=90 + i), distance=1.0 + 0.5 * i) for i in range(3)]
    out = torch_io.decode_batch_to_tensor(datas, dtype=torch.float16, mean=MEAN, std=STD, clamp=True)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (3, 3, 70, 257) and out.dtype == torch.float16
    for i, d in enumerate(datas):
        one = torch_io.decode_to_tensor(d, dtype=torch.float16, mean=MEAN, std=STD, clamp=True)
        torch.cuda.synchronize()
        _same(out[i].view(torch.int16).cpu().numpy(), one.view(torch.int16).cpu().numpy(), "frame %d" % i)
        v = _vardct(J, d, 3)[1]
        _same(one.view(torch.int16).cpu().numpy().transpose(1, 2, 0), _formula(v, torch_io.affine(MEAN, STD, 3), True, torch.float16), "frame %d formula" % i)


# --------------------------------------------------------------------------------------------------------- ordering
@pytest.mark.parametrize("route", ["fused", "generic"])
def test_ordering_against_the_consumer_s_stream(built, route):
    """No host wait anywhere: on a side stream a long sleep, then a NaN fill of the tensor; the decode bound to that stream
    is enqueued while the stream still sleeps; then a clone on that stream. The clone holds the decoded values: a missing
    wait before the writers lets the fill land on top of them (NaN), a missing wait behind them clones the fill (NaN)."""
    J = built
    data = _rgb_stream(J, 257, 70, epf_iters=1 if route == "fused" else 0)
    v = _reference(J, ("order", route), data, 3)[1]
    want = _formula(v, torch_io.affine(None, None, 3), False, torch.float32)
    f = J.Frame(data)
    c = J.HipContext()
    out = torch.zeros((3, 70, 257), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(100_000_000)  # the host runs far ahead of this stream
        out.fill_(float("nan"))
        torch_io.bind(c, out, "CHW")  # stream = the current one: `side`
        c.upload(f)
        c.run_entropy()
        c.run_transform()
        c.run_filter_color()
        copy = out.clone()
    torch.cuda.synchronize()
    assert c.pixel_route() == (3 if route == "fused" else 0)
    got = copy.view(torch.int32).cpu().numpy().transpose(1, 2, 0)
    assert not np.isnan(copy.cpu().numpy()).any(), "the clone saw the fill: an ordering edge is missing"
    _same(got, want, "clone")
    _same(out.view(torch.int32).cpu().numpy().transpose(1, 2, 0), want, "tensor")
    c.close()
    f.close()


# --------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(built):
    """A refused binding or upload is an error code and no launch: the tensor keeps its sentinel. Then the same context,
    unbound, decodes into its own buffer exactly like a fresh one."""
    J = built
    xs, ys = 121, 37
    data = _rgb_stream(J, xs, ys, epf_iters=1)
    fresh = _vardct(J, data, 3, fmt=(2, 3))[1]
    cv = Canvas(torch.float16, "CHW", 3, ys, xs, False)
    f = J.Frame(data)
    c = J.HipContext()
    ptr, room = cv.tensor.data_ptr(), 3 * ys * xs * 2
    chw = (ys * xs, xs, 1)

    def refused(code, bind_args, band=None, at_bind=False):
        if at_bind:
            with pytest.raises(J.JxlAmdError, match="code %d" % code):
                c.set_output_tensor(*bind_args)
            return
        c.set_output_tensor(*bind_args)
        with pytest.raises(J.JxlAmdError, match=r"\(%d\)|code %d" % (code, code)):
            c.upload(f, band=band)
        with pytest.raises(J.JxlAmdError):  # (no frame to run)
            c.run_all()
        c.sync()
        assert cv.untouched()

    refused(1, (ptr, room - 2, J.TENSOR_F16, 3, chw))                        # one element short
    refused(1, (ptr, room, J.TENSOR_F16, 3, (ys * xs, xs - 1, 1)))           # rows overlap
    refused(1, (ptr, room, J.TENSOR_F16, 3, (ys * xs - 1, xs, 1)))           # planes overlap
    refused(1, (ptr, room, J.TENSOR_U8, 3, chw, (2.0, 1.0, 1.0)), at_bind=True)  # uint8 with a scale
    refused(1, (ptr + 1, room, J.TENSOR_F16, 3, chw), at_bind=True)          # misaligned
    refused(1, (ptr, room, J.TENSOR_F16, 3, (ys * xs, xs, 0)), at_bind=True)  # a zero stride
    tall = _stream(J, "tall", lambda: J.encode_rgb8(J.synth_image(8, 520, seed=4)))
    ft = J.Frame(tall)
    tcv = Canvas(torch.float16, "CHW", 3, 520, 8, False)
    c.set_output_tensor(tcv.tensor.data_ptr(), 3 * 520 * 8 * 2, J.TENSOR_F16, 3, (520 * 8, 8, 1))
    with pytest.raises(J.JxlAmdError, match=r"\(4\)"):  # JXLHIP_ERR_UNSUPPORTED: a band with a tensor bound
        c.upload(ft, band=(1, 2))
    assert tcv.untouched()
    ft.close()
    # a good binding: the downloads of the context's own buffer are refused while it lasts
    c.set_output_tensor(ptr, room, J.TENSOR_F16, 3, chw)
    c.upload(f)
    c.run_all()
    for download in (c.rgb8, c.pixels, lambda: c.rgb8_rows(0, 8)):
        with pytest.raises(J.JxlAmdError, match="code 1"):
            download()
    assert J.lib().jxlhip_rgb8_device_ptr(c._h) is None
    c.sync()
    assert not cv.untouched()
    # unbound again: its own buffer, identical to a fresh context
    c.set_output_tensor(None)
    with pytest.raises(J.JxlAmdError):  # (the frame was uploaded for the tensor: upload again)
        c.run_all()
    c.upload(f)
    c.run_all()
    _same(c.rgb8(), fresh, "after unbinding")
    assert c.pixel_route() == 1
    # closed while bound (the context goes to the pool), the next context starts unbound
    c.set_output_tensor(ptr, room, J.TENSOR_F16, 3, chw)
    c.close()
    cv2 = Canvas(torch.float16, "CHW", 3, ys, xs, False)
    c = J.HipContext()
    c.upload(f)
    c.run_all()
    _same(c.rgb8(), fresh, "a context after one that was closed while bound")
    assert cv2.untouched()
    c.close()
    f.close()
