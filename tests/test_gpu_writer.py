"""GPU tests (-m gpu) of the pixel writers, held bit-exact to tests/writer_np.py, the float32 reading of the reference's
stage_write.cc. The images are lossless Modular frames of more than 8 bits (reference-encoder fixtures and this
repository's encode_lossless_samples), so the writer's input is exactly np_sample_to_float of the encoder's input and
the 8-bit dither, the bit-depth modes, the orientation and the extra-channel buffer all show in the output."""
import json
import os
import sys

import numpy as np
import pytest

import writer_np as W
from test_gpu_modular import np_sample_to_float

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
MANIFEST = json.load(open(os.path.join(ROOT, "tests", "golden", "fjxl_manifest.json")))
_FMT = {"u8": (2, np.uint8), "u16": (3, np.uint16), "f16": (5, np.float16), "f32": (0, np.float32)}


def _fixture(name):
    import make_fjxl_golden as G
    return open(os.path.join(ROOT, "tests", "golden", name + ".jxl"), "rb").read(), G.golden_image(name), MANIFEST[name]["bits"]


def _writer_input(img, bits, alpha_bits=None):
    """The floats the writer starts from: every channel through the reference's int -> float at its own depth."""
    f = np_sample_to_float(img, bits, 0)
    if alpha_bits is not None and alpha_bits != bits:
        f[..., -1] = np_sample_to_float(img[..., -1], alpha_bits, 0)
    return f


def _check(got, want, what):
    bad = got.view(np.uint8) != want.view(np.uint8) if got.dtype == np.float16 else got != want
    assert got.shape == want.shape, what
    assert not bad.any(), "%s: %d samples differ, first at %s" % (what, int(bad.sum()), np.argwhere(bad)[0].tolist())


def _decode_ctx(J, data, fmt, nc, bits=0, orientation=1):
    """decode_lossless with the writer's bits and orientation (HipContext)."""
    f = J.ModFrame(data)
    c = J.HipContext()
    try:
        c.set_output_format(_FMT[fmt][0], nc, bits)
        c.set_output_orientation(orientation)
        c.upload_modular(f)
        c.run_modular()
        r, status, _ = c.modular_status()
        assert r == 0 and not any(status)
        return c.pixels()
    finally:
        c.close()
        f.close()


# (fixture, bit-depth option of the replay program, output format, the writer's bits; None: the decoder must refuse)
_API_CASES = [
    ("fjxl_d10_280x36_rgba_e2", None, "u8", 8),
    ("fjxl_d10_280x36_rgba_e2", "depth=stream", "u8", None),   # 10 bits do not fit a u8 (decode.cc:2982)
    ("fjxl_d5_70x50_graya_e2_noise", "depth=stream", "u8", 5),
    ("fjxl_d12_48x40_rgba_e0_noise", "depth=1", "u8", 1),
    ("fjxl_d12_48x40_rgba_e0_noise", "depth=5", "u8", 5),
    ("fjxl_d16_270x24_rgb_e0", "depth=8", "u8", 8),
    ("fjxl_d10_280x36_rgba_e2", None, "u16", 16),
    ("fjxl_d10_280x36_rgba_e2", "depth=stream", "u16", 10),
    ("fjxl_d14_90x60_graya_e0", "depth=stream", "u16", 14),
    ("fjxl_d16_40x30_rgba_e2_noise", "depth=10", "u16", 10),
    ("fjxl_d12_100x80_gray_e2", "depth=12", "u16", 12),
    ("fjxl_d12_48x40_rgba_e0_noise", None, "f16", None),
    ("fjxl_d14_50x40_rgb_e2_noise", None, "f16", None),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,depth,fmt,bits", _API_CASES)
def test_writer_through_the_decoder_api(built, tmp_path, name, depth, fmt, bits):
    """JxlDecoderSetImageOutBitDepth (FROM_PIXEL_FORMAT, FROM_CODESTREAM, CUSTOM) through the C API, main buffer and the
    extra-channel buffer (fjxl's alpha has the colour's depth, so its 8-bit form is dithered too, as channel 0)."""
    import replay_util as R
    data, img, b = _fixture(name)
    h, w, nc = img.shape
    extra = [depth] if depth else []
    if nc in (2, 4):
        extra.append("ec")
    rc, events, out, px = R.run(data, tmp_path, fmt, nc, *extra)
    if fmt != "f16" and bits is None:
        assert rc != 0, out  # (refused at JxlDecoderSetImageOutBitDepth)
        return
    assert rc == 0 and events[-1] == "SUCCESS", out
    dt = _FMT[fmt][1]
    f = _writer_input(img, b)
    main = np.frombuffer(px[:h * w * nc * dt().itemsize], dt).reshape(h, w, nc)
    _check(main, W.write(f, fmt, bits or 0), name)
    if nc in (2, 4):
        ec = np.frombuffer(px[h * w * nc * dt().itemsize:], dt).reshape(h, w, 1)
        _check(ec, W.write(f[..., -1:], fmt, bits or 0), name + " ec")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fjxl_d10_280x36_rgba_e2", "fjxl_d5_300x40_rgb_e0", "fjxl_d16_40x30_rgba_e2_noise",
                                  "fjxl_d14_90x60_graya_e0", "fjxl_d1_40x30_rgba_e2"])
def test_writer_through_decode_lossless(built, name):
    """k_modular_output directly: u8 at 8 / 5 / 1 bits, u16 at 16 / the stream's bits, f16; every channel count."""
    J = built
    data, img, b = _fixture(name)
    f = _writer_input(img, b)
    nc = img.shape[2]
    for fmt, bits in (("u8", 8), ("u8", 5), ("u8", 1), ("u16", 16), ("u16", b), ("f16", 0)):
        _check(_decode_ctx(J, data, fmt, nc, bits), W.write(f, fmt, bits), "%s %s %d" % (name, fmt, bits))


@pytest.mark.gpu
@pytest.mark.parametrize("orientation", range(1, 9))
def test_writer_orientation_of_a_deep_image(built, tmp_path, orientation):
    """A 10-bit RGBA image (8-bit alpha) under each orientation: the flips move the dither cell, the transpose does not
    (stage_write.cc:341-342, 484-487, 662-699). The C API with the extra-channel buffer, and the context directly."""
    import replay_util as R
    J = built
    xs, ys = 71, 45
    rng = np.random.default_rng(orientation)
    v = rng.integers(0, 1024, (ys, xs, 3)).astype(np.int32)
    alpha = rng.integers(0, 256, (ys, xs, 1)).astype(np.int32)
    J.set_orientation(orientation)
    try:
        data = J.encode_lossless_samples(np.dstack([v, alpha]), 10, 0, flags=16)
    finally:
        J.set_orientation(1)
    f = np.dstack([np_sample_to_float(v, 10, 0), np_sample_to_float(alpha, 8, 0)])
    oxs, oys = (ys, xs) if orientation > 4 else (xs, ys)
    for fmt in ("u8", "u16"):
        rc, events, out, px = R.run(data, tmp_path, fmt, 4, "ec")
        assert rc == 0, out
        dt = _FMT[fmt][1]
        n = oxs * oys * 4 * dt().itemsize
        _check(np.frombuffer(px[:n], dt).reshape(oys, oxs, 4), W.write(f, fmt, 8 if fmt == "u8" else 16, orientation), fmt)
        _check(np.frombuffer(px[n:], dt).reshape(oys, oxs, 1), W.write(f[..., 3:], fmt, 8 if fmt == "u8" else 16, orientation), fmt + " ec")
    _check(_decode_ctx(J, data, "u8", 3, 8, orientation), W.write(f[..., :3], "u8", 8, orientation), "context u8")
    _check(_decode_ctx(J, data, "u8", 4, 6, orientation), W.write(f, "u8", 6, orientation), "context u8 at 6 bits")


def _fma_sensitive_image(bits=16, size=64, nc=3):
    """A `bits`-bit image whose samples sit, wherever such a value exists, at a dither cell (of their channel) where the
    reference's Mul-then-Add and a contracted FMA give different u8 values; random elsewhere."""
    v_all = np.arange(1 << bits)
    f_all = np_sample_to_float(v_all, bits, 0)
    d = W.dither32()
    pick = {}
    for cy in range(32):
        for cx in range(32):
            dd = np.full(f_all.shape, d[cy, cx], np.float32)
            hit = np.nonzero(W.make_unsigned(f_all, 255, dd) != W.make_unsigned(f_all, 255, dd, fused=True))[0]
            if len(hit):
                pick[(cy, cx)] = hit
    rng = np.random.default_rng(bits)
    img = rng.integers(0, 1 << bits, (size, size, nc)).astype(np.int32)
    for y in range(size):
        for x in range(size):
            for c in range(nc):
                hit = pick.get(((y + 13 * c) % 32, (x + 23 * c) % 32))
                if hit is not None:
                    img[y, x, c] = hit[(x + 7 * y + c) % len(hit)]
    return img


def test_writer_fused_and_separate_forms_differ_on_the_fma_image():
    """(CPU) The image of test_writer_on_the_fma_image can tell the reference's Mul-then-Add from a contracted FMA."""
    img = _fma_sensitive_image()
    f = np_sample_to_float(img, 16, 0)
    assert int((W.write(f, "u8", 8) != W.write(f, "u8", 8, fused=True)).sum()) >= 50


@pytest.mark.gpu
def test_writer_on_the_fma_image(built, tmp_path):
    """u8 of 16-bit samples chosen so that an FMA in the writer (f * mul + dither rounded once) changes the value:
    k_modular_output and the C API must give the reference's two-rounding result on every sample."""
    import replay_util as R
    J = built
    img = _fma_sensitive_image()
    data = J.encode_lossless_samples(img, 16, 0, flags=16)
    want = W.write(np_sample_to_float(img, 16, 0), "u8", 8)
    _check(J.decode_lossless(data, 3, data_type=2), want, "decode_lossless")
    rc, events, out, px = R.run(data, tmp_path, "u8", 3)
    assert rc == 0, out
    _check(np.frombuffer(px, np.uint8).reshape(want.shape), want, "C API")


@pytest.mark.gpu
@pytest.mark.parametrize("epf", [1, 2])
def test_vardct_u8_against_the_same_decodes_floats(built, tmp_path, epf):
    """VarDCT u8 where the writer's input float is observable: the linear target (JxlDecoderSetOutputColorProfile with a
    linear transfer function), where u8 RGB and f32 RGB both come from the fused filter kernel with the same arithmetic.
    (On the default sRGB target the 8-bit path has its own curve form, so its input is not the f32 output.)
    * RGB u8 (ToU8D in the fused kernel, which still contracts f * 255 + dither): every sample equals writer_np's
      Mul-then-Add reading of the f32 output, or, only where the two forms differ, the fused reading;
    * RGBA u8 (the generic writer, StorePixel): exactly the Mul-then-Add reading of the RGBA f32 output."""
    import replay_util as R
    J = built
    xs, ys = 520, 300
    rgb = J.synth_image(xs, ys, seed=40 + epf)
    alpha = ((np.mgrid[0:ys, 0:xs][0] * 5 + np.mgrid[0:ys, 0:xs][1] * 3) & 255).astype(np.uint8)
    for nc, data in ((3, J.encode_rgb8(rgb, epf_iters=epf)), (4, J.encode_rgba8(np.dstack([rgb, alpha]), epf_iters=epf))):
        rc, events, out, px = R.run(data, tmp_path, "f32", nc, "linear")
        assert rc == 0 and "COLOR_ENCODING tf=8" in out, out
        f = np.frombuffer(px, np.float32).reshape(ys, xs, nc).copy()
        rc, events, out, px = R.run(data, tmp_path, "u8", nc, "linear")
        assert rc == 0 and "COLOR_ENCODING tf=8" in out, out
        got = np.frombuffer(px, np.uint8).reshape(ys, xs, nc)
        sep, fused = W.write(f, "u8", 8), W.write(f, "u8", 8, fused=True)
        if nc == 4:
            _check(got, sep, "RGBA u8 (StorePixel)")
            continue
        assert np.all((got == sep) | (got == fused)), "%d samples are neither form" % int(((got != sep) & (got != fused)).sum())
        print("vardct linear u8, epf %d: %d of %d samples take the fused form, %d differ between the forms"
              % (epf, int((got != sep).sum()), got.size, int((sep != fused).sum())))
