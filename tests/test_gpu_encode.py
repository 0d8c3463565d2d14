"""GPU tests (-m gpu) of the forward VarDCT path (first slice): jxlhip_enc_forward against the CPU
stream writer's model of the same frame, array by array, and encode -> decode round trips through the GPU decoder.

What pins what: the decoder (inverse DCT, dequantisation, colour) is pinned against the reference, so a
round trip at a stated quality pins the forward transform, the quantiser and the colour conversion as its inverse; the
transform selection / quant field are this repo's own heuristics and are only checked against their CPU form."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("size,kw", [((301, 143), {}), ((512, 512), dict(distance=2.0)), ((640, 333), dict(strategy_mode=0)),
                                     ((257, 260), dict(gab=0, distance=0.5)), ((1000, 700), dict(distance=4.0)),
                                     ((777, 555), dict(cfl_fit=1)), ((640, 333), dict(cfl_fit=1, strategy_mode=0, distance=2.0))])
def test_forward_path_matches_the_cpu_model(built, size, kw):
    """Same float expressions in the same order with contraction off: transform selection and quant field agree except
    where log2f / cbrtf differ in the last place, coefficients and DC except at rounding ties."""
    J = built
    img = J.synth_image(size[0], size[1], seed=31)
    ctx = J.HipContext()
    gpu = J.enc_forward_model(img, ctx, **kw)
    cpu = J.enc_forward_model(img, None, **kw)
    ctx.close()
    same_acs = gpu["acs"] == cpu["acs"]
    assert same_acs.mean() > 0.995, "transform selection differs on %.3f%% of the blocks" % (100 - 100 * same_acs.mean())
    if same_acs.all():
        assert (gpu["qf"] != cpu["qf"]).mean() < 0.005 and np.abs(gpu["qf"] - cpu["qf"]).max() <= 1
        assert np.abs(gpu["dc"] - cpu["dc"]).max() <= 1 and (gpu["dc"] != cpu["dc"]).mean() < 0.002
        diff = gpu["coeffs"] != cpu["coeffs"]
        # (with the chroma-from-luma fit a tile whose least-squares factor lands on the other side of a rounding boundary,
        # sums in another order, changes every X or B coefficient of that tile: still a small fraction)
        assert diff.mean() < (0.01 if kw.get("cfl_fit") else 0.002), diff.mean()
        if (gpu["qf"] == cpu["qf"]).all() and not kw.get("cfl_fit"):
            assert np.abs(gpu["coeffs"] - cpu["coeffs"]).max() <= 1
    nz = np.count_nonzero(gpu["coeffs"])
    assert 0.5 < nz / max(1, np.count_nonzero(cpu["coeffs"])) < 2.0


@pytest.mark.parametrize("distance,floor,cfl", [(0.5, 39.0, 0), (1.0, 37.0, 0), (2.0, 33.5, 0), (4.0, 30.5, 0), (1.0, 37.3, 1)])
def test_gpu_encoded_stream_round_trips(built, distance, floor, cfl):
    """Encode on the GPU, decode on the GPU and with the oracle: same pixels from both decoders, quality as the CPU
    writer's stream of the same image, size within a few percent of it."""
    import jxlo
    J = built
    img = J.synth_image(777, 555, seed=17)
    ctx = J.HipContext()
    t = {}
    data = J.encode_rgb8_gpu(img, ctx, timings=t, distance=distance, cfl_fit=cfl)
    ctx.close()
    assert t["kernels_ms"] > 0
    ref = J.encode_rgb8(img, distance=distance, cfl_fit=cfl)
    if cfl:  # the fit of enc_chroma_from_luma.cc pays: smaller than the stream with the default factors
        assert len(data) < 0.99 * len(J.encode_rgb8(img, distance=distance))
    assert abs(len(data) - len(ref)) < 0.03 * len(ref)
    got = J.decode_rgb8(data)
    o = jxlo.Decoded(data, dumps=False)
    want = o.rgb8.copy()
    o.close()
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1
    p_gpu, p_cpu = _psnr(got, img), _psnr(J.decode_rgb8(ref), img)
    assert p_gpu > floor and abs(p_gpu - p_cpu) < 0.1, (p_gpu, p_cpu)


def test_forward_dct_of_the_basis_functions(built):
    """dct_test.cc's closed form, through the whole forward path: an image whose Y plane is one DCT basis function
    quantises to a single non-zero AC coefficient per block at that frequency. A grey cosine pattern has X = 0 and
    B = Y in XYB up to the opsin non-linearity, so the check is on the dominant coefficient of Y."""
    J = built
    ctx = J.HipContext()
    n = 64
    yy, xx = np.mgrid[0:n, 0:n]
    for (ky, kx) in ((0, 1), (3, 0), (2, 5), (7, 7)):
        wave = np.cos((xx % 8 + 0.5) * kx * np.pi / 8) * np.cos((yy % 8 + 0.5) * ky * np.pi / 8)
        grey = np.clip(128 + 60 * wave, 0, 255).astype(np.uint8)
        m = J.enc_forward_model(np.dstack([grey] * 3), ctx, strategy_mode=0, gab=0, distance=1.0)
        # 64 DCT8 blocks; a square transform's coefficients are stored transposed (coeff_order_fwd.h:27-43: [kx][ky])
        y = m["coeffs"][0, 1].reshape(-1, 8, 8)[:64]
        peak = np.abs(y).reshape(64, 64).argmax(axis=1)
        assert (peak == kx * 8 + ky).all(), (ky, kx, peak[:4])
        others = np.abs(y).reshape(64, 64).copy()
        others[:, kx * 8 + ky] = 0
        assert others.max() * 8 <= np.abs(y[:, kx, ky]).min(), (ky, kx)
    ctx.close()


def test_4k_encode_decodes_on_both_decoders(built):
    """BASELINE.json configs[4] at its size (3840x2160, d1.0, chroma-from-luma fit): the expectation is NOT the twin CPU
    model. The GPU-written stream is decoded by the GPU decoder and by the oracle (the two independent decoders agree
    to +-1 level), and is held to stated floors: PSNR against the source above 36.5 dB and between 0.9 and 2.0 bits per
    pixel (the CPU writer's stream of the same frame gives 37.1 dB at 1.26 bpp on this image class). The forward path has
    this repository's own transform / quant-field heuristics: the floors pin the arithmetic (colour, forward DCT,
    quantiser as the inverse of the reference-pinned decode path), not libjxl's effort-7 choices."""
    import jxlo
    J = built
    img = J.synth_image(3840, 2160, seed=177)
    ctx = J.HipContext()
    t = {}
    data = J.encode_rgb8_gpu(img, ctx, timings=t, distance=1.0, cfl_fit=1)
    ctx.close()
    assert t["kernels_ms"] > 0
    bpp = len(data) * 8.0 / (3840 * 2160)
    assert 0.9 < bpp < 2.0, bpp
    got = J.decode_rgb8(data)
    assert got.shape == img.shape
    o = jxlo.Decoded(data, dumps=False)
    want = o.rgb8.copy()
    o.close()
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3, (int(d.max()), float((d > 0).mean()))
    assert _psnr(got, img) > 36.5, _psnr(got, img)


@pytest.mark.parametrize("size,kw", [((777, 555), {}), ((301, 143), dict(distance=0.5)), ((1024, 768), dict(num_histograms=3, distance=2.0)),
                                     ((640, 333), dict(strategy_mode=0, cfl_fit=1)), ((256, 256), dict(distance=8.0)),
                                     ((2048, 1111), dict(cfl_fit=1)), ((8, 8), {}), ((263, 9), dict(distance=0.3))])
def test_device_tokenisation_writes_the_same_stream(built, size, kw):
    """The AC tokens built on the device (enc_entropy_coder.cc:153-255 restated as two kernels: a count and an emit pass
    per 256x256 group) against the host tokeniser on the coefficients copied back: the codestream is the same, byte for
    byte, so histograms, clustering and every context were the same."""
    J = built
    img = J.synth_image(size[0], size[1], seed=size[0] + 3)
    ctx = J.HipContext()
    host = J.encode_rgb8_gpu(img, ctx, **kw)
    t = {}
    dev = J.encode_rgb8_gpu(img, ctx, timings=t, device_tokens=True, **kw)
    again = J.encode_rgb8_gpu(img, ctx, **kw)  # the context serves both forms in any order
    ctx.close()
    assert host == again
    assert dev == host, (len(dev), len(host))
    assert t["kernels_ms"] > 0 and t["device_tokens"] >= 3 * ((size[0] + 7) // 8) * ((size[1] + 7) // 8) // 64


@pytest.mark.parametrize("size", [(301, 143), (640, 333), (56, 64), (57, 65), (8, 8), (1000, 260), (113, 4)])
def test_sharpening_forms_agree_bit_for_bit(built, size, monkeypatch):
    """The encoder-side sharpening (four rounds of y <- y + (x - K y), enc_gaborish.cc:21-70 in its iterated form) as the
    register-window row kernel against the one-round-per-launch kernel: the same operands in the same order, so every
    quantised coefficient, DC value, transform choice and quant-field entry is the same."""
    J = built
    img = J.synth_image(size[0], size[1], seed=size[0] * 7 + 1)
    ctx = J.HipContext()
    rows = J.enc_forward_model(img, ctx, distance=1.0)
    monkeypatch.setenv("JXLHIP_ENC_SHARPEN_ROUNDS", "1")
    rounds = J.enc_forward_model(img, ctx, distance=1.0)
    ctx.close()
    for key in ("acs", "qf", "dc", "coeffs"):
        assert np.array_equal(rows[key], rounds[key]), key
