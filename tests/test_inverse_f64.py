"""tests/inverse_f64.py, the float64 reading of dequantisation, chroma from luma, the lowest frequencies from DC and the
inverse transforms of all 27 strategies, on the CPU:
  (a) the oracle's planes against the reading, from the oracle's own coefficients and DC image, on every stream the GPU
      tests (test_gpu_inverse_f64.py) use: here one learns without a device whether the reading and the oracle agree;
  (b) known answers of the reading itself: a block without AC is the flat block of its DC for the nine strategies that are
      no plain DCT, and the reading's DCT is test_oracle.basis_function;
  (c) the mixed stream tells the reading from each of eleven named misreadings by more than ten times the bar.
The bar (test_gpu_parity.py: float planes of O(1) at 2e-5): 2e-5 * max(1, max |want| over the frame). Nothing is excluded,
except that a chroma-subsampled frame is compared on the frame's own rows and columns (test_gpu_parity._compare)."""
import numpy as np
import pytest

import inverse_f64 as R

BAR = 2e-5
CS420, CS422, CS440 = 4, 8, 12  # (test_gpu_parity.py) channel modes of Cb, Y, Cr: Y at 2x2 / 2x1 / 1x2 samples per MCU
NOT_DCT = (1, 2, 3, 12, 13, 14, 15, 16, 17)  # IDENTITY, DCT2X2, DCT4X4, DCT4X8, DCT8X4, AFV0-3: k_special


def bar(want):
    return BAR * max(1.0, float(np.abs(want).max()))


def strategy_stream(J, s):
    """The smallest frames that hold the case: two groups across with a ragged 8-pixel column and a ragged bottom; for the
    128 / 256 class whole 256 groups plus ragged edges. Two strategies get a frame 256 wider, because the generator
    places fewer than 8 of them in the nominal one: 64x64 (6 in 264x136) and 128x128 (5 in 520x264)."""
    w, h = (264, 136) if s <= 20 else (520, 264)
    if s in (18, 21):
        w += 256
    return J.encode_random(w, h, seed=100 + s, strategy_mask=(1 << s) | 1, gab=0, epf_iters=0)


MIXED = ("two_passes", "one_pass", "large")


def mixed_stream(J, which="two_passes"):
    """Non-default x_qm_scale / b_qm_scale, colour factor and base correlations and coded coefficient orders over a mix of
    strategies. With all 27 allowed the generator draws a strategy of 64 blocks and more with probability 16 / blocks, so a
    520x392 frame holds every strategy up to the 64 class and few larger ones: this seed's holds 128x64 and 64x128.
    "two_passes": the transforms read the natural, zero-filled coefficient layout; "one_pass": the same frame in one pass,
    which the device keeps in scan order with an extent per (varblock, channel), under coded orders. "large" allows the
    128 and 256 class beside 8x8 and IDENTITY only; the generator then starts every group with the largest that fits,
    which in 648x392 are 256x256, 256x128, 128x256 and 128x128. Together the streams hold all 27 under the coded header."""
    if which == "large":
        return J.encode_random(648, 392, seed=9, strategy_mask=0x7E00003, custom_cmap=1, custom_orders=1, num_passes=2)
    return J.encode_random(520, 392, seed=16, custom_cmap=1, custom_orders=1, num_passes=2 if which == "two_passes" else 1)


def assert_mixed_holds(acs, which):
    n = strategy_counts(acs)
    held = (0, 1, 21, 24, 25, 26) if which == "large" else tuple(range(21)) + (22, 23)
    assert all(n[s] > 0 for s in held), n.tolist()


def value_edge_stream(J, name):
    if name == "big_coeffs":  # coefficients beyond 16 bits
        return J.encode_random(264, 136, seed=11, big_coeffs=1, gab=0, epf_iters=0)
    if name == "zero_ac":  # every channel from its corner alone, behind the DC smoothing
        return J.encode_random(264, 136, seed=12, zero_ac=1, gab=0, epf_iters=0)
    if name == "d3":  # an image stream with dense +-1
        return J.encode_rgb8(J.synth_image(331, 245, seed=13), distance=3.0)
    raise KeyError(name)


IMAGE_KW = [dict(distance=0.5, cfl_fit=1), dict(distance=1.0, cfl_fit=1), dict(strategy_mode=0)]


def image_stream(J, kw):
    return J.encode_rgb8(J.synth_image(331, 245, seed=17), **kw)


SUBSAMPLED_KW = [dict(chroma_subsampling=CS420), dict(chroma_subsampling=CS422), dict(chroma_subsampling=CS440),
                 dict(chroma_subsampling=0b011011),  # Cb 1x2, Y 2x1, Cr 2x2: luma subsampled too
                 dict(chroma_subsampling=CS420, custom_cmap=1)]


def subsampled_stream(J, kw):
    return J.encode_random(264, 200, seed=20 + kw["chroma_subsampling"], color_transform=2, **kw)


BATCH = [((264, 136), dict(seed=31, strategy_mask=0x3F00F)), ((331, 245), dict(seed=32, strategy_mask=0x1C0FF1)),
         ((520, 264), dict(seed=33, custom_cmap=1))]  # k_special's set; k_idct_fast's; every strategy with coded correlation


def batch_stream(J, i):
    (w, h), kw = BATCH[i]
    return J.encode_random(w, h, gab=0, epf_iters=0, **kw)


def oracle_fields(data):
    """What the reading takes from the oracle beside coefficients and DC, and the oracle's own planes."""
    import jxlo
    o = jxlo.Decoded(data)
    try:
        i = o.info
        yb, xb = i["ysize_blocks"], i["xsize_blocks"]
        return dict(acs=o.buffer("acs").reshape(yb, xb), quant=o.buffer("quant").reshape(yb, xb), ytox=o.buffer("ytox"),
                    ytob=o.buffer("ytob"), header=o.quant_header, size=(i["xsize"], i["ysize"]), coeffs=o.planes("coeffs"),
                    dc=o.buffer("dc").reshape(3, yb, xb), planes=o.planes("xyb_idct"))
    finally:
        o.close()


def reading(fields, coeffs=None, dc=None, cs=0, misread=None):
    f = fields
    return R.inverse(f["coeffs"] if coeffs is None else coeffs, f["dc"] if dc is None else dc, f["acs"], f["quant"], f["ytox"],
                     f["ytob"], f["header"], cs=cs, size=f["size"], misread=misread)


def strategy_counts(acs):
    a = np.asarray(acs).reshape(-1)
    return np.bincount(a[(a & 1) == 1] >> 1, minlength=27)


def assert_holds(acs, strategies):
    """A named strategy must have at least 8 varblocks in the stream, one of the 256 class at least 1."""
    n = strategy_counts(acs)
    for s in strategies:
        assert n[s] >= (1 if s >= 24 else 8), "strategy %d: %d varblocks" % (s, n[s])


def distance(got, want, fields, cs):
    xs, ys = fields["size"]
    if cs:
        got, want = got[:, :ys, :xs], want[:, :ys, :xs]
    return float(np.abs(got - want).max())


def _oracle_against_reading(data, cs=0, strategies=()):
    f = oracle_fields(data)
    assert_holds(f["acs"], strategies)
    want = reading(f, cs=cs)
    d = distance(f["planes"], want, f, cs)
    print("oracle against the reading: %.3g (bar %.3g, max |want| %.3g)" % (d, bar(want), np.abs(want).max()))
    assert d < bar(want)
    return f, want


# ---- (a) the reading against the oracle
@pytest.mark.parametrize("strategy", list(range(27)))
def test_oracle_every_strategy(built, strategy):
    _oracle_against_reading(strategy_stream(built, strategy), strategies=[strategy])


def assert_custom_header(h):
    """(the frame header's defaults for an XYB frame are x_qm_scale 3, b_qm_scale 2; the colour correlation's 84, 0, 1)"""
    assert h["x_qm_scale"] != 3 and h["b_qm_scale"] != 2 and h["x_qm_scale"] != h["b_qm_scale"]
    assert h["color_factor"] != 84 and h["base_corr_x"] != 0.0 and h["base_corr_b"] != 1.0


@pytest.mark.parametrize("which", MIXED)
def test_oracle_mixed(built, which):
    f, _ = _oracle_against_reading(mixed_stream(built, which))
    assert_mixed_holds(f["acs"], which)
    assert_custom_header(f["header"])


@pytest.mark.parametrize("name", ["big_coeffs", "zero_ac", "d3"])
def test_oracle_value_edges(built, name):
    f, _ = _oracle_against_reading(value_edge_stream(built, name))
    check_value_edge(name, f["coeffs"])


def check_value_edge(name, coeffs):
    """The stream holds the values it is here for."""
    nz = coeffs[coeffs != 0]
    if name == "big_coeffs":
        assert np.abs(nz.astype(np.int64)).max() > 32767
    elif name == "zero_ac":
        assert nz.size == 0
    else:
        assert (np.abs(nz) == 1).mean() > 0.25, "+-1 are %.2f of the non-zero coefficients" % (np.abs(nz) == 1).mean()


def check_image_stream(kw, f):
    """The stream holds what it is for: fitted colour maps that are not constant, several transform sizes; or 8x8 alone."""
    n = strategy_counts(f["acs"])
    if kw.get("cfl_fit"):
        assert len(np.unique(f["ytox"])) > 1 and len(np.unique(f["ytob"])) > 1
        assert (n > 0).sum() >= 3, n.tolist()
    else:
        assert n[0] == f["acs"].size


@pytest.mark.parametrize("kw", IMAGE_KW)
def test_oracle_images(built, kw):
    f, _ = _oracle_against_reading(image_stream(built, kw))
    check_image_stream(kw, f)


@pytest.mark.parametrize("kw", SUBSAMPLED_KW)
def test_oracle_chroma_subsampled(built, kw):
    _oracle_against_reading(subsampled_stream(built, kw), cs=kw["chroma_subsampling"])


@pytest.mark.parametrize("i", range(len(BATCH)))
def test_oracle_batch_frames(built, i):
    _oracle_against_reading(batch_stream(built, i))


# ---- (b) known answers of the reading itself
@pytest.mark.parametrize("strategy", NOT_DCT)
def test_reading_without_ac_is_the_flat_block_of_its_dc(strategy):
    """ac_strategy_test.cc:96-222's property (test_oracle.test_dc_consistency_all_strategies) for one block."""
    block = np.zeros(64)
    block[0] = 0.37
    assert np.abs(R.to_pixels(strategy, block) - 0.37).max() < 1e-15


@pytest.mark.parametrize("strategy", [0, 4, 5, 6, 7, 8, 9, 10, 11, 18, 19, 20, 21, 22, 23, 24, 25, 26])
def test_reading_dct_is_the_basis_function(strategy):
    from test_oracle import DCT_STRATEGIES, basis_function
    rows, cols = DCT_STRATEGIES[strategy]
    cx, cy = R.covered(strategy)
    assert (rows, cols) == (cy * 8, cx * 8)
    rng = np.random.RandomState(strategy)
    for k in [0, 1, max(rows, cols), rows * cols - 1] + list(rng.randint(0, rows * cols, 4)):
        block = np.zeros(rows * cols)
        block[k] = 1.0
        assert np.abs(R.to_pixels(strategy, block) - basis_function(rows, cols, k)).max() < 1e-12


def test_reading_lowest_frequencies_invert_to_the_block_means():
    """LowestFrequenciesFromDC consistency for the DCT family: with no AC, the mean of every 8x8 block of the inverse is the
    DC sample it was made from."""
    rng = np.random.RandomState(5)
    for strategy in (4, 6, 7, 9, 10, 19, 21, 26):
        cx, cy = R.covered(strategy)
        dc = rng.randn(cy, cx)
        llf = R.lowest_frequencies(dc)
        block = np.zeros((min(cx, cy) * 8, max(cx, cy) * 8))
        block[:llf.shape[0], :llf.shape[1]] = llf
        px = R.to_pixels(strategy, block.reshape(-1))
        assert np.abs(px.reshape(cy, 8, cx, 8).mean(axis=(1, 3)) - dc).max() < 1e-6  # (the scales are listed as float32)


# ---- (c) the mixed stream discriminates
def test_mixed_stream_tells_the_named_misreadings_apart(built):
    f = oracle_fields(mixed_stream(built))
    want = reading(f)
    least = 10 * bar(want)
    rows = []
    for name in R.MISREADINGS:
        d = float(np.abs(reading(f, misread=name) - want).max())
        rows.append((name, d))
        print("%-32s %.3g" % (name, d))
    weak = [(n, d) for n, d in rows if not d > least]
    assert not weak, "the stream does not show %r (needs > %.3g)" % (weak, least)
