"""The transform kernel's wave-uniform shortcuts (-m gpu): a channel made from its lowest-frequency corner alone, staging
rounds no varblock of the wave reaches left out. Every stream is decoded once as usual and once with the option
"transform_dense", which makes the same kernel treat every coefficient extent as full:
  * download("xyb_idct") of the two decodes is equal under ==, rgb8() byte for byte;
  * both hold to the oracle at the suite's bars (test_gpu_parity.py): planes < 2e-5, pixels within one level;
  * the kend the device produced shows that the stream took the paths it is here for (coefficient_extents.wave_decisions
    restates the kernel's decisions): a stream that never takes a shortcut does not pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _decode(J, data, dense):
    f = J.Frame(data, threads=2)
    c = J.HipContext()
    try:
        c.set_option("transform_dense", 1 if dense else 0)
        c.upload(f)
        c.run_entropy()
        c.sync()
        r, flags = c.errors()
        assert r == 0 and not any(flags)
        import coefficient_extents as E
        extents = E.device_extents(c)
        c.run_transform()
        c.sync()
        planes = c.download("xyb_idct")
        c.run_filter_color()
        c.sync()
        return planes, c.rgb8(), extents
    finally:
        c.close()
        f.close()


def _both_paths(J, data, claims, strategies=None):
    """claims: what the stream is here for, of 'llf' (a wave with a channel from its corner alone), 'skip' (a staging round
    left out in a wave that stages others), 'full' (a wave with a channel that takes no shortcut); with '?': may occur."""
    import jxlo
    import coefficient_extents as E
    sparse, rgb_sparse, extents = _decode(J, data, dense=False)
    dense, rgb_dense, extents_dense = _decode(J, data, dense=True)
    assert extents == extents_dense
    dec = E.wave_decisions(extents)
    if strategies is not None:
        assert set(strategies) <= set(dec), "the stream lacks strategies %r" % sorted(set(strategies) - set(dec))
    got = E.exercised(dec)
    print("waves %d, channels from the corner alone %d, rounds left out beside staged ones %d, full waves %d" %
          (sum(d["waves"] for d in dec.values()), got["llf"], got["skip"], got["full"]))
    for what in claims:
        if what.endswith("?"):  # (may occur)
            continue
        assert got[what] > 0, "the stream never exercises '%s': %r" % (what, got)
    for what in ("llf", "skip", "full"):  # ... and nothing it is said not to have
        if what not in claims and what + "?" not in claims:
            assert got[what] == 0, "unexpected '%s': %r" % (what, got)
    assert np.array_equal(sparse, dense), "planes differ between the two paths: max |d| = %g" % np.abs(sparse - dense).max()
    assert np.array_equal(rgb_sparse, rgb_dense)
    o = jxlo.Decoded(data)
    try:
        ref = o.planes("xyb_idct")
        for x in (sparse, dense):
            assert np.abs(x - ref).max() < 2e-5
        for rgb in (rgb_sparse, rgb_dense):
            d = np.abs(rgb.astype(int) - o.rgb8.astype(int))
            assert d.max() <= 1
    finally:
        o.close()
    return dec


def test_zero_ac_every_channel_from_its_corner(built):
    """No AC anywhere: every channel of every wave, Y included, is made from the DC image alone."""
    import coefficient_extents as E
    J = built
    seen = set()
    for seed in (1, 2):
        data = J.encode_random(640, 520, seed=seed, zero_ac=1, skip_dc_smoothing=1, strategy_mask=0x1FFFFF)
        dec = _both_paths(J, data, {"llf"})
        for d in dec.values():
            assert d["llf_only"] == [d["waves"]] * 3
        seen |= set(dec)
    assert seen == set(E.FAST_STRATEGIES)


@pytest.mark.parametrize("strategy", [0, 4, 5, 6, 7, 8, 9, 10, 11, 18, 19, 20])
def test_basis_streams(built, strategy):
    """One non-zero Y coefficient per varblock, walking over the positions: X and B come from their corners in every wave, Y
    stages as far as the wave's furthest coefficient (rounds left out in the classes that have several) or entirely."""
    import coefficient_extents as E
    from test_oracle import basis_stream
    J = built
    data, _, _ = basis_stream(J, strategy)
    # (the 8x8 class has two rounds and eight varblocks per wave: one of the eight reaches the second in every wave here)
    multi_round = E.geometry(strategy)[3] > 1 and strategy != 0
    dec = _both_paths(J, data, {"llf", "full"} | ({"skip"} if multi_round else set()), [strategy])[strategy]
    assert dec["llf_only"][0] == dec["waves"] and dec["llf_only"][2] == dec["waves"]


def test_random_coefficients_every_fast_strategy(built):
    """encode_random: coefficients everywhere, in all three channels, over every strategy of the kernel: full waves, and
    rounds left out here and there."""
    import coefficient_extents as E
    J = built
    seen = set()
    for seed in (3, 4):
        data = J.encode_random(640, 520, seed=seed, strategy_mask=0x1C0FF1, gab=0, epf_iters=0)
        dec = _both_paths(J, data, {"full", "skip", "llf?"})
        seen |= set(st for st, d in dec.items() if d["full_waves"])
    assert seen == set(E.FAST_STRATEGIES)


def _smooth_colour_textured_luma(xs, ys, seed):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:ys, 0:xs].astype(np.float64)
    luma = 110 + 60 * np.sin(x / 90.0) * np.cos(y / 70.0)
    texture = rng.randn(ys, xs) * (0.5 + 22 * (np.sin(x / 130.0 + 1.0) * np.sin(y / 110.0) > 0.2))  # textured and calm regions
    tint = np.stack([12 * np.sin(x / 300.0), 9 * np.cos(y / 260.0), -14 * np.sin((x + y) / 340.0)], -1)
    return np.clip((luma + texture)[..., None] + tint, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("distance", [1.0, 3.0])
def test_image_smooth_colour_textured_luma(built, distance):
    """What the shortcuts are for: chroma without AC in the large varblocks next to luma with plenty."""
    J = built
    data = J.encode_rgb8(_smooth_colour_textured_luma(1024, 768, seed=11), distance=distance, strategy_mode=1)
    _both_paths(J, data, {"llf", "skip", "full"})
