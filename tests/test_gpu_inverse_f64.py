"""The HIP transform stage (-m gpu) against tests/inverse_f64.py, the float64 reading of the reference's text that
shares no code with the kernels or the oracle: k_idct_fast, k_dct_big, k_special and k_chroma_upsample with StageChannel,
QuantBias / QuantBiasNoBranch and LlfFromDc, from the quantised coefficients and the DC image the device itself holds
after its entropy stage (both held elsewhere: to the oracle bit for bit, to float64 in the DC path's tests) to
download("xyb_idct"). The kernels do not word the stage as the reference does (chroma from luma applied to pixels, the
corner staged as LLF_c - cc * LLF_Y, the hardware's reciprocal, whole channels made from the corner by pruned
butterflies); the reading does, and an error in any of those, or a misreading the oracle shares, shows here.

The streams, the bar (2e-5 * max(1, max |want| over the frame)) and the CPU half (the oracle against the same reading,
the misreadings the mixed stream tells apart) are in test_inverse_f64.py. Every test asserts from the block strategies
that its stream holds what it is for.

Out of scope: raw_quant and other coded dequantisation tables (their weights are held on the host by
test_host_tables.py), bands, anything downstream of "xyb_idct"."""
import numpy as np
import pytest

import test_inverse_f64 as S

pytestmark = pytest.mark.gpu


def _oracle_side(data):
    """acs, quant field, colour maps, header and frame size: what the reading takes beside the device's coefficients and DC."""
    f = S.oracle_fields(data)
    del f["planes"]
    return f


def _run(J, data, dense=False):
    """-> (coeffs, dc, xyb_idct, kend) of one frame through run_entropy / run_transform; kend: the extents of a frame the
    device keeps in scan order, else None."""
    fr = J.Frame(data, threads=2)
    c = J.HipContext()
    try:
        c.set_option("transform_dense", 1 if dense else 0)
        c.upload(fr)
        c.run_entropy()
        c.sync()
        r, flags = c.errors()
        assert r == 0 and not any(flags)
        coeffs = c.download("coeffs")
        try:
            kend = c.download("kend")
        except J.JxlAmdError:
            kend = None
        c.run_transform()
        c.sync()
        return coeffs, c.download("dc"), c.download("xyb_idct"), kend
    finally:
        c.close()
        fr.close()


def _check(f, coeffs, dc, planes, cs=0):
    assert np.array_equal(coeffs[0, :, :64].astype(np.int64), f["coeffs"][0, :, :64])  # (the first block: the same stream on both sides)
    want = S.reading(f, coeffs=coeffs, dc=dc, cs=cs)
    d = S.distance(planes.astype(np.float64), want, f, cs)
    print("kernels against the reading: %.3g (bar %.3g, max |want| %.3g)" % (d, S.bar(want), np.abs(want).max()))
    assert d < S.bar(want)
    return d


def _device_against_reading(J, data, cs=0, dense=False, strategies=()):
    f = _oracle_side(data)
    S.assert_holds(f["acs"], strategies)
    coeffs, dc, planes, kend = _run(J, data, dense)
    _check(f, coeffs, dc, planes, cs)
    f["kend"] = kend
    return f, coeffs


@pytest.mark.parametrize("strategy", list(range(27)))
def test_every_strategy(built, strategy):
    """One strategy beside 8x8 per stream, at least 8 varblocks of it (1 of the 256 class): two groups across, a ragged
    8-pixel column, a ragged bottom."""
    _device_against_reading(built, S.strategy_stream(built, strategy), strategies=[strategy])


@pytest.mark.parametrize("which", S.MIXED)
@pytest.mark.parametrize("dense", [False, True])
def test_mixed(built, which, dense):
    """Coded x_qm_scale / b_qm_scale, colour factor, base correlations and coefficient orders over all 27 strategies
    (test_inverse_f64.mixed_stream: in two passes, in one pass = scan-order layout with extents, and the 128 / 256 class),
    through the kernel's shortcuts and with "transform_dense"."""
    f, _ = _device_against_reading(built, S.mixed_stream(built, which), dense=dense)
    S.assert_mixed_holds(f["acs"], which)
    S.assert_custom_header(f["header"])
    assert (f["kend"] is not None) == (which == "one_pass")  # scan order with extents, or the natural layout


@pytest.mark.parametrize("name,dense", [("big_coeffs", False), ("zero_ac", False), ("d3", False), ("d3", True)])
def test_value_edges(built, name, dense):
    """Coefficients beyond 16 bits (the int32 CoefT instantiations); no AC behind the DC smoothing (every channel from its
    corner); an image at distance 3 with dense +-1 (more than a quarter of the non-zero coefficients), on both paths."""
    f, coeffs = _device_against_reading(built, S.value_edge_stream(built, name), dense=dense)
    S.check_value_edge(name, f["coeffs"])
    assert coeffs.dtype == (np.int32 if name == "big_coeffs" else np.int16)


@pytest.mark.parametrize("kw", S.IMAGE_KW)
def test_images(built, kw):
    """Encoded images: fitted chroma-from-luma maps at two distances over the encoder's own mix of strategies, and 8x8 alone."""
    f, _ = _device_against_reading(built, S.image_stream(built, kw))
    S.check_image_stream(kw, f)


@pytest.mark.parametrize("kw", S.SUBSAMPLED_KW)
def test_chroma_subsampled(built, kw):
    """4:2:0, 4:2:2, 4:4:0, a layout with luma subsampled too, and 4:2:0 under a coded colour correlation: which varblocks
    carry a channel, its own DC position, the chroma-from-luma term and k_chroma_upsample's weights, on the frame's own
    rows and columns."""
    cs = kw["chroma_subsampling"]
    f, _ = _device_against_reading(built, S.subsampled_stream(built, kw), cs=cs)
    hs, vs = S.R.shifts(cs)
    assert any(hs + vs)
    n = S.strategy_counts(f["acs"])
    assert (n[[1, 2, 3, 12, 13, 14, 15, 16, 17]] >= 8).all(), n.tolist()


def test_batch_of_three_frames(built):
    """Three frames of different sizes and strategy sets through run_entropy_batch / run_transform_batch, each against its
    own reading: the workgroup descriptors index frames, and a wrong index reads another frame's parameters."""
    J = built
    datas = [S.batch_stream(J, i) for i in range(len(S.BATCH))]
    fields = [_oracle_side(d) for d in datas]
    assert len(set(f["size"] for f in fields)) == 3 and len(set(f["header"]["global_scale"] for f in fields)) == 3
    S.assert_holds(fields[0]["acs"], S.NOT_DCT)
    S.assert_holds(fields[1]["acs"], (4, 6, 7, 8))
    frames = [J.Frame(d, threads=2) for d in datas]
    ctxs = [J.HipContext() for _ in datas]
    try:
        for c, fr in zip(ctxs, frames):
            c.upload(fr)
        J.run_entropy_batch(ctxs)
        J.run_transform_batch(ctxs)
        for c in ctxs:
            c.sync()
            r, flags = c.errors()
            assert r == 0 and not any(flags)
        for c, f in zip(ctxs, fields):
            _check(f, c.download("coeffs"), c.download("dc"), c.download("xyb_idct"))
    finally:
        for c, fr in zip(ctxs, frames):
            c.close()
            fr.close()


def test_one_batch_of_every_launch_kind_in_two_orders(built):
    """One run_transform_batch over the large-class frame, the scan-order frame, a 4:2:0 frame and a frame of k_special's
    strategies: every kind of launch the set's plan holds (descriptor lists 0 and 21 beside each other, the upsampling of
    two channels, chunks of the big class through the frame's resolved block), with the frames in two orders. Each frame
    against its own reading, and bit for bit what the same frame gives when it runs alone (a subsampled frame over its own
    rows and columns: the upsampling writes those, and nothing writes the padding of the planes beyond them)."""
    J = built
    cases = [(S.mixed_stream(J, "large"), 0), (S.mixed_stream(J, "one_pass"), 0), (S.subsampled_stream(J, S.SUBSAMPLED_KW[0]), S.CS420),
             (S.batch_stream(J, 0), 0)]
    assert S.SUBSAMPLED_KW[0] == dict(chroma_subsampling=S.CS420)
    fields = [_oracle_side(d) for d, _ in cases]
    assert fields[0]["size"] == (648, 392) and fields[2]["size"] == (264, 200)
    S.assert_mixed_holds(fields[0]["acs"], "large")
    S.assert_holds(fields[3]["acs"], S.NOT_DCT)
    alone = [_run(J, d) for d, _ in cases]
    alone = [a[2] for a in alone]  # (xyb_idct)
    frames = [J.Frame(d, threads=2) for d, _ in cases]
    ctxs = [J.HipContext() for _ in cases]
    try:
        for c, fr in zip(ctxs, frames):
            c.upload(fr)
            c.run_entropy()
            c.sync()
            r, flags = c.errors()
            assert r == 0 and not any(flags)
        for order in ((0, 1, 2, 3), (2, 3, 1, 0)):
            J.run_transform_batch([ctxs[i] for i in order])
            for c in ctxs:
                c.sync()
            for i in order:
                planes = ctxs[i].download("xyb_idct")
                _check(fields[i], ctxs[i].download("coeffs"), ctxs[i].download("dc"), planes, cases[i][1])
                w, h = fields[i]["size"] if cases[i][1] else planes.shape[:0:-1]
                assert np.array_equal(planes[:, :h, :w].view(np.uint32), alone[i][:, :h, :w].view(np.uint32)), "frame %d in order %s differs from its run alone" % (i, order)
    finally:
        for c, fr in zip(ctxs, frames):
            c.close()
            fr.close()


def test_planes_shared_after_the_upload(built):
    """jxlhip_share_planes behind the upload: the frame's block still names its own planes, the set's resolved block the
    lender's. Every transform class (the big one took the block as uploaded) must write where the filters read: the pixels
    of the large-class frame equal an unshared decode's. The lender holds the same frame and has not run, so its planes
    hold nothing a misdirected class could leave to be found there."""
    J = built
    data = S.mixed_stream(J, "large")
    S.assert_mixed_holds(_oracle_side(data)["acs"], "large")
    fr = J.Frame(data, threads=2)
    a, b, c = J.HipContext(), J.HipContext(), J.HipContext()
    try:
        c.upload(fr)
        c.run_entropy()
        c.run_transform()
        c.run_filter_color()
        want = c.rgb8().copy()
        a.upload(fr)
        b.upload(fr)
        b.share_planes(a)
        b.run_entropy()
        b.run_transform()
        b.run_filter_color()
        got = b.rgb8()
        assert got.shape == want.shape and want.max() > want.min()
        assert np.array_equal(got, want), "%d samples differ" % int((got != want).sum())
    finally:
        for x in (a, b, c):
            x.close()
        fr.close()
