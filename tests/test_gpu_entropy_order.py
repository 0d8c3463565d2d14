"""The order of the lane kernel's workgroups (libjxl_amd/csrc/host/jxh_launch_order.h, JXLHIP_WG_ORDER) changes which
workgroup decodes which unit and nothing else: twelve frames of mixed size, distance, histogram sets and passes decode to the
same coefficients, coefficient counts and section flag words in one launch under every order, in the sparse regime (several
waves per unit) and the dense one (JXLHIP_LANES=64), as each frame does alone; jxlhip_debug_entropy_order reports a
permutation of the planned workgroups, longest estimate first under the default order."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DISTANCES = (0.5, 1.0, 3.0)


def _streams(J):
    out = []
    for i in range(12):
        size = (520, 300) if i % 2 == 0 else (300, 280)  # six sections / four sections
        kw = dict(distance=DISTANCES[i % 3])
        if i == 4:
            kw["num_histograms"] = 2  # two units in one frame
        if i == 7:
            kw["num_passes"] = 2      # a unit per pass
        out.append(J.encode_rgb8(J.synth_image(size[0], size[1], seed=40 + i), **kw))
    return out


def _results(ctxs):
    out = []
    for c in ctxs:
        c.sync()
        r, flags = c.errors()
        assert r == 0
        # (kend: the scan-order layout's coefficient counts, which single-pass frames keep; a progressive frame's passes are
        # merged into the natural layout, which "coeffs" shows)
        kend = c.download("kend").copy() if c.frame_info.get("num_passes", 1) == 1 else np.zeros(0, np.uint32)
        out.append((c.download("coeffs").copy(), kend, list(flags)))
    return out


def _same(a, b, where):
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]), (where, i, "coefficients")
        assert np.array_equal(x[1], y[1]), (where, i, "kend")
        assert x[2] == y[2], (where, i, "flag words")


def test_every_order_decodes_the_same_bits(built, monkeypatch):
    J = built
    streams = _streams(J)
    frames = [J.Frame(s) for s in streams]
    ctxs = [J.HipContext() for _ in streams]
    try:
        monkeypatch.delenv("JXLHIP_WG_ORDER", raising=False)
        monkeypatch.delenv("JXLHIP_LANES", raising=False)
        for c, f in zip(ctxs, frames):
            c.upload(f)
            assert c.entropy_route() == 0
            J.run_entropy_batch([c])
        alone = _results(ctxs)
        assert all(not any(a[2]) for a in alone)
        for lanes in (None, "64"):
            if lanes:
                monkeypatch.setenv("JXLHIP_LANES", lanes)
            planned = None
            for order in ("1", "0", "2"):
                monkeypatch.setenv("JXLHIP_WG_ORDER", order)
                for c, f in zip(ctxs, frames):
                    c.upload(f)
                J.run_entropy_batch(ctxs)
                _same(_results(ctxs), alone, (lanes, order))
                unit, est = ctxs[0].entropy_order()
                units = int(unit.max()) + 1
                assert units >= len(ctxs) + 2  # the frame with two histogram sets and the two-pass frame hold two units each
                counts = np.bincount(unit, minlength=units)
                assert (counts > 0).all()
                if lanes is None:
                    assert counts.max() > 1  # sparse regime: several waves per unit
                else:
                    assert (counts == 1).all()  # dense regime: one wave per unit
                starts = np.flatnonzero(np.diff(unit.astype(np.int64), prepend=-1) != 0)
                assert len(starts) == units  # a permutation of the units, the waves of each adjacent
                for u in range(units):
                    assert len(set(est[unit == u].tolist())) == 1
                if order == "0":
                    assert (np.diff(unit.astype(np.int64)) >= 0).all()  # frame order
                    planned = (counts, {u: int(est[unit == u][0]) for u in range(units)})
                if order == "1":
                    assert (np.diff(est.astype(np.float64)) <= 0).all()  # longest estimate first ...
                    e = est[starts].astype(np.float64)
                    u = unit[starts].astype(np.int64)
                    assert ((np.diff(e) < 0) | (np.diff(u) > 0)).all()  # ... equal estimates in frame order
                    first = (counts, {v: int(est[unit == v][0]) for v in range(units)})
                if order == "2":
                    assert not (np.diff(unit.astype(np.int64)) >= 0).all()
                if planned is not None:  # every order holds the same workgroups and estimates
                    assert np.array_equal(planned[0], counts) and planned[1] == {v: int(est[unit == v][0]) for v in range(units)}
                    assert np.array_equal(first[0], counts) and first[1] == planned[1]
            assert len(set(planned[1].values())) > 4  # the estimates tell the frames apart
    finally:
        for c in ctxs:
            c.close()
        for f in frames:
            f.close()
