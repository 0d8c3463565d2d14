"""The cost estimate of the reference's AC-strategy search as the CPU stream writer states it (jxlenc_cpu_estimate_entropy,
the double of the device's jxlhip_enc_estimate_entropy) against the float64 reading of tests/acs_estimate_f64.py, which
shares no code with it. This is where DELTA_MEASURED and RTOL_MEASURED of that file were measured for the CPU double: run
with -s, every test prints its figures before it asserts."""
import numpy as np
import pytest

import acs_estimate_f64 as M
from enc_fwd_f64 import decide

_inputs, _product, _reading = {}, {}, {}


def factors(kind, size, distance):
    """One int8 pair per 64x64 tile: a fixed list that holds 0, positive and negative values, started at a place that
    depends on the case, so that the single-tile sizes meet all three over the kinds."""
    values = np.array([0, 9, -7, 21, -30, 4, 0, -2, 13, -11, 1, 6], np.int8)
    tiles = ((size[0] + 63) // 64) * ((size[1] + 63) // 64)
    at = M.KINDS.index(kind) + M.DISTANCES.index(distance)
    i = (at + np.arange(tiles)) % len(values)
    return values[i], values[(i + 5) % len(values)]


def inputs(J, kind, size, distance):
    """Planes, quant field, mask1x1 (the CPU entries' own, at the distance under test: inputs to both sides), factors,
    candidates. Computed once per case and left unchanged."""
    key = (kind, size, distance)
    if key not in _inputs:
        p = M.planes(kind, size)
        qf = J.initial_quant_field(p, distance)[0]
        mask = J.masking_1x1(p)
        ytox, ytob = factors(kind, size, distance)
        for a in (p, qf, mask, ytox, ytob):
            a.setflags(write=False)
        _inputs[key] = (p, qf, mask, ytox, ytob, distance, tuple(M.candidates(size[0], size[1])))
    return _inputs[key]


def product(J, ctx, kind, size, distance):
    """(estimates, scaled) of the stand-alone entry: the device's on `ctx`, the CPU double's without."""
    key = (id(ctx), kind, size, distance)
    if key not in _product:
        est, scaled = J.estimate_entropy(*inputs(J, kind, size, distance), ctx=ctx, want_scaled=True)
        est.setflags(write=False)
        scaled.setflags(write=False)
        _product[key] = (est, scaled)
    return _product[key]


def reading_val(J, kind, size, distance):
    key = (kind, size, distance)
    if key not in _reading:
        _reading[key] = M.estimate(*inputs(J, kind, size, distance))[1]
        _reading[key].setflags(write=False)
    return _reading[key]


def check_entry(J, ctx, kind):
    """One plane kind over every size and distance. Step 1: `scaled` against the reading's val by decide(): no rounding
    may be wrong, and the ambiguous band, summed over the kind's cases, holds less than MAX_BAND of the values. Step 2:
    every estimate within the tolerance of the reading evaluated under the product's own roundings. Returns the largest
    |scaled - val| and the largest relative deviation of an estimate."""
    worst_delta, worst_rel, band, total, bad = 0.0, 0.0, 0, 0, []
    for size in M.SIZES:
        for distance in M.DISTANCES:
            args = inputs(J, kind, size, distance)
            est, scaled = product(J, ctx, kind, size, distance)
            val = reading_val(J, kind, size, distance)
            assert est.dtype == scaled.dtype == np.float32 and est.shape == (len(args[6]),) and scaled.shape == val.shape
            assert np.isfinite(est).all() and np.isfinite(scaled).all()
            worst_delta = max(worst_delta, float(np.max(np.abs(scaled - val))))
            amb, wrong = decide(np.rint(scaled), val, np.rint, M.DELTA)
            assert not wrong.any(), (kind, size, distance, int(wrong.sum()), scaled[wrong][:4], val[wrong][:4])
            band, total = band + int(amb.sum()), total + amb.size
            want = M.estimate(*args, rounded=np.rint(scaled))[0]
            rel = np.abs(est - want) / np.abs(want)
            worst_rel = max(worst_rel, float(rel.max()))
            if not rel.max() <= M.rtol(kind):
                bad.append((size, distance, float(rel.max()), args[6][int(rel.argmax())]))
    print("%s: largest |scaled - val| %.3e steps (DELTA %.3e), band %d of %d; largest relative deviation %.3e (tolerance %.3e)" % (
        kind, worst_delta, M.DELTA, band, total, worst_rel, M.rtol(kind)))
    assert band < M.MAX_BAND * total, (band, total)
    assert not bad, bad
    return worst_delta, worst_rel


def check_misreading(J, ctx, wrong):
    """The product lies more than four tolerances from the misreading `wrong`, evaluated under the product's own
    roundings like the reading, for some candidate on some plane of every size that can show it (a misreading of how
    several blocks are combined cannot show on a single 8x8 transform). Distance 1; the kinds are tried until one shows."""
    for size in M.SIZES:
        if size == (8, 8) and wrong in M.NEEDS_SEVERAL_BLOCKS:
            continue
        margin = 0.0
        for kind in M.KINDS:
            args = inputs(J, kind, size, 1.0)
            est, scaled = product(J, ctx, kind, size, 1.0)
            r = np.rint(scaled)
            want = M.estimate(*args, rounded=r)[0]
            other = M.estimate(*args, rounded=r, wrong=wrong)[0]
            margin = max(margin, float(np.max(np.abs(est - other) / np.abs(want))) / M.rtol(kind))
            if margin > 4.0:
                break
        print("%s at %dx%d: %.1f tolerances away" % (wrong, size[0], size[1], margin))
        assert margin > 4.0, (wrong, size, margin)


@pytest.mark.parametrize("kind", M.KINDS)
def test_cpu_entry_matches_float64_reading(built, kind):
    check_entry(built, None, kind)


@pytest.mark.parametrize("wrong", M.MISREADINGS)
def test_each_misreading_bites(built, wrong):
    check_misreading(built, None, wrong)


def test_reading_of_a_flat_plane_and_the_candidate_lists():
    """Judged by the reading alone. A flat plane at zero (at any other level the lowest-frequency coefficient, which the
    loop :428-444 includes, is not zero) has no non-zero rounding and no error: no loss, and the bit estimate is exactly
    the three zeros_mul terms at zero non-zeros, nbits = 1 and CeilLog2(18) + 1 = 6 each, X's weighed by w for several
    blocks. The candidate lists hold every kind, edge positions and the unaligned positions at the two larger sizes."""
    z = np.zeros((3, 64, 64))
    cands = [(0, 3, 2, 1.0), (6, 1, 2, 1.0), (5, 4, 0, 1.0), (18, 0, 0, 1.0)]
    est = M.estimate(z, np.ones((8, 8)), np.full((64, 64), 3.0), [0], [0], 1.0, cands)[0]
    zm = M.init_weights(1.0)[1]
    assert np.allclose(est, [18 * zm, (1.25 * 6 + 12) * zm, (3 * 6 + 12) * zm, (4 * 6 + 12) * zm], rtol=1e-14)
    assert abs(zm - 9.3089059022677905) < 1e-12 and M.init_weights(4.0)[0] > 1.2 > M.init_weights(0.5)[0]
    assert [c[:3] for c in M.candidates(8, 8)] == [(0, 0, 0)]
    for xs, ys in M.SIZES[1:]:
        c = M.candidates(xs, ys)
        assert {s for s, _, _, _ in c} == set(M.STRATEGIES)
        assert any(s == 4 and bx % 2 and by % 2 for s, bx, by, _ in c) and any(s == 5 and bx % 4 and by % 4 for s, bx, by, _ in c)
        assert any(bx + M.COVERED[s][0] == xs // 8 for s, bx, by, _ in c) and any(by + M.COVERED[s][1] == ys // 8 for s, bx, by, _ in c)
        for s, bx, by, _ in c:
            assert bx % 8 + M.COVERED[s][0] <= 8 and by % 8 + M.COVERED[s][1] <= 8
    ox = np.concatenate([factors(k, (8, 8), d)[0] for k in M.KINDS for d in M.DISTANCES])
    assert (ox == 0).any() and (ox > 0).any() and (ox < 0).any()


def check_rejections(J, ctx):
    p, qf, mask, ytox, ytob, distance, _ = inputs(J, "noise", (200, 136), 1.0)
    ok = lambda cands: J.estimate_entropy(p, qf, mask, ytox, ytob, distance, cands, ctx=ctx)
    assert ok([(0, 24, 16, 1.0), (5, 20, 12, 1.0)]).shape == (2,) and ok([]).shape == (0,)
    for cands in ([(0, 25, 0, 1.0)], [(0, 0, 17, 1.0)], [(7, 24, 0, 1.0)], [(18, 16, 16, 1.0)],  # outside the planes
                  [(4, 7, 0, 1.0)], [(5, 2, 6, 1.0)], [(9, 6, 0, 1.0)],                       # across a tile boundary
                  [(1, 0, 0, 1.0)], [(2, 0, 0, 1.0)], [(3, 0, 0, 1.0)], [(12, 0, 0, 1.0)], [(21, 0, 0, 1.0)], [(27, 0, 0, 1.0)]):
        with pytest.raises(J.JxlAmdError):
            ok(cands)
    with pytest.raises(J.JxlAmdError):  # sizes that are no multiples of 8
        J.estimate_entropy(np.zeros((3, 12, 8), np.float32), np.ones((1, 1), np.float32), np.ones((12, 8), np.float32), [0], [0], 1.0,
                           [(0, 0, 0, 1.0)], ctx=ctx)
    with pytest.raises(J.JxlAmdError):
        J.estimate_entropy(p, qf, mask, ytox, ytob, 0.0, [(0, 0, 0, 1.0)], ctx=ctx)
    with pytest.raises(ValueError):
        J.estimate_entropy(p, qf[:-1], mask, ytox, ytob, distance, [(0, 0, 0, 1.0)], ctx=ctx)


def check_entropy_mul(J, ctx):
    """Multipliers 0, 1 and 2: the estimate grows by the bit share each time (the loss is not multiplied), and that share
    is the reading's."""
    args = inputs(J, "noise", (200, 136), 1.0)
    cands = [c[:3] for c in args[6][::7]]
    e0, e1, e2 = (J.estimate_entropy(*args[:6], [c + (m,) for c in cands], ctx=ctx) for m in (0.0, 1.0, 2.0))
    assert (e1 > e0).all() and (e0 > 0).all()
    assert np.allclose(e2 - e1, e1 - e0, rtol=1e-5)
    scaled = J.estimate_entropy(*args[:6], [c + (1.0,) for c in cands], ctx=ctx, want_scaled=True)[1]
    w0, w1 = (M.estimate(*args[:6], [c + (m,) for c in cands], rounded=np.rint(scaled))[0] for m in (0.0, 1.0))
    assert np.allclose(e1 - e0, w1 - w0, rtol=4 * M.RTOL + 1e-5)


def check_independence(J, ctx):
    """A candidate's estimate and scaled values are the same bits alone, in the full list and in shuffled lists."""
    args = inputs(J, "steps", (200, 136), 1.0)
    cands = list(args[6])
    est, scaled = product(J, ctx, "steps", (200, 136), 1.0)
    start, _ = M.offsets(cands)
    rng = np.random.default_rng(5)
    for _ in range(2):
        perm = rng.permutation(len(cands))
        e, s = J.estimate_entropy(*args[:6], [cands[i] for i in perm], ctx=ctx, want_scaled=True)
        assert np.array_equal(e, est[perm])
        pstart, _ = M.offsets([cands[i] for i in perm])
        for j in (0, len(perm) // 2, len(perm) - 1):
            n = 192 * M.COVERED[cands[perm[j]][0]][0] * M.COVERED[cands[perm[j]][0]][1]
            assert np.array_equal(s[pstart[j]:pstart[j] + n], scaled[start[perm[j]]:start[perm[j]] + n])
    for i in list(range(0, len(cands), 97)) + [len(cands) - 1]:
        assert J.estimate_entropy(*args[:6], [cands[i]], ctx=ctx)[0] == est[i], cands[i]


def test_entry_rejects_bad_arguments(built):
    check_rejections(built, None)


def test_entropy_mul_scales_exactly_the_bit_share(built):
    check_entropy_mul(built, None)


def test_estimate_does_not_depend_on_the_other_candidates(built):
    check_independence(built, None)
