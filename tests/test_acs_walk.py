"""The merge walk of the reference's AC-strategy search as the product states it (jxh::AcsWalkTile through
jxlenc_cpu_acs_walk, the double of the device's jxlhip_enc_acs_walk) against the numpy-float32 reading of
tests/acs_walk_np.py, which shares no code with it. The walk is additions in a stated order, min and <, so the two are
compared exactly: every strategy byte and every bit of the final entropy estimate. The check_* functions take the context
(None: the CPU double) so that tests/test_gpu_acs_walk.py runs the same checks on the device. Run with -s for the figures."""
import itertools

import numpy as np
import pytest

import acs_walk_np as W

DISTANCE = 1.0
SEEDS = (1, 4, 25)  # (4 and 25 are tables whose full tile ends as one 64x64: the coverage test says what the set must reach)
SHAPES = tuple(itertools.product(range(1, 9), range(1, 9)))  # (w, h) of a one-tile frame
FRAME = (19, 13)  # 3 x 2 tiles with a 3-wide column and a 5-high row
BLOCKS = np.array([cx * cy for _, _, cx, cy in W.KINDS], np.float32)

_tables, _reading, _product = {}, {}, {}


def random_table(seed, tiles):
    """An entry for a transform of n blocks is n * s * exp(N(0, 0.35)); s is 1 for 8x8, else drawn once per table from
    U(0.3, 1.2)."""
    r = np.random.default_rng(seed)
    s = np.float32(r.uniform(0.3, 1.2))
    t = np.exp(r.normal(0, 0.35, (tiles, 10, 8, 8))).astype(np.float32) * BLOCKS[None, :, None, None]
    t[:, 1:] *= s
    return t


def tie_tables():
    """Crafted ties, in units of m = mul8x8 (what an 8x8 entry of 1 becomes), times powers of two, so that every sum in
    them is exact. "equal": every candidate costs exactly what it would replace (nothing may merge under <).
    "branch": at the 16 level each rectangle pair saves the same, so costJxN == costNxJ and the else branch (KXJ) must
    take it; the levels above cost too much."""
    m = W.mul8x8(DISTANCE)
    equal = np.ones((1, 10, 8, 8), np.float32) * BLOCKS[None, :, None, None] * m
    equal[:, 0] = 1.0
    branch = equal.copy() * np.float32(4.0)
    branch[:, 0] = 1.0
    branch[:, 1, :, 0::2] = m  # 16x8 left halves cost m (save m), right halves 2m (save nothing)
    branch[:, 1, :, 1::2] = 2 * m
    branch[:, 2, 0::2, :] = m  # 8x16 top halves likewise
    branch[:, 2, 1::2, :] = 2 * m
    return {"equal": equal, "branch": branch}


def tables():
    """name -> (table [tiles][10][8][8], xb, yb): seeded one-tile tables for every shape, the frame, the crafted ties.
    Built once and left unchanged."""
    if not _tables:
        for seed in SEEDS:
            for w, h in SHAPES:
                _tables["s%d_%dx%d" % (seed, w, h)] = (random_table(1000 * seed + 8 * w + h, 1), w, h)
            _tables["s%d_frame" % seed] = (random_table(77 + seed, 6), FRAME[0], FRAME[1])
        for name, t in tie_tables().items():
            _tables["tie_" + name] = (t, 8, 8)
            _tables["tie_" + name + "_7x5"] = (t, 7, 5)
        for t, _, _ in _tables.values():
            t.setflags(write=False)
    return _tables


def reading(name, floating, misread=None):
    key = (name, floating, misread)
    if key not in _reading:
        t, xb, yb = tables()[name]
        _reading[key] = W.walk_frame(t, xb, yb, DISTANCE, floating, misread)
    return _reading[key]


def product(J, ctx, name, floating):
    key = (id(ctx), name, floating)
    if key not in _product:
        t, xb, yb = tables()[name]
        _product[key] = J.ac_strategy_walk(t, xb, yb, DISTANCE, floating, ctx=ctx, want_entropy=True)
    return _product[key]


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def check_equality(J, ctx, names):
    wrong = []
    for name in names:
        for floating in (0, 1):
            got, want = product(J, ctx, name, floating), reading(name, floating)
            if not same(got, want[:2]):
                wrong.append((name, floating))
            assert W.valid_tiling(got[0]), (name, floating)
    print("%d tables x 2 modes: %d differ from the reading" % (len(names), len(wrong)))
    assert not wrong, wrong[:8]


def check_misreading(J, ctx, wrong):
    """The first table (of those that can show it) on which the misreading differs from the product."""
    names = [n for n in tables() if not n.startswith("tie_")]
    if wrong in ("le_for_lt", "tie_other_way"):
        names = [n for n in tables() if n.startswith("tie_")]
    if wrong == "no_odd_leaks":
        names = [n for n in names if "frame" in n or int(n.split("_")[1][0]) % 2 or int(n.split("x")[1]) % 2]
    modes = (1,) if wrong in ("no_head_checks", "floating_swapped", "and_for_or") else (0, 1)
    tried = 0
    for name in names:
        for floating in modes:
            tried += 1
            if not same(product(J, ctx, name, floating), reading(name, floating, wrong)[:2]):
                print("%s: differs on table %s, floating %d (the %d. tried)" % (wrong, name, floating, tried))
                return
    raise AssertionError("%s differs from the product on none of %d tables" % (wrong, tried))


def hostile_table(seed):
    """What no estimate kernel should write and a caller's table may hold: NaN, infinities, zeros, negatives."""
    r = np.random.default_rng(seed)
    t = r.normal(0, 1, (1, 10, 8, 8)).astype(np.float32) * np.float32(r.choice([1, 10]))
    m = r.random(t.shape)
    t[m < 0.05] = np.nan
    t[(m >= 0.05) & (m < 0.08)] = np.inf
    t[(m >= 0.08) & (m < 0.11)] = -np.inf
    t[(m >= 0.11) & (m < 0.2)] = 0
    return t


def check_guards(J, ctx, seeds=range(30, 60)):
    """On any table the product writes a valid tiling and equals the reading; the reference's text without the two guards
    does not (seed 44, aligned, is one table where it leaves orphaned blocks)."""
    unguarded_invalid = 0
    with np.errstate(all="ignore"):
        for seed in seeds:
            t = hostile_table(seed)
            for floating in (0, 1):
                got = J.ac_strategy_walk(t, 8, 8, DISTANCE, floating, ctx=ctx, want_entropy=True)
                assert W.valid_tiling(got[0]), (seed, floating)
                assert same(got, W.walk_frame(t, 8, 8, DISTANCE, floating)[:2]), (seed, floating)
                unguarded_invalid += not W.valid_tiling(W.walk_frame(t, 8, 8, DISTANCE, floating, "reference_unguarded")[0])
    print("hostile tables: the text without the guards leaves %d invalid tilings of %d" % (unguarded_invalid, 2 * len(seeds)))
    assert unguarded_invalid > 0


def check_refusals(J, ctx):
    t = random_table(5, 1)
    for xb, yb, distance, floating in ((0, 8, 1.0, 0), (8, 0, 1.0, 0), (8, 8, 0.0, 0), (8, 8, -1.0, 1), (8, 8, float("nan"), 0), (8, 8, 1.0, 2)):
        with pytest.raises((J.JxlAmdError, ValueError)):
            J.ac_strategy_walk(t if xb and yb else np.zeros(0, np.float32), xb, yb, distance, floating, ctx=ctx)
    with pytest.raises(ValueError):
        J.ac_strategy_walk(t, 16, 8, 1.0, 0, ctx=ctx)  # a table of one tile for a frame of two


# ---------------------------------------------------------------------------------------------------------- the tests
def test_cpu_walk_equals_the_reading_on_every_tile_shape(built):
    check_equality(built, None, [n for n in tables() if "frame" not in n])


def test_cpu_walk_equals_the_reading_on_a_frame_and_a_tile_does_not_see_its_neighbours(built):
    J = built
    names = [n for n in tables() if "frame" in n]
    check_equality(J, None, names)
    for name in names:
        t, xb, yb = tables()[name]
        for floating in (0, 1):
            acs, ent = product(J, None, name, floating)
            for tile in range(6):
                bx0, by0 = (tile % 3) * 8, (tile // 3) * 8
                w, h = min(8, xb - bx0), min(8, yb - by0)
                alone = J.ac_strategy_walk(t[tile:tile + 1], w, h, DISTANCE, floating, want_entropy=True)
                assert same(alone, (acs[by0:by0 + h, bx0:bx0 + w], np.ascontiguousarray(ent[by0:by0 + h, bx0:bx0 + w])))


def test_the_tables_reach_every_kind_and_every_branch():
    """Conditions on the inputs, measured on the reading: every kind chosen, every branch of the square function taken, the
    early return taken, allow_KXJ false in the aligned walk, every TryMergeAcs kind accepted, a priority refusal."""
    took = {0: set(), 1: set()}
    kinds = set()
    for name in tables():
        for floating in (0, 1):
            acs, _, _, tk = reading(name, floating)
            took[floating] |= tk
            kinds |= set((acs[acs & 1 == 1] >> 1).tolist())
    print("aligned:", sorted(took[0]))
    print("floating adds:", sorted(took[1] - took[0]))
    assert kinds == {num for _, num, _, _ in W.KINDS}
    square = {"JXJ", "JXK_branch", "JXK_left", "JXK_right", "KXJ_branch", "KXJ_top", "KXJ_bottom", "skip_already_JXK"}
    merges = {"merge_" + n for n in ("DCT16X8", "DCT8X16", "DCT16X32", "DCT32X16", "DCT64X32", "DCT32X64")}
    assert square | merges | {"allow_KXJ_false_aligned", "priority_refused"} <= took[0]
    assert {"head_return", "allow_JXK_false_floating", "allow_KXJ_false_floating", "skip_already_KXJ"} <= took[1]
    assert "merge_refused_cut" not in took[0] | took[1]  # (a guard: never on finite estimates above zero)


@pytest.mark.parametrize("wrong", W.MISREADINGS)
def test_each_misreading_differs_from_the_cpu_walk(built, wrong):
    check_misreading(built, None, wrong)


def test_the_guards_refuse_nothing_on_finite_tables_and_keep_any_table_valid(built):
    for name in tables():
        for floating in (0, 1):
            assert same(reading(name, floating)[:2], reading(name, floating, "reference_unguarded")[:2]), (name, floating)
    check_guards(built, None)


def expected_tile_candidates(floating):
    """The candidates of a full tile from the loop bounds of ProcessRectACS, as (kind, cx, cy)."""
    K = W.KIND_OF
    out = {(K["DCT"], x, y) for x in range(8) for y in range(8)}

    def square(blocks, cx, cy):
        half = blocks // 2
        jxk = {2: "DCT16X8", 4: "DCT32X16", 8: "DCT64X32"}[blocks]
        kxj = {2: "DCT8X16", 4: "DCT16X32", 8: "DCT32X64"}[blocks]
        jxj = {2: "DCT16X16", 4: "DCT32X32", 8: "DCT64X64"}[blocks]
        return {(K[jxk], cx, cy), (K[jxk], cx + half, cy), (K[kxj], cx, cy), (K[kxj], cx, cy + half), (K[jxj], cx, cy)}

    for blocks in (2, 4, 8):  # the aligned squares; the TryMergeAcs of a full tile (DCT64X32 twice, DCT32X64 at (0, 4)) are among their halves
        for cy in range(0, 8, blocks):
            for cx in range(0, 8, blocks):
                out |= square(blocks, cx, cy)
    if floating:
        for cy in range(7):  # :1035-1044
            for cx in range(7):
                if (cy | cx) % 2 != 0:
                    out |= square(2, cx, cy)
        for cy in range(5):  # :1047-1057, step 1
            for cx in range(5):
                if (cy | cx) % 4 != 0:
                    out |= square(4, cx, cy)
    return out


def test_candidate_list(built):
    J = built
    for floating, total in ((0, 169), (1, 325)):
        want = expected_tile_candidates(floating)
        cand, index = J.acs_walk_candidates(8, 8, floating)
        strategies = [num for _, num, _, _ in W.KINDS]
        got = {(strategies.index(int(c["strategy"])), int(c["bx"]), int(c["by"])) for c in cand}
        print("full tile, floating %d: %d candidates, by kind %s" % (floating, len(cand), [sum(1 for k, _, _ in got if k == i) for i in range(10)]))
        assert len(cand) == len(got) == len(want) == total and got == want
    for xb, yb in ((8, 8), (3, 5), (5, 8), FRAME):
        for floating in (0, 1):
            cand, index = J.acs_walk_candidates(xb, yb, floating)
            assert len(set(index.tolist())) == len(index) == len(cand)  # no duplicates
            strategies = [num for _, num, _, _ in W.KINDS]
            tiles_x = (xb + 7) // 8
            for c, i in zip(cand, index):
                k = strategies.index(int(c["strategy"]))
                cx, cy = W.KINDS[k][2], W.KINDS[k][3]
                bx, by = int(c["bx"]), int(c["by"])
                assert bx + cx <= xb and by + cy <= yb and bx % 8 + cx <= 8 and by % 8 + cy <= 8
                assert int(i) == ((by // 8) * tiles_x + bx // 8) * 640 + k * 64 + (by % 8) * 8 + bx % 8
                assert np.float32(c["entropy_mul"]) == np.float32(W.MULTIPLIER[W.KINDS[k][0]])
            assert list(cand["strategy"]) == sorted(cand["strategy"], key=strategies.index)  # grouped by kind
    # what the reading asked for, over all tables, is in the list
    for name, (t, xb, yb) in tables().items():
        for floating in (0, 1):
            cand, _ = J.acs_walk_candidates(xb, yb, floating)
            strategies = [num for _, num, _, _ in W.KINDS]
            listed = {(strategies.index(int(c["strategy"])), int(c["bx"]), int(c["by"])) for c in cand}
            assert reading(name, floating)[2] <= listed, (name, floating)


def test_every_candidate_passes_the_estimate_argument_check(built):
    """jxlenc_cpu_estimate_entropy refuses the whole list if jxh::EncEstimateArgsOk refuses one entry."""
    J = built
    for xb, yb in ((8, 8), (3, 5), FRAME):
        cand, _ = J.acs_walk_candidates(xb, yb, 1)
        r = np.random.default_rng(xb)
        planes = (r.random((3, yb * 8, xb * 8)) * 0.1).astype(np.float32)
        tiles = ((xb + 7) // 8) * ((yb + 7) // 8)
        est = J.estimate_entropy(planes, np.full((yb, xb), 0.5, np.float32), np.ones((yb * 8, xb * 8), np.float32), np.zeros(tiles, np.int8),
                                 np.zeros(tiles, np.int8), 1.0, cand)
        assert len(est) == len(cand) and np.all(np.isfinite(est))


def test_refusals(built):
    check_refusals(built, None)
    with pytest.raises(built.JxlAmdError):
        built.acs_walk_candidates(8, 8, 2)
    with pytest.raises(built.JxlAmdError):
        built.acs_walk_candidates(0, 8, 0)
