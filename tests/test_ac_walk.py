"""tests/ac_walk_np.py, the plain reading of the AC coefficient walk written from the reference's text, on the CPU:
  (a) decode: from the tables the oracle parsed and the section bytes, the reading's coefficients equal the oracle's over
      the used slots of every group, and every section ends in the coder's start state at the bit the oracle stopped at;
  (b) tokenise: the jxlenc_cpu_* tokeniser (the stream writer's TokenizeAcGroup) gives the reading's totals and tokens pair
      for pair, under the descriptor variants the device tokeniser takes;
  (c) round trip: tokenising what the reading decoded reproduces the single-pass tokens its reader consumed;
  (d) every named misreading of ac_walk_np.MISREADINGS makes a listed case fail;
  (e) the conditions that make the cases mean something are asserted: see test_the_cases_hold_what_they_are_for.
The cases are shared with tests/test_gpu_ac_walk.py, which holds the device kernels to the same reading."""
import numpy as np
import pytest

import ac_walk_np as W
from host_tables_np import natural_order
from test_inverse_f64 import SUBSAMPLED_KW

# ---------------------------------------------------------------- decode cases


def _subsampled(J, kw, custom_bctx):
    return J.encode_random(264, 200, seed=20 + kw["chroma_subsampling"], color_transform=2, custom_bctx=custom_bctx, **kw)


def _rgba(J):
    return J.encode_rgba8(np.dstack([J.synth_image(264, 200), J.synth_image(264, 200, seed=5)[..., :1]]))


DECODE_CASES = {
    "rgb8": lambda J: J.encode_rgb8(J.synth_image(264, 200)),  # groups 32 + 1 blocks wide
    "random_bctx_orders_hist3": lambda J: J.encode_random(264, 200, custom_bctx=1, custom_orders=1, num_histograms=3),
    "passes2": lambda J: J.encode_random(520, 264, num_passes=2, custom_orders=1),
    "passes3": lambda J: J.encode_random(520, 264, num_passes=3, custom_orders=1),
    "prefix": lambda J: J.encode_rgb8(J.synth_image(264, 200), ac_code_mode=1),
    "lz77": lambda J: J.encode_rgb8(J.synth_image(264, 200), ac_code_mode=2),
    "prefix_lz77": lambda J: J.encode_rgb8(J.synth_image(264, 200), ac_code_mode=3),
    "d05_clusters200": lambda J: J.encode_rgb8(J.synth_image(264, 200), distance=0.5, max_clusters=200),
    "rgba": _rgba,
    # (the GPU file's further frames)
    "mixed_520": lambda J: J.encode_random(520, 264, seed=3),
    "int32": lambda J: J.encode_random(264, 200, seed=8, big_coeffs=1),
}
for _s in range(27):
    DECODE_CASES["strategy%d" % _s] = lambda J, s=_s: J.encode_random(256, 256, strategy_mask=(1 << s) | 1)
for _i, _kw in enumerate(SUBSAMPLED_KW):
    for _b in (0, 1):
        DECODE_CASES["subsampled%d_bctx%d" % (_i, _b)] = lambda J, kw=_kw, b=_b: _subsampled(J, kw, b)
# 4:2:0 with quant-field thresholds through the decoders' other symbol readers: prefix codes with LZ77, and so many
# histograms that their alias tables do not fit beside the context map in LDS (tests/test_gpu_ac_walk.py asserts the kernels)
DECODE_CASES["subsampled0_bctx1_prefix_lz77"] = lambda J: _subsampled(J, dict(SUBSAMPLED_KW[0], ac_code_mode=3), 1)
DECODE_CASES["subsampled0_bctx1_clusters"] = lambda J: _subsampled(J, dict(SUBSAMPLED_KW[0], max_clusters=-200, big_coeffs=1), 1)
# The section-per-workgroup kernels' pass accumulation and histogram selector (the other cases with passes or sets take the
# lane kernel or k_entropy_uni on the device): two passes, two histogram sets (the frame has two groups), custom orders,
# through the prefix / LZ77 reader and through alias tables beyond LDS. The writer cannot give the last of several passes
# tables that large (it carries the lowest bits alone: 32-entry tables, at most 64 KiB of them), so the two-pass frame is
# beyond LDS by its first pass, which decides for the frame, and hist2_clusters has every pass (its only one) beyond it.
_PASSES2_HIST2 = dict(num_passes=2, num_histograms=2, custom_orders=1)
DECODE_CASES["passes2_hist2_prefix_lz77"] = lambda J: J.encode_random(264, 200, ac_code_mode=3, **_PASSES2_HIST2)
DECODE_CASES["passes2_hist2_clusters"] = lambda J: J.encode_random(264, 200, max_clusters=-200, big_coeffs=1, **_PASSES2_HIST2)
DECODE_CASES["hist2_clusters"] = lambda J: J.encode_random(264, 200, max_clusters=-200, big_coeffs=1, num_histograms=2, custom_orders=1)
SUBSAMPLED_BCTX = ["subsampled%d_bctx1" % i for i in range(len(SUBSAMPLED_KW))] + ["subsampled0_bctx1_prefix_lz77", "subsampled0_bctx1_clusters"]

_cache = {}


def case(J, name):
    """The stream, what the oracle parsed and decoded, and the reading's result per group; computed once and left alone."""
    if name not in _cache:
        import jxlo
        data = DECODE_CASES[name](J)
        o = jxlo.Decoded(data, dumps=True, ac_export=True)
        try:
            i = o.info
            yb, xb = i["ysize_blocks"], i["xsize_blocks"]
            c = dict(data=data, tables=o.ac_tables, acs=o.buffer("acs").reshape(yb, xb), quant=o.buffer("quant").reshape(yb, xb),
                     quant_dc=o.buffer("quant_dc").reshape(yb, xb), oracle_coeffs=o.planes("coeffs"), info=dict(i))
        finally:
            o.close()
        c["groups"] = W.decode_frame(c["tables"], data, c["acs"], c["quant"], c["quant_dc"])
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = c
    return _cache[name]


@pytest.mark.parametrize("name", sorted(DECODE_CASES))
def test_the_oracles_coefficients_are_the_readings(built, name):
    c = case(built, name)
    T = c["tables"]
    assert len(c["groups"]) == T["num_groups"] == c["info"]["num_groups"]
    for g, r in enumerate(c["groups"]):
        n = r["used"]
        assert n == _used(c["acs"], g)
        bad = np.argwhere(r["coeffs"][:, :n] != c["oracle_coeffs"][g][:, :n])
        assert bad.size == 0, "group %d: %d coefficients differ, first at channel %d slot %d" % (g, len(bad), bad[0][0], bad[0][1])
        # (decode_group has checked that every pass's coder ended in its start state; the bit it stopped at is the oracle's)
        assert r["end_bits"] == [T["sections"][p][g][3] for p in range(T["num_passes"])]


def _alias_tables_beyond_lds(T, p):
    """jxlhip_frame_upload's condition for reading a pass's alias tables in place: 8 bytes an entry, beside the staged
    context map (one set's contexts + 16, rounded up to 16 bytes) and 1 KiB + 4 * 5 KiB of working space in 150 KiB."""
    ctx_bytes = (T["bctx"]["num_ctxs"] * 495 + 16 + 15) & ~15
    return (len(p["clusters"]) << p["log_alpha"]) * 8 + ctx_bytes + 1024 + 4 * 5120 > 150 * 1024


def _used(acs, g):
    bx0, by0, gw, gh = W._group_rect(g, acs.shape[1], acs.shape[0])
    return gw * gh * 64


def test_the_cases_hold_what_they_are_for(built):
    J = built
    # a quant-field bucket that differs between the channel's column and the frame's: in every custom_bctx subsampled case
    # that has a horizontally subsampled channel (4:4:0 has none: both columns are the same there)
    for name in SUBSAMPLED_BCTX:
        c = case(J, name)
        differs = sum(r["qf_column_differs"] for r in c["groups"])
        assert len(c["tables"]["bctx"]["qf_thresholds"]) > 0
        if any(c["tables"]["hshift"]):
            assert differs > 0, name
        else:
            assert differs == 0 and any(c["tables"]["vshift"]), name
    everything = [r for name in DECODE_CASES for r in case(J, name)["groups"]]
    assert sum(r["dense"] for r in everything) > 0 and sum(r["sparse"] for r in everything) > 0  # nzeros > size / 16 and not
    predicted = set().union(*[r["predicted"] for r in everything])
    assert any(8 <= p < 64 for p in predicted)
    # A predicted count of 64 and more cannot occur in a stream that decodes: a cell of the map is at most
    # (63 * covered + covered - 1) >> log2(covered) = 63 because nzeros <= size - covered, and the predictor averages two
    # cells or takes one, or 32. NonZeroContext's clamp at 64 (ac_context.h:136) is therefore held as a known answer.
    assert max(predicted) <= 63
    b = dict(num_ctxs=15)
    assert W.non_zero_context(b, 64, 3) == W.non_zero_context(b, 1008, 3) == 36 * 15 + 3 != W.non_zero_context(b, 63, 3)
    for name in ("lz77", "prefix_lz77"):
        c = case(J, name)
        assert all(p["lz77"] is not None for p in c["tables"]["passes"]) and sum(r["copies"] for r in c["groups"]) > 0
    assert all(p["use_prefix"] for p in case(J, "prefix")["tables"]["passes"] + case(J, "prefix_lz77")["tables"]["passes"])
    c = case(J, "random_bctx_orders_hist3")  # (the writer codes no more histogram sets than the frame has groups)
    assert c["tables"]["num_histograms"] == min(3, c["tables"]["num_groups"]) > 1 and any(r["ctx_offset"][0] for r in c["groups"])
    shifts = [[p["shift"] for p in case(J, n)["tables"]["passes"]] for n in ("passes2", "passes3")]
    assert shifts == [[1, 0], [2, 1, 0]], shifts
    for n in ("passes2", "passes3"):  # orders differ per pass
        P = case(J, n)["tables"]["passes"]
        assert not np.array_equal(P[0]["orders"], P[1]["orders"])
    assert len(case(J, "d05_clusters200")["tables"]["passes"][0]["clusters"]) > 1
    P = case(J, "subsampled0_bctx1_clusters")["tables"]["passes"][0]  # 200 alias tables of 128 entries: 200 KiB
    assert len(P["clusters"]) == 200 and P["log_alpha"] == 7 and not P["use_prefix"] and P["lz77"] is None
    for n in ("passes2_hist2_prefix_lz77", "passes2_hist2_clusters", "hist2_clusters"):
        T = case(J, n)["tables"]
        P = T["passes"]
        assert T["num_histograms"] == T["num_groups"] == 2 and any(any(r["ctx_offset"]) for r in case(J, n)["groups"]), n
        if n == "hist2_clusters":
            assert len(P) == 1 and _alias_tables_beyond_lds(T, P[0])
            continue
        assert [p["shift"] for p in P] == [1, 0] and not np.array_equal(P[0]["orders"], P[1]["orders"]), n
        if n == "passes2_hist2_prefix_lz77":
            assert all(p["use_prefix"] and p["lz77"] is not None for p in P)
        else:
            assert not any(p["use_prefix"] or p["lz77"] is not None for p in P)
            assert _alias_tables_beyond_lds(T, P[0])  # (the frame's route goes by its largest pass; the writer's last pass stays small)
    for s in range(27):  # every strategy is there
        assert ((case(J, "strategy%d" % s)["acs"] >> 1) == s).any(), s
    # the RGBA stream: Modular data sits behind the coefficients, so the section goes on behind the walk
    c = case(J, "rgba")
    for g, r in enumerate(c["groups"]):
        sec = c["tables"]["sections"][0][g]
        assert r["end_bits"][0] + 16 <= (sec[1] + sec[2]) * 8


# ---------------------------------------------------------------- round trip
@pytest.mark.parametrize("name", ["rgb8", "random_bctx_orders_hist3", "lz77", "strategy21", "subsampled0_bctx1", "subsampled3_bctx1"])
def test_tokenising_the_decoded_coefficients_gives_back_the_tokens_read(built, name):
    c = case(built, name)
    T = c["tables"]
    assert T["num_passes"] == 1
    for g, r in enumerate(c["groups"]):
        got = W.tokenize_group(r["coeffs"], g, c["acs"], c["quant"], c["quant_dc"], T["passes"][0]["orders"], T["bctx"], T["hshift"],
                               T["vshift"], ctx_offset=r["ctx_offset"][0])
        assert got == r["tokens"][0], "group %d" % g


# ---------------------------------------------------------------- misreadings
MISREADING_CASE = {
    "qf_frame_column": "subsampled0_bctx1",
    "predict_default_0": "rgb8",
    "predict_no_round": "rgb8",
    "nz_not_divided": "strategy5",
    "nz_one_cell": "strategy4",
    "prev_constant": "rgb8",
    "k_not_shifted": "strategy5",
    "channels_xyb": "rgb8",
    "bctx_channel_not_swapped": "rgb8",
    "no_selector_offset": "random_bctx_orders_hist3",
    "zero_density_base": "rgb8",
    "predict_across_group_edge": "rgb8",
    "ignore_pass_shift": "passes2",
    "subsampled_counts_on_frame_grid": "subsampled0_bctx0",
}


def test_every_misreading_is_listed():
    assert sorted(MISREADING_CASE) == sorted(W.MISREADINGS)


@pytest.mark.parametrize("mis", W.MISREADINGS)
def test_each_misreading_fails_its_case(built, mis):
    """By a decode error or by coefficients that are not the oracle's (which the test above shows the reading's to be)."""
    c = case(built, MISREADING_CASE[mis])
    try:
        groups = W.decode_frame(c["tables"], c["data"], c["acs"], c["quant"], c["quant_dc"], mis=(mis,))
    except ValueError:
        return
    assert any(not np.array_equal(r["coeffs"][:, :r["used"]], c["oracle_coeffs"][g][:, :r["used"]]) for g, r in enumerate(groups))


@pytest.mark.parametrize("mis", [m for m in W.MISREADINGS if m not in ("no_selector_offset", "predict_across_group_edge", "ignore_pass_shift")])
def test_the_misreadings_change_the_tokens_too(built, mis):
    """The encoder's direction (the three left out belong to the decoder alone: selector, group maps, passes)."""
    c = case(built, MISREADING_CASE[mis])
    T = c["tables"]
    if T["num_passes"] != 1:
        pytest.fail("a single-pass case is needed")
    same = True
    for g, r in enumerate(c["groups"]):
        args = (r["coeffs"], g, c["acs"], c["quant"], c["quant_dc"], T["passes"][0]["orders"], T["bctx"], T["hshift"], T["vshift"])
        try:
            same = same and W.tokenize_group(*args, mis=(mis,)) == W.tokenize_group(*args)
        except (AssertionError, IndexError):
            same = False
    assert not same


# ---------------------------------------------------------------- tokenise: the descriptor variants and the CPU tokeniser
BUCKET_STRATEGY = [0, 1, 4, 5, 6, 8, 10, 18, 19]  # one strategy of each order bucket the forward path selects (up to 64x64)
TOKEN_SIZES = [(8, 8), (257, 255), (264, 200)]
TOKEN_MODELS = [(size, distance, mode) for size in TOKEN_SIZES for distance in (0.3, 1.0, 8.0) for mode in (0, 1)]
# (map, orders, num_hist): every value of each with every value of each other one
TOKEN_VARIANTS = [("default", "natural", 1), ("seeded", "permuted", 3), ("default", "permuted", 3), ("seeded", "natural", 1),
                  ("seeded", "permuted", 1), ("default", "natural", 3)]


def token_descriptor(ctx_map_kind, orders_kind, seed=7):
    """-> (orders uint16, order_offset[13], ctx_map[39], num_ctxs) for the tokeniser entries, and the same orders as the
    reference lays them out, for the reading."""
    rng = np.random.RandomState(seed)
    flat_dev, offsets = [], [0] * 13
    flat_ref = np.zeros(W.coeff_order_offset(13, 0), np.int64)
    for b, s in enumerate(BUCKET_STRATEGY):
        assert W.STRATEGY_ORDER[s] == b
        covered = W.COVERED_X[s] * W.COVERED_Y[s]
        order = np.array(natural_order(W.COVERED_X[s], W.COVERED_Y[s]), np.int64)
        if orders_kind == "permuted":  # beyond the lowest-frequency entries, which no token reads
            order[covered:] = order[covered:][rng.permutation(len(order) - covered)]
        offsets[b] = len(flat_dev)
        flat_dev += order.tolist()
        for c in range(3):
            flat_ref[W.coeff_order_offset(b, c):W.coeff_order_offset(b, c) + len(order)] = order
    for b in range(9, 13):
        offsets[b] = len(flat_dev)
    if ctx_map_kind == "default":
        ctx_map, num_ctxs = list(W.DEFAULT_CTX_MAP), 15
    else:
        num_ctxs = 7
        ctx_map = list(range(num_ctxs)) + rng.randint(0, num_ctxs, 39 - num_ctxs).tolist()
        rng.shuffle(ctx_map)
    return np.array(flat_dev, np.uint16), offsets, ctx_map, num_ctxs, flat_ref


def reading_tokens(model, ctx_map, num_ctxs, num_hist, flat_ref):
    bctx = dict(num_ctxs=num_ctxs, num_dc_ctxs=1, qf_thresholds=[], ctx_map=ctx_map)
    ng = model["coeffs"].shape[0]
    return [W.tokenize_group(model["coeffs"][g], g, model["acs"], model["qf"], None, flat_ref, bctx,
                             ctx_offset=(g % num_hist) * W.num_ac_contexts(num_ctxs)) for g in range(ng)]


def check_tokens(J, ctx, model):
    """Every descriptor variant on the forward model `ctx` holds: totals, tokens, the guard behind `capacity`."""
    for kind, orders_kind, num_hist in TOKEN_VARIANTS:
        orders, offsets, ctx_map, num_ctxs, flat_ref = token_descriptor(kind, orders_kind)
        assert num_ctxs > 1
        totals, got, guard = J.enc_tokens(ctx, orders, offsets, ctx_map, num_ctxs, num_hist)
        want = reading_tokens(model, ctx_map, num_ctxs, num_hist, flat_ref)
        where = (kind, orders_kind, num_hist)
        assert totals.tolist() == [len(w) for w in want], where
        for g, w in enumerate(want):
            w = np.array(w, np.int64).reshape(-1, 2)
            bad = np.argwhere((got[g].astype(np.int64) != w).any(axis=1))
            assert bad.size == 0, "%r group %d: token %d is %r, the reading has %r" % (where, g, bad[0][0], got[g][bad[0][0]].tolist(),
                                                                                     w[bad[0][0]].tolist())
        assert (guard == 0xA5A5A5A5).all(), where


@pytest.mark.parametrize("size,distance,mode", TOKEN_MODELS)
def test_the_cpu_tokeniser_gives_the_readings_tokens(built, size, distance, mode):
    J = built
    ctx = J.CpuEncContext()
    try:
        model = J.enc_forward_model(J.synth_image(*size), ctx, distance=distance, strategy_mode=mode)
        check_tokens(J, ctx, model)
    finally:
        ctx.close()


def test_the_token_inputs_hold_several_transforms_and_groups(built):
    J = built
    m = J.enc_forward_model(J.synth_image(264, 200), None, distance=1.0, strategy_mode=1)
    assert len(np.unique(m["acs"][(m["acs"] & 1) == 1] >> 1)) > 3 and m["coeffs"].shape[0] == 2
    m = J.enc_forward_model(J.synth_image(264, 200), None, distance=1.0, strategy_mode=0)
    assert (np.unique(m["acs"] >> 1) == [0]).all()
