"""The inputs of the launch-order cost estimate (libjxl_amd/csrc/host/jxh_launch_order.h) for the benchmark's streams, made
without a GPU: per AC section its byte size (the oracle's section table), its block count (the forward model's AC-strategy
map) and its true token count (the stream writer's tokeniser through enc_tokens on a CpuEncContext). Shared by
tests/test_launch_order.py and scripts/fit_entropy_cost.py."""
import numpy as np

import ac_walk_np as W
from host_tables_np import natural_order

SEEDS = tuple(range(177, 185))  # bench.py's eight distinct streams


def natural_descriptor():
    """orders (uint16), order_offset[13], the default block-context map and its context count: what the stream writer uses."""
    flat, offsets = [], [0] * 13
    for b, s in enumerate([0, 1, 4, 5, 6, 8, 10, 18, 19]):  # one strategy of each order bucket the forward path selects
        assert W.STRATEGY_ORDER[s] == b
        offsets[b] = len(flat)
        flat += list(natural_order(W.COVERED_X[s], W.COVERED_Y[s]))
    for b in range(9, 13):
        offsets[b] = len(flat)
    return np.array(flat, np.uint16), offsets, list(W.DEFAULT_CTX_MAP), 15


def sections_of(J, jxlo, xsize, ysize, seed):
    """-> (groups, 3) int64: bytes, blocks, tokens of every AC section of the stream bench.py makes for `seed` at d1.0."""
    img = J.synth_image(xsize, ysize, seed)
    data = J.encode_rgb8(img, distance=1.0, strategy_mode=1)
    dec = jxlo.Decoded(data, dumps=False, ac_export=True)
    sizes = [s[2] for s in dec.ac_tables["sections"][0]]
    dec.close()
    ctx = J.CpuEncContext()
    try:
        model = J.enc_forward_model(img, ctx, distance=1.0, strategy_mode=1)
        totals = J.enc_tokens(ctx, *natural_descriptor())[0]
    finally:
        ctx.close()
    first = (model["acs"] & 1) == 1
    gx = (xsize + 255) // 256
    blocks = [int(first[(g // gx) * 32:(g // gx) * 32 + 32, (g % gx) * 32:(g % gx) * 32 + 32].sum()) for g in range(len(sizes))]
    assert len(totals) == len(sizes)
    return np.array([sizes, blocks, totals.tolist()], np.int64).T
