"""GPU tests (-m gpu): k_enc_acs_walk through jxlhip_enc_acs_walk against the numpy-float32 reading of tests/acs_walk_np.py
and the CPU double, with the tables, shapes and misreadings of test_acs_walk.py. Exact: the kernel compiles the text the CPU
double compiles, with contraction off, so every strategy byte and every bit of the final entropy estimate must agree. The
shapes are those at which the walk takes another path: every w x h in 1..8 as a one-tile frame, and a frame of 3 x 2 tiles
with partial ones (a launch of more than one workgroup)."""
import numpy as np
import pytest

import acs_walk_np as W
from test_acs_walk import (DISTANCE, check_equality, check_guards, check_misreading, check_refusals, product, reading, same, tables)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(built):
    c = built.HipContext()
    yield c
    c.close()


def test_device_walk_equals_the_reading_and_the_cpu_double(built, ctx):
    J = built
    check_equality(J, ctx, list(tables()))
    for name in tables():
        for floating in (0, 1):
            assert same(product(J, ctx, name, floating), product(J, None, name, floating)), (name, floating)


def test_a_tile_inside_a_frame_walks_as_it_does_alone(built, ctx):
    J = built
    for name in [n for n in tables() if "frame" in n]:
        t, xb, yb = tables()[name]
        for floating in (0, 1):
            acs, ent = product(J, ctx, name, floating)
            for tile in range(6):
                bx0, by0 = (tile % 3) * 8, (tile // 3) * 8
                w, h = min(8, xb - bx0), min(8, yb - by0)
                alone = J.ac_strategy_walk(t[tile:tile + 1], w, h, DISTANCE, floating, ctx=ctx, want_entropy=True)
                assert same(alone, (acs[by0:by0 + h, bx0:bx0 + w], np.ascontiguousarray(ent[by0:by0 + h, bx0:bx0 + w])))


@pytest.mark.parametrize("wrong", W.MISREADINGS)
def test_each_misreading_differs_from_the_device_walk(built, ctx, wrong):
    check_misreading(built, ctx, wrong)


def test_any_table_leaves_a_valid_tiling_on_the_device(built, ctx):
    check_guards(built, ctx)


def test_device_entry_refuses_bad_arguments_and_leaves_the_last_frame(built):
    J = built
    img = J.synth_image(136, 72, seed=3)
    ctx = J.HipContext()
    try:
        check_refusals(J, ctx)
        model = J.enc_forward_model(img, ctx, adaptive_quant=1, acs_search=2)
        before = J.enc_search_debug(ctx)
        t, xb, yb = tables()["s1_frame"]
        J.ac_strategy_walk(t, xb, yb, DISTANCE, 1, ctx=ctx)
        after = J.enc_search_debug(ctx)
        assert all(np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)) for k in before)
        ctx.enc_rerun(1)
        again = J.enc_forward_model(img, ctx, adaptive_quant=1, acs_search=2)
        assert all(np.array_equal(model[k], again[k]) for k in model)
    finally:
        ctx.close()
