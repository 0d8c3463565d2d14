"""GPU tests (-m gpu): k_enc_mask1x1 through jxlhip_enc_masking_1x1 against the float64 reading of
tests/masking_1x1_f64.py, with the planes, sizes, tolerances and misreadings of test_masking_1x1_f64.py. The sizes put
one, two and several workgroups (64 x 16 outputs each) on the plane, with partial ones in both axes."""
import numpy as np
import pytest

import masking_1x1_f64 as M
from test_masking_1x1_f64 import check_entry, check_misreading, planes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(built):
    c = built.HipContext()
    yield c
    c.close()


@pytest.mark.parametrize("kind", M.KINDS)
def test_device_entry_matches_float64_reading(built, ctx, kind):
    check_entry(built, ctx, kind)


@pytest.mark.parametrize("wrong", M.MISREADINGS)
def test_each_misreading_bites_on_the_device(built, ctx, wrong):
    check_misreading(built, ctx, wrong)


def test_device_and_cpu_double_agree_closely(built, ctx):
    """Both are float32 in one operation order with correctly rounded divisions; they differ only where the two log1pf do,
    a few ulps (1e-7 relative) of a term that is at most the whole denominator. A quarter of the tolerance against the
    reading (6.5e-6 for the bright kinds) leaves that fifty times over and still tells an operation order that differs."""
    J = built
    worst = 0.0
    for kind in M.KINDS:
        for size in M.SIZES:
            cpu, dev = J.masking_1x1(planes(kind, size)), J.masking_1x1(planes(kind, size), ctx=ctx)
            worst = max(worst, float(np.max(np.abs(dev - cpu) / np.abs(cpu)) / M.rtol(kind)))
    print("device against CPU double: at most %.3f of the tolerance" % worst)
    assert worst <= 0.25


def test_device_entry_rejects_bad_arguments_and_leaves_the_last_frame(built):
    J = built
    img = J.synth_image(136, 72, seed=3)
    ctx = J.HipContext()
    try:
        with pytest.raises(J.JxlAmdError):
            ctx.enc_masking_ms()
        with pytest.raises(J.JxlAmdError):
            J.masking_1x1(np.zeros((3, 12, 8), np.float32), ctx=ctx)
        stream = J.encode_rgb8_gpu(img, ctx, adaptive_quant=1)
        J.masking_1x1(planes("noise", (200, 136)), ctx=ctx)
        assert ctx.enc_masking_ms() > 0
        ctx.enc_rerun(1)
        assert J.encode_rgb8_gpu(img, ctx, adaptive_quant=1) == stream
    finally:
        ctx.close()
