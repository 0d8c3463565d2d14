"""GPU tests (-m gpu): k_enc_estimate through jxlhip_enc_estimate_entropy against the float64 reading of
tests/acs_estimate_f64.py, with the planes, sizes, candidates, tolerances and misreadings of test_acs_estimate_f64.py. The
sizes are the smallest at which each code path exists: (8, 8) one wave-form candidate in a workgroup whose other three waves
have none; (64, 64) every kind, so the wave form at 64 .. 512 samples, the workgroup form with 4 and with 8 outputs per
thread and the 64-point matrix read in place; (200, 136) several launches' worth of candidates over partial tiles."""
import numpy as np
import pytest

import acs_estimate_f64 as M
from test_acs_estimate_f64 import (check_entropy_mul, check_entry, check_independence, check_misreading, check_rejections, inputs,
                                   product)

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


def test_device_and_cpu_double_agree(built, ctx):
    """The kernel restates the CPU statement operation by operation, sums included; what can differ is sqrtf, powf and the
    division in the last place. The bar is the tolerance against the reading; the largest difference is printed."""
    J = built
    worst, worst_scaled = 0.0, 0.0
    for kind in M.KINDS:
        for size in M.SIZES:
            for distance in M.DISTANCES:
                cpu, cpu_scaled = product(J, None, kind, size, distance)
                dev, dev_scaled = product(J, ctx, kind, size, distance)
                worst = max(worst, float(np.max(np.abs(dev - cpu) / np.abs(cpu))) / M.rtol(kind))
                worst_scaled = max(worst_scaled, float(np.max(np.abs(dev_scaled - cpu_scaled))))
    print("device against CPU double: estimates at most %.3e of the tolerance apart, scaled at most %.3e steps" % (worst, worst_scaled))
    assert worst <= 1.0 and worst_scaled <= M.DELTA


def test_device_estimate_does_not_depend_on_the_other_candidates(built, ctx):
    check_independence(built, ctx)


def test_device_entropy_mul_scales_exactly_the_bit_share(built, ctx):
    check_entropy_mul(built, ctx)


def test_device_entry_rejects_bad_arguments_and_leaves_the_last_frame(built):
    J = built
    img = J.synth_image(136, 72, seed=3)
    ctx = J.HipContext()
    try:
        with pytest.raises(J.JxlAmdError):
            ctx.enc_estimate_ms()
        check_rejections(J, ctx)
        stream = J.encode_rgb8_gpu(img, ctx, adaptive_quant=1)
        J.estimate_entropy(*inputs(J, "noise", (200, 136), 1.0), ctx=ctx)
        assert ctx.enc_estimate_ms() > 0
        ctx.enc_rerun(1)
        assert J.encode_rgb8_gpu(img, ctx, adaptive_quant=1) == stream
    finally:
        ctx.close()
