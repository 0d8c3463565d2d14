"""The CPU stream writer's model of the forward VarDCT path (jxlenc_cpu_forward through enc_forward_model with no
context) against the float64 reading of tests/enc_fwd_f64.py, which shares no code or tables with it. The CPU model is
what the GPU kernels are held to array by array; this holds the pair's shared tables and conventions (resample scales,
coefficient layout, quantisation bias, sharpening edges, dead zone) to an independent reading, and is where the
comparison margins of enc_fwd_f64.DELTA were measured."""
import json
import os

import numpy as np
import pytest

import enc_fwd_f64 as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (size, kw): every size of the GPU cases up to 1000x700, distances 0.3 / 1 / 4, gab 0 / 1, strategy modes 0 / 1
CASES = [((8, 8), dict(distance=0.3, gab=0)), ((113, 4), dict(distance=1.0, strategy_mode=0)), ((263, 9), dict(distance=4.0)),
         ((257, 260), dict(distance=1.0, gab=0)), ((257, 260), dict(distance=0.3)), ((520, 300), dict(distance=1.0)),
         ((520, 300), dict(distance=4.0, gab=0, strategy_mode=0)), ((1000, 700), dict(distance=0.3)),
         ((1000, 700), dict(distance=4.0)), ((1000, 700), dict(distance=1.0, gab=0, strategy_mode=0))]
MOSAIC_KW = dict(distance=1.0, gab=0, strategy_mode=1)


def _reading_kw(kw):
    return dict(distance=kw.get("distance", 1.0), gab=kw.get("gab", 1), strategy_mode=kw.get("strategy_mode", 1))


def test_reading_constants_match_the_reference_text():
    """The reading's own derivations against values the reference lists: DCTResampleScales<16, 2> and <64, 8>
    (dct_scales.h) and the inverse of the opsin absorbance matrix (opsin_params.h, golden 'inverse_opsin')."""
    assert abs(E.resample_scales(2)[1] - 0.901764195028874394) < 1e-12
    assert np.allclose(E.resample_scales(8), [1.0, 0.9936866130906366, 0.9748868211368796, 0.9440180941651672, 0.9017641950288744,
                                              0.8490574973847023, 0.7870549181591013, 0.7171081282466044], atol=1e-12)
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_constant_floats.json")))
    inv = np.asarray(g["inverse_opsin"], np.float64).reshape(3, 3)
    assert np.allclose(np.linalg.inv(E.OPSIN), inv, rtol=1e-6, atol=1e-6)
    for n in (1, 2, 4, 8, 16, 32, 64):  # the scaled IDCT the DC path uses is the spec DCT's inverse
        assert np.allclose(E.idct_matrix(n) @ E.dct_matrix(n), np.eye(n), atol=1e-12)


@pytest.mark.parametrize("size,kw", CASES)
def test_forward_cpu_model_matches_float64_reading(built, size, kw):
    J = built
    img = J.synth_image(size[0], size[1], seed=size[0] + 11)
    header = E.header_scalars(J, kw.get("distance", 1.0))
    model = J.enc_forward_model(img, None, **kw)
    E.check_forward(model, img, header, **_reading_kw(kw))


def mosaic_coverage(J, model, header):
    """Per size class of the mosaic: how many transforms and how many non-zero quantised AC coefficients (3 channels)."""
    R = E.Reading(E.mosaic(), header, **MOSAIC_KW)
    where = R.layout(model["acs"])
    out = {}
    for s in E.KINDS:
        n = nz = 0
        if s in where:
            by, bx, g, off = where[s]
            idx = off[:, None] + np.arange(64 * E.COVERED[s][0] * E.COVERED[s][1])[None]
            n, nz = len(by), int(np.count_nonzero(model["coeffs"][g[:, None], :, idx]))
        out[s] = (n, nz)
    return out


def check_mosaic(J, model):
    """Every one of the 12 size classes is placed at least 4 times and carries at least 5 non-zero AC coefficients in
    total, and only then is the frame compared with the reading."""
    header = E.header_scalars(J, MOSAIC_KW["distance"])
    cov = mosaic_coverage(J, model, header)
    for s, (n, nz) in cov.items():
        assert n >= 4 and nz >= 5, (s, cov)
    return E.check_forward(model, E.mosaic(), header, **MOSAIC_KW)


def test_forward_cpu_model_every_size_class_matches_float64_reading(built):
    J = built
    check_mosaic(J, J.enc_forward_model(E.mosaic(), None, **MOSAIC_KW))
