"""CPU tests of the encode seam: the forward hook of the stream writer, without a GPU."""
import ctypes

import numpy as np
import pytest


def _hooks_call(J, img, p, names, want_stats=True):
    """jxlenc_encode_rgb8_hooks through ctypes with the CPU doubles named in `names` behind the hooks: (return code, the
    stream or None, JxlEncHookStats)."""
    E = J._enc_lib()
    hooks = J.EncHooks(**{k: ctypes.cast(getattr(E, "jxlenc_cpu_" + k), ctypes.c_void_p).value for k in names})
    out, n, st = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t(), J.EncHookStats()
    h = E.jxlenc_cpu_ctx_new()
    try:
        r = E.jxlenc_encode_rgb8_hooks(img.tobytes(), img.shape[1], img.shape[0], ctypes.byref(p), ctypes.byref(hooks), h, ctypes.byref(out),
                                       ctypes.byref(n), ctypes.byref(st) if want_stats else None)
    finally:
        E.jxlenc_cpu_ctx_free(h)
    return r, (J._finish(E, r, out, n, "jxlenc_encode_rgb8_hooks") if r == 0 else None), st


@pytest.mark.parametrize("kw", [dict(), dict(strategy_mode=0, distance=2.0), dict(gab=0, distance=0.5)])
def test_forward_hook_with_the_cpu_form_writes_the_same_stream(built, kw):
    """jxlenc_encode_rgb8_hooks hands the pixel-domain half to a function with jxlhip_enc_forward's signature; given
    the CPU form of that function (jxlenc_cpu_forward, without a context) the stream is byte-identical to
    jxlenc_encode_rgb8's: the descriptor (quantiser parameters, dequantisation tables) and the model hand-over lose nothing."""
    J = built
    E = J._enc_lib()
    img = J.synth_image(301, 143, seed=3)
    p = J._params(**kw)
    hooks = J.EncHooks(forward=ctypes.cast(E.jxlenc_cpu_forward, ctypes.c_void_p).value)
    out, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
    r = E.jxlenc_encode_rgb8_hooks(img.tobytes(), 301, 143, ctypes.byref(p), ctypes.byref(hooks), None, ctypes.byref(out), ctypes.byref(n), None)
    assert J._finish(E, r, out, n, "jxlenc_encode_rgb8_hooks") == J.encode_rgb8(img, **kw)


PAIR, TRIPLE = ["token_counts", "tokens"], ["histograms", "ans_sizes", "ans_write"]


@pytest.mark.parametrize("names", [["forward", "token_counts"], ["forward", "tokens"], ["forward"] + TRIPLE, ["forward", "tokens"] + TRIPLE,
                                   ["forward"] + PAIR + TRIPLE[:2], ["forward"] + PAIR + TRIPLE[1:], ["forward"] + PAIR + TRIPLE[::2],
                                   PAIR + TRIPLE])
def test_hook_entry_refuses_half_given_hooks(built, names):
    """A bad argument (-1): one of the token pair without the other, the entropy triple without the token pair, one of the
    triple missing, no forward function."""
    J = built
    r, data, _ = _hooks_call(J, J.synth_image(64, 48, seed=5), J._params(), names)
    assert r == -1 and data is None


@pytest.mark.parametrize("names", [["forward"], ["forward"] + PAIR, ["forward"] + PAIR + TRIPLE])
def test_hook_entry_routes_write_the_same_stream_and_count(built, names):
    """forward alone, forward + the token pair and all six hooks: each time jxlenc_encode_rgb8's bytes; the stats report
    tokens from behind the hooks exactly when the pair was given, tokens coded there exactly when all six were."""
    J = built
    img = J.synth_image(64, 48, seed=5)
    r, data, st = _hooks_call(J, img, J._params(), names)
    assert r == 0 and data == J.encode_rgb8(img)
    assert (st.device_tokens > 0) == (len(names) >= 3) and (st.device_coded > 0) == (len(names) == 6)
    assert st.device_coded in (0, st.device_tokens)
    assert _hooks_call(J, img, J._params(), names, want_stats=False)[1] == data  # (stats may be NULL)
    assert _hooks_call(J, img, J._params(upsampling=2), names)[0] == -1


def test_forward_model_shapes_and_refusals(built):
    J = built
    img = J.synth_image(300, 270, seed=4)
    m = J.enc_forward_model(img)  # CPU form
    assert m["acs"].shape == (34, 38) and m["coeffs"].shape == (4, 3, 65536)
    first = (m["acs"] & 1) == 1
    assert (m["qf"][first] >= 1).all() and (m["qf"][~first] == 0).all()
    # every block is covered by exactly one transform: the covered areas of the first blocks add up to the frame
    cov_x = np.array([1, 1, 1, 1, 2, 4, 1, 2, 1, 4, 2, 4, 1, 1, 1, 1, 1, 1, 8, 4, 8, 16, 8, 16, 32, 16, 32])
    cov_y = np.array([1, 1, 1, 1, 2, 4, 2, 1, 4, 1, 4, 2, 1, 1, 1, 1, 1, 1, 8, 8, 4, 16, 16, 8, 32, 32, 16])
    st = m["acs"][first] >> 1
    assert (cov_x[st] * cov_y[st]).sum() == 34 * 38
    with pytest.raises(J.JxlAmdError):
        J.enc_forward_model(img, None, strategy_mode=2)  # the random tiling mode is not a forward-path mode
