"""encode_rgb8_gpu(device_entropy=True): the AC tokens counted and rANS-coded on the device (k_enc_hist, k_enc_ans_records,
k_enc_ans_chain, k_enc_ans_scatter) against the host coder, byte for byte and bit for bit."""
import numpy as np
import pytest

import entropy_cases as ec

pytestmark = pytest.mark.gpu

STREAMS = [((777, 555), {}), ((301, 143), dict(distance=0.5)), ((1024, 768), dict(num_histograms=3, distance=2.0)),
           ((640, 333), dict(strategy_mode=0, cfl_fit=1)), ((256, 256), dict(distance=8.0)), ((2048, 1111), dict(cfl_fit=1)), ((8, 8), {}),
           ((263, 9), dict(distance=0.3)), ((301, 143), dict(max_clusters=1)), ((520, 300), dict(distance=0.3))]
FALLBACKS = [dict(ac_code_mode=1), dict(ac_code_mode=2), dict(ac_code_mode=3), dict(num_passes=2)]


def _same_stream(J, size, kw):
    img = J.synth_image(size[0], size[1], seed=size[0] + 3)
    ctx = J.HipContext()
    try:
        host = J.encode_rgb8_gpu(img, ctx, **kw)
        tt, te = {}, {}
        tok = J.encode_rgb8_gpu(img, ctx, timings=tt, device_tokens=True, **kw)
        dev = J.encode_rgb8_gpu(img, ctx, timings=te, device_entropy=True, **kw)
        again = J.encode_rgb8_gpu(img, ctx, **kw)  # the context serves the three forms in any order
        guards = ctx.check_guards()
    finally:
        ctx.close()
    assert host == again and tok == host
    assert dev == host, (len(dev), len(host))
    assert te["device_tokens"] == tt["device_tokens"]
    return tt, te, guards


@pytest.mark.parametrize("size,kw", STREAMS)
def test_device_entropy_writes_the_same_stream(built, size, kw):
    """Counts from the device -> the host's clustering and normalisation -> tables down -> every group's bit string up:
    the codestream is the host coder's, byte for byte, and every token the device produced was coded there."""
    tt, te, _ = _same_stream(built, size, kw)
    assert te["device_entropy"] == tt["device_tokens"] > 0
    assert te["entropy_kernels_ms"] > 0


@pytest.mark.parametrize("kw", FALLBACKS)
def test_device_route_falls_back_to_the_host_coder(built, kw):
    """Prefix codes, LZ77 and several passes stay with the host coder: 0 tokens coded on the device, the same stream."""
    _, te, _ = _same_stream(built, (301, 143), kw)
    assert te["device_entropy"] == 0


@pytest.mark.parametrize("n,clusters,log_alpha,special", ec.CASES, ids=ec.IDS)
def test_device_writer_equals_the_host_writer(built, n, clusters, log_alpha, special):
    """jxlhip_debug_ans_write against jxlenc_ans_write_tokens on the same tokens and code: the same length in bits, the same
    bytes (so the padding is zero), and the string decodes back through ans_np to the tokens with the coder in its start
    state. jxlhip_enc_histograms on the same resident tokens: exactly np.add.at's counts."""
    J = built
    c = ec.case(n, clusters, log_alpha, special)
    t = ec.tables(J, c, (3, 6))
    want, want_bits = J.ans_write_tokens(c["tokens"], t)
    ctx = J.HipContext()
    try:
        got, bits = ctx.debug_ans_write(c["tokens"], t)
        counts, mx = ctx.enc_histograms(c["num_ctx"], ec.CFG)
        ms = ctx.enc_entropy_ms()
    finally:
        ctx.close()
    assert bits == want_bits
    assert got == want
    prefix, values = ec.decode_back(got, bits, c, 3)
    assert prefix == 6 and np.array_equal(values, c["tokens"][:, 1])
    sym = ec.symbols(c["tokens"][:, 1])
    ref = np.zeros((c["num_ctx"], 256), np.uint32)
    np.add.at(ref, (c["tokens"][:, 0], sym), 1)
    assert np.array_equal(counts, ref) and mx == sym.max()
    assert ms[0] > 0 and ms[1] > 0


def _refusals(J, ctx):
    """Tables and tokens the entry points refuse at validation (nothing here relies on the device catching an access)."""
    c = ec.case(4097, 5, 8, None)
    t = ec.tables(J, c)
    good, bits = J.ans_write_tokens(c["tokens"], t)
    sym = int(ec.symbols(c["tokens"][:1, 1])[0])
    k = int(c["ctx_map"][c["tokens"][0, 0]])
    # a used symbol whose frequency is zero, in a cluster that still sums to 4096 with the right running sums: the tables
    # pass, the token raises its group's flag
    zero = dict(c)
    zero["freq"] = c["freq"].astype(np.int64)
    other = int(np.argmax(np.where(np.arange(256) == sym, 0, zero["freq"][k])))
    zero["freq"][k, other] += zero["freq"][k, sym]
    zero["freq"][k, sym] = 0
    zero["rev_start"], zero["rev"] = ec.tables_of(zero["freq"], c["log_alpha"])
    with pytest.raises(J.JxlAmdError):
        ctx.debug_ans_write(c["tokens"], ec.tables(J, zero))
    m = dict(c)
    m["ctx_map"] = c["ctx_map"].copy()
    m["ctx_map"][3] = 5  # a cluster that does not exist
    with pytest.raises(J.JxlAmdError):
        ctx.debug_ans_write(c["tokens"], ec.tables(J, m))
    bad = c["tokens"].copy()
    bad[4000, 0] = c["num_ctx"]  # a context beyond the map
    with pytest.raises(J.JxlAmdError):
        ctx.debug_ans_write(bad, t)
    with pytest.raises(J.JxlAmdError):
        ctx.enc_histograms(c["num_ctx"], ec.CFG)
    with pytest.raises(J.JxlAmdError):
        ctx.debug_ans_write(c["tokens"], t, capacity=len(good) - 1)
    got, got_bits = ctx.debug_ans_write(c["tokens"], t)
    assert (got, got_bits) == (good, bits)


def test_bad_tables_and_tokens_are_refused(built):
    J = built
    ctx = J.HipContext()
    try:
        _refusals(J, ctx)
        img = J.synth_image(301, 143, seed=304)
        assert J.encode_rgb8_gpu(img, ctx, device_entropy=True) == J.encode_rgb8(img)  # the context still encodes
    finally:
        ctx.close()


@pytest.mark.parametrize("part", ["small frames", "large frames", "sections"])
@pytest.mark.parametrize("byte", ["0xA5", "0xFF"])
def test_guard_bands_stay_clean(built, monkeypatch, byte, part):
    """JXLHIP_GUARD=1, two fills: no kernel of the route writes next to a buffer, none reads what nothing wrote (the streams
    and bit strings are the same under both fills)."""
    J = built
    monkeypatch.setenv("JXLHIP_GUARD", "1")
    monkeypatch.setenv("JXLHIP_GUARD_BYTE", byte)
    for size, kw in STREAMS:
        if part != ("large frames" if size[0] * size[1] > 640 * 333 else "small frames"):
            continue
        _, te, guards = _same_stream(J, size, kw)
        assert guards == 0 and te["device_entropy"] > 0, (size, kw, guards)
    if part != "sections":
        return
    for case in [(65, 5, 8, "skewed"), (4097, 5, 8, "single"), (20000, 5, 5, "skewed")]:
        c = ec.case(*case)
        t = ec.tables(J, c, (2, 1))
        ctx = J.HipContext()
        try:
            got = ctx.debug_ans_write(c["tokens"], t)
            counts, _ = ctx.enc_histograms(c["num_ctx"], ec.CFG)
            assert ctx.check_guards() == 0
        finally:
            ctx.close()
        assert got == J.ans_write_tokens(c["tokens"], t)
        assert counts.sum() == len(c["tokens"])
    ctx = J.HipContext()
    try:
        _refusals(J, ctx)
        assert ctx.check_guards() == 0
    finally:
        ctx.close()
