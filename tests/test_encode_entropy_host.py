"""The host side of the device entropy route (encode_rgb8_gpu(device_entropy=True)) without a GPU: the host rANS writer on
caller-supplied codes against an independent decoder, and the whole hook route with CPU doubles behind the hooks."""
import numpy as np
import pytest

import entropy_cases as ec


@pytest.mark.parametrize("n,clusters,log_alpha,special", ec.CASES, ids=ec.IDS)
def test_host_writer_decodes_back(built, n, clusters, log_alpha, special):
    """jxlenc_ans_write_tokens (WriteTokens on a caller's code) -> ans_np.decode: the same tokens, every bit consumed, the
    padding zero and the coder back in its start state 0x13 << 16. The prefix bits come back too."""
    J = built
    c = ec.case(n, clusters, log_alpha, special)
    for prefix in ((0, 0), (3, 5)):
        data, bits = J.ans_write_tokens(c["tokens"], ec.tables(J, c, prefix))
        assert len(data) == (bits + 7) // 8
        got_prefix, values = ec.decode_back(data, bits, c, prefix[0])
        assert got_prefix == prefix[1]
        assert np.array_equal(values, c["tokens"][:, 1])


def test_host_writer_refuses_what_it_cannot_code(built):
    J = built
    c = ec.case(65, 5, 8, None)
    t = ec.tables(J, c)
    bad = c["tokens"].copy()
    bad[7, 0] = c["num_ctx"]
    with pytest.raises(J.JxlAmdError):
        J.ans_write_tokens(bad, t)
    zero = dict(c)
    sym = int(ec.symbols(c["tokens"][:1, 1])[0])
    k = int(c["ctx_map"][c["tokens"][0, 0]])
    zero["freq"] = c["freq"].copy()
    zero["freq"][k, sym] = 0  # (the cluster no longer sums to 4096 either)
    with pytest.raises(J.JxlAmdError):
        J.ans_write_tokens(c["tokens"], ec.tables(J, zero))
    m = dict(c)
    m["ctx_map"] = c["ctx_map"].copy()
    m["ctx_map"][3] = 5
    with pytest.raises(J.JxlAmdError):
        J.ans_write_tokens(c["tokens"], ec.tables(J, m))
    data, bits = J.ans_write_tokens(c["tokens"], t)
    with pytest.raises(J.JxlAmdError):
        J.ans_write_tokens(c["tokens"], t, capacity=len(data) - 1)


ROUTE = [((8, 8), {}), ((263, 9), {}), ((301, 143), dict(distance=0.5)), ((600, 520), dict(num_histograms=3)), ((256, 256), dict(distance=8.0)),
         ((301, 143), dict(max_clusters=1))]


@pytest.mark.parametrize("size,kw", ROUTE)
def test_hook_route_with_cpu_doubles_writes_the_same_stream(built, size, kw):
    """Counts from the hook -> BuildCodeFromCounts -> tables down -> bit strings up -> BitWriter::AppendBits, against
    jxlenc_encode_rgb8 which counts, builds and writes in one place: byte for byte. (8, 8) and (263, 9) are single-group
    frames, where the AC group follows AC global inside one section at an arbitrary bit position."""
    J = built
    img = J.synth_image(size[0], size[1], seed=size[0] + 3)
    want = J.encode_rgb8(img, **kw)
    t = {}
    got = J.encode_rgb8_hooks_cpu(img, timings=t, **kw)
    assert got == want, (len(got), len(want))
    assert t["device_entropy"] == t["device_tokens"] > 0


@pytest.mark.parametrize("kw", [dict(ac_code_mode=1), dict(ac_code_mode=2), dict(ac_code_mode=3), dict(num_passes=2)])
def test_hook_route_falls_back_to_the_host_coder(built, kw):
    """Prefix codes, LZ77 and several passes are the host coder's: the route reports 0 tokens coded behind the hook and the
    stream is still jxlenc_encode_rgb8's."""
    J = built
    img = J.synth_image(301, 143, seed=304)
    t = {}
    got = J.encode_rgb8_hooks_cpu(img, timings=t, **kw)
    assert t["device_entropy"] == 0
    assert got == J.encode_rgb8(img, **kw)
