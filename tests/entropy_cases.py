"""Seeded token sets and ANS codes for the entropy-coder tests (host writer and device kernels alike). The codes are built
here from the *decoder's* tables (ans_np.alias_table), not by the encoder under test: normalised counts, their running sums
and the slot of every (symbol, offset)."""
import functools

import numpy as np

import ans_np

CFG = (4, 2, 0)  # split_exp, msb_in_token, lsb_in_token: the AC streams' configuration
SIZES = (1, 2, 63, 64, 65, 4097, 20000)
# (tokens, clusters, log_alpha, special cluster form or None)
CASES = [(n, k, la, None) for n in SIZES for k, la in ((1, 5), (1, 8), (5, 5), (5, 8))] + \
        [(65, 5, 5, "single"), (4097, 5, 8, "single"), (65, 5, 8, "skewed"), (20000, 5, 5, "skewed"), (20000, 1, 8, "skewed")]
IDS = ["n%d-k%d-a%d%s" % (n, k, la, "-" + sp if sp else "") for n, k, la, sp in CASES]


def symbols(values, cfg=CFG):
    """Hybrid-uint symbol of every value (dec_ans.h:226-257 read backwards)."""
    split_exp, msb, lsb = cfg
    v = np.asarray(values, np.uint64)
    n = (np.frexp(np.maximum(v, 1).astype(np.float64))[1] - 1).astype(np.uint64)  # floor(log2 v), exact below 2^53
    m = v - (np.uint64(1) << n)
    big = np.uint64(1 << split_exp) + ((n - np.uint64(split_exp)) << np.uint64(msb + lsb)) + \
        ((m >> (n - np.uint64(msb))) << np.uint64(lsb)) + (m & np.uint64((1 << lsb) - 1))
    return np.where(v < (1 << split_exp), v, big).astype(np.uint32)


def normalise(counts):
    """Frequencies summing to 4096, at least 1 for every symbol that occurs."""
    counts = np.asarray(counts, np.int64)
    total = counts.sum()
    f = np.zeros(256, np.int64)
    if total == 0:
        f[0] = 4096
        return f
    used = counts > 0
    f[used] = np.maximum(1, counts[used] * 4096 // total)
    while f.sum() != 4096:
        i = int(np.argmax(f))
        step = 4096 - f.sum()
        f[i] += max(step, 1 - f[i])
    return f


def tables_of(freqs, log_alpha):
    """freq -> (rev_start, rev): the running sums and the inverse of the decoder's alias table."""
    k = len(freqs)
    rev_start = np.zeros((k, 256), np.uint16)
    rev = np.zeros((k, 4096), np.uint16)
    log_entry = 12 - log_alpha
    for c in range(k):
        start = np.concatenate([[0], np.cumsum(freqs[c])[:-1]])
        rev_start[c] = np.where(np.asarray(freqs[c]) > 0, start, 0)
        table = ans_np.alias_table(freqs[c], log_alpha)
        seen = np.zeros(4096, bool)
        for slot in range(4096):
            idx, pos = slot >> log_entry, slot & ((1 << log_entry) - 1)
            cut, rv, f0, o1, f1 = table[idx]
            sym, off = (rv, o1 + pos) if pos >= cut else (idx, pos)
            at = int(start[sym]) + off
            assert off < freqs[c][sym] and not seen[at]
            seen[at] = True
            rev[c, at] = slot
        assert seen.all()
    return rev_start, rev


@functools.lru_cache(maxsize=None)
def case(n, clusters, log_alpha, special):
    """-> dict(tokens (n, 2) uint32, ctx_map, freq, rev_start, rev, log_alpha, num_ctx)."""
    rng = np.random.default_rng(1000 * n + 10 * clusters + log_alpha + (7 if special else 0))
    num_ctx = 3 * clusters + 2
    ctx_map = np.concatenate([np.arange(clusters), rng.integers(0, clusters, num_ctx - clusters)]).astype(np.uint8)
    rng.shuffle(ctx_map)
    ctx = rng.integers(0, num_ctx, n).astype(np.uint32)
    top = 255 if log_alpha == 5 else (1 << 20)  # symbols stay below 1 << log_alpha; extra bits reach 18
    small = rng.geometric(0.25, n) - 1
    wide = np.exp2(rng.uniform(0, np.log2(top), n)).astype(np.int64)
    val = np.where(rng.random(n) < 0.7, small, wide)
    if n >= 3:
        val[rng.integers(0, n)] = top  # the largest value, so the longest run of extra bits, occurs
    val = np.minimum(val, top).astype(np.uint32)
    cluster = ctx_map[ctx]
    last = clusters - 1
    if special == "single":  # the last cluster holds one symbol: frequency 4096, a coder state that never moves
        val[cluster == last] = 5
    if special == "skewed":  # ... or two, of frequencies 4095 and 1
        mine = np.flatnonzero(cluster == last)
        val[mine] = 2
        if len(mine):
            val[mine[rng.random(len(mine)) < 0.02]] = 300 if log_alpha == 8 else 77
            val[mine[-1]] = 300 if log_alpha == 8 else 77
    sym = symbols(val)
    assert sym.max(initial=0) < (1 << log_alpha)
    freq = np.zeros((clusters, 256), np.int64)
    for c in range(clusters):
        freq[c] = normalise(np.bincount(sym[cluster == c], minlength=256))
    if special == "skewed":
        freq[last] = 0
        freq[last, symbols([2])[0]] = 4095
        freq[last, symbols([300 if log_alpha == 8 else 77])[0]] = 1
    if special == "single":
        assert freq[last].max() == 4096
    rev_start, rev = tables_of(freq, log_alpha)
    tokens = np.stack([ctx, val], axis=1).astype(np.uint32)
    return dict(tokens=tokens, ctx_map=ctx_map, freq=freq.astype(np.uint16), rev_start=rev_start, rev=rev, log_alpha=log_alpha,
                num_ctx=num_ctx)


def tables(J, c, prefix=(0, 0)):
    return J.AnsTables(c["ctx_map"], c["freq"], c["rev_start"], c["rev"], c["log_alpha"], CFG, prefix)


def decode_back(data, nbits, c, prefix_bits=0):
    return ans_np.decode(data, nbits, c["tokens"][:, 0], c["ctx_map"], c["freq"].astype(np.int64), c["log_alpha"], CFG, prefix_bits)
