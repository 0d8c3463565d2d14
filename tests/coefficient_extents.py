"""Coefficient extents of VarDCT streams and what the fast transform kernel (k_idct_fast) decides from them.

kend of a (varblock, channel) is the scan position after its last non-zero coefficient. The kernel takes its shortcuts per
WAVE: consecutive varblocks of one strategy in decode order, 64 / max(rows, columns) of them, share one. This module
restates those decisions in numpy, for the tests (from the kend the device produced) and for the CPU statistics of
measure_coefficient_extents.py (from the oracle's coefficients through the natural coefficient order)."""
import numpy as np

from host_tables_np import natural_order

COVERED_X = [1, 1, 1, 1, 2, 4, 1, 2, 1, 4, 2, 4, 1, 1, 1, 1, 1, 1, 8, 4, 8, 16, 8, 16, 32, 16, 32]
COVERED_Y = [1, 1, 1, 1, 2, 4, 2, 1, 4, 1, 4, 2, 1, 1, 1, 1, 1, 1, 8, 8, 4, 16, 16, 8, 32, 32, 16]
FAST_STRATEGIES = (0, 4, 5, 6, 7, 8, 9, 10, 11, 18, 19, 20)  # the DCT family up to 64x64: k_idct_fast
NAMES = {0: "8x8", 4: "16x16", 5: "32x32", 6: "16x8", 7: "8x16", 8: "32x8", 9: "8x32", 10: "32x16", 11: "16x32", 18: "64x64",
         19: "64x32", 20: "32x64"}  # rows x columns of pixels


def geometry(strategy):
    """(positions, lowest-frequency positions, threads per varblock, staging rounds of the prefetching form or 0)."""
    cx, cy = COVERED_X[strategy], COVERED_Y[strategy]
    size, tb = cx * cy * 64, max(cx, cy) * 8
    rounds = size // (tb * 4)
    return size, cx * cy, tb, (rounds if rounds <= 4 else 0)


def oracle_extents(o):
    """[(strategy, (kend X, kend Y, kend B))] of every varblock of an oracle decode with dumps, in decode order (groups in
    raster order, varblocks by their top-left block in raster order inside the group), through the natural coefficient
    order: for streams that code no coefficient orders of their own."""
    i = o.info
    yb, xb = i["ysize_blocks"], i["xsize_blocks"]
    acs = o.buffer("acs").reshape(yb, xb)
    coeffs = o.planes("coeffs")
    inverse = {}
    out = []
    xg = (i["xsize"] + 255) // 256
    for g in range(i["num_groups"]):
        gy, gx = divmod(g, xg)
        offset = 0
        for by in range(gy * 32, min(gy * 32 + 32, yb)):
            for bx in range(gx * 32, min(gx * 32 + 32, xb)):
                a = int(acs[by, bx])
                if not a & 1:
                    continue
                st = a >> 1
                size = COVERED_X[st] * COVERED_Y[st] * 64
                if st not in inverse:  # scan index of every natural position
                    order = np.asarray(natural_order(COVERED_X[st], COVERED_Y[st]))
                    inv = np.empty(size, np.int64)
                    inv[order] = np.arange(size)
                    inverse[st] = inv
                ke = []
                for c in range(3):
                    nz = np.flatnonzero(coeffs[g, c, offset:offset + size])
                    ke.append(int(inverse[st][nz].max()) + 1 if nz.size else 0)
                out.append((st, tuple(ke)))
                offset += size
    return out


def device_extents(ctx):
    """The same from a HipContext after its entropy stage, in the order of the transform work lists."""
    kend = ctx.download("kend")
    return [(int(s), tuple(int(v) for v in kend[b])) for s, b in ctx.download("transform_lists")]


def wave_decisions(extents):
    """Per k_idct_fast strategy: counts of what its waves do, from [(strategy, kend[3])] in list order.
    'waves'; 'llf_only' [3]: waves whose channel c is its lowest-frequency corner alone; 'skipped_rounds' / 'rounds': staging
    rounds (prefetching classes, per channel) no varblock of the wave reaches / all of them; 'full_waves': waves with a
    channel that takes no shortcut; 'kend_sum' [3], 'positions': sum of kend and of block sizes; 'blocks'."""
    by_strategy = {}
    for st, ke in extents:
        by_strategy.setdefault(st, []).append(ke)
    res = {}
    for st, kes in by_strategy.items():
        if st not in FAST_STRATEGIES:
            continue
        size, llf, tb, pr = geometry(st)
        ke = np.minimum(np.asarray(kes, np.int64).reshape(-1, 3), size)
        per_wave = 64 // tb
        r = dict(waves=0, llf_only=[0, 0, 0], skipped_rounds=0, rounds=0, full_waves=0, kend_sum=ke.sum(axis=0).tolist(),
                 positions=size * len(kes), blocks=len(kes))
        for w in range(0, len(kes), per_wave):
            top = ke[w:w + per_wave].max(axis=0)
            r["waves"] += 1
            full = False
            for c in range(3):
                if top[c] <= llf:
                    r["llf_only"][c] += 1
                    run = 0
                else:
                    run = 1 + sum(1 for k in range(1, pr) if top[c] > k * tb * 4) if pr else 1
                if pr:
                    r["rounds"] += pr
                    r["skipped_rounds"] += pr - run
                full = full or (run == pr if pr else top[c] > llf)
            r["full_waves"] += 1 if full else 0
        res[st] = r
    return res


def exercised(decisions):
    """Over all strategies: 'llf' = (wave, channel) pairs made from the corner alone, 'skip' = staging rounds left out in a
    (wave, channel) that stages others, 'full' = waves with a channel that takes no shortcut."""
    return dict(llf=sum(sum(d["llf_only"]) for d in decisions.values()),
                skip=sum(d["skipped_rounds"] - sum(d["llf_only"]) * geometry(st)[3] for st, d in decisions.items()),
                full=sum(d["full_waves"] for d in decisions.values()))
