"""Fits the per-section cost model of libjxl_amd/csrc/host/jxh_launch_order.h on the CPU: tokens ~ a * bytes + b * blocks + c.

Token counts come from the stream writer's tokeniser (enc_tokens on a CpuEncContext), byte sizes from the oracle's section
table, block counts from the forward model's AC-strategy map. No GPU. For every stream it also replays the lane queue with
the true token counts and with the fitted estimate and prints how the two rank the frames.

usage: fit_entropy_cost.py [XSIZE YSIZE] [--check A B C]   (default 1024 768; --check skips the fit and ranks with A, B, C)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from launch_order_streams import SEEDS, sections_of  # noqa: E402  (tests/)


def replay(costs, lanes):
    """The kernel's queue: sections in the given order, each to the lane that is free first; the busiest lane's end."""
    free = [0] * lanes
    for c in costs:
        i = free.index(min(free))
        free[i] += int(c)
    return max(free)


def lanes_of(bytes_, section_bytes=4000):
    """PrepareBatch's dense regime: one wave of up to 64 lanes per unit."""
    return min(64, len(bytes_))


def main():
    import libjxl_amd as J
    import jxlo
    J.build()
    jxlo.build()
    args = sys.argv[1:]
    check = None
    if "--check" in args:
        i = args.index("--check")
        check = [float(v) for v in args[i + 1:i + 4]]
        args = args[:i]
    xsize, ysize = (int(args[0]), int(args[1])) if len(args) >= 2 else (1024, 768)
    per = [sections_of(J, jxlo, xsize, ysize, s) for s in SEEDS]
    rows = np.concatenate(per)
    A = np.stack([rows[:, 0], rows[:, 1], np.ones(len(rows))], 1).astype(np.float64)
    if check is None:
        coef, *_ = np.linalg.lstsq(A, rows[:, 2].astype(np.float64), rcond=None)
    else:
        coef = np.array(check)
    pred = A @ coef
    r = np.corrcoef(pred, rows[:, 2])[0, 1]
    old = np.corrcoef(rows[:, 0] + 4000, rows[:, 2])[0, 1]
    print("%dx%d: %d sections; tokens ~ %.4f * bytes + %.3f * blocks + %.1f   (r = %.4f; bytes + 4000: r = %.4f)"
          % (xsize, ysize, len(rows), coef[0], coef[1], coef[2], r, old))
    true_t, est_t, old_t = [], [], []
    for seed, p in zip(SEEDS, per):
        order = np.argsort(-p[:, 0], kind="stable")  # largest bytes first, as the section list is
        lanes = lanes_of(p[:, 0])
        e = np.maximum(0, np.rint(np.stack([p[:, 0], p[:, 1], np.ones(len(p))], 1) @ coef)).astype(np.int64)
        true_t.append(replay(p[order, 2], lanes))
        est_t.append(replay(e[order], lanes))
        old_t.append(replay(p[order, 0] + 4000, lanes))
        print("seed %d: sections %d lanes %d  bytes %d  blocks %d  tokens %d  longest lane: true %d  estimate %d  bytes+4000 %d"
              % (seed, len(p), lanes, p[:, 0].sum(), p[:, 1].sum(), p[:, 2].sum(), true_t[-1], est_t[-1], old_t[-1]))

    def ranks(v):
        return np.argsort(np.argsort(-np.array(v), kind="stable"), kind="stable")

    def spearman(a, b):
        return float(np.corrcoef(ranks(a), ranks(b))[0, 1])
    print("frame order by true finishing time:", np.argsort(-np.array(true_t), kind="stable").tolist())
    print("frame order by the estimate:       ", np.argsort(-np.array(est_t), kind="stable").tolist())
    print("Spearman rank agreement over the eight frames: estimate %.3f, bytes + 4000: %.3f" % (spearman(true_t, est_t), spearman(true_t, old_t)))


if __name__ == "__main__":
    main()
