#!/usr/bin/env python3
"""The cost estimate of the AC-strategy search on the device (jxlhip_enc_estimate_entropy): what one
4K frame's worth of candidates costs.

Workload: bench.py's seed-177 3840 x 2160 frame. The planes are formed here in float32 NumPy by the forward path's rules
(sRGB8 -> XYB, then four rounds of the inverse-Gaborish sharpening with clamped edges); the quant field and mask1x1 come
from the device entries on the planes BEFORE the sharpening, the transforms are taken of the planes after it. The
chroma-from-luma factors are 0 (the factor only scales Y's coefficients before a subtraction: it does not change the work).
Per 64x64 tile every aligned candidate of the ten kinds the reference's walk uses: 169 per full tile
(64 + 32 + 32 + 16 + 8 + 8 + 4 + 2 + 2 + 1), those that fit in the partial tiles of the bottom row.

  time    jxlhip_enc_estimate_last_ms (events around all launches, copies excluded): the median of --reps calls in each of
          --rounds fresh child processes, each under its own time limit and started only while the one before succeeded.
  bound   the multiply-adds of the four matrix passes (forward and inverse, rows and columns, three channels): per candidate
          of R x C samples 3 * 2 * R * C * (R + C), against the fp32 vector peak (--peak-tflops, two flops per multiply-add).
  --one-call  a single call (no repetition) for a kernel-trace run: rocprofv3 --kernel-trace --stats -- python this --one-call

  python scripts/measure_acs_estimate.py --out profiles/acs_estimate_mi355x.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

XS, YS = 3840, 2160
WALK_KINDS = {0: (1, 1), 6: (1, 2), 7: (2, 1), 4: (2, 2), 10: (2, 4), 11: (4, 2), 5: (4, 4), 19: (4, 8), 20: (8, 4), 18: (8, 8)}  # (cx, cy)


def xyb_planes(img):
    """sRGB8 [ys][xs][3] -> X, Y, B float32 [3][yp][xp], padded to whole blocks by edge replication (JPEG XL's opsin
    absorbance matrix and bias)."""
    import numpy as np
    ys, xs = img.shape[:2]
    v = img.astype(np.float32) / np.float32(255)
    lin = np.where(v <= 0.04045, v / np.float32(12.92), ((v + np.float32(0.055)) / np.float32(1.055)) ** np.float32(2.4)).astype(np.float32)
    lin = np.pad(lin, ((0, -ys % 8), (0, -xs % 8), (0, 0)), mode="edge")
    m = np.array([[0.30, 0.622, 0.078], [0.23, 0.692, 0.078], [0.24342268924547819, 0.20476744424496821, 0.55180986650955360]], np.float32)
    bias = np.float32(0.0037930732552754493)
    g = np.cbrt(lin @ m.T + bias) - np.cbrt(bias)
    return np.stack([0.5 * (g[..., 0] - g[..., 1]), 0.5 * (g[..., 0] + g[..., 1]), g[..., 2]]).astype(np.float32)


def sharpen(x, rounds=4):
    import numpy as np
    w1, w2 = np.float32(1.1 * 0.104699568), np.float32(1.1 * 0.055680538)
    nrm = np.float32(1.0) / (np.float32(1.0) + np.float32(4.0) * (w1 + w2))
    y = x.copy()
    _, h, w = x.shape
    for _ in range(rounds):
        p = np.pad(y, ((0, 0), (1, 1), (1, 1)), mode="edge")
        side = p[:, 1:h + 1, 0:w] + p[:, 1:h + 1, 2:w + 2] + p[:, 0:h, 1:w + 1] + p[:, 2:h + 2, 1:w + 1]
        corner = p[:, 0:h, 0:w] + p[:, 0:h, 2:w + 2] + p[:, 2:h + 2, 0:w] + p[:, 2:h + 2, 2:w + 2]
        y = y + (x - (y + w1 * side + w2 * corner) * nrm)
    return y.astype(np.float32)


def walk_candidates(J, xb, yb):
    import numpy as np
    parts = []
    for s, (cx, cy) in WALK_KINDS.items():
        by, bx = np.mgrid[0:yb - cy + 1:cy, 0:xb - cx + 1:cx]
        c = np.zeros(bx.size, J.ACS_CANDIDATE)
        c["strategy"], c["bx"], c["by"], c["entropy_mul"] = s, bx.ravel(), by.ravel(), 1.0
        parts.append(c)
    return np.concatenate(parts)


def child(args):
    import numpy as np
    import libjxl_amd as J
    img = J.synth_image(XS, YS, seed=177)
    before = xyb_planes(img)
    after = sharpen(before)
    ctx = J.HipContext(0)
    qf = J.initial_quant_field(before, 1.0, ctx=ctx)[0]
    mask = J.masking_1x1(before, ctx=ctx)
    yp, xp = before.shape[1:]
    tiles = ((yp + 63) // 64) * ((xp + 63) // 64)
    zeros = np.zeros(tiles, np.int8)
    cand = walk_candidates(J, xp // 8, yp // 8)
    ms = []
    for i in range(1 if args.one_call else args.warmup + args.reps):
        est = J.estimate_entropy(after, qf, mask, zeros, zeros, 1.0, cand, ctx=ctx)
        if args.one_call or i >= args.warmup:
            ms.append(ctx.enc_estimate_ms())
    assert np.isfinite(est).all() and (est > 0).all()
    ctx.close()
    per_kind = {int(s): int((cand["strategy"] == s).sum()) for s in WALK_KINDS}
    print("RESULT " + json.dumps({"estimate_ms": statistics.median(ms), "calls": len(ms), "candidates": int(len(cand)), "per_kind": per_kind,
                                  "estimate_sum": float(est.astype(np.float64).sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--one-call", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acs_estimate_mi355x.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=150)
    ap.add_argument("--peak-tflops", type=float, default=157.3, help="fp32 vector peak the bound is set against")
    args = ap.parse_args()
    if args.child or args.one_call:
        return child(args)
    rows = []
    for rnd in range(args.rounds):
        r = subprocess.run(["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--reps",
                            str(args.reps), "--warmup", str(args.warmup)], capture_output=True, text=True)
        sys.stdout.write(r.stdout[-1500:])
        sys.stdout.flush()
        if r.returncode != 0:  # nothing more is started on the device after a step that failed
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("child %d ended with status %d" % (rnd, r.returncode))
        rows.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
    med = [r["estimate_ms"] for r in rows]
    macs = sum(n * 3 * 2 * (64 * WALK_KINDS[int(s)][0] * WALK_KINDS[int(s)][1]) * 8 * (WALK_KINDS[int(s)][0] + WALK_KINDS[int(s)][1])
               for s, n in rows[0]["per_kind"].items())
    bound_ms = 2 * macs / (args.peak_tflops * 1e12) * 1e3
    rep = {"what": "jxlhip_enc_estimate_last_ms of one call over every aligned candidate of the walk's ten kinds in a %dx%d frame (seed 177, "
                   "d1.0); per process the median of %d calls, %d fresh processes" % (XS, YS, args.reps, args.rounds),
           "candidates": rows[0]["candidates"], "per_kind": rows[0]["per_kind"],
           "estimate_ms": {"process_medians": [round(v, 4) for v in med], "median": round(statistics.median(med), 4), "min": round(min(med), 4),
                           "max": round(max(med), 4)},
           "matrix_pass_multiply_adds": macs, "fp32_peak_tflops": args.peak_tflops, "bound_ms": round(bound_ms, 4),
           "fraction_of_bound": round(bound_ms / statistics.median(med), 4), "estimate_sum": rows[0]["estimate_sum"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
    print(json.dumps(rep, indent=1))


if __name__ == "__main__":
    main()
