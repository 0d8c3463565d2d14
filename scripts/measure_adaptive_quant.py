#!/usr/bin/env python3
"""The adaptive quant field on the device (adaptive_quant=1): what it costs, and that the default mode
costs what it did. One 3840 x 2160 frame (bench.py's seed 177, cfl_fit=1, device_tokens=True), the method of
scripts/measure_device_entropy.py: a fresh process per leg, the parent commit's build and this one alternating in one call,
each under its own `timeout -k 10` and only while the one before succeeded.

  mode 0   jxlhip_enc_last_ms of an encode (median of --reps) and of 20 replays of its kernel sequence on the resident
           input (jxlhip_enc_forward_rerun), and the `bench.py --workload encode` line: parent against this build. The bar
           is the spread between the parent's own processes; this build's median has to lie inside it.
  mode 1   the same two times with the field on, the time of its two kernels alone (events around them,
           jxlhip_enc_aq_last_ms, median over the replays), their algorithmic traffic, achieved GB/s and its fraction of the
           HBM peak as bench.py defines it.
  streams  bytes and PSNR (oracle decode against the input) of the frame in both modes at d1.0 and d4.0. No claim attached.

  python scripts/measure_adaptive_quant.py --parent-tree PARENT --out profiles/adaptive_quant_mi355x.json
(PARENT: a checkout of the parent commit with its libraries built.)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

HBM_PEAK_GBS = 8000.0  # as bench.py
XS, YS = 3840, 2160


def child(args):
    import numpy as np
    import libjxl_amd as J
    if args.build:
        J.LIB_PATH = os.path.abspath(os.path.join(args.build, "libjxl_amd.so"))
        J.ENC_PATH = os.path.abspath(os.path.join(args.build, "libjxlenc.so"))
    img = J.synth_image(XS, YS, seed=177)
    ctx = J.HipContext(0)
    out = {}
    for mode in [int(m) for m in args.modes.split(",")]:
        kw = dict(distance=1.0, cfl_fit=1, device_tokens=True)
        if mode:
            kw["adaptive_quant"] = 1
        ms = []
        for i in range(args.warmup + args.reps):
            t = {}
            J.encode_rgb8_gpu(img, ctx, timings=t, **kw)
            if i >= args.warmup:
                ms.append(t["kernels_ms"])
        row = {"last_ms": statistics.median(ms)}
        replay, aq = [], []
        for _ in range(args.reps):
            replay.append(ctx.enc_rerun(20)[0] / 20)
            if mode:
                aq.append(ctx.enc_aq_ms())
        row["replay_ms"] = statistics.median(replay)
        if mode:
            row["aq_kernels_ms"] = statistics.median(aq)
        out["mode%d" % mode] = row
    if args.streams:
        import jxlo
        rows = {}
        for d in (1.0, 4.0):
            for mode in (0, 1):
                data = J.encode_rgb8_gpu(img, ctx, distance=d, cfl_fit=1, device_tokens=True, adaptive_quant=mode)
                back = jxlo.Decoded(data, dumps=False).rgb8
                mse = float(np.mean((back.astype(np.float64) - img) ** 2))
                rows["d%.1f mode %d" % (d, mode)] = {"bytes": len(data), "psnr_db": round(10 * np.log10(255.0 ** 2 / mse), 3)}
        out["streams"] = rows
    ctx.close()
    print("RESULT " + json.dumps(out))


def run(cmd, timeout_s, what):
    r = subprocess.run(["timeout", "-k", "10", str(timeout_s)] + cmd, capture_output=True, text=True)
    sys.stdout.write(r.stdout[-1500:])
    sys.stdout.flush()
    if r.returncode != 0:  # nothing more is started on the device after a step that failed
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("step %s ended with status %d" % (what, r.returncode))
    return r.stdout


def spread(vals):
    return {"process_medians": [round(v, 5) for v in vals], "median": round(statistics.median(vals), 5), "min": round(min(vals), 5),
            "max": round(max(vals), 5)}


def driver(args):
    me = os.path.abspath(__file__)
    parent_build = os.path.join(args.parent_tree, "libjxl_amd", "_build")
    common = ["--reps", str(args.reps), "--warmup", str(args.warmup)]
    kern = {"parent": [], "this": []}
    bench = {"parent": [], "this": []}
    streams = None
    for rnd in range(args.rounds):
        order = ("parent", "this") if rnd % 2 == 0 else ("this", "parent")
        for who in order:
            cmd = [sys.executable, me, "--child", "--modes", "0" if who == "parent" else "0,1"] + common
            if who == "parent":
                cmd += ["--build", parent_build]
            elif streams is None:
                cmd += ["--streams"]
            o = run(cmd, args.step_timeout, "%s kernels (round %d)" % (who, rnd))
            res = json.loads([l for l in o.splitlines() if l.startswith("RESULT ")][-1][7:])
            streams = res.pop("streams", streams)
            kern[who].append(res)
        for who in order:
            tree = args.parent_tree if who == "parent" else ROOT
            o = run([sys.executable, os.path.join(tree, "bench.py"), "--workload", "encode", "--gpus", "1", "--steps", str(args.bench_steps),
                     "--warmup", "3"], args.step_timeout, "%s bench (round %d)" % (who, rnd))
            line = json.loads([l for l in o.splitlines() if l.startswith("{")][-1])
            bench[who].append({"value": line["value"], "unit": line.get("unit"), "e2e": line.get("e2e")})
    xp, yp = (XS + 7) // 8 * 8, (YS + 7) // 8 * 8
    plane = xp * yp * 4
    # three planes read once by the block kernel, Y once more by the cell kernel (its row and column halos are re-reads of
    # lines that sit in L2), the cell image written and read once, the two outputs
    traffic = 3 * plane + plane + 2 * (plane // 16) + 2 * (plane // 64)
    rep = {"what": "one %dx%d d1.0 frame (seed 177, cfl_fit=1, device_tokens=True); per process the median of %d encodes / replays, %d "
                   "processes per row, parent and this build alternating" % (XS, YS, args.reps, args.rounds)}
    m0 = {}
    for key in ("last_ms", "replay_ms"):
        p, t = [r["mode0"][key] for r in kern["parent"]], [r["mode0"][key] for r in kern["this"]]
        m0[key] = {"parent": spread(p), "this": spread(t), "this_median_inside_parent_spread": min(p) <= statistics.median(t) <= max(p)}
    pb, tb = [b["value"] for b in bench["parent"]], [b["value"] for b in bench["this"]]
    m0["bench_encode_value"] = {"unit": bench["this"][0]["unit"], "parent": spread(pb), "this": spread(tb),
                                "this_median_inside_parent_spread": min(pb) <= statistics.median(tb) <= max(pb)}
    rep["mode0"] = m0
    aq = [r["mode1"]["aq_kernels_ms"] for r in kern["this"]]
    gbs = traffic / (statistics.median(aq) * 1e-3) / 1e9
    rep["mode1"] = {"last_ms": spread([r["mode1"]["last_ms"] for r in kern["this"]]),
                    "replay_ms": spread([r["mode1"]["replay_ms"] for r in kern["this"]]), "aq_kernels_ms": spread(aq),
                    "algorithmic_bytes": traffic, "achieved_gbs": round(gbs, 1), "hbm_peak_gbs": HBM_PEAK_GBS,
                    "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
    rep["streams"] = streams
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
    print(json.dumps(rep, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--build")
    ap.add_argument("--modes", default="0")
    ap.add_argument("--streams", action="store_true")
    ap.add_argument("--parent-tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_quant_mi355x.json"))
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=150)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_tree:
        raise SystemExit("--parent-tree is needed (see the module's text)")
    driver(args)


if __name__ == "__main__":
    main()
