#!/usr/bin/env python3
"""The transform stage alone on the benchmark's frames, with and without the shortcuts k_idct_fast takes from the
coefficient counts.

64 resident 3840 x 2160 d1.0 frames (bench.py's seeds 177, 178, ... cycled), entropy once, then the batched transform
launches of the set alone, from the HIP events around them (jxlhip_last_stage_ms(1)).

  (a) parent           the library of the parent commit (--parent-lib)
  (b) this             this tree's library
  (c) this, dense      the same with the option "transform_dense": the same kernels taking no shortcut
  (d) all rounds       optional (--variant-lib): a library of this tree in which `rounds()` of k_idct_fast returns PR for
                       every channel that stages at all: channels made from their lowest-frequency corner alone, but no
                       staging round left out beside staged ones (part 2 of DESIGN.md 8.3 on its own)

Every number is the median of --reps launches in one process; the driver starts one process per library and round,
alternating the libraries, each under its own `timeout -k 10` and only while the one before succeeded, and writes the
per-process medians and their spread into the section "stage" of the json --out names (its other sections stay).

  python scripts/measure_sparse_transform.py --parent-lib PARENT/libjxl_amd.so [--variant-lib VARIANT/libjxl_amd.so] \\
         --out profiles/sparse_transform_mi355x.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import libjxl_amd as J
    J.LIB_PATH = os.path.abspath(args.lib)
    import numpy as np
    frames = [J.Frame(J.encode_rgb8(J.synth_image(3840, 2160, 177 + i), distance=1.0, strategy_mode=1), threads=8) for i in range(args.distinct)]
    out = {}
    for case in args.cases.split(","):
        ctxs = [J.HipContext(0) for _ in range(args.frames)]
        for i, c in enumerate(ctxs):
            if case == "dense":
                c.set_option("transform_dense", 1)
            c.upload(frames[i % len(frames)])
        J.run_entropy_batch(ctxs)
        ms = []
        for i in range(args.warmup + args.reps):
            J.run_transform_batch(ctxs)
            ctxs[0].sync()
            if i >= args.warmup:
                ms.append(ctxs[0].stage_ms(1))
        planes = ctxs[-1].download("xyb_idct")
        out[case] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "frames": args.frames,
                     "plane_sum": float(np.sum(planes, dtype=np.float64))}
        for c in ctxs:
            c.close()
    for f in frames:
        f.close()
    print("RESULT " + json.dumps(out))


def driver(args):
    libs = [("parent", args.parent_lib, "plain"), ("this", os.path.join(ROOT, "libjxl_amd", "_build", "libjxl_amd.so"), "plain,dense")]
    if args.variant_lib:
        libs.append(("variant", args.variant_lib, "plain"))
    keys = {("parent", "plain"): "a_parent", ("this", "plain"): "b_this", ("this", "dense"): "c_this_dense", ("variant", "plain"): "d_all_rounds"}
    runs, sums = {}, {}
    for rnd in range(args.rounds):
        for name, lib, cases in (libs if rnd % 2 == 0 else libs[::-1]):
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--lib", lib, "--cases", cases,
                   "--frames", str(args.frames), "--reps", str(args.reps), "--warmup", str(args.warmup), "--distinct", str(args.distinct)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout[-2000:])
            sys.stdout.flush()
            if r.returncode != 0:  # nothing more is started on the device after a step that failed
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit("step %s (round %d) ended with status %d" % (name, rnd, r.returncode))
            res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            for case, v in res.items():
                runs.setdefault(keys[(name, case)], []).append(v["median_ms"])
                sums.setdefault(keys[(name, case)], []).append(v["plane_sum"])
    report = {"what": "all transform launches of %d resident 3840x2160 d1.0 frames, ms per set; median of %d launches per process, "
                      "%d processes per row, libraries alternating" % (args.frames, args.reps, args.rounds),
              "frames": args.frames, "rows": {}}
    for k in sorted(runs):
        v = runs[k]
        report["rows"][k] = {"process_medians_ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4),
                             "spread_ms": round(max(v) - min(v), 4), "ms_per_640_frames": round(statistics.median(v) * 640.0 / args.frames, 3),
                             "plane_sum": sums[k][0], "plane_sum_same_in_every_process": len(set(sums[k])) == 1}
    rows = report["rows"]
    report["b_over_a"] = round(rows["b_this"]["median_ms"] / rows["a_parent"]["median_ms"], 4)
    report["b_over_c"] = round(rows["b_this"]["median_ms"] / rows["c_this_dense"]["median_ms"], 4)
    if "d_all_rounds" in rows:
        report["b_over_d"] = round(rows["b_this"]["median_ms"] / rows["d_all_rounds"]["median_ms"], 4)
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc["stage"] = report
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(report, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--cases", default="plain")
    ap.add_argument("--parent-lib")
    ap.add_argument("--variant-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_transform_mi355x.json"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=150)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib:
        raise SystemExit("--parent-lib is needed (see the module's text)")
    driver(args)


if __name__ == "__main__":
    main()
