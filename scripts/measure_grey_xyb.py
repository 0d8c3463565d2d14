#!/usr/bin/env python3
"""The filter-stage launch of a grey XYB image asked for as GRAY8, against the RGB8 headline and against the route the
same request would take without the one-channel kernel form.

A 3840 x 2160 d1.0 body (Gaborish + EPF1: bench.py's seed-177 frame) as a set of 64 resident frames; the filter + colour
stage of the set alone, from the HIP events around it (jxlhip_last_stage_ms(2)), entropy and transforms run once before.

  (a) rgb8 / parent    the untagged body to RGB8 with the library of the parent commit (--parent-lib)
  (b) rgb8 / this      the same with this tree's library
  (c) gray8 / this     the grey-tagged body to GRAY8: k_filter_rows2<true, 1, true, true>
  (d) gray8 / variant  the same with a library built with -DJXLHIP_NO_GRAY8_ROWS (--build-variant makes it):
                       k_filter_rows2<false> to the filtered planes, then k_color_out

Every number is the median of --reps launches in one process; the driver starts one process per library and round,
alternating the libraries, each under its own `timeout -k 10` and only while the one before succeeded, and writes the
per-process medians and their spread to --out.

  python scripts/measure_grey_xyb.py --build-variant libjxl_amd/_build/variant        (no GPU needed)
  python scripts/measure_grey_xyb.py --parent-lib PARENT/libjxl_amd.so --variant-lib libjxl_amd/_build/variant/libjxl_amd.so \\
         --out profiles/grey_xyb_mi355x.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_variant(out_dir):
    src = os.path.join(ROOT, "libjxl_amd")
    os.makedirs(out_dir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj = os.path.join(out_dir, "jxl_hip_api.o")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-fPIC", "-DJXLHIP_NO_GRAY8_ROWS",
                           "-I" + os.path.join(ROOT, "include"), "-c", "-o", obj, os.path.join(src, "csrc/hip/jxl_hip_api.hip")])
    api = os.path.join(src, "_build", "jxl_api.o")
    if not os.path.exists(api):
        raise SystemExit("build the library first (libjxl_amd.build()): %s is missing" % api)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", os.path.join(out_dir, "libjxl_amd.so"), obj, api, "-lpthread"])
    print(os.path.join(out_dir, "libjxl_amd.so"))


def child(args):
    import libjxl_amd as J
    J.LIB_PATH = os.path.abspath(args.lib)
    import numpy as np
    img = J.synth_image(3840, 2160, 177)
    out = {}
    for case in args.cases.split(","):
        grey = case == "gray8"
        if grey:
            J.set_xyb_color_encoding(white_point=1, transfer_function=13, gray=True)
        try:
            data = J.encode_rgb8(img, distance=1.0, strategy_mode=1)
        finally:
            J.set_xyb_color_encoding(None)
        frame = J.Frame(data, threads=8)
        assert (frame.info["gab"], frame.info["epf_iters"]) == (1, 1), frame.info
        ctxs = [J.HipContext(0) for _ in range(args.frames)]
        for c in ctxs:
            c.set_output_format(2, 1 if grey else 3)
            c.upload(frame)
        J.run_entropy_batch(ctxs)
        J.run_transform_batch(ctxs)
        ms = []
        for i in range(args.warmup + args.reps):
            J.run_filter_color_batch(ctxs)
            ctxs[0].sync()
            if i >= args.warmup:
                ms.append(ctxs[0].stage_ms(2))
        px = ctxs[-1].pixels()
        out[case] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "frames": args.frames,
                     "mean_sample": float(np.mean(px)), "bytes_per_pixel": int(px.shape[2])}
        for c in ctxs:
            c.close()
        frame.close()
    print("RESULT " + json.dumps(out))


def driver(args):
    libs = [("parent", args.parent_lib, "rgb8"), ("this", os.path.join(ROOT, "libjxl_amd", "_build", "libjxl_amd.so"), "rgb8,gray8"),
            ("variant", args.variant_lib, "gray8")]
    runs = {"a_rgb8_parent": [], "b_rgb8_this": [], "c_gray8_kernel": [], "d_gray8_generic": []}
    keys = {("parent", "rgb8"): "a_rgb8_parent", ("this", "rgb8"): "b_rgb8_this", ("this", "gray8"): "c_gray8_kernel",
            ("variant", "gray8"): "d_gray8_generic"}
    means = {}
    for rnd in range(args.rounds):
        for name, lib, cases in (libs if rnd % 2 == 0 else libs[::-1]):
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--lib", lib, "--cases", cases,
                   "--frames", str(args.frames), "--reps", str(args.reps), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout[-2000:])
            if r.returncode != 0:  # nothing more is started on the device after a step that failed
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit("step %s (round %d) ended with status %d" % (name, rnd, r.returncode))
            res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            for case, v in res.items():
                runs[keys[(name, case)]].append(v["median_ms"])
                means.setdefault(keys[(name, case)], []).append(v["mean_sample"])
    report = {"what": "filter(+colour) stage of 64 resident 3840x2160 d1.0 frames (Gaborish + EPF1), ms per launch of the set; "
                      "median of %d launches per process, %d processes per row, libraries alternating" % (args.reps, args.rounds),
              "frames": args.frames, "rows": {}}
    for k, v in runs.items():
        report["rows"][k] = {"process_medians_ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4),
                             "spread_ms": round(max(v) - min(v), 4), "ms_per_frame": round(statistics.median(v) / args.frames, 5),
                             "mean_sample": round(statistics.median(means[k]), 4)}
    rows = report["rows"]
    report["c_over_a"] = round(rows["c_gray8_kernel"]["median_ms"] / rows["a_rgb8_parent"]["median_ms"], 4)
    report["c_over_d"] = round(rows["c_gray8_kernel"]["median_ms"] / rows["d_gray8_generic"]["median_ms"], 4)
    report["b_over_a"] = round(rows["b_rgb8_this"]["median_ms"] / rows["a_rgb8_parent"]["median_ms"], 4)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-variant", metavar="DIR")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--cases", default="rgb8")
    ap.add_argument("--parent-lib")
    ap.add_argument("--variant-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grey_xyb_mi355x.json"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=150)
    args = ap.parse_args()
    if args.build_variant:
        return build_variant(args.build_variant)
    if args.child:
        return child(args)
    if not args.parent_lib or not args.variant_lib:
        raise SystemExit("--parent-lib and --variant-lib are needed (see the module's text)")
    driver(args)


if __name__ == "__main__":
    main()
