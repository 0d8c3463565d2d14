#!/usr/bin/env python3
"""One 3840 x 2160 d1.0 frame (bench.py's seed 177, cfl_fit=1), RGB8 -> codestream, with the AC tokens coded by the host
(device_tokens=True) and on the device (device_entropy=True): DESIGN.md section 7, f3.

Per encode: wall time of encode_rgb8_gpu, forward_s (the hook calls: pixel-domain kernels, tokenisation and, on the device
route, histograms + code construction + rANS kernels and their copies), assemble_s (what is left for the host: on the
token route tokens -> histograms -> clustering -> rANS -> headers, on the device route headers and DC only) and
entropy_kernels_ms (HIP events around the histogram, records + chain and scatter kernels).

  parent   the libraries of the parent commit (--parent-build DIR with libjxl_amd.so and libjxlenc.so), device_tokens=True
  alone    this tree's libraries, device_tokens=True only: the untouched route, to be held against the parent's spread
  this     this tree's libraries, the two routes alternating encode by encode in one process

Every row is the median of --reps encodes per process over --rounds processes; a fresh process per leg, parent and this
alternating, each under its own `timeout -k 10` and only while the one before succeeded. Writes --out.

  python scripts/measure_device_entropy.py --parent-build PARENT/libjxl_amd/_build --out profiles/device_entropy_mi355x.json
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("wall_s", "forward_s", "assemble_s", "entropy_kernels_ms")


def child(args):
    import libjxl_amd as J
    if args.build:
        J.LIB_PATH = os.path.abspath(os.path.join(args.build, "libjxl_amd.so"))
        J.ENC_PATH = os.path.abspath(os.path.join(args.build, "libjxlenc.so"))
    img = J.synth_image(3840, 2160, seed=177)
    ctx = J.HipContext(0)
    routes = args.routes.split(",")
    rows = {r: {k: [] for k in KEYS} for r in routes}
    digest = {}
    for i in range(args.warmup + args.reps):
        for r in routes:
            t = {}
            t0 = time.perf_counter()
            data = J.encode_rgb8_gpu(img, ctx, timings=t, distance=1.0, cfl_fit=1, **{r: True})
            wall = time.perf_counter() - t0
            digest[r] = hashlib.sha256(data).hexdigest()
            if i >= args.warmup:
                rows[r]["wall_s"].append(wall)
                rows[r]["forward_s"].append(t["forward_s"])
                rows[r]["assemble_s"].append(t["assemble_s"])
                rows[r]["entropy_kernels_ms"].append(t.get("entropy_kernels_ms", 0.0))
    out = {r: dict({k: statistics.median(v) for k, v in rows[r].items()}, sha256=digest[r], bytes=len(data),
                   tokens=t["device_tokens"]) for r in routes}
    if "device_entropy" in routes:
        out["device_entropy"]["histogram_ms"], out["device_entropy"]["ans_ms"] = ctx.enc_entropy_ms()
    ctx.close()
    print("RESULT " + json.dumps(out))


def driver(args):
    legs = [("parent", args.parent_build, "device_tokens"), ("alone", None, "device_tokens"), ("this", None, "device_tokens,device_entropy")]
    runs = {}
    for rnd in range(args.rounds):
        for name, build, routes in legs[rnd % 3:] + legs[:rnd % 3]:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--routes", routes,
                   "--reps", str(args.reps), "--warmup", str(args.warmup)] + (["--build", build] if build else [])
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout[-2000:])
            sys.stdout.flush()
            if r.returncode != 0:  # nothing more is started on the device after a step that failed
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit("step %s (round %d) ended with status %d" % (name, rnd, r.returncode))
            res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            for route, v in res.items():
                runs.setdefault("%s %s" % (name, route), []).append(v)
    report = {"what": "one 3840x2160 d1.0 frame (seed 177, cfl_fit=1), RGB8 -> codestream; median of %d encodes per process, %d "
                      "processes per row, parent and this build alternating, the two routes of this build alternating encode by "
                      "encode" % (args.reps, args.rounds), "rows": {}}
    for k, v in sorted(runs.items()):
        row = {"sha256": sorted(set(x["sha256"] for x in v)), "bytes": v[0]["bytes"], "tokens": v[0]["tokens"]}
        for key in KEYS + ("histogram_ms", "ans_ms"):
            if key in v[0]:
                vals = [x[key] for x in v]
                row[key] = {"process_medians": [round(x, 5) for x in vals], "median": round(statistics.median(vals), 5),
                            "spread": round(max(vals) - min(vals), 5)}
        report["rows"][k] = row
    rows = report["rows"]
    report["same_stream_in_every_row"] = len(set(s for r in rows.values() for s in r["sha256"])) == 1
    p, a, b = rows["parent device_tokens"]["wall_s"], rows["this device_tokens"]["wall_s"], rows["this device_entropy"]["wall_s"]
    alone = rows["alone device_tokens"]["wall_s"]
    report["untouched_route_inside_parent_spread"] = min(p["process_medians"]) <= alone["median"] <= max(p["process_medians"])
    report["device_entropy_over_device_tokens_wall"] = round(b["median"] / a["median"], 4)
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc["encode"] = report
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(report, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--build")
    ap.add_argument("--routes", default="device_tokens")
    ap.add_argument("--parent-build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_entropy_mi355x.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=150)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_build:
        raise SystemExit("--parent-build is needed (see the module's text)")
    driver(args)


if __name__ == "__main__":
    main()
