#!/usr/bin/env python3
"""The forward path with the reference's AC-strategy search on the device (strategy_mode 2 / 3 of jxlhip_enc_forward, DESIGN.md
section 7): what the search costs on a 4K frame beside the mode it replaces, and what it chooses.

Workload: bench.py's seed-177 3840 x 2160 frame, adaptive_quant=1, acs_search 0 (the activity rule, strategy_mode 1), 1 (the
aligned walk, strategy_mode 2) and 2 (with the floating passes, strategy_mode 3).

  time     per mode, in each of --rounds fresh child processes (each under its own time limit, started only while the one
           before succeeded): one encode, then --reps replays of its kernel sequence on the resident input
           (jxlhip_enc_forward_rerun); the medians of jxlhip_enc_last_ms and of the three figures of
           jxlhip_enc_search_last_ms (mask1x1, all estimate launches, the walk).
  quality  (first round only) at d1.0 and d4.0: stream bytes, PSNR of the oracle's decode against the image, and the
           histogram of the chosen kinds. No claim is attached to them.
  --one-call MODE  one encode in that mode and nothing else, for a kernel-trace run:
           rocprofv3 --kernel-trace --stats -- python this --one-call 2

  python scripts/measure_acs_search.py --out profiles/acs_search_mi355x.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

XS, YS = 3840, 2160


def child(args):
    import numpy as np
    import libjxl_amd as J
    img = J.synth_image(XS, YS, seed=177)
    ctx = J.HipContext(0)
    if args.one_call is not None:
        J.encode_rgb8_gpu(img, ctx, device_entropy=True, adaptive_quant=1, acs_search=args.one_call)
        ctx.close()
        return
    out = {"modes": {}, "quality": {}}
    for mode in (0, 1, 2):
        J.encode_rgb8_gpu(img, ctx, device_entropy=True, adaptive_quant=1, acs_search=mode)
        total, search = [], []
        for i in range(args.warmup + args.reps):
            ms = ctx.enc_rerun(1)[0]
            if i >= args.warmup:
                total.append(ms)
                if mode:
                    search.append(ctx.enc_search_ms())
        row = {"enc_last_ms": statistics.median(total)}
        if mode:
            row.update(mask1x1_ms=statistics.median(s[0] for s in search), estimates_ms=statistics.median(s[1] for s in search),
                       walk_ms=statistics.median(s[2] for s in search), candidates=int(len(J.acs_walk_candidates((XS + 7) // 8, (YS + 7) // 8, mode - 1)[0])))
        out["modes"][str(mode)] = row
    if args.quality:
        import jxlo
        for distance in (1.0, 4.0):
            for mode in (0, 1, 2):
                data = J.encode_rgb8_gpu(img, ctx, device_entropy=True, adaptive_quant=1, acs_search=mode, distance=distance)
                o = jxlo.Decoded(data, dumps=False)
                mse = float(np.mean((o.rgb8.astype(np.float64) - img) ** 2))
                o.close()
                acs = J.enc_forward_model(img, ctx, adaptive_quant=1, acs_search=mode, distance=distance)["acs"]
                kinds, counts = np.unique(acs[(acs & 1) == 1] >> 1, return_counts=True)
                out["quality"]["d%.1f mode %d" % (distance, mode)] = {"bytes": len(data), "psnr_db": round(10 * np.log10(255.0 ** 2 / mse), 3),
                                                                     "kinds": dict(zip((int(k) for k in kinds), (int(c) for c in counts)))}
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--one-call", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acs_search_mi355x.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=280)
    args = ap.parse_args()
    if args.child or args.one_call is not None:
        return child(args)
    rows = []
    for rnd in range(args.rounds):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps),
               "--warmup", str(args.warmup)] + (["--quality"] if rnd == 0 else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout[-3000:])
        sys.stdout.flush()
        if r.returncode != 0:  # nothing more is started on the device after a step that failed
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("child %d ended with status %d" % (rnd, r.returncode))
        rows.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
    rep = {"what": "%dx%d seed 177 d1.0, adaptive_quant=1; per process the median of %d replays of one encode's kernel sequence, %d fresh "
                   "processes; mode 0 = the activity rule (strategy_mode 1), 1 = the aligned walk (2), 2 = with the floating passes (3)" % (
                       XS, YS, args.reps, args.rounds), "modes": {}, "quality": rows[0]["quality"]}
    for mode in ("0", "1", "2"):
        rep["modes"][mode] = {}
        for key in rows[0]["modes"][mode]:
            vals = [r["modes"][mode][key] for r in rows]
            rep["modes"][mode][key] = vals[0] if key == "candidates" else {"process_medians": [round(v, 4) for v in vals], "median": round(statistics.median(vals), 4)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rep, f, indent=1)
        f.write("\n")
    print(json.dumps(rep, indent=1))


if __name__ == "__main__":
    main()
