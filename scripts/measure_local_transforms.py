#!/usr/bin/env python3
"""Measurement aid for group-local transforms on Modular frames.

  measure_local_transforms.py [--other-root DIR] [--reps N] [--batch 48] [--out FILE]

Streams (3840x2160, written once by this tree's stream writer into a temporary directory):
  rct        an RCT in every one of the 135 group headers, nothing else
  pal_rct    flat groups (a third of them, at most 64 colours) with an all-channel palette, an RCT in the others
  rct_same   the pal_rct IMAGE coded with an RCT in every group and no palette (the palette's cost beside it)
Each measurement is a fresh child process that decodes one stream with one build of the library: this tree's
(libjxl_amd/_build) or, with --other-root, another checkout's (e.g. the parent commit, to compare schedules; it cannot
decode pal_rct if it predates group palettes, which is reported as such). The children alternate between the builds,
`--reps` rounds, so that drift of the machine shows as spread inside each build's figures and not as a difference between
them. A child reports stage_ms(0) (the timed span of run_modular: streams + inverse transforms + output) of one frame and
of a set of --batch frames, 3 warm-up runs and 10 timed runs each. Kernel times come from a profiler run of its own:
`--write-streams DIR` only writes the three streams, and `--child --stream DIR/pal_rct.jxl [--root DIR]` is the program
to put behind `rocprofv3 --kernel-trace --stats --`. Prints a table and one JSON object; --out writes the JSON to a file.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(args):
    sys.path.insert(0, args.root)
    import libjxl_amd as J
    data = open(args.stream, "rb").read()
    out = {}
    try:
        frame = J.ModFrame(data)
    except J.JxlAmdError as e:
        print(json.dumps({"refused": str(e)}))
        return 0
    out["launch_levels"] = frame.info.get("launch_levels")
    out["num_ops"] = frame.info["num_ops"]
    for n in (1, args.batch):
        ctxs = [J.HipContext() for _ in range(n)]
        for c in ctxs:
            c.upload_modular(frame)
        times = []
        for i in range(3 + 10):
            J.run_modular_batch(ctxs)
            ctxs[0].sync()
            if i >= 3:
                times.append(ctxs[0].stage_ms(0))
        r, status, _ = ctxs[0].modular_status()
        assert r == 0 and not any(status)
        out["ms_%d" % n] = times
        for c in ctxs:
            c.close()
    frame.close()
    print(json.dumps(out))
    return 0


def write_streams(tmp):
    sys.path.insert(0, ROOT)
    import numpy as np
    import libjxl_amd as J
    rng = np.random.default_rng(12)
    img = J.synth_image(3840, 2160, seed=41)
    flat = img.copy()
    table = rng.integers(0, 256, (48, 3), dtype=np.uint8)
    for gy in range(9):
        for gx in range(15):
            if (gx + 2 * gy) % 3 == 0:
                a = flat[gy * 256:(gy + 1) * 256, gx * 256:(gx + 1) * 256]
                a[...] = table[rng.integers(0, 48, a.shape[:2]) % (4 + 4 * ((gx + gy) % 12))]
    streams = {"rct": J.encode_lossless(img, J.LOSSLESS_LOCAL_RCT),
               "pal_rct": J.encode_lossless(flat, J.LOSSLESS_LOCAL_PALETTE | J.LOSSLESS_LOCAL_RCT, palette_colors=64),
               "rct_same": J.encode_lossless(flat, J.LOSSLESS_LOCAL_RCT)}
    paths = {}
    for name, d in streams.items():
        paths[name] = os.path.join(tmp, name + ".jxl")
        open(paths[name], "wb").write(d)
    return paths


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--other-root", default=None, help="another checkout with built libraries, measured alternately with this one")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=48)
    ap.add_argument("--out", default=None)
    ap.add_argument("--write-streams", metavar="DIR", default=None, help="write the three streams into DIR and stop")
    ap.add_argument("--child", action="store_true", help="decode --stream with the build under --root; prints one JSON line")
    ap.add_argument("--root", default=ROOT, help="--child: the checkout whose libjxl_amd is loaded")
    ap.add_argument("--stream", default=None, help="--child: the stream file")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.write_streams:
        os.makedirs(args.write_streams, exist_ok=True)
        write_streams(args.write_streams)
        return 0
    builds = [("this", ROOT)]
    if args.other_root:
        builds.append(("other", os.path.abspath(args.other_root)))
    results = {}
    with tempfile.TemporaryDirectory() as tmp:
        paths = write_streams(tmp)
        for rep in range(args.reps):
            for stream in ("rct", "pal_rct", "rct_same"):
                for name, root in builds:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--stream", paths[stream],
                                        "--batch", str(args.batch)], capture_output=True, text=True, timeout=600)
                    if r.returncode:  # a child that failed ends the measurement: nothing more is started on the device
                        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
                        return 1
                    results.setdefault((stream, name), []).append(json.loads(r.stdout.strip().splitlines()[-1]))
                    sys.stderr.write("round %d %s/%s done\n" % (rep, stream, name))
                    sys.stderr.flush()
    summary = {}
    for (stream, name), reps in sorted(results.items()):
        row = {"launch_levels": reps[0].get("launch_levels"), "num_ops": reps[0].get("num_ops")}
        if "refused" in reps[0]:
            row["refused"] = reps[0]["refused"]
        else:
            for key in ("ms_1", "ms_%d" % args.batch):
                per_rep = [statistics.median(r[key]) for r in reps]  # one figure per child process
                row[key] = {"median_of_reps": round(statistics.median(per_rep), 3), "reps": [round(v, 3) for v in per_rep],
                            "min_run": round(min(min(r[key]) for r in reps), 3), "max_run": round(max(max(r[key]) for r in reps), 3)}
        summary["%s/%s" % (stream, name)] = row
        print("%-22s %s" % ("%s/%s" % (stream, name), json.dumps(row)))
    blob = json.dumps({"what": "stage_ms(0) of run_modular, 3840x2160, one frame and a set of %d; medians of 10 runs per child process, "
                               "%d alternating child processes per build" % (args.batch, args.reps), "results": summary})
    print(blob)
    if args.out:
        open(args.out, "w").write(blob + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
