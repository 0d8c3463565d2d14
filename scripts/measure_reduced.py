"""The reduced decode (torch_io's reduce=8: the image at 1/8 scale from the frame's DC image) against the only other route
to the same tensor: the full decode with the resized binding. bench.py's seed-177 3840x2160 d1.0 stream, to a normalised
float16 (3, 224, 224) tensor, one frame and a batch of 64.

The two routes run alternately, in one process, on contexts that are already uploaded: the timed window is the device
stages, from a host clock around work that ends in torch.cuda.synchronize(). The host parse (Frame(..., reduced=True)
against Frame(...)) and the upload are timed apart, the same way. Medians, the 10th and 90th percentile, need / len(data)
and the largest difference between the two tensors (they differ by construction: the full route filters, then averages)
are printed and written as JSON.

    python scripts/measure_reduced.py --out profiles/reduced_mi355x.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/measure_reduced.py --only reduced --cases batch64 --reps 5
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/measure_reduced.py --only dc_kernels --reps 5
(the launch's own time, and k_dc_dequant + k_dc_smooth + k_color_out at 480 x 270: see dc_kernels)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import libjxl_amd as J  # noqa: E402
from libjxl_amd import torch_io  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SIZE = (224, 224)


def stats(t):
    return None if not t else {"median_ms": float(np.median(t)), "p10_ms": float(np.percentile(t, 10)), "p90_ms": float(np.percentile(t, 90))}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


class Set:
    """n copies of one stream, uploaded twice: for the reduced route and for the full route with the resized binding."""

    def __init__(self, data, n, only):
        self.n = n
        self.need = J.frame_dc_extent(data)
        self.out_r = torch.zeros((n, 3) + SIZE, dtype=torch.float16, device="cuda")
        self.out_f = torch.zeros((n, 3) + SIZE, dtype=torch.float16, device="cuda")
        self.reduced, self.full, self.frames = [], [], []
        for i in range(n):
            if only != "full":
                f = J.Frame(data[:self.need], reduced=True)
                c = J.HipContext()
                torch_io.bind_resized(c, self.out_r[i], "CHW", None, MEAN, STD)
                c.upload_reduced(f)
                self.frames.append(f)
                self.reduced.append(c)
            if only != "reduced":
                f = J.Frame(data)
                c = J.HipContext()
                torch_io.bind_resized(c, self.out_f[i], "CHW", None, MEAN, STD)
                c.upload(f)
                self.frames.append(f)
                self.full.append(c)

    def run_reduced(self):
        J.run_reduced_batch(self.reduced)
        return self.out_r

    def run_full(self):
        J.run_entropy_batch(self.full)
        J.run_transform_batch(self.full)
        J.run_filter_color_batch(self.full)
        return self.out_f

    def close(self):
        for c in self.reduced + self.full:
            c.close()
        for f in self.frames:
            f.close()


def host_times(data, reps):
    """Parse and upload of one frame on the host, both routes alternating (the upload ends in a device copy it waits for)."""
    need = J.frame_dc_extent(data)
    prefix = data[:need]
    t = {"parse_reduced": [], "parse_full": [], "upload_reduced": [], "upload_full": []}
    out = torch.zeros((3,) + SIZE, dtype=torch.float16, device="cuda")
    a, b = J.HipContext(), J.HipContext()
    torch_io.bind_resized(a, out, "CHW", None, MEAN, STD)
    torch_io.bind_resized(b, out, "CHW", None, MEAN, STD)
    for i in range(reps + 2):
        t0 = time.perf_counter()
        fr = J.Frame(prefix, reduced=True)
        t1 = time.perf_counter()
        ff = J.Frame(data)
        t2 = time.perf_counter()
        a.upload_reduced(fr)
        t3 = time.perf_counter()
        b.upload(ff)
        t4 = time.perf_counter()
        if i >= 2:
            for k, v in zip(("parse_reduced", "parse_full", "upload_reduced", "upload_full"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                t[k].append(v * 1e3)
        fr.close()
        ff.close()
    a.close()
    b.close()
    return {k: stats(v) for k, v in t.items()}


def dc_kernels(reps):
    """For the kernel trace, the three kernels the reduced launch fuses, at the size of a 4K frame's DC image: uploads of
    the 3840 x 2160 stream launch k_dc_dequant and k_dc_smooth over 480 x 270 blocks (grid 8 x 68 workgroups); the whole
    route on a 480 x 270 pixel image with the generic f32 writer ends in k_color_out at that size (its own k_dc_* launches,
    over 60 x 34 blocks, are told apart by their grids)."""
    big = J.encode_rgb8(J.synth_image(3840, 2160, 177), distance=1.0, strategy_mode=1, max_clusters=0, ac_code_mode=0)
    f = J.Frame(big)
    c = J.HipContext()
    for _ in range(reps):
        c.upload(f)
        c.sync()
    c.close()
    f.close()
    data = J.encode_rgb8(J.synth_image(480, 270, 177), distance=1.0)
    f = J.Frame(data)
    c = J.HipContext()
    c.set_output_format(0, 3)
    c.set_output_orientation(2)  # (a mirrored f32 image: no filter kernel writes it, k_color_out does)
    for _ in range(reps):
        c.upload(f)
        c.run_all()
        c.sync()
    print("pixel route of the 480x270 frame: %d (0 = k_color_out)" % c.pixel_route())
    c.close()
    f.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["reduced", "full", "dc_kernels"], default=None)
    ap.add_argument("--cases", default="one,batch64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here is measured on a CPU")
    if a.only == "dc_kernels":
        dc_kernels(a.reps)
        return
    data = J.encode_rgb8(J.synth_image(3840, 2160, 177), distance=1.0, strategy_mode=1, max_clusters=0, ac_code_mode=0)  # bench.py make_stream
    results = {"stream_bytes": len(data), "dc_extent_bytes": J.frame_dc_extent(data)}
    results["dc_extent_share"] = results["dc_extent_bytes"] / len(data)
    if a.only is None:
        results["host"] = host_times(data, a.reps)
        print("host", json.dumps(results["host"]), flush=True)
    for case in a.cases.split(","):
        n = {"one": 1, "batch64": 64}[case]
        s = Set(data, n, a.only)
        for _ in range(a.warmup):
            if a.only != "full":
                s.run_reduced()
            if a.only != "reduced":
                s.run_full()
        torch.cuda.synchronize()
        t_r, t_f = [], []
        for _ in range(a.reps):  # alternating, so that what else the machine does meets both alike
            if a.only != "full":
                ms, r = timed(s.run_reduced)
                t_r.append(ms)
            if a.only != "reduced":
                ms, f = timed(s.run_full)
                t_f.append(ms)
        diff = None if a.only else float((r.float() - f.float()).abs().max())
        mean_diff = None if a.only else float((r.float() - f.float()).abs().mean())
        results[case] = {"frames": n, "reduced": stats(t_r), "full_resized": stats(t_f), "max_abs_difference_normalised_f16": diff,
                         "mean_abs_difference_normalised_f16": mean_diff}
        print(case, json.dumps(results[case]), flush=True)
        s.close()
    print("need / len(data) = %d / %d = %.4f" % (results["dc_extent_bytes"], results["stream_bytes"], results["dc_extent_share"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
