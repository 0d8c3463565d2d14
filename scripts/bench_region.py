"""Region decode (torch_io region=True: Frame.plan_window + HipContext.upload_window) against the whole-frame route of the
same tree (region=False), which is the route crops took before: a crop of a VarDCT frame resized to 224 x 224 float16.

Per case both forms run alternately in one process. Timed separately, each from a host clock around work that ends in
torch.cuda.synchronize() (as scripts/bench_resample.py): the decode stages of frames that are already uploaded, and the
upload (the window's includes its plan and k_dc_window). The host parse, which both forms share, is timed on its own.
Medians, the 10th and 90th percentile, the groups uploaded and whether the two tensors are equal bit for bit are printed
and written as JSON.

    python scripts/bench_region.py --out profiles/region_mi355x.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_region.py --only region --reps 5   (k_dc_window's own time)
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


class Set:
    """Frames of one case with a context each for the two forms, both bound to a (n, 3, 224, 224) float16 tensor of its own."""

    def __init__(self, datas, boxes):
        n = len(datas)
        self.boxes = boxes
        t0 = time.perf_counter()
        self.frames = [J.Frame(d) for d in datas]
        self.parse_ms = (time.perf_counter() - t0) * 1e3 / n
        self.out = {k: torch.empty((n, 3) + SIZE, dtype=torch.float16, device="cuda") for k in ("region", "whole")}
        self.ctxs = {k: [J.HipContext() for _ in range(n)] for k in ("region", "whole")}
        self.plans = [f.plan_window(b) for f, b in zip(self.frames, boxes)]
        self.upload("region")
        self.upload("whole")

    def upload(self, which):
        for i, (f, c) in enumerate(zip(self.frames, self.ctxs[which])):
            if which == "region":
                w = f.plan_window(self.boxes[i])
                torch_io.bind_resized(c, self.out[which][i], "CHW", w["box"], MEAN, STD)
                c.upload_window(f, w)
            else:
                torch_io.bind_resized(c, self.out[which][i], "CHW", self.boxes[i], MEAN, STD)
                c.upload(f)

    def stages(self, which):
        ctxs = self.ctxs[which]
        J.run_entropy_batch(ctxs)
        J.run_transform_batch(ctxs)
        J.run_filter_color_batch(ctxs)
        return self.out[which]

    def close(self):
        for k in self.ctxs:
            for c in self.ctxs[k]:
                c.close()
        for f in self.frames:
            f.close()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(t):
    return None if not t else {"median_ms": float(np.median(t)), "p10_ms": float(np.percentile(t, 10)), "p90_ms": float(np.percentile(t, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["region", "whole"], default=None)
    ap.add_argument("--cases", default="4k_crop224,4k_box1200,batch64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here is measured on a CPU")
    forms = [f for f in ("region", "whole") if a.only in (None, f)]
    results = {}
    big = None
    for case in a.cases.split(","):
        if case in ("4k_crop224", "4k_box1200"):
            big = big or J.encode_rgb8(J.synth_image(3840, 2160, seed=177), distance=1.0)  # (bench.py's stream)
            s = Set([big], [(1808, 968, 224, 224) if case == "4k_crop224" else (1320, 630, 1200, 900)])
        elif case == "batch64":
            four = [J.encode_rgb8(J.synth_image(512, 384, seed=10 + i), distance=1.0) for i in range(4)]
            rng = np.random.default_rng(3)
            s = Set([four[i % 4] for i in range(64)], [(int(rng.integers(0, 512 - 224 + 1)), int(rng.integers(0, 384 - 224 + 1)), 224, 224) for _ in range(64)])
        else:
            raise SystemExit("unknown case " + case)
        for _ in range(a.warmup):
            for f in forms:
                s.stages(f)
        torch.cuda.synchronize()
        t_stage = {f: [] for f in forms}
        t_upload = {f: [] for f in forms}
        outs = {}
        for _ in range(a.reps):  # alternating, so that what else the machine does meets both alike
            for f in forms:
                ms, outs[f] = timed(lambda: s.stages(f))
                t_stage[f].append(ms)
        for _ in range(max(3, a.reps // 4)):
            for f in forms:
                ms, _ = timed(lambda: s.upload(f))
                t_upload[f].append(ms)
        for f in forms:  # (the uploads above left the contexts without a decoded frame: decode once more for the comparison)
            outs[f] = s.stages(f)
        torch.cuda.synchronize()
        same = None if len(forms) < 2 else bool(torch.equal(outs["region"].view(torch.int16), outs["whole"].view(torch.int16)))
        results[case] = {"frames": len(s.frames), "image": [s.frames[0].info["xsize"], s.frames[0].info["ysize"]], "box": list(s.boxes[0]),
                         "groups_uploaded": sum(p["groups_taken"] for p in s.plans), "groups_in_frames": sum(p["groups_in_frame"] for p in s.plans),
                         "reasons": sorted({J.WINDOW_REASONS[p["reason"]] for p in s.plans}),
                         "host_parse_ms_per_frame": s.parse_ms,
                         "stages": {f: stats(t_stage[f]) for f in forms}, "upload": {f: stats(t_upload[f]) for f in forms},
                         "tensors_equal": same}
        print(case, json.dumps(results[case]), flush=True)
        s.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
