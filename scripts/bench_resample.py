"""Crop + resize on the device (torch_io.bind_resized) against what a user composes from torch calls without it: decode into
a full-size float32 tensor (torch_io.bind), then crop -> interpolate(antialias=True) -> normalise -> .to(float16).

Per case both forms run alternately on frames that are already uploaded: the timed window is the decode stages plus, for the
composition, the torch calls, from a host clock around work that ends in torch.cuda.synchronize() (the stages run on the
contexts' own streams, the torch calls on torch's: one device event pair cannot bracket both). Medians, the 10th and 90th
percentile, and the largest difference between the two results are printed and written as JSON.

    python scripts/bench_resample.py --out profiles/resample_mi355x.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_resample.py --only new --reps 5   (the passes' own times)
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
    """Frames of one case, uploaded twice: bound for the resized output and bound for the full-size float32 output."""

    def __init__(self, datas, boxes, modular):
        self.modular, self.boxes, n = modular, boxes, len(datas)
        self.frames = [J.ModFrame(d) if modular else J.Frame(d) for d in datas]
        info = self.frames[0].info
        self.w, self.h = (info["xsize"], info["ysize"]) if modular else (info["out_xsize"], info["out_ysize"])
        self.small = torch.empty((n, 3) + SIZE, dtype=torch.float16, device="cuda")
        self.full = torch.empty((n, 3, self.h, self.w), dtype=torch.float32, device="cuda")
        self.mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
        self.std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
        self.new, self.old = [], []
        for i, f in enumerate(self.frames):
            a, b = J.HipContext(), J.HipContext()
            torch_io.bind_resized(a, self.small[i], "CHW", boxes[i], MEAN, STD)
            torch_io.bind(b, self.full[i], "CHW")
            for c in (a, b):
                c.upload_modular(f) if modular else c.upload(f)
            self.new.append(a)
            self.old.append(b)

    def _stages(self, ctxs):
        if self.modular:
            J.run_modular_batch(ctxs)
        else:
            J.run_entropy_batch(ctxs)
            J.run_transform_batch(ctxs)
            J.run_filter_color_batch(ctxs)

    def run_new(self):
        self._stages(self.new)
        return self.small

    def run_old(self):
        self._stages(self.old)
        box = self.boxes[0]  # (one box per case)
        src = self.full if box is None else self.full[:, :, box[1]:box[1] + box[3], box[0]:box[0] + box[2]]
        r = torch.nn.functional.interpolate(src, size=SIZE, mode="bilinear", antialias=True, align_corners=False)
        return ((r - self.mean) / self.std).to(torch.float16)

    def bytes_needed(self):
        """What the two passes must move per frame: the box read, the intermediate written and read, the tensor written."""
        box = self.boxes[0] or (0, 0, self.w, self.h)
        return box[2] * box[3] * 3 * 4 + 2 * SIZE[0] * box[2] * 3 * 4 + SIZE[0] * SIZE[1] * 3 * 2

    def close(self):
        for c in self.new + self.old:
            c.close()
        for f in self.frames:
            f.close()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["new", "old"], default=None)
    ap.add_argument("--cases", default="4k_whole,4k_box,batch64,lossless1k")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here is measured on a CPU")
    results = {}
    big = None
    for case in a.cases.split(","):
        if case in ("4k_whole", "4k_box"):
            big = big or J.encode_rgb8(J.synth_image(3840, 2160, seed=1), distance=1.0)
            s = Set([big], [None if case == "4k_whole" else (1320, 630, 1200, 900)], False)
        elif case == "batch64":
            four = [J.encode_rgb8(J.synth_image(512, 384, seed=10 + i), distance=1.0) for i in range(4)]
            s = Set([four[i % 4] for i in range(64)], [None] * 64, False)
        elif case == "lossless1k":
            s = Set([J.encode_lossless(J.synth_image(1024, 1024, seed=2))], [None], True)
        else:
            raise SystemExit("unknown case " + case)
        for _ in range(a.warmup):
            if a.only != "old":
                s.run_new()
            if a.only != "new":
                s.run_old()
        torch.cuda.synchronize()
        t_new, t_old, diff = [], [], None
        for _ in range(a.reps):  # alternating, so that what else the machine does meets both alike
            if a.only != "old":
                ms, new = timed(s.run_new)
                t_new.append(ms)
            if a.only != "new":
                ms, old = timed(s.run_old)
                t_old.append(ms)
        if a.only is None:
            diff = float((new.float() - old.float()).abs().max())

        def stats(t):
            return None if not t else {"median_ms": float(np.median(t)), "p10_ms": float(np.percentile(t, 10)), "p90_ms": float(np.percentile(t, 90))}
        results[case] = {"frames": len(s.frames), "image": [s.w, s.h], "box": s.boxes[0], "new": stats(t_new), "composition": stats(t_old),
                         "max_abs_difference_f16": diff, "pass_bytes_per_frame": s.bytes_needed()}
        print(case, json.dumps(results[case]), flush=True)
        s.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
