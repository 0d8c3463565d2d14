#!/usr/bin/env python3
"""What a normalised float16 / bfloat16 CHW tensor of a decoded frame costs on the device, four ways.

A set of --frames resident 3840 x 2160 d1.0 frames (bench.py's synthetic frames, seeds 177, 178, ... cycled); entropy and
transforms run once, then per step the filter + colour launch of the set (HIP events: jxlhip_last_stage_ms(2)) plus the
torch passes a user needs behind it (torch events), both in device time:

  (a) rgb8 + torch     the RGB8 route, then permute().contiguous(), to(float16), one addcmul (x * scale + bias)
  (b) f32 + torch      the interleaved f32 route, then permute().contiguous(), one addcmul, to(float16)
  (c) f16 tensor       jxlhip_set_output_tensor: float16 CHW, normalised by the writer; no torch pass
  (d) bf16 tensor      the same in bfloat16

The four alternate within one process, --rounds times, the order reversed every other round; each figure is the median
of --reps steps of a round, the spread is that of the rounds' medians.

  python scripts/measure_tensor_out.py --out profiles/tensor_out_mi355x.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class _Raw:
    """Device memory of the context as a torch tensor (no copy)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_out_mi355x.json"))
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    import ctypes
    import torch
    import libjxl_amd as J
    from libjxl_amd import torch_io
    w, h = (int(v) for v in args.size.split("x"))
    frames = [J.Frame(J.encode_rgb8(J.synth_image(w, h, 177 + i), distance=1.0, strategy_mode=1), threads=8) for i in range(args.distinct)]
    scale, bias = torch_io.affine(MEAN, STD, 3)
    dev = torch.device("cuda:0")
    sc16 = torch.tensor(scale / 255.0, dtype=torch.float16, device=dev).view(3, 1, 1)
    bi16 = torch.tensor(bias, dtype=torch.float16, device=dev).view(3, 1, 1)
    sc32 = torch.tensor(scale, dtype=torch.float32, device=dev).view(3, 1, 1)
    bi32 = torch.tensor(bias, dtype=torch.float32, device=dev).view(3, 1, 1)
    L = J.lib()

    def make(case):
        ctxs, views = [], []
        out = torch.empty((args.frames, 3, h, w), dtype=torch.bfloat16 if case == "d_bf16_tensor" else torch.float16, device=dev)
        for i in range(args.frames):
            c = J.HipContext(0)
            if case == "a_rgb8_torch":
                c.set_output_format(2, 3)
            elif case == "b_f32_torch":
                c.set_output_format(0, 3)
            else:
                torch_io.bind(c, out[i], "CHW", MEAN, STD)
            c.upload(frames[i % len(frames)])
            ctxs.append(c)
        J.run_entropy_batch(ctxs)
        J.run_transform_batch(ctxs)
        J.run_filter_color_batch(ctxs)
        ctxs[0].sync()
        if case in ("a_rgb8_torch", "b_f32_torch"):
            typestr = "|u1" if case == "a_rgb8_torch" else "<f4"
            views = [torch.as_tensor(_Raw(int(L.jxlhip_rgb8_device_ptr(c._h)), (h, w, 3), typestr), device=dev) for c in ctxs]
        return ctxs, views, out

    def torch_passes(case, views, out):
        for i, v in enumerate(views):
            if case == "a_rgb8_torch":
                out[i] = torch.addcmul(bi16, v.permute(2, 0, 1).contiguous().to(torch.float16), sc16)
            else:
                out[i] = torch.addcmul(bi32, v.permute(2, 0, 1).contiguous(), sc32).to(torch.float16)

    def step(case, ctxs, views, out):
        J.run_filter_color_batch(ctxs)
        ctxs[0].sync()
        ms = ctxs[0].stage_ms(2)
        t_ms = 0.0
        if views:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch_passes(case, views, out)
            e1.record()
            e1.synchronize()
            t_ms = e0.elapsed_time(e1)
        return ms, t_ms

    cases = ["a_rgb8_torch", "b_f32_torch", "c_f16_tensor", "d_bf16_tensor"]
    sets = {k: make(k) for k in cases}
    assert all(c.pixel_route() == 3 for c in sets["c_f16_tensor"][0] + sets["d_bf16_tensor"][0])
    rows = {k: {"kernel_ms": [], "torch_ms": [], "total_ms": []} for k in cases}
    for rnd in range(args.rounds):
        for k in (cases if rnd % 2 == 0 else cases[::-1]):
            got = [step(k, *sets[k]) for _ in range(args.warmup + args.reps)][args.warmup:]
            rows[k]["kernel_ms"].append(statistics.median(g[0] for g in got))
            rows[k]["torch_ms"].append(statistics.median(g[1] for g in got))
            rows[k]["total_ms"].append(statistics.median(g[0] + g[1] for g in got))
    torch.cuda.synchronize()
    # the four hold the same picture: (c) against (a) and (b) within what float16 and the 8-bit rounding allow
    ref = sets["b_f32_torch"][2].float()
    agree = {k: float((sets[k][2].float() - ref).abs().max()) for k in cases}
    report = {"what": "filter + colour launch of %d resident %s d1.0 frames plus the torch passes to a normalised CHW tensor, device ms per "
                      "step; median of %d steps per round, %d rounds, cases alternating in one process" % (args.frames, args.size, args.reps, args.rounds),
              "frames": args.frames, "max_abs_difference_from_b": agree, "rows": {}}
    for k, v in rows.items():
        report["rows"][k] = {n: {"round_medians": [round(x, 4) for x in xs], "median": round(statistics.median(xs), 4),
                                 "spread": round(max(xs) - min(xs), 4)} for n, xs in v.items()}
    tot = {k: report["rows"][k]["total_ms"]["median"] for k in cases}
    ker = {k: report["rows"][k]["kernel_ms"]["median"] for k in cases}
    report["c_total_over_a_total"] = round(tot["c_f16_tensor"] / tot["a_rgb8_torch"], 4)
    report["c_total_over_b_total"] = round(tot["c_f16_tensor"] / tot["b_f32_torch"], 4)
    report["c_kernel_over_b_kernel"] = round(ker["c_f16_tensor"] / ker["b_f32_torch"], 4)
    report["d_kernel_over_b_kernel"] = round(ker["d_bf16_tensor"] / ker["b_f32_torch"], 4)
    for ctxs, _, _ in sets.values():
        for c in ctxs:
            c.close()
    for f in frames:
        f.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
