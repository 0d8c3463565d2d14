"""Timing aid for the colour stage of tagged XYB images: decodes one 3840x2160 frame `--frames` times through the
JxlDecoder API (RGB8 out), untagged (sRGB), tagged Display P3 with the sRGB curve, or tagged Rec.2100 PQ. Run it under
`rocprofv3 --kernel-trace --stats -- python scripts/color_target_timing.py --encoding pq` and divide the kernel totals by
--frames for the per-frame GPU time: P3 should show the sRGB image's kernels and times, PQ one more launch (k_color_out)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import libjxl_amd as J  # noqa: E402
import color_api as A  # noqa: E402

TAGS = {"srgb": None, "p3": dict(white_point=1, primaries=11, transfer_function=13),
        "pq": dict(white_point=1, primaries=9, transfer_function=16, intensity_target=10000.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encoding", choices=sorted(TAGS), default="srgb")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    a = ap.parse_args()
    img = J.synth_image(a.width, a.height, seed=7)
    if TAGS[a.encoding]:
        J.set_xyb_color_encoding(**TAGS[a.encoding])
    try:
        data = J.encode_rgb8(img)
    finally:
        J.set_xyb_color_encoding(None)
    L = A.setup(J.lib())
    shape = (a.height, a.width, 3)
    A.decode(L, data, shape, 2)  # warm-up
    t0 = time.perf_counter()
    for _ in range(a.frames):
        A.decode(L, data, shape, 2)
    dt = (time.perf_counter() - t0) / a.frames
    print("encoding %s: %dx%d, %d frames, %.2f ms per API decode (host included)" % (a.encoding, a.width, a.height, a.frames, dt * 1e3))


if __name__ == "__main__":
    main()
