"""Generates tests/golden/fjxl_*.jxl with the REFERENCE's own standalone lossless encoder.

The encoder binary is oracle/_ref/fjxl_enc, compiled in place from /root/reference/lib/jxl/enc_fast_lossless.cc by
`make -C oracle ref` (nothing of the reference is copied into this repository: the committed files are encoder OUTPUT,
i.e. data).  The expected pixels are not stored: every fixture's input image is a deterministic function of its name
(see `golden_image`), which the tests re-evaluate and compare bit-exactly with what the oracle decodes.

Run from the repository root:  python tests/golden/make_fjxl_golden.py [names]  (no names: the cases without a .jxl yet;
`make_fjxl_golden.py fjxl_7x5_rgb_e0 ...` rewrites those). The manifest records each case's bit depth.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ENC = os.path.join(ROOT, "oracle", "_ref", "fjxl_enc")

# name: (width, height, channels, kind, effort, bits). Samples above 8 bits are 16-bit little-endian in the raw input.
CASES = {
    "fjxl_1x1_rgb_e2": (1, 1, 3, "noise", 2, 8),
    "fjxl_7x5_rgb_e0": (7, 5, 3, "ramp", 0, 8),
    "fjxl_37x29_rgba_e2": (37, 29, 4, "smooth", 2, 8),
    "fjxl_64x64_gray_e5": (64, 64, 1, "smooth", 5, 8),
    "fjxl_64x64_graya_e2": (64, 64, 2, "noise", 2, 8),
    "fjxl_256x256_rgb_e1": (256, 256, 3, "smooth", 1, 8),
    "fjxl_300x280_rgb_e2": (300, 280, 3, "smooth", 2, 8),      # 4 groups: TOC, multi-group Modular, RCT
    "fjxl_300x280_rgb_e2_noise": (300, 280, 3, "noise", 2, 8),  # incompressible: long prefix codes, raw bits
    "fjxl_520x260_rgba_e5": (520, 260, 4, "ramp", 5, 8),        # LZ77 run-length path
    "fjxl_100x100_rgb_flat_e2": (100, 100, 3, "flat", 2, 8),    # palette + RLE
    # full-range noise at efforts 0 and 1, two groups wide (DESIGN.md "fjxl's AVX-512 path")
    "fjxl_264x40_rgb_e0_noise": (264, 40, 3, "noise", 0, 8),
    "fjxl_264x40_rgba_e0_noise": (264, 40, 4, "noise", 0, 8),
    "fjxl_264x40_rgb_e1_noise": (264, 40, 3, "noise", 1, 8),
    "fjxl_264x40_rgba_e1_noise": (264, 40, 4, "noise", 1, 8),
    # deep (and shallow) samples: fjxl's 16-bit residual paths, wider tokens, YCoCg chroma one bit wider
    "fjxl_d1_64x48_gray_e0_noise": (64, 48, 1, "noise", 0, 1),
    "fjxl_d1_40x30_rgba_e2": (40, 30, 4, "smooth", 2, 1),
    "fjxl_d5_70x50_graya_e2_noise": (70, 50, 2, "noise", 2, 5),
    "fjxl_d5_300x40_rgb_e0": (300, 40, 3, "smooth", 0, 5),       # across a group edge
    "fjxl_d10_64x64_rgb_e0_noise": (64, 64, 3, "noise", 0, 10),
    "fjxl_d10_280x36_rgba_e2": (280, 36, 4, "smooth", 2, 10),    # across a group edge
    "fjxl_d12_100x80_gray_e2": (100, 80, 1, "smooth", 2, 12),
    "fjxl_d12_48x40_rgba_e0_noise": (48, 40, 4, "noise", 0, 12),
    "fjxl_d14_90x60_graya_e0": (90, 60, 2, "smooth", 0, 14),
    "fjxl_d14_50x40_rgb_e2_noise": (50, 40, 3, "noise", 2, 14),
    "fjxl_d16_40x30_rgba_e2_noise": (40, 30, 4, "noise", 2, 16),
    "fjxl_d16_270x24_rgb_e0": (270, 24, 3, "smooth", 0, 16),     # across a group edge
    "fjxl_d16_33x17_gray_e0_noise": (33, 17, 1, "noise", 0, 16),
}


def golden_image(name):
    """The encoder's input: H x W x C, uint8 up to 8 bits, uint16 above."""
    w, h, nc, kind, _, bits = CASES[name]
    seed = int(hashlib.sha256(name.encode()).hexdigest()[:8], 16)
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise" and bits != 8:
        return rng.integers(0, 1 << bits, (h, w, nc)).astype(np.uint8 if bits <= 8 else np.uint16)
    if kind == "ramp":
        a = np.stack([(x * 3 + y * (c + 1)) % 256 for c in range(nc)], -1)
    elif kind == "noise":
        a = rng.integers(0, 256, (h, w, nc))
    elif kind == "flat":
        a = np.zeros((h, w, nc), np.int64) + np.array([200, 40, 90, 255][:nc])
        a[h // 3: h // 2, w // 4: w // 2] = np.array([10, 250, 30, 128][:nc])
    else:
        a = np.stack([128 + 60 * np.sin(x / 17.0 + c) + 50 * np.cos(y / 23.0) for c in range(nc)], -1)
        a = a + rng.integers(-3, 4, (h, w, nc))
        a[h // 4: h // 2, w // 4: w // 2] = 37
    a = np.clip(a, 0, 255)
    if bits == 8:
        return a.astype(np.uint8)
    a = np.round(a * (((1 << bits) - 1) / 255.0)).astype(np.int64)  # (the 8-bit picture at the case's depth)
    return a.astype(np.uint8 if bits <= 8 else np.uint16)


def main(names=None):
    """Regenerates the fixtures `names` (default: those without a .jxl yet); the manifest keeps every case."""
    assert os.path.exists(ENC), "build the reference encoder first: make -C oracle ref"
    path = os.path.join(HERE, "fjxl_manifest.json")
    manifest = json.load(open(path)) if os.path.exists(path) else {}
    for name, (w, h, nc, kind, effort, bits) in CASES.items():
        out = os.path.join(HERE, name + ".jxl")
        if names is None and os.path.exists(out) and name in manifest:
            continue
        if names is not None and name not in names:
            continue
        img = golden_image(name)
        raw = os.path.join("/tmp", name + ".raw")
        img.astype("<u2" if bits > 8 else np.uint8).tofile(raw)
        subprocess.run([ENC, raw, str(w), str(h), str(nc), str(bits), str(effort), out], check=True)
        manifest[name] = {"width": w, "height": h, "channels": nc, "kind": kind, "effort": effort, "bits": bits,
                          "jxl_bytes": os.path.getsize(out), "pixels_sha256": hashlib.sha256(img.tobytes()).hexdigest()}
        print(name, manifest[name]["jxl_bytes"])
    for name in manifest:
        manifest[name].setdefault("bits", CASES[name][5])
    json.dump(manifest, open(path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main(sys.argv[1:] or None)
