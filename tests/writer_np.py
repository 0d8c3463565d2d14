"""NumPy reading of the reference's pixel writer, in float32, held bit-exact against the device writers.

Written from the reference's text alone, sharing no code with the kernels (k_modular_output, StorePixel / WritePixel) or
the oracle:

* lib/jxl/render_pipeline/stage_write.cc:265-286, MakeUnsigned<T>: ``v = Mul(v, mul)``; for an 8-bit T only,
  ``v = Add(v, kDither[((y0 + 13c) % 32) * 48 + (x0 + 23c) % 32])``; ``v = Clamp(0, v, mul)``; ``NearestInt`` (round half
  to even); each step one float32 rounding, in that order. ``mul = 2^bits - 1`` (:550).
* :334-345 (ProcessRow): ``flip_y`` replaces ypos by ``height - 1 - ypos`` before any value is made;
  :484-487, :524-545 (OutputBuffers / FlipX): ``flip_x`` reverses the row and moves ``xstart`` to ``width - xstart - len``,
  so the dither cell is taken at the flipped x; :662-699 (WriteToOutput): the transpose happens after the values are made,
  the row ``ypos`` becoming a column. :441-458: which of the eight orientations flip x, flip y and transpose.
* :589-626 (StoreFloat16Row): float16 by DemoteTo, round to nearest even (``np.float16``).
* lib/jxl/decode.cc:179-189 (GetBitDepth): JXL_BIT_DEPTH_FROM_PIXEL_FORMAT takes 8 / 16 bits from the data type,
  FROM_CODESTREAM the image's (or, for an extra-channel buffer, that channel's) bits_per_sample, CUSTOM the caller's.
* lib/jxl/dec_external_image.cc: the same conversions for the extra-channel buffers, one channel each (c = 0).

The dither table is ``dither32`` of tests/golden/ref_constant_floats.json: the 32 columns of kDither's 48-wide rows
(stage_write.cc:64-256) the reference ever indexes, pinned by the KATs; it is not read from the product.
"""
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
FROM_PIXEL_FORMAT, FROM_CODESTREAM, CUSTOM = 0, 1, 2  # JxlBitDepthType
_DITHER = None


def dither32():
    global _DITHER
    if _DITHER is None:
        d = json.load(open(os.path.join(_HERE, "golden", "ref_constant_floats.json")))["dither32"]
        _DITHER = np.asarray(d, np.float32).reshape(32, 32)
    return _DITHER


def orientation_flags(orientation):
    """(flip_x, flip_y, transpose) of the orientation the writer undoes (EXIF numbering 1..8)."""
    return orientation in (2, 3, 7, 8), orientation in (3, 4, 6, 7), orientation in (5, 6, 7, 8)


def out_bits(mode, data_type, codestream_bits, custom_bits=0):
    """decode.cc GetBitDepth for integer output: the `bits` of mul = 2^bits - 1."""
    if mode == FROM_PIXEL_FORMAT:
        return 8 if data_type == "u8" else 16
    if mode == FROM_CODESTREAM:
        return codestream_bits
    return custom_bits


def make_unsigned(f, mul, dither=None, fused=False):
    """MakeUnsigned on float32 samples `f` -> int64. fused=True: the contracted form, one rounding of the exact f*mul+d
    (exact in float64: a 24-bit significand times mul < 2^16 plus a dither of 5 decimals), for telling a contraction
    difference from a real error."""
    f = np.asarray(f, np.float32)
    m = np.float32(mul)
    if fused:
        d = np.float64(0) if dither is None else np.asarray(dither, np.float32).astype(np.float64)
        v = (f.astype(np.float64) * np.float64(m) + d).astype(np.float32)
    else:
        v = (f * m).astype(np.float32)
        if dither is not None:
            v = (v + np.asarray(dither, np.float32)).astype(np.float32)
    v = np.minimum(np.maximum(v, np.float32(0)), m)
    return np.rint(v).astype(np.int64)


def write(planes, data_type, bits=8, orientation=1, fused=False):
    """The caller's buffer for writer input `planes` (float32, H x W x C, the interleave order of the output: colour then
    alpha, or one extra channel with C = 1). data_type: "u8", "u16", "f16" or "f32"; bits: of mul (out_bits)."""
    p = np.asarray(planes, np.float32)
    h, w, nc = p.shape
    flip_x, flip_y, transpose = orientation_flags(orientation)
    if flip_x:
        p = p[:, ::-1]
    if flip_y:
        p = p[::-1]
    # (x, y) now the dither coordinates: the flipped position, before the transpose
    if data_type == "f32":
        out = p.copy()
    elif data_type == "f16":
        out = p.astype(np.float16)
    else:
        mul = (1 << bits) - 1
        out = np.empty(p.shape, np.uint8 if data_type == "u8" else np.uint16)
        y, x = np.mgrid[0:h, 0:w]
        for c in range(nc):
            d = dither32()[(y + 13 * c) % 32, (x + 23 * c) % 32] if data_type == "u8" else None
            out[..., c] = make_unsigned(p[..., c], mul, d, fused)
    if transpose:
        out = out.transpose(1, 0, 2)
    return np.ascontiguousarray(out)
