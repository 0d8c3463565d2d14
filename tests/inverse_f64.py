"""A float64 reading of the middle of the VarDCT decode: quantised coefficients, DC image, quant field and
chroma-from-luma maps -> the planes the loop filters read ("xyb_idct"). Written from the reference's text and from nothing
under libjxl_amd/csrc or oracle/:
  * lib/jxl/dec_group.cc:116-181 (DequantLane, DequantBlock), :262-320 and :430-452 (the walk over a group, the colour
    tile of a varblock, which varblocks carry a subsampled channel and where its DC and its pixels lie);
  * lib/jxl/quantizer-inl.h:34-67 (AdjustQuantBias, as the comment in it words it: a division, not the approximate
    reciprocal), quantizer.h:83-85 (inv_global_scale), dec_cache.h:161-162 (x_dm / b_dm multipliers);
  * lib/jxl/chroma_from_luma.h:51-57 (YtoXRatio / YtoBRatio), :28-32 (tiles of 64 x 64 pixels);
  * lib/jxl/dec_transforms-inl.h:35-64 (ReinterpretingDCT), :66-93 (IDCT2TopBlock), :95-454 (AFV), :456-689
    (TransformToPixels, every case), :691-818 (LowestFrequenciesFromDC); dct-inl.h:354-397 for which index of a
    coefficient block is the horizontal frequency; dct_for_test.h:20-62 for the DCT itself;
  * lib/jxl/render_pipeline/stage_chroma_upsampling.cc:45-57 and :87-101, simple_render_pipeline.cc:129-164 (the
    mirroring about the channel's own size), dec_cache.cc:138-149 (horizontal before vertical), frame_header.cc:30-31.
What it shares with the rest of the suite: the constants the reference's source lists, as DATA (tests/golden/
ref_constant_floats.json: afv_basis, quant_bias, dct_resample_scales, quant_library; ref_constant_tables.json:
covered_blocks_x / _y, strategy_to_quant_table) and host_tables_np's dequantisation-table generator and natural order,
themselves readings of the reference's text. Both the oracle (oracle/jxlo_vardct.h) and the HIP kernels (k_idct_fast,
k_dct_big, k_special, k_chroma_upsample) are held to it: a misreading shared by those two shows here.

DCT-family inverses are plain matrix products with the float64 basis; nothing here is fast, pruned or reordered.
Out of scope: coded dequantisation tables (default library tables only), bands, anything behind "xyb_idct"."""
import functools
import json
import os

import numpy as np

import host_tables_np as T

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the named misreadings of tests/test_inverse_f64.py: inverse(..., misread=NAME) computes the stage with that one mistake
MISREADINGS = ("swap_x_dm_b_dm", "bias_of_channel_1", "no_bias_over_q", "no_base_correlation", "cfl_tile_of_last_block",
               "cfl_on_llf", "no_resample_scale_on_one_axis", "tall_not_transposed", "swap_afv1_afv2", "swap_dct4x8_dct8x4",
               "identity_corner_transposed")


@functools.lru_cache(maxsize=None)
def _constants():
    f = json.load(open(os.path.join(_GOLDEN, "ref_constant_floats.json")))
    t = json.load(open(os.path.join(_GOLDEN, "ref_constant_tables.json")))
    return f, t


def covered(strategy):
    """(blocks across, blocks down) of a strategy."""
    t = _constants()[1]
    return t["covered_blocks_x"][strategy], t["covered_blocks_y"][strategy]


@functools.lru_cache(maxsize=None)
def dequant_table(strategy):
    """[3][size] float64: the default table of the strategy, 1 / weights, in the coefficient layout (short side as rows)."""
    f, t = _constants()
    kind = t["strategy_to_quant_table"][strategy]
    w = T.compute_weights(kind, T.library_encoding(kind, f["quant_library"]))
    return 1.0 / w.astype(np.float64).reshape(3, -1)


@functools.lru_cache(maxsize=None)
def _idct_matrix(n):
    """[pixel][frequency]: IDCT1D of dct_for_test.h:44-62 (alpha(u) * sqrt 2 * cos((y + 1/2) u pi / N))."""
    y = (np.arange(n) + 0.5)[:, None]
    u = np.arange(n)[None, :]
    alpha = np.where(u == 0, np.sqrt(0.5), 1.0)
    return alpha * np.sqrt(2.0) * np.cos(y * u * np.pi / n)


@functools.lru_cache(maxsize=None)
def _dct_matrix(n):
    """[frequency][sample]: DCT1D of dct_for_test.h:23-40 (the same, divided by N)."""
    return _idct_matrix(n).T / n


def idct(block, rows, cols):
    """ComputeScaledIDCT<rows, cols> (dct-inl.h:377-397): `block` in the layout the reference stores, [rows][cols] =
    [vertical][horizontal frequency] when rows < cols, else [cols][rows] = [horizontal][vertical]; -> pixels [rows][cols]."""
    if rows < cols:
        f = np.asarray(block, np.float64).reshape(rows, cols)
    else:
        f = np.asarray(block, np.float64).reshape(cols, rows).T
    return _idct_matrix(rows) @ f @ _idct_matrix(cols).T


def lowest_frequencies(dc, misread=None):
    """ReinterpretingDCT (dec_transforms-inl.h:35-64) of the varblock's DC samples dc[cy][cx]: the cy x cx DCT, every
    coefficient times the resample scales of its two frequencies; returned in the coefficient layout's orientation
    ([cy][cx] when cy < cx, else transposed)."""
    scales = _constants()[0]["dct_resample_scales"]
    cy, cx = dc.shape
    g = _dct_matrix(cy) @ dc @ _dct_matrix(cx).T
    sy = np.asarray(scales["%d_%d" % (cy, cy * 8)], np.float64)
    sx = np.asarray(scales["%d_%d" % (cx, cx * 8)], np.float64)
    if misread == "no_resample_scale_on_one_axis":
        sx = np.ones_like(sx)
    g = g * sy[:, None] * sx[None, :]
    return g if cy < cx else g.T


def _idct2_top(block, s):
    """IDCT2TopBlock<S> (dec_transforms-inl.h:66-93) on an 8 x 8 array, in place."""
    n = s // 2
    temp = np.zeros((8, 8))
    for y in range(n):
        for x in range(n):
            c00, c01, c10, c11 = block[y, x], block[y, n + x], block[y + n, x], block[y + n, n + x]
            temp[y * 2, x * 2] = c00 + c01 + c10 + c11
            temp[y * 2, x * 2 + 1] = c00 + c01 - c10 - c11
            temp[y * 2 + 1, x * 2] = c00 - c01 + c10 - c11
            temp[y * 2 + 1, x * 2 + 1] = c00 - c01 - c10 + c11
    block[:s, :s] = temp[:s, :s]


def _afv(co, kind):
    """AFVTransformToPixels<kind> (dec_transforms-inl.h:399-454); co[8][8] as stored."""
    basis = np.asarray(_constants()[0]["afv_basis"], np.float64).reshape(16, 16)
    afv_x, afv_y = kind & 1, kind // 2
    px = np.zeros((8, 8))
    b00, b01, b10 = co[0, 0], co[0, 1], co[1, 0]
    dcs = ((b00 + b10 + b01) * 4.0, b00 + b10 - b01, b00 - b10)
    coeff = co[0:8:2, 0:8:2].copy().reshape(16)
    coeff[0] = dcs[0]
    block = (coeff @ basis).reshape(4, 4)  # pixel i = sum over j of coeff[j] * basis[j][i]
    for iy in range(4):
        for ix in range(4):
            px[iy + afv_y * 4, afv_x * 4 + ix] = block[3 - iy if afv_y == 1 else iy, 3 - ix if afv_x == 1 else ix]
    b = co[0:8:2, 1:8:2].copy()
    b[0, 0] = dcs[1]
    x0 = 0 if afv_x == 1 else 4
    px[afv_y * 4:afv_y * 4 + 4, x0:x0 + 4] = idct(b, 4, 4)
    b = co[1:8:2, :].copy()
    b[0, 0] = dcs[2]
    y0 = 0 if afv_y == 1 else 4
    px[y0:y0 + 4, :] = idct(b, 4, 8)
    return px


def to_pixels(strategy, flat, misread=None):
    """TransformToPixels (dec_transforms-inl.h:456-689): the strategy's coefficients as stored -> pixels [rows][cols]."""
    if misread == "swap_afv1_afv2" and strategy in (15, 16):
        strategy = 31 - strategy
    if misread == "swap_dct4x8_dct8x4" and strategy in (12, 13):
        strategy = 25 - strategy
    cx, cy = covered(strategy)
    rows, cols = cy * 8, cx * 8
    flat = np.asarray(flat, np.float64)
    if strategy not in (1, 2, 3, 12, 13, 14, 15, 16, 17):  # the DCT family
        if misread == "tall_not_transposed" and rows > cols:
            return _idct_matrix(rows) @ flat.reshape(rows, cols) @ _idct_matrix(cols).T
        return idct(flat, rows, cols)
    co = flat.reshape(8, 8)
    px = np.zeros((8, 8))
    if strategy == 1:  # IDENTITY
        b00, b01, b10, b11 = co[0, 0], co[0, 1], co[1, 0], co[1, 1]
        if misread == "identity_corner_transposed":
            b01, b10 = b10, b01
        dcs = (b00 + b01 + b10 + b11, b00 + b01 - b10 - b11, b00 - b01 + b10 - b11, b00 - b01 - b10 + b11)
        for y in range(2):
            for x in range(2):
                sub = co[y::2, x::2]  # sub[iy][ix] = coefficients[(y + iy * 2) * 8 + x + ix * 2]
                centre = dcs[y * 2 + x] - (sub.sum() - sub[0, 0]) * (1.0 / 16)
                out = sub + centre
                out[1, 1] = centre
                out[0, 0] = sub[1, 1] + centre
                px[y * 4:y * 4 + 4, x * 4:x * 4 + 4] = out
        return px
    if strategy == 2:  # DCT2X2
        b = co.copy()
        for s in (2, 4, 8):
            _idct2_top(b, s)
        return b
    if strategy == 3:  # DCT4X4
        b00, b01, b10, b11 = co[0, 0], co[0, 1], co[1, 0], co[1, 1]
        dcs = (b00 + b01 + b10 + b11, b00 + b01 - b10 - b11, b00 - b01 + b10 - b11, b00 - b01 - b10 + b11)
        for y in range(2):
            for x in range(2):
                b = co[y::2, x::2].copy()
                b[0, 0] = dcs[y * 2 + x]
                px[y * 4:y * 4 + 4, x * 4:x * 4 + 4] = idct(b, 4, 4)
        return px
    if strategy in (12, 13):  # DCT4X8: two 4 x 8 halves one above the other; DCT8X4: two 8 x 4 halves side by side
        dcs = (co[0, 0] + co[1, 0], co[0, 0] - co[1, 0])
        for h in range(2):
            b = co[h::2, :].copy()  # b[iy][ix] = coefficients[(h + iy * 2) * 8 + ix]
            b[0, 0] = dcs[h]
            if strategy == 12:
                px[h * 4:h * 4 + 4, :] = idct(b, 4, 8)
            else:
                px[:, h * 4:h * 4 + 4] = idct(b, 8, 4)
        return px
    return _afv(co, strategy - 14)


def adjust_quant_bias(q, c, biases, misread=None):
    """AdjustQuantBias (quantizer-inl.h:47-52): 0 -> 0, +-1 -> +-biases[c], else q - biases[3] / q."""
    q = np.asarray(q, np.float64)
    one = biases[1 if misread == "bias_of_channel_1" else c]
    safe = np.where(q == 0, 1.0, q)
    far = q if misread == "no_bias_over_q" else q - biases[3] / safe
    return np.where(q == 0, 0.0, np.where(np.abs(q) == 1, np.sign(q) * one, far))


def shifts(cs):
    """(hshift[3], vshift[3]) of a chroma_subsampling value: channel_mode of channel c in bits 2c, 2c + 1."""
    kh, kv = (0, 1, 1, 0), (0, 1, 0, 1)
    modes = [(cs >> (2 * c)) & 3 for c in range(3)]
    mh, mv = max(kh[m] for m in modes), max(kv[m] for m in modes)
    return [mh - kh[m] for m in modes], [mv - kv[m] for m in modes]


def _upsample2(p, axis):
    """One chroma upsampling stage along `axis`: out[2i] = 3/4 in[i] + 1/4 in[i - 1], out[2i + 1] = 3/4 in[i] + 1/4 in[i + 1],
    the input mirrored about its own size."""
    p = np.moveaxis(p, axis, 0)
    pp = np.concatenate([p[:1], p, p[-1:]])
    out = np.empty((2 * p.shape[0],) + p.shape[1:])
    out[0::2] = 0.75 * p + 0.25 * pp[:-2]
    out[1::2] = 0.75 * p + 0.25 * pp[2:]
    return np.moveaxis(out, 0, axis)


def inverse(coeffs, dc, acs, quant, ytox, ytob, header, cs=0, size=None, misread=None):
    """coeffs [groups][3][65536]: quantised coefficients, the varblocks of a group one after another in raster order of their
    top-left blocks, each in the reference's coefficient layout; dc [3][yb][xb]; acs [yb][xb] (strategy << 1 | first block);
    quant [yb][xb] (raw quant field); ytox / ytob: the colour tiles' factors, rows of ceil(xb / 8); header: the quantiser
    fields as coded (jxlo.Decoded.quant_header). cs: the frame's chroma_subsampling value; with cs != 0, size = (xsize, ysize)
    and the result is defined on the first ysize rows and xsize columns only. -> [3][yb * 8][xb * 8] float64."""
    f, _ = _constants()
    biases = [float(v) for v in f["quant_bias"]]
    acs = np.asarray(acs)
    yb, xb = acs.shape
    dc = np.asarray(dc, np.float64).reshape(3, yb, xb)
    quant = np.asarray(quant).reshape(yb, xb)
    xt = (xb + 7) // 8
    ytox = np.asarray(ytox, np.int64).reshape(-1, xt)
    ytob = np.asarray(ytob, np.int64).reshape(-1, xt)
    assert ytox.shape[0] >= (yb + 7) // 8
    inv_global_scale = 65536.0 / header["global_scale"]
    x_dm = 0.8 ** (header["x_qm_scale"] - 2.0)
    b_dm = 0.8 ** (header["b_qm_scale"] - 2.0)
    if misread == "swap_x_dm_b_dm":
        x_dm, b_dm = b_dm, x_dm
    dm = (x_dm, 1.0, b_dm)
    base = (0.0, 0.0) if misread == "no_base_correlation" else (header["base_corr_x"], header["base_corr_b"])
    hs, vs = shifts(cs)
    out = np.zeros((3, yb * 8, xb * 8))
    xg = (xb + 31) // 32
    for g in range(coeffs.shape[0]):
        gy, gx = divmod(g, xg)
        offset = 0
        for by in range(gy * 32, min(gy * 32 + 32, yb)):
            for bx in range(gx * 32, min(gx * 32 + 32, xb)):
                a = int(acs[by, bx])
                if not a & 1:
                    continue
                st = a >> 1
                cx, cy = covered(st)
                n = cx * cy * 64
                q = coeffs[g, :, offset:offset + n]
                offset += n
                table = dequant_table(st)
                scaled = inv_global_scale / float(quant[by, bx])
                block = [adjust_quant_bias(q[c], c, biases, misread) * table[c] * (scaled * dm[c]) for c in range(3)]
                ty, tx = (by // 8, bx // 8) if misread != "cfl_tile_of_last_block" else ((by + cy - 1) // 8, (bx + cx - 1) // 8)
                ratio_x = base[0] + ytox[ty, tx] / float(header["color_factor"])
                ratio_b = base[1] + ytob[ty, tx] / float(header["color_factor"])
                block[0] = block[0] + ratio_x * block[1]
                block[2] = block[2] + ratio_b * block[1]
                stride = max(cx, cy) * 8
                llf = []
                for c in range(3):
                    sby, sbx = by >> vs[c], bx >> hs[c]
                    llf.append(lowest_frequencies(dc[c, sby:sby + cy, sbx:sbx + cx], misread))
                if misread == "cfl_on_llf":
                    llf[0] = llf[0] + ratio_x * llf[1]
                    llf[2] = llf[2] + ratio_b * llf[1]
                for c in range(3):
                    sby, sbx = by >> vs[c], bx >> hs[c]
                    if (sbx << hs[c]) != bx or (sby << vs[c]) != by:
                        continue  # this varblock does not lie on the channel's grid
                    b = block[c].reshape(-1, stride).copy()
                    b[:llf[c].shape[0], :llf[c].shape[1]] = llf[c]
                    out[c, sby * 8:sby * 8 + cy * 8, sbx * 8:sbx * 8 + cx * 8] = to_pixels(st, b.reshape(-1), misread)
    if cs == 0:
        return out
    xsize, ysize = size
    res = np.zeros_like(out)
    for c in range(3):
        p = out[c, :-(-ysize // (1 << vs[c])), :-(-xsize // (1 << hs[c]))]
        if hs[c]:
            p = _upsample2(p, 1)[:, :xsize]
        if vs[c]:
            p = _upsample2(p, 0)[:ysize]
        res[c, :ysize, :xsize] = p
    return res
