"""The HIP blending kernels (-m gpu) against tests/blending_np.py, the reading of blending.cc, alpha.cc and
stage_blending.cc that shares no code with the kernels or the oracle: k_canvas_blend through jxlhip_debug_blend_rect and
k_patches_add through jxlhip_debug_patches, on crafted planes. The bar is the reading's: every sample equal to its float32
form (derived there). The inputs are blending_np.crafted_layers: colours in [-0.5, 1.5], alphas k / 64, -0.25 and 1.5,
paired so that a straight-alpha blend divides by 0 (the guard) or by at least 1 / 64.

k_canvas_blend: a 300 x 5 canvas (two workgroups of 256 columns) and an 80 x 3 frame at origins that stick out on every
side, lie wholly outside, or lie inside; all 5 x 5 modes x both clamps x premultiplied or not with alpha, modes 0..4 without;
the colour and the alpha background from different arrays, each NULL in turn.
k_patches_add: a 600 x 6 frame (three strides of 256 columns), slots of 64 x 48 and 300 x 4; every (colour mode, alpha mode)
pair once; positions that cross a stride, start in the second, are clipped by xsize, are wider than a stride, and three that
overlap in dictionary order; with and without an alpha plane; a band of rows."""
import ctypes
import itertools

import numpy as np
import pytest

import blending_np as B

pytestmark = pytest.mark.gpu

INVALID = 1  # JXLHIP_ERR_INVALID_ARGUMENT
F32 = np.float32
CW, CH, FW, FH = 300, 5, 80, 3
ORIGINS = ((-30, -1), (250, 3), (300, 0), (0, 5), (-80, 0), (110, 1))
PW, PH = 600, 6


class Blend(ctypes.Structure):
    _fields_ = [("x0", ctypes.c_int32), ("y0", ctypes.c_int32)] + [(n, ctypes.c_uint32) for n in (
        "mode", "alpha_mode", "source", "alpha_source", "clamp", "alpha_clamp")] + [("save_slot", ctypes.c_int32)]


class Patches(ctypes.Structure):  # JxlHipPatches, include/jxl_amd_hip.h
    _fields_ = [("num_positions", ctypes.c_uint32), ("num_row_entries", ctypes.c_uint32), ("records", ctypes.c_void_p),
                ("row_start", ctypes.c_void_p), ("row_list", ctypes.c_void_p), ("slot_planes", ctypes.c_void_p * 4),
                ("slot_w", ctypes.c_uint32 * 4), ("slot_h", ctypes.c_uint32 * 4), ("uses_alpha", ctypes.c_uint32),
                ("premultiplied", ctypes.c_uint32), ("slot_alpha", ctypes.c_void_p * 4)]


@pytest.fixture(scope="module")
def ctx(built):
    c = built.HipContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def lib(built):
    L = built.lib()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.jxlhip_debug_blend_rect.argtypes = [ctypes.c_int, u32, u32, vp, vp, vp, u32, u32, ctypes.POINTER(Blend), u32, u32, vp]
    L.jxlhip_debug_patches.argtypes = [vp, vp, vp, u32, u32, ctypes.POINTER(Patches), u32, u32, vp, vp]
    return L


# ---- k_canvas_blend
@pytest.fixture(scope="module")
def canvas_case():
    """The colour slot and the alpha slot ([4][CH][CW] each; what the other one would supply is different in each), and a
    canvas-sized foreground whose alphas are paired with the alpha slot's sample by sample."""
    bg, bga, fg, fga = B.crafted_layers(21, (CH, CW))
    assert B.blend_conditioning(bga, fga) >= 1 / 64
    rng = np.random.default_rng(22)
    color_slot = np.concatenate([bg, rng.choice(B.ALPHA_VALUES, (1, CH, CW)).astype(F32)])
    alpha_slot = np.concatenate([rng.uniform(-0.5, 1.5, (3, CH, CW)).astype(F32), bga[None]])
    return color_slot, alpha_slot, np.concatenate([fg, fga[None]])


def _frame_at(full_fg, x0, y0):
    """The FW x FH frame whose sample (fx, fy) is the canvas-sized foreground's at (x0 + fx, y0 + fy), wrapped: where the
    frame lies on the canvas it meets the sample it was paired with."""
    ys = (np.arange(FH) + y0) % CH
    xs = (np.arange(FW) + x0) % CW
    return np.ascontiguousarray(full_fg[:, ys][:, :, xs])


def _blend_rect(lib, color_slot, alpha_slot, frame, x0, y0, mode, alpha_mode, clamp, alpha_clamp, has_alpha, premultiplied):
    out = np.full((4, CH, CW), 7.0, F32)
    inter = np.ascontiguousarray(frame.transpose(1, 2, 0))
    b = Blend(x0, y0, mode, alpha_mode, 0, 0, clamp, alpha_clamp, -1)
    r = lib.jxlhip_debug_blend_rect(0, CW, CH, None if color_slot is None else color_slot.ctypes.data,
                                    None if alpha_slot is None else alpha_slot.ctypes.data, inter.ctypes.data, FW, FH, ctypes.byref(b),
                                    int(has_alpha), int(premultiplied), out.ctypes.data)
    assert r == 0, r
    return out


@pytest.mark.parametrize("premultiplied", [0, 1])
def test_canvas_blend_every_mode_pair_at_every_origin(lib, canvas_case, premultiplied):
    color_slot, alpha_slot, full_fg = canvas_case
    bad = []
    for (x0, y0) in ORIGINS:
        frame = _frame_at(full_fg, x0, y0)
        for mode, alpha_mode, clamp, alpha_clamp in itertools.product(range(5), range(5), (0, 1), (0, 1)):
            if clamp != alpha_clamp and (x0, y0) != (110, 1):  # (the two clamps apart: at the origin inside the canvas)
                continue
            want = B.blend_frame(CW, CH, color_slot, alpha_slot, frame, x0, y0, mode, alpha_mode, clamp, alpha_clamp, True, premultiplied)
            got = _blend_rect(lib, color_slot, alpha_slot, frame, x0, y0, mode, alpha_mode, clamp, alpha_clamp, True, premultiplied)
            if not np.array_equal(got, want):
                bad.append((x0, y0, mode, alpha_mode, clamp, alpha_clamp, float(np.abs(got - want).max())))
    assert not bad, (len(bad), bad[:8])


def test_canvas_blend_with_a_slot_never_written(lib, canvas_case):
    """Each background NULL in turn, and both: zeros (stage_blending.cc:165-177). With the alpha background 0 the new alpha of
    a blend is the frame's own: 0, at least 1 / 64, or not above 0 (-0.25 unclamped: the guard)."""
    color_slot, alpha_slot, full_fg = canvas_case
    bad = []
    for (x0, y0), (cs, als) in itertools.product(((110, 1), (-30, -1)), ((None, alpha_slot), (color_slot, None), (None, None))):
        frame = _frame_at(full_fg, x0, y0)
        for mode, alpha_mode, clamp, premultiplied in itertools.product(range(5), range(5), (0, 1), (0, 1)):
            want = B.blend_frame(CW, CH, cs, als, frame, x0, y0, mode, alpha_mode, clamp, clamp, True, premultiplied)
            got = _blend_rect(lib, cs, als, frame, x0, y0, mode, alpha_mode, clamp, clamp, True, premultiplied)
            if not np.array_equal(got, want):
                bad.append((x0, y0, cs is None, als is None, mode, alpha_mode, clamp, premultiplied, float(np.abs(got - want).max())))
    assert not bad, (len(bad), bad[:8])


def test_canvas_blend_without_alpha(lib, canvas_case):
    """blending.cc:150-184 on an image without alpha: blend replaces, alpha-weighted add adds. Only the colour planes are the
    image's."""
    color_slot, alpha_slot, full_fg = canvas_case
    bad = []
    for (x0, y0), cs in itertools.product(ORIGINS, (color_slot, None)):
        frame = _frame_at(full_fg, x0, y0)
        for mode, clamp in itertools.product(range(5), (0, 1)):
            want = B.blend_frame(CW, CH, cs, None, frame, x0, y0, mode, 0, clamp, 0, False, 0)
            got = _blend_rect(lib, cs, None, frame, x0, y0, mode, 0, clamp, 0, False, 0)
            if not np.array_equal(got[:3], want[:3]):
                bad.append((x0, y0, cs is None, mode, clamp, float(np.abs(got[:3] - want[:3]).max())))
    assert not bad, (len(bad), bad[:8])


def test_blend_rect_refuses_bad_arguments(lib, canvas_case):
    color_slot, alpha_slot, full_fg = canvas_case
    frame = np.ascontiguousarray(_frame_at(full_fg, 0, 0).transpose(1, 2, 0))
    out = np.full((4, CH, CW), 7.0, F32)
    c, a, f, o = color_slot.ctypes.data, alpha_slot.ctypes.data, frame.ctypes.data, out.ctypes.data
    ok = Blend(0, 0, 2, 2, 0, 0, 0, 0, -1)
    for args in ((0, CH, c, a, f, FW, FH, ok, o), (CW, 0, c, a, f, FW, FH, ok, o), (CW, CH, c, a, f, 0, FH, ok, o), (CW, CH, c, a, f, FW, 0, ok, o),
                 (CW, CH, c, a, None, FW, FH, ok, o), (CW, CH, c, a, f, FW, FH, None, o), (CW, CH, c, a, f, FW, FH, ok, None),
                 (1 << 15, CH, c, a, f, FW, FH, ok, o), (CW, CH, c, a, f, FW, 1 << 15, ok, o),
                 (CW, CH, c, a, f, FW, FH, Blend(0, 0, 5, 0, 0, 0, 0, 0, -1), o), (CW, CH, c, a, f, FW, FH, Blend(0, 0, 0, 5, 0, 0, 0, 0, -1), o),
                 (CW, CH, c, a, f, FW, FH, Blend(1 << 21, 0, 0, 0, 0, 0, 0, 0, -1), o), (CW, CH, c, a, f, FW, FH, Blend(0, -(1 << 21), 0, 0, 0, 0, 0, 0, -1), o)):
        b = args[7]
        r = lib.jxlhip_debug_blend_rect(0, *args[:7], None if b is None else ctypes.byref(b), 1, 0, args[8])
        assert r == INVALID, args[:2] + args[5:7]
    assert (out == 7.0).all()  # (nothing ran)


# ---- k_patches_add
SLOT_SIZES = {1: (64, 48), 2: (300, 4)}  # slot -> (width, height)


def _record(x, y, w, h, rx, ry, slot, mode, clamp=0, ec_mode=0, ec_clamp=0):
    return [x, y, w, h, rx, ry, slot, mode | clamp << 8 | ec_mode << 16 | ec_clamp << 24]


@pytest.fixture(scope="module")
def patch_case():
    """Frame planes and alpha, the two slots, and the two dictionaries.
    "modes": 64 rectangles of 8 x 2 that do not touch, one per (colour mode, alpha mode) pair, clamps as in test_patches.py's
    _alpha_case; the slot samples under each are the ones the frame's samples were paired with.
    "places": positions that cross the first stride (x = 250), start in the second (x = 300), are clipped by xsize (x = 590,
    20 wide), one 280 wide from the wide slot, and three that overlap in dictionary order (add, multiply, then blend above;
    this dictionary is run with premultiplied alpha, whose blend divides by nothing, since what an overlap leaves in the
    alpha plane is no longer on the grid)."""
    bg, bga, fg, fga = B.crafted_layers(31, (PH, PW))
    assert B.blend_conditioning(bga, fga) >= 1 / 64
    rng = np.random.default_rng(32)
    slots = {}
    for s, (w, h) in SLOT_SIZES.items():
        slots[s] = (rng.uniform(-0.5, 1.5, (3, h, w)).astype(F32), rng.choice(B.ALPHA_VALUES, (h, w)).astype(F32))
    modes = []
    for k, (mode, ec_mode) in enumerate(itertools.product(range(8), range(8))):
        x, y, rx, ry = 3 + (k % 32) * 18, 1 + (k // 32) * 3, (k % 8) * 8, (k // 8) * 2
        slots[1][0][:, ry:ry + 2, rx:rx + 8] = fg[:, y:y + 2, x:x + 8]
        slots[1][1][ry:ry + 2, rx:rx + 8] = fga[y:y + 2, x:x + 8]
        modes.append(_record(x, y, 8, 2, rx, ry, 1, mode, (k >> 1) & 1, ec_mode, k & 1))
    places = [_record(250, 1, 20, 4, 40, 20, 1, 2, 0, 2, 0),      # add, crosses x = 256
              _record(300, 0, 30, 5, 30, 40, 1, 6, 1, 4, 1),      # alpha-weighted add above, starts in the second stride
              _record(590, 2, 20, 3, 10, 30, 1, 1, 0, 1, 0),      # replace; columns 600 .. 609 are not there
              _record(40, 2, 280, 4, 15, 0, 2, 7, 0, 5, 1),       # alpha-weighted add below, 280 wide (two trips of a thread)
              _record(255, 0, 64, 3, 0, 16, 1, 2, 0, 0, 0),       # three that overlap each other (and the first and the
              _record(260, 1, 50, 4, 8, 24, 1, 3, 1, 3, 0),       # fourth): add, then multiply, then blend above, which do
              _record(270, 2, 40, 2, 20, 10, 1, 4, 1, 2, 0),      # not commute
              _record(100, 5, 300, 1, 0, 3, 2, 5, 0, 6, 0),       # blend below, the wide slot's last row on the last row
              _record(0, 0, 1, 1, 63, 47, 1, 0, 0, 1, 0)]         # colour mode none, alpha replaced: the slot's last sample
    return np.concatenate([bg, bga[None]]), slots, dict(modes=modes, places=places)


def _rows_of(records, ysize):
    starts, entries = [0], []
    for y in range(ysize):
        entries += [i for i, q in enumerate(records) if q[1] <= y < q[1] + q[3]]
        starts.append(len(entries))
    return np.array(starts, np.uint32), np.array(entries if entries else [0], np.uint32), len(entries)


def _patches_struct(records, slots, with_alpha, premultiplied, keep):
    rec = np.array(records, np.uint32).reshape(-1, 8)
    row_start, row_list, n = _rows_of(records, PH)
    p = Patches()
    p.num_positions, p.num_row_entries = len(rec), n
    p.records, p.row_start, p.row_list = rec.ctypes.data, row_start.ctypes.data, row_list.ctypes.data
    for s, (planes, alpha) in slots.items():
        p.slot_planes[s], p.slot_w[s], p.slot_h[s] = planes.ctypes.data, planes.shape[2], planes.shape[1]
        if with_alpha:
            p.slot_alpha[s] = alpha.ctypes.data
    p.uses_alpha, p.premultiplied = int(with_alpha), int(premultiplied)
    keep += [rec, row_start, row_list]
    return p


def _patches_reading(frame, slots, records, with_alpha, premultiplied, band):
    """Every position in dictionary order on the rows of the band it covers (dec_patch_dictionary.cc:317-356: a row applies
    the positions that contain it, in order; samples of different rows do not meet)."""
    planes, alpha = frame[:3].copy(), frame[3].copy() if with_alpha else None
    for (x, y, w, h, rx, ry, slot, word) in records:
        mode, clamp, ec_mode, ec_clamp = word & 255, (word >> 8) & 1, (word >> 16) & 255, (word >> 24) & 1
        y0, y1, x1 = max(y, band[0]), min(y + h, band[1]), min(x + w, PW)
        if y0 >= y1 or x >= x1:
            continue
        dst = (slice(y0, y1), slice(x, x1))
        src = (slice(ry + y0 - y, ry + y1 - y), slice(rx, rx + x1 - x))
        sp, sa = slots[slot]
        col, a = B.perform_blending(planes[(slice(None),) + dst], alpha[dst] if with_alpha else None, sp[(slice(None),) + src],
                                    sa[src] if with_alpha else None, mode, clamp, ec_mode, ec_clamp, premultiplied)
        planes[(slice(None),) + dst] = col
        if with_alpha:
            alpha[dst] = a
    return planes, alpha


@pytest.mark.parametrize("which,with_alpha,premultiplied", [("modes", True, 0), ("modes", True, 1), ("modes", False, 0), ("places", True, 1),
                                                            ("places", False, 0)])
def test_patches_on_crafted_planes(lib, ctx, patch_case, which, with_alpha, premultiplied):
    frame, slots, dictionaries = patch_case
    records = dictionaries[which]
    for band in ((0, PH), (1, 5)):
        keep = []
        p = _patches_struct(records, slots, with_alpha, premultiplied, keep)
        planes_in, alpha_in = np.ascontiguousarray(frame[:3]), np.ascontiguousarray(frame[3])
        planes_out, alpha_out = np.full((3, PH, PW), 7.0, F32), np.full((PH, PW), 7.0, F32)
        r = lib.jxlhip_debug_patches(ctx._h, planes_in.ctypes.data, alpha_in.ctypes.data if with_alpha else None, PW, PH, ctypes.byref(p),
                                     band[0], band[1], planes_out.ctypes.data, alpha_out.ctypes.data if with_alpha else None)
        assert r == 0, r
        want, want_a = _patches_reading(frame, slots, records, with_alpha, premultiplied, band)
        assert np.array_equal(planes_out, want), (band, float(np.abs(planes_out - want).max()))
        if with_alpha:
            assert np.array_equal(alpha_out, want_a), (band, float(np.abs(alpha_out - want_a).max()))
        outside = [y for y in range(PH) if not band[0] <= y < band[1]]
        assert np.array_equal(planes_out[:, outside].view(np.uint32), frame[:3][:, outside].view(np.uint32))  # bit for bit
        assert not np.array_equal(want, frame[:3])


def test_patches_entry_refuses_bad_arguments(lib, ctx, patch_case):
    frame, slots, dictionaries = patch_case
    planes_in, alpha_in = np.ascontiguousarray(frame[:3]), np.ascontiguousarray(frame[3])
    planes_out, alpha_out = np.full((3, PH, PW), 7.0, F32), np.full((PH, PW), 7.0, F32)
    pi, ai, po, ao = planes_in.ctypes.data, alpha_in.ctypes.data, planes_out.ctypes.data, alpha_out.ctypes.data
    keep = []
    good = dictionaries["places"]

    def call(records=good, with_alpha=True, h=ctx._h, planes=pi, alpha=ai, xs=PW, ys=PH, band=(0, PH), out=po, aout=ao, edit=None):
        p = _patches_struct(records, slots, with_alpha, 1, keep)
        if callable(edit):
            edit(p)
        return lib.jxlhip_debug_patches(h, planes, alpha, xs, ys, None if edit == "null" else ctypes.byref(p), band[0], band[1], out, aout)

    def first_entry_names(n):
        def edit(p):
            ctypes.cast(p.row_list, ctypes.POINTER(ctypes.c_uint32))[0] = n
        return edit

    def no_positions(p):
        p.num_positions = 0

    def slot_gone(p):
        p.slot_planes[2] = None

    def slot_alpha_gone(p):
        p.slot_alpha[1] = None

    def slot_empty(p):
        p.slot_w[1] = 0

    assert call(h=None) == INVALID and call(planes=None) == INVALID and call(out=None) == INVALID and call(edit="null") == INVALID
    assert call(alpha=None) == INVALID and call(aout=None) == INVALID and call(with_alpha=False) == INVALID  # alpha planes and uses_alpha disagree
    assert call(xs=0) == INVALID and call(ys=0) == INVALID and call(xs=1 << 15) == INVALID
    assert call(band=(2, 2)) == INVALID and call(band=(3, 2)) == INVALID and call(band=(0, PH + 1)) == INVALID
    assert call(edit=no_positions) == INVALID and call(edit=slot_gone) == INVALID and call(edit=slot_alpha_gone) == INVALID
    assert call(edit=slot_empty) == INVALID
    assert call(records=good[:-1] + [_record(10, 0, 8, 2, 60, 0, 1, 1)]) == INVALID  # reaches past the slot's last column
    assert call(records=good[:-1] + [_record(10, 0, 8, 2, 0, 47, 1, 1)]) == INVALID   # ... its last row
    assert call(records=good[:-1] + [_record(10, 0, 8, 2, 0, 0, 3, 1)]) == INVALID    # a slot that is not there
    assert call(records=good[:-1] + [_record(10, 0, 8, 2, 0, 0, 1, 8)]) == INVALID    # no such mode
    assert call(records=good[:-1] + [_record(10, 5, 8, 2, 0, 0, 1, 1)]) == INVALID    # rows past the frame
    assert call(edit=first_entry_names(len(good))) == INVALID  # a row list that names a missing position
    assert call(edit=first_entry_names(0)) == INVALID          # ... or a position that does not cover the row (row 0: places[0] starts at 1)
    assert (planes_out == 7.0).all() and (alpha_out == 7.0).all()  # (nothing ran)
    assert call() == 0 and not (planes_out == 7.0).any()
