"""A reading of the blending arithmetic, for patches and for frames composed on a canvas. Written from the reference's text
and from nothing under libjxl_amd/csrc or oracle/:
  * lib/jxl/alpha.cc:18-41 (PerformAlphaBlending of four planes: the premultiplied form, and the straight form with
    rnew_a = new_a > 0 ? 1 / new_a : 0), :42-65 (the same for one channel, with the form taken when the channel is its own
    alpha: bg == bga && fg == fga), :67-80 (PerformAlphaWeightedAdd; fg == fga copies the background), :82-93
    (PerformMulBlending: the clamp is on the top layer);
  * lib/jxl/blending.cc:57-112 (the extra channels first, from the values before blending), :114-148 (the colour helpers;
    blend_weighted writes the alpha channel too, after and over what the channel's own mode gave), :150-184 (the colour
    modes, and what each falls back to on an image without alpha: alpha-weighted add adds, and both blends, kBlendBelow
    as well, copy the foreground), :186-188 (all channels are stored at the end: nothing reads a blended value);
  * lib/jxl/dec_patch_dictionary.h:32-58 (PatchBlendMode 0 none, 1 replace, 2 add, 3 multiply, 4 / 5 blend above / below,
    6 / 7 alpha-weighted add above / below);
  * lib/jxl/render_pipeline/stage_blending.cc:100-125 (BlendMode 0 replace, 1 add, 2 blend, 3 alpha-weighted add, 4 multiply
    -> PatchBlendMode replace, add, blend above, alpha-weighted add above, multiply), :140-158 (the frame's rows against the
    canvas: rows and columns outside the image are dropped), :159-179 (the colour background from blending_info.source, the
    alpha background from extra_channel_blending_info[0].source, a row of zeros for a slot never written), :180-183 (the
    background is `bg`, the frame `fg`), :199-225 (outside the frame's rectangle the backgrounds show, each channel from its
    own slot).
Scope: images whose one extra channel, if any, is alpha. Both the oracle (oracle/jxlo_patches.h ApplyPatches, the canvas loop
of oracle/jxlo_decoder.cc) and the HIP kernels (k_patches_add, k_canvas_blend) are held to it: tests/test_blending_np.py,
tests/test_gpu_blending.py.

Formulation, on purpose unlike the kernels' per-sample switch: the three primitives of alpha.cc are array functions of
(bottom, top) layers, a table maps every mode to a primitive and to which of (background, foreground) is the bottom layer,
and the frame stage is slicing: the intersection of the frame's rectangle with the canvas is blended, the canvas starts as
a copy of the backgrounds.

Bars. Every operation here is one IEEE binary32 operation (NumPy does not contract a * b + c), in the reference's order;
the kernels are compiled with contraction off and no fast-math flag, their division is correctly rounded and they keep
denormals. So the bar is equality of every sample with dtype=float32 (np.array_equal: the sign of a zero is not compared,
since Clamp1, np.clip and a median-of-three may each return either zero for a zero of the other sign). No test's inputs
hold a NaN, and the alphas are chosen so that a straight-alpha blend never divides by less than 1 / 64: new_a is exactly 0
or at least that (k / 64 grids; -0.25 and 1.5 are only paired with values that keep it so: see test_gpu_blending.py).
With dtype=float64 the same text is the exact form; it is used only to show that the float32 form is a rounding of it.

Misreadings: each switch below is one plausible wrong reading; tests/test_blending_np.py shows that each changes some
sample of the listed cases by more than 1e-3 (the bar being 0, "ten times the bar" is any difference; 1e-3 keeps roundoff
out of the argument)."""
import numpy as np

PATCH_MISREADINGS = ("above_below_swapped", "clamp_on_bottom_alpha", "colour_sees_blended_alpha", "premultiplied_swapped",
                     "no_zero_guard", "weighted_add_adds_alpha", "multiply_clamps_background", "no_alpha_blend_adds",
                     "no_alpha_blend_below_keeps_background")
FRAME_MISREADINGS = ("outside_shows_zeros", "alpha_background_from_colour_slot")
MISREADINGS = PATCH_MISREADINGS + FRAME_MISREADINGS

NONE, REPLACE, ADD, MUL, BLEND_ABOVE, BLEND_BELOW, WEIGHTED_ADD_ABOVE, WEIGHTED_ADD_BELOW = range(8)
FRAME_TO_PATCH_MODE = {0: REPLACE, 1: ADD, 2: BLEND_ABOVE, 3: WEIGHTED_ADD_ABOVE, 4: MUL}


def _clamp(v, on):
    return np.clip(v, v.dtype.type(0), v.dtype.type(1)) if on else v


def _alpha_blend(bottom, bottom_a, top, top_a, premultiplied, clamp, misread):
    """alpha.cc:18-41. Returns (colour, new alpha)."""
    one = top_a.dtype.type(1)
    if misread == "clamp_on_bottom_alpha":
        bottom_a = _clamp(bottom_a, clamp)
        ta = top_a
    else:
        ta = _clamp(top_a, clamp)
    new_a = one - (one - ta) * (one - bottom_a)
    if premultiplied != (misread == "premultiplied_swapped"):
        return top + bottom * (one - ta), new_a
    with np.errstate(divide="ignore", invalid="ignore"):
        if misread == "no_zero_guard":
            r = one / new_a
        else:
            r = np.where(new_a > 0, one / new_a, one * 0).astype(new_a.dtype)
        return (top * ta + bottom * bottom_a * (one - ta)) * r, new_a


def _weighted_add(bottom, top, top_a, clamp):
    """alpha.cc:67-80, for a channel that is not its own alpha."""
    return bottom + top * _clamp(top_a, clamp)


def _mul(bottom, top, clamp, misread):
    """alpha.cc:82-93."""
    if misread == "multiply_clamps_background":
        return _clamp(bottom, clamp) * top
    return bottom * _clamp(top, clamp)


def perform_blending(bg, bga, fg, fga, mode, clamp, ec_mode=NONE, ec_clamp=0, premultiplied=False, dtype=np.float32, misread=None):
    """blending.cc:42-190 for an image whose one extra channel, if any, is alpha. bg / fg: [3][h][w] colour of the background
    (what is there) and the foreground (what is drawn); bga / fga: [h][w] their alpha, or both None for an image without
    alpha (ec_mode is then not used). mode / ec_mode: PatchBlendMode of the colour channels / of the alpha channel.
    Returns (colour, alpha or None); nothing is modified in place."""
    assert misread is None or misread in MISREADINGS
    bg, fg = np.asarray(bg, dtype), np.asarray(fg, dtype)
    has_alpha = bga is not None
    assert has_alpha == (fga is not None)
    if misread == "above_below_swapped":
        swap = {BLEND_ABOVE: BLEND_BELOW, BLEND_BELOW: BLEND_ABOVE, WEIGHTED_ADD_ABOVE: WEIGHTED_ADD_BELOW, WEIGHTED_ADD_BELOW: WEIGHTED_ADD_ABOVE}
        mode, ec_mode = swap.get(mode, mode), swap.get(ec_mode, ec_mode)
    a = None
    if has_alpha:
        bga, fga = np.asarray(bga, dtype), np.asarray(fga, dtype)
        one = dtype(1)
        # the alpha channel by its own mode; it is its own alpha: alpha.cc:45-49 and :69-70
        if ec_mode == NONE:
            a = bga
        elif ec_mode == REPLACE:
            a = fga
        elif ec_mode == ADD:
            a = bga + fga
        elif ec_mode == MUL:
            a = _mul(bga, fga, ec_clamp, misread)
        elif ec_mode in (BLEND_ABOVE, BLEND_BELOW):
            bot, top = (bga, fga) if ec_mode == BLEND_ABOVE else (fga, bga)
            if misread == "clamp_on_bottom_alpha":
                bot, top = _clamp(bot, ec_clamp), top
            else:
                top = _clamp(top, ec_clamp)
            a = one - (one - top) * (one - bot)
        else:  # alpha-weighted add of a channel with itself as alpha: the bottom layer, unchanged
            bot, top = (bga, fga) if ec_mode == WEIGHTED_ADD_ABOVE else (fga, bga)
            a = bot + top * _clamp(top, ec_clamp) if misread == "weighted_add_adds_alpha" else bot
        if misread == "colour_sees_blended_alpha":  # (the background's alpha as the colour channels see it)
            bga = a
    if mode == NONE:
        out = bg
    elif mode == REPLACE:
        out = fg
    elif mode == ADD:
        out = bg + fg
    elif mode == MUL:
        out = _mul(bg, fg, clamp, misread)
    elif mode in (BLEND_ABOVE, BLEND_BELOW):
        if has_alpha:
            bot, bot_a, top, top_a = (bg, bga, fg, fga) if mode == BLEND_ABOVE else (fg, fga, bg, bga)
            out, a = _alpha_blend(bot, bot_a, top, top_a, premultiplied, clamp, misread)
        elif misread == "no_alpha_blend_adds":
            out = bg + fg
        elif misread == "no_alpha_blend_below_keeps_background" and mode == BLEND_BELOW:
            out = bg
        else:
            out = fg
    else:
        if has_alpha:
            bot, top, top_a = (bg, fg, fga) if mode == WEIGHTED_ADD_ABOVE else (fg, bg, bga)
            out = _weighted_add(bot, top, top_a, clamp)
        else:
            out = bg + fg
    return np.array(out, dtype), (None if a is None else np.array(a, dtype))


def blend_frame(xsize, ysize, bg_color, bg_alpha, frame, x0, y0, mode, alpha_mode, clamp, alpha_clamp, has_alpha, premultiplied,
                dtype=np.float32, misread=None):
    """stage_blending.cc:100-225: one frame onto a canvas of xsize x ysize. bg_color / bg_alpha: the slots the colour and the
    alpha backgrounds come from, each [4][ysize][xsize] (R, G, B, alpha) or None for a slot never written; frame: [4][fh][fw]
    (plane 3 is not read without alpha) with its top-left sample at (x0, y0) of the canvas; mode / alpha_mode: BlendMode.
    Returns [4][ysize][xsize]; without alpha plane 3 is the alpha background (no channel of the image: not to be compared)."""
    assert misread is None or misread in MISREADINGS
    frame = np.asarray(frame, dtype)
    fh, fw = frame.shape[1:]
    canvas = np.zeros((4, ysize, xsize), dtype)
    if bg_color is not None:
        canvas[:3] = np.asarray(bg_color, dtype)[:3]
    alpha_slot = bg_color if misread == "alpha_background_from_colour_slot" else bg_alpha
    if alpha_slot is not None:
        canvas[3] = np.asarray(alpha_slot, dtype)[3]
    # the part of the frame that lies on the canvas (:144-158), as slices of both
    cx0, cx1, cy0, cy1 = max(x0, 0), min(x0 + fw, xsize), max(y0, 0), min(y0 + fh, ysize)
    out = np.zeros_like(canvas) if misread == "outside_shows_zeros" else canvas.copy()
    if cx0 >= cx1 or cy0 >= cy1:
        return out
    on_canvas = (slice(None), slice(cy0, cy1), slice(cx0, cx1))
    of_frame = (slice(None), slice(cy0 - y0, cy1 - y0), slice(cx0 - x0, cx1 - x0))
    bg, fg = canvas[on_canvas], frame[of_frame]
    col, a = perform_blending(bg[:3], bg[3] if has_alpha else None, fg[:3], fg[3] if has_alpha else None, FRAME_TO_PATCH_MODE[mode], clamp,
                              FRAME_TO_PATCH_MODE[alpha_mode], alpha_clamp, premultiplied, dtype, misread)
    out[on_canvas][:3] = col
    if has_alpha:
        out[on_canvas][3] = a
    else:
        out[on_canvas][3] = canvas[on_canvas][3]
    return out


def compose(xsize, ysize, layers, has_alpha, premultiplied, dtype=np.float32, misread=None):
    """A codestream's frames in order (frame_header.h:373-379 CanBeReferenced; dec_cache.cc:268-290: what is shown is the
    canvas). layers: dicts with frame ([4][h][w]) and optionally x0, y0, mode, alpha_mode, source, alpha_source, clamp,
    alpha_clamp, save_as, duration; the last one is the last frame. Returns the canvas after every layer."""
    slots = [None] * 4
    shown = []
    for k, L in enumerate(layers):
        src = L.get("source", 0)
        canvas = blend_frame(xsize, ysize, slots[src], slots[L.get("alpha_source", src)], L["frame"], L.get("x0", 0), L.get("y0", 0),
                             L.get("mode", 0), L.get("alpha_mode", 0), L.get("clamp", 0), L.get("alpha_clamp", L.get("clamp", 0)), has_alpha,
                             premultiplied, dtype, misread)
        last = k == len(layers) - 1
        if not last and (L.get("duration", 0) == 0 or L.get("save_as", 0) != 0):
            slots[L.get("save_as", 0)] = canvas
        shown.append(canvas)
    return shown


# ---- inputs shared by the CPU and the GPU tests
ALPHA_VALUES = np.concatenate([np.arange(65) / 64.0, [-0.25, 1.5]])


def _new_alphas(top, bottom):
    """The new alpha of a blend with `top` over `bottom`, with and without the clamp, in float64."""
    return [1.0 - (1.0 - t) * (1.0 - bottom) for t in (top, np.clip(top, 0.0, 1.0))]


def crafted_layers(seed, shape_bg, shape_fg=None):
    """(bg colour [3][h][w], bg alpha [h][w], fg colour, fg alpha) as float32: colours uniform in [-0.5, 1.5], alphas from
    the grid k / 64 and the values -0.25 and 1.5 (so that a clamp shows). Where both layers have the same shape the alphas
    are paired sample by sample so that the new alpha of a blend above or below, clamped or not, is exactly 0 or at least
    1 / 64 (a pair that is neither is drawn again from the grid alone, where it cannot happen: with alphas 1 - m / 64 and
    1 - n / 64 the new alpha is 1 - m n / 4096, exact, zero only for m = n = 64); the first row starts with the pairs
    (0, 0), (0, 1), (1, 0), (1.5, -0.25), (-0.25, 1), (1.5, 1.5)."""
    rng = np.random.default_rng(seed)
    shape_fg = shape_fg or shape_bg
    bg = rng.uniform(-0.5, 1.5, (3,) + tuple(shape_bg)).astype(np.float32)
    fg = rng.uniform(-0.5, 1.5, (3,) + tuple(shape_fg)).astype(np.float32)
    bga = rng.choice(ALPHA_VALUES, shape_bg)
    fga = rng.choice(ALPHA_VALUES, shape_fg)
    if tuple(shape_fg) == tuple(shape_bg):
        first = [(0, 0), (0, 1), (1, 0), (1.5, -0.25), (-0.25, 1), (1.5, 1.5)]
        if bga.shape[1] >= len(first):
            for i, (b, f) in enumerate(first):
                bga[0, i], fga[0, i] = b, f
        bad = np.zeros(bga.shape, bool)
        for t, b in ((fga, bga), (bga, fga)):
            for na in _new_alphas(t, b):
                bad |= (na != 0) & (na < 1 / 64)
        bga[bad] = rng.integers(0, 65, int(bad.sum())) / 64.0
        fga[bad] = rng.integers(0, 65, int(bad.sum())) / 64.0
    return bg, bga.astype(np.float32), fg, fga.astype(np.float32)


def blend_conditioning(bga, fga):
    """The smallest new alpha any blend of these two alpha planes divides by (both orders, clamp on and off; a new alpha that
    is not above 0 takes the guard and divides nothing)."""
    vals = np.concatenate([np.ravel(na) for t, b in ((fga, bga), (bga, fga)) for na in _new_alphas(np.float64(t), np.float64(b))])
    return float(vals[vals > 0].min())
