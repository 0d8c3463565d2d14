"""The oracle's blending held to tests/blending_np.py (the reading and its bars are described there), without a GPU:
  * ApplyPatches (oracle/jxlo_patches.h) through its one-sample hook on crafted floats: every PatchBlendMode of the colour
    channels x every one of the alpha channel x both clamps x premultiplied or straight alpha, and the eight colour modes on
    an image without alpha. Crafted floats reach what no stream can: alphas outside [0, 1], so that the clamps show;
  * the canvas loop of oracle/jxlo_decoder.cc through lossless layer stacks (whose samples, n / 255, the clamps leave
    alone: the clamps of the frame stage are held on the kernel, tests/test_gpu_blending.py);
  * every misreading of the reading shows on these cases."""
import ctypes
import itertools

import numpy as np
import pytest

import blending_np as B

F32 = np.float32
W, H = 96, 64


def _kat(built):
    import jxlo
    L = jxlo.lib()
    fp = ctypes.POINTER(ctypes.c_float)
    L.jxlo_patch_blend_kat.argtypes = [fp, ctypes.c_float, fp, ctypes.c_float] + [ctypes.c_int] * 6 + [fp]
    L.jxlo_patch_blend_kat.restype = None
    return L.jxlo_patch_blend_kat


@pytest.fixture(scope="module")
def samples():
    """One row of crafted samples: the six special alpha pairs and 26 drawn ones."""
    bg, bga, fg, fga = B.crafted_layers(11, (1, 32))
    assert B.blend_conditioning(bga, fga) >= 1 / 64 and ((bga == 0) & (fga == 0)).any()
    assert (bga > 1).any() and (bga < 0).any() and (fga > 1).any() and (fga < 0).any()
    return bg, bga, fg, fga


def test_oracle_patch_blending_is_the_reading_sample_for_sample(built, samples):
    kat = _kat(built)
    bg, bga, fg, fga = samples
    n = bga.shape[1]
    out = (ctypes.c_float * 4)()
    c3 = ctypes.c_float * 3
    cols = [(c3(*bg[:, 0, i]), float(bga[0, i]), c3(*fg[:, 0, i]), float(fga[0, i])) for i in range(n)]
    for mode, ec_mode, clamp, ec_clamp, premultiplied in itertools.product(range(8), range(8), (0, 1), (0, 1), (0, 1)):
        want, want_a = B.perform_blending(bg, bga, fg, fga, mode, clamp, ec_mode, ec_clamp, premultiplied)
        got = np.zeros((4, n), F32)
        for i, (b, ba, f, fa) in enumerate(cols):
            kat(b, ba, f, fa, mode, clamp, ec_mode, ec_clamp, premultiplied, 1, out)
            got[:, i] = out[:]
        assert np.array_equal(got[:3], want[:, 0]) and np.array_equal(got[3], want_a[0]), (mode, ec_mode, clamp, ec_clamp, premultiplied)
    for mode, clamp in itertools.product(range(8), (0, 1)):  # an image without alpha: blending.cc:150-184
        want, none = B.perform_blending(bg, None, fg, None, mode, clamp)
        assert none is None
        got = np.zeros((3, n), F32)
        for i, (b, ba, f, fa) in enumerate(cols):
            kat(b, ba, f, fa, mode, clamp, 0, 0, 0, 0, out)
            got[:, i] = out[:3]
        assert np.array_equal(got, want[:, 0]), (mode, clamp)


def test_float32_form_rounds_the_float64_form(samples):
    """The same text in float64 is the exact form: the float32 form stays within a few roundings of it, relative to the
    largest intermediate (|top| + |bottom|) / new_a <= 3 * 64."""
    bg, bga, fg, fga = samples
    for mode, ec_mode, clamp, premultiplied in itertools.product(range(8), range(8), (0, 1), (0, 1)):
        a32 = B.perform_blending(bg, bga, fg, fga, mode, clamp, ec_mode, clamp, premultiplied)
        a64 = B.perform_blending(bg, bga, fg, fga, mode, clamp, ec_mode, clamp, premultiplied, dtype=np.float64)
        for x, y in zip(a32, a64):
            assert x.dtype == F32 and y.dtype == np.float64 and np.abs(x - y).max() <= 8 * 2.0 ** -24 * 192


def _layer_img(J, w, h, seed, with_alpha, alpha_kind):
    rgb = J.synth_image(w, h, seed=seed)
    if not with_alpha:
        return rgb
    yy, xx = np.mgrid[0:h, 0:w]
    # alphas in steps of 4 / 255 (a blend's new alpha is then 0 or at least 1 / 64), with whole regions of 0 and of 255
    a = {0: (xx * 5 + yy * 3) & 252, 1: np.where((xx // 8 + yy // 8) % 3 == 0, 0, np.where((xx // 8 + yy // 8) % 3 == 1, 255, (xx * 7) & 252)),
         2: np.full((h, w), 255)}[alpha_kind]
    return np.dstack([rgb, a.astype(np.uint8)])


def _stacks(J):
    """name -> (layers with alpha?, premultiplied, list of layers for encode_layers)."""
    out = {}
    for premultiplied in (False, True):
        # every colour mode x every alpha mode, each over what the one before left in slot 1; clamp on every other one
        layers = [dict(img=_layer_img(J, W, H, 1, True, 0), save_as=1)]
        for k, (mode, alpha_mode) in enumerate(itertools.product(range(5), range(5))):
            layers.append(dict(img=_layer_img(J, 40, 24, 20 + k, True, k % 2), x0=(k * 13) % 70 - 8, y0=(k * 7) % 50 - 6, mode=mode,
                               alpha_mode=alpha_mode, source=1, clamp=k & 1, save_as=1))
        out["modes_premultiplied" if premultiplied else "modes_straight"] = (True, premultiplied, layers)
    # rectangles that stick out on each side and one wholly outside; a slot never written as the colour and as the alpha
    # background; colour and alpha backgrounds from different slots
    base = dict(img=_layer_img(J, W, H, 2, True, 0), save_as=1)
    other = dict(img=_layer_img(J, W, H, 3, True, 1), save_as=2, mode=0, alpha_mode=0)
    small = lambda k, kind=0: _layer_img(J, 40, 24, 50 + k, True, kind)
    out["placement"] = (True, False, [
        base, other,
        dict(img=small(0), x0=-30, y0=5, mode=2, alpha_mode=2, source=1, alpha_source=2, save_as=1),
        dict(img=small(1), x0=W - 10, y0=20, mode=2, alpha_mode=1, source=1, alpha_source=1, save_as=1),
        dict(img=small(2), x0=20, y0=-20, mode=3, alpha_mode=2, source=1, alpha_source=2, save_as=1),
        dict(img=small(3), x0=30, y0=H - 4, mode=2, alpha_mode=4, source=2, alpha_source=1, save_as=2),
        dict(img=small(4), x0=W + 3, y0=0, mode=0, alpha_mode=0, source=2, alpha_source=1, save_as=2),
        dict(img=small(5), x0=-40, y0=0, mode=1, alpha_mode=1, source=2, alpha_source=2, save_as=2),
        dict(img=small(6, 1), x0=10, y0=10, mode=2, alpha_mode=2, source=3, alpha_source=1, save_as=3),  # slot 3: never written
        dict(img=small(7), x0=50, y0=30, mode=1, alpha_mode=2, source=1, alpha_source=0, save_as=1),     # slot 0 likewise
        dict(img=small(8, 1), x0=5, y0=35, mode=2, alpha_mode=3, source=3, alpha_source=2)])
    # an image without alpha: modes 0..4, blend replaces and alpha-weighted add adds
    layers = [dict(img=_layer_img(J, W, H, 4, False, 0), save_as=1)]
    for mode in range(5):
        layers.append(dict(img=_layer_img(J, 40, 24, 70 + mode, False, 0), x0=mode * 17 - 10, y0=mode * 9 - 5, mode=mode, source=1, save_as=1))
    layers.append(dict(img=_layer_img(J, 40, 24, 80, False, 0), x0=60, y0=45, mode=2, source=2))  # slot 2: never written
    out["no_alpha"] = (False, False, layers)
    return out


@pytest.fixture(scope="module")
def decoded_stacks(built):
    """name -> (has_alpha, premultiplied, the reading's layers, the oracle's final canvas [4 or 3][H][W])."""
    import jxlo
    J = built
    out = {}
    for name, (has_alpha, premultiplied, layers) in _stacks(J).items():
        data = J.encode_layers(layers, lossless=True, premultiplied=premultiplied)
        o = jxlo.Decoded(data)
        got = o.planes("rgbf").copy()
        if has_alpha:
            got = np.concatenate([got, o.buffer("alphaf").reshape(1, H, W)])
        o.close()
        mine = []
        for L in layers:  # every layer as the oracle decodes it as a still of its own
            o = jxlo.Decoded(J.encode_lossless(L["img"]))
            h, w = L["img"].shape[:2]
            f = np.zeros((4, h, w), F32)
            f[:3] = o.planes("rgbf")[:, :h, :w]
            if has_alpha:
                f[3] = o.buffer("alphaf").reshape(h, w)
            o.close()
            mine.append(dict(L, frame=f))
        out[name] = (has_alpha, premultiplied, mine, got)
    return out


@pytest.mark.parametrize("name", ["modes_straight", "modes_premultiplied", "placement", "no_alpha"])
def test_oracle_canvas_is_the_frame_stage_reading(decoded_stacks, name):
    has_alpha, premultiplied, layers, got = decoded_stacks[name]
    want = B.compose(W, H, layers, has_alpha, premultiplied)[-1]
    nc = 4 if has_alpha else 3
    assert got.shape == (nc, H, W)
    assert np.array_equal(got, want[:nc]), np.abs(got - want[:nc]).max()
    assert np.abs(want[:3] - layers[0]["frame"][:3]).max() > 0.2  # (the layers are there)


def _differs(a, b):
    with np.errstate(invalid="ignore"):
        return bool((~(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) <= 1e-3)).any())  # (a NaN differs)


def test_every_misreading_shows(samples, decoded_stacks):
    """Each named misreading moves some sample of the cases above by more than 1e-3, while the reading as written is what the
    oracle computes on them (the tests above)."""
    bg, bga, fg, fga = samples
    shown = {}
    for m in B.PATCH_MISREADINGS:
        for mode, ec_mode, clamp, premultiplied, alpha in itertools.product(range(8), range(8), (0, 1), (0, 1), (True, False)):
            args = (bg, bga if alpha else None, fg, fga if alpha else None, mode, clamp, ec_mode, clamp, premultiplied)
            right, wrong = B.perform_blending(*args), B.perform_blending(*args, misread=m)
            if _differs(right[0], wrong[0]) or (alpha and _differs(right[1], wrong[1])):
                shown.setdefault(m, []).append((mode, ec_mode, clamp, premultiplied, alpha))
    for m in B.FRAME_MISREADINGS:
        for name in ("placement", "no_alpha"):
            has_alpha, premultiplied, layers, got = decoded_stacks[name]
            nc = 4 if has_alpha else 3
            if _differs(B.compose(W, H, layers, has_alpha, premultiplied, misread=m)[-1][:nc], got):
                shown.setdefault(m, []).append(name)
    for m in B.MISREADINGS:
        print(m, "shows on", len(shown.get(m, [])), "cases, first", shown.get(m, [None])[0])
    assert set(shown) == set(B.MISREADINGS), set(B.MISREADINGS) - set(shown)
    # and where they must: the fall-backs only without alpha, the zero guard only for straight alpha
    assert all(not c[4] for c in shown["no_alpha_blend_adds"] + shown["no_alpha_blend_below_keeps_background"])
    assert all(c[0] in (4, 5) and not c[3] and c[4] for c in shown["no_zero_guard"])
    assert "placement" in shown["alpha_background_from_colour_slot"] and "placement" in shown["outside_shows_zeros"]
