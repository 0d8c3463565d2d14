"""Lossless streams whose GROUP headers carry transforms (palette, RCT, Squeeze), as the reference encoder writes them at
its default effort, made by the repository's stream writer; shared by the CPU and the GPU tests of that path. Every case is
(name, image, stream bytes, expected launch levels or None); lossless, so the image is what every decoder must return."""
import numpy as np


def lossless_image(J, w, h, channels, seed):
    """The synthetic image with `channels` channels (grey, grey + alpha, RGB, RGBA; the alpha is a ramp pattern)."""
    rgb = J.synth_image(w, h, seed=seed)
    y, x = np.mgrid[0:h, 0:w]
    alpha = ((x * 3 + y * 5) % 256).astype(np.uint8)
    if channels == 1:
        return np.ascontiguousarray(rgb[..., 1:2])
    if channels == 2:
        return np.ascontiguousarray(np.dstack([rgb[..., 1], alpha]))
    return np.ascontiguousarray(rgb if channels == 3 else np.dstack([rgb, alpha]))


def mixed_image(w, h, channels, seed, colors=12):
    """Noise, except: the first 256 x 256 group holds `colors` colours in all channels (an all-channel palette fits), the
    group right of it few values in its first channel only (a single-channel palette fits), and, when the image is three
    groups wide, a third group few values in every channel but many combinations."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    table = rng.integers(0, 256, (colors, channels), dtype=np.uint8)
    a = img[:256, :256]
    a[...] = table[rng.integers(0, colors, a.shape[:2])]
    if w > 256:
        b = img[:256, 256:512, 0]
        b[...] = (rng.integers(0, 7, b.shape) * 30).astype(np.uint8)
    if w > 512:
        c = img[:256, 512:768]
        c[...] = (rng.integers(0, 9, c.shape) * 25).astype(np.uint8)
    return img


def cases(J, big=True):
    R, P, S, G = J.LOSSLESS_LOCAL_RCT, J.LOSSLESS_LOCAL_PALETTE, J.LOSSLESS_LOCAL_SQUEEZE, J.LOSSLESS_SQUEEZE
    spec = [
        # name, flags, seed, (w, h, channels), launch levels
        ("rct_4_groups", R, 0, (300, 280, 3), 1),
        ("rct_types_by_seed_ragged", R, 5, (700, 300, 3), 1),
        ("palette_some_groups", P, 0, (700, 300, 3), 1),           # one all-channel palette, single-channel ones: independent
        ("palettes_then_rct", P | R, 0, (700, 300, 3), 2),        # RCT over index channels, then the palettes
        ("squeeze", S, 0, (700, 300, 3), None),
        ("global_squeeze_local_squeeze", G | S, 0, (700, 300, 3), None),
        ("grey_palette_squeeze", P | S, 0, (700, 300, 1), None),
        ("rgba_everything", P | R | S | J.LOSSLESS_WP, 3, (700, 300, 4), None),
        ("grey_alpha_palette", P, 0, (520, 300, 2), 1),
    ]
    if big:  # more than one DC group; with the global Squeeze the DC-group streams carry channels and transforms of their own
        spec.append(("two_dc_groups_global_squeeze_everything", G | P | R | S, 0, (2300, 2100, 3), None))
    out = []
    for name, flags, seed, (w, h, c), levels in spec:
        img = mixed_image(w, h, c, seed=len(name) + w)
        out.append((name, img, J.encode_lossless(img, flags, seed, palette_colors=64), levels))
    return out


def implicit_image(bits, w=300, h=280, seed=1):
    """An image of nothing but implicit palette colours (tests/palette_np.py, nb_colors = 1) -- of the negative-index ones
    only those an unsigned `bits`-bit image can hold -- plus, once per group, one colour that is none of them."""
    import palette_np
    _, colors = palette_np.implicit_colors(1, bits)
    ok = ((colors >= 0) & (colors < (1 << bits))).all(axis=1)
    colors = colors[ok]
    rng = np.random.default_rng(seed)
    img = colors[rng.integers(0, len(colors), (h, w))]
    img[np.arange(h)[:, None] * w + np.arange(w)[None, :] < len(colors)] = colors  # every one of them occurs, in order
    lone = np.array([3, 5, 7]) * (1 << (bits - 8))
    assert not (colors == lone).all(axis=1).any()
    img[h // 2, w // 2] = lone
    img[h - 1, w - 1] = lone
    return img.astype(np.int32), int(ok.sum())
