"""The implicit colours of a Modular palette, restated in NumPy from the format's definition (reference
lib/jxl/modular/transform/palette.h:25-140, GetPaletteValue). Independent of the product (libjxl_amd/csrc) and of the
oracle: nothing here is shared with either, the delta table included, so a wrong table in one of them shows as a
difference. An index of a palette with `nb_colors` explicit entries means:
  index < 0                       a delta-table entry, sign by the parity of -(index + 1), scaled by 2^(bits - 8) above 8 bits;
  nb_colors .. nb_colors + 63     the 4x4x4 cube: two bits per channel, value * (2^bits - 1) >> 2 plus 2^max(0, bits - 3);
  nb_colors + 64 ..               the 5x5x5 cube: base-5 digits per channel, digit * (2^bits - 1) >> 2."""
import numpy as np

DELTAS = np.array([
    (0, 0, 0), (4, 4, 4), (11, 0, 0), (0, 0, -13), (0, -12, 0), (-10, -10, -10), (-18, -18, -18), (-27, -27, -27), (-18, -18, 0),
    (0, 0, -32), (-32, 0, 0), (-37, -37, -37), (0, -32, -32), (24, 24, 45), (50, 50, 50), (-45, -24, -24), (-24, -45, -45),
    (0, -24, -24), (-34, -34, 0), (-24, 0, -24), (-45, -45, -24), (64, 64, 64), (-32, 0, -32), (0, -32, 0), (-32, 0, 32),
    (-24, -45, -24), (45, 24, 45), (24, -24, -45), (-45, -24, 24), (80, 80, 80), (64, 0, 0), (0, 0, -64), (0, -64, -64),
    (-24, -24, 45), (96, 96, 96), (64, 64, 0), (45, -24, -24), (34, -34, 0), (112, 112, 112), (24, -45, -45), (45, 45, -24),
    (0, -32, 32), (24, -24, 45), (0, 96, 96), (45, -24, 24), (24, -45, -24), (-24, -45, 24), (0, -64, 0), (96, 0, 0),
    (128, 128, 128), (64, 0, 64), (144, 144, 144), (96, 96, 0), (-36, -36, 36), (45, -24, -45), (45, -45, -24), (0, 0, -96),
    (0, 128, 128), (0, 96, 0), (45, 24, -45), (-128, 0, 0), (24, -45, 24), (-45, 24, -45), (64, 0, -64), (64, -64, -64),
    (96, 0, 96), (45, -45, 24), (24, 45, -45), (64, 64, -64), (128, 128, 0), (0, 0, -128), (-24, 45, -45)], np.int64)
assert DELTAS.shape == (72, 3)


def implicit_color(index, nb_colors, bits):
    """The three colour components of `index` (not an explicit entry: index < 0 or index >= nb_colors)."""
    top = (1 << bits) - 1
    if index < 0:
        k = (-(index + 1)) % (2 * 71 + 1)
        v = DELTAS[(k + 1) >> 1] * (1 if k & 1 else -1)
        return v * (1 << (bits - 8)) if bits > 8 else v.copy()
    assert index >= nb_colors
    k = index - nb_colors
    if k < 64:
        return np.array([(((k >> (2 * c)) % 4) * top >> 2) + (1 << max(0, bits - 3)) for c in range(3)], np.int64)
    k -= 64
    return np.array([((k // 5 ** c) % 5) * top >> 2 for c in range(3)], np.int64)


def implicit_colors(nb_colors, bits):
    """(index, colour) of the indices nb_colors .. nb_colors + 188 and -1 .. -143."""
    idx = list(range(nb_colors, nb_colors + 189)) + list(range(-1, -144, -1))
    return idx, np.stack([implicit_color(i, nb_colors, bits) for i in idx])
