"""The cases of the Modular reading (tests/modular_np.py), defined once for tests/test_modular_np.py (both CPU front-ends)
and tests/test_gpu_modular_np.py (the kernels). A case is one Modular sub-bitstream: the channel list a decoder is handed,
the transforms and the tree the stream carries, the bytes the reading's writer made, and what the reading says the
channels hold before the transforms are undone (`pre`) and after (`final`). Sample content is a gradient plus bounded
noise from a fixed seed, so every leaf and every sub-predictor has work to do. Building a case runs the Python model over
it, which is the costly part: build() keeps every case it has made."""
import random

import modular_np as M
from modular_np import Chan

_BUILT = {}


def content(w, h, seed, amp=40, gx=3, gy=-2, base=100, hshift=0, vshift=0):
    r = random.Random(seed)
    return Chan(w, h, hshift, vshift, [[base + gx * x + gy * y + r.randint(-amp, amp) for x in range(w)] for y in range(h)])


class Case:
    """name; shapes, nb_meta: the channel list before the stream's transforms; transforms as written and `filled` (a default
    squeeze list spelled out by the case's builder; meta_apply must arrive at the same); tree; wp (None = the default
    header) and wp_values; stream_id; bit_depth; tokens; stream (modular_np.write_stream); pre, pre_nb_meta; final;
    gpu: False where the device path refuses the stream at parse."""

    def __init__(self, name, coded, nb_meta, transforms, nested, wp=None, stream_id=0, bit_depth=8, per_leaf=False, gpu=True,
                 image=None, quantize=False, filled=None):
        self.name, self.wp, self.stream_id, self.bit_depth, self.gpu = name, wp, stream_id, bit_depth, gpu
        self.wp_values = dict(M.DEFAULT_WP) if wp is None else wp
        self.tree = M.flatten(nested)
        self.transforms = list(transforms)
        self.pre = M.copy_channels(coded)
        self.pre_nb_meta = nb_meta
        self.tokens = M.tokenize(self.pre, self.tree, self.wp_values, stream_id, quantize=quantize)
        self.filled = list(filled) if filled is not None else self.transforms
        self.final = M.copy_channels(self.pre)
        self.nb_meta = M.inverse_transforms(self.final, nb_meta, self.filled, self.wp_values, bit_depth)
        self.shapes = [c.shape() for c in self.final]
        shapes, meta, again = M.meta_apply(self.shapes, self.nb_meta, self.transforms)
        assert shapes == [c.shape() for c in self.pre] and meta == nb_meta and again == self.filled, name
        if image is not None and not quantize:
            assert [c.d for c in image] == [c.d for c in self.final], name + ": forward and inverse do not meet"
        self.stream = M.write_stream(self.tokens, self.tree, wp, self.transforms, per_leaf_clusters=per_leaf)


def leaf(predictor, offset=0, multiplier=1):
    return ("leaf", predictor, offset, multiplier)


def split(prop, splitval, greater, not_greater):
    return ("split", prop, splitval, greater, not_greater)


def chain(splits, leaves):
    """property k > splitval k -> leaf k, else the next decision; the last leaf takes the rest."""
    assert len(leaves) == len(splits) + 1
    node = leaves[-1]
    for (prop, splitval), lf in zip(reversed(splits), reversed(leaves[:-1])):
        node = split(prop, splitval, lf, node)
    return node


PRED_WIDTHS, PRED_HEIGHTS = (1, 2, 3, 4, 5, 7, 8, 9, 13), (1, 2, 3, 6)
WP_HEADERS = {
    "default": None,
    "distinct": dict(p1C=19, p2C=11, p3Ca=5, p3Cb=8, p3Cc=3, p3Cd=23, p3Ce=2, w=(14, 9, 12, 6)),
    "north": dict(p1C=16, p2C=8, p3Ca=0, p3Cb=16, p3Cc=0, p3Cd=23, p3Ce=9, w=(13, 13, 12, 12)),
    "weights_0_15": dict(p1C=10, p2C=10, p3Ca=5, p3Cb=5, p3Cc=5, p3Cd=12, p3Ce=4, w=(0, 15, 15, 0)),
}
WP_SIZES = ((1, 7), (2, 5), (3, 3), (9, 6), (37, 11))
WP_TREES = {
    "leaf": leaf(6),
    "split15": split(15, 0, leaf(6, 1, 1), split(15, -40, leaf(6), leaf(6, -2, 2))),
    "prop15_only": split(15, 3, leaf(5), split(15, -30, leaf(1), leaf(2))),
}
SQUEEZE_SIZES = ((1, 4), (2, 1), (5, 3), (8, 8), (17, 9))


def _pred(p):
    chans = [content(w, h, 100 * p + 10 * w + h, base=-5, amp=4 if p == 4 else 40) for w in PRED_WIDTHS for h in PRED_HEIGHTS]
    return Case("pred%d" % p, chans, 0, [], leaf(p))


def _props():
    splits = [(2, 12), (3, 19), (4, 170), (5, 165), (6, 150), (7, 140), (8, 25), (9, 120), (10, 18), (11, 15), (12, 12), (13, 10),
              (14, 8), (15, 30)]
    leaves = [leaf(5), leaf(1), leaf(4, -5, 3), leaf(3), leaf(13), leaf(2, 0, 2 << 4), leaf(10), leaf(11), leaf(12), leaf(7), leaf(8),
              leaf(9), leaf(6), leaf(0, 90), leaf(5, 2)]
    chans = [content(23, 17, 7), content(23, 17, 8, amp=25, gx=-2, gy=4)]
    return Case("props", chans, 0, [], chain(splits, leaves), quantize=True)


def _static(stream_id):
    below = split(7, 120, split(0, 1, leaf(5), split(1, 4, leaf(1), leaf(2))), split(1, 3, split(0, 0, leaf(3), leaf(4)), leaf(11)))
    tree = split(1, 4, split(0, 0, below, leaf(7, 3)), split(0, 1, leaf(12), below))
    chans = [content(11, 9, 20 + c) for c in range(3)]
    return Case("static_s%d" % stream_id, chans, 0, [], tree, stream_id=stream_id)


def _wp(header, tree):
    chans = [content(w, h, 300 + w) for w, h in WP_SIZES]
    return Case("wp_%s_%s" % (header, tree), chans, 0, [], WP_TREES[tree], wp=WP_HEADERS[header], quantize=True)


def _prev():
    a = (13, 9)
    chans = [content(*a, 41), content(*a, 42, gx=-3), content(6, 5, 43), content(*a, 44, gy=5), content(*a, 45, hshift=1),
             content(*a, 46, amp=60), content(*a, 47)]
    splits = [(16, 150), (17, 160), (18, 45), (19, 30), (20, 140), (21, 135), (22, 40), (23, 25), (24, 130), (25, 120), (26, 35),
              (27, 20), (28, 110), (29, 100), (30, 30), (31, 10)]
    leaves = [leaf(p) for p in (5, 1, 2, 3, 4, 7, 8, 9, 10, 11, 12, 13, 0, 5, 1, 2)] + [leaf(5, 1)]
    return Case("prev", chans, 0, [], chain(splits, leaves))


def _prev_wp():
    chans = [content(9, 7, 51), content(9, 7, 52, gx=-1), content(9, 7, 53)]
    tree = split(19, 0, leaf(6), split(17, 110, leaf(5), split(15, 0, leaf(6, 1), leaf(1))))
    return Case("prev_wp", chans, 0, [], tree)


def _rects():
    chans = [content(7, 5, 61), Chan(0, 5), content(5, 3, 62), content(9, 4, 63)]
    return Case("rects", chans, 0, [], split(3, 2, leaf(5), leaf(2)))


def _rct(perm):
    image = [content(19, 5, 70 + k, gx=(k % 5) - 2, base=60 * (k % 3) - 70) for k in range(21)]
    transforms = [("rct", 3 * c, 7 * perm + c) for c in range(7)]
    coded = M.copy_channels(image)
    for t in transforms:
        M.rct_forward(coded, t[1], t[2])
    return Case("rct_perm%d" % perm, coded, 0, transforms, leaf(0), image=image)


def _rct_wrap(rct_type):
    big = 1 << 30
    r = random.Random(rct_type)
    image = [Chan(6, 3, rows=[[r.choice((big, -big, big - 1, -big + 1, 5, -7)) for _ in range(6)] for _ in range(3)]) for _ in range(3)]
    coded = M.copy_channels(image)
    M.rct_forward(coded, 0, rct_type)
    return Case("rct_wrap%d" % rct_type, coded, 0, [("rct", 0, rct_type)], leaf(0), image=image)


def _squeeze(w, h):
    image = [content(w, h, 80 + w, amp=12), content(w, h, 81 + h, amp=30, gx=-4)]
    steps = [(True, True, 0, 2), (False, False, 0, 1), (False, True, 1, 1)]
    coded = M.copy_channels(image)
    M.squeeze_forward(coded, 0, steps)
    return Case("squeeze_%dx%d" % (w, h), coded, 0, [("squeeze", steps)], leaf(0), image=image)


def tendency_line():
    """A line whose pairs take every branch of SmoothTendency (tests/test_modular_np.py asserts the set)."""
    r = random.Random(5)
    line = []
    for _ in range(24):  # runs: steep falls and rises (the limits bind), gentle ones (they do not), flats, zigzags
        kind, v = r.randrange(6), (line[-1] if line else 0)
        step = (-9, 9, -1, 1, 0, 0)[kind]
        for k in range(r.randint(3, 7)):
            v += step * (k + 1) if kind < 2 else step
            line.append(v + (r.randint(-6, 6) if kind == 5 else 0))
    return line


def _squeeze_line():
    image = [Chan(len(tendency_line()), 1, rows=[tendency_line()])]
    steps = [(True, True, 0, 1)]
    coded = M.copy_channels(image)
    M.squeeze_forward(coded, 0, steps)
    return Case("squeeze_line", coded, 0, [("squeeze", steps)], leaf(0), image=image)


def _squeeze_default():
    image = [content(40, 24, 90 + c, amp=20) for c in range(3)]
    steps = M.default_squeeze_steps(image, 0)
    coded = M.copy_channels(image)
    M.squeeze_forward(coded, 0, steps)
    return Case("squeeze_default", coded, 0, [("squeeze", [])], leaf(0), image=image, filled=[("squeeze", steps)])


def _palette_nb1():
    pal = Chan(5, 1, -1, -1, [[10, -3, 77, 200, 41]])
    r = random.Random(11)
    idx = Chan(11, 7, rows=[[r.randint(-3, 8) for _ in range(11)] for _ in range(7)])
    return Case("palette_nb1", [pal, idx], 1, [("palette", 0, 1, 5, 0, 0)], leaf(0))


def _palette_nb3(bits):
    top = (1 << bits) - 1
    r = random.Random(bits)
    pal = Chan(6, 3, -1, -1, [[r.randint(0, top) for _ in range(6)] for _ in range(3)])
    pool = list(range(6)) + list(range(6, 6 + 64, 5)) + list(range(70, 70 + 125, 7)) + [6 + 63, 70 + 124, 70 + 125, 300] + list(range(-1, -150, -4))
    idx = Chan(13, 7, rows=[[r.choice(pool) for _ in range(13)] for _ in range(7)])
    return Case("palette_nb3_%d" % bits, [pal, idx], 1, [("palette", 0, 3, 6, 0, 0)], leaf(0), bit_depth=bits)


def _palette_rct():
    r = random.Random(13)
    pal = Chan(7, 3, -1, -1, [[r.randint(0, 255) for _ in range(7)] for _ in range(3)])
    before = [pal, Chan(9, 6, rows=[[r.randint(-2, 80) for _ in range(9)] for _ in range(6)]), content(9, 6, 14), content(9, 6, 15)]
    coded = M.copy_channels(before)
    M.rct_forward(coded, 1, 10)
    return Case("palette_rct", coded, 1, [("palette", 0, 3, 7, 0, 0), ("rct", 1, 10)], leaf(0))


def _palette_delta(predictor):
    r = random.Random(17 + predictor)
    pal = Chan(9, 3, -1, -1, [[r.randint(-20, 20) if k < 3 else r.randint(0, 255) for k in range(9)] for _ in range(3)])
    idx = Chan(10, 6, rows=[[r.choice((0, 1, 2, 3, 4, 5, 8, -1, -5, 12, 80)) for _ in range(10)] for _ in range(6)])
    return Case("palette_delta_p%d" % predictor, [pal, idx], 1, [("palette", 0, 3, 6, 3, predictor)], leaf(0), gpu=False)


BUILDERS = {}
for _p in range(14):
    BUILDERS["pred%d" % _p] = (_pred, _p)
BUILDERS["props"] = (_props,)
BUILDERS["static_s3"] = (_static, 3)
BUILDERS["static_s5"] = (_static, 5)
for _h in WP_HEADERS:
    for _t in WP_TREES:
        BUILDERS["wp_%s_%s" % (_h, _t)] = (_wp, _h, _t)
BUILDERS["prev"] = (_prev,)
BUILDERS["prev_wp"] = (_prev_wp,)
BUILDERS["rects"] = (_rects,)
for _p in range(6):
    BUILDERS["rct_perm%d" % _p] = (_rct, _p)
BUILDERS["rct_wrap6"] = (_rct_wrap, 6)
BUILDERS["rct_wrap4"] = (_rct_wrap, 4)
for _w, _h in SQUEEZE_SIZES:
    BUILDERS["squeeze_%dx%d" % (_w, _h)] = (_squeeze, _w, _h)
BUILDERS["squeeze_line"] = (_squeeze_line,)
BUILDERS["squeeze_default"] = (_squeeze_default,)
BUILDERS["palette_nb1"] = (_palette_nb1,)
BUILDERS["palette_nb3_8"] = (_palette_nb3, 8)
BUILDERS["palette_nb3_12"] = (_palette_nb3, 12)
BUILDERS["palette_rct"] = (_palette_rct,)
for _p in (0, 5, 6):
    BUILDERS["palette_delta_p%d" % _p] = (_palette_delta, _p)
NAMES = tuple(BUILDERS)
GPU_NAMES = tuple(n for n in NAMES if not n.startswith("palette_delta"))


def build(name):
    if name not in _BUILT:
        f = BUILDERS[name]
        _BUILT[name] = f[0](*f[1:])
    return _BUILT[name]
