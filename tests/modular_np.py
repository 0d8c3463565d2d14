"""A plain reading of the Modular sample model, its transforms and one sub-bitstream, both ways, in Python integers,
written from the reference's text alone:

  tokenize / reconstruct  modular/encoding/encoding.cc:148-506 (DecodeModularChannelMAANS: the leaf gives
                          UnpackSigned(v) * multiplier + offset + prediction, :186-192), context_predict.h:372-590 (the
                          properties, the previous-channel properties, the fourteen predictors, the tree walk),
                          context_predict.h:66-218 (the weighted predictor and its header);
  rct_*                   modular/transform/rct.cc:30-147;
  squeeze_*               modular/transform/squeeze.cc:128-371 (InvHSqueeze / InvVSqueeze / InvSqueeze), :387-444 (the default step
                          list), :456-517 (MetaSqueeze), squeeze.h:54-77 (SmoothTendency);
  palette_*               modular/transform/palette.cc:26-202, palette.h:25-140 (implicit colours: tests/palette_np.py);
  write_stream            modular/encoding/encoding.h:30-49 (GroupHeader), transform.cc:36-88 and squeeze_params.cc:14-24
                          (the transform fields), dec_ma.cc:107-159 (the tree, six contexts), dec_ans.cc (LZ77 bit, simple
                          context map, log_alpha, hybrid-uint configuration, flat histograms), encoding.cc:554-724 (the order
                          of the parts).

Nothing here imports the product, the oracle or the test encoder. A channel is a Chan (w, h, hshift, vshift, rows of Python
ints); a value is narrowed to int32 exactly where the reference stores a pixel_type, everything between is exact. The model
asserts that no property leaves int32 (the RCT functions wrap on purpose).

A tree is a list of nodes in the order the stream carries them (dec_ma.cc:153-155: the children of the node read at size s
with d nodes still to read are s + d + 1 and s + d + 2): (property, splitval, lchild, rchild) for a decision and
(-1, context, predictor, offset, multiplier) for a leaf. flatten() makes one from a nested
("split", property, splitval, greater, not_greater) / ("leaf", predictor, offset, multiplier) description.

MISREADINGS names the ways these rules could be misread; each is a switch (`mis`, a set of names), off unless named, and
tests/test_modular_np.py shows that each one changes the result of a case named beside it."""
import ans_np
import palette_np

MISREADINGS = (
    "prop8_from_current_9",     # property 8 = left - this sample's gradient instead of the previous sample's
    "prop9_not_reset",          # property 9 carried over from the end of the previous row
    "avg0_floor",               # predictor 3 (left + top) / 2 with floor instead of C truncation
    "avg123_floor",             # predictors 10, 11, 12 likewise
    "avg4_floor",               # predictor 13's / 16 likewise
    "select_tie_other",         # Select: a on a tie (pa <= pb) instead of b
    "toprightright_to_top",     # toprightright falls back to top instead of topright
    "vtop_fallback_zero",       # previous channel: vtop in the first row 0 instead of vleft
    "refs_farthest_first",      # previous channels counted from channel 0 upwards
    "refs_ignore_shift",        # a channel of equal w, h but another shift signature counted
    "branch_ge",                # lchild on property >= splitval
    "multiplier_on_prediction", # (unpack(v) + prediction) * multiplier + offset
    "wp_round_4",               # (pred + 4) >> 3
    "wp_clamp_always",          # the clamp to min/max(W, NE, N) without the sign test
    "wp_no_above_right",        # UpdateErrors without pred_errors[prev_row + x + 1] += err
    "wp_ne_last_zero",          # at the last column the NE errors read as 0 instead of N's
    "wp_max_error_tie_later",   # max-error property: >= instead of >
    "wp_swap_p3d_p3e",          # p3Cd and p3Ce exchanged
    "rct_swap_permutation_23",  # the second and third outputs of the permutation exchanged
    "rct_avg_truncates",        # (First + Third) >> 1 as a truncating division
    "squeeze_diff_floor",       # A = avg + floor(diff / 2)
    "squeeze_limit_a",          # the first tendency limit without its +- 1
    "squeeze_limit_b",          # the second tendency limit with the first one's +- 1
    "squeeze_odd_from_residual",  # the odd last sample taken from the residual channel
    "palette_no_clamp",         # nb == 1 without the index clamp
    "palette_delta_parity",     # implicit delta colours: sign by the other parity
)

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
DEFAULT_WP = dict(p1C=16, p2C=10, p3Ca=7, p3Cb=7, p3Cc=7, p3Cd=0, p3Ce=0, w=(13, 12, 12, 12))  # context_predict.h:50-60
WP_FIELDS = ("p1C", "p2C", "p3Ca", "p3Cb", "p3Cc", "p3Cd", "p3Ce")
DIVLOOKUP = [(1 << 24) // (i + 1) for i in range(64)]  # context_predict.h:77-87


def i32(v):
    """What a pixel_type holds after `v` is stored into it."""
    return ((int(v) - I32_MIN) & 0xFFFFFFFF) + I32_MIN


def cdiv(a, b):
    """C division: towards zero."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def pack_signed(v):
    return 2 * v if v >= 0 else -2 * v - 1


def unpack_signed(u):
    return (u >> 1) if not u & 1 else -((u >> 1) + 1)


class Chan:
    def __init__(self, w, h, hshift=0, vshift=0, rows=None):
        self.w, self.h, self.hshift, self.vshift = int(w), int(h), int(hshift), int(vshift)
        self.d = [[0] * self.w for _ in range(self.h)] if rows is None else [[int(v) for v in r] for r in rows]
        assert len(self.d) == self.h and all(len(r) == self.w for r in self.d), (w, h)

    def copy(self):
        return Chan(self.w, self.h, self.hshift, self.vshift, self.d)

    def shape(self):
        return (self.w, self.h, self.hshift, self.vshift)

    def flat(self):
        return [v for r in self.d for v in r]


def copy_channels(chs):
    return [c.copy() for c in chs]


# ---------------------------------------------------------------- the tree
def flatten(nested):
    """The stream order of a nested tree; leaves get their context in the order they are read (dec_ma.cc:146-148)."""
    out, queue, leaf_id = [], [nested], 0
    while queue:
        n = queue.pop(0)
        if n[0] == "leaf":
            _, predictor, offset, multiplier = n
            out.append((-1, leaf_id, predictor, offset, multiplier))
            leaf_id += 1
        else:
            _, prop, splitval, greater, not_greater = n
            l = len(out) + len(queue) + 1
            out.append((prop, splitval, l, l + 1))
            queue += [greater, not_greater]
    return out


def num_leaves(tree):
    return sum(1 for n in tree if n[0] < 0)


def tree_uses_wp(tree):
    return any(n[0] == 15 or (n[0] < 0 and n[2] == 6) for n in tree)


def tree_num_props(tree):
    """encoding.cc:133-140: sixteen, and four per previous channel up to the highest property asked for."""
    top = max([n[0] for n in tree] + [15])
    return 16 + (top - 16 + 1 + 3) // 4 * 4 if top >= 16 else 16


# ---------------------------------------------------------------- the weighted predictor (context_predict.h:66-218)
class WpState:
    def __init__(self, header, xsize, mis):
        self.h, self.xs, self.mis = header, xsize, mis
        self.pred_errors = [[0] * ((xsize + 2) * 2) for _ in range(4)]
        self.error = [0] * ((xsize + 2) * 2)
        self.prediction = [0] * 4
        self.pred = 0

    @staticmethod
    def error_weight(x, maxweight):  # :103-107
        shift = max(0, (x + 1).bit_length() - 1 - 5)
        return 4 + ((maxweight * DIVLOOKUP[x >> shift]) >> shift)

    @staticmethod
    def weighted_average(p, w):  # :111-131
        log_weight = sum(w).bit_length() - 1
        w = [v >> (log_weight - 4) for v in w]
        weight_sum = sum(w)
        s = (weight_sum >> 1) - 1
        for i in range(4):
            s += p[i] * w[i]
        return (s * DIVLOOKUP[weight_sum - 1]) >> 24

    def predict(self, x, y, N, W, NE, NW, NN):
        """-> (prediction, max-error property) (:134-193)"""
        xs, h, mis = self.xs, self.h, self.mis
        cur = 0 if y & 1 else xs + 2
        prev = xs + 2 if y & 1 else 0
        pos_N = prev + x
        pos_NE = pos_N + 1 if x < xs - 1 else pos_N
        pos_NW = pos_N - 1 if x > 0 else pos_N
        ne_zero = "wp_ne_last_zero" in mis and not x < xs - 1
        weights = []
        for i in range(4):
            pe = self.pred_errors[i]
            weights.append(self.error_weight(pe[pos_N] + (0 if ne_zero else pe[pos_NE]) + pe[pos_NW], h["w"][i]))
        N, W, NE, NW, NN = N * 8, W * 8, NE * 8, NW * 8, NN * 8
        teW = 0 if x == 0 else self.error[cur + x - 1]
        teN, teNW = self.error[pos_N], self.error[pos_NW]
        teNE = 0 if ne_zero else self.error[pos_NE]
        sumWN = teN + teW
        p = teW
        later = "wp_max_error_tie_later" in mis
        for t in (teN, teNW, teNE):
            if abs(t) > abs(p) or (later and abs(t) == abs(p)):
                p = t
        p3d, p3e = (h["p3Ce"], h["p3Cd"]) if "wp_swap_p3d_p3e" in mis else (h["p3Cd"], h["p3Ce"])
        pr = self.prediction
        pr[0] = W + NE - N
        pr[1] = N - (((sumWN + teNE) * h["p1C"]) >> 5)
        pr[2] = W - (((sumWN + teNW) * h["p2C"]) >> 5)
        pr[3] = N - ((teNW * h["p3Ca"] + teN * h["p3Cb"] + teNE * h["p3Cc"] + (NN - N) * p3d + (NW - W) * p3e) >> 5)
        self.pred = self.weighted_average(pr, weights)
        rnd = 4 if "wp_round_4" in mis else 3
        if ((teN ^ teW) | (teN ^ teNW)) > 0 and "wp_clamp_always" not in mis:  # all three of one sign: no clamp
            return (self.pred + rnd) >> 3, p
        self.pred = max(min(W, NE, N), min(max(W, NE, N), self.pred))
        return (self.pred + rnd) >> 3, p

    def update(self, val, x, y):  # :195-210
        xs = self.xs
        cur = 0 if y & 1 else xs + 2
        prev = xs + 2 if y & 1 else 0
        val *= 8
        self.error[cur + x] = i32(self.pred - val)
        for i in range(4):
            err = (abs(self.prediction[i] - val) + 3) >> 3
            assert err <= 0xFFFFFFFF or self.mis  # (a uint32 in the reference; a model case stays far below)
            err &= 0xFFFFFFFF
            self.pred_errors[i][cur + x] = err
            if "wp_no_above_right" not in self.mis:
                self.pred_errors[i][prev + x + 1] = (self.pred_errors[i][prev + x + 1] + err) & 0xFFFFFFFF


# ---------------------------------------------------------------- predictors (context_predict.h:385-409, :472-512)
def clamped_gradient(n, w, l):
    m, M = min(n, w), max(n, w)
    grad = i32(n + w - l)
    return m if l > M else (M if l < m else grad)


def predict_one(p, left, top, toptop, topleft, topright, leftleft, toprightright, wp_pred, mis=()):
    def half(v, name):
        return v >> 1 if name in mis else cdiv(v, 2)
    if p == 0:
        return 0
    if p == 1:
        return left
    if p == 2:
        return top
    if p == 3:
        return half(left + top, "avg0_floor")
    if p == 4:
        g = left + top - topleft
        pa, pb = abs(g - left), abs(g - top)
        return left if (pa <= pb if "select_tie_other" in mis else pa < pb) else top
    if p == 5:
        return clamped_gradient(left, top, topleft)
    if p == 6:
        return wp_pred
    if p == 7:
        return topright
    if p == 8:
        return topleft
    if p == 9:
        return leftleft
    if p == 10:
        return half(left + topleft, "avg123_floor")
    if p == 11:
        return half(topleft + top, "avg123_floor")
    if p == 12:
        return half(top + topright, "avg123_floor")
    if p == 13:
        v = 6 * top - 2 * toptop + 7 * left + leftleft + toprightright + 3 * topright + 8
        return v >> 4 if "avg4_floor" in mis else cdiv(v, 16)
    raise ValueError("predictor %d" % p)


def neighbours(d, x, y, w, mis=()):
    """left, top, toptop, topleft, topright, leftleft, toprightright with every edge fallback (context_predict.h:525-532)."""
    row = d[y]
    up = d[y - 1] if y else None
    left = row[x - 1] if x else (up[x] if y else 0)
    top = up[x] if y else left
    topleft = up[x - 1] if x and y else left
    topright = up[x + 1] if x + 1 < w and y else top
    leftleft = row[x - 2] if x > 1 else left
    toptop = d[y - 2][x] if y > 1 else top
    toprightright = up[x + 2] if x + 2 < w and y else (top if "toprightright_to_top" in mis else topright)
    return left, top, toptop, topleft, topright, leftleft, toprightright


def reference_channels(chs, i, num_props, mis=()):
    """The channels whose samples make properties 16.. of channel i, in property order (context_predict.h:418-425)."""
    c, out = chs[i], []
    order = range(i) if "refs_farthest_first" in mis else range(i - 1, -1, -1)
    for j in order:
        if len(out) * 4 >= num_props - 16:
            break
        r = chs[j]
        if r.w != c.w or r.h != c.h:
            continue
        if (r.hshift != c.hshift or r.vshift != c.vshift) and "refs_ignore_shift" not in mis:
            continue
        out.append(j)
    return out


def _check_props(props):
    for k, v in enumerate(props):
        assert I32_MIN <= v <= I32_MAX, "property %d = %d leaves int32: not a model case" % (k, v)


def _channel(chs, i, tree, wp, stream_id, first_channel, mis, values, quantize):
    """One channel, either way. values is None: the samples of chs[i] are tokenized -> [(context, token)]; with
    `quantize` a sample no leaf can reach (multiplier > 1) is replaced by the nearest one it can. Otherwise values(context)
    gives the next unsigned token value and the samples are filled in -> [(context, token)] all the same."""
    c = chs[i]
    out = []
    if c.w == 0 or c.h == 0:  # encoding.cc:165
        return out
    uses_wp = tree_uses_wp(tree)
    num_props = tree_num_props(tree)
    refs = reference_channels(chs, i, num_props, mis)
    wps = WpState(wp, c.w, mis) if uses_wp else None
    props = [0] * num_props
    d, w = c.d, c.w
    ge = "branch_ge" in mis
    single = len(tree) == 1
    for y in range(c.h):
        props[0], props[1], props[2] = i + first_channel, stream_id, y  # InitPropsRow, context_predict.h:452-461
        if "prop9_not_reset" not in mis:
            props[9] = 0
        row = d[y]
        for x in range(w):
            left, top, toptop, topleft, topright, leftleft, toprightright = nb = neighbours(d, x, y, w, mis)
            pos = 0
            wp_pred = 0
            if single and uses_wp:  # (a tree of one leaf: no property is worked out, encoding.cc:212-216, :380-397)
                wp_pred = wps.predict(x, y, top, left, topright, topleft, toptop)[0]
            if not single:
                props[3] = x
                props[4] = abs(top)
                props[5] = abs(left)
                props[6] = top
                props[7] = left
                grad = left + top - topleft
                props[8] = left - (grad if "prop8_from_current_9" in mis else props[9])
                props[9] = grad
                props[10] = left - topleft
                props[11] = topleft - top
                props[12] = top - topright
                props[13] = top - toptop
                props[14] = left - leftleft
                if uses_wp:
                    wp_pred, props[15] = wps.predict(x, y, top, left, topright, topleft, toptop)
                k = 16
                for j in refs:  # context_predict.h:426-440
                    rd = chs[j].d
                    v = rd[y][x]
                    vleft = rd[y][x - 1] if x else 0
                    vtop = rd[y - 1][x] if y else (0 if "vtop_fallback_zero" in mis else vleft)
                    vtopleft = rd[y - 1][x - 1] if x and y else vleft
                    vp = clamped_gradient(vleft, vtop, vtopleft)
                    props[k], props[k + 1], props[k + 2], props[k + 3] = abs(v), v, abs(v - vp), v - vp
                    k += 4
                if not mis:
                    _check_props(props)
                while tree[pos][0] >= 0:  # context_predict.h:351-366: properties[p] <= splitval goes to the second child
                    prop, splitval, l, r = tree[pos]
                    pos = l if (props[prop] >= splitval if ge else props[prop] > splitval) else r
            _, ctx, predictor, offset, multiplier = tree[pos]
            guess = predict_one(predictor, *nb, wp_pred, mis)
            if values is None:
                v = row[x]
                q, rem = divmod(v - offset - guess, multiplier)  # (the misreadings of the leaf are read back only)
                if 2 * rem >= multiplier:
                    q += 1
                token = pack_signed(q)
                exact = q * multiplier + offset + guess
                assert quantize or exact == v, "sample %d of channel %d is not on the leaf's lattice" % (v, i)
                assert I32_MIN <= exact <= I32_MAX
                row[x] = exact
            else:
                token = values(ctx)
                q = unpack_signed(token)
                if "multiplier_on_prediction" in mis:
                    row[x] = i32((q + guess) * multiplier + offset)
                else:
                    row[x] = i32(q * multiplier + offset + guess)  # make_pixel, encoding.cc:186-192
            assert token <= 0xFFFFFFFF
            out.append((ctx, token))
            if uses_wp:
                wps.update(row[x], x, y)
    return out


def tokenize(channels, tree, wp=DEFAULT_WP, stream_id=0, first_channel=0, mis=(), quantize=False):
    """(context, unsigned token value) of every sample, channel by channel. The channels are left as the decoder will
    have them (they change only under `quantize`)."""
    mis = frozenset(mis)
    out = []
    for i in range(len(channels)):
        out += _channel(channels, i, tree, wp, stream_id, first_channel, mis, None, quantize)
    return out


def reconstruct(values, shapes, tree, wp=DEFAULT_WP, stream_id=0, first_channel=0, mis=()):
    """The inverse. `values` is the sequence of unsigned token values in stream order, or a function of the context
    that reads the next one (ans_np.Reader.read); shapes = [(w, h, hshift, vshift)] -> the channels."""
    mis = frozenset(mis)
    chs = [Chan(*s) for s in shapes]
    if not callable(values):
        it = iter(values)
        values = lambda ctx: next(it)
    for i in range(len(chs)):
        _channel(chs, i, tree, wp, stream_id, first_channel, mis, values, False)
    return chs


# ---------------------------------------------------------------- RCT (rct.cc:30-147), in wrapping int32 like PixelAdd
def _rct_places(perm, mis):
    """Where the three outputs go (rct.cc:137-141)."""
    second, third = (perm + 1 + perm // 3) % 3, (perm + 2 - perm // 3) % 3
    if "rct_swap_permutation_23" in mis:
        second, third = third, second
    return perm % 3, second, third


def _half(v, mis):
    return cdiv(v, 2) if "rct_avg_truncates" in mis else v >> 1


def rct_inverse(chs, begin_c, rct_type, mis=()):
    a, b, c = chs[begin_c:begin_c + 3]
    assert a.shape() == b.shape() == c.shape()
    if rct_type == 0:
        return
    perm, custom = rct_type // 7, rct_type % 7
    second, third = custom >> 1, custom & 1
    outs = [Chan(*a.shape()) for _ in range(3)]
    for y in range(a.h):
        for x in range(a.w):
            v0, v1, v2 = a.d[y][x], b.d[y][x], c.d[y][x]
            if custom == 6:
                tmp = i32(v0 - (v2 >> 1))
                g = i32(v2 + tmp)
                bl = i32(tmp - (v1 >> 1))
                v0, v1, v2 = i32(bl + v1), g, bl
            else:
                if third:
                    v2 = i32(v2 + v0)
                if second == 1:
                    v1 = i32(v1 + v0)
                elif second == 2:
                    v1 = i32(v1 + _half(i32(v0 + v2), mis))
            outs[0].d[y][x], outs[1].d[y][x], outs[2].d[y][x] = v0, v1, v2
    for o, place in zip(outs, _rct_places(perm, mis)):
        chs[begin_c + place] = o


def rct_forward(chs, begin_c, rct_type):
    """What a writer stores so that rct_inverse gives `chs` back, in the same wrapping arithmetic."""
    if rct_type == 0:
        return
    perm, custom = rct_type // 7, rct_type % 7
    second, third = custom >> 1, custom & 1
    a, b, c = [chs[begin_c + place] for place in _rct_places(perm, ())]
    outs = [Chan(*a.shape()) for _ in range(3)]
    for y in range(a.h):
        for x in range(a.w):
            v0, v1, v2 = a.d[y][x], b.d[y][x], c.d[y][x]
            if custom == 6:  # v0 = R, v1 = G, v2 = B
                co = i32(v0 - v2)
                tmp = i32(v2 + (co >> 1))
                cg = i32(v1 - tmp)
                v0, v1, v2 = i32(tmp + (cg >> 1)), co, cg
            else:
                if second == 1:
                    v1 = i32(v1 - v0)
                elif second == 2:
                    v1 = i32(v1 - (i32(v0 + v2) >> 1))
                if third:
                    v2 = i32(v2 - v0)
            outs[0].d[y][x], outs[1].d[y][x], outs[2].d[y][x] = v0, v1, v2
    chs[begin_c:begin_c + 3] = outs


# ---------------------------------------------------------------- Squeeze (squeeze.cc, squeeze.h:54-77)
def smooth_tendency(B, a, n, mis=()):
    diff = 0
    la, lb = "squeeze_limit_a" in mis, "squeeze_limit_b" in mis
    if B >= a and a >= n:
        diff = cdiv(4 * B - 3 * n - a + 6, 12)
        if diff - (diff & 1) > 2 * (B - a):
            diff = 2 * (B - a) + (0 if la else 1)
        if diff + (diff & 1) > 2 * (a - n):
            diff = 2 * (a - n) + (1 if lb else 0)
    elif B <= a and a <= n:
        diff = cdiv(4 * B - 3 * n - a - 6, 12)
        if diff + (diff & 1) < 2 * (B - a):
            diff = 2 * (B - a) - (0 if la else 1)
        if diff - (diff & 1) < 2 * (a - n):
            diff = 2 * (a - n) - (1 if lb else 0)
    return diff


def tendency_branch(B, a, n):
    """Which way SmoothTendency went, for the test that a constructed line takes every one."""
    if B >= a >= n or B <= a <= n:
        falling = B >= a >= n
        diff = cdiv(4 * B - 3 * n - a + (6 if falling else -6), 12)
        if falling:
            first = diff - (diff & 1) > 2 * (B - a)
            if first:
                diff = 2 * (B - a) + 1
            second = diff + (diff & 1) > 2 * (a - n)
        else:
            first = diff + (diff & 1) < 2 * (B - a)
            if first:
                diff = 2 * (B - a) - 1
            second = diff - (diff & 1) < 2 * (a - n)
        kind = "equal" if B == a == n else ("falling" if falling else "rising")
        return kind + ("+a" if first else "") + ("+b" if second else "")
    return "neither"


def unsqueeze_line(avg, res, mis=(), branches=None):
    """One line (squeeze.cc:158-175; the vertical form :283-326 is the same along y): len(avg) averages and len(res)
    residuals (as many or one fewer) -> len(avg) + len(res) samples."""
    out = [0] * (len(avg) + len(res))
    for x in range(len(res)):
        a = avg[x]
        nxt = avg[x + 1] if x + 1 < len(avg) else a
        left = out[2 * x - 1] if x else a
        if branches is not None:
            branches.add(tendency_branch(left, a, nxt))
        diff = res[x] + smooth_tendency(left, a, nxt, mis)
        first = a + (diff >> 1 if "squeeze_diff_floor" in mis else cdiv(diff, 2))
        out[2 * x] = i32(first)
        out[2 * x + 1] = i32(first - diff)
    if len(out) & 1:
        out[-1] = res[-1] if "squeeze_odd_from_residual" in mis and res else avg[-1]
    return out


def squeeze_line(samples):
    """The forward step of one line: averages round towards the first sample of the pair, the residual is the pair's
    difference minus the tendency predicted from the sample before the pair, its average and the next."""
    n = len(samples)
    na = (n + 1) // 2
    avg = [0] * na
    for x in range(n // 2):
        A, B = samples[2 * x], samples[2 * x + 1]
        avg[x] = (A + B + (1 if A > B else 0)) >> 1
    if n & 1:
        avg[-1] = samples[-1]
    res = []
    for x in range(n // 2):
        nxt = avg[x + 1] if x + 1 < na else avg[x]
        left = samples[2 * x - 1] if x else avg[x]
        res.append(samples[2 * x] - samples[2 * x + 1] - smooth_tendency(left, avg[x], nxt))
    return avg, res


def default_squeeze_steps(chs, nb_meta):
    """squeeze.cc:387-444 -> [(horizontal, in_place, begin_c, num_c)]"""
    count = len(chs) - nb_meta
    w, h = chs[nb_meta].w, chs[nb_meta].h
    steps = []
    if count > 2 and chs[nb_meta + 1].w == w and chs[nb_meta + 1].h == h:
        steps += [(True, False, nb_meta + 1, 2), (False, False, nb_meta + 1, 2)]
    if not w > h and h > 8:
        steps.append((False, True, nb_meta, count))
        h = (h + 1) // 2
    while w > 8 or h > 8:
        if w > 8:
            steps.append((True, True, nb_meta, count))
            w = (w + 1) // 2
        if h > 8:
            steps.append((False, True, nb_meta, count))
            h = (h + 1) // 2
    return steps


def _columns(c):
    return [[c.d[y][x] for y in range(c.h)] for x in range(c.w)]


def _from_columns(cols, h, hshift, vshift):
    return Chan(len(cols), h, hshift, vshift, [[col[y] for col in cols] for y in range(h)])


def squeeze_forward(chs, nb_meta, steps):
    """The channel-list changes of MetaSqueeze (squeeze.cc:456-517) with the data split as the inverse expects it.
    -> the new nb_meta."""
    for horizontal, in_place, begin_c, num_c in steps:
        end = begin_c + num_c
        if begin_c < nb_meta:
            assert end <= nb_meta and in_place
            nb_meta += num_c
        at = end if in_place else len(chs)
        for c in range(begin_c, end):
            src = chs[c]
            assert src.w and src.h
            hs = src.hshift + 1 if horizontal and src.hshift >= 0 else src.hshift
            vs = src.vshift + 1 if not horizontal and src.vshift >= 0 else src.vshift
            if horizontal:
                pairs = [squeeze_line(r) for r in src.d]
                chs[c] = Chan((src.w + 1) // 2, src.h, hs, vs, [p[0] for p in pairs])
                res = Chan(src.w // 2, src.h, hs, vs, [p[1] for p in pairs])
            else:
                pairs = [squeeze_line(col) for col in _columns(src)]
                chs[c] = _from_columns([p[0] for p in pairs], (src.h + 1) // 2, hs, vs)
                res = _from_columns([p[1] for p in pairs], src.h // 2, hs, vs)
            chs.insert(at + (c - begin_c), res)
    return nb_meta


def squeeze_meta(shapes, nb_meta, steps):
    """The same on shapes alone."""
    chs = [Chan(*s) for s in shapes]
    nb_meta = squeeze_forward(chs, nb_meta, steps)
    return [c.shape() for c in chs], nb_meta


def squeeze_inverse(chs, nb_meta, steps, mis=(), branches=None):
    """squeeze.cc:331-371 (InvSqueeze: the steps backwards, the residual channels removed) -> the new nb_meta."""
    for horizontal, in_place, begin_c, num_c in reversed(steps):
        end = begin_c + num_c
        first_res = end if in_place else len(chs) + begin_c - end
        if begin_c < nb_meta:
            nb_meta -= num_c
        for c in range(begin_c, end):
            a, r = chs[c], chs[first_res + c - begin_c]
            if horizontal:
                assert a.w == (a.w + r.w + 1) // 2 and a.h == r.h
                rows = [unsqueeze_line(a.d[y], r.d[y], mis, branches) for y in range(a.h)] if r.w else a.d
                chs[c] = Chan(a.w + r.w, a.h, a.hshift - 1, a.vshift, rows)
            else:
                assert a.h == (a.h + r.h + 1) // 2 and a.w == r.w
                if r.h:
                    cols = [unsqueeze_line(ca, cr, mis, branches) for ca, cr in zip(_columns(a), _columns(r))]
                    chs[c] = _from_columns(cols, a.h + r.h, a.hshift, a.vshift - 1)
                else:
                    chs[c] = Chan(a.w, a.h, a.hshift, a.vshift - 1, a.d)
        del chs[first_res:first_res + num_c]
    return nb_meta


# ---------------------------------------------------------------- Palette (palette.cc:26-202, palette.h:25-140)
def palette_value(pal, index, c, bit_depth, mis=()):
    """GetPaletteValue: an explicit entry, or an implicit colour (0 beyond the third channel)."""
    if 0 <= index < pal.w:
        return pal.d[c][index]
    if c >= 3:
        return 0
    v = int(palette_np.implicit_color(index, pal.w, bit_depth)[c])
    return -v if index < 0 and "palette_delta_parity" in mis else v


def palette_meta(shapes, nb_meta, begin_c, num_c, nb_colors, nb_deltas):
    """MetaPalette (palette.cc:177-200) on shapes -> (shapes, nb_meta)."""
    end_c = begin_c + num_c - 1
    assert all(s == shapes[begin_c] for s in shapes[begin_c:end_c + 1])
    if begin_c >= nb_meta:
        nb_meta += 1
    else:
        assert end_c < nb_meta
        nb_meta += 2 - num_c
    shapes = list(shapes)
    del shapes[begin_c + 1:end_c + 1]
    return [(nb_colors + nb_deltas, num_c, -1, -1)] + shapes, nb_meta


def palette_inverse(chs, nb_meta, begin_c, nb_deltas, predictor, wp, bit_depth, mis=()):
    """InvPalette (palette.cc:28-175) -> the new nb_meta. chs[0] is the palette, chs[begin_c + 1] the indices."""
    pal = chs[0]
    nb = pal.h
    c0 = begin_c + 1
    idx = chs[c0]
    w, h = idx.w, idx.h
    bit_depth = min(bit_depth, 24)
    outs = [Chan(w, h, idx.hshift, idx.vshift) for _ in range(nb)]
    for c in range(nb):
        o = outs[c]
        wps = WpState(wp, w, frozenset()) if predictor == 6 else None
        for y in range(h):
            for x in range(w):
                index = idx.d[y][x]
                if nb_deltas == 0 and predictor == 0:
                    if nb == 1 and "palette_no_clamp" not in mis:
                        index = max(0, min(index, pal.w - 1))
                    o.d[y][x] = palette_value(pal, index, c, bit_depth, mis)
                    continue
                entry = palette_value(pal, index, c, bit_depth, mis)
                left, top, toptop, topleft, topright, leftleft, toprightright = nbr = neighbours(o.d, x, y, w)
                wp_pred = wps.predict(x, y, top, left, topright, topleft, toptop)[0] if wps else 0
                val = entry
                if index < nb_deltas:
                    val += predict_one(predictor, *nbr, wp_pred)
                o.d[y][x] = i32(val)
                if wps:
                    wps.update(o.d[y][x], x, y)
    chs[c0:c0 + 1] = outs
    nb_meta += -1 if c0 >= nb_meta else -(2 - nb)
    del chs[0]
    return nb_meta


# ---------------------------------------------------------------- a transform list on a channel list (MetaApply / Inverse)
# A transform is ("rct", begin_c, rct_type), ("palette", begin_c, num_c, nb_colors, nb_deltas, predictor) or
# ("squeeze", steps) with steps = [(horizontal, in_place, begin_c, num_c)] ([] = the default list).
def meta_apply(shapes, nb_meta, transforms):
    """transform.cc:109-144 (Transform::MetaApply) in stream order -> (shapes, nb_meta, the transforms with a default
    squeeze list filled in)."""
    filled = []
    for t in transforms:
        if t[0] == "rct":
            assert shapes[t[1]] == shapes[t[1] + 1] == shapes[t[1] + 2]
        elif t[0] == "palette":
            shapes, nb_meta = palette_meta(shapes, nb_meta, *t[1:5])
        else:
            steps = list(t[1]) or default_squeeze_steps([Chan(s[0], s[1]) for s in shapes], nb_meta)
            shapes, nb_meta = squeeze_meta(shapes, nb_meta, steps)
            t = ("squeeze", steps)
        filled.append(t)
    return shapes, nb_meta, filled


def inverse_transforms(chs, nb_meta, filled, wp=DEFAULT_WP, bit_depth=8, mis=(), branches=None):
    """The transforms undone last to first (encoding.cc:686-724, modular_image.cc:33-50 Image::undo_transforms) -> nb_meta."""
    mis = frozenset(mis)
    for t in reversed(filled):
        if t[0] == "rct":
            rct_inverse(chs, t[1], t[2], mis)
        elif t[0] == "palette":
            nb_meta = palette_inverse(chs, nb_meta, t[1], t[4], t[5], wp, bit_depth, mis)
        else:
            nb_meta = squeeze_inverse(chs, nb_meta, t[1], mis, branches)
    return nb_meta


# ---------------------------------------------------------------- the writer of one sub-bitstream
class BitWriter:
    def __init__(self):
        self.v, self.n = 0, 0

    def write(self, nbits, value):
        assert 0 <= value < (1 << nbits), (nbits, value)
        self.v |= value << self.n
        self.n += nbits

    def u32(self, value, *dists):
        """fields.h U32: a 2-bit selector, then the distribution's bits. dists: int = Val, (bits, offset) = BitsOffset."""
        for sel, d in enumerate(dists):
            if isinstance(d, int):
                if value == d:
                    self.write(2, sel)
                    return
            elif d[1] <= value < d[1] + (1 << d[0]):
                self.write(2, sel)
                self.write(d[0], value - d[1])
                return
        raise ValueError("no U32 selector holds %d" % value)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


BEGIN_C = ((3, 0), (6, 8), (10, 72), (13, 1096))
CFG = (4, 2, 0)  # the one hybrid-uint configuration of these streams: split_exponent, msb_in_token, lsb_in_token
LOG_ALPHA = 8


def hybrid_token(v, cfg=CFG):
    """-> (token, nbits, bits): the inverse of dec_ans.h:226-257."""
    split_exp, msb, lsb = cfg
    if v < (1 << split_exp):
        return v, 0, 0
    n = v.bit_length() - 1
    m = v - (1 << n)
    token = (1 << split_exp) + ((n - split_exp) << (msb + lsb)) + ((m >> (n - msb)) << lsb) + (m & ((1 << lsb) - 1))
    nbits = n - msb - lsb
    return token, nbits, (m >> lsb) & ((1 << nbits) - 1)


def flat_distribution(alphabet):
    """dec_ans.cc:58-191 ReadHistogram, is_flat: 4096 spread evenly, the remainder over the first symbols."""
    return [ANS_TAB // alphabet + (1 if i < ANS_TAB % alphabet else 0) for i in range(alphabet)]


ANS_TAB = ans_np.ANS_TAB_SIZE


def _inverse_alias(dist):
    """(symbol, offset within the symbol) -> state residue, by walking the decoder's table."""
    table = ans_np.alias_table(dist, LOG_ALPHA)
    log_entry = ans_np.ANS_LOG_TAB_SIZE - LOG_ALPHA
    inv = {}
    for res in range(ANS_TAB):
        idx, pos = res >> log_entry, res & ((1 << log_entry) - 1)
        cut, rv, f0, o1, f1 = table[idx]
        inv[(rv, o1 + pos) if pos >= cut else (idx, pos)] = res
    return inv


def write_histograms(bw, num_contexts, ctx_map, alphabets):
    """DecodeHistograms (dec_ans.cc:341-376) for: no LZ77, a simple context map, rANS at log_alpha 8, CFG per cluster, flat
    histograms of the given alphabet sizes."""
    bw.write(1, 0)  # lz77.enabled
    if num_contexts > 1:  # dec_context_map.cc:48-95: is_simple, bits per entry
        nbits = max(ctx_map).bit_length()
        assert nbits <= 3 and sorted(set(ctx_map)) == list(range(max(ctx_map) + 1))
        bw.write(1, 1)
        bw.write(2, nbits)
        for c in ctx_map:
            bw.write(nbits, c)
    bw.write(1, 0)  # use_prefix_code
    bw.write(2, LOG_ALPHA - 5)
    for _ in alphabets:  # DecodeUintConfig, dec_ans.cc:272-295
        bw.write(4, CFG[0])  # CeilLog2(log_alpha + 1) bits
        bw.write((CFG[0] + 1 - 1).bit_length(), CFG[1])
        bw.write((CFG[0] - CFG[1] + 1 - 1).bit_length(), CFG[2])
    for alphabet in alphabets:
        assert 1 <= alphabet <= 256
        bw.write(1, 0)  # not the one-or-two-symbols form
        bw.write(1, 1)  # is_flat
        v = alphabet - 1  # U8: 0, or 1 then three bits n and n bits
        if v == 0:
            bw.write(1, 0)
        else:
            n = v.bit_length() - 1
            bw.write(1, 1)
            bw.write(3, n)
            bw.write(n, v - (1 << n))


def write_tokens(bw, tokens, ctx_map, dists):
    """rANS-codes [(context, value)]: a reverse pass works out every state and which symbols make the decoder refill, then
    the 32-bit start state, each symbol's 16 refill bits and its extra bits go out in reading order. -> the bit position
    of the start state."""
    inv = [_inverse_alias(d) for d in dists]
    parts = [hybrid_token(v) for _, v in tokens]
    state = ans_np.ANS_SIGNATURE << 16
    refill = [None] * len(tokens)
    for i in range(len(tokens) - 1, -1, -1):
        cluster = ctx_map[tokens[i][0]]
        sym = parts[i][0]
        freq = dists[cluster][sym]
        if (state >> 20) >= freq:
            refill[i] = state & 0xFFFF
            state >>= 16
        state = ((state // freq) << ans_np.ANS_LOG_TAB_SIZE) + inv[cluster][(sym, state % freq)]
    begin = bw.n
    bw.write(32, state)
    for i, (_, nbits, bits) in enumerate(parts):
        if refill[i] is not None:
            bw.write(16, refill[i])
        bw.write(nbits, bits)
    return begin


def _alphabets(tokens, ctx_map, margin):
    top = [0] * (max(ctx_map) + 1)
    for ctx, v in tokens:
        top[ctx_map[ctx]] = max(top[ctx_map[ctx]], hybrid_token(v)[0])
    return [min(256, t + 1 + margin) for t in top]


def tree_tokens(tree):
    """dec_ma.cc:109-157: per node (context, value); contexts: 0 splitval, 1 property + 1, 2 predictor, 3 offset,
    4 multiplier log, 5 multiplier bits."""
    out = []
    for n in tree:
        if n[0] >= 0:
            out += [(1, n[0] + 1), (0, pack_signed(n[1]))]
        else:
            _, _, predictor, offset, multiplier = n
            mul_log = (multiplier & -multiplier).bit_length() - 1
            out += [(1, 0), (2, predictor), (3, pack_signed(offset)), (4, mul_log), (5, (multiplier >> mul_log) - 1)]
    return out


def write_transform(bw, t):
    if t[0] == "rct":
        bw.u32(0, 0, 1, 2, 3)
        bw.u32(t[1], *BEGIN_C)
        bw.u32(t[2], 6, (2, 0), (4, 2), (6, 10))
    elif t[0] == "palette":
        _, begin_c, num_c, nb_colors, nb_deltas, predictor = t
        bw.u32(1, 0, 1, 2, 3)
        bw.u32(begin_c, *BEGIN_C)
        bw.u32(num_c, 1, 3, 4, (13, 1))
        bw.u32(nb_colors, (8, 0), (10, 256), (12, 1280), (16, 5376))
        bw.u32(nb_deltas, 0, (8, 1), (10, 257), (16, 1281))
        bw.write(4, predictor)
    else:
        bw.u32(2, 0, 1, 2, 3)
        bw.u32(len(t[1]), 0, (4, 1), (6, 9), (8, 41))
        for horizontal, in_place, begin_c, num_c in t[1]:
            bw.write(1, int(horizontal))
            bw.write(1, int(in_place))
            bw.u32(begin_c, *BEGIN_C)
            bw.u32(num_c, 1, 2, 3, (4, 4))


def write_stream(tokens, tree, wp=None, transforms=(), per_leaf_clusters=False, margin=2):
    """One Modular sub-bitstream with its own tree (encoding.cc:554-724): the group header, the tree, the data code's
    histograms, the samples. tokens = tokenize(...) of the coded channels; wp None writes "default"; transforms as the
    stream carries them (a default squeeze as ("squeeze", [])). -> dict(data, data_bit (where the samples' ANS state
    begins), end_bit, ctx_map, dists (per cluster))."""
    bw = BitWriter()
    bw.write(1, 0)  # use_global_tree
    if wp is None:
        bw.write(1, 1)  # all_default
    else:
        bw.write(1, 0)
        for f in WP_FIELDS:
            bw.write(5, wp[f])
        for v in wp["w"]:
            bw.write(4, v)
    bw.u32(len(transforms), 0, 1, (4, 2), (8, 18))
    for t in transforms:
        write_transform(bw, t)
    tt = tree_tokens(tree)
    tree_alpha = _alphabets(tt, [0] * 6, margin)
    write_histograms(bw, 6, [0] * 6, tree_alpha)
    write_tokens(bw, tt, [0] * 6, [flat_distribution(a) for a in tree_alpha])
    n = num_leaves(tree)
    ctx_map = list(range(n)) if per_leaf_clusters else [0] * n
    assert n <= 8 or not per_leaf_clusters
    used = sorted(set(ctx for ctx, _ in tokens))
    if per_leaf_clusters:
        assert used == list(range(n)), "a cluster per leaf needs every leaf used"
    alphabets = _alphabets(tokens, ctx_map, margin)
    write_histograms(bw, n, ctx_map, alphabets)
    dists = [flat_distribution(a) for a in alphabets]
    data_bit = write_tokens(bw, tokens, ctx_map, dists)
    return dict(data=bw.bytes(), data_bit=data_bit, end_bit=bw.n, ctx_map=ctx_map, dists=dists)


def read_back(stream, shapes, tree, wp=DEFAULT_WP, stream_id=0, first_channel=0):
    """The samples of a written stream through ans_np.Reader and reconstruct(): -> (channels, the reader)."""
    code = ans_np.Code(False, LOG_ALPHA, stream["ctx_map"], [dict(cfg=CFG, table=d) for d in stream["dists"]])
    reader = ans_np.Reader(code, stream["data"], stream["data_bit"], len(stream["data"]) * 8)
    return reconstruct(reader.read, shapes, tree, wp, stream_id, first_channel), reader
