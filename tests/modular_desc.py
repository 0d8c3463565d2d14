"""Hand-made JxlHipModFrameDesc descriptors for tests/test_gpu_modular_np.py: ctypes mirrors of the structs of
include/jxl_amd_hip.h (tests/test_modular_np.py holds their layout against the header with a compiler) and a builder that
puts cases of tests/modular_cases.py into one frame. Everything a descriptor says comes from the reading (modular_np): the
bytes and the bit position of the sample data from its writer, the tree nodes and the weighted-predictor values as the case
states them, the alias entries from ans_np.alias_table packed as the header documents; rectangles, buffers and operations
are laid out here. Nothing of the product's front-end is asked."""
import ctypes
import struct

import numpy as np

import ans_np
import modular_np as M

u32, i32, vp = ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p


class TreeNode(ctypes.Structure):
    _fields_ = [("property", i32), ("splitval", i32), ("lchild", u32), ("rchild", u32), ("predictor", u32), ("offset", i32),
                ("multiplier", u32), ("pad", u32)]


class Code(ctypes.Structure):
    _fields_ = [("ctx_map", vp), ("ctx_map_size", u32), ("num_clusters", u32), ("use_prefix", u32), ("log_alpha", u32), ("alias", vp),
                ("uint_cfg", vp), ("prefix_table", vp), ("prefix_table_size", u32), ("prefix_offset", vp), ("lz77", u32),
                ("lz_min_symbol", u32), ("lz_min_length", u32), ("lz_len_cfg", u32), ("lz_dist_ctx", u32)]


class Rect(ctypes.Structure):
    _fields_ = [("buffer", u32), ("x0", u32), ("y0", u32), ("w", u32), ("h", u32), ("sig", u32)]


class Stream(ctypes.Structure):
    _fields_ = [("section", u32), ("bit_offset", u32), ("stream_id", u32), ("first_channel_index", u32), ("tree", u32), ("code", u32),
                ("first_rect", u32), ("num_rects", u32), ("wp", i32 * 11), ("uses_wp", u32), ("num_props", u32), ("dist_multiplier", u32),
                ("max_width", u32), ("num_samples", u32)]


class Buffer(ctypes.Structure):
    _fields_ = [("w", u32), ("h", u32)]


class Op(ctypes.Structure):
    _fields_ = [("kind", u32), ("buf", u32 * 6), ("ox", u32 * 6), ("oy", u32 * 6), ("w", u32), ("h", u32), ("param", u32), ("nb", u32),
                ("bit_depth", u32), ("level", u32), ("local", u32)]


class Splines(ctypes.Structure):
    _fields_ = [("num_segments", u32), ("num_row_segments", u32), ("segments", vp), ("row_start", vp), ("row_segments", vp)]


class Patches(ctypes.Structure):
    _fields_ = [("num_positions", u32), ("num_row_entries", u32), ("records", vp), ("row_start", vp), ("row_list", vp), ("slot_planes", vp * 4),
                ("slot_w", u32 * 4), ("slot_h", u32 * 4), ("uses_alpha", u32), ("premultiplied", u32), ("slot_alpha", vp * 4)]


class FrameDesc(ctypes.Structure):
    _fields_ = [("xsize", u32), ("ysize", u32), ("codestream", vp), ("section_offset", vp), ("section_size", vp), ("num_sections", u32),
                ("trees", vp), ("tree_size", vp), ("num_trees", u32), ("codes", vp), ("num_codes", u32), ("buffers", vp), ("num_buffers", u32),
                ("rects", vp), ("num_rects", u32), ("streams", vp), ("num_streams", u32), ("ops", vp), ("num_ops", u32),
                ("out_buffer", u32 * 4), ("num_color", u32), ("has_alpha", u32), ("bits", u32), ("alpha_bits", u32), ("splines", Splines),
                ("patches", Patches), ("xyb", u32), ("xyb_factor", ctypes.c_float * 3), ("opsin_inv", ctypes.c_float * 9),
                ("opsin_bias", ctypes.c_float * 3), ("linear_output", i32), ("color_target", vp)]


MIRRORS = {"JxlHipModTreeNode": TreeNode, "JxlHipModCode": Code, "JxlHipModRect": Rect, "JxlHipModStream": Stream, "JxlHipModBuffer": Buffer,
           "JxlHipModOp": Op, "JxlHipSplines": Splines, "JxlHipPatches": Patches, "JxlHipModFrameDesc": FrameDesc}


def pack_alias(dists):
    """num_clusters << log_alpha entries of 8 bytes: u8 cutoff, u8 right, u16 freq0, u16 offsets1, u16 freq1."""
    out = b""
    for d in dists:
        for cut, right, f0, o1, f1 in ans_np.alias_table(d, M.LOG_ALPHA):
            assert 0 <= o1 < 65536 and cut < 256 and right < 256
            out += struct.pack("<BBHHH", cut, right, f0, o1, f1)
    return out


class Frame:
    """Streams of cases in one frame. add() gives every channel of a case a buffer of its own (placed: a wider one, the
    rectangle at x0 in {1, 3}, y0 = 2) and plans the case's inverse transforms as operations local to the stream, one level
    per operation, so that operations of one level and kind of different streams share a launch. expect lists
    (label, buffer, x0, y0, the channel the reading says lies there)."""

    def __init__(self):
        self.data = b""
        self.sections, self.trees, self.codes, self.buffers, self.rects, self.streams, self.ops = [], [], [], [], [], [], []
        self.expect, self.end_bits, self.tables = [], [], {}
        self.out_buffer = self._buffer(4, 4)  # what the output kernel reads: zeros

    def _buffer(self, w, h):
        self.buffers.append((max(w, 1), max(h, 1)))
        return len(self.buffers) - 1

    def _channel(self, c, placed, k):
        if placed and c.hshift >= 0 and c.w and c.h:  # (a palette is always a whole buffer)
            x0, y0 = (1, 3)[k % 2], 2
            return dict(buffer=self._buffer(c.w + x0 + 2, c.h + y0 + 1), x0=x0, y0=y0, w=c.w, h=c.h, hs=c.hshift, vs=c.vshift)
        return dict(buffer=self._buffer(c.w, c.h), x0=0, y0=0, w=c.w, h=c.h, hs=c.hshift, vs=c.vshift)

    def _op(self, level, kind, chans, w, h, param=0, nb=0, bit_depth=0):
        self.ops.append(dict(kind=kind, buf=[c["buffer"] for c in chans], ox=[c["x0"] for c in chans], oy=[c["y0"] for c in chans], w=w, h=h,
                             param=param, nb=nb, bit_depth=bit_depth, level=level, local=1))
        return level + 1

    def add(self, case, placed=False):
        if case.name not in self.tables:  # streams of one case share its tree and code: one table set, one address
            self.tables[case.name] = len(self.trees)
            self.trees.append(case.tree)
            self.codes.append((case.stream["ctx_map"], case.stream["dists"]))
        table = self.tables[case.name]
        self.sections.append((len(self.data), len(case.stream["data"])))
        self.data += case.stream["data"]
        ch = [self._channel(c, placed, k) for k, c in enumerate(case.pre)]
        first_rect = len(self.rects)
        for c in ch:
            self.rects.append((c["buffer"], c["x0"], c["y0"], c["w"], c["h"], (c["hs"] + 2) * 64 + c["vs"] + 2))
        widths = [c["w"] for c in ch if c["w"] and c["h"]]
        self.streams.append(dict(section=len(self.sections) - 1, bit_offset=case.stream["data_bit"], stream_id=case.stream_id, first_channel_index=0,
                                 tree=table, code=table, first_rect=first_rect, num_rects=len(ch),
                                 wp=[case.wp_values[f] for f in M.WP_FIELDS] + list(case.wp_values["w"]), uses_wp=int(M.tree_uses_wp(case.tree)),
                                 num_props=M.tree_num_props(case.tree), dist_multiplier=max(widths), max_width=max(widths),
                                 num_samples=sum(c["w"] * c["h"] for c in ch)))
        self.end_bits.append(case.stream["end_bit"])
        level = 0
        for t in reversed(case.filled):  # the inverse transforms, last first, as jxl_amd_hip.h describes the operations
            if t[0] == "rct":
                a = ch[t[1]]
                if t[2]:
                    level = self._op(level, 0, ch[t[1]:t[1] + 3], a["w"], a["h"], param=t[2])
            elif t[0] == "palette":
                pal, c0 = ch[0], t[1] + 1
                idx, nb = ch[c0], ch[0]["h"]
                outs = [idx] + [dict(idx, buffer=self._buffer(idx["w"], idx["h"]), x0=0, y0=0) for _ in range(nb - 1)]
                level = self._op(level, 1, [pal, idx] + outs, idx["w"], idx["h"], param=pal["w"], nb=nb, bit_depth=min(case.bit_depth, 24))
                ch[c0:c0 + 1] = outs
                del ch[0]
            else:
                for horizontal, in_place, begin_c, num_c in reversed(t[1]):
                    end = begin_c + num_c
                    first_res = end if in_place else len(ch) + begin_c - end
                    for c in range(begin_c, end):
                        a, r = ch[c], ch[first_res + c - begin_c]
                        if (r["w"] if horizontal else r["h"]) == 0:  # nothing to interleave: the averages are the channel
                            ch[c] = dict(a, hs=a["hs"] - 1) if horizontal else dict(a, vs=a["vs"] - 1)
                            continue
                        w, h = (a["w"] + r["w"], a["h"]) if horizontal else (a["w"], a["h"] + r["h"])
                        out = dict(buffer=self._buffer(w, h), x0=0, y0=0, w=w, h=h, hs=a["hs"] - (1 if horizontal else 0),
                                   vs=a["vs"] - (0 if horizontal else 1))
                        if w and h:
                            level = self._op(level, 2 if horizontal else 3, [a, r, out], w, h)
                        ch[c] = out
                    del ch[first_res:first_res + num_c]
        want = case.final if case.filled else case.pre
        assert [(c["w"], c["h"], c["hs"], c["vs"]) for c in ch] == [c.shape() for c in want], case.name
        for k, (c, chan) in enumerate(zip(ch, want)):
            self.expect.append(("%s stream %d channel %d" % (case.name, len(self.streams) - 1, k), c["buffer"], c["x0"], c["y0"], chan))

    def descriptor(self):
        """-> (FrameDesc, the objects its pointers need alive)"""
        keep = []

        def array(ctype, values):
            a = (ctype * max(len(values), 1))(*values)
            keep.append(a)
            return a

        d = FrameDesc()
        d.xsize = d.ysize = 4
        data = array(ctypes.c_uint8, list(self.data))
        d.codestream = ctypes.addressof(data)
        d.section_offset = ctypes.addressof(array(ctypes.c_uint64, [s[0] for s in self.sections]))
        d.section_size = ctypes.addressof(array(u32, [s[1] for s in self.sections]))
        d.num_sections = len(self.sections)
        tree_arrays = []
        for tree in self.trees:
            nodes = []
            for n in tree:
                if n[0] >= 0:
                    nodes.append(TreeNode(n[0], n[1], n[2], n[3], 0, 0, 1, 0))
                else:
                    nodes.append(TreeNode(-1, 0, n[1], 0, n[2], n[3], n[4], 0))
            tree_arrays.append(array(TreeNode, nodes))
        d.trees = ctypes.addressof(array(vp, [ctypes.addressof(t) for t in tree_arrays]))
        d.tree_size = ctypes.addressof(array(u32, [len(t) for t in self.trees]))
        d.num_trees = d.num_codes = len(self.trees)
        codes = []
        for ctx_map, dists in self.codes:
            k = Code()
            k.ctx_map = ctypes.addressof(array(ctypes.c_uint8, list(ctx_map)))
            k.ctx_map_size, k.num_clusters, k.use_prefix, k.log_alpha = len(ctx_map), len(dists), 0, M.LOG_ALPHA
            alias = pack_alias(dists)
            assert len(alias) == (len(dists) << M.LOG_ALPHA) * 8
            k.alias = ctypes.addressof(array(ctypes.c_uint8, list(alias)))
            k.uint_cfg = ctypes.addressof(array(u32, [M.CFG[0] | M.CFG[1] << 8 | M.CFG[2] << 16] * len(dists)))
            codes.append(k)
        d.codes = ctypes.addressof(array(Code, codes))
        d.buffers = ctypes.addressof(array(Buffer, [Buffer(w, h) for w, h in self.buffers]))
        d.num_buffers = len(self.buffers)
        d.rects = ctypes.addressof(array(Rect, [Rect(*r) for r in self.rects]))
        d.num_rects = len(self.rects)
        streams = []
        for s in self.streams:
            q = Stream()
            for name, v in s.items():
                setattr(q, name, (i32 * 11)(*v) if name == "wp" else v)
            streams.append(q)
        d.streams = ctypes.addressof(array(Stream, streams))
        d.num_streams = len(streams)
        ops = []
        for o in self.ops:
            q = Op()
            for name, v in o.items():
                setattr(q, name, (u32 * 6)(*(list(v) + [0] * (6 - len(v)))) if isinstance(v, list) else v)
            ops.append(q)
        d.ops = ctypes.addressof(array(Op, ops))
        d.num_ops = len(ops)
        d.out_buffer = (u32 * 4)(self.out_buffer, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
        d.num_color, d.has_alpha, d.bits, d.alpha_bits = 1, 0, 8, 8
        return d, keep

    def check(self, ctx):
        """Every expected channel against its rectangle of the downloaded buffer, exactly."""
        for label, buffer, x0, y0, chan in self.expect:
            w, h = self.buffers[buffer]
            got = ctx.modular_buffer(buffer, shape=(h, w))[y0:y0 + chan.h, x0:x0 + chan.w]
            want = np.array(chan.d, np.int64).reshape(chan.h, chan.w)
            assert np.array_equal(got, want), "%s: %d of %d samples differ" % (label, int((got != want).sum()), want.size)
