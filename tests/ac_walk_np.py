"""A plain reading of the AC coefficient walk, both ways, written from the reference's text alone:

  decode_group    dec_group.cc:470-542 (DecodeACVarBlock) driven as dec_group.cc:549-639 drives it (StartRow / LoadBlock /
                  Init: the selector bits, the context offset, one reader, one non-zero map and one shift per pass, the
                  subsampled grids) inside the block loop of dec_group.cc:275-359;
  tokenize_group  enc_entropy_coder.cc:153-255 (TokenizeCoefficients), for the single-pass form.

They share only the small context functions: entropy_coder.h:25-35 (PredictFromTopAndLeft), ac_context.h:25-143
(ZeroDensityContext, BlockCtxMap::Context with its c < 2 ? c ^ 1 : 2 channel index, NonZeroContext,
ZeroDensityContextsOffset, NumACContexts) and coeff_order.h:26-47 (kStrategyOrder, CoeffOrderOffset). The constants come from
tests/golden/ref_constant_tables.json, the symbol reader from tests/ans_np.py, ZeroDensityContext from
tests/host_tables_np.py. Nothing here imports the product or the oracle: the tables a decoder parsed (histograms, context
maps, coded orders, the block context map) are inputs.

MISREADINGS names the ways this walk has been or could be misread; each is a switch (`mis`), off unless named, and
tests/test_ac_walk.py shows that each one makes a listed case fail."""
import json
import os

import numpy as np

import ans_np
from host_tables_np import zero_density_context

_T = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_constant_tables.json")))
FREQ_CTX, NNZ_CTX = _T["kCoeffFreqContext"], _T["kCoeffNumNonzeroContext"]
DEFAULT_CTX_MAP = list(_T["kDefaultCtxMap"])
STRATEGY_ORDER = _T["kStrategyOrder"]
COVERED_X, COVERED_Y = _T["covered_blocks_x"], _T["covered_blocks_y"]
NUM_ORDERS = 13            # coeff_order_fwd.h:25
NON_ZERO_BUCKETS = 37      # ac_context.h:27
ZERO_DENSITY_COUNT = 458   # ac_context.h:45
CHANNEL_ORDER = (1, 0, 2)  # dec_group.cc:569, enc_entropy_coder.cc:201: Y, X, B
GROUP_BLOCKS = 32

MISREADINGS = (
    "qf_frame_column",           # quant field taken at the frame's block column instead of the channel's
    "predict_default_0",         # predictor default 0 instead of 32
    "predict_no_round",          # (top + left) / 2 without the + 1
    "nz_not_divided",            # the non-zero map not divided by the covered blocks
    "nz_one_cell",               # the non-zero map written to one cell only
    "prev_constant",             # prev started at a constant
    "k_not_shifted",             # k not shifted by log2_covered
    "channels_xyb",              # channels walked X, Y, B
    "bctx_channel_not_swapped",  # the block-context channel index not swapped
    "no_selector_offset",        # the selector's context offset left out
    "zero_density_base",         # the zero-density base not 37 * num_ctxs + 458 * block_ctx
    "predict_across_group_edge",  # the predictor reading across a group edge
    "ignore_pass_shift",         # the pass shift ignored
    "subsampled_counts_on_frame_grid",  # a subsampled channel's counts kept on the frame's grid
)


def coeff_order_offset(ord_, c):
    """CoeffOrderOffset (coeff_order.h:28-37): the orders of (bucket, channel) follow each other, each as long as the
    largest transform of its bucket; kCoeffOrderOffset is the running sum of the covered blocks."""
    size = [0] * NUM_ORDERS
    for s, o in enumerate(STRATEGY_ORDER):
        size[o] = max(size[o], COVERED_X[s] * COVERED_Y[s])
    return 64 * (3 * sum(size[:ord_]) + (c * size[ord_] if c else 0))  # (ord_ = 13, c = 0: the end, kCoeffOrderLimit)


def num_ac_contexts(num_ctxs):
    return num_ctxs * (NON_ZERO_BUCKETS + ZERO_DENSITY_COUNT)


def predict_from_top_and_left(top, row, x, mis=()):
    """entropy_coder.h:25-35 with default_val = 32; top is None in the first row of the map."""
    if x == 0:
        return (0 if "predict_default_0" in mis else 32) if top is None else int(top[x])
    if top is None:
        return int(row[x - 1])
    return (int(top[x]) + int(row[x - 1]) + (0 if "predict_no_round" in mis else 1)) // 2


def block_context(bctx, dc_idx, qf, ord_, c, mis=()):
    """BlockCtxMap::Context (ac_context.h:101-111)."""
    qf_idx = sum(1 for t in bctx["qf_thresholds"] if qf > t)
    idx = c if "bctx_channel_not_swapped" in mis else (c ^ 1 if c < 2 else 2)
    idx = idx * NUM_ORDERS + ord_
    idx = idx * (len(bctx["qf_thresholds"]) + 1) + qf_idx
    idx = idx * bctx["num_dc_ctxs"] + dc_idx
    return bctx["ctx_map"][idx]


def non_zero_context(bctx, non_zeros, block_ctx):
    """ac_context.h:134-143."""
    non_zeros = min(non_zeros, 64)
    ctx = non_zeros if non_zeros < 8 else 4 + non_zeros // 2
    return ctx * bctx["num_ctxs"] + block_ctx


def zero_density_contexts_offset(bctx, block_ctx, mis=()):
    """ac_context.h:114-117."""
    if "zero_density_base" in mis:
        return bctx["num_ctxs"] * NON_ZERO_BUCKETS + 474 * block_ctx  # (kZeroDensityContextLimit in the place of ..Count)
    return bctx["num_ctxs"] * NON_ZERO_BUCKETS + ZERO_DENSITY_COUNT * block_ctx


def _zdc(nzeros, k, log2c, prev, mis):
    if "k_not_shifted" in mis:
        covered = 1 << log2c
        return (NNZ_CTX[((nzeros + covered - 1) >> log2c) & 63] + FREQ_CTX[k & 63]) * 2 + prev
    return zero_density_context(nzeros, k, log2c, prev, FREQ_CTX, NNZ_CTX)


class _NzMap:
    """One channel's non-zero counts of one pass: GroupDecCache::num_nzeroes, a 32 x 32 map per group whose first row has no
    row above it (dec_group.cc:556-560). `frame` = (map of the whole frame, row, column of this group's corner in it) is the
    misreading that lets the predictor see the neighbouring groups."""

    def __init__(self, frame=None):
        if frame is None:
            self.m, self.y0, self.x0 = np.zeros((GROUP_BLOCKS, GROUP_BLOCKS), np.int64), 0, 0
        else:
            self.m, self.y0, self.x0 = frame

    def rows(self, y):
        """(row above or None, this row, the column of the group's first block in them)."""
        y += self.y0
        return (self.m[y - 1] if y else None), self.m[y], self.x0


def _group_rect(group, xsize_blocks, ysize_blocks):
    xg = -(-xsize_blocks // GROUP_BLOCKS)
    bx0, by0 = (group % xg) * GROUP_BLOCKS, (group // xg) * GROUP_BLOCKS
    return bx0, by0, min(GROUP_BLOCKS, xsize_blocks - bx0), min(GROUP_BLOCKS, ysize_blocks - by0)


def make_codes(tables):
    """One ans_np.Code per pass from the tables as parsed (oracle/jxlo.py Decoded.ac_tables documents the dict)."""
    return [ans_np.Code(p["use_prefix"], p["log_alpha"], p["ctx_map"], p["clusters"], p["lz77"]) for p in tables["passes"]]


def decode_group(tables, data, group, acs, quant, quant_dc, codes=None, mis=(), frame_nz=None):
    """The AC coefficients of one group from the bytes of its sections.
      tables    as parsed (see make_codes); sections[pass][group][0] is the first bit of the walk in `data`, [1] and [2] the
                byte offset and size of the section that holds it
      acs       [ysize_blocks][xsize_blocks] (strategy << 1) | first-block bit; quant: the raw quant field; quant_dc: the
                DC-derived context of every block
    Returns dict: coeffs int32 [3][65536] (block-contiguous, the natural layout, value << shift added over the passes:
    dec_group.cc:337, 359, 524-529), last[pass] = [varblock][3] scan position behind the last coefficient read (0 where none
    was), end_bits[pass] = the bit of `data` behind the walk, tokens[pass] = the (context, value) pairs read, ctx_offset[pass] = the selected histogram set's first context, and what the
    tests' conditions ask about: predicted (set of predicted counts), dense / sparse (blocks on either side of
    nzeros > size / 16), qf_column_differs (blocks whose quant-field bucket at the channel's column is not the one at the
    frame's column), copies (LZ77 copy commands).
    Raises ValueError on nzeros > size - covered, on nzeros != 0 at a block's end, on a bad final state and on a read past
    the section."""
    mis = frozenset(mis)
    assert mis <= set(MISREADINGS), mis - set(MISREADINGS)
    acs = np.asarray(acs)
    yb, xb = acs.shape
    quant, quant_dc = np.asarray(quant).reshape(yb, xb), np.asarray(quant_dc).reshape(yb, xb)
    bx0, by0, gw, gh = _group_rect(group, xb, yb)
    bctx, hshift, vshift = tables["bctx"], tables["hshift"], tables["vshift"]
    num_passes = tables["num_passes"]
    codes = codes or make_codes(tables)
    # Init (dec_group.cc:616-631): per pass the selector, the context offset, the reader
    selector_bits = (tables["num_histograms"] - 1).bit_length()  # CeilLog2Nonzero(num_histograms), dec_group.cc:718-719
    readers, ctx_offset, shifts = [], [], []
    for p in range(num_passes):
        start, sec_off, sec_size = tables["sections"][p][group][:3]
        sel = ans_np.ByteBits(data, start, (sec_off + sec_size) * 8)
        cur = sel.read(selector_bits)
        if cur >= tables["num_histograms"]:
            raise ValueError("invalid histogram selector")
        ctx_offset.append(0 if "no_selector_offset" in mis else cur * num_ac_contexts(bctx["num_ctxs"]))
        readers.append(ans_np.Reader(codes[p], data, sel.pos, (sec_off + sec_size) * 8))
        shifts.append(0 if "ignore_pass_shift" in mis else tables["passes"][p]["shift"])
    if frame_nz is not None:
        assert "predict_across_group_edge" in mis
        nz = [[_NzMap((frame_nz[p][c], by0 >> vshift[c], bx0 >> hshift[c])) for c in range(3)] for p in range(num_passes)]
    else:
        nz = [[_NzMap() for c in range(3)] for p in range(num_passes)]
    coeffs = np.zeros((3, 65536), np.int64)
    last = [[] for _ in range(num_passes)]
    tokens = [[] for _ in range(num_passes)]
    predicted_seen, dense, sparse, qf_differs = set(), 0, 0, 0
    offset = 0
    channels = (0, 1, 2) if "channels_xyb" in mis else CHANNEL_ORDER
    for by in range(gh):
        for bx in range(gw):
            a = int(acs[by0 + by, bx0 + bx])
            if not a & 1:  # dec_group.cc:325
                continue
            s = a >> 1
            cx, cy = COVERED_X[s], COVERED_Y[s]
            covered = cx * cy
            log2c = covered.bit_length() - 1
            size = covered * 64
            ord_ = STRATEGY_ORDER[s]
            for p in range(num_passes):
                last[p].append([0, 0, 0])
            for c in channels:  # LoadBlock, dec_group.cc:569-590
                sbx, sby = bx >> hshift[c], by >> vshift[c]
                if (sbx << hshift[c]) != bx or (sby << vshift[c]) != by:
                    continue
                # qf_row = rect.ConstRow(*qf, by) indexed by the channel's column (dec_group.cc:551, 492 with bx = sbx at :585);
                # qdc_row by the frame's (lbx)
                qf_here = int(quant[by0 + by, bx0 + ((bx if "qf_frame_column" in mis else sbx))])
                qf_idx = lambda v: sum(1 for t in bctx["qf_thresholds"] if v > t)
                if qf_idx(int(quant[by0 + by, bx0 + sbx])) != qf_idx(int(quant[by0 + by, bx0 + bx])):
                    qf_differs += 1
                block_ctx = block_context(bctx, int(quant_dc[by0 + by, bx0 + bx]), qf_here, ord_, c, mis)
                nx, ny = (bx, by) if "subsampled_counts_on_frame_grid" in mis else (sbx, sby)
                order = None
                for p in range(num_passes):  # DecodeACVarBlock
                    rd, off, out = readers[p], ctx_offset[p], tokens[p]
                    top, row, x0 = nz[p][c].rows(ny)
                    predicted = predict_from_top_and_left(top, row, x0 + nx, mis)  # (x0 != 0 only in the frame-wide misreading)
                    predicted_seen.add(predicted)
                    order = tables["passes"][p]["orders"][coeff_order_offset(ord_, c):]
                    nzero_ctx = non_zero_context(bctx, predicted, block_ctx) + off
                    nzeros = rd.read(nzero_ctx)
                    out.append((nzero_ctx, nzeros))
                    if nzeros > size - covered:
                        raise ValueError("nzeros %d too large for %d blocks" % (nzeros, covered))
                    cell = nzeros if "nz_not_divided" in mis else (nzeros + covered - 1) >> log2c
                    m, my, mx = nz[p][c].m, nz[p][c].y0 + ny, nz[p][c].x0 + nx
                    if "nz_one_cell" in mis:
                        m[my, mx] = cell
                    else:
                        m[my:my + COVERED_Y[s], mx:mx + COVERED_X[s]] = cell  # (not the canonical dimensions: dec_group.cc:503-508)
                    histo_offset = off + zero_density_contexts_offset(bctx, block_ctx, mis)
                    if nzeros > size // 16:
                        prev, dense = 0, dense + 1
                    else:
                        prev, sparse = 1, sparse + 1
                    if "prev_constant" in mis:
                        prev = 1
                    k, shift = covered, shifts[p]
                    base = offset
                    while k < size and nzeros != 0:
                        ctx = histo_offset + _zdc(nzeros, k, log2c, prev, mis)
                        u = rd.read(ctx)
                        out.append((ctx, u))
                        magnitude, neg_sign = u >> 1, (~u) & 1
                        coeffs[c, base + order[k]] += (-(magnitude + 1) if neg_sign == 0 else magnitude) << shift  # m ^ (neg - 1)
                        prev = 1 if u else 0
                        nzeros -= prev
                        k += 1
                    if nzeros != 0:
                        raise ValueError("nzeros at end of block is %d, should be 0: block (%d, %d), channel %d" % (nzeros, bx, by, c))
                    last[p][-1][c] = k if k > covered else 0
            offset += size
    end_bits = []
    for p in range(num_passes):
        if not readers[p].final_state_ok():
            raise ValueError("pass %d: the coder does not end in its start state" % p)
        end_bits.append(readers[p].pos)
    lim = np.iinfo(np.int32)
    assert coeffs.min(initial=0) >= lim.min and coeffs.max(initial=0) <= lim.max
    return dict(coeffs=coeffs.astype(np.int32), last=[np.array(x, np.int64).reshape(-1, 3) for x in last], end_bits=end_bits,
                tokens=tokens, ctx_offset=ctx_offset, predicted=predicted_seen, dense=dense, sparse=sparse, qf_column_differs=qf_differs,
                copies=sum(r.copies for r in readers), used=offset)


def decode_frame(tables, data, acs, quant, quant_dc, mis=()):
    """decode_group over every group of the frame, in order: a list of its results."""
    mis = frozenset(mis)
    yb, xb = np.asarray(acs).shape
    codes = make_codes(tables)
    frame_nz = None
    if "predict_across_group_edge" in mis:
        frame_nz = [[np.zeros((yb + GROUP_BLOCKS, xb + GROUP_BLOCKS), np.int64) for _ in range(3)] for _ in range(tables["num_passes"])]
    return [decode_group(tables, data, g, acs, quant, quant_dc, codes, mis, frame_nz) for g in range(tables["num_groups"])]


def pack_signed(v):
    """PackSigned (pack_signed.h)."""
    return (v << 1) if v >= 0 else (((~v) << 1) | 1)


def tokenize_group(coeffs, group, acs, quant, quant_dc, orders, bctx, hshift=(0, 0, 0), vshift=(0, 0, 0), ctx_offset=0, mis=(),
                   dense_channels=False):
    """TokenizeCoefficients (enc_entropy_coder.cc:153-255) on one group: the (context, value) pairs of the single-pass form, in
    bitstream order, with `ctx_offset` (the group's histogram set times NumACContexts: enc_frame.cc adds it when it writes)
    added to every context.
      coeffs  [3][65536] of the group, block-contiguous in the natural layout. Every channel's block sits at the offset the
              frame's varblocks give it (the decoder's layout, dec_group.cc:337, 359); dense_channels: a subsampled channel's
              blocks follow each other instead (the encoder's own offset[c], enc_entropy_coder.cc:168, 240)
      orders  as the reference lays them out: the order of (bucket, channel) at coeff_order_offset(bucket, channel)
      quant_dc may be None (every block in DC context 0)."""
    mis = frozenset(mis)
    assert mis <= set(MISREADINGS), mis - set(MISREADINGS)
    acs = np.asarray(acs)
    yb, xb = acs.shape
    quant = np.asarray(quant).reshape(yb, xb)
    quant_dc = np.zeros((yb, xb), np.int64) if quant_dc is None else np.asarray(quant_dc).reshape(yb, xb)
    bx0, by0, gw, gh = _group_rect(group, xb, yb)
    nz = [np.zeros((GROUP_BLOCKS, GROUP_BLOCKS), np.int64) for _ in range(3)]  # tmp_num_nzeroes
    out = []
    offset = [0, 0, 0]
    channels = (0, 1, 2) if "channels_xyb" in mis else CHANNEL_ORDER
    for by in range(gh):
        for bx in range(gw):
            a = int(acs[by0 + by, bx0 + bx])
            if not a & 1:
                continue
            s = a >> 1
            covered = COVERED_X[s] * COVERED_Y[s]
            log2c = covered.bit_length() - 1
            size = covered * 64
            ord_ = STRATEGY_ORDER[s]
            for c in channels:
                sbx, sby = bx >> hshift[c], by >> vshift[c]
                if (sbx << hshift[c]) != bx or (sby << vshift[c]) != by:
                    continue
                block = coeffs[c][offset[c]:offset[c] + size]
                order = orders[coeff_order_offset(ord_, c):coeff_order_offset(ord_, c) + size]
                # NumNonZeroExceptLLF / NumNonZero8x8ExceptDC (enc_entropy_coder.cc:46-145): everything outside the cx x cy
                # corner of the canonical layout, which the order lists first (k < covered)
                values = [int(block[order[k]]) for k in range(covered, size)]
                nzeros = sum(1 for v in values if v != 0)
                nx, ny = (bx, by) if "subsampled_counts_on_frame_grid" in mis else (sbx, sby)
                cell = nzeros if "nz_not_divided" in mis else (nzeros + covered - 1) >> log2c
                top = nz[c][ny - 1] if ny else None
                predicted = predict_from_top_and_left(top, nz[c][ny], nx, mis)
                if "nz_one_cell" in mis:
                    nz[c][ny, nx] = cell
                else:
                    nz[c][ny:ny + COVERED_Y[s], nx:nx + COVERED_X[s]] = cell
                qf_here = int(quant[by0 + by, bx0 + (bx if "qf_frame_column" in mis else sbx)])  # row_qf[sbx[c]], :220
                block_ctx = block_context(bctx, int(quant_dc[by0 + by, bx0 + bx]), qf_here, ord_, c, mis)
                out.append((ctx_offset + non_zero_context(bctx, predicted, block_ctx), nzeros))
                histo_offset = ctx_offset + zero_density_contexts_offset(bctx, block_ctx, mis)
                prev = 0 if nzeros > size // 16 else 1
                if "prev_constant" in mis:
                    prev = 1
                k = covered
                while k < size and nzeros != 0:
                    coeff = values[k - covered]
                    out.append((histo_offset + _zdc(nzeros, k, log2c, prev, mis), pack_signed(coeff)))
                    prev = 1 if coeff != 0 else 0
                    nzeros -= prev
                    k += 1
                assert nzeros == 0
                if dense_channels:
                    offset[c] += size
            if not dense_channels:
                offset = [offset[0] + size] * 3
    return out
