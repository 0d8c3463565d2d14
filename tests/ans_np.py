"""A plain reading of the rANS *decoder* for the entropy tests: alias tables (lib/jxl/ans_common.cc InitAliasTable,
ans_common.h:102-142 Lookup), the symbol read (dec_ans.h:170-197) and the hybrid-uint read (dec_ans.h:226-257), on an
LSB-first bit string. It shares nothing with the encoder under test: what that writes must come back through here token
for token, and the coder must end in its start state (dec_ans.h:222).

For the AC coefficient walk (tests/ac_walk_np.py) there is also a streaming reader, Reader.read(context), over a Code as a
decoder parsed it: a hybrid-uint configuration per cluster, rANS or prefix codes rebuilt canonically from their code
lengths (huffman_table.cc:64-146, dec_huffman.cc), and the LZ77 layer of dec_ans.h:287-353."""
import numpy as np

ANS_LOG_TAB_SIZE = 12
ANS_TAB_SIZE = 1 << ANS_LOG_TAB_SIZE
ANS_SIGNATURE = 0x13


class Bits:
    def __init__(self, data, nbits=None):
        self.v = int.from_bytes(bytes(data), "little")
        self.n = len(data) * 8 if nbits is None else int(nbits)
        self.pos = 0

    def read(self, k):
        if self.pos + k > self.n:
            raise ValueError("read past the end of the bit string (%d + %d > %d)" % (self.pos, k, self.n))
        r = (self.v >> self.pos) & ((1 << k) - 1)
        self.pos += k
        return r


def alias_table(distribution, log_alpha):
    """-> per table entry (cutoff, right_value, freq0, offsets1, freq1)."""
    dist = [int(x) for x in distribution]
    table_size = 1 << log_alpha
    while dist and dist[-1] == 0:
        dist.pop()
    if not dist:
        dist = [ANS_TAB_SIZE]
    assert len(dist) <= table_size and sum(dist) == ANS_TAB_SIZE, (len(dist), sum(dist))
    entry_size = ANS_TAB_SIZE >> log_alpha
    if ANS_TAB_SIZE in dist:
        sym = dist.index(ANS_TAB_SIZE)
        return [(0, sym, 0, entry_size * i, ANS_TAB_SIZE) for i in range(table_size)]
    cutoffs = [0] * table_size
    right = [0] * table_size
    offsets1 = [0] * table_size
    under, over = [], []
    for i, c in enumerate(dist):
        cutoffs[i] = c
        if c > entry_size:
            over.append(i)
        elif c < entry_size:
            under.append(i)
    under.extend(range(len(dist), table_size))
    while over:
        o = over.pop()
        u = under.pop()
        by = entry_size - cutoffs[u]
        cutoffs[o] -= by
        right[u] = o
        offsets1[u] = cutoffs[o]
        if cutoffs[o] < entry_size:
            under.append(o)
        elif cutoffs[o] > entry_size:
            over.append(o)
    out = []
    for i in range(table_size):
        if cutoffs[i] == entry_size:
            rv, o1, cut = i, 0, 0
        else:
            rv, o1, cut = right[i], offsets1[i] - cutoffs[i], cutoffs[i]
        f0 = dist[i] if i < len(dist) else 0
        f1 = dist[rv] if rv < len(dist) else 0
        out.append((cut, rv, f0, o1, f1))
    return out


def read_hybrid(br, token, split_exp, msb, lsb):
    split_token = 1 << split_exp
    if token < split_token:
        return token
    nbits = (split_exp - (msb + lsb) + ((token - split_token) >> (msb + lsb))) & 31
    low = token & ((1 << lsb) - 1)
    token >>= lsb
    bits = br.read(nbits)
    return ((((((1 << msb) | (token & ((1 << msb) - 1))) << nbits) | bits) << lsb) | low) & 0xFFFFFFFF


def decode(data, nbits, contexts, ctx_map, freqs, log_alpha, cfg=(4, 2, 0), prefix_bits=0):
    """Decodes len(contexts) tokens from the first `nbits` bits of `data`. freqs: [cluster][symbol] summing to 4096 each.
    Returns (prefix value, values); raises if the coder does not end in its start state, if bits are left over or missing,
    or if padding bits of the last byte are set."""
    br = Bits(data, nbits)
    total = len(bytes(data)) * 8
    assert nbits <= total and total - nbits < 8, (nbits, total)
    assert (int.from_bytes(bytes(data), "little") >> nbits) == 0, "padding bits are not zero"
    prefix = br.read(prefix_bits)
    tables = [alias_table(f, log_alpha) for f in freqs]
    log_entry = ANS_LOG_TAB_SIZE - log_alpha
    state = br.read(32)
    values = np.zeros(len(contexts), np.uint32)
    for i, ctx in enumerate(contexts):
        table = tables[ctx_map[ctx]]
        res = state & (ANS_TAB_SIZE - 1)
        idx, pos = res >> log_entry, res & ((1 << log_entry) - 1)
        cut, rv, f0, o1, f1 = table[idx]
        if pos >= cut:
            sym, off, freq = rv, o1 + pos, f1
        else:
            sym, off, freq = idx, pos, f0
        state = freq * (state >> ANS_LOG_TAB_SIZE) + off
        if state < (1 << 16):
            state = (state << 16) | br.read(16)
        values[i] = read_hybrid(br, sym, *cfg)
    if state != ANS_SIGNATURE << 16:
        raise ValueError("final state %#x" % state)
    if br.pos != nbits:
        raise ValueError("%d bits left" % (nbits - br.pos))
    return prefix, values


# ---------------------------------------------------------------- the streaming reader (dec_ans.h:162-353, dec_ans.cc:334-377)
LZ_WINDOW = 1 << 20  # dec_ans.h:105 kWindowSize


class ByteBits:
    """LSB-first bits [begin, end) of `data`; reading past `end` is an error (the reference zero-fills and fails at Close)."""

    def __init__(self, data, begin, end):
        self.d = bytes(data)
        self.pos, self.end = int(begin), int(end)

    def read(self, k):
        p = self.pos
        if p + k > self.end:
            raise ValueError("read past the end of the section (%d + %d > %d)" % (p, k, self.end))
        self.pos = p + k
        return (int.from_bytes(self.d[p >> 3:(p >> 3) + 8], "little") >> (p & 7)) & ((1 << k) - 1)


def canonical_prefix_code(lengths):
    """{(length, code read first bit first): symbol} of the canonical code with these lengths: codes are handed out by
    length, then by symbol (huffman_table.cc:64-146 sorts the symbols so; its table is indexed by the bit-reversed code,
    which is the same as reading the code's bits first to last). A code with one used symbol has no bits."""
    used = [i for i, n in enumerate(lengths) if n]
    if len(used) <= 1:
        return {(0, 0): used[0] if used else 0}
    out, code = {}, 0
    for n in range(1, max(lengths) + 1):
        for sym in used:
            if lengths[sym] == n:
                out[(n, code)] = sym
                code += 1
        code <<= 1
    if code != 1 << (max(lengths) + 1):
        raise ValueError("the code lengths do not fill the code space")
    return out


class Code:
    """An entropy code as a decoder parsed it: use_prefix, log_alpha, ctx_map (context -> cluster), per cluster cfg =
    (split_exponent, msb_in_token, lsb_in_token) and table = symbol frequencies (rANS) or code lengths (prefix), lz77 = None
    or dict(min_symbol, min_length, length_cfg, dist_ctx (clustered))."""

    def __init__(self, use_prefix, log_alpha, ctx_map, clusters, lz77=None):
        self.use_prefix, self.log_alpha, self.ctx_map, self.lz77 = bool(use_prefix), int(log_alpha), list(ctx_map), lz77
        self.cfg = [tuple(c["cfg"]) for c in clusters]
        if self.use_prefix:
            self.prefix = [canonical_prefix_code(c["table"]) for c in clusters]
        else:
            log_entry = ANS_LOG_TAB_SIZE - self.log_alpha
            self.lookup = []  # per cluster, per state residue: (symbol, offset, frequency) (ans_common.h:102-142 Lookup)
            for c in clusters:
                table = alias_table(c["table"], self.log_alpha)
                rows = []
                for res in range(ANS_TAB_SIZE):
                    idx, pos = res >> log_entry, res & ((1 << log_entry) - 1)
                    cut, rv, f0, o1, f1 = table[idx]
                    rows.append((rv, o1 + pos, f1) if pos >= cut else (idx, pos, f0))
                self.lookup.append(rows)


class Reader:
    """ANSSymbolReader on bits [begin, end) of `data`: Create reads the 32-bit state of a rANS code (dec_ans.cc:351-355);
    read(context) is ReadHybridUintClusteredInlined behind the context map. `copies` counts LZ77 copy commands."""

    def __init__(self, code, data, begin, end, distance_multiplier=0):
        assert distance_multiplier == 0, "special distances (dec_ans.h:141-145) are not read here: AC streams have none"
        self.c, self.br = code, ByteBits(data, begin, end)
        self.state = ANS_SIGNATURE << 16 if code.use_prefix else self.br.read(32)
        self.window = {} if code.lz77 else None  # position & mask -> value
        self.num_decoded = self.num_to_copy = self.copy_pos = self.copies = 0

    @property
    def pos(self):
        return self.br.pos

    def final_state_ok(self):
        return self.state == ANS_SIGNATURE << 16

    def _symbol(self, cluster):
        if self.c.use_prefix:
            table = self.c.prefix[cluster]
            if (0, 0) in table:
                return table[(0, 0)]
            n = code = 0
            while True:
                code, n = (code << 1) | self.br.read(1), n + 1
                if (n, code) in table:
                    return table[(n, code)]
                if n > 15:
                    raise ValueError("no such prefix code")
        sym, off, freq = self.c.lookup[cluster][self.state & (ANS_TAB_SIZE - 1)]
        state = freq * (self.state >> ANS_LOG_TAB_SIZE) + off
        if state < (1 << 16):
            state = (state << 16) | self.br.read(16)
        self.state = state
        return sym

    def _copy(self):
        r = self.window.get(self.copy_pos & (LZ_WINDOW - 1), 0)
        self.copy_pos += 1
        self.num_to_copy -= 1
        self.window[self.num_decoded & (LZ_WINDOW - 1)] = r
        self.num_decoded += 1
        return r

    def read(self, ctx):
        if not 0 <= ctx < len(self.c.ctx_map) - (1 if self.c.lz77 else 0):
            raise ValueError("context %d is beyond the context map" % ctx)
        cluster = self.c.ctx_map[ctx]
        lz = self.c.lz77
        if lz is None:
            return read_hybrid(self.br, self._symbol(cluster), *self.c.cfg[cluster])
        if self.num_to_copy > 0:
            return self._copy()
        token = self._symbol(cluster)
        if token >= lz["min_symbol"]:
            self.num_to_copy = read_hybrid(self.br, token - lz["min_symbol"], *lz["length_cfg"]) + lz["min_length"]
            distance = read_hybrid(self.br, self._symbol(lz["dist_ctx"]), *self.c.cfg[lz["dist_ctx"]]) + 1  # no special distances
            distance = min(distance, self.num_decoded, LZ_WINDOW)
            self.copy_pos = self.num_decoded - distance
            if distance == 0:  # nothing decoded yet: the copy reads zeros (dec_ans.h:323-328)
                self.window = {}
            self.copies += 1
            return self._copy()
        r = read_hybrid(self.br, token, *self.c.cfg[cluster])
        self.window[self.num_decoded & (LZ_WINDOW - 1)] = r
        self.num_decoded += 1
        return r
