"""A plain reading of the rANS *decoder* for the entropy tests: alias tables (lib/jxl/ans_common.cc InitAliasTable,
ans_common.h:102-142 Lookup), the symbol read (dec_ans.h:170-197) and the hybrid-uint read (dec_ans.h:226-257), on an
LSB-first bit string. It shares nothing with the encoder under test: what that writes must come back through here token
for token, and the coder must end in its start state (dec_ans.h:222)."""
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
