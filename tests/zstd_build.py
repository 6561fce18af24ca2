"""A hand encoder for Zstandard compressed blocks and a plain model of what
they decode to, written from RFC 8878 alone: nothing here comes from pqgpu,
pqg_zstd.h or the host model, so a table or a rule that is wrong there is not
wrong here in the same way.

The encoder writes what it is told, valid or not: sequence tables in any of
the four modes with any normalized count, literals sections of every type and
size format, Huffman trees described by direct or FSE-compressed weights.
FrameB builds one frame block by block while the plain model (Plain) follows
the output and the repeat offsets, so a generator always knows which offsets
are legal; expand() is the same model over a frame's recorded description."""
import random

import zstd_util as Z

# ---- code tables (RFC 8878 3.1.1.3.2.1.1): extra bits per code, baselines cumulative
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def _bases(bits, first):
    out, b = [], first
    for k in bits:
        out.append(b)
        b += 1 << k
    return out


LL_BASE = _bases(LL_BITS, 0)
ML_BASE = _bases(ML_BITS, 3)
assert len(LL_BASE) == 36 and LL_BASE[16] == 16 and LL_BASE[24] == 48 and LL_BASE[25] == 64 and LL_BASE[35] == 65536
assert len(ML_BASE) == 53 and ML_BASE[32] == 35 and ML_BASE[42] == 99 and ML_BASE[43] == 131 and ML_BASE[52] == 65539
MAX_SYM = {"ll": 35, "of": 31, "ml": 52}
MAX_LOG = {"ll": 9, "of": 8, "ml": 9}

# ---- default distributions (RFC 8878 3.1.1.3.2.2)
DEFAULT = {
    "ll": (6, [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1,
               -1, -1, -1, -1]),
    "of": (5, [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]),
    "ml": (6, [1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
               1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1]),
}
for _log, _n in DEFAULT.values():
    assert sum(abs(c) for c in _n) == 1 << _log


def ll_code(v):
    c = max(i for i in range(36) if LL_BASE[i] <= v)
    assert v - LL_BASE[c] < 1 << LL_BITS[c]
    return c, v - LL_BASE[c], LL_BITS[c]


def ml_code(v):
    c = max(i for i in range(53) if ML_BASE[i] <= v)
    assert v - ML_BASE[c] < 1 << ML_BITS[c]
    return c, v - ML_BASE[c], ML_BITS[c]


def of_code(ofv):
    """ofv: the offset value, 1..3 a repeat code, else offset + 3."""
    c = ofv.bit_length() - 1
    return c, ofv - (1 << c), c


# ---- bit streams
def backward_bits(fields):
    """fields: (value, bits) in the order the decoder reads them.  The leading 1 is the padding marker."""
    s = "1" + "".join(format(v, "0%db" % k) for v, k in fields if k)
    for v, k in fields:
        assert 0 <= v < 1 << k, (v, k)
    return int(s, 2).to_bytes((len(s) + 7) // 8, "little")


class _Fwd:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, k):
        assert 0 <= v < 1 << k
        self.acc |= v << self.n
        self.n += k

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


# ---- FSE
class Fse:
    """The decoding table of a normalized count (RFC 8878 4.1.1): per state (symbol, nbits, base)."""

    def __init__(self, norm, log):
        size = 1 << log
        assert sum(abs(c) for c in norm) == size, (sum(abs(c) for c in norm), size)
        sym, high = [0] * size, size
        for s, c in enumerate(norm):
            if c == -1:
                high -= 1
                sym[high] = s
        pos, step = 0, (size >> 1) + (size >> 3) + 3
        for s, c in enumerate(norm):
            for _ in range(max(c, 0)):
                sym[pos] = s
                pos = (pos + step) & (size - 1)
                while pos >= high:
                    pos = (pos + step) & (size - 1)
        assert pos == 0
        nxt = [1 if c == -1 else c for c in norm]
        self.log, self.ent, self.by_sym = log, [], {}
        for i in range(size):
            s = sym[i]
            x = nxt[s]
            nxt[s] += 1
            nb = log - (x.bit_length() - 1)
            self.ent.append((s, nb, (x << nb) - size))
            self.by_sym.setdefault(s, []).append(i)

    @classmethod
    def rle(cls, s):
        t = cls.__new__(cls)
        t.log, t.ent, t.by_sym = 0, [(s, 0, 0)], {s: [0]}
        return t

    def states(self, syms, rng):
        """The state of every symbol, chosen backwards: the last takes any state of its symbol, symbol i the
        one state of its symbol whose range holds state i + 1."""
        st = [0] * len(syms)
        st[-1] = rng.choice(self.by_sym[syms[-1]])
        for i in range(len(syms) - 2, -1, -1):
            nx = st[i + 1]
            hit = [q for q in self.by_sym[syms[i]] if self.ent[q][2] <= nx < self.ent[q][2] + (1 << self.ent[q][1])]
            assert len(hit) == 1, (syms[i], nx, hit)
            st[i] = hit[0]
        return st

    def update(self, frm, to):
        """The bits that take state frm to state to."""
        _, nb, base = self.ent[frm]
        return to - base, nb


def write_ncount(norm, log):
    """The normalized-count header.  norm ends where the decoder's total reaches 2^log; it is written as given."""
    w = _Fwd()
    w.put(log - 5, 4)
    remaining, s = 1 << log, 0
    while s < len(norm):
        nb = (remaining + 1).bit_length()
        lower = (1 << (nb - 1)) - 1
        threshold = (1 << nb) - 1 - (remaining + 1)
        v = norm[s] + 1
        assert 0 <= v <= remaining + 1, "a value the header cannot hold"
        if v < threshold:
            w.put(v, nb - 1)
        elif v <= lower:
            w.put(v, nb)
        else:
            w.put(v + threshold, nb)
        remaining -= abs(norm[s])
        s += 1
        if norm[s - 1] == 0:
            r = 0
            while s + r < len(norm) and norm[s + r] == 0:
                r += 1
            s += r
            while r >= 3:
                w.put(3, 2)
                r -= 3
            w.put(r, 2)
    return w.bytes()


def make_norm(used, log, rng, less1=(), extra=(), cap=None):
    """A valid count over the symbols used + extra + less1 (those of less1 get -1); cap: the most one symbol gets."""
    syms = sorted(set(used) | set(extra) | set(less1))
    size = 1 << log
    assert 2 <= len(syms) <= size
    norm = [0] * (syms[-1] + 1)
    for s in syms:
        norm[s] = -1 if s in less1 else 1
    free = [s for s in syms if s not in less1]
    assert free
    left = size - len(syms)
    while left:
        s = rng.choice(free)
        k = rng.randint(1, left)
        if cap is not None:
            k = min(k, cap - norm[s])
            if k <= 0:
                continue
        norm[s] += k
        left -= k
    return norm


# ---- Huffman
def huf_lengths(n, maxlen, rng, flat=False):
    """Code lengths of a complete prefix code of n symbols whose longest code has maxlen bits: a chain down to
    maxlen, then leaves split at random (flat: the shallowest first, which keeps the weights' entropy low)."""
    assert maxlen + 1 <= n <= 1 << maxlen
    leaves = list(range(1, maxlen)) + [maxlen, maxlen]
    while len(leaves) < n:
        cand = [i for i, l in enumerate(leaves) if l < maxlen]
        i = min(cand, key=lambda q: leaves[q]) if flat else rng.choice(cand)
        l = leaves.pop(i)
        leaves += [l + 1, l + 1]
    return leaves


class Huf:
    """lens: symbol -> code length (0: unused); the last symbol is used."""

    def __init__(self, lens):
        self.lens = list(lens)
        assert self.lens[-1] > 0
        self.log = max(self.lens)
        self.weights = [self.log + 1 - l if l else 0 for l in self.lens]
        assert sum((1 << w) >> 1 for w in self.weights) == 1 << self.log
        # codes in weight order, then symbol order: a code is the first table slot >> (w - 1)
        self.code, slot = {}, 0
        for w in range(1, self.log + 1):
            for s, ws in enumerate(self.weights):
                if ws == w:
                    self.code[s] = (slot >> (w - 1), self.log + 1 - w)
                    slot += 1 << (w - 1)
        assert slot == 1 << self.log

    def stream(self, data):
        return backward_bits([self.code[b] for b in data])

    def direct(self):
        w = self.weights[:-1]
        assert 1 <= len(w) <= 128
        w2 = w + [0] * (len(w) & 1)
        return bytes([127 + len(w)]) + bytes(w2[i] << 4 | w2[i + 1] for i in range(0, len(w2), 2))

    def fse(self, log, rng, norm=None):
        """The FSE-compressed description: two interleaved states, even weights on the first; no update bits
        after the last two weights.  At most size / 2 per symbol, so that every state reads a bit."""
        w = self.weights[:-1]
        assert len(w) >= 2
        if norm is None:
            norm = weight_norm(w, log, rng)
        t = Fse(norm, log)
        assert all(e[1] >= 1 for e in t.ent)
        st = [t.states(w[0::2], rng), t.states(w[1::2], rng)]
        fields = [(st[0][0], log), (st[1][0], log)]
        for i in range(len(w) - 2):
            fields.append(t.update(st[i & 1][i >> 1], st[i & 1][(i >> 1) + 1]))
        body = write_ncount(norm, log) + backward_bits(fields)
        assert len(body) < 128, "weights too costly for an FSE description: %d" % len(body)
        return bytes([len(body)]) + body


def weight_norm(w, log, rng):
    size = 1 << log
    used = sorted(set(w))
    extra = [] if len(used) > 1 else [used[0] + 1 if used[0] < 11 else used[0] - 1]
    syms = sorted(set(used) | set(extra))
    # counts by frequency, at most size / 2 each, at least 1
    norm = [0] * (syms[-1] + 1)
    for s in syms:
        norm[s] = 1
    left = size - len(syms)
    order = sorted(syms, key=lambda s: -w.count(s))
    while left:
        moved = False
        for s in order:
            k = min(left, size // 2 - norm[s], max(1, left // 2))
            if k > 0:
                norm[s] += k
                left -= k
                moved = True
            if not left:
                break
        assert moved
    return norm


def lit_header(kind, sf, size, csize=None):
    """kind 0 raw, 1 RLE, 2 Huffman, 3 treeless; sf: the size format."""
    if kind < 2:
        if sf in (0, 2):
            assert size < 32
            return bytes([kind | sf << 2 | size << 3])
        if sf == 1:
            assert size < 1 << 12
            return (kind | sf << 2 | size << 4).to_bytes(2, "little")
        assert size < 1 << 20
        return (kind | sf << 2 | size << 4).to_bytes(3, "little")
    bits = {0: 10, 1: 10, 2: 14, 3: 18}[sf]
    assert size < 1 << bits and csize < 1 << bits, (sf, size, csize)
    return (kind | sf << 2 | size << 4 | csize << (4 + bits)).to_bytes({10: 3, 14: 4, 18: 5}[bits], "little")


def huf_streams(h, data, four):
    if not four:
        return h.stream(data)
    seg = (len(data) + 3) // 4
    parts = [h.stream(data[k * seg:(k + 1) * seg]) for k in range(3)] + [h.stream(data[3 * seg:])]
    assert all(len(p) < 65536 for p in parts)
    return b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)


def smallest_sf(kind, size, csize=0, four=False):
    if kind < 2:
        return 0 if size < 32 else 1 if size < 4096 else 3
    if not four:
        return 0
    m = max(size, csize)
    return 1 if m < 1 << 10 else 2 if m < 1 << 14 else 3


# ---- the plain model
def rep_rule(rep, ofv, ll0):
    """RFC 8878 3.1.1.5: the offset of offset value ofv, and the new repeat offsets.  None: offset 0."""
    if ofv > 3:
        return ofv - 3, [ofv - 3, rep[0], rep[1]]
    idx = ofv - 1 + (1 if ll0 else 0)  # 0 rep1, 1 rep2, 2 rep3, 3 rep1 - 1
    off = rep[0] - 1 if idx == 3 else rep[idx]
    if off == 0:
        return None, rep
    if idx == 0:
        return off, rep
    if idx == 1:
        return off, [off, rep[0], rep[2]]
    return off, [off, rep[0], rep[1]]


class Plain:
    """One frame's output and repeat offsets."""

    def __init__(self):
        self.out, self.rep = bytearray(), [1, 4, 8]

    def seq(self, lit, ofv, ml):
        self.out += lit
        off, self.rep = rep_rule(self.rep, ofv, len(lit) == 0)
        if off is None or off > len(self.out):
            raise ValueError("offset")
        if off >= ml:
            self.out += self.out[len(self.out) - off:len(self.out) - off + ml]
        else:
            for _ in range(ml):
                self.out.append(self.out[-off])
        return off


def expand(frames):
    """frames: [[block]], block ("raw", bytes) | ("rle", byte, n) | ("comp", literals, [(ll, ofv, ml)]).
    The bytes they decode to; ValueError where a sequence is invalid."""
    total = bytearray()
    for blocks in frames:
        p = Plain()
        for b in blocks:
            if b[0] == "raw":
                p.out += b[1]
            elif b[0] == "rle":
                p.out += bytes([b[1]]) * b[2]
            else:
                lits, at = b[1], 0
                for ll, ofv, ml in b[2]:
                    if at + ll > len(lits):
                        raise ValueError("literals")
                    p.seq(lits[at:at + ll], ofv, ml)
                    at += ll
                p.out += lits[at:]
        total += p.out
    return bytes(total)


# ---- blocks and frames
def seq_count(n, form=None):
    if form is None:
        form = 0 if n < 128 else 1 if n < 0x7F00 else 2
    if form == 0:
        assert n < 128
        return bytes([n])
    if form == 1:
        assert n < 0x8000 - 0x100
        return bytes([0x80 + (n >> 8), n & 255])
    assert 0x7F00 <= n <= 0x7F00 + 0xFFFF
    return b"\xff" + (n - 0x7F00).to_bytes(2, "little")


MODE = {"predef": 0, "rle": 1, "fse": 2, "repeat": 3}


class FrameB:
    """One frame, built block by block.  Literal bytes come from the caller; offsets are checked by Plain.
    desc is the description expand() takes; blocks what Z.frame takes."""

    def __init__(self, seed=0):
        self.rng = random.Random(seed)
        self.p = Plain()
        self.desc, self.blocks = [], []
        self.tab = {"ll": None, "of": None, "ml": None}  # the tables a Repeat mode would use
        self.huf = None
        self.lits, self.seqs = bytearray(), []

    # -- what the block being built holds
    @property
    def pos(self):
        return len(self.p.out)

    @property
    def rep(self):
        return self.p.rep

    def seq(self, lit, ofv, ml):
        off = self.p.seq(lit, ofv, ml)
        self.lits += lit
        self.seqs.append((len(lit), ofv, ml))
        return off

    def force(self, lit, ofv, ml, ll=None):
        """A sequence as it is, not followed by the plain model (for streams that are meant to be invalid)."""
        self.lits += lit
        self.seqs.append((len(lit) if ll is None else ll, ofv, ml))
        self.p.out += bytes(lit) + bytes(ml)  # the size it would have

    def new(self, lit, off, ml):
        return self.seq(lit, off + 3, ml)

    def tail(self, lit):
        self.p.out += lit
        self.lits += lit

    def raw(self, data):
        self.p.out += data
        self.desc.append(("raw", bytes(data)))
        self.blocks.append((0, bytes(data), None))

    def rle(self, byte, n):
        self.p.out += bytes([byte]) * n
        self.desc.append(("rle", byte, n))
        self.blocks.append((1, bytes([byte]), n))

    # -- sections
    def literals(self, lit="raw", sf=None, huf=None, four=False, desc="direct", wlog=6):
        """lit: raw | rle | huf | treeless.  huf: the Huf to use (huf), else one over the literals' bytes."""
        data = bytes(self.lits)
        if lit == "raw":
            return lit_header(0, smallest_sf(0, len(data)) if sf is None else sf, len(data)) + data
        if lit == "rle":
            assert data and data == data[:1] * len(data)
            return lit_header(1, smallest_sf(1, len(data)) if sf is None else sf, len(data)) + data[:1]
        if lit == "huf":
            if huf is None:
                syms = sorted(set(data))
                assert len(syms) >= 2
                ln = huf_lengths(len(syms), min(11, max(1, len(syms) - 1)), self.rng)
                self.rng.shuffle(ln)
                lens = [0] * (syms[-1] + 1)
                for s, l in zip(syms, ln):
                    lens[s] = l
                huf = Huf(lens)
            self.huf = huf
            tree = huf.direct() if desc == "direct" else huf.fse(wlog, self.rng)
        else:
            assert self.huf is not None
            tree = b""
        body = tree + huf_streams(self.huf, data, four)
        if sf is None:
            sf = smallest_sf(2, len(data), len(body), four)
        assert (sf > 0) == four
        return lit_header(2 if lit == "huf" else 3, sf, len(data), len(body)) + body

    def table(self, which, mode, codes, log=None, norm=None, less1=(), extra=(), desc=None, tab=None):
        """(description bytes, the decoding table) of one sequence table.  desc / tab: given as they are
        (for descriptions that are meant to be invalid)."""
        if desc is not None:
            return desc, tab
        if mode == "predef":
            lg, n = DEFAULT[which]
            return b"", Fse(n, lg)
        if mode == "rle":
            assert len(set(codes)) == 1
            return bytes([codes[0]]), Fse.rle(codes[0])
        if mode == "repeat":
            assert self.tab[which] is not None
            return b"", self.tab[which]
        if norm is None:
            used = set(codes)
            if log is None:
                log = max(5, (len(used | set(less1) | set(extra)) - 1).bit_length())
            if len(used | set(less1) | set(extra)) < 2:
                extra = set(extra) | {min(used) + 1 if min(used) < 28 else min(used) - 1}
            norm = make_norm(used, log, self.rng, less1=less1, extra=extra)
        return write_ncount(norm, log), Fse(norm, log)

    def sequences(self, ll="predef", of="predef", ml="predef", form=None, opts=None, modes_or=0, nseq=None):
        """The sequences section.  ll / of / ml: predef | rle | fse | repeat; opts: which -> table() keywords."""
        if not self.seqs:
            return seq_count(0, form)
        opts = opts or {}
        cl = [ll_code(s[0]) for s in self.seqs]
        co = [of_code(s[1]) for s in self.seqs]
        cm = [ml_code(s[2]) for s in self.seqs]
        modes = {"ll": ll, "of": of, "ml": ml}
        out = seq_count(len(self.seqs) if nseq is None else nseq, form) + \
            bytes([MODE[ll] << 6 | MODE[of] << 4 | MODE[ml] << 2 | modes_or])
        t = {}
        for which, cs in (("ll", cl), ("of", co), ("ml", cm)):
            d, t[which] = self.table(which, modes[which], [c[0] for c in cs], **opts.get(which, {}))
            out += d
        self.tab = dict(t)
        sl = t["ll"].states([c[0] for c in cl], self.rng)
        so = t["of"].states([c[0] for c in co], self.rng)
        sm = t["ml"].states([c[0] for c in cm], self.rng)
        f = [(sl[0], t["ll"].log), (so[0], t["of"].log), (sm[0], t["ml"].log)]
        n = len(self.seqs)
        for i in range(n):
            f += [co[i][1:], cm[i][1:], cl[i][1:]]
            if i + 1 < n:
                f += [t["ll"].update(sl[i], sl[i + 1]), t["ml"].update(sm[i], sm[i + 1]),
                      t["of"].update(so[i], so[i + 1])]
        return out + backward_bits(f)

    def end(self, lit="raw", ll="predef", of="predef", ml="predef", form=None, opts=None, modes_or=0, nseq=None,
            **litkw):
        """Close the block being built; returns its payload (also appended to the frame)."""
        payload = self.literals(lit, **litkw) + self.sequences(ll, of, ml, form, opts, modes_or, nseq)
        self.push(payload)
        return payload

    def push(self, payload):
        self.desc.append(("comp", bytes(self.lits), list(self.seqs)))
        self.blocks.append((2, payload, None))
        self.lits, self.seqs = bytearray(), []

    def frame(self, fcs_bytes=None, **kw):
        content = bytes(self.p.out)
        if fcs_bytes is None:
            fcs_bytes = 4 if len(content) >= 256 else 0
        return Z.frame(self.blocks, content, fcs_bytes=fcs_bytes, **kw)
