"""A DEFLATE (RFC 1951) writer and a model of the format, in plain Python, for
streams that zlib's encoder never emits (tests/test_inflate_layouts.py).

Tokens.  A literal is an int 0..255, a run of literals a bytes object, a match
a tuple (length 3..258, distance 1..32768); (258, distance, 284) writes the
length as symbol 284 with extra bits 31 and not as symbol 285.  For the error
cases a token may also name a raw symbol: ("lsym", s) writes literal/length
symbol s and nothing else, ("dsym", length, ds) a length and then distance
symbol ds without extra bits, ("draw", length, code, nbits) a length and then
the bits of `code` (most significant first) where the distance code belongs.

model(tokens) is the definition of what a stream decodes to; the writer
(Deflate) never looks at it.  member() frames a stream as a gzip member
(RFC 1952)."""
import zlib

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
# a complete code over all 19 code-length symbols: 13 / 16 + 6 / 32 = 1
CL_DEFAULT = [4] * 13 + [5] * 6

# length 3..258 -> (symbol - 257, extra bits, extra value); distance likewise
_LEN_OF = {}
for _s in range(28):
    for _e in range(1 << LEN_EXTRA[_s]):
        _LEN_OF.setdefault(LEN_BASE[_s] + _e, (_s, LEN_EXTRA[_s], _e))
_LEN_OF[258] = (28, 0, 0)  # symbol 285, not 284 + 31


def len_sym(length):
    return 257 + _LEN_OF[length][0]


def dist_sym(dist):
    for ds in range(29, -1, -1):
        if dist >= DIST_BASE[ds]:
            return ds
    raise ValueError(dist)


def model(tokens):
    """The bytes a token list stands for: byte by byte, a match copies
    out[-distance] `length` times (so it may overlap itself)."""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif isinstance(t, (bytes, bytearray)):
            out += t
        else:
            length, d = t[0], t[1]
            assert 3 <= length <= 258 and 1 <= d <= 32768 and d <= len(out), t
            for _ in range(length):
                out.append(out[-d])
    return bytes(out)


def kraft(lens):
    """Sum of 2^-l over the non-zero lengths, in units of 2^-15."""
    return sum(1 << (15 - x) for x in lens if x)


def canonical(lens):
    """RFC 1951 3.2.2: {symbol: (code, length)}, the code's first bit in its
    most significant bit."""
    count = [0] * 17
    for x in lens:
        count[x] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for s, x in enumerate(lens):
        if x:
            out[s] = (nxt[x], x)
            nxt[x] += 1
    return out


def _rev(code, n):
    r = 0
    for _ in range(n):
        r = r << 1 | (code & 1)
        code >>= 1
    return r


def _stream_codes(lens):
    """{symbol: (code as written, least significant bit first; length)}"""
    return {s: (_rev(c, n), n) for s, (c, n) in canonical(lens).items()}


# ---------------------------------------------------------------- code length generators
def balanced(m, depth=0):
    """m leaves filling the subtree below one node at `depth`."""
    assert m >= 1
    k = m.bit_length() - 1
    if m == 1 << k:
        return [depth + k] * m
    return [depth + k] * ((2 << k) - m) + [depth + k + 1] * (2 * (m - (1 << k)))


def skewed_lens(order, maxlen, size):
    """A complete code over the symbols `order` (shortest code first): a chain
    1, 2, ..., c and a balanced subtree for the rest, c such that the deepest
    code is exactly maxlen bits."""
    n = len(order)
    for c in range(n - 1):
        tail = balanced(n - c, c)
        if tail[-1] == maxlen:
            ls = list(range(1, c + 1)) + tail
            break
    else:
        raise ValueError("no chain gives %d bits over %d symbols" % (maxlen, n))
    lens = [0] * size
    for s, x in zip(order, ls):
        lens[s] = x
    assert kraft(lens) == 1 << 15 and max(lens) == maxlen
    return lens


def random_lens(rng, symbols, maxlen, size):
    """A random complete code over `symbols` (two at least), no code longer
    than maxlen: leaves are split at random until there is one per symbol."""
    symbols = list(symbols)
    n = len(symbols)
    assert 2 <= n <= 1 << maxlen <= 1 << 15
    leaves = [1, 1]
    while len(leaves) < n:
        open_ = [i for i, x in enumerate(leaves) if x < maxlen]
        i = open_[int(rng.integers(0, len(open_)))]
        leaves[i] += 1
        leaves.append(leaves[i])
    order = rng.permutation(n)
    lens = [0] * size
    for k, x in zip(order, leaves):
        lens[symbols[int(k)]] = x
    assert kraft(lens) == 1 << 15
    return lens


def used_symbols(tokens):
    """(literal/length symbols incl. 256, distance symbols) a token list needs."""
    lit, dist = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            lit.add(t)
        elif isinstance(t, (bytes, bytearray)):
            lit.update(t)
        else:
            lit.add(284 if len(t) == 3 else len_sym(t[0]))
            dist.add(dist_sym(t[1]))
    return lit, dist


def cl_symbols(seq, runs=True):
    """The code-length symbols [(symbol, extra value)] for the length
    sequence `seq` (literal/length lengths then distance lengths, as one
    sequence: a run does not care where the first list ends).  runs: greedy
    18 / 17 for zeros and 16 for repeats; otherwise one symbol per length."""
    out, i, n = [], 0, len(seq)
    while i < n:
        x = seq[i]
        j = i
        while j < n and seq[j] == x:
            j += 1
        run = j - i
        if not runs:
            out += [(x, 0)] * run
        elif x == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11))
                run -= k
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((x, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
            out += [(x, 0)] * run
        i = j
    return out


_CL_EXTRA = {16: 2, 17: 3, 18: 7}


# ---------------------------------------------------------------- the writer
class Deflate:
    """A bit writer (fields least significant bit first, Huffman codes most
    significant bit first) with one method per block type; blocks follow each
    other at the bit where the last one ended."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def bits(self, v, k):
        assert 0 <= v < (1 << k) or k == 0
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        self.bits(_rev(code, n), n)

    def align(self):
        if self.n:
            self.out.append(self.acc)
            self.acc = self.n = 0

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")

    def _literals(self, data, codes):
        """A run of literals at once (the same bits as one by one)."""
        tab_c = np.zeros(256, np.uint32)
        tab_n = np.zeros(256, np.uint8)
        for s in set(data):
            tab_c[s], tab_n[s] = codes[s]
        a = np.frombuffer(bytes(data), np.uint8)
        c, n = tab_c[a], tab_n[a]
        k = np.arange(15, dtype=np.uint32)
        bit = ((c[:, None] >> k) & 1).astype(np.uint8)[k < n[:, None]]
        head = np.array([(self.acc >> i) & 1 for i in range(self.n)], np.uint8)
        bit = np.concatenate([head, bit])
        whole = len(bit) // 8 * 8
        self.out += np.packbits(bit[:whole], bitorder="little").tobytes()
        self.acc, self.n = 0, 0
        for i, b in enumerate(bit[whole:]):
            self.acc |= int(b) << i
            self.n += 1

    def _tokens(self, tokens, lit, dist):
        for t in tokens:
            if isinstance(t, int):
                self.bits(*lit[t])
            elif isinstance(t, (bytes, bytearray)):
                if len(t) < 32:
                    for b in t:
                        self.bits(*lit[b])
                else:
                    self._literals(t, lit)
            elif t[0] == "lsym":
                self.bits(*lit[t[1]])
            else:
                raw = isinstance(t[0], str)
                length = t[1] if raw else t[0]
                s, xb, xv = (27, 5, 31) if len(t) == 3 and not raw else _LEN_OF[length]
                self.bits(*lit[257 + s])
                self.bits(xv, xb)
                if not raw:
                    ds = dist_sym(t[1])
                    self.bits(*dist[ds])
                    self.bits(t[1] - DIST_BASE[ds], DIST_EXTRA[ds])
                elif t[0] == "dsym":
                    self.bits(*dist[t[2]])
                else:
                    self.code(t[2], t[3])
        self.bits(*lit[256])

    def stored(self, data, last, len_=None, nlen=None):
        """BTYPE 00.  len_ / nlen: the LEN and NLEN fields when they are not
        len(data) and its complement."""
        assert len(data) <= 65535
        self.bits(1 if last else 0, 1)
        self.bits(0, 2)
        self.align()
        ln = len(data) if len_ is None else len_
        self.out += ln.to_bytes(2, "little") + ((~ln & 0xffff) if nlen is None else nlen).to_bytes(2, "little")
        self.out += data
        return self

    def fixed(self, tokens, last):
        """BTYPE 01; symbols 286 / 287 and distance codes 30 / 31 can be named raw."""
        self.bits(1 if last else 0, 1)
        self.bits(1, 2)
        self._tokens(tokens, _stream_codes(FIXED_LIT), _stream_codes(FIXED_DIST))
        return self

    def dynamic(self, tokens, lit_lens, dist_lens, last, hlit=None, hdist=None, cl_lens=None, hclen=None,
                runs=True, cl_syms=None, eob=True):
        """BTYPE 10.  hlit / hdist: the counts the header announces (default:
        up to the last non-zero length; 287, 288, 31 and 32 can be written).
        cl_lens: the code-length code's 19 lengths (or a function of the
        symbols written that gives them); hclen: how many of them
        are written.  runs: see cl_symbols; cl_syms: the code-length symbols
        as given, whatever the lengths say.  Returns the (symbol, extra) list
        written.  eob: False leaves the end-of-block code out."""
        def upto(lens, least):
            n = len(lens)
            while n > least and lens[n - 1] == 0:
                n -= 1
            return n

        hlit = upto(lit_lens, 257) if hlit is None else hlit
        hdist = upto(dist_lens, 1) if hdist is None else hdist
        seq = (list(lit_lens) + [0] * 288)[:hlit] + (list(dist_lens) + [0] * 32)[:hdist]
        assert all(x == 0 for x in lit_lens[hlit:]) and all(x == 0 for x in dist_lens[hdist:])
        syms = cl_symbols(seq, runs) if cl_syms is None else cl_syms
        cl_lens = CL_DEFAULT if cl_lens is None else cl_lens(syms) if callable(cl_lens) else cl_lens
        if hclen is None:
            hclen = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]))
        assert all(cl_lens[s] == 0 for s in CL_ORDER[hclen:])
        cl = _stream_codes(cl_lens)
        self.bits(1 if last else 0, 1)
        self.bits(2, 2)
        self.bits(hlit - 257, 5)
        self.bits(hdist - 1, 5)
        self.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            self.bits(cl_lens[s], 3)
        for s, x in syms:
            self.bits(*cl[s])
            if s >= 16:
                self.bits(x, _CL_EXTRA[s])
        self.header_end = self.bitpos
        lit, dist = _stream_codes(lit_lens), _stream_codes(dist_lens)
        if not eob:
            lit[256] = (0, 0)
        self._tokens(tokens, lit, dist)
        return syms


def member(deflate, raw, extra=None, name=None, crc=None, isize=None):
    """A gzip member around a DEFLATE stream that decodes to `raw`.  extra:
    the FEXTRA field's bytes (None: no field), which move the stream's byte
    position; crc / isize: trailer values other than the right ones."""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0)
    hdr = bytes([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 3])
    if extra is not None:
        hdr += len(extra).to_bytes(2, "little") + extra
    if name is not None:
        hdr += name + b"\0"
    crc = zlib.crc32(raw) & 0xffffffff if crc is None else crc
    isize = len(raw) & 0xffffffff if isize is None else isize
    return hdr + deflate + crc.to_bytes(4, "little") + isize.to_bytes(4, "little")
