"""A Snappy block writer that places every tag by hand, a model of which path
of the GPU decoder (pqg_snappy.hip) each tag takes, and the directed cases of
tests/test_snappy_edges.py.

`lit`, `copy`, `uvarint` and the random `stream` are the tag writers the older
Snappy tests share.  `Builder` tracks the compressed position `s` (after the
length varint), the output position `d` and the plaintext, and logs every tag,
so a case can put a tag on one of the decoder's constants and a test can
recompute from the log that it is there.  `trace` restates the control flow
of SnapBlock::run / serial (windows of kPos positions, the dense/sparse
switch, the batch cut, the literal writers) over a tag log: it never touches a
byte of data and is not a decoder; it only names the path of each tag."""
import numpy as np

# The decoder's constants (parquet-go_amd/csrc/pqg_snappy.hip, top of the K2
# section; kSnapSub / kSnapSeg: pqg_common.h).
K_POS = 128          # kPos: tag positions parsed per window
K_DENSE = 8          # kDense: chain tags of a first window for the batched path
K_WIN = 4096         # kSnWin: compressed bytes held in LDS
K_WIN_NEED = 2048    # kSnWinNeed: window bytes wanted ahead of a tag
K_SPAN = 1024        # kSpan: output bytes of a batch
K_RING = 4096        # kRing (PQG_SNAPPY_RING): output history held in LDS
K_LONG_PIECE = 1024  # kLongPiece: piece of a long literal
K_WIN_LIT = 1024     # kWinLit: longest literal moved from the window
K_BATCH_WIN = 3      # kBatchWin: windows one batch may take
K_BATCH_TAGS = 256   # kBatchTags
K_BATCH_ROOM = 192   # kBatchRoom: a batch with less room takes no further window
K_SERIAL = 64        # tags serial() takes after a sparse window or a long literal
K_STREAK = 4         # short tags (< K_SHORT bytes) in a row that end serial()
K_SHORT = 16
K_SUB = 65536        # kSnapSub: output bytes of a sub-block
K_SEG = 4096         # kSnapSeg: compressed bytes of a segment of the chain search


def lit_header(n, form=None):
    """The 1..5-byte header of an n-byte literal; `form`: that many bytes."""
    n -= 1
    if form is None:
        form = 1 if n < 60 else 2 if n < 1 << 8 else 3 if n < 1 << 16 else 4 if n < 1 << 24 else 5
    if form == 1:
        assert 0 <= n < 60
        return bytes([n << 2])
    assert 2 <= form <= 5 and 0 <= n < 1 << (8 * (form - 1))
    return bytes([(58 + form) << 2]) + n.to_bytes(form - 1, "little")


def lit(b, form=None):
    return lit_header(len(b), form) + bytes(b)


def copy(off, ln, form):
    """Copy tag of form 1, 2 or 4 (offset bytes); the fields are not checked
    against any output, so corrupt tags are written the same way."""
    if form == 1:
        assert 4 <= ln <= 11 and 0 <= off < 2048
        return bytes([1 | (ln - 4) << 2 | (off >> 8) << 5, off & 255])
    if form == 2:
        assert 1 <= ln <= 64 and 0 <= off < 65536
        return bytes([2 | (ln - 1) << 2, off & 255, off >> 8])
    assert form == 4 and 1 <= ln <= 64 and 0 <= off < 1 << 32
    return bytes([3 | (ln - 1) << 2]) + off.to_bytes(4, "little")


def uvarint(n, size=0):
    """n as a varint; size > 0: padded with zero groups to that many bytes
    (non-minimal, as binary.Uvarint accepts)."""
    o = bytearray()
    while n >= 0x80:
        o.append(n & 0x7F | 0x80)
        n >>= 7
    o.append(n)
    if size:
        assert size >= len(o)
        while len(o) < size:
            o[-1] |= 0x80
            o.append(0)
    return bytes(o)


def stream(rng, target, far_frac=0.2, lit_max=40, long_lit=0.01):
    """Random tag stream of about `target` output bytes -> (compressed, plaintext)."""
    out = bytearray()
    tags = []
    while len(out) < target:
        r = rng.random()
        if not out or r < 0.3:
            n = int(rng.integers(1, lit_max + 1)) if rng.random() > long_lit else int(rng.integers(60, 5000))
            b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            tags.append(lit(b))
            out += b
            continue
        d = len(out)
        if r < 0.45:  # overlapping run-length copy
            off = int(rng.integers(1, min(d, 8) + 1))
        elif r < 0.45 + far_frac and d > 17000:
            off = int(rng.integers(16400, min(d, 65535) + 1))
        else:
            off = int(rng.integers(1, min(d, 3000) + 1))
        ln = int(rng.integers(1, 65))
        if off < 2048 and 4 <= ln <= 11 and rng.random() < 0.5:
            form = 1
        elif rng.random() < 0.1:
            form = 4
        else:
            form = 2
        tags.append(copy(off, ln, form))
        for _ in range(ln):
            out.append(out[-off])
    return uvarint(len(out)) + b"".join(tags), bytes(out)


class T:
    """One logged tag: kind 'L' or 'C', its compressed position s (after the
    varint), output position d, output length, header bytes, copy offset."""
    __slots__ = ("kind", "s", "d", "ln", "hdr", "off")

    def __init__(self, kind, s, d, ln, hdr, off=0):
        self.kind, self.s, self.d, self.ln, self.hdr, self.off = kind, s, d, ln, hdr, off

    @property
    def next_s(self):
        return self.s + self.hdr + (self.ln if self.kind == "L" else 0)


class Builder:
    def __init__(self, seed=0):
        self.rng = np.random.default_rng(seed)
        self.comp = bytearray()
        self.out = bytearray()
        self.log = []

    @property
    def s(self):
        return len(self.comp)

    @property
    def d(self):
        return len(self.out)

    @property
    def last(self):
        return len(self.log) - 1

    # ---- tags
    def lit(self, data, form=None):
        if isinstance(data, int):
            data = self.rng.integers(0, 256, data, dtype=np.uint8).tobytes()
        h = lit_header(len(data), form)
        self.log.append(T("L", self.s, self.d, len(data), len(h)))
        self.comp += h
        self.comp += data
        self.out += data
        return self.last

    def copy(self, off, ln, form=2):
        assert 1 <= off <= self.d
        t = copy(off, ln, form)
        self.log.append(T("C", self.s, self.d, ln, len(t), off))
        self.comp += t
        lo = self.d - off
        if off >= ln:
            self.out += self.out[lo:lo + ln]
        else:
            self.out += (bytes(self.out[lo:]) * (ln // off + 1))[:ln]
        return self.last

    # ---- placement
    def to_d(self, target, piece=None):
        """Literals until the next tag's output starts at `target` (pieces of
        at most `piece` bytes; default: one literal)."""
        assert target >= self.d
        while self.d < target:
            self.lit(min(target - self.d, piece or target - self.d))

    def to_s(self, target):
        """Filler until the next tag starts at compressed position `target`,
        moving d as little as it can: one-byte literals under long headers."""
        ds = target - self.s
        assert ds == 0 or ds >= 2, ds
        while ds >= 8:
            self.lit(1, form=5)
            ds -= 6
        if ds == 7:
            self.lit(1, form=1)
            ds -= 2
        if ds:
            self.lit(1, form=ds - 1)
        assert self.s == target

    def to(self, s, d):
        """Filler until the next tag starts at compressed position s AND
        output position d.  A literal of n bytes under an h-byte header moves
        (s, d) by (h + n, n); a copy-2 by (3, 1..64)."""
        fits = {1: 60, 2: 1 << 8, 3: 1 << 16, 4: 1 << 24, 5: 1 << 32}
        while (self.s, self.d) != (s, d):
            ds, dd = s - self.s, d - self.d
            assert ds >= 2 and dd >= 1, (ds, dd)
            h = ds - dd  # header bytes still to spend: h per literal, 3 - ln per copy
            rest = -(-(h - 3) // 5)  # one-byte literals that spend h - 3 more header bytes
            if h < 1 or (h < 3 and dd > fits[h]):
                assert self.d >= 1 and ds >= 7 and dd >= 2, (ds, dd)
                self.copy(1, min(64, 6 - h, dd - 1), 2)  # up to h == 3
            elif h <= 5 and dd <= fits[h]:
                self.lit(dd, form=h)
            elif 1 <= dd - rest <= fits[3]:
                self.lit(dd - rest, form=3)
            else:
                assert dd >= 2
                self.lit(1, form=5)

    def long_then(self, n=1100, follow=2):
        """A literal longer than one batch, then `follow` literals of 20 bytes
        (>= K_SHORT: no streak; at most 7 of them start in a window): the tags
        after it are taken one at a time."""
        i = self.lit(n)
        for _ in range(follow):
            self.lit(20)
        return i

    def dense_here(self, n=12):
        """K_STREAK tags shorter than K_SHORT bytes, which end a serial()
        streak, then n >= K_DENSE two-byte literals in 3 n <= 128 positions:
        the window that starts at the first of them is dense, and the caller's
        next tags join its batch while they start inside it."""
        assert n >= K_DENSE
        for _ in range(K_STREAK):
            self.lit(3)
        first = self.last + 1
        for _ in range(n):
            self.lit(2)
        return first

    # ---- results
    def finish(self, varint_pad=0):
        return uvarint(self.d, varint_pad) + bytes(self.comp), bytes(self.out)

    def block_shaped(self):
        """No tag's output crosses a multiple of K_SUB and no copy reaches
        before the start of its own K_SUB output block."""
        for t in self.log:
            base = t.d // K_SUB * K_SUB
            if t.d + t.ln > base + K_SUB:
                return False
            if t.kind == "C" and t.d - t.off < base:
                return False
        return True


# ---------------------------------------------------------------------------
# The path model
# ---------------------------------------------------------------------------
class Step:
    """Where the model puts one tag: path 'dense' | 'sparse' | 'serial' |
    'first' (a literal too long for a batch at a window's first position);
    writer 'dense' | 'window_literal' | 'long_literal' | 'copy_bytes'; rel: its
    position in the parsed window (None in serial()); win / batch: indices of
    the parsed window and of the dense batch; ring_lo: the ring's low edge the
    writer compares copy sources with; streak: serial()'s short_streak after
    the tag; nth: its index within the serial() call."""
    __slots__ = ("path", "writer", "rel", "win", "batch", "ring_lo", "streak", "nth", "bwin", "in_base")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


class Trace:
    def __init__(self):
        self.steps = []    # per tag
        self.windows = []  # per parsed window: dict(s, tags=[log indices], cut, batch, nwin, filled (after it))
        self.batches = []  # per dense batch: dict(a0, pre, filled, ntag, nwin, ring_lo, first, last)
        self.fills = []    # (s, in_base) of every window fill
        self.serials = []  # per serial() call: number of tags it took

    def counts(self):
        """dense batches, sparse windows, serial() tags, tags of the dense batches"""
        return (len(self.batches), sum(1 for w in self.windows if w["kind"] == "sparse"),
                sum(self.serials), sum(b["ntag"] for b in self.batches))


def trace(log, hl=1, src_align=0):
    """The decoder's path over a valid whole block whose tags are `log`, the
    varint taking hl bytes, the block's first byte at address src_align mod 16."""
    tr = Trace()
    pos = {hl + t.s: i for i, t in enumerate(log)}
    slen = hl + (log[-1].next_s if log else 0)
    s, d, in_base, serial_next = hl, 0, -(1 << 30), 0
    steps = [None] * len(log)

    def writer_of(t, d):
        if t.kind == "C":
            return "copy_bytes"
        return "window_literal" if (d & 15) + t.ln <= K_WIN_LIT else "long_literal"

    while s < slen:
        if s < in_base or s + K_WIN_NEED > in_base + K_WIN:
            in_base = s - ((src_align + s) & 15)
            tr.fills.append((s, in_base))
        if serial_next > 0:
            streak = n = 0
            while n < serial_next and s < slen and streak < K_STREAK:
                i = pos[s]
                t = log[i]
                ns = hl + t.next_s
                streak = streak + 1 if t.ln < K_SHORT else 0
                next_in = ns < slen and ns >= in_base and ns + K_WIN_NEED <= in_base + K_WIN
                w = writer_of(t, d)
                if w == "window_literal" and hl + t.s + t.hdr + t.ln > in_base + K_WIN:
                    w = "long_literal"
                steps[i] = Step(path="serial", writer=w, ring_lo=((d + 15) & ~15) - K_RING, streak=streak, nth=n,
                                in_base=in_base)
                d += t.ln
                s = ns
                n += 1
                if not next_in:
                    break
            tr.serials.append(n)
            serial_next = 0
            continue
        a0 = d & ~15
        pre = d - a0
        filled, ntag, nwin, sparse_done = pre, 0, 0, False
        batch_tags = []
        cut0 = False  # the batch ended at a literal too long for it, at a later window's first position
        while True:
            chain = []
            p = s
            while p < slen and p - s < K_POS:
                chain.append(pos[p])
                p = hl + log[pos[p]].next_s
            st, cut = 0, None
            for k, i in enumerate(chain):
                t = log[i]
                if filled + st + t.ln > K_SPAN or (t.kind == "L" and hl + t.s + t.hdr + t.ln > in_base + K_WIN):
                    cut = k
                    break
                st += t.ln
            win = dict(s=s, tags=chain, cut=cut, nwin=nwin, kind="dense", in_base=in_base)
            if cut == 0:
                if nwin > 0:
                    cut0 = True
                    break
                i = chain[0]
                steps[i] = Step(path="first", writer="long_literal", rel=0, win=len(tr.windows), in_base=in_base)
                win.update(kind="first", tags=chain[:1])
                tr.windows.append(win)
                d += log[i].ln
                s = hl + log[i].next_s
                serial_next = K_SERIAL
                sparse_done = True
                break
            take = chain if cut is None else chain[:cut]
            s1 = p if cut is None else hl + log[chain[cut]].s
            win["tags"] = take
            if nwin == 0 and len(take) < K_DENSE:
                win["kind"] = "sparse"
                for i in take:
                    t = log[i]
                    steps[i] = Step(path="sparse", writer=writer_of(t, d), rel=hl + t.s - s, win=len(tr.windows),
                                    ring_lo=((d + 15) & ~15) - K_RING, in_base=in_base)
                    d += t.ln
                tr.windows.append(win)
                s = s1
                serial_next = K_SERIAL
                sparse_done = True
                break
            for i in take:
                steps[i] = Step(path="dense", writer="dense", rel=hl + log[i].s - s, win=len(tr.windows),
                                batch=len(tr.batches), ring_lo=((d + 15) & ~15) - K_RING, bwin=nwin, in_base=in_base)
            batch_tags += take
            ntag += len(take)
            filled += st
            s = s1
            nwin += 1
            win.update(batch=len(tr.batches), filled=filled)
            tr.windows.append(win)
            if (cut is not None or nwin >= K_BATCH_WIN or filled > K_SPAN - K_BATCH_ROOM or s >= slen or
                    s + K_WIN_NEED // 2 > in_base + K_WIN):
                break
        if sparse_done:
            continue
        tr.batches.append(dict(a0=a0, pre=pre, filled=filled, ntag=ntag, nwin=nwin, ring_lo=((d + 15) & ~15) - K_RING,
                               tags=batch_tags, in_base=in_base, cut0=cut0))
        d = a0 + filled
    tr.steps = steps
    return tr


# ---------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------
class Case:
    """A named stream.  Valid cases carry their builder and `claims`: tuples
    (kind, ...) that tests/test_snappy_edges.py recomputes from the tag log and
    the path model (check_claim there).  Corrupt cases have plain None; `path`
    names the code that meets the bad tag first."""

    def __init__(self, name, comp, plain, b=None, claims=(), hl=1, path=None, pyarrow=True):
        self.name, self.comp, self.plain, self.b = name, comp, plain, b
        self.claims, self.hl, self.path, self.pyarrow = list(claims), hl, path, pyarrow

    @property
    def log(self):
        return self.b.log

    @property
    def family(self):
        return self.name[0]


def _case(name, b, claims=(), varint_pad=0, **kw):
    comp, plain = b.finish(varint_pad)
    return Case(name, comp, plain, b, claims, hl=len(comp) - len(b.comp), **kw)


def ring_lo(d):
    return ((d + 15) & ~15) - K_RING


def open_batch(b, pre=0, n=1100):
    """At a block's start: a literal longer than a batch (taken whole at the
    window's first position), then K_STREAK three-byte literals, which
    serial() takes and stops at.  The next tag opens a window, and a batch if
    the window is dense, at an output position = pre (mod 16)."""
    assert not b.log
    b.lit(n + (pre - n - 3 * K_STREAK) % 16)
    for _ in range(K_STREAK):
        b.lit(3)
    assert b.d % 16 == pre
    return b.d


def open_tags(b, dm=0, n=1100):
    """At a block's start: a long literal, then two 20-byte literals, so that
    the next tags are taken one at a time, the first at d = dm (mod 16)."""
    assert not b.log
    b.lit(n + (dm - n - 40) % 16)
    b.lit(20)
    b.lit(20)
    assert b.d % 16 == dm
    return b.d


def family_a():
    """Parse window (kPos 128).  Every block's first window starts at its
    first tag, so a tag's window position is its compressed position."""
    cs = []
    for p in (63, 64, 127):
        b = Builder(100 + p)
        if p % 2:
            b.lit(2)
        while b.s < p:
            b.lit(1)
        i = b.lit(5)
        for _ in range(20):
            b.copy(3, 7, 1)
        cs.append(_case("a_pos%d" % p, b, [("rel", i, p), ("path", i, "dense")]))
    for form, starts in ((4, range(124, 128)), (5, range(123, 128))):
        for p in starts:
            b = Builder(200 + 10 * form + p)
            for _ in range(10):
                b.lit(1)
            b.lit(p - b.s - 2, form=2)
            i = b.copy(9, 30, 4) if form == 4 else b.lit(40, form=5)
            for _ in range(12):
                b.copy(2, 5, 1)
            cs.append(_case("a_%s_header_at_%d" % ("copy4" if form == 4 else "lit5", p), b,
                            [("rel", i, p), ("path", i, "dense"), ("hdr_straddles", i)]))
    b = Builder(300)
    for _ in range(64):
        b.lit(1)
    for _ in range(64):
        b.copy(7, 4, 1)
    for _ in range(10):
        b.lit(2)
    cs.append(_case("a_64_literals_then_64_copy1", b, [("wintags", 0, 64, "L"), ("wintags", 1, 64, "C")]))
    for succ in (128, 129):
        b = Builder(310 + succ)
        for _ in range(30):
            b.lit(1)
        b.lit(succ - 3 - b.s - 2, form=2)
        i = b.copy(5, 9, 2)  # the window's last chain tag
        j = b.lit(3)
        for _ in range(10):
            b.copy(1, 4, 1)
        cs.append(_case("a_successor_%d" % succ, b, [("rel", i, succ - 3), ("rel", j, 0), ("win_of", j, 1)]))
    return cs


def family_b():
    """Path switches: kDense, serial()'s short-streak rule and its 64 tags."""
    cs = []
    for n in (7, 8):  # a first window of exactly n chain tags
        b = Builder(400 + n)
        for _ in range(n - 1):
            b.lit(3)
        b.lit(K_POS - b.s + 20)  # starts inside the window; the next tag is outside
        for _ in range(30):
            b.copy(4, 6, 1)
        cs.append(_case("b_first_window_%d_tags" % n, b,
                        [("wintags", 0, n, None), ("winkind", 0, "sparse" if n < K_DENSE else "dense")]))
    for shorts in (3, 4, 5):
        b = Builder(420 + shorts)
        open_tags(b)
        first = b.last + 1
        for _ in range(shorts):
            b.lit(5)
        i = b.lit(24)
        for _ in range(12):
            b.copy(8, 6, 1)
        k = min(shorts, K_STREAK)
        cs.append(_case("b_streak_%d_short_tags" % shorts, b,
                        [("path", first, "serial"), ("streak", first + k - 1, k),
                         ("path", i, "serial" if shorts < K_STREAK else "notserial")]))
    for ln in (15, 16):
        b = Builder(430 + ln)
        open_tags(b)
        for _ in range(3):
            b.lit(5)
        i = b.copy(30, ln, 2)
        j = b.lit(5)
        b.lit(40)
        for _ in range(12):
            b.copy(8, 6, 1)
        cs.append(_case("b_streak_tag_of_%d_bytes" % ln, b,
                        [("path", i, "serial"), ("streak", i, K_STREAK if ln < K_SHORT else 0),
                         ("path", j, "notserial" if ln < K_SHORT else "serial")]))
    b = Builder(440)
    b.lit(1100)
    first = b.last + 1
    for k in range(K_SERIAL + 6):
        if k % 2:
            b.copy(100 + k, 16 + k % 40, 2 if k % 3 else 4)
        else:
            b.lit(16)
    cs.append(_case("b_serial_takes_64_tags", b, [("serial_run", first, K_SERIAL)]))
    return cs


def _span_window(b, total):
    """One window's worth (< 128 positions) of dense tags producing exactly
    `total` (897 .. 1088) output bytes: eight 8-byte literals, fourteen 64-byte
    copies, then two copies; returns the last tag."""
    for _ in range(8):
        b.lit(8)
    for _ in range(14):
        b.copy(40, 64, 2)
    rest = total - 64 - 14 * 64
    b.copy(40, rest // 2, 2)
    return b.copy(40, rest - rest // 2, 2)


def family_c():
    """Batch cut (kSpan 1024, kBatchRoom 192, kBatchWin 3, kBatchTags 256)."""
    cs = []
    for pre in (0, 1, 15):
        for delta in (0, -1, 1):
            b = Builder(500 + 16 * pre + delta + 1)
            open_batch(b, pre)
            first = b.last + 1
            i = _span_window(b, K_SPAN - pre + delta)
            for _ in range(12):
                b.lit(2)
            cs.append(_case("c_batch_of_1024_minus_pre%d_%+d" % (pre, delta), b, [("span", first, i, pre, delta)]))
    b = Builder(520)
    _span_window(b, 1023)
    i = b.copy(50, 64, 2)
    for _ in range(12):
        b.lit(2)
    cs.append(_case("c_copy64_at_batch_byte_1023", b, [("cut_tag", i, 1023)]))
    for filled in (832, 833):
        b = Builder(530 + filled)
        for _ in range(8):
            b.lit(8)
        for _ in range(11):
            b.copy(40, 64, 2)
        i = b.lit(filled - b.d)  # 64 or 65 bytes from position 105: the chain leaves the window uncut
        for _ in range(30):
            b.lit(1)
        cs.append(_case("c_filled_%d_at_window_end" % filled, b, [("winfilled", 0, filled, filled <= K_SPAN - K_BATCH_ROOM)]))
    b = Builder(540)
    for _ in range(192 + 70):
        b.lit(1)
    cs.append(_case("c_three_windows_of_2_byte_tags", b, [("batch", 0, "nwin", 3), ("batch", 0, "ntag", 192),
                                                          ("batch", 1, "nwin", 2)]))
    b = Builder(541)
    for _ in range(64):
        b.lit(1)
    i = b.lit(1500)
    for _ in range(12):
        b.copy(9, 4, 1)
    cs.append(_case("c_long_literal_opens_second_window", b, [("path", i, "first"), ("cut0", 0)]))
    for over in (0, 1):  # an aligned block's first window is [0, 4096) of the block
        b = Builder(550 + over)
        n = 2500
        for _ in range(20):
            b.lit(2)
        b.to_s(K_WIN + over - n - 3 - 2)  # (the varint takes two bytes: hl below)
        i = b.lit(n)
        for _ in range(12):
            b.copy(9, 4, 1)
        cs.append(_case("c_literal_ends_at_window_end_%+d" % over, b, [("hl", 2), ("lit_end_minus_window", i, over)]))
    return cs


def family_d():
    """Same-batch copies (pointer doubling)."""
    cs = []
    for off in (1, 2, 3, 5, 15, 16, 17, 63, 64, 65):
        b = Builder(600 + off)
        b.lit(off)
        while b.d + 64 <= K_SPAN + 200:
            b.copy(off, 64, 2)
        cs.append(_case("d_period_%d" % off, b, [("path", 1, "dense"), ("same_batch_source", 1)]))
    b = Builder(620)
    for _ in range(10):
        b.lit(2)
    b.lit(24)
    for _ in range(8):
        last = b.copy(24, 24, 2)
    for _ in range(12):
        b.copy(3, 4, 1)
    cs.append(_case("d_copy_chain_8_deep", b, [("path", last, "dense"), ("copy_depth", last, 8)]))
    b = Builder(621)
    open_batch(b, 5)
    for _ in range(10):
        b.lit(2)
    i = b.copy(40, 64, 2)  # source [d - 40, d + 24): from the history into this batch
    for _ in range(12):
        b.copy(3, 4, 1)
    cs.append(_case("d_source_runs_from_history_into_batch", b, [("path", i, "dense"), ("source_straddles_batch_start", i)]))
    b = Builder(622)
    for _ in range(9):
        b.lit(2)
    j = b.lit(30)
    i = b.copy(20, 20, 2)
    for _ in range(12):
        b.copy(3, 4, 1)
    cs.append(_case("d_source_is_literal_of_batch", b, [("path", i, "dense"), ("source_in_tag", i, j)]))
    b = Builder(623)
    open_batch(b, 3, n=5000)
    for _ in range(10):
        b.lit(2)
    j = b.copy(b.d - 100, 32, 2)  # source [100, 132): far below ring_lo
    i = b.copy(32, 32, 2)         # a copy of that copy
    for _ in range(12):
        b.copy(3, 4, 1)
    cs.append(_case("d_copy_of_copy_from_below_ring", b, [("path", i, "dense"), ("path", j, "dense"),
                                                          ("source_in_tag", i, j), ("below_ring", j)]))
    return cs


def family_e():
    """Ring (kRing 4096)."""
    cs = []
    for dm in (0, 1, 8, 15):
        for ln in (1, 4, 64):
            for delta in (-1, 0, 1):
                b = Builder(700 + dm * 8 + ln + delta)
                open_tags(b, dm, n=6000)
                i = b.copy(b.d - (ring_lo(b.d) + delta), ln, 2)
                b.lit(20)
                b.lit(20)
                cs.append(_case("e_tag_d%d_len%d_ring_lo%+d" % (dm, ln, delta), b,
                                [("writer", i, "copy_bytes"), ("src_minus_ring_lo", i, delta)]))
                # dense: the copy is the batch's first tag, so ring_lo is taken at its d; its source
                # range [ring_lo + delta, + ln) straddles ring_lo for delta -1 and ln > 1
                b = Builder(750 + dm * 8 + ln + delta)
                open_batch(b, dm, n=6000)
                i = b.copy(b.d - (ring_lo(b.d) + delta), ln, 2)
                for _ in range(14):
                    b.lit(2)
                cs.append(_case("e_dense_d%d_len%d_ring_lo%+d" % (dm, ln, delta), b,
                                [("path", i, "dense"), ("rel", i, 0), ("src_minus_ring_lo", i, delta)]))
    for off, form in ((4095, 2), (4096, 2), (4097, 2), (65535, 2), (65536, 4), (70000, 4), (100000, 4)):
        for dense in (0, 1):
            b = Builder(800 + off % 97 + dense)
            n = max(off, 5000) + 37
            if dense:
                open_batch(b, 7, n)
                for _ in range(8):
                    b.lit(2)
            else:
                open_tags(b, 7, n)
            i = b.copy(off, 50, form)
            b.copy(off, 3, form)
            for _ in range(12):
                b.lit(2 if dense else 20)
            cs.append(_case("e_offset_%d_%s" % (off, "dense" if dense else "tag"), b,
                            [("path", i, "dense") if dense else ("writer", i, "copy_bytes")]))
    for dense in (0, 1):
        b = Builder(820 + dense)
        if dense:
            open_batch(b, 11, 5000)
            for _ in range(8):
                b.lit(2)
        else:
            open_tags(b, 11, 5000)
        i = b.copy(b.d, 40, 2)
        for _ in range(12):
            b.lit(2 if dense else 20)
        cs.append(_case("e_offset_equals_d_%s" % ("dense" if dense else "tag"), b,
                        [("off_is_d", i), ("path", i, "dense") if dense else ("writer", i, "copy_bytes")]))
    # a tag whose output crosses a multiple of kRing, once per writer
    b = Builder(830)
    open_tags(b, 0, 4000)  # d = 4048
    i = b.lit(60)
    b.lit(20)
    cs.append(_case("e_window_literal_crosses_4096", b, [("writer", i, "window_literal"), ("crosses", i, K_RING)]))
    b = Builder(831)
    open_tags(b, 0, 3000)
    i = b.lit(1200)
    b.lit(20)
    cs.append(_case("e_long_literal_crosses_4096", b, [("writer", i, "long_literal"), ("crosses", i, K_RING)]))
    b = Builder(832)
    open_tags(b, 0, 4000)
    i = b.copy(1000, 60, 2)
    b.lit(20)
    cs.append(_case("e_copy_bytes_crosses_4096", b, [("writer", i, "copy_bytes"), ("crosses", i, K_RING)]))
    b = Builder(833)
    open_batch(b, 0, 4000)  # d = 4016
    for _ in range(20):
        b.lit(2)
    b.lit(30)
    i = b.copy(500, 40, 2)  # [4086, 4126)
    for _ in range(12):
        b.lit(2)
    cs.append(_case("e_dense_store_crosses_4096", b, [("path", i, "dense"), ("crosses", i, K_RING)]))
    # hardly any literal bytes (a base for mutations): copies build 5 000 bytes of history, then 150
    # copies start within a byte of the ring's low edge at their own d
    b = Builder(840)
    b.lit(64)
    while b.d < 5000:
        b.copy(64, 64, 2)
    for k in range(150):
        i = b.copy(b.d - (ring_lo(b.d) + k % 3 - 1), (1, 4, 64)[k // 3 % 3], 2)
        if k % 5 == 0:
            b.lit(2)
    cs.append(_case("e_copies_along_ring_edge", b, [("path", i, "dense"), ("near_ring_edge", i)]))
    return cs


def _align_literal(b, hl, pre, sa, hdr):
    """Filler of k literals of 40 to 55 bytes (never K_DENSE tags in a window,
    no short streak) until a literal with an hdr-byte header would have its
    first byte at block offset sa (mod 16) and its output at pre (mod 16)."""
    k = 1
    while True:
        dd = 40 * k + (pre - b.d - 40 * k) % 16
        h = (sa - hdr - hl - b.s - dd) % 16 or 16  # header bytes to spend (mod 16): 1..5 per literal
        if k <= h <= 5 * k:
            break
        k += 1
    for j in range(k):
        b.lit(40 if j < k - 1 else dd - 40 * (k - 1), form=h // k + (j < h % k))


def family_f():
    """Literal writers (kLongPiece 1024, kWinLit 1024) at every source
    alignment and every `pre`.  A 17-byte literal moves from the window
    (window_literal: (d & 15) + 17 <= kWinLit), a 1 025-byte one in pieces from
    the block (long_literal)."""
    cs = []
    for ln, hl in ((17, 3), (1025, 3)):  # hl: the varint's bytes, which the alignments count on
        b = Builder(900 + ln)
        claims = []
        hdr = len(lit_header(ln))
        b.lit(1100)
        for pre in range(16):
            for sa in range(16):
                _align_literal(b, hl, pre, sa, hdr)
                i = b.lit(ln)
                claims += [("pre_salign", i, pre, sa), ("writer", i, "window_literal" if ln == 17 else "long_literal")]
        c = _case("f_all_alignments_len_%d" % ln, b, claims)
        assert c.hl == hl
        cs.append(c)
    for pre in (0, 9):
        b = Builder(920 + pre)
        claims = []
        for ln in list(range(1008, 1041)) + [2047, 2048, 2049, 4095, 4096, 4097, 65536, 70000]:
            b.lit(20 + (pre - b.d - 20) % 16)
            i = b.lit(ln)
            claims.append(("pre", i, pre))
        cs.append(_case("f_lengths_pre%d" % pre, b, claims))
    for end in (0, 1, 15):
        b = Builder(930 + end)
        b.lit(20)
        n = 3000
        while (len(uvarint(20 + n)) + b.s + 3 + n) % 16 != end:
            n += 1
        i = b.lit(n)
        cs.append(_case("f_last_literal_ends_at_%d_mod_16" % end, b, [("slen_mod16", end), ("writer", i, "long_literal")]))
    # as many header bytes as literal bytes (a base for mutations)
    b = Builder(940)
    b.lit(1025)
    for _ in range(300):
        b.lit(2, form=5)
    i = b.lit(1025)
    cs.append(_case("f_padded_headers_between_long_literals", b, [("writer", i, "long_literal"), ("path", i - 1, "dense")]))
    return cs


def family_g():
    """Output lengths (the ragged last granule) and length varints."""
    cs = []
    for n in list(range(0, 34)) + [1023, 1024, 1025, 4095, 4096, 4097]:
        b = Builder(1000 + n)
        k = 0
        while b.d < n:
            left = n - b.d
            if k % 2 and b.d >= 3:
                b.copy(3, min(left, 7), 2)
            else:
                b.lit(min(left, 5 if n < 100 else 300))
            k += 1
        cs.append(_case("g_len_%d" % n, b, [("dlen", n)]))
        if n >= 28:  # the same length from tags of at most 5 bytes: the dense store's last granule
            b = Builder(1050 + n)
            b.lit(3)
            while b.d < n:
                b.copy(2, min(n - b.d, 5), 2) if len(b.log) % 2 else b.lit(min(n - b.d, 2))
            cs.append(_case("g_len_%d_dense" % n, b, [("dlen", n), ("path", b.last, "dense")]))
    for size in (2, 3, 4, 5, 10):
        b = Builder(1100 + size)
        b.lit(40)
        b.copy(7, 30, 2)
        # a 10-byte varint is the longest binary.Uvarint takes; other Snappy decoders stop at 5
        cs.append(_case("g_varint_of_%d_bytes" % size, b, [("hl", size)], varint_pad=size, pyarrow=size <= 5))
    return cs


def family_g_corrupt():
    return [Case("g_zero_length_then_tag", uvarint(0) + lit(b"a"), None, path="header"),
            Case("g_varint_above_2_32", uvarint(1 << 32) + lit(b"a"), None, path="header"),
            Case("g_varint_of_11_bytes", uvarint(5, 11) + lit(b"abcde"), None, path="header")]


def _fill_block(b, upto):
    """Mixed tags up to output position `upto` (at most the next multiple of
    K_SUB), none crossing it, every copy inside its own sub-block."""
    k = len(b.log)
    while b.d < upto:
        left = upto - b.d
        room = b.d % K_SUB
        if k % 4 == 0 or room < 70:
            b.lit(min(left, 37 + 13 * (k % 5)))
        elif k % 4 == 1:
            b.lit(min(left, 2500))
        else:
            b.copy(1 + (k * 7) % min(room, 3000), min(left, 1 + (k * 11) % 64), 2)
        k += 1


def family_h():
    """Split (kSnapSub 65536, kSnapSeg 4096)."""
    cs = []
    for n in (65535, 65536, 65537, 131072):
        b = Builder(1200 + n % 100)
        for base in range(0, n, K_SUB):
            _fill_block(b, min(base + K_SUB, n))
        cs.append(_case("h_len_%d" % n, b, [("dlen", n), ("shaped", True)]))
    b = Builder(1209)
    _fill_block(b, K_SUB)
    b.lit(1)
    cs.append(_case("h_last_sub_block_of_1_byte", b, [("dlen", K_SUB + 1), ("shaped", True)]))
    b = Builder(1210)
    _fill_block(b, K_SUB - 40)
    i = b.copy(100, 40, 2)
    _fill_block(b, K_SUB + 3000)
    cs.append(_case("h_tag_ends_on_boundary", b, [("ends_at", i, K_SUB), ("shaped", True)]))
    b = Builder(1211)
    _fill_block(b, K_SUB - 39)
    i = b.lit(40)
    _fill_block(b, K_SUB + 3000)
    cs.append(_case("h_literal_crosses_boundary_by_1", b, [("ends_at", i, K_SUB + 1), ("shaped", False)]))
    b = Builder(1212)
    _fill_block(b, K_SUB - 39)
    i = b.copy(100, 40, 2)
    _fill_block(b, K_SUB + 3000)
    cs.append(_case("h_copy_crosses_boundary_by_1", b, [("ends_at", i, K_SUB + 1), ("shaped", False)]))
    for extra in (0, 1):
        b = Builder(1213 + extra)
        _fill_block(b, K_SUB)
        b.lit(700)
        i = b.copy(b.d - K_SUB + extra, 30, 2)
        _fill_block(b, K_SUB + 3000)
        cs.append(_case("h_copy_source_at_sub_block_start_%+d" % -extra, b,
                        [("src_minus_base", i, -extra), ("shaped", not extra)]))
    # sub-block 1's first tag follows a literal that ends at segment-relative position rel
    for rel in (63, 64, 65):
        b = Builder(1220 + rel)
        _fill_block(b, 30000)
        n = 20000
        ts = b.s + (K_SUB - n - b.d) + 1
        ts += (rel - (ts + 3 + n)) % K_SEG
        b.to(ts, K_SUB - n)
        b.lit(n)
        j = b.lit(33)
        _fill_block(b, K_SUB + 5000)
        cs.append(_case("h_sub_block_starts_at_segment_byte_%d" % rel, b,
                        [("seg_rel", j, rel), ("starts_at", j, K_SUB), ("shaped", True)]))
    # one literal carries the chain from one segment into the first 64 bytes of the k-th after it
    for k in (7, 8, 15, 16, 17):
        b = Builder(1230 + k)
        b.to(4000, 1000)
        i = b.lit(k * K_SEG - 4000 + 10 - 3)
        shaped = b.d <= K_SUB
        _fill_block(b, -(-b.d // K_SUB) * K_SUB)
        _fill_block(b, b.d + 4000)
        cs.append(_case("h_literal_jumps_%d_segments" % k, b, [("seg_jump", i, k), ("shaped", shaped)]))
    # two sub-blocks of 64-byte copies (a base for mutations)
    b = Builder(1235)
    for end in (K_SUB, 70000):
        b.lit(64)
        while b.d + 64 <= end:
            b.copy(64, 64, 2)
        b.to_d(end)
    cs.append(_case("h_two_sub_blocks_of_copies", b, [("dlen", 70000), ("shaped", True)]))
    for delta in (-1, 0, 1):
        b = Builder(1240 + delta + 1)
        _fill_block(b, K_SUB)
        _fill_block(b, K_SUB + 100)
        target = ((b.s + 5000) // K_SEG + 1) * K_SEG + delta
        n = target - b.s - 3
        assert 256 < n <= K_SUB - 100
        b.lit(n)
        cs.append(_case("h_compressed_length_4096k%+d" % delta, b, [("clen_minus_hdr_mod", delta % K_SEG), ("shaped", True)]))
    return cs


def _prefix(path):
    """A valid start after which the next tag is met by the dense check of
    run(), by the check of a window too sparse for a batch, by serial(), or
    ('split') by the chain search and the decode of sub-block 1."""
    b = Builder(1300)
    if path == "dense":
        open_batch(b, 4)
        for _ in range(12):
            b.lit(2)
    elif path == "sparse":
        open_batch(b, 4)
        b.lit(30)
    elif path == "serial":
        open_tags(b, 4)
    else:
        _fill_block(b, K_SUB)
        b.lit(300)
        for _ in range(K_STREAK):
            b.lit(3)
        for _ in range(12):
            b.lit(2)
    return b


def family_i():
    """Directed corruptions, each once per path."""
    cs = []
    for path in ("dense", "sparse", "serial", "split"):
        b = _prefix(path)
        d0, body = b.d, bytes(b.comp)
        dense_tail = lit(b"ab") * 12 if path in ("dense", "split") else b""

        def mk(name, bad, out_len, tail=b"", declared=None):
            n = d0 + out_len + len(tail) // 3 * 2 if declared is None else declared
            cs.append(Case("i_%s_%s" % (name, path), uvarint(n) + body + bad + tail, None, path=path))

        mk("offset_d_plus_1", copy(d0 + 1, 8, 4), 8, dense_tail)
        mk("offset_0", copy(0, 8, 2), 8, dense_tail)
        mk("literal_1_past_block", lit_header(10) + b"123456789", 10)
        mk("literal_length_ffffffff", bytes([63 << 2]) + b"\xff\xff\xff\xff" + b"abcd", 4)
        mk("overshoots_by_1", copy(3, 9, 2), 8)
        mk("ends_1_byte_short", copy(3, 8, 2), 9)
        mk("header_truncated", bytes([61 << 2, 5]), 6)
    return cs


FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e, "f": family_f, "g": family_g,
            "h": family_h}


def valid_cases():
    return [c for f in FAMILIES.values() for c in f()]


def corrupt_cases():
    return family_g_corrupt() + family_i()
