"""ZSTD decode on compressed blocks that libzstd's encoder never emits.

Every compressed block tests/test_zstd.py and tests/test_zstd_model.py feed
the decoder was written by libzstd's encoder, so k_zstd only ever saw what one
encoder chooses.  Here the blocks are built by hand (tests/zstd_build.py: a
backward bit writer, FSE tables from any normalized count, the state choice run
backwards, Huffman trees from chosen code lengths, every header format)
together with a plain model of the format:

    literals are appended      match (offset, length): out.append(out[-offset]), length times
    repeat offsets by RFC 8878 3.1.1.5, from (1, 4, 8) in every frame

For every valid stream three things agree byte for byte on the CPU: the plain
model (B.expand), libzstd (through pyarrow, with the exact size) and the host
model (tools/zstd_model.cpp, the Decoder of pqg_zstd.h with a serial IO
policy); libzstd accepts every one of them.  Every invalid stream is rejected
by libzstd and gets ZSTD from the model.  The whole set runs once more through
the model's stand-alone AddressSanitizer / UBSan build.  The generators follow
the output and the repeat offsets themselves, so no generated stream is ever
dropped because a reference rejects it.

The GPU tests run every family two ways: each stream through
pqg_block_decompress with cap = len + 100 (nothing may be written past the
decoded bytes), and all of a family's streams as the PLAIN INT64 V1 pages of
one chunk in one decode call, so that unlike pages sit side by side in
kQueueZstd and one page's tables are live in LDS when the next one starts on
the same persistent wave.  Invalid streams go as the middle page of
good + bad + good (ZSTD, error page 1) and as bare blocks.

What the families are sized by (pqg_zstd.h, pqg_zstd.hip, pqg_wavecopy.h):
  A  seq_table / read_ncount / fse_build: the accuracy-log limits 9 / 8 / 9 (and 5 below), kMaxLL 35,
     kMaxOF 31, kMaxML 52, the -1 symbols placed from the table's top, the 2-bit zero-run flags chained
     3, 3, ..., the `symb <= max_sym` exits, fse_rle, Tables::fse_valid (Repeat mode; reset per frame)
  B  ll_base / ll_bits / ml_base / ml_bits at every code boundary, codes 35 and 52 with 16 extra bits,
     parse_seq_header's three forms at 127 / 128 and 0x7EFF / 0x7F00, offset codes up to what the output allows
  C  rep_update: every row of the rule with ll > 0 and ll == 0, rep1 - 1, across blocks, reset per frame
  D  huf_read_table: direct weights up to 128 listed (header byte 255), FSE weights up to 255 listed
     (the `nw > 253` checks), table logs 5 and 6, kHufLogMax 12; huf_stream on one lane and on four
     (seg = (n + 3) / 4, the `fast` rule of four streams of >= 8 bytes); parse_lit_header's size formats;
     Tables::huf_log (treeless; reset per frame); kWsBytes = kBlockMax + 64
  E  WaveCopy::copy<false> (raw literals), out_fill (RLE literals), copy<true> from ws + lp (Huffman):
     head = (4 - dst & 3) & 3 bytes, a body of dwords, 64 lanes x 4 = 256 bytes a round, a tail of < 4
     bytes; the funnel shift sh = (src & 3) * 8
  F  WaveCopy::out_match: `off >= len` (dword copy) against the bytewise overlap path in rounds of 64, and
     `src_end > stored`: the drain of the wave's own stores before a match reads them
  G  parse_frame_header, Decoder::block_max = min(window, kBlockMax), the checksum's out_get through L2
  H  all of it, at random

The mode triples over Predefined, RLE and FSE are 27; each stands as a
frame's first, second and third block (81 blocks).

The oversized block: a compressed block whose sequences regenerate more than
the block maximum is decoded (output stays bounded by cap); see
test_oversized_block."""
import functools
import random

import numpy as np
import pytest

import zstd_build as B
import zstd_util as Z
from pqgpu import abi

pa = pytest.importorskip("pyarrow")

ZSTD = abi.STATUS_CODES["ZSTD"]
KB = 1024
BMAX = 128 * KB
WHICH = ("ll", "of", "ml")


def R(*key):
    return random.Random(repr(key))


def rb(rng, n, alpha=None):
    if alpha is None:
        return rng.randbytes(n)
    return bytes(rng.choice(alpha) for _ in range(n))


class Cases:
    def __init__(self):
        self.valid, self.invalid = [], []

    def ok(self, name, *fbs, **kw):
        """A stream of the frames fbs; what it decodes to is the plain model's answer."""
        z = b"".join(fb.frame(**kw) for fb in fbs)
        exp = B.expand([fb.desc for fb in fbs])
        assert exp == b"".join(bytes(fb.p.out) for fb in fbs), name
        for fb in fbs:  # every compressed block within the block maximum (see test_oversized_block)
            bm = min(BMAX, _window(kw, fb))
            for d, b in zip(fb.desc, fb.blocks):
                assert d[0] != "comp" or (len(d[1]) + sum(s[2] for s in d[2]) <= bm and len(b[1]) <= bm), name
        self.valid.append((name, z, exp))

    def bad(self, name, *fbs, z=None, **kw):
        """A stream meant to be invalid; n: the size it would decode to."""
        if z is None:
            z = b"".join(fb.frame(**kw) for fb in fbs)
        self.invalid.append((name, z, sum(len(fb.p.out) for fb in fbs)))


def _window(kw, fb):
    if kw.get("single"):
        return len(fb.p.out)
    wd = kw.get("window", 0x50)
    return (1 << (10 + (wd >> 3))) + ((1 << (10 + (wd >> 3))) >> 3) * (wd & 7)


def rand_seqs(fb, rng, n, room, max_ll=24, max_ml=40, rep_p=0.35, alpha=None):
    """Up to n sequences of random legal choices that regenerate at most room bytes: the generator follows
    the position and the repeat offsets, so every offset is valid.  Returns the bytes regenerated."""
    used = 0
    for _ in range(n):
        ll = rng.choice((0, 0, 1, 2, 3, rng.randint(0, max_ll)))
        if fb.pos == 0 and ll == 0:
            ll = 1
        ml = rng.choice((3, 4, rng.randint(3, max_ml)))
        if used + ll + ml > room:
            break
        ofv = None
        if rng.random() < rep_p:
            c = rng.randint(1, 3)
            off, _ = B.rep_rule(fb.rep, c, ll == 0)
            if off is not None and off <= fb.pos + ll:
                ofv = c
        if ofv is None:
            m = fb.pos + ll
            hi = min(m, 1 << rng.randint(0, m.bit_length()))
            ofv = rng.randint(max(1, hi // 2), hi) + 3
        fb.seq(rb(rng, ll, alpha), ofv, ml)
        used += ll + ml
    return used


def use_codes(fb, rng, which, codes, top=False):
    """One sequence per code of table `which` (its lowest value, top: its highest); the other two fields small."""
    for c in codes:
        ll, ml, ofv = rng.randint(1, 4), rng.randint(3, 6), None
        if which == "ll":
            ll = B.LL_BASE[c] + ((1 << B.LL_BITS[c]) - 1 if top else 0)
        elif which == "ml":
            ml = B.ML_BASE[c] + ((1 << B.ML_BITS[c]) - 1 if top else 0)
        else:
            ofv = (2 << c) - 1 if top and c else 1 << c
            if ofv > 3:
                ll = max(ll, ofv - 3 - fb.pos)
        if fb.pos + ll == 0:
            ll = 1
        if ofv is None:
            ofv = rng.randint(1, min(fb.pos + ll, 16)) + 3
        elif ofv <= 3:  # a repeat code: it must name a valid offset here
            off, _ = B.rep_rule(fb.rep, ofv, ll == 0)
            assert off is not None and off <= fb.pos + ll, (ofv, fb.rep, fb.pos)
        fb.seq(rb(rng, ll), ofv, ml)


def const_seqs(fb, rng, n=5):
    """n sequences of one LL, OF and ML code each (what RLE mode needs)."""
    for _ in range(n):
        fb.seq(rb(rng, 2), 5, 4)


def predef_tab(which):
    return B.Fse(B.DEFAULT[which][1], B.DEFAULT[which][0])


# ---- A: sequence tables
def _fam_A():
    c = Cases()
    for w in WHICH:
        for log in (5, B.MAX_LOG[w]):
            rng = R("A", w, log)
            fb = B.FrameB(rng.random())
            rand_seqs(fb, rng, 40, 4000, max_ml=30)
            fb.tail(rb(rng, 7))
            fb.end(**{w: "fse"}, opts={w: {"log": log}})
            c.ok("fse_%s_log%d" % (w, log), fb)
        # -1 probabilities, on the last symbol and on symbol 0 too
        rng = R("A", w, "less1")
        fb = B.FrameB(rng.random())
        rand_seqs(fb, rng, 60, 6000)
        used = sorted({(B.ll_code(s[0]), B.of_code(s[1]), B.ml_code(s[2]))[WHICH.index(w)][0] for s in fb.seqs})
        less1 = {0, B.MAX_SYM[w]} | set(used[1::2])
        fb.end(**{w: "fse"}, opts={w: {"log": B.MAX_LOG[w] - 1, "less1": less1}})
        c.ok("less1_%s" % w, fb)
        # zero runs: a zero probability, then r more of them by the 2-bit flags
        for r in (0, 1, 2, 3, 4, 6, 7, 9, 10):
            rng = R("A", w, "run", r)
            fb = B.FrameB(rng.random())
            fb.raw(rb(rng, 3))
            hi = 2 + r
            if w == "of":
                use_codes(fb, rng, "of", [hi])
                fb.seq(rb(rng, 2), 1, 4)
                fb.seq(rb(rng, 1), 1, 3)
                use_codes(fb, rng, "of", [hi], top=True)
            else:
                use_codes(fb, rng, w, [hi, 0, 0, hi])
            a = rng.randint(1, 63)
            fb.end(**{w: "fse"}, opts={w: {"log": 6, "norm": [a] + [0] * (1 + r) + [64 - a]}})
            c.ok("zero_run_%s_%d" % (w, r), fb)
        # a run that reaches the alphabet's last symbol; the last probability lands on max_sym exactly
        for last in (3, -1):
            rng = R("A", w, "last", last)
            fb = B.FrameB(rng.random())
            fb.raw(rb(rng, 5))
            use_codes(fb, rng, w, [0, 0, 0])
            norm = [32 - abs(last)] + [0] * (B.MAX_SYM[w] - 1) + [last]
            fb.end(**{w: "fse"}, opts={w: {"log": 5, "norm": norm}})
            c.ok("run_to_last_%s_%d" % (w, last), fb)
        rng = R("A", w, "dense_last")
        fb = B.FrameB(rng.random())
        rand_seqs(fb, rng, 30, 3000)
        fb.end(**{w: "fse"}, opts={w: {"log": B.MAX_LOG[w], "extra": set(range(B.MAX_SYM[w] - 6, B.MAX_SYM[w] + 1))}})
        c.ok("dense_to_last_%s" % w, fb)
    # RLE mode with symbol 0 and the largest symbol (for offsets: the largest the output allows)
    rng = R("A", "rle")
    for w, sym in (("ll", 0), ("ll", 35), ("of", 0), ("of", 15), ("ml", 0), ("ml", 52)):
        fb = B.FrameB(rng.random())
        fb.raw(rb(rng, 40000 if (w, sym) == ("of", 15) else 9))
        use_codes(fb, rng, w, [sym] * (1 if sym in (35, 52) else 4))
        fb.end(**{w: "rle"})
        c.ok("rle_%s_%d" % (w, sym), fb)
    # predefined tables over their symbols (the codes with 15 and 16 extra bits are family B's)
    fb = B.FrameB(1)
    use_codes(fb, rng, "ll", range(34))
    fb.end()
    use_codes(fb, rng, "ml", range(51))
    fb.end()
    use_codes(fb, rng, "of", list(range(2, 15)) + [0, 1])
    fb.end()
    c.ok("predef_every_symbol", fb)
    # all 27 mode triples over Predefined, RLE, FSE, each as a frame's first, second and third block (81
    # blocks): a table of one block must not leak into the next
    modes = ("predef", "rle", "fse")
    triples = [(a, b, d) for a in modes for b in modes for d in modes]
    for t in range(27):
        rng = R("A", "modes", t)
        fb = B.FrameB(rng.random())
        for j in range(3):
            ll_, of_, ml_ = triples[(t + 10 * j) % 27]
            for _ in range(5):  # one code per table (what RLE mode needs), another one in every block
                fb.seq(rb(rng, 2 + j), 5 + j, 4 + j)
            fb.tail(rb(rng, 3))
            fb.end(ll=ll_, of=of_, ml=ml_)
        c.ok("modes_%s_%s_%s" % triples[t], fb)
    # Repeat of each table on its own in the second block and of all three in the third, after a
    # Predefined, an RLE and an FSE table; the same across a block with no sequences
    for w in WHICH:
        for m in modes:
            for gap in (False, True):
                rng = R("A", "repeat", w, m, gap)
                fb = B.FrameB(rng.random())
                const_seqs(fb, rng)
                fb.end(ll=m, of=m, ml=m)
                if gap:
                    fb.tail(rb(rng, 11))
                    fb.end()
                const_seqs(fb, rng, 3)
                fb.end(**{w: "repeat"})
                const_seqs(fb, rng, 70)
                fb.end(ll="repeat", of="repeat", ml="repeat")
                c.ok("repeat_%s_after_%s%s" % (w, m, "_gap" if gap else ""), fb)
    # ---- invalid
    for w in WHICH:
        rng = R("A", "bad", w)

        def one(first=None):
            fbs = []
            if first:
                f1 = B.FrameB(1)
                const_seqs(f1, rng)
                f1.end(ll=first, of=first, ml=first)
                fbs.append(f1)
            fb = B.FrameB(2)
            const_seqs(fb, rng)
            return fbs, fb

        fbs, fb = one()
        fb.tab = {k: predef_tab(k) for k in WHICH}
        fb.end(**{w: "repeat"})
        c.bad("repeat_first_block_%s" % w, fb)
        fbs, fb = one("fse")
        fb.tab = dict(fbs[0].tab)
        fb.end(**{w: "repeat"})
        c.bad("repeat_second_frame_%s" % w, fbs[0], fb)
        code = {"ll": 2, "of": 2, "ml": 1}[w]
        fbs, fb = one()
        fb.end(**{w: "rle"}, opts={w: {"desc": bytes([B.MAX_SYM[w] + 1]), "tab": B.Fse.rle(code)}})
        c.bad("rle_symbol_%s" % w, fb)
        fbs, fb = one()
        fb.end(**{w: "fse"}, opts={w: {"log": B.MAX_LOG[w] + 1}})
        c.bad("accuracy_log_%s" % w, fb)
        # a count that needs a symbol above max_sym; one that ends short of 2^log at max_sym.  (A value
        # above what is left cannot be written: the field's largest value is exactly what is left.)
        fbs, fb = one()
        norm = [0] * (B.MAX_SYM[w] + 2)
        norm[code], norm[-1] = 60, 4
        fb.end(**{w: "fse"}, opts={w: {"desc": B.write_ncount(norm, 6), "tab": B.Fse(norm, 6)}})
        c.bad("symbol_above_max_%s" % w, fb)
        fbs, fb = one()
        short = [0] * (B.MAX_SYM[w] + 1)
        short[code], short[-1] = 60, 3
        norm = list(short)
        norm[-1] = 4
        fb.end(**{w: "fse"}, opts={w: {"desc": B.write_ncount(short, 6), "tab": B.Fse(norm, 6)}})
        c.bad("count_short_%s" % w, fb)
    for bits in (1, 2, 3):
        fb = B.FrameB(3)
        const_seqs(fb, rng)
        fb.end(modes_or=bits)
        c.bad("reserved_modes_%d" % bits, fb)
    fb = B.FrameB(4)  # an RLE offset code of 31: 31 extra bits, an offset no output holds
    fb.raw(rb(rng, 20))
    fb.force(b"ab", (1 << 31) + 12345, 4)
    fb.end(of="rle")
    c.bad("rle_of_31", fb)
    return c


# ---- B: codes and lengths
def _fam_B():
    c = Cases()
    rng = R("B")
    for w, n, first in (("ll", 36, 16), ("ml", 53, 32)):
        bits = B.LL_BITS if w == "ll" else B.ML_BITS
        small = [k for k in range(first, n) if bits[k] <= 12]
        fb = B.FrameB(1)
        use_codes(fb, rng, w, [k - 1 for k in small], top=True)  # base - 1 ...
        fb.end()
        use_codes(fb, rng, w, small)                             # ... and base
        fb.end()
        c.ok("%s_boundaries" % w, fb)
        for k in range(first, n):
            if bits[k] <= 12:
                continue
            for top in (False, True):
                if bits[k] == 16 and top:
                    continue
                fb = B.FrameB(k)
                if w == "ml":
                    fb.raw(rb(rng, 3))
                use_codes(fb, rng, w, [k], top=top)
                fb.end()
                c.ok("%s_code%d_%s" % (w, k, "top" if top else "base"), fb)
    # codes 35 and 52 with the largest extra bits a block holds
    fb = B.FrameB(1)
    fb.new(rb(rng, BMAX - 3, bytes(range(5))), 77, 3)  # Huffman literals: raw ones would not fit the block
    fb.end(lit="huf", four=True)
    c.ok("ll_131069", fb)
    fb = B.FrameB(1)
    fb.new(rb(rng, 3), 2, BMAX - 3)
    fb.end()
    c.ok("ml_131069", fb)
    # the sequence-count forms
    for n, form in ((0, 0), (1, 0), (127, 0), (127, 1), (128, 1), (129, 1), (5, 1), (0x7EFF, 1), (0x7F00, 2)):
        fb = B.FrameB(n)
        fb.raw(rb(rng, 8))
        for i in range(n):
            fb.seq(rb(rng, i & 1), rng.randint(1, 8) + 3, 3)
        fb.tail(rb(rng, 3))
        fb.end(form=form)
        c.ok("nseq_%d_form%d" % (n, form), fb)
    # offset codes from 2 up to the largest the output allows
    fb = B.FrameB(1)
    use_codes(fb, rng, "of", range(2, 16))
    use_codes(fb, rng, "of", range(2, 15), top=True)
    fb.end()
    c.ok("of_codes_2_15", fb)
    fb = B.FrameB(1)
    fb.raw(rb(rng, BMAX))
    for off in (65533, 131068, 131069, BMAX + 40):
        fb.new(rb(rng, 5), off, 9)
    fb.end()
    c.ok("of_codes_16_17", fb)
    # ---- invalid
    fb = B.FrameB(1)
    fb.new(rb(rng, 9), 4, 5)
    fb.force(rb(rng, 4), 5, 3, ll=5)
    fb.end()
    c.bad("ll_beyond_literals", fb)
    for d in (-1, 1):
        fb = B.FrameB(1)
        for _ in range(6):
            fb.new(rb(rng, 3), 2, 4)
        fb.end(nseq=6 + d)
        c.bad("nseq_%+d" % d, fb)
    fb = B.FrameB(1)
    for _ in range(6):
        fb.new(rb(rng, 3), 2, 4)
    fb.push(fb.literals() + fb.sequences() + b"\x00")
    c.bad("last_byte_zero", fb)
    return c


# ---- C: repeat offsets
ROWS = [(ofv, ll0) for ofv in (1, 2, 3) for ll0 in (False, True)]


def _fam_C():
    c = Cases()
    seen = set()

    def row(fb, rng, ofv, ll0):
        """Force one row of the rule; a new offset first where the row would not be valid here."""
        ll = 0 if ll0 else rng.randint(1, 5)
        off, _ = B.rep_rule(fb.rep, ofv, ll0)
        if off is None or off > fb.pos + ll:
            fb.new(rb(rng, 2), rng.randint(2, min(fb.pos + 2, 40)), 3)
            off, _ = B.rep_rule(fb.rep, ofv, ll0)
        assert off is not None and off <= fb.pos + ll
        fb.seq(rb(rng, ll), ofv, rng.randint(3, 12))
        seen.add((ofv, ll0))

    for k in range(12):  # every row, in a shuffled order, in one block; then across blocks and frames
        rng = R("C", k)
        order = ROWS * 2
        rng.shuffle(order)
        f1 = B.FrameB(k)
        f1.new(rb(rng, 30), rng.randint(2, 30), 4)
        for r in order[:8]:
            row(f1, rng, *r)
        f1.end()
        for r in order[8:]:  # the history of the first block
            row(f1, rng, *r)
        f1.end()
        f2 = B.FrameB(k + 100)  # (1, 4, 8) again: repeat codes 1 .. 3 with just enough output
        f2.seq(rb(rng, 9), [1, 2, 3][k % 3], 5)
        c2 = [1, 2, 3][(k // 3) % 3]
        off, _ = B.rep_rule(f2.rep, c2, True)
        if off is not None and off <= f2.pos:
            f2.seq(b"", c2, 4)
        f2.end()
        c.ok("rows_%d" % k, f1, f2)
    assert seen == set(ROWS)
    # rep1 - 1 as a valid offset, with rep1 == 2 (offset 1)
    fb = B.FrameB(1)
    fb.new(b"abcdef", 2, 3)
    fb.seq(b"", 3, 5)
    assert fb.rep[0] == 1
    fb.end()
    c.ok("rep1_minus_1_is_1", fb)
    for k in range(10):  # chains of 300 sequences that mix new and repeat offsets
        rng = R("C", "chain", k)
        fb = B.FrameB(k)
        rand_seqs(fb, rng, 150, 20000, max_ll=6, max_ml=12, rep_p=0.6)
        fb.end(lit="raw")
        rand_seqs(fb, rng, 150, 20000, max_ll=6, max_ml=12, rep_p=0.6)
        fb.end()
        c.ok("chain_%d" % k, fb)
    # ---- invalid
    rng = R("C", "bad")
    fb = B.FrameB(1)
    fb.raw(rb(rng, 12))
    fb.force(b"", 3, 4)
    fb.end()
    c.bad("rep1_minus_1_is_0", fb)
    fb = B.FrameB(1)
    fb.force(rb(rng, 7), 3, 4)
    fb.end()
    c.bad("rep3_with_7_bytes", fb)
    f1 = B.FrameB(1)
    f1.new(rb(rng, 100), 50, 20)
    f1.end()
    f2 = B.FrameB(2)
    f2.force(rb(rng, 10), 11 + 3, 4)
    f2.end()
    c.bad("offset_into_first_frame", f1, f2)
    return c


# ---- D: Huffman literals
def huf_for(rng, nsym, maxlen, flat=False, top=None):
    """A tree over nsym symbols of the byte values below top (the last is top - 1)."""
    top = nsym if top is None else top
    ln = B.huf_lengths(nsym, maxlen, rng, flat)
    rng.shuffle(ln)
    syms = sorted(rng.sample(range(top - 1), nsym - 1)) + [top - 1]
    lens = [0] * top
    for s, l in zip(syms, ln):
        lens[s] = l
    return B.Huf(lens), bytes(syms)


def _fam_D():
    c = Cases()

    def lits_block(fb, rng, h, alpha, n, seqs=True, **kw):
        """A block of n literals with a few sequences among them where they fit."""
        data = rb(rng, n, alpha)
        at = 0
        if seqs and n >= 12 and rng.random() < 0.5:
            for _ in range(rng.randint(1, 3)):
                k = rng.randint(1, n // 4)
                fb.new(data[at:at + k], rng.randint(1, fb.pos + k), rng.randint(3, 9))
                at += k
        fb.tail(data[at:])
        fb.end(huf=h, **kw)

    def one(name, nsym, maxlen, desc, n, four=False, flat=False, top=None, wlog=6, sf=None, seqs=True):
        rng = R("D", name)
        fb = B.FrameB(rng.random())
        h, alpha = huf_for(rng, nsym, maxlen, flat, top)
        lits_block(fb, rng, h, alpha, n, lit="huf", desc=desc, four=four, wlog=wlog, sf=sf, seqs=seqs)
        c.ok(name, fb)

    for nsym, top in ((2, 2), (2, 9), (3, 3), (4, 20), (127, 127), (128, 128), (129, 129), (40, 129)):
        one("direct_%d_of_%d" % (nsym, top), nsym, min(11, nsym - 1, 3 + nsym // 8), "direct", 500, top=top)
    for nsym, top in ((3, 3), (129, 129), (200, 200), (255, 255), (256, 256), (130, 256), (3, 256)):
        for wlog in (5, 6):
            one("fse_%d_of_%d_log%d" % (nsym, top, wlog), nsym, min(10, nsym - 1), "fse", 2000, flat=True, top=top,
                wlog=wlog, four=True)
    for maxlen, nsym in ((1, 2), (2, 3), (2, 4), (8, 9), (8, 100), (11, 12), (11, 128), (12, 13), (12, 129)):
        one("maxlen_%d_%dsym" % (maxlen, nsym), nsym, maxlen, "direct", 3000 if nsym > 50 else 1000, four=nsym > 50)
    one("maxlen_12_fse", 256, 12, "fse", 3000, flat=True, four=True)
    for n in range(1, 1024):  # every size one stream holds
        one("one_stream_%d" % n, 9, 5, "direct", n)
    for n in (6, 7, 8, 9, 10, 11, 12, 13) + tuple(range(1021, 1028)):
        one("four_streams_%d" % n, 9, 5, "direct", n, four=True)
    # four streams: all of >= 8 bytes (libzstd's fast loop), one of < 8 bytes
    for name in ("all_long", "fourth_short", "first_short"):
        rng = R("D", name)
        fb = B.FrameB(1)
        h = B.Huf([1, 3, 3, 3, 4, 4])
        seg = 40
        parts = [rb(rng, seg, bytes(range(1, 6))) for _ in range(4)]
        if name == "fourth_short":
            parts[3] = bytes(seg - 3)
        if name == "first_short":
            parts[0] = bytes(seg)
        data = b"".join(parts)
        assert (len(data) + 3) // 4 == seg
        fb.tail(data)
        fb.end(lit="huf", huf=h, four=True)
        c.ok("four_%s" % name, fb)
    # the size formats of four streams at their edges (and a small section in the widest)
    for n, sf in ((1023, 1), (1023, 2), (1023, 3), (1024, 2), (16383, 2), (16383, 3), (16384, 3), (100, 3), (100, 2)):
        one("size_format_%d_sf%d" % (n, sf), 6, 4, "direct", n, four=True, sf=sf)
    one("literals_131072", 5, 3, "fse", BMAX, four=True, seqs=False)
    # treeless literals in the second and third blocks, with one and four streams, and across blocks of
    # raw and RLE literals
    for between in (None, "raw", "rle"):
        for four in (False, True):
            rng = R("D", "treeless", between, four)
            fb = B.FrameB(rng.random())
            h, alpha = huf_for(rng, 12, 6)
            lits_block(fb, rng, h, alpha, 300, lit="huf", desc="direct", four=not four)
            if between:
                fb.new(b"\x07" * 20, 5, 6)
                fb.tail(b"\x07" * 3)
                fb.end(lit=between)
            lits_block(fb, rng, None, alpha, 200, lit="treeless", four=four)
            lits_block(fb, rng, None, alpha, 77, lit="treeless", four=not four)
            c.ok("treeless_%s_%d" % (between, 4 if four else 1), fb)
    # ---- invalid
    rng = R("D", "bad")
    h, alpha = huf_for(rng, 12, 6)
    for four in (False, True):
        fb = B.FrameB(1)
        fb.huf = h
        fb.tail(rb(rng, 100, alpha))
        fb.end(lit="treeless", four=four)
        c.bad("treeless_first_%d" % (4 if four else 1), fb)
        f1 = B.FrameB(1)
        f1.tail(rb(rng, 100, alpha))
        f1.end(lit="huf", huf=h, four=four)
        f2 = B.FrameB(2)
        f2.huf = h
        f2.tail(rb(rng, 100, alpha))
        f2.end(lit="treeless", four=four)
        c.bad("treeless_second_frame_%d" % (4 if four else 1), f1, f2)
    fb = B.FrameB(1)
    fb.tail(rb(rng, 5, alpha))
    fb.end(lit="huf", huf=h, four=True)
    c.bad("four_streams_of_5", fb)

    def patched(name, n, four, patch):
        fb = B.FrameB(1)
        fb.tail(rb(rng, n, alpha))
        tree = h.direct()
        body = patch(tree, B.huf_streams(h, bytes(fb.lits), four), bytes(fb.lits))
        fb.push(B.lit_header(2, 1 if four else 0, n, len(body)) + body + B.seq_count(0))
        c.bad(name, fb)

    patched("jump_table_past_section", 200, True, lambda t, s, d: t + (len(s)).to_bytes(2, "little") + s[2:])
    patched("one_stream_left_over", 50, False, lambda t, s, d: t + h.stream(d + d[:1]))
    patched("one_stream_short", 50, False, lambda t, s, d: t + h.stream(d[:-1]))
    patched("direct_weights_missing", 50, False, lambda t, s, d: bytes([255]) + bytes([0x11] * 10))
    return c


# ---- E: literal routing and the wave copies
RUNS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 260, 1023, 1024)
HUF6 = [2, 2, 2, 3, 4, 4]


def _route(src, d, s, run):
    """A frame whose second literal run has `run` bytes, lands on output offset = d mod 4 (d swept over
    0..3) and starts at literal offset lp = 4 + s; trailing literals of the same length."""
    rng = R("E", src, d, s, run)
    fb = B.FrameB(rng.random())
    fb.raw(rb(rng, 8 + d))
    fill = rng.randint(1, 255)

    def lit(n):
        if src == "raw":
            return rb(rng, n)
        if src == "rle":
            return bytes([fill]) * n
        return rb(rng, n, bytes(range(6)))

    for n in (4 + s, run):  # each run, then a short match out of the frame's first bytes
        k = rng.randint(0, 4)
        fb.new(lit(n), fb.pos + n - k, rng.randint(3, 4))
    fb.tail(lit(run))
    kw = {}
    if src == "huf":
        kw = dict(huf=B.Huf(HUF6), four=len(fb.lits) >= 6 and (rng.random() < 0.6 or len(fb.lits) > 1023), desc=rng.choice(("direct", "fse")))
    fb.end(lit=src, **kw)
    return fb


def _fam_E():
    c = Cases()
    for src in ("raw", "rle", "huf"):
        for d in range(4):
            for s in range(4):
                for run in RUNS:
                    c.ok("%s_d%d_s%d_run%d" % (src, d, s, run), _route(src, d, s, run))
            for n in (1, 2, 3, 4, 5, 6, 63, 64, 65, 255, 256, 257, 260, 1023, 1024):  # no sequences at all
                rng = R("E", "nseq0", src, d, n)
                fb = B.FrameB(rng.random())
                if d:
                    fb.raw(rb(rng, d))
                kw = {}
                if src == "huf":
                    kw = dict(huf=B.Huf(HUF6), four=n >= 6 and n & 1 == 0)
                    fb.tail(rb(rng, n, bytes(range(6))))
                else:
                    fb.tail(rb(rng, n) if src == "raw" else bytes([n & 255]) * n)
                fb.end(lit=src, **kw)
                c.ok("%s_d%d_only%d" % (src, d, n), fb)
    return c


# ---- F: matches and the stored watermark
def _watermark(fb, rng, run, delta, ml=8):
    """A match that reads its own sequence's literals (the wave drains its stores: stored = d1, the output
    position of that match), then `run` literals and a match whose source ends at stored + delta."""
    fb.new(rb(rng, 40), 30, 10)
    d1 = fb.pos - 10
    d = fb.pos + run
    fb.new(rb(rng, run), d + ml - d1 - delta, ml)


def _fam_F():
    c = Cases()

    def frame_with(name, build, blocks=1):
        rng = R("F", name)
        fb = B.FrameB(rng.random())
        for _ in range(blocks):
            fb.new(rb(rng, 300), rng.randint(1, 300), 5)
            build(fb, rng)
            fb.tail(rb(rng, rng.randint(0, 9)))
            fb.end()
        c.ok(name, fb)
        return fb

    for ml in (3, 4, 5, 63, 64, 65, 256, 257):
        frame_with("off_eq_ml_%d" % ml, lambda fb, rng: fb.new(rb(rng, 2), ml, ml))
        frame_with("off_eq_ml_plus_1_%d" % ml, lambda fb, rng: fb.new(rb(rng, 2), ml + 1, ml))
        frame_with("off_far_%d" % ml, lambda fb, rng: fb.new(rb(rng, 800), 700 + ml, ml))
    for off in (1, 2, 3, 4, 5, 7, 63, 64, 65, 100, 255, 256, 257):
        for ml in sorted({max(off + 1, 3), 64, 65, 128, 300, 1000}):
            frame_with("overlap_off%d_ml%d" % (off, ml), lambda fb, rng: fb.new(rb(rng, rng.randint(0, 3)), off, ml))
    # the source is the literals of the match's own sequence
    for ll in (1, 5, 64, 300):
        for off in sorted({1, ll, max(1, ll - 1), ll + 1, ll + 7}):
            for ml in (3, 70):
                frame_with("own_literals_ll%d_off%d_ml%d" % (ll, off, ml),
                           lambda fb, rng: fb.new(rb(rng, ll), off, ml))
    # ll == 0 after ll == 0: all of the previous match's output, its last byte, one byte before it
    for m1 in (3, 9, 64, 200):
        for off2, ml2 in ((m1, m1), (m1, 3 * m1), (1, 40), (m1 + 1, m1 + 1), (m1 + 1, 300)):
            def build(fb, rng):
                fb.new(rb(rng, 6), 250, m1)
                fb.new(b"", off2, ml2)
                fb.new(b"", 3, 5)
            frame_with("chain_m%d_off%d_ml%d" % (m1, off2, ml2), build)
    # around the stored watermark
    for run in (0, 5, 300, 2000):
        for delta in (-20, -1, 0, 1):
            frame_with("stored_run%d_delta%+d" % (run, delta), lambda fb, rng: _watermark(fb, rng, run, delta))
            frame_with("stored_block2_run%d_delta%+d" % (run, delta),
                       lambda fb, rng: _watermark(fb, rng, run, delta), blocks=2)
    for delta in (-1, 0, 1):  # the same in a second frame: stored counts from the page's first byte
        rng = R("F", "frame2", delta)
        f1 = B.FrameB(1)
        f1.new(rb(rng, 500), 100, 30)
        f1.end()
        f2 = B.FrameB(2)
        _watermark(f2, rng, 7, delta)
        f2.end()
        c.ok("stored_frame2_delta%+d" % delta, f1, f2)
    rng = R("F", "far")
    fb = B.FrameB(1)
    fb.raw(rb(rng, BMAX))
    fb.new(rb(rng, 900), 70000, 140000 - BMAX - 900 - 28)
    fb.tail(rb(rng, 28))
    fb.end()
    assert fb.pos == 140000
    c.ok("far_70000", fb)
    return c


# ---- G: frames and windows around compressed blocks
def _fill_block(fb, rng, size):
    """A compressed block that regenerates exactly size bytes."""
    left = size - rand_seqs(fb, rng, 60, size - 1)
    fb.tail(rb(rng, left))
    fb.end()


def _bit_heavy(fb, rng, nseq):
    """A block of nseq 3-byte matches whose sequences cost 26 bits each: its compressed size passes what
    it regenerates.  All three tables at their largest logs, every used symbol with a -1 probability."""
    fb.new(rb(rng, 2), 1, 3)
    for _ in range(nseq - 1):
        fb.new(b"", 1, 3)
    opts = {"ll": {"log": 9, "less1": {0, 2}, "extra": {1}}, "of": {"log": 8, "less1": {2}, "extra": {1}},
            "ml": {"log": 9, "less1": {0}, "extra": {1}}}
    return fb.end(ll="fse", of="fse", ml="fse", opts=opts)


def _fam_G():
    c = Cases()
    for wd, bmax in ((0x00, KB), (0x18, 8 * KB), (0x50, BMAX)):
        rng = R("G", wd)
        fb = B.FrameB(wd)
        # a block of exactly the block maximum of the 1 KiB and 8 KiB windows; 8 KiB at 0x50 too (blocks of
        # exactly 128 KiB are B's ml_131069 and D's literals_131072: raw literals would not fit such a block)
        _fill_block(fb, rng, min(bmax, 8 * KB))
        _fill_block(fb, rng, 100)
        c.ok("window_%02x" % wd, fb, window=wd, fcs_bytes=0)
        c.ok("window_%02x_checksum" % wd, fb, window=wd, fcs_bytes=4, checksum=True)
    for fcs, size in ((1, 200), (2, 256), (2, 3000), (4, 700), (8, 700)):
        fb = B.FrameB(fcs)
        _fill_block(fb, R("G", fcs, size), size)  # single segment: the window is the content size
        c.ok("single_fcs%d_%d" % (fcs, size), fb, single=True, fcs_bytes=fcs)
    fb = B.FrameB(9)
    _fill_block(fb, R("G", "ck"), 5000)
    fb.raw(rb(R("G", "ck2"), 33))
    c.ok("checksum_matches", fb, checksum=True, fcs_bytes=2)
    # ---- invalid, at a 1 KiB window and at 128 KiB
    for wd, bmax in ((0x00, KB), (0x50, BMAX)):
        rng = R("G", "bad", wd)
        fb = B.FrameB(1)
        payload = _bit_heavy(fb, rng, bmax // 3 - 10)
        assert fb.pos <= bmax < len(payload), (fb.pos, len(payload))
        c.bad("compressed_size_above_max_%02x" % wd, fb, window=wd)
        fb = B.FrameB(2)
        fb.tail(b"\x33" * (bmax + 1))
        fb.end(lit="rle", sf=3)
        c.bad("literal_size_above_max_%02x" % wd, fb, window=wd)
    return c


# ---- H: seeded fuzz
def _fuzz_frame(k):
    rng = R("H", k)
    fb = B.FrameB(rng.random())
    alpha = bytes(rng.sample(range(129), rng.randint(2, 20)))
    for _ in range(rng.randint(1, 3)):
        kind = rng.random()
        if kind < 0.1:
            fb.raw(rb(rng, rng.randint(0, 300)))
            continue
        if kind < 0.2:
            fb.rle(rng.randint(0, 255), rng.randint(1, 300))
            continue
        lit = rng.choice(("raw", "rle", "huf", "huf", "treeless", "treeless"))
        la = alpha[:1] if lit == "rle" else alpha
        if rng.random() < 0.3:  # one code per table, so that RLE mode is open
            n = rng.randint(0, 40)
            ll, off, ml = rng.randint(0, 3), rng.randint(1, 4), rng.randint(3, 6)
            for i in range(n):
                fb.new(rb(rng, ll if fb.pos or ll else 1, la), min(off, fb.pos + ll) if fb.pos + ll else 1, ml)
        else:
            rand_seqs(fb, rng, rng.randint(0, 200), 6000, max_ll=rng.choice((3, 30)), alpha=la)
        fb.tail(rb(rng, rng.randint(0, 40) if rng.random() < 0.8 else rng.randint(200, 2000), la))
        data = bytes(fb.lits)
        kw = {}
        if lit == "treeless" and not (fb.huf and data and all(b in fb.huf.code for b in data)):
            lit = "huf"
        if lit == "rle" and not data:
            lit = "raw"
        if lit == "huf" and len(set(data)) < 2:
            lit = "raw"
        if lit in ("huf", "treeless"):
            kw["four"] = len(data) >= 6 and (rng.random() < 0.5 or len(data) > 1023)
        if lit == "huf":
            kw["desc"] = rng.choice(("direct", "fse"))
            kw["wlog"] = rng.choice((5, 6))
        else:
            kw["sf"] = None
        modes = {}
        cs = {"ll": {B.ll_code(s[0])[0] for s in fb.seqs}, "of": {B.of_code(s[1])[0] for s in fb.seqs},
              "ml": {B.ml_code(s[2])[0] for s in fb.seqs}}
        for w in WHICH:
            can = ["predef", "fse"]
            if len(cs[w]) == 1:
                can += ["rle", "rle"]
            if fb.tab[w] is not None and all(x in fb.tab[w].by_sym for x in cs[w]):
                can += ["repeat", "repeat"]
            modes[w] = rng.choice(can)
        opts = {w: {"log": rng.randint(6, B.MAX_LOG[w])} for w in WHICH if modes[w] == "fse" and rng.random() < 0.5}
        fb.end(lit=lit, opts=opts, **modes, **kw)
    return fb


def _fam_H():
    c = Cases()
    for k in range(300):
        fb = _fuzz_frame(k)
        kw = dict(fcs_bytes=(0, 4, 8)[k % 3], window=(0x50, 0x38, 0x51)[k % 3])
        if k % 4 == 3 and all(len(b[1]) <= fb.pos for b in fb.blocks):  # single segment: the content size is the window
            kw = dict(single=True, fcs_bytes=1 if fb.pos < 256 else 2 if k % 8 == 3 else 4)
        c.ok("fuzz_%d" % k, fb, checksum=k % 5 == 0, **kw)
    return c


FAMILIES = "ABCDEFGH"
# the model's counters every family must reach (tools/zstd_model.cpp): a family that silently stops
# reaching its cell fails
COVER = {
    "A": ["ll_predef", "ll_rle", "ll_fse", "ll_repeat", "of_predef", "of_rle", "of_fse", "of_repeat",
          "ml_predef", "ml_rle", "ml_fse", "ml_repeat", "seq_none", "frame_multi_block"],
    "B": ["seq_none", "seq_short", "seq_mid", "seq_long", "match_overlap"],
    "C": ["rep_offset", "frame_multi_block"],
    "D": ["lit_huf1", "lit_huf4", "lit_treeless1", "lit_treeless4", "huf_direct", "huf_fse", "lit_raw", "lit_rle"],
    "E": ["lit_raw", "lit_rle", "lit_huf1", "lit_huf4", "seq_none", "huf_direct", "huf_fse"],
    "F": ["match_overlap", "frame_multi_block", "blk_raw"],
    "G": ["frame_single", "frame_window", "fcs1", "fcs2", "fcs4", "fcs8", "frame_checksum"],
    "H": [k for k in Z.CELLS if k != "seq_long"] + ["rep_offset", "match_overlap", "frame_checksum"],
}


@functools.lru_cache(maxsize=None)
def family(f):
    c = globals()["_fam_" + f]()
    names = [v[0] for v in c.valid] + [v[0] for v in c.invalid]
    assert len(names) == len(set(names))
    return c.valid, c.invalid


def _first_diff(valid, got):
    at = 0
    for name, _, exp in valid:
        if got[at:at + len(exp)] != exp:
            return name
        at += len(exp)
    return None


def _libzstd_rejects(z, n):
    """libzstd itself raises on z, with room for the n bytes it would decode to and with room to spare: a
    decode to some other length is no rejection."""
    for cap in (n, n + 4096):
        try:
            pa.Codec("zstd").decompress(z, decompressed_size=cap, asbytes=True)
            return False
        except Exception:
            pass
    return True


@pytest.mark.parametrize("f", FAMILIES)
def test_family_cpu(f):
    """expand == libzstd == the model on every valid stream; both reject every invalid one; the family
    reaches its cells."""
    valid, invalid = family(f)
    for name, z, exp in valid:
        assert Z.libzstd(z, len(exp)) == exp, name
    res, _ = Z.model_corpus([(len(exp), z) for _, z, exp in valid])
    for (name, _, exp), (rc, ln, _) in zip(valid, res):
        assert (rc, ln) == (0, len(exp)), (name, rc, ln, len(exp))
    # the bytes: all the family's frames as one stream (tables of one frame are not the next one's)
    want = b"".join(exp for _, _, exp in valid)
    r = Z.model(b"".join(z for _, z, _ in valid), cap=len(want))
    assert r["status"] == 0 and r["len"] == len(want)
    assert r["bytes"] == want, _first_diff(valid, r["bytes"])
    missing = [k for k in COVER[f] if not r[k]]
    assert not missing, missing
    res, _ = Z.model_corpus([(n, z) for _, z, n in invalid])
    for (name, z, n), (rc, _, _) in zip(invalid, res):
        assert _libzstd_rejects(z, n), name
        assert rc == ZSTD, (name, rc)


# valid and invalid streams per family: what the GPU tests' parts are cut from
COUNTS = {"A": (97, 22), "B": (29, 4), "C": (23, 3), "D": (1089, 9), "E": (900, 0), "F": (192, 0), "G": (12, 4),
          "H": (300, 0)}
# the streams that decode to more than 64 KiB + 600 (a code of 16 extra bits starts at 64 KiB): each is
# about a size
BIG = {"A": ["predef_every_symbol"],
       "B": ["ll_131069", "ml_131069", "nseq_32511_form1", "nseq_32512_form2", "of_codes_16_17"],
       "D": ["literals_131072"], "F": ["far_70000"]}


def test_family_sizes():
    """The families hold the streams the GPU parts are cut from; streams stay at or below 64 KiB decoded,
    but for the named ones that are about a size."""
    for f in FAMILIES:
        valid, invalid = family(f)
        assert (len(valid), len(invalid)) == COUNTS[f], f
        over = [name for name, _, exp in valid if len(exp) > 64 * KB + 600]
        assert over == BIG.get(f, []), (f, over)


def test_sanitizer_clean():
    """The model built with -fsanitize=address,undefined (a stand-alone program) over every stream of every
    family, the invalid ones with room for what they would decode to and with no room at all."""
    cases = []
    for f in FAMILIES:
        valid, invalid = family(f)
        cases += [(len(exp), z) for _, z, exp in valid] + [(n, z) for _, z, n in invalid]
        cases += [(0, z) for _, z, _ in invalid] + [(max(len(exp) - 1, 0), z) for _, z, exp in valid[::7]]
    res, err = Z.model_corpus(cases, sanitize=True)
    assert len(res) == len(cases)
    assert "Sanitizer" not in err and "runtime error" not in err, err[-3000:]


# ---- the oversized block
def _oversized(wd, bmax, total):
    rng = R("over", wd, total)
    fb = B.FrameB(1)
    fb.new(b"\x41" * (bmax - 24), 9, 6)
    left = total - fb.pos
    while left:
        k = min(left, 60000)
        if 0 < left - k < 3:  # no match is shorter than 3
            k = left - 3
        fb.new(b"", rng.randint(1, 50), k)
        left -= k
    fb.end(lit="rle")
    assert fb.pos == total and len(fb.lits) == 0
    exp = B.expand([fb.desc])
    return fb.frame(window=wd, fcs_bytes=0), exp


OVERSIZED = [(wd, bmax, total) for wd, bmax in ((0x00, KB), (0x18, 8 * KB), (0x50, BMAX))
             for total in (bmax + 1, 2 * bmax)]


@pytest.mark.parametrize("wd,bmax,total", OVERSIZED)
def test_oversized_block(wd, bmax, total):
    """A compressed block whose sequences regenerate more than the block maximum min(window, 128 KiB).
    No writer emits one.  The model decodes it at any size, to the plain model's bytes: every write is
    bounded by cap, and neither limit below can be mirrored exactly.  The RFC forbids it.  libzstd accepts
    it up to the block maximum + 67 bytes, an accident of where it keeps the block's literals, and rejects
    it when sequence execution passes that point: the first rejected totals measured (libzstd 1.5.x through
    pyarrow) are 1 092 / 8 260 / 131 140 for windows of 1 KiB / 8 KiB / 2 MiB; trailing literals may
    pass it by any amount.  Its verdict is asserted only at the block maximum + 1, where it accepts."""
    z, exp = _oversized(wd, bmax, total)
    assert len(exp) == total
    r = Z.model(z, cap=total)
    assert r["status"] == 0 and r["bytes"] == exp
    if total == bmax + 1:
        assert Z.libzstd(z, total) == exp
    # with no cap given the model decodes into zstd::decoded_bound bytes, as pqg_block_decompress does: the
    # block maximum of 128 KiB per compressed block, whatever the window.  Past that the verdict is ZSTD.
    assert Z.model(z, want_bytes=False)["status"] == (0 if total <= BMAX else ZSTD)


# ---- the GPU
@pytest.fixture(scope="module")
def dec():
    import pqgpu
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


def _parts(f, size=200):
    return [(f, i) for i in range(0, COUNTS[f][0], size)]


BLOCK_PARTS = [p for f in FAMILIES for p in _parts(f)]


@pytest.mark.gpu
@pytest.mark.parametrize("f,start", BLOCK_PARTS, ids=["%s%d" % p for p in BLOCK_PARTS])
def test_gpu_family_blocks(dec, f, start):
    """Each valid stream through pqg_block_decompress: the bytes, and nothing written past them."""
    from test_zstd import _gpu_block
    bad = []
    for name, z, exp in family(f)[0][start:start + 200]:
        rc, n, dst = _gpu_block(dec, z, len(exp) + 100)
        if rc != 0 or n != len(exp) or dst[:n].tobytes() != exp or dst[n:].any():
            got = dst[:len(exp)].tobytes()
            first = next((i for i in range(min(n, len(exp))) if got[i] != exp[i]), -1)
            bad.append((name, abi.status_name(rc), n, len(exp), first, bool(dst[max(n, 0):].any())))
    assert not bad, (len(bad), bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("f", [f for f in FAMILIES if COUNTS[f][1]])
def test_gpu_family_invalid_blocks(dec, f):
    from test_zstd import _gpu_block
    bad = []
    for name, z, n in family(f)[1]:
        rc, _, _ = _gpu_block(dec, z, n + 100)
        if rc != ZSTD:
            bad.append((name, abi.status_name(rc)))
    assert not bad, bad


def _as_page(z, exp):
    """A PLAIN INT64 V1 page of the stream, its content padded to whole values by a frame of one raw block."""
    from test_zstd import _zpage
    pad = -len(exp) % 8
    if pad:
        z, exp = z + Z.frame([(0, bytes(pad), None)], bytes(pad)), exp + bytes(pad)
    return _zpage(exp, z, len(exp) // 8), exp


def _pages_gpu(dec, cases):
    """The cases as the pages of one chunk in one decode call, against the oracle's decode of the twin
    chunk of uncompressed pages."""
    import parity as P
    import pqtest_util as U
    from oracle import pyoracle as O
    from test_zstd import _chunk_gpu, _plain_page
    cases = [c for c in cases if len(c[2])]
    pages = [_as_page(z, exp) for _, z, exp in cases]
    got = _chunk_gpu(dec, b"".join(p for p, _ in pages), ptype=abi.INT64, codec=abi.CODEC_ZSTD)
    keep = []
    job, _ = U.chunk_job(b"".join(_plain_page(raw, len(raw) // 8) for _, raw in pages), ptype=abi.INT64, codec=0,
                         keep=keep)
    exp = O.decode_chunk(job)
    assert exp.status == 0 and len(exp.pages) == len(pages)
    assert got.status == 0, (abi.status_name(got.status), got.error_page, cases[got.error_page][0])
    P.compare_chunk(exp, got, "pages")
    assert np.asarray(got.values).tobytes() == b"".join(raw for _, raw in pages)


PAGE_PARTS = [p for f in "ABCDEFG" for p in _parts(f, 400)] + [("H", i) for i in range(0, 300, 50)]


@pytest.mark.gpu
@pytest.mark.parametrize("f,start", PAGE_PARTS, ids=["%s%d" % p for p in PAGE_PARTS])
def test_gpu_family_pages(dec, f, start):
    _pages_gpu(dec, family(f)[0][start:start + (50 if f == "H" else 400)])


@pytest.mark.gpu
@pytest.mark.parametrize("f", [f for f in FAMILIES if COUNTS[f][1]])
def test_gpu_family_invalid_pages(dec, f):
    """good + bad + good: ZSTD on page 1."""
    from test_zstd import _chunk_gpu, _zpage
    good, _ = _as_page(*family("C")[0][0][1:])
    bad = []
    for name, z, n in family(f)[1]:
        page = _zpage(bytes(n + (-n % 8)), z, (n + 7) // 8)
        got = _chunk_gpu(dec, good + page + good, ptype=abi.INT64, codec=abi.CODEC_ZSTD)
        if got.status != ZSTD or got.error_page != 1:
            bad.append((name, abi.status_name(got.status), got.error_page))
    assert not bad, bad


@pytest.mark.gpu
def test_gpu_oversized_block(dec):
    """What the model says (see test_oversized_block): decoded as a page, whose buffer is the page's
    uncompressed size; as a bare block decoded into zstd::decoded_bound bytes, ZSTD past them."""
    from test_zstd import _gpu_block
    for wd, bmax, total in OVERSIZED:
        z, exp = _oversized(wd, bmax, total)
        want = Z.model(z, want_bytes=False)["status"]
        assert want == (0 if total <= BMAX else ZSTD)
        rc, n, dst = _gpu_block(dec, z, total + 100)
        assert rc == want, (wd, total, abi.status_name(rc))
        if rc == 0:
            assert n == total and dst[:n].tobytes() == exp and not dst[n:].any(), (wd, total)
    _pages_gpu(dec, [("oversized", *_oversized(*o)) for o in OVERSIZED])
