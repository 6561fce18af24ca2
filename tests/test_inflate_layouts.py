"""GZIP inflate on DEFLATE streams that zlib's encoder never emits.

Every stream tests/test_gzip.py feeds pqg_inflate.hip was written by zlib, so
the kernels only ever saw what one encoder chooses: code lengths of 11-12 bits
at most, HLIT / HDIST below their maxima, no empty stored block, distances
wherever the data put them.  Here the streams are built by hand
(tests/deflate_build.py: a bit writer, explicit code lengths and headers)
together with a plain model of the format:

    literal: out.append(b)      match (length, distance): out.append(out[-distance]), length times

For every valid stream four things agree byte for byte: the model, Python's
zlib, the oracle (gzip_decode and the chunk decode) and the GPU, the last both
through pqg_block_decompress (k_inflate: the 32 KiB ring, 64-bit indices) and
as a PLAIN INT64 v1 page (k_inflate_s: the 8 KiB ring, 32-bit indices; no page
may need the second pass, PQG_PAGE_FLAG_INFLATE_REDO).  The model is there so
that a misreading shared by zlib and a kernel cannot hide.  For every invalid
stream Python's zlib raises (with the message the case is named for), the
oracle says GZIP, and the GPU says what the oracle says.

The reference inflates with Go's compress/flate (stdlib, not in the tree); the
oracle's stated rule is zlib's classification of malformed streams
(oracle/pq_oracle.cpp gzip_decode), and the oracle is the expectation here.

The CPU tests check every stream of every family, the whole fuzz and mutation
sets included, against the model, zlib and the oracle: they prove that the
inputs are what they claim to be.  The GPU tests run a family's cases as the
pages of one chunk (valid ones) and as the jobs of one decode call (invalid
ones: a failing page fails its chunk), so unlike pages sit side by side in
the inflate queue.

Constants of pqg_inflate.hip the cases are sized by:
  kFastBits = 9        codes of 10-15 bits take decode()'s bit-by-bit walk; lit_run leaves at any code that is
                       not a literal of the fast table (families A, C)
  PQG_INFLATE_RING = 8192 (kRingSmall)
                       copy() reads distances above kRingT - 64 = 8128 back from the stored output and copies
                       smaller ones inside the ring: 8127 / 8128 / 8129, 8191 / 8192 / 8193 (family B).  A round
                       of the ring copy reads its 64 bytes before it writes any, so it is exact up to a distance
                       of kRingT itself: a threshold anywhere in 8128..8192 decodes the same bytes, and 8193 is
                       the first distance a larger one gets wrong
  kFlushT = kRingT / 2 = 4096 (16384 for the 32 KiB ring)
                       literal runs of 4095 / 4096 / 4097 / 4160 = kFlushT + 64 (family C), the 300 KiB page:
                       several wraps of both rings
  copy rounds of min(dist, 64) bytes
                       distances 63 / 64 / 65, lengths 64 / 65 (family B)
  lit_run batches of 64 literals, two per step
                       runs of 63 / 64 / 65 / 127 / 128 / 129, literal prefixes 0..63 (families B, C)
  kInStage = 1024      compressed bytes per refill, staged from the 16-byte aligned address below: FEXTRA
                       lengths 0..15 move a header, a code with its extra bits, LEN / NLEN and the trailer
                       across byte 1024 k (family E)
  lens[32..348)        nlen = 286 and ndist = 30 at most, runs across the nlen boundary (family A)
  stored(): a flush check every 256 bytes
                       LEN 255 / 256 / 257 / 65535 (family D)

HCLEN = 4 leaves only the symbols 16, 17, 18 and 0 with a code, so every length
is 0 and the end-of-block code is missing: that header is an error case; the
smallest valid one is HCLEN = 5 (16, 17, 18, 0, 8)."""
import collections
import functools
import zlib

import numpy as np
import pytest

import deflate_build as B
import parity as P
import pqtest_util as U
from gen import pqwrite as W
from oracle import pyoracle as O
from pqgpu import abi
from test_gzip import REDO, _gpu_block, _gz_page

GZIP = abi.STATUS_CODES["GZIP"]
RING, FAR, FLUSH, STAGE, FAST = 8192, 8192 - 64, 4096, 1024, 9
EDGE_DIST = [1, 2, 3, 63, 64, 65, 4095, 4096, 4097, FAR - 1, FAR, FAR + 1, RING - 1, RING, RING + 1, 16384, 32767,
             32768]
EDGE_LEN = [3, 4, 64, 65, 257, 258]
LIT_RUNS = [0, 1, 2, 63, 64, 65, 127, 128, 129, FLUSH - 1, FLUSH, FLUSH + 1, FLUSH + 64]

# ok: True (valid: raw is the model's bytes), False (invalid: zlib raises with
# `why` in its message and the oracle says GZIP; raw is None)
Case = collections.namedtuple("Case", "name gz raw ok why")


def _ok(name, deflate, raw, **kw):
    assert len(raw) <= 1 << 16 or name.startswith(("G/big", "H/")), name
    return Case(name, B.member(deflate, raw, **kw), raw, True, None)


def _bad(name, deflate, why, raw=b"12345678"):
    return Case(name, B.member(deflate, raw), None, False, why)


def _rbytes(rng, n, alphabet=None):
    if alphabet is None:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return bytes(np.asarray(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)])


def _size(t):
    return 1 if isinstance(t, int) else len(t) if isinstance(t, (bytes, bytearray)) else t[0]


def _codes_for(rng, tokens, maxlen):
    """Random complete codes over exactly the symbols `tokens` use; a single
    distance symbol gets the one-bit code, none the empty code."""
    lit, dist = B.used_symbols(tokens)
    need = lambda n: max(maxlen, (n - 1).bit_length())  # noqa: E731
    if len(lit) == 1:
        ll = [0] * 256 + [1]
    else:
        ll = B.random_lens(rng, sorted(lit), need(len(lit)), 286)
    if len(dist) < 2:
        dl = [0] * 30
        for ds in dist:
            dl[ds] = 1
    else:
        dl = B.random_lens(rng, sorted(dist), need(len(dist)), 30)
    return ll, dl


def _dyn(w, rng, tokens, maxlen, last, **kw):
    ll, dl = _codes_for(rng, tokens, maxlen)
    return w.dynamic(tokens, ll, dl, last, **kw)


def _stream(rng, blocks):
    """blocks: (kind, tokens, maxlen) -> (deflate bytes, model bytes); a
    stored block holds the model's bytes of its tokens."""
    raw = B.model([t for _, toks, _ in blocks for t in toks])
    w, at = B.Deflate(), 0
    for i, (kind, toks, maxlen) in enumerate(blocks):
        last = i + 1 == len(blocks)
        size = sum(_size(t) for t in toks)
        if kind == "stored":
            w.stored(raw[at:at + size], last)
        elif kind == "fixed":
            w.fixed(toks, last)
        else:
            _dyn(w, rng, toks, maxlen, last)
        at += size
    return w.getvalue(), raw


def _one(rng, kind, tokens, maxlen=12):
    return _stream(rng, [(kind, tokens, maxlen)])


# ---------------------------------------------------------------- A: Huffman tables
def _matches(rng, lengths, dists, n, lits):
    toks = []
    for _ in range(n):
        toks.append((int(rng.choice(lengths)), int(rng.choice(dists))))
        toks.append(_rbytes(rng, int(rng.integers(0, 6)), lits))
    return toks


@functools.lru_cache(None)
def family_a():
    rng = np.random.default_rng(0xA)
    out = []

    def dyn(name, tokens, ll, dl, check=None, **kw):
        w = B.Deflate()
        syms = w.dynamic(tokens, ll, dl, True, **kw)
        if check:
            check(syms)
        out.append(_ok("A/" + name, w.getvalue(), B.model(tokens)))

    # lengths 1..15, the match symbols and the end code deepest: 12 literals
    # take 1..12 bits, 257 (length 3) 13, 270 (23..26) 14, 285 (258) and 256 15
    lits = list(range(65, 77))
    ll = B.skewed_lens(lits + [257, 270, 285, 256], 15, 286)
    assert sorted(x for x in ll if x) == list(range(1, 16)) + [15] and ll[256] == 15 and ll[270] == 14
    toks = [_rbytes(rng, 40, lits)] + _matches(rng, [3, 23, 24, 25, 26, 258], [1, 5, 20], 60, lits)
    dl = _codes_for(rng, toks, 3)[1]
    dyn("depth_match_symbols", toks, ll, dl)
    # the same block with a code-length code of 7-bit lengths
    dyn("cl_7bit", toks, ll, dl, cl_lens=lambda syms: B.skewed_lens(sorted({s for s, _ in syms}), 7, 19))

    # a third of the literals in use above the fast table: 16 literals, the
    # end code and two length symbols at 2..9 bits, 8 literals at 11..15
    short, long_ = list(range(97, 113)), list(range(113, 121))
    ll = [0] * 286
    for s, x in zip(short + [256, 257, 260], B.balanced(11, 1) + list(range(2, 10))):
        ll[s] = x
    for s, x in zip(long_, [11, 11, 11, 12, 13, 14, 15, 15]):
        ll[s] = x
    assert B.kraft(ll) == 1 << 15 and all(ll[s] <= FAST for s in short) and all(ll[s] > FAST for s in long_)
    toks = []
    for _ in range(300):
        toks.append(bytes(int(rng.choice(long_ if rng.random() < 1 / 3 else short)) for _ in range(10)))
        toks.append((int(rng.choice([3, 6])), int(rng.choice([1, 2, 9, 10]))))
    dyn("depth_literals", toks, ll, _codes_for(rng, toks, 4)[1])

    # a distance code over 20 symbols, the deepest 15 bits: both ends of every symbol's range
    dl = B.skewed_lens(list(range(20)), 15, 30)
    toks = [_rbytes(rng, 1100)]
    for k in range(3):
        for ds in range(20):
            for d in (B.DIST_BASE[ds], B.DIST_BASE[ds] + (1 << B.DIST_EXTRA[ds]) - 1):
                toks += [(int(rng.integers(3, 40)), d), int(rng.integers(0, 256))]
    dyn("depth_distances", toks, _codes_for(rng, toks, 9)[0], dl)

    # 9- and 10-bit codes side by side: literal 0 at 1 bit (256 / 512), 150
    # literals at 9 (150), 100 at 10 (50), 256 / 257 / 258 at 6 (24), 285 at 4 (32)
    ll = [0] * 286
    ll[0] = 1
    nine, ten = list(range(1, 151)), list(range(151, 251))
    for s in nine:
        ll[s] = FAST
    for s in ten:
        ll[s] = FAST + 1
    ll[256] = ll[257] = ll[258] = 6
    ll[285] = 4
    assert B.kraft(ll) == 1 << 15
    toks = [_rbytes(rng, 3000, nine + ten), (258, 100), (3, 1), (4, 2999), _rbytes(rng, 500, nine + ten + [0])]
    dyn("nine_and_ten_bits", toks, ll, _codes_for(rng, toks, 2)[1])

    # HLIT = 286 and HDIST = 30, every symbol used
    hist = _rbytes(rng, 33000)
    assert len(set(hist)) == 256
    toks = [hist]
    for i in range(60):
        s, ds = i % 29, i % 30
        toks.append((B.LEN_BASE[s] + min(i // 29, 1) * ((1 << B.LEN_EXTRA[s]) - 1),
                     B.DIST_BASE[ds] + (i // 30) * ((1 << B.DIST_EXTRA[ds]) - 1)))
    lit, dist = B.used_symbols(toks)
    assert len(lit) == 286 and len(dist) == 30
    ll, dl = _codes_for(rng, toks, 15)
    dyn("hlit_286_hdist_30", toks, ll, dl, runs=False)
    dyn("hlit_286_hdist_30_runs", toks, ll, dl)

    # length 258 written as symbol 284 with extra bits 31, next to symbol 285
    toks = [_rbytes(rng, 300), (258, 300, 284), (258, 1), (258, 258, 284), (257, 9)]
    ll, dl = _codes_for(rng, toks, 10)
    assert ll[284] and ll[285]
    dyn("length_258_as_284", toks, ll, dl)
    w = B.Deflate()
    w.fixed(toks, True)
    out.append(_ok("A/length_258_as_284_fixed", w.getvalue(), B.model(toks)))

    # HLIT = 257 and HDIST = 1; both larger than needed, trailing zero lengths
    toks = [_rbytes(rng, 200, [1, 2, 3, 200])]
    ll, _ = _codes_for(rng, toks, 3)
    dyn("hlit_257_hdist_1", toks, ll, [1], hlit=257, hdist=1)
    toks = [_rbytes(rng, 100, [1, 2, 3, 200]), (5, 3), (9, 17)]
    ll, dl = _codes_for(rng, toks, 3)
    dyn("hlit_hdist_larger", toks, ll, dl, hlit=270, hdist=12)
    dyn("hlit_hdist_largest", toks, ll, dl, hlit=286, hdist=30)

    # incomplete codes that are allowed: one distance code of one bit; no distance code at all
    for ds in (0, 5, 29):
        d0 = B.DIST_BASE[ds]
        d1 = d0 + (1 << B.DIST_EXTRA[ds]) - 1
        toks = [_rbytes(rng, d1 + 11), (7, d0), 4, (258, d1), (3, d0)]
        ll, dl = _codes_for(rng, toks, 9)
        assert B.kraft(dl) == 1 << 14
        dyn("distance_single_code_%d" % ds, toks, ll, dl)
    toks = [_rbytes(rng, 300, list(range(40)))]
    ll, _ = _codes_for(rng, toks, 7)
    dyn("distance_lengths_zero", toks, ll, [0])
    dyn("distance_lengths_zero_30", toks, ll, [0] * 30, hdist=30)

    # a literal code that is only the end code (one bit): an empty block between two real ones
    w = B.Deflate()
    t1 = [_rbytes(rng, 500, list(range(60)))]
    _dyn(w, rng, t1, 8, False)
    w.dynamic([], [0] * 256 + [1], [0], False)
    t3 = [(20, 500), 7, (100, 1), _rbytes(rng, 20)]
    w.fixed(t3, False)
    w.dynamic([], [0] * 256 + [1], [0], True)
    out.append(_ok("A/end_code_only_blocks", w.getvalue(), B.model(t1 + t3)))

    # HCLEN = 5: 16, 17, 18, 0 and 8 (see the module docstring for HCLEN = 4)
    cl = [0] * 19
    cl[16] = cl[17] = cl[18] = 2
    cl[0] = cl[8] = 3
    toks = [_rbytes(rng, 400, list(range(255)))]

    def has(sym, extra=None):
        return lambda syms: [x for x in syms if x[0] == sym and extra in (None, x[1])][0]

    dyn("hclen_5_repeat_16", toks, [8] * 255 + [0, 8], [0], cl_lens=cl, hclen=5, check=has(16, 3))
    # 18 with 138 repeats: lengths 50..187 are zero
    toks = [_rbytes(rng, 600, list(range(50)) + list(range(188, 256))), (10, 30)]
    ll, dl = _codes_for(rng, toks, 9)
    assert not any(ll[50:188]) and ll[49] and ll[188]
    dyn("run_18_138", toks, ll, dl, check=has(18, 127))

    # runs across the nlen boundary: the last 60 literal/length lengths and
    # the first two distance lengths are 9; then zeros on both sides of it
    def crosses(nlen):
        def check(syms):
            at, hit = 0, False
            for s, x in syms:
                n = 1 if s < 16 else x + (11 if s == 18 else 3)
                hit |= s >= 16 and at < nlen < at + n
                at += n
            assert hit
        return check

    ll = B.balanced(286)
    dl = [9, 9, 1, 2, 3, 4, 5, 6, 7, 8]
    assert B.kraft(ll) == B.kraft(dl) == 1 << 15 and ll[-60:] == [9] * 60
    toks = [_rbytes(rng, 2000)] + _matches(rng, [3, 30, 258], [1, 2, 3, 4, 5, 8, 12, 16, 24, 32], 50, None)
    dyn("run_16_across_nlen", toks, ll, dl, check=crosses(286))
    toks = [_rbytes(rng, 2000, list(range(100))), (4, 1025), (9, 2000)]
    ll, dl = _codes_for(rng, toks, 9)
    assert not any(dl[:20])
    dyn("run_18_across_nlen", toks, ll, dl, hlit=286, check=crosses(286))
    return out


@functools.lru_cache(None)
def family_a_bad():
    rng = np.random.default_rng(0xAB)
    out = []
    toks = [_rbytes(rng, 100, list(range(100))), (3, 2), 7]

    def dyn(name, why, tokens, ll, dl, **kw):
        w = B.Deflate()
        w.dynamic(tokens, ll, dl, True, **kw)
        out.append(_bad("A/" + name, w.getvalue() + bytes(8), why))

    eight = [8] * 100 + [0] * 156 + [8, 8]  # 102 codes of 8 bits: incomplete
    dyn("lit_oversubscribed", "invalid literal/lengths set", toks, [8] * 258, [1, 1])
    dyn("lit_incomplete", "invalid literal/lengths set", toks, eight, [1, 1])
    full = [8] * 100 + [0] * 2 + [8] * 156  # 256 codes of 8 bits
    assert B.kraft(full) == 1 << 15 and len(full) == 258
    dyn("dist_incomplete_two", "invalid distances set", toks, full[:258], [2, 2])
    dyn("dist_single_two_bits", "invalid distances set", toks, full[:258], [0, 2])
    dyn("dist_oversubscribed", "invalid distances set", toks, full[:258], [1, 1, 1])
    cl = [0] * 19
    cl[0], cl[8], cl[16], cl[17], cl[18] = 2, 2, 3, 3, 4
    dyn("cl_incomplete", "invalid code lengths set", toks[:1], full[:258], [0], cl_lens=cl)
    cl[17] = cl[18] = 2
    dyn("cl_oversubscribed", "invalid code lengths set", toks[:1], full[:258], [0], cl_lens=cl)
    no_eob = [8] * 256 + [0]
    dyn("missing_end_code", "missing end-of-block", [toks[0]], no_eob, [0], eob=False)
    cl = [0] * 19
    cl[16] = cl[17] = cl[18] = cl[0] = 2
    dyn("hclen_4", "missing end-of-block", [], [0] * 257, [0], cl_lens=cl, hclen=4, eob=False,
        cl_syms=[(18, 127), (18, 109)])
    good = B.cl_symbols(full[:258] + [1, 1])
    dyn("repeat_16_first", "invalid bit length repeat", toks, full[:258], [1, 1], cl_syms=[(16, 0)] + good)
    dyn("run_overshoots", "invalid bit length repeat", toks, full[:258], [1, 1], cl_syms=good[:-2] + [(17, 0)])
    dyn("run_overshoots_18", "invalid bit length repeat", toks, full[:258], [1, 1], cl_syms=good[:-2] + [(18, 127)])
    for hlit in (287, 288):
        dyn("hlit_%d" % hlit, "too many length or distance symbols", toks, full[:258], [1, 1], hlit=hlit)
    for hdist in (31, 32):
        dyn("hdist_%d" % hdist, "too many length or distance symbols", toks, full[:258], [1, 1], hdist=hdist)
    for s in (286, 287):
        w = B.Deflate()
        w.fixed([toks[0], ("lsym", s), 5], True)
        out.append(_bad("A/fixed_symbol_%d" % s, w.getvalue() + bytes(8), "invalid literal/length code"))
    for ds in (30, 31):
        w = B.Deflate()
        w.fixed([toks[0], ("dsym", 4, ds), 5, 6, 7, 8, 9], True)
        out.append(_bad("A/fixed_distance_%d" % ds, w.getvalue() + bytes(8), "invalid distance code"))
    dyn("match_without_distance_code", "invalid distance code", [toks[0], ("draw", 3, 0, 1), 5, 6, 7], full[:258],
        [0])
    dyn("distance_single_code_unused", "invalid distance code", [toks[0], (3, 1), ("draw", 3, 1, 1), 5, 6, 7],
        full[:258], [1])
    # the input ends inside a dynamic header (no trailer: the page ends there)
    w = B.Deflate()
    ll, dl = _codes_for(rng, toks, 12)
    w.dynamic(toks, ll, dl, True, runs=False)
    hdr = B.member(b"", b"")[:10]
    assert w.header_end // 8 > 60
    for cut in (0, 1, 2, 3, 9, 30, w.header_end // 8 - 1, w.header_end // 8):
        out.append(Case("A/header_cut_%d" % cut, hdr + w.getvalue()[:cut], None, False, "truncated"))
    return out


# ---------------------------------------------------------------- B: match edges
def _edge_tokens(hist, dist):
    toks = [hist]
    for n in EDGE_LEN:
        toks += [(n, dist), (n * 7 + dist) & 255]  # a literal between matches
    toks += [(n, dist) for n in EDGE_LEN]           # back to back
    return toks


@functools.lru_cache(None)
def family_b_pairs():
    out = []
    for kind in ("fixed", "dynamic"):
        for dist in EDGE_DIST:
            rng = np.random.default_rng(dist * 2 + (kind == "fixed"))
            # more than the window of history; the last bytes differ from
            # their neighbours 64 and 8192 back, so a wrong source shows
            d, raw = _one(rng, kind, _edge_tokens(_rbytes(rng, 33000), dist))
            out.append(_ok("B/%s/dist_%d" % (kind, dist), d, raw))
    return out


@functools.lru_cache(None)
def family_b_prefix():
    out = []
    for kind in ("fixed", "dynamic"):
        for dist in (FAR, FAR + 1, RING):
            for pre in range(64):
                rng = np.random.default_rng(dist * 128 + pre * 2 + (kind == "fixed"))
                d, raw = _one(rng, kind, _edge_tokens(_rbytes(rng, RING + 64 + pre), dist), 10)
                out.append(_ok("B/%s/dist_%d_prefix_%d" % (kind, dist, pre), d, raw))
    return out


@functools.lru_cache(None)
def family_b_members():
    """A distance of exactly the member's bytes so far, and one more."""
    out, bad = [], []
    rng = np.random.default_rng(0xB)
    first_raw = _rbytes(rng, 9000)
    first = B.member(_one(rng, "fixed", [first_raw])[0], first_raw)
    for kind in ("fixed", "dynamic"):
        for n in (1, 2, 64, 100, FAR, FAR + 1, 9000, 32768):
            hist = _rbytes(rng, n)
            toks = [hist, (258, n), 3, (3, n), (65, n)]
            if n + 327 <= 32768:
                toks.append((4, n + 327))  # again everything so far
            d, raw = _one(rng, kind, toks)
            name = "B/%s/whole_member_%d" % (kind, n)
            out.append(_ok(name + "_first", d, raw))
            out.append(Case(name + "_second", first + B.member(d, raw), first_raw + raw, True, None))
            for over, tag in ((1, "one_past"), (100, "into_first")):
                if n + 258 + over > 32768:
                    continue
                w = B.Deflate()
                far = [hist, (258, n), (5, n + 258 + over), 9]
                if kind == "fixed":
                    w.fixed(far, True)
                else:
                    _dyn(w, rng, far, 12, True)
                c = _bad("%s_%s" % (name, tag), w.getvalue(), "invalid distance too far back")
                if tag == "one_past":
                    bad.append(c)
                bad.append(Case(c.name + "_second", first + c.gz, None, False, c.why))
    return out, bad


# ---------------------------------------------------------------- C: literal runs
@functools.lru_cache(None)
def family_c():
    out = []
    rng = np.random.default_rng(0xC)
    # runs between matches; the dynamic code keeps every literal in the fast table
    toks = [_rbytes(rng, 100)]
    for n in LIT_RUNS:
        toks += [(10, 50), _rbytes(rng, n)]
    toks.append((10, 50))
    for kind, maxlen in (("fixed", 0), ("dynamic", FAST), ("dynamic", 15)):
        d, raw = _one(rng, kind, toks, maxlen)
        out.append(_ok("C/runs_%s_%d" % (kind, maxlen), d, raw))
        # ... and as the last block of the first of two members
        d2, raw2 = _one(rng, "fixed", [b"second member", (5, 6)])
        out.append(Case("C/runs_%s_%d_two_members" % (kind, maxlen), B.member(d, raw) + B.member(d2, raw2),
                        raw + raw2, True, None))

    # every pattern of up to four literals inside (F) and outside (S) the fast
    # table after a match: lit_run's first and second literal of a step
    fast, slow = list(range(97, 113)), list(range(113, 121))
    ll = [0] * 286
    for s, x in zip(fast + [256, 257, 260], B.balanced(11, 1) + list(range(2, 10))):
        ll[s] = x
    for s, x in zip(slow, [11, 11, 11, 12, 13, 14, 15, 15]):
        ll[s] = x
    toks = [_rbytes(rng, 20, fast)]
    for n in range(1, 5):
        for pat in range(1 << n):
            toks.append((3, 4))
            toks += [int(rng.choice(slow if pat >> k & 1 else fast)) for k in range(n)]
    toks.append((6, 3))
    w = B.Deflate()
    w.dynamic(toks, ll, [1, 2, 3, 3], True)
    out.append(_ok("C/fast_slow_patterns", w.getvalue(), B.model(toks)))

    # the stream ends 0..8 literals after a match, then an end code of 1..15
    # bits: L - 1 literals on a chain 1..L-1, one more literal and 256 at L
    d2, raw2 = _one(rng, "fixed", [b"second member", (5, 6)])
    second = B.member(d2, raw2)
    for L in range(1, 16):
        ll = [0] * 286
        ll[256] = L
        if L < 15:  # the chain, then a literal and the match symbol one level below the end code
            lits, ll[257] = list(range(48, 48 + L)), L + 1
            lens = list(range(1, L)) + [L + 1]
        else:       # the match symbol takes the chain's 2
            lits, ll[257] = list(range(48, 48 + 14)), 2
            lens = [1] + list(range(3, 15)) + [15]
        for s, x in zip(lits, lens):
            ll[s] = x
        assert B.kraft(ll) == 1 << 15 and ll[256] == L
        for k in range(9):
            toks = [_rbytes(rng, 30, lits), (3, 1), _rbytes(rng, k, lits)]
            w = B.Deflate()
            w.dynamic(toks, ll, [1], True)
            raw = B.model(toks)
            out.append(_ok("C/end_code_%d_after_%d" % (L, k), w.getvalue(), raw))
            out.append(Case("C/end_code_%d_after_%d_two_members" % (L, k), B.member(w.getvalue(), raw) + second,
                            raw + raw2, True, None))
    return out


# ---------------------------------------------------------------- D: stored blocks
@functools.lru_cache(None)
def family_d():
    out, bad = [], []
    rng = np.random.default_rng(0xD)
    for n in (0, 1, 255, 256, 257, 65535):
        data = _rbytes(rng, n)
        w = B.Deflate().stored(data, True)
        out.append(_ok("D/len_%d_alone" % n, w.getvalue(), data))
        if n < 65535:
            w = B.Deflate()
            w.fixed([b"before", (4, 3)], False)
            w.stored(data, False)
            w.fixed([b"after", (6, 8)], True)
            out.append(_ok("D/len_%d_between" % n, w.getvalue(),
                           B.model([b"before", (4, 3), data, b"after", (6, 8)])))
    # the flush check every 256 bytes: blocks of 256 k + 1 across more than a flush of both rings
    w, raw = B.Deflate(), b""
    for k in range(1, 17):
        data = _rbytes(rng, 256 * k + 1)
        w.stored(data, k == 16)
        raw += data
    out.append(_ok("D/many_stored", w.getvalue(), raw))
    # empty stored blocks between Huffman blocks
    w = B.Deflate()
    t = [_rbytes(rng, 300), (30, 300)]
    w.fixed(t, False).stored(b"", False).stored(b"", False)
    _dyn(w, rng, t, 12, False)
    w.stored(b"", False).fixed(t, False).stored(b"", True)
    out.append(_ok("D/empty_between", w.getvalue(), B.model(t) * 3))
    # the same from zlib: Z_SYNC_FLUSH and Z_FULL_FLUSH end in an empty stored block
    parts = [_rbytes(rng, 3000, list(range(30))) for _ in range(3)]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    d = c.compress(parts[0]) + c.flush(zlib.Z_SYNC_FLUSH)
    assert d.endswith(b"\x00\x00\xff\xff")
    d += c.compress(parts[1]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(parts[2]) + c.flush()
    out.append(_ok("D/zlib_sync_full_flush", d, b"".join(parts)))
    # a stored block after a Huffman block that ends at each bit phase: 3
    # header bits, 8 bits per literal below 144, 9 above, 7 for the end code
    phases = set()
    for nine in range(8):
        w = B.Deflate()
        t = [bytes([65] * 5 + [200] * nine)]
        w.fixed(t, False)
        phases.add(w.bitpos % 8)
        data = _rbytes(rng, 700)
        w.stored(data, False)
        w.fixed([(9, 700 + nine)], True)
        out.append(_ok("D/stored_at_phase_%d" % (nine + 2 & 7), w.getvalue(), B.model([t[0], data, (9, 700 + nine)])))
    assert phases == set(range(8))
    # Huffman matches reaching more than 8128 bytes back into a stored block
    for kind in ("fixed", "dynamic"):
        data = _rbytes(rng, 9000)
        t = [(n, d_) for n in EDGE_LEN for d_ in (FAR + 1, RING, 9000)] + [_rbytes(rng, 70), (258, RING + 1)]
        w = B.Deflate().stored(data, False)
        if kind == "fixed":
            w.fixed(t, True)
        else:
            _dyn(w, rng, t, 12, True)
        out.append(_ok("D/far_match_into_stored_%s" % kind, w.getvalue(), B.model([data] + t)))
    # errors
    data = _rbytes(rng, 500)
    w = B.Deflate().stored(data, True, nlen=(~500 & 0xffff) ^ 0x100)
    bad.append(_bad("D/nlen_mismatch", w.getvalue(), "invalid stored block lengths", data))
    w = B.Deflate().stored(data, True, len_=0, nlen=0)
    bad.append(_bad("D/nlen_zero", w.getvalue(), "invalid stored block lengths", data))
    hdr = B.member(b"", b"")[:10]
    w = B.Deflate().stored(data, True)
    for cut in (1, 3, 5, 300):
        bad.append(Case("D/stored_cut_%d" % cut, hdr + w.getvalue()[:cut], None, False, "truncated"))
    # LEN larger than what is there: the trailer is taken for data, then the input ends
    w = B.Deflate().stored(data, True, len_=600, nlen=~600 & 0xffff)
    bad.append(_bad("D/len_past_end", w.getvalue(), "truncated", data))
    return out, bad


# ---------------------------------------------------------------- E: input staging
def _e_dynamic_headers(rng):
    """Blocks whose header (286 + 30 lengths, one symbol each: about 170
    bytes) is most of the block: a refill lands inside one at nearly every k."""
    w, raw = B.Deflate(), []
    for i in range(18):
        t = [_rbytes(rng, 30)] + ([(5, 7), (40, 25)] if i else [])
        ll = B.random_lens(rng, range(286), 12, 286)
        dl = B.random_lens(rng, range(30), 9, 30)
        w.dynamic(t, ll, dl, i == 17, runs=False)
        raw += t
    return w.getvalue(), B.model(raw)


def _e_long_codes(rng):
    """800 literals, then 640 matches of 39..43 bits each (a 15-bit length
    code with 1 extra bit, a 15-bit distance code with 7 or 8): some code or
    its extra bits lies across every refill from 1024 to 3072."""
    ll = [0] * 286
    for s in range(64):
        ll[s] = 7
    ll[256] = 2
    for s, x in zip(range(64, 76), range(3, 15)):
        ll[s] = x
    ll[265] = ll[266] = 15
    dl = [0] * 30
    for s, x in zip(range(14), range(1, 15)):
        dl[s] = x
    dl[17] = dl[18] = 15
    assert B.kraft(ll) == B.kraft(dl) == 1 << 15
    t = [_rbytes(rng, 800, list(range(64)))]
    for _ in range(640):
        t.append((int(rng.integers(11, 15)), int(rng.integers(385, 769))))
    w = B.Deflate()
    w.dynamic(t, ll, dl, True)
    assert len(w.getvalue()) > 3 * STAGE + 64
    return w.getvalue(), B.model(t)


def _e_stored_headers(rng):
    """Stored blocks of 0 and 1 bytes, 5 and 6 bytes each: a LEN / NLEN pair across every refill."""
    w, raw = B.Deflate(), bytearray()
    w.fixed([b"head"], False)
    raw += b"head"
    for i in range(600):
        data = bytes([i & 255]) if i % 3 == 0 else b""
        w.stored(data, False)
        raw += data
    w.fixed([(4, 3), b"tail"], True)
    raw += B.model([bytes(raw[-3:]), (4, 3), b"tail"])[3:]
    return w.getvalue(), bytes(raw)


@functools.lru_cache(None)
def family_e():
    out = []
    rng = np.random.default_rng(0xE)
    second = _one(rng, "fixed", [b"the second member", (9, 4)])
    streams = [("dynamic_headers",) + _e_dynamic_headers(rng), ("long_codes",) + _e_long_codes(rng),
               ("stored_headers",) + _e_stored_headers(rng)]
    for x in range(16):
        extra = bytes(range(x))
        for name, d, raw in streams:
            out.append(_ok("E/%s_fextra_%d" % (name, x), d, raw, extra=extra))
        # the trailer (and the next member's header) from byte `base` + x on:
        # with x = 0..15 it starts at every byte of 1000..1023 and 2016..2047
        # (a refill's window starts 16-byte aligned at or below the first byte
        # it lacks).  Literals below 144 are 8 bits each, so n of them and the
        # header / end code make n + 2 bytes of DEFLATE
        for base in (STAGE - 24, STAGE - 16, 2 * STAGE - 32, 2 * STAGE - 16):
            n = base - 14
            d, raw = _one(rng, "fixed", [_rbytes(rng, n, list(range(144)))])
            m = B.member(d, raw, extra=extra)
            assert len(d) == n + 2 and len(m) == base + x + 8
            out.append(Case("E/trailer_at_%d_fextra_%d" % (base, x), m + B.member(second[0], second[1]),
                            raw + second[1], True, None))
    return out


# ---------------------------------------------------------------- F: V2 pages
@functools.lru_cache(None)
def family_f():
    """(name, chunk bytes, def levels, values): an OPTIONAL INT64 column, raw
    RLE def levels in front of a GZIP body with matches further than 8128."""
    rng = np.random.default_rng(0xF)

    def half(size):
        toks = [_rbytes(rng, 9008)]
        while sum(_size(t) for t in toks) < size - 600:
            toks += [(int(rng.choice(EDGE_LEN)), int(rng.choice([FAR, FAR + 1, RING, 9000]))),
                     _rbytes(rng, int(rng.integers(0, 4)))]
        return toks + [_rbytes(rng, size - sum(_size(t) for t in toks))]

    pages = {"one_member": [], "two_members": []}
    defs_all, vals_all = [], []
    for nslots in (4000, 4501):
        defs = (rng.random(nslots) >= 0.2).astype(np.uint8)
        nn = int(defs.sum())
        t1, t2 = half(12000), half(nn * 8 - 12000)  # the second half's matches stay inside it
        d, raw = _one(rng, "dynamic", t1 + t2)
        (d1, r1), (d2, r2) = _one(rng, "dynamic", t1), _one(rng, "fixed", t2)
        assert r1 + r2 == raw and len(raw) == nn * 8
        lv = W.hybrid_encode(defs, 1)
        for name, gz in (("one_member", B.member(d, raw)), ("two_members", B.member(d1, r1) + B.member(d2, r2))):
            hdr = U.page_header_v2(len(lv) + len(raw), len(lv) + len(gz), nslots, nslots - nn, nslots, abi.ENC_PLAIN,
                                   len(lv), 0)
            pages[name].append(hdr + lv + gz)
        defs_all.append(defs)
        vals_all.append(raw)
    out = [(name, b"".join(pp), np.concatenate(defs_all), b"".join(vals_all)) for name, pp in pages.items()]
    return out


# ---------------------------------------------------------------- G: seeded structured fuzz
def _fuzz_tokens(rng, limit):
    toks, size = [_rbytes(rng, int(rng.integers(1, 300)))], 0
    size = len(toks[0])
    alphabet = list(rng.integers(0, 256, int(rng.integers(2, 200))))
    while size < limit:
        if rng.random() < 0.5:
            t = _rbytes(rng, int(rng.integers(1, 40) if rng.random() < 0.9 else rng.integers(40, 5000)), alphabet)
        else:
            ok = [d for d in EDGE_DIST if d <= size]
            d = int(rng.choice(ok)) if rng.random() < 0.5 else int(rng.integers(1, min(size, 32768) + 1))
            n = int(rng.choice(EDGE_LEN)) if rng.random() < 0.3 else int(rng.integers(3, 259))
            t = (n, d)
        if size + _size(t) > limit:
            break
        toks.append(t)
        size += _size(t)
    return toks


def _fuzz_stream(rng, limit):
    toks = _fuzz_tokens(rng, limit)
    nb = int(rng.integers(1, 7))
    cuts = sorted(int(c) for c in rng.integers(0, len(toks) + 1, nb - 1))
    blocks = []
    for lo, hi in zip([0] + cuts, cuts + [len(toks)]):
        kind = ("fixed", "dynamic", "dynamic", "stored")[int(rng.integers(0, 4))]
        if kind == "stored" and sum(_size(t) for t in toks[lo:hi]) > 65535:
            kind = "dynamic"
        blocks.append((kind, toks[lo:hi], int(rng.integers(1, 16))))
    return _stream(rng, blocks)


@functools.lru_cache(None)
def family_g():
    out = []
    for i in range(200):
        rng = np.random.default_rng(7000 + i)
        d, raw = _fuzz_stream(rng, int(rng.integers(1, 1 << 16) if i % 4 else rng.integers(40000, 1 << 16)))
        out.append(_ok("G/fuzz_%d" % i, d, raw))
    # one page of about 300 KiB: several wraps of the 32 KiB ring and of both index widths' flushes
    d, raw = _fuzz_stream(np.random.default_rng(7999), 300 * 1024)
    assert len(raw) > 290 * 1024
    out.append(_ok("G/big_300k", d, raw))
    return out


# ---------------------------------------------------------------- H: mutations
H_CASES, H_CAP = 200, 1 << 20


@functools.lru_cache(None)
def family_h():
    """(valid cases, error cases, dropped): 1-3 bytes of a DEFLATE stream
    overwritten.  zlib decides: a stream that still ends is framed with the
    CRC-32 and ISIZE of its new output (the GPU must give those bytes), any
    other keeps the original trailer (an error)."""
    rng = np.random.default_rng(0x11)
    toks = _fuzz_tokens(rng, 20000)
    bases = {"one_dynamic": _stream(rng, [("dynamic", toks, 12)]),
             "dynamic_500": _stream(rng, [("dynamic", toks[i:i + 500], 11) for i in range(0, len(toks), 500)]),
             "fixed": _stream(rng, [("fixed", toks, 0)])}
    good, bad, dropped = [], [], 0
    for name, (d, raw) in bases.items():
        for i in range(H_CASES):
            m = bytearray(d)
            for _ in range(int(rng.integers(1, 4))):
                m[int(rng.integers(0, len(m)))] = int(rng.integers(0, 256))
            m = bytes(m)
            z = zlib.decompressobj(-15)
            try:
                got = z.decompress(m, H_CAP)
            except zlib.error:
                got = None
            cname = "H/%s_%d" % (name, i)
            if got is not None and z.eof:
                good.append(_ok(cname, m[:len(m) - len(z.unused_data)], got))
            elif got is not None and len(got) >= H_CAP:
                dropped += 1
            else:
                bad.append(Case(cname, B.member(m, raw), None, False, ""))
    return good, bad, dropped


# ---------------------------------------------------------------- the checks
def _py_gunzip(gz):
    """Python's zlib, member by member."""
    out = b""
    while gz:
        z = zlib.decompressobj(31)
        out += z.decompress(gz)
        if not z.eof:
            raise zlib.error("truncated")
        gz = z.unused_data
    return out


def check_inputs(cases):
    """Model, zlib and oracle on every case (CPU)."""
    for c in cases:
        if c.ok:
            assert _py_gunzip(c.gz) == c.raw, c.name
            assert O.gzip_decode(c.gz, len(c.raw) + 64) == (0, c.raw), c.name
        else:
            with pytest.raises(zlib.error) as e:
                _py_gunzip(c.gz)
            assert c.why in str(e.value), (c.name, str(e.value))
            assert O.gzip_decode(c.gz, 1 << 21)[0] == GZIP, c.name


def _page(c):
    if c.ok:
        return _gz_page(c.raw, c.gz, len(c.raw) // 8)
    return U.page_header_v1(4096, len(c.gz), 512, abi.ENC_PLAIN) + c.gz


def _decode_chunks(dec, chunks, npages, **kw):
    """[(oracle, GPU)] of chunks (of npages[i] pages) decoded as the jobs of
    one call (dec None: the oracle twice)."""
    keep, jobs, exps = [], [], []
    for ch, n in zip(chunks, npages):
        job, _ = U.chunk_job(ch, keep=keep, **kw)
        exps.append(O.decode_chunk(job, page_cap=n + 8))
        jobs.append(job)
    if dec is None:
        return list(zip(exps, exps))
    blob, offs = bytearray(), []
    for buf in keep:
        blob += bytes(-len(blob) % 16)
        offs.append(len(blob))
        blob += buf.tobytes()
    blob += bytes(-len(blob) % 16)
    dev = dec.upload(np.frombuffer(bytes(blob), np.uint8))
    try:
        for job, off in zip(jobs, offs):
            job.data = dev + off
        res = dec.decode_jobs(jobs)
        gots = [dec.download(r) for r in res]
        for i, (g, n) in enumerate(zip(gots, npages)):
            g.pages = dec.pages(i, cap=n + 8)
        return list(zip(exps, gots))
    finally:
        dec.free(dev)


def check_pages(dec, cases, per_chunk=8 << 20):
    """Valid cases as the pages of a few chunks, invalid ones a chunk each, all in one decode."""
    groups, size = [[]], 0
    for c in cases:
        if not c.ok:
            continue
        if groups[-1] and size + len(c.raw) > per_chunk:
            groups.append([])
            size = 0
        groups[-1].append(c)
        size += len(c.raw)
    groups = [g for g in groups if g] + [[c] for c in cases if not c.ok]
    res = _decode_chunks(dec, [b"".join(_page(c) for c in g) for g in groups], [len(g) for g in groups],
                         ptype=abi.INT64, codec=abi.CODEC_GZIP)
    fails = []
    for g, (exp, got) in zip(groups, res):
        if not g[0].ok:
            assert exp.status == GZIP and exp.error_page == 0, g[0].name
            if (got.status, got.error_page) != (GZIP, 0):
                fails.append((g[0].name, abi.status_name(got.status)))
            continue
        assert exp.status == 0, (g[0].name, abi.status_name(exp.status), exp.error_page)
        if got.status != 0:
            fails.append((g[got.error_page].name, abi.status_name(got.status)))
            continue
        at, have = 0, np.asarray(got.values).tobytes()
        for c, pg in zip(g, got.pages):
            want = c.raw[:len(c.raw) // 8 * 8]  # trailing bytes are no value
            if have[at:at + len(want)] != want:
                fails.append((c.name, "bytes"))
            if pg.flags & REDO:
                fails.append((c.name, "second pass"))
            at += len(want)
        assert at == len(have) and len(got.pages) == len(g)
    if not fails:
        for exp, got in res:
            P.compare_chunk(exp, got, "chunk")
    return fails


def check_blocks(dec, cases):
    """pqg_block_decompress (k_inflate) on every case."""
    fails = []
    for c in cases:
        rc, n, dst = _gpu_block(dec, c.gz, (len(c.raw) if c.ok else 1 << 16) + 64)
        if c.ok and (rc != 0 or dst[:n].tobytes() != c.raw):
            fails.append((c.name, abi.status_name(rc)))
        elif not c.ok and rc != GZIP:
            fails.append((c.name, abi.status_name(rc)))
    return fails


def check_family(dec, cases, block_every=1):
    fails = []
    if dec is None:
        check_inputs(cases)
    else:
        fails += [("block",) + f for f in check_blocks(dec, cases[::block_every])]
    fails += [("page",) + f for f in check_pages(dec, cases)]
    assert not fails, "%d wrong:\n%s" % (len(fails), "\n".join(" ".join(f) for f in fails[:60]))


def check_v2(dec):
    for name, chunk, defs, vals in family_f():
        exp, got = _decode_chunks(dec, [chunk], [2], ptype=abi.INT64, codec=abi.CODEC_GZIP, max_def=1)[0]
        assert exp.status == 0, (name, abi.status_name(exp.status))
        P.compare_chunk(exp, got, name)
        assert np.array_equal(np.asarray(got.def_levels), defs), name
        assert np.asarray(got.values).tobytes() == vals, name
        assert not any(p.flags & REDO for p in got.pages), name


FAMILIES = {
    "A_tables": lambda: family_a(),
    "A_tables_invalid": lambda: family_a_bad(),
    "B_pairs": lambda: family_b_pairs(),
    "B_prefix": lambda: family_b_prefix(),
    "B_members": lambda: family_b_members()[0] + family_b_members()[1],
    "C_literal_runs": lambda: family_c(),
    "D_stored": lambda: family_d()[0] + family_d()[1],
    "E_staging": lambda: family_e(),
}
for _base in ("one_dynamic", "dynamic_500", "fixed"):
    FAMILIES["H_mutations_" + _base] = lambda b=_base: [c for c in family_h()[0] + family_h()[1]
                                                        if c.name.startswith("H/%s_" % b)]



# ---------------------------------------------------------------- CPU: model, zlib and oracle
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_oracle_family(family):
    check_family(None, FAMILIES[family]())


def test_oracle_fuzz():
    cases = family_g()
    assert len(cases) == 201 and all(c.ok for c in cases)
    check_family(None, cases)


def test_oracle_v2_pages():
    check_v2(None)


def test_mutation_conditions():
    """Conditions on the inputs of family H: few cases dropped for their
    size, and at least a quarter of the rest still valid for the oracle."""
    good, bad, dropped = family_h()
    total = 3 * H_CASES
    assert len(good) + len(bad) + dropped == total
    assert dropped < 0.05 * total, dropped
    ok = sum(O.gzip_decode(c.gz, H_CAP + 64)[0] == 0 for c in good + bad)
    assert ok == len(good) and ok >= 0.25 * (len(good) + len(bad)), (ok, len(bad), dropped)


def test_families_cover_their_edges():
    """What the case lists claim, counted."""
    names = {c.name for f in FAMILIES.values() for c in f()}
    for kind in ("fixed", "dynamic"):
        for d in EDGE_DIST:
            assert "B/%s/dist_%d" % (kind, d) in names
        for d in (FAR, FAR + 1, RING):
            for pre in range(64):
                assert "B/%s/dist_%d_prefix_%d" % (kind, d, pre) in names
    for L in range(1, 16):
        for k in range(9):
            assert "C/end_code_%d_after_%d" % (L, k) in names
    for x in range(16):
        for what in ("dynamic_headers", "long_codes", "stored_headers", "trailer_at_%d" % (STAGE - 16)):
            assert "E/%s_fextra_%d" % (what, x) in names


def test_model_bites():
    """The comparison is not vacuous: a match one byte nearer gives other bytes."""
    rng = np.random.default_rng(3)
    hist = _rbytes(rng, 9000)
    a = B.model([hist, (258, FAR)])
    b = B.model([hist, (258, FAR - 1)])
    assert a[:9000] == b[:9000] and a[9000:] != b[9000:]
    d, raw = _one(rng, "dynamic", [hist, (258, FAR)])
    assert raw == a and zlib.decompress(d, -15) == a


# ---------------------------------------------------------------- GPU: both kernels against all of it
@pytest.fixture(scope="module")
def dec():
    import pqgpu
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_gpu_family(dec, family):
    check_family(dec, FAMILIES[family]())


@pytest.mark.gpu
def test_gpu_fuzz(dec):
    check_family(dec, family_g(), block_every=8)


@pytest.mark.gpu
def test_gpu_v2_pages(dec):
    check_v2(dec)
