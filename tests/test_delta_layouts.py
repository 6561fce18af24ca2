"""DELTA_BINARY_PACKED on layouts the generator's writer cannot make.

The writer (gen/pqwrite.cpp) emits 128-value blocks of 4 x 32 miniblocks only,
so most of k_values<3> (pqg_values.hip: dbp_decode, dbp_tile, dbp_decode_rest,
store_run64) and of k_str_delta's walker (pqg_strings.hip) never saw valid data
of any other shape.  Here the streams are built by hand (dbp_stream /
dbp_from_values) together with a plain model of the format in Python integers:

    v[0] = first, v[p + 1] = (v[p] + packed[p] + min_delta[block(p)]) mod 2^bits

The CPU tests pin the oracle (deltabp_decoder.go:14-334 restated) on the model;
the GPU tests compare the kernels with the oracle byte for byte
(parity.compare_chunk_bytes) and, wherever the model applies, with the model
directly, so that a misreading shared by the oracle and a kernel cannot hide.

The model is not consulted only for layouts whose miniblock value count is no
multiple of 8 (the reference reads mbvc / 8 groups per miniblock there, which
is not the format: the oracle alone is the expectation) and for truncated or
failing streams.

Constants of pqg_values.hip the cases are sized by: the LDS stage of the staged
path holds 4096 bytes (PQG_DBP_STAGE), a batch is at most 64 blocks (kBlocks),
the tile split packs at most 8 miniblock widths (kMaxMb), a tile is 256
positions (4 per lane)."""
import functools
import math

import numpy as np
import pytest

import parity as P
import pqtest_util as U
from gen import pqwrite as W
from oracle import pyoracle as O
from pqgpu import abi

DBP = W.DELTA_BINARY_PACKED
DLBA = W.DELTA_LENGTH_BYTE_ARRAY
STAGE, KBLOCKS, KMAXMB, TILE = 4096, 64, 8, 256
EOF = abi.STATUS_CODES["EOF"]
DELTA = abi.STATUS_CODES["DELTA"]
BIT_WIDTH = abi.STATUS_CODES["BIT_WIDTH"]


# ---------------------------------------------------------------- builder and model
def _pack8(vals, w):
    """Eight w-bit values, least significant bit first: w bytes."""
    acc = 0
    for i, v in enumerate(vals):
        acc |= v << (i * w)
    return acc.to_bytes(w, "little")


def _served(mbvc):
    """Positions one miniblock serves as the reference reads it: a miniblock
    starts at a group start (a multiple of 8) that is a multiple of mbvc, so
    lcm(8, mbvc); mbvc itself for every layout that follows the format."""
    return mbvc // math.gcd(mbvc, 8) * 8


def _signed(vals, bits):
    if bits == 32:
        return np.array(vals, dtype=np.uint32).view(np.int32)
    return np.array(vals, dtype=np.uint64).view(np.int64)


class Built:
    """A built stream: bytes, the model's values, and per block the stream
    offsets of its header, width bytes, body and end, and its widths."""

    def __init__(self, stream, expected, blocks, bs, mbc):
        self.stream, self.expected, self.blocks, self.bs, self.mbc = stream, expected, blocks, bs, mbc

    def group_end(self, P_):
        """End offset of the last group that a position below P_ reads."""
        mbvc = self.bs // self.mbc
        pos = (P_ - 1) // 8 * 8
        blk = self.blocks[pos // self.bs]
        rel = pos % self.bs
        m_last, g = rel // mbvc, (rel % mbvc) // 8
        off = blk["body"] + sum(mbvc // 8 * w for w in blk["widths"][:m_last])
        return off + (g + 1) * blk["widths"][m_last]


def build_stream(rng, bits, bs, mbc, n, widths, *, first=None, mind=None, announce=None, ones=False,
                 mind_raw=None):
    """See dbp_stream.  mind: list or callable of the block; mind_raw(b): the
    bytes of block b's min delta when not None (for redundant varint forms);
    ones: every packed delta is 2^w - 1."""
    mbvc = bs // mbc
    L = _served(mbvc)
    ebs = L * mbc
    mask = (1 << bits) - 1
    if first is None:
        first = int(rng.integers(-100000, 100000))
    out = bytearray(U.uvarint(bs) + U.uvarint(mbc) + U.uvarint(n if announce is None else announce) + U.zigzag(first))
    packed, minds, blocks = [], [], []
    for b in range(-(-n // ebs)):
        if mind is None:
            md = int(rng.integers(-3000, 3000))
        else:
            md = mind(b) if callable(mind) else mind[b]
        raw = mind_raw(b) if mind_raw is not None else None
        hdr = len(out)
        out += U.zigzag(md) if raw is None else raw
        ws = [widths(b, m) for m in range(mbc)]
        wat = len(out)
        out += bytes(ws)
        body = len(out)
        for w in ws:
            wm = (1 << w) - 1
            if ones:
                d = [wm] * L
            else:
                d = (rng.integers(0, 256, size=(L, 8), dtype=np.uint8).view(np.uint64).reshape(L)
                     & np.uint64(wm)).tolist()
                if w:
                    d[int(rng.integers(0, L))] |= 1 << (w - 1)  # the width's top bit is used
            for g in range(0, L, 8):
                out += _pack8(d[g:g + 8], w)
            packed += d
        minds.append(md)
        blocks.append(dict(hdr=hdr, widths_at=wat, body=body, end=len(out), widths=ws))
    v, vals = first & mask, []
    for p in range(n):
        vals.append(v)
        v = (v + packed[p] + minds[p // ebs]) & mask
    return Built(bytes(out), _signed(vals, bits), blocks, bs, mbc)


def dbp_stream(rng, bits, bs, mbc, n, widths, *, first=None, mind=None, announce=None, **kw):
    """A DBP stream of n values in blocks of bs values and mbc miniblocks:
    uvarint(bs) uvarint(mbc) uvarint(announce or n) zigzag(first), then per
    block zigzag(min delta), mbc width bytes (widths(b, m)) and every
    miniblock in full, random deltas in [0, 2^w).  ceil(n / bs) blocks: the
    reference reads a delta for the last position too
    (deltabp_decoder.go:114-175, Q3).  Returns (bytes, expected): expected from
    Python integers, wrapping at `bits`, viewed as signed."""
    b = build_stream(rng, bits, bs, mbc, n, widths, first=first, mind=mind, announce=announce, **kw)
    return b.stream, b.expected


def dbp_from_values(values, bits, bs, mbc, widen=0):
    """Encode `values`: per block the minimum delta, per miniblock the bit
    length of its largest packed delta plus `widen`.  The stream ends where the
    reference's reader stops after the last group (deltabp_decoder.go:154-171):
    the whole last block when mbvc % 8 == 0 (its unused miniblocks hold only
    padding, so they share one width and the skip with
    miniBlockBitWidth[currentMiniBlock] is exact), the end of the last group
    otherwise."""
    vals = [int(v) for v in values]
    n = len(vals)
    mbvc = bs // mbc
    L = _served(mbvc)
    ebs = L * mbc
    out = bytearray(U.uvarint(bs) + U.uvarint(mbc) + U.uvarint(n) + U.zigzag(vals[0]))
    deltas = [vals[p + 1] - vals[p] for p in range(n - 1)]
    last = (n - 1) // 8 * 8  # the last group read
    stop = None
    for b in range(-(-n // ebs)):
        real = deltas[b * ebs:(b + 1) * ebs]
        md = min(real) if real else 0
        pk = [d - md for d in real] + [0] * (ebs - len(real))
        ws = [min(bits, max(x.bit_length() for x in pk[m * L:(m + 1) * L]) + widen) for m in range(mbc)]
        out += U.zigzag(md) + bytes(ws)
        for m, w in enumerate(ws):
            for g in range(0, L, 8):
                out += _pack8(pk[m * L + g:m * L + g + 8], w)
                if b * ebs + m * L + g == last:
                    mbpos = (g // 8 + 1) * w
                    assert mbvc // 8 * w - mbpos >= 0, "the reference rejects this count (invalid stream)"
                    stop = len(out) + mbvc // 8 * w - mbpos
                    if m + 1 < mbc:
                        stop += (mbc - m - 1) * (mbvc // 8) * ws[m + 1]
    if mbvc % 8 == 0:
        assert stop == len(out)
    return bytes(out[:stop])


def _rand_widths(rng, bits, lo=0):
    return lambda b, m: int(rng.integers(lo, bits + 1))


def _ptype(bits):
    return abi.INT32 if bits == 32 else abi.INT64


def _dtype(bits):
    return np.int32 if bits == 32 else np.int64


# ---------------------------------------------------------------- the cases
# A case is a list of pages (stream, page value count, model values or None)
# that make one chunk of v1 pages.
def _sweep_pages(bits, w):
    """Four 128/4 pages of 333, 334, 335 and 338 values: the pages' values
    start at 0, 4, 12, 8 bytes mod 16 (INT32: every store_run_aligned<4>
    shift) and 0, 8, 8, 0 (INT64: store_run64 unshifted and shifted); each is
    one full tile of 256 positions (Full) plus a ragged one whose last lane
    holds 1, 2, 3 or 2 values.  Block 0: four miniblocks of width w; block 1:
    (w, bits - w, 0, w); block 2: random.  Each miniblock holds 32 values, so
    a width w puts values at every bit offset w * j mod 32: both unpack
    branches (<= 32, > 32: three dwords) at every offset, width 0 and 64."""
    rng = np.random.default_rng(1000 * bits + w)
    fixed = {0: (w, w, w, w), 1: (w, bits - w, 0, w)}

    def widths(b, m):
        return fixed[b][m] if b in fixed else int(rng.integers(0, bits + 1))

    pages = []
    for n in (333, 334, 335, 338):
        assert TILE < n < 2 * TILE
        s, e = dbp_stream(rng, bits, 128, 4, n, widths)
        pages.append((s, n, e))
    return pages


SWEEP = [(bits, w) for bits in (32, 64) for w in range(bits + 1)]

# Regular layouts (mbvc % 8 == 0, mbc <= kMaxMb = 8): powers of two take
# the shift split of dbp_tile, 384/3, 640/5, 24/3, 40/5 the division split;
# 8/1 is the smallest block (32 blocks per tile).  144/9 (mbc > kMaxMb) and
# 12/1, 40/2 (mbvc % 8 != 0) take the one-lane walk.
LAYOUTS = [(128, 1), (128, 2), (128, 8), (256, 4), (256, 8), (512, 4), (1024, 4),
           (384, 3), (640, 5), (24, 3), (40, 5), (8, 1), (144, 9), (12, 1), (40, 2)]


def _counts(bs, mbc):
    # 3 * bs + 77: a partial last block; 66 * bs + 5: more than kBlocks = 64
    # blocks, so a second batch with a carried value
    out = [3 * bs + 77] + ([(KBLOCKS + 2) * bs + 5] if bs <= 256 else [])
    if (bs // mbc) % 8:
        # mbvc % 8 != 0: the reference reads mbvc / 8 groups per miniblock and
        # calls a stream whose last group is not the first of its miniblock
        # invalid (deltabp_decoder.go:154-158), so 3 * bs + 77 fails with DELTA
        # for 12/1 and 40/2 (asserted); 66 * bs + 5 and this count decode
        out.append(3 * _served(bs // mbc) * mbc + 3)
    return out


def _last_group_first(n, bs, mbc):
    """The last group a stream of n values reads is the first of its miniblock."""
    return (n - 1) // 8 * 8 % _served(bs // mbc) == 0


assert all(mbc <= KMAXMB for bs, mbc in LAYOUTS[:12]) and LAYOUTS[12][1] > KMAXMB
LAYOUT_CASES = [(bits, bs, mbc, n) for bits in (32, 64) for bs, mbc in LAYOUTS for n in _counts(bs, mbc)]


def layout_pages(bits, bs, mbc, n):
    """An odd count, then a second page in the same chunk: its values start at
    an odd element offset (4 mod 8 / 8 mod 16 bytes)."""
    rng = np.random.default_rng(bits * 100003 + bs * 101 + mbc * 7 + n)
    model = (bs // mbc) % 8 == 0
    # mbvc % 8 != 0: a second count the reference accepts, and no zero widths
    # (a zero-width last miniblock would hide the invalid-stream rule)
    n2 = 2 * bs + 10 if model else 2 * _served(bs // mbc) * mbc + 5
    assert n % 2 == 1 and (model or _last_group_first(n2, bs, mbc))
    pages = []
    for cnt in (n, n2):
        s, e = dbp_stream(rng, bits, bs, mbc, cnt, _rand_widths(rng, bits, lo=0 if model else 1))
        pages.append((s, cnt, e if model else None))
    return pages


# Blocks larger than the stage: a 1024/4 block's body is 32 * (sum of
# widths) bytes (8192 at 4 x 64, 4096 at 4 x 32), a 512/4 block's 16 * sumw
# (4096 at 4 x 64): none fits the 4096-byte stage together with its header, so
# dbp_decode hands the first block to dbp_decode_rest (entered directly, p0 =
# 0).  The counts leave a partial last block.
BIG_BLOCKS = [(64, 1024, 4, 64), (32, 1024, 4, 32), (64, 512, 4, 64)]


def big_block_pages(bits, bs, mbc, w):
    rng = np.random.default_rng(bits + bs + w)
    assert 1 + mbc + bs // 8 * w > STAGE  # the shortest header and the body
    n = 2 * bs + 301
    s, e = dbp_stream(rng, bits, bs, mbc, n, lambda b, m: w)
    s2, e2 = dbp_stream(rng, bits, bs, mbc, bs + 3, lambda b, m: w)
    return [(s, n, e), (s2, bs + 3, e2)]


# The fit / no-fit edge.  A block is staged from the 16-byte aligned address
# at or below its header, so it fits when (header address mod 16) + (min delta
# bytes) + mbc + body <= 4096.  1024/4: body = 32 * sumw, so sumw <= 127 fits at
# every address (4064 + 4 + 10 + 15 <= 4096) and sumw = 128 never does.  512/4:
# body = 16 * sumw, so sumw = 255 (4080 bytes) fits only when address mod 16 +
# min delta bytes <= 12: there the edge moves with the address and the varint.
_MD_BY_LEN = {1: -7, 2: 1000, 5: 1 << 30, 10: -(1 << 63)}
EDGE_CASES = [(1024, sumw, vl) for sumw in (125, 126, 127, 128) for vl in (1, 2, 5, 10)] + \
             [(512, sumw, vl) for sumw in (254, 255, 256) for vl in (1, 2, 5, 10)]
# def-level sections of four lengths in front of the values: RLE runs of value
# 1, (count << 1) as a varint and one value byte each
_DEF_PADS = [[], [1], [64], [1, 64]]  # + 0, 2, 3, 5 bytes


def _split_widths(sumw):
    ws, left = [], sumw
    for _ in range(4):
        ws.append(min(64, left))
        left -= ws[-1]
    return ws


def _all_defined(n, pad):
    runs = pad + [n - sum(pad)]
    return b"".join(U.uvarint(c << 1) + b"\x01" for c in runs)


def edge_streams(bs, sumw, vl):
    """INT64 (a 10-byte min delta is valid there): three blocks of the same
    widths and min delta length, then a partial one."""
    rng = np.random.default_rng(bs * 1000 + sumw * 16 + vl)
    ws = _split_widths(sumw)
    n = 3 * bs + 45
    assert len(U.zigzag(_MD_BY_LEN[vl])) == vl
    return build_stream(rng, 64, bs, 4, n, lambda b, m: ws[m], mind=lambda b: _MD_BY_LEN[vl]), n


# The hand-over.  1024/4, INT64, 10 blocks + 19 values.  Narrow blocks have
# widths (3, 3, 3, 3): 6 + 32 * 12 = 390 bytes, so the stage (4096) takes the
# first six with room to spare and the staged path batches and decodes them;
# the large block (4 x 64: body 8192 > 4096) cannot be staged even from a fresh
# fill, so dbp_decode_rest is entered at p0 = 6 * 1024 with the carried value,
# and decodes the narrow blocks after it and the partial last block too.
# `large_at` = 0: the large block is first (entered directly).
def handover_build(large_at):
    rng = np.random.default_rng(77 + large_at)
    n = 10 * 1024 + 19
    assert 15 + 6 * (2 + 4 + 32 * 12) < STAGE < 32 * 256
    return build_stream(rng, 64, 1024, 4, n, lambda b, m: 64 if b == large_at else 3, first=123456789), n


# A valid min delta with redundant zero continuation bytes (binary.ReadUvarint
# takes them): 0x80 0x00 and ten bytes 0x80 x 9 + 0x00, both the value 0.
def redundant_build(form, bs):
    rng = np.random.default_rng(5 + len(form) + bs)
    n = 5 * bs + 9
    # 128/4: the staged walk (init reads block 0's header, the exact walk block
    # 2's, block 3 follows a block of another length).  1024/4 at width 64
    # (body 8192 > the 4096-byte stage): read_signed of dbp_decode_rest
    widths = _rand_widths(rng, 20) if bs == 128 else (lambda b, m: 64)
    return build_stream(rng, 64, bs, 4, n, widths, mind=lambda b: 0,
                        mind_raw=lambda b: form if b in (0, 2, 3) else None), n


REDUNDANT = [(bytes([0x80, 0x00]), 128), (bytes([0x80] * 9 + [0x00]), 128), (bytes([0x80] * 9 + [0x00]), 1024)]

# Where the count ends (k = 2 whole blocks before): block start + 1,
# inside a miniblock, the last value of a group, the first value of a group,
# a block end.
END_LAYOUTS = [(bits, bs, mbc) for bits in (32, 64) for bs, mbc in ((128, 4), (256, 8))]


def _end_counts(bs, mbc):
    mbvc = bs // mbc
    return [2 * bs + 1, 2 * bs + mbvc + 13, 2 * bs + mbvc + 16, 2 * bs + mbvc + 9, 3 * bs]


# Arithmetic edges, 128/4.
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


@functools.lru_cache(None)
def arith_builds():
    """(name, bits, Built, n): the model applies to each."""
    out = []
    rng = np.random.default_rng(31)
    n = 4 * 128 + 50
    for name, first, minds in (("i64_min_first_max", I64_MAX, [I64_MIN, I64_MAX, I64_MIN, -1, I64_MAX]),
                               ("i64_max_first_min", I64_MIN, [I64_MAX, I64_MIN, 1, I64_MAX, I64_MIN])):
        out.append((name, 64, build_stream(rng, 64, 128, 4, n, _rand_widths(rng, 64), first=first, mind=minds), n))
        out.append((name + "_ones", 64, build_stream(rng, 64, 128, 4, n, lambda b, m: 64, first=first, mind=minds,
                                                     ones=True), n))
    for name, first, minds in (("i32_min", I32_MAX, [I32_MIN, I32_MAX, I32_MIN, -1, I32_MAX]),
                               ("i32_max", I32_MIN, [I32_MAX, I32_MIN, 1, I32_MAX, I32_MIN])):
        out.append((name, 32, build_stream(rng, 32, 128, 4, n, lambda b, m: 32, first=first, mind=minds, ones=True),
                    n))
    return out


@functools.lru_cache(None)
def bad_header_chunks():
    """(name, bits, chunk, expected status): 128/4 streams of 72 equal-length
    blocks.  Block 0's header is read by init; block 1 by the exact walk;
    block 70 lies past the first batch of kBlocks = 64 and within the 64
    headers the speculative walk reads from block 64 on (equal block lengths
    keep it going up to the bad one)."""
    out = []
    n = 72 * 128
    for bits in (32, 64):
        for blk in (0, 70):
            rng = np.random.default_rng(bits + blk)
            b = build_stream(rng, bits, 128, 4, n, lambda b_, m: 9, mind=lambda b_: 5)
            s = bytearray(b.stream)
            s[b.blocks[blk]["widths_at"] + 2] = bits + 1
            out.append(("width_%d_blk%d" % (bits, blk), bits, U.v1_page(bytes(s), n, DBP), BIT_WIDTH))
    for blk in (0, 1, 70):
        for md in (1 << 31, -(1 << 31) - 1):
            rng = np.random.default_rng(blk)
            # five-byte min deltas in every block: equal block lengths
            b = build_stream(rng, 32, 128, 4, n, lambda b_, m: 9,
                             mind=lambda b_, blk=blk, md=md: md if b_ == blk else (1 << 30))
            out.append(("md_%s_blk%d" % ("hi" if md > 0 else "lo", blk), 32, U.v1_page(b.stream, n, DBP), DELTA))
    return out


# Optional column, 256/8, three pages, about 10 % nulls.
def optional_pages(bits):
    rng = np.random.default_rng(600 + bits)
    pages = []
    for nvals in (1501, 1800, 777):
        defs = (rng.random(nvals) >= 0.1).astype(np.uint8)
        if not pages and defs.sum() % 2 == 0:
            defs[np.nonzero(defs)[0][0]] = 0  # an odd count in the first page
        nn = int(defs.sum())
        s, e = dbp_stream(rng, bits, 256, 8, nn, _rand_widths(rng, bits))
        pages.append((s, nvals, e, defs))
    # the second page's values start at an odd element offset
    assert len(pages[0][2]) % 2 == 1
    return pages


# DELTA_LENGTH_BYTE_ARRAY lengths.
DLBA_CASES = [(bs, mbc, widen) for bs, mbc in ((256, 8), (1024, 4), (384, 3), (24, 3), (12, 1)) for widen in (0, 3)]


def dlba_page(bs, mbc, widen):
    rng = np.random.default_rng(bs * 10 + mbc + widen)
    lens = rng.integers(0, 41, 700)
    chars = rng.integers(97, 123, int(lens.sum()), dtype=np.uint8)
    stream = dbp_from_values(lens, 32, bs, mbc, widen)
    return stream, lens, chars


# ---------------------------------------------------------------- the checks
# Every check takes `dec`: a GpuDecoder (the -m gpu tests: the kernels against
# the oracle, then against the model) or None (the CPU tests: the oracle's
# chunk decode stands in for the GPU's, so the same assertions pin the oracle
# on the model and on the expected statuses).
def _through(dec, chunk, **kw):
    if dec is not None:
        return P.compare_chunk_bytes(chunk, dec, **kw)
    keep = []
    exp = O.decode_chunk(U.chunk_job(chunk, keep=keep, **kw)[0], page_cap=16)
    return exp, exp


def _chunk(pages):
    return b"".join(U.v1_page(p[0], p[1], DBP) for p in pages)


def _pages(dec, pages, bits, want=0):
    """The chunk of `pages` (stream, count, model values or None); `want`: the
    status the oracle must give (None: whatever it gives)."""
    exp, got = _through(dec, _chunk(pages), ptype=_ptype(bits))
    if want is not None:
        assert exp.status == want, abi.status_name(exp.status)
    if exp.status == 0 and all(p[2] is not None for p in pages):
        model = np.concatenate([p[2] for p in pages])
        have = np.asarray(got.values).view(_dtype(bits))
        assert have.shape == model.shape
        assert np.array_equal(have, model), "first difference at value %d" % int(np.nonzero(have != model)[0][0])
        if dec is None:  # the stream decoder on its own too
            for s, n, e in pages:
                rc, v = O.delta_decode(s, n, bits)
                assert rc == 0 and v.dtype == e.dtype and np.array_equal(v, e)
    return exp, got


def check_width_sweep(dec, bits, w):
    _pages(dec, _sweep_pages(bits, w), bits)


def check_layout(dec, bits, bs, mbc, n):
    # regular layouts and 144/9 decode; so do 12/1 and 40/2 (every value
    # against the oracle's) unless the count is one the reference rejects
    ok = (bs // mbc) % 8 == 0 or _last_group_first(n, bs, mbc)
    exp, _ = _pages(dec, layout_pages(bits, bs, mbc, n), bits, want=0 if ok else DELTA)
    if not ok:
        assert exp.error_page == 0
    else:
        assert exp.num_values > n and exp.values.nbytes == exp.num_values * bits // 8


def check_big_blocks(dec, bits, bs, mbc, w):
    _pages(dec, big_block_pages(bits, bs, mbc, w), bits)


def check_stage_edge(dec, bs, sumw, vl):
    b, n = edge_streams(bs, sumw, vl)
    at = set()
    for pad in _DEF_PADS:
        chunk = U.v1_page(b.stream, n, DBP, defs=_all_defined(n, list(pad)))
        at.add((len(chunk) - len(b.stream)) % 16)
        exp, got = _through(dec, chunk, ptype=abi.INT64, max_def=1)
        assert exp.status == 0 and exp.num_values == n
        assert np.array_equal(np.asarray(got.values).view(np.int64), b.expected), pad
    assert len(at) == 4  # four addresses mod 16


def check_handover(dec, large_at):
    b, n = handover_build(large_at)
    _pages(dec, [(b.stream, n, b.expected)], 64)


def check_redundant(dec, form, bs):
    b, n = redundant_build(form, bs)
    _pages(dec, [(b.stream, n, b.expected)], 64)


def check_count_ends(dec, bits, bs, mbc):
    rng = np.random.default_rng(bits + bs)
    for n in _end_counts(bs, mbc):
        s, e = dbp_stream(rng, bits, bs, mbc, n, _rand_widths(rng, bits))
        _pages(dec, [(s, n, e)], bits)
        # announce > nn: P = nn, the page takes fewer values than the stream holds
        _pages(dec, [(s, n - 37, e[:n - 37])], bits)
        _pages(dec, [(s, 1, e[:1])], bits)
        # announce < nn: the positions run out (EOF)
        _pages(dec, [(s, n + 1, None)], bits, want=EOF)
        _pages(dec, [(s, n + 300, None)], bits, want=EOF)


def _cuts(dec, b, bits, counts):
    """The stream cut around the end of the last group that a position below
    the page's count reads (g_end of dbp_decode / dbp_decode_rest): whole ->
    OK, one byte short -> EOF, anywhere up to the block's end -> OK."""
    for cnt in counts:
        ge = b.group_end(cnt)
        blk = b.blocks[(cnt - 1) // b.bs]
        # widths >= 2 and counts that end before a miniblock's last group
        assert ge - 1 > blk["body"] and ge + 2 <= blk["end"]
        _pages(dec, [(b.stream[:ge], cnt, b.expected[:cnt])], bits)
        _pages(dec, [(b.stream[:ge - 1], cnt, None)], bits, want=EOF)
        _pages(dec, [(b.stream[:ge + 1], cnt, b.expected[:cnt])], bits)
        _pages(dec, [(b.stream[:(ge + blk["end"]) // 2], cnt, b.expected[:cnt])], bits)
    # one delta missing: a stream of n - 1 deltas with (n - 1) % bs == 0 lacks
    # the block that position n - 1 reads (Q3) -> EOF; n - 1 values are there
    n = 2 * b.bs + 1
    assert b.blocks[1]["end"] == b.blocks[2]["hdr"]
    _pages(dec, [(b.stream[:b.blocks[1]["end"]], n, None)], bits, want=EOF)
    _pages(dec, [(b.stream[:b.blocks[1]["end"]], n - 1, b.expected[:n - 1])], bits)


def check_stream_cuts(dec, bits, bs, mbc):
    """Staged path.  The stream announces 3 * bs values; the page takes fewer
    (nn < total) and ends in the third block: one value into it, inside a
    miniblock, at a group's last and first value, and in the last miniblock."""
    rng = np.random.default_rng(bits * 3 + bs)
    b = build_stream(rng, bits, bs, mbc, 3 * bs, _rand_widths(rng, bits, lo=2))  # lo: see _cuts
    mbvc = bs // mbc
    _cuts(dec, b, bits, [2 * bs + 1, 2 * bs + mbvc + 13, 2 * bs + mbvc + 16, 2 * bs + mbvc + 9, 3 * bs - 9])


def check_stream_cuts_rest(dec):
    """The same through dbp_decode_rest: 1024/4 at width 64 (body 8192 > the
    4096-byte stage), which is entered with a partial last block."""
    rng = np.random.default_rng(9)
    bs = 1024
    b = build_stream(rng, 64, bs, 4, 3 * bs, lambda b_, m: 64)
    _cuts(dec, b, 64, [2 * bs + 1, 2 * bs + 256 + 13, 2 * bs + 256 + 16, 2 * bs + 256 + 9, 3 * bs - 9])


def check_arithmetic(dec, name):
    _, bits, b, n = next(c for c in arith_builds() if c[0] == name)
    _pages(dec, [(b.stream, n, b.expected)], bits)


def check_bad_header(dec, name):
    _, bits, chunk, want = next(c for c in bad_header_chunks() if c[0] == name)
    exp, _ = _through(dec, chunk, ptype=_ptype(bits))
    assert exp.status == want, abi.status_name(exp.status)


def check_optional(dec, bits):
    pages = optional_pages(bits)
    chunk = b"".join(U.v1_page(s, nvals, DBP, defs=W.hybrid_encode(defs, 1)) for s, nvals, _, defs in pages)
    exp, got = _through(dec, chunk, ptype=_ptype(bits), max_def=1)
    assert exp.status == 0
    assert np.array_equal(np.asarray(got.def_levels), np.concatenate([p[3] for p in pages]))
    assert np.array_equal(np.asarray(got.values).view(_dtype(bits)), np.concatenate([p[2] for p in pages]))


def check_dlba(dec, bs, mbc, widen):
    stream, lens, chars = dlba_page(bs, mbc, widen)
    # the stream ends where the reference's reader does: the value bytes start there
    assert O.delta_lengths_end(stream, len(lens)) == (0, len(stream), len(lens))
    exp, got = _through(dec, U.v1_page(stream + chars.tobytes(), len(lens), DLBA), ptype=abi.BYTE_ARRAY)
    assert exp.status == 0
    assert np.array_equal(np.asarray(got.offsets), np.concatenate([[0], np.cumsum(lens)]))
    assert np.array_equal(np.asarray(got.values), chars)


_form_id = lambda v: "%dbytes" % len(v) if isinstance(v, bytes) else str(v)  # noqa: E731
ARITH = ["i64_min_first_max", "i64_min_first_max_ones", "i64_max_first_min", "i64_max_first_min_ones", "i32_min",
         "i32_max"]
BAD_HEADERS = ["width_%d_blk%d" % (bits, blk) for bits in (32, 64) for blk in (0, 70)] + \
              ["md_%s_blk%d" % (s, blk) for blk in (0, 1, 70) for s in ("hi", "lo")]


# ---------------------------------------------------------------- CPU: the oracle against the model
@pytest.mark.parametrize("bits,w", SWEEP)
def test_oracle_width_sweep(bits, w):
    check_width_sweep(None, bits, w)


@pytest.mark.parametrize("bits,bs,mbc,n", LAYOUT_CASES)
def test_oracle_layouts(bits, bs, mbc, n):
    check_layout(None, bits, bs, mbc, n)


@pytest.mark.parametrize("bits,bs,mbc,w", BIG_BLOCKS)
def test_oracle_big_blocks(bits, bs, mbc, w):
    check_big_blocks(None, bits, bs, mbc, w)


@pytest.mark.parametrize("bs,sumw,vl", EDGE_CASES)
def test_oracle_stage_edge(bs, sumw, vl):
    check_stage_edge(None, bs, sumw, vl)


@pytest.mark.parametrize("large_at", [6, 0])
def test_oracle_handover(large_at):
    check_handover(None, large_at)


@pytest.mark.parametrize("form,bs", REDUNDANT, ids=_form_id)
def test_oracle_redundant_varint(form, bs):
    check_redundant(None, form, bs)


@pytest.mark.parametrize("bits,bs,mbc", END_LAYOUTS)
def test_oracle_count_ends(bits, bs, mbc):
    check_count_ends(None, bits, bs, mbc)


@pytest.mark.parametrize("bits,bs,mbc", END_LAYOUTS)
def test_oracle_stream_cuts(bits, bs, mbc):
    check_stream_cuts(None, bits, bs, mbc)


def test_oracle_stream_cuts_rest():
    check_stream_cuts_rest(None)


@pytest.mark.parametrize("name", ARITH)
def test_oracle_arithmetic(name):
    check_arithmetic(None, name)


@pytest.mark.parametrize("name", BAD_HEADERS)
def test_oracle_bad_headers(name):
    check_bad_header(None, name)


@pytest.mark.parametrize("bits", [32, 64])
def test_oracle_optional(bits):
    check_optional(None, bits)


@pytest.mark.parametrize("bs,mbc,widen", DLBA_CASES)
def test_oracle_dlba_lengths(bs, mbc, widen):
    check_dlba(None, bs, mbc, widen)


def test_oracle_model_bites():
    """The comparison is not vacuous: one flipped payload bit changes the
    oracle's answer from that position on."""
    n = 3 * 128 + 77
    b = build_stream(np.random.default_rng(0), 64, 128, 8, n, lambda b_, m: 7)
    s = bytearray(b.stream)
    s[b.blocks[0]["body"]] ^= 0x01  # the delta of position 0
    rc, got = O.delta_decode(bytes(s), n, 64)
    assert rc == 0 and got[0] == b.expected[0] and np.all(got[1:] != b.expected[1:])
    # the last byte belongs to a group that no position below n reads
    s = bytearray(b.stream)
    s[-1] ^= 0x80
    rc, got = O.delta_decode(bytes(s), n, 64)
    assert rc == 0 and np.array_equal(got, b.expected)


# ---------------------------------------------------------------- GPU against the oracle and the model
@pytest.fixture(scope="module")
def dec():
    import pqgpu
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bits,w", SWEEP)
def test_gpu_width_sweep(dec, bits, w):
    check_width_sweep(dec, bits, w)


@pytest.mark.gpu
@pytest.mark.parametrize("bits,bs,mbc,n", LAYOUT_CASES)
def test_gpu_layouts(dec, bits, bs, mbc, n):
    check_layout(dec, bits, bs, mbc, n)


@pytest.mark.gpu
@pytest.mark.parametrize("bits,bs,mbc,w", BIG_BLOCKS)
def test_gpu_big_blocks(dec, bits, bs, mbc, w):
    check_big_blocks(dec, bits, bs, mbc, w)


@pytest.mark.gpu
@pytest.mark.parametrize("bs,sumw,vl", EDGE_CASES)
def test_gpu_stage_edge(dec, bs, sumw, vl):
    check_stage_edge(dec, bs, sumw, vl)


@pytest.mark.gpu
@pytest.mark.parametrize("large_at", [6, 0])
def test_gpu_handover(dec, large_at):
    check_handover(dec, large_at)


@pytest.mark.gpu
@pytest.mark.parametrize("form,bs", REDUNDANT, ids=_form_id)
def test_gpu_redundant_varint(dec, form, bs):
    check_redundant(dec, form, bs)


@pytest.mark.gpu
@pytest.mark.parametrize("bits,bs,mbc", END_LAYOUTS)
def test_gpu_count_ends(dec, bits, bs, mbc):
    check_count_ends(dec, bits, bs, mbc)


@pytest.mark.gpu
@pytest.mark.parametrize("bits,bs,mbc", END_LAYOUTS)
def test_gpu_stream_cuts(dec, bits, bs, mbc):
    check_stream_cuts(dec, bits, bs, mbc)


@pytest.mark.gpu
def test_gpu_stream_cuts_rest(dec):
    check_stream_cuts_rest(dec)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ARITH)
def test_gpu_arithmetic(dec, name):
    check_arithmetic(dec, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", BAD_HEADERS)
def test_gpu_bad_headers(dec, name):
    check_bad_header(dec, name)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [32, 64])
def test_gpu_optional(dec, bits):
    check_optional(dec, bits)


@pytest.mark.gpu
@pytest.mark.parametrize("bs,mbc,widen", DLBA_CASES)
def test_gpu_dlba_lengths(dec, bs, mbc, widen):
    check_dlba(dec, bs, mbc, widen)
