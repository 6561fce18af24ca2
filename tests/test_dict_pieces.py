"""Piece seams of the dictionary kernels (k_dict4 / k_dict4_big, pqg_dict.hip)
against the oracle.  A wave decodes a page piece by piece -- the leading blocks
(512 values each) whose runs and bit-packed payload lie in one round of loads:
128 run entries and a 4096-byte payload window from a 16-byte aligned address
-- and loads the next piece while it stores the current one.  The streams here
put what can go wrong at the seams: the layout of the file writer (bit-packed
runs of exactly 64 groups: one block each up to 15 bits, two-run blocks of
400-496 values above, where a block's payload is capped) at every dictionary path, pieces
that end on the run table or hold no payload, streams that end inside a window
(the zero padding of short reads must hold on a window loaded ahead), keys
past the dictionary on either side of a seam, and a batch whose queue items
mix jobs and dictionaries.

The geometry helpers below restate the walker's block rule and the piece rule
to *place* the cases (they assume what hipMalloc gives: chunk buffers aligned
to at least 16 bytes), and the CPU tests assert the placement; the
expected values come from the oracle alone, and the CPU tests pin the oracle's
counts and statuses so that no GPU case passes on an input both sides reject."""
import numpy as np
import pytest

import parity as P
import pqtest_util as U
from oracle import pyoracle as O
from pqgpu import abi
from test_levels import uvarint

WINDOW = 4096       # payload bytes of a piece (kPPay)
BLOCK = 512         # values of a block (kHBlock)
DICT_INDEX = abi.STATUS_CODES["DICT_INDEX"]


def bitpack(vals, w):
    """LSB-first w-bit fields (test_levels.bitpack, vectorised)."""
    v = np.asarray(vals, dtype=np.uint64)
    bits = ((v[:, None] >> np.arange(w, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8).ravel()
    return np.packbits(bits, bitorder="little").tobytes()


def dict_page(rng, dcount):
    ents = rng.integers(-2**31, 2**31 - 1, dcount, dtype=np.int64).astype("<i4").tobytes()
    return U.page_header_dict(len(ents), len(ents), dcount) + ents


def bp_runs(keys, w, groups=64, pad=()):
    """`keys` as bit-packed runs of `groups` groups (the last one shorter);
    pad[i]: redundant header bytes of run i.  -> (stream, [(payload offset, bytes)] per run)"""
    out, lay = bytearray(), []
    per = 8 * groups
    for i, a in enumerate(range(0, len(keys), per)):
        ks = list(keys[a:a + per])
        ks += [0] * (-len(ks) % 8)
        out += uvarint((len(ks) // 8) << 1 | 1, pad=pad[i] if i < len(pad) else 0)
        lay.append((len(out), len(ks) // 8 * w))
        out += bitpack(ks, w)
    return bytes(out), lay


def data_page(stream, w, n, defs=None):
    return U.v1_page(bytes([w]) + stream, n, 8, defs=defs)


def windows(blocks):
    """Pieces of payload blocks [(address, bytes)]: [(window start, first block, end block)]."""
    out, i = [], 0
    while i < len(blocks):
        plo = blocks[i][0] & ~15
        j = i
        while j < len(blocks) and j - i < 63 and blocks[j][0] + blocks[j][1] <= plo + WINDOW:
            j += 1
        assert j > i
        out.append((plo, i, j))
        i = j
    return out


def nullable(rng, nn):
    """Def levels of a page of nn non-null values -> (values in the page, level bytes)."""
    d = np.ones(nn + int(rng.integers(0, nn // 8 + 2)), dtype=np.int64)
    d[rng.choice(len(d), len(d) - nn, replace=False)] = 0
    from test_levels import bitpack as bp1
    return len(d), uvarint(((len(d) + 7) // 8) << 1 | 1) + bp1(d, 1)


# ---------------------------------------------------------------- generators
WRITER_DICTS = {1: (4096, 4097), 8: (4096, 4097, 79872, 79873), 12: (4096, 4097, 79872, 79873),
                13: (4096, 4097, 79872, 79873), 16: (4096, 4097, 79872, 79873),
                20: (4096, 4097, 79872, 79873, 1 << 20), 32: (4096, 4097, 79872, 79873)}


def writer_chunk(rng, w, dcount, pages=3, lo=2000, hi=7000):
    """The file writer's layout: every run 64 groups.  -> (chunk, non-null values)"""
    parts, total = [dict_page(rng, dcount)], 0
    for _ in range(pages):
        nn = int(rng.integers(lo, hi + 1))
        keys = rng.integers(0, min(dcount, 1 << w), nn)
        n, defs = nullable(rng, nn)
        parts.append(data_page(bp_runs(keys, w)[0], w, n, defs))
        total += nn
    return b"".join(parts), total


def rle_runs_chunk(rng, w=9, dcount=400):
    """300 RLE runs of 1-3 values (three run tables' worth, multi-run blocks), then two bit-packed runs."""
    rb = (w + 7) // 8
    s, nn = bytearray(), 0
    for _ in range(300):
        c = int(rng.integers(1, 4))
        s += uvarint(c << 1) + int(rng.integers(0, dcount)).to_bytes(rb, "little")
        nn += c
    s += bp_runs(rng.integers(0, dcount, 1024), w)[0]
    nn += 1000
    return dict_page(rng, dcount) + data_page(bytes(s), w, nn) * 2, 2 * nn


def long_rle_chunk(rng, w=14, dcount=9000):
    """One RLE run of 40 000 values (78 blocks without payload: more than a
    piece holds), then bit-packed runs: the window moves to the first payload."""
    s = uvarint(40000 << 1) + int(rng.integers(0, dcount)).to_bytes(2, "little")
    s += bp_runs(rng.integers(0, dcount, 6 * BLOCK + 100), w)[0]
    nn = 40000 + 6 * BLOCK + 77
    return dict_page(rng, dcount) + data_page(s, w, nn) + data_page(s, w, nn - 1), 2 * nn - 1


def header_at_window_end(rng, w=16, dcount=60000):
    """Redundant header bytes that end within the last 16 bytes of the first
    window (which starts at the first block's payload, whatever the blocks
    are).  -> (chunk, values, geometry)"""
    head = dict_page(rng, dcount)
    for g3 in range(40, 64):
        for pad in (1, 2, 3, 4, 5):
            keys = rng.integers(0, dcount, 8 * (3 * 64 + g3) + 3 * BLOCK)
            a = keys[:8 * (3 * 64 + g3)]
            s1, lay1 = bp_runs(a[:3 * BLOCK], w)
            s2, lay2 = bp_runs(a[3 * BLOCK:], w, groups=g3)
            s3, lay3 = bp_runs(keys[len(a):], w, pad=(pad,))
            stream = s1 + s2 + s3
            nn = len(keys) - 5
            page = data_page(stream, w, nn)
            base = len(head) + len(page) - len(stream)  # chunk offset of stream byte 0
            hdr_end = base + len(s1) + len(s2) + 2 + pad  # end of the padded header
            wend = ((base + lay1[0][0]) & ~15) + WINDOW
            if wend - 16 < hdr_end <= wend:
                return head + page + data_page(stream, w, nn - 9), 2 * nn - 9, (hdr_end, wend)
    raise AssertionError("no layout puts the header at the window's end")


# Layouts whose blocks are single runs on the device (asserted by the CPU
# tests through device_blocks): (bit width, groups per run, redundant header
# bytes of every run, dictionary entries).  Up to 15 bits a 64-group run is one
# 512-value block.  At 20 bits a block's payload is capped at 1008 bytes: a
# 50-group run (1000 bytes) behind a 7-byte header leaves no room for a value
# of the next run, so each run is one 400-value block -- the only way to reach
# the straight-line block path with a global dictionary.  "global64" is the
# writer's own 64-group layout at 20 bits: blocks of ~402 values over two runs.
LAYOUTS = {"lds": (12, 64, 0, 4096), "lds9": (9, 64, 0, 512), "prefix": (15, 64, 0, 32768), "global": (20, 50, 6, 1 << 20),
           "global64": (20, 64, 0, 1 << 20)}
CUTS = (("lds9", "first16"), ("lds", "window_end"), ("lds", "third"), ("prefix", "window_end"), ("prefix", "third"),
        ("global", "window_end"), ("global", "third"))


def device_blocks(lay, w, count):
    """The walker's blocks (k_hybrid_walk, pqg_levels.hip) of a stream of
    bit-packed runs `lay` = [(payload offset, bytes)] of which the page takes
    `count` values: a block closes at 512 values, at 64 runs, or where not one
    more value ends within 1008 bytes of its first payload byte.
    -> [(first value, values, payload offset, payload bytes, runs)]"""
    out = []
    bv0, bn, blo, bhi, produced = 0, 0, None, 0, 0

    def close(v):
        if bn:
            out.append((bv0, v - bv0, blo, bhi - blo, bn))

    for src, nbytes in lay:
        if produced >= count:
            break
        take = min((nbytes + w - 1) // w * 8, count - produced)  # a partly present last group counts (zero padded)
        rend, v = produced + take, produced
        while v < rend:
            if bn == 64 or v >= bv0 + BLOCK:
                close(v)
                bv0, bn, blo, bhi = v, 0, None, 0
            pe = min(rend, bv0 + BLOCK)
            rbit = src * 8
            b0 = (rbit + (v - produced) * w) >> 3
            org = b0 if blo is None else min(blo, b0)
            lim = (org + 1008) * 8
            fit = (lim - rbit) // w if lim > rbit else 0
            if produced + fit <= v:
                close(v)
                bv0, bn, blo, bhi = v, 0, None, 0
                continue
            pe = min(pe, produced + fit)
            blo, bhi = org, max(bhi, (rbit + (pe - produced) * w + 7) >> 3)
            bn += 1
            v = pe
        produced = rend
    close(produced)
    return out


def device_pieces(blocks):
    """Pieces of device blocks at their addresses: [(window start, first block, end block)]."""
    return windows([(b[2], b[3]) for b in blocks])


def laid_out(kind, keys, extra_pad=0):
    """Stream of `keys` in the kind's layout -> (stream, [(payload offset, bytes)], values per run)"""
    w, groups, pad, _ = LAYOUTS[kind]
    nruns = (len(keys) + 8 * groups - 1) // (8 * groups)
    stream, lay = bp_runs(keys, w, groups=groups, pad=[pad + extra_pad] + [pad] * (nruns - 1))
    return stream, lay, 8 * groups


def cut_chunk(rng, kind, where):
    """A page whose stream ends inside a bit-packed run, its last group partly
    present (read zero padded), followed by a whole page, so the bytes behind
    the cut are the next page's header.  where: "first16" (the cut within the
    first 16 bytes of the device's second window: kind "lds9"), "window_end" (exactly on the
    second window's end, inside the third piece) or "third" (mid third piece).
    Every key of w bits is inside the dictionary.  -> (chunk, values, geometry)"""
    w, groups, pad, dcount = LAYOUTS[kind]
    head = dict_page(rng, dcount)
    if where == "first16":
        return cut_first16(rng, kind, head)
    for extra in range(0, 6):
        keys = rng.integers(0, 1 << w, 24 * BLOCK)
        stream, lay, per = laid_out(kind, keys, extra)
        base = len(head) + len(U.page_header_v1(0, 0, 0, 8)) + 1  # refined below
        for _ in range(3):  # the page header's length depends on the sizes in it
            blocks = device_blocks([(base + o, b) for o, b in lay], w, len(keys))
            assert all(b[4] == 1 and b[1] == per for b in blocks[:-1]), "one run per block"
            (p1, b1, e1), (p2, b2, e2) = device_pieces(blocks)[1:3]
            if where == "first16":
                blk, cut = b1, blocks[b1][2] + 1
                ok = p1 < cut < p1 + 16
            elif where == "window_end":
                blk, cut = b2, p1 + WINDOW
                ok = blocks[b2][2] < cut < blocks[b2][2] + blocks[b2][3]
            else:
                blk, cut = b2 + 1, blocks[b2 + 1][2] + 5 * w + 3
                ok = True
            inside = cut - blocks[blk][2]
            ok = ok and inside % w != 0
            nn = blk * per + 8 * (inside // w + 1)
            page = data_page(stream[:cut - base], w, nn)
            nbase = len(head) + len(page) - (cut - base)
            if nbase == base:
                break
            base = nbase
        else:
            continue
        if ok:
            # what the device sees: the cut stream's own blocks and windows
            cb = device_blocks([(base + o, min(b, cut - base - o)) for o, b in lay if base + o < cut], w, nn)
            tail = data_page(laid_out(kind, keys[:3000])[0], w, 2990)
            assert tail[0] != 0
            return head + page + tail, nn + 2990, dict(cut=cut, windows=[p[0] for p in device_pieces(cb)],
                                                         group_bytes=inside % w, nn=nn, per=per, blk=blk)
    raise AssertionError("no layout for %s/%s" % (kind, where))


def cut_first16(rng, kind, head):
    """The cut one byte into a block that starts at or past the first window's
    end (a block that ends inside the window joins the first piece, however
    short).  Only a width whose runs nearly tile the window gets there with
    header bytes alone: 9 bits, 7 runs of 576 bytes, their headers padded until
    the 8th run's payload starts in the 16 bytes from the window's end on."""
    w, groups, _, dcount = LAYOUTS[kind]
    per = 8 * groups
    keys = rng.integers(0, 1 << w, 8 * per)
    for full in (7, 6, 8):
        for e in range(0, 8):
            for f in range(0, 8):
                s1, lay1 = bp_runs(keys[:full * per], w, groups=groups, pad=[f] + [e] * (full - 1))
                s3, lay3 = bp_runs(keys[full * per:full * per + 8], w, groups=1, pad=[e])
                cutlen = len(s1) + lay3[0][0] + 1  # one byte of the last group
                nn = full * per + 8
                page = data_page((s1 + s3)[:cutlen], w, nn)
                base = len(head) + len(page) - cutlen
                lay = [(base + o, b) for o, b in lay1] + [(base + len(s1) + lay3[0][0], 1)]
                blocks = device_blocks(lay, w, nn)
                win = [p[0] for p in device_pieces(blocks)]
                cut = base + cutlen
                if len(win) == 2 and 0 < cut - win[1] < 16 and all(b[4] == 1 for b in blocks):
                    tail = data_page(laid_out(kind, keys[:3000])[0], w, 2990)
                    assert tail[0] != 0
                    return head + page + tail, nn + 2990, dict(cut=cut, windows=win, group_bytes=1, nn=nn, per=per,
                                                                 blk=full)
    raise AssertionError("no layout for %s/first16" % kind)


BAD = {"lds": 4000, "prefix": 30000, "global": 1000000, "global64": 1000000}


def bad_key_chunk(rng, kind, side):
    """One key >= the dictionary's size in the last block of the device's first
    piece (side 0) or the first block of its second (side 1), in the middle
    page of three.  -> (chunk, geometry of the middle page)"""
    w = LAYOUTS[kind][0]
    dcount = BAD[kind]
    head = dict_page(rng, dcount)
    nn = 12 * BLOCK + 40
    pages, geo = [], None
    for p in range(3):
        keys = rng.integers(0, dcount, nn)
        stream, lay, per = laid_out(kind, keys)
        if p == 1:
            base = len(head) + sum(map(len, pages)) + len(data_page(stream, w, nn)) - len(stream)
            blocks = device_blocks([(base + o, b) for o, b in lay], w, nn)
            pieces = device_pieces(blocks)
            e0 = pieces[0][2]
            at = blocks[e0 - 1][0] + 100 if side == 0 else blocks[e0][0] + 7
            keys[at] = (1 << w) - 3
            stream = laid_out(kind, keys)[0]
            geo = dict(at=at, blocks=blocks, pieces=pieces)
        pages.append(data_page(stream, w, nn))
    return head + b"".join(pages), geo


def batch_chunks(rng):
    """Six small chunks for one decode_jobs call: (chunk, non-null values)."""
    out = []
    for w, dcount in ((4, 16), (12, 4096), (13, 4097), (15, 30000), (17, 79873)):
        out.append(writer_chunk(rng, w, dcount, pages=int(rng.integers(1, 4)), lo=200, hi=3000))
    parts, total = [dict_page(rng, 5)], 0
    for _ in range(2):  # zero-width indices: every value is entry 0
        nn = int(rng.integers(200, 3001))
        n, defs = nullable(rng, nn)
        parts.append(data_page(b"", 0, n, defs))
        total += nn
    out.insert(3, (b"".join(parts), total))
    return out


# ---------------------------------------------------------------- CPU: the generators mean what they say
def oracle(chunk, max_def=0):
    keep = []
    return O.decode_chunk(U.chunk_job(chunk, abi.INT32, max_def=max_def, keep=keep)[0], page_cap=16)


def test_generators_decode_on_the_oracle():
    rng = np.random.default_rng(11)
    for w in (1, 13, 20):
        c, nn = writer_chunk(rng, w, WRITER_DICTS[w][1])
        e = oracle(c, 1)
        assert (e.status, e.num_values) == (0, nn)
    for gen in (rle_runs_chunk, long_rle_chunk):
        c, nn = gen(rng)
        e = oracle(c)
        assert (e.status, e.num_values) == (0, nn)
    c, nn, (hdr_end, wend) = header_at_window_end(rng)
    e = oracle(c)
    assert (e.status, e.num_values) == (0, nn) and wend - 16 < hdr_end <= wend
    for c, nn in batch_chunks(rng):
        e = oracle(c, 1)
        assert (e.status, e.num_values) == (0, nn)


def test_cut_streams_decode_zero_padded_on_the_oracle():
    rng = np.random.default_rng(12)
    for kind, where in CUTS:
        c, nn, g = cut_chunk(rng, kind, where)
        e = oracle(c)
        assert (e.status, e.num_values) == (0, nn), (kind, where)
        win = g["windows"]  # of the cut stream, from the walker's block rule
        assert 0 < g["group_bytes"] < LAYOUTS[kind][0], "the last group is partly present"
        if where == "first16":
            assert len(win) == 2 and 0 < g["cut"] - win[1] < 16
        elif where == "window_end":
            assert len(win) == 3 and g["cut"] == win[1] + WINDOW
        else:
            assert len(win) == 3 and win[2] + 16 < g["cut"] < win[2] + WINDOW


def test_bad_keys_fail_on_the_oracle():
    rng = np.random.default_rng(13)
    for kind in BAD:
        for side in (0, 1):
            c, g = bad_key_chunk(rng, kind, side)
            e = oracle(c)
            assert e.status == DICT_INDEX and e.error_page == 2, (kind, side, e.status, e.error_page)
            blocks, (_, b0, e0), at = g["blocks"], g["pieces"][0], g["at"]
            assert b0 == 0 and e0 >= 3 and len(g["pieces"]) >= 2
            blk = e0 - 1 if side == 0 else e0
            assert blocks[blk][0] <= at < blocks[blk][0] + blocks[blk][1], (kind, side)
            if kind == "global64":
                assert blocks[1][4] == 2 and blocks[e0 - 1][4] == 2, "the writer's runs straddle the blocks"
            else:  # the straight-line block path: the pieces open with single-run blocks
                assert all(b[4] == 1 for b in blocks), kind


def test_device_blocks_of_the_writer_layout():
    """The block rule as restated here gives what the kernels' counters show:
    400-403 values per block at 20 bits, 4 blocks to a piece."""
    lay = bp_runs(np.zeros(16 * BLOCK, dtype=np.int64), 20)[1]
    blocks = device_blocks([(96 + o, b) for o, b in lay], 20, 16 * BLOCK)
    assert [b[0] for b in blocks[:4]] == [0, 403, 805, 1207]
    assert device_pieces(blocks)[0][1:] == (0, 4)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dec():
    import pqgpu
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w", sorted(WRITER_DICTS))
def test_writer_layout_pieces(dec, w):
    """Bit-packed runs of 64 groups, 3 pages of 2 000-7 000 non-null values, a
    partial last block, on each side of every dictionary path switch."""
    rng = np.random.default_rng(100 + w)
    for dcount in WRITER_DICTS[w]:
        chunk, nn = writer_chunk(rng, w, dcount)
        exp, _ = P.compare_chunk_bytes(chunk, dec, ptype=abi.INT32, max_def=1)
        assert (exp.status, exp.num_values) == (0, nn)


@pytest.mark.gpu
def test_pieces_bounded_by_runs_and_blocks(dec):
    rng = np.random.default_rng(200)
    for gen in (rle_runs_chunk, long_rle_chunk):
        chunk, nn = gen(rng)
        exp, _ = P.compare_chunk_bytes(chunk, dec, ptype=abi.INT32)
        assert (exp.status, exp.num_values) == (0, nn)
    chunk, nn, _ = header_at_window_end(rng)
    exp, _ = P.compare_chunk_bytes(chunk, dec, ptype=abi.INT32)
    assert (exp.status, exp.num_values) == (0, nn)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,where", CUTS)
def test_stream_ends_at_piece_seams(dec, kind, where):
    """The values of the partly present last group are the oracle's (zero past
    the stream's end), whatever follows the stream in memory."""
    chunk, nn, _ = cut_chunk(np.random.default_rng(300), kind, where)
    exp, _ = P.compare_chunk_bytes(chunk, dec, ptype=abi.INT32)
    assert (exp.status, exp.num_values) == (0, nn)


@pytest.mark.gpu
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("kind", sorted(BAD))
def test_bad_keys_at_piece_seams(dec, kind, side):
    exp, got = P.compare_chunk_bytes(bad_key_chunk(np.random.default_rng(400), kind, side)[0], dec, ptype=abi.INT32)
    assert exp.status == DICT_INDEX and (got.status, got.error_page) == (exp.status, exp.error_page)


@pytest.mark.gpu
def test_mixed_batch(dec):
    """Six small chunks in one call: 4-wave and 8-wave items hold pages of
    several jobs, and the LDS dictionary changes inside an item."""
    chunks = batch_chunks(np.random.default_rng(500))
    keep, jobs, exps, devs = [], [], [], []
    try:
        for chunk, nn in chunks:
            job, buf = U.chunk_job(chunk, abi.INT32, max_def=1, keep=keep)
            exps.append(O.decode_chunk(job))
            assert (exps[-1].status, exps[-1].num_values) == (0, nn)
            devs.append(dec.upload(buf))
            job.data = devs[-1]
            jobs.append(job)
        res = dec.decode_jobs(jobs)
        for i, (e, r) in enumerate(zip(exps, res)):
            P.compare_chunk(e, dec.download(r, i), "chunk %d" % i)
    finally:
        for d in devs:
            dec.free(d)
