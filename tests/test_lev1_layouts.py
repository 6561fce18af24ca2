"""The whole-page 1-bit level decoder (pqg_lev1.h, k_page_levels_w1) against
the oracle on hand-built def streams, layout by layout: every header form on
the chain (one-, two-, three-byte and longer, non-minimal varints, bad RLE
values), payloads whose every byte looks like a header, streams that end
inside a header / a value byte / a payload, every small stream length, stream
and output misalignments, page counts that end inside runs, lanes with very
unequal work, and chains that run through positions the exit table calls
"far".  Status, level bytes and not_null of every page are compared
(parity.compare_chunk_bytes); a page the decoder does not take goes to the
exact batch decoder and is compared just the same."""
import numpy as np
import pytest

import parity as P
import pqtest_util as U
from pqgpu import abi
from test_levels import bitpack, uvarint


@pytest.fixture(scope="module")
def dec():
    import pqgpu
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


# ---- stream pieces: (bytes, values) -------------------------------------------
def bp(g, rng=None, fill=None, pad=0):
    """Bit-packed run of g groups: random payload, or every payload byte `fill`."""
    if fill is None:
        vs = (rng.random(8 * g) < 0.85).astype(np.int64)
        return uvarint(g << 1 | 1, pad) + bitpack(vs, 1), [int(x) for x in vs]
    return uvarint(g << 1 | 1, pad) + bytes([fill]) * g, [(fill >> k) & 1 for k in range(8)] * g


def rle(cnt, v, pad=0):
    return uvarint(cnt << 1, pad) + bytes([v]), [v] * cnt


def small(rng, k):
    """k short runs of the writer's shape (8-value bit-packed groups, short RLE runs)."""
    out = []
    for _ in range(k):
        out.append(bp(int(rng.integers(1, 4)), rng) if rng.random() < 0.5
                   else rle(int(rng.integers(8, 40)), int(rng.integers(0, 2))))
    return out


def cat(pieces):
    s, v = bytearray(), []
    for b, vals in pieces:
        s += b
        v += vals
    return bytes(s), v


def page(stream, count, extra=0):
    """A V1 PLAIN INT32 page of `count` slots with def stream `stream` (+ `extra` unused value bytes)."""
    vals = np.arange(count, dtype="<i4").tobytes() + b"\x5a" * extra
    return U.v1_page(vals, count, 0, defs=stream)


def check(dec, pages):
    return P.compare_chunk_bytes(b"".join(pages), dec, ptype=abi.INT32, max_def=1)


def good_page(rng):
    s, v = cat(small(rng, 6))
    return page(s, len(v))


# ---- header forms on the chain -----------------------------------------------------
BP_GROUPS = [1, 63, 64, 125, 126, 127, 128, 191, 192, 512]
RLE_COUNTS = [1, 63, 64, 8191, 8192, 32752]


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [None, 0x00, 0xFF])
def test_bit_packed_header_forms(dec, fill):
    """g across the one-/two-byte header edge (63 | 64) and the exit table's
    length byte (g + 2 = 253, 254, 255 at g = 251..253; 125..128: g + 1 or
    g + 2 around 127 / 128), each between short runs; payloads random, all
    0x00 (every position an empty RLE run) and all 0xff (a 5-byte header)."""
    rng = np.random.default_rng(11)
    pages, everything = [], []
    for g in BP_GROUPS + [250, 251, 252, 253, 254]:
        run = bp(g, rng, fill)
        s, v = cat(small(rng, 3) + [run] + small(rng, 3))
        pages.append(page(s, len(v)))
        if g <= 192:
            everything += [run] + small(rng, 1)
    s, v = cat(everything)  # all of them on one chain
    pages.append(page(s, len(v)))
    check(dec, pages)


@pytest.mark.gpu
@pytest.mark.parametrize("v", [0, 1])
def test_rle_header_forms(dec, v):
    rng = np.random.default_rng(12)
    pages = []
    for cnt in RLE_COUNTS:
        pre = [] if cnt == 32752 else small(rng, 2)
        s, vals = cat(pre + [rle(cnt, v)] + (pre and small(rng, 2)))
        pages.append(page(s, len(vals)))
    s, vals = cat([rle(c, v ^ (i & 1)) for i, c in enumerate(RLE_COUNTS[:5])] + small(rng, 2))
    pages.append(page(s, len(vals)))
    check(dec, pages)


@pytest.mark.gpu
@pytest.mark.parametrize("raw", ["8000", "8100", "828000", "82808000", "8280808000", "908000", "83808000",
                                 "8380808000", "ffffffff0f", "ffffffff7f", "808080808000"])
@pytest.mark.parametrize("where", ["before", "after"])
def test_non_minimal_varint_headers(dec, raw, where):
    """Headers with redundant continuation bytes: an empty RLE run (80 00), an
    empty bit-packed run (81 00), one RLE value in 3 / 4 / 5 bytes, 8 values,
    one bit-packed group in 4 / 5 bytes, headers past MaxInt32 and past 5
    bytes; read by the page (`before` its count is reached) or behind it."""
    rng = np.random.default_rng(13)
    hdr = bytes.fromhex(raw)
    h = 0
    for i, b in enumerate(hdr):
        h |= (b & 0x7F) << (7 * i)
    tail = bytes([0xA5]) if h & 1 else bytes([1])  # one group's payload / the RLE value
    nv = 8 * (h >> 1) if h & 1 else h >> 1
    s0, v0 = cat(small(rng, 5))
    s1, v1 = cat(small(rng, 5))
    stream = s0 + hdr + tail + s1
    if where == "before":
        count = len(v0) + (nv if nv < 1000 else 0) + len(v1)
    else:
        stream, count = s0 + s1 + hdr + tail, len(v0) + len(v1)
    check(dec, [good_page(rng), page(stream, count)])


@pytest.mark.gpu
@pytest.mark.parametrize("vb", [0, 1, 2, 255])
@pytest.mark.parametrize("cnt", [20, 100, 8191])  # a one-byte and two two-byte headers
@pytest.mark.parametrize("where", ["before", "after"])
def test_rle_value_bytes(dec, vb, cnt, where):
    rng = np.random.default_rng(14)
    s0, v0 = cat(small(rng, 7))
    s1, v1 = cat(small(rng, 7))
    run = uvarint(cnt << 1) + bytes([vb])
    if where == "before":
        stream, count = s0 + run + s1, len(v0) + cnt + len(v1)
    else:
        stream, count = s0 + s1 + run + s0, len(v0) + len(v1)
    check(dec, [good_page(rng), page(stream, count)])


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x03, 0x02, 0x80, None])
def test_payloads_that_look_like_headers(dec, fill):
    """Bit-packed payloads of one repeated byte (0x00 an empty run, 0xff a
    5-byte header, 0x03 / 0x02 valid one-byte headers, 0x80 a continuation
    byte) or random, in runs of many lengths between RLE runs."""
    rng = np.random.default_rng(15)
    pages = []
    for _ in range(4):
        pieces = []
        for g in rng.integers(1, 140, 12):
            pieces += [bp(int(g), rng, fill), rle(int(rng.integers(1, 90)), int(rng.integers(0, 2)))]
        s, v = cat(pieces)
        pages.append(page(s, len(v) - int(rng.integers(0, 9))))
    check(dec, pages)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", range(8))
def test_payload_chain_that_rejoins(dec, shift):
    """A two-byte bit-packed header (64 groups) whose last payload byte is a
    valid header (one group), with the next run's first payload byte another
    (two groups): a parse that takes the long run one byte short finds a
    chain that rejoins the true one.  At every offset from a segment's end."""
    rng = np.random.default_rng(16)
    pages = []
    for n_pad in (0, 90):  # two segment sizes
        pieces = [bp(2, rng)] * (shift % 2) + [rle(9, 1)] * (shift // 2) + small(rng, 30)
        for _ in range(12):
            b, v = bp(64, rng)
            b = b[:-1] + b"\x03"
            b2, v2 = bp(3, rng)
            b2 = b2[:1] + b"\x05" + b2[2:]
            pieces += [(b, v[:-8] + [1, 1, 0, 0, 0, 0, 0, 0]), (b2, [1, 0, 1, 0, 0, 0, 0, 0] + v2[8:])]
            pieces += small(rng, int(rng.integers(0, 3)))
        pieces += [rle(40, 0)] * n_pad
        s, v = cat(pieces)
        pages.append(page(s, len(v)))
    check(dec, pages)


# ---- stream ends --------------------------------------------------------------------
ENDS = {
    "bp_header_at_n-1": (b"\x03", 8),                    # one group, no payload
    "rle_header_no_value": (b"\x10", 8),                 # header at n - 1
    "rle_header_at_n-2": (b"\x10\x01", 8),               # complete: the stream's last two bytes
    "bp_header_at_n-2": (b"\x03\xa5", 8),
    "rle2_header_no_value": (b"\xc8\x01", 100),          # two-byte header at n - 2, value missing
    "rle2_header_at_n-3": (b"\xc8\x01\x01", 100),
    "bp2_header_at_n-3": (b"\x81\x01\xff", 512),         # 64 groups, one byte of payload
    "two_byte_header_cut": (b"\x91", 8),                 # a continuation byte at n - 1
    "three_byte_header_cut": (b"\x80\x80", 8),
    "bp_short_by_a_byte": (b"\x0b" + b"\xa5" * 4, 40),   # 5 groups, 4 bytes
    "bp_short_by_a_group": (b"\x0b" + b"\xa5" * 3, 40),
    "bp_short_by_all_but_one": (b"\x0b\xa5", 40),
    "rle_bad_value_at_n-1": (b"\x10\x02", 8),
    "garbage": (bytes(range(200, 217)), 0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("end", sorted(ENDS))
def test_stream_ends(dec, end):
    """The stream's last bytes, for pages that stop before them (trailing
    bytes: parsed by the table, never decoded), inside them, and that need
    every value they announce (or more: EOF)."""
    rng = np.random.default_rng(17)
    tail, nv = ENDS[end]
    for k in (3, 20, 150):  # S = 4 (few and most lanes used), S = 8
        s0, v0 = cat(small(rng, k))
        for count in {len(v0), len(v0) - 3, len(v0) + 1, len(v0) + max(nv - 9, 1), len(v0) + nv, len(v0) + nv + 1}:
            if count > 0:
                check(dec, [good_page(rng), page(s0 + tail, count)])


# ---- sizes and alignment -------------------------------------------------------------
def exact_length(rng, n):
    """A valid stream of exactly n bytes (n >= 2)."""
    pieces, left = [], n
    while left:
        if left == 2 or (left != 3 and rng.random() < 0.4):
            pieces.append(rle(int(rng.integers(1, 60)), int(rng.integers(0, 2))))
            left -= 2
        else:
            g = int(rng.integers(1, min(left - 1, 63) + 1))
            if left - 1 - g == 1:
                g = g - 1 if g > 1 else g + 1
            pieces.append(bp(g, rng))
            left -= 1 + g
    s, v = cat(pieces)
    assert len(s) == n
    return s, v


@pytest.mark.gpu
@pytest.mark.parametrize("lengths", [range(2, 71), list(range(250, 266)) + list(range(508, 518)),
                                     list(range(4086, 4101))], ids=["2-70", "250-265,508-517", "4086-4100"])
def test_stream_lengths(dec, lengths):
    """Every stream length of up to 70 bytes, every residue of 4 around the
    segment sizes' steps (S = 4 | 8 at 256, 8 | 12 at 512) and around the
    longest stream the whole-page decoder takes (4096)."""
    rng = np.random.default_rng(18)
    pages = []
    for n in lengths:
        s, v = exact_length(rng, n)
        if len(v) > 32000:  # past 4096 bytes the batch decoder takes the page
            v = v[:32000]
        pages.append(page(s, len(v) - int(rng.integers(0, 8)) if len(v) > 8 else len(v)))
    check(dec, pages)


@pytest.mark.gpu
def test_one_byte_streams(dec):
    rng = np.random.default_rng(19)
    for b in (0x00, 0x01, 0x02, 0x03, 0x10, 0x80, 0xFF):
        check(dec, [good_page(rng), page(bytes([b]), 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("mis", range(16))
def test_stream_and_output_misalignment(dec, mis):
    """The def stream at every offset from a 16-byte boundary (unused value
    bytes behind the page before it) and the page's first level byte at every
    offset (pages of 1..16 slots before it)."""
    rng = np.random.default_rng(20 + mis)
    s, v = cat(small(rng, 40) + [bp(70, rng)] + small(rng, 40))
    lead, lv = cat([rle(50, 1)])
    for out_mis in (mis, (5 * mis + 3) % 16):
        first = page(lead, out_mis + 1, extra=mis)
        check(dec, [first, page(s, len(v) - mis), page(s, 7)])


@pytest.mark.gpu
def test_counts(dec):
    """Counts that are no multiple of 8, end inside a bit-packed run, inside
    an RLE run, at a run's last value, and a count of 1."""
    rng = np.random.default_rng(21)
    pieces = small(rng, 10) + [bp(40, rng), rle(300, 1), bp(3, rng), rle(5, 0)]
    s, v = cat(pieces)
    base = len(cat(pieces[:10])[1])
    pages = [page(s, c) for c in (1, 2, 7, 9, base, base + 1, base + 37, base + 319, base + 320, base + 321,
                                  base + 320 + 299, base + 320 + 300, base + 320 + 301, len(v) - 1, len(v))]
    check(dec, pages)
    for first in (bp(1, rng), rle(1, 1), rle(1, 0), rle(9000, 1)):
        check(dec, [page(cat([first])[0], 1)])


# ---- emission balance -----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("long_run", ["rle1000", "bp125", "rle1000_first", "bp125_last"])
def test_one_long_run_among_short_ones(dec, long_run):
    """One lane's segment holds a 1 000-value run, its neighbours many 8-value runs."""
    rng = np.random.default_rng(22)
    shorts = lambda k: [bp(1, rng) if rng.random() < 0.7 else rle(8, int(rng.integers(0, 2))) for _ in range(k)]
    big = rle(1000, 1) if long_run.startswith("rle") else bp(125, rng)
    if long_run.endswith("first"):
        pieces = [big] + shorts(300)
    elif long_run.endswith("last"):
        pieces = shorts(300) + [big]
    else:
        pieces = shorts(150) + [big] + shorts(150)
    s, v = cat(pieces)
    check(dec, [page(s, len(v)), page(s, len(v) - 1001)])


@pytest.mark.gpu
def test_single_run_pages(dec):
    """A page that is one RLE run (most lanes place nothing; their first
    value lies past the count), of zeros and of ones, short and long; one
    bit-packed run."""
    rng = np.random.default_rng(23)
    pages = []
    for cnt, v in ((5000, 0), (5000, 1), (32752, 0), (32752, 1), (3, 1), (64, 0)):
        s, vals = cat([rle(cnt, v)])
        pages += [page(s, cnt), page(s, max(1, cnt - 13))]
    s, vals = cat([bp(500, rng)])
    pages += [page(s, 4000), page(s, 3999)]
    # a long run first, then trailing runs the count never reaches (lanes whose first value is past it)
    s, vals = cat([rle(20000, 1)] + small(rng, 200))
    pages += [page(s, 20000), page(s, 19999), page(s, 20001)]
    check(dec, pages)


@pytest.mark.gpu
@pytest.mark.parametrize("runs", [1, 2, 10, 63, 64, 65, 130, 600])
def test_run_counts(dec, runs):
    rng = np.random.default_rng(24 + runs)
    s, v = cat(small(rng, runs))
    check(dec, [page(s, len(v)), page(s, max(1, len(v) - 5))])


# ---- far links ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rle3", "bp_long", "mixed", "pad"])
def test_far_positions_on_the_chain(dec, kind):
    """Chains through positions the exit table does not settle, in several
    consecutive segments: three-byte RLE headers (counts >= 8192), bit-packed
    runs of 200 and more groups (252+: the length does not fit the table's
    byte), and padded one-value headers."""
    rng = np.random.default_rng(25)
    if kind == "rle3":
        pieces = [rle(8192 + i, i & 1) for i in range(3)] + small(rng, 4)
        pieces = small(rng, 2) + pieces
    elif kind == "bp_long":
        pieces = [bp(g, rng) for g in (200, 252, 300, 251, 260, 400, 253)]
    elif kind == "mixed":
        pieces = []
        for g in (300, 260, 280):
            pieces += [bp(g, rng), rle(8200, 1)] + small(rng, 1)
    else:
        pieces = []
        for i in range(40):
            pieces += [rle(1 + i, i & 1, pad=1 + i % 3), bp(1 + i % 5, rng, pad=i % 3)]
    s, v = cat(pieces)
    assert len(v) <= 32752
    check(dec, [good_page(rng), page(s, len(v)), page(s, len(v) - 77), good_page(rng)])
