"""K1 (pqg_scan.hip) on page headers no test writer emits: long headers (Statistics), headers
that miss the candidate scan's shape, headers past the limits of the bounded candidate parse,
damaged long headers, odd checksum fields — built by hdr_util — and pyarrow's own headers.

Every chunk goes through two decoders, the default one (prewalk, stride walk, candidate scan,
serial walk) and one without the stride walk (PQG_STRIDE=0), and every result is the oracle's:
status, error page, levels, values (parity.compare_chunk*) and each page record (check_pages).
Where the code makes the route determinate, debug_job(0)[0] (`serial_walk`: 0 candidate scan,
1 serial walk, 2 prewalk / stride walk) is asserted, so that a test takes the route it names.

A decoder remembers the chunks (by address and size) that its prewalk did not settle and skips the
prewalk, and with it the stride walk, for them.  So every test that asserts the stride walk's
route (2), or that a chunk leaves it, runs on a default decoder of its own (`dec1`), whose memory
is empty: neither the order of the tests nor the addresses the allocator returns bear on a route.
"""
import io
import os
import zlib

import numpy as np
import pytest

import hdr_util as H
import parity as P
from oracle import pyoracle as O
import pqgpu
import pqtest_util as U
from pqgpu import abi

pytestmark = pytest.mark.gpu

WIN = 160        # candidate window: 16 * kCandWin bytes from the header's granule
STRIDE_MAX = 64  # the stride walk's longest header
CRC = abi.STATUS_CODES["CRC"]


@pytest.fixture(scope="module")
def dec():
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


@pytest.fixture
def dec1():
    """A default decoder made for one test: it remembers no chunk (see the module's docstring)."""
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dec_scan():
    """A decoder without the K1 stride walk (PQG_STRIDE=0, read at context
    creation): chunks of equal PLAIN pages take the candidate scan."""
    old = os.environ.get("PQG_STRIDE")
    os.environ["PQG_STRIDE"] = "0"
    try:
        d = pqgpu.GpuDecoder(0)
    finally:
        if old is None:
            os.environ.pop("PQG_STRIDE", None)
        else:
            os.environ["PQG_STRIDE"] = old
    yield d
    d.close()


# ---------------------------------------------------------------- helpers
def vals(n, start=0):
    """n distinct int32 values none of whose bytes is 0x15 (no header candidates in a payload)."""
    i = np.arange(start, start + n, dtype=np.int64)
    v = 0x20202020 | (i & 0xF) | ((i >> 4) & 0xF) << 8 | ((i >> 8) & 0xF) << 16 | ((i >> 12) & 0xF) << 24
    return v.astype(np.int32)


def rle_ones(n):
    return U.uvarint(n << 1) + b"\x01"


def snappy_literals(d):
    out = bytearray(U.uvarint(len(d)))
    for i in range(0, len(d), 60):
        part = d[i:i + 60]
        out.append((len(part) - 1) << 2)
        out += part
    return bytes(out)


class Variant:
    """How the data pages of a chunk are written: plain (V1, REQUIRED), optional (V1, def levels),
    v2 (OPTIONAL, def levels), snappy (V1), dict (a dictionary page first, RLE_DICTIONARY pages)."""

    def __init__(self, name):
        self.name = name
        self.kw = dict(ptype=abi.INT32)
        if name in ("optional", "v2"):
            self.kw["max_def"] = 1
        if name == "snappy":
            self.kw["codec"] = 1

    def page(self, spec, n, start):
        """[spec with the page's fields, payload, uncompressed size]"""
        raw = vals(n, start).tobytes()
        if self.name == "optional":
            lv = rle_ones(n)
            raw = U.u32(len(lv)) + lv + raw
        if self.name == "v2":
            lv = rle_ones(n)
            spec = spec.with_(kind=2, nvals=n, def_len=len(lv))
            return [spec, lv + raw, len(lv) + len(raw)]
        if self.name == "dict":
            raw = b"\x04" + b"".join(bytes([2, (start + i) % 16]) for i in range(n))
            return [spec.with_(nvals=n, enc=8), raw, len(raw)]
        if self.name == "snappy":
            return [spec.with_(nvals=n), snappy_literals(raw), len(raw)]
        return [spec.with_(nvals=n), raw, len(raw)]

    def first(self):
        if self.name != "dict":
            return []
        raw = vals(16, 7000).tobytes()
        return [[H.Hdr("dict", nvals=16, enc=0), raw, len(raw)]]


PLAIN = Variant("plain")


def build(specs, rows, variant=PLAIN, last_rows=None):
    """Chunk of one page per spec, `rows` values each (the last page `last_rows`)."""
    pages = variant.first()
    for k, spec in enumerate(specs):
        n = last_rows if (last_rows is not None and k == len(specs) - 1) else rows
        pages.append(variant.page(spec, n, k * rows))
    data, at = H.chunk(pages)
    return data, at


def check_pages(exp, got):
    """Each page record of the GPU (dec.pages) against the oracle's, for every page both report
    (all of them; after a read-phase error, the pages up to the failing one): header_offset,
    payload_offset, page_type, encoding, num_values, compressed_size, uncompressed_size and status
    on every page; def_len and rep_len on DATA_PAGE_V2 pages and the level encodings on DATA_PAGE
    pages whose header parsed (the oracle fills them there only; the GPU record also carries
    whatever the other page-header struct of the header held).  The GPU records the encoding its
    decoder runs: PLAIN_DICTIONARY (2) of a data page reads RLE_DICTIONARY (8)."""
    assert got.pages is not None and len(got.pages) == len(exp.pages), (len(got.pages), len(exp.pages))
    for k, (g, e) in enumerate(zip(got.pages, exp.pages)):
        enc = 8 if (e.encoding == 2 and e.page_type in (0, 3)) else e.encoding
        a = (g.header_offset, g.payload_offset, g.page_type, g.encoding, g.num_values, g.compressed_size,
             g.uncompressed_size)
        b = (e.header_offset, e.payload_offset, e.page_type, enc, e.num_values, e.compressed_size,
             e.uncompressed_size)
        assert a == b, "page %d: gpu %s oracle %s" % (k, a, b)
        if exp.status != 0 and k == len(exp.pages) - 1:
            assert g.status == e.status, (k, g.status, e.status)
        if e.status == 0 and e.page_type == 3:
            assert (g.def_len, g.rep_len) == (e.def_len, e.rep_len), k
        if e.status == 0 and e.page_type == 0:
            assert (g.def_encoding, g.rep_encoding) == (e.def_encoding, e.rep_encoding), k


PAGE_CAP = 2048  # page records fetched per chunk (the largest chunk here has 1031)


def run(d, data, offset=0, walk=None, exp=None, **kw):
    """One chunk through one decoder: the oracle's result (`exp`: from an earlier run of the same
    chunk), page by page; the route if given (a value or a tuple of values)."""
    try:
        exp, got = P.compare_chunk_bytes(data, d, offset=offset, exp=exp, page_cap=PAGE_CAP, **(kw or PLAIN.kw))
    except pqgpu.PqgError as err:
        if err.code == abi.STATUS_CODES["HIP"]:  # a failed launch or copy: nothing more may run on this GPU
            pytest.exit("decode failed: %s" % err, returncode=3)
        raise
    check_pages(exp, got)
    w = d.debug_job(0)[0]
    if walk is not None:
        assert w in (walk if isinstance(walk, tuple) else (walk,)), "serial_walk %d, expected %s" % (w, walk)
    return exp, got


def both(dec, dec_scan, data, walk_scan=None, walk_default=None, offsets=(0,), **kw):
    exp = None
    for off in offsets:
        exp, _ = run(dec_scan, data, off, walk_scan, exp, **kw)
        run(dec, data, off, walk_default, exp, **kw)
    return exp


# ---------------------------------------------------------------- length edges
LENGTHS = list(range(56, 71)) + list(range(140, 166)) + list(range(1016, 1033)) + list(range(2040, 2057))


@pytest.mark.parametrize("n", LENGTHS)
def test_header_length_edges(request, dec_scan, n):
    """12 equal pages whose headers are exactly n bytes, the chunk at each of 16 byte offsets of the
    uploaded buffer.  The payload length goes with n so that the page length mod 16, and with it
    the alignment of the 12 header starts, varies too.  Routes: without the stride walk the
    candidate scan settles headers that end inside the window from any alignment (<= 144 bytes)
    and hands longer ones than the window to the serial walk; the stride walk takes equal pages
    with headers of at most 64 bytes."""
    dec = request.getfixturevalue("dec1" if n <= STRIDE_MAX else "dec")
    rows = 7 + n % 13
    spec, hb = H.pad_to(n, 4 * rows, 4 * rows, H.Hdr(1, nvals=rows))
    assert len(hb) == n
    data, at = build([spec] * 12, rows)
    assert [p - h for h, p in at] == [n] * 12
    scan = 0 if n <= WIN - 16 else 1 if n > WIN else (0, 1)
    default = 2 if n <= STRIDE_MAX else scan
    both(dec, dec_scan, data, scan, default, offsets=range(16))


@pytest.mark.parametrize("n", [56, 61, 64, 65, 150, 1030])
def test_header_length_edges_v2(request, dec_scan, n):
    dec = request.getfixturevalue("dec1" if n <= STRIDE_MAX else "dec")
    rows = 9
    v = Variant("v2")
    lv = rle_ones(rows)
    base = H.Hdr(2, nvals=rows, def_len=len(lv))
    spec, hb = H.pad_to(n, len(lv) + 4 * rows, len(lv) + 4 * rows, base)
    data, at = build([spec] * 12, rows, v)
    assert [p - h for h, p in at] == [n] * 12
    scan = 0 if n <= WIN - 16 else 1 if n > WIN else (0, 1)
    both(dec, dec_scan, data, scan, 2 if n <= STRIDE_MAX else scan, offsets=(0, 5, 11), **v.kw)


# ---------------------------------------------------------------- equal pages, unequal headers
def _stat_spec(tag):
    return H.Hdr(1, stats=H.stats_fields(max_value=b"mmmmmmm" + tag, min_value=b"aaaa", null_count=0))


def test_equal_pages_equal_headers(dec1, dec_scan):
    """130 equal pages with Statistics stay on the stride walk.  Without it such small pages give
    more header candidates than a scan tile holds (64 in 16 KiB), so the serial walk reads the chunk."""
    data, at = build([_stat_spec(b"m")] * 130, 9)
    assert at[0][1] - at[0][0] <= STRIDE_MAX
    run(dec_scan, data, walk=1)
    run(dec1, data, walk=2)


def _leaves_the_stride_walk(dec1, dec_scan, data):
    """On a decoder of its own: the chunk of equal headers takes the stride walk (the control:
    the same size, the same decoder, just before), the chunk `data` of that size does not."""
    control, _ = build([_stat_spec(b"m")] * 130, 9)
    assert len(control) == len(data) and control != data
    run(dec1, control, walk=2)
    exp, _ = run(dec_scan, data, walk=1)
    run(dec1, data, walk=1, exp=exp)
    return exp


@pytest.mark.parametrize("odd", [1, 63, 64, 65, 128, 129])
def test_equal_pages_unequal_headers(dec1, dec_scan, odd):
    """130 pages of one length, headers of at most 64 bytes; one Statistics byte differs on one
    page: the stride walk's byte compare must see it.  The differing byte is not a field K1 keeps,
    so the result would be right either way: the route is what shows it (1, not the control's 2:
    the chunk leaves the stride path, and the scan tile's candidates overflow)."""
    specs = [_stat_spec(b"m")] * 130
    specs[odd] = _stat_spec(b"n")
    data, at = build(specs, 9)
    assert len({p - h for h, p in at}) == 1 and at[0][1] - at[0][0] <= STRIDE_MAX
    _leaves_the_stride_walk(dec1, dec_scan, data)


@pytest.mark.parametrize("odd", [1, 63, 64, 65, 128, 129])
def test_equal_pages_unequal_num_values(dec1, dec_scan, odd):
    """The same with a byte that counts: one page's header says 8 values, not 9 (its page is as
    long as the others: the ninth value's bytes are left unread).  Here a compare that missed the
    byte would also give a wrong count."""
    pages = [PLAIN.page(_stat_spec(b"m"), 9, 9 * k) for k in range(130)]
    pages[odd][0] = pages[odd][0].with_(nvals=8)
    data, _ = H.chunk(pages)
    exp = _leaves_the_stride_walk(dec1, dec_scan, data)
    assert exp.status == 0 and exp.num_values == 130 * 9 - 1


def test_short_last_page_with_statistics(dec1, dec_scan):
    specs = [_stat_spec(b"m")] * 129 + [_stat_spec(b"z")]
    data, _ = build(specs, 9, last_rows=4)
    run(dec_scan, data, walk=1)
    run(dec1, data, walk=2)


# ---------------------------------------------------------------- bounded-parse edges
@pytest.mark.parametrize("k", range(20, 41))
def test_unknown_bool_fields(dec1, dec_scan, k):
    """Every header carries k unknown one-byte bool fields: 10 + k parse steps against kCandSteps = 40."""
    spec = H.Hdr(1, order=[1, 2, 3, ("x", lambda w: w.bools(20, k)), "5"])
    data, at = build([spec] * 12, 9)
    hl = at[0][1] - at[0][0]
    scan = 0 if 10 + k <= 40 else 1
    both(dec1, dec_scan, data, scan, 2 if (scan == 0 and hl <= STRIDE_MAX) else scan, offsets=(0, 9))


@pytest.mark.parametrize("depth", [2, 3, 4, 5, 6, 7])
def test_nested_unknown_structs(dec1, dec_scan, depth):
    """An unknown struct nested `depth` deep in every header: kCandFrames = 4 skip frames."""
    spec = H.Hdr(1, order=[1, 2, 3, "5", ("x", lambda w: w.nested(9, depth))])
    data, _ = build([spec] * 12, 9)
    scan = 0 if depth <= 4 else 1
    both(dec1, dec_scan, data, scan, 2 if scan == 0 else 1, offsets=(0, 9))


@pytest.mark.parametrize("depth", [1, 4, 5])
@pytest.mark.parametrize("variant", ["plain", "v2"])
def test_statistics_with_unknown_nested_fields(dec, dec_scan, depth, variant):
    """Unknown fields of every type and a nested struct inside Statistics (3 known structs deep)."""
    v = Variant(variant)
    st = H.stats_fields(max_value=b"zz", null_count=3, extra=lambda w: w.byte(9, 0x15).nested(10, depth).boolean(11, 1))
    data, _ = build([H.Hdr(1, stats=st)] * 12, 9, v)
    both(dec, dec_scan, data, 0 if depth <= 4 else 1, offsets=(0, 9), **v.kw)
    st = H.stats_fields(max_value=b"zz", extra=lambda w: w.every_type(9))  # 12 more fields: past the steps
    data, _ = build([H.Hdr(1, stats=st)] * 12, 9, v)
    both(dec, dec_scan, data, offsets=(0,), **v.kw)


# ---------------------------------------------------------------- one odd page among canonical ones
ODD = {
    # name: (spec, serial_walk without the stride walk when the chunk's tiles do not overflow)
    "long200": (lambda: H.pad_to(200, 28, 28, H.Hdr(1, nvals=7))[0], 1),            # past the window
    "padded_type": (lambda: H.Hdr(1, pad={1: 1}), 1),                               # no `15 xx 15`: no candidate
    "long_form_2": (lambda: H.Hdr(1, long=(2,)), 1),
    "out_of_order": (lambda: H.Hdr(1, order=[1, 3, 2, "5"]), 1),
    "usize_5_bytes": (lambda: H.Hdr(1, pad={2: 4}), 0),                             # the pre-check's last length
    "usize_6_bytes": (lambda: H.Hdr(1, pad={2: 5}), 1),                             # one past it (_odd_chunk sizes both)
    "wrapped_id": (lambda: H.Hdr(1, wrap=(3,)), 1),
    "both_structs": (lambda: H.Hdr(1, second=(8, 77, 5)), 0),                       # the page's type picks the struct
    "both_structs_rev": (lambda: H.Hdr(2, second=(5, 3, 0), type_=0), None),        # type 0: 3 values, not 7
}


def _odd_chunk(name, pages, at, rows, variant=PLAIN):
    specs = [H.Hdr(1)] * pages
    specs[at] = ODD[name][0]()
    if name == "long200":  # sized for this variant's payload
        pg = variant.page(H.Hdr(1), rows, at * rows)
        specs[at] = H.pad_to(200, pg[2], len(pg[1]), pg[0])[0]
    if name.startswith("usize_"):  # the varint of uncompressed_page_size padded to 5 or 6 bytes
        usize = variant.page(H.Hdr(1), rows, at * rows)[2]
        specs[at] = H.Hdr(1, pad={2: int(name[6]) - len(H.uvarint(H.zz(usize)))})
    data, offs = build(specs, rows, variant)
    if name.startswith("usize_"):
        k = at + len(variant.first())
        hb = data[offs[k][0]:offs[k][1]]
        assert hb[0] == hb[2] == 0x15 and hb[3 + int(name[6])] == 0x15 and all(b & 0x80 for b in hb[3:2 + int(name[6])])
    return data, offs


@pytest.mark.parametrize("at", [0, 1, 6, 11])
@pytest.mark.parametrize("name", list(ODD))
def test_one_odd_page_of_12(dec, dec_scan, name, at):
    data, offs = _odd_chunk(name, 12, at, 7)
    both(dec, dec_scan, data, ODD[name][1], offsets=(0, 13))
    if name.startswith("both_structs"):  # the regression case of the one num_values slot K1 had
        exp, _ = run(dec_scan, data)
        assert exp.status == 0 and exp.pages[at].num_values == (3 if name.endswith("rev") else 7)


@pytest.mark.parametrize("at", [0, 1, 515, 1023, 1024, 1025, 1029])
@pytest.mark.parametrize("name", ["long200", "padded_type", "long_form_2", "out_of_order", "usize_5_bytes"])
def test_one_odd_page_of_1030(dec, dec_scan, name, at):
    """1030 pages of 7 rows: more header candidates than a scan tile holds, so the serial walk
    reads the chunk (asserted), the odd page at its 1024-page block edges."""
    data, _ = _odd_chunk(name, 1030, at, 7)
    both(dec, dec_scan, data, 1)


@pytest.mark.parametrize("at", [1023, 1024, 1025])
@pytest.mark.parametrize("name", ["long200", "padded_type", "usize_5_bytes", "both_structs"])
def test_one_odd_page_of_1030_on_the_chain(dec, dec_scan, name, at):
    """The same with pages of 320 rows, few enough candidates per tile for k_page_chain to run:
    a chain that reaches a candidate it cannot use (kSuccComplex), or no candidate (kSuccMissing),
    at a block edge hands the chunk to the serial walk; an odd page it can use stays on the chain."""
    data, _ = _odd_chunk(name, 1030, at, 320)
    both(dec, dec_scan, data, ODD[name][1])


@pytest.mark.parametrize("variant", ["dict", "v2", "snappy", "optional"])
@pytest.mark.parametrize("pages,at", [(12, 6), (1030, 1024)])
@pytest.mark.parametrize("name", ["long200", "padded_type", "long_form_2", "out_of_order", "usize_5_bytes"])
def test_one_odd_page_variants(dec, dec_scan, name, pages, at, variant):
    v = Variant(variant)
    data, offs = _odd_chunk(name, pages, at, 7, v)
    exp, _ = run(dec_scan, data, walk=1 if pages == 1030 else ODD[name][1], **v.kw)
    assert exp.status == 0 and exp.num_values == 7 * pages
    run(dec, data, **v.kw)


# ---------------------------------------------------------------- a header inside a header
def _inner_header_chunk(miss):
    """12 pages; page 3's Statistics.min_value holds a complete DataPageHeader whose next-page
    position is page 6's header (miss: one byte past it)."""
    inner = H.Hdr(1, nvals=5).build(100, 100)  # a first guess: its length decides the layout
    for _ in range(4):
        specs = [H.Hdr(1)] * 12
        specs[3] = H.Hdr(1, stats=H.stats_fields(min_value=inner))
        data, at = build(specs, 9)
        q = data.index(inner, at[3][0])
        size = at[6][0] + miss - (q + len(inner))
        fit = H.Hdr(1, nvals=5).build(size, size)
        if fit == inner:
            return data, at, q
        inner = fit
    raise AssertionError("the inner header did not settle")


@pytest.mark.parametrize("miss", [0, 1], ids=["lands_on_a_page", "lands_on_no_page"])
def test_header_inside_a_header(dec, dec_scan, miss):
    """A false candidate that classifies ok, inside a true header, with a link into the true chain
    (or to a position without a candidate): the chain from position 0 never takes it."""
    data, at, q = _inner_header_chunk(miss)
    rc, n, h = O.read_page_header(data[q:])
    assert rc == 0 and q + n + h.compressed_size == at[6][0] + miss and at[3][0] < q < at[3][1]
    exp, _ = run(dec_scan, data, walk=0)
    assert exp.status == 0 and len(exp.pages) == 12
    run(dec, data, walk=0)


# ---------------------------------------------------------------- errors in long headers
def _damaged(kind):
    big = b"s" * 300
    if kind == "binary_past_the_end":
        return H.Hdr(1, stats=lambda w: w.binary(5, big, claim=1 << 24))
    if kind == "negative_length":
        return H.Hdr(1, stats=lambda w: w.binary(5, big).binary(6, b"", claim=-5))
    if kind == "missing_required":
        return H.Hdr(1, stats=H.stats_fields(max_value=big), inner_order=[5, 1, 2, 3])
    if kind == "lost_stop":
        return H.Hdr(1, stats=H.stats_fields(max_value=big[:200]), order=[1, 2, 3, "5", ("x", lambda w: w.raw(b"\x1d"))])
    raise ValueError(kind)


@pytest.mark.parametrize("pages,at", [(12, 5), (1030, 1024)])
@pytest.mark.parametrize("kind", ["binary_past_the_end", "negative_length", "missing_required", "lost_stop"])
def test_errors_in_long_headers(dec, dec_scan, kind, pages, at):
    specs = [H.Hdr(1)] * pages
    specs[at] = _damaged(kind)
    data, _ = build(specs, 7)
    for d in (dec_scan, dec):
        exp, got = run(d, data)
        assert exp.status == abi.STATUS_CODES["THRIFT"] and exp.error_page == at
        assert (got.status, got.error_page) == (exp.status, exp.error_page)


# ---------------------------------------------------------------- checksums
def _crc_chunk(shape, good=True):
    pages = []
    for k in range(12):
        raw = vals(9, 9 * k).tobytes()
        c = zlib.crc32(raw) ^ (0 if good else 0x10)
        if shape == "long_form":
            spec = H.Hdr(1, nvals=9, crcs=[c], long=(4,))
        elif shape == "twice":
            spec = H.Hdr(1, nvals=9, crcs=[c ^ 0xFFFF, c], order=[1, 2, 3, 4, "5", 4])
        else:  # after the page-header struct, in a 200-byte header
            spec = H.pad_to(200, len(raw), len(raw), H.Hdr(1, nvals=9, crcs=[c], order=[1, 2, 3, "5", 4]))[0]
        pages.append((spec, raw, c))
    data, _ = H.chunk([p[:2] for p in pages])
    return data, [p[2] for p in pages], [zlib.crc32(p[1]) for p in pages]


@pytest.mark.parametrize("shape", ["long_form", "twice", "after_the_struct_200"])
def test_checksum_fields(dec, dec_scan, shape):
    """PageHeader.crc in long form, written twice (the last one read counts, as k_crc_plan
    documents) and after the page-header struct of a long header."""
    data, stored, want = _crc_chunk(shape)
    for d in (dec_scan, dec):
        d.set_verify_crc(True)
        try:
            run(d, data)
            crcs = d.page_crcs(0)
            assert [(c.state, c.stored, c.computed) for c in crcs] == [(abi.CRC_VERIFIED, s, w) for s, w in zip(stored, want)]
            assert stored == want
            # the control: the value that counts is wrong
            bad, bstored, _ = _crc_chunk(shape, good=False)
            keep = []
            job, buf = U.chunk_job(bad, keep=keep, **PLAIN.kw)
            dev = d.upload(buf)
            try:
                job.data = dev
                r = d.decode_jobs([job])[0]
                assert (r.status, r.error_page) == (CRC, 0)
                c0 = d.page_crcs(0)[0]
                assert (c0.state, c0.stored, c0.computed) == (abi.CRC_MISMATCH, bstored[0], want[0])
            finally:
                d.free(dev)
        finally:
            d.set_verify_crc(False)


# ---------------------------------------------------------------- pyarrow: an independent writer and reader
def _arrow_table():
    """4000 rows: strings of 10, 70 and 600 bytes (a random 5-letter word repeated: every codec
    shrinks them, so that V2 pages are stored compressed, which the reference takes for granted)
    and an INT64 column of small numbers."""
    import pyarrow as pa
    rng = np.random.default_rng(31)
    n = 4000
    words = ["".join(chr(c) for c in w) for w in rng.integers(97, 123, size=(n, 5))]
    return pa.table({"s10": [w * 2 for w in words], "s70": [w * 14 for w in words], "s600": [w * 120 for w in words],
                     "i64": rng.integers(0, 1000, size=n, dtype=np.int64)})


@pytest.fixture(scope="module")
def arrow_table():
    pytest.importorskip("pyarrow")
    return _arrow_table()


MIN_HEADER = {"s10": 0, "s70": 160, "s600": 1024, "i64": 64}


# (data page version, compression, dictionary).  No 2.0 + snappy + dictionary: its index pages do
# not shrink, pyarrow stores them uncompressed (is_compressed = false), and the reference, which
# ignores that flag, fails on them.
ARROW_FILES = [(v, c, False) for v in ("1.0", "2.0") for c in ("none", "snappy")] + \
    [("1.0", "none", True), ("2.0", "none", True), ("1.0", "snappy", True)]


@pytest.mark.parametrize("version,compression,dictionary", ARROW_FILES)
def test_pyarrow_headers_with_statistics(dec, dec_scan, arrow_table, version, compression, dictionary):
    """pyarrow's headers at default statistics: past the stride walk's 64 bytes (INT64), past the
    candidate window (70-byte strings), past kCandParseBytes and a kWin window (600-byte strings).
    Values: the GPU's equal the oracle's (compare_file), the oracle's equal pq.read_table's."""
    pq = pytest.importorskip("pyarrow.parquet")
    buf = io.BytesIO()
    pq.write_table(arrow_table, buf, data_page_version=version, compression=compression, data_page_size=2048,
                   write_batch_size=64, use_dictionary=dictionary)
    data = buf.getvalue()
    back = pq.read_table(io.BytesIO(data))
    pf = pqgpu.ParquetFile(data)
    names = arrow_table.column_names
    assert pf.num_columns == len(names) and pf.num_row_groups == 1
    for d in (dec_scan, dec):
        try:
            P.compare_file(data, d)
        except pqgpu.PqgError as err:
            if err.code == abi.STATUS_CODES["HIP"]:
                pytest.exit("decode failed: %s" % err, returncode=3)
            raise
    for c, name in enumerate(names):
        exp = P.oracle_chunk(pf, 0, c)
        assert exp.status == 0 and exp.num_values == 4000
        dp = [p for p in exp.pages if p.page_type in (0, 3)]
        assert len(dp) >= (2 if dictionary else 12), (name, len(dp))
        assert min(p.payload_offset - p.header_offset for p in dp) > MIN_HEADER[name], name
        col = back.column(name).combine_chunks()
        if name == "i64":
            assert np.array_equal(exp.values.view(np.int64), col.to_numpy())
        else:
            want = "".join(col.to_pylist()).encode()
            assert exp.values.tobytes() == want
            assert np.array_equal(np.diff(exp.offsets), np.full(4000, len(want) // 4000))
