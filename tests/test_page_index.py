"""Located decode (pqg_decode_chunks_located) and pqg_range_bitmap on the GPU.

The located decode of a job J with page locations L must give what the scanned decode gives for
the job J' whose data is the bytes of L's pages back to back (total_compressed_size = the sum of
the sizes, no dictionary page offset): every expectation here is the CPU oracle's (or the scanned
GPU decode's) result for J', never the located path's own."""
import io
import os
import re

import numpy as np
import pytest

import hdr_util as H
import parity
import pqgpu
import pqtest_util as U
from oracle import pyoracle as O
from pqgpu import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX = abi.STATUS_CODES["INDEX"]
INVALID = abi.STATUS_CODES["INVALID_ARG"]
# every page-table field the equivalence covers (header_offset / payload_offset stay relative to J.data)
PAGE_FIELDS = ("slot_offset", "value_offset", "page_type", "encoding", "num_values", "not_null", "compressed_size",
               "uncompressed_size", "def_len", "rep_len", "def_encoding", "rep_encoding", "status")


@pytest.fixture(scope="module")
def dec():
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


def cand_win_bytes():
    """Bytes of a lane's header window (kCandWin 16-byte granules, pqg_common.h)."""
    text = open(os.path.join(ROOT, "parquet-go_amd", "csrc", "pqg_common.h")).read()
    return 16 * int(re.search(r"constexpr int kCandWin = (\d+);", text).group(1))


def packed(chunk, locs):
    """The bytes of J' and the locations rebased to them."""
    out, rebased, at = bytearray(), [], 0
    for off, size in locs:
        out += chunk[off:off + size]
        rebased.append((at, size))
        at += size
    return bytes(out), rebased


def oracle_packed(chunk, locs, **kw):
    b, _ = packed(chunk, locs)
    job, _buf = U.chunk_job(b, keep=[], **kw)
    return O.decode_chunk(job)


def decode_located(dec, data, locs, keep_flag=False, **kw):
    """Job over `data` (uploaded whole) decoded by the locations: (DecodedColumn, debug_job)."""
    job, buf = U.chunk_job(data, keep=[], **kw)
    if keep_flag:
        job.col.flags |= abi.COL_KEEP_DICT
    dev = dec.upload(buf)
    try:
        job.data = dev
        r = dec.decode_located([job], [locs])[0]
        return dec.download(r, 0), dec.debug_job(0)
    finally:
        dec.free(dev)


def same_pages(got, exp, locs, where="", fields=PAGE_FIELDS):
    assert len(got) == len(exp), "%s pages %d vs %d" % (where, len(got), len(exp))
    for k, (a, b) in enumerate(zip(got, exp)):
        for f in fields:
            x, y = getattr(a, f), getattr(b, f)
            assert x == y, "%s page %d %s: %s vs %s" % (where, k, f, x, y)
        assert a.header_offset == locs[k][0], "%s page %d header_offset" % (where, k)


def check_subset(dec, chunk, locs, **kw):
    """Located decode of `locs` against the oracle on J', with the whole chunk resident (the gaps
    skipped) and with only J' uploaded (locations rebased)."""
    exp = oracle_packed(chunk, locs, **kw)
    for name, (data, ls) in (("resident", (chunk, locs)), ("packed", packed(chunk, locs))):
        got, dbg = decode_located(dec, data, ls, **kw)
        parity.compare_chunk(exp, got, name)
        if exp.status == 0:
            same_pages(got.pages, exp.pages, ls, name)
        else:
            # the oracle fills in no page after the one that fails, and decodes none when the read phase
            # fails: the header fields of the pages before it, and the failing page's status
            k = exp.error_page
            same_pages(got.pages[:k], exp.pages[:k], ls, name,
                       [f for f in PAGE_FIELDS if f not in ("not_null", "value_offset")])
            assert got.pages[k].status == exp.pages[k].status == exp.status, name
        assert dbg[0] == 3 and dbg[1] == 0, dbg
    return exp


def locs_of(pages):
    return [(p.header_offset, p.payload_offset - p.header_offset + p.compressed_size) for p in pages]


# ------------------------------------------------------------------ all pages located == the scanned decode
def fixture_file(compression, version, rows=20000, page_index=True, checksum=False):
    pa = pytest.importorskip("pyarrow")
    pq = pytest.importorskip("pyarrow.parquet")
    rng = np.random.default_rng(7)
    a = np.arange(rows, dtype=np.int64) * 3
    words = np.array(["w%03d" % i for i in range(200)], dtype=object)
    s = words[rng.integers(0, 200, rows)]
    s[rng.random(rows) < 0.2] = None
    s[4096:14000] = None  # whole pages of nulls
    lens = rng.integers(0, 5, rows)
    flat = rng.integers(0, 1000, int(lens.sum())).astype(np.int32)
    offs = np.zeros(rows + 1, np.int32)
    np.cumsum(lens, out=offs[1:])
    t = pa.table({"a": pa.array(a), "s": pa.array(list(s), pa.string()),
                  "l": pa.ListArray.from_arrays(pa.array(offs), pa.array(flat))})
    buf = io.BytesIO()
    pq.write_table(t, buf, compression=compression.upper(), data_page_version=version, data_page_size=4096,
                   write_page_index=page_index, use_dictionary=["s"], write_page_checksum=checksum)
    return buf.getvalue(), t


@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("compression", ["none", "snappy", "zstd"])
def test_all_pages_located_equals_scan(dec, compression, version):
    data, _ = fixture_file(compression, version)
    pf = pqgpu.ParquetFile(data)
    dev = dec.upload(pf.data)
    try:
        jobs = [pqgpu.device_job(pf, 0, c, dev) for c in range(pf.num_columns)]
        res = dec.decode_jobs(jobs)
        scanned = [dec.download(r, i) for i, r in enumerate(res)]
        # (a V2 page that pyarrow stores uncompressed in a compressed chunk is a size mismatch to the
        # scanned decode: the located one must report that chunk as the scan does)
        assert scanned[0].status == 0 and scanned[2].status == 0 and all(len(s.pages) > 1 for s in scanned)
        lists = [locs_of(s.pages) for s in scanned]
        for i, s in enumerate(scanned):
            if s.status != 0:  # the scan stopped at a page: J' is the pages up to it, scanned on their own
                m = pf.chunk_meta(0, i)
                b, _ = packed(bytes(pf.read_range(m.start, m.start + m.total_compressed_size)), lists[i])
                pdev = dec.upload(np.frombuffer(b, np.uint8))
                j = pqgpu.device_job(pf, 0, i, dev)
                j.data, j.data_len, j.total_compressed_size, j.has_dict_page_offset = pdev, len(b), len(b), 0
                scanned[i] = dec.download(dec.decode_jobs([j])[0], 0)
                dec.free(pdev)
                assert scanned[i].status == s.status and scanned[i].error_page == s.error_page
        res = dec.decode_located(jobs, lists)
        for i, (r, exp) in enumerate(zip(res, scanned)):
            got = dec.download(r, i)
            assert (got.status, got.error_page, got.num_slots, got.num_values) == \
                (exp.status, exp.error_page, exp.num_slots, exp.num_values)
            for f in ("def_levels", "rep_levels", "values", "offsets"):
                a, b = getattr(got, f), getattr(exp, f)
                assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), (i, f)
            assert [bytes(p) for p in got.pages] == [bytes(p) for p in exp.pages], i
            dbg = dec.debug_job(i)
            assert dbg[0] == 3 and dbg[1] == 0, dbg
    finally:
        dec.free(dev)


# ------------------------------------------------------------------ page counts at the kernel's edges
def one_value_pages(n):
    pages = [U.v1_page(U.u32(i), 1, abi.ENC_PLAIN) for i in range(n)]
    locs, at = [], 0
    for p in pages:
        locs.append((at, len(p)))
        at += len(p)
    return b"".join(pages), locs


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 32769])
def test_page_counts(dec, n):
    chunk, locs = one_value_pages(n)
    job, _ = U.chunk_job(chunk, keep=[], ptype=abi.INT32)
    exp = O.decode_chunk(job)
    assert exp.status == 0 and exp.num_values == n
    got, dbg = decode_located(dec, chunk, locs, ptype=abi.INT32)
    parity.compare_chunk(exp, got, "n=%d" % n)
    same_pages(got.pages, exp.pages, locs)
    assert dbg[0] == 3 and dbg[1] == 0


# ------------------------------------------------------------------ subsets
def dict_chunk(n_data=6, second_dict_at=None):
    """INT32 chunk: a PLAIN dictionary page of 4 entries, then RLE_DICTIONARY pages of 5 equal keys;
    `second_dict_at`: another dictionary page before that data page.  (bytes, [(offset, size)])."""
    entries = H.plain_i32([10, 20, 30, 40])
    dpage = U.page_header_dict(len(entries), len(entries), 4) + entries
    pages = [dpage]
    for k in range(n_data):
        if second_dict_at == k:
            pages.append(dpage)
        body = bytes([2]) + U.uvarint(5 << 1) + bytes([k % 4])
        pages.append(U.page_header_v1(len(body), len(body), 5, abi.ENC_RLE_DICTIONARY) + body)
    locs, at = [], 0
    for p in pages:
        locs.append((at, len(p)))
        at += len(p)
    return b"".join(pages), locs


def test_subsets(dec):
    chunk, locs = dict_chunk()
    kw = dict(ptype=abi.INT32)
    full = check_subset(dec, chunk, locs, **kw)
    assert full.status == 0 and full.num_values == 30
    e = check_subset(dec, chunk, locs[:2], **kw)          # the dictionary and the first data page
    assert e.status == 0 and e.num_values == 5
    e = check_subset(dec, chunk, [locs[0], locs[-1]], **kw)   # ... and the last page only
    assert e.status == 0 and e.num_values == 5
    e = check_subset(dec, chunk, [locs[0]] + locs[1::2], **kw)  # every other data page
    assert e.status == 0 and e.num_values == 15
    e = check_subset(dec, chunk, locs[:1], **kw)          # the dictionary page alone
    assert e.status == 0 and e.num_slots == 0 and len(e.pages) == 1
    check_subset(dec, chunk, locs[1:], **kw)              # dictionary-encoded pages without it: what J' says
    check_subset(dec, chunk, locs[2:4], **kw)
    plain, plocs = one_value_pages(9)                     # no dictionary at all: first, last, every other
    for sub in (plocs[:1], plocs[-1:], plocs[::2]):
        e = check_subset(dec, plain, sub, **kw)
        assert e.status == 0 and e.num_values == len(sub)


def test_dictionary_listed_twice(dec):
    chunk, locs = dict_chunk(second_dict_at=1)  # dictionary, data, dictionary, data ...
    exp = check_subset(dec, chunk, locs, ptype=abi.INT32)
    assert exp.status == abi.STATUS_CODES["DICT_PAGE"] and exp.error_page == 2
    exp = check_subset(dec, chunk, locs[:4], ptype=abi.INT32)
    assert exp.status == abi.STATUS_CODES["DICT_PAGE"] and exp.error_page == 2
    exp = check_subset(dec, chunk, locs[2:], ptype=abi.INT32)  # the second one alone is a first one
    assert exp.status == 0


# ------------------------------------------------------------------ headers the lane parse cannot finish
def odd_chunk(spec, at, n=70):
    plain = H.Hdr(1, nvals=1)
    chunk, pos = H.chunk([(spec if k == at else plain, H.plain_i32([k])) for k in range(n)])
    ends = [p[0] for p in pos[1:]] + [len(chunk)]
    return chunk, [(p[0], e - p[0]) for p, e in zip(pos, ends)], pos


@pytest.mark.parametrize("at", [0, 35, 69])
@pytest.mark.parametrize("kind", ["long_statistics", "no_short_prefix"])
def test_headers_past_the_lane_parse(dec, kind, at):
    if kind == "long_statistics":
        spec = H.Hdr(1, nvals=1, stats=H.stats_fields(max_value=b"m" * (2 * cand_win_bytes()), null_count=0))
    else:
        spec = H.Hdr(1, nvals=1, long=(1,))
    chunk, locs, pos = odd_chunk(spec, at)
    if kind == "long_statistics":
        assert pos[at][1] - pos[at][0] > cand_win_bytes()
    else:
        assert chunk[pos[at][0]] != 0x15
    exp = check_subset(dec, chunk, locs, ptype=abi.INT32)
    assert exp.status == 0 and exp.num_values == 70
    check_subset(dec, chunk, locs[at:at + 1], ptype=abi.INT32)


# ------------------------------------------------------------------ PQG_ERR_INDEX and host rejections
def junk_led_page(k):
    """A one-value page whose header starts with a skipped field (a BOOL of id 1, one byte) before
    long-form fields 1-3: the bytes from its second byte on are a header too, with the same sizes."""
    body = H.plain_i32([k])
    w = H.HW()
    w.boolean(1, False)
    w.i32(1, 0, True).i32(2, len(body), True).i32(3, len(body), True)
    w.begin(5, True).i32(1, 1).i32(2, 0).i32(3, 3).i32(4, 3).end()
    return w.stop() + body


@pytest.mark.parametrize("at", [0, 4, 8])
@pytest.mark.parametrize("case", ["offset+1", "size+1", "size-1"])
def test_err_index(dec, case, at):
    """A listed page that does not end at offset + size.  INDEX is the error of a page whose own
    read phase is fine, so the offset case lists a page whose bytes from the second one on are a
    header as well (junk_led_page): one byte into an ordinary header, the parse itself fails and
    the page reports that error, as J' does."""
    n = 9
    pages = [junk_led_page(k) if (case == "offset+1" and k == at) else U.v1_page(U.u32(k), 1, abi.ENC_PLAIN)
             for k in range(n)]
    locs, pos = [], 0
    for p in pages:
        locs.append((pos, len(p)))
        pos += len(p)
    chunk = b"".join(pages) + b"\0\0"  # room for a last page listed one byte too long
    job, _ = U.chunk_job(chunk[:pos], keep=[], ptype=abi.INT32)
    scan = O.decode_chunk(job)
    assert scan.status == 0
    bad = list(locs)
    off, size = locs[at]
    bad[at] = {"offset+1": (off + 1, size), "size+1": (off, size + 1), "size-1": (off, size - 1)}[case]
    if case != "size-1" and at + 1 < n:
        del bad[at + 1]  # the page after would overlap
    got, _ = decode_located(dec, chunk, bad, ptype=abi.INT32)
    assert abi.status_name(got.status) == "INDEX" and got.error_page == at
    assert len(got.pages) == at + 1 and got.pages[at].status == INDEX
    same_pages(got.pages[:at], scan.pages[:at], locs)


def test_host_rejections(dec):
    chunk, locs = one_value_pages(5)
    got, dbg = decode_located(dec, chunk, locs, ptype=abi.INT32)
    assert got.status == 0
    job, buf = U.chunk_job(chunk, keep=[], ptype=abi.INT32)
    dev = dec.upload(buf)
    try:
        job.data = dev
        (o0, s0), (o1, s1) = locs[0], locs[1]
        for bad in ([locs[1], locs[0]], [(o0, s0 + 1), (o1, s1)], [(o0, s0), (o0, s0)], [(-1, s0)],
                    [(o0, 0)], [(o0, -3)], [(len(chunk) - 1, 2)], [(len(chunk), 1)]):
            with pytest.raises(pqgpu.PqgError) as e:
                dec.decode_located([job], [bad])
            assert e.value.code == INVALID, bad
            assert dec.debug_job(0) == dbg  # nothing was enqueued: the last decode's record stands
    finally:
        dec.free(dev)


# ------------------------------------------------------------------ mixed batches, kept dictionaries, checksums
def test_mixed_batch_and_keep_dict(dec):
    chunk, locs = dict_chunk()
    plain, plocs = one_value_pages(70)
    bufs = [np.frombuffer(chunk, np.uint8), np.frombuffer(plain, np.uint8)]
    devs = [dec.upload(b) for b in bufs]
    try:
        def job(i, flags=0):
            j, _ = U.chunk_job([chunk, plain][i], keep=[], ptype=abi.INT32)
            j.data = devs[i]
            j.col.flags |= flags
            return j
        jobs = [job(0), job(1), job(0, abi.COL_KEEP_DICT), job(1), job(0, abi.COL_KEEP_DICT)]
        res = dec.decode_located(jobs, [locs, None, locs, plocs[::2], None])
        got = [dec.download(r, i) for i, r in enumerate(res)]
        assert [dec.debug_job(i)[0] == 3 for i in range(5)] == [True, False, True, True, False]
        e0 = oracle_packed(chunk, locs, ptype=abi.INT32)
        parity.compare_chunk(e0, got[0], "located")
        parity.compare_chunk(oracle_packed(plain, plocs, ptype=abi.INT32), got[1], "scanned")
        parity.compare_chunk(oracle_packed(plain, plocs[::2], ptype=abi.INT32), got[3], "subset")
        a, b = got[2], got[4]  # the located keep-dictionary job against the scanned one
        assert a.status == b.status == 0 and a.dictionary is not None and b.dictionary is not None
        assert np.array_equal(a.keys(), b.keys()) and np.array_equal(a.dictionary.table(), b.dictionary.table())
        assert np.array_equal(a.materialize().values, e0.values)
    finally:
        for d in devs:
            dec.free(d)


def test_verify_crc_located(dec):
    data, _ = fixture_file("snappy", "1.0", rows=6000, checksum=True)
    pf = pqgpu.ParquetFile(data)
    m = pf.chunk_meta(0, 0)
    chunk = bytes(pf.read_range(m.start, m.start + m.total_compressed_size))
    kw = dict(ptype=abi.INT64, codec=abi.CODEC_SNAPPY)
    hjob, _hbuf = U.chunk_job(chunk, keep=[], **kw)
    scan = O.decode_chunk(hjob)
    assert scan.status == 0 and len(scan.pages) >= 3
    locs = locs_of(scan.pages)
    dec.set_verify_crc(True)
    try:
        got, _ = decode_located(dec, chunk, locs, **kw)
        parity.compare_chunk(scan, got, "clean")
        job, buf = U.chunk_job(chunk, keep=[], **kw)
        dev = dec.upload(buf)
        try:
            job.data = dev
            dec.decode_located([job], [locs])
            assert [c.state for c in dec.page_crcs(0)] == [abi.CRC_VERIFIED] * len(locs)
        finally:
            dec.free(dev)
        bad = bytearray(chunk)
        bad[scan.pages[1].payload_offset + 3] ^= 0x40
        got, _ = decode_located(dec, bytes(bad), locs, **kw)
        assert abi.status_name(got.status) == "CRC" and got.error_page == 1
    finally:
        dec.set_verify_crc(False)


# ------------------------------------------------------------------ pqg_range_bitmap
def bitmap_model(ranges, n):
    bits = np.zeros(((n + 31) // 32) * 32, np.uint8)
    for lo, hi in ranges:
        bits[lo:hi] = 1
    return np.packbits(bits, bitorder="little")


def range_cases(n):
    yield []
    yield [(0, n)]
    yield [(0, 0), (0, n), (n, n)]
    yield [(k, k + 1) for k in range(0, min(n, 2000), 2)][:1000]
    edges = [e for e in (0, 1, 31, 32, 33, 64, 96, 2047, 2048, n - 1, n) if 0 <= e <= n]
    edges = sorted(set(edges))
    yield list(zip(edges[:-1], edges[1:]))              # adjacent ranges, on and off dword edges
    yield list(zip(edges[:-1:2], edges[1::2]))
    yield [(a, a) for a in edges]                       # empty ranges only
    if n > 64:
        yield [(32, 64)]
        yield [(31, 33), (33, 33), (63, 65)]


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 2047, 2048, 100003])
def test_range_bitmap(dec, n):
    nbytes = 4 * ((n + 31) // 32)
    ptr = dec.upload(np.full(max(nbytes, 4), 0xFF, np.uint8))
    try:
        cases = list(range_cases(n))
        if n == 100003:
            cases.append([(k, k + 1) for k in range(5, 100003, 100)][:1000])
        for ranges in cases:
            dec.range_bitmap(ranges, n, ptr)
            got = dec.d2h(ptr, nbytes)
            assert np.array_equal(got, bitmap_model(ranges, n)), ranges[:8]
        for bad in ([(1, 0)], [(0, n + 1)], [(-1, 0)], [(0, 1), (0, 1)] if n else [(0, 1)]):
            with pytest.raises(pqgpu.PqgError) as e:
                dec.range_bitmap(bad, n, ptr)
            assert e.value.code == INVALID
    finally:
        dec.free(ptr)


# ------------------------------------------------------------------ FileReader: use_page_index, rows=, filters
def col_tuple(c):
    """A flat DecodedColumn (materialised) as comparable host data."""
    c = c.materialize()
    return (c.status, c.num_slots, c.num_values,
            None if c.def_levels is None else c.def_levels.tobytes(),
            None if c.values is None else np.asarray(c.values).tobytes(),
            None if c.offsets is None else np.asarray(c.offsets).tobytes())


def slice_col(c, lo, hi):
    """Rows [lo, hi) of an unfiltered flat DecodedColumn, as col_tuple gives them."""
    c = c.materialize()
    d = c.def_levels
    nn = np.concatenate([[0], np.cumsum(d == d.max() if len(d) else d)]) if d is not None else np.arange(c.num_slots + 1)
    v0, v1 = int(nn[lo]), int(nn[hi])
    if c.offsets is not None:
        o = np.asarray(c.offsets)
        vals = np.asarray(c.values)[o[v0]:o[v1]].tobytes()
        offs = (o[v0:v1 + 1] - o[v0]).astype(np.int64).tobytes()
    else:
        w = c.value_width
        vals, offs = np.asarray(c.values)[v0 * w:v1 * w].tobytes(), None
    return (0, hi - lo, v1 - v0, None if d is None else d[lo:hi].tobytes(), vals, offs)


@pytest.fixture(scope="module")
def indexed():
    data, table = fixture_file("snappy", "1.0")
    return data, table


@pytest.mark.parametrize("cols", [("a",), ("s",), ("a", "s")])
def test_reader_rows(dec, indexed, cols):
    data, _ = indexed
    n = 20000
    full = pqgpu.FileReader(data, *cols, decoder=dec).read_row_group(0)
    for lo, hi in [(0, 0), (0, 1), (n - 1, n), (1000, 1030), (1024, 2048), (1000, 9000), (0, n)]:
        got, sent = {}, {}
        for use in (False, True):
            fr = pqgpu.FileReader(data, *cols, decoder=dec, use_page_index=use)
            out = fr.read_row_group(0, rows=(lo, hi) if use else slice(lo, hi))
            got[use] = {k: col_tuple(v) for k, v in out.items()}
            sent[use] = fr.uploaded_bytes
            assert fr.last_read["row_ranges"] == ([(lo, hi)] if hi > lo else [])
            if use and (lo, hi) == (0, n):
                assert fr.last_read["pages_decoded"] == fr.last_read["pages_total"] > 0
            elif use:
                assert fr.last_read["pages_decoded"] < max(fr.last_read["pages_total"], 1)
        assert got[True] == got[False]
        if hi == lo:  # no rows: neither reader uploads anything
            assert sent[True] == sent[False] == 0
        elif (lo, hi) != (0, n):  # fewer bytes than the read of the same range without the index
            assert 0 < sent[True] < sent[False], (lo, hi, sent)
        else:
            assert sent[True] == sent[False] > 0
        for name in cols:
            exp = slice_col(full[name], lo, hi)
            if hi == lo:
                assert got[True][name][1:3] == (0, 0)
            else:
                assert got[True][name] == exp, (name, lo, hi)


def test_reader_rows_rejects_lists(dec, indexed):
    data, _ = indexed
    fr = pqgpu.FileReader(data, "l", decoder=dec, use_page_index=True)
    before = fr.uploaded_bytes
    with pytest.raises(pqgpu.PqgError) as e:
        fr.read_row_group(0, rows=(0, 10))
    assert abi.status_name(e.value.code) == "UNSUPPORTED" and fr.uploaded_bytes == before


def page_may_pass(pi, k, col, op, val):
    """Can a row of page k pass `col op val`, going by the page's ColumnIndex entry alone?  The test's
    own reading of the index (min / max as int64 or bytes, null_counts), for the operators used here."""
    a, b = pi.page_rows(k)
    nulls = pi.null_counts[k]
    if op == "is":
        return nulls > 0
    if pi.null_pages[k] or nulls == b - a:
        return False
    if op == "is not":
        return True
    lo, hi = pi.min_values[k], pi.max_values[k]
    if col == "a":
        lo, hi = int.from_bytes(lo, "little", signed=True), int.from_bytes(hi, "little", signed=True)
    else:
        val = val.encode()
    return {"==": lo <= val <= hi, "!=": not (lo == hi == val), "<": lo < val, "<=": lo <= val, ">": hi > val,
            ">=": hi >= val}[op]


def brute_pages(pf, fr, dnf, rows=None):
    """(pages listed, pages in all) over the needed columns, by brute force from the index: a row is
    kept when it lies in `rows` and, for some conjunction, every term's page holding it may pass."""
    n = 20000
    conjs = dnf if isinstance(dnf[0], list) else [dnf]
    inside = np.zeros(n, bool)
    for conj in conjs:
        m = np.ones(n, bool)
        for col, op, val in conj:
            pi = pf.page_index(0, pf.column_index(col))
            t = np.zeros(n, bool)
            for k in range(len(pi.locations)):
                if page_may_pass(pi, k, col, op, val):
                    t[slice(*pi.page_rows(k))] = True
            m &= t
        inside |= m
    if rows is not None:
        lim = np.zeros(n, bool)
        lim[rows[0]:rows[1]] = True
        inside &= lim
    assert fr.last_read["row_ranges"] == [(int(a), int(b)) for a, b in zip(
        np.flatnonzero(np.diff(np.r_[0, inside.view(np.int8)]) == 1),
        np.flatnonzero(np.diff(np.r_[inside.view(np.int8), 0]) == -1) + 1)]
    cols = set(fr.selected) | {pf.column_index(t[0]) for conj in (dnf if isinstance(dnf[0], list) else [dnf]) for t in conj}
    listed = total = 0
    for c in cols:
        pi = pf.page_index(0, c)
        total += len(pi.locations)
        listed += sum(bool(inside[slice(*pi.page_rows(k))].any()) for k in range(len(pi.locations)))
    return listed, total


FILTER_CASES = [
    (("a", "s"), {}, [("a", ">=", 15000), ("a", "<", 15300)], None, True),
    (("a", "s"), {}, [("s", "==", "w017")], None, False),
    (("a", "s"), {"read_dictionary": ("s",)}, [("s", "==", "w017")], None, False),
    (("a", "s"), {}, [("s", "is", None)], None, False),
    (("a",), {}, [("a", "!=", 30)], None, False),
    (("a", "s"), {}, [[("a", "<", 900)], [("a", ">", 59000)]], None, True),
    (("s",), {}, [("a", ">=", 30000), ("a", "<", 30030)], None, True),          # the predicate column is not selected
    (("a", "s"), {}, [("a", "<", 0)], None, True),                              # no page can pass
    (("a", "s"), {}, [("a", ">=", 3000), ("s", "is not", None)], (900, 1100), True),
]


@pytest.mark.parametrize("case", range(len(FILTER_CASES)))
def test_reader_filters_with_the_index(dec, indexed, case):
    data, _ = indexed
    cols, kw, dnf, rows, strict = FILTER_CASES[case]
    plain = pqgpu.FileReader(data, *cols, decoder=dec, **kw)
    exp = plain.read_row_group(0, filters=dnf, rows=rows)
    fr = pqgpu.FileReader(data, *cols, decoder=dec, use_page_index=True, **kw)
    got = fr.read_row_group(0, filters=dnf, rows=rows)
    assert {k: col_tuple(v) for k, v in got.items()} == {k: col_tuple(v) for k, v in exp.items()}
    listed, total = brute_pages(fr.file, fr, dnf, rows)
    assert (fr.last_read["pages_decoded"], fr.last_read["pages_total"]) == (listed, total if listed else 0)
    if strict:
        assert listed < total and fr.uploaded_bytes < plain.uploaded_bytes
    if dnf == [("a", "<", 0)]:
        assert fr.uploaded_bytes == 0 and all(v.num_slots == 0 for v in got.values())


def test_reader_without_an_index_in_the_file(dec):
    data, _ = fixture_file("snappy", "1.0", page_index=False)
    a = pqgpu.FileReader(data, "a", "s", decoder=dec)
    b = pqgpu.FileReader(data, "a", "s", decoder=dec, use_page_index=True)
    for kw in ({}, {"rows": (1000, 1030)}, {"filters": [("a", "<", 900)]}):
        x, y = a.read_row_group(0, **kw), b.read_row_group(0, **kw)
        assert {k: col_tuple(v) for k, v in x.items()} == {k: col_tuple(v) for k, v in y.items()}
        assert not any(b.last_read["located"].values()) and b.last_read["fell_back"] == []


def test_reader_falls_back_on_a_wrong_index(dec, indexed, monkeypatch):
    data, _ = indexed
    exp = pqgpu.FileReader(data, "a", "s", decoder=dec).read_row_group(0)
    fr = pqgpu.FileReader(data, "a", "s", decoder=dec, use_page_index=True)
    real = fr.file.page_index

    def wrong(rg, col):
        pi = real(rg, col)
        if col == 0:
            locs = list(pi.locations)
            locs[3] = (locs[3][0], locs[3][1] - 1, locs[3][2])  # a page listed one byte short
            pi = pqgpu.reader.PageIndex(locs, pi.rows)
        return pi
    monkeypatch.setattr(fr.file, "page_index", wrong)
    got = fr.read_row_group(0)
    assert {k: col_tuple(v) for k, v in got.items()} == {k: col_tuple(v) for k, v in exp.items()}
    assert fr.last_read["fell_back"] == [(0, 0)] and fr.last_read["located"][(0, 0)] is False


def test_reader_nested_and_tree_with_the_index(dec, indexed):
    data, _ = indexed
    a = pqgpu.FileReader(data, decoder=dec)
    b = pqgpu.FileReader(data, decoder=dec, use_page_index=True)
    x, y = a.read_row_group_nested(0), b.read_row_group_nested(0)
    assert all(b.last_read["located"].values()) and not any(a.last_read["located"].values())
    assert x.keys() == y.keys()
    for k in x:
        assert x[k].to_pylist() == y[k].to_pylist(), k
    tx, ty = a.read_row_group_tree(0), b.read_row_group_tree(0)
    assert tx.to_pylist() == ty.to_pylist()


def test_short_last_page_of_a_packed_upload(dec):
    """A page listed one byte short reports INDEX where the bytes after it are resident
    (test_err_index), and what J' reports, a size mismatch, where the list ends the data."""
    chunk, locs = one_value_pages(5)
    bad = locs[:-1] + [(locs[-1][0], locs[-1][1] - 1)]
    b, rebased = packed(chunk, bad)
    exp = oracle_packed(chunk, bad, ptype=abi.INT32)
    assert abi.status_name(exp.status) == "SIZE" and exp.error_page == 4
    got, _ = decode_located(dec, b, rebased, ptype=abi.INT32)
    parity.compare_chunk(exp, got, "packed")
    got, _ = decode_located(dec, chunk, bad, ptype=abi.INT32)
    assert abi.status_name(got.status) == "INDEX" and got.error_page == 4


@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("compression", ["none", "snappy", "zstd"])
def test_offset_index_matches_the_scanned_page_table(dec, compression, version):
    """The OffsetIndex of every chunk against the page table of the scanned GPU decode (which, unlike the
    oracle, reads ZSTD): offset, size, and first_row of the flat columns."""
    data, _ = fixture_file(compression, version)
    pf = pqgpu.ParquetFile(data)
    dev = dec.upload(pf.data)
    try:
        res = dec.decode_jobs([pqgpu.device_job(pf, 0, c, dev) for c in range(3)])
        for c, r in enumerate(res):
            m, pi = pf.chunk_meta(0, c), pf.page_index(0, c)
            pages = [p for p in dec.pages(c, 4096) if p.page_type != abi.PAGE_DICTIONARY]
            if r.status != 0:
                pages = pages[:-1]  # the pages before the one the scan stopped at
            assert r.status != 0 or len(pages) == len(pi.locations)
            for p, (off, size, first_row) in zip(pages, pi.locations):
                assert off == m.start + p.header_offset
                assert size == p.payload_offset - p.header_offset + p.compressed_size
                assert c == 2 or first_row == p.slot_offset
    finally:
        dec.free(dev)


def test_reader_rows_without_a_column_index(dec):
    """An OffsetIndex alone: rows= still lists only the pages of its range; filters prune nothing."""
    pa = pytest.importorskip("pyarrow")
    pq = pytest.importorskip("pyarrow.parquet")
    n = 20000
    buf = io.BytesIO()
    pq.write_table(pa.table({"a": pa.array(np.arange(n, dtype=np.int64))}), buf, data_page_size=4096,
                   write_page_index=True, write_statistics=False)
    data = buf.getvalue()
    full = pqgpu.FileReader(data, decoder=dec).read_row_group(0)
    fr = pqgpu.FileReader(data, decoder=dec, use_page_index=True)
    assert fr.file.page_index(0, 0).null_pages is None
    got = fr.read_row_group(0, rows=(3000, 3100))
    assert col_tuple(got["a"]) == slice_col(full["a"], 3000, 3100)
    assert 0 < fr.last_read["pages_decoded"] <= 2 < fr.last_read["pages_total"]
    got = fr.read_row_group(0, filters=[("a", "<", 10)])
    assert got["a"].num_slots == 10
    assert fr.last_read["pages_decoded"] == fr.last_read["pages_total"] and fr.last_read["row_ranges"] == [(0, n)]
