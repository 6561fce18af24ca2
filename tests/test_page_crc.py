"""PageHeader.crc verified on the GPU (K1c: k_crc_plan, k_page_crc, k_crc_fin in pqg_crc.hip).

The reference is zlib.crc32 over the page's compressed_size bytes at payload_offset
(test_crc_model.py pins that this is what pyarrow stores) and, for corrupted files, pyarrow's own
reader with page_checksum_verification=True.  CRC-32 detects every single-bit error, so nothing here
has a tolerance.  Page tables are the GPU's own from a decode with verification off (the oracle reads
neither ZSTD nor LZ4_RAW)."""
import ctypes as C
import io
import os
import re
import zlib

import numpy as np
import pytest

import crc_util as K
import pqtest_util as U
from pqgpu import abi

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")

pytestmark = pytest.mark.gpu

CRC, EOF, SIZE = (abi.STATUS_CODES[k] for k in ("CRC", "EOF", "SIZE"))
NONE, VERIFIED, MISMATCH, NOT_CHECKED = abi.CRC_NONE, abi.CRC_VERIFIED, abi.CRC_MISMATCH, abi.CRC_NOT_CHECKED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = int(re.search(r"#define PQG_CRC_TILE (\d+)", open(os.path.join(ROOT, "parquet-go_amd", "csrc", "pqg_crc.h")).read()).group(1))
VERSIONS = ["1.0", "2.0"]
CODECS = ["none", "snappy", "gzip", "zstd", "lz4"]


@pytest.fixture(scope="module")
def dec():
    import pqgpu
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def files():
    """The clean four-column file of every (version, codec), written once."""
    table, kw = K.four_columns(5000)
    return {(v, c): K.write_table(table, v, c, **kw) for v in VERSIONS for c in CODECS}


class Chunk:
    """A column chunk's bytes with what a job needs to know about it."""

    def __init__(self, pf, col):
        job, m = pf.host_job(0, col)
        self.desc = job.col
        self.bytes = bytes(pf.data[m.start:m.start + m.total_compressed_size])
        self.dpo = m.data_page_offset - m.start
        self.has_dict_off = m.has_dict_page_offset
        self.num_values = m.num_values

    def edited(self, data, dpo=None):
        c = Chunk.__new__(Chunk)
        c.__dict__.update(self.__dict__)
        c.bytes = bytes(data)
        if dpo is not None:
            c.dpo = dpo
        return c


def decode(dec, chunks, verify, lead=3, cut=0):
    """One decode call over `chunks`, chunk k at `lead + k` bytes past a 256-byte boundary of one
    upload (payloads then start on any alignment); `cut`: the jobs' bytes end that many bytes before
    the chunk's end.  -> [(DecodedColumn, [PageCrc])]"""
    blob, offs = bytearray(), []
    for k, ch in enumerate(chunks):
        blob += bytes(-len(blob) % 256 + (lead + k) % 16)
        offs.append(len(blob))
        blob += ch.bytes
    dev = dec.upload(bytes(blob) + bytes(64))
    dec.set_verify_crc(verify)
    try:
        jobs = []
        for off, ch in zip(offs, chunks):
            j = abi.ChunkJob()
            j.col = ch.desc
            j.data = dev + off
            j.data_len = j.total_compressed_size = j.total_uncompressed_size = len(ch.bytes) - cut
            j.data_page_offset = ch.dpo
            j.has_dict_page_offset = ch.has_dict_off
            j.num_values_hint = ch.num_values
            jobs.append(j)
        res = dec.decode_jobs(jobs)
        return [(dec.download(r, i), dec.page_crcs(i)) for i, r in enumerate(res)]
    finally:
        dec.set_verify_crc(False)
        dec.free(dev)


def same_outputs(a, b):
    assert (a.status, a.error_page, a.num_slots, a.num_values, a.value_width) == \
        (b.status, b.error_page, b.num_slots, b.num_values, b.value_width)
    for x, y in ((a.values, b.values), (a.def_levels, b.def_levels), (a.rep_levels, b.rep_levels), (a.offsets, b.offsets)):
        assert (x is None) == (y is None)
        assert x is None or np.asarray(x).tobytes() == np.asarray(y).tobytes()
    assert len(a.pages) == len(b.pages)
    for p, q in zip(a.pages, b.pages):
        assert bytes(p) == bytes(q)


def chunks_of(data):
    import pqgpu
    pf = pqgpu.ParquetFile(data)
    return pf, [Chunk(pf, c) for c in range(pf.num_columns)]


def pages_of(dec, ch):
    """The chunk's pages (crc_util.Page) by the GPU's page table of a decode with verification off."""
    got, _ = decode(dec, [ch], False)[0]
    assert got.status == 0
    return K.split_pages(ch.bytes, got.pages), got


# ---- pqg_crc32 against zlib ----------------------------------------------------------------------

def test_gpu_crc32_matches_zlib(dec):
    """Sub-ranges of one uploaded buffer: lengths 0..600 at every start alignment, every length within
    17 of a lane slice, a wave row, one, two and three tiles at 4 alignments."""
    rng = np.random.default_rng(11)
    buf = rng.integers(0, 256, 3 * TILE + 64, dtype=np.uint8).tobytes()
    dev = dec.upload(buf)
    try:
        cases = [(n, al) for al in range(16) for n in range(601)]
        cases += [(n, al) for mk in (256, 1024, TILE, 2 * TILE, 3 * TILE) for al in (0, 1, 7, 15) for n in range(mk - 17, mk + 18)]
        bad = [(n, al) for n, al in cases if dec.crc32(dev + al, n) != zlib.crc32(buf[al:al + n])]
        assert not bad, bad[:10]
        assert dec.crc32(dev, 0) == 0 and dec.crc32(0, 0) == 0
    finally:
        dec.free(dev)


def test_gpu_crc32_many_tiles(dec):
    """4 MiB + 5 bytes from an odd address: the page combine runs over more than 256 tiles."""
    buf = np.random.default_rng(12).integers(0, 256, (4 << 20) + 5 + 3, dtype=np.uint8).tobytes()
    dev = dec.upload(buf)
    try:
        assert dec.crc32(dev + 3, (4 << 20) + 5) == zlib.crc32(buf[3:])
        assert dec.crc32(dev, len(buf)) == zlib.crc32(buf)
    finally:
        dec.free(dev)


# ---- clean files ---------------------------------------------------------------------------------

@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("version", VERSIONS)
def test_gpu_clean_file(dec, files, version, codec):
    pf, chunks = chunks_of(files[version, codec])
    off = decode(dec, chunks, False)
    on = decode(dec, chunks, True)
    top_bit = 0
    for ch, (a, ca), (b, cb) in zip(chunks, off, on):
        assert b.status == 0, (abi.status_name(b.status), b.error_page)
        same_outputs(a, b)
        assert [c.state for c in ca] == [NOT_CHECKED] * len(a.pages) and len(cb) == len(b.pages) >= 2
        pages = K.split_pages(ch.bytes, b.pages)
        for p, c in zip(pages, cb):
            assert p.crc is not None
            assert (c.state, c.stored, c.computed) == (VERIFIED, p.crc, K.crc32(p.payload))
            top_bit += p.crc >> 31
    assert sum(p.page_type == abi.PAGE_DICTIONARY for p in on[2][0].pages) == 1
    assert len(on[0][0].pages) >= 24 and top_bit > 0
    # against pyarrow's values, once per file
    t = pq.read_table(io.BytesIO(files[version, codec]), page_checksum_verification=True)
    assert np.asarray(on[0][0].values).view(np.int32).tolist() == t.column("i32").to_pylist()


def test_gpu_file_without_crc_fields(dec):
    """Verification on, no page carries the field: every state 0, outputs and page table as with it off."""
    table, kw = K.four_columns(5000)
    for version in VERSIONS:
        pf, chunks = chunks_of(K.write_table(table, version, "snappy", checksum=False, **kw))
        for (a, ca), (b, cb) in zip(decode(dec, chunks, False), decode(dec, chunks, True)):
            assert a.status == 0
            same_outputs(a, b)
            assert [c.state for c in ca] == [NOT_CHECKED] * len(a.pages)
            assert [(c.state, c.stored, c.computed) for c in cb] == [(NONE, 0, 0)] * len(b.pages)


# ---- one flipped bit -----------------------------------------------------------------------------

def _targets(pages, table):
    data = [i for i, p in enumerate(table) if p.page_type != abi.PAGE_DICTIONARY]
    t = {"first": data[0], "middle": data[len(data) // 2], "last": data[-1]}
    if table[0].page_type == abi.PAGE_DICTIONARY:
        t["dict"] = 0
    return t


@pytest.mark.parametrize("codec", ["none", "snappy", "zstd"])
@pytest.mark.parametrize("version", VERSIONS)
@pytest.mark.parametrize("col", [0, 2], ids=["int32", "dict_strings"])
def test_gpu_flipped_bit(dec, files, col, version, codec):
    data = files[version, codec]
    pf, chunks = chunks_of(data)
    ch = chunks[col]
    pages, clean = pages_of(dec, ch)
    rng = np.random.default_rng(col + 7)
    cases, bad_chunks = [], []
    for name, k in sorted(_targets(pages, clean.pages).items()):
        n = len(pages[k].payload)
        for at in (0, n - 1, int(rng.integers(0, n))):
            bit = int(rng.integers(0, 8))
            ps = list(pages)
            ps[k] = K.Page(ps[k].header, K.flip(ps[k].payload, at, bit))
            b, dpo = K.join_pages(ps)
            assert len(b) == len(ch.bytes) and dpo == ch.dpo
            cases.append((name, k, at, bit))
            bad_chunks.append(ch.edited(b))
    assert len(cases) == (12 if col == 2 else 9)
    for (name, k, at, bit), (got, crcs) in zip(cases, decode(dec, bad_chunks, True)):
        where = (name, k, at, bit)
        assert (got.status, got.error_page) == (CRC, k), (where, abi.status_name(got.status), got.error_page)
        assert len(crcs) == k + 1 and [c.state for c in crcs] == [VERIFIED] * k + [MISMATCH], where
        bad = K.flip(pages[k].payload, at, bit)
        assert (crcs[k].stored, crcs[k].computed) == (pages[k].crc, K.crc32(bad)), where
    # verification off: whatever these bytes decode to today, and no page is looked at
    for got, crcs in decode(dec, bad_chunks, False):
        assert got.status != CRC and all(c.state == NOT_CHECKED for c in crcs)
    # the reference verdict: pyarrow refuses the same flip (one per target page)
    m = pf.chunk_meta(0, col)
    for name, k, at, bit in cases[::3]:
        b = bytearray(data)
        b[m.start + clean.pages[k].payload_offset + at] ^= 1 << bit
        with pytest.raises(OSError, match="CRC checksum verification failed"):
            pq.read_table(io.BytesIO(bytes(b)), columns=[pf.columns[col].path.decode()], page_checksum_verification=True)


# ---- the stored field instead of the payload ------------------------------------------------------

@pytest.mark.parametrize("version", VERSIONS)
def test_gpu_stored_field_changed(dec, files, version):
    pf, chunks = chunks_of(files[version, "none"])
    ch = chunks[2]  # dictionary strings: page 0 is the dictionary page
    pages, clean = pages_of(dec, ch)
    assert clean.pages[0].page_type == abi.PAGE_DICTIONARY and len(pages) >= 4

    def edit(fn):
        ps = [K.Page(fn(k, p), p.payload) for k, p in enumerate(pages)]
        return ch.edited(*K.join_pages(ps))

    k = 2
    set_top = edit(lambda i, p: K.with_crc(p.header, p.crc | 0x80000000 if not p.crc >> 31 else p.crc & 0x7FFFFFFF) if i == k else p.header)
    zero = edit(lambda i, p: K.with_crc(p.header, 0) if i == k else p.header)
    removed = edit(lambda i, p: K.with_crc(p.header, None) if i == k else p.header)
    dict_only = edit(lambda i, p: p.header if i == 0 else K.with_crc(p.header, None))
    dict_only_bad = edit(lambda i, p: K.with_crc(p.header, p.crc ^ 1) if i == 0 else K.with_crc(p.header, None))
    # the field twice (the second one in the long form, its id spelled out): the last one read counts
    def doubled(p, first, second):
        fs = [f for f in K.header_fields(p.header)[0] if f[0] != 4]
        fs += [(4, K.T_I32, U.zigzag(first)), (4, K.T_I32, U.zigzag(second))]
        return K.build_header(sorted(fs, key=lambda f: f[0]))

    i32 = lambda v: v - (1 << 32) if v >> 31 else v
    twice_bad = edit(lambda i, p: doubled(p, i32(p.crc), 5) if i == k else p.header)
    twice_ok = edit(lambda i, p: doubled(p, 5, i32(p.crc)) if i == k else p.header)
    res = decode(dec, [set_top, zero, removed, dict_only, dict_only_bad, twice_bad, twice_ok], True)
    for got, crcs in res[:2]:
        assert (got.status, got.error_page) == (CRC, k)
        assert [c.state for c in crcs] == [VERIFIED] * k + [MISMATCH] and crcs[k].computed == pages[k].crc
    assert res[0][1][k].stored == pages[k].crc ^ 0x80000000 and res[1][1][k].stored == 0
    got, crcs = res[2]
    same = decode(dec, [removed], False)[0][0]
    same_outputs(same, got)
    assert got.status == 0 and [c.state for c in crcs] == [VERIFIED] * k + [NONE] + [VERIFIED] * (len(pages) - k - 1)
    assert np.asarray(got.values).tobytes() == np.asarray(clean.values).tobytes()
    got, crcs = res[3]
    assert got.status == 0 and [c.state for c in crcs] == [VERIFIED] + [NONE] * (len(pages) - 1)
    got, crcs = res[4]
    assert (got.status, got.error_page) == (CRC, 0) and [c.state for c in crcs] == [MISMATCH]
    got, crcs = res[5]
    assert (got.status, got.error_page, crcs[k].state, crcs[k].stored) == (CRC, k, MISMATCH, 5)
    got, crcs = res[6]
    assert got.status == 0 and (crcs[k].state, crcs[k].stored) == (VERIFIED, pages[k].crc)


# ---- precedence ----------------------------------------------------------------------------------

def test_gpu_crc_error_comes_before_decode_errors(dec, files):
    """A decode error on page 1 (an index past the dictionary, on a page without the field) and a CRC
    mismatch on page 3: the read phase comes first."""
    pf, chunks = chunks_of(files["1.0", "none"])
    ch = chunks[2]
    pages, clean = pages_of(dec, ch)
    assert len(pages) >= 5
    ps = list(pages)
    body = bytearray(ps[1].payload)
    body[-1] = 0x3F  # the last RLE run's value: no such dictionary entry
    ps[1] = K.Page(K.with_crc(ps[1].header, None), body)
    only_decode = ch.edited(*K.join_pages(ps))
    ps[3] = K.Page(ps[3].header, K.flip(ps[3].payload, 5))
    both = ch.edited(*K.join_pages(ps))
    (a, _), (b, cb) = decode(dec, [only_decode, both], True)
    assert a.error_page == 1 and a.status not in (0, CRC)
    assert (b.status, b.error_page) == (CRC, 3)
    assert [c.state for c in cb] == [VERIFIED, NONE, VERIFIED, MISMATCH]
    (a0, _), (b0, _) = decode(dec, [only_decode, both], False)
    assert (a0.status, a0.error_page) == (a.status, 1) == (b0.status, b0.error_page)


def test_gpu_page_past_the_jobs_bytes_keeps_its_status(dec, files):
    pf, chunks = chunks_of(files["1.0", "none"])
    ch = chunks[0]
    (a, ca), = decode(dec, [ch], False, cut=10)
    (b, cb), = decode(dec, [ch], True, cut=10)
    assert a.status in (EOF, SIZE) and (b.status, b.error_page) == (a.status, a.error_page)
    k = b.error_page
    assert k == len(b.pages) - 1 >= 24
    assert [c.state for c in cb] == [VERIFIED] * k + [NOT_CHECKED]


def test_gpu_pages_without_room_in_the_tile_table(files):
    """PQG_CRC_TILE_CAP=2 (a context reads it when it is created) leaves each region of the tile table
    two records, so most pages find no room and k_crc_fin reads them itself: the same verdicts."""
    import pqgpu
    old = os.environ.get("PQG_CRC_TILE_CAP")
    os.environ["PQG_CRC_TILE_CAP"] = "2"
    try:
        d = pqgpu.GpuDecoder(0)
    finally:
        if old is None:
            del os.environ["PQG_CRC_TILE_CAP"]
        else:
            os.environ["PQG_CRC_TILE_CAP"] = old
    try:
        pf, chunks = chunks_of(files["1.0", "none"])
        pages, clean = pages_of(d, chunks[0])
        bad = chunks[0].edited(*K.join_pages(pages[:7] + [K.Page(pages[7].header, K.flip(pages[7].payload, 100, 3))] + pages[8:]))
        res = decode(d, chunks + [bad], True)
        for ch, (got, crcs) in zip(chunks, res):
            assert got.status == 0 and len(crcs) >= 2
            for p, c in zip(K.split_pages(ch.bytes, got.pages), crcs):
                assert (c.state, c.stored, c.computed) == (VERIFIED, p.crc, K.crc32(p.payload))
        got, crcs = res[-1]
        assert (got.status, got.error_page) == (CRC, 7) and [c.state for c in crcs] == [VERIFIED] * 7 + [MISMATCH]
        # one range of three tiles: no room either
        buf = np.random.default_rng(4).integers(0, 256, 3 * TILE + 11, dtype=np.uint8).tobytes()
        dev = d.upload(buf)
        assert d.crc32(dev + 5, 3 * TILE) == zlib.crc32(buf[5:5 + 3 * TILE])
    finally:
        d.close()


# ---- one large page ------------------------------------------------------------------------------

def test_gpu_large_single_page(dec):
    n = 300_000
    vals = np.random.default_rng(3).integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    data = K.write_table(pa.table({"v": pa.array(vals)}), "1.0", "none", data_page_size=1 << 22, write_batch_size=n,
                         max_rows_per_page=n, use_dictionary=False, column_encoding={"v": "PLAIN"})
    pf, (ch,) = chunks_of(data)
    pages, clean = pages_of(dec, ch)
    assert len(pages) == 1 and len(pages[0].payload) >= 4 * n > 73 * TILE  # (+ the def levels of a nullable column)
    at = 39 * TILE + TILE // 2  # inside the 40th tile
    bad = ch.edited(*K.join_pages([K.Page(pages[0].header, K.flip(pages[0].payload, at, 6))]))
    (a, ca), (b, cb) = decode(dec, [ch, bad], True, lead=5)
    assert a.status == 0 and np.asarray(a.values).tobytes() == vals.tobytes()
    assert (ca[0].state, ca[0].stored, ca[0].computed) == (VERIFIED, pages[0].crc, zlib.crc32(pages[0].payload))
    assert (b.status, b.error_page, cb[0].state) == (CRC, 0, MISMATCH)
    assert cb[0].computed == zlib.crc32(K.flip(pages[0].payload, at, 6))


# ---- pqg_decode_page, FileReader -----------------------------------------------------------------

def _decode_page(dec, col, page, dict_page=b""):
    pj = abi.PageJob()
    pj.col = col
    pp = dec.upload(page)
    dp = dec.upload(dict_page) if dict_page else None
    pj.page, pj.page_len = pp, len(page)
    pj.dict_page, pj.dict_page_len = dp, len(dict_page)
    r = abi.ChunkResult()
    rc = dec.L.pqg_decode_page(dec.ctx, C.byref(pj), C.byref(r))
    assert rc == 0, rc
    got = dec.download(r, 0), dec.page_crcs(0)
    for p in (pp, dp):
        if p:
            dec.free(p)
    return got


def test_gpu_decode_page(dec, files):
    pf, chunks = chunks_of(files["2.0", "snappy"])
    ch = chunks[2]
    pages, clean = pages_of(dec, ch)
    d, p = pages[0], pages[2]
    whole = lambda x: x.header + x.payload
    dec.set_verify_crc(True)
    try:
        got, crcs = _decode_page(dec, ch.desc, whole(p), whole(d))
        assert got.status == 0 and got.num_values == clean.pages[2].not_null
        assert [c.state for c in crcs] == [VERIFIED, VERIFIED]
        got, crcs = _decode_page(dec, ch.desc, p.header + K.flip(p.payload, 1), whole(d))
        assert (got.status, got.error_page) == (CRC, 1) and [c.state for c in crcs] == [VERIFIED, MISMATCH]
        got, crcs = _decode_page(dec, ch.desc, whole(p), d.header + K.flip(d.payload, len(d.payload) - 1, 7))
        assert (got.status, got.error_page) == (CRC, 0) and [c.state for c in crcs] == [MISMATCH]
    finally:
        dec.set_verify_crc(False)


def test_gpu_file_reader_raises_crc(dec, files):
    import pqgpu
    data = files["1.0", "snappy"]
    pf, chunks = chunks_of(data)
    pages, clean = pages_of(dec, chunks[0])
    m = pf.chunk_meta(0, 0)
    b = bytearray(data)
    b[m.start + clean.pages[4].payload_offset + 2] ^= 0x10
    try:
        fr = pqgpu.FileReader(bytes(data), "i32", decoder=dec, verify_crc=True)
        assert [r.status for _, _, r in fr.decode_row_groups([0])] == [0]
        fr = pqgpu.FileReader(bytes(b), "i32", decoder=dec, verify_crc=True)
        assert [(r.status, r.error_page) for _, _, r in fr.decode_row_groups([0])] == [(CRC, 4)]
        with pytest.raises(pqgpu.PqgError) as e:
            fr.read_row_group_nested(0)
        assert e.value.code == CRC == -18
    finally:
        dec.set_verify_crc(False)
