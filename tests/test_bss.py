"""BYTE_STREAM_SPLIT data pages on the GPU (k_bss, pqg_bss.hip).  The reference has no decoder for
encoding 9 and the oracle answers UNSUPPORTED for it, so nothing here asks the oracle about a BSS
page.  Expected values come from two places: the numpy model (bss_util.encode / decode, pinned
against pyarrow by test_bss_model.py) for hand-built pages, and the oracle's decode of a PLAIN twin
(the same table written by pyarrow without the encoding, uncompressed, V1; or the same hand-built
chunk with PLAIN pages) for files and for the order of errors.

Statuses (this project's decisions, include/pqgpu.h): value bytes fewer than nn * w: EOF; more: SIZE;
BOOLEAN / INT96 / BYTE_ARRAY / FLBA of type_length 0: UNSUPPORTED."""
import ctypes as C

import numpy as np
import pytest

import bss_util as B
import pqtest_util as U
from oracle import pyoracle as O
from pqgpu import abi

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")

pytestmark = pytest.mark.gpu

EOF, SIZE, UNSUPPORTED = (abi.STATUS_CODES[k] for k in ("EOF", "SIZE", "UNSUPPORTED"))
NNS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 1023, 1024, 1025, 4095, 4097]
# every width as FLBA, and the native types of widths 4 and 8
COLS = {"flba%d" % w: B.flba(w) for w in (1, 2, 3, 4, 8, 12, 16, 17)}
COLS.update(B.TYPES)


@pytest.fixture(scope="module")
def dec():
    import pqgpu
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


def _check(got, values, mask, where):
    assert got.status == 0, (where, abi.status_name(got.status), got.error_page)
    w = got.value_width
    assert got.num_values == len(values) // w, where
    assert np.asarray(got.values).tobytes() == values, where
    if mask is not None:
        assert got.num_slots == len(mask) and np.array_equal(got.def_levels, mask.astype(np.uint8)), where


# ---- hand-built V1 chunks against the model -----------------------------------------------------

@pytest.mark.parametrize("col", sorted(COLS))
def test_gpu_bss_hand_pages(dec, col):
    """Every nn, required and optional (the level prefix puts the value bytes on any offset, and
    nn < num_values), all in one call: pages of different nn share a launch."""
    ptype, tl, w = COLS[col]
    cases = []
    for nn in NNS:
        v = B.random_values(nn, w, 1)
        cases.append((v, None))
        cases.append((B.random_values(nn, w, 2), B.mask_for(nn)))
    got = B.decode_chunks(dec, [(B.page(v, w, m), ptype, tl, 0 if m is None else 1) for v, m in cases], lead=1)
    for k, ((v, m), g) in enumerate(zip(cases, got)):
        assert g.value_width == w
        _check(g, v, m, (col, NNS[k // 2], "optional" if m is not None else "required"))
        assert [(p.encoding, p.not_null) for p in g.pages] == [(B.ENC, len(v) // w)]


@pytest.mark.parametrize("w", [2, 3, 4, 8, 16, 17])
def test_gpu_bss_three_pages(dec, w):
    """Pages of unequal nn in one chunk: the output of pages 2 and 3 starts w-aligned only."""
    ptype, tl, _ = B.flba(w)
    chunks, want = [], []
    for nns, optional in (((17, 1025, 63), False), ((255, 1, 4097), False), ((65, 1023, 15), True)):
        vs = [B.random_values(nn, w, 3 + i) for i, nn in enumerate(nns)]
        ms = [B.mask_for(nn, i) if optional else None for i, nn in enumerate(nns)]
        chunks.append((b"".join(B.page(v, w, m) for v, m in zip(vs, ms)), ptype, tl, int(optional)))
        want.append((b"".join(vs), np.concatenate(ms) if optional else None, nns))
    for g, (v, m, nns) in zip(B.decode_chunks(dec, chunks, lead=7), want):
        _check(g, v, m, (w, nns))
        assert [p.not_null for p in g.pages] == list(nns)


@pytest.mark.parametrize("col", ["float", "double"])
def test_gpu_bss_big_pages(dec, col):
    """Pages past kSplitMin = 65 536 values: parts of 4096 values that begin inside streams of odd stride."""
    ptype, tl, w = B.TYPES[col]
    cases = [(B.random_values(65537, w, 5), None), (B.random_values(70001, w, 6), None),
             (B.random_values(65537, w, 7), B.mask_for(65537))]
    got = B.decode_chunks(dec, [(B.page(v, w, m), ptype, tl, 0 if m is None else 1) for v, m in cases], lead=3)
    for (v, m), g in zip(cases, got):
        _check(g, v, m, (col, len(v) // w))


@pytest.mark.parametrize("w", [2, 3, 4, 8, 16])
def test_gpu_bss_end_of_buffer(dec, w):
    """The last stream's last byte is the last byte of the device buffer (nn = 17)."""
    ptype, tl, _ = B.flba(w)
    v = B.random_values(17, w, 8)
    for lead in (0, 5):
        g = B.decode_chunks(dec, [(B.page(v, w), ptype, tl, 0)], lead=lead, tail=0)[0]
        _check(g, v, None, (w, lead))


# ---- errors -------------------------------------------------------------------------------------

@pytest.mark.parametrize("col", ["flba2", "flba3", "float", "double", "flba16"])
def test_gpu_bss_size_errors(dec, col):
    ptype, tl, w = COLS[col]
    chunks, want = [], []
    for nn in (1, 17, 1025):
        v = B.random_values(nn, w, 9)
        e = B.encode(v, w)
        for val, st in ((e[:-1], EOF), (e + b"\0", SIZE), (e + bytes(w), SIZE), (e, 0)):
            chunks.append((B.page(v, w, val_bytes=val), ptype, tl, 0))
            want.append(st)
            m = B.mask_for(nn)
            chunks.append((B.page(v, w, m, val_bytes=val), ptype, tl, 1))
            want.append(st)
    # no value: nothing is read, whatever follows the levels
    chunks.append((B.page(b"", w, B.mask_for(0), val_bytes=b"\1\2\3"), ptype, tl, 1))
    want.append(0)
    for k, (g, st) in enumerate(zip(B.decode_chunks(dec, chunks), want)):
        assert g.status == st, (k, abi.status_name(g.status), abi.status_name(st))
        if st:
            assert g.error_page == 0 and g.pages[0].status == st


def test_gpu_bss_unsupported_types(dec):
    v = B.random_values(24, 4, 10)
    chunks = [(U.v1_page(v, 24, B.ENC), abi.BOOLEAN, -1, 0), (U.v1_page(v, 8, B.ENC), abi.INT96, -1, 0),
              (U.v1_page(v, 4, B.ENC), abi.BYTE_ARRAY, -1, 0), (U.v1_page(v, 4, B.ENC), abi.FIXED_LEN_BYTE_ARRAY, 0, 0),
              (U.v1_page(B.encode(v, 4), 24, B.ENC), abi.FIXED_LEN_BYTE_ARRAY, 4, 0)]
    got = B.decode_chunks(dec, chunks)
    for g in got[:4]:
        assert g.status == UNSUPPORTED and g.error_page == 0
    _check(got[4], v, None, "flba4 next to them")


def test_gpu_bss_error_order(dec):
    """A short middle page, and a short page next to a page with a bad header (num_values -1): what the
    oracle answers for the same chunks with PLAIN pages (a read error wins over a decode error)."""
    w = 4
    vs = [B.random_values(nn, w, 11 + i) for i, nn in enumerate((100, 200, 300))]
    bad = U.page_header_v1(16, 16, -1, B.ENC) + bytes(16)

    def chunks(enc):
        pages = [B.page(v, w, enc=enc, val_bytes=(B.encode(v, w) if enc == B.ENC else v)) for v in vs]
        short = B.page(vs[1], w, enc=enc, val_bytes=B.encode(vs[1], w)[:-1])
        return [pages[0] + short + pages[2], bad + short, short + bad, pages[0] + short + bad]

    want = []
    for ch in chunks(abi.ENC_PLAIN):
        j, _ = U.chunk_job(ch, ptype=abi.FLOAT)
        e = O.decode_chunk(j)
        want.append((e.status, e.error_page))
    assert want[0] == (EOF, 1) and want[1][1] == 0 and want[2][1] == 1 and want[3][1] == 2
    assert all(st not in (0, EOF) for st, _ in want[1:])
    got = B.decode_chunks(dec, [(ch, abi.FLOAT, -1, 0) for ch in chunks(B.ENC)])
    assert [(g.status, g.error_page) for g in got] == want


def test_gpu_bss_value_byte_flips(dec):
    """100 seeded single-byte changes inside the value bytes: still status 0, the model's bytes."""
    rng = np.random.default_rng(12)
    chunks, want = [], []
    for k in range(100):
        w = (2, 4, 8, 16, 3)[k % 5]
        nn = (17, 255, 1025)[k % 3]
        v = B.random_values(nn, w, 13)
        e = bytearray(B.encode(v, w))
        e[int(rng.integers(0, len(e)))] ^= int(rng.integers(1, 256))
        chunks.append((B.page(v, w, val_bytes=bytes(e)), *B.flba(w)[:2], 0))
        want.append(B.decode(bytes(e), nn, w))
        assert want[-1] != v
    for k, (g, v) in enumerate(zip(B.decode_chunks(dec, chunks, lead=2), want)):
        _check(g, v, None, k)


# ---- pyarrow files against the oracle's decode of their PLAIN twins -------------------------------

def _decode_file(dec, data):
    import pqgpu
    pf = pqgpu.ParquetFile(data)
    dev = dec.upload(pf.data)
    try:
        keys = [(rg, c) for rg in range(pf.num_row_groups) for c in range(pf.num_columns)]
        res = dec.decode_jobs([pqgpu.device_job(pf, rg, c, dev) for rg, c in keys])
        return pf, [(k, dec.download(r, i)) for i, (k, r) in enumerate(zip(keys, res))]
    finally:
        dec.free(dev)


@pytest.fixture(scope="module")
def twins():
    """kind -> (the table, the oracle's decode of the twin file's chunk); computed once."""
    import pqgpu
    import parity as P
    out = {}
    for kind in ("float32", "float64", "int32", "int64", "float16"):
        t = pa.table({"c": B.arrow_array(kind, 5000)})
        pt = pqgpu.ParquetFile(B.write(t, False))
        exp = P.oracle_chunk(pt, 0, 0)
        assert exp.status == 0 and len(exp.pages) >= (2 if kind == "float16" else 3)  # 4096-byte pages
        out[kind] = (t, exp)
    return out


@pytest.mark.parametrize("codec", ["none", "snappy", "gzip", "zstd", "lz4"])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("kind", ["float32", "float64", "int32", "int64", "float16"])
def test_gpu_bss_pyarrow_twin(dec, twins, kind, version, codec):
    t, exp = twins[kind]
    data = B.write(t, True, compression=codec, data_page_version=version)
    pf, got = _decode_file(dec, data)
    g = got[0][1]
    assert {p.encoding for p in g.pages} == {B.ENC}
    where = "%s v%s %s" % (kind, version, codec)
    assert g.status == exp.status == 0 and g.error_page == -1, (where, abi.status_name(g.status), g.error_page)
    assert (g.num_slots, g.num_values) == (exp.num_slots, exp.num_values), where
    assert np.array_equal(g.def_levels, exp.def_levels) and exp.rep_levels is None and g.rep_levels is None, where
    assert np.asarray(g.values).tobytes() == np.asarray(exp.values).tobytes(), where
    # per page; the twin is V1 whatever the file is, so a V2 file's pages differ from it in their type (and only there)
    ptype = abi.PAGE_DATA_V2 if version == "2.0" else abi.PAGE_DATA
    assert [(p.page_type, p.num_values, p.not_null) for p in g.pages] == \
        [(ptype if p.page_type == abi.PAGE_DATA else p.page_type, p.num_values, p.not_null) for p in exp.pages], where
    if kind == "float32":
        assert [p.num_values for p in g.pages] == [2048, 2048, 904]
    if codec != "none":
        assert pf.chunk_meta(0, 0).codec != 0
        if version == "2.0":  # the case cannot pass by never decompressing
            assert any(p.compressed_size < p.uncompressed_size for p in g.pages)


def test_gpu_bss_nested_list(dec, tmp_path):
    """list<float32> leaves through read_row_group_nested, against the same call on the twin."""
    import pqgpu
    rng = np.random.default_rng(14)
    pool = rng.standard_normal(16).astype(np.float32)
    rows = [None if i % 11 == 0 else [float(pool[(i + k) % 16]) for k in range(i % 5)] for i in range(4000)]
    t = pa.table({"l": pa.array(rows, type=pa.list_(pa.float32()))})
    out = {}
    for split in (True, False):
        path = str(tmp_path / ("l%d.parquet" % split))
        open(path, "wb").write(B.write(t, split, compression="zstd"))
        fr = pqgpu.FileReader(path, "l", decoder=dec)
        out[split] = fr.read_row_group_nested(0)["l.list.element"].to_pylist()
    md = pq.ParquetFile(str(tmp_path / "l1.parquet")).metadata.row_group(0).column(0)
    assert "BYTE_STREAM_SPLIT" in md.encodings
    assert out[True] == out[False] == t.column("l").to_pylist()


def test_gpu_bss_filereader_rows(dec, tmp_path):
    """A two-column file through FileReader(path, "col") and next_row(), against the twin."""
    import pqgpu
    t = pa.table({"f": B.arrow_array("float32", 3000), "d": B.arrow_array("float64", 3000, null_every=7, seed=4)})
    got = {}
    for split in (True, False):
        path = str(tmp_path / ("r%d.parquet" % split))
        open(path, "wb").write(B.write(t, split, compression="lz4", row_group_size=1100))
        one = pqgpu.FileReader(path, "d", decoder=dec)
        cols = [one.read_row_group(rg)["d"] for rg in range(3)]
        assert all(c.status == 0 for c in cols)
        fr = pqgpu.FileReader(path, decoder=dec)
        rows = []
        while True:
            try:
                rows.append(fr.next_row())
            except EOFError:
                break
        got[split] = ([np.asarray(c.values).tobytes() for c in cols], [np.asarray(c.def_levels).tobytes() for c in cols], rows)
    assert got[True] == got[False]
    assert len(got[True][2]) == 3000
    want = t.column("d").combine_chunks().drop_null().to_numpy().tobytes()
    assert b"".join(got[True][0]) == want


# ---- the page-level entry ----------------------------------------------------------------------

def test_gpu_bss_decode_page(dec):
    """pqg_decode_page on one BSS page equals the chunk path on the same page."""
    w = 8
    v, m = B.random_values(1025, w, 15), B.mask_for(1025)
    page = B.page(v, w, m)
    chunk = B.decode_chunks(dec, [(page, abi.DOUBLE, -1, 1)])[0]
    pj = abi.PageJob()
    pj.col.physical_type, pj.col.type_length, pj.col.max_def, pj.col.max_rep, pj.col.codec = abi.DOUBLE, -1, 1, 0, 0
    pp = dec.upload(page)
    try:
        pj.page, pj.page_len = pp, len(page)
        pj.dict_page, pj.dict_page_len = None, 0
        r = abi.ChunkResult()
        rc = dec.L.pqg_decode_page(dec.ctx, C.byref(pj), C.byref(r))
        assert rc == 0, rc
        got = dec.download(r, 0)
    finally:
        dec.free(pp)
    _check(got, v, m, "page")
    assert (got.num_slots, got.num_values) == (chunk.num_slots, chunk.num_values)
    assert np.array_equal(got.values, chunk.values) and np.array_equal(got.def_levels, chunk.def_levels)
