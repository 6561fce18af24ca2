"""LZ4_RAW column chunks on the GPU (K2l, pqg_lz4.hip), every case on both of
its decoders (k_lz4, one sequence at a time; k_lz4_batch, 64 sequences parsed
ahead and executed together: the sequence counts 63 .. 129 straddle its batch,
literal lengths 32 / 33 its longest batched run): pqg_block_decompress
on hand-built blocks at every boundary of the format, of k_lz4's LDS window
and of its lane copies, on invalid blocks and on seeded mutations; hand-built
V1 / V2 pages; pyarrow-written lz4 files against pyarrow's own columns and
against the oracle's decode of a twin file written uncompressed.  The judge
here is the host model (tools/lz4_model.cpp), which test_lz4_model.py ties to
liblz4; the oracle answers UNSUPPORTED for LZ4_RAW, so nothing here asks it to
decode an LZ4 chunk."""
import ctypes as C
import io

import numpy as np
import pytest

import pqtest_util as U
import lz4_util as Z
from oracle import pyoracle as O
from pqgpu import abi

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")

CODEC = 7
HAND = sorted(Z.hand_blocks().keys())
CORPUS = sorted(Z.corpus().keys())
BAD = sorted(Z.bad_blocks().keys())


@pytest.fixture(scope="module", params=["step_a", "step_b"])
def dec(request):
    """A decode context for each of pqg_lz4.hip's decoders: k_lz4 (one sequence at a time) and
    k_lz4_batch (64 sequences parsed ahead and executed together); a context reads PQG_LZ4_BATCH
    when it is created."""
    import os
    import pqgpu
    old = os.environ.get("PQG_LZ4_BATCH")
    os.environ["PQG_LZ4_BATCH"] = "1" if request.param == "step_b" else "0"
    try:
        d = pqgpu.GpuDecoder(0)
    finally:
        if old is None:
            del os.environ["PQG_LZ4_BATCH"]
        else:
            os.environ["PQG_LZ4_BATCH"] = old
    yield d
    d.close()


def _gpu_block(dec, src, cap):
    dst = np.zeros(max(cap, 1), np.uint8)
    n = C.c_int64(-7)
    rc = dec.L.pqg_block_decompress(dec.ctx, CODEC, bytes(src), len(src), dst.ctypes.data, cap, C.byref(n))
    return rc, n.value, dst


def _write(t, **kw):
    buf = io.BytesIO()
    pq.write_table(t, buf, **kw)
    return buf.getvalue()


# ---- the codec number -------------------------------------------------------

@pytest.mark.parametrize("name", ["lz4", "lz4_raw"])
def test_pyarrow_lz4_is_codec_7(name):
    """Both of pyarrow's names for it put LZ4_RAW (7) into ColumnMetaData.codec, never the Hadoop-framed 5."""
    import pqgpu
    t = pa.table({"a": pa.array(np.arange(1000) // 7)})
    data = _write(t, compression=name)
    assert pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0).column(0).compression == "LZ4"
    assert pqgpu.ParquetFile(data).chunk_meta(0, 0).codec == abi.CODEC_LZ4_RAW == CODEC


# ---- bare blocks ------------------------------------------------------------

def _valid_case(name):
    if name.startswith("corpus:"):
        raw = Z.corpus()[name[7:]]
        return Z.compress(raw), raw
    return Z.hand_blocks()[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", HAND + ["corpus:" + n for n in CORPUS])
def test_gpu_lz4_block(dec, name):
    z, raw = _valid_case(name)
    rc, n, dst = _gpu_block(dec, z, len(raw) + 100)
    assert rc == 0, abi.status_name(rc)
    assert n == len(raw) and dst[:n].tobytes() == raw
    assert not dst[n:].any()
    if raw:  # a too small output buffer: the length, nothing written
        rc, n, dst = _gpu_block(dec, z, len(raw) - 1)
        assert rc == abi.ERR_CAPACITY and n == len(raw)
        assert not dst.any()


@pytest.fixture(scope="module")
def bad_verdicts():
    """name -> (the model's status as a bare block, as a page of u bytes)"""
    B = Z.bad_blocks()
    res, _ = Z.model_corpus([(None, B[k][0]) for k in BAD] + [B[k][::-1] for k in BAD])
    return {k: (res[i][0], res[len(BAD) + i][0]) for i, k in enumerate(BAD)}


def test_bad_blocks_are_bad(bad_verdicts):
    assert all(page != 0 for _, page in bad_verdicts.values())
    assert {b for b, _ in bad_verdicts.values()} == {0, Z.LZ4}  # some decode as bare blocks, to another length
    assert {p for _, p in bad_verdicts.values()} == {Z.SIZE, Z.LZ4}


@pytest.mark.gpu
@pytest.mark.parametrize("name", BAD)
def test_gpu_lz4_block_errors(dec, bad_verdicts, name):
    z, u = Z.bad_blocks()[name]
    rc, n, dst = _gpu_block(dec, z, u + 64)
    assert rc == bad_verdicts[name][0], abi.status_name(rc)
    if rc == 0:
        assert dst[:n].tobytes() == Z.model(z)["bytes"]


@pytest.mark.gpu
def test_gpu_lz4_block_codec5_unsupported(dec):
    z, _ = Z.hand_blocks()["ml19"]
    dst = np.zeros(256, np.uint8)
    n = C.c_int64(0)
    rc = dec.L.pqg_block_decompress(dec.ctx, 5, z, len(z), dst.ctypes.data, 256, C.byref(n))
    assert rc == abi.STATUS_CODES["UNSUPPORTED"]


# ---- pages ------------------------------------------------------------------

def _decode_chunks(dec, chunks, ptype=None, lead=0, light=False):
    """One pqg_decode_chunks call over hand-built chunks of one upload, chunk k `lead + k` bytes
    past a 256-byte boundary (every alignment of the compressed bytes): [DecodedColumn], or with
    `light` [(status, error page, the values' bytes when the status is 0)] (no page tables fetched)"""
    ptype = abi.INT32 if ptype is None else ptype
    blob, offs = bytearray(), []
    for k, ch in enumerate(chunks):
        blob += bytes(-len(blob) % 256 + (lead + k) % 16)
        offs.append(len(blob))
        blob += ch
    dev = dec.upload(bytes(blob) + bytes(64))
    try:
        jobs = []
        for off, ch in zip(offs, chunks):
            j, _ = U.chunk_job(ch, ptype=ptype, codec=CODEC)
            j.data = dev + off
            jobs.append(j)
        res = dec.decode_jobs(jobs)
        if light:
            return [(r.status, r.error_page, dec.d2h(r.values, r.values_bytes).tobytes() if r.status == 0 else None)
                    for r in res]
        return [dec.download(r, i) for i, r in enumerate(res)]
    finally:
        dec.free(dev)


def _page_v1(z, usize, nvals):
    return U.page_header_v1(usize, len(z), nvals, abi.ENC_PLAIN) + z


@pytest.mark.gpu
def test_gpu_lz4_mutations_bare(dec):
    """300 of the seeded mutations as bare blocks: the model's status, length and bytes."""
    muts = Z.mutations(2000)[:300]
    bare, _ = Z.model_corpus([(None, m) for m in muts])
    assert min(sum(p[0] == s for p in bare) for s in (0, Z.LZ4)) >= 10
    for i, (m, (st, ln, h)) in enumerate(zip(muts, bare)):
        rc, n, dst = _gpu_block(dec, m, 70000)
        assert rc == st, (i, abi.status_name(rc), st)
        if st == 0:
            assert n == ln and Z.fnv(dst[:n].tobytes()) == h, i


@pytest.mark.gpu
def test_gpu_lz4_mutations_pages(dec):
    """The same 300 as pages of the block's size, in one batch: the model's status and bytes."""
    raw, _ = Z.mutation_block()
    muts = Z.mutations(2000)[:300]
    page, _ = Z.model_corpus([(len(raw), m) for m in muts])
    assert min(sum(p[0] == s for p in page) for s in (0, Z.SIZE, Z.LZ4)) >= 10
    got = _decode_chunks(dec, [_page_v1(m, len(raw), len(raw) // 4) for m in muts], light=True)
    for i, ((status, error_page, values), (st, ln, h)) in enumerate(zip(got, page)):
        assert status == st, (i, abi.status_name(status), st)
        if st == 0:
            assert len(values) == ln == len(raw) and Z.fnv(values) == h, i
        else:
            assert error_page == 0, i


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(Z.huge_blocks().keys()))
def test_gpu_lz4_huge_extension_runs(dec, name):
    """An extension run that claims 2^31 bytes ends in a verdict, as a page and as a bare block."""
    z, u, want = Z.huge_blocks()[name]
    g = _decode_chunks(dec, [_page_v1(z, u, u // 4)])[0]
    assert g.status == want, abi.status_name(g.status)
    rc, n, dst = _gpu_block(dec, z, 1 << 20)
    if name == "ext_2g":
        assert rc == Z.LZ4
    else:  # a well-formed block of 2 GiB and some
        assert rc == abi.ERR_CAPACITY and n == 12 + 4 + 15 + (1 << 31) // 255 * 255 + 255 + 17 and not dst.any()


def _decode_page(dec, col, page):
    pj = abi.PageJob()
    pj.col = col
    pp = dec.upload(page)
    pj.page, pj.page_len = pp, len(page)
    pj.dict_page, pj.dict_page_len = None, 0
    r = abi.ChunkResult()
    rc = dec.L.pqg_decode_page(dec.ctx, C.byref(pj), C.byref(r))
    assert rc == 0, rc
    got = dec.download(r, 0)
    dec.free(pp)
    return got


def _col(ptype, max_def=0, codec=CODEC):
    c = abi.ColumnDesc()
    c.physical_type, c.type_length, c.max_def, c.max_rep, c.codec = ptype, -1, max_def, 0, codec
    return c


def _v2_parts():
    """3000 optional int64 slots, 2000 of them values: the def-level bytes (RLE, no length prefix) and the values."""
    defs = U.uvarint(2000 << 1) + b"\x01" + U.uvarint(1000 << 1) + b"\x00"
    vals = ((np.arange(2000, dtype=np.int64) * 7) % 1000).tobytes()
    return defs, vals


def _page(version, vals_z, usize_delta=0):
    """A V1 page of 2000 required int64, or a V2 page of 3000 optional ones with its level bytes raw in front."""
    defs, vals = _v2_parts()
    if version == 1:
        return U.page_header_v1(len(vals) + usize_delta, len(vals_z), 2000, abi.ENC_PLAIN) + vals_z
    return U.page_header_v2(len(defs) + len(vals) + usize_delta, len(defs) + len(vals_z), 3000, 1000, 3000,
                            abi.ENC_PLAIN, len(defs), 0) + defs + vals_z


def _twin(version):
    """The oracle's decode of the page stored uncompressed."""
    _, vals = _v2_parts()
    job, _ = U.chunk_job(_page(version, vals), ptype=abi.INT64, max_def=version - 1, codec=0)
    exp = O.decode_chunk(job)
    assert exp.status == 0
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("version", [1, 2])
def test_gpu_lz4_hand_pages(dec, version):
    import parity as P
    _, vals = _v2_parts()
    z = Z.compress(vals)
    assert len(z) < len(vals) // 2
    exp = _twin(version)
    got = _decode_page(dec, _col(abi.INT64, version - 1), _page(version, z))
    P.compare_chunk(exp, got, "v%d" % version)
    assert got.num_values == 2000 and got.pages[0].status == 0
    # the same bytes, hand-laid: literals only, and the values' period (1000 values) as one long match
    assert vals[8000:] == vals[:8000]
    for zz in (Z.block([], vals), Z.block([(vals[:8000], 8000, 8000 - 17)], vals[-17:])):
        got = _decode_page(dec, _col(abi.INT64, version - 1), _page(version, zz))
        P.compare_chunk(exp, got, "v%d hand" % version)


@pytest.mark.gpu
@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("how", ["size_more", "size_less", "size_more_1", "size_less_1", "corrupt", "truncated",
                                 "trailing", "empty", "offset0"])
def test_gpu_lz4_page_errors(dec, version, how):
    """One bad page on its own, and in the middle of a three-page chunk: the model's class, the error page."""
    _, vals = _v2_parts()
    z = Z.compress(vals)
    delta = {"size_more": 8, "size_less": -8, "size_more_1": 1, "size_less_1": -1}.get(how, 0)
    zb = z
    if how == "corrupt":
        zb = bytearray(z)
        zb[len(zb) // 2] ^= 0x55
        zb[len(zb) // 2 + 1] ^= 0xaa
        zb = bytes(zb)
    elif how == "truncated":
        zb = z[:-7]
    elif how == "trailing":
        zb = z + b"\x00"
    elif how == "empty":
        zb = b""
    elif how == "offset0":  # decodes, to other bytes of the right length: no error to liblz4
        zb = Z.block([(vals[:40], 0, len(vals) - 40 - 17)], vals[-17:])
    want = Z.model(zb, len(vals) + delta, want_bytes=False)["status"]
    assert want == (Z.SIZE if how.startswith("size") else 0 if how == "offset0" else Z.LZ4)
    bad = _page(version, zb, delta)
    got = _decode_page(dec, _col(abi.INT64, version - 1), bad)
    assert got.status == want, (abi.status_name(got.status), abi.status_name(want))
    if want == 0:
        v = np.asarray(got.values).tobytes()
        assert v[:40] == vals[:40] and v[40:-17] == bytes(len(vals) - 57) and v[-17:] == vals[-17:]
        return
    assert got.error_page == 0
    if version == 1:
        good = _page(1, z)
        g = _decode_chunks(dec, [good + bad + good], ptype=abi.INT64, lead=5)[0]
        assert g.status == want and g.error_page == 1


@pytest.mark.gpu
def test_gpu_lz4_page_past_64k(dec):
    """One page of 300 KB whose matches reach 65 535 bytes back all along it: history far past any LDS ring."""
    import parity as P
    rng = np.random.default_rng(41)
    seg = rng.integers(0, 256, 65535, dtype=np.uint8).tobytes()
    seqs = [(seg, 65535, 30000)] + [(rng.integers(0, 256, 9, dtype=np.uint8).tobytes(), 65535 - 9 * (i % 3), 20000 + i)
                                    for i in range(10)]
    z, raw = Z.block(seqs, Z.TAIL + b"\0" * 7), Z.expand(seqs, Z.TAIL + b"\0" * 7)
    raw = raw[:len(raw) // 8 * 8]
    z = Z.block(seqs, (Z.TAIL + b"\0" * 7)[:len(raw) - len(Z.expand(seqs))])
    assert Z.expand(seqs, (Z.TAIL + b"\0" * 7)[:len(raw) - len(Z.expand(seqs))]) == raw and len(raw) > 290_000
    assert Z.model(z, len(raw))["bytes"] == raw
    job, _ = U.chunk_job(U.page_header_v1(len(raw), len(raw), len(raw) // 8, abi.ENC_PLAIN) + raw, ptype=abi.INT64, codec=0)
    exp = O.decode_chunk(job)
    got = _decode_chunks(dec, [_page_v1(z, len(raw), len(raw) // 8)], ptype=abi.INT64, lead=3)[0]
    P.compare_chunk(exp, got, "past 64k")
    assert got.status == 0
    # and pyarrow's own encoder on a page of that size
    raw2 = (raw[:100000] + raw[:100000])[:160000]
    got = _decode_chunks(dec, [_page_v1(Z.compress(raw2), len(raw2), len(raw2) // 8)], ptype=abi.INT64)[0]
    assert got.status == 0 and np.asarray(got.values).tobytes() == raw2


# ---- files ------------------------------------------------------------------

def _table(n=6000):
    rng = np.random.default_rng(42)
    words = ["w%03d" % i for i in range(120)]
    # compressible throughout, so that pyarrow compresses every V2 page (Q4: the flag is ignored)
    return pa.table({
        "o32": pa.array([None if i % 6 == 0 else (i * i % 60) * 27 for i in range(n)], type=pa.int32()),
        "d64": pa.array(np.cumsum(np.repeat(rng.integers(1, 50, n // 16 + 1), 16)[:n]).astype(np.int64)),
        "sd": pa.array([words[(i * i) % 120] for i in range(n)]),
        "sp": pa.array(["row-%06d" % (i // 3) for i in range(n)]),
        "l32": pa.array([None if i % 11 == 0 else [(i + k) % 50 for k in range(i % 5)] for i in range(n)],
                        type=pa.list_(pa.int32())),
    })


def _file_kw(version):
    return dict(data_page_version=version, data_page_size=2048, write_batch_size=256, row_group_size=2500,
                use_dictionary=["o32", "sd"], column_encoding={"d64": "DELTA_BINARY_PACKED", "sp": "PLAIN",
                                                               "l32.list.element": "PLAIN"})


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


@pytest.mark.gpu
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_gpu_pyarrow_lz4_file(dec, version, tmp_path):
    import pqgpu
    import parity as P
    t = _table()
    zdata = _write(t, compression="lz4", **_file_kw(version))
    twin = _write(t, compression="none", **_file_kw(version))
    # 1: every chunk against the oracle's decode of the uncompressed twin
    pf, got = _decode_file(dec, zdata)
    pt = pqgpu.ParquetFile(twin)
    assert (pt.num_row_groups, pt.num_columns) == (pf.num_row_groups, pf.num_columns) == (3, 5)
    npages = 0
    for (rg, c), g in got:
        assert pf.chunk_meta(rg, c).codec == CODEC and pt.chunk_meta(rg, c).codec == 0
        assert g.status == 0 and g.error_page == -1, ((rg, c), abi.status_name(g.status), g.error_page)
        exp = P.oracle_chunk(pt, rg, c)
        assert exp.status == 0 and exp.error_page == g.error_page
        P.compare_chunk(exp, g, "rg%d col%d" % (rg, c))  # levels, values, chars, offsets
        assert len(g.pages) == len(exp.pages)
        for a, b in zip(g.pages, exp.pages):
            assert (a.page_type, a.encoding, a.num_values, a.not_null, a.status, a.uncompressed_size) == \
                (b.page_type, b.encoding, b.num_values, b.not_null, b.status, b.uncompressed_size)
        v2 = [p for p in g.pages if p.page_type == abi.PAGE_DATA_V2]
        assert (len(v2) > 0) == (version == "2.0")
        assert all(p.compressed_size != p.uncompressed_size for p in v2), (rg, c)  # none left raw by the writer
        npages += len(g.pages)
    assert npages > 50
    encs = {c: {p.encoding for (rg, cc), g in got if cc == c for p in g.pages if p.page_type != abi.PAGE_DICTIONARY}
            for c in range(5)}
    assert encs[1] == {abi.ENC_DELTA_BINARY_PACKED} and encs[3] == {abi.ENC_PLAIN}
    assert encs[0] <= {abi.ENC_RLE_DICTIONARY, abi.ENC_PLAIN_DICTIONARY} and encs[0] == encs[2]
    # 2, 3: a path-backed FileReader against pyarrow's own columns, flat and nested
    path = str(tmp_path / "f.parquet")
    open(path, "wb").write(zdata)
    ref = pq.ParquetFile(path)
    fr = pqgpu.FileReader(path, "o32", "d64", "sd", "sp", decoder=dec)
    for rg in range(3):
        cols = fr.read_row_group(rg)
        rt = ref.read_row_group(rg)
        for name, dt in (("o32", np.int32), ("d64", np.int64)):
            col = rt.column(name).combine_chunks()
            assert cols[name].status == 0
            assert np.array_equal(np.asarray(cols[name].values).view(dt), col.drop_null().to_numpy().astype(dt)), name
        assert np.array_equal(np.asarray(cols["o32"].def_levels) != 0, np.asarray(rt.column("o32").combine_chunks().is_valid()))
        for name in ("sd", "sp"):
            offs, chars = np.asarray(cols[name].offsets), np.asarray(cols[name].values).tobytes()
            assert [chars[offs[i]:offs[i + 1]].decode() for i in range(len(offs) - 1)] == rt.column(name).to_pylist()
    # only the selected chunks are uploaded
    sel = sum(pf.chunk_meta(rg, c).total_compressed_size for rg in range(3) for c in range(4))
    assert fr.uploaded_bytes == sel < len(zdata)
    one = pqgpu.FileReader(path, "d64", decoder=dec)
    one.read_row_group(1)
    assert one.uploaded_bytes == pf.chunk_meta(1, 1).total_compressed_size
    fn = pqgpu.FileReader(path, "l32", "sd", decoder=dec)
    for rg in range(3):
        got_n = fn.read_row_group_nested(rg)
        assert set(got_n) == {"l32.list.element", "sd"}
        assert got_n["l32.list.element"].to_pylist() == ref.read_row_group(rg).column("l32").to_pylist()
        assert got_n["sd"].to_pylist() == [s.encode() for s in ref.read_row_group(rg).column("sd").to_pylist()]


@pytest.mark.gpu
def test_gpu_lz4_filereader_rows(dec, tmp_path):
    import pqgpu
    t = _table(3000).select(["o32", "sp"])
    path = str(tmp_path / "r.parquet")
    pq.write_table(t, path, compression="lz4", row_group_size=1100, data_page_size=2048)
    fr = pqgpu.FileReader(path, decoder=dec)
    rows = []
    while True:
        try:
            rows.append(fr.next_row())
        except EOFError:
            break
    want = [{k: (v.encode() if isinstance(v, str) else v) for k, v in r.items() if v is not None} for r in t.to_pylist()]
    assert rows == want


@pytest.mark.gpu
def test_gpu_lz4_file_corrupt_page(dec):
    """A pyarrow file with one byte changed in the middle page of a chunk: the
    chunk fails at that page with the model's verdict on that page's block."""
    import pqgpu
    t = _table(20000).select(["d64"])
    data = bytearray(_write(t, compression="lz4", data_page_version="1.0", data_page_size=2048, write_batch_size=256,
                            use_dictionary=False, column_encoding={"d64": "DELTA_BINARY_PACKED"}))
    pf, got = _decode_file(dec, bytes(data))
    g = got[0][1]
    m = pf.chunk_meta(0, 0)
    assert g.status == 0 and len(g.pages) >= 5
    k = len(g.pages) // 2
    p = g.pages[k]
    lo = m.start + p.payload_offset
    # the first single-byte change the model rejects as malformed, and the first it finds well-formed but short or long
    picks = {}
    for at in range(p.compressed_size):
        block = bytearray(data[lo:lo + p.compressed_size])
        block[at] ^= 0x5f
        want = Z.reference(bytes(block), p.uncompressed_size)[0] if Z.liblz4() else \
            Z.model(bytes(block), p.uncompressed_size, want_bytes=False)["status"]
        if want != 0:
            picks.setdefault(want, at)
        if len(picks) == 2:
            break
    assert set(picks) == {Z.SIZE, Z.LZ4}
    for want, at in picks.items():
        bad = bytearray(data)
        bad[lo + at] ^= 0x5f
        assert Z.model(bytes(bad[lo:lo + p.compressed_size]), p.uncompressed_size, want_bytes=False)["status"] == want
        _, got_bad = _decode_file(dec, bytes(bad))
        gb = got_bad[0][1]
        assert gb.status == want, (at, abi.status_name(gb.status), want)
        assert gb.error_page == k


@pytest.mark.gpu
def test_gpu_lz4_mixed_batch(dec):
    """One pqg_decode_chunks call with LZ4_RAW, ZSTD, GZIP, SNAPPY and uncompressed chunks."""
    import pqgpu
    import parity as P
    rng = np.random.default_rng(43)
    t = pa.table({"a": pa.array(rng.integers(0, 1 << 10, 20000)), "b": pa.array(np.repeat(rng.standard_normal(2000), 10))})
    files = {k: _write(t, compression=k, data_page_size=16 * 1024) for k in ("lz4", "zstd", "gzip", "snappy", "none")}
    pfs = {k: pqgpu.ParquetFile(v) for k, v in files.items()}
    devs = {k: dec.upload(pf.data) for k, pf in pfs.items()}
    try:
        jobs, keys = [], []
        for k, pf in pfs.items():
            for c in range(pf.num_columns):
                jobs.append(pqgpu.device_job(pf, 0, c, devs[k]))
                keys.append((k, c))
        assert {j.col.codec for j in jobs} == {0, 1, 2, 6, 7}
        res = dec.decode_jobs(jobs)
        for i, ((k, c), r) in enumerate(zip(keys, res)):
            g = dec.download(r, i)
            P.compare_chunk(P.oracle_chunk(pfs["none" if k in ("lz4", "zstd") else k], 0, c), g, "%s col%d" % (k, c))
            assert g.status == 0
    finally:
        for d in devs.values():
            dec.free(d)
