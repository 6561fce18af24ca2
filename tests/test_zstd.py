"""ZSTD column chunks on the GPU (K2z, pqg_zstd.hip): pqg_block_decompress on
every cell of the format libzstd's encoder emits, hand-built frames, the
lane / batch shapes and seeded mutations (the verdict must be libzstd's, as in
test_zstd_model.py); pyarrow-written ZSTD files against pyarrow's own columns
and against the oracle's decode of a twin file written uncompressed; hand-built
pages; and a ZSTD file through FileReader.  The oracle answers UNSUPPORTED for
ZSTD, so nothing here asks it to decode a ZSTD chunk."""
import ctypes as C
import io

import numpy as np
import pytest

import pqtest_util as U
import zstd_util as Z
from oracle import pyoracle as O
from pqgpu import abi

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")

ZSTD = abi.STATUS_CODES["ZSTD"]

# the (input, level) pairs that between them pass through every cell of Z.CELLS
BLOCK_CASES = [("text", -5), ("text", 1), ("text", 3), ("text", 9), ("text", 19), ("text3000", 3), ("text200", 1),
               ("text200", 19), ("random", 3), ("constant", 3), ("arange", 1), ("arange", 9), ("arange", 19),
               ("arange", 22), ("small_range", 1), ("small_range", 9), ("coin", 3), ("rle_literals", 19),
               ("rle_literals", 1), ("three_symbols", 3), ("tokens", 1), ("tokens", 9), ("tokens", 19),
               ("two_blocks", 3), ("two_blocks", 19)]
VALID_HAND = ["checksum_ok", "no_fcs_window", "single_fcs1", "fcs8", "skip_first", "skip_between", "skip_last",
              "two_frames", "three_frames", "empty_frame", "empty_last_block", "rle_only", "dict_id_zero",
              "block_128k_plus_1"]
INVALID_HAND = ["checksum_bad", "dict_id", "reserved_bit", "block_type3", "fcs_mismatch", "window_too_large",
                "trailing1", "trailing2", "trailing3", "truncated_header", "truncated_block", "bad_magic"]
SEQ_COUNTS = [63, 64, 65, 127, 128, 129]


def _block_case(name):
    """name -> (raw, frame)"""
    if name.startswith("hand:"):
        z, content = Z.hand_frames()[name[5:]]
        return content, z
    if name.startswith("shape:"):
        raw = Z.lane_shapes()[name[6:]]
        return raw, Z.compress(raw, 3)
    if name.startswith("seqs:"):
        z, raw = Z.seq_count_frame(int(name[5:]))
        return raw, z
    inp, lvl = name.rsplit("@", 1)
    raw = Z.corpus()[inp]
    return raw, Z.compress(raw, int(lvl))


BLOCK_NAMES = ["%s@%d" % c for c in BLOCK_CASES] + ["hand:" + n for n in VALID_HAND] + \
    ["shape:" + n for n in sorted(Z.lane_shapes().keys())] + ["seqs:%d" % k for k in SEQ_COUNTS]


@pytest.fixture(scope="module")
def dec():
    import pqgpu
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


def _gpu_block(dec, src, cap):
    dst = np.zeros(max(cap, 1), np.uint8)
    n = C.c_int64(0)
    rc = dec.L.pqg_block_decompress(dec.ctx, abi.CODEC_ZSTD, src, len(src), dst.ctypes.data, cap, C.byref(n))
    return rc, n.value, dst


def test_block_cases_cover_every_cell():
    """The GPU block cases are a covering set (checked on the host model)."""
    seen = {c: 0 for c in Z.CELLS}
    for name, lvl in BLOCK_CASES:
        r = Z.model(Z.compress(Z.corpus()[name], lvl), want_bytes=False)
        for c in Z.CELLS:
            seen[c] += r[c]
    assert all(seen.values()), [c for c, v in seen.items() if not v]


@pytest.mark.gpu
@pytest.mark.parametrize("name", BLOCK_NAMES)
def test_gpu_zstd_block(dec, name):
    raw, z = _block_case(name)
    assert Z.libzstd(z, len(raw)) == raw
    rc, n, dst = _gpu_block(dec, z, len(raw) + 100)
    assert rc == 0, abi.status_name(rc)
    assert n == len(raw) and dst[:n].tobytes() == raw
    if raw:  # a too small output buffer: the length, nothing written
        rc, n, dst = _gpu_block(dec, z, len(raw) - 1)
        assert rc == abi.ERR_CAPACITY and n == len(raw)
        assert not dst.any()


def _corruptions():
    """name -> (frame, n): targeted corruptions of compressed blocks, found with the model's counters."""
    c = Z.corpus()
    out = {}

    def first_block(z):
        # frame header size (single segment or not, FCS) -> offset of the first block's payload
        fhd = z[4]
        fcs = {0: 1 if fhd & 0x20 else 0, 1: 2, 2: 4, 3: 8}[fhd >> 6]
        return 5 + (0 if fhd & 0x20 else 1) + fcs + 3

    # a direct-weights Huffman tree whose weights do not sum to a power of two
    raw = c["three_symbols"]
    z = bytearray(Z.compress(raw, 3))
    assert Z.model(bytes(z), want_bytes=False)["huf_direct"] == 1
    b = first_block(z)
    lh = {0: 3, 1: 3, 2: 4, 3: 5}[(z[b] >> 2) & 3]
    assert z[b] & 3 == 2 and z[b + lh] >= 128
    assert z[b + lh] == 129  # two weights in one byte; the third is implied
    z[b + lh + 1] = 0x31    # 2^2 + 2^0 = 5: what is left to 8 is no power of two
    out["weight_sum"] = (bytes(z), len(raw))
    # FSE table descriptions: an accuracy log past the table's limit (low 4 bits of the first byte = log - 5)
    raw = c["text3000"]
    z0 = Z.compress(raw, 3)
    r = Z.model(z0, want_bytes=False)
    assert r["ll_fse"] == 1 and r["lit_huf4"] == 1 and r["huf_fse"] == 1 and r["blk_comp"] == 1
    b = first_block(z0)
    lhs = {0: 3, 1: 3, 2: 4, 3: 5}[(z0[b] >> 2) & 3]
    v = int.from_bytes(z0[b:b + 4], "little")
    csize = (v >> 14) & 0x3ff if lhs == 3 else v >> 18
    seq = b + lhs + csize  # sequences section
    nb = 1 if z0[seq] < 128 else 2
    assert z0[seq + nb] >> 6 == 2  # LL table FSE-compressed
    z = bytearray(z0)
    z[seq + nb + 1] |= 0x0f  # accuracy log 20
    out["accuracy_log"] = (bytes(z), len(raw))
    z = bytearray(z0)
    z[b + lhs + 1] |= 0x0f  # the Huffman weights' FSE table: accuracy log 20 (limit 6)
    out["weights_accuracy_log"] = (bytes(z), len(raw))
    # treeless literals with no table before them, Repeat mode with no table before it
    z = bytearray(z0)
    z[b] |= 3
    out["treeless_without_table"] = (bytes(z), len(raw))
    z = bytearray(z0)
    z[seq + nb] |= 0xc0
    out["repeat_without_table"] = (bytes(z), len(raw))
    # the sequence bitstream not consumed exactly: one more / one less sequence than it holds
    z = bytearray(z0)
    z[seq + nb - 1] = (z[seq + nb - 1] - 1) & 0xff
    out["bitstream_left_over"] = (bytes(z), len(raw))
    # literal sizes that disagree: the regenerated size one more than the streams hold (and the sequences use)
    z = bytearray(z0)
    v2 = int.from_bytes(z[b:b + 3], "little") + (1 << 4)
    z[b:b + 3] = v2.to_bytes(3, "little")
    out["literal_size"] = (bytes(z), len(raw))
    # compressed size of the literals past the block
    z = bytearray(z0)
    z[b + 2] |= 0xfc
    out["literal_csize"] = (bytes(z), len(raw))
    # an offset past the start of the output: the first sequence of a hand-made block
    # (raw literals "ab", one sequence: ll 2, offset 3 + ..., predefined tables)
    blk = bytes([2 << 3 | 0]) + b"ab" + bytes([1, 0x00]) + bytes([0x00, 0x06, 0x01])
    out["offset_past_start"] = (struct_frame(blk, 16), 16)
    # a stream cut inside the block, the block header left as it is
    out["truncated_block_body"] = (z0[:len(z0) // 2], len(raw))
    return out


def struct_frame(comp_block, fcs):
    """A single-segment frame of one compressed block."""
    return Z.struct.pack("<IBB", Z.MAGIC, 0x20, fcs) + Z.block(2, comp_block, True)


ERROR_NAMES = ["hand:" + n for n in INVALID_HAND] + ["weight_sum", "accuracy_log", "weights_accuracy_log",
                                                      "treeless_without_table", "repeat_without_table",
                                                      "bitstream_left_over", "literal_size", "literal_csize",
                                                      "offset_past_start", "truncated_block_body"]


def test_corruptions_fail_in_libzstd_and_model():
    co = _corruptions()
    assert sorted(co) == sorted(n for n in ERROR_NAMES if not n.startswith("hand:"))
    for name, (z, n) in co.items():
        assert Z.libzstd(z, n) is None, name
        assert Z.model(z, cap=n, want_bytes=False)["status"] == ZSTD, name


@pytest.mark.gpu
@pytest.mark.parametrize("how", ERROR_NAMES)
def test_gpu_zstd_block_errors(dec, how):
    if how.startswith("hand:"):
        z, content = Z.hand_frames()[how[5:]]
        n = len(content)
    else:
        z, n = _corruptions()[how]
    assert Z.libzstd(z, n) is None
    rc, _, _ = _gpu_block(dec, z, n + 64)
    assert rc == ZSTD, abi.status_name(rc)


@pytest.mark.gpu
def test_gpu_zstd_mutations(dec):
    """200 of the seeded mutations on the three smallest frames: libzstd's verdict, and its bytes."""
    frames = sorted(Z.mutation_frames(), key=lambda f: len(f[1]))[:3]
    muts = Z.mutations(200, frames, seed=321)
    n_ok = 0
    for i, (f, z) in enumerate(muts):
        raw = frames[f][0]
        ref = Z.libzstd(z, len(raw))
        rc, n, dst = _gpu_block(dec, z, len(raw))
        if ref is None:
            # a decode to another length is a failure on both sides
            assert rc != 0 or n != len(raw), (i, f, n)
            assert rc in (0, ZSTD, abi.ERR_CAPACITY), (i, abi.status_name(rc))
        else:
            n_ok += 1
            assert rc == 0 and n == len(raw) and dst[:n].tobytes() == ref, (i, f, abi.status_name(rc), n)
    assert 5 < n_ok < 195


# ---- files -----------------------------------------------------------------

def _table():
    rng = np.random.default_rng(31)
    n = 30000
    words = ["g%04d" % i for i in range(300)]
    # the four columns of the GZIP file test, compressible enough that pyarrow compresses every V2 page
    # (periodic dictionary indices: random ones do not shrink, and pyarrow then stores the page raw)
    return pa.table({
        "i64": pa.array(rng.integers(0, 1 << 12, n)),
        "f64": pa.array(np.round(rng.standard_normal(n), 1)),
        "o32": pa.array([None if i % 7 == 0 else (i % 37) * 27 for i in range(n)], type=pa.int32()),
        "s": pa.array([words[(i * i) % 300] for i in range(n)]),
    })


def _write(t, **kw):
    buf = io.BytesIO()
    pq.write_table(t, buf, **kw)
    return buf.getvalue()


def _decode_file(dec, data):
    """Every chunk of a file on the GPU: [((rg, col), DecodedColumn)]"""
    import pqgpu
    pf = pqgpu.ParquetFile(data)
    dev = dec.upload(pf.data)
    try:
        jobs, keys = [], []
        for rg in range(pf.num_row_groups):
            for c in range(pf.num_columns):
                jobs.append(pqgpu.device_job(pf, rg, c, dev))
                keys.append((rg, c))
        res = dec.decode_jobs(jobs)
        return pf, [(k, dec.download(r, i)) for i, (k, r) in enumerate(zip(keys, res))]
    finally:
        dec.free(dev)


def _check_against_twin(dec, zdata, twin, t=None):
    """The GPU's decode of the ZSTD file against the oracle's decode of its
    uncompressed twin (and pyarrow's own columns when t is given)."""
    import pqgpu
    import parity as P
    pf, got = _decode_file(dec, zdata)
    pt = pqgpu.ParquetFile(twin)
    assert (pt.num_row_groups, pt.num_columns) == (pf.num_row_groups, pf.num_columns)
    for (rg, c), g in got:
        assert pf.chunk_meta(rg, c).codec == abi.CODEC_ZSTD and pt.chunk_meta(rg, c).codec == 0
        assert g.status == 0, ("rg%d col%d" % (rg, c), abi.status_name(g.status), g.error_page)
        exp = P.oracle_chunk(pt, rg, c)
        assert exp.status == 0
        # the twin's page table: page count, type, encoding, num_values, usize
        assert len(g.pages) == len(exp.pages), (rg, c)
        for a, b in zip(g.pages, exp.pages):
            assert (a.page_type, a.encoding, a.num_values, a.uncompressed_size) == \
                (b.page_type, b.encoding, b.num_values, b.uncompressed_size)
        P.compare_chunk(exp, g, "rg%d col%d" % (rg, c))
    return pf, got


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 19])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_gpu_pyarrow_zstd_file(dec, version, level):
    t = _table()
    kw = dict(data_page_version=version, data_page_size=64 * 1024, use_dictionary=["s", "o32"])
    zdata = _write(t, compression="zstd", compression_level=level, **kw)
    twin = _write(t, compression="none", **kw)
    pf, got = _check_against_twin(dec, zdata, twin)
    for (rg, c), g in got:
        # no V2 page left uncompressed by the writer (is_compressed=false keeps csize == usize, and the
        # GPU, ignoring the flag as the reference does, would have failed the chunk above: Q4)
        v2 = [p for p in g.pages if p.page_type == abi.PAGE_DATA_V2]
        assert (len(v2) > 0) == (version == "2.0")
        assert all(p.compressed_size != p.uncompressed_size for p in v2), (rg, c)
        col = t.column(c).combine_chunks()
        vals = col.drop_null()
        if c == 3:
            offs = np.asarray(g.offsets)
            chars = np.asarray(g.values)
            assert [bytes(chars[offs[i]:offs[i + 1]]).decode() for i in range(len(offs) - 1)] == vals.to_pylist()
        else:
            dt = {0: np.int64, 1: np.float64, 2: np.int32}[c]
            assert np.array_equal(np.asarray(g.values).view(dt), np.asarray(vals.to_numpy()).astype(dt))
        if c == 2:
            assert np.array_equal(np.asarray(g.def_levels) != 0, np.asarray(col.is_valid()))


@pytest.mark.gpu
def test_gpu_zstd_many_pages(dec):
    """Many ZSTD pages in one batch (the k_zstd queue)."""
    rng = np.random.default_rng(32)
    n = 400_000
    t = pa.table({"a": pa.array(rng.integers(0, 1 << 20, n)),
                  "b": pa.array(np.repeat(rng.standard_normal(n // 8), 8)),
                  "c": pa.array([None if x % 5 == 0 else int(x) for x in rng.integers(0, 40, n)], type=pa.int32())})
    kw = dict(data_page_size=16 * 1024, row_group_size=150_000)
    pf, got = _check_against_twin(dec, _write(t, compression="zstd", **kw), _write(t, compression="none", **kw))
    assert pf.num_row_groups == 3 and sum(len(g.pages) for _, g in got) > 100


def _chunk_gpu(dec, chunk, **kw):
    keep = []
    job, buf = U.chunk_job(chunk, keep=keep, **kw)
    dev = dec.upload(buf)
    try:
        job.data = dev
        r = dec.decode_jobs([job])[0]
        return dec.download(r, 0)
    finally:
        dec.free(dev)


def _zpage(raw, z, nvals, usize=None):
    return U.page_header_v1(len(raw) if usize is None else usize, len(z), nvals, abi.ENC_PLAIN) + z


def _plain_page(raw, nvals):
    return U.page_header_v1(len(raw), len(raw), nvals, abi.ENC_PLAIN) + raw


def _oracle_plain(raw, nvals):
    """The oracle's decode of the page's uncompressed twin."""
    keep = []
    job, _ = U.chunk_job(_plain_page(raw, nvals), ptype=abi.INT64, codec=0, keep=keep)
    return O.decode_chunk(job)


@pytest.mark.gpu
def test_gpu_zstd_mixed_batch(dec):
    """One pqg_decode_chunks call with ZSTD, GZIP, SNAPPY and uncompressed chunks."""
    import pqgpu
    import parity as P
    rng = np.random.default_rng(33)
    t = pa.table({"a": pa.array(rng.integers(0, 1 << 10, 50000)), "b": pa.array(np.repeat(rng.standard_normal(5000), 10))})
    files = {k: _write(t, compression=k, data_page_size=32 * 1024) for k in ("zstd", "gzip", "snappy", "none")}
    pfs = {k: pqgpu.ParquetFile(v) for k, v in files.items()}
    devs = {k: dec.upload(pf.data) for k, pf in pfs.items()}
    try:
        jobs, keys = [], []
        for k, pf in pfs.items():
            for c in range(pf.num_columns):
                jobs.append(pqgpu.device_job(pf, 0, c, devs[k]))
                keys.append((k, c))
        assert {j.col.codec for j in jobs} == {0, 1, 2, 6}
        res = dec.decode_jobs(jobs)
        for i, ((k, c), r) in enumerate(zip(keys, res)):
            g = dec.download(r, i)
            exp = P.oracle_chunk(pfs["none" if k == "zstd" else k], 0, c)
            P.compare_chunk(exp, g, "%s col%d" % (k, c))
            assert g.status == 0
    finally:
        for d in devs.values():
            dec.free(d)


def _hand_bodies():
    v = (np.arange(6000, dtype=np.int64) * 7) % 1000
    raw = v.tobytes()
    rawf = lambda x: (0, x, None)  # noqa: E731
    return raw, {
        "one_frame": Z.compress(raw, 3),
        "multi_frame": Z.compress(raw[:16000], 3) + Z.skippable(b"pad") + Z.compress(raw[16000:], 19),
        "checksum": Z.frame([rawf(raw[:20000]), rawf(raw[20000:])], raw, fcs_bytes=4, checksum=True),
        "raw_block": Z.frame([rawf(raw)], raw),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_frame", "multi_frame", "checksum", "raw_block", "rle_block"])
def test_gpu_zstd_hand_pages(dec, name):
    import parity as P
    raw, bodies = _hand_bodies()
    if name == "rle_block":
        raw = b"\x00" * 8000
        z = Z.frame([(1, b"\x00", 8000)], raw, fcs_bytes=2)
    else:
        z = bodies[name]
    assert Z.libzstd(z, len(raw)) == raw
    nv = len(raw) // 8
    got = _chunk_gpu(dec, _zpage(raw, z, nv), ptype=abi.INT64, codec=abi.CODEC_ZSTD)
    exp = _oracle_plain(raw, nv)
    assert exp.status == 0
    P.compare_chunk(exp, got, name)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["size_more", "size_less", "corrupt", "truncated", "trailing", "empty", "v2_uncompressed"])
def test_gpu_zstd_page_errors(dec, how):
    """A three-page chunk whose second page is bad: the status and the error page."""
    raw = (np.arange(3000, dtype=np.int64) % 97).tobytes()
    z = Z.compress(raw, 3)
    good = _zpage(raw, z, 3000)
    want = ZSTD
    if how == "size_more":
        bad, want = _zpage(raw, z, 3000, usize=len(raw) + 8), abi.STATUS_CODES["SIZE"]
    elif how == "size_less":
        bad, want = _zpage(raw, z, 3000, usize=len(raw) - 8), abi.STATUS_CODES["SIZE"]
    elif how == "corrupt":
        zb = bytearray(z)
        zb[len(zb) // 2] ^= 0x55
        zb[len(zb) // 2 + 1] ^= 0xaa
        assert Z.libzstd(bytes(zb), len(raw)) is None
        bad = _zpage(raw, bytes(zb), 3000)
    elif how == "truncated":
        bad = _zpage(raw, z[:-7], 3000)
    elif how == "trailing":
        bad = _zpage(raw, z + b"\x00\x01", 3000)
    elif how == "empty":
        bad = _zpage(raw, b"", 3000)
        want = abi.STATUS_CODES["SIZE"]  # no frame: zero bytes decoded, not the page's size
    else:
        # Q4: a V2 page stored raw with is_compressed=false is decompressed all the same
        bad = U.page_header_v2(len(raw), len(raw), 3000, 0, 3000, abi.ENC_PLAIN, 0, 0, is_comp=False) + raw
    got = _chunk_gpu(dec, good + bad + good, ptype=abi.INT64, codec=abi.CODEC_ZSTD)
    assert got.status == want, (abi.status_name(got.status), abi.status_name(want))
    assert got.error_page == 1


@pytest.mark.gpu
def test_gpu_zstd_far_window(dec):
    """One 3 MiB page whose second half repeats the first: matches more than
    1 MiB back, in multi-block, windowed frames."""
    import parity as P
    rng = np.random.default_rng(35)
    half = rng.integers(0, 256, 3 << 19, dtype=np.uint8).tobytes()
    raw = half + half
    z = Z.compress(raw, 3)  # a 2 MiB window: a frame with a window descriptor, the second half found 1.5 MiB back
    r = Z.model(z, want_bytes=False)
    assert r["status"] == 0 and r["frame_multi_block"] == 1 and r["frame_window"] == 1
    assert r["match_bytes"] > (1 << 20) and len(z) < 2 << 20
    nv = len(raw) // 8
    got = _chunk_gpu(dec, _zpage(raw, z, nv), ptype=abi.INT64, codec=abi.CODEC_ZSTD)
    exp = _oracle_plain(raw, nv)
    P.compare_chunk(exp, got, "far window")
    assert got.status == 0


@pytest.mark.gpu
def test_zstd_filereader(tmp_path):
    """A pyarrow ZSTD file with an optional int32, a string and a list<string>
    column through FileReader: rows and the nested export equal pyarrow's."""
    import pqgpu
    rng = np.random.default_rng(36)
    n = 5000
    words = ["tag%03d" % i for i in range(200)]
    o32 = [None if x % 6 == 0 else int(x) for x in rng.integers(0, 5000, n)]
    s = [words[int(i)] for i in rng.integers(0, 200, n)]
    ls = [None if k == 7 else [words[int(j)] for j in rng.integers(0, 200, k)] for k in rng.integers(0, 8, n)]
    t = pa.table({"o32": pa.array(o32, type=pa.int32()), "s": pa.array(s), "ls": pa.array(ls, type=pa.list_(pa.string()))})
    path = str(tmp_path / "z.parquet")
    pq.write_table(t, path, compression="zstd", row_group_size=2000, data_page_size=8 * 1024)
    assert pq.ParquetFile(path).metadata.row_group(0).column(0).compression == "ZSTD"
    _filereader_check(pqgpu, path, t)


def _filereader_check(pqgpu, path, t):
    dec = pqgpu.GpuDecoder(0)
    try:
        fr = pqgpu.FileReader(path, "o32", "s", decoder=dec)
        rows = []
        while True:
            try:
                rows.append(fr.next_row())
            except EOFError:
                break
        want = [{k: (v.encode() if isinstance(v, str) else v) for k, v in r.items() if v is not None}
                for r in t.select(["o32", "s"]).to_pylist()]
        assert rows == want
        fr = pqgpu.FileReader(path, "ls", decoder=dec)
        ref = pq.ParquetFile(path)
        assert ref.metadata.num_row_groups == 3
        enc = lambda x: x.encode() if isinstance(x, str) else ([enc(y) for y in x] if isinstance(x, list) else x)  # noqa: E731
        for rg in range(3):
            got = fr.read_row_group_nested(rg)
            assert set(got) == {"ls.list.element"}
            assert got["ls.list.element"].to_pylist() == enc(ref.read_row_group(rg).column("ls").to_pylist())
    finally:
        dec.close()
