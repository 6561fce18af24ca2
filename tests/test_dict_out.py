"""Keep-dictionary decode on the GPU (PQG_COL_KEEP_DICT, K4i: k_dict_idx, k_dict_export).

The yardstick is the oracle's decode of the same bytes without the flag: status, error page, levels
and the page table must be equal, and the flagged result's materialize() (the host gather
dictionary[keys]) bit-equal to the oracle's values / chars / offsets.  Hand-built chunks also check
that the keys returned are exactly the keys encoded."""
import io

import numpy as np
import pytest

import dictout_util as D
import pqgpu
import pqtest_util as U
from gen import pqwrite as W
from oracle import pyoracle as O
from pqgpu import abi

pytestmark = pytest.mark.gpu
KEEP = abi.COL_KEEP_DICT


@pytest.fixture(scope="module")
def dec():
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


# ---- hand-built chunks: the keys returned are the keys encoded ---------------------------------------
NNS = (0, 1, 7, 8, 9, 511, 512, 513, 4095, 4097)  # kHBlock and part edges


def _count_for(w):
    return 1 if w == 0 else min(1 << w, 70000)


@pytest.mark.parametrize("kind", ["rle", "packed", "mixed"])
@pytest.mark.parametrize("w", [0, 1, 3, 8, 13, 20, 32])
def test_keys_widths_and_sizes(dec, w, kind):
    count = _count_for(w)
    dpage = D.int32_dict(count, seed=w)
    chunks, want = [], []
    for nn in NNS:
        keys = D.gen_keys(nn, count, kind, seed=w)
        if nn and w:
            keys[-1] = count - 1  # the largest valid key, in the last (ragged) group
        chunks.append((dpage + D.data_page(keys, w, kind), dict(ptype=abi.INT32, data_page_offset=len(dpage))))
        want.append(keys)
    for nn, keys, (exp, r, got) in zip(NNS, want, D.run_batch(dec, chunks)):
        assert exp.status == 0
        d = D.check_kept(exp, r, got, "w%d %s nn%d" % (w, kind, nn), keys=keys)
        assert d.count == count and d.page == 0 and d.nil_entry == -1 and d.offsets is None


@pytest.mark.parametrize("w", [1, 5, 13])
def test_three_pages_every_output_alignment(dec, w):
    """Pages of nn = 1, 2, 3 mod 4 values: the later pages' keys start 4, 12 and 8 bytes past a granule."""
    count = min(1 << w, 5000)
    dpage = D.int32_dict(count)
    chunks, want = [], []
    for nns in ((513, 1026, 1539), (9, 4098, 515), (4097, 514, 7)):
        ks = [D.gen_keys(nn, count, "mixed", seed=k + nn) for k, nn in enumerate(nns)]
        chunks.append((dpage + b"".join(D.data_page(k, w) for k in ks),
                       dict(ptype=abi.FLOAT, data_page_offset=len(dpage))))
        want.append(np.concatenate(ks))
    for keys, (exp, r, got) in zip(want, D.run_batch(dec, chunks)):
        assert exp.status == 0 and len(exp.pages) == 4
        D.check_kept(exp, r, got, "3 pages", keys=keys)


def test_big_page_decoded_as_parts(dec):
    """One page of 70 000 values, 10 % of the slots null: above kSplitMin, so cut at block starts."""
    rng = np.random.default_rng(3)
    nn = 70000
    slots = nn * 10 // 9
    mask = np.zeros(slots, bool)
    mask[rng.permutation(slots)[:nn]] = True
    count = 3000
    dpage = D.int32_dict(count)
    keys = D.gen_keys(nn, count, "mixed", seed=9)
    chunk = dpage + D.data_page(keys, 12, "mixed", mask=mask)
    (exp, r, got), = D.run_batch(dec, [(chunk, dict(ptype=abi.INT32, max_def=1, data_page_offset=len(dpage)))])
    assert exp.status == 0 and exp.num_values == nn > 65536
    D.check_kept(exp, r, got, "big page", keys=keys)


# ---- dictionaries ------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 4096, 4097])
def test_dictionary_sizes(dec, count):
    w = max(1, int(count - 1).bit_length())
    dpage = D.int32_dict(count, seed=count)
    keys = D.gen_keys(3000, count, "mixed", seed=count)
    keys[[0, -1]] = count - 1
    chunk = dpage + D.data_page(keys, w)
    (exp, r, got), = D.run_batch(dec, [(chunk, dict(ptype=abi.INT32, data_page_offset=len(dpage)))])
    d = D.check_kept(exp, r, got, "count %d" % count, keys=keys)
    raw = np.frombuffer(dpage[-4 * count:], np.uint8)
    assert d.count == count and np.array_equal(d.values, raw)


def test_empty_dictionary_under_all_null_column(dec):
    dpage = D.dict_page(b"", 0)
    mask = np.zeros(300, bool)
    chunk = dpage + D.data_page(np.zeros(0, np.uint32), 1, mask=mask)
    for ptype in (abi.INT32, abi.BYTE_ARRAY):
        (exp, r, got), = D.run_batch(dec, [(chunk, dict(ptype=ptype, max_def=1, data_page_offset=len(dpage)))])
        assert exp.status == 0 and exp.num_values == 0 and exp.num_slots == 300
        d = D.check_kept(exp, r, got, "empty dictionary")
        assert d.count == 0 and d.page == 0 and np.asarray(d.values).nbytes == 0


def test_byte_array_dictionary_empty_and_long_strings(dec):
    words = [b"", b"a", b"", b"L" * 300, b"parquet", b"x" * 64, b"y" * 63, b"", b"tail" * 20]
    entries = b"".join(U.u32(len(s)) + s for s in words)
    dpage = D.dict_page(entries, len(words))
    keys = D.gen_keys(2000, len(words), "mixed", seed=4)
    keys[:len(words)] = np.arange(len(words))
    chunk = dpage + D.data_page(keys, 4)
    (exp, r, got), = D.run_batch(dec, [(chunk, dict(ptype=abi.BYTE_ARRAY, data_page_offset=len(dpage)))])
    d = D.check_kept(exp, r, got, "strings", keys=keys)
    assert d.value_width == 0 and d.pylist(abi.BYTE_ARRAY) == words
    assert np.array_equal(d.offsets, np.r_[0, np.cumsum([len(s) for s in words])])


def test_truncated_int96_dictionary_nil_entry(dec):
    """A dictionary page of 3 INT96 entries holding 29 bytes: the last one reads as zero bytes (Q8)."""
    entries = bytes(range(1, 30))
    dpage = D.dict_page(entries, 3)
    keys = np.array([2, 0, 1, 2, 1, 0, 2] * 40, np.uint32)
    chunk = dpage + D.data_page(keys, 2)
    (exp, r, got), = D.run_batch(dec, [(chunk, dict(ptype=abi.INT96, data_page_offset=len(dpage)))])
    assert exp.status == 0
    d = D.check_kept(exp, r, got, "int96 q8", keys=keys)
    assert d.nil_entry == 2 and d.count == 3 and d.value_width == 12
    assert np.asarray(d.values).tobytes() == entries


# ---- types, codecs, page versions, repetitions ---------------------------------------------------------
def _typed_columns(codec, version, rng, n=2500):
    nn = n - n // 7
    dl = np.zeros(n, np.uint8)
    dl[rng.permutation(n)[:nn]] = 1
    kw = dict(encoding=W.RLE_DICTIONARY, codec=codec, page_version=version, rows_per_page=700)
    pool5 = rng.integers(0, 256, (11, 5), dtype=np.uint8)
    pool12 = rng.integers(0, 256, (7, 12), dtype=np.uint8)
    words = [b"", b"go", b"parquet", b"w" * 70, b"dict"]
    pick = rng.integers(0, len(words), nn)
    offs = np.zeros(nn + 1, np.int64)
    np.cumsum([len(words[k]) for k in pick], out=offs[1:])
    # a LIST column: every slot holds an element (def 3), three elements per row
    ln = 3 * n
    rep = (np.arange(ln) % 3 != 0).astype(np.uint8)
    return [
        W.Column("i32", W.INT32, rng.integers(-9, 9, n).astype(np.int32), **kw),
        W.Column("i64", W.INT64, rng.integers(0, 2 ** 40, 30)[rng.integers(0, 30, nn)], repetition=W.OPTIONAL,
                 def_levels=dl, **kw),
        W.Column("f32", W.FLOAT, rng.standard_normal(20).astype(np.float32)[rng.integers(0, 20, n)], **kw),
        W.Column("f64", W.DOUBLE, rng.standard_normal(600)[rng.integers(0, 600, nn)], repetition=W.OPTIONAL,
                 def_levels=dl, **kw),
        W.Column("i96", W.INT96, pool12[rng.integers(0, 7, n)].reshape(-1), **kw),
        W.Column("fl5", W.FLBA, pool5[rng.integers(0, 11, n)].reshape(-1), type_length=5, **kw),
        W.Column("str", W.BYTE_ARRAY, np.frombuffer(b"".join(words[k] for k in pick), np.uint8), offsets=offs,
                 repetition=W.OPTIONAL, def_levels=dl, **kw),
        W.Column("lst", W.INT32, rng.integers(0, 50, ln).astype(np.int32), repetition=W.LIST,
                 def_levels=np.full(ln, 3, np.uint8), rep_levels=rep, **kw),
    ], n


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("codec", [W.UNCOMPRESSED, W.SNAPPY, W.GZIP])
def test_types_codecs_versions(dec, codec, version):
    cols, n = _typed_columns(codec, version, np.random.default_rng(17 + codec))
    data = W.write_file(cols, n)
    out = D.run_file(dec, data)
    assert len(out) == 8
    for c, (exp, r, got) in zip(cols, out):
        assert exp.status == 0 and exp.num_values > 0, c.name
        assert all(p.encoding == 8 for p in exp.pages if p.page_type in (0, 3)), c.name
        d = D.check_kept(exp, r, got, "%s codec %d v%d" % (c.name, codec, version))
        assert d.page == 0


def _arrow_table(n=3000, seed=2):
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    words = np.array(["", "alpha", "beta" * 9, "g", "delta-delta"], dtype=object)

    def runs(k):  # a random pattern of 64 picks over and over: bit-packed keys that every codec compresses
        return np.tile(rng.integers(0, k, 64), n // 64 + 1)[:n]

    return pa.table({
        "i": pa.array(runs(60).astype(np.int32), mask=np.arange(n) % 6 == 0),
        "d": pa.array(rng.standard_normal(40)[runs(40)]),
        "s": pa.array(words[runs(5)], pa.string(), mask=np.arange(n) % 9 == 0),
    })


def _arrow_write(t, **kw):
    import pyarrow.parquet as pq
    buf = io.BytesIO()
    args = dict(use_dictionary=True, write_statistics=False, data_page_size=2048, compression="none")
    args.update(kw)
    pq.write_table(t, buf, **args)
    return buf.getvalue()


@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("codec", ["zstd", "lz4", "snappy"])
def test_arrow_files_dictionary_in_scratch(dec, codec, version):
    """pyarrow files under ZSTD, LZ4_RAW and snappy: the dictionary page is read from the ctx scratch.
    The oracle has no ZSTD or LZ4 decoder: it decodes the same table written uncompressed, whose page
    table has the same pages at other offsets."""
    pytest.importorskip("pyarrow")
    t = _arrow_table(n=6000)
    data = _arrow_write(t, compression=codec, data_page_version=version)
    out = D.run_file(dec, data, twin=_arrow_write(t, data_page_version=version))
    assert len(out) == 3
    for k, (exp, r, got) in enumerate(out):
        assert exp.status == 0 and len(exp.pages) > 2
        D.check_kept(exp, r, got, "%s v%s col %d" % (codec, version, k), pages=False)
        assert [(p.page_type, p.encoding, p.num_values, p.not_null, p.uncompressed_size) for p in got.pages] == \
            [(p.page_type, p.encoding, p.num_values, p.not_null, p.uncompressed_size) for p in exp.pages]
        assert any(p.compressed_size != p.uncompressed_size for p in got.pages)


# ---- errors ---------------------------------------------------------------------------------------------
def _error_chunks():
    count = 50
    dpage = D.int32_dict(count)
    ok = D.gen_keys(900, count, "packed", seed=1)
    kw = dict(ptype=abi.INT32, data_page_offset=len(dpage))
    cases = {}
    # key == count as the 600th key of page 2
    bad = D.gen_keys(900, count, "packed", seed=2)
    bad[599] = count
    cases["key_eq_count"] = (dpage + D.data_page(ok, 6) + D.data_page(bad, 6), kw, abi.STATUS_CODES["DICT_INDEX"], 2)
    # an RLE run of a bad key
    runs = np.r_[D.gen_keys(520, count, "packed", seed=3), np.full(100, 63), D.gen_keys(30, count, "packed", seed=4)]
    cases["rle_bad_key"] = (dpage + D.data_page(runs.astype(np.uint32), 6, "mixed"), kw,
                            abi.STATUS_CODES["DICT_INDEX"], 1)
    # a truncated stream: the page's values section ends inside the bit-packed run
    full = D.key_stream(ok, 6, "packed")
    cases["truncated"] = (dpage + D.data_page(ok, 6, values=full[:len(full) // 2]), kw, None, 1)
    # a bad key before the truncation: "dict: invalid index" wins
    cases["bad_then_truncated"] = (dpage + D.data_page(bad, 6, values=D.key_stream(bad, 6, "packed")[:600]), kw,
                                   abi.STATUS_CODES["DICT_INDEX"], 1)
    cases["width_33"] = (dpage + D.data_page(ok, 6) + D.data_page(ok, 6, values=bytes([33]) + full[1:]), kw,
                         abi.STATUS_CODES["BIT_WIDTH"], 2)
    cases["no_values_section"] = (dpage + D.data_page(ok, 6, values=b""), kw, abi.STATUS_CODES["EOF"], 1)
    cases["no_dictionary_page"] = (D.data_page(ok, 6), dict(ptype=abi.INT32), abi.STATUS_CODES["DICT_INDEX"], 0)
    cases["no_dictionary_width0"] = (D.data_page(np.zeros(40, np.uint32), 0), dict(ptype=abi.INT32),
                                     abi.STATUS_CODES["DICT_INDEX"], 0)
    cases["second_dictionary"] = (dpage + D.data_page(ok, 6) + dpage + D.data_page(ok, 6), kw, None, None)
    strs = b"".join(U.u32(3) + b"abc" for _ in range(5))
    cases["bad_string_dictionary"] = (D.dict_page(strs[:-2], 5) + D.data_page(ok % 5, 3),
                                      dict(ptype=abi.BYTE_ARRAY, data_page_offset=len(D.dict_page(strs[:-2], 5))),
                                      None, 0)
    return cases


def test_errors_are_the_unflagged_ones(dec):
    cases = _error_chunks()
    names = list(cases)
    out = D.run_batch(dec, [(cases[k][0], cases[k][1]) for k in names])
    for name, (exp, r, got) in zip(names, out):
        _, _, status, page = cases[name]
        assert exp.status != 0, name
        if status is not None:
            assert exp.status == status, "%s: oracle %s" % (name, abi.status_name(exp.status))
        if page is not None:
            assert exp.error_page == page, name
        D.check_kept(exp, r, got, name)


def test_flag_argument_errors(dec):
    dpage = D.int32_dict(4)
    chunk = dpage + D.data_page(np.array([0, 1, 2, 3] * 5, np.uint32), 2)
    keep = []
    dev = dec.upload(chunk)
    try:
        # BOOLEAN has no dictionary encoding
        j, _ = U.chunk_job(chunk, ptype=abi.BOOLEAN, data_page_offset=len(dpage), keep=keep)
        j.data, j.col.flags = dev, KEEP
        res = (abi.ChunkResult * 1)()
        arr = (abi.ChunkJob * 1)(j)
        assert dec.L.pqg_decode_chunks(dec.ctx, arr, 1, res) == abi.STATUS_CODES["INVALID_ARG"]
        # the page entry
        pj = abi.PageJob()
        pj.col.physical_type, pj.col.type_length, pj.col.flags = abi.INT32, -1, KEEP
        pj.page, pj.page_len = dev + len(dpage), len(chunk) - len(dpage)
        pj.dict_page, pj.dict_page_len = dev, len(dpage)
        import ctypes as C
        assert dec.L.pqg_decode_page(dec.ctx, C.byref(pj), res) == abi.STATUS_CODES["INVALID_ARG"]
        pj.col.flags = 0
        assert dec.L.pqg_decode_page(dec.ctx, C.byref(pj), res) == 0 and res[0].status == 0
        # pqg_get_dictionary on a job without the flag, and on a job index out of range
        j, _ = U.chunk_job(chunk, ptype=abi.INT32, data_page_offset=len(dpage), keep=keep)
        j.data = dev
        r = dec.decode_jobs([j])[0]
        assert r.status == 0 and r.value_width == 4 and not (r.col_flags & KEEP)
        for idx in (0, 1, -1):
            with pytest.raises(pqgpu.PqgError) as e:
                dec.dictionary(idx)
            assert e.value.code == abi.STATUS_CODES["INVALID_ARG"]
    finally:
        dec.free(dev)


# ---- NOT_DICT: a writer's PLAIN fallback ---------------------------------------------------------------
@pytest.fixture(scope="module")
def fallback_file():
    pa = pytest.importorskip("pyarrow")
    rng = np.random.default_rng(8)
    n = 6000
    vals = np.array(["%018d" % v for v in rng.integers(0, 10 ** 17, 3000)], dtype=object)
    col = np.r_[vals, vals[rng.integers(0, 3000, n - 3000)]]
    t = pa.table({"s": pa.array(col, pa.string()), "k": pa.array((np.arange(n) % 11).astype(np.int32))})
    return _arrow_write(t, dictionary_pagesize_limit=4096, data_page_size=8192), t


def test_not_dict_on_fallback_chunk(dec, fallback_file):
    data, t = fallback_file
    pf = pqgpu.ParquetFile(data)
    exp = O.decode_chunk(pf.host_job(0, 0)[0])
    encs = [p.encoding for p in exp.pages if p.page_type in (0, 3)]
    assert exp.status == 0 and 8 in encs and 0 in encs, encs
    first_plain = next(i for i, p in enumerate(exp.pages) if p.page_type in (0, 3) and p.encoding == 0)
    (e0, r0, got0), (e1, r1, got1) = D.run_file(dec, data)
    assert got0.status == D.NOT_DICT == abi.STATUS_CODES["NOT_DICT"] and got0.error_page == first_plain
    assert got0.dictionary is None
    D.check_kept(e1, r1, got1, "the dictionary column next to it")
    # FileReader: the chunk is decoded once more without the flag and comes back materialised
    fr = pqgpu.FileReader(data, decoder=dec, read_dictionary=("s", "k"))
    cols = fr.read_row_group(0)
    s, k = cols["s"], cols["k"]
    assert s.status == 0 and s.dictionary is None and s.value_width == 0
    b, o = s.values.tobytes(), s.offsets
    assert [b[o[i]:o[i + 1]].decode() for i in range(s.num_values)] == t.column("s").to_pylist()
    assert k.status == 0 and k.dictionary is not None and k.dictionary.count == 11
    assert k.materialize().values.view(np.int32).tolist() == t.column("k").to_pylist()
    # the device results of decode_row_groups tell which chunks kept their dictionary
    flags = {c: r.col_flags & KEEP for _, c, r in fr.decode_row_groups([0])}
    assert flags == {0: 0, 1: KEEP}


# ---- mixed batches --------------------------------------------------------------------------------------
def test_mixed_batch(dec):
    """Flagged and unflagged jobs of the same file in one call, of every type: each result is right."""
    cols, n = _typed_columns(W.SNAPPY, 1, np.random.default_rng(23))
    data = W.write_file(cols, n)
    for flags in ([KEEP, 0] * 4, [0, KEEP] * 4):
        out = D.run_file(dec, data, flags)
        for c, f, (exp, r, got) in zip(cols, flags, out):
            if f:
                D.check_kept(exp, r, got, "mixed " + c.name)
            else:
                assert not (r.col_flags & KEEP) and got.dictionary is None, c.name
                import parity as P
                P.compare_chunk(exp, got, "mixed unflagged " + c.name)
    # the same chunks decoded both ways, one after the other, on one context: what either decode
    # learned about a chunk's sizes does not fail the other
    pf = pqgpu.ParquetFile(data)
    dev = dec.upload(pf.data)
    try:
        for f in (KEEP, 0, KEEP):
            jobs = [pqgpu.device_job(pf, 0, c, dev) for c in range(pf.num_columns)]
            for j in jobs:
                j.col.flags |= f
            assert [r.status for r in dec.decode_jobs(jobs)] == [0] * len(jobs)
    finally:
        dec.free(dev)


# ---- mutations ------------------------------------------------------------------------------------------
def test_mutations(dec):
    """200 single-byte mutations of a small three-column file: the flagged status and error page are
    the oracle's, except where a data page of another encoding makes the flagged decode NOT_DICT."""
    not_dict = 0
    for k, data in enumerate(D.mutations()):
        took = False
        for c, (exp, r, got) in enumerate(D.run_file(dec, data)):
            where = "mutation %d col %d" % (k, c)
            if got.status == D.NOT_DICT:
                assert D.other_encoding_page(exp), where
                took = True
                continue
            D.check_kept(exp, r, got, where)
        not_dict += took
    assert not_dict <= D.MUTATIONS // 10, not_dict


# ---- pyarrow cross-checks ---------------------------------------------------------------------------------
def test_file_reader_against_pyarrow_read_dictionary(dec):
    pytest.importorskip("pyarrow")
    import pyarrow.parquet as pq
    t = _arrow_table(n=4000, seed=6)
    data = _arrow_write(t, compression="snappy", row_group_size=1500)
    ref = pq.read_table(io.BytesIO(data), read_dictionary=["s", "i"])
    fr = pqgpu.FileReader(data, decoder=dec, read_dictionary=("s", "i"))
    got = {"i": [], "d": [], "s": []}
    for rg in range(fr.row_group_count()):
        cols = fr.read_row_group(rg)
        assert cols["s"].dictionary is not None and cols["i"].dictionary is not None and cols["d"].dictionary is None
        for name, dt in (("i", np.int32), ("d", np.float64)):
            c = cols[name].materialize()
            vals = iter(c.values.view(dt).tolist())
            dl = c.def_levels if c.def_levels is not None else np.ones(c.num_slots, np.uint8)
            got[name] += [next(vals) if x else None for x in dl]
        c = cols["s"]
        ent = c.dictionary.pylist(abi.BYTE_ARRAY)
        keys = iter(c.keys().tolist())
        got["s"] += [ent[next(keys)].decode() if x else None for x in c.def_levels]
    # each side's own lookup: pyarrow may reorder or unify dictionaries, so keys are not compared
    for name in ("i", "d", "s"):
        assert got[name] == ref.column(name).to_pylist(), name


def test_nested_lists_against_pyarrow(dec):
    pa = pytest.importorskip("pyarrow")
    import pyarrow.parquet as pq
    rng = np.random.default_rng(12)
    words = ["", "x", "list", "of" * 20, "strings"]

    def rows(pick):
        out = []
        for _ in range(700):
            u = rng.random()
            if u < 0.1:
                out.append(None)
            else:
                out.append([None if rng.random() < 0.15 else pick() for _ in range(int(rng.integers(0, 5)))])
        return out

    t = pa.table({"ls": pa.array(rows(lambda: words[int(rng.integers(0, 5))]), pa.list_(pa.string())),
                  "li": pa.array(rows(lambda: int(rng.integers(0, 30))), pa.list_(pa.int32()))})
    data = _arrow_write(t)
    ref = pq.read_table(io.BytesIO(data))
    plain = pqgpu.FileReader(data, decoder=dec).read_row_group_nested(0)
    kept = pqgpu.FileReader(data, decoder=dec, read_dictionary=("ls", "li")).read_row_group_nested(0)
    for name in ("ls", "li"):
        path = name + ".list.element"
        k = kept[path]
        assert k.dictionary is not None and k.value_width == 4 and plain[path].dictionary is None
        want = ref.column(name).to_pylist()
        if name == "ls":
            want = [None if r is None else [None if s is None else s.encode() for s in r] for r in want]
        assert k.to_pylist() == want, name
        assert k.to_pylist() == plain[path].to_pylist(), name


# ---- FileReader: device results and rows -------------------------------------------------------------------
def test_decode_row_groups_in_place_dictionaries_stay_valid(dec):
    """decode_row_groups returns device results; the dictionary of an uncompressed fixed-width chunk
    lies inside the uploaded chunk bytes, which must outlive the call: dictionary[keys] of every
    chunk, fetched after other device memory was allocated, equals the oracle's values."""
    cols, n = _typed_columns(W.UNCOMPRESSED, 1, np.random.default_rng(31))
    data = W.write_file(cols, n, row_groups=2)
    pf = pqgpu.ParquetFile(data)
    fr = pqgpu.FileReader(data, decoder=dec, read_dictionary=tuple(c.path.decode() for c in pf.columns))
    res = fr.decode_row_groups([0, 1])
    assert len(res) == 2 * len(cols) and fr.uploaded_bytes > 0
    junk = dec.upload(np.full(fr.uploaded_bytes, 0xA5, np.uint8))  # takes a freed block of that size, if any
    try:
        for i, (rg, c, r) in enumerate(res):
            exp = O.decode_chunk(pf.host_job(rg, c)[0], D.PAGE_CAP)
            D.check_kept(exp, r, D.download(dec, r, i), "rg%d %s" % (rg, cols[c].name))
    finally:
        dec.free(junk)
    # the next decode of the reader lets the upload go; so does close()
    held = fr._held
    assert held is not None
    fr.read_row_group(0)
    assert fr._held is None
    fr.decode_row_groups([1])
    assert fr._held is not None
    fr.close()
    assert fr._held is None
    # a reader that keeps no dictionary holds nothing
    fr = pqgpu.FileReader(data, decoder=dec)
    fr.decode_row_groups([0])
    assert fr._held is None


def test_next_row_ignores_read_dictionary(dec):
    """Rows need values: next_row returns the same rows with the option as without it."""
    cols, n = _typed_columns(W.SNAPPY, 1, np.random.default_rng(37), n=300)
    data = W.write_file(cols, n, row_groups=2)
    names = ("i32", "i64", "f64", "fl5", "str", "lst")
    a = pqgpu.FileReader(data, *names, decoder=dec)
    b = pqgpu.FileReader(data, *names, decoder=dec, read_dictionary=names)
    assert len(b.keep_dict) == len(names)
    rows = 0
    while True:
        try:
            ra = a.next_row()
        except EOFError:
            with pytest.raises(EOFError):
                b.next_row()
            break
        assert b.next_row() == ra
        rows += 1
    assert rows == n
