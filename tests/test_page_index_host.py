"""The page index on the host: the footer planner's index ranges, the OffsetIndex / ColumnIndex parsers
(pqg_page_index.h) against the oracle's page table and decoded values, hand-written indexes, the
stand-alone fuzz program (plain and under sanitizers), and FileReader's row-range planner."""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import pqgpu
import pqtest_util as U
from oracle import pyoracle as O
from pqgpu import abi
from pqgpu import filters as F
from pqgpu._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METADATA = abi.STATUS_CODES["METADATA"]
ROWS = 20000


def fixture_file(compression="snappy", version="1.0", row_groups=1, page_index=True):
    pa = pytest.importorskip("pyarrow")
    pq = pytest.importorskip("pyarrow.parquet")
    rng = np.random.default_rng(7)
    a = np.arange(ROWS, dtype=np.int64) * 3
    words = np.array(["w%03d" % i for i in range(200)], dtype=object)
    s = words[rng.integers(0, 200, ROWS)]
    s[rng.random(ROWS) < 0.2] = None
    s[4096:14000] = None  # whole pages of nulls
    lens = rng.integers(0, 5, ROWS)
    flat = rng.integers(0, 1000, int(lens.sum())).astype(np.int32)
    offs = np.zeros(ROWS + 1, np.int32)
    np.cumsum(lens, out=offs[1:])
    t = pa.table({"a": pa.array(a), "s": pa.array(list(s), pa.string()),
                  "l": pa.ListArray.from_arrays(pa.array(offs), pa.array(flat))})
    buf = io.BytesIO()
    pq.write_table(t, buf, compression=compression.upper(), data_page_version=version, data_page_size=4096,
                   write_page_index=page_index, use_dictionary=["s"], row_group_size=-(-ROWS // row_groups))
    return buf.getvalue(), t


# ------------------------------------------------------------------ OffsetIndex against the oracle's page table
@pytest.mark.parametrize("row_groups", [1, 3])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("compression", ["none", "snappy", "zstd"])
def test_offset_index_matches_page_table(compression, version, row_groups):
    data, _ = fixture_file(compression, version, row_groups)
    pf = pqgpu.ParquetFile(data)
    assert pf.num_row_groups == row_groups
    for rg in range(row_groups):
        for c in range(3):
            m = pf.chunk_meta(rg, c)
            pi = pf.page_index(rg, c)
            locs = pi.locations
            assert len(locs) > 1 or row_groups == 3
            # the locations tile [data_page_offset, start + total_compressed_size); the dictionary page is the gap
            assert locs[0][0] == m.data_page_offset
            assert all(locs[k][0] + locs[k][1] == locs[k + 1][0] for k in range(len(locs) - 1))
            assert locs[-1][0] + locs[-1][1] == m.start + m.total_compressed_size
            assert locs[0][2] == 0 and all(x[2] < y[2] for x, y in zip(locs, locs[1:]))
            ch = O.decode_chunk(pf.host_job(rg, c)[0])
            if compression == "zstd":
                continue  # the oracle has no ZSTD: the tiling above is what can be said
            pages = [p for p in ch.pages if p.page_type != abi.PAGE_DICTIONARY]
            if ch.status != 0:
                pages = pages[:-1]  # (a V2 page pyarrow leaves uncompressed stops the oracle: the pages before it)
            assert ch.status != 0 or len(pages) == len(locs)
            rep0 = np.cumsum(ch.rep_levels == 0) if (ch.status == 0 and ch.rep_levels is not None) else None
            for p, (off, size, first_row) in zip(pages, locs):
                assert off == m.start + p.header_offset
                assert size == p.payload_offset - p.header_offset + p.compressed_size
                if rep0 is None:
                    assert pf.columns[c].desc.max_rep > 0 or first_row == p.slot_offset
                else:  # rows, not slots: the rep == 0 slots before the page
                    assert first_row == (rep0[p.slot_offset - 1] if p.slot_offset else 0)


def test_no_index_in_the_file():
    data, _ = fixture_file(page_index=False)
    pf = pqgpu.ParquetFile(data)
    assert all(pf.page_index(0, c) is None for c in range(3))


# ------------------------------------------------------------------ ColumnIndex against the oracle's values
def test_column_index_matches_decoded_values():
    data, _ = fixture_file("none", "1.0")
    pf = pqgpu.ParquetFile(data)
    for c, name in ((0, "a"), (1, "s")):
        pi = pf.page_index(0, c)
        ch = O.decode_chunk(pf.host_job(0, c)[0])
        assert ch.status == 0
        pages = [p for p in ch.pages if p.page_type != abi.PAGE_DICTIONARY]
        assert len(pages) == len(pi.locations) == len(pi.null_pages)
        assert pi.boundary_order == (1 if name == "a" else pi.boundary_order)
        for k, p in enumerate(pages):
            assert pi.null_counts[k] == p.num_values - p.not_null
            assert pi.null_pages[k] == (p.not_null == 0)
            lo, hi, nulls = pi.stats(k)
            if p.not_null == 0:
                assert lo is None and hi is None and nulls == p.num_values
                continue
            if name == "a":
                v = ch.values.view("<i8")[p.value_offset:p.value_offset + p.not_null]
                exp = (int(v.min()).to_bytes(8, "little", signed=True), int(v.max()).to_bytes(8, "little", signed=True))
            else:
                o = ch.offsets[p.value_offset:p.value_offset + p.not_null + 1]
                b = ch.values.tobytes()
                vals = [b[o[i]:o[i + 1]] for i in range(p.not_null)]
                exp = (min(vals), max(vals))
            assert (lo, hi) == exp, (name, k)


def test_column_index_all_null_page():
    """A column whose last page holds only nulls: null_pages, no bounds, the page's rows as its nulls."""
    pa = pytest.importorskip("pyarrow")
    pq = pytest.importorskip("pyarrow.parquet")
    n = 8000
    v = [2 * i if i < 3072 else None for i in range(n)]
    buf = io.BytesIO()
    pq.write_table(pa.table({"n": pa.array(v, pa.int64())}), buf, compression="NONE", data_page_size=1024,
                   write_page_index=True, use_dictionary=False)
    pf = pqgpu.ParquetFile(buf.getvalue())
    pi = pf.page_index(0, 0)
    ch = O.decode_chunk(pf.host_job(0, 0)[0])
    assert ch.status == 0 and len(ch.pages) == len(pi.locations)
    assert [p.not_null == 0 for p in ch.pages] == pi.null_pages and pi.null_pages[-1] and not pi.null_pages[0]
    assert pi.null_counts == [p.num_values - p.not_null for p in ch.pages]
    lo, hi = pi.page_rows(len(pi.locations) - 1)
    assert pi.stats(len(pi.locations) - 1) == (None, None, hi - lo)
    fr = pqgpu.FileReader(buf.getvalue(), decoder=object(), use_page_index=True)
    assert fr._row_ranges(0, F.parse([("n", ">", 0)]), None) == [(0, lo)]     # an all-null page passes only `is None`
    assert fr._row_ranges(0, F.parse([("n", "is", None)]), None) == [(lo, hi)]


def test_offset_index_without_a_column_index():
    """A file with an OffsetIndex and no ColumnIndex: the locations stand, the ColumnIndex parts are
    None, a filter rules no page out, and a row range still picks its pages."""
    pa = pytest.importorskip("pyarrow")
    pq = pytest.importorskip("pyarrow.parquet")
    n = 20000
    buf = io.BytesIO()
    pq.write_table(pa.table({"a": pa.array(np.arange(n, dtype=np.int64))}), buf, data_page_size=4096,
                   write_page_index=True, write_statistics=False)
    pf = pqgpu.ParquetFile(buf.getvalue())
    ir = abi.IndexRanges()
    assert lib().pqg_file_chunk_index(pf._h, 0, 0, C.byref(ir)) == 0
    assert ir.offset_index_length > 0 and ir.column_index_length == 0
    pi = pf.page_index(0, 0)
    assert len(pi.locations) > 4
    assert (pi.null_pages, pi.min_values, pi.max_values, pi.null_counts, pi.boundary_order) == (None,) * 5
    assert all(pi.stats(k) == (None, None, -1) for k in range(len(pi.locations)))
    fr = pqgpu.FileReader(buf.getvalue(), decoder=object(), use_page_index=True)
    assert fr._row_ranges(0, F.parse([("a", "<", 10)]), None) == [(0, n)]
    assert fr._row_ranges(0, F.parse([("a", "<", 10)]), (100, 200)) == [(100, 200)]
    first = [l[2] for l in pi.locations]
    got = [k for k in range(len(first)) if pqgpu.reader._intersect([pi.page_rows(k)], [(first[2], first[3] + 1)])]
    assert got == [2, 3]


# ------------------------------------------------------------------ hand-written indexes
def tlist(etype, items):
    n = len(items)
    head = bytes([(n << 4) | etype]) if n < 15 else bytes([0xF0 | etype]) + U.uvarint(n)
    return head + b"".join(items)


def offset_index(locs):
    items = [U.TW().i64(1, o).i32(2, s).i64(3, r).stop() for o, s, r in locs]
    w = U.TW()
    w.field(1, 9)
    w.b += tlist(12, items)
    return w.stop()


def column_index(null_pages, mins, maxs, order=0, null_counts=None, skip=()):
    w = U.TW()
    if 1 not in skip:
        w.field(1, 9)
        w.b += tlist(1, [b"\x01" if x else b"\x02" for x in null_pages])
    w.field(2, 9)
    w.b += tlist(8, [U.uvarint(len(x)) + x for x in mins])
    w.field(3, 9)
    w.b += tlist(8, [U.uvarint(len(x)) + x for x in maxs])
    w.i32(4, order)
    if null_counts is not None:
        w.field(5, 9)
        w.b += tlist(6, [U.zigzag(x) for x in null_counts])
    return w.stop()


def parse_offsets(b, cap=64):
    out = (abi.PageLoc * cap)()
    n = lib().pqg_parse_offset_index(b, len(b), out, cap)
    return n if n < 0 else [(out[k].offset, out[k].size, out[k].first_row) for k in range(min(n, cap))]


def parse_column(b):
    L = lib()
    h = C.c_void_p()
    rc = L.pqg_column_index_parse(b, len(b), C.byref(h))
    if rc != 0:
        assert not h.value
        return rc
    try:
        pages = []
        for k in range(L.pqg_column_index_pages(h)):
            st, np_ = abi.ChunkStats(), C.c_int32()
            assert L.pqg_column_index_page(h, k, C.byref(st), C.byref(np_)) == 0
            pages.append((bool(np_.value), C.string_at(st.min_value, st.min_len) if st.min_value else None,
                          C.string_at(st.max_value, st.max_len) if st.max_value else None, st.null_count))
        assert L.pqg_column_index_page(h, len(pages), C.byref(abi.ChunkStats()), None) == abi.STATUS_CODES["INVALID_ARG"]
        return pages, L.pqg_column_index_boundary_order(h)
    finally:
        L.pqg_column_index_free(h)


def test_hand_written_offset_indexes():
    locs = [(100, 50, 0), (150, 7, 10), (400, 1 << 20, 11)]
    assert parse_offsets(offset_index(locs)) == locs
    assert parse_offsets(offset_index([])) == []                      # 0 pages
    assert parse_offsets(offset_index(locs), cap=2) == locs[:2]       # the count is known without room for all
    assert lib().pqg_parse_offset_index(offset_index(locs), len(offset_index(locs)), None, 0) == 3
    for bad in ([(100, 50, 0), (149, 7, 10)],      # overlapping
                [(100, 50, 0), (90, 7, 10)],       # offsets that descend
                [(100, -5, 0)], [(100, 0, 0)],     # sizes
                [(-1, 5, 0)], [(100, 5, -1)],
                [(100, 50, 10), (150, 7, 5)]):     # rows that descend
        assert parse_offsets(offset_index(bad)) == METADATA, bad
    assert parse_offsets(U.TW().stop()) == METADATA                   # no list at all
    assert parse_offsets(offset_index(locs) + b"\0") == METADATA       # bytes left over
    one = U.TW().i64(1, 5).i32(2, 5).stop()                           # a location without its first row
    w = U.TW()
    w.field(1, 9)
    w.b += tlist(12, [one])
    assert parse_offsets(w.stop()) == METADATA
    w = U.TW()
    w.field(1, 9)
    w.b += bytes([0xFC]) + U.uvarint(1 << 30)                         # a list longer than the bytes
    assert parse_offsets(w.stop()) == METADATA


def test_hand_written_column_indexes():
    pages, order = parse_column(column_index([False, True, False], [b"a", b"", b"c"], [b"b", b"", b"zz"], 1, [0, 9, 2]))
    assert order == 1
    assert pages == [(False, b"a", b"b", 0), (True, None, None, 9), (False, b"c", b"zz", 2)]  # empty bounds: a null page
    pages, order = parse_column(column_index([False], [b"\x01\0\0\0"], [b"\x02\0\0\0"], 2))
    assert pages == [(False, b"\x01\0\0\0", b"\x02\0\0\0", -1)] and order == 2          # no null_counts
    assert parse_column(column_index([], [], [], 0, [])) == ([], 0)                         # 0 pages
    for bad in (column_index([False, False], [b"a"], [b"b", b"c"]),                        # lists of unequal length
                column_index([False], [b"a"], [b"b"], 0, [1, 2]),
                column_index([False], [b"a"], [b"b"], 0, [-1]),
                column_index([False], [b"a"], [b"b"], 3),
                column_index([False], [b"a"], [b"b"], skip=(1,)),
                column_index([False], [b"a"], [b"b"]) + b"\0",
                U.TW().stop()):
        assert parse_column(bad) == METADATA


def test_index_ranges_of_the_planner():
    data, _ = fixture_file()
    pf = pqgpu.ParquetFile(data)
    for c in range(3):
        ir = abi.IndexRanges()
        assert lib().pqg_file_chunk_index(pf._h, 0, c, C.byref(ir)) == 0
        assert ir.offset_index_length > 0 and ir.column_index_length > 0
        assert 0 < ir.column_index_offset < ir.offset_index_offset < len(data)
    ir = abi.IndexRanges()
    data2, _ = fixture_file(page_index=False)
    assert lib().pqg_file_chunk_index(pqgpu.ParquetFile(data2)._h, 0, 0, C.byref(ir)) == 0
    assert ir.offset_index_length == 0 and ir.column_index_length == 0
    assert lib().pqg_file_chunk_index(pf._h, 0, 3, C.byref(ir)) == abi.STATUS_CODES["INVALID_ARG"]


# ------------------------------------------------------------------ truncated and garbage input (stand-alone)
def build_model(tmp_path, name, extra=()):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / name)
    subprocess.run([cxx, "-O1", "-std=c++17", *extra, os.path.join(ROOT, "tools", "page_index_model.cpp"), "-o", exe],
                   check=True)
    return exe


@pytest.mark.parametrize("san", [False, True])
def test_parsers_on_prefixes_and_flipped_bytes(tmp_path, san):
    """tools/page_index_model.cpp: every prefix of a valid index and every copy with one byte changed
    parses or is METADATA; the second build runs it under -fsanitize=address,undefined."""
    exe = build_model(tmp_path, "pim_san" if san else "pim",
                      ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all") if san else ())
    data, _ = fixture_file()
    pf = pqgpu.ParquetFile(data)
    ir = abi.IndexRanges()
    assert lib().pqg_file_chunk_index(pf._h, 0, 1, C.byref(ir)) == 0
    inputs = {"offset": [data[ir.offset_index_offset:ir.offset_index_offset + ir.offset_index_length],
                         offset_index([(100, 50, 0), (150, 7, 10)])],
              "column": [data[ir.column_index_offset:ir.column_index_offset + ir.column_index_length],
                         column_index([False, True], [b"a", b""], [b"b", b""], 1, [0, 9])]}
    for kind, blobs in inputs.items():
        for k, b in enumerate(blobs):
            path = tmp_path / ("%s%d.bin" % (kind, k))
            path.write_bytes(b)
            r = subprocess.run([exe, "fuzz", kind, str(path)], capture_output=True, text=True)
            assert r.returncode == 0 and r.stdout.startswith("valid "), (kind, k, r.returncode, r.stdout, r.stderr[-2000:])
            assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


# ------------------------------------------------------------------ the planner, brute force
def random_dnf(rng):
    def term():
        k = rng.integers(0, 6)
        x = int(rng.integers(-100, 3 * ROWS + 100))
        if k == 0:
            return ("a", [">", ">=", "<", "<=", "==", "!="][rng.integers(0, 6)], x)
        if k == 1:
            return ("a", "in", [x, x + 3, 30])
        if k == 2:
            return ("s", ["==", "!=", "<", ">="][rng.integers(0, 4)], "w%03d" % rng.integers(0, 220))
        if k == 3:
            return ("s", "is", None)
        if k == 4:
            return ("s", "is not", None)
        return ("a", "<", int(rng.integers(0, 6000)))
    return [[term() for _ in range(rng.integers(1, 3))] for _ in range(rng.integers(1, 3))]


def passes(table, dnf):
    a = table["a"].to_numpy()
    s = np.array(table["s"].to_pylist(), dtype=object)
    null = np.array([x is None for x in s])
    sv = np.where(null, "", s).astype(str)
    keep = np.zeros(len(a), bool)
    for terms in dnf:
        m = np.ones(len(a), bool)
        for col, op, val in terms:
            if op in ("is", "is not"):
                m &= null if op == "is" else ~null
                continue
            v, ok = (a, np.ones(len(a), bool)) if col == "a" else (sv, ~null)
            if op == "in":
                m &= ok & np.isin(v, val)
            else:
                m &= ok & {"==": v == val, "!=": v != val, "<": v < val, "<=": v <= val, ">": v > val, ">=": v >= val}[op]
        keep |= m
    return keep


ROW_CASES = [None, (0, ROWS), (0, 0), (1024, 2048), (0, 1024), (1000, 1030), (1000, 9000), (ROWS - 1, ROWS), (5000, 5000)]


def test_planner_brute_force():
    data, table = fixture_file()
    fr = pqgpu.FileReader(data, decoder=object(), use_page_index=True)
    pf = fr.file
    rng = np.random.default_rng(11)
    pruned = 0
    for trial in range(60):
        dnf = random_dnf(rng) if trial % 4 else None
        rows = ROW_CASES[trial % len(ROW_CASES)]
        R = fr._row_ranges(0, F.parse(dnf) if dnf is not None else None, rows)
        assert R == sorted(R) and all(a < b for a, b in R) and all(x[1] < y[0] for x, y in zip(R, R[1:]))
        inside = np.zeros(ROWS, bool)
        for a, b in R:
            inside[a:b] = True
        want = np.ones(ROWS, bool) if dnf is None else passes(table, dnf)
        if rows is not None:
            lim = np.zeros(ROWS, bool)
            lim[rows[0]:rows[1]] = True
            want &= lim
            assert not (inside & ~lim).any()
        assert not (want & ~inside).any(), (dnf, rows)  # no passing row lies outside R
        if dnf is None:
            assert R == ([(0, ROWS)] if rows is None else [r for r in [rows] if r[1] > r[0]])
        pruned += inside.sum() < (ROWS if rows is None else rows[1] - rows[0])
        # the pages of each column are exactly those meeting R
        for c in range(2):
            pi = pf.page_index(0, c)
            got = [k for k in range(len(pi.locations)) if pqgpu.reader._intersect([pi.page_rows(k)], R)]
            exp = [k for k in range(len(pi.locations)) if inside[slice(*pi.page_rows(k))].any()]
            assert got == exp
    assert pruned > 5  # the index did rule pages out
    # a sorted column: a range keeps only the pages that hold it
    R = fr._row_ranges(0, F.parse([("a", ">=", 3 * 5000), ("a", "<", 3 * 5100)]), None)
    assert R == [(4096, 5120)]
    assert fr._row_ranges(0, F.parse([("a", "<", -5)]), None) == []
    assert pqgpu.FileReader(data, decoder=object())._row_ranges(0, F.parse([("a", "<", -5)]), None) == [(0, ROWS)]
