"""The host half of filtered reads, without a GPU: footer statistics (pqg_file_chunk_stats) against
pyarrow's, DNF parsing, and FileReader.prune_row_groups.

Pruning is judged by soundness: a pruned row group holds no row that an evaluation of the filter in
Python selects (pqg_filter's rules: a null passes only `is null`, NaN passes only !=).  pyarrow is
the yardstick only on NaN-free data: on a row group holding [NaN, 1.0] it writes min = max = 1.0
and drops the NaN row for `!= 1.0`."""
import io
import struct

import numpy as np
import pytest

import pqgpu
from pqgpu import abi
from pqgpu import filters as F

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")

NAN = float("nan")
ROWS = 40  # per row group


class _NoGpu:
    """Stands in for the GpuDecoder of a FileReader that only plans."""


def _write(table, **kw):
    buf = io.BytesIO()
    pq.write_table(table, buf, row_group_size=ROWS, **kw)
    return buf.getvalue()


def _table(nan=True):
    """Three row groups of 40 rows: ascending, disjoint ranges per row group (so that statistics
    decide most filters exactly), nulls in the first, an all-null row group for `n`, a constant
    string column, NaN / +-0.0 / empty strings / bytes >= 0x80 where asked."""
    n = 3 * ROWS
    i64 = [None if k % 7 == 3 and k < ROWS else k * 10 - 500 for k in range(n)]
    i32 = [(-2 ** 31 if k == 0 else k) for k in range(n)]
    u32 = [k * 35_000_000 for k in range(n)]          # crosses 2^31 inside the second row group
    f32 = [k * 0.5 - 10.0 for k in range(n)]
    f64 = [k * 0.25 - 5.0 for k in range(n)]
    if nan:
        f32[5], f64[ROWS + 5] = NAN, NAN
        f64[20], f64[21] = -0.0, 0.0                    # the row group's minimum is a zero
    s = ["%03d" % k if k % 5 else "" for k in range(n)]
    s[ROWS + 1] = "\u0080x"                             # 0xc2 0x80 ...: above every ASCII string
    s[2] = None
    const = ["same"] * ROWS + ["b%d" % k for k in range(ROWS)] + ["same"] * ROWS
    flba = [bytes([k, 255 - k, 0x80]) for k in range(n)]
    b = [k >= ROWS for k in range(n)]
    b[ROWS + 3] = None
    nul = [None] * ROWS + [float(k) for k in range(2 * ROWS)]
    return pa.table({
        "i64": pa.array(i64, pa.int64()), "i32": pa.array(i32, pa.int32()), "u32": pa.array(u32, pa.uint32()),
        "f32": pa.array(f32, pa.float32()), "f64": pa.array(f64, pa.float64()), "s": pa.array(s, pa.string()),
        "const": pa.array(const, pa.string()), "flba": pa.array(flba, pa.binary(3)), "b": pa.array(b, pa.bool_()),
        "n": pa.array(nul, pa.float64()), "rg": pa.array([k // ROWS for k in range(n)], pa.int32())})


def _stat_value(desc, raw):
    if raw is None:
        return None
    t = desc.physical_type
    if t == abi.INT32:
        return struct.unpack("<I" if desc.flags & 1 else "<i", raw)[0]
    if t == abi.INT64:
        return struct.unpack("<Q" if desc.flags & 1 else "<q", raw)[0]
    if t == abi.FLOAT:
        return struct.unpack("<f", raw)[0]
    if t == abi.DOUBLE:
        return struct.unpack("<d", raw)[0]
    if t == abi.BOOLEAN:
        return bool(raw[0])
    return raw


def _same(a, b):
    if isinstance(a, float) and isinstance(b, float):
        return struct.pack("<d", a) == struct.pack("<d", b)  # the sign of a zero too
    if isinstance(b, str):
        b = b.encode()
    return a == b


@pytest.mark.parametrize("nan", [False, True], ids=["plain", "nan_zero"])
def test_chunk_stats_equal_pyarrow(nan):
    data = _write(_table(nan))
    pf = pqgpu.ParquetFile(data)
    md = pq.ParquetFile(io.BytesIO(data)).metadata
    assert pf.num_row_groups == 3
    seen_all_null = seen_nulls = 0
    for rg in range(3):
        for c in range(pf.num_columns):
            st = md.row_group(rg).column(c).statistics
            lo, hi, nulls = pf.chunk_stats(rg, c)
            desc = pf.columns[c].desc
            assert st is not None and nulls == st.null_count
            if st.has_min_max:
                assert _same(_stat_value(desc, lo), st.min) and _same(_stat_value(desc, hi), st.max), (rg, c)
            else:
                assert lo is None and hi is None
                seen_all_null += nulls == ROWS
            seen_nulls += 0 < nulls < ROWS
    assert seen_all_null == 1 and seen_nulls >= 3


def test_chunk_stats_absent():
    pf = pqgpu.ParquetFile(_write(_table(), write_statistics=False))
    for rg in range(pf.num_row_groups):
        for c in range(pf.num_columns):
            assert pf.chunk_stats(rg, c) == (None, None, -1)
    with pytest.raises(pqgpu.PqgError):
        pf.chunk_stats(3, 0)
    with pytest.raises(pqgpu.PqgError):
        pf.chunk_stats(0, pf.num_columns)


def test_statistics_struct_cut_short():
    """One chunk's Statistics struct loses its STOP byte to a field header of an unknown type.  The
    generic skip of the footer parse reads that as the struct's end, as it always did, so the file
    opens and plans exactly as before; the statistics reader does not accept it, and then no chunk
    of the file reports statistics."""
    data = bytearray(_write(pa.table({"a": pa.array([-7777777, 5, 9], pa.int64()), "b": pa.array(["x", "y", "z"])})))
    good = pqgpu.ParquetFile(bytes(data))
    assert good.chunk_stats(0, 0) == (struct.pack("<q", -7777777), struct.pack("<q", 9), 0)
    flen = int.from_bytes(data[-8:-4], "little")
    foot = len(data) - 8 - flen
    # field 5 (max_value: two past null_count) and field 6 (min_value), binaries of 8 bytes each
    at = data.index(b"\x28\x08" + struct.pack("<q", 9) + b"\x18\x08" + struct.pack("<q", -7777777), foot) + 20
    while data[at] in (0x11, 0x12):  # is_max_value_exact / is_min_value_exact: one byte each
        at += 1
    assert data[at] == 0x00  # the struct's STOP
    data[at] = 0x1F          # field id + 1, type 15: no such type
    bad = pqgpu.ParquetFile(bytes(data))
    assert (bad.num_columns, bad.num_row_groups, bad.num_rows) == (2, 1, 3)
    for c in range(2):
        assert bytes(bad.chunk_meta(0, c)) == bytes(good.chunk_meta(0, c))
        assert bad.chunk_stats(0, c) == (None, None, -1)
    r = pqgpu.FileReader(bytes(data), decoder=_NoGpu())
    assert r.prune_row_groups([("a", ">", 100)]) == [0]  # nothing to prune by
    assert pqgpu.FileReader(bytes(good.data), decoder=_NoGpu()).prune_row_groups([("a", ">", 100)]) == []


def test_crash_fixtures_still_open_or_fail_cleanly():
    """tests/golden/crash_files.json (the reference's fuzz-crash files): opening one ends in a status
    or a file, as before, and asking any chunk of an opened one for its statistics ends in a
    result or METADATA."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crash_files.json")
    files = json.load(open(path))["files"]
    assert files
    for f in files:
        try:
            pf = pqgpu.ParquetFile(bytes.fromhex(f["data"]))
        except pqgpu.PqgError:
            continue
        for rg in range(pf.num_row_groups):
            for c in range(pf.num_columns):
                try:
                    lo, hi, nulls = pf.chunk_stats(rg, c)
                    assert (lo is None or isinstance(lo, bytes)) and (hi is None or isinstance(hi, bytes))
                except pqgpu.PqgError as e:
                    assert e.code == abi.STATUS_CODES["METADATA"]


# ---- DNF parsing ------------------------------------------------------------------------------------
def test_parse_dnf():
    one = F.parse([("a", "=", 1), ("b", "not  in", (1, 2)), ("c", "IS", None), ("c", "is not", None)])
    assert len(one) == 1 and [t.op for t in one[0]] == [abi.OP_EQ, "not in", abi.OP_IS_NULL, abi.OP_NOT_NULL]
    assert one[0][1].values == [1, 2]
    two = F.parse([[("a", "<=", 1)], [("b", ">", 2), ("a", "!=", 3)]])
    assert [[t.op for t in c] for c in two] == [[abi.OP_LE], [abi.OP_GT, abi.OP_NE]]
    assert F.columns_of(two) == ["a", "b"]
    assert F.parse(None) is None
    steps = F.Term("a", "in", [5, 6, 7]).steps()
    assert steps == [(abi.OP_EQ, 5, abi.COMBINE_SET), (abi.OP_EQ, 6, abi.COMBINE_OR), (abi.OP_EQ, 7, abi.COMBINE_OR)]
    steps = F.Term("a", "not in", [5, 6]).steps()
    assert steps == [(abi.OP_NE, 5, abi.COMBINE_SET), (abi.OP_NE, 6, abi.COMBINE_AND)]
    for bad in ([], [()], [("a", "~", 1)], [("a", "is", 1)], [("a", "in", 5)], [("a", "in", "xy")], [[]], "a > 1"):
        with pytest.raises(ValueError):
            F.parse(bad)


def test_literals():
    d = abi.ColumnDesc(abi.INT32, -1, 1, 0, 0, 0)
    assert F.literal(d, -2) == struct.pack("<i", -2)
    with pytest.raises(ValueError):
        F.literal(d, 2 ** 31)
    d.flags = abi.COL_UNSIGNED
    assert F.literal(d, 2 ** 31) == struct.pack("<I", 2 ** 31)
    with pytest.raises(ValueError):
        F.literal(d, -1)
    assert F.literal(abi.ColumnDesc(abi.DOUBLE, -1, 0, 0, 0, 0), 1) == struct.pack("<d", 1.0)
    assert F.literal(abi.ColumnDesc(abi.BYTE_ARRAY, -1, 0, 0, 0, 0), "é") == b"\xc3\xa9"
    assert F.literal(abi.ColumnDesc(abi.BOOLEAN, -1, 0, 0, 0, 0), True) == b"\x01"


# ---- pruning ---------------------------------------------------------------------------------------
OPS = ["==", "!=", "<", "<=", ">", ">="]
LITERALS = {
    "i64": [-500, -501, -110, 0, 290, 300, 690, 700, 10 ** 12],
    "i32": [-2 ** 31, 0, 39, 40, 119, 120, 2 ** 31 - 1],
    "u32": [0, 39 * 35_000_000, 2 ** 31, 2 ** 31 + 1, 79 * 35_000_000, 119 * 35_000_000, 2 ** 32 - 1],
    "f32": [-10.0, -10.5, 0.0, -0.0, 9.5, 10.0, 49.5, 50.0, NAN, float("inf")],
    "f64": [-5.0, 0.0, -0.0, 4.75, 5.0, 24.75, 25.0, NAN, float("-inf")],
    "s": ["", "000", "039", "04", "079", "08", "119", "12", "\u0080x", "\u0080", "zzz"],
    "const": ["same", "sam", "samf", "b0", "b9", "a"],
    "flba": [bytes([0, 255, 0x80]), bytes([39, 216, 0x80]), bytes([40, 0, 0]), bytes([119, 136, 0x80]), b"\xff\xff\xff"],
    "b": [False, True],
    "n": [-1.0, 0.0, 79.0, 80.0],
}


def _passes(v, op, lit):
    """pqg_filter's rule for one row: a null passes only `is null`; Python's float comparisons are
    IEEE (NaN != x, nothing else)."""
    if op == "is":
        return v is None
    if v is None:
        return False
    if op == "is not":
        return True
    if op == "in":
        return any(v == x for x in lit)
    if op == "not in":
        return all(v != x for x in lit)
    if isinstance(v, str):
        v = v.encode()
    if isinstance(lit, str):
        lit = lit.encode()
    return {"==": v == lit, "=": v == lit, "!=": v != lit, "<": v < lit, "<=": v <= lit, ">": v > lit, ">=": v >= lit}[op]


def _selected_groups(cols, dnf):
    n = len(cols["rg"])
    out = set()
    for k in range(n):
        if any(all(_passes(cols[c][k], op, lit) for c, op, lit in conj) for conj in dnf):
            out.add(cols["rg"][k])
    return out


def _filters_for(col):
    lits = LITERALS[col]
    fs = [[(col, op, v)] for op in OPS for v in lits]
    fs += [[(col, "is", None)], [(col, "is not", None)], [(col, "in", lits[:3])], [(col, "in", [])],
           [(col, "not in", lits[-2:])], [(col, "in", lits[-1:])]]
    return fs


@pytest.mark.parametrize("nan", [False, True], ids=["plain", "nan_zero"])
def test_prune_is_sound_for_every_operator_and_type(nan):
    t = _table(nan)
    data = _write(t)
    r = pqgpu.FileReader(data, decoder=_NoGpu())
    cols = {name: t.column(name).to_pylist() for name in t.column_names}
    pruned_some = 0
    for col in LITERALS:
        for f in _filters_for(col):
            kept = r.prune_row_groups(f)
            need = _selected_groups(cols, [f])
            assert need <= set(kept), (f, kept, need)
            pruned_some += len(kept) < 3
    assert pruned_some > 100  # the check is not vacuous
    # conjunctions and disjunctions
    dnf = [[("i64", ">", 290), ("s", "<", "08")], [("n", "is", None), ("b", "==", True)]]
    assert _selected_groups(cols, dnf) <= set(r.prune_row_groups(dnf))
    assert r.prune_row_groups([[("i64", ">", 10 ** 9)], [("i32", "<", -2 ** 31)]]) == []
    assert r.prune_row_groups([("n", "is", None), ("rg", "==", 1)]) == []  # n's nulls are in row group 0


def test_prune_float_rules():
    """Never on != / not in; never on a NaN bound; a zero minimum counts as -0.0, a zero maximum as 0.0."""
    d = abi.ColumnDesc(abi.DOUBLE, -1, 1, 0, 0, 0)
    p = lambda x: struct.pack("<d", x)
    out = lambda op, v, lo, hi, nulls=0: F.term_rules_out(d, F.parse([("x", op, v)])[0][0], (lo, hi, nulls), 10)
    assert not out("!=", 1.0, p(1.0), p(1.0))
    assert not out("not in", [1.0], p(1.0), p(1.0))
    assert out("==", 2.0, p(1.0), p(1.0)) and not out("==", 2.0, p(NAN), p(1.0)) and not out("<", 0.0, p(1.0), p(NAN))
    # a minimum of 0.0 may stand for a row of -0.0, and the two are equal in every comparison
    assert not out("==", -0.0, p(0.0), p(5.0)) and not out("<=", -0.0, p(0.0), p(5.0)) and out("<", 0.0, p(0.0), p(5.0))
    assert not out(">=", 0.0, p(-5.0), p(-0.0)) and out(">", 0.0, p(-5.0), p(-0.0))
    assert not out("==", NAN, p(1.0), p(2.0))
    assert out("==", 1.5, p(1.0), p(2.0), nulls=10) and not out("is", None, p(1.0), p(2.0), nulls=10)
    assert out("is", None, p(1.0), p(2.0), nulls=0) and not out("is", None, p(1.0), p(2.0), nulls=-1)
    assert not out("==", 5.0, None, p(2.0)) and not out("==", 5.0, p(1.0)[:4], p(2.0)) and not out("==", 5.0, p(3.0), p(2.0))
    i = abi.ColumnDesc(abi.INT32, -1, 1, 0, 0, 0)
    q = lambda x: struct.pack("<i", x)
    assert F.term_rules_out(i, F.parse([("x", "!=", 4)])[0][0], (q(4), q(4), 3), 10)
    assert not F.term_rules_out(i, F.parse([("x", "!=", 4)])[0][0], (q(4), q(5), 0), 10)
    assert not F.term_rules_out(i, F.parse([("x", "==", 2 ** 40)])[0][0], (q(4), q(5), 0), 10)  # no such int32: in doubt


def test_prune_equals_pyarrow_on_nan_free_file():
    """On the NaN-free file, for filters that the row groups' disjoint ranges decide exactly, the row
    groups kept are those that contribute rows to pq.read_table(filters=...)."""
    t = _table(nan=False)
    data = _write(t)
    r = pqgpu.FileReader(data, decoder=_NoGpu())
    fs = [[("i64", ">", 290)], [("i64", "<=", -110)], [("i32", "==", 40)], [("i32", "in", [1, 119])],
          [("u32", ">=", 2 ** 31)], [("u32", "<", 35_000_000 * 40)], [("f32", "<", 10.0)], [("f64", ">=", 25.0)],
          [("s", ">", "08")], [("s", "==", "\u0080x")], [("const", "!=", "same")], [("const", "==", "b3")],
          [("flba", "<", bytes([40, 0, 0]))], [("b", "==", False)], [("n", "is", None)], [("n", "is not", None)],
          [("n", ">", 39.5)], [("i64", ">", 290), ("s", "<", "08")],
          [[("i64", "<", -400)], [("f64", ">", 24.0)]], [("i64", ">", 10 ** 9)]]
    import pyarrow.compute as pc
    as_expr = {"is": lambda c: pc.field(c).is_null(), "is not": lambda c: pc.field(c).is_valid()}
    for f in fs:
        # pyarrow's DNF has no `is` / `is not`: those two go as expressions
        pf = as_expr[f[0][1]](f[0][0]) if len(f) == 1 and f[0][1] in as_expr else f
        got = pq.read_table(io.BytesIO(data), filters=pf)
        want = sorted(set(got.column("rg").to_pylist()))
        assert r.prune_row_groups(f) == want, f
