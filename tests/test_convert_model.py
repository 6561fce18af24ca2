"""Logical types without a GPU: the numpy model the GPU tests judge pqg_convert by (convert_util)
against pyarrow, the footer planner's logical types against pyarrow's schema, the lane code of the
conversion kernels (pqg_convert.h) run on the host by tools/convert_model.cpp, and the typed
literals and orders of pqgpu.filters.

The first two tests pass with or without the feature: they pin the yardstick, not the kernels."""
import datetime
import decimal
import io
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import convert_util as CU
import parity as P
import pqgpu
from pqgpu import abi
from pqgpu import filters as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = decimal.Decimal

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")


# ---- 1. the yardstick ---------------------------------------------------------------------------

@pytest.mark.parametrize("as_integer", [False, True])
def test_model_matches_pyarrow_decimals(as_integer):
    """The oracle's raw values of pyarrow-written decimals through the model are the bytes pyarrow reads."""
    names = ("d7", "d15") if as_integer else ("d7", "d30", "d50")
    table = CU.decimal_table(2000, names=names)
    data = CU.write(table, store_decimal_as_integer=True) if as_integer else CU.write(table)
    pf = pqgpu.ParquetFile(data)
    got = CU.read(data)
    want_type = {"d7": (abi.INT32, 4), "d15": (abi.INT64, 8)} if as_integer else \
        {"d7": (abi.FIXED_LEN_BYTE_ARRAY, 4), "d30": (abi.FIXED_LEN_BYTE_ARRAY, 13), "d50": (abi.FIXED_LEN_BYTE_ARRAY, 21)}
    for c, name in enumerate(names):
        desc = pf.columns[c].desc
        ptype, w = want_type[name]
        assert desc.physical_type == ptype
        assert as_integer or desc.type_length == w
        exp = P.oracle_chunk(pf, 0, c)
        assert exp.status == 0 and exp.value_width == w and exp.num_values == 1600
        ow = 16 if CU.DECIMALS[name][0] <= 38 else 32
        model = CU.int_to_le(exp.values, w, ow) if as_integer else CU.decimal_be_to_le(exp.values, w, ow)
        assert np.array_equal(model, CU.value_bytes(got[name], ow)), name


def test_model_matches_pyarrow_int96():
    table = CU.int96_table(2000)
    data = CU.write(table, use_deprecated_int96_timestamps=True)
    pf = pqgpu.ParquetFile(data)
    assert pf.columns[0].desc.physical_type == abi.INT96
    exp = P.oracle_chunk(pf, 0, 0)
    assert exp.status == 0 and exp.value_width == 12
    ns = table["ts"].combine_chunks().drop_null().cast(pa.int64()).to_numpy()
    assert list(ns[:8]) == CU.INT96_NS
    assert np.array_equal(exp.values, CU.int96_bytes(ns))
    for unit in ("ns", "us", "ms", "s"):
        got = CU.read(data, coerce_int96_timestamp_unit=unit)["ts"]
        assert str(got.type) == "timestamp[%s]" % unit
        want = CU.value_bytes(got, 8).view("<i8")
        model = CU.int96_to_time(exp.values, unit)
        assert np.array_equal(model, want), unit
    # what the project checked by hand on pyarrow 25.0.0
    head = CU.int96_bytes(CU.INT96_NS[:6])
    assert CU.int96_to_time(head, "us").tolist() == [0, -1, 0, -86400000001, 4611686018427387, -4611686018427388]
    assert CU.int96_to_time(head, "s").tolist() == [0, -1, 0, -86401, 4611686018, -4611686019]


# ---- 2. the footer --------------------------------------------------------------------------------

KIND = {"NONE": abi.LT_NONE, "STRING": abi.LT_STRING, "DECIMAL": abi.LT_DECIMAL, "DATE": abi.LT_DATE,
        "TIME": abi.LT_TIME, "TIMESTAMP": abi.LT_TIMESTAMP, "INT": abi.LT_INTEGER, "FLOAT16": abi.LT_FLOAT16}
UNIT = {"milliseconds": abi.UNIT_MILLIS, "microseconds": abi.UNIT_MICROS, "nanoseconds": abi.UNIT_NANOS}
CONVERTED = {"UTF8": 0, "DECIMAL": 5, "DATE": 6, "TIME_MILLIS": 7, "TIME_MICROS": 8, "TIMESTAMP_MILLIS": 9,
             "TIMESTAMP_MICROS": 10, "UINT_8": 11, "UINT_16": 12, "UINT_32": 13, "UINT_64": 14, "INT_8": 15,
             "INT_16": 16, "INT_32": 17, "INT_64": 18}


def fields(lt):
    return {f: getattr(lt, f) for f, _ in abi.LogicalType._fields_}


def check_against_pyarrow(data):
    pf = pqgpu.ParquetFile(data)
    schema = pq.ParquetFile(io.BytesIO(data)).schema
    assert len(pf.logical_types) == pf.num_columns == len(schema.names)
    seen = set()
    for i, lt in enumerate(pf.logical_types):
        col = schema.column(i)
        assert col.path == pf.columns[i].path.decode()
        js = json.loads(col.logical_type.to_json())
        want = dict(kind=KIND[col.logical_type.type], precision=0, scale=0, unit=0, utc=0, bit_width=0, is_signed=0)
        if want["kind"] == abi.LT_DECIMAL:
            want.update(precision=col.precision, scale=col.scale)
            assert (js["precision"], js["scale"]) == (col.precision, col.scale)
        if want["kind"] in (abi.LT_TIME, abi.LT_TIMESTAMP):
            want.update(unit=UNIT[js["timeUnit"]], utc=int(js["isAdjustedToUTC"]))
        if want["kind"] == abi.LT_INTEGER:
            want.update(bit_width=js["bitWidth"], is_signed=int(js["isSigned"]))
        got = fields(lt)
        conv = got.pop("converted_type")
        assert got == want, col.path
        if col.converted_type != "NONE":  # pyarrow hides the converted type of a local timestamp
            assert conv == CONVERTED[col.converted_type], col.path
        seen.add(want["kind"])
    return pf, seen


# (path, physical_type, type_length, max_def, max_rep, codec, flags): what the commit before the
# logical types reported for these files; every one of them must stay
DESC_LOGICAL = [
    ('dec_flba', 7, 4, 1, 0, 0, 0), ('dec_wide', 7, 21, 1, 0, 0, 0), ('ts_ms', 2, -1, 1, 0, 0, 0),
    ('ts_ms_utc', 2, -1, 1, 0, 0, 0), ('ts_us', 2, -1, 1, 0, 0, 0), ('ts_us_utc', 2, -1, 1, 0, 0, 0),
    ('ts_ns', 2, -1, 1, 0, 0, 0), ('ts_ns_utc', 2, -1, 1, 0, 0, 0), ('date', 1, -1, 1, 0, 0, 0),
    ('t32', 1, -1, 1, 0, 0, 0), ('t64', 2, -1, 1, 0, 0, 0), ('u8', 1, -1, 1, 0, 0, 1), ('u16', 1, -1, 1, 0, 0, 1),
    ('u32', 1, -1, 1, 0, 0, 1), ('u64', 2, -1, 1, 0, 0, 1), ('i8', 1, -1, 1, 0, 0, 0), ('i16', 1, -1, 1, 0, 0, 0),
    ('i32', 1, -1, 1, 0, 0, 0), ('i64', 2, -1, 1, 0, 0, 0), ('s', 6, -1, 1, 0, 0, 0), ('f16', 7, 2, 1, 0, 0, 0),
    ('lst.list.element', 7, 4, 3, 1, 0, 0),
]
DESC_INT = [('dec_i32', 1, -1, 1, 0, 0, 0), ('dec_i64', 2, -1, 1, 0, 0, 0)]
DESC_INT96 = [('ts', 3, -1, 1, 0, 0, 0)]
DESC_CONVERTED = [('dec', 7, 5, 1, 0, 0, 0), ('ts', 2, -1, 1, 0, 0, 0), ('u32', 1, -1, 0, 0, 0, 1), ('s', 6, -1, 1, 0, 0, 0)]


def descs(pf):
    return [(c.path.decode(), c.desc.physical_type, c.desc.type_length, c.desc.max_def, c.desc.max_rep, c.desc.codec,
             c.desc.flags) for c in pf.columns]


def test_footer_logical_types_match_pyarrow():
    pf, seen = check_against_pyarrow(CU.write(CU.logical_table()))
    assert seen == set(KIND.values())
    assert descs(pf) == DESC_LOGICAL
    pf, _ = check_against_pyarrow(CU.write(CU.logical_int_table(), store_decimal_as_integer=True))
    assert [lt.kind for lt in pf.logical_types] == [abi.LT_DECIMAL] * 2
    assert descs(pf) == DESC_INT
    # pyarrow's INT96 switch turns every timestamp column into an INT96 one: a file of its own
    pf, _ = check_against_pyarrow(CU.write(CU.int96_table(20), use_deprecated_int96_timestamps=True))
    assert fields(pf.logical_types[0]) == dict(kind=0, precision=0, scale=0, unit=0, utc=0, bit_width=0, is_signed=0,
                                               converted_type=-1)
    assert descs(pf) == DESC_INT96


CONVERTED_LEAVES = [
    dict(name="dec", typ=7, type_length=5, rep=1, converted=5, scale=2, precision=11),
    dict(name="ts", typ=2, rep=1, converted=10),
    dict(name="u32", typ=1, rep=0, converted=13),
    dict(name="s", typ=6, rep=1, converted=0)]


def test_footer_converted_types_only():
    """A footer as parquet-go writes it: no LogicalType union anywhere (pyarrow always writes one, so
    the SchemaElements are built here)."""
    data = CU.converted_only_file(CONVERTED_LEAVES)
    schema = pq.ParquetFile(io.BytesIO(data)).schema  # pyarrow reads the hand-built footer too
    assert [schema.column(i).converted_type for i in range(4)] == ["DECIMAL", "TIMESTAMP_MICROS", "UINT_32", "UTF8"]
    pf = pqgpu.ParquetFile(data)
    zero = dict(kind=0, precision=0, scale=0, unit=0, utc=0, bit_width=0, is_signed=0, converted_type=-1)
    assert [fields(lt) for lt in pf.logical_types] == [
        dict(zero, kind=abi.LT_DECIMAL, precision=11, scale=2, converted_type=5),
        dict(zero, kind=abi.LT_TIMESTAMP, unit=abi.UNIT_MICROS, utc=1, converted_type=10),
        dict(zero, kind=abi.LT_INTEGER, bit_width=32, is_signed=0, converted_type=13),
        dict(zero, kind=abi.LT_STRING, converted_type=0)]
    assert descs(pf) == DESC_CONVERTED
    # nothing is validated: a precision of 0 is reported as 0, a missing one too
    data = CU.converted_only_file([dict(name="d", typ=2, rep=1, converted=5, scale=3, precision=0),
                                   dict(name="e", typ=1, rep=1, converted=5)])
    pf = pqgpu.ParquetFile(data)
    assert [(lt.kind, lt.precision, lt.scale) for lt in pf.logical_types] == [(abi.LT_DECIMAL, 0, 3), (abi.LT_DECIMAL, 0, 0)]


# ---- 3. the host model of the kernels ------------------------------------------------------------

def build_model(tmp_path, name, extra=()):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / name)
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wno-unknown-pragmas", *extra, "-I",
                    os.path.join(ROOT, "parquet-go_amd", "csrc"), os.path.join(ROOT, "tools", "convert_model.cpp"),
                    "-o", exe], check=True)
    return exe


def test_host_model_of_the_kernels(tmp_path):
    """tools/convert_model.cpp: pqg_convert.h's lane code over the sweep of widths, counts, alignments
    and value patterns, every load and store checked against what it may touch."""
    r = subprocess.run([build_model(tmp_path, "convert_model")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


def test_host_model_sanitizer_clean(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined."""
    exe = build_model(tmp_path, "convert_model_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


# ---- 4. literals and orders ----------------------------------------------------------------------

def lt_decimal(precision, scale):
    return abi.LogicalType(kind=abi.LT_DECIMAL, precision=precision, scale=scale)


def flba(w, flags=0):
    return abi.ColumnDesc(abi.FIXED_LEN_BYTE_ARRAY, w, 1, 0, 0, flags)


def test_decimal_literals():
    d4, lt = flba(4), lt_decimal(7, 2)
    assert F.literal(d4, D("-1.23"), lt) == bytes([0xff, 0xff, 0xff, 0x85])
    assert F.literal(d4, D("1.23"), lt) == bytes([0, 0, 0, 0x7b])
    assert F.literal(d4, 5, lt) == (500).to_bytes(4, "big")
    assert F.literal(d4, D("1.2"), lt) == (120).to_bytes(4, "big")
    assert F.literal(d4, D("1E+2"), lt) == (10000).to_bytes(4, "big")
    assert F.literal(flba(13), D("-0.01"), lt_decimal(30, 2)) == b"\xff" * 13
    for bad in (D("1.234"), D("21474836.48"), D("-21474836.49"), D("NaN"), D("Infinity")):
        with pytest.raises(ValueError):
            F.literal(d4, bad, lt)
    assert F.literal(d4, D("21474836.47"), lt) == b"\x7f\xff\xff\xff"
    assert F.literal(d4, D("-21474836.48"), lt) == b"\x80\x00\x00\x00"
    i32 = abi.ColumnDesc(abi.INT32, -1, 1, 0, 0, 0)
    i64 = abi.ColumnDesc(abi.INT64, -1, 1, 0, 0, 0)
    assert F.literal(i32, D("-1.23"), lt) == np.int32(-123).tobytes()
    assert F.literal(i64, D("-1.234"), lt_decimal(15, 3)) == np.int64(-1234).tobytes()
    with pytest.raises(ValueError):
        F.literal(i32, D("21474836.48"), lt)
    with pytest.raises(ValueError):
        F.literal(i64, D("0.0001"), lt_decimal(15, 3))
    # without the logical type everything is as it was
    assert F.literal(d4, b"abcd") == b"abcd" and F.literal(i32, -123) == np.int32(-123).tobytes()
    assert F.literal(d4, b"abcd", lt) == b"abcd"


def test_signed_order_of_decimals():
    rng = np.random.default_rng(5)
    vals = [D(int(v)).scaleb(-2) for v in rng.integers(-2 ** 31, 2 ** 31, 200)] + [D(0), D("-0.01"), D("0.01")]
    lt = lt_decimal(10, 2)
    for desc, logical in ((flba(5), lt), (flba(5, abi.COL_SIGNED_BE), None)):
        lits = [F.literal(flba(5), v, lt) for v in vals]
        import functools
        order = sorted(range(len(vals)), key=functools.cmp_to_key(lambda a, b: F.compare(desc, lits[a], lits[b], logical)))
        assert [vals[i] for i in order] == sorted(vals)
    # without flag or logical type the order stays unsigned lexicographic: a negative sorts above
    assert F.compare(flba(5), F.literal(flba(5), D(-1), lt), F.literal(flba(5), D(1), lt)) == 1
    assert F.compare(flba(5), F.literal(flba(5), D(-1), lt), F.literal(flba(5), D(1), lt), lt) == -1
    assert F.compare(flba(5), b"\x00" * 4, b"\x00" * 5, lt) is None


def test_time_literals():
    i64 = abi.ColumnDesc(abi.INT64, -1, 1, 0, 0, 0)
    i32 = abi.ColumnDesc(abi.INT32, -1, 1, 0, 0, 0)
    when = datetime.datetime(2021, 3, 4, 5, 6, 7, 891000)
    for unit, name in ((abi.UNIT_MILLIS, "ms"), (abi.UNIT_MICROS, "us"), (abi.UNIT_NANOS, "ns")):
        lt = abi.LogicalType(kind=abi.LT_TIMESTAMP, unit=unit)
        want = np.datetime64(when).astype("datetime64[%s]" % name).astype(np.int64)
        assert F.literal(i64, when, lt) == want.tobytes()
        assert F.literal(i64, np.datetime64(when), lt) == want.tobytes()
        assert F.literal(i64, np.datetime64("1969-12-31T23:59:59"), lt) == \
            np.datetime64("1969-12-31T23:59:59").astype("datetime64[%s]" % name).astype(np.int64).tobytes()
        assert F.literal(i64, 17, lt) == np.int64(17).tobytes()  # plain integers stay the column's own unit
    aware = when.replace(tzinfo=datetime.timezone(datetime.timedelta(hours=2)))
    lt_us = abi.LogicalType(kind=abi.LT_TIMESTAMP, unit=abi.UNIT_MICROS)
    assert F.literal(i64, aware, lt_us) == (np.datetime64(when).astype("datetime64[us]").astype(np.int64)
                                            - 7200 * 10 ** 6).tobytes()
    with pytest.raises(ValueError):  # microseconds that milliseconds cannot hold
        F.literal(i64, when.replace(microsecond=891001), abi.LogicalType(kind=abi.LT_TIMESTAMP, unit=abi.UNIT_MILLIS))
    lt_date = abi.LogicalType(kind=abi.LT_DATE)
    day = datetime.date(1969, 7, 20)
    want = np.datetime64(day).astype("datetime64[D]").astype(np.int64).astype(np.int32)
    assert F.literal(i32, day, lt_date) == want.tobytes() and int(want) == -165
    assert F.literal(i32, np.datetime64("1969-07-20"), lt_date) == want.tobytes()
    with pytest.raises(ValueError):
        F.literal(i32, datetime.datetime(1969, 7, 20, 1), lt_date)


class NoDecoder:
    """prune_row_groups is host only: a reader that must not touch a GPU gets this decoder."""


def test_prune_row_groups_orders_decimal_statistics_signed():
    neg = [D(-i - 1).scaleb(-2) for i in range(100)]
    pos = [D(i + 1).scaleb(-2) for i in range(100)]
    data = CU.write(pa.table({"d": pa.array(neg + pos, pa.decimal128(7, 2))}), row_group_size=100)
    fr = pqgpu.FileReader(data, decoder=NoDecoder(), convert_logical=True)
    assert fr.file.num_row_groups == 2 and fr.file.columns[0].desc.physical_type == abi.FIXED_LEN_BYTE_ARRAY
    lo, hi, _ = fr.file.chunk_stats(0, 0)
    assert (lo, hi) == (F.literal(flba(4), D("-1.00"), lt_decimal(7, 2)), F.literal(flba(4), D("-0.01"), lt_decimal(7, 2)))
    assert fr.prune_row_groups([("d", "<", D(0))]) == [0]
    assert fr.prune_row_groups([("d", ">", D(0))]) == [1]
    assert fr.prune_row_groups([("d", ">=", D("-0.01"))]) == [0, 1]
    assert fr.prune_row_groups([("d", "in", [D("-0.50"), D("-2.00")])]) == [0]
    assert fr.prune_row_groups([("d", "==", D("0.001"))]) == [0, 1]  # not exact at the scale: nothing is ruled out
    # the default reader keeps what it did: bytes literals in unsigned order
    raw = pqgpu.FileReader(data, decoder=NoDecoder())
    assert raw.prune_row_groups([("d", "<", b"\x80\x00\x00\x00")]) == [1]
    # an INT96 column never prunes
    data = CU.write(CU.int96_table(200), use_deprecated_int96_timestamps=True, row_group_size=100)
    fr = pqgpu.FileReader(data, decoder=NoDecoder(), convert_logical=True)
    assert fr.prune_row_groups([("ts", "<", datetime.datetime(1700, 1, 1))]) == [0, 1]


def test_abi_mirrors_the_header():
    import ctypes as C
    assert C.sizeof(abi.LogicalType) == 32 and C.sizeof(abi.ConvertArgs) == 64
    assert abi.ConvertArgs.out.offset == 48 and abi.ConvertArgs.num_bad.offset == 56
    text = open(os.path.join(ROOT, "include", "pqgpu.h")).read()
    assert "PQG_COL_SIGNED_BE = %d" % abi.COL_SIGNED_BE in text
    assert "PQG_LT_FLOAT16, PQG_LT_OTHER" in text and abi.LT_OTHER == 12 and abi.UNIT_NANOS == 4
