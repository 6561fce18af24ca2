"""Logical-type conversion on the GPU: pqg_convert against the numpy model that test_convert_model.py
pins to pyarrow, FileReader(convert_logical=True) end to end against pyarrow (plain, kept
dictionaries, filtered, nested), and pqg_filter's signed big-endian order."""
import ctypes as C
import decimal
import io

import numpy as np
import pytest

import convert_util as CU
import parity as P
import pqgpu
from pqgpu import abi

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")

pytestmark = pytest.mark.gpu

D = decimal.Decimal
INVALID_ARG, SIZE, UNSUPPORTED = (abi.STATUS_CODES[k] for k in ("INVALID_ARG", "SIZE", "UNSUPPORTED"))
COUNTS = (0, 1, 64, 65, 4096, 4097, 8193)  # lane, segment (4096) and tile edges
FILL = 0x3C


@pytest.fixture(scope="module")
def dec():
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


class Out:
    """A device output buffer of `cap` bytes and 16 guard bytes, refilled with FILL before each call."""

    def __init__(self, dec, cap):
        self.dec, self.cap = dec, cap
        self.fill = np.full(cap + 16, FILL, np.uint8)
        self.ptr = dec.upload(self.fill)

    def reset(self):
        rc = self.dec.L.pqg_memcpy_h2d(self.dec.ctx, C.c_void_p(self.ptr), self.fill.ctypes.data, self.cap + 16)
        assert rc == 0

    def get(self):
        return self.dec.d2h(self.ptr, self.cap + 16)

    def free(self):
        self.dec.free(self.ptr)


def convert(dec, values, n, values_bytes, kind, w, ow, out, unit=0, offsets=None):
    a = abi.ConvertArgs()
    a.values, a.offsets, a.num_values, a.values_bytes = values or None, offsets or None, n, values_bytes
    a.kind, a.in_width, a.out_width, a.unit, a.out = kind, w, ow, unit, out or None
    a.num_bad = -7
    return dec.L.pqg_convert(dec.ctx, C.byref(a)), a


def check(out, n_bytes, want):
    got = out.get()
    assert np.array_equal(got[:n_bytes], want)
    assert (got[n_bytes:] == FILL).all(), "bytes past the output changed"


# ---- 5. pqg_convert against the model --------------------------------------------------------------

@pytest.mark.parametrize("w,ow", [(w, 16) for w in (1, 2, 3, 4, 5, 8, 9, 12, 13, 16)] + [(w, 32) for w in (16, 17, 21, 32)])
def test_decimal_be_fixed(dec, w, ow):
    rng = np.random.default_rng(w * 100 + ow)
    nmax = max(COUNTS)
    host = rng.integers(0, 256, nmax * w + 16, dtype=np.uint8)
    dev = dec.upload(host)
    out = Out(dec, nmax * ow)
    try:
        for off in (0, 1, 7, 15):
            for n in COUNTS:
                out.reset()
                rc, a = convert(dec, dev + off, n, n * w, abi.CONV_DECIMAL_BE, w, ow, out.ptr)
                assert rc == 0 and a.num_bad == 0, (off, n)
                check(out, n * ow, CU.decimal_be_to_le(host[off:off + n * w], w, ow))
    finally:
        out.free()
        dec.free(dev)


def test_decimal_be_edge_values(dec):
    for w, ow in ((1, 16), (5, 16), (16, 16), (17, 32), (32, 32)):
        pats = [bytes(w), b"\xff" * w, b"\x80" + bytes(w - 1), b"\x7f" + b"\xff" * (w - 1)]
        host = np.frombuffer(b"".join(pats) * 70, np.uint8)  # 280 values: five rounds of a wave
        dev = dec.upload(np.r_[np.zeros(3, np.uint8), host])
        out = Out(dec, 280 * ow)
        try:
            rc, _ = convert(dec, dev + 3, 280, 280 * w, abi.CONV_DECIMAL_BE, w, ow, out.ptr)
            assert rc == 0
            check(out, 280 * ow, CU.decimal_be_to_le(host, w, ow))
            got = out.get()[:4 * ow].reshape(4, ow)
            assert not got[0].any() and (got[1] == 0xff).all()
            assert got[2][w - 1] == 0x80 and (got[2][w:] == 0xff).all() and not got[2][:w - 1].any()
            assert got[3][w - 1] == 0x7f and not got[3][w:].any()
        finally:
            out.free()
            dec.free(dev)


@pytest.mark.parametrize("w", [4, 8])
@pytest.mark.parametrize("ow", [16, 32])
def test_decimal_int(dec, w, ow):
    rng = np.random.default_rng(w + ow)
    nmax = max(COUNTS)
    host = rng.integers(0, 256, nmax * w + 16, dtype=np.uint8)
    dev = dec.upload(host)
    out = Out(dec, nmax * ow)
    try:
        for off in (0, 1, 7, 15):
            for n in COUNTS:
                out.reset()
                rc, _ = convert(dec, dev + off, n, n * w, abi.CONV_DECIMAL_INT, w, ow, out.ptr)
                assert rc == 0, (off, n)
                check(out, n * ow, CU.int_to_le(host[off:off + n * w], w, ow))
    finally:
        out.free()
        dec.free(dev)


@pytest.mark.parametrize("unit", ["s", "ms", "us", "ns"])
def test_int96_time(dec, unit):
    rng = np.random.default_rng(96)
    n = 8 + 10000
    vals = np.zeros((n, 12), np.uint8)
    vals[:8] = CU.int96_bytes(CU.INT96_NS).reshape(8, 12)
    vals[8:] = rng.integers(0, 256, (10000, 12), dtype=np.uint8)  # any day, nanos at and above 2^63 too
    vals[8, 8:] = np.frombuffer(np.int32(2 ** 31 - 1).tobytes(), np.uint8)
    vals[9, 8:] = np.frombuffer(np.int32(-2 ** 31).tobytes(), np.uint8)
    vals[10] = 0  # a dictionary's nil entry
    host = np.r_[vals.reshape(-1), np.zeros(16, np.uint8)]
    out = Out(dec, n * 8)
    devs = []
    try:
        for off in (0, 1, 7, 15):
            dev = dec.upload(np.r_[np.zeros(off, np.uint8), host])
            devs.append(dev)
            for k in (n, 8, 129, 641):
                out.reset()
                rc, _ = convert(dec, dev + off, k, k * 12, abi.CONV_INT96_TIME, 12, 8, out.ptr, unit=abi.UNITS[unit])
                assert rc == 0
                want = CU.int96_to_time(host[:k * 12], unit)
                check(out, k * 8, want.view(np.uint8))
        # as pyarrow reads the hand-checked values
        if unit == "us":
            assert want[:6].tolist() == [0, -1, 0, -86400000001, 4611686018427387, -4611686018427388]
        if unit == "s":
            assert want[:6].tolist() == [0, -1, 0, -86401, 4611686018, -4611686019]
    finally:
        out.free()
        for d in devs:
            dec.free(d)


def byte_array_case(lens, rng):
    offs = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    chars = rng.integers(0, 256, max(int(offs[-1]), 1), dtype=np.uint8)
    return chars, offs


@pytest.mark.parametrize("ow", [16, 32])
def test_decimal_byte_arrays(dec, ow):
    rng = np.random.default_rng(ow)
    out = Out(dec, 8193 * ow)
    try:
        for n in (0, 1, 65, 4097, 8193):
            lens = rng.integers(1, ow + 1, n)
            chars, offs = byte_array_case(lens, rng)
            dc, do = dec.upload(np.r_[np.zeros(1, np.uint8), chars]), dec.upload(offs)
            try:
                out.reset()
                rc, a = convert(dec, dc + 1, n, int(offs[-1]), abi.CONV_DECIMAL_BE, 0, ow, out.ptr, offsets=do)
                assert rc == 0 and a.num_bad == 0
                check(out, n * ow, CU.bytes_be_to_le(chars, offs, ow))
            finally:
                dec.free(dc)
                dec.free(do)
        # a length of 0 and a length above the output width are bad values: counted, nothing written
        for bad_lens, nbad in (([0], 1), ([ow + 1], 1), ([0, ow + 1, 0], 3)):
            lens = rng.integers(1, ow + 1, 5000)
            at = [17, 4096, 4000][:len(bad_lens)]  # not the last value: it goes bad below
            lens[at] = bad_lens
            chars, offs = byte_array_case(lens, rng)
            dc, do = dec.upload(chars), dec.upload(offs)
            try:
                out.reset()
                rc, a = convert(dec, dc, 5000, int(offs[-1]), abi.CONV_DECIMAL_BE, 0, ow, out.ptr, offsets=do)
                assert rc == SIZE and a.num_bad == nbad
                check(out, 0, np.zeros(0, np.uint8))
                # offsets that leave the chars are bad values too
                out.reset()
                rc, a = convert(dec, dc, 5000, int(offs[-1]) - 1, abi.CONV_DECIMAL_BE, 0, ow, out.ptr, offsets=do)
                assert rc == SIZE and a.num_bad == nbad + 1
                check(out, 0, np.zeros(0, np.uint8))
            finally:
                dec.free(dc)
                dec.free(do)
    finally:
        out.free()


def test_convert_argument_errors(dec):
    n = 100
    dev = dec.upload(np.zeros(n * 32, np.uint8))
    offs = dec.upload(np.arange(n + 1, dtype=np.int64))
    out = Out(dec, n * 32)
    BE, INT, T96 = abi.CONV_DECIMAL_BE, abi.CONV_DECIMAL_INT, abi.CONV_INT96_TIME
    try:
        def status(kind, w, ow, values_bytes=None, out_ptr=None, **kw):
            rc, _ = convert(dec, dev, n, n * max(w, 1) if values_bytes is None else values_bytes, kind, w, ow,
                            out.ptr if out_ptr is None else out_ptr, **kw)
            assert (out.get() == FILL).all()
            return rc

        assert status(BE, 17, 16) == INVALID_ARG          # wider than the output
        assert status(BE, 0, 16) == INVALID_ARG           # in_width outside 1..32
        assert status(BE, 33, 32) == INVALID_ARG
        assert status(BE, -1, 16) == INVALID_ARG
        assert status(BE, 4, 8) == INVALID_ARG            # out_width not 16 / 32
        assert status(BE, 4, 24) == INVALID_ARG
        assert status(BE, 4, 16, values_bytes=4 * n - 1) == INVALID_ARG
        assert status(BE, 4, 16, out_ptr=out.ptr + 8) == INVALID_ARG
        assert status(BE, 4, 16, offsets=offs) == INVALID_ARG  # byte arrays take in_width 0
        assert status(INT, 2, 16) == INVALID_ARG
        assert status(INT, 12, 16) == INVALID_ARG
        assert status(INT, 4, 8) == INVALID_ARG
        assert status(T96, 12, 16, unit=abi.UNIT_NANOS) == INVALID_ARG
        assert status(T96, 8, 8, unit=abi.UNIT_NANOS) == INVALID_ARG
        assert status(T96, 12, 8, unit=abi.UNIT_NONE) == INVALID_ARG
        assert status(T96, 12, 8, unit=5) == INVALID_ARG
        assert status(3, 4, 16) == INVALID_ARG
        rc, _ = convert(dec, dev, -1, 0, BE, 4, 16, out.ptr)
        assert rc == INVALID_ARG
        # the same call with right arguments works, and the wrapper allocates and times it
        assert convert(dec, dev, n, 4 * n, BE, 4, 16, out.ptr)[0] == 0
        p = dec.convert(dev, n, 4 * n, BE, 4, 16)
        assert not dec.d2h(p, n * 16).any() and dec.last_convert_ms() > 0
        dec.free(p)
        with pytest.raises(pqgpu.PqgError) as e:
            dec.convert(dev, n, 4 * n, BE, 17, 16)
        assert e.value.code == INVALID_ARG
    finally:
        out.free()
        dec.free(dev)
        dec.free(offs)


# ---- 6. end to end against pyarrow ------------------------------------------------------------------

ROWS = 20000
WIDTH = {"d7": 16, "d15": 16, "d30": 16, "d50": 32, "ts": 8}


@pytest.fixture(scope="module")
def tables():
    """name -> (table, write options): FLBA decimals, integer-backed decimals, INT96; values repeat
    (2000 distinct) so that a dictionary page holds them."""
    rng = np.random.default_rng(11)

    import pyarrow.compute as pc

    def repeated(t):
        idx = pa.array(rng.integers(0, 2000, ROWS))
        keep = pa.array(np.arange(ROWS) % 5 != 4)
        return pa.table({n: pc.if_else(keep, t[n].combine_chunks().take(idx), pa.scalar(None, t[n].type))
                         for n in t.column_names})

    return {"flba": (repeated(CU.decimal_table(2000, names=("d7", "d30", "d50"), null_every=0)), {}),
            "ints": (repeated(CU.decimal_table(2000, names=("d7", "d15"), null_every=0)), {"store_decimal_as_integer": True}),
            "int96": (repeated(CU.int96_table(2000, null_every=0)), {"use_deprecated_int96_timestamps": True})}


_files = {}


def file_of(tables, name, dictionary, compression):
    key = (name, dictionary, compression)
    if key not in _files:
        table, kw = tables[name]
        data = CU.write(table, dictionary, compression, **kw)
        _files[key] = (data, CU.read(data))
    return _files[key]


CASES = [(n, d, c) for n in ("flba", "ints", "int96") for d in (False, True) for c in ("NONE", "SNAPPY")]


@pytest.mark.parametrize("name,dictionary,compression", CASES)
def test_read_row_group_converts(dec, tables, name, dictionary, compression):
    data, want = file_of(tables, name, dictionary, compression)
    fr = pqgpu.FileReader(data, decoder=dec, convert_logical=True)
    got = fr.read_row_group(0)
    raw = pqgpu.FileReader(data, decoder=dec).read_row_group(0)
    for c, col in enumerate(want.column_names):
        g, ow = got[col], WIDTH[col]
        assert g.status == 0 and g.value_width == ow and g.offsets is None and g.dictionary is None
        assert g.num_slots == ROWS and g.num_values == ROWS - ROWS // 5
        assert np.array_equal(g.values, CU.value_bytes(want[col], ow)), col
        assert np.array_equal(g.def_levels, raw[col].def_levels)
        lt = fr.file.logical_types[c]
        assert bytes(g.logical) == bytes(lt) and (lt.kind == abi.LT_DECIMAL) == (name != "int96")
        # the default reader returns what it always did: the raw bytes, the oracle's
        assert raw[col].logical is None
        P.compare_chunk(P.oracle_chunk(fr.file, 0, c), raw[col], col)
    if name == "int96":
        for unit in ("s", "ms", "us"):
            g = pqgpu.FileReader(data, decoder=dec, convert_logical=True, int96_unit=unit).read_row_group(0)["ts"]
            w = CU.read(data, coerce_int96_timestamp_unit=unit)["ts"]
            assert np.array_equal(g.values, CU.value_bytes(w, 8)), unit
    with pytest.raises(ValueError):
        pqgpu.FileReader(data, decoder=dec, int96_unit="h")


def test_unconvertible_leaves_come_back_raw(dec):
    """A DECIMAL of precision 0 (a converted-type footer without field 8) stays as it is, with `logical` set."""
    t = pa.table({"d": pa.array([D("1.23"), None, D("-1.23")], pa.decimal128(7, 2))})
    data = CU.write(t)
    good = pqgpu.FileReader(data, decoder=dec, convert_logical=True)
    assert good.read_row_group(0)["d"].value_width == 16
    good.file.logical_types[0].precision = 0
    col = good.read_row_group(0)["d"]
    assert col.value_width == 4 and col.logical.kind == abi.LT_DECIMAL
    assert bytes(col.values) == (123).to_bytes(4, "big") + (-123).to_bytes(4, "big", signed=True)
    good.file.logical_types[0].precision = 77
    assert good.read_row_group(0)["d"].value_width == 4


# ---- 7. kept dictionaries ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["flba", "ints", "int96"])
@pytest.mark.parametrize("compression", ["NONE", "SNAPPY"])  # NONE: the dictionary is read in place, unaligned
def test_kept_dictionaries_convert_only_the_dictionary(dec, tables, name, compression):
    data, want = file_of(tables, name, True, compression)
    cols = tuple(want.column_names)
    fr = pqgpu.FileReader(data, decoder=dec, convert_logical=True, read_dictionary=cols)
    got = fr.read_row_group(0)
    raw = pqgpu.FileReader(data, decoder=dec, read_dictionary=cols).read_row_group(0)
    for col in cols:
        g, r, ow = got[col], raw[col], WIDTH[col]
        assert g.dictionary is not None and r.dictionary is not None, "the writer fell back to PLAIN"
        assert g.value_width == 4 and np.array_equal(g.values, r.values)  # the keys are untouched
        d = g.dictionary
        assert d.value_width == ow and d.count == r.dictionary.count and len(d.values) == d.count * ow
        rw = r.dictionary.value_width
        model = CU.int96_to_time(r.dictionary.table().reshape(-1), "ns").view(np.uint8) if name == "int96" else \
            CU.int_to_le(r.dictionary.values, rw, ow) if name == "ints" else CU.decimal_be_to_le(r.dictionary.values, rw, ow)
        assert np.array_equal(d.values, model)
        m = g.materialize()
        assert m.value_width == ow and bytes(m.logical) == bytes(g.logical)
        assert np.array_equal(m.values, CU.value_bytes(want[col], ow)), col


# ---- 8. filters -------------------------------------------------------------------------------------

FROWS = 6000
OPS = ["<", "<=", "==", "!=", ">", ">=", "in"]


@pytest.fixture(scope="module")
def filter_files(tables):
    """The first FROWS rows of the dictionary-encoded files, with literals taken from their values."""
    out = {}
    for name, col in (("flba", "d7"), ("ints", "d15"), ("int96", "ts")):
        table, kw = tables[name]
        table = table.slice(0, FROWS)
        out[name] = (CU.write(table, True, "SNAPPY", **kw), table, col)
    return out


def dense(table, col):
    return CU.value_bytes(table[col], WIDTH[col])


@pytest.mark.parametrize("keep", [False, True], ids=["materialised", "read_dictionary"])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", ["flba", "ints"])
def test_filtered_reads_of_decimals(dec, filter_files, name, op, keep):
    data, table, col = filter_files[name]
    vals = sorted(v for v in table[col].to_pylist() if v is not None)
    lits = [vals[len(vals) // 3], vals[len(vals) // 2], vals[-1]]
    assert vals[0] < 0 < vals[-1]  # the values straddle zero
    flt = [(col, op, lits if op == "in" else lits[0])]
    want = pq.read_table(io.BytesIO(data), filters=flt)
    assert 0 < want.num_rows < FROWS
    fr = pqgpu.FileReader(data, decoder=dec, convert_logical=True, read_dictionary=(col,) if keep else ())
    got = fr.read_row_group(0, filters=flt)
    for c in table.column_names:
        g = got[c].materialize()
        assert (got[c].dictionary is not None) == (keep and c == col)
        assert g.num_slots == want.num_rows and g.value_width == WIDTH[c] and g.logical.kind == abi.LT_DECIMAL
        assert np.array_equal(g.values, dense(want, c)), (c, op)


@pytest.mark.parametrize("op", OPS)
def test_filtered_reads_of_int96(dec, filter_files, op):
    data, table, col = filter_files["int96"]
    arr = CU.read(data)[col].combine_chunks()  # pyarrow's unfiltered read
    valid = np.asarray(arr.is_valid())          # a null row fails every comparison
    ns = arr.cast(pa.int64()).fill_null(0).to_numpy()
    all_ns = np.sort(ns[valid])
    picks = [int(all_ns[len(all_ns) // 3]), int(all_ns[len(all_ns) // 2]), int(all_ns[-1])]
    lit = [np.datetime64(p, "ns") for p in picks]
    import operator
    fn = {"<": operator.lt, "<=": operator.le, "==": operator.eq, "!=": operator.ne, ">": operator.gt, ">=": operator.ge}
    rows = valid & (np.isin(ns, picks) if op == "in" else fn[op](ns, picks[0]))
    assert 0 < rows.sum() < FROWS
    for keep in ((), (col,)):  # a predicate column that names read_dictionary comes back materialised
        fr = pqgpu.FileReader(data, decoder=dec, convert_logical=True, read_dictionary=keep)
        got = fr.read_row_group(0, filters=[(col, op, lit if op == "in" else lit[0])])[col]
        assert got.dictionary is None and got.value_width == 8 and got.num_slots == rows.sum()
        assert np.array_equal(got.values.view("<i8"), ns[rows])
    # a plain integer literal is nanoseconds since the epoch
    got = fr.read_row_group(0, filters=[(col, "<", picks[0])])[col]
    assert got.num_slots == (valid & (ns < picks[0])).sum()


def test_filter_on_byte_array_decimal_is_refused(dec):
    """A predicate on a BYTE_ARRAY decimal raises before any GPU work; reading one converts it."""
    data = CU.converted_only_file([dict(name="d", typ=6, rep=1, converted=5, scale=2, precision=9)])
    fr = pqgpu.FileReader(data, decoder=dec, convert_logical=True)
    with pytest.raises(pqgpu.PqgError) as e:
        fr.read_row_group(0, filters=[("d", "<", D(1))])
    assert e.value.code == UNSUPPORTED


def test_pqg_filter_signed_be_flag(dec):
    """PQG_COL_SIGNED_BE: two's-complement order on FLBA, INVALID_ARG elsewhere, nothing new without it."""
    rng = np.random.default_rng(8)
    n, w = 4097, 5
    ints = rng.integers(-2 ** 39, 2 ** 39, n)
    ints[:4] = [0, -1, 2 ** 39 - 1, -2 ** 39]
    host = np.frombuffer(b"".join(int(v).to_bytes(w, "big", signed=True) for v in ints), np.uint8)
    dev = dec.upload(host)
    nbm = (n + 31) // 32 * 4
    bm = dec.upload(np.full(nbm, FILL, np.uint8))
    try:
        import operator
        fn = {abi.OP_EQ: operator.eq, abi.OP_NE: operator.ne, abi.OP_LT: operator.lt, abi.OP_LE: operator.le,
              abi.OP_GT: operator.gt, abi.OP_GE: operator.ge}
        unsigned = np.array([int.from_bytes(int(v).to_bytes(w, "big", signed=True), "big") for v in ints], dtype=object)
        for lit in (0, -1, int(ints[100])):
            lb = int(lit).to_bytes(w, "big", signed=True)
            for op, f in fn.items():
                for flags, vals, l in ((abi.COL_SIGNED_BE, ints, lit), (0, unsigned, int.from_bytes(lb, "big"))):
                    desc = abi.ColumnDesc(abi.FIXED_LEN_BYTE_ARRAY, w, 0, 0, 0, flags)
                    a = dec.filter(bm, desc, op, lb, values_ptr=dev, num_rows=n, num_values=n, values_bytes=n * w)
                    want = np.array([bool(f(int(v), l)) for v in vals])
                    bits = np.unpackbits(dec.d2h(bm, nbm), bitorder="little")[:n].astype(bool)
                    assert np.array_equal(bits, want) and a.num_selected == want.sum(), (lit, op, flags)
        for t in (abi.INT32, abi.INT64, abi.BYTE_ARRAY, abi.INT96, abi.BOOLEAN, abi.DOUBLE):
            before = dec.d2h(bm, nbm).copy()
            with pytest.raises(pqgpu.PqgError) as e:
                dec.filter(bm, abi.ColumnDesc(t, -1, 0, 0, 0, abi.COL_SIGNED_BE), abi.OP_EQ, bytes(4), values_ptr=dev,
                           num_rows=16, num_values=16, values_bytes=n * w)
            assert e.value.code == INVALID_ARG and np.array_equal(dec.d2h(bm, nbm), before)
    finally:
        dec.free(dev)
        dec.free(bm)


# ---- nested ----------------------------------------------------------------------------------------

def test_nested_decimals_convert_before_assembly(dec):
    rng = np.random.default_rng(21)
    pool = [v for v in CU.random_decimals(300, 9, 1, 4, null_every=0)]
    rows = []
    for i in range(3000):
        k = int(rng.integers(0, 5))
        rows.append(None if i % 11 == 10 else [None if rng.integers(0, 7) == 0 else pool[int(rng.integers(0, 300))]
                                               for _ in range(k)])
    t = pa.table({"lst": pa.array(rows, pa.list_(pa.decimal128(9, 1)))})
    for dictionary in (False, True):
        data = CU.write(t, dictionary)
        fr = pqgpu.FileReader(data, decoder=dec, convert_logical=True,
                              read_dictionary=("lst",) if dictionary else ())
        col = fr.read_row_group_nested(0)["lst.list.element"]
        assert (col.dictionary is not None) == dictionary
        got = col.to_pylist()

        def dec_of(b):
            return None if b is None else D(int.from_bytes(b, "little", signed=True)).scaleb(-1)

        assert [None if r is None else [dec_of(b) for b in r] for r in got] == rows
        if not dictionary:
            assert col.value_width == 16 and col.leaf_offsets is None
