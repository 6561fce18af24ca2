"""K9s on the GPU: pqg_filter (row predicates into a bitmap), pqg_select (compaction by a bitmap) and
FileReader.read_row_group(filters=...).

The yardstick is a numpy evaluation of the predicate over the ORACLE's decode of the same bytes
(oracle.pyoracle), applied with boolean indexing: a null row passes only IS_NULL, NaN passes only NE,
integers compare signed or unsigned by the column's flag, byte strings as Python bytes do (unsigned
lexicographic, a proper prefix first).  The whole bitmap buffer is compared, the bits past num_rows
included, and every pqg_select output sits between 64 guard bytes."""
import contextlib
import ctypes as C
import io
import struct

import numpy as np
import pytest

import dictout_util as D
import parity as P
import pqgpu
import pqtest_util as U
from oracle import pyoracle as O
from pqgpu import abi
from pqgpu import filters as F

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 4095, 4096, 4097, 8193, 3 * 4096 + 1)  # wave, word and segment edges (0: its own test)
NULLS = ("required", "none", "all", "tenth", "last")
OPS = list(range(8))
UNSUPPORTED, INVALID_ARG = abi.STATUS_CODES["UNSUPPORTED"], abi.STATUS_CODES["INVALID_ARG"]
NAN, INF = float("nan"), float("inf")
LONG = b"q" * 5000


@pytest.fixture(scope="module")
def dec():
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


# ---- columns, literals, and the numpy evaluation ---------------------------------------------------
def _flba(w):
    return [bytes([0] * w), bytes([0x7f] + [0] * (w - 1)), bytes([0x80] + [0] * (w - 1)), bytes([0xff] * w),
            bytes([0x41] * w), bytes([0x41] * (w - 1) + [0x42])]


BIN = [b"", b"a", b"ab", b"abc", b"\x7f", b"\x80", b"ab\x00", b"x" * 65, b"x" * 65 + b"y", b"x" * 200]
KINDS = {  # name: (arrow type, values the column draws from, literals)
    "i32": (pa.int32(), [0, 1, -1, 2 ** 31 - 1, -2 ** 31, 1000, -1000], [0, 2 ** 31 - 1, -2 ** 31, 1000]),
    "u32": (pa.uint32(), [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1, 1000], [0, 2 ** 31, 2 ** 32 - 1, 2 ** 31 - 1]),
    "i64": (pa.int64(), [0, 1, -1, 2 ** 63 - 1, -2 ** 63, 1 << 40, -(1 << 40)], [0, 2 ** 63 - 1, -2 ** 63, -1]),
    "u64": (pa.uint64(), [0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 1, 1 << 40], [0, 2 ** 63, 2 ** 64 - 1, 1]),
    "f32": (pa.float32(), [0.0, -0.0, 1.5, -1.5, INF, -INF, NAN, 3.0e38, 1e-45], [0.0, -0.0, NAN, INF, -INF, 1.5]),
    "f64": (pa.float64(), [0.0, -0.0, 1.5, -1.5, INF, -INF, NAN, 1.7e308, 5e-324], [0.0, -0.0, NAN, INF, -INF, 1.5]),
    "b": (pa.bool_(), [False, True], [False, True]),
    "bin": (pa.binary(), BIN, [b"", b"ab", b"abc", b"abcd", b"\x7f", b"\x80", b"x" * 65, b"x" * 66]),
    "f3": (pa.binary(3), _flba(3), _flba(3)[:4] + [b"\x41\x41\x42"]),
    "f16": (pa.binary(16), _flba(16), _flba(16)[1:5]),
    "f17": (pa.binary(17), _flba(17), _flba(17)[2:6]),
}
NP_TYPE = {abi.INT32: ("<i4", "<u4"), abi.INT64: ("<i8", "<u8"), abi.FLOAT: ("<f4", "<f4"), abi.DOUBLE: ("<f8", "<f8"),
           abi.BOOLEAN: ("u1", "u1")}


def make_table(n, nulls, seed, extra=False):
    """One column per kind, n rows.  extra: an INT96 column and 5000-byte strings (pqg_select)."""
    rng = np.random.default_rng(seed)
    if nulls in ("required", "none"):
        valid = np.ones(n, bool)
    elif nulls == "all":
        valid = np.zeros(n, bool)
    elif nulls == "tenth":
        valid = rng.random(n) >= 0.1
    else:
        valid = np.arange(n) != n - 1
    arrays, fields = [], []
    kinds = dict(KINDS)
    if extra:
        kinds["ts"] = (pa.timestamp("ns"), [0, 1, 86_400_000_000_000 * 20000 + 12345, -1], [])
    for name, (typ, dom, _) in kinds.items():
        pick = rng.integers(0, len(dom), n)
        vals = [dom[k] if ok else None for k, ok in zip(pick, valid)]
        if extra and name == "bin":
            vals = [LONG if v is not None and i % 97 == 5 else v for i, v in enumerate(vals)]
        arrays.append(pa.array(vals, typ))
        fields.append(pa.field(name, typ, nullable=nulls != "required"))
    return pa.Table.from_arrays(arrays, schema=pa.schema(fields))


def write(table, **kw):
    buf = io.BytesIO()
    kw.setdefault("compression", "none")
    pq.write_table(table, buf, row_group_size=1 << 24, use_deprecated_int96_timestamps=True, **kw)
    return buf.getvalue()


@contextlib.contextmanager
def decoded(dec, data, keep=(), rg=0):
    """The columns of one row group on the GPU (ChunkResults, valid inside the block) and from the oracle."""
    pf = pqgpu.ParquetFile(data)
    specs = [(rg, c) for c in range(pf.num_columns)]
    keep = {pf.column_index(k) for k in keep}
    res, dev, _ = pqgpu.decode_spans(pf, specs, dec, keep_dict=keep)
    try:
        exps = [P.oracle_chunk(pf, rg, c) for c in range(pf.num_columns)]
        for r, e in zip(res, exps):
            assert r.status == 0 and e.status == 0 and r.num_slots == e.num_slots and r.num_values == e.num_values
        yield pf, res, exps
    finally:
        dec.free(dev)


def dense(exp, desc):
    """The oracle's dense values as a numpy array (numbers) or an object array of bytes."""
    if getattr(exp, "_dense", None) is None:
        exp._dense = _dense(exp, desc)
        exp._cmp = {}
    return exp._dense


def _dense(exp, desc):
    raw = np.asarray(exp.values, np.uint8) if exp.values is not None else np.zeros(0, np.uint8)
    t = desc.physical_type
    if t in NP_TYPE:
        return raw.view(NP_TYPE[t][desc.flags & 1])[:exp.num_values]
    b = raw.tobytes()
    if t == abi.BYTE_ARRAY:
        o = np.asarray(exp.offsets, np.int64)
        vals = [b[o[i]:o[i + 1]] for i in range(exp.num_values)]
    else:
        w = {abi.INT96: 12}.get(t, desc.type_length)
        vals = [b[i * w:(i + 1) * w] for i in range(exp.num_values)]
    out = np.empty(len(vals), object)
    out[:] = vals
    return out


def valid_rows(exp, desc):
    if desc.max_def == 0 or exp.def_levels is None:
        return np.ones(exp.num_slots, bool)
    return np.asarray(exp.def_levels) == desc.max_def


def expect_rows(exp, desc, op, lit):
    """The rows that pass `op lit` (lit: physical bytes), by numpy over the oracle's decode."""
    valid = valid_rows(exp, desc)
    if op == abi.OP_IS_NULL:
        return ~valid
    if op == abi.OP_NOT_NULL:
        return valid
    v = dense(exp, desc)
    if desc.physical_type in NP_TYPE:
        x = np.frombuffer(lit, NP_TYPE[desc.physical_type][desc.flags & 1])[0]
        with np.errstate(invalid="ignore"):
            ok = [v == x, v != x, v < x, v <= x, v > x, v >= x][op]
    else:
        if lit not in exp._cmp:  # Python's bytes order, three-way, once per literal
            exp._cmp[lit] = np.array([(a > lit) - (a < lit) for a in v], np.int8)
        c = exp._cmp[lit]
        ok = [c == 0, c != 0, c < 0, c <= 0, c > 0, c >= 0][op]
    rows = np.zeros(exp.num_slots, bool)
    rows[valid] = ok
    return rows


def pack(rows):
    """A row bitmap as pqg_filter lays it out: LSB first, whole dwords, zero past the last row."""
    out = np.zeros((len(rows) + 31) // 32 * 4, np.uint8)
    b = np.packbits(np.asarray(rows, bool), bitorder="little")
    out[:len(b)] = b
    return out


class Guarded:
    """A device buffer of n bytes between two 64-byte guards."""

    def __init__(self, dec, n, fill=0xCD, content=None):
        self.dec, self.n = dec, n
        host = np.full(n + 128, 0xA5, np.uint8)
        host[64:64 + n] = fill if content is None else np.frombuffer(bytes(content), np.uint8)
        self.base = dec.upload(host)
        self.ptr = self.base + 64

    def set(self, content):
        c = np.frombuffer(bytes(content), np.uint8)
        assert len(c) == self.n
        if self.n:
            pqgpu.reader._check(self.dec.L.pqg_memcpy_h2d(self.dec.ctx, C.c_void_p(self.ptr), c.ctypes.data, self.n), "h2d")

    def get(self):
        d = self.dec.d2h(self.base, self.n + 128)
        assert (d[:64] == 0xA5).all() and (d[64 + self.n:] == 0xA5).all(), "guard bytes changed"
        return d[64:64 + self.n]

    def free(self):
        self.dec.free(self.base)


def run_filter(dec, bm, r, desc, op, lit, combine=abi.COMBINE_SET, dictionary=None):
    a = dec.filter_result(bm.ptr, r, desc, op, lit, combine, dictionary)
    return a.num_selected, a.num_valid


def device_dictionary(dec, job):
    d = abi.Dictionary()
    pqgpu.reader._check(dec.L.pqg_get_dictionary(dec.ctx, job, C.byref(d)), "pqg_get_dictionary")
    return d


def literals(name, desc, which):
    lits = KINDS[name][2]
    return [F.literal(desc, lits[k % len(lits)]) for k in which]


# ---- pqg_filter on decoded chunks -------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_filter_decoded_chunks(dec, n):
    for pat, nulls in enumerate(NULLS):
        data = write(make_table(n, nulls, seed=n * 7 + pat))
        with decoded(dec, data) as (pf, res, exps):
            bm = Guarded(dec, (n + 31) // 32 * 4)
            try:
                for c, (r, exp) in enumerate(zip(res, exps)):
                    name, desc = pf.columns[c].path.decode(), pf.columns[c].desc
                    assert desc.max_def == (0 if nulls == "required" else 1)
                    nlit = len(KINDS[name][2])
                    for op in OPS:
                        which = range(nlit) if n <= 65 else (op + pat, op + pat + 3)
                        for lit in literals(name, desc, which):
                            want = expect_rows(exp, desc, op, lit)
                            bm.set(b"\xff" * bm.n)  # a SET overwrites every bit, the tail's too
                            nsel, nvalid = run_filter(dec, bm, r, desc, op, lit)
                            where = "%s %s n=%d op=%d lit=%r" % (name, nulls, n, op, lit[:8])
                            assert np.array_equal(bm.get(), pack(want)), where
                            assert (nsel, nvalid) == (int(want.sum()), int(valid_rows(exp, desc).sum())), where
            finally:
                bm.free()


def test_filter_selects_something_of_everything(dec):
    """The cases above are not vacuous: over the 10 %-null column of every kind each operator passes
    some rows and fails some (IS_NULL / NOT_NULL included)."""
    n = 4097
    data = write(make_table(n, "tenth", seed=5))
    with decoded(dec, data) as (pf, res, exps):
        for c, exp in enumerate(exps):
            name, desc = pf.columns[c].path.decode(), pf.columns[c].desc
            for op in OPS:
                counts = [int(expect_rows(exp, desc, op, lit).sum()) for lit in literals(name, desc, range(8))]
                assert any(0 < k < n for k in counts), (name, op)


def test_filter_zero_rows(dec):
    """num_rows == 0: OK, counts 0, nothing written."""
    bm = Guarded(dec, 8, fill=0x5A)
    try:
        desc = abi.ColumnDesc(abi.INT32, -1, 1, 0, 0, 0)
        a = dec.filter(bm.ptr, desc, abi.OP_NE, struct.pack("<i", 1), num_rows=0)
        assert (a.num_selected, a.num_valid) == (0, 0) and (bm.get() == 0x5A).all()
        s = dec.select(bm.ptr, None, None, None, 0, 0, 0, 1, 4)
        assert (s.rows_out, s.values_out, s.bytes_out) == (0, 0, 0) and dec.last_filter_ms() == 0.0
    finally:
        bm.free()


# ---- combine modes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 4097])
def test_combine_chains_and_tail_bits(dec, n):
    data = write(make_table(n, "tenth", seed=n))
    with decoded(dec, data) as (pf, res, exps):
        col = {pf.columns[c].path.decode(): c for c in range(pf.num_columns)}
        bm = Guarded(dec, (n + 31) // 32 * 4)
        try:
            def term(name, op, value):
                c = col[name]
                desc = pf.columns[c].desc
                lit = F.literal(desc, value) if value is not None else None
                return (res[c], desc, op, lit), expect_rows(exps[c], desc, op, lit)

            # SET, then AND, then OR: ((i32 >= 0) & (bin != "ab")) | (f64 is null) | (u32 > 2^31)
            chain = [(term("i32", abi.OP_GE, 0), abi.COMBINE_SET), (term("bin", abi.OP_NE, b"ab"), abi.COMBINE_AND),
                     (term("f64", abi.OP_IS_NULL, None), abi.COMBINE_OR), (term("u32", abi.OP_GT, 2 ** 31), abi.COMBINE_OR)]
            want = None
            bm.set(b"\xff" * bm.n)
            for (args, rows), mode in chain:
                want = rows if mode == abi.COMBINE_SET else (want & rows if mode == abi.COMBINE_AND else want | rows)
                nsel, _ = run_filter(dec, bm, *args, combine=mode)
                assert np.array_equal(bm.get(), pack(want)) and nsel == int(want.sum())
            assert 0 < want.sum() < n
            # NE, IS_NULL and OR onto a full bitmap (tail bits set): the tail comes back zero
            for (args, rows), mode in [(term("i64", abi.OP_NE, 0), abi.COMBINE_SET), (term("i64", abi.OP_NE, 0), abi.COMBINE_AND),
                                       (term("f32", abi.OP_IS_NULL, None), abi.COMBINE_OR), (term("f32", abi.OP_NE, NAN), abi.COMBINE_OR),
                                       (term("b", abi.OP_IS_NULL, None), abi.COMBINE_AND)]:
                bm.set(b"\xff" * bm.n)
                full = np.ones(n, bool)
                exp_rows = rows if mode != abi.COMBINE_OR else full
                nsel, _ = run_filter(dec, bm, *args, combine=mode)
                got = bm.get()
                assert np.array_equal(got, pack(exp_rows)) and nsel == int(exp_rows.sum())
                assert not np.unpackbits(got, bitorder="little")[n:].any()
        finally:
            bm.free()


# ---- kept dictionaries -----------------------------------------------------------------------------
def _dict_table(count, n, seed):
    """Dictionary-encoded columns of `count` distinct values each over n rows, a tenth of them null."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, count, n)
    keys[:min(count, n)] = np.arange(min(count, n))  # every entry used, in first-use order
    valid = rng.random(n) >= 0.1
    valid[:count] = True
    step = 2 ** 32 // max(count, 1)
    cols = {
        "i32": pa.array((keys * step - 2 ** 31).astype(np.int32), mask=~valid),
        "u64": pa.array((keys.astype(np.uint64) << np.uint64(44)) + np.uint64(3), mask=~valid),
        "f64": pa.array(keys * 0.5 - count / 4.0, mask=~valid),
        "bin": pa.array([None if not ok else b"k%05d" % k for k, ok in zip(keys, valid)], pa.binary()),
        "f3": pa.array([None if not ok else bytes([k & 0xff, (k >> 8) & 0xff, k >> 16]) for k, ok in zip(keys, valid)],
                       pa.binary(3)),
    }
    return pa.table(cols)


DICT_LITS = {
    "i32": lambda count: [-2 ** 31, (count // 2) * (2 ** 32 // count) - 2 ** 31, 7],
    "u64": lambda count: [3, ((count // 2) << 44) + 3, 2 ** 63],
    "f64": lambda count: [-count / 4.0, 0.0, NAN],
    "bin": lambda count: [b"k00000", b"k%05d" % (count // 2), b"k", b"zzz"],
    "f3": lambda count: [bytes(3), bytes([(count // 2) & 0xff, ((count // 2) >> 8) & 0xff, (count // 2) >> 16]), b"\xff\xff\xff"],
}


@pytest.mark.parametrize("count", [1, 4096, 4097, 70000])  # 70000: more entries than kLdsEntries stages in LDS
def test_kept_dictionary_equals_materialised(dec, count):
    n = max(count + 1500, 5000)
    data = write(_dict_table(count, n, seed=count), use_dictionary=True, dictionary_pagesize_limit=4 << 20,
                 data_page_size=1 << 20)
    names = list(DICT_LITS)
    plain = {}
    with decoded(dec, data) as (pf, res, exps):
        bm = Guarded(dec, (n + 31) // 32 * 4)
        try:
            for c, (r, exp) in enumerate(zip(res, exps)):
                name, desc = pf.columns[c].path.decode(), pf.columns[c].desc
                for op in OPS:
                    for k, v in enumerate(DICT_LITS[name](count)):
                        lit = F.literal(desc, v)
                        nsel, nvalid = run_filter(dec, bm, r, desc, op, lit)
                        got = bm.get().copy()
                        assert np.array_equal(got, pack(expect_rows(exp, desc, op, lit))), (name, op, k)
                        plain[name, op, k] = (got, nsel, nvalid)
        finally:
            bm.free()
    with decoded(dec, data, keep=names) as (pf, res, exps):
        bm = Guarded(dec, (n + 31) // 32 * 4)
        try:
            for c, r in enumerate(res):
                name, desc = pf.columns[c].path.decode(), pf.columns[c].desc
                assert r.col_flags & abi.COL_KEEP_DICT and r.value_width == 4, name  # the dictionary path is the one under test
                d = device_dictionary(dec, c)
                assert d.count == count
                for op in OPS:
                    for k, v in enumerate(DICT_LITS[name](count)):
                        bm.set(b"\xff" * bm.n)
                        nsel, nvalid = run_filter(dec, bm, r, desc, op, F.literal(desc, v), dictionary=d)
                        want, wsel, wvalid = plain[name, op, k]
                        assert np.array_equal(bm.get(), want) and (nsel, nvalid) == (wsel, wvalid), (name, op, k)
        finally:
            bm.free()


def test_dictionary_with_unused_entries(dec):
    """A hand-built chunk: 300 INT32 entries of which the keys use every third; 10 % nulls."""
    count, n = 300, 4097 + 64
    rng = np.random.default_rng(11)
    valid = rng.random(n) >= 0.1
    keys = (rng.integers(0, count // 3, int(valid.sum())) * 3).astype(np.uint32)
    dpage = D.int32_dict(count, seed=4)
    entries = (np.arange(count, dtype=np.int64) * 2654435761 + 4).astype(np.uint32).view(np.int32)
    chunk = dpage + D.data_page(keys, 9, "mixed", mask=valid)
    keep = []
    job, buf = U.chunk_job(chunk, abi.INT32, max_def=1, data_page_offset=len(dpage), keep=keep)
    exp = O.decode_chunk(job)
    assert exp.status == 0 and exp.num_values == len(keys)
    dev = dec.upload(bytes(buf) + bytes(64))
    bm = Guarded(dec, (n + 31) // 32 * 4)
    try:
        job.data = dev
        job.col.flags |= abi.COL_KEEP_DICT
        r = dec.decode_jobs([job])[0]
        assert r.status == 0 and r.col_flags & abi.COL_KEEP_DICT
        d = device_dictionary(dec, 0)
        assert d.count == count
        desc = job.col
        unused = int(entries[1])  # an entry no key uses: == selects nothing, != every non-null row
        for op in OPS:
            for v in (int(entries[0]), unused, int(entries[297]), 0):
                lit = struct.pack("<i", v)
                bm.set(b"\xff" * bm.n)
                nsel, nvalid = run_filter(dec, bm, r, desc, op, lit, dictionary=d)
                want = expect_rows(exp, desc, op, lit)
                assert np.array_equal(bm.get(), pack(want)) and nsel == int(want.sum()) and nvalid == len(keys), (op, v)
        assert not expect_rows(exp, desc, abi.OP_EQ, struct.pack("<i", unused)).any()
        # the keys are a 4-byte column to pqg_select; the dictionary is untouched
        sel = rng.random(n) < 0.5
        bm.set(pack(sel))
        a = dec.select(bm.ptr, r.def_levels, r.values, None, n, r.num_values, r.values_bytes, 1, 4)
        try:
            got_keys = dec.d2h(a.out_values, a.bytes_out).view("<i4")
            assert np.array_equal(got_keys, keys.astype(np.int32)[sel[valid]]) and a.rows_out == int(sel.sum())
            assert np.array_equal(dec.d2h(a.out_def_levels, a.rows_out), valid[sel].astype(np.uint8))
        finally:
            dec.free_select(a)
        assert np.array_equal(dec.dictionary(0).table().reshape(-1).view("<i4"), entries)
    finally:
        bm.free()
        dec.free(dev)


# ---- pqg_select --------------------------------------------------------------------------------------
def bitmaps(n, rng):
    i = np.arange(n)
    return {"zero": np.zeros(n, bool), "one": np.ones(n, bool), "alternating": i % 2 == 1,
            "segment_first": i % 4096 == 0, "segment_last": (i % 4096 == 4095) | (i == n - 1),
            "one_percent": rng.random(n) < 0.01, "half": rng.random(n) < 0.5}


def select_exact(dec, bm_ptr, r, desc, want):
    """pqg_select into exactly sized, guarded outputs; `want`: (def, values, offsets) bytes."""
    wdef, wval, woff = want
    outs = [Guarded(dec, len(wdef)), Guarded(dec, len(wval)), Guarded(dec, len(woff))]
    try:
        a = abi.SelectArgs()
        a.bitmap, a.def_levels, a.values, a.offsets = bm_ptr, r.def_levels, r.values, r.offsets
        a.num_rows, a.num_values, a.values_bytes = r.num_slots, r.num_values, r.values_bytes
        a.max_def, a.value_width = desc.max_def, r.value_width
        a.out_def_levels = outs[0].ptr if desc.max_def else None
        a.out_values = outs[1].ptr
        a.out_offsets = outs[2].ptr if r.value_width == 0 else None
        pqgpu.reader._check(dec.L.pqg_select(dec.ctx, C.byref(a)), "pqg_select")
        return a, [o.get().tobytes() for o in outs]
    finally:
        for o in outs:
            o.free()


def expect_select(exp, desc, sel):
    valid = valid_rows(exp, desc)
    wdef = np.asarray(exp.def_levels, np.uint8)[sel].tobytes() if desc.max_def else b""
    take = sel[valid]  # per dense value
    raw = np.asarray(exp.values, np.uint8) if exp.values is not None else np.zeros(0, np.uint8)
    if exp.value_width == 0:
        vals = dense(exp, desc)[take]
        offs = np.zeros(len(vals) + 1, np.int64)
        np.cumsum([len(v) for v in vals], out=offs[1:])
        return (wdef, b"".join(vals), offs.tobytes()), int(sel.sum()), len(vals)
    w = exp.value_width
    vals = raw[:exp.num_values * w].reshape(-1, w)[take]
    return (wdef, vals.tobytes(), b""), int(sel.sum()), len(vals)


@pytest.mark.parametrize("n", NS)
def test_select(dec, n):
    """Widths 1 (BOOLEAN), 4, 8, 12 (INT96), FLBA 3 and 17, byte arrays with empty, > 64-byte and
    5000-byte values; every bitmap pattern; every null pattern."""
    cols = ("b", "i32", "i64", "ts", "f3", "f17", "bin")
    for pat, nulls in enumerate(NULLS):
        rng = np.random.default_rng(n + pat)
        data = write(make_table(n, nulls, seed=n * 3 + pat, extra=True).select(list(cols)))
        with decoded(dec, data) as (pf, res, exps):
            bm = Guarded(dec, (n + 31) // 32 * 4)
            try:
                for kind, sel in bitmaps(n, rng).items():
                    bits = np.unpackbits(pack(sel), bitorder="little")
                    bits[n:] = 1  # bits past num_rows are ignored
                    bm.set(np.packbits(bits, bitorder="little"))
                    for c, (r, exp) in enumerate(zip(res, exps)):
                        desc = pf.columns[c].desc
                        want, rows, vals = expect_select(exp, desc, sel)
                        a, got = select_exact(dec, bm.ptr, r, desc, want)
                        where = "%s %s %s n=%d" % (cols[c], nulls, kind, n)
                        assert (a.rows_out, a.values_out, a.bytes_out) == (rows, vals, len(want[1])), where
                        assert got[0] == want[0], where + " def levels"
                        assert got[1] == want[1], where + " values"
                        assert got[2] == want[2], where + " offsets"
            finally:
                bm.free()
    assert [exps[c].value_width for c in range(len(cols))] == [1, 4, 8, 12, 3, 17, 0]


def test_select_count_only_and_input_sized(dec):
    n = 8193
    data = write(make_table(n, "tenth", seed=2, extra=True).select(["i64", "bin"]))
    sel = np.random.default_rng(3).random(n) < 0.3
    with decoded(dec, data) as (pf, res, exps):
        bm = Guarded(dec, (n + 31) // 32 * 4, content=pack(sel))
        try:
            for c, (r, exp) in enumerate(zip(res, exps)):
                desc = pf.columns[c].desc
                want, rows, vals = expect_select(exp, desc, sel)
                a = dec.select(bm.ptr, r.def_levels, r.values, r.offsets, n, r.num_values, r.values_bytes, 1, r.value_width,
                               count_only=True)
                assert (a.rows_out, a.values_out, a.bytes_out) == (rows, vals, len(want[1]))
                assert not (a.out_def_levels or a.out_values or a.out_offsets)
                a = dec.select(bm.ptr, r.def_levels, r.values, r.offsets, n, r.num_values, r.values_bytes, 1, r.value_width)
                try:
                    assert dec.d2h(a.out_values, a.bytes_out).tobytes() == want[1]
                    assert dec.d2h(a.out_def_levels, a.rows_out).tobytes() == want[0]
                    if r.value_width == 0:
                        assert dec.d2h(a.out_offsets, (a.values_out + 1) * 8).tobytes() == want[2]
                finally:
                    dec.free_select(a)
                assert dec.last_filter_ms() > 0
        finally:
            bm.free()


# ---- errors ------------------------------------------------------------------------------------------
def test_errors_leave_outputs_untouched(dec):
    n = 100
    vals = dec.upload(np.arange(3 * n, dtype=np.int32))
    bm = Guarded(dec, (n + 31) // 32 * 4, fill=0x3C)
    try:
        def status(desc, op, lit, **kw):
            with pytest.raises(pqgpu.PqgError) as e:
                dec.filter(bm.ptr, desc, op, lit, values_ptr=vals, num_rows=n, num_values=n, values_bytes=12 * n, **kw)
            assert (bm.get() == 0x3C).all()
            return e.value.code

        assert status(abi.ColumnDesc(abi.INT96, -1, 0, 0, 0, 0), abi.OP_EQ, bytes(12)) == UNSUPPORTED
        assert status(abi.ColumnDesc(abi.INT96, -1, 0, 0, 0, 0), abi.OP_IS_NULL, None) == UNSUPPORTED
        assert status(abi.ColumnDesc(abi.INT32, -1, 1, 1, 0, 0), abi.OP_EQ, bytes(4)) == UNSUPPORTED  # max_rep 1
        assert status(abi.ColumnDesc(abi.FIXED_LEN_BYTE_ARRAY, 0, 0, 0, 0, 0), abi.OP_EQ, b"") == UNSUPPORTED
        for t, tl, bad in ((abi.INT32, -1, 8), (abi.INT64, -1, 4), (abi.FLOAT, -1, 0), (abi.DOUBLE, -1, 7),
                           (abi.BOOLEAN, -1, 4), (abi.FIXED_LEN_BYTE_ARRAY, 3, 4), (abi.FIXED_LEN_BYTE_ARRAY, 3, 2)):
            assert status(abi.ColumnDesc(t, tl, 0, 0, 0, 0), abi.OP_LT, bytes(bad)) == INVALID_ARG, (t, bad)
        assert status(abi.ColumnDesc(abi.INT32, -1, 0, 0, 0, 0), 8, bytes(4)) == INVALID_ARG       # no such operator
        assert status(abi.ColumnDesc(abi.INT32, -1, 0, 0, 0, 0), abi.OP_EQ, bytes(4), combine=3) == INVALID_ARG
        # the same call with a right literal works
        a = dec.filter(bm.ptr, abi.ColumnDesc(abi.INT32, -1, 0, 0, 0, 0), abi.OP_LT, struct.pack("<i", 10), values_ptr=vals,
                       num_rows=n, num_values=n, values_bytes=4 * n)
        assert a.num_selected == 10 and a.num_valid == n and np.array_equal(bm.get(), pack(np.arange(n) < 10))
    finally:
        bm.free()
        dec.free(vals)


# ---- end to end --------------------------------------------------------------------------------------
ROWS, RGS = 3400, 3


@pytest.fixture(scope="module")
def e2e_file():
    n = ROWS * RGS
    rng = np.random.default_rng(42)
    i = rng.integers(-1000, 1000, n)
    d = np.round(rng.normal(0, 100, n), 3)
    s = ["row-%d-%s" % (k, "x" * (k % 90)) for k in range(n)]
    ds = ["cat%02d" % k for k in rng.integers(0, 50, n)]
    nul = lambda frac: rng.random(n) < frac
    t = pa.table({
        "i": pa.array(i, pa.int64(), mask=nul(0.1)), "d": pa.array(d, pa.float64(), mask=nul(0.05)),
        "s": pa.array([None if m else v for v, m in zip(s, nul(0.1))], pa.string()),
        "ds": pa.array([None if m else v for v, m in zip(ds, nul(0.2))], pa.string())})
    buf = io.BytesIO()
    pq.write_table(t, buf, row_group_size=ROWS, compression="snappy", use_dictionary=["ds", "i"])
    return t, buf.getvalue()


E2E_FILTERS = {
    "single": [("i", ">", 990)],                                              # about 0.5 % of the rows
    "and": [("i", "<=", 0), ("ds", "==", "cat07")],
    "or_of_ands": [[("d", ">", 150.0), ("ds", "!=", "cat01")], [("i", "==", 5), ("s", ">=", "row-5")]],
    "in": [("ds", "in", ["cat03", "cat49", "nope"]), ("i", "in", [1, 2, 3, 4, 5, 6, 7, 8])],
    "is_null": [("s", "is", None)],
    "unprojected": [("d", "<", -200.0)],                                       # d is not read back
}


def _row_passes(v, op, lit):
    if op == "is":
        return v is None
    if v is None:
        return False
    if op == "in":
        return v in lit
    return {"==": v == lit, "!=": v != lit, "<": v < lit, "<=": v <= lit, ">": v > lit, ">=": v >= lit}[op]


def _pylist(col, desc):
    """A DecodedColumn of a flat column as Python values."""
    col = col.materialize()
    valid = np.asarray(col.def_levels) == desc.max_def if col.def_levels is not None else np.ones(col.num_slots, bool)
    if col.value_width == 0:
        b, o = np.asarray(col.values, np.uint8).tobytes(), np.asarray(col.offsets, np.int64)
        vals = [b[o[k]:o[k + 1]].decode() for k in range(col.num_values)]
    else:
        vals = np.asarray(col.values, np.uint8).view(NP_TYPE[desc.physical_type][0])[:col.num_values].tolist()
    it = iter(vals)
    return [next(it) if ok else None for ok in valid]


@pytest.mark.parametrize("keep", [(), ("ds", "i")], ids=["materialised", "read_dictionary"])
@pytest.mark.parametrize("name", list(E2E_FILTERS))
def test_read_row_group_with_filters(dec, e2e_file, name, keep):
    import pyarrow.compute as pc
    table, data = e2e_file
    f = E2E_FILTERS[name]
    project = ("i", "s", "ds") if name == "unprojected" else ()
    r = pqgpu.FileReader(data, *project, decoder=dec, read_dictionary=keep)
    plain = pqgpu.FileReader(data, *project, decoder=dec)
    dnf = [f] if isinstance(f[0], tuple) else f
    cols = {c: table.column(c).to_pylist() for c in table.column_names}
    names = [c for c in table.column_names if not project or c in project]
    got_all = {c: [] for c in names}
    for rg in range(RGS):
        lo = rg * ROWS
        sel = np.array([any(all(_row_passes(cols[c][lo + k], op, lit) for c, op, lit in conj) for conj in dnf)
                        for k in range(ROWS)])
        base = plain.read_row_group(rg)
        got = r.read_row_group(rg, filters=f)
        assert sorted(got) == sorted(names)
        for c in names:
            desc = r.file.columns[r.file.column_index(c)].desc
            g, b = got[c], base[c]
            kept = c in keep
            assert (g.dictionary is not None) == kept, c
            m = g.materialize()
            assert g.status == 0 and g.num_slots == int(sel.sum()), (c, rg)
            # the numpy-filtered unfiltered read, buffer by buffer
            valid = np.asarray(b.def_levels) == desc.max_def
            assert np.array_equal(g.def_levels, np.asarray(b.def_levels)[sel]), c
            take = sel[valid]
            if b.value_width == 0:
                chars, o = np.asarray(b.values, np.uint8), np.asarray(b.offsets, np.int64)
                lens = (o[1:] - o[:-1])[take]
                offs = np.zeros(len(lens) + 1, np.int64)
                np.cumsum(lens, out=offs[1:])
                want = b"".join(chars[o[k]:o[k + 1]].tobytes() for k in np.nonzero(take)[0])
                assert np.array_equal(m.offsets, offs) and np.asarray(m.values, np.uint8).tobytes() == want, c
            else:
                w = b.value_width
                assert np.array_equal(np.asarray(m.values, np.uint8),
                                      np.asarray(b.values, np.uint8).reshape(-1, w)[take].reshape(-1)), c
            assert m.num_values == int(take.sum())
            got_all[c] += _pylist(g, desc)
    # the NaN-free file: pyarrow's own filtered read gives the same rows
    if name == "is_null":
        expr = pc.field("s").is_null()
    else:
        expr = f
    want = pq.read_table(io.BytesIO(data), filters=expr, columns=names)
    for c in names:
        assert got_all[c] == want.column(c).to_pylist(), c
    assert 0 < len(got_all[names[0]]) < ROWS * RGS


def test_filtered_read_downloads_less_and_plain_read_is_unchanged(dec, e2e_file):
    table, data = e2e_file
    r = pqgpu.FileReader(data, decoder=dec)
    d0 = dec.downloaded_bytes
    base = r.read_row_group(1)
    d1 = dec.downloaded_bytes
    got = r.read_row_group(1, filters=[("i", ">", 980)])  # about 1 % of the rows
    d2 = dec.downloaded_bytes
    n = got["i"].num_slots
    assert 0 < n < ROWS // 20
    # the page tables are host copies, not downloads: d2h counts only device bytes
    assert 0 < d2 - d1 < (d1 - d0) // 10
    # without filters: what the oracle decodes, as before
    for c in range(r.file.num_columns):
        P.compare_chunk(P.oracle_chunk(r.file, 1, c), base[r.file.columns[c].path.decode()], "col%d" % c)
    # no row selected: every column comes back empty
    none = r.read_row_group(0, filters=[("i", ">", 10 ** 6)])
    for c, col in none.items():
        assert col.num_slots == 0 and col.num_values == 0 and len(col.values) == 0, c
        assert col.offsets is None or np.array_equal(col.offsets, [0])
    with pytest.raises(ValueError):
        r.read_row_group(0, filters=[("i", "~", 1)])
    with pytest.raises(KeyError):
        r.read_row_group(0, filters=[("nope", "==", 1)])


def test_repeated_columns_are_unsupported_before_any_gpu_work(dec):
    t = pa.table({"a": pa.array([1, 2, 3], pa.int64()), "l": pa.array([[1], [2, 3], []], pa.list_(pa.int32()))})
    buf = io.BytesIO()
    pq.write_table(t, buf)
    for cols, f in (((), [("a", ">", 1)]), (("a",), [("l.list.element", "==", 2)])):
        r = pqgpu.FileReader(buf.getvalue(), *cols, decoder=dec)
        up = r.uploaded_bytes
        with pytest.raises(pqgpu.PqgError) as e:
            r.read_row_group(0, filters=f)
        assert e.value.code == UNSUPPORTED and r.uploaded_bytes == up
    r = pqgpu.FileReader(buf.getvalue(), "a", decoder=dec)
    assert _pylist(r.read_row_group(0, filters=[("a", ">", 1)])["a"], r.file.columns[0].desc) == [2, 3]
