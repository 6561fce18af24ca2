"""Helpers of the logical-type conversion tests (test_convert_model.py, test_convert.py): the numpy
model of pqg_convert, pyarrow-written files of decimals and INT96 timestamps with what pyarrow
reads from them, and hand-built footers of converted types only."""
import decimal
import io

import numpy as np

D = decimal.Decimal

# ---- the model ----------------------------------------------------------------------------------


def _sign_extend(le, ow):
    """(n, w) little-endian two's-complement rows -> n * ow bytes."""
    n, w = le.shape
    out = np.zeros((n, ow), np.uint8)
    out[:, :w] = le
    if w < ow and n:
        out[:, w:] = np.where(le[:, w - 1:w] & 0x80, 0xff, 0x00).astype(np.uint8)
    return out.reshape(-1)


def decimal_be_to_le(raw, w, ow):
    """n big-endian two's-complement values of w bytes -> n * ow little-endian bytes, sign-extended."""
    raw = np.frombuffer(bytes(raw), np.uint8) if not isinstance(raw, np.ndarray) else raw.view(np.uint8).reshape(-1)
    assert 1 <= w <= ow and len(raw) % w == 0
    return _sign_extend(raw.reshape(-1, w)[:, ::-1], ow)


def bytes_be_to_le(chars, offsets, ow):
    """BYTE_ARRAY decimals (each its own length, 1..ow) -> n * ow little-endian bytes."""
    chars = np.asarray(chars, np.uint8)
    o = np.asarray(offsets, np.int64)
    out = np.zeros((len(o) - 1, ow), np.uint8)
    for i in range(len(o) - 1):
        v = chars[o[i]:o[i + 1]][::-1]
        assert 1 <= len(v) <= ow
        out[i, :len(v)] = v
        out[i, len(v):] = 0xff if v[-1] & 0x80 else 0
    return out.reshape(-1)


def int_to_le(raw, w, ow):
    """n little-endian int32 / int64 values -> n * ow bytes, sign-extended."""
    raw = np.frombuffer(bytes(raw), np.uint8) if not isinstance(raw, np.ndarray) else raw.view(np.uint8).reshape(-1)
    assert w in (4, 8) and len(raw) % w == 0
    return _sign_extend(raw.reshape(-1, w), ow)


JULIAN_EPOCH = 2440588
UNIT_PER_DAY = {"s": 86400, "ms": 86400 * 10 ** 3, "us": 86400 * 10 ** 6, "ns": 86400 * 10 ** 9}
NS_PER_UNIT = {"s": 10 ** 9, "ms": 10 ** 6, "us": 10 ** 3, "ns": 1}


def int96_to_time(raw, unit):
    """n INT96 values (nanos of the day u64, julian day i32) -> int64 in `unit`: an unsigned
    truncating divide, a multiply and an add that wrap in 64 bits."""
    raw = np.frombuffer(bytes(raw), np.uint8) if not isinstance(raw, np.ndarray) else raw.view(np.uint8).reshape(-1)
    v = raw.reshape(-1, 12)
    nanos = np.ascontiguousarray(v[:, :8]).view("<u8").reshape(-1)
    day = np.ascontiguousarray(v[:, 8:]).view("<i4").reshape(-1).astype(np.int64)
    with np.errstate(over="ignore"):
        days = (day - JULIAN_EPOCH).astype(np.uint64)
        return (days * np.uint64(UNIT_PER_DAY[unit]) + nanos // np.uint64(NS_PER_UNIT[unit])).astype(np.int64)


def int96_bytes(ns):
    """int64 nanoseconds since the epoch as INT96 values, the way writers store them."""
    ns = np.asarray(ns, np.int64)
    per = 86400 * 10 ** 9
    out = np.zeros((len(ns), 12), np.uint8)
    out[:, :8] = np.mod(ns, per).astype("<u8").view(np.uint8).reshape(-1, 8)
    out[:, 8:] = (np.floor_divide(ns, per) + JULIAN_EPOCH).astype("<i4").view(np.uint8).reshape(-1, 4)
    return out.reshape(-1)


# ns timestamps whose conversion the project checked against pyarrow by hand, and two day boundaries
INT96_NS = [0, -1, 1, -86400000000001, 2 ** 62, -2 ** 62, 86400 * 10 ** 9 - 1, -86400 * 10 ** 9]

# ---- pyarrow files --------------------------------------------------------------------------------


def _pa():
    import pyarrow as pa
    import pyarrow.parquet as pq
    return pa, pq


def random_decimals(n, precision, scale, seed, null_every=5):
    """n Decimals across zero that use the whole precision now and then, every null_every-th None."""
    rng = np.random.default_rng(seed)
    digits = rng.integers(1, precision + 1, n)
    out = []
    for i in range(n):
        if null_every and i % null_every == null_every - 1:
            out.append(None)
            continue
        u = int.from_bytes(rng.bytes(32), "little") % (10 ** int(digits[i]))
        if rng.integers(0, 2):
            u = -u
        out.append(D(u).scaleb(-scale))
    return out


DECIMALS = {"d7": (7, 2), "d30": (30, 2), "d50": (50, 0), "d15": (15, 3)}


def decimal_table(n, seed=1, names=("d7", "d30", "d50"), null_every=5):
    pa, _ = _pa()
    cols = {}
    for k, name in enumerate(names):
        p, s = DECIMALS[name]
        typ = pa.decimal128(p, s) if p <= 38 else pa.decimal256(p, s)
        cols[name] = pa.array(random_decimals(n, p, s, seed + k, null_every), typ)
    return pa.table(cols)


def int96_table(n, seed=3, null_every=5):
    """ns timestamps: INT96_NS, then random ones inside pyarrow's datetime range."""
    pa, _ = _pa()
    rng = np.random.default_rng(seed)
    ns = np.r_[np.array(INT96_NS, np.int64), rng.integers(-2 ** 62, 2 ** 62, max(n - len(INT96_NS), 0))][:n]
    mask = np.zeros(n, bool)
    if null_every:
        mask[null_every + 4::null_every] = True  # the hand-checked values stay
    return pa.table({"ts": pa.array(ns, pa.timestamp("ns"), mask=mask)})


def write(table, dictionary=False, compression="NONE", **kw):
    _, pq = _pa()
    b = io.BytesIO()
    kw.setdefault("data_page_size", 1 << 16)
    pq.write_table(table, b, use_dictionary=dictionary, compression=compression, **kw)
    return b.getvalue()


def value_bytes(column, w):
    """The value buffer of a pyarrow (chunked) array of w-byte values with nulls dropped."""
    arr = column.combine_chunks() if hasattr(column, "combine_chunks") else column
    arr = arr.drop_null()
    buf = np.frombuffer(arr.buffers()[1], np.uint8)
    return buf[arr.offset * w:(arr.offset + len(arr)) * w].copy()


def read(data, **kw):
    _, pq = _pa()
    return pq.read_table(io.BytesIO(data), **kw)


# ---- hand-built footers: SchemaElements of converted types only ------------------------------------


def _uv(v):
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7f | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _zz(v):
    return _uv((v << 1) ^ (v >> 63))


def _elem(name, typ=None, type_length=None, rep=None, num_children=None, converted=None, scale=None, precision=None):
    """A thrift-compact SchemaElement with the given fields (ids 1..8), in id order."""
    out, last = bytearray(), 0
    for fid, kind, v in ((1, 5, typ), (2, 5, type_length), (3, 5, rep), (4, 8, name), (5, 5, num_children),
                         (6, 5, converted), (7, 5, scale), (8, 5, precision)):
        if v is None:
            continue
        out.append((fid - last) << 4 | kind)
        last = fid
        if kind == 8:
            b = v.encode()
            out += _uv(len(b)) + b
        else:
            out += _zz(v)
    out.append(0)
    return bytes(out)


def converted_only_file(leaves):
    """A parquet file of no row groups whose footer holds a root and `leaves`: dicts of _elem's
    arguments.  Only the footer planner reads it."""
    elems = [_elem("schema", num_children=len(leaves))] + [_elem(**l) for l in leaves]
    assert len(elems) < 15
    meta = bytearray()
    meta += bytes([0x15]) + _zz(1)                                   # 1: version
    meta += bytes([0x19, len(elems) << 4 | 12]) + b"".join(elems)    # 2: schema
    meta += bytes([0x16]) + _zz(0)                                   # 3: num_rows
    meta += bytes([0x19, 0x0c])                                      # 4: row_groups, empty
    meta.append(0)
    return b"PAR1" + bytes(meta) + len(meta).to_bytes(4, "little") + b"PAR1"


def logical_table():
    """One column per logical type the footer planner tells apart (INT96 has a file of its own:
    pyarrow's INT96 switch turns every timestamp column into one)."""
    pa, _ = _pa()
    three = [1, 2, None]
    return pa.table({
        "dec_flba": pa.array([D("1.23"), None, D("-1.23")], pa.decimal128(7, 2)),
        "dec_wide": pa.array([D("1"), None, D("-1")], pa.decimal256(50, 0)),
        "ts_ms": pa.array(three, pa.timestamp("ms")),
        "ts_ms_utc": pa.array(three, pa.timestamp("ms", tz="UTC")),
        "ts_us": pa.array(three, pa.timestamp("us")),
        "ts_us_utc": pa.array(three, pa.timestamp("us", tz="UTC")),
        "ts_ns": pa.array(three, pa.timestamp("ns")),
        "ts_ns_utc": pa.array(three, pa.timestamp("ns", tz="UTC")),
        "date": pa.array(three, pa.date32()),
        "t32": pa.array(three, pa.time32("ms")),
        "t64": pa.array(three, pa.time64("us")),
        "u8": pa.array(three, pa.uint8()),
        "u16": pa.array(three, pa.uint16()),
        "u32": pa.array(three, pa.uint32()),
        "u64": pa.array(three, pa.uint64()),
        "i8": pa.array(three, pa.int8()),
        "i16": pa.array(three, pa.int16()),
        "i32": pa.array(three, pa.int32()),
        "i64": pa.array(three, pa.int64()),
        "s": pa.array(["a", "b", None]),
        "f16": pa.array(np.array([1, 2, 3], np.float16)),
        "lst": pa.array([[D("1.5")], None, [D("-2.5"), None]], pa.list_(pa.decimal128(9, 1))),
    })


def logical_int_table():
    """Decimals that store_decimal_as_integer writes as INT32 / INT64."""
    pa, _ = _pa()
    return pa.table({"dec_i32": pa.array([D("1.23"), None, D("-1.23")], pa.decimal128(7, 2)),
                     "dec_i64": pa.array([D("1.234"), None, D("-1.234")], pa.decimal128(15, 3))})
