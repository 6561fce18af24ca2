"""Page checksums for the tests: a small compact-thrift walk over the top-level fields of a
PageHeader that reads PageHeader.crc (field 4, i32), and rebuilds a header with the field set to
another value, added or removed; pyarrow files written with page checksums; chunks rebuilt from
edited pages.  zlib.crc32 is the reference."""
import io
import zlib

import numpy as np

import pqtest_util as U

T_BOOL_TRUE, T_BOOL_FALSE, T_BYTE, T_I16, T_I32, T_I64, T_DOUBLE, T_BINARY, T_LIST, T_SET, T_MAP, T_STRUCT = range(1, 13)


def _uvarint(b, p):
    v = s = 0
    while True:
        x = b[p]
        p += 1
        v |= (x & 0x7F) << s
        if x < 0x80:
            return v, p
        s += 7


def _unzig(v):
    return (v >> 1) ^ -(v & 1)


def _skip(b, p, t):
    """Position after the value of compact type `t` at p."""
    if t in (T_BOOL_TRUE, T_BOOL_FALSE):
        return p
    if t == T_BYTE:
        return p + 1
    if t in (T_I16, T_I32, T_I64):
        return _uvarint(b, p)[1]
    if t == T_DOUBLE:
        return p + 8
    if t == T_BINARY:
        n, p = _uvarint(b, p)
        return p + n
    if t in (T_LIST, T_SET):
        h = b[p]
        p += 1
        n = h >> 4
        if n == 15:
            n, p = _uvarint(b, p)
        for _ in range(n):
            p = _skip(b, p + (1 if (h & 15) in (T_BOOL_TRUE, T_BOOL_FALSE) else 0), h & 15)
        return p
    if t == T_MAP:
        n, p = _uvarint(b, p)
        if n:
            kv = b[p]
            p += 1
            for _ in range(n):
                p = _skip(b, p, kv >> 4)
                p = _skip(b, p, kv & 15)
        return p
    if t == T_STRUCT:
        while True:
            h = b[p]
            p += 1
            if h == 0:
                return p
            if h >> 4 == 0:
                p = _uvarint(b, p)[1]
            p = _skip(b, p, h & 15)
    raise ValueError("compact type %d" % t)


def header_fields(b, p=0):
    """Top-level fields of the struct at p: ([(id, type, value bytes)], position after its STOP)."""
    out, last = [], 0
    while True:
        h = b[p]
        p += 1
        if h == 0:
            return out, p
        if h >> 4:
            fid = last + (h >> 4)
        else:
            z, p = _uvarint(b, p)
            fid = _unzig(z)
        e = _skip(b, p, h & 15)
        out.append((fid, h & 15, bytes(b[p:e])))
        last = fid
        p = e


def header_crc(b, p=0):
    """(PageHeader.crc as uint32 or None, header length): the last field 4 of type i32."""
    fields, end = header_fields(b, p)
    v = None
    for fid, t, raw in fields:
        if fid == 4 and t == T_I32:
            v = _unzig(_uvarint(raw, 0)[0]) & 0xFFFFFFFF
    return v, end - p


def build_header(fields):
    out, last = bytearray(), 0
    for fid, t, raw in fields:
        d = fid - last
        if 0 < d <= 15:
            out.append((d << 4) | t)
        else:
            out.append(t)
            out += U.zigzag(fid)
        out += raw
        last = fid
    out.append(0)
    return bytes(out)


def with_crc(header, value):
    """The header with PageHeader.crc set to the uint32 `value` (None: without the field).  The varint
    may change length: the caller rebuilds the chunk."""
    fields, end = header_fields(header, 0)
    assert end == len(header)
    fields = [f for f in fields if f[0] != 4]
    if value is not None:
        v = value - (1 << 32) if value >= 1 << 31 else value  # the stored field is an i32
        fields.append((4, T_I32, U.zigzag(v)))
        fields.sort(key=lambda f: f[0])
    return build_header(fields)


class Page:
    def __init__(self, header, payload):
        self.header, self.payload = bytes(header), bytes(payload)

    @property
    def crc(self):
        return header_crc(self.header)[0]


def split_pages(chunk, table):
    """The chunk's pages from a page table (oracle or GPU: header_offset, payload_offset, compressed_size)."""
    out = []
    for p in table:
        out.append(Page(chunk[p.header_offset:p.payload_offset], chunk[p.payload_offset:p.payload_offset + p.compressed_size]))
    assert sum(len(p.header) + len(p.payload) for p in out) == len(chunk)
    return out


def join_pages(pages):
    """(chunk bytes, data_page_offset: where the first non-dictionary page starts)."""
    chunk, dpo = bytearray(), 0
    for k, p in enumerate(pages):
        if k == 1 and header_fields(pages[0].header)[0][0][2] == U.zigzag(2):
            dpo = len(chunk)
        chunk += p.header + p.payload
    return bytes(chunk), dpo


def flip(payload, at, bit=0):
    b = bytearray(payload)
    b[at] ^= 1 << bit
    return bytes(b)


def write_table(table, version="1.0", compression="none", checksum=True, **kw):
    import pyarrow.parquet as pq
    buf = io.BytesIO()
    args = dict(data_page_version=version, compression=compression, write_page_checksum=checksum,
                write_statistics=False, data_page_size=512, write_batch_size=32)
    args.update(kw)
    pq.write_table(table, buf, **args)
    return buf.getvalue()


def four_columns(n=5000, seed=1):
    """int32 PLAIN, int64 DELTA_BINARY_PACKED, dictionary strings, an optional float with nulls.
    The PLAIN values repeat in runs of 16 out of 16 distinct ones, so that every page compresses under
    every codec (a V2 page that does not is stored uncompressed by pyarrow, is_compressed = false,
    which this decoder does not honour)."""
    import pyarrow as pa
    rng = np.random.default_rng(seed)

    def runs(pool):
        return np.repeat(pool[rng.integers(0, len(pool), n // 16 + 1)], 16)[:n]
    words = ["w%03d" % i * (1 + i % 3) for i in range(40)]
    return pa.table({
        "i32": pa.array(runs(rng.integers(-2 ** 31, 2 ** 31, 16).astype(np.int32))),
        "i64": pa.array(np.cumsum(1 + (np.arange(n) % 32) * 37).astype(np.int64)),  # every miniblock the same bytes
        "s": pa.array([words[(i // 16) % 3] for i in range(n)]),  # index runs with a short period
        "f": pa.array(runs(rng.standard_normal(16).astype(np.float32)), mask=np.arange(n) % 7 == 0),
    }), dict(use_dictionary=["s"], column_encoding={"i32": "PLAIN", "i64": "DELTA_BINARY_PACKED", "f": "PLAIN"})


def crc32(b):
    return zlib.crc32(bytes(b)) & 0xFFFFFFFF
