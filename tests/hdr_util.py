"""Page headers no ordinary writer emits, and chunks made of them.

`HW` writes thrift compact-protocol bytes field by field: short- or long-form field headers, ids
that wrap as int16, padded varints, values of every compact type, nested containers.  `Hdr` is a
PageHeader spec built on it (field order, repeats, wrong types, Statistics, unknown fields);
`pad_to` sizes a Statistics binary so that a header has an exact length; `chunk` joins
(spec, payload) pages into chunk bytes for parity.compare_chunk_bytes; `random_header` and `mutate`
feed the host model of the parser (test_thrift_model.py).
"""
import numpy as np

# compact-protocol type nibbles
C_TRUE, C_FALSE, C_BYTE, C_I16, C_I32, C_I64, C_DOUBLE, C_BIN, C_LIST, C_SET, C_MAP, C_STRUCT = range(1, 13)


def uvarint(v, pad=0):
    """LEB128 of v >= 0; `pad` extra continuation bytes (0x80 .. 0x00) that add nothing."""
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    if pad:
        out[-1] |= 0x80
        out += b"\x80" * (pad - 1) + b"\x00"
    return bytes(out)


def zz(v):
    return (v << 1) ^ (v >> 63) if v < 0 else v << 1


class HW:
    """Compact-protocol writer.  `long=True` writes a field header in long form (type byte, then
    the id as a zigzag varint: any integer, read as int16); `pad` pads the value's varint."""

    def __init__(self):
        self.b = bytearray()
        self.last = [0]

    def field(self, fid, ctype, long=False, idpad=0):
        d = fid - self.last[-1]
        if not long and 0 < d <= 15:
            self.b.append((d << 4) | ctype)
        else:
            self.b.append(ctype)
            self.b += uvarint(zz(fid), idpad)
        self.last[-1] = ((fid + 0x8000) & 0xFFFF) - 0x8000  # the reader keeps it as int16
        return self

    def raw(self, data):
        self.b += bytes(data)
        return self

    def i32(self, fid, v, long=False, pad=0, ctype=C_I32):
        self.field(fid, ctype, long)
        self.b += uvarint(zz(v), pad)
        return self

    def i64(self, fid, v, long=False, pad=0):
        return self.i32(fid, v, long, pad, C_I64)

    def boolean(self, fid, v, long=False):
        return self.field(fid, C_TRUE if v else C_FALSE, long)

    def byte(self, fid, v, long=False):
        self.field(fid, C_BYTE, long)
        self.b.append(v & 0xFF)
        return self

    def double(self, fid, long=False):
        self.field(fid, C_DOUBLE, long)
        self.b += b"\x18\x2d\x44\x54\xfb\x21\x09\x40"
        return self

    def binary(self, fid, data, long=False, pad=0, claim=None):
        """`claim`: the length written, when not len(data) (negative values wrap as int32)."""
        self.field(fid, C_BIN, long)
        n = len(data) if claim is None else claim & 0xFFFFFFFF
        self.b += uvarint(n, pad) + bytes(data)
        return self

    def begin(self, fid, long=False):
        self.field(fid, C_STRUCT, long)
        self.last.append(0)
        return self

    def end(self):
        self.b.append(0)
        self.last.pop()
        return self

    def list_of(self, fid, etype, items, ctype=C_LIST, long=False):
        """A list (or set) header and its elements' bytes (`items`: a list of bytes)."""
        self.field(fid, ctype, long)
        n = len(items)
        self.b += bytes([(n << 4) | etype]) if n < 15 else bytes([0xF0 | etype]) + uvarint(n)
        for it in items:
            self.b += it
        return self

    def map_of(self, fid, ktype, vtype, pairs, long=False):
        self.field(fid, C_MAP, long)
        self.b += uvarint(len(pairs))
        if pairs:
            self.b.append((ktype << 4) | vtype)
        for k, v in pairs:
            self.b += k + v
        return self

    def nested(self, fid, depth, long=False):
        """An unknown struct nested `depth` deep, an i32 in the innermost."""
        for k in range(depth):
            self.begin(fid if k == 0 else 1, long and k == 0)
        self.i32(1, 5)
        for _ in range(depth):
            self.end()
        return self

    def bools(self, first, k):
        """k unknown one-byte bool fields with ids first, first + 1, ..."""
        for i in range(k):
            self.boolean(first + i, i & 1)
        return self

    def every_type(self, first):
        """One unknown field of every compact type, ids first ..: 12 fields."""
        f = first
        self.boolean(f, True).boolean(f + 1, False).byte(f + 2, 0x15).i32(f + 3, -300, ctype=C_I16)
        self.i32(f + 4, 1 << 20).i64(f + 5, -(1 << 40)).double(f + 6).binary(f + 7, b"\x15\x00\x15\x02")
        self.list_of(f + 8, C_TRUE, [b"\x01", b"\x00", b"\x02"])  # bools in a list: one byte each
        self.list_of(f + 9, C_I32, [b"\x02"], ctype=C_SET)
        self.map_of(f + 10, C_I32, C_BIN, [(b"\x02", b"\x01a"), (b"\x04", b"\x00")])
        self.nested(f + 11, 2)
        return self

    def stop(self):
        self.b.append(0)
        return bytes(self.b)


def struct_bytes(fn):
    """The bytes of a struct VALUE (fields and STOP) written by fn(HW): a list element, a map value."""
    w = HW()
    fn(w)
    return w.stop()


class Hdr:
    """A PageHeader spec; build(usize, csize) gives its bytes.

    kind       1 (DataPageHeader, field 5), 2 (DataPageHeaderV2, field 8) or "dict" (field 7)
    nvals, enc, def_len, rep_len, nnulls, nrows: the page-header struct's fields
    stats      None, or a function(HW) writing the fields of a Statistics struct (field 5 of a
               DataPageHeader, 8 of a V2); see `stats_fields`
    order      the top-level field ids in the order written; an id may repeat (the last one read
               wins: an earlier copy of 1-3 is written with `stale` added to its value), "5"
               stands for the page-header struct of `kind`; 4 is the crc (values from `crcs`, in turn);
               6 an IndexPageHeader; ("x", fn) calls fn(HW) there (unknown fields)
    long       top-level ids written in long form; `wrap`: long-form ids written + 65536
    pad        {top-level id: varint padding bytes}
    wide       top-level ids whose varint gets bit 36 set (wider than 32 bits: the i32 read drops it)
    wrong      top-level ids written with the wrong type (i64): skipped, so a required one is missing
    inner      function(HW) called inside the page-header struct after its own fields
    inner_order the page-header struct's field ids in the order written (default: id order)
    second     another page-header struct in the same header: (field id 5 or 8, nvals, enc)
    type_      the PageHeader.type written (default: what `kind` means)
    """

    def __init__(self, kind=1, nvals=0, enc=0, **kw):
        self.kind, self.nvals, self.enc = kind, nvals, enc
        self.def_len = self.rep_len = self.nnulls = 0
        self.nrows = None
        self.stats = None
        self.order = None
        self.long, self.wrap, self.pad, self.wide, self.wrong = (), (), {}, (), ()
        self.inner = None
        self.inner_order = None
        self.second = None
        self.type_ = None
        self.crcs = ()
        self.stale = 1000
        self.def_enc = self.rep_enc = 3
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError(k)
            setattr(self, k, v)

    def with_(self, **kw):
        h = Hdr.__new__(Hdr)
        h.__dict__.update(self.__dict__)
        for k, v in kw.items():
            if not hasattr(h, k):
                raise TypeError(k)
            setattr(h, k, v)
        return h

    def _page_struct(self, w, fid, kind, nvals, enc):
        w.begin(fid, fid in self.long or fid in self.wrap)
        if kind == 1:
            fields = {1: nvals, 2: enc, 3: self.def_enc, 4: self.rep_enc}
            sid = 5
        elif kind == 2:
            fields = {1: nvals, 2: self.nnulls, 3: nvals if self.nrows is None else self.nrows, 4: enc,
                      5: self.def_len, 6: self.rep_len}
            sid = 8
        else:
            fields = {1: nvals, 2: enc}
            sid = None
        order = self.inner_order or (sorted(fields) + ([7] if kind == 2 else []) + ([sid] if sid else []))
        for f in order:
            if f in fields:
                w.i32(f, fields[f])
            elif f == 7 and kind == 2:
                w.boolean(7, True)
            elif f == sid and self.stats is not None:
                w.begin(sid)
                self.stats(w)
                w.end()
        if self.inner:
            self.inner(w)
        w.end()

    def build(self, usize, csize):
        w = HW()
        type_ = self.type_ if self.type_ is not None else {1: 0, 2: 3, "dict": 2}[self.kind]
        vals = {1: type_, 2: usize, 3: csize}
        order = list(self.order or [1, 2, 3] + ([4] if self.crcs else []) + ["5"])
        crcs = list(self.crcs)
        left = {f: order.count(f) for f in (1, 2, 3)}
        for f in order:
            if isinstance(f, tuple):
                f[1](w)
            elif f == "5":
                self._page_struct(w, {1: 5, 2: 8, "dict": 7}[self.kind], self.kind, self.nvals, self.enc)
                if self.second:
                    sf, nv, en = self.second
                    self._page_struct(w, sf, {5: 1, 8: 2}[sf], nv, en)
            elif f == 6:
                w.begin(6, 6 in self.long).end()
            elif f in (1, 2, 3, 4):
                if f == 4:
                    v = crcs.pop(0)
                    v = v - (1 << 32) if v >= 1 << 31 else v  # the i32 that reads back as this u32
                else:
                    left[f] -= 1
                    v = vals[f] + (self.stale if left[f] else 0)
                # wide: bit 36 set on top of the value's 32 bits (the i32 read truncates it away)
                raw = uvarint((zz(v) & 0xFFFFFFFF) | (1 << 36)) if f in self.wide else None
                fid = f + 65536 if f in self.wrap else f
                if f in self.wrong:
                    w.i64(fid, v, f in self.long or f in self.wrap)
                elif raw is not None:
                    w.field(fid, C_I32, f in self.long or f in self.wrap).raw(raw)
                else:
                    w.i32(fid, v, f in self.long or f in self.wrap, self.pad.get(f, 0))
            else:
                raise ValueError(f)
        return w.stop()


def stats_fields(min_value=None, max_value=None, null_count=None, distinct=None, maxd=None, mind=None, extra=None):
    """A Statistics writer: ids 5 (max_value), 6 (min_value), 3 (null_count), 4 (distinct_count),
    1 (max, deprecated), 2 (min, deprecated), in id order; `extra`(HW) writes unknown fields after."""
    def fn(w):
        if maxd is not None:
            w.binary(1, maxd)
        if mind is not None:
            w.binary(2, mind)
        if null_count is not None:
            w.i64(3, null_count)
        if distinct is not None:
            w.i64(4, distinct)
        if max_value is not None:
            w.binary(5, max_value)
        if min_value is not None:
            w.binary(6, min_value)
        if extra:
            extra(w)
    return fn


def pad_to(n, usize, csize, base=None, fill=0x61):
    """(spec, header bytes): `base` (default a V1 header of 12 values) with a Statistics whose
    max_value is sized so that the header is exactly n bytes for these sizes."""
    base = base or Hdr(1, nvals=12)

    def spec_of(k, pad):
        return base.with_(stats=lambda w: w.i64(3, 0).binary(5, bytes([fill]) * k, pad=pad))
    empty = len(spec_of(0, 0).build(usize, csize))
    # the binary's length varint grows with it: a few candidates below the difference, and one
    # padding byte for the length that the growth steps over
    for k in range(max(0, n - empty - 3), max(0, n - empty) + 1):
        for pad in (0, 1):
            spec = spec_of(k, pad)
            b = spec.build(usize, csize)
            if len(b) == n:
                return spec, b
    raise ValueError("no header of %d bytes" % n)


def plain_i32(values):
    return np.asarray(values, dtype="<i4").tobytes()


def chunk(pages):
    """Chunk bytes of (spec, payload[, usize]) pages, and each page's (header_offset, payload_offset)."""
    out = bytearray()
    at = []
    for pg in pages:
        spec, payload = pg[0], pg[1]
        h = spec.build(pg[2] if len(pg) > 2 else len(payload), len(payload))
        at.append((len(out), len(out) + len(h)))
        out += h + payload
    return bytes(out), at


# ---------------------------------------------------------------- generated headers (host model)
def random_header(rng):
    """One generated header (rng: a random.Random): mostly valid, every feature of Hdr / HW with some probability."""
    kind = (1, 1, 2, 2, "dict")[rng.randrange(5)]
    kw = {}
    r = rng.random
    ri = rng.randrange
    if kind != "dict" and r() < 0.5:
        ex = None
        if r() < 0.3:
            d = ri(1, 8)
            ex = lambda w, d=d: w.nested(9, d).bools(20, int(d))  # noqa: E731
        kw["stats"] = stats_fields(max_value=b"z" * ri(0, 200) if r() < 0.8 else None,
                                   min_value=b"a" * ri(0, 40) if r() < 0.8 else None,
                                   null_count=ri(0, 1 << 40) if r() < 0.7 else None,
                                   distinct=7 if r() < 0.2 else None, maxd=b"q" if r() < 0.2 else None,
                                   mind=b"" if r() < 0.2 else None, extra=ex)
    order = [1, 2, 3, "5"]
    if r() < 0.3:
        order.insert(ri(0, 5), 4)
        kw["crcs"] = [ri(0, 1 << 32), 5]
    if r() < 0.2:
        order = rng.sample(order, len(order))
    if r() < 0.15:
        order.insert(ri(0, len(order) + 1), ri(1, 4))
        if 4 in order:
            order.append(4)
    if r() < 0.1:
        order.insert(ri(0, len(order) + 1), 6)
    if r() < 0.35:
        k = ri(0, 6)
        n = ri(1, 45)
        fn = [lambda w: w.every_type(30), lambda w: w.bools(40, n), lambda w: w.nested(60, 1 + n % 10),
              lambda w: w.list_of(70, C_STRUCT, [struct_bytes(lambda s: s.nested(1, n % 5 + 1))] * (n % 4)),
              lambda w: w.map_of(80, C_BIN, C_STRUCT, [(b"\x01k", struct_bytes(lambda s: s.i32(1, 1)))] * (n % 3)),
              lambda w: w.list_of(90, C_LIST, [bytes([0x25, 2, 4])] * (n % 17))][k]
        order.insert(ri(0, len(order) + 1), ("x", fn))
    kw["order"] = order
    if r() < 0.15:
        kw["long"] = (ri(1, 9), ri(1, 9))
    if r() < 0.08:
        kw["wrap"] = (ri(1, 4),)
    if r() < 0.15:
        kw["pad"] = {ri(1, 4): ri(1, 12)}
    if r() < 0.05:
        kw["wide"] = (ri(1, 4),)
    if r() < 0.05:
        kw["wrong"] = (ri(1, 4),)
    if r() < 0.1 and kind != "dict":
        kw["second"] = ((5, 8)[kind == 1], ri(0, 99), ri(0, 9))
    if r() < 0.1:
        kw["type_"] = ri(0, 5)
    if r() < 0.2:
        n = ri(1, 30)
        kw["inner"] = [lambda w: w.bools(20, n), lambda w: w.every_type(20), lambda w: w.nested(20, 1 + n % 8)][n % 3]
    if kind != "dict" and r() < 0.1:
        io = [1, 2, 3, 4] + ([5] if kind == 1 else [5, 6, 7, 8])
        kw["inner_order"] = rng.sample(io, len(io))
    spec = Hdr(kind, nvals=ri(0, 70000), enc=ri(0, 9), **kw)
    return spec.build(ri(0, 1 << 20), ri(0, 1 << 20))


def mutate(rng, b):
    """Truncation, a byte set, or a bit flipped (rng: a random.Random; b not empty)."""
    b = bytearray(b)
    k = rng.randrange(3)
    i = rng.randrange(len(b))
    if k == 0:
        return bytes(b[:i])
    if k == 1:
        b[i] = (0x00, 0x15, 0x80, 0xFF, 0x1C, 0x19, 0x1B, 0x0D)[rng.randrange(8)]
    else:
        b[i] ^= 1 << rng.randrange(8)
    return bytes(b)
