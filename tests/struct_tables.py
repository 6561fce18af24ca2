"""The nested rows the struct tests share: plain Python rows with structs, lists
and maps (nulls at every level), and the pyarrow table of them.  The values come from small ranges, so
that even a page of a few dozen PLAIN values compresses: a V2 page that does not is stored
uncompressed by pyarrow, which the decoders here refuse as the reference does."""
import numpy as np


def rows(n, seed=5):
    """n rows of: s struct<a, b>; o struct<i struct<x, y>, z> with null outers and inners;
    ls list<struct<a, b>>; sl struct<l list<int>>; m map<string, int>; r a required struct."""
    rng = np.random.default_rng(seed)

    def maybe(p, make):
        return None if rng.random() < p else make()

    def i32():
        return int(rng.integers(0, 30))

    def word():
        return "w%d" % rng.integers(0, 20)

    def ab():
        return {"a": maybe(0.2, i32), "b": maybe(0.2, word)}

    def lst(make, p_empty=0.15, max_len=4):
        return [] if rng.random() < p_empty else [make() for _ in range(int(rng.integers(1, max_len + 1)))]

    out = []
    for _ in range(n):
        out.append({
            "s": maybe(0.2, ab),
            "o": maybe(0.2, lambda: {"i": maybe(0.25, lambda: {"x": maybe(0.2, lambda: int(rng.integers(0, 30)) << 33),
                                                                "y": maybe(0.2, lambda: float(rng.integers(0, 30)) / 4)}),
                                     "z": maybe(0.2, i32)}),
            "ls": maybe(0.15, lambda: lst(lambda: maybe(0.2, ab))),
            "sl": maybe(0.2, lambda: {"l": maybe(0.2, lambda: lst(lambda: maybe(0.2, i32)))}),
            "m": maybe(0.15, lambda: lst(lambda: (word(), maybe(0.2, i32)))),
            "r": {"p": i32(), "q": maybe(0.3, word)},
        })
    return out


def arrow_schema():
    import pyarrow as pa
    ab = pa.struct([("a", pa.int32()), ("b", pa.string())])
    return pa.schema([
        pa.field("s", ab),
        pa.field("o", pa.struct([("i", pa.struct([("x", pa.int64()), ("y", pa.float64())])), ("z", pa.int32())])),
        pa.field("ls", pa.list_(ab)),
        pa.field("sl", pa.struct([("l", pa.list_(pa.int32()))])),
        pa.field("m", pa.map_(pa.string(), pa.int32())),
        pa.field("r", pa.struct([pa.field("p", pa.int32(), nullable=False), pa.field("q", pa.string())]),
                 nullable=False),
    ])


def table(rs):
    import pyarrow as pa
    sch = arrow_schema()
    return pa.table([pa.array([r[f.name] for r in rs], f.type) for f in sch], schema=sch)


def file_bytes(t, **kw):
    import io
    import pyarrow.parquet as pq
    buf = io.BytesIO()
    pq.write_table(t, buf, **kw)
    return buf.getvalue()


def fit(rs, rg_rows):
    """pyarrow cuts a nested column's pages every 1024 slots, and the rest of the chunk is its last
    page; a V2 page of a handful of values does not shrink under snappy, pyarrow then stores it
    raw, and the decoders here, like the reference, unpack it regardless and fail.  So the last row
    of each row group gets lists that bring each list column's slots to 512 past a multiple of
    1024: every page then holds hundreds of values.  Changes `rs` in place and returns it."""
    def slots(x):
        return len(x) if x else 1

    cols = {"ls": (lambda r: r["ls"], lambda k: {"a": k % 7, "b": "w%d" % (k % 5)}),
            "sl": (lambda r: r["sl"] and r["sl"]["l"], lambda k: k % 7),
            "m": (lambda r: r["m"], lambda k: ("w%d" % (k % 5), k % 7))}
    for lo in range(0, len(rs), rg_rows):
        hi = min(lo + rg_rows, len(rs))
        for name, (get, make) in cols.items():
            have = sum(slots(get(r)) for r in rs[lo:hi - 1])
            long = [make(k) for k in range((512 - have) % 1024 or 1024)]
            rs[hi - 1][name] = {"l": long} if name == "sl" else long
    return rs
