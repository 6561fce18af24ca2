"""Helpers of the keep-dictionary tests (test_dict_out.py on the GPU, test_dict_out_host.py on the
CPU): hand-built dictionary chunks, the seeded single-byte mutations of a small three-column file,
and what the oracle's page tables say about them."""
import numpy as np

import pqgpu
import pqtest_util as U
from gen import pqwrite as W
from oracle import pyoracle as O
from pqgpu import abi

NOT_DICT = -19
PAGE_CAP = 4096  # page-table entries asked for per chunk (the default of 2^20 costs 80 MB per call)


def download(dec, r, i):
    """GpuDecoder.download with a page table of PAGE_CAP entries."""
    got = dec.download(r, None)
    got.pages = dec.pages(i, PAGE_CAP)
    if r.status == 0 and r.col_flags & abi.COL_KEEP_DICT:
        got.dictionary = dec.dictionary(i)
    return got


# ---- hand-built chunks ---------------------------------------------------------------------------
def dict_page(entries: bytes, count, enc=0):
    return U.page_header_dict(len(entries), len(entries), count, enc) + entries


def int32_dict(count, seed=0):
    """A PLAIN INT32 dictionary page of `count` distinct entries."""
    vals = (np.arange(count, dtype=np.int64) * 2654435761 + seed).astype(np.uint32).astype("<u4")
    return dict_page(vals.tobytes(), count)


def key_stream(keys, width, kind="mixed"):
    """The values section of an RLE_DICTIONARY page: the width byte and the hybrid stream of `keys`
    as RLE runs only, bit-packed runs only, or whatever the encoder picks (runs of >= 8 as RLE)."""
    if width == 0:
        return bytes([0])
    min_rle = {"rle": 1, "packed": 1 << 30, "mixed": 8}[kind]
    return bytes([width]) + W.hybrid_encode(np.asarray(keys, np.uint32), width, min_rle)


def gen_keys(nn, count, kind, seed):
    """nn keys below `count`: long runs for "rle", no two equal neighbours for "packed", both for "mixed"."""
    rng = np.random.default_rng(seed * 1000003 + nn * 31 + count)
    if count <= 1 or nn == 0:
        return np.zeros(nn, np.uint32)
    if kind == "rle":
        return np.repeat(rng.integers(0, count, nn // 37 + 1), 37)[:nn].astype(np.uint32)
    k = rng.integers(0, count, nn).astype(np.int64)
    if kind == "packed":
        same = np.r_[False, k[1:] == k[:-1]]
        k[same] = (k[same] + 1) % count
        return k.astype(np.uint32)
    runs = np.repeat(rng.integers(0, count, nn // 23 + 1), 23)[:nn]
    return np.where((np.arange(nn) // 61) % 2 == 0, k, runs).astype(np.uint32)


def def_stream(mask) -> bytes:
    """A 1-bit def-level stream (one bit-packed run) for a boolean mask."""
    mask = np.asarray(mask, bool)
    groups = (len(mask) + 7) // 8
    bits = np.zeros(groups * 8, np.uint8)
    bits[:len(mask)] = mask
    return U.uvarint(groups << 1 | 1) + np.packbits(bits, bitorder="little").tobytes()


def data_page(keys, width, kind="mixed", mask=None, values=None):
    """A V1 RLE_DICTIONARY page of `keys` (required, or optional with `mask` as its def levels);
    `values` replaces the values section."""
    val = key_stream(keys, width, kind) if values is None else values
    if mask is None:
        return U.v1_page(val, len(keys), 8)
    return U.v1_page(val, len(mask), 8, defs=def_stream(mask))


# ---- one batch through both decoders ---------------------------------------------------------------
def run_batch(dec, chunks, flags=None):
    """chunks: [(bytes, kwargs of pqtest_util.chunk_job)]; one pqg_decode_chunks call with
    pqg_column_desc.flags |= flags[k] (default: COL_KEEP_DICT on every job).
    -> [(oracle chunk of the job without the flag, ChunkResult, DecodedColumn)]"""
    flags = [abi.COL_KEEP_DICT] * len(chunks) if flags is None else flags
    blob, offs = bytearray(), []
    for ch, _ in chunks:
        blob += bytes(-len(blob) % 256)
        offs.append(len(blob))
        blob += ch
    exps, jobs, keep = [], [], []
    for ch, kw in chunks:
        j, _ = U.chunk_job(ch, keep=keep, **kw)
        exps.append(O.decode_chunk(j, PAGE_CAP))
        jobs.append(j)
    dev = dec.upload(bytes(blob) + bytes(64))
    try:
        for j, off, f in zip(jobs, offs, flags):
            j.data = dev + off
            j.col.flags |= f
        plain_pages(dec, jobs, exps)
        res = dec.decode_jobs(jobs)
        return [(e, r, download(dec, r, i)) for i, (e, r) in enumerate(zip(exps, res))]
    finally:
        dec.free(dev)


def plain_pages(dec, jobs, exps):
    """The page tables of the same jobs decoded on the GPU without the flag, kept as exp.gpu_pages: what a
    failed chunk's flagged page table is compared with (see check_kept)."""
    saved = [j.col.flags for j in jobs]
    for j in jobs:
        j.col.flags &= ~abi.COL_KEEP_DICT
    res = dec.decode_jobs(jobs)
    for i, (e, r) in enumerate(zip(exps, res)):
        assert r.status == e.status and r.error_page == e.error_page, "job %d without the flag" % i
        e.gpu_pages = dec.pages(i, PAGE_CAP)
    for j, f in zip(jobs, saved):
        j.col.flags = f


HEADER_FIELDS = ("header_offset", "payload_offset", "page_type", "encoding", "num_values", "compressed_size",
                 "uncompressed_size")
DECODE_FIELDS = ("slot_offset", "value_offset", "not_null", "status")


def same_pages(got, exp, where="", fields=HEADER_FIELDS + DECODE_FIELDS):
    assert len(got) == len(exp), "%s: %d pages vs %d" % (where, len(got), len(exp))
    for k, (a, b) in enumerate(zip(got, exp)):
        fa, fb = [getattr(a, f) for f in fields], [getattr(b, f) for f in fields]
        assert fa == fb, "%s page %d: %s vs %s" % (where, k, fa, fb)


def check_kept(exp, r, got, where="", keys=None, pages=True):
    """The flagged result (r, got) against the oracle's decode `exp` of the same bytes without the flag
    (pages=False: of an uncompressed twin, whose page table has other offsets and sizes)."""
    assert got.status == exp.status, "%s status %s, oracle %s (pages %d / %d)" % (
        where, abi.status_name(got.status), abi.status_name(exp.status), got.error_page, exp.error_page)
    assert got.error_page == exp.error_page, "%s error page %d vs %d" % (where, got.error_page, exp.error_page)
    assert r.col_flags & abi.COL_KEEP_DICT, where
    if exp.status != 0:
        # The page table of a failed chunk.  The oracle stops where the reference stops, so from the
        # failing page on its counts and offsets (not_null, slot_offset, value_offset) stay 0, while
        # the GPU decodes every listed page, with or without the flag; the failing page's own record
        # holds what the oracle had parsed of its header when it stopped.  Against the oracle: the
        # same number of pages, and what the headers of the pages before the failing one say; every
        # field of every page against the GPU's own table without the flag.
        if pages:
            assert len(got.pages) == len(exp.pages), where
            ep = max(exp.error_page, 0)
            same_pages(got.pages[:ep], exp.pages[:ep], where, HEADER_FIELDS)
            same_pages(got.pages, exp.gpu_pages, where + " (GPU without the flag)")
        return None
    assert r.value_width == 4 and not r.offsets and r.values_bytes == 4 * exp.num_values, where
    assert (got.num_slots, got.num_values) == (exp.num_slots, exp.num_values), where
    for a, b, what in ((got.def_levels, exp.def_levels, "def"), (got.rep_levels, exp.rep_levels, "rep")):
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), "%s %s levels" % (where, what)
    if pages:
        same_pages(got.pages, exp.pages, where)
    d = got.dictionary
    assert d is not None and d.value_width == exp.value_width, where
    k = got.keys()
    assert len(k) == exp.num_values and (len(k) == 0 or (k.min() >= 0 and k.max() < d.count)), where
    if keys is not None:
        assert np.array_equal(k, np.asarray(keys).astype(np.int32)), where + " keys"
    m = got.materialize()
    assert m.dictionary is None and m.value_width == exp.value_width, where
    ev = np.asarray(exp.values if exp.values is not None else np.zeros(0, np.uint8), np.uint8)
    assert m.values.nbytes == ev.nbytes and np.array_equal(m.values, ev), where + " values"
    if exp.value_width == 0:
        assert np.array_equal(m.offsets, exp.offsets), where + " offsets"
    return d


def run_file(dec, data, flags=None, twin=None):
    """Every chunk of a file in one batch, flagged (or as `flags` says) -> run_batch's triples.
    `twin`: the same table written uncompressed, for the oracle (it has no ZSTD or LZ4 decoder)."""
    pf = pqgpu.ParquetFile(data)
    specs = [(rg, c) for rg in range(pf.num_row_groups) for c in range(pf.num_columns)]
    flags = [abi.COL_KEEP_DICT] * len(specs) if flags is None else flags
    po = pf if twin is None else pqgpu.ParquetFile(twin)
    exps = [O.decode_chunk(po.host_job(rg, c)[0], PAGE_CAP) for rg, c in specs]
    dev = dec.upload(pf.data)
    try:
        jobs = [pqgpu.device_job(pf, rg, c, dev) for rg, c in specs]
        for j, f in zip(jobs, flags):
            j.col.flags |= f
        plain_pages(dec, jobs, exps)
        res = dec.decode_jobs(jobs)
        return [(e, r, download(dec, r, i)) for i, (e, r) in enumerate(zip(exps, res))]
    finally:
        dec.free(dev)


# ---- mutations -------------------------------------------------------------------------------------
MUTATION_SEED = 20
MUTATIONS = 200


def mutation_base():
    """A small three-column file, every chunk dictionary encoded: optional INT32 (V1), BYTE_ARRAY
    (V2, snappy), INT64 (V1)."""
    rng = np.random.default_rng(5)
    n = 1500
    nn = n - 200
    d = np.zeros(n, np.uint8)
    d[rng.choice(n, nn, replace=False)] = 1
    words = [b"", b"ab", b"dictionary", b"k" * 33, b"page"]
    pick = rng.integers(0, len(words), n)
    offs = np.zeros(n + 1, np.int64)
    np.cumsum([len(words[k]) for k in pick], out=offs[1:])
    cols = [W.Column("a", W.INT32, rng.integers(0, 40, nn).astype(np.int32), encoding=W.RLE_DICTIONARY,
                     repetition=W.OPTIONAL, def_levels=d, rows_per_page=400),
            W.Column("s", W.BYTE_ARRAY, np.frombuffer(b"".join(words[k] for k in pick), np.uint8), offsets=offs,
                     encoding=W.RLE_DICTIONARY, page_version=2, codec=W.SNAPPY, rows_per_page=500),
            W.Column("l", W.INT64, rng.integers(0, 300, n), encoding=W.RLE_DICTIONARY, rows_per_page=600)]
    return W.write_file(cols, n)


def mutations(seed=MUTATION_SEED, count=MUTATIONS):
    """[bytes]: `count` single-byte mutations of mutation_base(), inside its chunks' bytes."""
    base = mutation_base()
    pf = pqgpu.ParquetFile(base)
    spans = [(m.start, m.start + m.total_compressed_size) for m in (pf.chunk_meta(0, c) for c in range(3))]
    lo, hi = min(s[0] for s in spans), max(s[1] for s in spans)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        b = bytearray(base)
        pos = int(rng.integers(lo, hi))
        b[pos] ^= int(rng.integers(1, 256))
        out.append(bytes(b))
    return out


def other_encoding_page(exp):
    """The oracle's page list shows a data page that is not RLE_DICTIONARY / PLAIN_DICTIONARY."""
    return any(p.page_type in (0, 3) and p.encoding not in (2, 8) for p in exp.pages)
