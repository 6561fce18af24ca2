"""Helpers of the BYTE_STREAM_SPLIT tests (test_bss_model.py, test_bss.py): the numpy model of the
encoding, hand-built V1 pages and chunks, pyarrow-written files with their PLAIN twins."""
import io

import numpy as np

import pqtest_util as U
from pqgpu import abi

ENC = abi.ENC_BYTE_STREAM_SPLIT  # 9

# (physical type, type_length) -> bytes per value
TYPES = {"int32": (abi.INT32, -1, 4), "float": (abi.FLOAT, -1, 4), "int64": (abi.INT64, -1, 8),
         "double": (abi.DOUBLE, -1, 8)}


def flba(w):
    return (abi.FIXED_LEN_BYTE_ARRAY, w, w)


# ---- the model ----------------------------------------------------------------------------------

def encode(values: bytes, w: int) -> bytes:
    """nn values of w bytes -> w streams of nn bytes: val[k * nn + i] = values[i * w + k]."""
    nn = len(values) // w
    assert nn * w == len(values)
    return np.frombuffer(values, np.uint8).reshape(nn, w).T.tobytes()


def decode(val: bytes, nn: int, w: int) -> bytes:
    """The inverse: the streams' stride is nn, whatever len(val) is (it must be nn * w)."""
    assert len(val) == nn * w
    return np.frombuffer(val, np.uint8).reshape(w, nn).T.tobytes()


# ---- hand-built pages ---------------------------------------------------------------------------

def def_levels(mask) -> bytes:
    """A 1-bit level stream (RLE/bit-packed hybrid, one bit-packed run) for a boolean mask."""
    mask = np.asarray(mask, bool)
    groups = (len(mask) + 7) // 8
    bits = np.zeros(groups * 8, np.uint8)
    bits[:len(mask)] = mask
    return U.uvarint(groups << 1 | 1) + np.packbits(bits, bitorder="little").tobytes()


def mask_for(nn, seed=0):
    """num_values > nn slots with exactly nn of them set (an odd count, so the level prefix of a V1 page
    leaves the value bytes on an odd offset for most nn)."""
    slots = nn + 3 + nn // 5
    rng = np.random.default_rng(1000 + seed + nn)
    m = np.zeros(slots, bool)
    m[rng.permutation(slots)[:nn]] = True
    return m


def page(values: bytes, w: int, mask=None, enc=ENC, val_bytes=None):
    """A V1 page of BSS values (required, or optional with `mask` as its def levels); `val_bytes`
    replaces the encoded value bytes (for pages that are short or long)."""
    nn = len(values) // w
    val = encode(values, w) if val_bytes is None else val_bytes
    if mask is None:
        return U.v1_page(val, nn, enc)
    assert int(np.sum(mask)) == nn
    return U.v1_page(val, len(mask), enc, defs=def_levels(mask))


def random_values(nn, w, seed):
    return np.random.default_rng(seed * 7919 + nn * 31 + w).integers(0, 256, nn * w, dtype=np.uint8).tobytes()


def decode_chunks(dec, chunks, lead=0, tail=64):
    """One pqg_decode_chunks call over hand-built chunks [(bytes, ptype, type_length, max_def)] of one
    upload, chunk k `lead + k` bytes past a 256-byte boundary; `tail` bytes follow the last chunk in
    the device buffer (0: its last byte is the buffer's last).  -> [DecodedColumn]"""
    blob, offs = bytearray(), []
    for k, (ch, _, _, _) in enumerate(chunks):
        blob += bytes(-len(blob) % 256 + (lead + k) % 16)
        offs.append(len(blob))
        blob += ch
    dev = dec.upload(bytes(blob) + bytes(tail))
    try:
        jobs = []
        for off, (ch, ptype, tl, max_def) in zip(offs, chunks):
            j, _ = U.chunk_job(ch, ptype=ptype, type_length=tl, max_def=max_def)
            j.data = dev + off
            jobs.append(j)
        res = dec.decode_jobs(jobs)
        return [dec.download(r, i) for i, r in enumerate(res)]
    finally:
        dec.free(dev)


# ---- pyarrow files and their twins --------------------------------------------------------------

def arrow_array(kind, n, null_every=5, seed=3, distinct=16):
    """n values of `kind`: random choices from `distinct` values, each repeated 16 times (so that every
    page compresses under the codecs without an entropy stage too: the streams of random choices among
    16 bytes are nothing snappy or lz4 can shorten), every `null_every`-th one null."""
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    np_dt = {"float32": np.float32, "float64": np.float64, "int32": np.int32, "int64": np.int64,
             "float16": np.float16}[kind]
    pool = (rng.standard_normal(distinct) * 1000).astype(np_dt) if kind.startswith("float") else \
        rng.integers(-2 ** 30, 2 ** 30, distinct).astype(np_dt)
    vals = np.repeat(pool[rng.integers(0, distinct, n // 16 + 1)], 16)[:n]
    mask = np.arange(n) % null_every == 0 if null_every else np.zeros(n, bool)
    return pa.array(vals, mask=mask)


def write(table, split, **kw):
    """The BSS file (`split`) or its twin: the same table, pages cut the same, PLAIN, uncompressed, V1."""
    import pyarrow.parquet as pq
    buf = io.BytesIO()
    args = dict(use_dictionary=False, write_statistics=False, data_page_size=4096, compression="none")
    args.update(kw)
    if not split:
        args.update(compression="none", data_page_version="1.0")
    pq.write_table(table, buf, use_byte_stream_split=bool(split), **args)
    return buf.getvalue()
