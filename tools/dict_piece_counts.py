#!/usr/bin/env python3
"""Diagnostic: which piece paths of dict_page (pqg_dict.hip) the shapes of
tests/test_dict_pieces.py take, from the DProf counters of the -DPQG_PROFILE
build (make prof; PQG_LIB=.../libpqgpu_prof.so python tools/dict_piece_counts.py).
Per shape: used = pieces whose loads landed behind the head's stores, dropped =
loads past the page's end or issued again, fallback = pieces landed with a
plain wait, cold = a page's first piece, pieces = pieces staged."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "parquet-go_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import pqgpu  # noqa: E402
import parity as P  # noqa: E402
from pqgpu import abi  # noqa: E402
import test_dict_pieces as T  # noqa: E402

dec = pqgpu.GpuDecoder(0)
out = (C.c_uint64 * 192)()


def counts(name=None):
    k = dec.L.pqg_debug_counters(dec.ctx, out, 192)  # read + reset
    assert k >= 160, "not a -DPQG_PROFILE library"
    if name:
        print("%-34s used %5d  dropped %4d  fallback %4d  cold %4d  pieces %5d" % (
            name, out[140], out[141], out[142], out[143], out[132]), flush=True)


counts()
for w in sorted(T.WRITER_DICTS):
    rng = np.random.default_rng(100 + w)
    for dc in T.WRITER_DICTS[w]:
        P.compare_chunk_bytes(T.writer_chunk(rng, w, dc)[0], dec, ptype=abi.INT32, max_def=1)
        counts("writer w=%d dict=%d" % (w, dc))
rng = np.random.default_rng(200)
for gen in (T.rle_runs_chunk, T.long_rle_chunk):
    P.compare_chunk_bytes(gen(rng)[0], dec, ptype=abi.INT32)
    counts(gen.__name__)
P.compare_chunk_bytes(T.header_at_window_end(rng)[0], dec, ptype=abi.INT32)
counts("header_at_window_end")
for kind, where in T.CUTS:
    P.compare_chunk_bytes(T.cut_chunk(np.random.default_rng(300), kind, where)[0], dec, ptype=abi.INT32)
    counts("cut %s %s" % (kind, where))
for kind in sorted(T.BAD):
    for side in (0, 1):
        P.compare_chunk_bytes(T.bad_key_chunk(np.random.default_rng(400), kind, side)[0], dec, ptype=abi.INT32)
        counts("bad key %s side %d" % (kind, side))
T.test_mixed_batch(dec)
counts("mixed batch")
dec.close()
