#!/usr/bin/env python3
"""Diagnostic: which paths of the Snappy decoder (pqg_snappy.hip) the directed
cases of tests/snappy_build.py take, from SnapBlock's counters in the
-DPQG_PROFILE build (make prof; PQG_LIB=.../libpqgpu_prof.so python
tools/snappy_path_counts.py [family letters]).  One markdown table row per
case, each decoded as a bare block: dense batches, sparse windows, serial()
tags, batches with loads from below the ring, pointer-doubling rounds, tags
per dense batch; then what the path model (snappy_build.trace) says for the
first three, for blocks of one sub-block (the model walks a whole block; the
split decode starts afresh at every 64 KiB).  `!` marks a disagreement."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "parquet-go_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import pqgpu  # noqa: E402
from pqgpu import abi  # noqa: E402
import snappy_build as B  # noqa: E402

SN = 3 * 32  # pqg_debug_counters: 32 slots per translation unit; values, levels, strings, snappy
DENSE, SPARSE, TAGS, ROUNDS, FAR, SERIAL = SN + 9, SN + 10, SN + 12, SN + 13, SN + 14, SN + 21

dec = pqgpu.GpuDecoder(0)
out = (C.c_uint64 * 192)()
dst = np.zeros(1 << 20, np.uint8)
n = C.c_int64(0)


def counters():
    k = dec.L.pqg_debug_counters(dec.ctx, out, 192)  # read + reset
    assert k >= 128, "not a -DPQG_PROFILE library"
    return [int(out[i]) for i in (DENSE, SPARSE, SERIAL, FAR, ROUNDS, TAGS)]


families = sys.argv[1] if len(sys.argv) > 1 else "abcdefgh"
counters()
print("| case | dense batches | sparse windows | serial() tags | far batches | doubling rounds | tags / batch | model |")
print("|---|---|---|---|---|---|---|---|")
total = {}
wrong = 0
for c in B.valid_cases():
    if c.family not in families:
        continue
    rc = dec.L.pqg_block_decompress(dec.ctx, abi.CODEC_SNAPPY, c.comp, len(c.comp), dst.ctypes.data, len(dst), C.byref(n))
    assert rc == 0 and dst[:n.value].tobytes() == c.plain, (c.name, rc)
    v = counters()
    model = ""
    if len(c.plain) <= B.K_SUB:
        m = B.trace(c.log, c.hl).counts()
        model = "%d / %d / %d" % m[:3]
        if tuple(v[:3]) != m[:3] or v[5] != m[3]:
            model += " !"
            wrong += 1
    print("| %s | %d | %d | %d | %d | %d | %s | %s |" % (c.name, v[0], v[1], v[2], v[3], v[4],
                                                      "%.1f" % (v[5] / v[0]) if v[0] else "-", model), flush=True)
    t = total.setdefault(c.family, [0] * 6)
    for k in range(6):
        t[k] += v[k]
print()
print("| family | dense batches | sparse windows | serial() tags | far batches | doubling rounds | tags / batch |")
print("|---|---|---|---|---|---|---|")
for f, t in sorted(total.items()):
    print("| %s | %d | %d | %d | %d | %d | %s |" % (f.upper(), t[0], t[1], t[2], t[3], t[4],
                                                  "%.1f" % (t[5] / t[0]) if t[0] else "-"))
print()
print("cases the model disagrees on: %d" % wrong)
dec.close()
