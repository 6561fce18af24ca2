#!/usr/bin/env python3
"""Keep-dictionary decode (PQG_COL_KEEP_DICT, k_dict_idx) against the materialising decode of the
same chunk.  Three files: a C4-shaped string column (gen.config_c4 with a dictionary limit no
chunk reaches, so that every data page is dictionary encoded) and the C2 columns of b = 8 and
b = 20 index bits.  Each is decoded three ways with the runtime's timed stage events, all in one
run on one GPU:

  values    the decode without the flag (k_dict4, or k_str_count -> k_char_scan -> k_str_copy)
  keys      the decode with the flag (k_dict_idx; strings: k_str_dict, k_dict_idx, k_dict_export)
  values-0  the decode without the flag on a context created under PQG_DICT4=0: 4-byte
            dictionary pages go through k_values<1>, hybrid_expand plus a gather, which is what
            k_dict_idx does less the gather (the same as `values` for the string file)

Per way: the values stage, the strings stage, their sum and the whole step in ms, of the step
with the smallest sum among --steps steps after a sizing step; each way is measured --rounds
times.  The keys are checked once per file: dictionary[keys] must be the materialised bytes.

  python tools/dictout_probe.py [--string-rows N] [--c2-rows N] [--steps K] [--rounds R] [--only c4,c2b8,c2b20]

The library under test is the one PQG_LIB names, or the tree's."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "parquet-go_amd")]
import pqgpu  # noqa: E402
from gen import pqwrite as W  # noqa: E402
from pqgpu import abi  # noqa: E402

# pqg_last_timings: the whole step, then scan, list, decompression, setup, walk, levels, nn_scan, values, strings, finalize
STEP, STAGE_VALUES, STAGE_STRINGS = 0, 8, 9


def decoder(dict4):
    old = os.environ.get("PQG_DICT4")
    if not dict4:
        os.environ["PQG_DICT4"] = "0"
    try:
        d = pqgpu.GpuDecoder(0)
    finally:
        if not dict4:
            if old is None:
                os.environ.pop("PQG_DICT4", None)
            else:
                os.environ["PQG_DICT4"] = old
    d.L.pqg_set_timing(d.ctx, 1)
    return d


def measure(dec, job, steps):
    best, r = None, None
    for _ in range(steps + 1):  # the first step sizes the arenas
        r = dec.decode_jobs([job])[0]
        assert r.status == 0, abi.status_name(r.status)
        t = dec.timings()
        if best is None or t[STAGE_VALUES] + t[STAGE_STRINGS] < best[STAGE_VALUES] + best[STAGE_STRINGS]:
            best = t
    return best, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--string-rows", type=int, default=4_000_000)
    ap.add_argument("--c2-rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", default="c4,c2b8,c2b20")
    args = ap.parse_args()
    makers = {
        "c4": lambda: W.config_c4(rows=args.string_rows, dict_limit=1 << 26)[0],
        "c2b8": lambda: W.config_c2(rows=args.c2_rows, bits=8)[0],
        "c2b20": lambda: W.config_c2(rows=args.c2_rows, bits=20)[0],
    }
    dec, dec0 = decoder(True), decoder(False)
    try:
        for name in args.only.split(","):
            data = makers[name]()
            pf = pqgpu.ParquetFile(data)
            ways = []
            for d, way, flag in ((dec, "values", 0), (dec, "keys", abi.COL_KEEP_DICT), (dec0, "values-0", 0)):
                dev = d.upload(pf.data)
                job = pqgpu.device_job(pf, 0, 0, dev)
                job.col.flags |= flag
                ways.append((d, way, job, dev))
            # dictionary[keys] against the materialised decode, once
            d, _, job, _ = ways[0]
            r = d.decode_jobs([job])[0]
            assert r.status == 0, abi.status_name(r.status)
            plain = d.download(r, 0)
            d, _, job, _ = ways[1]
            r = d.decode_jobs([job])[0]
            assert r.status == 0, abi.status_name(r.status)
            kept = d.download(r, 0)
            m = kept.materialize()
            assert kept.dictionary is not None and m.values.tobytes() == plain.values.tobytes(), name
            assert (plain.offsets is None) == (m.offsets is None) and (m.offsets is None or
                                                                     np.array_equal(m.offsets, plain.offsets)), name
            print("%s: file %.1f MB, %d pages, %d values, dictionary of %d entries; keys verified" % (
                name, len(data) / 1e6, len(plain.pages), plain.num_values, kept.dictionary.count), flush=True)
            del plain, kept, m
            for rnd in range(args.rounds):
                for d, way, job, _ in ways:
                    t, _ = measure(d, job, args.steps)
                    print("%-6s %-8s round %d  values %7.3f ms  strings %7.3f ms  values+strings %7.3f ms  step %8.3f ms"
                          % (name, way, rnd, t[STAGE_VALUES], t[STAGE_STRINGS], t[STAGE_VALUES] + t[STAGE_STRINGS],
                             t[STEP]), flush=True)
            for d, _, _, dev in ways:
                d.free(dev)
    finally:
        dec.close()
        dec0.close()


if __name__ == "__main__":
    main()
