#!/usr/bin/env python3
"""pqg_filter / pqg_select (K9s) on columns a user would filter, against two yardsticks taken in the
same run on the same GPU: the decoder's own copy of the same value bytes (k_values<0>: the values
stage of a PLAIN, uncompressed decode) and the download of the unfiltered column.

  int64    --rows optional rows, 10 % nulls, PLAIN: `v < literal` at about 1 %, 50 % and 100 % of the rows
  strings  the same rows of a C4-shaped string column (65536-word vocabulary, Zipf ranks, 4..32 bytes),
           dictionary encoded: `s < literal` at the same three selectivities, on the materialised
           decode and through the kept dictionary (int32 keys), the latter with the entry bitmap
           staged in LDS and read through L2 (PQG_FILTER_LDS=0)

Per case: pqg_filter and pqg_select device time (pqg_last_filter_ms, best of --steps), the D2H of
the selected column (host clock around the synchronous copies), rows and bytes out.  Writes a
markdown table to --out as well as to stdout.

  python tools/filter_probe.py [--rows N] [--steps K] [--out FILE] [--only int64,strings]"""
import argparse
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "parquet-go_amd")]
import pqgpu  # noqa: E402
from gen import pqwrite as W  # noqa: E402
from pqgpu import abi  # noqa: E402

STAGE_VALUES, STAGE_STRINGS = 8, 9
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def decoder(lds=True):
    old = os.environ.get("PQG_FILTER_LDS")
    if not lds:
        os.environ["PQG_FILTER_LDS"] = "0"
    try:
        d = pqgpu.GpuDecoder(0)
    finally:
        if not lds:
            if old is None:
                os.environ.pop("PQG_FILTER_LDS", None)
            else:
                os.environ["PQG_FILTER_LDS"] = old
    d.L.pqg_set_timing(d.ctx, 1)
    return d


def decode(dec, pf, dev, flags=0, steps=2):
    """The chunk decoded (the last of `steps` decodes) and the best stage timings."""
    job = pqgpu.device_job(pf, 0, 0, dev)
    job.col.flags |= flags
    best = None
    for _ in range(steps + 1):  # the first sizes the arenas
        r = dec.decode_jobs([job])[0]
        assert r.status == 0, abi.status_name(r.status)
        t = dec.timings()
        if best is None or t[STAGE_VALUES] + t[STAGE_STRINGS] < best[STAGE_VALUES] + best[STAGE_STRINGS]:
            best = t
    return r, best


def timed_d2h(dec, parts):
    t0 = time.perf_counter()
    n = 0
    for ptr, nbytes in parts:
        if ptr and nbytes:
            dec.d2h(ptr, nbytes)
            n += nbytes
    return (time.perf_counter() - t0) * 1e3, n


def run_case(dec, label, r, desc, lit, op, steps, dictionary=None):
    rows = r.num_slots
    bm = dec.alloc((rows + 31) // 32 * 4)
    f_ms = []
    for _ in range(steps):
        a = dec.filter_result(bm, r, desc, op, lit, abi.COMBINE_SET, dictionary)
        f_ms.append(dec.last_filter_ms())
    s_ms = []
    sel = None
    for _ in range(steps):
        if sel is not None:
            dec.free_select(sel)
        sel = dec.select(bm, r.def_levels, r.values, r.offsets, rows, r.num_values, r.values_bytes, desc.max_def,
                         r.value_width)
        s_ms.append(dec.last_filter_ms())
    d_ms, d_bytes = timed_d2h(dec, [(sel.out_def_levels, sel.rows_out), (sel.out_values, sel.bytes_out),
                                   (sel.out_offsets, (sel.values_out + 1) * 8 if sel.out_offsets else 0)])
    out = dict(label=label, rows=rows, sel=a.num_selected, filter_ms=min(f_ms), select_ms=min(s_ms), d2h_ms=d_ms,
               d2h_bytes=d_bytes, bytes_out=sel.bytes_out)
    dec.free_select(sel)
    dec.free(bm)
    return out


def table(cases, copy_ms, copy_bytes, full_ms, full_bytes, in_bytes):
    say("| case | rows selected | pqg_filter ms | pqg_select ms | D2H ms (MB) | select / copy | (filter+select+D2H) / unfiltered D2H |")
    say("|---|---|---|---|---|---|---|")
    for c in cases:
        say("| %s | %d (%.1f %%) | %.3f | %.3f | %.2f (%.1f) | %.2f | %.3f |" % (
            c["label"], c["sel"], 100.0 * c["sel"] / max(c["rows"], 1), c["filter_ms"], c["select_ms"], c["d2h_ms"],
            c["d2h_bytes"] / 1e6, c["select_ms"] / copy_ms, (c["filter_ms"] + c["select_ms"] + c["d2h_ms"]) / full_ms))
    say()
    say("k_values<0> copy of the same value bytes: %.3f ms for %.1f MB (%.0f GB/s read + write counted once); "
        "pqg_select reads %.1f MB of levels, bitmap, values and offsets; unfiltered D2H: %.1f ms for %.1f MB (%.1f GB/s)."
        % (copy_ms, copy_bytes / 1e6, copy_bytes / copy_ms / 1e6, in_bytes / 1e6, full_ms, full_bytes / 1e6,
           full_bytes / full_ms / 1e6))
    say()


def plain_copy_ms(dec, nbytes, steps):
    """The values stage of a PLAIN, uncompressed, required INT64 column of nbytes: k_values<0>'s copy."""
    n = max(nbytes // 8, 1)
    col = W.Column("c", W.INT64, W.splitmix64(9, n).view(np.int64))
    pf = pqgpu.ParquetFile(np.frombuffer(W.write_file([col], n), np.uint8))
    dev = dec.upload(pf.data)
    try:
        _, t = decode(dec, pf, dev, steps=steps)
        return t[STAGE_VALUES]
    finally:
        dec.free(dev)


def probe_int64(dec, rows, steps):
    rng = np.random.default_rng(1)
    defs = (rng.random(rows) >= 0.10).astype(np.uint8)
    nn = int(defs.sum())
    vals = W.splitmix64(7, nn).view(np.int64)
    col = W.Column("v", W.INT64, vals, repetition=W.OPTIONAL, def_levels=defs)
    pf = pqgpu.ParquetFile(np.frombuffer(W.write_file([col], rows), np.uint8))
    del vals
    dev = dec.upload(pf.data)
    try:
        r, t = decode(dec, pf, dev, steps=steps)
        desc = pf.columns[0].desc
        copy_ms = t[STAGE_VALUES]
        full_ms, full_bytes = timed_d2h(dec, [(r.def_levels, r.num_slots), (r.values, r.values_bytes)])
        say("## int64: %d optional rows, %d non-null (PLAIN, uncompressed)" % (rows, nn))
        say()
        cases = []
        for label, op, lit in (("v < 1 % quantile", abi.OP_LT, -2 ** 63 + int(0.01 * 2 ** 64)), ("v < 0 (50 %)", abi.OP_LT, 0),
                               ("v <= max (100 %)", abi.OP_LE, 2 ** 63 - 1)):
            cases.append(run_case(dec, label, r, desc, struct.pack("<q", lit), op, steps))
        table(cases, copy_ms, r.values_bytes, full_ms, full_bytes, r.num_slots + r.num_slots // 8 + r.values_bytes)
    finally:
        dec.free(dev)


def string_column(rows, vocab=65536, seed=4):
    """C4's shape (gen.config_c4) with 10 % nulls: the dense values' chars, offsets, def levels, and
    literals at the 1 % and 50 % quantiles of the non-null rows in byte order."""
    rng = np.random.default_rng(seed)
    chars, offs = W.make_vocab(vocab, seed)
    defs = (rng.random(rows) >= 0.10).astype(np.uint8)
    nn = int(defs.sum())
    ranks = np.zeros(0, np.int64)
    while len(ranks) < nn:
        more = rng.zipf(1.1, size=nn)
        ranks = np.concatenate([ranks, more[more <= vocab][: nn - len(ranks)] - 1])
    lens = (offs[1:] - offs[:-1])[ranks]
    out_offs = np.zeros(nn + 1, dtype=np.int64)
    out_offs[1:] = np.cumsum(lens)
    starts = offs[:-1][ranks]
    out_chars = np.empty(int(out_offs[-1]), dtype=np.uint8)
    step = 1 << 21
    for r0 in range(0, nn, step):
        r1 = min(nn, r0 + step)
        c0, c1 = int(out_offs[r0]), int(out_offs[r1])
        idx = np.repeat(starts[r0:r1] - out_offs[r0:r1], lens[r0:r1]) + np.arange(c0, c1, dtype=np.int64)
        out_chars[c0:c1] = chars[idx]
    words = [chars[offs[i]:offs[i + 1]].tobytes() for i in range(vocab)]
    order = sorted(range(vocab), key=lambda i: words[i])
    cum = np.cumsum(np.bincount(ranks, minlength=vocab)[order])
    lits = [words[order[int(np.searchsorted(cum, q * nn))]] for q in (0.01, 0.5)]
    return out_chars, out_offs, defs, lits


def probe_strings(dec, dec_l2, rows, steps):
    chars, offs, defs, lits = string_column(rows)
    col = W.Column("s", W.BYTE_ARRAY, chars, offsets=offs, repetition=W.OPTIONAL, def_levels=defs,
                   encoding=W.RLE_DICTIONARY, dict_limit=1 << 26)
    pf = pqgpu.ParquetFile(np.frombuffer(W.write_file([col], rows), np.uint8))
    nbytes = len(chars)
    del chars, offs
    desc = pf.columns[0].desc
    preds = (("s < 1 % quantile", abi.OP_LT, lits[0]), ("s < median (50 %)", abi.OP_LT, lits[1]), ('s >= "" (100 %)', abi.OP_GE, b""))
    copy_ms = plain_copy_ms(dec, nbytes, steps)
    dev = dec.upload(pf.data)
    try:
        r, t = decode(dec, pf, dev, steps=steps)
        full_ms, full_bytes = timed_d2h(dec, [(r.def_levels, r.num_slots), (r.values, r.values_bytes),
                                              (r.offsets, (r.num_values + 1) * 8)])
        say("## strings, materialised: %d optional rows, %d non-null, %.1f MB of chars (decode: strings stage %.3f ms)"
            % (rows, r.num_values, r.values_bytes / 1e6, t[STAGE_STRINGS]))
        say()
        cases = [run_case(dec, label, r, desc, lit, op, steps) for label, op, lit in preds]
        table(cases, copy_ms, nbytes, full_ms, full_bytes, r.num_slots + r.num_slots // 8 + r.values_bytes + 8 * r.num_values)
        for d, how in ((dec, "entry bitmap staged in LDS"), (dec_l2, "entry bitmap read through L2")):
            dv = dev if d is dec else d.upload(pf.data)
            try:
                r, t = decode(d, pf, dv, flags=abi.COL_KEEP_DICT, steps=steps)
                assert r.col_flags & abi.COL_KEEP_DICT
                dic = abi.Dictionary()
                assert d.L.pqg_get_dictionary(d.ctx, 0, dic) == 0
                full_ms, full_bytes = timed_d2h(d, [(r.def_levels, r.num_slots), (r.values, r.values_bytes)])
                say("## strings, kept dictionary of %d entries (%s): int32 keys" % (dic.count, how))
                say()
                cases = [run_case(d, label, r, desc, lit, op, steps, dictionary=dic) for label, op, lit in preds]
                key_copy = plain_copy_ms(d, r.values_bytes, steps)
                table(cases, key_copy, r.values_bytes, full_ms, full_bytes, r.num_slots + r.num_slots // 8 + r.values_bytes)
            finally:
                if d is not dec:
                    d.free(dv)
    finally:
        dec.free(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default="int64,strings")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dec, dec_l2 = decoder(True), decoder(False)
    try:
        say("# pqg_filter / pqg_select probe: %d rows, best of %d" % (args.rows, args.steps))
        say()
        if "int64" in args.only:
            probe_int64(dec, args.rows, args.steps)
        if "strings" in args.only:
            probe_strings(dec, dec_l2, args.rows, args.steps)
    finally:
        dec.close()
        dec_l2.close()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
