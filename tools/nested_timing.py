#!/usr/bin/env python3
"""Device time of the K8 list exports on the C5 `lst` shape.

One row group of gen.pqwrite.c5_row_group_columns' LIST<double> (the same
draws, without the other eight columns): pqg_assemble_list against
pqg_assemble_nested at depth 1 (the two taken in turn), then depth 2 on a
list<list<double>> of the same slot count.  Every output is requested.
Prints mean and range of pqg_last_assemble_ms over --calls calls after
--warmup, and the bytes moved.

    python tools/nested_timing.py [--rows 15625000] [--calls 10] [--warmup 2]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "parquet-go_amd")]


def c5_lst(rows, rg=0, seed=5):
    """The `lst` arrays of c5_row_group_columns(rg, rows): its first draws."""
    rng = np.random.default_rng([seed, rg])
    null_list = rng.random(rows) < 0.05
    lens = rng.integers(0, 4, size=rows)
    lens[null_list] = 0
    per_row = np.where(lens == 0, 1, lens)
    starts = np.zeros(rows + 1, np.int64)
    starts[1:] = np.cumsum(per_row)
    slots = int(starts[-1])
    rep = np.ones(slots, np.uint8)
    rep[starts[:-1]] = 0
    row_of = np.repeat(np.arange(rows), per_row)
    defs = np.full(slots, 3, np.uint8)
    defs[rng.random(slots) < 0.05] = 2
    defs[(lens == 0)[row_of]] = 1
    defs[null_list[row_of]] = 0
    return defs, rep, rng.standard_normal(int((defs == 3).sum()))


def depth2(defs1, rep1, n, seed=6):
    """A list<list<double>> shredding of n slots (pyarrow's levels: list_def
    1, 3; elem_def 2, 4; max_def 5): the depth-1 stream's rows become inner
    lists, and a random 40% of them start a new outer row; 3% of the rows are
    null or empty outer lists instead."""
    rng = np.random.default_rng(seed)
    defs = defs1[:n].astype(np.uint8) + 2      # 2 null inner, 3 empty inner, 4 null leaf, 5 value
    rep = rep1[:n].astype(np.uint8) + 1        # 1 starts an inner list, 2 continues it
    starts = np.flatnonzero(rep == 1)
    outer = starts[rng.random(len(starts)) < 0.4]
    rep[outer] = 0
    rep[0] = 0
    solo = outer[(rng.random(len(outer)) < 0.03) & (np.r_[rep[outer[:-1] + 1], 0] < 2)]
    defs[solo] = rng.integers(0, 2, size=len(solo))  # a one-slot row: null (0) or empty (1) outer list
    # the slot after a one-slot row must start a row of its own
    nxt = solo + 1
    rep[nxt[nxt < n]] = 0
    return defs, rep, rng.standard_normal(int((defs == 5).sum()))


def stats(ms):
    return dict(mean_ms=round(float(np.mean(ms)), 4), min_ms=round(float(np.min(ms)), 4),
                max_ms=round(float(np.max(ms)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=15_625_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import pqgpu
    dec = pqgpu.GpuDecoder(0)
    defs, rep, vals = c5_lst(a.rows)
    n = len(defs)

    def timed(*calls):
        """Device ms of each call, the calls taken in turn so that they share
        whatever else the machine is doing."""
        ms = [[] for _ in calls]
        for i in range(a.warmup + a.calls):
            for k, call in enumerate(calls):
                free = call()
                if i >= a.warmup:
                    ms[k].append(dec.last_assemble_ms())
                free()
        return ms

    def traffic(n, entries, leaf, valid, passes=2):
        """Bytes in (both level streams in both passes, the dense values) and
        out (per depth offsets + bitmap, leaf bitmap + values)."""
        rd = passes * 2 * n + 8 * valid
        wr = sum(4 * (e + 1) + (e + 7) // 8 for e in entries) + (leaf + 7) // 8 + 8 * leaf
        return rd, wr

    out = {"slots": n, "rows": a.rows, "calls": a.calls, "warmup": a.warmup}
    dp, rp, vp = dec.upload(defs), dec.upload(rep), dec.upload(vals.view(np.uint8))

    def run_list():
        r = dec.assemble_list(dp, rp, vp, n, 3, 1, 2, 8)
        run_list.counts = (r[0].num_rows, r[0].num_elements, r[0].num_valid)
        return lambda: [dec.free(p) for p in r[1:]]

    def run_nested(d, r_, v, md, ld, ed):
        def call():
            x = dec.assemble_nested(d, r_, v, n, md, ld, ed, value_width=8)
            call.args = x
            return lambda: dec.free_nested(x)
        return call

    ms_list, ms = timed(run_list, run_nested(dp, rp, vp, 3, [1], [2]))
    rows, el, valid = run_list.counts
    rd, wr = traffic(n, [rows], el, valid)
    out["assemble_list"] = dict(stats(ms_list), bytes_in=rd, bytes_out=wr,
                                tb_per_s=round((rd + wr) / np.mean(ms_list) / 1e9, 3))
    out["assemble_nested_depth1"] = dict(stats(ms), bytes_in=rd, bytes_out=wr,
                                         tb_per_s=round((rd + wr) / np.mean(ms) / 1e9, 3))
    for p in (dp, rp, vp):
        dec.free(p)

    d2, r2, v2 = depth2(defs, rep, n)
    dp, rp, vp = dec.upload(d2), dec.upload(r2), dec.upload(v2.view(np.uint8))
    call = run_nested(dp, rp, vp, 5, [1, 3], [2, 4])
    ms, = timed(call)
    x = call.args
    rd, wr = traffic(n, [x.level[0].num_entries, x.level[1].num_entries], x.num_leaf, x.num_valid)
    out["assemble_nested_depth2"] = dict(stats(ms), bytes_in=rd, bytes_out=wr,
                                         tb_per_s=round((rd + wr) / np.mean(ms) / 1e9, 3),
                                         rows=int(x.num_rows), inner_lists=int(x.level[1].num_entries),
                                         leaf=int(x.num_leaf))
    dec.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
