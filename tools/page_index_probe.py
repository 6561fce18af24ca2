"""Located against scanned decode, and selective reads over the page index, on one GPU.

    python tools/page_index_probe.py [--repeats 12] [--rows 100000000] [--select-rows 50000000]
        [--parent-lib LIB] [--out FILE]

1. Scan stage.  Each shape's chunks are uploaded once; the page locations come from the page table of a
   first scanned decode (no index-writing generator is needed).  The scanned and the located decode of the
   same resident chunks then alternate, `repeats` times each after two warm-up rounds, and the scan stage
   (pqg_last_timings stage 0: ev[0]..ev[1]) and the whole pipeline are reported as median and min..max.
2. Selective read.  A file with a sorted int64 column and a dictionary string column, written by pyarrow
   with the page index; predicates on the sorted column keep about 1 %, 10 % and 100 % of the pages.  With
   With and without use_page_index, alternating: bytes uploaded, pages decoded / total, the device time
   of decode + trim + filter + select, and the wall time of read_row_group beside it.
3. With --parent-lib: bench.py's headline on the parent commit's library and on this tree's, alternating.
Prints markdown."""
import argparse
import io
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "parquet-go_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pqgpu  # noqa: E402
from gen import pqwrite as W  # noqa: E402


def spread(xs):
    return "%.3f (%.3f..%.3f)" % (statistics.median(xs), min(xs), max(xs))


def scan_stage(dec, name, data, repeats, out):
    pf = pqgpu.ParquetFile(data)
    dev = dec.upload(pf.data)
    try:
        jobs = [pqgpu.device_job(pf, rg, c, dev) for rg in range(pf.num_row_groups) for c in range(pf.num_columns)]
        res = dec.decode_jobs(jobs)
        assert all(r.status == 0 for r in res), [r.status for r in res]
        lists = []
        for i in range(len(jobs)):
            pages = dec.pages(i, 1 << 16)
            lists.append([(p.header_offset, p.payload_offset - p.header_offset + p.compressed_size) for p in pages])
        t = {"scanned": ([], []), "located": ([], [])}
        for k in range(repeats + 2):
            for kind in ("scanned", "located"):
                if kind == "scanned":
                    dec.decode_jobs(jobs)
                else:
                    r = dec.decode_located(jobs, lists)
                    assert all(x.status == 0 for x in r)
                tm = dec.timings()
                if k >= 2:
                    t[kind][0].append(tm[1])
                    t[kind][1].append(tm[0])
        npages = sum(len(x) for x in lists)
        out.append("| %s | %d | %d | %s | %s | %s | %s |" % (
            name, len(jobs), npages, spread(t["scanned"][0]), spread(t["located"][0]), spread(t["scanned"][1]),
            spread(t["located"][1])))
    finally:
        dec.free(dev)


class TimedDecoder(pqgpu.GpuDecoder):
    """A decoder that adds up the device time of what a reader runs on it: every decode's pipeline
    (pqg_last_timings, all stages) and every pqg_filter / pqg_select / pqg_range_bitmap call
    (pqg_last_filter_ms)."""
    device_ms = 0.0

    def decode_jobs(self, jobs):
        r = super().decode_jobs(jobs)
        self.device_ms += (self.timings() or [0.0])[0]
        return r

    def decode_located(self, jobs, locations):
        r = super().decode_located(jobs, locations)
        self.device_ms += (self.timings() or [0.0])[0]
        return r

    def filter(self, *a, **kw):
        r = super().filter(*a, **kw)
        self.device_ms += self.last_filter_ms()
        return r

    def select(self, *a, **kw):
        r = super().select(*a, **kw)
        self.device_ms += self.last_filter_ms()
        return r

    def range_bitmap(self, *a, **kw):
        r = super().range_bitmap(*a, **kw)
        self.device_ms += self.last_filter_ms()
        return r


def selective(dec, rows, repeats, out):
    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(3)
    a = np.arange(rows, dtype=np.int64)
    words = pa.array(["word%05d" % i for i in range(5000)])
    s = pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, 5000, rows).astype(np.int32)), words)
    buf = io.BytesIO()
    pq.write_table(pa.table({"a": pa.array(a), "s": s}), buf, compression="SNAPPY", write_page_index=True,
                   row_group_size=rows)
    data = np.frombuffer(buf.getvalue(), np.uint8)
    for frac in (0.01, 0.10, 1.0):
        hi = int(rows * frac)
        f = [("a", ">=", 0), ("a", "<", hi)]
        dev_ms, wall_ms, last = {False: [], True: []}, {False: [], True: []}, {}
        for k in range(repeats + 1):  # round 0 warms up; the two variants alternate
            for use in (False, True):
                fr = pqgpu.FileReader(data, "a", "s", decoder=dec, use_page_index=use, read_dictionary=("s",))
                dec.device_ms = 0.0
                t0 = time.perf_counter()
                cols = fr.read_row_group(0, filters=f)
                wall = (time.perf_counter() - t0) * 1e3
                assert cols["a"].num_slots == hi
                if k:
                    dev_ms[use].append(dec.device_ms)
                    wall_ms[use].append(wall)
                last[use] = fr
        for use in (False, True):
            fr = last[use]
            lr = fr.last_read
            out.append("| %d %% | %s | %.1f | %d / %d | %s | %s |" % (
                round(frac * 100), "index" if use else "scan", fr.uploaded_bytes / 1e6, lr.get("pages_decoded", 0),
                lr.get("pages_total", 0), spread(dev_ms[use]), spread(wall_ms[use])))


def headline(parent_lib, repeats, out):
    """bench.py's headline, this tree's library and the parent commit's (a libpqgpu.so built from it, named
    by PQG_LIB) alternating, one process each."""
    import json
    import subprocess
    ms = {"this tree": [], "parent": []}
    for k in range(repeats):
        for who in ("this tree", "parent"):
            env = dict(os.environ)
            if who == "parent":
                env["PQG_LIB"] = parent_lib
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup",
                                "5"], env=env, capture_output=True, text=True, check=True)
            line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
            ms[who].append(json.loads(line)["ms_per_step"])
    out += ["", "## The default path: bench.py headline (C2, no located job), ms per step", "",
            "%d alternating runs each, median (min..max)." % repeats, "", "| library | ms per step |", "|---|---|"]
    for who in ms:
        out.append("| %s | %s |" % (who, spread(ms[who])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--select-rows", type=int, default=50_000_000)
    ap.add_argument("--parent-lib", default=None, help="libpqgpu.so built from the parent commit: adds step 3")
    ap.add_argument("--headline-runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dec = TimedDecoder(0)
    out = ["## Scan stage: scanned against located, same build, same resident chunks", "",
           "ms, median (min..max) of %d alternating repeats after 2 warm-up rounds." % a.repeats, "",
           "| shape | chunks | pages | scan stage, scanned | scan stage, located | pipeline, scanned | pipeline, located |",
           "|---|---|---|---|---|---|---|"]
    shapes = [("C2 b=8, %d rows" % a.rows, lambda: W.config_c2(rows=a.rows, bits=8)[0]),
              ("C2 b=20, %d rows" % a.rows, lambda: W.config_c2(rows=a.rows, bits=20)[0]),
              ("C2 run-heavy b=8, %d rows" % a.rows, lambda: W.config_c2(rows=a.rows, bits=8, run_heavy=True)[0]),
              ("C3 snappy, %d rows" % a.rows, lambda: W.config_c3(rows=a.rows)[0])]
    for name, make in shapes:
        scan_stage(dec, name, make(), a.repeats, out)
    out += ["", "## Selective read: %d rows, sorted int64 `a` + dictionary strings `s`, snappy" % a.select_rows, "",
            "Predicate `0 <= a < k`, the two paths alternating, %d repeats each after one warm-up round.  Device ms:"
            % a.repeats,
            "the decode pipeline (pqg_last_timings) plus every pqg_range_bitmap / pqg_filter / pqg_select call",
            "(pqg_last_filter_ms).  Wall ms: read_row_group as a whole (index fetch, packing, upload, download).",
            "Median (min..max).", "",
            "| pages kept | path | MB uploaded | pages decoded / total | device ms | wall ms |", "|---|---|---|---|---|---|"]
    selective(dec, a.select_rows, a.repeats, out)
    dec.close()
    if a.parent_lib:
        headline(a.parent_lib, a.headline_runs, out)
    text = "\n".join(out) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
