"""50 M-slot depth-2 level streams: pqg_assemble_structs (1, 4, 8 structs) and pqg_assemble_nested,
device time by pqg_last_assemble_ms (5 calls each, the first of all includes the kernels' load).
Prints one JSON object (profiles/r17_struct_probe.md holds a recorded run)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "parquet-go_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import pqgpu
import struct_model as S
from pqgpu import tree as T
from pqgpu.nested import leaf_thresholds

O, P = S.OPT, S.REP
# s0 t0 u0 { l1: list<s1 t1 u1 { l2: list<s2 t2 { v }> }> }: 8 optional structs, 3 + 3 + 2 a depth
f = ("s2", O, S.PLAIN, [("t2", O, S.PLAIN, [("v", O)])])
f = ("l2", O, S.LIST, [("list", P, S.PLAIN, [f])])
f = ("s1", O, S.PLAIN, [("t1", O, S.PLAIN, [("u1", O, S.PLAIN, [f])])])
f = ("l1", O, S.LIST, [("list", P, S.PLAIN, [f])])
f = ("s0", O, S.PLAIN, [("t0", O, S.PLAIN, [("u0", O, S.PLAIN, [f])])])
nodes, kinds = S.schema([f])
root = T.plan(nodes, kinds)
structs = [(n.depth, n.struct_def) for n in T.walk(root) if n.kind == "struct" and n.nullable]
assert len(structs) == 8
list_def, elem_def = leaf_thresholds(nodes, 0)
max_def = nodes[-1].max_def
rng = np.random.default_rng(1)
d, r, _ = S.shred(root, S.random_rows(root, rng, 20000, max_len=4))[0]
N = 50_000_000
times = N // len(d) + 1
defs, reps = np.tile(d, times)[:N], np.tile(r, times)[:N]
nvalid = int((defs == max_def).sum())
dec = pqgpu.GpuDecoder(0)
dp, rp = dec.upload(defs), dec.upload(reps)
vp = dec.upload(np.zeros(nvalid * 4, np.uint8))
out = {"slots": N, "max_def": max_def, "elem_def": elem_def, "list_def": list_def, "valid": nvalid, "runs": {}}


def best(run, reps_=5):
    ms = []
    for _ in range(reps_):
        run()
        ms.append(dec.last_assemble_ms())
    return {"ms_min": min(ms), "ms_median": sorted(ms)[len(ms) // 2], "ms_all": ms}


for ns, pick in ((1, [0]), (4, [0, 3, 4, 6]), (8, list(range(8)))):
    info = {}

    def run():
        a = dec.assemble_structs(dp, rp, N, max_def, elem_def, [structs[j] for j in pick])
        info["entries"] = [int(a.st[j].num_entries) for j in range(ns)]
        info["nulls"] = [int(a.st[j].null_count) for j in range(ns)]
        dec.free_structs(a)

    res = best(run)
    res.update(info)
    out["runs"]["structs_%d" % ns] = res
    res = {}

    def run_count():
        a = dec.assemble_structs(dp, rp, N, max_def, elem_def, [structs[j] for j in pick], validity=False)
        dec.free_structs(a)

    out["runs"]["structs_%d_count_only" % ns] = best(run_count)

info = {}


def run_nested():
    a = dec.assemble_nested(dp, rp, vp, N, max_def, list_def, elem_def, value_width=4)
    info.update(rows=int(a.num_rows), leaf=int(a.num_leaf), entries=[int(a.level[k].num_entries) for k in range(2)])
    dec.free_nested(a)


res = best(run_nested)
res.update(info)
out["runs"]["nested"] = res
dec.close()
print(json.dumps(out))
