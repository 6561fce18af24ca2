"""The nested export's model (tests/nested_model.py) and the schema-derived
thresholds (pqgpu.nested.leaf_thresholds), without a GPU.

The model is pinned from three sides: the reference's own Dremel vectors
(data_store_test.go, tests/golden/dremel.json and rows.json), pyarrow's array
layout of random nested rows, and files pyarrow (and the synthetic writer)
wrote, decoded by the CPU oracle."""
import io
import json
import os

import numpy as np
import pytest

import nested_model as M
from pqgpu import nested as N

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROWS = json.load(open(os.path.join(GOLD, "rows.json")))


class _N:
    def __init__(self, d):
        self.__dict__.update(d)


def test_model_twitter_blog():
    g = json.load(open(os.path.join(GOLD, "dremel.json")))
    vals = np.array(g["values"], np.int32)
    m = M.assemble(g["def_levels"], g["rep_levels"], g["max_def"], [0, 1], [1, 2], vals, 4)
    assert M.column(m, np.int32).to_pylist() == g["rows"]
    assert m.levels[0][0].tolist() == [0, 2, 4] and m.levels[1][0].tolist() == [0, 3, 7, 8, 10]
    assert (m.num_rows, m.num_leaf, m.num_valid) == (2, 10, 10)
    assert [l[2] for l in m.levels] == [0, 0]


def _nesting(obj, path):
    """What a row holds along `path` (schema nodes): a list per REPEATED node,
    None below a missing OPTIONAL node, the leaf's value at the end.  A
    REPEATED field with no key is an empty list (the reference drops it)."""
    if not path:
        return obj
    n, rest = path[0], path[1:]
    if n.repetition == N.REPEATED:
        if obj is None:
            return None
        return [_nesting(e, rest) for e in obj.get(n.name, [])]
    if obj is None:
        return _nesting(None, rest)
    return _nesting(obj.get(n.name), rest)


_ROW_LEAVES = [(case, lf) for case in ROWS for lf in range(len(case["leaves"]))
               if [n for n in case["nodes"] if n["leaf"] == lf][0]["max_rep"] >= 1]


@pytest.mark.parametrize("case,lf", _ROW_LEAVES, ids=lambda x: x["source"].split()[-1] if isinstance(x, dict) else str(x))
def test_model_reference_row_vectors(case, lf):
    nodes = [_N(n) for n in case["nodes"]]
    path = N.leaf_path(nodes, lf)
    list_def, elem_def = N.leaf_thresholds(nodes, lf)
    assert len(elem_def) == path[-1].max_rep
    c = case["leaves"][lf]
    m = M.assemble(c["def"], c["rep"], path[-1].max_def, list_def, elem_def, np.array(c["values"], np.int64), 8)
    assert m.num_valid == len(c["values"])
    assert M.column(m, np.int64).to_pylist() == [_nesting(r, path) for r in case["rows"]]


def test_thresholds_of_reference_schemas():
    by = {c["source"].split()[-1]: [_N(n) for n in c["nodes"]] for c in ROWS}
    assert N.leaf_thresholds(by["TestOneColumn"], 0) == ([], [])
    assert N.leaf_thresholds(by["TestOneColumnOptional"], 0) == ([], [])
    assert N.leaf_thresholds(by["TestOneColumnRepeated"], 0) == ([0], [1])       # a bare repeated leaf
    assert N.leaf_thresholds(by["TestTwitterBlog"], 0) == ([0, 1], [1, 2])
    assert N.leaf_thresholds(by["TestComplex"], 4) == ([0, 1], [1, 2])           # Name.Language.Country
    assert N.leaf_thresholds(by["TestComplex"], 1) == ([1], [2])                 # optional Links, repeated Backward
    assert N.leaf_thresholds(by["TestEmptyParent"], 0) == ([1], [2])


# ---------------------------------------------------------------- pyarrow's layout

@pytest.mark.parametrize("K,typ", [(2, "int32"), (3, "float64")])
def test_model_equals_pyarrow_layout(K, typ):
    pa = pytest.importorskip("pyarrow")
    rng = np.random.default_rng(K)
    dt = np.dtype(typ)
    value = (lambda: int(rng.integers(-1000, 1000))) if typ == "int32" else (lambda: float(rng.standard_normal()))
    rows = M.random_rows(rng, 3000 if K == 2 else 1500, K, value)
    t = pa.int32() if typ == "int32" else pa.float64()
    for _ in range(K):
        t = pa.list_(t)
    arr = pa.array(rows, t)
    list_def, elem_def, max_def = M.pyarrow_thresholds(K)
    defs, reps, vals = M.shred(rows, list_def, elem_def, max_def)
    # nulls and empties at every depth, and null leaves
    for k in range(K):
        assert (defs == list_def[k] - 1).any() and (defs == list_def[k]).any()
    assert (defs == max_def - 1).any()
    m = M.assemble(defs, reps, max_def, list_def, elem_def, np.array(vals, dt), dt.itemsize)
    exp_levels, exp_leaf_valid, exp_leaf = M.arrow_layout(arr, K)
    assert m.num_rows == len(rows)
    for (offs, bits, nulls, entries), (eo, ev) in zip(m.levels, exp_levels):
        assert np.array_equal(offs, eo)
        assert entries == len(ev) and nulls == int((~ev).sum())
        assert np.array_equal(N._bits(bits, entries), ev)
    assert m.num_leaf == len(exp_leaf) and m.num_valid == int(exp_leaf_valid.sum())
    assert np.array_equal(N._bits(m.leaf_validity, m.num_leaf), exp_leaf_valid)
    exp_vals = np.asarray(exp_leaf.fill_null(0)).astype(dt)
    assert np.array_equal(m.leaf_values.view(dt).view(np.uint8), exp_vals.view(np.uint8))
    assert M.column(m, dt).to_pylist() == rows


# ---------------------------------------------------------------- thresholds against files

def _oracle_column(pf, path):
    """Decode `path` of row group 0 on the CPU, run the model with the
    schema-derived thresholds, and hand back the NestedColumn."""
    from oracle import pyoracle as O
    c = pf.column_index(path)
    ch = O.decode_chunk(pf.host_job(0, c)[0])
    assert ch.status == 0
    desc = pf.columns[c].desc
    list_def, elem_def = N.leaf_thresholds(pf.schema_nodes, c)
    assert len(elem_def) == desc.max_rep
    m = M.assemble(ch.def_levels, ch.rep_levels, desc.max_def, list_def, elem_def,
                   ch.values if ch.offsets is None else None, ch.value_width if ch.offsets is None else 0,
                   ch.offsets, num_slots=ch.num_slots)
    dt = {1: np.int32, 2: np.int64, 4: np.float32, 5: np.float64}.get(desc.physical_type)
    return M.column(m, dt, chars=ch.values), (list_def, elem_def)


def test_thresholds_agree_with_pyarrow_files():
    pa = pytest.importorskip("pyarrow")
    pq = pytest.importorskip("pyarrow.parquet")
    import pqgpu
    rng = np.random.default_rng(11)
    n = 400
    ll = M.random_rows(rng, n, 2, lambda: int(rng.integers(0, 99)))
    ls = M.random_rows(rng, n, 1, lambda: "s%d" % rng.integers(0, 50))
    st = [None if rng.random() < 0.2 else {"l": x} for x in M.random_rows(rng, n, 1, lambda: int(rng.integers(0, 9)))]
    t = pa.table({"ll": pa.array(ll, pa.list_(pa.list_(pa.int32()))),
                  "ls": pa.array(ls, pa.list_(pa.string())),
                  "st": pa.array(st, pa.struct([("l", pa.list_(pa.int32()))]))})
    buf = io.BytesIO()
    pq.write_table(t, buf, compression="snappy")
    pf = pqgpu.ParquetFile(buf.getvalue())
    back = pq.read_table(io.BytesIO(buf.getvalue()))
    col, thr = _oracle_column(pf, "ll.list.element.list.element")
    assert thr == ([1, 3], [2, 4])
    assert col.to_pylist() == back.column("ll").to_pylist() == ll
    col, thr = _oracle_column(pf, "ls.list.element")
    assert thr == ([1], [2])
    assert col.to_pylist() == [None if r is None else [None if s is None else s.encode() for s in r] for r in ls]
    col, thr = _oracle_column(pf, "st.l.list.element")
    assert thr == ([2], [3])   # null struct (0) and null list (1) both below list_def
    assert col.to_pylist() == [None if r is None else r["l"] for r in back.column("st").to_pylist()]


def test_thresholds_agree_with_pyarrow_on_synthetic_list():
    """The synthetic writer's LIST column (its 3-level optional list of
    optional doubles), read by pyarrow."""
    pytest.importorskip("pyarrow")
    pq = pytest.importorskip("pyarrow.parquet")
    import pqgpu
    from gen import pqwrite as W
    data, _ = W.config_c5(row_groups=(0,), rows_per_rg=600, rows_per_page=250)
    pf = pqgpu.ParquetFile(data)
    col, thr = _oracle_column(pf, "lst.list.element")
    assert thr == ([1], [2])
    assert col.to_pylist() == pq.read_table(io.BytesIO(data)).column("lst").to_pylist()
