"""The struct export's model (tests/struct_model.py) and the schema-derived
column tree (pqgpu.tree.plan / build), without a GPU.

The model is pinned against pyarrow: files pyarrow wrote are decoded by the CPU
oracle, the model's struct bitmaps must equal pyarrow's own validity wherever
the ancestors are valid, and the whole tree must give pyarrow's rows.  A legacy
2-level list, which pyarrow does not write, is written by hand."""
import io

import numpy as np
import pytest

import struct_model as S
import struct_tables as ST
import pqgpu
from pqgpu import abi
from pqgpu import tree as T
from pqgpu.nested import _bits, leaf_thresholds

N_ROWS = 400


@pytest.fixture(scope="module")
def pa_file():
    """(rows, table, ParquetFile, pyarrow's read of the file) of the shared nested table."""
    pytest.importorskip("pyarrow")
    pq = pytest.importorskip("pyarrow.parquet")
    rows = ST.rows(N_ROWS)
    t = ST.table(rows)
    data = ST.file_bytes(t, compression="snappy")
    return rows, t, pqgpu.ParquetFile(data), pq.read_table(io.BytesIO(data))


def check_validity(node, arr, mask):
    """node's struct bitmaps against the pyarrow array `arr`, at the slots whose ancestors are
    all valid (mask); returns how many struct slots were compared."""
    seen = 0
    if isinstance(node, T.StructNode):
        assert node.length == len(arr)
        valid = np.asarray(arr.is_valid())
        if node.validity is not None:
            got = _bits(node.validity, node.length)
            assert np.array_equal(got[mask], valid[mask]), node.name
            assert not _bits(node.validity, len(node.validity) * 32)[node.length:].any()
            seen += int(mask.sum())
            if mask.all():
                assert node.null_count == arr.null_count
        else:
            assert arr.null_count == 0
        for i, c in enumerate(node.children):
            seen += check_validity(c, arr.field(i), mask & valid)
    elif isinstance(node, T.ListNode):
        assert node.length == len(arr)
        valid = np.asarray(arr.is_valid()) & mask
        o = np.asarray(arr.offsets).astype(np.int64)
        assert o[0] == 0
        child = arr.values
        if node.is_map:  # pyarrow: keys and items side by side; here: one struct of both
            import pyarrow as pa
            child = pa.StructArray.from_arrays([arr.keys, arr.items], [c.name for c in node.child.children])
        seen += check_validity(node.child, child, np.repeat(valid, np.diff(o)))
    return seen


def test_tree_and_struct_bitmaps_equal_pyarrow(pa_file):
    rows, t, pf, back = pa_file
    root = T.plan(pf.schema_nodes, pf.schema_kinds)
    tree = S.host_tree(root, pf.schema_nodes, S.oracle_leaves(pf, 0), pf.row_group_rows(0))
    assert tree.length == N_ROWS and tree.validity is None
    assert tree.to_pylist() == S.encode(back.to_pylist()) == S.encode(rows)
    seen = 0
    for i, c in enumerate(tree.children):
        seen += check_validity(c, back.column(i).combine_chunks(), np.ones(N_ROWS, bool))
    assert seen > 3 * N_ROWS  # s, o, o.i, sl and the structs inside ls


def test_tree_to_arrow_equals_pyarrow(pa_file):
    _, _, pf, back = pa_file
    root = T.plan(pf.schema_nodes, pf.schema_kinds)
    arr = S.host_tree(root, pf.schema_nodes, S.oracle_leaves(pf, 0), pf.row_group_rows(0)).to_arrow()
    arr.validate(full=True)
    for i, name in enumerate(back.column_names):
        assert arr.type.field(i).name == name
        assert arr.field(i).equals(back.column(i).combine_chunks()), name


def test_shred_gives_the_levels_pyarrow_wrote(pa_file):
    rows, _, pf, _ = pa_file
    root = T.plan(pf.schema_nodes, pf.schema_kinds)
    mine, theirs = S.shred(root, rows), S.oracle_leaves(pf, 0)
    assert sorted(mine) == sorted(theirs)
    for lf, (d, r, _) in mine.items():
        assert np.array_equal(d, theirs[lf]["defs"]), lf
        if theirs[lf]["reps"] is not None:
            assert np.array_equal(r, theirs[lf]["reps"]), lf
        else:
            assert not r.any()


def test_same_bits_from_every_leaf_below_a_struct(pa_file):
    rows, _, pf, _ = pa_file
    root = T.plan(pf.schema_nodes, pf.schema_kinds)
    lv = S.shred(root, rows)
    structs = [n for n in T.walk(root) if n.kind == "struct" and n.nullable]
    assert len(structs) >= 5
    for st in structs:
        below = [n.leaf for n in T.walk(st) if n.kind == "leaf"]
        got = []
        for lf in below:
            ed = leaf_thresholds(pf.schema_nodes, lf)[1]
            w, nulls, entries = S.struct_bits(lv[lf][0], lv[lf][1], st.depth, st.struct_def, ed)
            got.append((w.tolist(), nulls, entries))
        assert all(g == got[0] for g in got), st.name
        assert 0 < got[0][1] < got[0][2]
    assert any(len([n for n in T.walk(st) if n.kind == "leaf"]) > 1 for st in structs)


def test_plan_shapes_of_a_pyarrow_file(pa_file):
    _, _, pf, _ = pa_file
    by_name = {n.name.decode(): k for n, k in zip(pf.schema_nodes, pf.schema_kinds)}
    assert by_name["ls"] == by_name["l"] == abi.NODE_LIST and by_name["m"] == abi.NODE_MAP
    assert by_name["s"] == by_name["o"] == by_name["key_value"] == by_name["list"] == by_name["a"] == abi.NODE_PLAIN
    assert len(pf.schema_kinds) == len(pf.schema_nodes)
    ab = [("leaf", "a", True), ("leaf", "b", True)]
    assert T.plan(pf.schema_nodes, pf.schema_kinds).shape() == ("struct", "", False, [
        ("struct", "s", True, ab),
        ("struct", "o", True, [("struct", "i", True, [("leaf", "x", True), ("leaf", "y", True)]), ("leaf", "z", True)]),
        ("list", "ls", True, ("struct", "element", True, ab)),
        ("struct", "sl", True, [("list", "l", True, ("leaf", "element", True))]),
        ("map", "m", True, ("struct", "key_value", False, [("leaf", "key", False), ("leaf", "value", True)])),
        ("struct", "r", False, [("leaf", "p", False), ("leaf", "q", True)]),
    ])
    root = T.plan(pf.schema_nodes, pf.schema_kinds)
    node = {n.name: n for n in T.walk(root) if n.kind != "leaf"}
    assert (node["s"].depth, node["s"].struct_def) == (0, 1)
    assert (node["i"].depth, node["i"].struct_def) == (0, 2)
    assert (node["element"].depth, node["element"].struct_def) == (1, 3)   # list 1, elements 2, the struct 3
    assert (node["ls"].depth, node["ls"].elem_def) == (1, 2)
    assert (node["l"].depth, node["l"].elem_def) == (1, 3)
    assert node["ls"].rep_leaf == pf.column_index("ls.list.element.a")
    # projection: only s.b keeps s and drops s.a and every other field
    only = T.plan(pf.schema_nodes, pf.schema_kinds, [pf.column_index("s.b")])
    assert only.shape() == ("struct", "", False, [("struct", "s", True, [("leaf", "b", True)])])
    assert T.structs_by_leaf(only) == {pf.column_index("s.b"): [only.children[0]]}


def test_plan_backward_compatibility_rules():
    R, O, P = S.REQ, S.OPT, S.REP
    nodes, kinds = S.schema([
        ("two", O, S.LIST, [("array", P)]),                                           # repeated leaf: the element
        ("tup", O, S.LIST, [("tup_tuple", P, S.PLAIN, [("v", O)])]),                  # <parent>_tuple: a struct element
        ("arr", R, S.LIST, [("array", P, S.PLAIN, [("v", O)])]),                      # named array: a struct element
        ("many", O, S.LIST, [("e", P, S.PLAIN, [("v", O), ("w", R)])]),               # several fields: a struct element
        ("std", O, S.LIST, [("list", P, S.PLAIN, [("element", O)])]),                 # 3-level
        ("bare", P),                                                                  # unannotated repeated leaf
        ("rg", P, S.PLAIN, [("v", O)]),                                               # unannotated repeated group
        ("mp", O, S.MAP, [("key_value", P, S.PLAIN, [("key", R), ("value", O)])]),
        ("g", R, S.PLAIN, [("h", O, S.PLAIN, [("v", R)])]),
    ])
    shape = T.plan(nodes, kinds).shape()[3]
    assert shape == [
        ("list", "two", True, ("leaf", "array", False)),
        ("list", "tup", True, ("struct", "tup_tuple", False, [("leaf", "v", True)])),
        ("list", "arr", False, ("struct", "array", False, [("leaf", "v", True)])),
        ("list", "many", True, ("struct", "e", False, [("leaf", "v", True), ("leaf", "w", False)])),
        ("list", "std", True, ("leaf", "element", True)),
        ("list", "bare", False, ("leaf", "bare", False)),
        ("list", "rg", False, ("struct", "rg", False, [("leaf", "v", True)])),
        ("map", "mp", True, ("struct", "key_value", False, [("leaf", "key", False), ("leaf", "value", True)])),
        ("struct", "g", False, [("struct", "h", True, [("leaf", "v", False)])]),
    ]
    # a group with no selected leaf below it is left out
    assert [n.leaf for n in nodes if n.name == "bare"] == [6]
    assert [c[1] for c in T.plan(nodes, kinds, [0, 6]).shape()[3]] == ["two", "bare"]


def test_plan_refuses_five_list_depths():
    f = ("v", S.OPT)
    for _ in range(5):
        f = ("l", S.OPT, S.LIST, [("list", S.REP, S.PLAIN, [f])])
    nodes, kinds = S.schema([f, ("flat", S.OPT)])
    with pytest.raises(pqgpu.PqgError) as e:
        T.plan(nodes, kinds)
    assert e.value.code == abi.STATUS_CODES["UNSUPPORTED"]
    assert T.plan(nodes, kinds, [1]).shape() == ("struct", "", False, [("leaf", "flat", True)])


def test_legacy_two_level_list_file():
    rng = np.random.default_rng(3)
    nodes, kinds = S.schema([("a", S.OPT, S.LIST, [("array", S.REP)]), ("b", S.OPT, S.LIST, [("array", S.REP)])])
    root = T.plan(nodes, kinds)

    def lst():
        u = rng.random()
        return None if u < 0.2 else [] if u < 0.35 else [int(x) for x in rng.integers(-99, 99, rng.integers(1, 5))]

    rows = [{"a": lst(), "b": lst()} for _ in range(300)]
    lv = S.shred(root, rows)
    data = S.legacy_list_file([(n, lv[i][0], lv[i][1], lv[i][2]) for i, n in enumerate("ab")], len(rows))
    pf = pqgpu.ParquetFile(data)
    assert [n.name for n in pf.schema_nodes] == [b"a", b"array", b"b", b"array"]
    assert pf.schema_kinds == [abi.NODE_LIST, abi.NODE_PLAIN, abi.NODE_LIST, abi.NODE_PLAIN]
    assert [(n.max_def, n.max_rep) for n in pf.schema_nodes] == [(1, 0), (2, 1)] * 2
    root = T.plan(pf.schema_nodes, pf.schema_kinds)
    assert root.shape()[3] == [("list", "a", True, ("leaf", "array", False)),
                               ("list", "b", True, ("leaf", "array", False))]
    tree = S.host_tree(root, pf.schema_nodes, S.oracle_leaves(pf, 0), len(rows))
    assert tree.to_pylist() == rows
    pa = pytest.importorskip("pyarrow")
    assert tree.to_arrow().field(0).to_pylist() == [r["a"] for r in rows]
    assert tree.to_arrow().type.field(0).type == pa.list_(pa.field("array", pa.int32(), nullable=False))


def test_struct_bits_small_cases():
    # optional struct of one optional leaf, flat: def 0 null struct, 1 null leaf, 2 value
    w, nulls, n = S.struct_bits([2, 0, 1, 0, 2], None, 0, 1, [])
    assert (w.tolist(), nulls, n) == ([0b10101], 2, 5)
    # list<struct>: def 0 null list, 1 empty, 2 null struct, 3.. present; the struct sits under one list
    defs, reps = [0, 1, 2, 3, 4, 2, 4], [0, 0, 0, 1, 1, 0, 0]
    w, nulls, n = S.struct_bits(defs, reps, 1, 3, [2])
    assert (w.tolist(), nulls, n) == ([0b10110], 2, 5)
    # the same levels, a struct above the list (depth 0): one slot per row
    w, nulls, n = S.struct_bits(defs, reps, 0, 1, [2])
    assert (w.tolist(), nulls, n) == ([0b11110], 1, 5)
