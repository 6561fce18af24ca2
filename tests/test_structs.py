"""K8 struct export (pqg_assemble_structs) against the cursor-walk model
(tests/struct_model.py), bitmaps as whole dwords and every count; then whole
files through FileReader.read_row_group_tree against pyarrow and against a
committed file."""
import ctypes as C
import io
import json
import os

import numpy as np
import pytest

import nested_model as M
import struct_model as S
import struct_tables as ST
from pqgpu import abi
from pqgpu import tree as T
from pqgpu.nested import _bits, leaf_thresholds

pytestmark = pytest.mark.gpu

SEG = 4096  # slots per wave segment (pqg_assemble.hip)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CANARY = 0xA5
TAIL = 64   # canary bytes after each bitmap


@pytest.fixture(scope="module")
def dec():
    import pqgpu
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


# ---------------------------------------------------------------- level streams

def _schema(K):
    """One leaf under K lists with optional structs at every depth: s0 { t0 { l1: list<s1 { t1 {
    l2: ... sK { v } } }> } }, two structs a depth while that keeps them within 8."""
    f = ("s%d" % K, S.OPT, S.PLAIN, [("v", S.OPT)])
    for k in range(K, 0, -1):
        f = ("l%d" % k, S.OPT, S.LIST, [("list", S.REP, S.PLAIN, [f])])
        if k - 1 < 3:
            f = ("t%d" % (k - 1), S.OPT, S.PLAIN, [f])
        f = ("s%d" % (k - 1), S.OPT, S.PLAIN, [f])
    if K == 0:
        f = ("a", S.OPT, S.PLAIN, [("b", S.OPT, S.PLAIN, [f])])
    return S.schema([f])


_CASES = {}


def _case(K, min_slots=70_001):
    """(defs, reps, max_def, elem_def, [(depth, struct_def)]) of a valid shredding under
    _schema(K), at least min_slots long, made once per depth.  A prefix is the shredding of the
    rows before the cut and a shorter last row."""
    if K not in _CASES:
        nodes, kinds = _schema(K)
        root = T.plan(nodes, kinds)
        rng = np.random.default_rng(200 + K)
        defs, reps, have = [], [], 0
        while have < min_slots:
            d, r, _ = S.shred(root, S.random_rows(root, rng, 2000))[0]
            defs.append(d)
            reps.append(r)
            have += len(d)
        structs = [(n.depth, n.struct_def) for n in T.walk(root) if n.kind == "struct" and n.nullable]
        assert len(structs) == [3, 3, 5, 7, 8][K] and {d for d, _ in structs} == set(range(K + 1))
        _CASES[K] = (np.concatenate(defs), np.concatenate(reps), nodes[-1].max_def, leaf_thresholds(nodes, 0)[1],
                     structs)
    return _CASES[K]


def _expected(defs, reps, n, elem_def, structs):
    return [S.struct_bits(defs[:n], reps[:n] if reps is not None else None, d, sd, elem_def, n) for d, sd in structs]


# ---------------------------------------------------------------- the call, on canaried buffers

def _call(dec, defs, reps, n, max_def, elem_def, structs, shift=(0, 0), validity=True, depth=None,
          num_structs=None, keep_def=True):
    """pqg_assemble_structs on uploaded arrays.  Every bitmap buffer is 4 * ceil(n / 32) + TAIL
    bytes of CANARY before the call and is downloaded whole.  Returns (status, StructArgs,
    [buffer bytes or None])."""
    ptrs = []

    def up(a):
        p = dec.upload(np.ascontiguousarray(a, dtype=np.uint8))
        ptrs.append(p)
        return p

    a = abi.StructArgs()
    if defs is not None and keep_def:
        a.def_levels = up(np.r_[np.zeros(shift[0], np.uint8), defs[:n], np.zeros(4, np.uint8)]) + shift[0]
    if reps is not None:
        a.rep_levels = up(np.r_[np.zeros(shift[1], np.uint8), reps[:n], np.zeros(4, np.uint8)]) + shift[1]
    a.num_slots, a.max_def = n, max_def
    a.depth = len(elem_def) if depth is None else depth
    for k, e in enumerate(elem_def[:abi.MAX_LIST_DEPTH]):
        a.elem_def[k] = e
    a.num_structs = len(structs) if num_structs is None else num_structs
    bm = (max(n, 0) + 31) // 32 * 4
    for j, (d, sd) in enumerate(structs[:abi.MAX_STRUCTS]):
        a.st[j].depth, a.st[j].struct_def = d, sd
        a.st[j].num_entries = a.st[j].null_count = -7
        if validity:
            a.st[j].validity = up(np.full(bm + TAIL, CANARY, np.uint8))
    rc = dec.L.pqg_assemble_structs(dec.ctx, C.byref(a))
    bufs = [dec.d2h(a.st[j].validity, bm + TAIL) if a.st[j].validity else None
            for j in range(min(len(structs), abi.MAX_STRUCTS))]
    for p in ptrs:
        dec.free(p)
    return rc, a, bufs


def _check(a, bufs, n, exp, what=""):
    bm = (n + 31) // 32 * 4
    for j, (words, nulls, entries) in enumerate(exp):
        assert (a.st[j].num_entries, a.st[j].null_count) == (entries, nulls), "%s struct %d counts" % (what, j)
        if bufs[j] is None:
            continue
        assert (bufs[j][bm:] == CANARY).all(), "%s struct %d: bytes past the bitmap" % (what, j)
        got = bufs[j][:bm].view(np.uint32)
        want = np.zeros(bm // 4, np.uint32)  # whole dwords, zero at and past num_entries
        want[:len(words)] = words
        assert np.array_equal(got, want), "%s struct %d bitmap" % (what, j)


SIZES = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 3 * SEG + 5, 70_001]


@pytest.mark.parametrize("n,K", [(n, i % 5) for i, n in enumerate(SIZES)] + [(4097, K) for K in range(5)])
def test_structs_equal_model(dec, n, K):
    defs, reps, max_def, elem_def, structs = _case(K)
    rc, a, bufs = _call(dec, defs, reps if K else None, n, max_def, elem_def, structs)
    assert rc == 0
    _check(a, bufs, n, _expected(defs, reps, n, elem_def, structs))


@pytest.mark.parametrize("shift", [(1, 1), (2, 3), (3, 0), (0, 2), (0, 0)])
@pytest.mark.parametrize("K", [1, 3])
def test_structs_unaligned_level_pointers(dec, K, shift):
    defs, reps, max_def, elem_def, structs = _case(K)
    n = 3 * SEG + 5
    rc, a, bufs = _call(dec, defs, reps, n, max_def, elem_def, structs, shift=shift)
    assert rc == 0
    _check(a, bufs, n, _expected(defs, reps, n, elem_def, structs))


@pytest.mark.parametrize("K", [0, 2, 4])
@pytest.mark.parametrize("fill", ["null", "valid", "random"])
def test_structs_all_null_all_valid_random(dec, K, fill):
    _, reps, max_def, elem_def, structs = _case(K)
    n = 2 * SEG + 77
    rng = np.random.default_rng(K)
    if fill == "null":      # every row a null outermost struct
        defs, reps = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    elif fill == "valid":   # every slot a value: the repetition levels of the shredding as they are
        defs, reps = np.full(n, max_def, np.uint8), reps[:n]
    else:                   # any levels at all, a valid shredding or not
        defs = rng.integers(0, max_def + 1, n).astype(np.uint8)
        reps = rng.integers(0, K + 1, n).astype(np.uint8)
    rc, a, bufs = _call(dec, defs, reps, n, max_def, elem_def, structs)
    assert rc == 0
    exp = _expected(defs, reps, n, elem_def, structs)
    _check(a, bufs, n, exp, fill)
    if fill == "null":
        assert all(nulls == entries for _, nulls, entries in exp) and exp[0][2] == n
    if fill == "valid":
        assert all(nulls == 0 for _, nulls, _ in exp)


def test_eight_structs_equal_eight_single_calls(dec):
    defs, reps, max_def, elem_def, structs = _case(4)
    assert len(structs) == abi.MAX_STRUCTS
    n = 3 * SEG + 5
    rc, a, bufs = _call(dec, defs, reps, n, max_def, elem_def, structs)
    assert rc == 0
    order = [5, 0, 7, 2, 4, 1, 6, 3]  # mixed depths, in no order
    rc, b, mixed = _call(dec, defs, reps, n, max_def, elem_def, [structs[j] for j in order])
    assert rc == 0
    for j, st in enumerate(structs):
        rc, one, buf = _call(dec, defs, reps, n, max_def, elem_def, [st])
        assert rc == 0
        assert (one.st[0].num_entries, one.st[0].null_count) == (a.st[j].num_entries, a.st[j].null_count)
        assert np.array_equal(buf[0], bufs[j])
        k = order.index(j)
        assert (b.st[k].num_entries, b.st[k].null_count) == (a.st[j].num_entries, a.st[j].null_count)
        assert np.array_equal(mixed[k], bufs[j])
    _check(a, bufs, n, _expected(defs, reps, n, elem_def, structs))


def test_structs_count_only(dec):
    defs, reps, max_def, elem_def, structs = _case(2)
    n = 2 * SEG + 9
    rc, a, bufs = _call(dec, defs, reps, n, max_def, elem_def, structs, validity=False)
    assert rc == 0 and bufs == [None] * len(structs)
    _check(a, bufs, n, _expected(defs, reps, n, elem_def, structs))


def test_structs_past_the_scan_round(dec):
    """Just above 1024 segments: the scan carries its totals into a second round.  The stream is
    whole rows repeated, so the walk of it is the walk of one copy, repeated."""
    defs, reps, max_def, elem_def, structs = _case(2)
    starts = np.flatnonzero(reps == 0)
    cut = int(starts[starts <= 50_021][-1])   # whole rows, not a multiple of the ballot or the segment
    times = (1024 * SEG) // cut + 1
    n = cut * times
    assert 1024 * SEG < n < 1025 * SEG + cut
    two = [structs[0], structs[-1]]           # depth 0 and depth 2
    rc, a, bufs = _call(dec, np.tile(defs[:cut], times), np.tile(reps[:cut], times), n, max_def, elem_def, two)
    assert rc == 0
    exp = []
    for d, sd in two:
        bits = np.tile(np.asarray(S.struct_bit_list(defs[:cut], reps[:cut], d, sd, elem_def), bool), times)
        exp.append((M._pack(bits), int((~bits).sum()), len(bits)))
    _check(a, bufs, n, exp)


# ---------------------------------------------------------------- arguments

def test_structs_argument_errors_write_nothing(dec):
    defs, reps, max_def, elem_def, structs = _case(2)
    n = SEG + 3
    INV, UNS = abi.STATUS_CODES["INVALID_ARG"], abi.STATUS_CODES["UNSUPPORTED"]
    ed = list(elem_def)
    d1 = [s for s in structs if s[0] == 1][0]
    bad = [
        (UNS, dict(depth=5)),
        (UNS, dict(depth=-1)),
        (INV, dict(num_structs=9)),
        (INV, dict(num_structs=-1)),
        (INV, dict(structs=[(3, max_def)])),                       # a depth above args.depth
        (INV, dict(structs=[(-1, 1)])),
        (INV, dict(elem_def=[ed[1], ed[0]])),                      # not increasing
        (INV, dict(elem_def=[ed[0], ed[0]])),                      # not strictly
        (INV, dict(elem_def=[ed[0], max_def + 1], structs=[structs[0]])),
        (INV, dict(structs=[(1, ed[0])])),                         # not above elem_def[R]
        (INV, dict(structs=[(0, 0)])),
        (INV, dict(structs=[(2, max_def + 1)])),                   # above max_def
        (INV, dict(structs=[(1, ed[1])])),                         # not below elem_def[R + 1]
        (INV, dict(structs=[(0, ed[0])])),
        (INV, dict(keep_def=False)),                               # def_levels NULL with structs and slots
        (INV, dict(reps=None)),                                    # rep_levels NULL with depth > 0
    ]
    assert ed[0] < d1[1] < ed[1]
    for want, change in bad:
        kw = dict(defs=defs, reps=reps, n=n, max_def=max_def, elem_def=ed, structs=structs)
        kw.update(change)
        rc, a, bufs = _call(dec, **kw)
        assert rc == want, change
        for j, b in enumerate(bufs):
            assert (b == CANARY).all(), change
            assert (a.st[j].num_entries, a.st[j].null_count) == (-7, -7), change
    rc, a, bufs = _call(dec, defs, reps, n, max_def, ed, [d1])    # and the call they were made from passes
    assert rc == 0
    _check(a, bufs, n, _expected(defs, reps, n, ed, [d1]))


def test_structs_no_slots_does_nothing(dec):
    _, _, max_def, elem_def, structs = _case(2)
    rc, a, bufs = _call(dec, np.zeros(0, np.uint8), np.zeros(0, np.uint8), 0, max_def, elem_def, structs)
    assert rc == 0
    assert all((a.st[j].num_entries, a.st[j].null_count) == (0, 0) for j in range(len(structs)))
    assert all((b == CANARY).all() for b in bufs)
    rc, a, _ = _call(dec, None, None, 0, 1, [], [(0, 1)])        # no levels at all
    assert rc == 0 and a.st[0].num_entries == 0
    rc, a, _ = _call(dec, None, None, 100, 1, [], [])             # no struct: nothing to read
    assert rc == 0


def test_structs_rep_null_at_depth_zero_and_timing(dec):
    defs, _, max_def, elem_def, structs = _case(0)
    n = 5 * SEG + 1
    rc, a, bufs = _call(dec, defs, None, n, max_def, elem_def, structs)
    assert rc == 0 and a.st[0].num_entries == n
    _check(a, bufs, n, _expected(defs, None, n, elem_def, structs))
    assert dec.last_assemble_ms() > 0
    # the decoder's own wrapper: allocates, downloads entries' worth of words
    dp = dec.upload(defs[:n])
    a = dec.assemble_structs(dp, None, n, max_def, elem_def, structs)
    try:
        for (words, nulls, entries), exp in zip(dec.download_structs(a), _expected(defs, None, n, elem_def, structs)):
            assert np.array_equal(words, exp[0]) and (nulls, entries) == exp[1:]
    finally:
        dec.free_structs(a)
        dec.free(dp)


# ---------------------------------------------------------------- whole files

def _jsonable(x):
    if isinstance(x, bytes):
        return x.decode()
    if isinstance(x, dict):
        return {k: _jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_jsonable(v) for v in x]
    return x


@pytest.fixture(scope="module")
def pa_rows():
    pytest.importorskip("pyarrow")
    rows = ST.rows(600)
    return rows, ST.table(rows)


@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_read_row_group_tree_equals_pyarrow(dec, pa_rows, version):
    """V1: dictionary pages and data pages of a few dozen values.  V2: PLAIN pages cut every 1024
    slots, the row groups fitted so that every page compresses (struct_tables.fit)."""
    import pqgpu
    import pyarrow.parquet as pq
    if version == "1.0":
        (rows, t), per_rg = pa_rows, 300
        kw = dict(write_batch_size=50)
    else:
        rows, per_rg = ST.fit(ST.rows(3000, seed=6), 1500), 1500
        t, kw = ST.table(rows), dict(use_dictionary=False)
    data = ST.file_bytes(t, compression="snappy", data_page_version=version, data_page_size=500, row_group_size=per_rg,
                         **kw)
    back = pq.ParquetFile(io.BytesIO(data))
    fr = pqgpu.FileReader(data, decoder=dec)
    assert fr.row_group_count() == 2
    for rg in range(2):
        tree = fr.read_row_group_tree(rg)
        pages = [len(dec.pages(i)) for i in range(12)]
        assert min(pages) >= 2 and max(pages) > 2   # several pages a chunk
        want = back.read_row_group(rg)
        assert tree.length == per_rg and tree.validity is None
        assert tree.to_pylist() == S.encode(want.to_pylist()) == S.encode(rows[per_rg * rg:per_rg * (rg + 1)])
        arr = tree.to_arrow()
        arr.validate(full=True)
        for i, name in enumerate(want.column_names):
            assert arr.field(i).equals(want.column(i).combine_chunks()), name
    fr.close()


def test_read_row_group_tree_golden(dec):
    import pqgpu
    exp = json.load(open(os.path.join(GOLD, "structs_expected.json")))
    fr = pqgpu.FileReader(os.path.join(GOLD, "structs.parquet"), decoder=dec)
    got = []
    for rg in range(fr.row_group_count()):
        tree = fr.read_row_group_tree(rg)
        assert tree.length == fr.file.row_group_rows(rg)
        got += tree.to_pylist()
    fr.close()
    assert fr.row_group_count() == 2 and len(got) == len(exp) == 120
    assert _jsonable(got) == exp
    names = {n.name for n in T.walk(T.plan(fr.file.schema_nodes, fr.file.schema_kinds)) if n.kind != "leaf"}
    assert {"s", "o", "i", "ls", "sl", "m", "r"} <= names
    assert any(r["s"] is None for r in exp) and any(r["s"] is not None and r["s"]["a"] is None for r in exp)


def test_more_structs_than_one_call_takes(dec):
    """Ten optional structs above one leaf: two pqg_assemble_structs calls for its levels."""
    pa = pytest.importorskip("pyarrow")
    import pqgpu
    rng = np.random.default_rng(12)
    depth = abi.MAX_STRUCTS + 2

    def make(k):
        if rng.random() < 0.12:
            return None
        return int(rng.integers(0, 30)) if k == depth else {"n%d" % k: make(k + 1)}

    col = [make(0) for _ in range(700)]
    typ = pa.int32()
    for k in range(depth - 1, -1, -1):
        typ = pa.struct([("n%d" % k, typ)])
    t = pa.table({"top": pa.array(col, typ)})
    fr = pqgpu.FileReader(ST.file_bytes(t, compression="snappy"), decoder=dec)
    root = T.plan(fr.file.schema_nodes, fr.file.schema_kinds)
    assert [len(v) for v in T.structs_by_leaf(root).values()] == [depth]
    tree = fr.read_row_group_tree(0)
    fr.close()
    assert tree.to_pylist() == [{"top": c} for c in col]
    assert tree.to_arrow().field(0).equals(t.column(0).combine_chunks())
    for k in range(depth):   # every depth has nulls of its own
        assert sum(1 for c in col if _depth_of_null(c) == k) > 0


def _depth_of_null(c, k=0):
    return k if c is None else _depth_of_null(next(iter(c.values())), k + 1) if isinstance(c, dict) else -1


@pytest.fixture(scope="module")
def typed_file():
    """struct<d decimal(9, 2), w string, n int32> and a list of the same, written by pyarrow."""
    pa = pytest.importorskip("pyarrow")
    import decimal
    rng = np.random.default_rng(8)

    def maybe(p, make):
        return None if rng.random() < p else make()

    def one():
        return {"d": maybe(0.2, lambda: decimal.Decimal(int(rng.integers(-10 ** 8, 10 ** 8))).scaleb(-2)),
                "w": maybe(0.2, lambda: "k%d" % rng.integers(0, 12)), "n": maybe(0.2, lambda: int(rng.integers(0, 99)))}

    rows = [{"st": maybe(0.2, one), "ls": maybe(0.2, lambda: [maybe(0.2, one) for _ in range(rng.integers(0, 4))])}
            for _ in range(500)]
    typ = pa.struct([("d", pa.decimal128(9, 2)), ("w", pa.string()), ("n", pa.int32())])
    t = pa.table({"st": pa.array([r["st"] for r in rows], typ), "ls": pa.array([r["ls"] for r in rows], pa.list_(typ))})
    return rows, t, ST.file_bytes(t, compression="snappy", data_page_size=500, write_batch_size=50)


def _map_leaves(x, f):
    """x with f applied to every dict value that is not a container."""
    if isinstance(x, dict):
        return {k: _map_leaves(v, f) if isinstance(v, (dict, list)) else f(k, v) for k, v in x.items()}
    if isinstance(x, list):
        return [_map_leaves(v, f) for v in x]
    return x


def test_tree_projection_dictionary_and_logical(dec, typed_file):
    import pqgpu
    import pyarrow.parquet as pq
    rows, t, data = typed_file
    fr = pqgpu.FileReader(data, decoder=dec)
    full = fr.read_row_group_tree(0)
    full_rows = full.to_pylist()
    fr.close()
    assert _map_leaves(full_rows, lambda k, v: v if k != "d" else None) == \
        _map_leaves(S.encode(rows), lambda k, v: v if k != "d" else None)
    # a projected sub-struct: st.w and ls's n keep their structs and drop the rest
    fr = pqgpu.FileReader(data, "st.w", "ls.list.element.n", decoder=dec)
    part = fr.read_row_group_tree(0)
    fr.close()
    assert part.to_pylist() == [
        {"st": None if r["st"] is None else {"w": r["st"]["w"]},
         "ls": None if r["ls"] is None else [None if e is None else {"n": e["n"]} for e in r["ls"]]} for r in full_rows]
    # leaves that keep their dictionaries, inside a struct and inside a list of structs
    fr = pqgpu.FileReader(data, decoder=dec, read_dictionary=("st.w", "ls.list.element.w"))
    kept = fr.read_row_group_tree(0)
    fr.close()
    w = [c for c in kept.children[0].children if c.name == "w"][0]
    assert w.column.dictionary is not None and w.column.value_width == 4
    assert kept.to_pylist() == full_rows
    back = pq.read_table(io.BytesIO(data), read_dictionary=["st.w", "ls.list.element.w"])
    assert kept.to_arrow().field(0).field(1).equals(back.column(0).combine_chunks().field(1))
    # decimals converted on the GPU: what the unconverted big-endian bytes convert to on the host
    fr = pqgpu.FileReader(data, decoder=dec, convert_logical=True)
    conv = fr.read_row_group_tree(0)
    fr.close()

    def widen(k, v):
        return v if k != "d" or v is None else int.from_bytes(v, "big", signed=True).to_bytes(16, "little", signed=True)

    assert any(r["st"] is not None and r["st"]["d"] is not None for r in full_rows)
    assert conv.to_pylist() == _map_leaves(full_rows, widen)
    arr = conv.to_arrow()
    arr.validate(full=True)
    back = pq.read_table(io.BytesIO(data))
    for i in range(2):
        assert arr.field(i).equals(back.column(i).combine_chunks())


def test_read_row_group_nested_is_unchanged(dec, pa_rows):
    """The flat per-leaf view of the same file: every leaf exactly what the nested export's model
    gives for the levels the oracle decodes, struct nulls as leaf nulls."""
    import pqgpu
    _, t = pa_rows
    data = ST.file_bytes(t, compression="snappy", data_page_size=500, write_batch_size=50)
    fr = pqgpu.FileReader(data, decoder=dec)
    got = fr.read_row_group_nested(0)
    pf = fr.file
    leaves = S.oracle_leaves(pf, 0)
    assert sorted(got) == sorted(c.path.decode() for c in pf.columns) and len(got) == 12
    for c, lf in leaves.items():
        col = got[pf.columns[c].path.decode()]
        list_def, elem_def = leaf_thresholds(pf.schema_nodes, c)
        strings = lf["offsets"] is not None
        m = M.assemble(lf["defs"], lf["reps"], pf.columns[c].desc.max_def, list_def, elem_def,
                       None if strings else lf["values"], 0 if strings else lf["width"], lf["offsets"],
                       num_slots=lf["num_slots"])
        assert (col.num_rows, col.num_leaf) == (m.num_rows, m.num_leaf)
        assert len(col.levels) == len(m.levels)
        for (o, v, nc), (eo, ev, enc, _) in zip(col.levels, m.levels):
            assert np.array_equal(o, eo) and np.array_equal(v, ev) and nc == enc
        assert np.array_equal(col.leaf_validity, m.leaf_validity)
        if strings:
            assert np.array_equal(col.leaf_offsets, m.leaf_offsets) and np.array_equal(col.chars, lf["chars"])
        else:
            assert np.array_equal(col.values, m.leaf_values)
    fr.close()
