"""K8 nested export (pqg_assemble_nested) against the cursor-walk model
(tests/nested_model.py), byte for byte: offsets, bitmaps as whole dwords, leaf
values, leaf offsets and every count; then whole files through
FileReader.read_row_group_nested against pyarrow."""
import ctypes as C
import io

import numpy as np
import pytest

import nested_model as M
from pqgpu.nested import _bits

pytestmark = pytest.mark.gpu

SEG = 4096  # slots per wave segment (pqg_assemble.hip)


@pytest.fixture(scope="module")
def dec():
    import pqgpu
    d = pqgpu.GpuDecoder(0)
    yield d
    d.close()


def _thresholds(K):
    return M.pyarrow_thresholds(K) if K else ([], [], 1)


_STREAMS = {}


def _stream(K, min_slots=3 * SEG + 17):
    """A valid shredding K lists deep with at least `min_slots` slots, made
    once per depth.  Any prefix of it is a valid shredding too (of the rows
    before the cut and a shorter last row)."""
    if K not in _STREAMS:
        rng = np.random.default_rng(100 + K)
        list_def, elem_def, max_def = _thresholds(K)
        defs, reps, have = [], [], 0
        while have < min_slots:  # whole rows, a few hundred at a time
            rows = M.random_rows(rng, 400, K, lambda: 1, p_null=0.12, p_empty=0.12)
            d, r, _ = M.shred(rows, list_def, elem_def, max_def)
            defs.append(d)
            reps.append(r)
            have += len(d)
        _STREAMS[K] = (np.concatenate(defs), np.concatenate(reps))
    return _STREAMS[K]


def _values(defs, max_def, width, seed=1):
    nv = int((np.asarray(defs) == max_def).sum())
    return np.random.default_rng(seed).integers(1, 256, size=nv * width, dtype=np.uint8)


def _gpu_nested(dec, defs, reps, max_def, list_def, elem_def, values=None, width=0, value_offsets=None, n=None,
                shift=(0, 0)):
    """Run the call on uploaded arrays and download every output whole.
    `shift`: bytes the def / rep streams start past their (aligned) buffers."""
    n = n if n is not None else len(defs)
    ptrs = []

    def up(a, dtype=None):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)  # dtype None: the array's own bytes, whatever its type
        p = dec.upload(a.view(np.uint8) if a.nbytes else b"\0")
        ptrs.append(p)
        return p

    if width:  # the call reads num_valid x width bytes of `values`: never hand it less
        assert np.asarray(values).nbytes >= (n if defs is None else int((np.asarray(defs) == max_def).sum())) * width
    dp = up(np.r_[np.zeros(shift[0], np.uint8), defs]) + shift[0] if defs is not None else None
    rp = up(np.r_[np.zeros(shift[1], np.uint8), reps]) + shift[1] if reps is not None else None
    vp = up(values) if values is not None else None
    op = up(value_offsets, np.int64) if value_offsets is not None else None
    a = dec.assemble_nested(dp, rp, vp, n, max_def, list_def, elem_def, value_width=width, value_offsets_ptr=op)
    got = M.Model()
    for k in range(len(elem_def)):
        l = a.level[k]
        got.levels.append((dec.d2h(l.offsets, (l.num_entries + 1) * 4, np.int32),
                           dec.d2h(l.validity, (l.num_entries + 31) // 32 * 4, np.uint32),
                           int(l.null_count), int(l.num_entries)))
    got.num_rows, got.num_leaf, got.num_valid = int(a.num_rows), int(a.num_leaf), int(a.num_valid)
    got.leaf_validity = dec.d2h(a.leaf_validity, (a.num_leaf + 31) // 32 * 4, np.uint32)
    got.leaf_values = dec.d2h(a.leaf_values, a.num_leaf * width) if a.leaf_values else None
    got.leaf_offsets = dec.d2h(a.leaf_offsets, (a.num_leaf + 1) * 8, np.int64) if a.leaf_offsets else None
    got.values_after = dec.d2h(vp, np.asarray(values).nbytes) if vp and values is not None else None
    dec.free_nested(a)
    for p in ptrs:
        dec.free(p)
    return got


def _same(got, exp):
    assert (got.num_rows, got.num_leaf, got.num_valid) == (exp.num_rows, exp.num_leaf, exp.num_valid), "counts"
    assert len(got.levels) == len(exp.levels)
    for k, (g, e) in enumerate(zip(got.levels, exp.levels)):
        assert g[3] == e[3] and g[2] == e[2], "depth %d entries / null count" % (k + 1)
        assert np.array_equal(g[0], e[0]), "depth %d offsets" % (k + 1)
        assert np.array_equal(g[1], e[1]), "depth %d validity" % (k + 1)
    assert np.array_equal(got.leaf_validity, exp.leaf_validity), "leaf validity"
    for name in ("leaf_values", "leaf_offsets"):
        g, e = getattr(got, name), getattr(exp, name)
        assert (g is None) == (e is None), name
        assert g is None or np.array_equal(g, e), name


def _run(dec, defs, reps, K, width=4, thresholds=None):
    list_def, elem_def, max_def = thresholds or _thresholds(K)
    vals = _values(defs, max_def, width) if width else None
    exp = M.assemble(defs, reps, max_def, list_def, elem_def, vals, width, num_slots=len(defs))
    got = _gpu_nested(dec, defs, reps, max_def, list_def, elem_def, vals, width)
    _same(got, exp)
    return exp


# ---------------------------------------------------------------- ballot and segment edges

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, SEG - 1, SEG, SEG + 1, 3 * SEG + 17])
@pytest.mark.parametrize("K", [0, 1, 2, 3, 4])
def test_nested_sizes(dec, K, n):
    defs, reps = _stream(K)
    width = {0: 4, 1: 8, 2: 12, 3: 1, 4: 4}[K]
    _run(dec, defs[:n], reps[:n] if K else None, K, width)


@pytest.mark.parametrize("width", [1, 4, 8, 12])
def test_nested_widths(dec, width):
    defs, reps = _stream(2)
    exp = _run(dec, defs[:2 * SEG + 100], reps[:2 * SEG + 100], 2, width)
    assert exp.num_valid > 0 and exp.num_leaf > exp.num_valid


@pytest.mark.parametrize("shift", [(1, 2), (0, 3), (2, 0), (3, 3)])
def test_nested_unaligned_levels(dec, shift):
    """Level streams that do not start on a 4-byte boundary (a chunk result's
    levels start wherever the chunk's slots do): the kernels then read bytes,
    not dwords, for whole segments."""
    defs, reps = _stream(2)
    n = 2 * SEG + 300
    list_def, elem_def, max_def = _thresholds(2)
    vals = _values(defs[:n], max_def, 8)
    exp = M.assemble(defs[:n], reps[:n], max_def, list_def, elem_def, vals, 8)
    _same(_gpu_nested(dec, defs[:n], reps[:n], max_def, list_def, elem_def, vals, 8, shift=shift), exp)


def test_nested_no_def_levels(dec):
    """max_def == 0 with def_levels NULL: everything present (a required flat column)."""
    n = SEG + 9
    vals = _values(np.zeros(n, np.uint8), 0, 8)
    exp = M.assemble(None, None, 0, [], [], vals, 8, num_slots=n)
    _same(_gpu_nested(dec, None, None, 0, [], [], vals, 8, n=n), exp)


# ---------------------------------------------------------------- lists over segment edges

def test_nested_inner_list_spans_three_segments(dec):
    rng = np.random.default_rng(5)
    list_def, elem_def, max_def = _thresholds(2)
    big = [None if j % 97 == 0 else j for j in range(9000)]
    rows = M.random_rows(rng, 300, 2, lambda: 7) + [[[1, 2], big, [], None, [3]]] + \
        M.random_rows(rng, 300, 2, lambda: 7)
    defs, reps, _ = M.shred(rows, list_def, elem_def, max_def)
    exp = _run(dec, defs, reps, 2, 8)
    lens = np.diff(exp.levels[1][0])
    assert int(lens.max()) == 9000
    # the slot it starts at: the entry of that inner list
    first = int(np.flatnonzero((reps <= 1) & (defs >= elem_def[0]))[int(lens.argmax())])
    assert (first + 8999) // SEG - first // SEG >= 2


def test_nested_segment_of_null_outer_lists(dec):
    """Every slot of a whole segment is a null outer list: that stretch of the
    depth-1 bitmap is zero words between two carried ranks, and no other
    output moves."""
    rng = np.random.default_rng(6)
    list_def, elem_def, max_def = _thresholds(2)
    rows = M.random_rows(rng, 700, 2, lambda: 7) + [None] * (2 * SEG + 50) + M.random_rows(rng, 700, 2, lambda: 7)
    defs, reps, _ = M.shred(rows, list_def, elem_def, max_def)
    s = int(np.flatnonzero(defs == 0)[0] // SEG + 1)
    assert (defs[s * SEG:(s + 1) * SEG] == 0).all()
    exp = _run(dec, defs, reps, 2, 4)
    assert exp.levels[0][2] >= 2 * SEG + 50


# ---------------------------------------------------------------- scan carry

def test_nested_scan_second_round(dec):
    """1024 * 4096 + 5000 slots at depth 2: more segments than the scan
    block's first round, so the later segments' bases come through the carry.
    (Long inner lists: the model walks every slot, and leaf slots are its
    cheapest.)"""
    rng = np.random.default_rng(8)
    list_def, elem_def, max_def = _thresholds(2)
    rows = M.random_rows(rng, 1500, 2, lambda: 1, max_len=24)
    defs0, reps0, _ = M.shred(rows, list_def, elem_def, max_def)
    n = 1024 * SEG + 5000
    t = n // len(defs0) + 1  # whole rows: tiling them is a valid shredding
    defs, reps = np.tile(defs0, t)[:n], np.tile(reps0, t)[:n]
    vals = np.arange(int((defs == max_def).sum()), dtype=np.int32)
    exp = M.assemble(defs, reps, max_def, list_def, elem_def, vals, 4)
    assert len(defs0) % SEG and exp.num_leaf > exp.num_valid > 0 and exp.levels[0][2] > 0 and exp.levels[1][2] > 0
    got = _gpu_nested(dec, defs, reps, max_def, list_def, elem_def, vals, 4)
    _same(got, exp)


# ---------------------------------------------------------------- byte-array leaf

@pytest.mark.parametrize("K", [0, 1, 2])
def test_nested_byte_array_leaf(dec, K):
    defs, reps = _stream(K)
    n = 2 * SEG + 333
    defs, reps = defs[:n], (reps[:n] if K else None)
    list_def, elem_def, max_def = _thresholds(K)
    rng = np.random.default_rng(K)
    nv = int((defs == max_def).sum())
    voffs = np.r_[0, np.cumsum(rng.integers(0, 9, size=nv))].astype(np.int64) + 5  # a chunk's offsets need not start at 0
    chars = rng.integers(0, 256, size=int(voffs[-1]), dtype=np.uint8)
    exp = M.assemble(defs, reps, max_def, list_def, elem_def, value_offsets=voffs)
    got = _gpu_nested(dec, defs, reps, max_def, list_def, elem_def, chars, 0, voffs)
    _same(got, exp)
    assert np.array_equal(got.values_after, chars), "chars untouched"
    lens = np.diff(got.leaf_offsets)
    assert (lens[~_bits(exp.leaf_validity, exp.num_leaf)] == 0).all(), "a null is an empty string"


# ---------------------------------------------------------------- bitmap alignment

@pytest.mark.parametrize("first", [64 + 0, 64 + 31, 64 + 32, 64 + 33])
@pytest.mark.parametrize("K", [1, 2])
def test_nested_bitmap_alignment(dec, K, first):
    """The first segment holds exactly `first` rows, so the second segment's
    row bits start at bit 0, 31, 32 (0 of the next word) or 33 (1) of a dword:
    or_bits' split of a 64-bit group over two or three words."""
    rng = np.random.default_rng(first)
    list_def, elem_def, max_def = _thresholds(K)
    inner = (lambda x: x) if K == 1 else (lambda x: [x])
    head = [None if j % 3 == 0 else ([] if j % 3 == 1 else inner([j])) for j in range(first - 1)]
    head.append(inner([None if j % 5 == 0 else j for j in range(SEG - (first - 1))]))
    rows = head + M.random_rows(rng, 2000, K, lambda: 3, p_null=0.3, p_empty=0.2, max_len=2)
    defs, reps, _ = M.shred(rows, list_def, elem_def, max_def)
    assert int((reps[:SEG] == 0).sum()) == first and reps[SEG] == 0
    _run(dec, defs, reps, K, 4)


# ---------------------------------------------------------------- K = 1 against pqg_assemble_list

def test_nested_depth1_equals_list_export(dec):
    defs, reps = _stream(1)
    n = 3 * SEG + 17
    defs, reps = defs[:n], reps[:n]
    vals = _values(defs, 3, 8)
    got = _gpu_nested(dec, defs, reps, 3, [1], [2], vals, 8)
    dp, rp, vp = dec.upload(defs), dec.upload(reps), dec.upload(vals)
    a, lvp, lop, evp, vvp = dec.assemble_list(dp, rp, vp, n, 3, 1, 2, 8)
    rows, el = a.num_rows, a.num_elements
    assert (rows, el, a.num_valid, a.null_lists) == (got.num_rows, got.num_leaf, got.num_valid, got.levels[0][2])
    assert np.array_equal(dec.d2h(lvp, (rows + 31) // 32 * 4, np.uint32), got.levels[0][1])
    assert np.array_equal(dec.d2h(lop, (rows + 1) * 4, np.int32), got.levels[0][0])
    assert np.array_equal(dec.d2h(evp, (el + 31) // 32 * 4, np.uint32), got.leaf_validity)
    assert np.array_equal(dec.d2h(vvp, el * 8), got.leaf_values)
    for p in (dp, rp, vp, lvp, lop, evp, vvp):
        dec.free(p)


# ---------------------------------------------------------------- argument errors

_ERRORS = {
    "depth 5": ("UNSUPPORTED", lambda a: setattr(a, "depth", 5)),
    "depth -1": ("UNSUPPORTED", lambda a: setattr(a, "depth", -1)),
    "list_def below the parent's elem_def": ("INVALID_ARG", lambda a: setattr(a.level[1], "list_def", 1)),
    "list_def above elem_def": ("INVALID_ARG", lambda a: setattr(a.level[0], "list_def", 3)),
    "elem_def above max_def": ("INVALID_ARG", lambda a: setattr(a.level[1], "elem_def", 6)),
    "elem_def not increasing": ("INVALID_ARG", lambda a: (setattr(a.level[1], "elem_def", 2),
                                                          setattr(a.level[1], "list_def", 2))),
    "negative list_def": ("INVALID_ARG", lambda a: setattr(a.level[0], "list_def", -1)),
    "leaf_values without values": ("INVALID_ARG", lambda a: setattr(a, "values", None)),
    "leaf_values with width 0": ("INVALID_ARG", lambda a: setattr(a, "value_width", 0)),
    "leaf_offsets without value_offsets": ("INVALID_ARG", lambda a: setattr(a, "value_offsets", None)),
    "no def_levels with max_def > 0": ("INVALID_ARG", lambda a: setattr(a, "def_levels", None)),
}


@pytest.mark.parametrize("what", list(_ERRORS))
def test_nested_argument_errors(dec, what):
    """Each rejected call returns its status and writes no output: every
    output buffer still holds its poison."""
    from pqgpu import abi
    status, spoil = _ERRORS[what]
    defs, reps = _stream(2)
    n = SEG + 100
    defs, reps = defs[:n], reps[:n]
    vals = _values(defs, 5, 4)
    voffs = np.arange(len(vals) // 4 + 1, dtype=np.int64)
    poison = np.full((n + 1) * 8, 0xAB, np.uint8)
    ins = [dec.upload(x.view(np.uint8)) for x in (defs, reps, vals, voffs)]
    outs = [dec.upload(poison) for _ in range(7)]
    a = abi.NestedArgs()
    a.def_levels, a.rep_levels, a.values, a.value_offsets = ins
    a.num_slots, a.max_def, a.depth, a.value_width = n, 5, 2, 4
    for k, (ld, ed) in enumerate([(1, 2), (3, 4)]):
        a.level[k].list_def, a.level[k].elem_def = ld, ed
        a.level[k].validity, a.level[k].offsets = outs[2 * k], outs[2 * k + 1]
    a.leaf_validity, a.leaf_values, a.leaf_offsets = outs[4:7]
    spoil(a)
    rc = dec.L.pqg_assemble_nested(dec.ctx, C.byref(a))
    assert abi.status_name(rc) == status
    for p in outs:
        assert np.array_equal(dec.d2h(p, poison.nbytes), poison), "an output was written"
    for p in ins + outs:
        dec.free(p)


def test_nested_valid_call_of_the_error_fixture(dec):
    """The same arguments unspoiled succeed (with both leaf outputs at once)."""
    from pqgpu import abi
    defs, reps = _stream(2)
    n = SEG + 100
    defs, reps = defs[:n], reps[:n]
    vals = _values(defs, 5, 4)
    voffs = np.arange(len(vals) // 4 + 1, dtype=np.int64)
    exp = M.assemble(defs, reps, 5, [1, 3], [2, 4], vals, 4, voffs)
    ins = [dec.upload(x.view(np.uint8)) for x in (defs, reps, vals, voffs)]
    a = abi.NestedArgs()
    a.def_levels, a.rep_levels, a.values, a.value_offsets = ins
    a.num_slots, a.max_def, a.depth, a.value_width = n, 5, 2, 4
    a.level[0].list_def, a.level[0].elem_def, a.level[1].list_def, a.level[1].elem_def = 1, 2, 3, 4
    lv, lo = dec.upload(np.zeros(n * 4, np.uint8)), dec.upload(np.zeros((n + 1) * 8, np.uint8))
    a.leaf_values, a.leaf_offsets = lv, lo
    assert dec.L.pqg_assemble_nested(dec.ctx, C.byref(a)) == 0
    assert (a.num_rows, a.num_leaf, a.num_valid) == (exp.num_rows, exp.num_leaf, exp.num_valid)
    assert [(a.level[k].num_entries, a.level[k].null_count) for k in range(2)] == [(l[3], l[2]) for l in exp.levels]
    assert np.array_equal(dec.d2h(lv, a.num_leaf * 4), exp.leaf_values)
    assert np.array_equal(dec.d2h(lo, (a.num_leaf + 1) * 8, np.int64), exp.leaf_offsets)
    for p in ins + [lv, lo]:
        dec.free(p)


# ---------------------------------------------------------------- end to end

RG_ROWS = 1200  # rows per row group of the end-to-end file


def _slots(x, k, K):
    return 1 if k == K or not x else sum(_slots(y, k + 1, K) for y in x)


def _fit(rows, K, value):
    """pyarrow cuts a nested column's pages every 1024 slots, and the rest of
    the chunk is its last page.  A V2 page of a handful of values does not
    shrink under snappy; pyarrow then stores it raw and says so in the page
    header, and the decoder, like the reference, unpacks it regardless and
    fails.  So the last row of each row group is made one long
    list that brings the chunk's slots to 512 past a multiple of 1024: every
    page then holds hundreds of values."""
    for hi in range(RG_ROWS, len(rows) + RG_ROWS, RG_ROWS):
        hi = min(hi, len(rows))
        have = sum(_slots(r, 0, K) for r in rows[hi - RG_ROWS if hi % RG_ROWS == 0 else hi - hi % RG_ROWS:hi - 1])
        row = [value() for _ in range((512 - have) % 1024 or 1024)]
        for _ in range(K - 1):
            row = [row]
        rows[hi - 1] = row
    return rows


def _e2e_table(pa, n=2000):
    """Leaf values cycle through a few per column, so that the values of every
    page compress (see _fit)."""
    rng = np.random.default_rng(21)
    count = [0]

    def cyc(vals):
        def value():
            count[0] += 1
            return vals[count[0] % len(vals)]
        return value
    ival, sval = cyc([-7, 300, 12, -999, 5, 77, 1000003]), cyc(["s%d" % (j * j) for j in range(11)])
    fval = cyc([0.5, -2.25, 1e9, 3.0, -0.125])
    aval, bval = cyc([1, -2, 3, 40000, 5]), cyc(["b", "bb", "", "bbbb%d" % 7, "b5", "b66", "b-7"])
    sct = lambda: None if rng.random() < 0.15 else {  # noqa: E731
        "a": None if rng.random() < 0.2 else aval(), "b": None if rng.random() < 0.2 else bval()}
    return pa.table({
        "ll": pa.array(_fit(M.random_rows(rng, n, 2, ival), 2, ival), pa.list_(pa.list_(pa.int32()))),
        "ls": pa.array(_fit(M.random_rows(rng, n, 1, sval), 1, sval), pa.list_(pa.string())),
        "lll": pa.array(_fit(M.random_rows(rng, n, 3, fval, max_len=3), 3, fval),
                        pa.list_(pa.list_(pa.list_(pa.float64())))),
        "s": pa.array([None if rng.random() < 0.2 else "v%d" % (i % 13) for i in range(n)], pa.string()),
        "lst": pa.array(_fit(M.random_rows(rng, n, 1, sct, p_null_leaf=0.0), 1, sct),
                        pa.list_(pa.struct([("a", pa.int32()), ("b", pa.string())]))),
    })


@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_read_row_group_nested_matches_pyarrow(dec, version):
    pa = pytest.importorskip("pyarrow")
    pq = pytest.importorskip("pyarrow.parquet")
    import pqgpu
    from pqgpu import abi
    buf = io.BytesIO()
    pq.write_table(_e2e_table(pa), buf, data_page_size=500, data_page_version=version, compression="snappy",
                   row_group_size=RG_ROWS, use_dictionary=version == "1.0")
    data = buf.getvalue()
    ref = pq.ParquetFile(io.BytesIO(data))
    assert ref.metadata.num_row_groups == 2
    fr = pqgpu.FileReader(data, decoder=dec)
    from oracle import pyoracle as O
    pages = O.decode_chunk(fr.file.host_job(0, 0)[0]).pages
    assert sum(p.page_type != abi.PAGE_DICTIONARY for p in pages) >= 3  # several data pages
    paths = {"ll": ("ll.list.element.list.element", 2), "ls": ("ls.list.element", 1),
             "lll": ("lll.list.element.list.element.list.element", 3), "s": ("s", 0),
             "lst.a": ("lst.list.element.a", 1), "lst.b": ("lst.list.element.b", 1)}
    for rg in range(2):
        got = fr.read_row_group_nested(rg)
        tab = ref.read_row_group(rg)
        assert set(got) == {p for p, _ in paths.values()}
        for name, (path, K) in paths.items():
            col = got[path]
            arr = tab.column(name.split(".")[0]).combine_chunks()
            levels, leaf_valid, leaf = M.arrow_layout(arr, K)
            assert col.num_rows == len(arr) and len(col.levels) == K
            for (offs, bits, nulls), (eo, ev) in zip(col.levels, levels):
                assert np.array_equal(offs, eo), "%s offsets" % path
                assert np.array_equal(_bits(bits, len(ev)), ev), "%s validity" % path
                assert nulls == int((~ev).sum())
            if "." in name:  # a struct's field: the leaf is null when the struct or the field is
                leaf_valid = leaf_valid & np.asarray(leaf.field(name.split(".")[1]).is_valid())
            assert col.num_leaf == len(leaf_valid)
            assert np.array_equal(_bits(col.leaf_validity, col.num_leaf), leaf_valid), "%s leaf validity" % path
            if "." not in name:
                exp = arr.to_pylist()
                if pa.types.is_string(leaf.type):
                    enc = lambda x: x.encode() if isinstance(x, str) else ([enc(y) for y in x] if isinstance(x, list) else x)  # noqa: E731
                    exp = enc(exp)
                assert col.to_pylist() == exp, path
        # both fields of the struct give the same lists
        la, lb = got[paths["lst.a"][0]].levels[0], got[paths["lst.b"][0]].levels[0]
        assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1]) and la[2] == lb[2]


def test_depth_5_is_unsupported(dec):
    pa = pytest.importorskip("pyarrow")
    pq = pytest.importorskip("pyarrow.parquet")
    import pqgpu
    from pqgpu import abi
    t = pa.int32()
    for _ in range(5):
        t = pa.list_(t)
    buf = io.BytesIO()
    pq.write_table(pa.table({"ok": pa.array([[1], [2]], pa.list_(pa.int32())), "deep": pa.array([[[[[[1]]]]], None], t)}),
                   buf)
    fr = pqgpu.FileReader(buf.getvalue(), decoder=dec)
    with pytest.raises(pqgpu.PqgError) as e:
        fr.read_row_group_nested(0)
    assert e.value.code == abi.STATUS_CODES["UNSUPPORTED"] and "deep.list.element" in str(e.value)
    # the supported column of the same file still reads
    ok = pqgpu.FileReader(buf.getvalue(), "ok", decoder=dec).read_row_group_nested(0)
    assert ok["ok.list.element"].to_pylist() == [[1], [2]]
    # the same from rows.json-style schema nodes: five bare REPEATED groups
    nodes = [type("N", (), dict(name="l%d" % k, repetition=2, num_children=1 if k < 4 else 0, leaf=0 if k == 4 else -1,
                                max_def=k + 1, max_rep=k + 1)) for k in range(5)]
    list_def, elem_def = pqgpu.leaf_thresholds(nodes, 0)
    assert elem_def == [1, 2, 3, 4, 5]
    one = dec.upload(np.array([5], np.uint8))
    with pytest.raises(pqgpu.PqgError) as e:
        dec.assemble_nested(one, one, None, 1, 5, list_def, elem_def)
    assert e.value.code == abi.STATUS_CODES["UNSUPPORTED"]
    dec.free(one)
