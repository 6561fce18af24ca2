"""The expected answer of the nested export (pqg_assemble_nested), as a cursor
walk over the slots.

Like ColumnStore.get / Column.getData (data_store.go:158-203,
schema.go:235-264) it reads one (rep, def) pair at a time and keeps one open
list per depth: a slot with repetition level r continues the open list of
depth r (a new row for r = 0), which closes every deeper list; the definition
level then says how far down new lists are opened below that element.  The
Arrow buffers fall out of the lengths of the open lists; nothing here ranks or
scans, so it shares no arithmetic with the kernels or with the closed form in
include/pqgpu.h.  Also here: shredding of nested Python rows into levels
(Dremel's write side), to make valid level streams for the tests."""
import numpy as np


class Model:
    """levels[k-1] = (offsets int32, validity uint32 words, null_count, entries)."""

    def __init__(self):
        self.levels = []
        self.leaf_validity = None
        self.leaf_values = None    # bytes of the spaced fixed-width values
        self.leaf_offsets = None   # int64, byte-array leaf
        self.num_rows = self.num_leaf = self.num_valid = 0


def _pack(bits):
    """LSB-first bits as whole uint32 words."""
    b = np.asarray(bits, dtype=np.uint8)
    pad = (-len(b)) % 32
    if pad:
        b = np.concatenate([b, np.zeros(pad, np.uint8)])
    return np.packbits(b, bitorder="little").view(np.uint32)


def assemble(defs, reps, max_def, list_def, elem_def, values=None, width=0, value_offsets=None, num_slots=None):
    """Walk the slots.  `values`: dense fixed-width values (any array, taken as
    bytes, `width` bytes each); `value_offsets`: int64[num_valid + 1] of a
    byte-array leaf."""
    K = len(elem_def)
    n = num_slots if num_slots is not None else (len(defs) if defs is not None else len(reps))
    d_l = np.asarray(defs).tolist() if defs is not None else None
    r_l = np.asarray(reps).tolist() if reps is not None else None
    ed = [0] + list(elem_def)           # ed[k]: def level at which the depth-k list has an element
    ld = [0] + list(list_def)
    length = [0] * (K + 1)              # length[k]: elements put into depth-k lists so far (k = 0: rows)
    offs = [[] for _ in range(K + 1)]   # offs[k]: where each depth-k list began among the depth-k elements
    bits = [[] for _ in range(K + 1)]
    leaf_bits, leaf_src = [], []        # per leaf slot: valid?, the value cursor when it was reached
    vpos = 0                            # the dense value cursor (getNext)
    ed_leaf = ed[K]
    put_bit, put_src = leaf_bits.append, leaf_src.append
    for r, d in zip(r_l if r_l is not None else [0] * n, d_l if d_l is not None else [0] * n):
        k = r                           # lists deeper than r are closed; this slot goes on at depth r
        while k < K and d >= ed[k]:     # one more element in the open depth-k list, which opens a list below it
            length[k] += 1
            offs[k + 1].append(length[k + 1])
            bits[k + 1].append(d >= ld[k + 1])
            k += 1
        if k == K and d >= ed_leaf:     # one more element in the open innermost list: a leaf slot
            length[K] += 1
            put_bit(d == max_def)
            put_src(vpos)
        if d == max_def:
            vpos += 1
    m = Model()
    for k in range(1, K + 1):
        o = np.array(offs[k] + [length[k]], dtype=np.int64)
        assert o[-1] <= np.iinfo(np.int32).max
        m.levels.append((o.astype(np.int32), _pack(bits[k]), len(bits[k]) - int(np.sum(bits[k], dtype=np.int64)),
                         len(bits[k])))
    m.num_rows, m.num_leaf, m.num_valid = length[0], length[K], vpos
    m.leaf_validity = _pack(leaf_bits)
    valid = np.asarray(leaf_bits, dtype=bool)
    src = np.asarray(leaf_src, dtype=np.int64)
    if width:
        dense = np.ascontiguousarray(values).view(np.uint8).reshape(-1, width)
        out = np.zeros((m.num_leaf, width), np.uint8)
        out[valid] = dense[src[valid]]
        m.leaf_values = out.reshape(-1)
    if value_offsets is not None:
        vo = np.asarray(value_offsets, dtype=np.int64)
        m.leaf_offsets = np.append(vo[src], vo[vpos]).astype(np.int64)
    return m


def column(m, values_dtype=None, chars=None):
    """The model's buffers as a pqgpu.nested.NestedColumn (for to_pylist)."""
    from pqgpu import abi
    from pqgpu.nested import NestedColumn
    t = {np.dtype(np.int32): abi.INT32, np.dtype(np.int64): abi.INT64, np.dtype(np.float32): abi.FLOAT,
         np.dtype(np.float64): abi.DOUBLE}.get(np.dtype(values_dtype)) if values_dtype is not None else None
    w = np.dtype(values_dtype).itemsize if values_dtype is not None else 0
    return NestedColumn([(o, v, nc) for o, v, nc, _ in m.levels], m.leaf_validity, m.num_leaf, values=m.leaf_values,
                        value_width=w, chars=chars, leaf_offsets=m.leaf_offsets, physical_type=t,
                        num_rows=m.num_rows)


# ---------------------------------------------------------------- shredding (the write side)

def shred(rows, list_def, elem_def, max_def):
    """Nested Python rows -> (def, rep, leaf values in order).  A row is K
    lists deep; None at a list position is a null list (needs list_def[k] <
    elem_def[k], and list_def[k] > elem_def[k-1] ... i.e. a level of its own),
    [] an empty one, None at the leaf a null value (needs elem_def[K] <
    max_def)."""
    K = len(elem_def)
    ed = [0] + list(elem_def)
    ld = [0] + list(list_def)
    defs, reps, vals = [], [], []

    def put(x, k, rep):
        # x: what sits at an element of depth k (k = 0: the row); below it, a depth-(k+1) list or the leaf
        if k == K:
            if x is None:
                assert ed[K] < max_def, "null leaf needs an optional leaf"
                defs.append(max_def - 1)
            else:
                defs.append(max_def)
                vals.append(x)
            reps.append(rep)
            return
        if x is None:
            assert ld[k + 1] > ed[k], "null list needs an optional list"
            defs.append(ld[k + 1] - 1)
            reps.append(rep)
        elif len(x) == 0:
            assert ed[k + 1] > ld[k + 1], "an empty list needs a level below its elements'"
            defs.append(ld[k + 1])
            reps.append(rep)
        else:
            for j, y in enumerate(x):
                put(y, k + 1, rep if j == 0 else k + 1)

    for row in rows:
        put(row, 0, 0)
    return np.array(defs, np.uint8), np.array(reps, np.uint8), vals


def arrow_layout(arr, K):
    """A pyarrow (Large)ListArray K lists deep -> ([(offsets from 0, valid
    bools)] per depth, leaf valid bools, leaf array)."""
    levels = []
    for _ in range(K):
        o = np.asarray(arr.offsets).astype(np.int64)
        levels.append(((o - o[0]).astype(np.int32), np.asarray(arr.is_valid())))
        arr = arr.values[int(o[0]):int(o[-1])]
    return levels, np.asarray(arr.is_valid()), arr


def pyarrow_thresholds(K, optional_leaf=True):
    """pyarrow's shredding of K nested optional 3-level lists over an optional
    (or required) leaf: depth k has a null level, an empty level, then its
    elements'."""
    list_def = [2 * k + 1 for k in range(K)]
    elem_def = [2 * k + 2 for k in range(K)]
    return list_def, elem_def, 2 * K + (1 if optional_leaf else 0)


def random_rows(rng, n_rows, K, value, p_null=0.1, p_empty=0.1, max_len=4, p_null_leaf=0.15):
    """Random rows K lists deep with nulls and empties at every depth."""
    def make(k):
        if k == K:
            return None if rng.random() < p_null_leaf else value()
        u = rng.random()
        if u < p_null:
            return None
        if u < p_null + p_empty:
            return []
        return [make(k + 1) for _ in range(int(rng.integers(1, max_len + 1)))]
    return [make(0) for _ in range(n_rows)]
