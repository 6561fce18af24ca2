"""The expected answer of the struct export (pqg_assemble_structs) and of the
column tree (pqgpu.tree), as cursor walks, and the write side that makes level
streams for them.

struct_bits reads one (rep, def) pair at a time, as nested_model.assemble
does: a slot with repetition level r goes on at depth r, the definition level
says how far down it reaches, and a slot that reaches the struct's depth is one
struct slot, present when the level reaches the struct's own.  Nothing here
ranks or scans, so it shares no arithmetic with the kernels or with the closed
form in include/pqgpu.h.

shred writes nested Python rows (dicts for structs, lists for lists, lists of
(key, value) tuples for maps, None for a null) as the per-leaf (def, rep,
values) of a plan (pqgpu.tree.plan): Dremel's write side over structs."""
import numpy as np

import nested_model as M
from pqgpu import tree as T
from pqgpu.nested import NestedColumn, leaf_thresholds


def struct_bit_list(defs, reps, depth, struct_def, elem_def, num_slots=None):
    """The validity bits, one per struct slot, of a struct under `depth` lists,
    present at def >= struct_def; elem_def as in pqg_nested_level."""
    n = num_slots if num_slots is not None else len(defs)
    ed = [0] + list(elem_def)
    d_l = np.asarray(defs).tolist()
    r_l = np.asarray(reps).tolist() if reps is not None else [0] * n
    bits = []
    for r, d in zip(r_l[:n], d_l[:n]):
        k = r                            # lists deeper than r are closed; the slot goes on at depth r
        while k <= depth and d >= ed[k]:  # one more element in the open depth-k list
            if k == depth:               # it reached the struct's depth: one struct slot
                bits.append(d >= struct_def)
            k += 1
    return bits


def struct_bits(defs, reps, depth, struct_def, elem_def, num_slots=None):
    """(validity uint32 words, null_count, entries) of struct_bit_list's bits."""
    bits = struct_bit_list(defs, reps, depth, struct_def, elem_def, num_slots)
    return M._pack(bits), len(bits) - int(np.sum(bits, dtype=np.int64)), len(bits)


class _SN:
    """A schema node record, as pqg_file_schema_node gives them."""

    def __init__(self, name, repetition, num_children, leaf, max_def, max_rep):
        self.name, self.repetition, self.num_children, self.leaf = name, repetition, num_children, leaf
        self.max_def, self.max_rep = max_def, max_rep


REQ, OPT, REP = 0, 1, 2
PLAIN, LIST, MAP = 0, 1, 2


def schema(fields):
    """(schema_nodes, schema_kinds) of a small description: a field is
    (name, repetition, kind, children) for a group, (name, repetition) for a leaf."""
    nodes, kinds, leaves = [], [], [0]

    def put(f, d, r):
        name, rep = f[0], f[1]
        d += rep != REQ
        r += rep == REP
        if len(f) == 2:
            nodes.append(_SN(name, rep, 0, leaves[0], d, r))
            kinds.append(PLAIN)
            leaves[0] += 1
            return
        nodes.append(_SN(name, rep, len(f[3]), -1, d, r))
        kinds.append(f[2])
        for c in f[3]:
            put(c, d, r)

    for f in fields:
        put(f, 0, 0)
    return nodes, kinds


def shred(root, rows):
    """{leaf: (def uint8, rep uint8, values)} of `rows` (dicts of the top-level
    fields) under the plan `root`."""
    out = {n.leaf: ([], [], []) for n in T.walk(root) if n.kind == "leaf"}

    def absent(node, d, rep):            # nothing below `node`: one slot per leaf, at level d
        for n in T.walk(node):
            if n.kind == "leaf":
                out[n.leaf][0].append(d)
                out[n.leaf][1].append(rep)

    def put(node, v, rep, k):
        if node.kind == "leaf":
            if v is None:
                assert node.nullable
                absent(node, node.max_def - 1, rep)
            else:
                absent(node, node.max_def, rep)
                out[node.leaf][2].append(v)
        elif node.kind == "struct":
            if v is None:
                assert node.nullable
                absent(node, node.struct_def - 1, rep)
            else:
                for c in node.children:
                    put(c, v.get(c.name), rep, k)
        else:
            if v is None:
                assert node.nullable
                absent(node, node.elem_def - 2, rep)
            elif len(v) == 0:
                absent(node, node.elem_def - 1, rep)
            else:
                for j, x in enumerate(v):
                    if node.is_map:
                        x = dict(zip([c.name for c in node.child.children], x))
                    put(node.child, x, rep if j == 0 else k + 1, k + 1)

    for row in rows:
        for c in root.children:
            put(c, row.get(c.name), 0, 0)
    return {lf: (np.array(d, np.uint8), np.array(r, np.uint8), v) for lf, (d, r, v) in out.items()}


def random_rows(root, rng, n, p_null=0.15, p_empty=0.1, max_len=3):
    """n random rows of the plan `root`, with nulls wherever the plan allows them."""
    def make(node):
        if node.nullable and rng.random() < p_null:
            return None
        if node.kind == "leaf":
            return int(rng.integers(0, 1000))
        if node.kind == "struct":
            return {c.name: make(c) for c in node.children}
        if rng.random() < p_empty:
            return []
        items = [make(node.child) for _ in range(int(rng.integers(1, max_len + 1)))]
        return [tuple(x[c.name] for c in node.child.children) for x in items] if node.is_map else items

    return [{c.name: make(c) for c in root.children} for _ in range(n)]


def host_tree(root, schema_nodes, leaves, num_rows):
    """The tree of plan `root` by the models alone.  leaves: {leaf: dict(defs, reps, num_slots,
    values, width, offsets, chars, physical_type[, flags, logical])} with dense values as the decoders give them."""
    columns, structs = {}, {}
    for lf, c in leaves.items():
        node = [n for n in schema_nodes if n.leaf == lf][0]
        list_def, elem_def = leaf_thresholds(schema_nodes, lf)
        strings = c.get("offsets") is not None
        m = M.assemble(c["defs"], c["reps"], node.max_def, list_def, elem_def,
                       None if strings else c["values"], 0 if strings else c["width"], c.get("offsets"),
                       num_slots=c["num_slots"])
        columns[lf] = NestedColumn([(o, v, nc) for o, v, nc, _ in m.levels], m.leaf_validity, m.num_leaf,
                                   values=m.leaf_values, value_width=0 if strings else c["width"],
                                   chars=c.get("chars"), leaf_offsets=m.leaf_offsets,
                                   physical_type=c["physical_type"], flags=c.get("flags", 0), num_rows=m.num_rows)
    for lf, todo in T.structs_by_leaf(root).items():
        c = leaves[lf]
        elem_def = leaf_thresholds(schema_nodes, lf)[1]
        for p in todo:
            structs[p.node] = struct_bits(c["defs"], c["reps"], p.depth, p.struct_def, elem_def, c["num_slots"])
    info = {lf: dict(logical=c["logical"]) for lf, c in leaves.items() if c.get("logical") is not None}
    return T.build(root, columns, structs, num_rows, info)


def oracle_leaves(pf, rg, selected=None):
    """The `leaves` of host_tree from a file's chunks, decoded by the CPU oracle."""
    from oracle import pyoracle as O
    out = {}
    for c in (selected if selected is not None else range(pf.num_columns)):
        ch = O.decode_chunk(pf.host_job(rg, c)[0])
        assert ch.status == 0
        desc = pf.columns[c].desc
        strings = ch.offsets is not None
        out[c] = dict(defs=ch.def_levels if ch.def_levels is not None else np.zeros(ch.num_slots, np.uint8),
                      reps=ch.rep_levels, num_slots=ch.num_slots,
                      values=None if strings else ch.values, width=ch.value_width, offsets=ch.offsets,
                      chars=ch.values if strings else None, physical_type=desc.physical_type, flags=desc.flags,
                      logical=pf.logical_types[c])
    return out


def encode(x):
    """pyarrow's to_pylist with strings as bytes and nothing else changed."""
    if isinstance(x, str):
        return x.encode()
    if isinstance(x, dict):
        return {k: encode(v) for k, v in x.items()}
    if isinstance(x, list):
        return [encode(v) for v in x]
    if isinstance(x, tuple):
        return tuple(encode(v) for v in x)
    return x


# ---------------------------------------------------------------- a file no writer here emits
# A legacy 2-level list, `optional group <name> (LIST) { repeated int32 array; }`, written by
# hand: one uncompressed V1 data page of PLAIN values per column, and a footer in thrift's compact
# protocol with just the fields a reader needs.

def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _zz(v):
    return _varint((v << 1) ^ (v >> 63))


class _Struct:
    """A thrift compact struct under construction: fields in increasing id order."""
    I32, I64, BINARY, LIST, STRUCT = 5, 6, 8, 9, 12

    def __init__(self):
        self.b, self.last = bytearray(), 0

    def _head(self, fid, t):
        d = fid - self.last
        self.b += bytes([(d << 4) | t]) if 0 < d <= 15 else bytes([t]) + _zz(fid)
        self.last = fid

    def i32(self, fid, v):
        self._head(fid, self.I32)
        self.b += _zz(v)
        return self

    def i64(self, fid, v):
        self._head(fid, self.I64)
        self.b += _zz(v)
        return self

    def string(self, fid, s):
        self._head(fid, self.BINARY)
        self.b += _varint(len(s)) + s
        return self

    def struct(self, fid, s):
        self._head(fid, self.STRUCT)
        self.b += s.done()
        return self

    def list(self, fid, etype, items):
        """items: encoded elements (structs: done(); i32: _zz; strings: length + bytes)."""
        self._head(fid, self.LIST)
        n = len(items)
        self.b += bytes([(n << 4) | etype]) if n < 15 else bytes([0xf0 | etype]) + _varint(n)
        for it in items:
            self.b += it
        return self

    def done(self):
        return bytes(self.b) + b"\x00"


def legacy_list_file(columns, num_rows):
    """A one-row-group file of legacy 2-level lists.  columns: [(name, def uint8, rep uint8,
    int32 values)], each an `optional group name (LIST) { repeated int32 array; }` (max_def 2:
    0 a null list, 1 an empty one)."""
    from gen import pqwrite as W
    S = _Struct
    body, chunks = bytearray(b"PAR1"), []
    schema = [S().string(4, b"schema").i32(5, len(columns)).done()]
    for name, defs, reps, vals in columns:
        schema.append(S().i32(3, OPT).string(4, name.encode()).i32(5, 1).i32(6, 3).done())   # converted type LIST
        schema.append(S().i32(1, 1).i32(3, REP).string(4, b"array").done())                   # INT32
        lv = b""
        for levels, width in ((reps, 1), (defs, 2)):
            h = W.hybrid_encode(np.asarray(levels, np.uint8), width)
            lv += len(h).to_bytes(4, "little") + h
        page = lv + np.asarray(vals, "<i4").tobytes()
        head = S().i32(1, 0).i32(2, len(page)).i32(3, len(page)).struct(
            5, S().i32(1, len(defs)).i32(2, 0).i32(3, 3).i32(4, 3)).done()
        at = len(body)
        body += head + page
        size = len(head) + len(page)
        meta = S().i32(1, 1).list(2, S.I32, [_zz(0), _zz(3)]).list(
            3, S.BINARY, [_varint(len(p)) + p for p in (name.encode(), b"array")]).i32(4, 0).i64(
            5, len(defs)).i64(6, size).i64(7, size).i64(9, at)
        chunks.append((S().i64(2, at).struct(3, meta).done(), size))
    rg = S().list(1, S.STRUCT, [c for c, _ in chunks]).i64(2, sum(s for _, s in chunks)).i64(3, num_rows).done()
    footer = S().i32(1, 1).list(2, S.STRUCT, schema).i64(3, num_rows).list(4, S.STRUCT, [rg]).done()
    return bytes(body) + footer + len(footer).to_bytes(4, "little") + b"PAR1"
