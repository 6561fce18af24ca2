"""A row group as one Arrow column tree: structs, lists and maps over the leaves
of pqgpu.nested.

plan() reads the shape from the schema alone (pqg_file_schema_node and
pqg_file_schema_node_kind): which groups are lists, maps and structs, which of
them can be null, and where each takes its buffers from.  A list takes its
offsets and validity from one depth of pqg_assemble_nested's output for the
first selected leaf below it (its representative leaf); a nullable struct takes
its validity from pqg_assemble_structs on the levels of its representative
leaf, with (depth, struct_def) = the group's (max_rep, max_def).  build() puts
the downloaded buffers into StructNode / ListNode / LeafNode, which give Python
rows (to_pylist) or pyarrow arrays (to_arrow) from the buffers alone.

The reference returns a row as nested maps, Column.getData (schema.go:235-264);
the shapes here follow the backward-compatibility rules of the format's
LogicalTypes document for LIST and MAP groups."""
import numpy as np

from . import abi
from .nested import OPTIONAL, REPEATED, _bits


# ------------------------------------------------------------------ the plan (schema only)

class PlanLeaf:
    kind = "leaf"

    def __init__(self, name, nullable, leaf, node, max_def, max_rep):
        self.name, self.nullable, self.leaf, self.node = name, nullable, leaf, node
        self.max_def, self.max_rep = max_def, max_rep
        self.rep_leaf = leaf

    def shape(self):
        return ("leaf", self.name, self.nullable)


class PlanStruct:
    """depth R = lists above the struct, struct_def D = the level at which it is present
    (pqg_struct_level); both mean something only for a nullable struct."""
    kind = "struct"

    def __init__(self, name, nullable, depth, struct_def, children, node):
        self.name, self.nullable, self.depth, self.struct_def = name, nullable, depth, struct_def
        self.children, self.node = children, node
        self.rep_leaf = children[0].rep_leaf if children else -1

    def shape(self):
        return ("struct", self.name, self.nullable, [c.shape() for c in self.children])


class PlanList:
    """depth k (1-based): level[k - 1] of the representative leaf's nested export holds this
    list's offsets and validity; elem_def: the level of its REPEATED node."""
    kind = "list"

    def __init__(self, name, nullable, is_map, depth, elem_def, child, node):
        self.name, self.nullable, self.is_map, self.depth, self.elem_def = name, nullable, is_map, depth, elem_def
        self.child, self.node = child, node
        self.rep_leaf = child.rep_leaf

    def shape(self):
        return ("map" if self.is_map else "list", self.name, self.nullable, self.child.shape())


class _Raw:
    def __init__(self, index, n, kind):
        self.index, self.kind = index, kind
        self.name = n.name.decode() if isinstance(n.name, bytes) else n.name
        self.repetition, self.leaf, self.max_def, self.max_rep = n.repetition, n.leaf, n.max_def, n.max_rep
        self.children = []


def _raw_tree(schema_nodes, schema_kinds):
    it = iter(range(len(schema_nodes)))

    def take():
        i = next(it)
        r = _Raw(i, schema_nodes[i], schema_kinds[i])
        for _ in range(schema_nodes[i].num_children):
            r.children.append(take())
        return r

    top = []
    while True:
        try:
            top.append(take())
        except StopIteration:
            return top


def _leaf(raw, sel, nullable):
    return PlanLeaf(raw.name, nullable, raw.leaf, raw.index, raw.max_def, raw.max_rep) if raw.leaf in sel else None


def _struct(raw, sel, nullable):
    kids = [f for f in (_field(c, sel) for c in raw.children) if f is not None]
    return PlanStruct(raw.name, nullable, raw.max_rep, raw.max_def, kids, raw.index) if kids else None


def _element(rep, sel):
    """The REPEATED node itself as a list element: a leaf, or a non-nullable struct of its fields."""
    return _leaf(rep, sel, False) if rep.leaf >= 0 else _struct(rep, sel, False)


def _field(raw, sel):
    if raw.repetition == REPEATED:  # no LIST / MAP group above it: a non-nullable list of itself
        elem = _element(raw, sel)
        return PlanList(raw.name, False, False, raw.max_rep, raw.max_def, elem, raw.index) if elem else None
    if raw.leaf >= 0:
        return _leaf(raw, sel, raw.repetition == OPTIONAL)
    nullable = raw.repetition == OPTIONAL
    one = raw.children[0] if len(raw.children) == 1 and raw.children[0].repetition == REPEATED else None
    if one is not None and raw.kind == abi.NODE_LIST:
        if one.leaf < 0 and len(one.children) == 1 and one.name != "array" and one.name != raw.name + "_tuple":
            elem = _field(one.children[0], sel)  # 3-level: the element is the grandchild
        else:
            elem = _element(one, sel)            # legacy 2-level: the repeated child is the element
        return PlanList(raw.name, nullable, False, one.max_rep, one.max_def, elem, raw.index) if elem else None
    if one is not None and raw.kind == abi.NODE_MAP and one.leaf < 0:
        elem = _struct(one, sel, False)
        return PlanList(raw.name, nullable, True, one.max_rep, one.max_def, elem, raw.index) if elem else None
    return _struct(raw, sel, nullable)


def walk(node):
    """Every plan node below and including `node`, parents first."""
    yield node
    for c in (node.children if node.kind == "struct" else [node.child] if node.kind == "list" else []):
        yield from walk(c)


def plan(schema_nodes, schema_kinds, selected_leaves=None):
    """The shape of the selected leaves' tree (None: every leaf), from the schema alone: a
    non-nullable PlanStruct named "" whose children are the top-level fields.  A group with no
    selected leaf below it is left out.  A leaf under more than abi.MAX_LIST_DEPTH lists raises
    PqgError(UNSUPPORTED)."""
    from .reader import PqgError
    sel = set(selected_leaves) if selected_leaves is not None else {n.leaf for n in schema_nodes if n.leaf >= 0}
    for n in schema_nodes:
        if n.leaf in sel and n.max_rep > abi.MAX_LIST_DEPTH:
            name = n.name.decode() if isinstance(n.name, bytes) else n.name
            raise PqgError(abi.STATUS_CODES["UNSUPPORTED"], "column %s: %d list depths (at most %d)"
                           % (name, n.max_rep, abi.MAX_LIST_DEPTH))
    kids = [f for f in (_field(r, sel) for r in _raw_tree(schema_nodes, schema_kinds)) if f is not None]
    return PlanStruct("", False, 0, 0, kids, -1)


def structs_by_leaf(root):
    """{representative leaf: [nullable PlanStruct, ...]}: the pqg_assemble_structs calls of a plan."""
    out = {}
    for n in walk(root):
        if n.kind == "struct" and n.nullable:
            out.setdefault(n.rep_leaf, []).append(n)
    return out


def list_leaves(root):
    """The leaves whose nested export supplies some list's offsets and validity."""
    return {n.rep_leaf for n in walk(root) if n.kind == "list"}


# ------------------------------------------------------------------ the tree (buffers)

def _buf(a):
    import pyarrow as pa
    return pa.py_buffer(np.ascontiguousarray(a).view(np.uint8).tobytes()) if a is not None else None


class LeafNode:
    """A leaf: the NestedColumn of pqg_assemble_nested (`column`: leaf validity, values or string
    offsets over chars, dictionary), its abi.LogicalType and whether its values went through
    pqg_convert (`converted`: decimals as 16 / 32 bytes, INT96 as int64 in `unit`)."""

    def __init__(self, name, nullable, column, logical=None, converted=False, unit=abi.UNIT_NANOS):
        self.name, self.nullable, self.column = name, nullable, column
        self.logical, self.converted, self.unit = logical, converted, unit
        self.length = column.num_leaf

    def to_pylist(self):
        return self.column.leaf_pylist()

    def _type(self):
        import pyarrow as pa
        c, lt = self.column, self.logical
        kind = lt.kind if lt is not None else abi.LT_NONE
        t = c.physical_type
        if self.converted:
            if t == abi.INT64:
                return pa.timestamp({v: k for k, v in abi.UNITS.items()}[self.unit])
            width = c.dictionary.value_width if c.dictionary is not None else c.value_width
            return (pa.decimal128 if width == 16 else pa.decimal256)(lt.precision, lt.scale)
        if t == abi.BOOLEAN:
            return pa.bool_()
        if t in (abi.INT32, abi.INT64):
            bits = 32 if t == abi.INT32 else 64
            if kind == abi.LT_INTEGER and lt.bit_width in (8, 16, 32, 64):
                return getattr(pa, ("int%d" if lt.is_signed else "uint%d") % lt.bit_width)()
            if kind == abi.LT_DATE and t == abi.INT32:
                return pa.date32()
            if kind == abi.LT_TIMESTAMP and t == abi.INT64:
                unit = {abi.UNIT_MILLIS: "ms", abi.UNIT_MICROS: "us", abi.UNIT_NANOS: "ns"}[lt.unit]
                return pa.timestamp(unit, tz="UTC" if lt.utc else None)
            if kind == abi.LT_TIME:
                return pa.time32("ms") if t == abi.INT32 else pa.time64("us" if lt.unit == abi.UNIT_MICROS else "ns")
            return getattr(pa, ("uint%d" if c.flags & 1 else "int%d") % bits)()
        if t == abi.FLOAT:
            return pa.float32()
        if t == abi.DOUBLE:
            return pa.float64()
        if t == abi.BYTE_ARRAY:
            return pa.string() if kind in (abi.LT_STRING, abi.LT_ENUM, abi.LT_JSON) else pa.binary()
        width = c.dictionary.value_width if c.dictionary is not None else c.value_width
        return pa.binary(width)  # FIXED_LEN_BYTE_ARRAY and raw INT96

    @staticmethod
    def _values(typ, n, validity, values, offsets, chars):
        """n values of arrow type `typ` from this module's buffers."""
        import pyarrow as pa
        if offsets is not None:
            o = np.asarray(offsets, dtype=np.int64)
            if len(o) and o[-1] > np.iinfo(np.int32).max:
                typ = pa.large_string() if typ == pa.string() else pa.large_binary()
            else:
                o = o.astype(np.int32)
            return pa.Array.from_buffers(typ, n, [validity, _buf(o), _buf(chars if chars is not None else
                                                                        np.zeros(0, np.uint8))])
        raw = np.asarray(values, dtype=np.uint8)
        if typ == pa.bool_():
            raw = np.packbits(raw[:n] != 0, bitorder="little")
        return pa.Array.from_buffers(typ, n, [validity, _buf(raw)])

    def to_arrow(self):
        import pyarrow as pa
        c, n = self.column, self.column.num_leaf
        validity = _buf(c.leaf_validity) if self.nullable else None
        typ = self._type()
        if c.dictionary is not None:
            d = c.dictionary
            keys = pa.Array.from_buffers(pa.int32(), n, [validity, _buf(np.asarray(c.values, np.uint8)[:4 * n])])
            vals = d.table().reshape(-1) if d.value_width else d.values
            return pa.DictionaryArray.from_arrays(keys, self._values(typ, d.count, None, vals, d.offsets, d.values))
        return self._values(typ, n, validity, c.values, c.leaf_offsets, c.chars)


class StructNode:
    """validity: uint32 words (None: the struct cannot be null), null_count, length, children in
    schema order."""

    def __init__(self, name, nullable, validity, null_count, length, children):
        self.name, self.nullable, self.validity, self.null_count = name, nullable, validity, null_count
        self.length, self.children = length, children

    def to_pylist(self):
        cols = [(c.name, c.to_pylist()) for c in self.children]
        valid = _bits(self.validity, self.length) if self.validity is not None else np.ones(self.length, bool)
        return [{name: col[i] for name, col in cols} if valid[i] else None for i in range(self.length)]

    def to_arrow(self):
        import pyarrow as pa
        kids = [c.to_arrow() for c in self.children]
        typ = pa.struct([pa.field(c.name, a.type, nullable=c.nullable) for c, a in zip(self.children, kids)])
        return pa.Array.from_buffers(typ, self.length, [_buf(self.validity)],
                                     null_count=self.null_count if self.validity is not None else 0, children=kids)


class ListNode:
    """offsets: int32[length + 1] into the child's slots; validity: uint32 words (None: the list
    cannot be null); is_map: the child is the non-nullable struct of a map's key and value."""

    def __init__(self, name, nullable, offsets, validity, null_count, is_map, child):
        self.name, self.nullable, self.offsets, self.validity = name, nullable, offsets, validity
        self.null_count, self.is_map, self.child = null_count, is_map, child
        self.length = len(offsets) - 1

    def to_pylist(self):
        cur = self.child.to_pylist()
        if self.is_map:
            names = [c.name for c in self.child.children]
            cur = [tuple(e[k] for k in names) for e in cur]
        o = np.asarray(self.offsets).tolist()
        valid = _bits(self.validity, self.length) if self.validity is not None else np.ones(self.length, bool)
        return [cur[o[i]:o[i + 1]] if valid[i] else None for i in range(self.length)]

    def to_arrow(self):
        import pyarrow as pa
        kid = self.child.to_arrow()
        if self.is_map and len(self.child.children) == 2:
            k, v = self.child.children
            typ = pa.map_(kid.type.field(0).type, pa.field(v.name, kid.type.field(1).type, nullable=v.nullable))
        else:
            typ = pa.list_(pa.field(self.child.name, kid.type, nullable=self.child.nullable))
        return pa.Array.from_buffers(typ, self.length, [_buf(self.validity), _buf(np.asarray(self.offsets, np.int32))],
                                     null_count=self.null_count if self.validity is not None else 0, children=[kid])


def build(root, columns, structs, num_rows, leaf_info=None):
    """The tree of a plan from its buffers.  columns: {leaf: NestedColumn} (list levels are read
    from the representative leaves'); structs: {PlanStruct.node: (validity words, null_count,
    num_entries)} for the nullable structs; leaf_info: {leaf: LeafNode keyword arguments}."""
    leaf_info = leaf_info or {}

    def make(p):
        if p.kind == "leaf":
            return LeafNode(p.name, p.nullable, columns[p.leaf], **leaf_info.get(p.leaf, {}))
        if p.kind == "list":
            offsets, validity, nulls = columns[p.rep_leaf].levels[p.depth - 1]
            return ListNode(p.name, p.nullable, offsets, validity if p.nullable else None,
                            nulls if p.nullable else 0, p.is_map, make(p.child))
        kids = [make(c) for c in p.children]
        if p.nullable:
            validity, nulls, entries = structs[p.node]
            return StructNode(p.name, True, validity, int(nulls), int(entries), kids)
        return StructNode(p.name, False, None, 0, kids[0].length if p.node >= 0 else num_rows, kids)

    return make(root)
