"""Nested columns in Arrow layout: the thresholds of a leaf's list depths and
the host view of pqg_assemble_nested's outputs (include/pqgpu.h, K8).

The reference assembles a nested value by recursion, Column.getData /
getNextData (schema.go:171-264) over ColumnStore.get (data_store.go:158-203),
one slot at a time.  pqg_assemble_nested evaluates the same walk for every
slot at once and leaves, per list depth, offsets and a validity bitmap, and
for the leaf a validity bitmap and values (or string offsets).  This module
derives the definition-level thresholds that call needs from the schema, and
holds what it returns."""
import numpy as np

from . import abi

REQUIRED, OPTIONAL, REPEATED = 0, 1, 2


def leaf_path(schema_nodes, leaf):
    """The schema nodes from the root's child down to leaf column `leaf`, from
    the depth-first records of pqg_file_schema_node."""
    it = iter(schema_nodes)

    def take(path):
        n = next(it)
        here = path + [n]
        if n.num_children > 0:
            found = None
            for _ in range(n.num_children):
                found = take(here) or found
            return found
        return here if n.leaf == leaf else None

    found = None
    while found is None:
        try:
            found = take([])
        except StopIteration:
            raise KeyError("no leaf %d in the schema" % leaf)
    return found


def leaf_thresholds(schema_nodes, leaf):
    """(list_def[], elem_def[]) of leaf column `leaf`, one entry per REPEATED
    node on its path (depth k = the k-th of them).

    OPTIONAL and REPEATED nodes each add one definition level.  elem_def[k] is
    the level reached at the k-th REPEATED node: the list at depth k has an
    element.  list_def[k] is elem_def[k] - 1 when an OPTIONAL node lies between
    the previous REPEATED node (or the root) and this one, and the list is then
    null when it or any optional ancestor since its parent list is null;
    otherwise the list cannot be null and list_def[k] = elem_def[k-1]
    (elem_def[0] = 0).

    Struct validity is not part of these thresholds: a leaf under an optional
    struct reports def == max_def as its validity, so in this per-leaf view a
    null struct and a null field of a present struct both come out as a null
    leaf.  pqgpu.tree (FileReader.read_row_group_tree) tells them apart: it
    adds the structs' own bitmaps (pqg_assemble_structs) and nests the leaves
    under their structs, lists and maps."""
    list_def, elem_def = [], []
    level, prev_elem, optional_since = 0, 0, False
    for n in leaf_path(schema_nodes, leaf):
        if n.repetition == OPTIONAL:
            level += 1
            optional_since = True
        elif n.repetition == REPEATED:
            level += 1
            elem_def.append(level)
            list_def.append(level - 1 if optional_since else prev_elem)
            prev_elem, optional_since = level, False
    return list_def, elem_def


def _bits(bitmap, n):
    return np.unpackbits(np.asarray(bitmap).view(np.uint8), bitorder="little")[:n].astype(bool)


_FIXED_DTYPE = {abi.INT32: np.int32, abi.INT64: np.int64, abi.FLOAT: np.float32, abi.DOUBLE: np.float64}


def fixed_pylist(raw, physical_type, width, flags, n):
    """n fixed-width values of `width` bytes in `raw` as Python values."""
    raw = np.asarray(raw, dtype=np.uint8)
    if physical_type == abi.BOOLEAN:
        return [bool(x) for x in raw]
    if physical_type in _FIXED_DTYPE:
        dt = _FIXED_DTYPE[physical_type]
        if flags & 1:
            dt = {np.int32: np.uint32, np.int64: np.uint64}.get(dt, dt)
        return raw.view(dt).tolist()
    b = raw.tobytes()
    return [b[i * width:(i + 1) * width] for i in range(n)]


class NestedColumn:
    """One leaf column in Arrow layout.

    levels         [(offsets int32[entries + 1], validity bits (uint32 words), null_count)],
                   outermost list first; offsets index the next depth's
                   entries, the last depth's index the leaf slots
    leaf_validity  validity bits of the leaf slots (uint32 words)
    values         fixed-width leaf: num_leaf x value_width bytes, nulls zeroed
    chars, leaf_offsets   byte-array leaf: int64[num_leaf + 1] into chars
    dictionary     a leaf that kept its dictionary (FileReader's read_dictionary): the
                   pqgpu.reader.Dictionary; values are then int32 keys (value_width 4, a null
                   slot's key is 0 and means nothing), else None
    """

    def __init__(self, levels, leaf_validity, num_leaf, values=None, value_width=0, chars=None, leaf_offsets=None,
                 physical_type=None, flags=0, num_rows=None, dictionary=None):
        self.dictionary = dictionary
        self.levels = levels
        self.leaf_validity = leaf_validity
        self.num_leaf = num_leaf
        self.values = values
        self.value_width = value_width
        self.chars = chars
        self.leaf_offsets = leaf_offsets
        self.physical_type = physical_type
        self.flags = flags
        self.num_rows = num_rows if num_rows is not None else (len(levels[0][0]) - 1 if levels else num_leaf)

    def leaf_pylist(self):
        """The leaf slots as Python values, None for a null."""
        valid = _bits(self.leaf_validity, self.num_leaf)
        if self.dictionary is not None:  # keys: looked up, so the result is the materialised leaf's
            entries = self.dictionary.pylist(self.physical_type, self.flags)
            keys = np.asarray(self.values, dtype=np.uint8).view("<i4")[:self.num_leaf].tolist()
            return [entries[k] if ok else None for k, ok in zip(keys, valid)]
        if self.leaf_offsets is not None:
            b = np.asarray(self.chars, dtype=np.uint8).tobytes()
            o = np.asarray(self.leaf_offsets)
            return [b[o[i]:o[i + 1]] if valid[i] else None for i in range(self.num_leaf)]
        vals = fixed_pylist(self.values, self.physical_type, self.value_width, self.flags, self.num_leaf)
        return [v if ok else None for v, ok in zip(vals, valid)]

    def to_pylist(self):
        """Python rows rebuilt from the buffers alone: nested lists, None for a
        null list or a null leaf."""
        cur = self.leaf_pylist()
        for offsets, validity, _ in reversed(self.levels):
            o = np.asarray(offsets).tolist()
            valid = _bits(validity, len(o) - 1)
            cur = [cur[o[i]:o[i + 1]] if valid[i] else None for i in range(len(o) - 1)]
        return cur
