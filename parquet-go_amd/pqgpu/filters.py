"""Filter planning on the host: pyarrow's DNF `filters=` into pqg_filter steps, and row-group
pruning from footer statistics.

A filter is a list of (column, op, value) tuples (AND) or a list of such lists (OR of ANDs).
Operators: == = != < <= > >= in not in, and (col, "is", None) / (col, "is not", None).
Comparison orders are pqg_filter's (include/pqgpu.h): signed / unsigned integers, IEEE floats
(NaN fails everything but !=), BOOLEAN 0 < 1, byte strings unsigned lexicographic.  A null row
fails every comparison and passes only `is null`.

With a column's abi.LogicalType, literals may be typed (pqgpu.logical): decimal.Decimal / int on a
DECIMAL column, datetime / np.datetime64 on a TIMESTAMP column, date on a DATE column; and a
FIXED_LEN_BYTE_ARRAY decimal (abi.COL_SIGNED_BE in the description's flags) orders as the
big-endian two's complement it is.
"""
import struct

import numpy as np

from . import abi

_OPS = {"==": abi.OP_EQ, "=": abi.OP_EQ, "!=": abi.OP_NE, "<": abi.OP_LT, "<=": abi.OP_LE, ">": abi.OP_GT,
        ">=": abi.OP_GE}
_NUM = {abi.INT32: ("<i", "<I"), abi.INT64: ("<q", "<Q"), abi.FLOAT: ("<f", "<f"), abi.DOUBLE: ("<d", "<d")}


class Term:
    """One (column, op, value) of a filter.  op: an abi.OP_* code, or "in" / "not in" with
    `values` a list."""

    def __init__(self, column, op, values):
        self.column = column
        self.op = op
        self.values = values

    def steps(self):
        """The pqg_filter calls of this term alone: [(op code, value, combine)].  `in` is OR-ed ==,
        `not in` AND-ed !=; an empty `in` selects nothing, an empty `not in` every non-null row."""
        if self.op == "in":
            if not self.values:
                return [(abi.OP_IS_NULL, None, abi.COMBINE_SET), (abi.OP_NOT_NULL, None, abi.COMBINE_AND)]
            return [(abi.OP_EQ, v, abi.COMBINE_OR if k else abi.COMBINE_SET) for k, v in enumerate(self.values)]
        if self.op == "not in":
            if not self.values:
                return [(abi.OP_NOT_NULL, None, abi.COMBINE_SET)]
            return [(abi.OP_NE, v, abi.COMBINE_AND if k else abi.COMBINE_SET) for k, v in enumerate(self.values)]
        return [(self.op, self.values, abi.COMBINE_SET)]

    def chains_with_and(self):
        """Its steps may follow another term's in one bitmap, each with COMBINE_AND."""
        return self.op != "in" or not self.values


def parse(filters):
    """pyarrow's DNF into [[Term]]: the OR of the inner lists' ANDs."""
    if filters is None:
        return None
    if not isinstance(filters, (list, tuple)) or not filters:
        raise ValueError("filters: a non-empty list of (column, op, value) tuples or of lists of them")
    if isinstance(filters[0], (list, tuple)) and len(filters[0]) == 3 and isinstance(filters[0][0], str):
        filters = [filters]
    out = []
    for conj in filters:
        if not isinstance(conj, (list, tuple)) or not conj:
            raise ValueError("filters: an empty conjunction")
        terms = []
        for t in conj:
            if not isinstance(t, (list, tuple)) or len(t) != 3 or not isinstance(t[0], str):
                raise ValueError("filters: %r is not a (column, op, value) tuple" % (t,))
            col, op, val = t
            op = " ".join(str(op).lower().split())
            if op in ("is", "is not"):
                if val is not None:
                    raise ValueError("filters: %r takes None" % op)
                terms.append(Term(col, abi.OP_IS_NULL if op == "is" else abi.OP_NOT_NULL, None))
            elif op in ("in", "not in"):
                if isinstance(val, (str, bytes)) or not hasattr(val, "__iter__"):
                    raise ValueError("filters: %r takes a collection" % op)
                terms.append(Term(col, op, list(val)))
            elif op in _OPS:
                terms.append(Term(col, _OPS[op], val))
            else:
                raise ValueError("filters: unknown operator %r" % (t[1],))
        out.append(terms)
    return out


def columns_of(dnf):
    """The column names a parsed filter reads, in first-use order."""
    seen = []
    for conj in dnf:
        for t in conj:
            if t.column not in seen:
                seen.append(t.column)
    return seen


def signed_be(desc, logical=None):
    """The column orders as big-endian two's complement: a FIXED_LEN_BYTE_ARRAY with
    abi.COL_SIGNED_BE, or with a DECIMAL logical type."""
    if desc.physical_type != abi.FIXED_LEN_BYTE_ARRAY:
        return False
    return bool(desc.flags & abi.COL_SIGNED_BE) or (logical is not None and logical.kind == abi.LT_DECIMAL)


def literal(desc, value, logical=None):
    """`value` as the bytes pqg_filter takes for a column of this description (its physical
    little-endian layout).  With the column's `logical` type: a decimal.Decimal or int on a
    DECIMAL column is the scaled integer (type_length big-endian bytes for FLBA, the int32 / int64
    for integer-backed decimals), a datetime / np.datetime64 on a TIMESTAMP column and a date on a
    DATE column the integer in the column's unit.  ValueError when the value does not fit the
    type or is not exact at the column's scale or unit."""
    from .logical import typed_literal
    typed = typed_literal(desc, value, logical)
    if typed is not None:
        return typed
    t = desc.physical_type
    if t in _NUM:
        fmt = _NUM[t][1 if desc.flags & abi.COL_UNSIGNED else 0]
        if t in (abi.INT32, abi.INT64):
            if isinstance(value, (float, np.floating)) and float(value) != int(value):
                raise ValueError("a fractional literal for an integer column")
            value = int(value)
        else:
            value = float(value)
        try:
            return struct.pack(fmt, value)
        except (struct.error, OverflowError) as e:
            raise ValueError("literal %r does not fit the column's type" % (value,)) from e
    if t == abi.BOOLEAN:
        return b"\x01" if value else b"\x00"
    if t in (abi.BYTE_ARRAY, abi.FIXED_LEN_BYTE_ARRAY, abi.INT96):
        b = value.encode() if isinstance(value, str) else bytes(value)
        return b
    raise ValueError("no literal for physical type %d" % t)


def compare(desc, a, b, logical=None):
    """pqg_filter's order of two values given as physical bytes: -1, 0, 1, or None when they are
    unordered (a NaN) or not values of the type (a wrong length).  A FIXED_LEN_BYTE_ARRAY that is
    signed_be() orders as big-endian two's complement."""
    t = desc.physical_type
    if t in _NUM:
        fmt = _NUM[t][1 if desc.flags & abi.COL_UNSIGNED else 0]
        if len(a) != struct.calcsize(fmt) or len(b) != struct.calcsize(fmt):
            return None
        x, y = struct.unpack(fmt, a)[0], struct.unpack(fmt, b)[0]
        if x != x or y != y:
            return None
    elif t == abi.BOOLEAN:
        if len(a) != 1 or len(b) != 1:
            return None
        x, y = a[0], b[0]
    elif t == abi.BYTE_ARRAY:
        x, y = bytes(a), bytes(b)
    elif t == abi.FIXED_LEN_BYTE_ARRAY:
        if desc.type_length < 1 or len(a) != desc.type_length or len(b) != desc.type_length:
            return None
        x, y = bytes(a), bytes(b)
        if signed_be(desc, logical):
            x, y = bytes([x[0] ^ 0x80]) + x[1:], bytes([y[0] ^ 0x80]) + y[1:]
    else:
        return None
    return -1 if x < y else 1 if x > y else 0


def _rules_out(desc, op, lit, lo, hi, logical=None):
    """No value in [lo, hi] passes `op lit` (all as physical bytes); False when in doubt."""
    is_float = desc.physical_type in (abi.FLOAT, abi.DOUBLE)
    c_lo, c_hi = compare(desc, lo, lit, logical), compare(desc, hi, lit, logical)  # bound against the literal
    if c_lo is None or c_hi is None:
        return False
    if op == abi.OP_EQ:
        return c_lo > 0 or c_hi < 0
    if op == abi.OP_NE:  # a NaN row passes != and is in no statistic
        return not is_float and c_lo == 0 and c_hi == 0
    if op == abi.OP_LT:
        return c_lo >= 0
    if op == abi.OP_LE:
        return c_lo > 0
    if op == abi.OP_GT:
        return c_hi <= 0
    if op == abi.OP_GE:
        return c_hi < 0
    return False


def term_rules_out(desc, term, stats, rows, logical=None):
    """The statistics of a chunk of `rows` rows show that no row passes `term`.  stats: (min bytes
    or None, max bytes or None, null_count or -1).  Conservative: a missing or odd statistic
    rules nothing out.  logical: the column's abi.LogicalType, for typed literals and the signed
    order of FLBA decimals; with it a BYTE_ARRAY decimal's statistics rule nothing out."""
    lo, hi, nulls = stats
    if desc.max_rep > 0 or rows <= 0:
        return False
    nulls_known = 0 <= nulls <= rows
    if term.op == abi.OP_IS_NULL:
        return nulls_known and nulls == 0
    all_null = nulls_known and nulls == rows
    if all_null:
        return True  # only `is null` passes a null row
    if term.op == abi.OP_NOT_NULL:
        return False
    if lo is None or hi is None:
        return False
    if logical is not None and logical.kind == abi.LT_DECIMAL and desc.physical_type == abi.BYTE_ARRAY:
        return False  # values of different lengths: neither byte order is the numeric one
    if desc.physical_type in (abi.FLOAT, abi.DOUBLE):
        # a NaN bound says nothing; writers disagree on the sign of a zero bound
        fmt = _NUM[desc.physical_type][0]
        if len(lo) != struct.calcsize(fmt) or len(hi) != struct.calcsize(fmt):
            return False
        x, y = struct.unpack(fmt, lo)[0], struct.unpack(fmt, hi)[0]
        if x != x or y != y:
            return False
        if x == 0:
            lo = struct.pack(fmt, -0.0)
        if y == 0:
            hi = struct.pack(fmt, 0.0)
    c = compare(desc, lo, hi, logical)
    if c is None or c > 0:
        return False
    try:
        if term.op == "in":
            return all(_rules_out(desc, abi.OP_EQ, literal(desc, v, logical), lo, hi, logical) for v in term.values)
        if term.op == "not in":
            return any(_rules_out(desc, abi.OP_NE, literal(desc, v, logical), lo, hi, logical) for v in term.values)
        return _rules_out(desc, term.op, literal(desc, term.values, logical), lo, hi, logical)
    except (ValueError, TypeError, AttributeError):
        return False
