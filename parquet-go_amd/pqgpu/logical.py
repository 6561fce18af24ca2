"""Logical types on the host: which leaves pqg_convert converts and how, and Python values
(decimal.Decimal, datetime, date, np.datetime64) as the integers a column of a logical type stores.

A DECIMAL of precision p is stored as the integer value * 10**scale: big-endian two's complement in
FIXED_LEN_BYTE_ARRAY / BYTE_ARRAY, or an INT32 / INT64.  Arrow holds it as 16 (p <= 38) or 32
little-endian bytes.  An INT96 timestamp is (nanoseconds of the day, julian day)."""
import datetime
import decimal

import numpy as np

from . import abi

MAX_PRECISION = 76
_EPOCH = datetime.datetime(1970, 1, 1)
_EPOCH_DATE = datetime.date(1970, 1, 1)


class Conversion:
    """One pqg_convert call shape: kind, in_width (0: BYTE_ARRAY decimals), out_width, unit."""

    def __init__(self, kind, in_width, out_width, unit=abi.UNIT_NONE):
        self.kind, self.in_width, self.out_width, self.unit = kind, in_width, out_width, unit

    @property
    def physical_type(self):
        """The physical type whose layout the converted values have (for Python views of them)."""
        return abi.INT64 if self.kind == abi.CONV_INT96_TIME else abi.FIXED_LEN_BYTE_ARRAY


def decimal_width(precision):
    """Arrow's bytes per decimal of this precision: 16 (decimal128) or 32 (decimal256)."""
    return 16 if precision <= 38 else 32


def conversion(desc, lt, int96_unit=abi.UNIT_NANOS):
    """The Conversion of a leaf (its abi.ColumnDesc and abi.LogicalType), or None for a leaf that
    stays as it is: INT96 leaves, and DECIMAL leaves of precision 1..76 on FLBA (type_length 1 up to
    the output width), BYTE_ARRAY, INT32 and INT64."""
    t = desc.physical_type
    if t == abi.INT96:
        return Conversion(abi.CONV_INT96_TIME, 12, 8, int96_unit)
    if lt is None or lt.kind != abi.LT_DECIMAL or not 1 <= lt.precision <= MAX_PRECISION:
        return None
    ow = decimal_width(lt.precision)
    if t == abi.FIXED_LEN_BYTE_ARRAY:
        return Conversion(abi.CONV_DECIMAL_BE, desc.type_length, ow) if 1 <= desc.type_length <= ow else None
    if t == abi.BYTE_ARRAY:
        return Conversion(abi.CONV_DECIMAL_BE, 0, ow)
    if t in (abi.INT32, abi.INT64):
        return Conversion(abi.CONV_DECIMAL_INT, abi.FIXED_WIDTH[t], ow)
    return None


def int96_zero(unit):
    """What twelve zero bytes convert to (a dictionary's nil entry): julian day 0, as int64 in `unit`."""
    per_day = 86400 * abi.UNIT_PER_SECOND[unit]
    v = (-2440588 * per_day) & (2 ** 64 - 1)
    return v - 2 ** 64 if v >= 2 ** 63 else v


def decimal_unscaled(value, scale):
    """value * 10**scale as an int; ValueError when that is no integer (or no finite number)."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer, decimal.Decimal)):
        raise ValueError("a decimal column takes decimal.Decimal or int literals, not %r" % (value,))
    d = decimal.Decimal(int(value)) if not isinstance(value, decimal.Decimal) else value
    if not d.is_finite():
        raise ValueError("literal %r is not finite" % (value,))
    with decimal.localcontext() as ctx:
        ctx.prec = 200
        s = d.scaleb(scale)
        i = s.to_integral_value(rounding=decimal.ROUND_FLOOR)
        if i != s:
            raise ValueError("literal %r is not exact at scale %d" % (value, scale))
        return int(i)


def decimal_bytes(unscaled, width):
    """An unscaled decimal as `width` big-endian two's-complement bytes; ValueError when it does not fit."""
    try:
        return int(unscaled).to_bytes(width, "big", signed=True)
    except OverflowError as e:
        raise ValueError("literal does not fit %d bytes" % width) from e


def _to_unit(ns, unit, what):
    per = 10 ** 9 // abi.UNIT_PER_SECOND[unit]
    if ns % per:
        raise ValueError("literal %r is not exact in the column's unit" % (what,))
    return ns // per


def timestamp_value(value, unit):
    """A datetime.datetime (naive: UTC) or np.datetime64 as the integer since the epoch in `unit`
    (abi.UNIT_*); ValueError when it is not exact in that unit."""
    if isinstance(value, np.datetime64):
        if np.isnat(value):
            raise ValueError("NaT is no literal")
        name = np.datetime_data(value.dtype)[0]
        per_ns = {"ns": 1, "us": 10 ** 3, "ms": 10 ** 6, "s": 10 ** 9, "m": 60 * 10 ** 9, "h": 3600 * 10 ** 9,
                  "D": 86400 * 10 ** 9}.get(name)
        if per_ns is None:
            raise ValueError("no timestamp from a datetime64[%s]" % name)
        return _to_unit(int(value.astype(np.int64)) * per_ns, unit, value)
    if isinstance(value, datetime.datetime):
        if value.tzinfo is not None:
            value = value.astimezone(datetime.timezone.utc).replace(tzinfo=None)
        d = value - _EPOCH
        return _to_unit(((d.days * 86400 + d.seconds) * 10 ** 6 + d.microseconds) * 1000, unit, value)
    raise ValueError("a timestamp column takes datetime.datetime or np.datetime64 literals, not %r" % (value,))


def date_value(value):
    """A datetime.date (or a datetime / np.datetime64 at midnight) as days since the epoch."""
    if isinstance(value, np.datetime64) or isinstance(value, datetime.datetime):
        ns = timestamp_value(value, abi.UNIT_NANOS)
        if ns % (86400 * 10 ** 9):
            raise ValueError("literal %r is not a whole day" % (value,))
        return ns // (86400 * 10 ** 9)
    if isinstance(value, datetime.date):
        return (value - _EPOCH_DATE).days
    raise ValueError("a date column takes datetime.date literals, not %r" % (value,))


def typed_literal(desc, value, lt):
    """`value` as the bytes pqg_filter takes when the column's logical type decides them, or None
    when it does not (the physical rules of filters.literal apply)."""
    t = desc.physical_type
    if lt is None:
        return None
    if lt.kind == abi.LT_DECIMAL and isinstance(value, (int, np.integer, decimal.Decimal)) and \
            not isinstance(value, bool):
        u = decimal_unscaled(value, lt.scale)
        if t == abi.FIXED_LEN_BYTE_ARRAY and desc.type_length >= 1:
            return decimal_bytes(u, desc.type_length)
        if t in (abi.INT32, abi.INT64):
            w = abi.FIXED_WIDTH[t]
            return decimal_bytes(u, w)[::-1]
        raise ValueError("no decimal literal for physical type %d" % t)
    if lt.kind == abi.LT_TIMESTAMP and t == abi.INT64 and isinstance(value, (datetime.datetime, np.datetime64)):
        return decimal_bytes(timestamp_value(value, lt.unit), 8)[::-1]
    if lt.kind == abi.LT_DATE and t == abi.INT32 and isinstance(value, (datetime.date, np.datetime64)):
        return decimal_bytes(date_value(value), 4)[::-1]
    return None
