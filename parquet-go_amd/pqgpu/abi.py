"""ctypes mirror of include/pqgpu.h (the C ABI of libpqgpu).

Only plain structs and enums live here; no library is loaded by this module.
"""
import ctypes as C

# parquet.thrift enums
BOOLEAN, INT32, INT64, INT96, FLOAT, DOUBLE, BYTE_ARRAY, FIXED_LEN_BYTE_ARRAY = range(8)
ENC_PLAIN = 0
ENC_PLAIN_DICTIONARY = 2
ENC_RLE = 3
ENC_BIT_PACKED = 4
ENC_DELTA_BINARY_PACKED = 5
ENC_DELTA_LENGTH_BYTE_ARRAY = 6
ENC_DELTA_BYTE_ARRAY = 7
ENC_RLE_DICTIONARY = 8
ENC_BYTE_STREAM_SPLIT = 9
CODEC_UNCOMPRESSED, CODEC_SNAPPY, CODEC_GZIP = 0, 1, 2
CODEC_ZSTD = 6
CODEC_LZ4_RAW = 7
PAGE_DATA, PAGE_INDEX, PAGE_DICTIONARY, PAGE_DATA_V2 = 0, 1, 2, 3

STATUS = {
    0: "OK",
    -1: "EOF",
    -2: "THRIFT",
    -3: "PAGE_HEADER",
    -4: "SIZE",
    -5: "SNAPPY",
    -6: "RLE",
    -7: "DICT_INDEX",
    -8: "BIT_WIDTH",
    -9: "DELTA",
    -10: "UNSUPPORTED",
    -11: "DICT_PAGE",
    -12: "BYTE_ARRAY",
    -13: "LEVELS",
    -14: "FIXED_LEN",
    -15: "GZIP",
    -16: "ZSTD",
    -17: "LZ4",
    -18: "CRC",
    -19: "NOT_DICT",
    -20: "CAPACITY",
    -21: "INVALID_ARG",
    -22: "HIP",
    -23: "METADATA",
    -24: "NOT_BUILT",
    -25: "INDEX",
}
OK = 0
ERR_CAPACITY = -20
STATUS_CODES = {v: k for k, v in STATUS.items()}

FIXED_WIDTH = {BOOLEAN: 1, INT32: 4, INT64: 8, INT96: 12, FLOAT: 4, DOUBLE: 8}

# pqg_column_desc.flags
COL_UNSIGNED, COL_KEEP_DICT = 1, 2
COL_SIGNED_BE = 4  # pqg_filter only: FLBA values order as big-endian two's complement (a DECIMAL)


class ColumnDesc(C.Structure):
    _fields_ = [
        ("physical_type", C.c_int32),
        ("type_length", C.c_int32),
        ("max_def", C.c_int32),
        ("max_rep", C.c_int32),
        ("codec", C.c_int32),
        ("flags", C.c_int32),
    ]


class ChunkJob(C.Structure):
    _fields_ = [
        ("col", ColumnDesc),
        ("data", C.c_void_p),
        ("data_len", C.c_int64),
        ("total_compressed_size", C.c_int64),
        ("data_page_offset", C.c_int64),
        ("num_values_hint", C.c_int64),
        ("total_uncompressed_size", C.c_int64),
        ("has_dict_page_offset", C.c_int32),
        ("quirks", C.c_int32),
    ]


QUIRK_Q1_PAGE_NILS, QUIRK_Q2_DICT_ALIAS = 1, 2


class PageLoc(C.Structure):
    """pqg_page_loc (include/pqgpu.h): one page of a located decode."""
    _fields_ = [("offset", C.c_int64), ("size", C.c_int32), ("reserved", C.c_int32), ("first_row", C.c_int64)]


class ChunkPages(C.Structure):
    """pqg_chunk_pages (include/pqgpu.h): the page list of one job (n == 0: the job is scanned)."""
    _fields_ = [("locs", C.POINTER(PageLoc)), ("n", C.c_int32), ("reserved", C.c_int32)]


class PageJob(C.Structure):
    """pqg_page_job (include/pqgpu.h)."""
    _fields_ = [("col", ColumnDesc), ("page", C.c_void_p), ("page_len", C.c_int64), ("dict_page", C.c_void_p),
                ("dict_page_len", C.c_int64)]


class ChunkResult(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("error_page", C.c_int32),
        ("num_pages", C.c_int32),
        ("value_width", C.c_int32),
        ("col_flags", C.c_int32),
        ("reserved", C.c_int32),
        ("num_slots", C.c_int64),
        ("num_values", C.c_int64),
        ("values_bytes", C.c_int64),
        ("def_levels", C.c_void_p),
        ("rep_levels", C.c_void_p),
        ("values", C.c_void_p),
        ("offsets", C.c_void_p),
    ]


class Dictionary(C.Structure):
    """pqg_dictionary (include/pqgpu.h): the dictionary of a COL_KEEP_DICT job, device pointers."""
    _fields_ = [
        ("values", C.c_void_p),
        ("offsets", C.c_void_p),
        ("count", C.c_int64),
        ("values_bytes", C.c_int64),
        ("value_width", C.c_int32),
        ("nil_entry", C.c_int32),
        ("page", C.c_int32),
        ("reserved", C.c_int32),
    ]


class PageInfo(C.Structure):
    _fields_ = [
        ("header_offset", C.c_int64),
        ("payload_offset", C.c_int64),
        ("slot_offset", C.c_int64),
        ("value_offset", C.c_int64),
        ("page_type", C.c_int32),
        ("encoding", C.c_int32),
        ("num_values", C.c_int32),
        ("not_null", C.c_int32),
        ("compressed_size", C.c_int32),
        ("uncompressed_size", C.c_int32),
        ("def_len", C.c_int32),
        ("rep_len", C.c_int32),
        ("def_encoding", C.c_int32),
        ("rep_encoding", C.c_int32),
        ("status", C.c_int32),
        ("flags", C.c_int32),
    ]


CRC_NONE, CRC_VERIFIED, CRC_MISMATCH, CRC_NOT_CHECKED = 0, 1, 2, 3


class PageCrc(C.Structure):
    """pqg_page_crc (include/pqgpu.h): PageHeader.crc of one page and what the GPU computed."""
    _fields_ = [("stored", C.c_uint32), ("computed", C.c_uint32), ("state", C.c_int32), ("reserved", C.c_int32)]


class ColumnInfo(C.Structure):
    _fields_ = [("desc", ColumnDesc), ("path", C.c_char * 256)]


class SchemaNode(C.Structure):
    _fields_ = [("name", C.c_char * 128), ("repetition", C.c_int32), ("num_children", C.c_int32),
                ("leaf", C.c_int32), ("max_def", C.c_int32), ("max_rep", C.c_int32), ("reserved", C.c_int32)]


class ChunkMeta(C.Structure):
    _fields_ = [
        ("start", C.c_int64),
        ("total_compressed_size", C.c_int64),
        ("total_uncompressed_size", C.c_int64),
        ("data_page_offset", C.c_int64),
        ("num_values", C.c_int64),
        ("has_dict_page_offset", C.c_int32),
        ("codec", C.c_int32),
        ("type", C.c_int32),
        ("reserved", C.c_int32),
    ]


class AssembleArgs(C.Structure):
    """pqg_assemble_args (include/pqgpu.h, K8)."""
    _fields_ = [("def_levels", C.c_void_p), ("rep_levels", C.c_void_p), ("values", C.c_void_p),
                ("num_slots", C.c_int64), ("max_def", C.c_int32), ("boundary_level", C.c_int32),
                ("value_width", C.c_int32), ("reserved", C.c_int32),
                ("validity", C.c_void_p), ("values_spaced", C.c_void_p), ("offsets", C.c_void_p),
                ("num_valid", C.c_int64), ("null_count", C.c_int64), ("num_boundaries", C.c_int64)]


class ListArgs(C.Structure):
    """pqg_list_args (include/pqgpu.h, K8 list export)."""
    _fields_ = [("def_levels", C.c_void_p), ("rep_levels", C.c_void_p), ("values", C.c_void_p),
                ("num_slots", C.c_int64), ("max_def", C.c_int32), ("list_def", C.c_int32),
                ("elem_def", C.c_int32), ("value_width", C.c_int32),
                ("list_validity", C.c_void_p), ("list_offsets", C.c_void_p), ("elem_validity", C.c_void_p),
                ("elem_values", C.c_void_p),
                ("num_rows", C.c_int64), ("num_elements", C.c_int64), ("num_valid", C.c_int64),
                ("null_lists", C.c_int64)]


MAX_LIST_DEPTH = 4


class NestedLevel(C.Structure):
    """pqg_nested_level (include/pqgpu.h, K8 nested export)."""
    _fields_ = [("list_def", C.c_int32), ("elem_def", C.c_int32), ("validity", C.c_void_p),
                ("offsets", C.c_void_p), ("num_entries", C.c_int64), ("null_count", C.c_int64)]


class NestedArgs(C.Structure):
    """pqg_nested_args (include/pqgpu.h, K8 nested export)."""
    _fields_ = [("def_levels", C.c_void_p), ("rep_levels", C.c_void_p), ("values", C.c_void_p),
                ("value_offsets", C.c_void_p), ("num_slots", C.c_int64),
                ("max_def", C.c_int32), ("depth", C.c_int32), ("value_width", C.c_int32), ("reserved", C.c_int32),
                ("level", NestedLevel * MAX_LIST_DEPTH),
                ("leaf_validity", C.c_void_p), ("leaf_values", C.c_void_p), ("leaf_offsets", C.c_void_p),
                ("num_rows", C.c_int64), ("num_leaf", C.c_int64), ("num_valid", C.c_int64)]


MAX_STRUCTS = 8


class StructLevel(C.Structure):
    """pqg_struct_level (include/pqgpu.h, K8 struct export)."""
    _fields_ = [("depth", C.c_int32), ("struct_def", C.c_int32), ("validity", C.c_void_p),
                ("num_entries", C.c_int64), ("null_count", C.c_int64)]


class StructArgs(C.Structure):
    """pqg_struct_args (include/pqgpu.h, K8 struct export)."""
    _fields_ = [("def_levels", C.c_void_p), ("rep_levels", C.c_void_p), ("num_slots", C.c_int64),
                ("max_def", C.c_int32), ("depth", C.c_int32), ("elem_def", C.c_int32 * MAX_LIST_DEPTH),
                ("num_structs", C.c_int32), ("reserved", C.c_int32), ("st", StructLevel * MAX_STRUCTS)]


# pqg_file_schema_node_kind
NODE_PLAIN, NODE_LIST, NODE_MAP = 0, 1, 2


class ChunkStats(C.Structure):
    """pqg_chunk_stats (include/pqgpu.h): ColumnMetaData.statistics of one chunk."""
    _fields_ = [("min_value", C.c_void_p), ("max_value", C.c_void_p), ("min_len", C.c_int32),
                ("max_len", C.c_int32), ("null_count", C.c_int64)]


class IndexRanges(C.Structure):
    """pqg_index_ranges (include/pqgpu.h): where a chunk's page indexes lie in the file (length 0: none)."""
    _fields_ = [("offset_index_offset", C.c_int64), ("column_index_offset", C.c_int64),
                ("offset_index_length", C.c_int32), ("column_index_length", C.c_int32)]


# pqg_filter operators and combine modes
OP_EQ, OP_NE, OP_LT, OP_LE, OP_GT, OP_GE, OP_IS_NULL, OP_NOT_NULL = range(8)
COMBINE_SET, COMBINE_AND, COMBINE_OR = range(3)


class FilterArgs(C.Structure):
    """pqg_filter_args (include/pqgpu.h, K9s)."""
    _fields_ = [("def_levels", C.c_void_p), ("values", C.c_void_p), ("offsets", C.c_void_p),
                ("num_rows", C.c_int64), ("num_values", C.c_int64), ("values_bytes", C.c_int64),
                ("col", ColumnDesc), ("op", C.c_int32), ("combine", C.c_int32),
                ("literal", C.c_void_p), ("literal_len", C.c_int64), ("dictionary", C.POINTER(Dictionary)),
                ("bitmap", C.c_void_p), ("num_selected", C.c_int64), ("num_valid", C.c_int64)]


class SelectArgs(C.Structure):
    """pqg_select_args (include/pqgpu.h, K9s)."""
    _fields_ = [("bitmap", C.c_void_p), ("def_levels", C.c_void_p), ("values", C.c_void_p), ("offsets", C.c_void_p),
                ("num_rows", C.c_int64), ("num_values", C.c_int64), ("values_bytes", C.c_int64),
                ("max_def", C.c_int32), ("value_width", C.c_int32),
                ("out_def_levels", C.c_void_p), ("out_values", C.c_void_p), ("out_offsets", C.c_void_p),
                ("rows_out", C.c_int64), ("values_out", C.c_int64), ("bytes_out", C.c_int64)]


# pqg_logical_type.kind / .unit
(LT_NONE, LT_STRING, LT_ENUM, LT_DECIMAL, LT_DATE, LT_TIME, LT_TIMESTAMP, LT_INTEGER, LT_JSON, LT_BSON, LT_UUID,
 LT_FLOAT16, LT_OTHER) = range(13)
UNIT_NONE, UNIT_SECONDS, UNIT_MILLIS, UNIT_MICROS, UNIT_NANOS = range(5)
UNITS = {"s": UNIT_SECONDS, "ms": UNIT_MILLIS, "us": UNIT_MICROS, "ns": UNIT_NANOS}
UNIT_PER_SECOND = {UNIT_SECONDS: 1, UNIT_MILLIS: 10 ** 3, UNIT_MICROS: 10 ** 6, UNIT_NANOS: 10 ** 9}


class LogicalType(C.Structure):
    """pqg_logical_type (include/pqgpu.h): the logical type of a leaf column."""
    _fields_ = [("kind", C.c_int32), ("precision", C.c_int32), ("scale", C.c_int32), ("unit", C.c_int32),
                ("utc", C.c_int32), ("bit_width", C.c_int32), ("is_signed", C.c_int32), ("converted_type", C.c_int32)]


# pqg_convert kinds
CONV_DECIMAL_BE, CONV_DECIMAL_INT, CONV_INT96_TIME = range(3)


class ConvertArgs(C.Structure):
    """pqg_convert_args (include/pqgpu.h, K10)."""
    _fields_ = [("values", C.c_void_p), ("offsets", C.c_void_p), ("num_values", C.c_int64), ("values_bytes", C.c_int64),
                ("kind", C.c_int32), ("in_width", C.c_int32), ("out_width", C.c_int32), ("unit", C.c_int32),
                ("out", C.c_void_p), ("num_bad", C.c_int64)]


def status_name(code):
    return STATUS.get(int(code), str(code))
