"""Loader for libpqgpu.so (the HIP product library, built in-tree)."""
import ctypes as C
import os

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(HERE), "csrc", "libpqgpu.so")
# diagnostics only: PQG_LIB may name the -DPQG_PROFILE build (libpqgpu_prof.so)
LIB_PATH = os.environ.get("PQG_LIB") or LIB_PATH

_lib = None


def lib():
    """Load libpqgpu.so; raise loudly if it has not been built (no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libpqgpu.so not built (%s): run __graft_entry__.build() or make -C parquet-go_amd/csrc"
                           % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    P, I, I64 = C.c_void_p, C.c_int, C.c_int64
    sig = {
        "pqg_ctx_create": ([I, C.POINTER(P)], I),
        "pqg_ctx_destroy": ([P], None),
        "pqg_status_string": ([I], C.c_char_p),
        "pqg_device_alloc": ([P, I64, C.POINTER(P)], I),
        "pqg_device_free": ([P, P], I),
        "pqg_memcpy_h2d": ([P, P, P, I64], I),
        "pqg_memcpy_d2h": ([P, P, P, I64], I),
        "pqg_decode_chunks_async": ([P, C.POINTER(abi.ChunkJob), I], I),
        "pqg_sync": ([P, C.POINTER(abi.ChunkResult), I], I),
        "pqg_decode_chunks": ([P, C.POINTER(abi.ChunkJob), I, C.POINTER(abi.ChunkResult)], I),
        "pqg_decode_chunks_located_async": ([P, C.POINTER(abi.ChunkJob), C.POINTER(abi.ChunkPages), I], I),
        "pqg_decode_chunks_located": ([P, C.POINTER(abi.ChunkJob), C.POINTER(abi.ChunkPages), I,
                                       C.POINTER(abi.ChunkResult)], I),
        "pqg_file_chunk_index": ([P, I, I, C.POINTER(abi.IndexRanges)], I),
        "pqg_parse_offset_index": ([C.c_char_p, I64, C.POINTER(abi.PageLoc), I], I),
        "pqg_column_index_parse": ([C.c_char_p, I64, C.POINTER(P)], I),
        "pqg_column_index_pages": ([P], I),
        "pqg_column_index_page": ([P, I, C.POINTER(abi.ChunkStats), C.POINTER(C.c_int32)], I),
        "pqg_column_index_boundary_order": ([P], I),
        "pqg_column_index_free": ([P], None),
        "pqg_range_bitmap": ([P, C.POINTER(I64), I, I64, P], I),
        "pqg_get_pages": ([P, I, C.POINTER(abi.PageInfo), I], I),
        "pqg_get_dictionary": ([P, I, C.POINTER(abi.Dictionary)], I),
        "pqg_last_timings": ([P, C.POINTER(C.c_float), I], I),
        "pqg_set_timing": ([P, I], I),
        "pqg_set_verify_crc": ([P, I], I),
        "pqg_get_page_crcs": ([P, I, C.POINTER(abi.PageCrc), I], I),
        "pqg_crc32": ([P, P, I64, C.POINTER(C.c_uint32)], I),
        "pqg_last_crc_ms": ([P, C.POINTER(C.c_float)], I),
        "pqg_debug_job": ([P, I, C.POINTER(I64), I], I),
        "pqg_debug_counters": ([P, C.POINTER(C.c_uint64), I], I),
        "pqg_bench_decode": ([P, C.POINTER(abi.ChunkJob), I, I, C.POINTER(C.c_float), C.POINTER(C.c_float), I], I),
        "pqg_assemble": ([P, C.POINTER(abi.AssembleArgs)], I),
        "pqg_assemble_list": ([P, C.POINTER(abi.ListArgs)], I),
        "pqg_assemble_nested": ([P, C.POINTER(abi.NestedArgs)], I),
        "pqg_assemble_structs": ([P, C.POINTER(abi.StructArgs)], I),
        "pqg_last_assemble_ms": ([P, C.POINTER(C.c_float)], I),
        "pqg_decode_page": ([P, C.POINTER(abi.PageJob), C.POINTER(abi.ChunkResult)], I),
        "pqg_block_decompress": ([P, I, C.c_char_p, I64, P, I64, C.POINTER(I64)], I),
        "pqg_pack_levels": ([P, P, I64, I, P], I),
        "pqg_file_open": ([C.c_char_p, I64, C.POINTER(P)], I),
        "pqg_file_open_tail": ([C.c_char_p, I64, C.c_char_p, I64, I64, C.POINTER(P)], I),
        "pqg_file_close": ([P], None),
        "pqg_file_num_columns": ([P], I),
        "pqg_file_num_row_groups": ([P], I),
        "pqg_file_num_rows": ([P], I64),
        "pqg_file_row_group_rows": ([P, I], I64),
        "pqg_file_column": ([P, I, C.POINTER(abi.ColumnInfo)], I),
        "pqg_file_chunk": ([P, I, I, C.POINTER(abi.ChunkMeta)], I),
        "pqg_file_num_schema_nodes": ([P], I),
        "pqg_file_schema_node": ([P, I, C.POINTER(abi.SchemaNode)], I),
        "pqg_file_schema_node_kind": ([P, I], I),
        "pqg_file_chunk_stats": ([P, I, I, C.POINTER(abi.ChunkStats)], I),
        "pqg_filter": ([P, C.POINTER(abi.FilterArgs)], I),
        "pqg_select": ([P, C.POINTER(abi.SelectArgs)], I),
        "pqg_last_filter_ms": ([P, C.POINTER(C.c_float)], I),
        "pqg_convert": ([P, C.POINTER(abi.ConvertArgs)], I),
        "pqg_last_convert_ms": ([P, C.POINTER(C.c_float)], I),
        "pqg_file_column_logical": ([P, I, C.POINTER(abi.LogicalType)], I),
    }
    for name, (args, res) in sig.items():
        # a library named by PQG_LIB may be an older build (A/B runs against a parent's library):
        # what it lacks fails at the call; the tree's own library must have every symbol
        fn = getattr(L, name, None) if os.environ.get("PQG_LIB") else getattr(L, name)
        if fn is None:
            continue
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


EXPORTED = [
    "pqg_ctx_create", "pqg_ctx_destroy", "pqg_status_string", "pqg_device_alloc", "pqg_device_free",
    "pqg_memcpy_h2d", "pqg_memcpy_d2h", "pqg_decode_chunks_async", "pqg_sync", "pqg_decode_chunks",
    "pqg_get_pages", "pqg_last_timings", "pqg_set_timing", "pqg_debug_job", "pqg_debug_counters", "pqg_bench_decode", "pqg_assemble",
    "pqg_assemble_list", "pqg_assemble_nested", "pqg_last_assemble_ms", "pqg_decode_page", "pqg_block_decompress", "pqg_pack_levels", "pqg_file_open", "pqg_file_open_tail",
    "pqg_file_close", "pqg_set_verify_crc", "pqg_get_page_crcs", "pqg_crc32", "pqg_last_crc_ms",
    "pqg_file_num_columns", "pqg_file_num_row_groups", "pqg_file_num_rows", "pqg_file_row_group_rows",
    "pqg_file_column", "pqg_file_chunk", "pqg_file_num_schema_nodes", "pqg_file_schema_node",
    "pqg_get_dictionary", "pqg_file_chunk_stats", "pqg_filter", "pqg_select", "pqg_last_filter_ms",
    "pqg_convert", "pqg_last_convert_ms", "pqg_file_column_logical",
    "pqg_assemble_structs", "pqg_file_schema_node_kind",
    "pqg_decode_chunks_located_async", "pqg_decode_chunks_located", "pqg_range_bitmap",
    "pqg_file_chunk_index", "pqg_parse_offset_index", "pqg_column_index_parse", "pqg_column_index_pages",
    "pqg_column_index_page", "pqg_column_index_boundary_order", "pqg_column_index_free",
]
