"""pqgpu — MI355X (gfx950) Parquet column-chunk decoder behind parquet-go's page-decode surface.

The decode runs in hand-written HIP kernels (parquet-go_amd/csrc, libpqgpu.so);
this package is the host-side binding (ctypes over the C ABI in include/pqgpu.h).
"""
from . import abi  # noqa: F401
from .nested import NestedColumn, leaf_thresholds  # noqa: F401
from .tree import LeafNode, ListNode, StructNode  # noqa: F401
from .reader import (DecodedColumn, Dictionary, FileReader, GpuDecoder, ParquetFile, PqgError, chunk_ranges,  # noqa: F401
                     chunk_span, decode_spans, device_job, span_jobs)
