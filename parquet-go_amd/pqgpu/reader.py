"""Host-side mirror of parquet-go's reader surface over libpqgpu.

parquet-go (fraugster/parquet-go v0.2.1) reads a file with
    NewFileReader(r, columns...)      file_reader.go:27-48
    FileReader.readRowGroup / PreLoad file_reader.go:51-98  → readRowGroup chunk_reader.go:404-431
and decodes each selected column chunk with readChunk → readPages →
readPageData (chunk_reader.go:206-402).  This module keeps those names and
meanings; the page decode itself runs in the HIP kernels of libpqgpu.
Column projection follows schema.isSelected (schema.go:296-312): an empty
selection reads every column.
"""
import ctypes as C
import os

import numpy as np

from . import abi
from ._lib import lib


class PqgError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = int(code)
        super().__init__("%s: %s (%d)" % (what, abi.status_name(code), code))


def _check(rc, what):
    if rc != 0:
        raise PqgError(rc, what)


class PageIndex:
    """The page index of one column chunk (ParquetFile.page_index).

    locations      [(offset, size, first_row)] per page of the OffsetIndex: absolute file offset of the
                   page header, header + body bytes, first row of the page in its row group
    null_pages, min_values, max_values, null_counts, boundary_order: the ColumnIndex, None when the
                   chunk has only an OffsetIndex (null_counts also when the index has none); a null
                   page's bounds are None, the others physical little-endian bytes or raw strings"""

    def __init__(self, locations, rows, column=None):
        self.locations = locations
        self.rows = rows  # of the row group
        self.null_pages = self.min_values = self.max_values = self.null_counts = self.boundary_order = None
        if column is not None:
            self.null_pages, self.min_values, self.max_values, self.null_counts, self.boundary_order = column

    def page_rows(self, page):
        """[first, end) rows of a page."""
        end = self.locations[page + 1][2] if page + 1 < len(self.locations) else self.rows
        return self.locations[page][2], end

    def stats(self, page):
        """(min, max, null_count) of a page, as filters.term_rules_out takes a chunk's: (None, None, -1)
        without a ColumnIndex; an all-null page reports its row count as its null count."""
        if self.null_pages is None:
            return None, None, -1
        nulls = self.null_counts[page] if self.null_counts is not None else -1
        if self.null_pages[page]:
            lo, hi = self.page_rows(page)
            return None, None, hi - lo
        return self.min_values[page], self.max_values[page], nulls


class ParquetFile:
    """Footer + schema of a parquet file (readFileMetaData file_meta.go:14-62).

    ParquetFile(data) holds the whole file in host memory; ParquetFile.open(path)
    reads only the first 4 bytes and the footer, and chunk bytes are fetched by
    byte range on demand (read_range), as readChunk seeks to each chunk
    (chunk_reader.go:332-340)."""

    def __init__(self, data=None, *, _path=None):
        L = lib()
        h = C.c_void_p()
        self.path = _path
        if _path is None:
            if isinstance(data, np.ndarray) and data.dtype == np.uint8 and data.ndim == 1 and data.flags.c_contiguous:
                self.data = data  # a large file (the bench's C5 shard): no second copy
                self._buf = data
            else:
                self.data = bytes(data)
                self._buf = np.frombuffer(self.data, dtype=np.uint8)
            self.size = len(self.data)
            ptr = self._buf.ctypes.data if self.size else None
            _check(L.pqg_file_open(C.cast(ptr, C.c_char_p) if ptr else b"", self.size, C.byref(h)), "pqg_file_open")
        else:
            self.data = None
            self._buf = None
            self.size = os.path.getsize(_path)
            with open(_path, "rb") as f:
                head = f.read(4)
                f.seek(max(0, self.size - 8))
                last8 = f.read(8)
                fl = int.from_bytes(last8[:4], "little", signed=True) if len(last8) == 8 else 0
                n = min(self.size, max(fl, 0) + 8)
                f.seek(self.size - n)
                tail = f.read(n)
            _check(L.pqg_file_open_tail(head, len(head), tail, len(tail), self.size, C.byref(h)), "pqg_file_open_tail")
        self._h = h
        self.num_columns = L.pqg_file_num_columns(h)
        self.num_row_groups = L.pqg_file_num_row_groups(h)
        self.num_rows = L.pqg_file_num_rows(h)
        self.columns = []
        for i in range(self.num_columns):
            ci = abi.ColumnInfo()
            _check(L.pqg_file_column(h, i, C.byref(ci)), "pqg_file_column")
            self.columns.append(ci)
        self.logical_types = []  # abi.LogicalType per column, parallel to `columns`
        # an older library named by PQG_LIB (A/B runs against a parent's build) has no logical types
        known = hasattr(L, "pqg_file_column_logical")
        for i in range(self.num_columns):
            lt = abi.LogicalType(converted_type=-1)
            if known:
                _check(L.pqg_file_column_logical(h, i, C.byref(lt)), "pqg_file_column_logical")
            self.logical_types.append(lt)
        self.schema_nodes = []  # depth first, below the root (pqg_file_schema_node)
        for i in range(L.pqg_file_num_schema_nodes(h)):
            sn = abi.SchemaNode()
            _check(L.pqg_file_schema_node(h, i, C.byref(sn)), "pqg_file_schema_node")
            self.schema_nodes.append(sn)
        # abi.NODE_* per schema node, parallel to `schema_nodes` (an older library named by PQG_LIB has none)
        kinds = getattr(L, "pqg_file_schema_node_kind", None)
        self.schema_kinds = [kinds(h, i) if kinds else abi.NODE_PLAIN for i in range(len(self.schema_nodes))]

    @classmethod
    def open(cls, path):
        return cls(_path=path)

    def read_range(self, lo, hi):
        """Bytes [lo, hi) of the file (shorter at its end)."""
        lo, hi = max(0, lo), min(hi, self.size)
        if hi <= lo:
            return np.zeros(0, np.uint8)
        if self.path is None:
            return self._buf[lo:hi]
        fd = os.open(self.path, os.O_RDONLY)
        try:
            return np.frombuffer(os.pread(fd, hi - lo, lo), dtype=np.uint8)
        finally:
            os.close(fd)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().pqg_file_close(h)
            self._h = None

    def column_index(self, path):
        for i, c in enumerate(self.columns):
            if c.path.decode() == path:
                return i
        raise KeyError(path)

    def row_group_rows(self, rg):
        return lib().pqg_file_row_group_rows(self._h, rg)

    def chunk_meta(self, rg, col):
        m = abi.ChunkMeta()
        _check(lib().pqg_file_chunk(self._h, rg, col, C.byref(m)), "pqg_file_chunk")
        return m

    def chunk_stats(self, rg, col):
        """ColumnMetaData.statistics of a chunk: (min_value, max_value, null_count), the values
        as the physical little-endian bytes the footer holds, None / -1 for what is absent."""
        st = abi.ChunkStats()
        _check(lib().pqg_file_chunk_stats(self._h, rg, col, C.byref(st)), "pqg_file_chunk_stats")
        lo = C.string_at(st.min_value, st.min_len) if st.min_value else None
        hi = C.string_at(st.max_value, st.max_len) if st.max_value else None
        return lo, hi, int(st.null_count)

    def page_index(self, rg, col):
        """The PageIndex of a chunk, None when the file holds no OffsetIndex for it.  The index bytes of
        a row group are fetched with one read_range on first use and cached.  A ColumnIndex that does
        not parse, or whose page count is not the OffsetIndex's, is left out (the locations stand);
        an OffsetIndex that does not parse raises PqgError(METADATA)."""
        cache = self.__dict__.setdefault("_page_index", {})
        if (rg, col) in cache:
            return cache[(rg, col)]
        L = lib()
        raw = self.__dict__.setdefault("_index_bytes", {})
        if rg not in raw:  # one range over every index of the row group
            rs = []
            for c in range(self.num_columns):
                ir = abi.IndexRanges()
                _check(L.pqg_file_chunk_index(self._h, rg, c, C.byref(ir)), "pqg_file_chunk_index")
                rs.append(ir)
            spans = [(r.offset_index_offset, r.offset_index_offset + r.offset_index_length) for r in rs
                     if r.offset_index_length] + \
                    [(r.column_index_offset, r.column_index_offset + r.column_index_length) for r in rs
                     if r.column_index_length]
            lo = min((a for a, _ in spans), default=0)
            hi = max((b for _, b in spans), default=0)
            raw[rg] = (rs, lo, bytes(self.read_range(lo, hi)))
            self.index_bytes_read = getattr(self, "index_bytes_read", 0) + (hi - lo)
        rs, lo, blob = raw[rg]
        ir = rs[col]
        out = None
        if ir.offset_index_length:
            b = blob[ir.offset_index_offset - lo:ir.offset_index_offset - lo + ir.offset_index_length]
            n = L.pqg_parse_offset_index(b, len(b), None, 0)
            if n < 0 or len(b) != ir.offset_index_length:
                raise PqgError(n if n < 0 else abi.STATUS_CODES["METADATA"], "pqg_parse_offset_index")
            locs = (abi.PageLoc * max(n, 1))()
            L.pqg_parse_offset_index(b, len(b), locs, n)
            column = None
            if ir.column_index_length:
                cb = blob[ir.column_index_offset - lo:ir.column_index_offset - lo + ir.column_index_length]
                h = C.c_void_p()
                if L.pqg_column_index_parse(cb, len(cb), C.byref(h)) == 0:
                    try:
                        if L.pqg_column_index_pages(h) == n:
                            nulls, mins, maxs, counts = [], [], [], []
                            for k in range(n):
                                st, np_ = abi.ChunkStats(), C.c_int32()
                                _check(L.pqg_column_index_page(h, k, C.byref(st), C.byref(np_)), "pqg_column_index_page")
                                nulls.append(bool(np_.value))
                                mins.append(C.string_at(st.min_value, st.min_len) if st.min_value else None)
                                maxs.append(C.string_at(st.max_value, st.max_len) if st.max_value else None)
                                counts.append(int(st.null_count))
                            column = (nulls, mins, maxs, counts if all(x >= 0 for x in counts) and n else None,
                                      L.pqg_column_index_boundary_order(h))
                    finally:
                        L.pqg_column_index_free(h)
            out = PageIndex([(int(locs[k].offset), int(locs[k].size), int(locs[k].first_row)) for k in range(n)],
                            self.row_group_rows(rg), column)
        cache[(rg, col)] = out
        return out

    def host_job(self, rg, col):
        """A chunk job whose data pointer is HOST memory (for the CPU oracle)."""
        m = self.chunk_meta(rg, col)
        job = abi.ChunkJob()
        job.col = self.columns[col].desc
        job.col.codec = m.codec
        start = max(0, min(m.start, self.size))
        if self.path is None:
            job.data = self._buf.ctypes.data + start
            job.data_len = self.size - start
        else:  # the chunk's own bytes, kept alive by the job (not the file)
            b = np.ascontiguousarray(self.read_range(start, start + m.total_compressed_size))
            job._keep = b
            job.data = b.ctypes.data if b.nbytes else None
            job.data_len = b.nbytes
        job.total_compressed_size = m.total_compressed_size
        job.data_page_offset = m.data_page_offset - m.start
        job.num_values_hint = m.num_values
        job.total_uncompressed_size = m.total_uncompressed_size
        job.has_dict_page_offset = m.has_dict_page_offset
        return job, m


class Dictionary:
    """The dictionary of a column chunk decoded with abi.COL_KEEP_DICT, on the host.

    values       fixed width: count x value_width entry bytes as the page stores them (fewer for a
                 truncated INT96 page, see nil_entry); byte arrays: the entries' chars back to back
    offsets      byte arrays: int64[count + 1] into values; else None
    value_width  bytes per entry, 0 for byte arrays
    nil_entry    the INT96 entry whose value reads as zero bytes (Q8), -1 if none
    page         index of the dictionary page in the chunk's page list, -1 if the chunk has none"""

    def __init__(self, values, offsets, count, value_width, nil_entry=-1, page=-1):
        self.values = values
        self.offsets = offsets
        self.count = int(count)
        self.value_width = int(value_width)
        self.nil_entry = int(nil_entry)
        self.page = int(page)

    def table(self):
        """Fixed width: the entries as a (count, value_width) uint8 array, nil_entry as zeros."""
        w, n = self.value_width, self.count
        t = np.zeros(n * w, np.uint8)
        raw = np.asarray(self.values, dtype=np.uint8).reshape(-1)[:n * w]
        t[:len(raw)] = raw
        t = t.reshape(n, w)
        if 0 <= self.nil_entry < n:
            t[self.nil_entry] = 0
        return t

    def pylist(self, physical_type, flags=0):
        """The entries as Python values (bytes for byte arrays, FLBA and INT96)."""
        if self.value_width == 0:
            b = np.asarray(self.values, dtype=np.uint8).tobytes()
            o = np.asarray(self.offsets, dtype=np.int64).tolist()
            return [b[o[i]:o[i + 1]] for i in range(self.count)]
        from .nested import fixed_pylist
        return fixed_pylist(self.table().reshape(-1), physical_type, self.value_width, flags, self.count)

    def lookup(self, keys):
        """dictionary[keys] in the layout of a materialised decode: (dense bytes, None) for fixed
        width, (chars, int64 offsets[len(keys) + 1]) for byte arrays."""
        keys = np.asarray(keys).astype(np.int64, copy=False)
        if len(keys) and (keys.min() < 0 or keys.max() >= self.count):
            raise IndexError("dictionary key out of range")
        if self.value_width > 0:
            return np.ascontiguousarray(self.table()[keys]).reshape(-1), None
        o = np.asarray(self.offsets, dtype=np.int64)
        lens = (o[1:] - o[:-1])[keys]
        out = np.zeros(len(keys) + 1, np.int64)
        np.cumsum(lens, out=out[1:])
        src = np.repeat(o[:-1][keys] - out[:-1], lens) + np.arange(out[-1], dtype=np.int64)
        return np.asarray(self.values, dtype=np.uint8)[src], out


class DecodedColumn:
    """Decoded chunk on the host: def/rep levels + dense values[:nn] (readValues outputs).

    A chunk decoded with abi.COL_KEEP_DICT holds its `dictionary` (None when materialised):
    values are then num_values little-endian int32 keys and value_width is 4; materialize()
    gives the column as the decode without the flag lays it out.

    `logical` is the column's abi.LogicalType when the reader ran with convert_logical (None
    otherwise): DECIMAL values (or dictionary entries) are then 16 / 32 little-endian
    two's-complement bytes and INT96 values int64 in the reader's int96_unit, unless the column
    could not be converted (a precision outside 1..76, an FLBA wider than the output) and came
    back raw."""

    def __init__(self, status, error_page, num_slots, num_values, value_width, def_levels, rep_levels, values,
                 pages, offsets=None, dictionary=None, logical=None):
        self.dictionary = dictionary
        self.logical = logical
        self.status = status
        self.error_page = error_page
        self.num_slots = num_slots
        self.num_values = num_values
        self.value_width = value_width
        self.def_levels = def_levels
        self.rep_levels = rep_levels
        self.values = values          # fixed width: dense values; variable length: chars
        self.offsets = offsets        # variable length: int64[num_values + 1]
        self.pages = pages

    def keys(self):
        """The int32 dictionary keys of a column that kept its dictionary."""
        return np.asarray(self.values, dtype=np.uint8).view("<i4")[:self.num_values]

    def materialize(self):
        """The host gather dictionary[keys]: this column in the layout of a decode without
        abi.COL_KEEP_DICT (dense fixed-width bytes, or chars + int64 offsets; the dictionary's
        nil_entry as zero bytes).  A materialised column (or a failed decode) is returned as it is."""
        d = self.dictionary
        if d is None or self.values is None:
            return self
        vals, offs = d.lookup(self.keys())
        return DecodedColumn(self.status, self.error_page, self.num_slots, self.num_values, d.value_width,
                             self.def_levels, self.rep_levels, vals, self.pages, offs, logical=self.logical)


class GpuDecoder:
    """One decode context per GPU (pqg_ctx)."""

    def __init__(self, device=0):
        self.L = lib()
        h = C.c_void_p()
        _check(self.L.pqg_ctx_create(device, C.byref(h)), "pqg_ctx_create")
        self.ctx = h
        self._bufs = []
        self.downloaded_bytes = 0  # D2H bytes so far (d2h)

    def close(self):
        for p in self._bufs:
            self.L.pqg_device_free(self.ctx, p)
        self._bufs = []
        if self.ctx:
            self.L.pqg_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- device memory
    def upload(self, data):
        arr = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        p = C.c_void_p()
        _check(self.L.pqg_device_alloc(self.ctx, max(arr.nbytes, 1), C.byref(p)), "pqg_device_alloc")
        if arr.nbytes:
            _check(self.L.pqg_memcpy_h2d(self.ctx, p, arr.ctypes.data, arr.nbytes), "pqg_memcpy_h2d")
        self._bufs.append(p)
        return p.value

    def upload_ranges(self, buf, ranges):
        """One device buffer holding buf[lo:hi] for each (lo, hi) of `ranges`,
        packed in order, copied range by range (no packed host copy)."""
        total = sum(hi - lo for lo, hi in ranges)
        p = C.c_void_p()
        _check(self.L.pqg_device_alloc(self.ctx, max(total, 1), C.byref(p)), "pqg_device_alloc")
        self._bufs.append(p)
        at = 0
        for lo, hi in ranges:
            if hi > lo:
                src = buf[lo:hi]
                _check(self.L.pqg_memcpy_h2d(self.ctx, C.c_void_p(p.value + at), src.ctypes.data, hi - lo),
                       "pqg_memcpy_h2d")
            at += hi - lo
        return p.value

    def free(self, ptr):
        for i, p in enumerate(self._bufs):
            if p.value == ptr:
                self.L.pqg_device_free(self.ctx, p)
                del self._bufs[i]
                return

    def d2h(self, ptr, nbytes, dtype=np.uint8):
        out = np.empty(max(nbytes, 0), dtype=np.uint8)
        if nbytes > 0:
            _check(self.L.pqg_memcpy_d2h(self.ctx, out.ctypes.data, C.c_void_p(ptr), nbytes), "pqg_memcpy_d2h")
            self.downloaded_bytes += nbytes
        return out.view(dtype) if dtype != np.uint8 else out

    # ---- decode
    def decode_jobs(self, jobs):
        n = len(jobs)
        arr = (abi.ChunkJob * max(n, 1))(*jobs)
        res = (abi.ChunkResult * max(n, 1))()
        _check(self.L.pqg_decode_chunks(self.ctx, arr, n, res), "pqg_decode_chunks")
        return [res[i] for i in range(n)]

    def decode_located(self, jobs, locations):
        """pqg_decode_chunks_located: `locations[i]` lists job i's pages as (offset, size) pairs
        relative to the job's data, in ascending order; None or an empty list: the job is scanned.
        A listed page is decoded where the list says it is and no chunk byte is searched for page
        headers; a page that does not end at offset + size is the read-phase error INDEX (-25)."""
        n = len(jobs)
        arr = (abi.ChunkJob * max(n, 1))(*jobs)
        res = (abi.ChunkResult * max(n, 1))()
        pages = (abi.ChunkPages * max(n, 1))()
        keep = []
        for i, locs in enumerate(locations):
            locs = list(locs or ())
            if locs:
                t = (abi.PageLoc * len(locs))()
                for k, l in enumerate(locs):
                    t[k].offset, t[k].size = int(l[0]), int(l[1])
                keep.append(t)
                pages[i].locs = t
                pages[i].n = len(locs)
        _check(self.L.pqg_decode_chunks_located(self.ctx, arr, pages, n, res), "pqg_decode_chunks_located")
        return [res[i] for i in range(n)]

    def range_bitmap(self, ranges, num_rows, bitmap_ptr):
        """pqg_range_bitmap: the rows of the ascending, disjoint `ranges` ((lo, hi) pairs) as a row bitmap of
        pqg_filter's layout at the device pointer `bitmap_ptr` (4 * ceil(num_rows / 32) bytes)."""
        flat = np.ascontiguousarray(np.asarray(list(ranges), dtype=np.int64).reshape(-1))
        _check(self.L.pqg_range_bitmap(self.ctx, flat.ctypes.data_as(C.POINTER(C.c_int64)), len(flat) // 2, num_rows,
                                       C.c_void_p(bitmap_ptr)), "pqg_range_bitmap")

    def pages(self, job_index, cap=1 << 20):
        buf = (abi.PageInfo * cap)()
        k = self.L.pqg_get_pages(self.ctx, job_index, buf, cap)
        if k < 0:
            raise PqgError(k, "pqg_get_pages")
        return [buf[i] for i in range(k)]

    def dictionary(self, job_index):
        """The dictionary of job `job_index` of the last decode, downloaded (a Dictionary).  The job
        must carry abi.COL_KEEP_DICT (else PqgError INVALID_ARG); valid until the next decode."""
        d = abi.Dictionary()
        _check(self.L.pqg_get_dictionary(self.ctx, job_index, C.byref(d)), "pqg_get_dictionary")
        vals = self.d2h(d.values, d.values_bytes) if d.values else np.zeros(0, np.uint8)
        offs = None
        if d.value_width == 0:
            offs = self.d2h(d.offsets, (d.count + 1) * 8, np.int64) if d.offsets else np.zeros(1, np.int64)
        return Dictionary(vals, offs, d.count, d.value_width, d.nil_entry, d.page)

    # ---- page checksums (PageHeader.crc)
    def set_verify_crc(self, on):
        """Verify PageHeader.crc of every page that carries one, in later decodes on this context
        (off by default; a mismatch is the page's read-phase error PQG_ERR_CRC, -18)."""
        _check(self.L.pqg_set_verify_crc(self.ctx, 1 if on else 0), "pqg_set_verify_crc")

    def page_crcs(self, job_index, cap=1 << 20):
        """[abi.PageCrc] of the pages `pages(job_index)` reports, in the same order."""
        buf = (abi.PageCrc * cap)()
        k = self.L.pqg_get_page_crcs(self.ctx, job_index, buf, cap)
        if k < 0:
            raise PqgError(k, "pqg_get_page_crcs")
        return [buf[i] for i in range(k)]

    def crc32(self, ptr, n):
        """zlib.crc32 of the device bytes [ptr, ptr + n), computed by the page-checksum kernel."""
        out = C.c_uint32()
        _check(self.L.pqg_crc32(self.ctx, C.c_void_p(ptr), n, C.byref(out)), "pqg_crc32")
        return out.value

    def last_crc_ms(self):
        ms = C.c_float()
        _check(self.L.pqg_last_crc_ms(self.ctx, C.byref(ms)), "pqg_last_crc_ms")
        return ms.value

    def debug_job(self, job_index):
        """(serial_walk, candidates, pages, scratch_bytes, pipeline_launches) of the last decode;
        serial_walk is 3 (with 0 candidates) for a located job."""
        out = (C.c_int64 * 5)()
        k = self.L.pqg_debug_job(self.ctx, job_index, out, 5)
        if k < 0:
            raise PqgError(k, "pqg_debug_job")
        return tuple(int(out[i]) for i in range(k))

    def timings(self):
        out = (C.c_float * 16)()
        k = self.L.pqg_last_timings(self.ctx, out, 16)
        return [out[i] for i in range(max(k, 0))]

    def assemble(self, def_ptr, rep_ptr, values_ptr, num_slots, max_def, boundary_level=0, value_width=0,
                 validity=True, spaced=False, offsets=True):
        """K8 on device arrays (e.g. a ChunkResult's levels/values): allocates the
        requested outputs and returns (AssembleArgs, validity_ptr, spaced_ptr,
        offsets_ptr).  Mirrors ColumnStore.get (data_store.go:158-203)."""
        a = abi.AssembleArgs()
        a.def_levels, a.rep_levels, a.values = def_ptr or None, rep_ptr or None, values_ptr or None
        a.num_slots, a.max_def, a.boundary_level, a.value_width = num_slots, max_def, boundary_level, value_width

        def alloc(nbytes):
            p = C.c_void_p()
            _check(self.L.pqg_device_alloc(self.ctx, max(nbytes, 1), C.byref(p)), "pqg_device_alloc")
            self._bufs.append(p)
            return p.value

        vp = alloc((num_slots + 7) // 8) if validity else None
        sp = alloc(num_slots * value_width) if spaced else None
        op = alloc((num_slots + 1) * 8) if offsets else None
        a.validity, a.values_spaced, a.offsets = vp, sp, op
        _check(self.L.pqg_assemble(self.ctx, C.byref(a)), "pqg_assemble")
        return a, vp, sp, op

    def assemble_list(self, def_ptr, rep_ptr, values_ptr, num_slots, max_def, list_def=1, elem_def=2,
                      value_width=0, values=True):
        """K8 list export (Arrow LIST layout) of device level/value arrays.
        Returns (ListArgs, list_validity, list_offsets, elem_validity, elem_values)
        device pointers (elem_values None unless `values`)."""
        a = abi.ListArgs()
        a.def_levels, a.rep_levels, a.values = def_ptr, rep_ptr or None, values_ptr or None
        a.num_slots, a.max_def, a.list_def, a.elem_def = num_slots, max_def, list_def, elem_def
        a.value_width = value_width

        def alloc(nbytes):
            p = C.c_void_p()
            _check(self.L.pqg_device_alloc(self.ctx, max(nbytes, 1), C.byref(p)), "pqg_device_alloc")
            self._bufs.append(p)
            return p.value

        bm = (num_slots + 31) // 32 * 4
        a.list_validity, a.list_offsets, a.elem_validity = alloc(bm), alloc((num_slots + 1) * 4), alloc(bm)
        a.elem_values = alloc(num_slots * value_width) if values and value_width else None
        _check(self.L.pqg_assemble_list(self.ctx, C.byref(a)), "pqg_assemble_list")
        return a, a.list_validity, a.list_offsets, a.elem_validity, a.elem_values

    def assemble_nested(self, def_ptr, rep_ptr, values_ptr, num_slots, max_def, list_def=(), elem_def=(),
                        value_width=0, value_offsets_ptr=None, validity=True, offsets=True, leaf_validity=True,
                        values=True):
        """K8 nested export (Arrow layout of every list depth) of device
        level/value arrays; the counterpart of assemble_list for any depth and
        for byte-array leaves (value_offsets_ptr: the chunk result's offsets).
        Allocates the requested outputs and returns the NestedArgs, whose
        level[k].validity / offsets, leaf_validity, leaf_values and
        leaf_offsets are the device pointers."""
        depth = len(elem_def)
        if depth > abi.MAX_LIST_DEPTH:
            raise PqgError(abi.STATUS_CODES["UNSUPPORTED"], "pqg_assemble_nested: %d list depths" % depth)
        a = abi.NestedArgs()
        a.def_levels, a.rep_levels, a.values = def_ptr or None, rep_ptr or None, values_ptr or None
        a.value_offsets = value_offsets_ptr or None
        a.num_slots, a.max_def, a.depth, a.value_width = num_slots, max_def, depth, value_width

        def alloc(nbytes):
            p = C.c_void_p()
            _check(self.L.pqg_device_alloc(self.ctx, max(nbytes, 1), C.byref(p)), "pqg_device_alloc")
            self._bufs.append(p)
            return p.value

        bm = (num_slots + 31) // 32 * 4
        for k in range(depth):
            a.level[k].list_def, a.level[k].elem_def = list_def[k], elem_def[k]
            a.level[k].validity = alloc(bm) if validity else None
            a.level[k].offsets = alloc((num_slots + 1) * 4) if offsets else None
        a.leaf_validity = alloc(bm) if leaf_validity else None
        if values and value_offsets_ptr:
            a.leaf_offsets = alloc((num_slots + 1) * 8)
        elif values and value_width:
            a.leaf_values = alloc(num_slots * value_width)
        try:
            _check(self.L.pqg_assemble_nested(self.ctx, C.byref(a)), "pqg_assemble_nested")
        except PqgError:
            self.free_nested(a)
            raise
        return a

    def free_nested(self, a):
        """Free the outputs assemble_nested allocated."""
        for p in [a.leaf_validity, a.leaf_values, a.leaf_offsets] + \
                 [x for k in range(a.depth) for x in (a.level[k].validity, a.level[k].offsets)]:
            if p:
                self.free(p)

    def assemble_structs(self, def_ptr, rep_ptr, num_slots, max_def, elem_def=(), structs=(), validity=True):
        """K8 struct export of device level arrays: the validity bitmaps of up to abi.MAX_STRUCTS
        structs above one leaf, `structs` = [(depth, struct_def)], elem_def as for
        assemble_nested.  Allocates the bitmaps (validity=False: counts only) and returns the
        StructArgs, whose st[j].validity are the device pointers (free_structs)."""
        depth = len(elem_def)
        if depth > abi.MAX_LIST_DEPTH:
            raise PqgError(abi.STATUS_CODES["UNSUPPORTED"], "pqg_assemble_structs: %d list depths" % depth)
        if len(structs) > abi.MAX_STRUCTS:
            raise PqgError(abi.STATUS_CODES["INVALID_ARG"], "pqg_assemble_structs: %d structs" % len(structs))
        a = abi.StructArgs()
        a.def_levels, a.rep_levels = def_ptr or None, rep_ptr or None
        a.num_slots, a.max_def, a.depth, a.num_structs = num_slots, max_def, depth, len(structs)
        for k in range(depth):
            a.elem_def[k] = elem_def[k]
        bm = (num_slots + 31) // 32 * 4
        for j, (d, sd) in enumerate(structs):
            a.st[j].depth, a.st[j].struct_def = d, sd
            a.st[j].validity = self.alloc(bm) if validity else None
        try:
            _check(self.L.pqg_assemble_structs(self.ctx, C.byref(a)), "pqg_assemble_structs")
        except PqgError:
            self.free_structs(a)
            raise
        return a

    def free_structs(self, a):
        """Free the bitmaps assemble_structs allocated."""
        for j in range(a.num_structs):
            if a.st[j].validity:
                self.free(a.st[j].validity)

    def download_structs(self, a):
        """[(validity uint32 words or None, null_count, num_entries)] of an assemble_structs call."""
        out = []
        for j in range(a.num_structs):
            s = a.st[j]
            val = self.d2h(s.validity, (s.num_entries + 31) // 32 * 4, np.uint32) if s.validity else None
            out.append((val, int(s.null_count), int(s.num_entries)))
        return out

    def last_assemble_ms(self):
        ms = C.c_float()
        _check(self.L.pqg_last_assemble_ms(self.ctx, C.byref(ms)), "pqg_last_assemble_ms")
        return ms.value

    # ---- K9s: row predicates and row selection
    def alloc(self, nbytes):
        """A device buffer of nbytes (at least 1), freed by free() or close()."""
        p = C.c_void_p()
        _check(self.L.pqg_device_alloc(self.ctx, max(nbytes, 1), C.byref(p)), "pqg_device_alloc")
        self._bufs.append(p)
        return p.value

    def filter(self, bitmap_ptr, desc, op, literal=None, *, def_ptr=None, values_ptr=None, offsets_ptr=None,
               num_rows=0, num_values=0, values_bytes=0, combine=abi.COMBINE_SET, dictionary=None):
        """pqg_filter: `column op literal` into the row bitmap at bitmap_ptr (4 * ceil(num_rows / 32)
        device bytes; combine: abi.COMBINE_*).  desc: the column's abi.ColumnDesc; literal: bytes in
        its physical layout; dictionary: the abi.Dictionary (device pointers) of a column whose
        values are its int32 keys.  Returns the FilterArgs (num_selected, num_valid)."""
        a = abi.FilterArgs()
        a.def_levels, a.values, a.offsets = def_ptr or None, values_ptr or None, offsets_ptr or None
        a.num_rows, a.num_values, a.values_bytes = num_rows, num_values, values_bytes
        a.col, a.op, a.combine = desc, op, combine
        lit = np.frombuffer(bytes(literal), dtype=np.uint8) if literal is not None else np.zeros(0, np.uint8)
        a.literal = lit.ctypes.data if len(lit) else None
        a.literal_len = len(lit)
        if dictionary is not None:
            a.dictionary = C.pointer(dictionary)
        a.bitmap = bitmap_ptr or None
        _check(self.L.pqg_filter(self.ctx, C.byref(a)), "pqg_filter")
        return a

    def filter_result(self, bitmap_ptr, r, desc, op, literal=None, combine=abi.COMBINE_SET, dictionary=None):
        """filter() on a decoded chunk (a ChunkResult of this decoder's last decode)."""
        return self.filter(bitmap_ptr, desc, op, literal, def_ptr=r.def_levels, values_ptr=r.values,
                           offsets_ptr=r.offsets, num_rows=r.num_slots, num_values=r.num_values,
                           values_bytes=r.values_bytes, combine=combine, dictionary=dictionary)

    def select(self, bitmap_ptr, def_ptr, values_ptr, offsets_ptr, num_rows, num_values, values_bytes, max_def,
               value_width, count_only=False):
        """pqg_select: the column compacted by the row bitmap, into newly allocated device buffers
        of the inputs' sizes (which the outputs never exceed): the SelectArgs, whose out_* are the
        device pointers (free_select) and rows_out / values_out / bytes_out the counts.  count_only:
        no buffers, only the counts."""
        a = abi.SelectArgs()
        a.bitmap, a.def_levels, a.values, a.offsets = bitmap_ptr or None, def_ptr or None, values_ptr or None, \
            offsets_ptr or None
        a.num_rows, a.num_values, a.values_bytes = num_rows, num_values, values_bytes
        a.max_def, a.value_width = max_def, value_width
        if not count_only and num_rows > 0:
            a.out_def_levels = self.alloc(num_rows) if def_ptr and max_def > 0 else None
            a.out_values = self.alloc(values_bytes)
            a.out_offsets = self.alloc((num_values + 1) * 8) if value_width == 0 else None
        try:
            _check(self.L.pqg_select(self.ctx, C.byref(a)), "pqg_select")
        except PqgError:
            self.free_select(a)
            raise
        return a

    def free_select(self, a):
        """Free the outputs select allocated."""
        for p in (a.out_def_levels, a.out_values, a.out_offsets):
            if p:
                self.free(p)

    def last_filter_ms(self):
        ms = C.c_float()
        _check(self.L.pqg_last_filter_ms(self.ctx, C.byref(ms)), "pqg_last_filter_ms")
        return ms.value

    # ---- K10: logical-type conversion
    def convert(self, values_ptr, num_values, values_bytes, kind, in_width, out_width, unit=abi.UNIT_NONE,
                offsets_ptr=None):
        """pqg_convert on device values (abi.CONV_*): decimals to out_width (16 / 32) little-endian
        bytes, INT96 to int64 in `unit` (abi.UNIT_*).  offsets_ptr: the int64 offsets of BYTE_ARRAY
        decimals (in_width 0).  Returns the device pointer of the num_values * out_width output
        bytes, allocated here: the caller frees it (free).  A BYTE_ARRAY decimal of length 0 or
        above out_width raises PqgError(SIZE) with the count in its `num_bad`."""
        a = abi.ConvertArgs()
        a.values, a.offsets = values_ptr or None, offsets_ptr or None
        a.num_values, a.values_bytes = num_values, values_bytes
        a.kind, a.in_width, a.out_width, a.unit = kind, in_width, out_width, unit
        a.out = self.alloc(num_values * out_width)
        rc = self.L.pqg_convert(self.ctx, C.byref(a))
        if rc != 0:
            self.free(a.out)
            e = PqgError(rc, "pqg_convert")
            e.num_bad = int(a.num_bad)
            raise e
        return a.out

    def last_convert_ms(self):
        ms = C.c_float()
        _check(self.L.pqg_last_convert_ms(self.ctx, C.byref(ms)), "pqg_last_convert_ms")
        return ms.value

    def convert_dictionary(self, job_index, cv):
        """The dictionary of job `job_index` (dictionary()) with its entries converted on the device
        by `cv` (a pqgpu.logical.Conversion): values are count * out_width bytes, value_width the
        output width.  Entries the page does not hold and the nil entry are what zero bytes convert
        to; nil_entry is then -1."""
        from .logical import int96_zero
        d = abi.Dictionary()
        _check(self.L.pqg_get_dictionary(self.ctx, job_index, C.byref(d)), "pqg_get_dictionary")
        ow, n = cv.out_width, int(d.count)
        held = n if cv.in_width == 0 else min(n, int(d.values_bytes) // cv.in_width)
        vals = np.zeros(n * ow, np.uint8)
        if held > 0:
            out = self.convert(d.values, held, d.values_bytes, cv.kind, cv.in_width, ow, cv.unit,
                               d.offsets if cv.in_width == 0 else None)
            try:
                vals[:held * ow] = self.d2h(out, held * ow)
            finally:
                self.free(out)
        if cv.kind == abi.CONV_INT96_TIME:
            zero = np.frombuffer(np.int64(int96_zero(cv.unit)).tobytes(), np.uint8)
            t = vals.reshape(n, ow)
            t[held:] = zero
            if 0 <= d.nil_entry < n:
                t[d.nil_entry] = zero
        return Dictionary(vals, None, n, ow, -1, d.page)

    def download_nested(self, a, chars=None, physical_type=None, flags=0, dictionary=None):
        """The outputs of an assemble_nested call as a NestedColumn on the host
        (`chars`: the decoded chars of a byte-array leaf, already downloaded; `dictionary`:
        the Dictionary of a leaf whose values are its keys)."""
        from .nested import NestedColumn
        levels = []
        for k in range(a.depth):
            l = a.level[k]
            offs = self.d2h(l.offsets, (l.num_entries + 1) * 4, np.int32) if l.offsets else None
            val = self.d2h(l.validity, (l.num_entries + 31) // 32 * 4, np.uint32) if l.validity else None
            levels.append((offs, val, int(l.null_count)))
        lv = self.d2h(a.leaf_validity, (a.num_leaf + 31) // 32 * 4, np.uint32) if a.leaf_validity else None
        vals = self.d2h(a.leaf_values, a.num_leaf * a.value_width) if a.leaf_values else None
        lo = self.d2h(a.leaf_offsets, (a.num_leaf + 1) * 8, np.int64) if a.leaf_offsets else None
        return NestedColumn(levels, lv, int(a.num_leaf), values=vals, value_width=a.value_width, chars=chars,
                            leaf_offsets=lo, physical_type=physical_type, flags=flags, num_rows=int(a.num_rows),
                            dictionary=dictionary)

    def download(self, r, job_index=None):
        lv_def = self.d2h(r.def_levels, r.num_slots) if (r.def_levels and r.status == 0) else None
        lv_rep = self.d2h(r.rep_levels, r.num_slots) if (r.rep_levels and r.status == 0) else None
        vals = self.d2h(r.values, r.values_bytes) if r.status == 0 else None
        offs = self.d2h(r.offsets, (r.num_values + 1) * 8, np.int64) if (r.offsets and r.status == 0) else None
        pages = self.pages(job_index) if job_index is not None else None
        # a job that kept its dictionary (abi.COL_KEEP_DICT): the keys, and the dictionary with them
        keep = bool(r.col_flags & abi.COL_KEEP_DICT) and r.status == 0 and job_index is not None
        return DecodedColumn(r.status, r.error_page, r.num_slots, r.num_values, r.value_width, lv_def, lv_rep,
                             vals, pages, offs, dictionary=self.dictionary(job_index) if keep else None)


def device_job(pf: ParquetFile, rg, col, dev_ptr_of_file):
    """Chunk job pointing into a device copy of the whole file."""
    job, m = pf.host_job(rg, col)
    start = max(0, min(m.start, len(pf.data)))
    job.data = dev_ptr_of_file + start
    return job


def chunk_span(pf: ParquetFile, specs):
    """The byte span [lo, hi) covering the chunks of (rg, col) pairs
    ([start, start + TotalCompressedSize) each, chunk_reader.go:332-340) and
    their ChunkMetas."""
    metas = [pf.chunk_meta(rg, c) for rg, c in specs]
    lo = min(m.start for m in metas)
    hi = max(m.start + m.total_compressed_size for m in metas)
    return max(0, lo), min(hi, pf.size), metas


def chunk_ranges(pf: ParquetFile, specs, to_eof=()):
    """The byte ranges the chunks of (rg, col) pairs occupy ([start, start +
    TotalCompressedSize) each, clipped to the file; [start, end of file) for the
    spec indices in `to_eof`), sorted, with overlapping or adjacent ranges
    merged: [(lo, hi)], and the chunks' ChunkMetas."""
    metas = [pf.chunk_meta(rg, c) for rg, c in specs]
    rs = sorted((max(0, min(m.start, pf.size)),
                 pf.size if i in to_eof else max(0, min(m.start + m.total_compressed_size, pf.size)))
                for i, m in enumerate(metas))
    out = []
    for lo, hi in rs:
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [tuple(r) for r in out], metas


def span_jobs(pf: ParquetFile, specs, dec, to_eof=()):
    """Chunk jobs for (rg, col) pairs with only their chunks' bytes uploaded,
    packed into one device buffer (merged ranges, chunk_ranges), each job
    pointing into it.  Unselected chunks are never read, as skipChunk seeks past
    them (chunk_reader.go:286-312).  A job's readable bytes run to the end of
    its merged range.  That range holds every page HEADER readPages reads (it
    reads headers while TotalCompressedSize - Count() > 0, chunk_reader.go:212-
    217), but the reference then reads the whole page from the file, so a last
    page overrunning an understated TotalCompressedSize needs bytes past it:
    decode_spans re-uploads such chunks to the end of the file (`to_eof`).
    Returns (jobs, device pointer, bytes uploaded)."""
    ranges, metas = chunk_ranges(pf, specs, to_eof)
    total = sum(hi - lo for lo, hi in ranges)
    base = []  # packed offset of each range
    at = 0
    for lo, hi in ranges:
        base.append(at)
        at += hi - lo
    if pf._buf is not None:  # the file in host memory: each range straight from it
        dev = dec.upload_ranges(pf._buf, ranges)
    else:
        host = np.empty(max(total, 1), dtype=np.uint8)
        for (lo, hi), b in zip(ranges, base):
            host[b:b + hi - lo] = pf.read_range(lo, hi)
        dev = dec.upload(host)
        del host
    jobs = []
    for (rg, c), m in zip(specs, metas):
        job = abi.ChunkJob()
        job.col = pf.columns[c].desc
        job.col.codec = m.codec
        job.total_compressed_size = m.total_compressed_size
        job.data_page_offset = m.data_page_offset - m.start
        job.num_values_hint = m.num_values
        job.total_uncompressed_size = m.total_uncompressed_size
        job.has_dict_page_offset = m.has_dict_page_offset
        start = max(0, min(m.start, pf.size))
        k = max(i for i, (lo, _) in enumerate(ranges) if lo <= start)
        lo, hi = ranges[k]
        job.data = dev + base[k] + (start - lo)
        job.data_len = hi - start
        jobs.append(job)
    return jobs, dev, total


def _merge(ranges):
    """Sorted, disjoint, non-empty row ranges covering `ranges` (adjacent ones joined)."""
    out = []
    for a, b in sorted(r for r in ranges if r[1] > r[0]):
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def _intersect(x, y):
    """The rows in both of two sorted lists of disjoint row ranges."""
    out, i, j = [], 0, 0
    while i < len(x) and j < len(y):
        a, b = max(x[i][0], y[j][0]), min(x[i][1], y[j][1])
        if b > a:
            out.append((a, b))
        if x[i][1] < y[j][1]:
            i += 1
        else:
            j += 1
    return out


def located_jobs(pf: ParquetFile, specs, dec, pages=None):
    """Chunk jobs for (rg, col) pairs decoded by page location where the file has an OffsetIndex: of
    such a chunk only the listed pages are uploaded, packed, with their locations rebased to the packed
    bytes (the dictionary page, the gap between the chunk's start and its first data page, goes first).  `pages`: {spec index:
    sorted data page numbers} to list only those (default: all).  Chunks without an index are uploaded
    whole and scanned.  Returns (jobs, location lists (None: scanned), device buffer, bytes uploaded,
    (pages listed, pages in all) per spec)."""
    parts, plan = [], []
    for i, (rg, c) in enumerate(specs):
        m = pf.chunk_meta(rg, c)
        start = max(0, min(m.start, pf.size))
        pi = pf.page_index(rg, c)
        if pi is None or not pi.locations:
            plan.append((m, [(start, max(0, min(m.start + m.total_compressed_size, pf.size)))], None, (0, 0)))
            continue
        want = range(len(pi.locations)) if pages is None or i not in pages else pages[i]
        ranges = []
        first = pi.locations[0][0]
        if start < first:  # whatever lies before the first data page: the dictionary page, with or
            ranges.append((start, first))  # without a dictionary_page_offset in the footer
        ranges += [(pi.locations[k][0], pi.locations[k][0] + pi.locations[k][1]) for k in want]
        plan.append((m, ranges, True, (len(want), len(pi.locations))))
    flat = []  # in packing order; neighbours that touch in the file are one copy
    for _, ranges, _, _ in plan:
        for lo, hi in ranges:
            if flat and flat[-1][1] == lo:
                flat[-1] = (flat[-1][0], hi)
            else:
                flat.append((lo, hi))
    total = sum(hi - lo for lo, hi in flat)
    if pf._buf is not None:
        dev = dec.upload_ranges(pf._buf, flat)
    else:
        host = np.empty(max(total, 1), dtype=np.uint8)
        at = 0
        for lo, hi in flat:
            host[at:at + hi - lo] = pf.read_range(lo, hi)
            at += hi - lo
        dev = dec.upload(host)
    jobs, lists, counts, at = [], [], [], 0
    for (rg, c), (m, ranges, located, cnt) in zip(specs, plan):
        size = sum(hi - lo for lo, hi in ranges)
        job = abi.ChunkJob()
        job.col = pf.columns[c].desc
        job.col.codec = m.codec
        job.total_compressed_size = m.total_compressed_size if not located else size
        job.data_page_offset = m.data_page_offset - m.start
        job.num_values_hint = m.num_values
        job.total_uncompressed_size = m.total_uncompressed_size
        job.has_dict_page_offset = m.has_dict_page_offset if not located else 0
        job.data = dev + at
        job.data_len = size
        locs, o = None, 0
        if located:
            locs = []
            for lo, hi in ranges:
                locs.append((o, hi - lo))
                o += hi - lo
        jobs.append(job)
        lists.append(locs)
        counts.append(cnt)
        at += size
    return jobs, lists, dev, total, counts


def _decode_spans_located(pf, specs, dec, keep_dict, info):
    """decode_spans with use_page_index: the chunks that have an OffsetIndex by location (all pages,
    the dictionary page first), the others scanned, in one batch.  A chunk that comes back INDEX (its
    index is wrong) sends the batch to the scan once more, and so does any other failing chunk: the
    scanned path has second batches of its own (NOT_DICT, EOF, SIZE), and what it reports for a chunk
    that does not decode is what the caller gets."""
    jobs, lists, dev, nbytes, counts = located_jobs(pf, specs, dec)
    for i, (_, c) in enumerate(specs):
        if c in keep_dict:
            jobs[i].col.flags |= abi.COL_KEEP_DICT
    res = dec.decode_located(jobs, lists)
    code = abi.STATUS_CODES
    bad = [i for i, r in enumerate(res) if lists[i] is not None and r.status == code["INDEX"]]
    if info is not None:
        info["located"] = {specs[i]: lists[i] is not None and i not in bad for i in range(len(specs))}
        info["fell_back"] = [specs[i] for i in bad]
        info["pages_decoded"] = sum(a for a, _ in counts)
        info["pages_total"] = sum(b for _, b in counts)
    if not any(r.status != 0 for r in res):
        return res, dev, nbytes
    dec.free(dev)
    res, dev, nb2 = decode_spans(pf, specs, dec, keep_dict)
    return res, dev, nbytes + nb2


def decode_spans(pf: ParquetFile, specs, dec, keep_dict=(), use_page_index=False, info=None):
    """span_jobs + pqg_decode_chunks for (rg, col) pairs.  The chunks of the columns in
    `keep_dict` (column indices) are decoded with abi.COL_KEEP_DICT; those that come back
    NOT_DICT (a data page that is not dictionary encoded: a writer's fallback) are decoded
    once more without it, in one second batch of the same jobs, so their results are
    materialised (col_flags tells which).  A chunk whose decode
    ends in EOF / size mismatch while the file holds bytes past its uploaded
    range (a page overrunning TotalCompressedSize, which the reference still
    reads whole: chunk_reader.go:212-280) is decoded again with the bytes to the
    end of the file, in a second batched call (device outputs are only valid
    until the next decode on `dec`).  Returns (results, device buffer, bytes
    uploaded); the caller frees the buffer after using the outputs.
    use_page_index: chunks with an OffsetIndex are decoded by location (_decode_spans_located);
    info: a dict that receives located / fell_back / pages_decoded / pages_total."""
    if use_page_index:
        return _decode_spans_located(pf, specs, dec, keep_dict, info)
    if info is not None:
        info.update(located={s: False for s in specs}, fell_back=[], pages_decoded=0, pages_total=0)
    jobs, dev, nbytes = span_jobs(pf, specs, dec)
    keep = {i for i, (_, c) in enumerate(specs) if c in keep_dict}
    for i in keep:
        jobs[i].col.flags |= abi.COL_KEEP_DICT
    res = dec.decode_jobs(jobs)
    not_dict = {i for i in keep if res[i].status == abi.STATUS_CODES["NOT_DICT"]}
    if not_dict:
        keep -= not_dict
        for i in not_dict:
            jobs[i].col.flags &= ~abi.COL_KEEP_DICT
        res = dec.decode_jobs(jobs)
    retry = set()
    for i, (job, r) in enumerate(zip(jobs, res)):
        m = pf.chunk_meta(*specs[i])
        start = max(0, min(m.start, pf.size))
        if r.status in (abi.STATUS_CODES["EOF"], abi.STATUS_CODES["SIZE"]) and job.data_len < pf.size - start:
            retry.add(i)
    if retry:
        dec.free(dev)
        jobs, dev, nb2 = span_jobs(pf, specs, dec, to_eof=retry)
        nbytes += nb2
        for i in keep:
            jobs[i].col.flags |= abi.COL_KEEP_DICT
        res = dec.decode_jobs(jobs)
    return res, dev, nbytes


class FileReader:
    """Mirror of parquet-go's FileReader (file_reader.go:27-118): the selected
    columns of a file (dotted paths, schema.isSelected schema.go:296-312; none =
    all), decoded one row group at a time on the GPU.  `source` is the file's
    bytes or a path (then only the footer and the selected chunks are read);
    each row group uploads only its selected chunks' bytes (span_jobs).
    `verify_crc`: check PageHeader.crc of the pages that carry one (GpuDecoder.set_verify_crc);
    a page that fails makes the readers that raise PqgError raise it with code -18 (CRC).
    `read_dictionary`: dotted paths (as `columns`: a path or a prefix) of columns to keep
    dictionary encoded, as pyarrow's read_dictionary= does: read_row_group, decode_row_groups and
    read_row_group_nested decode their chunks with abi.COL_KEEP_DICT (int32 keys plus a
    Dictionary instead of values).  A chunk with a data page that is not dictionary encoded is
    decoded again without the flag and comes back materialised (dictionary None).  BOOLEAN
    columns are never flagged; next_row ignores the option, rows need values.
    `convert_logical`: read_row_group (filtered or not) and read_row_group_nested convert, on the
    GPU before the download (pqg_convert; after pqg_select in a filtered read), DECIMAL leaves of
    precision 1..76 on FLBA (type_length up to the output width) / BYTE_ARRAY / INT32 / INT64 to 16
    (precision <= 38) or 32 little-endian two's-complement bytes, and INT96 leaves to int64 in
    `int96_unit` ("s", "ms", "us", "ns"); every DecodedColumn then carries its column's
    abi.LogicalType in `logical`, and a leaf that cannot be converted comes back raw.  Of a column
    that keeps its dictionary only the dictionary's entries are converted.  Filters then take
    typed literals (pqgpu.filters.literal), order FLBA decimals signed, and compare an INT96 column
    as int64 nanoseconds since the epoch (such a predicate column is decoded materialised, whatever
    read_dictionary says); a predicate on a BYTE_ARRAY decimal raises PqgError(UNSUPPORTED).
    next_row ignores the option.  Off (the default), every method returns what it always did.
    `use_page_index`: chunks for which the file holds an OffsetIndex are decoded by page location
    (pqg_decode_chunks_located: no chunk byte is scanned for page headers) in every reader; chunks
    without one are scanned, and a chunk whose index proves wrong (INDEX) is decoded again by the
    scan.  read_row_group then also uploads and decodes only the pages that its `rows=` range and
    the ColumnIndex bounds of its `filters=` cannot rule out.  `last_read` tells what the last
    decode did: pages_total, pages_decoded, located {(rg, col): bool}, fell_back [(rg, col)] and,
    after read_row_group, row_ranges (the rows that were decoded and kept before the filter ran)."""

    def __init__(self, source, *columns, device=0, decoder=None, verify_crc=False, read_dictionary=(),
                 convert_logical=False, int96_unit="ns", use_page_index=False):
        self.use_page_index = bool(use_page_index)
        self.last_read = {}
        if int96_unit not in abi.UNITS:
            raise ValueError("int96_unit: one of %s" % ", ".join(sorted(abi.UNITS)))
        self.convert_logical = bool(convert_logical)
        self.int96_unit = abi.UNITS[int96_unit]
        self.file = ParquetFile.open(source) if isinstance(source, (str, os.PathLike)) else ParquetFile(source)
        self.dec = decoder or GpuDecoder(device)
        if verify_crc:
            self.dec.set_verify_crc(True)
        self.selected = self._select(columns)
        # every column read_dictionary names: a predicate column need not be selected
        self._dict_named = frozenset(
            i for i in (self._select(tuple(read_dictionary)) if read_dictionary else [])
            if self.file.columns[i].desc.physical_type != abi.BOOLEAN)
        self.keep_dict = frozenset(i for i in self._dict_named if i in self.selected)
        self.row_group_position = 0
        self.uploaded_bytes = 0   # H2D bytes so far (projection pushdown check)
        self._rows = None         # NextRow state (pqgpu.rows.RowReader)
        self._held = None         # chunk bytes decode_row_groups left on the device (in-place dictionaries)

    def _decode_spans(self, specs, keep_dict):
        info = {}
        out = decode_spans(self.file, specs, self.dec, keep_dict, self.use_page_index, info)
        self.last_read = info
        return out

    def _release(self):
        """Free the chunk bytes the last decode_row_groups kept for its dictionaries."""
        if self._held is not None:
            self.dec.free(self._held)
            self._held = None

    def _select(self, columns):
        if not columns:
            return list(range(self.file.num_columns))
        out = []
        for i, c in enumerate(self.file.columns):
            path = c.path.decode()
            if any(path == p or path.startswith(p + ".") for p in columns):
                out.append(i)
        return out

    def _logical(self, c):
        """Column c's abi.LogicalType when convert_logical is on, else None."""
        return self.file.logical_types[c] if self.convert_logical else None

    def _conversion(self, c):
        """Column c's pqgpu.logical.Conversion, None when it stays as it is."""
        if not self.convert_logical:
            return None
        from .logical import conversion
        return conversion(self.file.columns[c].desc, self.file.logical_types[c], self.int96_unit)

    def _convert_values(self, cv, values, num_values, values_bytes, offsets):
        """pqg_convert of dense device values by `cv`, downloaded."""
        out = self.dec.convert(values, num_values, values_bytes, cv.kind, cv.in_width, cv.out_width, cv.unit,
                               offsets if cv.in_width == 0 else None)
        try:
            return self.dec.d2h(out, num_values * cv.out_width)
        finally:
            self.dec.free(out)

    def _download(self, r, i, c):
        """Job i's result (column c) on the host, converted when convert_logical asks for it."""
        cv = self._conversion(c)
        if cv is None or r.status != 0:
            col = self.dec.download(r, i)
        else:
            dec = self.dec
            lv_def = dec.d2h(r.def_levels, r.num_slots) if r.def_levels else None
            lv_rep = dec.d2h(r.rep_levels, r.num_slots) if r.rep_levels else None
            if r.col_flags & abi.COL_KEEP_DICT:  # the keys as they are, the dictionary's entries converted
                col = DecodedColumn(r.status, r.error_page, r.num_slots, r.num_values, r.value_width, lv_def, lv_rep,
                                    dec.d2h(r.values, r.values_bytes), dec.pages(i), None,
                                    dictionary=dec.convert_dictionary(i, cv))
            else:
                vals = self._convert_values(cv, r.values, r.num_values, r.values_bytes, r.offsets)
                col = DecodedColumn(r.status, r.error_page, r.num_slots, r.num_values, cv.out_width, lv_def, lv_rep,
                                    vals, dec.pages(i), None)
        col.logical = self._logical(c)
        return col

    def row_group_count(self):
        return self.file.num_row_groups

    def num_rows(self):
        return self.file.num_rows

    def decode_row_groups(self, rgs):
        """readRowGroup (chunk_reader.go:404-431) for the selected columns of
        every row group in `rgs`, one batched decode: [(rg, col, ChunkResult)]
        with device outputs (valid until the next decode on the decoder).
        Result i is job i of that decode: for one whose col_flags carry
        abi.COL_KEEP_DICT, self.dec.dictionary(i) is its dictionary.  A
        fixed-width dictionary of an uncompressed chunk is handed out in place,
        inside the uploaded chunk bytes, so when any chunk kept its dictionary
        the upload stays on the device until this reader's next decode (any of
        its read / decode methods) or close(); otherwise it is freed here."""
        self._release()
        specs = [(rg, c) for rg in rgs for c in self.selected]
        if not specs:
            return []
        res, dev, nbytes = self._decode_spans(specs, self.keep_dict)
        self.uploaded_bytes += nbytes
        if any(r.col_flags & abi.COL_KEEP_DICT for r in res):
            self._held = dev
        else:
            self.dec.free(dev)
        return [(rg, c, r) for (rg, c), r in zip(specs, res)]

    def read_row_group(self, rg, filters=None, rows=None):
        """One row group's selected columns, downloaded: {path: DecodedColumn}.  `filters`
        (pyarrow's DNF, pqgpu.filters) keeps only the rows that pass: see _read_filtered.
        `rows`: (start, stop) or a slice of the row group's rows (flat columns only): only those
        rows come back, and with use_page_index only the pages that hold them are uploaded."""
        if filters is not None or rows is not None:
            return self._read_filtered(rg, filters, rows)
        self._release()
        specs = [(rg, c) for c in self.selected]
        if not specs:
            return {}
        res, dev, nbytes = self._decode_spans(specs, self.keep_dict)
        self.uploaded_bytes += nbytes
        try:
            return {self.file.columns[c].path.decode(): self._download(r, i, c)
                    for i, ((_, c), r) in enumerate(zip(specs, res))}
        finally:
            self.dec.free(dev)

    def _row_ranges(self, rg, dnf, rows):
        """The sorted, disjoint row ranges R a planned read keeps before its filter runs: `rows`, and
        with use_page_index and filters, intersected with the union over the conjunctions of the rows
        of the pages that no term's ColumnIndex bounds rule out (conservative, as prune_row_groups)."""
        from . import filters as F
        n = self.file.row_group_rows(rg)
        if rows is None:
            R = [(0, n)]
        else:
            if isinstance(rows, slice):
                if rows.step not in (None, 1):
                    raise ValueError("rows: a slice of step 1")
                lo, hi, _ = rows.indices(n)
            else:
                lo, hi = rows
                lo, hi = max(0, min(int(lo), n)), max(0, min(int(hi), n))
            R = [(lo, hi)] if hi > lo else []
        if dnf is not None and self.use_page_index:
            keep = []
            for terms in dnf:
                conj = [(0, n)]
                for t in terms:
                    c = self.file.column_index(t.column)
                    desc, lt = self.file.columns[c].desc, self._logical(c)
                    pi = self.file.page_index(rg, c)
                    if pi is None or pi.null_pages is None or (lt is not None and desc.physical_type == abi.INT96):
                        continue  # never prunes
                    spans = []
                    for k in range(len(pi.locations)):
                        a, b = pi.page_rows(k)
                        if b > a and not F.term_rules_out(desc, t, pi.stats(k), b - a, lt):
                            spans.append((a, b))
                    conj = _intersect(conj, _merge(spans))
                keep += conj
            R = _intersect(R, _merge(keep))
        return R

    def _decode_planned(self, rg, cols, keep_named, R, temps, sels):
        """Decode the chunks of `cols` for the rows R of row group rg and trim each to R: with
        use_page_index only the pages meeting R (and the dictionary page) are uploaded, packed, and
        decoded by location; pqg_range_bitmap + pqg_select then drop the rows of those pages outside R.
        Returns ([ChunkResult whose arrays hold exactly R's rows], device buffer)."""
        n = self.file.row_group_rows(rg)
        specs = [(rg, c) for c in cols]
        info = {}
        whole = [(0, n)]
        spans = {i: whole for i in range(len(cols))}
        res = None
        if self.use_page_index and R != whole:
            pages = {}
            for i, c in enumerate(cols):
                pi = self.file.page_index(rg, c)
                if pi is not None and pi.locations:
                    pages[i] = [k for k in range(len(pi.locations))
                                if _intersect([pi.page_rows(k)], R)]
                    spans[i] = _merge([pi.page_rows(k) for k in pages[i]])
            jobs, lists, dev, nbytes, counts = located_jobs(self.file, specs, self.dec, pages)
            for i, c in enumerate(cols):
                if c in keep_named:
                    jobs[i].col.flags |= abi.COL_KEEP_DICT
            res = self.dec.decode_located(jobs, lists)
            code = abi.STATUS_CODES
            bad = [i for i, r in enumerate(res) if lists[i] is not None and r.status == code["INDEX"]]
            info = dict(located={specs[i]: lists[i] is not None and i not in bad for i in range(len(specs))},
                        fell_back=[specs[i] for i in bad], pages_decoded=sum(a for a, _ in counts),
                        pages_total=sum(b for _, b in counts))
            if any(r.status != 0 for r in res):
                self.dec.free(dev)  # the scan, on the whole chunks
                self.uploaded_bytes += nbytes
                res = None
                spans = {i: whole for i in range(len(cols))}
        if res is None:
            fell = info.get("fell_back", [])
            res, dev, nbytes = decode_spans(self.file, specs, self.dec, keep_named, self.use_page_index and not fell, info)
            if fell:
                info["fell_back"] = fell
        self.uploaded_bytes += nbytes
        info["row_ranges"] = list(R)
        self.last_read = info
        out = []
        try:
            for i, (c, r) in enumerate(zip(cols, res)):
                if r.status != 0:
                    raise PqgError(r.status, "column %s of row group %d" % (self.file.columns[c].path.decode(), rg))
                have = sum(b - a for a, b in spans[i])
                if r.num_slots != have:
                    raise PqgError(abi.STATUS_CODES["INVALID_ARG"], "row group %d: column %s has %d rows, not %d"
                                   % (rg, self.file.columns[c].path.decode(), r.num_slots, have))
                if spans[i] == R:
                    out.append(r)
                    continue
                rel, at = [], 0  # R in the numbering of the decoded rows
                for a, b in spans[i]:
                    rel += [(at + x - a, at + y - a) for x, y in _intersect([(a, b)], R)]
                    at += b - a
                bm = self.dec.alloc((have + 31) // 32 * 4)
                temps.append(bm)
                self.dec.range_bitmap(rel, have, bm)
                sel = self.dec.select(bm, r.def_levels, r.values, r.offsets, have, r.num_values, r.values_bytes,
                                      self.file.columns[c].desc.max_def, r.value_width)
                sels.append(sel)
                t = abi.ChunkResult.from_buffer_copy(r)
                t.def_levels, t.values, t.offsets = sel.out_def_levels, sel.out_values, sel.out_offsets
                t.num_slots, t.num_values, t.values_bytes = sel.rows_out, sel.values_out, sel.bytes_out
                out.append(t)
        except Exception:
            for a in sels:
                self.dec.free_select(a)
            for p in temps:
                self.dec.free(p)
            del sels[:], temps[:]
            self.dec.free(dev)
            raise
        return out, dev

    def _no_rows(self, cols):
        """Zero-row columns: what a read of no rows returns, with nothing uploaded or decoded."""
        out = {}
        for c in cols:
            d = self.file.columns[c].desc
            w = abi.FIXED_WIDTH.get(d.physical_type, max(d.type_length, 0) if d.physical_type == 7 else 0)
            out[self.file.columns[c].path.decode()] = DecodedColumn(
                0, -1, 0, 0, w, np.zeros(0, np.uint8) if d.max_def > 0 else None, None, np.zeros(0, np.uint8), [],
                np.zeros(1, np.int64) if w == 0 else None, logical=self._logical(c))
        return out

    def _read_filtered(self, rg, filters, rows=None):
        """read_row_group with filters: a list of (column, op, value) tuples (AND) or a list of
        such lists (OR of ANDs); op is one of == = != < <= > >= in not in, or "is" / "is not" with
        None.  The predicate columns (selected or not) are decoded in the same batch as the
        selected ones, pqg_filter builds the row bitmap on the GPU, pqg_select compacts every
        selected column by it and only the selected rows are downloaded: each DecodedColumn holds
        them in the layout of an unfiltered read (num_slots == 0 when no row passes).  Columns
        named in read_dictionary are filtered through their dictionary and come back as keys; a
        chunk that fell back is filtered materialised.  A repeated column, selected or in a
        predicate, raises PqgError(UNSUPPORTED) before any GPU work; a chunk that does not decode
        raises its status, a value that does not fit its column's type ValueError.  No row group
        is pruned here (prune_row_groups).  `rows` and use_page_index: the rows R of _row_ranges
        are decoded and trimmed first (_decode_planned), and the predicates run on them; without
        filters the trimmed columns are the result."""
        from . import filters as F
        dnf = F.parse(filters) if filters is not None else None
        pred_cols = [self.file.column_index(name) for name in F.columns_of(dnf)] if dnf is not None else []
        cols = list(self.selected) + [c for c in pred_cols if c not in self.selected]
        for c in cols:
            if self.file.columns[c].desc.max_rep > 0:
                raise PqgError(abi.STATUS_CODES["UNSUPPORTED"], "filtered read of the repeated column %s"
                               % self.file.columns[c].path.decode())
        keep_named = self._dict_named
        if self.convert_logical:
            for c in pred_cols:
                d, lt = self.file.columns[c].desc, self.file.logical_types[c]
                if d.physical_type == abi.BYTE_ARRAY and lt.kind == abi.LT_DECIMAL:
                    raise PqgError(abi.STATUS_CODES["UNSUPPORTED"], "predicate on the BYTE_ARRAY decimal column %s"
                                   % self.file.columns[c].path.decode())
            # an INT96 predicate column is compared as converted int64 values: decoded materialised
            keep_named = frozenset(c for c in keep_named if not (
                c in pred_cols and self.file.columns[c].desc.physical_type == abi.INT96))
        self._release()
        specs = [(rg, c) for c in cols]
        R = self._row_ranges(rg, dnf, rows)
        if not R:
            self.last_read = dict(located={s: False for s in specs}, fell_back=[], pages_decoded=0, pages_total=0,
                                  row_ranges=[])
            return self._no_rows(self.selected)
        job = {c: i for i, c in enumerate(cols)}
        temps, sels = [], []
        res, dev = self._decode_planned(rg, cols, keep_named if dnf is not None else self.keep_dict, R, temps, sels)
        try:
            if dnf is None:  # a row-range read: the trimmed columns as they are
                return {self.file.columns[c].path.decode(): self._download(r, i, c)
                        for i, (c, r) in enumerate(zip(cols, res))}
            for (_, c), r in zip(specs, res):
                if r.status != 0:
                    raise PqgError(r.status, "column %s of row group %d" % (self.file.columns[c].path.decode(), rg))
            rows = res[0].num_slots
            if any(r.num_slots != rows for r in res):
                raise PqgError(abi.STATUS_CODES["INVALID_ARG"], "row group %d: columns of different lengths" % rg)
            bm_bytes = (rows + 31) // 32 * 4
            dicts = {}
            as_ns = {}  # INT96 predicate columns (convert_logical): their values as int64 ns, on the device

            def run(term, bitmap, first_combine):
                c = self.file.column_index(term.column)
                r, desc, lt = res[job[c]], self.file.columns[c].desc, self._logical(c)
                if r.col_flags & abi.COL_KEEP_DICT and c not in dicts:
                    d = abi.Dictionary()
                    _check(self.dec.L.pqg_get_dictionary(self.dec.ctx, job[c], C.byref(d)), "pqg_get_dictionary")
                    dicts[c] = d
                values, values_bytes = r.values, r.values_bytes
                if lt is not None and desc.physical_type == abi.INT96:
                    if c not in as_ns:
                        as_ns[c] = self.dec.convert(r.values, r.num_values, r.values_bytes, abi.CONV_INT96_TIME, 12, 8,
                                                    abi.UNIT_NANOS)
                        temps.append(as_ns[c])
                    values, values_bytes = as_ns[c], r.num_values * 8
                    desc = abi.ColumnDesc(abi.INT64, -1, desc.max_def, desc.max_rep, desc.codec, 0)
                    lt = abi.LogicalType(kind=abi.LT_TIMESTAMP, unit=abi.UNIT_NANOS)
                elif lt is not None and F.signed_be(desc, lt) and desc.type_length >= 1:
                    desc = abi.ColumnDesc.from_buffer_copy(desc)
                    desc.flags |= abi.COL_SIGNED_BE
                for k, (op, val, comb) in enumerate(term.steps()):
                    lit = F.literal(desc, val, lt) if val is not None else None
                    self.dec.filter(bitmap, desc, op, lit, def_ptr=r.def_levels, values_ptr=values,
                                    offsets_ptr=r.offsets, num_rows=r.num_slots, num_values=r.num_values,
                                    values_bytes=values_bytes, combine=first_combine if k == 0 else comb,
                                    dictionary=dicts.get(c))

            def conj_bitmap(terms):
                """One conjunction into a new device bitmap: the terms chain with AND; an `in`
                that cannot go first gets a bitmap of its own, AND-ed on the host."""
                terms = sorted(terms, key=lambda t: t.chains_with_and())  # an `in` first, if any
                bm = self.dec.alloc(bm_bytes)
                temps.append(bm)
                run(terms[0], bm, abi.COMBINE_SET)
                extra = []
                for t in terms[1:]:
                    if t.chains_with_and():
                        run(t, bm, abi.COMBINE_AND)
                    else:
                        e = self.dec.alloc(bm_bytes)
                        temps.append(e)
                        run(t, e, abi.COMBINE_SET)
                        extra.append(e)
                return bm, extra

            parts = [conj_bitmap(terms) for terms in dnf]
            bitmap = parts[0][0]
            if rows > 0 and (len(parts) > 1 or parts[0][1]):
                # bitmaps of one bit per row, combined on the host: OR of (AND of a conjunction's)
                acc = np.zeros(bm_bytes, np.uint8)
                for bm, extra in parts:
                    w = self.dec.d2h(bm, bm_bytes)
                    for e in extra:
                        w = w & self.dec.d2h(e, bm_bytes)
                    acc |= w
                _check(self.dec.L.pqg_memcpy_h2d(self.dec.ctx, C.c_void_p(bitmap), acc.ctypes.data, bm_bytes),
                       "pqg_memcpy_h2d")
            out = {}
            for c in self.selected:
                i, r = job[c], res[job[c]]
                desc = self.file.columns[c].desc
                a = self.dec.select(bitmap, r.def_levels, r.values, r.offsets, rows, r.num_values, r.values_bytes,
                                    desc.max_def, r.value_width)
                keep = bool(r.col_flags & abi.COL_KEEP_DICT)
                cv = self._conversion(c)
                width = r.value_width
                try:
                    lv = self.dec.d2h(a.out_def_levels, a.rows_out) if desc.max_def > 0 else None
                    offs = None
                    if cv is not None and not keep:  # only the selected values are converted
                        vals = self._convert_values(cv, a.out_values, a.values_out, a.bytes_out, a.out_offsets)
                        width = cv.out_width
                    else:
                        vals = self.dec.d2h(a.out_values, a.bytes_out)
                        if r.value_width == 0:
                            offs = self.dec.d2h(a.out_offsets, (a.values_out + 1) * 8, np.int64) if a.out_offsets \
                                else np.zeros(1, np.int64)
                finally:
                    self.dec.free_select(a)
                dic = None
                if keep:
                    dic = self.dec.convert_dictionary(i, cv) if cv is not None else self.dec.dictionary(i)
                out[self.file.columns[c].path.decode()] = DecodedColumn(
                    r.status, r.error_page, int(a.rows_out), int(a.values_out), width, lv, None, vals,
                    self.dec.pages(i), offs, dictionary=dic, logical=self._logical(c))
            return out
        finally:
            for a in sels:
                self.dec.free_select(a)
            for p in temps:
                self.dec.free(p)
            self.dec.free(dev)

    def prune_row_groups(self, filters):
        """The row groups whose footer statistics cannot rule out `filters` (as read_row_group
        takes them), in file order: a row group is dropped when every conjunction holds a term
        that no row of it can pass.  Conservative: a missing, truncated or odd statistic keeps the
        row group; FLOAT / DOUBLE never prune on != / not in or on a NaN bound.  With convert_logical
        the statistics of FLBA decimals order signed, literals may be typed, and an INT96 or
        BYTE_ARRAY decimal column never prunes.  Host only."""
        from . import filters as F
        dnf = F.parse(filters)
        keep = []
        for rg in range(self.file.num_row_groups):
            rows = self.file.row_group_rows(rg)

            def out(term):
                c = self.file.column_index(term.column)
                try:
                    st = self.file.chunk_stats(rg, c)
                except PqgError:
                    return False
                desc, lt = self.file.columns[c].desc, self._logical(c)
                if lt is not None and desc.physical_type == abi.INT96:
                    return False
                return F.term_rules_out(desc, term, st, rows, lt)

            if not all(any(out(t) for t in terms) for terms in dnf):
                keep.append(rg)
        return keep

    def read_row_group_nested(self, rg):
        """One row group's selected columns in Arrow layout: {path:
        NestedColumn} (pqgpu.nested).  Each chunk is decoded on the GPU, its
        device levels and values go through pqg_assemble_nested with the
        thresholds of the leaf's path (nested.leaf_thresholds), and only the
        Arrow buffers are downloaded: no level leaves the device.  A leaf under
        more than abi.MAX_LIST_DEPTH lists raises PqgError(UNSUPPORTED)."""
        from .nested import leaf_thresholds
        self._release()
        specs = [(rg, c) for c in self.selected]
        if not specs:
            return {}
        thr = {}
        for _, c in specs:  # before any decode: an unsupported depth costs no GPU work
            ld, ed = leaf_thresholds(self.file.schema_nodes, c)
            if len(ed) > abi.MAX_LIST_DEPTH:
                raise PqgError(abi.STATUS_CODES["UNSUPPORTED"], "column %s: %d list depths (at most %d)"
                               % (self.file.columns[c].path.decode(), len(ed), abi.MAX_LIST_DEPTH))
            thr[c] = (ld, ed)
        res, dev, nbytes = self._decode_spans(specs, self.keep_dict)
        self.uploaded_bytes += nbytes
        try:
            return {self.file.columns[c].path.decode(): self._nested_leaf(rg, i, c, r, thr[c])
                    for i, ((_, c), r) in enumerate(zip(specs, res))}
        finally:
            self.dec.free(dev)

    def _nested_leaf(self, rg, i, c, r, thr, lists=True):
        """Job i's result (column c, thresholds thr) through pqg_assemble_nested, downloaded as a
        NestedColumn; lists=False leaves the list depths' offsets and validity on the device."""
        path = self.file.columns[c].path.decode()
        if r.status != 0:
            raise PqgError(r.status, "column %s of row group %d" % (path, rg))
        desc = self.file.columns[c].desc
        ld, ed = thr
        # a leaf that kept its dictionary goes through as the 4-byte fixed-width leaf its keys are
        keep = bool(r.col_flags & abi.COL_KEEP_DICT)
        cv = self._conversion(c)
        values, width, offsets, ptype, flags, conv = r.values, r.value_width, r.offsets, desc.physical_type, \
            desc.flags, None
        if cv is not None:
            ptype, flags = cv.physical_type, 0
            if not keep:  # the dense leaf values converted: a fixed-width leaf of the output width
                conv = self.dec.convert(r.values, r.num_values, r.values_bytes, cv.kind, cv.in_width,
                                        cv.out_width, cv.unit, r.offsets if cv.in_width == 0 else None)
                values, width, offsets = conv, cv.out_width, None
        try:
            dic = None
            if keep:
                dic = self.dec.convert_dictionary(i, cv) if cv is not None else self.dec.dictionary(i)
            a = self.dec.assemble_nested(r.def_levels, r.rep_levels, values, r.num_slots, desc.max_def, ld, ed,
                                         value_width=width, value_offsets_ptr=offsets, validity=lists,
                                         offsets=lists)
            try:
                chars = self.dec.d2h(r.values, r.values_bytes) if offsets else None
                return self.dec.download_nested(a, chars, ptype, flags, dic)
            finally:
                self.dec.free_nested(a)
        finally:
            if conv is not None:
                self.dec.free(conv)

    def read_row_group_tree(self, rg):
        """One row group's selected columns as one Arrow column tree (pqgpu.tree): a non-nullable
        StructNode of `rows` slots whose children are the top-level fields, with structs, lists
        and maps as the schema nests them (tree.plan).  One decode of the selected chunks; per
        leaf one pqg_assemble_nested call; per representative leaf one pqg_assemble_structs call
        for the nullable structs it stands for (several when there are more than
        abi.MAX_STRUCTS).  Only Arrow buffers are downloaded: no level leaves the device.
        read_dictionary and convert_logical apply to the leaves as in read_row_group_nested; a
        chunk that fails raises the same PqgError, a leaf under more than abi.MAX_LIST_DEPTH lists
        PqgError(UNSUPPORTED) before any GPU work."""
        from . import tree
        from .nested import leaf_thresholds
        root = tree.plan(self.file.schema_nodes, self.file.schema_kinds, self.selected)
        rows = self.file.row_group_rows(rg)
        self._release()
        specs = [(rg, c) for c in self.selected]
        if not specs:
            return tree.build(root, {}, {}, rows)
        thr = {c: leaf_thresholds(self.file.schema_nodes, c) for _, c in specs}
        by_leaf, with_lists = tree.structs_by_leaf(root), tree.list_leaves(root)
        res, dev, nbytes = self._decode_spans(specs, self.keep_dict)
        self.uploaded_bytes += nbytes
        columns, structs, info = {}, {}, {}
        try:
            for i, ((_, c), r) in enumerate(zip(specs, res)):
                columns[c] = self._nested_leaf(rg, i, c, r, thr[c], lists=c in with_lists)
                cv = self._conversion(c)
                info[c] = dict(logical=self.file.logical_types[c], converted=cv is not None, unit=self.int96_unit)
                todo = by_leaf.get(c, [])
                desc = self.file.columns[c].desc
                for at in range(0, len(todo), abi.MAX_STRUCTS):
                    part = todo[at:at + abi.MAX_STRUCTS]
                    a = self.dec.assemble_structs(r.def_levels, r.rep_levels, r.num_slots, desc.max_def, thr[c][1],
                                                  [(p.depth, p.struct_def) for p in part])
                    try:
                        for p, st in zip(part, self.dec.download_structs(a)):
                            structs[p.node] = st
                    finally:
                        self.dec.free_structs(a)
            return tree.build(root, columns, structs, rows, info)
        finally:
            self.dec.free(dev)

    def next_row(self):
        """NextRow (file_reader.go:101-108): the next row of the selected
        columns as a dict (pqgpu.rows), decoding the next row group on the GPU
        when the current one is used up; EOFError after the last row."""
        if self._rows is None:
            from .rows import RowReader
            self._rows = RowReader(self.file, self.selected, self._decode_for_rows)
        return self._rows.next_row()

    def _decode_for_rows(self, rg):
        self._release()
        specs = [(rg, c) for c in self.selected]
        if not specs:
            return {}
        res, dev, nbytes = self._decode_spans(specs, ())
        self.uploaded_bytes += nbytes
        try:
            return {c: self.dec.download(r, i) for i, ((_, c), r) in enumerate(zip(specs, res))}
        finally:
            self.dec.free(dev)

    def close(self):
        self._release()
