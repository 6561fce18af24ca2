/*
 * pqgpu.h — C ABI of the MI355X (gfx950) Parquet column-chunk decoder.
 *
 * This is the drop-in boundary for parquet-go's page-decode path
 * (fraugster/parquet-go v0.2.1, mounted read-only at /root/reference).  Every
 * entry point below names the reference interface it replaces.  Signatures use
 * plain pointers and sizes only (no torch / HIP types), so a cgo, ctypes or
 * JNI binding can call them directly.
 *
 * Two libraries implement (parts of) this header:
 *   libpqgpu.so   (parquet-go_amd/csrc)  the product: HIP kernels + host runtime
 *   liboracle.so  (oracle/)              TEST INFRASTRUCTURE ONLY: the CPU
 *                                        restatement of the reference algorithm
 *                                        (pqo_* symbols), used as the parity checker.
 *
 * Semantics: a "chunk job" is one column chunk (ColumnChunk / ColumnMetaData of
 * one row group).  Decoding a job is what the reference does in
 *   readChunk      chunk_reader.go:314-378   (seek, level-decoder factories)
 *   readPages      chunk_reader.go:206-284   (page-header walk, dict page, V1/V2)
 *   readPageData   chunk_reader.go:380-402   (per page readValues)
 * and the per-page outputs are exactly pageReader.readValues
 * (interfaces.go:10-17; page_v1.go:27-55, page_v2.go:26-54):
 *   rLevels[numValues], dLevels[numValues], values[:notNull]
 * concatenated over the data pages of the chunk in file order (spec-correct
 * stitching; see DESIGN.md "Quirk policy" for the reference's Q1/Q2 defects).
 */
#ifndef PQGPU_H
#define PQGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- parquet.thrift enums (reference parquet/parquet.go: Type, Encoding :343,
 *      CompressionCodec :442, PageType :525) ------------------------------- */
enum {
  PQG_BOOLEAN = 0,
  PQG_INT32 = 1,
  PQG_INT64 = 2,
  PQG_INT96 = 3,
  PQG_FLOAT = 4,
  PQG_DOUBLE = 5,
  PQG_BYTE_ARRAY = 6,
  PQG_FIXED_LEN_BYTE_ARRAY = 7
};
enum {
  PQG_ENC_PLAIN = 0,
  PQG_ENC_PLAIN_DICTIONARY = 2,
  PQG_ENC_RLE = 3,
  PQG_ENC_BIT_PACKED = 4,
  PQG_ENC_DELTA_BINARY_PACKED = 5,
  PQG_ENC_DELTA_LENGTH_BYTE_ARRAY = 6,
  PQG_ENC_DELTA_BYTE_ARRAY = 7,
  PQG_ENC_RLE_DICTIONARY = 8,
  /* BYTE_STREAM_SPLIT (beyond the reference, which has no such decoder): data pages of
   * INT32 / INT64 / FLOAT / DOUBLE and of FIXED_LEN_BYTE_ARRAY with type_length >= 1;
   * on BOOLEAN / INT96 / BYTE_ARRAY / type_length < 1 the page's read error is
   * PQG_ERR_UNSUPPORTED.  A page of nn non-null values of w bytes holds w streams of nn
   * bytes, so its value bytes must be exactly nn * w: fewer is PQG_ERR_EOF (as for
   * PLAIN), more is PQG_ERR_SIZE (unlike PLAIN, which ignores trailing bytes: with
   * extra bytes the streams' stride is ambiguous); both are decode errors of the page. */
  PQG_ENC_BYTE_STREAM_SPLIT = 9
};
enum {
  PQG_CODEC_UNCOMPRESSED = 0,
  PQG_CODEC_SNAPPY = 1,
  PQG_CODEC_GZIP = 2,
  PQG_CODEC_ZSTD = 6,         /* parquet's CompressionCodec number, as 1 and 2 are */
  PQG_CODEC_LZ4_RAW = 7       /* one bare LZ4 block per page; 5, the Hadoop-framed LZ4, is unsupported */
};
enum {
  PQG_PAGE_DATA = 0,
  PQG_PAGE_INDEX = 1,
  PQG_PAGE_DICTIONARY = 2,
  PQG_PAGE_DATA_V2 = 3
};

/* ---- status codes --------------------------------------------------------
 * The reference returns a Go error (wrapped with github.com/pkg/errors) and
 * treats ANY error inside readPages/readPageData as fatal for the row group.
 * Parity is defined on error/no-error per page and per chunk; the class below
 * is this library's own classification, identical between libpqgpu and the
 * oracle (both follow the same cited reference lines). */
enum {
  PQG_OK = 0,
  PQG_ERR_EOF = -1,           /* io.EOF / io.ErrUnexpectedEOF inside a stream       */
  PQG_ERR_THRIFT = -2,        /* PageHeader thrift-compact decode failed            */
  PQG_ERR_PAGE_HEADER = -3,   /* missing sub-header, negative count/size            */
  PQG_ERR_SIZE = -4,          /* block shorter than compressed size / size mismatch; */
                              /* BYTE_STREAM_SPLIT: more value bytes than nn * w     */
  PQG_ERR_SNAPPY = -5,        /* snappy: corrupt input                              */
  PQG_ERR_RLE = -6,           /* hybrid: empty run, RLE value too large, bad varint */
  PQG_ERR_DICT_INDEX = -7,    /* dict: invalid index                                */
  PQG_ERR_BIT_WIDTH = -8,     /* dict/delta: invalid bit width                      */
  PQG_ERR_DELTA = -9,         /* DELTA_BINARY_PACKED header/stream invalid          */
  PQG_ERR_UNSUPPORTED = -10,  /* encoding / codec / type / page type                */
  PQG_ERR_DICT_PAGE = -11,    /* second dictionary page                             */
  PQG_ERR_BYTE_ARRAY = -12,   /* bytearray/plain: negative length                   */
  PQG_ERR_LEVELS = -13,       /* level decoder not initialised (V2, zero length)    */
  PQG_ERR_GZIP = -15,         /* gzip: invalid header / data / checksum (compress.go:63-76) */
  PQG_ERR_ZSTD = -16,         /* zstd: invalid frame / block / checksum             */
  PQG_ERR_LZ4 = -17,          /* lz4_raw: a block liblz4's LZ4_decompress_safe rejects */
  PQG_ERR_CRC = -18,          /* PageHeader.crc does not match the page's bytes; a   */
                              /* read-phase error, only with pqg_set_verify_crc on   */
  PQG_ERR_FIXED_LEN = -14,    /* DELTA_BYTE_ARRAY on FIXED_LEN_BYTE_ARRAY: a value  */
                              /* whose length is not type_length (the reference     */
                              /* returns it; the fixed-width output cannot hold it) */
  PQG_ERR_NOT_DICT = -19,     /* PQG_COL_KEEP_DICT: a data page that is not dictionary */
                              /* encoded (a read-phase error of that page)            */
  PQG_ERR_CAPACITY = -20,     /* internal: arena too small; host grows and retries  */
  PQG_ERR_INVALID_ARG = -21,
  PQG_ERR_HIP = -22,
  PQG_ERR_METADATA = -23,     /* footer / FileMetaData problems                      */
  PQG_ERR_NOT_BUILT = -24,
  PQG_ERR_INDEX = -25         /* located decode: a listed page whose header and body do */
                              /* not end at offset + size (a read-phase error)           */
};

/* page_info.flags */
enum {
  PQG_PAGE_FLAG_INT96_NIL = 1,  /* Q8: truncated final INT96 value left nil by the
                                   reference (type_int96.go:21-42); bytes are 0 */
  PQG_PAGE_FLAG_SNAPPY_SERIAL = 2, /* libpqgpu diagnostic: the page's snappy block was
                                   decoded whole by one wave (its 64 KiB sub-block
                                   split failed: a copy across a 64 KiB block
                                   boundary, or a corrupt block) */
  PQG_PAGE_FLAG_INFLATE_REDO = 64 /* libpqgpu diagnostic: the page's GZIP stream was
                                   decoded again with the full 32 KiB window ring
                                   (a match reached back past the 8 KiB ring to
                                   bytes past the page's size) */
};

/* ---- column / chunk description ----------------------------------------- */

/* What readChunk learns from the schema (schema.go:789-894) and the chunk's
 * ColumnMetaData (parquet.go ColumnMetaData). */
typedef struct pqg_column_desc {
  int32_t physical_type; /* PQG_INT32 ...                                        */
  int32_t type_length;   /* FIXED_LEN_BYTE_ARRAY length; -1 = unset (nil)        */
  int32_t max_def;       /* Column.MaxDefinitionLevel()  (0..255)                */
  int32_t max_rep;       /* Column.MaxRepetitionLevel()  (0..255)                */
  int32_t codec;         /* ColumnMetaData.codec                                 */
  int32_t flags;         /* bit0: unsigned (uint32/uint64 Go type; bits identical) */
                         /* bit1: PQG_COL_KEEP_DICT                               */
} pqg_column_desc;

/* pqg_column_desc.flags.  PQG_COL_KEEP_DICT (pqg_decode_chunks[_async] / pqg_sync only):
 * the chunk is not materialised.  Its result holds the dictionary keys the file stores:
 * value_width = 4, `values` = num_values little-endian int32 keys, dense, in page order,
 * offsets = NULL, values_bytes = 4 * num_values; levels, num_slots, num_values, num_pages
 * and the page table are those of the decode without the flag.  The dictionary itself
 * comes from pqg_get_dictionary.  A data page of such a job whose encoding is not
 * RLE_DICTIONARY / PLAIN_DICTIONARY (the PLAIN pages after a writer's dictionary overflow,
 * DELTA_*, BYTE_STREAM_SPLIT) fails its read phase with PQG_ERR_NOT_DICT; every other
 * error is the one the decode without the flag reports, on the same page.  BOOLEAN
 * columns have no dictionary encoding: the flag on one is PQG_ERR_INVALID_ARG at submit,
 * and so is the flag in pqg_decode_page. */
enum {
  PQG_COL_UNSIGNED = 1,
  PQG_COL_KEEP_DICT = 2,
  PQG_COL_SIGNED_BE = 4  /* pqg_filter only: FIXED_LEN_BYTE_ARRAY values are big-endian two's
                            complement (a DECIMAL) and order as such; never set by pqg_file_column */
};

/* One column chunk to decode.  `data` points at the chunk's first page
 * (DictionaryPageOffset when set, else DataPageOffset — chunk_reader.go:332-340).
 * For pqg_decode_chunks it is a DEVICE pointer (bytes resident in HBM); for the
 * oracle it is a host pointer. */
typedef struct pqg_chunk_job {
  pqg_column_desc col;
  const uint8_t* data;
  int64_t data_len;              /* readable bytes at data (>= total_compressed_size) */
  int64_t total_compressed_size; /* ColumnMetaData.total_compressed_size              */
  int64_t data_page_offset;      /* DataPageOffset - first-page offset (>= 0)          */
  int64_t num_values_hint;       /* ColumnMetaData.num_values (capacity hint only)     */
  int64_t total_uncompressed_size; /* ColumnMetaData.total_uncompressed_size (hint)     */
  int32_t has_dict_page_offset;  /* ColumnMetaData.DictionaryPageOffset != nil         */
  int32_t quirks;                /* PQG_QUIRK_* mask; libpqgpu decodes spec-correctly
                                    and rejects a non-zero mask (PQG_ERR_INVALID_ARG):
                                    quirk reproduction is the oracle's triage mode
                                    (pqo_decode_column_store)                        */
} pqg_chunk_job;

/* The reference's caller-side stitching defects (DESIGN.md "Quirk
 * policy").  Q1: readPageData appends each page's whole numValues-long slice,
 * numValues - notNull trailing nils included (chunk_reader.go:394-397).  Q2:
 * from the second row group on, the dictionary page decodes into the column
 * store's reused backing array (chunk_reader.go:235, page_dict.go:50-53), which
 * the first data page's append then overwrites (type_dict.go:72-79). */
enum {
  PQG_QUIRK_Q1_PAGE_NILS = 1,
  PQG_QUIRK_Q2_DICT_ALIAS = 2
};

/* Decoded column chunk.  Fixed-width physical types (INT32/INT64/INT96/FLOAT/
 * DOUBLE/FLBA>0/BOOLEAN) store values densely, little endian, `value_width`
 * bytes each (BOOLEAN: one byte 0/1).  BYTE_ARRAY (and FLBA with length 0)
 * store the value bytes back to back in `values` (values_bytes = chars) and
 * num_values+1 int64 `offsets` (offsets[0] = 0, value i = chars
 * [offsets[i], offsets[i+1]); Arrow large-binary layout).  Pointers are DEVICE
 * pointers for libpqgpu (owned by the ctx, valid until the next decode on that
 * ctx or pqg_ctx_destroy) and malloc'ed host pointers for the oracle. */
typedef struct pqg_chunk_result {
  int32_t status;      /* first error in reference order (read phase, then decode) */
  int32_t error_page;  /* index into the page list of the failing page, -1 if none */
  int32_t num_pages;   /* pages seen (dictionary page included)                    */
  int32_t value_width; /* bytes per value; 0 = variable length (offsets)           */
  int32_t col_flags;   /* the job's pqg_column_desc.flags, echoed: bit0 unsigned,  */
                       /* bit1 PQG_COL_KEEP_DICT (values are int32 keys)           */
                       /* (the Go adapter boxes uint32/uint64 from it, as          */
                       /* int32PlainDecoder.unSigned does, type_int32.go:29-33)    */
  int32_t reserved;
  int64_t num_slots;   /* Σ data-page num_values  (= level entries)                */
  int64_t num_values;  /* Σ notNull                                                */
  int64_t values_bytes;
  uint8_t* def_levels; /* num_slots bytes, NULL when max_def == 0                  */
  uint8_t* rep_levels; /* num_slots bytes, NULL when max_rep == 0                  */
  uint8_t* values;
  int64_t* offsets;    /* variable-length values only                              */
} pqg_chunk_result;

/* Per page bookkeeping (dictionary page included, in file order). */
typedef struct pqg_page_info {
  int64_t header_offset;     /* relative to job.data                    */
  int64_t payload_offset;    /* first byte after the thrift header      */
  int64_t slot_offset;       /* Σ num_values of preceding data pages    */
  int64_t value_offset;      /* Σ not_null  of preceding data pages     */
  int32_t page_type;
  int32_t encoding;
  int32_t num_values;        /* header NumValues                        */
  int32_t not_null;          /* #(dLevel == maxD)                        */
  int32_t compressed_size;
  int32_t uncompressed_size;
  int32_t def_len;           /* V2 DefinitionLevelsByteLength           */
  int32_t rep_len;           /* V2 RepetitionLevelsByteLength           */
  int32_t def_encoding;      /* V1 definition_level_encoding            */
  int32_t rep_encoding;
  int32_t status;
  int32_t flags;             /* PQG_PAGE_FLAG_*                          */
} pqg_page_info;

/* ======================= libpqgpu (product) =============================== */

typedef struct pqg_ctx pqg_ctx;

/* One context per GPU; owns a HIP stream and grow-only device arenas.
 * (No reference counterpart: parquet-go's reader is one goroutine per FileReader.) */
int pqg_ctx_create(int device, pqg_ctx** out);
void pqg_ctx_destroy(pqg_ctx* ctx);
const char* pqg_status_string(int status);

/* Device memory helpers for callers without their own allocator (cgo). */
int pqg_device_alloc(pqg_ctx* ctx, int64_t bytes, void** dptr);
int pqg_device_free(pqg_ctx* ctx, void* dptr);
int pqg_memcpy_h2d(pqg_ctx* ctx, void* dst, const void* src, int64_t bytes);
int pqg_memcpy_d2h(pqg_ctx* ctx, void* dst, const void* src, int64_t bytes);

/* Decode a batch of column chunks already resident in HBM.  Replaces, for
 * every job, readChunk+readPages+readPageData (chunk_reader.go:206-402) and the
 * valuesDecoder / levelDecoder implementations they call (interfaces.go:28-38,
 * hybrid_decoder.go:17-28).  Enqueues work on the ctx stream and returns;
 * pqg_sync waits and fills `results` (n_jobs entries). */
int pqg_decode_chunks_async(pqg_ctx* ctx, const pqg_chunk_job* jobs, int n_jobs);
int pqg_sync(pqg_ctx* ctx, pqg_chunk_result* results, int n_jobs);
/* Convenience: async + sync. */
int pqg_decode_chunks(pqg_ctx* ctx, const pqg_chunk_job* jobs, int n_jobs,
                      pqg_chunk_result* results);

/* ---- located decode: the pages of a chunk given by the caller (an OffsetIndex) ---------
 *
 * A job decoded with a list of page locations is not scanned for page headers: each listed
 * page's header is parsed where the list says it is.  The list may be any subset of the
 * chunk's pages, in ascending order.  Its meaning is that of a scanned decode: the located
 * decode of job J with locations L gives what pqg_decode_chunks gives for the job J' whose
 * `data` is the bytes of L's pages back to back, with total_compressed_size = the sum of the
 * sizes, has_dict_page_offset = 0 and everything else as in J -- levels, values, offsets,
 * num_slots, num_values, status, error_page and every page-table field but header_offset and
 * payload_offset, which stay relative to J.data.  So the dictionary page, when wanted, is
 * simply the first location; a list without it, of it alone, or of every other data page is
 * legal and means what J' means.  One addition: a listed page whose own read phase is fine
 * but whose header and body do not end at offset + size fails its read phase with
 * PQG_ERR_INDEX; it ranks like any read-phase error (the first failing page in list order
 * wins, the pages before it are reported, no decoder reads it).
 *
 * pages[i].n == 0: job i is scanned as by pqg_decode_chunks; one batch may mix both kinds.
 * Of a located job, total_compressed_size, data_page_offset and has_dict_page_offset are
 * capacity hints only.  PQG_ERR_INVALID_ARG, with nothing enqueued: n < 0, an offset < 0, a
 * size <= 0, offset + size > data_len, offsets that do not ascend or ranges that overlap.
 * PQG_COL_KEEP_DICT, pqg_set_verify_crc, pqg_get_pages, pqg_get_dictionary,
 * pqg_get_page_crcs and pqg_last_timings work as after a scanned decode; pqg_debug_job
 * reports out[0] = 3 and 0 candidates for a located job.  The lists are copied at submit. */
typedef struct pqg_page_loc {
  int64_t offset;      /* of the PageHeader; for the decode: relative to job.data */
  int32_t size;        /* header + body, PageLocation.compressed_page_size */
  int32_t reserved;
  int64_t first_row;   /* PageLocation.first_row_index; not used by the decode */
} pqg_page_loc;
typedef struct pqg_chunk_pages {
  const pqg_page_loc* locs; /* HOST */
  int32_t n;
  int32_t reserved;
} pqg_chunk_pages;
int pqg_decode_chunks_located_async(pqg_ctx* ctx, const pqg_chunk_job* jobs, const pqg_chunk_pages* pages, int n_jobs);
/* Convenience: async + pqg_sync. */
int pqg_decode_chunks_located(pqg_ctx* ctx, const pqg_chunk_job* jobs, const pqg_chunk_pages* pages, int n_jobs,
                              pqg_chunk_result* results);

/* More of the located contract.  A `pages[i]` with n > 0 and a NULL `locs` is PQG_ERR_INVALID_ARG, and so
 * is a batch that lists more than INT32_MAX / 2 pages in all.  A listed page's header is read within
 * [offset, offset + size), but its body is checked against job.data_len, as a scanned page's is: a page
 * listed too short reports PQG_ERR_INDEX where the bytes after it are resident, and PQG_ERR_SIZE where
 * the list's end is the end of the data (the last page of a packed upload). */

/* ---- the page index (host parsers; parquet.thrift OffsetIndex / ColumnIndex) --------------
 * pqg_file_chunk_index: where a chunk's indexes lie in the file (ColumnChunk fields 4-7); a length of 0
 * means that index is absent.  The parsers take the index's bytes as the file holds them and trust
 * nothing: PQG_ERR_METADATA for a truncated or malformed struct, bytes left over, parallel lists of
 * different lengths, a size <= 0, negative or descending offsets or first rows, overlapping pages, a
 * negative null count or an unknown boundary order.
 * pqg_parse_offset_index returns the number of locations (the first `cap` are written; offsets are
 * absolute file offsets as stored).  A parsed ColumnIndex is a handle: pqg_column_index_page gives page
 * `page`'s bounds and null count as a pqg_chunk_stats: pointers owned by the handle, min / max NULL for a
 * null page, null_count -1 when the index has none; and whether it is a null page.
 * pqg_column_index_boundary_order is 0 unordered, 1 ascending, 2 descending. */
typedef struct pqg_index_ranges {
  int64_t offset_index_offset;
  int64_t column_index_offset;
  int32_t offset_index_length;
  int32_t column_index_length;
} pqg_index_ranges;
typedef struct pqg_column_index pqg_column_index;
struct pqg_file;
struct pqg_chunk_stats;
int pqg_file_chunk_index(const struct pqg_file* f, int row_group, int col, pqg_index_ranges* out);
int pqg_parse_offset_index(const uint8_t* buf, int64_t len, pqg_page_loc* out, int cap);
int pqg_column_index_parse(const uint8_t* buf, int64_t len, pqg_column_index** out);
int pqg_column_index_pages(const pqg_column_index* ci);
int pqg_column_index_page(const pqg_column_index* ci, int page, struct pqg_chunk_stats* out, int32_t* null_page);
int pqg_column_index_boundary_order(const pqg_column_index* ci);
void pqg_column_index_free(pqg_column_index* ci);

/* ---- page-level and codec-level entries ------------------------------------ */

/* One data page (and optionally its chunk's dictionary page), both DEVICE
 * pointers to a thrift PageHeader followed by the page body.  Decoding it is
 * pageReader.read + readValues (interfaces.go:10-17; page_v1.go:27-108,
 * page_v2.go:26-129, dictionary: page_dict.go:30-64): the result holds that
 * page's rLevels, dLevels and values[:notNull] (or chars + offsets), the page
 * table lists the dictionary page (if any) and the data page. */
typedef struct pqg_page_job {
  pqg_column_desc col;
  const uint8_t* page;       /* DEVICE: PageHeader + body of a DATA_PAGE / DATA_PAGE_V2 */
  int64_t page_len;
  const uint8_t* dict_page;  /* DEVICE: PageHeader + body of the DICTIONARY_PAGE, or NULL */
  int64_t dict_page_len;
} pqg_page_job;
int pqg_decode_page(pqg_ctx* ctx, const pqg_page_job* job, pqg_chunk_result* result);

/* BlockCompressor.DecompressBlock (compress.go:24-27, 46-48, registered with
 * RegisterBlockCompressor compress.go:124-135): decompress one HOST block
 * synchronously on the GPU.  codec SNAPPY (snappy.Decode semantics: decoded
 * length from the block's varint header, ErrCorrupt -> PQG_ERR_SNAPPY), GZIP
 * (gzipCompressor.DecompressBlock, compress.go:63-76: multistream members,
 * a bad header / block / CRC / ISIZE or trailing bytes -> PQG_ERR_GZIP), ZSTD
 * (libzstd's ZSTD_decompress over the whole block: any number of frames and
 * skippable frames, content checksums verified, no dictionaries; an invalid
 * frame / block / checksum, a content size that differs from the decoded one
 * or trailing bytes -> PQG_ERR_ZSTD), LZ4_RAW (one bare LZ4 block, as liblz4's
 * LZ4_decompress_safe decodes it into a buffer of 255 * n + 64 bytes, which no
 * block can fill; a block it rejects, n == 0 among them -> PQG_ERR_LZ4) or
 * UNCOMPRESSED (a copy).  *out_len is the decoded length; PQG_ERR_CAPACITY
 * when it exceeds `cap` (nothing written). */
int pqg_block_decompress(pqg_ctx* ctx, int codec, const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap,
                         int64_t* out_len);

/* ColumnStore refill (the Go adapter's half of the drop-in): pack `n` levels
 * (u8, DEVICE) the way packedArray stores them (packed_array.go:34-101): width
 * bw = bits.Len16(max_level), each group of 8 levels in bw bytes in the
 * unpack8int32 layout (LSB first, bitbacking32.go), the last group zero padded
 * (packedArray.flush).  `packed` (DEVICE) receives ceil(n/8) * bw bytes; a
 * packedArray refill takes the floor(n/8) * bw bytes as `data` and the last
 * n % 8 levels as its pending buffer. */
int pqg_pack_levels(pqg_ctx* ctx, const uint8_t* levels, int64_t n, int max_level, uint8_t* packed);

/* After pqg_sync: page table of job `job` (host copy).  Returns pages written
 * or a negative status. */
int pqg_get_pages(pqg_ctx* ctx, int job, pqg_page_info* out, int cap);

/* The dictionary of a PQG_COL_KEEP_DICT job, after the batch's pqg_sync and until the
 * next decode on the ctx (PQG_ERR_INVALID_ARG for a job without the flag).  Pointers are
 * DEVICE pointers.  Fixed-width columns: `values` are the count entries of value_width
 * bytes, read in place as the decoder reads them (the chunk's own bytes, or the ctx
 * scratch for a compressed dictionary page; the former are the caller's buffer, which must
 * stay allocated while the dictionary is used), values_bytes = count * value_width -- less
 * for a truncated INT96 page, whose entry nil_entry has fewer than 12 bytes there and
 * reads as zero bytes (Q8).  Byte arrays: `values` are the entries' chars back to back
 * and `offsets` count + 1 int64 (entry i = chars [offsets[i], offsets[i+1])).  A chunk
 * without a (valid) dictionary page reports count 0, page -1 and NULL pointers. */
typedef struct pqg_dictionary {
  const uint8_t* values;   /* DEVICE                                              */
  const int64_t* offsets;  /* DEVICE, count + 1 entries; NULL for fixed width     */
  int64_t count;
  int64_t values_bytes;
  int32_t value_width;     /* bytes per entry; 0 = byte arrays                    */
  int32_t nil_entry;       /* the INT96 entry that reads as zero bytes, -1: none  */
  int32_t page;            /* index of the dictionary page in the page list, -1   */
  int32_t reserved;
} pqg_dictionary;
int pqg_get_dictionary(pqg_ctx* ctx, int job, pqg_dictionary* out);

/* Kernel timing of the last decode (HIP events on the ctx stream), in ms:
 * out[0] = whole pipeline, out[1..] = per stage. Returns the
 * number of entries written. */
int pqg_last_timings(pqg_ctx* ctx, float* out, int cap);

/* Per-stage HIP events on the ctx stream (on by default): `on` = 0 records
 * none (pqg_last_timings then returns 0 entries until a timed decode), 1
 * records them.  The
 * events are instrumentation: each costs a few microseconds of stream time,
 * which matters for small batches. */
int pqg_set_timing(pqg_ctx* ctx, int on);

/* ---- page checksums (PageHeader.crc, field 4) -----------------------------
 * Off by default (PQG_VERIFY_CRC=0/1 in the environment sets a new context's
 * value); `on` holds for later decodes on the ctx, pqg_decode_page included.
 * With it on, every page whose header holds field 4 as an i32 (the last one
 * if it appears twice) and whose own read phase is OK is checked before any
 * decoder reads it: CRC-32 as in zlib / gzip over the compressed_page_size
 * bytes that follow the thrift header, as stored (V2: levels and values
 * together; dictionary pages the same), compared as uint32.  A mismatch is a
 * read-phase error of that page, PQG_ERR_CRC: it ranks in
 * pqg_chunk_result.status / error_page before any decode error, the first
 * failing page in file order wins, and no decoder reads the page.  Pages
 * without the field decode as with verification off. */
int pqg_set_verify_crc(pqg_ctx* ctx, int on);

typedef struct pqg_page_crc {
  uint32_t stored;    /* PageHeader.crc as uint32 (0 when absent)                */
  uint32_t computed;  /* CRC-32 of the page's bytes (states 1 and 2)             */
  int32_t state;      /* PQG_CRC_*                                               */
  int32_t reserved;
} pqg_page_crc;
enum {
  PQG_CRC_NONE = 0,         /* the header has no crc field                       */
  PQG_CRC_VERIFIED = 1,
  PQG_CRC_MISMATCH = 2,
  PQG_CRC_NOT_CHECKED = 3,  /* verification off, or a read error of the page itself */
};
/* After pqg_sync: the checksum record of each page pqg_get_pages reports for
 * job `job`, in the same order.  Returns entries written or a negative status. */
int pqg_get_page_crcs(pqg_ctx* ctx, int job, pqg_page_crc* out, int cap);

/* zlib's crc32 of the device buffer [dev, dev + n), by the kernel that checks
 * the pages (n == 0 -> 0).  Only 16-byte granules that hold a byte of the
 * range are loaded.  Synchronises the ctx stream. */
int pqg_crc32(pqg_ctx* ctx, const uint8_t* dev, int64_t n, uint32_t* out);

/* Device time in ms of the checksum kernels of the last decode (0 when it
 * ran none: verification off, or stage timing off). */
int pqg_last_crc_ms(pqg_ctx* ctx, float* ms);

/* Optional: run `iters` back-to-back decodes of the same jobs on the ctx
 * stream and return the device time in ms (used by bench.py).  */
int pqg_bench_decode(pqg_ctx* ctx, const pqg_chunk_job* jobs, int n_jobs, int iters,
                     float* ms_total, float* ms_stage, int stage_cap);

/* Diagnostics of the last decode for job `job` (after pqg_sync): out[0] = 1
 * when its page list came from the serial header walk (K1e) instead of the
 * speculative parallel scan, out[1] = header candidates found, out[2] =
 * pages, out[3] = decompressed scratch bytes, out[4] = pipeline launches of
 * the whole last decode call (1 unless an arena had to grow; grown capacities
 * are remembered per chunk for later calls).  Returns entries written. */
int pqg_debug_job(pqg_ctx* ctx, int job, int64_t* out, int cap);

/* Diagnostic builds only (compiled with -DPQG_PROFILE): in-kernel phase cycle
 * counters accumulated since the last call, then reset.  Returns the number of
 * counters written (0 in normal builds). */
int pqg_debug_counters(pqg_ctx* ctx, uint64_t* out, int cap);

/* ---- K8: level assembly (null scatter / record and list offsets) ----------
 * Replaces the per-slot cursor walk of ColumnStore.get (data_store.go:158-203)
 * and Column.getData (schema.go:235-264): a slot with dLevel < maxD is a null
 * (level cursor advances, value cursor does not); a slot with rLevel <
 * maxR ends the current repeated object.  Evaluated for every slot at once:
 *   valid(i)    = def[i] == max_def          (def_levels NULL → all valid)
 *   boundary(i) = rep[i] <= boundary_level   (rep_levels NULL → every slot)
 * boundary_level 0 = record starts (rLevel 0 → new row); max_rep-1 = the
 * objects ColumnStore.get returns.  All pointers are DEVICE pointers (e.g. a
 * pqg_chunk_result's def_levels/rep_levels/values); any output may be NULL. */
typedef struct pqg_assemble_args {
  const uint8_t* def_levels; /* num_slots bytes or NULL                          */
  const uint8_t* rep_levels; /* num_slots bytes or NULL                          */
  const uint8_t* values;     /* dense fixed-width values (num_valid × width)     */
  int64_t num_slots;
  int32_t max_def;
  int32_t boundary_level;
  int32_t value_width;       /* bytes per value; needed when values_spaced set   */
  int32_t reserved;
  uint8_t* validity;         /* out: ceil(num_slots/8) bytes, LSB-first bits     */
  uint8_t* values_spaced;    /* out: num_slots × value_width, nulls zeroed       */
  int64_t* offsets;          /* out: num_boundaries+1 entries (cap num_slots+1): */
                             /* the SLOT index of each boundary, then num_slots  */
                             /* (a null or empty list still takes its slot; for  */
                             /* Arrow LIST element offsets: pqg_assemble_list)   */
  int64_t num_valid;         /* out: #valid slots (= notNull total)              */
  int64_t null_count;        /* out: num_slots - num_valid                       */
  int64_t num_boundaries;    /* out: #boundary slots (rows / objects)            */
} pqg_assemble_args;

/* Enqueue K8 on the ctx stream and wait; fills the three counts. */
int pqg_assemble(pqg_ctx* ctx, pqg_assemble_args* args);

/* ---- K8 list export: Arrow LIST layout of a repeated leaf (max_rep == 1) ----
 * The record assembly of a LIST column (Column.getData schema.go:235-264 over
 * ColumnStore.get data_store.go:158-203) evaluated for every slot at once:
 *   row start     rep[i] == 0 (rep_levels NULL: every slot)
 *   element slot  def[i] >= elem_def          (the repeated group is present)
 *   valid element def[i] == max_def           (consumes the next dense value)
 *   row validity  def[row start] >= list_def  (else the list itself is null)
 * For the 3-level LIST<T> written by parquet-mr / pyarrow (optional group (LIST)
 * { repeated group list { optional T element } }: maxD = 3, maxR = 1):
 * list_def = 1, elem_def = 2 — def 0 null list, 1 empty list, 2 null element,
 * 3 value.  Outputs (DEVICE pointers, any may be NULL):
 *   list_validity  one bit per row, LSB first           (zeroed by the call)
 *   list_offsets   int32[rows + 1]: elements before each row, then the total
 *   elem_validity  one bit per element, LSB first       (zeroed by the call)
 *   elem_values    elements x value_width, null elements zeroed
 * Buffers must hold rows / elements <= num_slots entries; the two bitmaps are
 * written as whole dwords: give them 4 * ceil(num_slots / 32) bytes. */
typedef struct pqg_list_args {
  const uint8_t* def_levels; /* num_slots bytes (required)                        */
  const uint8_t* rep_levels; /* num_slots bytes or NULL                           */
  const uint8_t* values;     /* dense values (num_valid x value_width)            */
  int64_t num_slots;
  int32_t max_def;
  int32_t list_def;
  int32_t elem_def;
  int32_t value_width;
  uint8_t* list_validity;
  int32_t* list_offsets;
  uint8_t* elem_validity;
  uint8_t* elem_values;
  int64_t num_rows;          /* out */
  int64_t num_elements;      /* out */
  int64_t num_valid;         /* out: valid elements (= dense values consumed)     */
  int64_t null_lists;        /* out */
} pqg_list_args;

/* Enqueue the list export on the ctx stream and wait; fills the counts.
 * PQG_ERR_INVALID_ARG when elements exceed int32 offsets. */
int pqg_assemble_list(pqg_ctx* ctx, pqg_list_args* args);

/* ---- K8 nested export: Arrow layout of every list depth on a leaf's path ----
 * The general form of the list export, for a leaf under depth = max_rep lists
 * (0..PQG_MAX_LIST_DEPTH) with a fixed-width or a byte-array value.  It
 * replaces the recursion of Column.getData / getNextData (schema.go:171-264)
 * over ColumnStore.get (data_store.go:158-203).  Depth k (1..depth) has two
 * definition-level thresholds, level[k-1].elem_def (the k-th REPEATED node of
 * the path: the list has an element) and level[k-1].list_def (the list is not
 * null).  With elem_def[0] = 0, for slot i:
 *   entry_k(i) = rep[i] <= k-1 && def[i] >= elem_def[k-1]   a depth-k list starts
 *   valid_k(i) = def[i] >= list_def[k]                      its validity bit
 *   elem_k(i)  = rep[i] <= k   && def[i] >= elem_def[k]     (= entry_{k+1})
 *   leaf(i)    = elem_depth(i);  leaf_valid(i) = def[i] == max_def
 *   offsets_k[rank entry_k(i)] = #elem_k before i;  offsets_k[#entry_k] = #elem_k
 * valid_k's bit goes at rank entry_k(i), the leaf's at rank leaf(i).  A
 * fixed-width leaf value is dense[rank leaf_valid], zeros for a null; a
 * byte-array leaf gets leaf_offsets[e] = value_offsets[#valid before e] and
 * leaf_offsets[num_leaf] = value_offsets[num_valid], so a null is an empty
 * string over the decoded chars as they are.  rep_levels NULL: every rep is 0;
 * def_levels NULL (only with max_def == 0): everything is present.  depth 1 is
 * pqg_assemble_list; depth 0 is flat validity and spaced values / offsets.
 * Required: elem_def[k-1] <= list_def[k] <= elem_def[k] <= max_def with
 * elem_def strictly increasing (PQG_ERR_INVALID_ARG); depth outside
 * 0..PQG_MAX_LIST_DEPTH is PQG_ERR_UNSUPPORTED; leaf_values needs values and
 * value_width > 0, leaf_offsets needs value_offsets.  More elements at any
 * depth than int32 offsets hold is PQG_ERR_INVALID_ARG.  No output is written
 * when the call fails.  Bitmaps are zeroed by the call and written as whole
 * dwords. */
#define PQG_MAX_LIST_DEPTH 4
typedef struct pqg_nested_level {
  int32_t list_def, elem_def;
  uint8_t* validity;     /* out, DEVICE, 4*ceil(num_slots/32) bytes, or NULL */
  int32_t* offsets;      /* out, DEVICE, entries+1 (cap num_slots+1), or NULL */
  int64_t num_entries;   /* out */
  int64_t null_count;    /* out */
} pqg_nested_level;
typedef struct pqg_nested_args {
  const uint8_t *def_levels, *rep_levels, *values;
  const int64_t* value_offsets;     /* byte-array leaf: the chunk result's offsets, else NULL */
  int64_t num_slots;
  int32_t max_def, depth, value_width, reserved;
  pqg_nested_level level[PQG_MAX_LIST_DEPTH];
  uint8_t* leaf_validity; /* out: 4*ceil(num_slots/32) bytes */
  uint8_t* leaf_values;   /* out: num_leaf x value_width (cap num_slots) */
  int64_t* leaf_offsets;  /* out: num_leaf+1 (cap num_slots+1); any of the three may be NULL */
  int64_t num_rows, num_leaf, num_valid;                                /* out */
} pqg_nested_args;
int pqg_assemble_nested(pqg_ctx* ctx, pqg_nested_args* args);

/* ---- K8 struct export: validity bitmaps of the structs on a leaf's path ------
 * The nested export gives the lists and the leaf; this gives the structs (the
 * groups that are neither lists nor maps) above the same leaf, up to
 * PQG_MAX_STRUCTS of them a call, all from one read of the level streams.  A
 * struct under R lists (R = 0..depth) that is present at def >= struct_def has,
 * with elem_def[0] = 0 and elem_def as in pqg_nested_level, for slot i:
 *   entry(i) = rep[i] <= R && def[i] >= elem_def[R]    one struct slot (R = 0: one per row)
 *   valid(i) = def[i] >= struct_def
 * valid's bit goes at rank entry(i); num_entries = #entry, null_count =
 * #(entry && !valid).  Every level up to struct_def lies on the part of the
 * path that all leaves below the struct share, so any of them gives the same
 * bits.  A struct below a null ancestor struct still has its slot, with bit 0.
 * validity NULL: the struct is only counted.  rep_levels NULL (depth 0 only):
 * every rep is 0.  depth outside 0..PQG_MAX_LIST_DEPTH is PQG_ERR_UNSUPPORTED;
 * PQG_ERR_INVALID_ARG: num_structs outside 0..PQG_MAX_STRUCTS, a struct's
 * depth outside 0..depth, elem_def not strictly increasing or above max_def, a
 * struct_def not in (elem_def[R], max_def] or (R < depth) not below
 * elem_def[R+1], def_levels NULL with structs and slots, rep_levels NULL with
 * depth > 0.  num_slots == 0 does nothing (all counts 0).  No output is
 * written when the call fails.  Bitmaps are zeroed by the call and written as
 * whole dwords; bits at and past num_entries are zero. */
#define PQG_MAX_STRUCTS 8
typedef struct pqg_struct_level {
  int32_t depth;        /* lists above the struct on the path: 0 .. args.depth            */
  int32_t struct_def;   /* the struct is present when def >= struct_def                   */
  uint8_t* validity;    /* out, DEVICE, 4 * ceil(num_slots / 32) bytes, or NULL (count)   */
  int64_t num_entries;  /* out: struct slots                                              */
  int64_t null_count;   /* out                                                            */
} pqg_struct_level;
typedef struct pqg_struct_args {
  const uint8_t *def_levels, *rep_levels;   /* DEVICE; rep NULL: every rep is 0           */
  int64_t num_slots;
  int32_t max_def, depth;                   /* depth = lists on the leaf's path (max_rep) */
  int32_t elem_def[PQG_MAX_LIST_DEPTH];     /* as in pqg_nested_level                     */
  int32_t num_structs, reserved;
  pqg_struct_level st[PQG_MAX_STRUCTS];
} pqg_struct_args;
/* Enqueue the struct export on the ctx stream and wait; fills the counts. */
int pqg_assemble_structs(pqg_ctx* ctx, pqg_struct_args* args);

/* Device time (ms) of the K8 kernels of the last pqg_assemble /
 * pqg_assemble_list / pqg_assemble_nested / pqg_assemble_structs call: HIP events on the ctx
 * stream around its kernel launches (the count read-back and host syncs excluded). */
int pqg_last_assemble_ms(pqg_ctx* ctx, float* ms);

/* ---- K9s: row predicates and row selection (beyond the reference, which has no
 * filter: FileReader returns every row of a row group) ------------------------
 * Rows are those of a FLAT column (max_rep == 0: num_rows == num_slots).  Row i is
 * null when def[i] < max_def (def_levels NULL: no row is null), and dense value r
 * belongs to the r-th non-null row.  All array pointers are DEVICE pointers (e.g. a
 * pqg_chunk_result's); both entries enqueue on the ctx stream and wait, write no
 * output when they fail, and do nothing when num_rows == 0 (counts 0). */
enum {
  PQG_OP_EQ = 0, PQG_OP_NE = 1, PQG_OP_LT = 2, PQG_OP_LE = 3, PQG_OP_GT = 4, PQG_OP_GE = 5,
  PQG_OP_IS_NULL = 6, PQG_OP_NOT_NULL = 7
};
enum {
  PQG_COMBINE_SET = 0,  /* bitmap  = result          */
  PQG_COMBINE_AND = 1,  /* bitmap &= result          */
  PQG_COMBINE_OR = 2    /* bitmap |= result          */
};

/* pqg_filter: one comparison `column op literal` into a row bitmap: one bit per row,
 * LSB first, 4 * ceil(num_rows / 32) bytes, read (AND / OR) and written as whole
 * dwords.  Bits at and past num_rows are zero after every call, whatever the operator
 * or mode.  A null row fails every comparison, NE included, and passes only IS_NULL.
 * Comparison by col.physical_type: INT32 / INT64 signed, or unsigned with
 * PQG_COL_UNSIGNED in col.flags; FLOAT / DOUBLE IEEE (NaN, as value or as literal,
 * fails everything but NE, which it passes; -0.0 == 0.0); BOOLEAN one byte, 0 < 1;
 * BYTE_ARRAY and FIXED_LEN_BYTE_ARRAY (type_length >= 1) unsigned lexicographic over
 * the bytes (a proper prefix sorts first, the empty string lowest); with PQG_COL_SIGNED_BE in
 * col.flags a FIXED_LEN_BYTE_ARRAY column orders as big-endian two's complement (a DECIMAL: the
 * same compare with bit 7 of byte 0 flipped on both sides), and the flag on any other physical
 * type is PQG_ERR_INVALID_ARG; INT96, and FLBA with
 * type_length < 1, are PQG_ERR_UNSUPPORTED, and so is col.max_rep > 0.  `literal` is
 * HOST memory in the column's physical little-endian layout (ignored by IS_NULL /
 * NOT_NULL): a length other than 4 / 8 / 1 / type_length for a fixed-width type is
 * PQG_ERR_INVALID_ARG.  Fixed-width values must be naturally aligned (4- and 8-byte
 * types; a chunk result's are); a dictionary's entries need no alignment.
 * Kept dictionaries: for a column decoded with PQG_COL_KEEP_DICT pass its
 * pqg_dictionary; `values` are then the int32 keys.  The comparison runs once per
 * dictionary entry (a nil_entry, or an entry the page does not hold, reads as zero
 * bytes) and a row passes when its key's entry does; a key outside [0, count) fails.
 * A non-null row whose rank is at or past num_values fails every operator but IS_NULL. */
typedef struct pqg_filter_args {
  const uint8_t* def_levels;   /* num_rows bytes, or NULL                               */
  const uint8_t* values;       /* dense values / chars, or int32 keys with `dictionary` */
  const int64_t* offsets;      /* BYTE_ARRAY without `dictionary`: num_values + 1       */
  int64_t num_rows;
  int64_t num_values;          /* dense values at `values`                              */
  int64_t values_bytes;        /* bytes at `values` (chars for byte arrays)             */
  pqg_column_desc col;         /* physical_type, type_length, max_def, max_rep, flags   */
  int32_t op;                  /* PQG_OP_*                                              */
  int32_t combine;             /* PQG_COMBINE_*                                         */
  const uint8_t* literal;      /* HOST                                                  */
  int64_t literal_len;
  const pqg_dictionary* dictionary; /* HOST struct of DEVICE pointers, or NULL          */
  uint8_t* bitmap;             /* in (AND / OR) and out                                 */
  int64_t num_selected;        /* out: popcount of the bitmap after combining           */
  int64_t num_valid;           /* out: non-null rows                                    */
} pqg_filter_args;
int pqg_filter(pqg_ctx* ctx, pqg_filter_args* args);

/* pqg_select: compact one column by a row bitmap (pqg_filter's layout; bits at and past
 * num_rows are ignored) into the chunk-result layout, so that pqg_assemble*, a download
 * or a dictionary lookup work on the filtered column unchanged: the selected rows' def
 * levels, the dense values of the selected non-null rows (any value_width >= 1), and for
 * byte arrays (value_width 0) int64 offsets rebased to 0 (values_out + 1 of them) plus
 * the selected chars back to back.  A column of int32 dictionary keys is a 4-byte
 * column; its dictionary is untouched.  Outputs are caller-allocated; each may be NULL
 * (not written), and with all three NULL the call only counts.  They never exceed the
 * inputs: num_rows bytes, values_bytes bytes and num_values + 1 offsets always suffice,
 * and a counting call gives the exact sizes.  Inputs and outputs must not overlap. */
typedef struct pqg_select_args {
  const uint8_t* bitmap;       /* 4 * ceil(num_rows / 32) bytes                          */
  const uint8_t* def_levels;   /* num_rows bytes, or NULL                                */
  const uint8_t* values;
  const int64_t* offsets;      /* byte arrays: num_values + 1                            */
  int64_t num_rows;
  int64_t num_values;
  int64_t values_bytes;
  int32_t max_def;
  int32_t value_width;         /* bytes per value; 0 = byte arrays                       */
  uint8_t* out_def_levels;     /* rows_out bytes                                         */
  uint8_t* out_values;         /* values_out x value_width, or bytes_out chars           */
  int64_t* out_offsets;        /* byte arrays: values_out + 1                            */
  int64_t rows_out;            /* out: selected rows                                     */
  int64_t values_out;          /* out: selected non-null rows                            */
  int64_t bytes_out;           /* out: value bytes (chars for byte arrays)               */
} pqg_select_args;
int pqg_select(pqg_ctx* ctx, pqg_select_args* args);

/* Row ranges into a row bitmap of pqg_filter's layout (LSB first, 4 * ceil(num_rows / 32) bytes at
 * `bitmap`, a 4-byte aligned DEVICE pointer): bit r is set exactly when one of the n ranges
 * [lo, hi) (`ranges`: n pairs of int64 on the HOST) holds r.  Whole dwords are written; the bits at
 * and past num_rows are zero.  The ranges must ascend and be disjoint, with
 * 0 <= lo <= hi <= num_rows (empty ranges are allowed), else PQG_ERR_INVALID_ARG with nothing
 * written.  With pqg_select it trims a decoded column to a set of row ranges.  Synchronous; its
 * device time is what pqg_last_filter_ms reports next. */
int pqg_range_bitmap(pqg_ctx* ctx, const int64_t* ranges, int n, int64_t num_rows, uint8_t* bitmap);

/* Device time (ms) of the kernels of the last pqg_filter / pqg_select call (an event
 * pair on the ctx stream; the literal upload and the count read-back excluded). */
int pqg_last_filter_ms(pqg_ctx* ctx, float* ms);

/* pqg_convert: decoded dense values of a logical type into the layout Arrow gives it.
 * DECIMAL_BE: big-endian two's complement of in_width bytes (FIXED_LEN_BYTE_ARRAY decimals), or
 * with `offsets` of each value's own length (BYTE_ARRAY decimals), to out_width (16 / 32)
 * little-endian bytes, sign-extended: out[i*ow + k] = in[i*w + w-1-k] for k < w, the sign byte
 * above.  DECIMAL_INT: 4 / 8 little-endian bytes sign-extended to out_width.  INT96_TIME:
 * (nanos of the day u64, julian day i32) to int64
 *   (int64)(day - 2440588) * units_per_day + (int64)(nanos / ns_per_unit)
 * with an unsigned, truncating divide and a multiply and add that wrap in 64 bits (a nil entry's
 * zero bytes convert like any value).  `values` may have any alignment (a dictionary read in
 * place); `out` is caller-allocated, 16-byte aligned, num_values * out_width bytes, and must not
 * overlap the input.  PQG_ERR_INVALID_ARG: an in_width / out_width / unit the kind does not take,
 * in_width > out_width, values_bytes < num_values * in_width, a misaligned `out`.  BYTE_ARRAY
 * decimals are counted first: a value of length 0 or above out_width (Arrow's FromBigEndian
 * rejects both), or whose offsets are negative, not ascending or past values_bytes, is a bad
 * value; with any, num_bad is set and the call is PQG_ERR_SIZE.  The call enqueues on the ctx
 * stream and waits; it does nothing for num_values == 0; a failing call writes no output. */
enum {
  PQG_CONV_DECIMAL_BE = 0,
  PQG_CONV_DECIMAL_INT = 1,
  PQG_CONV_INT96_TIME = 2
};
enum { PQG_UNIT_NONE = 0, PQG_UNIT_SECONDS, PQG_UNIT_MILLIS, PQG_UNIT_MICROS, PQG_UNIT_NANOS };
typedef struct pqg_convert_args {
  const uint8_t* values;   /* DEVICE: dense values or chars; any alignment                      */
  const int64_t* offsets;  /* DEVICE: BYTE_ARRAY decimals (num_values + 1), else NULL            */
  int64_t num_values, values_bytes;
  int32_t kind, in_width;  /* in_width: DECIMAL_BE 1..32 (0 with offsets), DECIMAL_INT 4 / 8, INT96 12 */
  int32_t out_width;       /* decimals: 16 or 32; INT96_TIME: 8                                  */
  int32_t unit;            /* INT96_TIME: PQG_UNIT_SECONDS .. PQG_UNIT_NANOS                     */
  uint8_t* out;            /* DEVICE, 16-byte aligned, num_values * out_width bytes              */
  int64_t num_bad;         /* out: bad BYTE_ARRAY decimals                                       */
} pqg_convert_args;
int pqg_convert(pqg_ctx* ctx, pqg_convert_args* args);
/* Device time (ms) of the kernels of the last pqg_convert call (the count pass included). */
int pqg_last_convert_ms(pqg_ctx* ctx, float* ms);

/* ---- host-side planner: footer / schema (file_meta.go:14-62, schema.go) --- */
typedef struct pqg_file pqg_file;

typedef struct pqg_column_info {
  pqg_column_desc desc;
  char path[256];        /* dotted flat name (schema.go flatName) */
} pqg_column_info;

typedef struct pqg_chunk_meta {
  int64_t start;                 /* DictionaryPageOffset if set else DataPageOffset */
  int64_t total_compressed_size;
  int64_t total_uncompressed_size;
  int64_t data_page_offset;      /* absolute */
  int64_t num_values;
  int32_t has_dict_page_offset;
  int32_t codec;
  int32_t type;                  /* ColumnMetaData.type */
  int32_t reserved;
} pqg_chunk_meta;

/* Parse a whole parquet file held in host memory: PAR1 magic at both ends,
 * footer length, thrift FileMetaData, schema → leaf columns with maxD/maxR. */
int pqg_file_open(const uint8_t* file, int64_t len, pqg_file** out);
/* The same from the file's first head_len bytes and its LAST tail_len bytes
 * (file_len in all): a range reader's footer fetch.  PQG_ERR_INVALID_ARG when
 * the tail is shorter than the footer + 8 bytes (read the i32 footer length
 * in the last 8 bytes, then fetch footer + 8). */
int pqg_file_open_tail(const uint8_t* head, int64_t head_len, const uint8_t* tail, int64_t tail_len, int64_t file_len,
                       pqg_file** out);
void pqg_file_close(pqg_file* f);
int pqg_file_num_columns(const pqg_file* f);
int pqg_file_num_row_groups(const pqg_file* f);
int64_t pqg_file_num_rows(const pqg_file* f);
/* PQG_ERR_METADATA when the column's dotted path does not fit pqg_column_info.path */
int pqg_file_column(const pqg_file* f, int col, pqg_column_info* out);
int pqg_file_chunk(const pqg_file* f, int row_group, int col, pqg_chunk_meta* out);
int64_t pqg_file_row_group_rows(const pqg_file* f, int row_group);

/* ColumnMetaData.statistics (field 12) of a chunk: null_count (3), max_value (5) and
 * min_value (6) only.  The deprecated max / min (1, 2) are skipped: their sort order is
 * undefined for unsigned types and byte arrays.  Values are the column's physical
 * little-endian bytes, as the file stores them; the pointers stay valid until
 * pqg_file_close.  A file in which any statistics struct does not parse reports no
 * statistics for any chunk (and opens as it did before). */
typedef struct pqg_chunk_stats {
  const uint8_t *min_value, *max_value;  /* owned by the pqg_file; NULL = absent */
  int32_t min_len, max_len;
  int64_t null_count;                    /* -1 = absent */
} pqg_chunk_stats;
int pqg_file_chunk_stats(const pqg_file* f, int row_group, int col, pqg_chunk_stats* out);

/* The logical type of a leaf: SchemaElement.logicalType (field 10) when the element has one
 * that parses, else what converted_type (6) with scale (7) / precision (8) says (UTF8 STRING,
 * DECIMAL, DATE, TIME_MILLIS / TIME_MICROS TIME, TIMESTAMP_MILLIS / TIMESTAMP_MICROS TIMESTAMP
 * (utc = 1, as the format defines them), UINT_* / INT_* INTEGER, ENUM, JSON, BSON).  Nothing
 * is validated: a precision of 0 is reported as 0.  Fields that do not apply are 0. */
enum { PQG_LT_NONE = 0, PQG_LT_STRING, PQG_LT_ENUM, PQG_LT_DECIMAL, PQG_LT_DATE, PQG_LT_TIME,
       PQG_LT_TIMESTAMP, PQG_LT_INTEGER, PQG_LT_JSON, PQG_LT_BSON, PQG_LT_UUID, PQG_LT_FLOAT16, PQG_LT_OTHER };
typedef struct pqg_logical_type {
  int32_t kind, precision, scale, unit, utc, bit_width, is_signed;
  int32_t converted_type;   /* SchemaElement.converted_type as stored, -1 when absent */
} pqg_logical_type;
int pqg_file_column_logical(const pqg_file* f, int col, pqg_logical_type* out);

/* The schema tree below the root, depth first (makeSchema / readGroupSchema
 * schema.go:789-894, 996-1025): what NextRow's row assembly walks
 * (Column.getData schema.go:171-264).  Replaces the Column tree the reference
 * builds for FileReader. */
typedef struct pqg_schema_node {
  char name[128];
  int32_t repetition;    /* 0 REQUIRED, 1 OPTIONAL, 2 REPEATED */
  int32_t num_children;  /* 0 for a leaf */
  int32_t leaf;          /* column index of a leaf (pqg_file_column), -1 for a group */
  int32_t max_def, max_rep;
  int32_t reserved;
} pqg_schema_node;
int pqg_file_num_schema_nodes(const pqg_file* f);
/* PQG_ERR_METADATA when the node's name does not fit pqg_schema_node.name (a
 * truncated name would be a different map key than the reference's) */
int pqg_file_schema_node(const pqg_file* f, int i, pqg_schema_node* out);
/* The annotation of schema node i (the index of pqg_file_schema_node): PQG_NODE_LIST for
 * LogicalType LIST or converted type LIST (3), PQG_NODE_MAP for LogicalType MAP or converted
 * type MAP (1) / MAP_KEY_VALUE (2), PQG_NODE_PLAIN for everything else, leaves included.  A
 * LogicalType LIST or MAP wins over the converted type.  A negative status on a bad index. */
enum { PQG_NODE_PLAIN = 0, PQG_NODE_LIST = 1, PQG_NODE_MAP = 2 };
int pqg_file_schema_node_kind(const pqg_file* f, int i);

/* ======================= oracle (TEST INFRASTRUCTURE) ===================== */
/* Implemented only by oracle/liboracle.so.  Host pointers everywhere. */
int pqo_decode_chunk(const pqg_chunk_job* job, pqg_chunk_result* res,
                     pqg_page_info* pages, int page_cap, int* n_pages);
void pqo_free_result(pqg_chunk_result* res);
/* The oracle's PageHeader.Read over buf[0, len): the status (PQG_OK or PQG_ERR_THRIFT), the bytes
 * the reader consumed (also on an error: where it stopped) and every field it keeps, each
 * page-header struct's on its own (a header may carry several). */
typedef struct pqo_page_header {
  int32_t type, uncompressed_size, compressed_size;
  int32_t has_dph, has_dict, has_v2;
  int32_t dph_num_values, dph_encoding, dph_def_encoding, dph_rep_encoding;
  int32_t dict_num_values, dict_encoding;
  int32_t v2_num_values, v2_num_nulls, v2_num_rows, v2_encoding, v2_def_len, v2_rep_len;
  int32_t v2_is_compressed;
} pqo_page_header;
int pqo_read_page_header(const uint8_t* buf, int64_t len, int64_t* consumed, pqo_page_header* out);
int pqo_unpack8_32(const uint8_t* data, int width, int32_t* out8);
int pqo_unpack8_64(const uint8_t* data, int width, int64_t* out8);
/* hybrid RLE/bit-pack: decode `count` values of `width` bits (levelDecoder.next) */
int pqo_hybrid_decode(const uint8_t* buf, int64_t len, int width, int64_t count, int32_t* out);
int pqo_snappy_decode(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap, int64_t* out_len);
int pqo_delta_decode64(const uint8_t* buf, int64_t len, int64_t count, int64_t* out);
int pqo_delta_decode32(const uint8_t* buf, int64_t len, int64_t count, int32_t* out);
/* Reference column-store contents (triage of Q1/Q2): decode the chunks of one
 * column over `n_row_groups` consecutive row groups the way readRowGroup fills
 * ColumnStore.values (readPageData chunk_reader.go:380-402), with the quirks in
 * `quirks` reproduced (Q2 requires Q1, as in the reference).  Per row group:
 * `entries` store slots, `nil_flags` one byte per entry; fixed width:
 * `values` entries x value_width bytes (a nil slot is zeros); byte arrays
 * (value_width 0): `values` the entries' bytes back to back (`chars` of them)
 * and `offsets[entries + 1]` (a nil entry is empty).  Q2 follows Go 1.13's
 * slice growth (runtime growslice + malloc size classes) for []interface{}:
 * outside /root/reference, stated in the oracle, so parity for it is unpinned. */
typedef struct pqo_store_rg {
  int32_t status;
  int32_t value_width;
  int64_t entries;
  uint8_t* values;
  uint8_t* nil_flags;
  int64_t* offsets;
  int64_t chars;
} pqo_store_rg;
int pqo_decode_column_store(const pqg_chunk_job* jobs, int n_row_groups, int quirks, pqo_store_rg* out);
void pqo_free_store(pqo_store_rg* out, int n_row_groups);
/* CPU-baseline helper: decode data pages [page_lo, page_hi) of a chunk (its
 * dictionary page always), for a thread pool over pages; *out_bytes = output
 * bytes of those pages.  Returns the number of data pages, or a status < 0. */
int64_t pqo_decode_page_range(const pqg_chunk_job* job, int page_lo, int page_hi, int64_t* out_bytes);
/* K8 restatements (host pointers): the ColumnStore.get / getData cursor walks */
int pqo_assemble(pqg_assemble_args* args);
int pqo_assemble_list(pqg_list_args* args);
/* packedArray layout of levels (host pointers): see pqg_pack_levels */
int pqo_pack_levels(const uint8_t* levels, int64_t n, int max_level, uint8_t* packed);
/* test hook of the Q2 emulation: Go 1.13 malloc size-class rounding */
int64_t pqo_go_roundupsize(int64_t size);

#ifdef __cplusplus
}
#endif
#endif /* PQGPU_H */
