// pqg_ops.hip — the single-shot entry points of include/pqgpu.h: one compressed block, one page, the
// assemble / filter / select passes over decoded columns, level packing, one CRC.  Each call uploads or
// takes device data, launches its kernels on the context's stream and waits; none of it is part of
// the batch pipeline (pqg_runtime.hip), whose context (pqg_ctx.h) they share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "pqg_ctx.h"
#include "pqg_convert.h"
#include "pqg_crc.h"
#include "pqg_filter.h"
#include "pqg_kernels.h"
#include "pqg_lz4.h"
#include "pqg_zstd.h"

using namespace pqg;

namespace {

// The count pass of an entry: `launch` between the events ev[0] and ev[1], its n totals copied from `tot` to
// the host's h, the wait for them, and the pass's device time in *ms.
template <class Launch>
int count_pass(pqg_ctx* c, hipEvent_t* ev, Launch launch, const int64_t* tot, int64_t* h, int n, float* ms) {
  hipEventRecord(ev[0], c->stream);
  const int e = launch();
  if (e) return e;
  hipEventRecord(ev[1], c->stream);
  if (copy_sync(c, h, tot, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost)) return PQG_ERR_HIP;
  hipEventElapsedTime(ms, ev[0], ev[1]);
  return PQG_OK;
}

// The write pass of the list exports, after the host checked the count pass's totals: `launch` between
// ev_k8[2] and ev_k8[3], the wait, and both passes' device time.
template <class Launch>
int write_pass(pqg_ctx* c, float count_ms, Launch launch) {
  hipEventRecord(c->ev_k8[2], c->stream);
  int e = launch();
  if (e) return e;
  hipEventRecord(c->ev_k8[3], c->stream);
  e = hip_ok(hipStreamSynchronize(c->stream));
  float ms = 0.f;
  hipEventElapsedTime(&ms, c->ev_k8[2], c->ev_k8[3]);
  c->k8_ms = count_ms + ms;
  return e;
}

// ---- one bare block as the only page of a one-job batch (pqg_block_decompress) --------------------
// What differs between the codecs' blocks.
struct BlockKind {
  int codec;
  int32_t flags;   // PageDev.flags: kPageBareBlock for the decoders that count the decoded bytes into gz_len
  int64_t gz_len;  // PageDev.gz_len before the decode
  int queues;      // zeroed queue regions
};
// The block on the device, in blk_meta: the job, its page, then ints [0] the page list, [1] its total,
// [2..3] spare (the snappy split counters), [4..] the queue regions; the decoded bytes go to blk_dst.
struct BlockDev {
  JobDev* job;
  PageDev* page;
  int* ints;
  int* queue;
  uint8_t* dst;
};

// Grows blk_src / blk_dst / blk_meta, uploads src[0..n) (src == nullptr: blk_src holds the block already),
// sets up the job, a page with room for `store` decoded bytes in blk_dst, its list and queues, has
// `launch` start the decoder on them, and returns the page record as the kernels left it.
template <class Launch>
int block_decode(pqg_ctx* c, const BlockKind& k, const uint8_t* src, int64_t n, int64_t store, PageDev* out,
                 Launch launch) {
  hipSetDevice(c->device);
  if (c->blk_src.grow((size_t)n + 64) || c->blk_dst.grow((size_t)store + 64) ||
      c->blk_meta.grow(sizeof(JobDev) + sizeof(PageDev) + (4 + 2 * kQueueInts) * sizeof(int)))
    return PQG_ERR_HIP;
  JobDev jd;
  memset(&jd, 0, sizeof(jd));
  jd.data = (const uint8_t*)c->blk_src.p;
  jd.data_len = n;
  jd.tcs = n;
  jd.codec = k.codec;
  jd.scratch_cap = store + 16;
  PageDev pd;
  memset(&pd, 0, sizeof(pd));
  pd.page_type = PQG_PAGE_DICTIONARY;  // no values-decoder check after the block
  pd.flags = k.flags;
  pd.csize = (int32_t)n;
  pd.usize = (int32_t)store;
  pd.gz_len = k.gz_len;
  pd.read_status = kOK;
  uint8_t* meta = (uint8_t*)c->blk_meta.p;
  const BlockDev b{(JobDev*)meta, (PageDev*)(meta + sizeof(JobDev)), (int*)(meta + sizeof(JobDev) + sizeof(PageDev)),
                   (int*)(meta + sizeof(JobDev) + sizeof(PageDev)) + 4, (uint8_t*)c->blk_dst.p};
  const int hi[2] = {0, 1};
  if ((src && n && hipMemcpyAsync(c->blk_src.p, src, (size_t)n, hipMemcpyHostToDevice, c->stream) != hipSuccess) ||
      hipMemcpyAsync(b.job, &jd, sizeof(jd), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(b.page, &pd, sizeof(pd), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(b.ints, hi, sizeof(hi), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemsetAsync(b.queue, 0, sizeof(int) * (size_t)k.queues * kQueueInts, c->stream) != hipSuccess)
    return PQG_ERR_HIP;
  launch(b);
  if (hipGetLastError() != hipSuccess) return PQG_ERR_HIP;
  return copy_sync(c, out, b.page, sizeof(PageDev), hipMemcpyDeviceToHost);
}

// the decoded bytes of such a block, from blk_dst to the caller
int block_copy_back(pqg_ctx* c, uint8_t* dst, int64_t len) {
  return len ? copy_sync(c, dst, c->blk_dst.p, (size_t)len, hipMemcpyDeviceToHost) : PQG_OK;
}

// gzipCompressor.DecompressBlock (compress.go:63-76): gzip.NewReader +
// ioutil.ReadAll.  The decoded length is not in the block, so k_inflate decodes
// it as a bare block (kPageBareBlock): bytes past the device buffer's `store`
// are counted and CRC'd but not stored, and the count comes back in
// PageDev.gz_len.  The first pass stores at most kInflateFirst bytes; a block
// that decodes to more (and fits `cap`) is decoded again into a buffer of its
// size, so the device buffer never grows to `cap` before the length is known,
// and no byte past what k_inflate stored is ever copied out.
int block_inflate(pqg_ctx* c, const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap, int64_t* out_len) {
  constexpr int64_t kInflateFirst = 64 << 20;
  const BlockKind kind{PQG_CODEC_GZIP, kPageBareBlock, 0, 1};
  auto launch = [&](const BlockDev& b) {
    hipLaunchKernelGGL(k_inflate, dim3(qgrid(1)), dim3(64), 0, c->stream, b.job, b.page, b.ints, b.ints + 1, b.queue,
                       b.dst, 0);
  };
  int64_t store = std::min<int64_t>(std::max<int64_t>(cap, 0), kInflateFirst);
  PageDev pd;
  int e = block_decode(c, kind, src, n, store, &pd, launch);
  if (e) return e;
  if (pd.read_status != kOK) return pd.read_status;
  *out_len = pd.gz_len;
  if (pd.gz_len > cap) return PQG_ERR_CAPACITY;
  if (pd.gz_len > INT32_MAX) return PQG_ERR_UNSUPPORTED;  // one block of >= 2 GiB: the kernel's 32-bit offsets
  if (pd.gz_len > store) {  // decoded length known now: again, storing all of it (the block is in blk_src)
    store = pd.gz_len;
    e = block_decode(c, kind, nullptr, n, store, &pd, launch);
    if (e) return e;
    if (pd.read_status != kOK) return pd.read_status;
    if (pd.gz_len != store) return PQG_ERR_HIP;  // the same bytes decode to the same length
  }
  return block_copy_back(c, dst, pd.gz_len);
}

// zstd's ZSTD_decompress over one host block.  The output buffer is sized
// before the decode from the block itself (zstd::decoded_bound: the frames'
// content sizes, or per block its size / the 128 KiB block maximum), so one
// pass decodes it whatever `cap` is; k_zstd never stores past that buffer.
int block_zstd(pqg_ctx* c, const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap, int64_t* out_len) {
  bool exact = false;
  const int64_t store = zstd::decoded_bound(src, n, &exact);
  if (store > INT32_MAX) return PQG_ERR_UNSUPPORTED;  // one block of >= 2 GiB
  hipSetDevice(c->device);
  if (c->zstd_ws.grow((size_t)zstd_grid(c) * zstd::kWsBytes)) return PQG_ERR_HIP;
  PageDev pd;
  const int e = block_decode(c, BlockKind{PQG_CODEC_ZSTD, kPageBareBlock, -1, 1}, src, n, store, &pd, [&](const BlockDev& b) {
    hipLaunchKernelGGL(k_zstd, dim3(qgrid(1)), dim3(64), 0, c->stream, b.job, b.page, b.ints, b.ints + 1, b.queue, b.dst,
                       (uint8_t*)c->zstd_ws.p);
  });
  if (e) return e;
  if (pd.read_status != kOK) return pd.read_status;
  *out_len = pd.gz_len;
  if (pd.gz_len > cap) return PQG_ERR_CAPACITY;
  return block_copy_back(c, dst, pd.gz_len);
}

// LZ4_decompress_safe over one host block, into a buffer no block can fill.
// The host walks the sequences first (lz4::decoded_length: the exact decoded
// length, or the verdict on a malformed block), so the device buffer is sized
// once, a too small `cap` is answered without a launch, and the kernel never
// stores past the walked length.
int block_lz4(pqg_ctx* c, const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap, int64_t* out_len) {
  const int64_t len = lz4::decoded_length(src, n);
  if (len < 0) return PQG_ERR_LZ4;
  *out_len = len;
  if (len > cap) return PQG_ERR_CAPACITY;
  if (len > INT32_MAX) return PQG_ERR_UNSUPPORTED;  // one block of >= 2 GiB
  PageDev pd;
  const int e = block_decode(c, BlockKind{PQG_CODEC_LZ4_RAW, kPageBareBlock, -1, 1}, src, n, len, &pd, [&](const BlockDev& b) {
    hipLaunchKernelGGL(c->lz4_batch ? k_lz4_batch : k_lz4, dim3(qgrid(1)), dim3(64), 0, c->stream, b.job, b.page, b.ints,
                       b.ints + 1, b.queue, b.dst);
  });
  if (e) return e;
  if (pd.read_status != kOK) return pd.read_status;
  if (pd.gz_len != len) return PQG_ERR_LZ4;  // the kernel and the host walk are one decoder: never
  return block_copy_back(c, dst, len);
}

// snappy.Decode over one host block: the page decode's own snappy stage (launch_snappy), on a one-page list.
int block_snappy(pqg_ctx* c, const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap, int64_t* out_len) {
  // decodedLen (decode.go:32-43): the varint header, on the host to size the output
  uint64_t v = 0;
  int hl = 0;
  for (unsigned sft = 0;; hl++, sft += 7) {
    if (hl >= n) return PQG_ERR_SNAPPY;
    const uint8_t b = src[hl];
    if (b < 0x80) {
      if (hl > 9 || (hl == 9 && b > 1)) return PQG_ERR_SNAPPY;
      v |= sft < 64 ? (uint64_t)b << sft : 0;
      hl++;
      break;
    }
    if (sft < 64) v |= (uint64_t)(b & 0x7f) << sft;
  }
  if (v > 0xffffffffull || v > (uint64_t)INT32_MAX) return PQG_ERR_SNAPPY;
  *out_len = (int64_t)v;
  if ((int64_t)v > cap) return PQG_ERR_CAPACITY;
  hipSetDevice(c->device);
  const int64_t bsub = (int64_t)v / kSnapSub + 2, bseg = n / kSnapSeg + 2;
  if (c->blk_subs.grow(sizeof(SnapSub) * (size_t)bsub) || c->blk_segpage.grow(sizeof(int) * (size_t)bseg) ||
      c->blk_F.grow(sizeof(uint2) * 64 * (size_t)bseg))
    return PQG_ERR_HIP;
  const SnapTables T{(SnapSub*)c->blk_subs.p, (int)bsub, (int*)c->blk_segpage.p, (int)bseg, (uint2*)c->blk_F.p};
  PageDev pd;
  // no page flag: k_snappy decodes the page's usize bytes into scratch as for any page; two queues, and
  // the split counters in the spare ints
  const int e = block_decode(c, BlockKind{PQG_CODEC_SNAPPY, 0, 0, 2}, src, n, (int64_t)v, &pd, [&](const BlockDev& b) {
    launch_snappy(c, c->stream, b.job, b.page, b.ints, b.ints + 1, 1, b.ints + 2, b.queue, b.queue + kQueueInts, b.dst, T);
  });
  if (e) return e;
  if (pd.read_status != kOK) return pd.read_status;
  return block_copy_back(c, dst, (int64_t)v);
}

}  // namespace

extern "C" {

int pqg_assemble(pqg_ctx* c, pqg_assemble_args* a) {
  if (!c || !a || a->num_slots < 0 || a->max_def < 0 || a->max_def > 255 || a->boundary_level < 0)
    return PQG_ERR_INVALID_ARG;
  if (a->values_spaced && (a->value_width <= 0 || (!a->values && a->num_slots > 0))) return PQG_ERR_INVALID_ARG;
  hipSetDevice(c->device);
  const int64_t nseg = (a->num_slots + 4095) / 4096;
  if (c->asm_seg.grow((size_t)(2 * nseg + 2) * sizeof(int64_t))) return PQG_ERR_HIP;
  int64_t* seg = (int64_t*)c->asm_seg.p;
  int64_t* tot = seg + 2 * nseg;
  int64_t h[2] = {0, 0};
  const int e = count_pass(c, c->ev_k8, [&] { return assemble_launch(c->stream, a, seg, tot); }, tot, h, 2, &c->k8_ms);
  if (e) return e;
  a->num_valid = h[0];
  a->null_count = a->num_slots - h[0];
  a->num_boundaries = h[1];
  return PQG_OK;
}

int pqg_assemble_list(pqg_ctx* c, pqg_list_args* a) {
  if (!c || !a || a->num_slots < 0 || !a->def_levels || a->max_def < 0 || a->max_def > 255 || a->value_width < 0)
    return PQG_ERR_INVALID_ARG;
  if (a->elem_values && (a->value_width <= 0 || (!a->values && a->num_slots > 0))) return PQG_ERR_INVALID_ARG;
  hipSetDevice(c->device);
  const int64_t nseg = (a->num_slots + 4095) / 4096;
  if (c->asm_seg.grow((size_t)(4 * nseg + 4) * sizeof(int64_t))) return PQG_ERR_HIP;
  int64_t* seg = (int64_t*)c->asm_seg.p;
  int64_t* tot = seg + 4 * nseg;
  int64_t h[4] = {0, 0, 0, 0};
  float count_ms = 0.f;
  const int e = count_pass(c, c->ev_k8, [&] { return list_count_launch(c->stream, a, seg, tot); }, tot, h, 4, &count_ms);
  if (e) return e;
  a->num_rows = h[0];
  a->num_elements = h[1];
  a->num_valid = h[2];
  a->null_lists = h[3];
  // int32 offsets cannot hold the elements: fail before any output is written
  if (h[1] > INT32_MAX) return PQG_ERR_INVALID_ARG;
  return write_pass(c, count_ms, [&] { return list_write_launch(c->stream, a, seg); });
}

// Nested export: replaces the getData / getNextData recursion (schema.go:171-264)
// over ColumnStore.get (data_store.go:158-203) for a leaf under `depth` lists.
int pqg_assemble_nested(pqg_ctx* c, pqg_nested_args* a) {
  if (!c || !a) return PQG_ERR_INVALID_ARG;
  if (a->depth < 0 || a->depth > PQG_MAX_LIST_DEPTH) return PQG_ERR_UNSUPPORTED;
  if (a->num_slots < 0 || a->max_def < 0 || a->max_def > 255 || a->value_width < 0) return PQG_ERR_INVALID_ARG;
  if (!a->def_levels && a->max_def > 0) return PQG_ERR_INVALID_ARG;
  const int K = a->depth;
  int prev = 0;  // elem_def[k-1] <= list_def[k] <= elem_def[k] <= max_def, elem_def strictly increasing
  for (int k = 0; k < K; k++) {
    const pqg_nested_level& l = a->level[k];
    if (l.list_def < prev || l.elem_def < l.list_def || l.elem_def <= prev || l.elem_def > a->max_def)
      return PQG_ERR_INVALID_ARG;
    prev = l.elem_def;
  }
  if (a->leaf_values && (a->value_width <= 0 || !a->values)) return PQG_ERR_INVALID_ARG;
  if (a->leaf_offsets && !a->value_offsets) return PQG_ERR_INVALID_ARG;
  hipSetDevice(c->device);
  const int C = 2 * K + 2;
  const int64_t nseg = (a->num_slots + 4095) / 4096;
  if (c->asm_seg.grow((size_t)(C * nseg + C) * sizeof(int64_t))) return PQG_ERR_HIP;
  int64_t* seg = (int64_t*)c->asm_seg.p;
  int64_t* tot = seg + C * nseg;
  int64_t h[2 * PQG_MAX_LIST_DEPTH + 2] = {0};
  float count_ms = 0.f;
  const int e = count_pass(c, c->ev_k8, [&] { return nested_count_launch(c->stream, a, seg, tot); }, tot, h, C, &count_ms);
  if (e) return e;
  // int32 offsets cannot hold some depth's elements: fail before any output is written
  for (int k = 1; k <= K; k++)
    if (h[k] > INT32_MAX) return PQG_ERR_INVALID_ARG;
  a->num_rows = h[0];
  a->num_leaf = h[K];
  a->num_valid = h[K + 1];
  for (int k = 0; k < K; k++) {
    a->level[k].num_entries = h[k];
    a->level[k].null_count = h[K + 2 + k];
  }
  return write_pass(c, count_ms, [&] { return nested_write_launch(c->stream, a, seg, tot); });
}

// Struct export: the validity of the groups Column.getData (schema.go:235-264) returns as nil or as
// a map, for up to PQG_MAX_STRUCTS structs above one leaf.
int pqg_assemble_structs(pqg_ctx* c, pqg_struct_args* a) {
  if (!c || !a) return PQG_ERR_INVALID_ARG;
  if (a->depth < 0 || a->depth > PQG_MAX_LIST_DEPTH) return PQG_ERR_UNSUPPORTED;
  if (a->num_slots < 0 || a->max_def < 0 || a->max_def > 255) return PQG_ERR_INVALID_ARG;
  if (a->num_structs < 0 || a->num_structs > PQG_MAX_STRUCTS) return PQG_ERR_INVALID_ARG;
  const int K = a->depth, ns = a->num_structs;
  int ed[PQG_MAX_LIST_DEPTH + 1] = {0};  // ed[k]: elem_def of depth k, ed[0] = 0
  for (int k = 1; k <= K; k++) {
    ed[k] = a->elem_def[k - 1];
    if (ed[k] <= ed[k - 1] || ed[k] > a->max_def) return PQG_ERR_INVALID_ARG;
  }
  for (int j = 0; j < ns; j++) {
    const pqg_struct_level& s = a->st[j];
    if (s.depth < 0 || s.depth > K) return PQG_ERR_INVALID_ARG;
    if (s.struct_def <= ed[s.depth] || s.struct_def > a->max_def) return PQG_ERR_INVALID_ARG;
    if (s.depth < K && s.struct_def >= ed[s.depth + 1]) return PQG_ERR_INVALID_ARG;
  }
  if (!a->def_levels && ns > 0 && a->num_slots > 0) return PQG_ERR_INVALID_ARG;
  if (!a->rep_levels && K > 0) return PQG_ERR_INVALID_ARG;
  if (a->num_slots == 0 || ns == 0) {  // nothing to read or nothing asked for
    for (int j = 0; j < ns; j++) a->st[j].num_entries = a->st[j].null_count = 0;
    c->k8_ms = 0.f;
    return PQG_OK;
  }
  hipSetDevice(c->device);
  constexpr int C = PQG_MAX_LIST_DEPTH + 1 + PQG_MAX_STRUCTS;
  const int64_t nseg = (a->num_slots + 4095) / 4096;
  if (c->asm_seg.grow((size_t)(C * nseg + C) * sizeof(int64_t))) return PQG_ERR_HIP;
  int64_t* seg = (int64_t*)c->asm_seg.p;
  int64_t* tot = seg + C * nseg;
  int64_t h[C] = {0};
  float count_ms = 0.f;
  const int e = count_pass(c, c->ev_k8, [&] { return struct_count_launch(c->stream, a, seg, tot); }, tot, h, C, &count_ms);
  if (e) return e;
  bool any = false;
  for (int j = 0; j < ns; j++) any = any || a->st[j].validity;
  if (any) {
    const int w = write_pass(c, count_ms, [&] { return struct_write_launch(c->stream, a, seg); });
    if (w) return w;
  } else {
    c->k8_ms = count_ms;
  }
  for (int j = 0; j < ns; j++) {
    a->st[j].num_entries = h[a->st[j].depth];
    a->st[j].null_count = h[PQG_MAX_LIST_DEPTH + 1 + j];
  }
  return PQG_OK;
}

int pqg_last_assemble_ms(pqg_ctx* c, float* ms) {
  if (!c || !ms) return PQG_ERR_INVALID_ARG;
  *ms = c->k8_ms;
  return PQG_OK;
}

// K9s: `column op literal` per row into a row bitmap (pqg_filter.hip).
int pqg_filter(pqg_ctx* c, pqg_filter_args* a) {
  if (!c || !a) return PQG_ERR_INVALID_ARG;
  if (a->num_rows < 0 || a->num_values < 0 || a->values_bytes < 0 || a->col.max_def < 0 || a->col.max_def > 255 ||
      a->op < PQG_OP_EQ || a->op > PQG_OP_NOT_NULL || a->combine < PQG_COMBINE_SET || a->combine > PQG_COMBINE_OR)
    return PQG_ERR_INVALID_ARG;
  if (a->col.max_rep > 0) return PQG_ERR_UNSUPPORTED;
  const int type = a->col.physical_type;
  const bool uns = (a->col.flags & PQG_COL_UNSIGNED) != 0;
  const bool sbe = (a->col.flags & PQG_COL_SIGNED_BE) != 0;  // FLBA only: big-endian two's complement order
  if (sbe && type != PQG_FIXED_LEN_BYTE_ARRAY) return PQG_ERR_INVALID_ARG;
  flt::Pred p;
  memset(&p, 0, sizeof(p));
  p.op = a->op;
  switch (type) {
    case PQG_BOOLEAN: p.kind = flt::K_U8; p.width = 1; break;
    case PQG_INT32: p.kind = uns ? flt::K_U32 : flt::K_I32; p.width = 4; break;
    case PQG_INT64: p.kind = uns ? flt::K_U64 : flt::K_I64; p.width = 8; break;
    case PQG_FLOAT: p.kind = flt::K_F32; p.width = 4; break;
    case PQG_DOUBLE: p.kind = flt::K_F64; p.width = 8; break;
    case PQG_BYTE_ARRAY: p.kind = flt::K_BYTES; p.width = 0; break;
    case PQG_FIXED_LEN_BYTE_ARRAY:
      if (a->col.type_length < 1) return PQG_ERR_UNSUPPORTED;
      p.kind = sbe ? flt::K_FLBA_SBE : flt::K_FLBA;
      p.width = a->col.type_length;
      break;
    default: return PQG_ERR_UNSUPPORTED;  // INT96
  }
  const bool cmp = a->op != PQG_OP_IS_NULL && a->op != PQG_OP_NOT_NULL;
  const bool bytes = p.kind == flt::K_BYTES || p.kind == flt::K_FLBA || p.kind == flt::K_FLBA_SBE;
  if (cmp) {
    if (a->literal_len < 0 || (a->literal_len > 0 && !a->literal)) return PQG_ERR_INVALID_ARG;
    if (p.kind != flt::K_BYTES && a->literal_len != p.width) return PQG_ERR_INVALID_ARG;
    if (!bytes) memcpy(&p.lit, a->literal, (size_t)p.width);  // little endian
    p.lit_len = a->literal_len;
  }
  const pqg_dictionary* d = a->dictionary;
  const int64_t n = a->num_rows;
  if (n > 0) {
    if (!a->bitmap) return PQG_ERR_INVALID_ARG;
    if (a->num_values > 0 && !a->values) return PQG_ERR_INVALID_ARG;
    if (d) {
      if (d->count < 0 || d->value_width != p.width || a->values_bytes < 4 * a->num_values ||
          ((uintptr_t)a->values & 3) || (d->count > 0 && (!d->values && d->values_bytes > 0)) ||
          (p.kind == flt::K_BYTES && d->count > 0 && !d->offsets))
        return PQG_ERR_INVALID_ARG;
    } else {
      if (p.kind == flt::K_BYTES ? (a->num_values > 0 && !a->offsets) : a->values_bytes < (int64_t)p.width * a->num_values)
        return PQG_ERR_INVALID_ARG;
      if ((p.width == 4 || p.width == 8) && !bytes && ((uintptr_t)a->values & (uintptr_t)(p.width - 1)))
        return PQG_ERR_INVALID_ARG;
    }
  }
  a->num_selected = 0;
  a->num_valid = 0;
  c->flt_ms = 0.f;
  if (n == 0) return PQG_OK;
  hipSetDevice(c->device);
  const int64_t nseg = (n + flt::kSeg - 1) / flt::kSeg;
  const size_t o_tot = sizeof(int64_t) * (size_t)nseg, o_lit = o_tot + 2 * sizeof(int64_t);
  const size_t o_eb = o_lit + (((size_t)p.lit_len + 7) & ~(size_t)7);
  const size_t eb_bytes = d ? (size_t)((d->count + 31) / 32) * 4 : 0;
  if (c->flt_buf.grow(o_eb + eb_bytes + 8)) return PQG_ERR_HIP;
  uint8_t* base = (uint8_t*)c->flt_buf.p;
  int64_t* seg = (int64_t*)base;
  int64_t* tot = (int64_t*)(base + o_tot);
  if (cmp && bytes && p.lit_len > 0 &&
      hipMemcpyAsync(base + o_lit, a->literal, (size_t)p.lit_len, hipMemcpyHostToDevice, c->stream) != hipSuccess)
    return PQG_ERR_HIP;
  p.lit_bytes = (uintptr_t)(base + o_lit);
  flt::Col col;
  memset(&col, 0, sizeof(col));
  col.def = a->col.max_def > 0 ? (uintptr_t)a->def_levels : 0;
  col.values = (uintptr_t)a->values;
  col.offsets = (uintptr_t)a->offsets;
  col.num_values = a->num_values;
  col.values_bytes = a->values_bytes;
  col.max_def = a->col.max_def;
  col.dict = d != nullptr;
  col.ebits = (uintptr_t)(base + o_eb);
  col.dict_count = d ? d->count : 0;
  int64_t h[2] = {0, 0};
  const int e = count_pass(
      c, c->ev_flt,
      [&] {
        return filter_launch(c->stream, p, col, d, (uint32_t*)(base + o_eb), a->bitmap, n, a->combine, c->flt_lds, seg, tot);
      },
      tot, h, 2, &c->flt_ms);
  if (e) return e;
  a->num_valid = col.def ? h[0] : n;
  a->num_selected = h[1];
  return PQG_OK;
}

// K9s: compact one column by a row bitmap into the chunk-result layout (pqg_filter.hip).
int pqg_select(pqg_ctx* c, pqg_select_args* a) {
  if (!c || !a || a->num_rows < 0 || a->num_values < 0 || a->values_bytes < 0 || a->max_def < 0 || a->max_def > 255 ||
      a->value_width < 0)
    return PQG_ERR_INVALID_ARG;
  const int64_t n = a->num_rows;
  const int w = a->value_width;
  if (n > 0) {
    if (!a->bitmap || (a->num_values > 0 && !a->values)) return PQG_ERR_INVALID_ARG;
    if (w == 0 ? (a->num_values > 0 && !a->offsets) : a->values_bytes < (int64_t)w * a->num_values)
      return PQG_ERR_INVALID_ARG;
    if (w == 0 && a->out_offsets && ((uintptr_t)a->out_offsets & 7)) return PQG_ERR_INVALID_ARG;
  }
  a->rows_out = a->values_out = a->bytes_out = 0;
  c->flt_ms = 0.f;
  if (n == 0) return PQG_OK;
  hipSetDevice(c->device);
  const int64_t nseg = (n + flt::kSeg - 1) / flt::kSeg;
  if (c->flt_buf.grow(sizeof(int64_t) * (size_t)(4 * nseg + 4))) return PQG_ERR_HIP;
  int64_t* seg = (int64_t*)c->flt_buf.p;
  int64_t* tot = seg + 4 * nseg;
  flt::Sel s;
  memset(&s, 0, sizeof(s));
  s.bitmap = (uintptr_t)a->bitmap;
  s.def = a->max_def > 0 ? (uintptr_t)a->def_levels : 0;
  s.values = (uintptr_t)a->values;
  s.offsets = (uintptr_t)a->offsets;
  s.out_def = (uintptr_t)a->out_def_levels;
  s.out_values = (uintptr_t)a->out_values;
  s.out_offsets = w == 0 ? (uintptr_t)a->out_offsets : 0;
  s.n = n;
  s.num_values = a->num_values;
  s.values_bytes = a->values_bytes;
  s.max_def = a->max_def;
  s.width = w;
  int64_t h[4] = {0, 0, 0, 0};
  const int e = count_pass(c, c->ev_flt, [&] { return select_launch(c->stream, s, seg, tot); }, tot, h, 4, &c->flt_ms);
  if (e) return e;
  a->rows_out = h[1];
  a->values_out = h[2];
  a->bytes_out = w == 0 ? h[3] : h[2] * w;
  return PQG_OK;
}

// K9s: row ranges into a row bitmap of pqg_filter's layout (pqg_filter.hip).
int pqg_range_bitmap(pqg_ctx* c, const int64_t* ranges, int n, int64_t num_rows, uint8_t* bitmap) {
  if (!c || n < 0 || num_rows < 0 || (n > 0 && !ranges) || (num_rows > 0 && !bitmap) || ((uintptr_t)bitmap & 3))
    return PQG_ERR_INVALID_ARG;
  int64_t end = 0;  // of the range before
  for (int k = 0; k < n; k++) {
    const int64_t lo = ranges[2 * k], hi = ranges[2 * k + 1];
    if (lo < end || hi < lo || hi > num_rows) return PQG_ERR_INVALID_ARG;
    end = hi;
  }
  c->flt_ms = 0.f;
  if (num_rows == 0) return PQG_OK;
  hipSetDevice(c->device);
  const size_t bytes = sizeof(int64_t) * 2 * (size_t)n;
  if (c->flt_buf.grow(bytes + 16)) return PQG_ERR_HIP;
  if (n > 0 && copy_sync(c, c->flt_buf.p, ranges, bytes, hipMemcpyHostToDevice)) return PQG_ERR_HIP;
  hipEventRecord(c->ev_flt[0], c->stream);
  const int e = range_bitmap_launch(c->stream, (const int64_t*)c->flt_buf.p, n, num_rows, bitmap);
  if (e) return e;
  hipEventRecord(c->ev_flt[1], c->stream);
  if (hipStreamSynchronize(c->stream) != hipSuccess) return PQG_ERR_HIP;
  hipEventElapsedTime(&c->flt_ms, c->ev_flt[0], c->ev_flt[1]);
  return PQG_OK;
}

int pqg_last_filter_ms(pqg_ctx* c, float* ms) {
  if (!c || !ms) return PQG_ERR_INVALID_ARG;
  *ms = c->flt_ms;
  return PQG_OK;
}

// K10: logical-type conversion of dense values (pqg_convert.hip).
int pqg_convert(pqg_ctx* c, pqg_convert_args* a) {
  if (!c || !a || a->num_values < 0 || a->values_bytes < 0) return PQG_ERR_INVALID_ARG;
  a->num_bad = 0;
  const int64_t n = a->num_values;
  const int w = a->in_width, ow = a->out_width;
  const bool var = a->offsets != nullptr;
  switch (a->kind) {
    case PQG_CONV_DECIMAL_BE:
      if (ow != 16 && ow != 32) return PQG_ERR_INVALID_ARG;
      if (var ? w != 0 : (w < 1 || w > 32 || w > ow)) return PQG_ERR_INVALID_ARG;
      break;
    case PQG_CONV_DECIMAL_INT:
      if ((ow != 16 && ow != 32) || (w != 4 && w != 8) || var) return PQG_ERR_INVALID_ARG;
      break;
    case PQG_CONV_INT96_TIME:
      if (ow != 8 || w != 12 || var || a->unit < PQG_UNIT_SECONDS || a->unit > PQG_UNIT_NANOS) return PQG_ERR_INVALID_ARG;
      break;
    default: return PQG_ERR_INVALID_ARG;
  }
  if (!var && a->values_bytes / w < n) return PQG_ERR_INVALID_ARG;  // values_bytes < n * w, without the product
  if (n > INT64_MAX / ow) return PQG_ERR_INVALID_ARG;
  if (((uintptr_t)a->out & 15) || (var && ((uintptr_t)a->offsets & 7))) return PQG_ERR_INVALID_ARG;
  c->conv_ms = 0.f;
  if (n == 0) return PQG_OK;
  if (!a->out || (!a->values && a->values_bytes > 0) || (!var && !a->values)) return PQG_ERR_INVALID_ARG;
  hipSetDevice(c->device);
  float count_ms = 0.f;
  if (var) {
    if (c->conv_buf.grow(sizeof(int64_t))) return PQG_ERR_HIP;
    int64_t* tot = (int64_t*)c->conv_buf.p;
    int64_t bad = 0;
    const int e = count_pass(c, c->ev_conv, [&] { return convert_count_launch(c->stream, a, tot); }, tot, &bad, 1, &count_ms);
    if (e) return e;
    c->conv_ms = count_ms;
    if (bad > 0) {
      a->num_bad = bad;
      return PQG_ERR_SIZE;
    }
  }
  hipEventRecord(c->ev_conv[2], c->stream);
  int e = convert_launch(c->stream, a);
  if (e) return e;
  hipEventRecord(c->ev_conv[3], c->stream);
  e = hip_ok(hipStreamSynchronize(c->stream));
  float ms = 0.f;
  hipEventElapsedTime(&ms, c->ev_conv[2], c->ev_conv[3]);
  c->conv_ms = count_ms + ms;
  return e;
}

int pqg_last_convert_ms(pqg_ctx* c, float* ms) {
  if (!c || !ms) return PQG_ERR_INVALID_ARG;
  *ms = c->conv_ms;
  return PQG_OK;
}

int pqg_decode_page(pqg_ctx* c, const pqg_page_job* pj, pqg_chunk_result* result) {
  if (!c || !pj || !result || !pj->page || pj->page_len <= 0 || pj->dict_page_len < 0 ||
      (pj->dict_page_len > 0 && !pj->dict_page))
    return PQG_ERR_INVALID_ARG;
  if (pj->col.flags & PQG_COL_KEEP_DICT) return PQG_ERR_INVALID_ARG;  // a chunk-level result (pqg_get_dictionary)
  hipSetDevice(c->device);
  const int64_t dl = pj->dict_page ? pj->dict_page_len : 0, total = dl + pj->page_len;
  // the page (after its dictionary) as a one-page column chunk
  if (c->page_stage.grow((size_t)total + 64)) return PQG_ERR_HIP;
  uint8_t* st = (uint8_t*)c->page_stage.p;
  if ((dl && hipMemcpyAsync(st, pj->dict_page, (size_t)dl, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) ||
      hipMemcpyAsync(st + dl, pj->page, (size_t)pj->page_len, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
    return PQG_ERR_HIP;
  pqg_chunk_job job;
  memset(&job, 0, sizeof(job));
  job.col = pj->col;
  job.data = st;
  job.data_len = total;
  job.total_compressed_size = total;
  job.data_page_offset = dl;
  job.total_uncompressed_size = total;
  return pqg_decode_chunks(c, &job, 1, result);
}

int pqg_block_decompress(pqg_ctx* c, int codec, const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap,
                         int64_t* out_len) {
  if (!c || (!src && n > 0) || n < 0 || n > INT32_MAX || !out_len) return PQG_ERR_INVALID_ARG;
  *out_len = 0;
  if (codec == PQG_CODEC_UNCOMPRESSED) {
    *out_len = n;
    if (n > cap) return PQG_ERR_CAPACITY;
    if (n) memcpy(dst, src, (size_t)n);
    return PQG_OK;
  }
  if (codec == PQG_CODEC_GZIP) return block_inflate(c, src, n, dst, cap, out_len);
  if (codec == PQG_CODEC_ZSTD) return block_zstd(c, src, n, dst, cap, out_len);
  if (codec == PQG_CODEC_LZ4_RAW) return block_lz4(c, src, n, dst, cap, out_len);
  if (codec == PQG_CODEC_SNAPPY) return block_snappy(c, src, n, dst, cap, out_len);
  return PQG_ERR_UNSUPPORTED;
}

int pqg_pack_levels(pqg_ctx* c, const uint8_t* levels, int64_t n, int max_level, uint8_t* packed) {
  if (!c || n < 0 || max_level < 0 || max_level > 255 || (n > 0 && (!levels || !packed))) return PQG_ERR_INVALID_ARG;
  hipSetDevice(c->device);
  int bw = 0;
  while ((max_level >> bw) != 0) bw++;  // bits.Len16(maxLevel)
  int e = pack_levels_launch(c->stream, levels, n, bw, packed);
  if (e) return e;
  return hip_ok(hipStreamSynchronize(c->stream));
}

int pqg_crc32(pqg_ctx* c, const uint8_t* dev, int64_t n, uint32_t* out) {
  if (!c || !out || n < 0 || (!dev && n > 0)) return PQG_ERR_INVALID_ARG;
  *out = 0;
  if (n == 0) return PQG_OK;
  hipSetDevice(c->device);
  const int64_t nt = crc::num_tiles((uintptr_t)dev, n);
  if (nt > INT32_MAX) return PQG_ERR_UNSUPPORTED;
  // [Rec][counter + queue ints][TileRec nt][raw nt]
  const size_t o_q = sizeof(crc::Rec), o_t = o_q + sizeof(int) * kQueueInts, o_r = o_t + sizeof(crc::TileRec) * (size_t)nt;
  if (c->crc_one.grow(o_r + sizeof(uint32_t) * (size_t)nt)) return PQG_ERR_HIP;
  uint8_t* b = (uint8_t*)c->crc_one.p;
  crc::Rec* rec = (crc::Rec*)b;
  int* q = (int*)(b + o_q);
  crc::TileRec* tiles = (crc::TileRec*)(b + o_t);
  uint32_t* raws = (uint32_t*)(b + o_r);
  crc::Rec h;
  memset(&h, 0, sizeof(h));
  h.p = dev;
  h.n = n;
  h.state = crc::kPending;
  if (hipMemcpyAsync(rec, &h, sizeof(h), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemsetAsync(q, 0, sizeof(int) * kQueueInts, c->stream) != hipSuccess)
    return PQG_ERR_HIP;
  const int cap = (int)(c->crc_cap_limit > 0 ? std::min<int64_t>(nt, c->crc_cap_limit) : nt);
  hipLaunchKernelGGL(k_crc_plan, dim3(1), dim3(64), 0, c->stream, nullptr, nullptr, nullptr, nullptr, 1, rec, tiles,
                     cap, q + kCrcTileCtr);
  hipLaunchKernelGGL(k_page_crc, dim3(qgrid(std::min<int64_t>((nt + 3) / 4, (int64_t)c->num_cus * c->crc_per_cu))), dim3(kCrcThreads), 0,
                     c->stream, rec, tiles, q + kCrcTileCtr, cap, q, raws);
  hipLaunchKernelGGL(k_crc_fin, dim3(1), dim3(64), 0, c->stream, nullptr, nullptr, nullptr, 1, rec, raws);
  if (hipGetLastError() != hipSuccess || copy_sync(c, &h, rec, sizeof(h), hipMemcpyDeviceToHost)) return PQG_ERR_HIP;
  if (h.state != crc::kVerified && h.state != crc::kMismatch) return PQG_ERR_HIP;
  *out = h.computed;
  return PQG_OK;
}

}  // extern "C"
