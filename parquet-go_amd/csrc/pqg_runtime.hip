// pqg_runtime.hip — host runtime behind include/pqgpu.h (libpqgpu.so): the batch pipeline.
//
// One pqg_ctx per GPU (pqg_ctx.h): a HIP stream, grow-only device arenas and a pinned
// host mirror of the job table.  pqg_decode_chunks_async enqueues the kernel
// pipeline (the kernels of pqg_kernels.h) for a batch of column chunks whose bytes are
// already resident in HBM; pqg_sync waits and reports per-chunk status.  No
// allocation or host synchronisation happens inside the enqueue once the
// arenas have grown to the working-set size (capture-safe steady state).
// The single-shot entry points (one block, one page, assemble, filter, ...) are in pqg_ops.hip.
#include <hip/hip_runtime.h>
#include <cstdlib>

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "pqg_ctx.h"
#include "pqg_crc.h"
#include "pqg_kernels.h"
#include "pqg_zstd.h"

using namespace pqg;

namespace {

constexpr int kMaxAttempts = 6;  // decode + up to 5 arena grows in one pqg_sync

JobKey job_key(const pqg_chunk_job& j) {
  return JobKey{(uintptr_t)j.data, j.total_compressed_size, j.num_values_hint, (j.col.flags & PQG_COL_KEEP_DICT) ? 1 : 0};
}

int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

int value_width_of(const pqg_column_desc& c) {
  switch (c.physical_type) {
    case PQG_BOOLEAN: return 1;
    case PQG_INT32: case PQG_FLOAT: return 4;
    case PQG_INT64: case PQG_DOUBLE: return 8;
    case PQG_INT96: return 12;
    case PQG_FIXED_LEN_BYTE_ARRAY: return c.type_length > 0 ? c.type_length : 0;
  }
  return 0;
}

// The capacities a job ran with; grow: at least what the job reported it needs (PQG_ERR_CAPACITY), too.
Caps caps_of(const JobDev& d, bool grow) {
  auto cap = [&](int64_t need, int64_t had) { return grow ? std::max(need, had) : had; };
  Caps f;
  f.pages = cap((int64_t)d.num_pages + 16, d.page_cap);
  f.slots = cap(d.num_slots + 64, d.slot_cap);
  f.scratch = cap(d.need_scratch + 1024, d.scratch_cap);
  f.values = cap(d.value_width > 0 ? std::max<int64_t>(d.num_values, d.num_slots) * d.value_width + 64 : d.values_bytes + 1024,
                 d.value_cap);
  f.runs = cap(d.run_used + 64, d.run_cap);
  f.blks = cap(d.blk_used + 64, d.blk_cap);
  f.doffs = cap(d.need_doffs + 64, d.doffs_cap);
  f.dchars = cap(d.need_dchars + 64, d.dchars_cap);
  return f;
}

// Environment knobs of a context: a boolean (NAME=0/1), a positive integer (anything else leaves the default).
void env_flag(const char* name, bool* v) {
  if (const char* e = getenv(name)) *v = atoi(e) != 0;
}
template <class T>
void env_positive(const char* name, T* v) {
  if (const char* e = getenv(name))
    if (atoi(e) > 0) *v = atoi(e);
}

// resident workgroups of `threads` threads per CU, where the query answers; else *per_cu keeps its default
template <class K>
void occupancy(K* kernel, int threads, int* per_cu) {
  int o = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, reinterpret_cast<const void*>(kernel), threads, 0) == hipSuccess && o > 0)
    *per_cu = o;
}

}  // namespace

void pqg::launch_snappy(pqg_ctx* c, hipStream_t s, JobDev* jobs, PageDev* pages, const int* list, const int* total,
                        int64_t list_cap, int* sctr, int* q_split, int* q_serial, uint8_t* scratch,
                        const SnapTables& T) {
  const int waves = c->num_cus * c->snappy_per_cu;  // as many as fit (LDS: the history ring)
  hipMemsetAsync(sctr, 0, 2 * sizeof(int), s);
  hipLaunchKernelGGL(k_snap_plan, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((list_cap + 255) / 256, c->num_cus * 4))),
                     dim3(256), 0, s, jobs, pages, list, total, sctr, T.subs, T.sub_cap, T.segpage, T.seg_cap);
  hipLaunchKernelGGL(k_snap_seg, dim3(c->num_cus * c->seg_waves), dim3(64), 0, s, jobs, pages, T.segpage, sctr + 1, T.seg_cap, T.F);
  hipLaunchKernelGGL(k_snap_link, dim3(c->num_cus * c->link_waves), dim3(64), 0, s, jobs, pages, list, total, T.subs, T.F);
  hipLaunchKernelGGL(k_snap_decode, dim3(qgrid(waves)), dim3(64), 0, s, jobs, pages, T.subs, sctr, T.sub_cap, q_split,
                     scratch);
  hipLaunchKernelGGL(k_snappy, dim3(qgrid(waves)), dim3(64), 0, s, jobs, pages, list, total, q_serial, scratch);
}

extern "C" {

const char* pqg_status_string(int s) {
  switch (s) {
    case PQG_OK: return "ok";
    case PQG_ERR_EOF: return "unexpected end of stream";
    case PQG_ERR_THRIFT: return "page header: thrift decode failed";
    case PQG_ERR_PAGE_HEADER: return "page header: missing or negative field";
    case PQG_ERR_SIZE: return "page size mismatch";
    case PQG_ERR_SNAPPY: return "snappy: corrupt input";
    case PQG_ERR_RLE: return "rle: invalid run";
    case PQG_ERR_DICT_INDEX: return "dict: invalid index";
    case PQG_ERR_BIT_WIDTH: return "invalid bit width";
    case PQG_ERR_DELTA: return "delta: invalid stream";
    case PQG_ERR_UNSUPPORTED: return "unsupported encoding/codec/type";
    case PQG_ERR_DICT_PAGE: return "there should be only one dictionary";
    case PQG_ERR_BYTE_ARRAY: return "bytearray/plain: len is negative";
    case PQG_ERR_LEVELS: return "level reader is not initialized";
    case PQG_ERR_FIXED_LEN: return "bytearray/delta: value length is not the fixed length";
    case PQG_ERR_GZIP: return "gzip: invalid data";
    case PQG_ERR_ZSTD: return "zstd: invalid frame / block / checksum";
    case PQG_ERR_LZ4: return "lz4: invalid block";
    case PQG_ERR_CRC: return "page checksum mismatch";
    case PQG_ERR_NOT_DICT: return "keep dictionary: data page is not dictionary encoded";
    case PQG_ERR_CAPACITY: return "capacity";
    case PQG_ERR_INVALID_ARG: return "invalid argument";
    case PQG_ERR_HIP: return "HIP runtime error";
    case PQG_ERR_METADATA: return "invalid file metadata";
    case PQG_ERR_INDEX: return "page index: a located page does not end at offset + size";
  }
  return "unknown";
}

int pqg_ctx_create(int device, pqg_ctx** out) {
  if (!out) return PQG_ERR_INVALID_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return PQG_ERR_HIP;
  if (hipSetDevice(device) != hipSuccess) return PQG_ERR_HIP;
  pqg_ctx* c = new pqg_ctx();
  c->device = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cus = prop.multiProcessorCount;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return PQG_ERR_HIP;
  }
  for (auto& e : c->events) hipEventCreate(&e);
  env_flag("PQG_FILTER_LDS", &c->flt_lds);
  env_flag("PQG_VERIFY_CRC", &c->verify_crc);
  env_positive("PQG_CRC_TILE_CAP", &c->crc_cap_limit);
  env_flag("PQG_DICT4", &c->dict4);
  env_flag("PQG_DICT_BIG", &c->dict_big);
  env_flag("PQG_STRIDE", &c->stride);
  env_flag("PQG_LEV1", &c->lev1);
  env_positive("PQG_SEG_WAVES", &c->seg_waves);
  env_positive("PQG_LEVLONG_WAVES", &c->levlong_waves);
  env_positive("PQG_LINK_WAVES", &c->link_waves);
  env_flag("PQG_LZ4_BATCH", &c->lz4_batch);
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_dict4)) == hipSuccess && fa.maxThreadsPerBlock > 0)
    c->dict4_threads = fa.maxThreadsPerBlock;  // kDWaves * 64 (pqg_dict.hip)
  occupancy(&k_dict4, c->dict4_threads, &c->dict4_per_cu);
  occupancy(&k_snappy, 64, &c->snappy_per_cu);
  occupancy(&k_inflate_s, 64, &c->inflate_per_cu);
  occupancy(&k_zstd, 64, &c->zstd_per_cu);
  occupancy(c->lz4_batch ? &k_lz4_batch : &k_lz4, 64, &c->lz4_per_cu);
  occupancy(&k_page_crc, kCrcThreads, &c->crc_per_cu);
  // the counters, then the kQShards-sharded work queues and the per-stage flags (pqg_common.h)
  if (c->counters.grow(sizeof(int) * (size_t)(kQueueBase + kQueueSlots * kQueueInts))) {
    pqg_ctx_destroy(c);
    return PQG_ERR_HIP;
  }
  *out = c;
  return PQG_OK;
}

void pqg_ctx_destroy(pqg_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  for (auto& e : c->events) hipEventDestroy(e);
  if (c->h_jobs) hipHostFree(c->h_jobs);
  hipStreamDestroy(c->stream);
  delete c;  // every DevBuf frees its memory
}

int pqg_device_alloc(pqg_ctx* c, int64_t bytes, void** dptr) {
  if (!c || !dptr) return PQG_ERR_INVALID_ARG;
  hipSetDevice(c->device);
  return hip_ok(hipMalloc(dptr, (size_t)std::max<int64_t>(bytes, 1)));
}
int pqg_device_free(pqg_ctx* c, void* dptr) {
  if (!c) return PQG_ERR_INVALID_ARG;
  hipSetDevice(c->device);
  return hip_ok(hipFree(dptr));
}
int pqg_memcpy_h2d(pqg_ctx* c, void* dst, const void* src, int64_t bytes) {
  if (!c) return PQG_ERR_INVALID_ARG;
  hipSetDevice(c->device);
  return copy_sync(c, dst, src, (size_t)bytes, hipMemcpyHostToDevice);
}
int pqg_memcpy_d2h(pqg_ctx* c, void* dst, const void* src, int64_t bytes) {
  if (!c) return PQG_ERR_INVALID_ARG;
  hipSetDevice(c->device);
  return copy_sync(c, dst, src, (size_t)bytes, hipMemcpyDeviceToHost);
}

// Plan arena regions for the current batch and upload the job table.
static int plan_batch(pqg_ctx* c) {
  const int n = c->n_jobs;
  if (c->h_jobs_cap < n) {
    if (c->h_jobs) hipHostFree(c->h_jobs);
    c->h_jobs_cap = std::max(n, 64);
    if (hipHostMalloc((void**)&c->h_jobs, sizeof(JobDev) * (size_t)c->h_jobs_cap) != hipSuccess) return PQG_ERR_HIP;
  }
  int64_t page_total = 0, slot_total = 0, value_total = 0, scratch_total = 0, tile_total = 0, run_total = 0,
          blk_total = 0, offs_total = 0, doffs_total = 0, seg_total = 0, dchars_total = 0;
  // a job's region of an arena: the estimate unless a capacity is forced, at the arena's end so far,
  // which moves on by the capacity rounded up to `align`
  auto region = [](int64_t estimate, int64_t forced, int64_t align, auto& cap, int64_t& base, int64_t& total) {
    const int64_t v = forced > 0 ? forced : estimate;
    cap = (std::remove_reference_t<decltype(cap)>)v;
    base = total;
    total += align_up(v, align);
    return v;
  };
  c->plan.resize((size_t)n);
  for (int i = 0; i < n; i++) {
    const pqg_chunk_job& in = c->cur[(size_t)i];
    const Caps& f = c->force[(size_t)i];
    JobDev d;
    memset(&d, 0, sizeof(d));
    d.data = in.data;
    d.data_len = in.data_len;
    d.tcs = in.total_compressed_size;
    d.data_page_offset = in.data_page_offset;
    d.type = in.col.physical_type;
    d.type_length = in.col.type_length;
    d.max_def = in.col.max_def;
    d.max_rep = in.col.max_rep;
    d.codec = in.col.codec;
    d.has_dict_off = in.has_dict_page_offset;
    // a keep-dictionary job stores int32 keys: a 4-byte value arena, no offsets, no chars
    d.keep_dict = (in.col.flags & PQG_COL_KEEP_DICT) ? 1 : 0;
    d.entry_width = value_width_of(in.col);
    d.value_width = d.keep_dict ? 4 : d.entry_width;
    // a located job (its pages are listed: no tiles, nothing walked): it means the job of its pages back to
    // back, which has no dictionary page offset
    d.n_locs = c->n_locs[(size_t)i];
    d.loc_base = c->loc_base[(size_t)i];
    const bool located = d.n_locs > 0;
    d.no_prewalk = !located && c->many_pages.count(job_key(in)) ? 1 : 0;
    if (located) {
      d.scan_fallback = 3;
      d.has_dict_off = 0;
    }
    const int64_t page_max = (int64_t)1 << 30;
    const int64_t pcap = region(located ? (int64_t)d.n_locs + 16 : std::min(in.total_compressed_size / 256 + 16, page_max),
                                std::min(f.pages, page_max), 1, d.page_cap, d.page_base, page_total);
    const int64_t scap =
        region(std::max<int64_t>(in.num_values_hint, 0) + 64, f.slots, 256, d.slot_cap, d.slot_base, slot_total);
    // variable-length values: chars estimated from the page bytes (dictionary
    // chunks may need more: the first decode reports it and the arena grows)
    region(d.value_width > 0 ? scap * d.value_width
                             : std::max<int64_t>(in.total_uncompressed_size, in.total_compressed_size) + 1024,
           f.values, 256, d.value_cap, d.value_base, value_total);
    const int64_t xcap = region(in.col.codec != PQG_CODEC_UNCOMPRESSED
                                    ? std::max<int64_t>(in.total_uncompressed_size, in.total_compressed_size) + pcap * 16 + 1024
                                    : 0,
                                f.scratch, 256, d.scratch_cap, d.scratch_base, scratch_total);
    if (in.col.codec != PQG_CODEC_UNCOMPRESSED) seg_total += in.total_compressed_size / kSnapSeg + pcap;
    d.dict_page = -1;
    d.error_page = -1;
    const int64_t lim = std::max<int64_t>(0, std::min(in.total_compressed_size, in.data_len));
    // hybrid run tables: a stream of n bytes has at most n/2 + 2 runs, and a
    // page at most three streams (see reg_stream)
    const int64_t rcap =
        region((in.total_compressed_size + xcap) / 2 + 6 * pcap + 64, f.runs, 1, d.run_cap, d.run_base, run_total);
    region(3 * (scap / kHBlock + 3 * pcap) + rcap / kHBlockRuns + 2 * rcap / (kHBlockBytes / 2) + 64, f.blks, 1, d.blk_cap,
           d.blk_base, blk_total);
    // offsets: variable-length values; FLBA columns too (their DELTA_BYTE_ARRAY
    // pages park prefix / suffix lengths there, k_str_delta)
    if (d.value_width == 0 || (d.type == PQG_FIXED_LEN_BYTE_ARRAY && !d.keep_dict))
      region(scap + 1, 0, 32, d.offs_cap, d.offs_base, offs_total);
    if (d.entry_width == 0) {
      // dictionary entries take >= 4 bytes each
      region(std::min<int64_t>(std::max<int64_t>(in.total_uncompressed_size, 0) / 4, 1 << 17) + 64, f.doffs, 32, d.doffs_cap,
             d.doffs_base, doffs_total);
      if (d.keep_dict)  // the dictionary's chars (k_dict_export); a larger page: the first decode reports it
        region(std::min<int64_t>(std::max<int64_t>(in.total_uncompressed_size, 0), 1 << 20) + 64, f.dchars, 256,
               d.dchars_cap, d.dchars_base, dchars_total);
    }
    d.tile_base = tile_total;
    d.n_tiles = located ? 0 : (int32_t)((lim + kScanTile - 1) / kScanTile);
    tile_total += d.n_tiles;
    c->plan[(size_t)i] = d;
    c->h_jobs[i] = d;
  }
  c->list_cap = page_total;
  // big pages (pqg_common.h): a page of nn values has <= nn / kPart + 1 parts;
  // a long level run (rep and def streams) has > kLongLev values, a long
  // value-stream run > kLongWalk
  c->parts_cap = page_total + slot_total / kPart + n + 64;
  c->lev_long_cap = 2 * slot_total / kLongLev + 64;
  c->lev_piece_cap = 2 * slot_total / kLevPiece + 2 * c->lev_long_cap + 64;
  c->walk_long_cap = slot_total / kLongWalk + 64;
  if (c->parts.grow(sizeof(PartRec) * (size_t)c->parts_cap) || c->lev_long.grow(sizeof(LongLev) * (size_t)c->lev_long_cap) ||
      c->lev_pieces.grow(sizeof(LevPiece) * (size_t)c->lev_piece_cap) ||
      c->walk_long.grow(sizeof(LongWalk) * (size_t)c->walk_long_cap))
    return PQG_ERR_HIP;
  // K2 split tables: a page of u bytes has ceil(u / 64 KiB) sub-blocks (>= 1)
  // and a block of b bytes ceil(b / 4 KiB) segments
  c->sn_sub_cap = scratch_total / kSnapSub + page_total + 64;
  c->sn_seg_cap = seg_total + 64;
  // k_zstd: one literal workspace per wave of its grid
  if (c->batch.any_zstd && c->zstd_ws.grow((size_t)zstd_grid(c) * zstd::kWsBytes)) return PQG_ERR_HIP;
  if (c->sn_subs.grow(sizeof(SnapSub) * (size_t)c->sn_sub_cap) || c->sn_segpage.grow(sizeof(int) * (size_t)c->sn_seg_cap) ||
      c->sn_F.grow(sizeof(uint2) * 64 * (size_t)c->sn_seg_cap))
    return PQG_ERR_HIP;
  if (c->jobs.grow(sizeof(JobDev) * (size_t)n) || c->pages.grow(sizeof(PageDev) * (size_t)page_total) ||
      c->list.grow(sizeof(int) * (size_t)std::max<int64_t>(page_total, 1)) || c->def_arena.grow((size_t)slot_total + 64) ||
      c->rep_arena.grow((size_t)slot_total + 64) || c->value_arena.grow((size_t)value_total + 64) ||
      c->scratch.grow((size_t)scratch_total + 64) || c->tile_count.grow(sizeof(int) * (size_t)tile_total + 64) ||
      c->tile_off.grow(sizeof(int) * (size_t)tile_total + 64) || c->tile_okc.grow(sizeof(int) * (size_t)tile_total + 64) ||
      c->tile_okoff.grow(sizeof(int) * (size_t)tile_total + 64) || c->tile_job.grow(sizeof(int) * (size_t)tile_total + 64) ||
      c->ok2slot.grow(sizeof(int) * (size_t)tile_total * kCandPerTile + 64) ||
      c->cand_pos.grow(sizeof(int64_t) * (size_t)tile_total * kCandPerTile + 64) ||
      c->cand_list.grow(sizeof(int) * (size_t)(tile_total + kQShards) * kCandPerTile + 64) ||
      // the tiles' candidates, then the located region: one record per listed page
      c->cands.grow(sizeof(Cand) * ((size_t)tile_total * kCandPerTile + c->h_locs.size()) + 64) ||
      c->succ.grow(sizeof(int) * (size_t)tile_total * kCandPerTile + 64) ||
      c->idx2slot.grow(sizeof(int) * (size_t)tile_total * kCandPerTile + 64) ||
      c->order.grow(sizeof(int) * (size_t)page_total + 64) ||
      c->streams.grow(sizeof(HStream) * 3 * (size_t)page_total + 64) ||
      // slack past the last entry: k_dict4 stages run / descriptor granules past a stream's end
      c->runs.grow(sizeof(RunEnt) * (size_t)run_total + 8192) || c->blks.grow(sizeof(BlockDesc) * (size_t)blk_total + 8192) ||
      c->vrecs.grow(sizeof(VRec) * (size_t)std::max<int64_t>(c->parts_cap, 1)) ||
      c->offs_arena.grow(sizeof(int64_t) * (size_t)offs_total + 64) ||
      c->doffs_arena.grow(sizeof(int64_t) * (size_t)doffs_total + 64))
    return PQG_ERR_HIP;
  if (c->batch.any_keep_var &&
      (c->aoffs_arena.grow(sizeof(int64_t) * (size_t)doffs_total + 64) || c->dchars_arena.grow((size_t)dchars_total + 64)))
    return PQG_ERR_HIP;
  if (c->verify_crc) {
    // pages do not overlap: a page of s bytes has at most s / kTile + 2 tiles (a table too small for
    // a chunk whose pages do overlap is no error: k_crc_fin reads what did not fit itself)
    int64_t ct = 2 * page_total + 64;
    for (int i = 0; i < n; i++) ct += std::max<int64_t>(0, c->cur[(size_t)i].data_len) / crc::kTile;
    c->crc_tile_cap = std::min<int64_t>(ct, INT32_MAX / kQShards);
    if (c->crc_cap_limit > 0) c->crc_tile_cap = std::min(c->crc_tile_cap, c->crc_cap_limit);
    if (c->crc_recs.grow(sizeof(crc::Rec) * (size_t)std::max<int64_t>(page_total, 1)) ||
        c->crc_tiles.grow(sizeof(crc::TileRec) * kQShards * (size_t)c->crc_tile_cap) ||  // a region per counter shard
        c->crc_raws.grow(sizeof(uint32_t) * kQShards * (size_t)c->crc_tile_cap))
      return PQG_ERR_HIP;
  }
  c->total_tiles = tile_total;
  int64_t max_tiles = 0, max_pages = 0;
  for (int i = 0; i < n; i++) {
    max_tiles = std::max<int64_t>(max_tiles, c->plan[(size_t)i].n_tiles);
    max_pages = std::max<int64_t>(max_pages, c->plan[(size_t)i].page_cap);
  }
  c->tile_blocks = (int)std::max<int64_t>(1, (max_tiles + kChunkBlock - 1) / kChunkBlock);
  c->page_blocks = (int)std::min<int64_t>(kChunkBlocks, std::max<int64_t>(1, (max_pages + kChunkBlock - 1) / kChunkBlock));
  if (c->nn_sums.grow(sizeof(NnSums) * (size_t)n * (size_t)c->page_blocks) || c->nn_jobs.grow(sizeof(NnJob) * (size_t)n))
    return PQG_ERR_HIP;
  return hip_ok(hipMemcpyAsync(c->jobs.p, c->h_jobs, sizeof(JobDev) * (size_t)n, hipMemcpyHostToDevice, c->stream));
}

static int launch_pipeline(pqg_ctx* c) {
  const int n = c->n_jobs;
  const BatchTraits& b = c->batch;
  c->launches++;
  c->last_timed = c->timed;
  JobDev* jobs = (JobDev*)c->jobs.p;
  PageDev* pages = (PageDev*)c->pages.p;
  int* list = (int*)c->list.p;
  int* ctr = (int*)c->counters.p;  // [0] total pages in the list
  // work queue k (sharded over the XCDs, see queue_pull) and the stage flags: the kQueue* names of pqg_common.h
  auto Q = [&](int k) { return ctr + kQueueBase + k * kQueueInts; };
  uint8_t* scratch = (uint8_t*)c->scratch.p;
  // page-queue kernels: one wave per page; enough waves per SIMD to hide the
  // dependent HBM reads (bounded by VGPRs / LDS per kernel)
  const int waves = c->num_cus * 20;
  hipStream_t s = c->stream;
  if (c->timed) hipEventRecord(c->ev[0], s);
  hipMemsetAsync(ctr + kQueueBase, 0, sizeof(int) * kQueueSlots * kQueueInts, s);  // queues + the stage flags (kModePresentOff)
  const int64_t nt = c->total_tiles;
  int* tcount = (int*)c->tile_count.p;
  int* toff = (int*)c->tile_off.p;
  Cand* cands = (Cand*)c->cands.p;
  int* tokc = (int*)c->tile_okc.p;
  int* tokoff = (int*)c->tile_okoff.p;
  // chunks of a few big pages (parquet-go's writer layout) are walked first
  // and skipped by the candidate scan
  if (b.prewalk) hipLaunchKernelGGL(k_scan_pages, dim3(n), dim3(64), 0, s, jobs, pages, n, kPrewalkPages, (int)c->stride);
  if (nt > 0) {
    int64_t* cpos = (int64_t*)c->cand_pos.p;
    int* clist = (int*)c->cand_list.p;
    const int region = (int)((nt + kQShards - 1) / kQShards) * kCandPerTile;  // one list region per head
    hipLaunchKernelGGL(k_tile_jobs, dim3(n, (unsigned)std::min(c->tile_blocks, 64)), dim3(256), 0, s, jobs, (int*)c->tile_job.p);
    hipLaunchKernelGGL(k_page_cands, dim3((unsigned)nt), dim3(256), 0, s, jobs, (const int*)c->tile_job.p, tcount, tokc,
                       cpos, clist, Q(kQueueCands),
                       region);
    hipLaunchKernelGGL(k_cand_parse, dim3((unsigned)std::min<int64_t>((nt * kCandPerTile + 255) / 256, c->num_cus * 4)),
                       dim3(256), 0, s, jobs, (const int*)c->tile_job.p, clist, Q(kQueueCands), region, tokc, cpos, cands);
  }
  const dim3 tile_grid(n, (unsigned)c->tile_blocks), page_grid(n, (unsigned)c->page_blocks);
  hipLaunchKernelGGL(k_tile_scan, tile_grid, dim3(1024), 0, s, jobs, tcount, tokc, toff, tokoff);
  // located jobs: one lane per listed page (after k_tile_scan, which resets their results)
  const int nl = (int)c->h_locs.size();
  Cand* lcands = cands + nt * kCandPerTile;
  if (nl > 0)
    hipLaunchKernelGGL(k_scan_located, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, s, jobs, (const LocDev*)c->locs.p, nl,
                       lcands);
  if (nt > 0)
    hipLaunchKernelGGL(k_cand_link, dim3((unsigned)((nt * kCandPerTile + 255) / 256)), dim3(256), 0, s, jobs,
                       (const int*)c->tile_job.p, nt,
                       tcount, toff, tokoff, cands, (int*)c->succ.p, (int*)c->idx2slot.p, (int*)c->ok2slot.p);
  hipLaunchKernelGGL(k_page_chain, page_grid, dim3(1024), 0, s, jobs, pages, cands, (const int*)c->succ.p,
                     (const int*)c->idx2slot.p, (const int*)c->ok2slot.p, (int*)c->order.p);
  if (nl > 0) hipLaunchKernelGGL(k_chain_located, page_grid, dim3(1024), 0, s, jobs, pages, lcands, (int*)c->order.p);
  hipLaunchKernelGGL(k_scan_pages, dim3(n), dim3(64), 0, s, jobs, pages, n, 0, 0);
  if (c->timed) hipEventRecord(c->ev[1], s);
  hipLaunchKernelGGL(k_page_list, page_grid, dim3(1024), 0, s, jobs, pages, n, list,
                     (int)std::min<int64_t>(c->list_cap, INT32_MAX), ctr, ctr + kCtrZeroed);
  if (c->timed) hipEventRecord(c->ev[2], s);
  c->crc_ran = c->verify_crc;
  c->crc_timed = c->verify_crc && c->timed;
  if (c->verify_crc) {
    // K1c (pqg_crc.hip), before any decompressor: a page that fails gets read_status = kCRC here, and
    // they, the level stage and the values stages skip pages whose read phase failed; k_finalize
    // then ranks it among the read-phase errors.  Part of the decompression stage's time (ev[2] .. ev[3]).
    crc::Rec* recs = (crc::Rec*)c->crc_recs.p;
    crc::TileRec* ctiles = (crc::TileRec*)c->crc_tiles.p;
    uint32_t* raws = (uint32_t*)c->crc_raws.p;
    int* tile_ctr = Q(kQueueCrc) + kCrcTileCtr;
    const unsigned page_waves = (unsigned)std::max<int64_t>(1, std::min<int64_t>(c->list_cap, (int64_t)c->num_cus * 16));
    if (c->timed) hipEventRecord(c->ev_crc[0], s);
    hipLaunchKernelGGL(k_crc_plan, dim3(page_waves), dim3(64), 0, s, jobs, pages, list, ctr, 0, recs, ctiles,
                       (int)c->crc_tile_cap, tile_ctr);
    hipLaunchKernelGGL(k_page_crc, dim3(qgrid((int64_t)c->num_cus * c->crc_per_cu)), dim3(kCrcThreads), 0, s, recs, ctiles, tile_ctr,
                       (int)c->crc_tile_cap, Q(kQueueCrc), raws);
    hipLaunchKernelGGL(k_crc_fin, dim3(page_waves), dim3(64), 0, s, pages, list, ctr, 0, recs, raws);
    if (c->timed) hipEventRecord(c->ev_crc[1], s);
  }
  if (b.any_snappy) {
    const SnapTables T{(SnapSub*)c->sn_subs.p, (int)std::min<int64_t>(c->sn_sub_cap, INT32_MAX), (int*)c->sn_segpage.p,
                       (int)std::min<int64_t>(c->sn_seg_cap, INT32_MAX), (uint2*)c->sn_F.p};
    launch_snappy(c, s, jobs, pages, list, ctr, c->list_cap, ctr + kCtrSnapSplit, Q(kQueueSnapSplit), Q(kQueueSnapSerial),
                  scratch, T);
  }
  if (b.any_gzip) {  // one wave per GZIP page (pqg_inflate.hip): the 8 KiB ring, then the pages it left
    hipLaunchKernelGGL(k_inflate_s, dim3(qgrid(c->num_cus * c->inflate_per_cu)), dim3(64), 0, s, jobs, pages, list, ctr,
                       Q(kQueueInflate), scratch);
    hipLaunchKernelGGL(k_inflate, dim3(qgrid(c->num_cus * 4)), dim3(64), 0, s, jobs, pages, list, ctr,
                       Q(kQueueInflateRedo), scratch, 1);
  }
  if (b.any_zstd)  // one wave per ZSTD page (pqg_zstd.hip), each with its literal workspace (plan_batch)
    hipLaunchKernelGGL(k_zstd, dim3(zstd_grid(c)), dim3(64), 0, s, jobs, pages, list, ctr, Q(kQueueZstd), scratch,
                       (uint8_t*)c->zstd_ws.p);
  if (b.any_lz4)  // one wave per LZ4_RAW page (pqg_lz4.hip); no workspace
    hipLaunchKernelGGL(c->lz4_batch ? k_lz4_batch : k_lz4, dim3(qgrid((int64_t)c->num_cus * c->lz4_per_cu)), dim3(64), 0, s, jobs, pages, list, ctr,
                       Q(kQueueLz4), scratch);
  if (c->timed) hipEventRecord(c->ev[3], s);
  HStream* streams = (HStream*)c->streams.p;
  RunEnt* runs = (RunEnt*)c->runs.p;
  BlockDesc* blks = (BlockDesc*)c->blks.p;
  // setup + def/rep levels, one wave per data page (value streams registered
  // for the walk); long level runs then expand in pieces over the whole chip
  LongLev* llong = (LongLev*)c->lev_long.p;
  LevPiece* lpieces = (LevPiece*)c->lev_pieces.p;
  const int llc = (int)std::min<int64_t>(c->lev_long_cap, INT32_MAX), lpc = (int)std::min<int64_t>(c->lev_piece_cap, INT32_MAX);
  // each job's dictionary page
  hipLaunchKernelGGL(k_dict_resolve, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, jobs, n, pages, scratch);
  // pages of jobs with 1-bit levels (maxR = 0, maxD <= 1) to the w = 1
  // decoder, the others to the general one; a kernel with no job stays idle
  const int split = b.any_w1 && b.any_gen;
  if (b.any_w1)
    hipLaunchKernelGGL(k_page_levels_w1, dim3(qgrid(c->num_cus * 32)), dim3(64), 0, s, jobs, pages, list, ctr,
                       Q(kQueueLevels), scratch, streams, (uint8_t*)c->def_arena.p, (uint8_t*)c->rep_arena.p, llong, llc,
                       lpieces, lpc, split | (c->lev1 ? 2 : 0));
  if (b.any_gen)
    hipLaunchKernelGGL(k_page_levels, dim3(qgrid(c->num_cus * 24)), dim3(64), 0, s, jobs, pages, list, ctr,
                       Q(split ? kQueueLevGen : kQueueLevels), scratch, streams, (uint8_t*)c->def_arena.p,
                       (uint8_t*)c->rep_arena.p, llong, llc, lpieces, lpc, split);
  // stages with no possible work are not launched (BatchTraits)
  if (b.any_levels)
    hipLaunchKernelGGL(k_level_long, dim3(qgrid(c->num_cus * c->levlong_waves)), dim3(64), 0, s, pages, ctr, llong, llc, lpieces, lpc,
                       Q(kQueueLevLong));
  if (c->timed) hipEventRecord(c->ev[4], s);
  const unsigned walk_blocks = (unsigned)std::max<int64_t>(
      1, std::min<int64_t>((c->list_cap + kWalkLanes - 1) / kWalkLanes, c->num_cus * (2048 / kWalkLanes)));
  LongWalk* wlong = (LongWalk*)c->walk_long.p;
  const int wlc = (int)std::min<int64_t>(c->walk_long_cap, INT32_MAX);
  // one lane per value stream
  hipLaunchKernelGGL(k_hybrid_walk, dim3(walk_blocks), dim3(kWalkLanes), 0, s, pages, list, ctr, streams, runs, blks,
                     wlong, wlc);
  hipLaunchKernelGGL(k_walk_long, dim3(c->num_cus * 2), dim3(256), 0, s, ctr, wlong, wlc, blks);
  if (c->timed) hipEventRecord(c->ev[5], s);
  if (c->timed) hipEventRecord(c->ev[6], s);
  PartRec* parts = (PartRec*)c->parts.p;
  NnSums* nsums = (NnSums*)c->nn_sums.p;
  NnJob* njobs = (NnJob*)c->nn_jobs.p;
  hipLaunchKernelGGL(k_nn_scan_sums, page_grid, dim3(1024), 0, s, jobs, pages, scratch, streams, nsums, njobs, ctr,
                     c->parts_cap);
  hipLaunchKernelGGL(k_nn_scan, page_grid, dim3(1024), 0, s, jobs, pages, scratch, streams, blks, ctr, parts, c->parts_cap,
                     nsums, njobs);
  if (c->timed) hipEventRecord(c->ev[7], s);
  // every values kernel takes the work items (the pages' parts) and keeps the
  // ones whose vmode (set by k_page_levels) is its own
  const int64_t items_cap = c->parts_cap;
  if (!b.any_w4) {
    // no 4-byte column: no mode 1 page
  } else if (c->dict4) {  // 4-byte dictionary pages: pieces staged in LDS, small dictionaries in LDS (pqg_dict.hip)
    VRec* recs = (VRec*)c->vrecs.p;
    hipLaunchKernelGGL(k_dict_plan, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((items_cap + 255) / 256, c->num_cus * 4))),
                       dim3(256), 0, s, jobs, pages, parts, ctr, (uint8_t*)c->value_arena.p, streams, runs, blks, recs);
    // dictionaries past 4096 entries: k_dict4_big (a 104 KiB LDS prefix, one
    // 8-wave workgroup per CU) takes their run-table pages (PQG_DICT_BIG=0: k_dict4)
    hipLaunchKernelGGL(k_dict4, dim3(qgrid(c->num_cus * c->dict4_per_cu)), dim3(c->dict4_threads), 0, s, pages, ctr,
                       Q(kQueueDict4), recs, (int)c->dict_big);
    if (c->dict_big)
      hipLaunchKernelGGL(k_dict4_big, dim3(qgrid(c->num_cus)), dim3(kBigDictThreads), 0, s, pages, ctr,
                         Q(kQueueDictBig), recs);
  } else
    hipLaunchKernelGGL(k_values<1>, dim3(qgrid(waves)), dim3(64), 0, s, jobs, pages, parts, ctr, Q(kQueueDict4),
                       (uint8_t*)c->value_arena.p, streams, runs, blks);
  if (b.any_fixed_other) {
    hipLaunchKernelGGL(k_values<0>, dim3(qgrid(waves)), dim3(64), 0, s, jobs, pages, parts, ctr, Q(kQueueValues),
                       (uint8_t*)c->value_arena.p, streams, runs, blks);
    hipLaunchKernelGGL(k_values<3>, dim3(qgrid(waves)), dim3(64), 0, s, jobs, pages, parts, ctr, Q(kQueueDbp),
                       (uint8_t*)c->value_arena.p, streams, runs, blks);
    // BYTE_STREAM_SPLIT pages (pqg_bss.hip): part of the values stage's time (ev[7] .. ev[8])
    hipLaunchKernelGGL(k_bss, dim3(qgrid(waves)), dim3(64), 0, s, jobs, pages, parts, ctr, Q(kQueueBss),
                       (uint8_t*)c->value_arena.p);
  }
  // K4i (pqg_dictidx.hip): the pages of keep-dictionary jobs, keys stored as they are.  With a byte-array
  // job among them the kernel waits for k_str_dict (the entry count of such a dictionary) and counts
  // in the strings stage's time; no such job in the batch: no launch.
  auto launch_dict_idx = [&]() {
    hipLaunchKernelGGL(k_dict_idx, dim3(qgrid(waves)), dim3(64), 0, s, jobs, pages, parts, ctr, Q(kQueueDictIdx),
                       (uint8_t*)c->value_arena.p, streams, runs, blks);
  };
  if (b.any_keep && !b.any_keep_var) launch_dict_idx();
  if (c->timed) hipEventRecord(c->ev[8], s);
  if (b.any_var)
    hipLaunchKernelGGL(k_str_dict, dim3(n), dim3(512), 0, s, jobs, pages, (int64_t*)c->doffs_arena.p);
  if (b.any_keep_var) {
    launch_dict_idx();
    hipLaunchKernelGGL(k_dict_export, dim3(n, kExportGridY), dim3(kExportThreads), 0, s, jobs, pages,
                       (int64_t*)c->aoffs_arena.p, (uint8_t*)c->dchars_arena.p);
  }
  if (b.any_var_out) {
    int64_t* offs = (int64_t*)c->offs_arena.p;
    hipLaunchKernelGGL(k_str_plain, dim3(qgrid(c->num_cus * 4 * 512 / kPwThreads)), dim3(kPwThreads), 0, s, jobs, pages, list, ctr,
                       Q(kQueueStrPlain), offs);
    hipLaunchKernelGGL(k_str_count, dim3(qgrid(waves)), dim3(64), 0, s, jobs, pages, parts, ctr, Q(kQueueStrCount), offs,
                       streams, runs, blks);
    hipLaunchKernelGGL(k_str_delta, dim3(qgrid(c->num_cus * 8)), dim3(64), 0, s, jobs, pages, list, ctr,
                       Q(kQueueStrDelta), offs);
    hipLaunchKernelGGL(k_char_scan, dim3(n), dim3(256), 0, s, jobs, pages, parts, offs);
    hipLaunchKernelGGL(k_str_copy, dim3(qgrid(c->num_cus * 4)), dim3(512), 0, s, jobs, pages, parts, ctr,
                       Q(kQueueStrCopy), (uint8_t*)c->value_arena.p, offs);
    hipLaunchKernelGGL(k_str_dba, dim3(qgrid(c->num_cus * 6)), dim3(64), 0, s, jobs, pages, list, ctr,
                       Q(kQueueStrDba), (uint8_t*)c->value_arena.p, offs);
  }
  if (c->timed) hipEventRecord(c->ev[9], s);
  hipLaunchKernelGGL(k_finalize, page_grid, dim3(1024), 0, s, jobs, n, pages);
  if (c->timed) hipEventRecord(c->ev[10], s);
  return hip_ok(hipGetLastError());
}

// What the batch holds (BatchTraits, pqg_ctx.h), from the jobs and the chunks known to have many pages.
static BatchTraits batch_traits(const pqg_ctx* c, const pqg_chunk_job* jobs, int n_jobs) {
  BatchTraits b;
  for (int i = 0; i < n_jobs; i++) {
    const pqg_column_desc& d = jobs[i].col;
    const int width = value_width_of(d);
    if (c->n_locs[(size_t)i] == 0) b.prewalk |= c->many_pages.find(job_key(jobs[i])) == c->many_pages.end();
    b.any_snappy |= d.codec == PQG_CODEC_SNAPPY;
    b.any_gzip |= d.codec == PQG_CODEC_GZIP;
    b.any_zstd |= d.codec == PQG_CODEC_ZSTD;
    b.any_lz4 |= d.codec == PQG_CODEC_LZ4_RAW;
    (d.max_rep == 0 && d.max_def <= 1 ? b.any_w1 : b.any_gen) = true;
    b.any_levels |= d.max_def > 0 || d.max_rep > 0;
    if (d.flags & PQG_COL_KEEP_DICT) {
      // only k_dict_idx takes such a job's pages; a byte-array dictionary still needs k_str_dict
      b.any_keep = true;
      b.any_keep_var |= width == 0;
      b.any_var |= width == 0;
      continue;
    }
    // the strings stage: variable-length columns, and FLBA (DELTA_BYTE_ARRAY pages)
    b.any_var |= width == 0 || d.physical_type == PQG_FIXED_LEN_BYTE_ARRAY;
    b.any_var_out |= width == 0 || d.physical_type == PQG_FIXED_LEN_BYTE_ARRAY;
    // k_values<0>: every fixed-width column but 4-byte ones with only dictionary pages
    b.any_fixed_other |= width != 0;
    b.any_w4 |= width == 4;
  }
  return b;
}

// Submit a batch; `pages`: the located jobs' lists (null: every job is scanned).
static int submit(pqg_ctx* c, const pqg_chunk_job* jobs, const pqg_chunk_pages* pages, int n_jobs) {
  if (!c || (!jobs && n_jobs) || n_jobs < 0) return PQG_ERR_INVALID_ARG;
  hipSetDevice(c->device);
  int64_t total_locs = 0;
  for (int i = 0; pages && i < n_jobs; i++) {
    const pqg_chunk_pages& p = pages[i];
    if (p.n < 0 || (p.n > 0 && !p.locs)) return PQG_ERR_INVALID_ARG;
    int64_t end = 0;  // of the page before
    for (int k = 0; k < p.n; k++) {
      const pqg_page_loc& l = p.locs[k];
      if (l.offset < 0 || l.size <= 0 || l.offset < end || l.offset > jobs[i].data_len - l.size) return PQG_ERR_INVALID_ARG;
      end = l.offset + l.size;
    }
    total_locs += p.n;
  }
  if (total_locs > INT32_MAX / 2) return PQG_ERR_INVALID_ARG;
  for (int i = 0; i < n_jobs; i++) {
    const pqg_column_desc& d = jobs[i].col;
    if (d.max_def < 0 || d.max_def > 255 || d.max_rep < 0 || d.max_rep > 255) return PQG_ERR_INVALID_ARG;
    if (jobs[i].data_len < 0 || jobs[i].total_compressed_size < 0 || (!jobs[i].data && jobs[i].data_len > 0))
      return PQG_ERR_INVALID_ARG;
    if (jobs[i].quirks != 0) return PQG_ERR_INVALID_ARG;  // spec-correct only (quirks: oracle triage mode)
    // BOOLEAN has no dictionary encoding (chunk_reader.go:143-196): nothing to keep
    if ((d.flags & PQG_COL_KEEP_DICT) && d.physical_type == PQG_BOOLEAN) return PQG_ERR_INVALID_ARG;
  }
  c->cur.assign(jobs, jobs + n_jobs);
  c->n_jobs = n_jobs;
  c->launches = 0;
  c->force.assign((size_t)n_jobs, Caps());
  c->h_locs.clear();
  c->loc_base.assign((size_t)n_jobs, 0);
  c->n_locs.assign((size_t)n_jobs, 0);
  for (int i = 0; i < n_jobs; i++) {
    if (pages && pages[i].n > 0) {  // the flat location table, each entry with its job
      c->loc_base[(size_t)i] = (int64_t)c->h_locs.size();
      c->n_locs[(size_t)i] = pages[i].n;
      for (int k = 0; k < pages[i].n; k++) c->h_locs.push_back(LocDev{pages[i].locs[k].offset, pages[i].locs[k].size, i});
      continue;  // no learned capacities: see pqg_ctx.h
    }
    auto it = c->learned.find(job_key(jobs[i]));
    if (it != c->learned.end()) c->force[(size_t)i] = it->second;
  }
  c->batch = batch_traits(c, jobs, n_jobs);
  if (n_jobs == 0) return PQG_OK;
  if (!c->h_locs.empty()) {
    const size_t bytes = sizeof(LocDev) * c->h_locs.size();
    if (c->locs.grow(bytes)) return PQG_ERR_HIP;
    if (copy_sync(c, c->locs.p, c->h_locs.data(), bytes, hipMemcpyHostToDevice)) return PQG_ERR_HIP;
  }
  int e = plan_batch(c);
  if (e) return e;
  return launch_pipeline(c);
}

int pqg_decode_chunks_async(pqg_ctx* c, const pqg_chunk_job* jobs, int n_jobs) { return submit(c, jobs, nullptr, n_jobs); }

int pqg_decode_chunks_located_async(pqg_ctx* c, const pqg_chunk_job* jobs, const pqg_chunk_pages* pages, int n_jobs) {
  if (!pages && n_jobs) return PQG_ERR_INVALID_ARG;
  return submit(c, jobs, pages, n_jobs);
}

int pqg_decode_chunks_located(pqg_ctx* c, const pqg_chunk_job* jobs, const pqg_chunk_pages* pages, int n_jobs,
                              pqg_chunk_result* results) {
  int e = pqg_decode_chunks_located_async(c, jobs, pages, n_jobs);
  if (e) return e;
  return pqg_sync(c, results, n_jobs);
}

// Copy job results back; grow and re-run chunks that ran out of arena space.
int pqg_sync(pqg_ctx* c, pqg_chunk_result* results, int n_jobs) {
  if (!c || n_jobs != c->n_jobs) return PQG_ERR_INVALID_ARG;
  hipSetDevice(c->device);
  const int n = c->n_jobs;
  if (n == 0) return PQG_OK;
  // Every launch is followed by a copy-back and a sync, so the results below
  // never describe a pipeline still in flight; a job still short of space
  // after the last attempt reports PQG_ERR_CAPACITY.
  for (int attempt = 0;; attempt++) {
    if (copy_sync(c, c->h_jobs, c->jobs.p, sizeof(JobDev) * (size_t)n, hipMemcpyDeviceToHost)) return PQG_ERR_HIP;
    bool retry = false;
    for (int i = 0; i < n; i++) {
      const JobDev& d = c->h_jobs[i];
      if (d.status != PQG_ERR_CAPACITY) continue;
      retry = true;
      c->force[(size_t)i] = caps_of(d, true);
      if (d.n_locs == 0) c->learned[job_key(c->cur[(size_t)i])] = c->force[(size_t)i];
    }
    if (!retry || attempt + 1 >= kMaxAttempts) break;
    int e = plan_batch(c);
    if (e) return e;
    e = launch_pipeline(c);
    if (e) return e;
  }
  for (int i = 0; i < n; i++) {
    const JobDev& d = c->h_jobs[i];
    if (d.status != PQG_ERR_CAPACITY && d.scan_fallback != 2 && d.n_locs == 0) {  // neither walked nor stride-walked by the prewalk
      if (c->many_pages.size() >= 65536) c->many_pages.clear();  // bounded: a cache, not a record
      const pqg_chunk_job& in = c->cur[(size_t)i];
      c->many_pages[job_key(in)] = true;
    }
    pqg_chunk_result& r = results[i];
    memset(&r, 0, sizeof(r));
    r.status = d.status;
    r.error_page = d.error_page;
    r.num_pages = d.status == PQG_ERR_CAPACITY ? 0 : d.n_out_pages;
    r.value_width = d.value_width;
    r.col_flags = c->cur[(size_t)i].col.flags;
    r.num_slots = d.num_slots;
    r.num_values = d.num_values;
    r.values_bytes = d.values_bytes;
    r.def_levels = d.max_def > 0 ? (uint8_t*)c->def_arena.p + d.slot_base : nullptr;
    r.rep_levels = d.max_rep > 0 ? (uint8_t*)c->rep_arena.p + d.slot_base : nullptr;
    r.values = (uint8_t*)c->value_arena.p + d.value_base;
    r.offsets = d.value_width == 0 ? (int64_t*)c->offs_arena.p + d.offs_base : nullptr;
  }
  return PQG_OK;
}

int pqg_decode_chunks(pqg_ctx* c, const pqg_chunk_job* jobs, int n_jobs, pqg_chunk_result* results) {
  int e = pqg_decode_chunks_async(c, jobs, n_jobs);
  if (e) return e;
  return pqg_sync(c, results, n_jobs);
}

int pqg_get_dictionary(pqg_ctx* c, int job, pqg_dictionary* out) {
  if (!c || !out || job < 0 || job >= c->n_jobs) return PQG_ERR_INVALID_ARG;
  const JobDev& d = c->h_jobs[job];  // as pqg_sync copied it back
  if (!d.keep_dict) return PQG_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  out->value_width = d.entry_width;
  out->nil_entry = -1;
  out->page = -1;
  if (d.status == PQG_ERR_CAPACITY || d.dict_page < 0) return PQG_OK;
  if (d.entry_width == 0) {
    if (!d.dict_offs || !d.dict_aoffs) return PQG_OK;  // the page's walk failed: no dictionary
    out->page = d.dict_page;
    out->count = d.dict_count;
    out->values = d.dict_chars;
    out->offsets = d.dict_aoffs;
    out->values_bytes = d.dict_chars_len;
    return PQG_OK;
  }
  if (!d.dict_data) return PQG_OK;  // the page's read phase failed
  out->page = d.dict_page;
  out->count = d.dict_count;
  out->values = d.dict_data;
  out->values_bytes = std::min<int64_t>(d.dict_count * d.entry_width, d.dict_len);
  if (d.flags & 1) out->nil_entry = (int32_t)(d.dict_count - 1);  // INT96, Q8
  return PQG_OK;
}

int pqg_get_pages(pqg_ctx* c, int job, pqg_page_info* out, int cap) {
  if (!c || job < 0 || job >= c->n_jobs) return PQG_ERR_INVALID_ARG;
  hipSetDevice(c->device);
  const JobDev& d = c->h_jobs[job];
  int np = std::min<int>(d.n_out_pages, d.page_cap);
  if (d.status == PQG_ERR_CAPACITY) np = 0;
  std::vector<PageDev> tmp((size_t)np);
  if (np > 0 && copy_sync(c, tmp.data(), (PageDev*)c->pages.p + d.page_base, sizeof(PageDev) * (size_t)np, hipMemcpyDeviceToHost))
    return PQG_ERR_HIP;
  int k = 0;
  for (int i = 0; i < np && i < cap; i++, k++) {
    const PageDev& p = tmp[(size_t)i];
    pqg_page_info& o = out[i];
    memset(&o, 0, sizeof(o));
    o.header_offset = p.header_offset;
    o.payload_offset = p.payload_offset;
    o.slot_offset = p.slot_offset;
    o.value_offset = p.value_offset;
    o.page_type = p.page_type;
    o.encoding = p.encoding;
    o.num_values = p.num_values;
    o.not_null = p.not_null;
    o.compressed_size = p.csize;
    o.uncompressed_size = p.usize;
    o.def_len = p.def_len;
    o.rep_len = p.rep_len;
    o.def_encoding = p.def_enc;
    o.rep_encoding = p.rep_enc;
    o.status = p.read_status != PQG_OK ? p.read_status : p.decode_status;
    // bits 8+: why the split snappy decode gave the page up (diagnostics, pqg_snappy.hip)
    o.flags = p.flags | (p.sn_fallback ? PQG_PAGE_FLAG_SNAPPY_SERIAL | (p.sn_fallback << 8) : 0);
  }
  return k;
}

// Diagnostic builds (-DPQG_PROFILE): in-kernel phase cycle counters of the
// values (slots 0-31), levels (slots 32-63), strings (64-95), snappy
// (96-127), dictionary (128-159), inflate (160-191) and BYTE_STREAM_SPLIT
// (192-223, pqg_bss.hip) translation units; read + reset.
int pqg_debug_counters(pqg_ctx* c, uint64_t* out, int cap) {
  if (!c || !out) return PQG_ERR_INVALID_ARG;
#ifdef PQG_PROFILE
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  // a reader per translation unit, 32 slots of `out` each, in the order above
  int (*const readers[])(unsigned long long*) = {prof_read_values, prof_read_levels,  prof_read_strings, prof_read_snappy,
                                                 prof_read_dict,   prof_read_inflate, prof_read_bss};
  constexpr int kUnits = (int)(sizeof(readers) / sizeof(readers[0]));
  unsigned long long v[kUnits][64];
  for (int u = 0; u < kUnits; u++)
    if (readers[u](v[u])) return PQG_ERR_HIP;
  int k = 0;
  for (; k < 32 * kUnits && k < cap; k++) out[k] = v[k / 32][k % 32];
  return k;
#else
  return 0;
#endif
}

int pqg_debug_job(pqg_ctx* c, int job, int64_t* out, int cap) {
  if (!c || !out || job < 0 || job >= c->n_jobs) return PQG_ERR_INVALID_ARG;
  const JobDev& d = c->h_jobs[job];
  const int64_t v[5] = {d.scan_fallback, d.n_cands, d.num_pages, d.need_scratch, c->launches};
  int k = 0;
  for (; k < 5 && k < cap; k++) out[k] = v[k];
  return k;
}

int pqg_set_timing(pqg_ctx* c, int on) {
  if (!c) return PQG_ERR_INVALID_ARG;
  c->timed = on != 0;
  return PQG_OK;
}

int pqg_set_verify_crc(pqg_ctx* c, int on) {
  if (!c) return PQG_ERR_INVALID_ARG;
  c->verify_crc = on != 0;
  return PQG_OK;
}

int pqg_last_crc_ms(pqg_ctx* c, float* ms) {
  if (!c || !ms) return PQG_ERR_INVALID_ARG;
  *ms = 0.f;
  if (c->crc_timed && hipEventElapsedTime(ms, c->ev_crc[0], c->ev_crc[1]) != hipSuccess) *ms = 0.f;
  return PQG_OK;
}

int pqg_get_page_crcs(pqg_ctx* c, int job, pqg_page_crc* out, int cap) {
  if (!c || job < 0 || job >= c->n_jobs || (!out && cap > 0)) return PQG_ERR_INVALID_ARG;
  hipSetDevice(c->device);
  const JobDev& d = c->h_jobs[job];
  int np = std::min<int>(d.n_out_pages, d.page_cap);  // the pages pqg_get_pages reports
  if (d.status == PQG_ERR_CAPACITY) np = 0;
  np = std::min(np, std::max(cap, 0));
  std::vector<crc::Rec> tmp((size_t)std::max(np, 0));
  if (np > 0 && c->crc_ran &&
      copy_sync(c, tmp.data(), (crc::Rec*)c->crc_recs.p + d.page_base, sizeof(crc::Rec) * (size_t)np, hipMemcpyDeviceToHost))
    return PQG_ERR_HIP;
  for (int i = 0; i < np; i++) {
    pqg_page_crc& o = out[i];
    memset(&o, 0, sizeof(o));
    o.state = PQG_CRC_NOT_CHECKED;
    if (!c->crc_ran) continue;
    const crc::Rec& r = tmp[(size_t)i];
    if (r.state == crc::kNoField || r.state == crc::kVerified || r.state == crc::kMismatch) {
      o.state = r.state;
      o.stored = r.stored;
      o.computed = r.computed;
    }
  }
  return np;
}

// the device time of each stage of the last timed launch (ev[i] .. ev[i + 1]); returns how many fit `cap`
static int stage_times(pqg_ctx* c, float* out, int cap) {
  int k = 0;
  for (; k < kStages && k < cap; k++) {
    out[k] = 0;
    hipEventElapsedTime(&out[k], c->ev[k], c->ev[k + 1]);
  }
  return k;
}

int pqg_last_timings(pqg_ctx* c, float* out, int cap) {
  if (!c || !out) return PQG_ERR_INVALID_ARG;
  if (!c->last_timed || cap < 1) return 0;  // the last decode recorded no events: nothing to report
  out[0] = 0;
  hipEventElapsedTime(&out[0], c->ev[0], c->ev[kStages]);
  return 1 + stage_times(c, out + 1, cap - 1);
}

int pqg_bench_decode(pqg_ctx* c, const pqg_chunk_job* jobs, int n_jobs, int iters, float* ms_total, float* ms_stage,
                     int stage_cap) {
  if (!c || iters < 1) return PQG_ERR_INVALID_ARG;
  hipSetDevice(c->device);
  std::vector<pqg_chunk_result> res((size_t)std::max(n_jobs, 1));
  // first call sizes the arenas (and retries on capacity)
  int e = pqg_decode_chunks(c, jobs, n_jobs, res.data());
  if (e) return e;
  // the first call grew the arenas; its capacities are the learned ones now
  for (int i = 0; i < n_jobs; i++) c->force[(size_t)i] = caps_of(c->h_jobs[i], false);
  e = plan_batch(c);
  if (e) return e;
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  hipEventRecord(a, c->stream);
  for (int it = 0; it < iters; it++) {
    e = launch_pipeline(c);
    if (e) break;
  }
  hipEventRecord(b, c->stream);
  hipStreamSynchronize(c->stream);
  float ms = 0;
  hipEventElapsedTime(&ms, a, b);
  if (ms_total) *ms_total = ms / (float)iters;
  if (ms_stage) stage_times(c, ms_stage, stage_cap);
  hipEventDestroy(a);
  hipEventDestroy(b);
  return e;
}

}  // extern "C"
