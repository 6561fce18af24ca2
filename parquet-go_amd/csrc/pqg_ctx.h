// pqg_ctx.h — the context behind include/pqgpu.h's pqg_ctx, shared by the two host files:
// pqg_runtime.hip (the batch pipeline) and pqg_ops.hip (the single-shot entry points).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <vector>

#include "pqgpu.h"
#include "pqg_common.h"

// Which of pqg_lz4.hip's two decoders the runtime launches unless the environment says otherwise: 1, step B
// (k_lz4_batch), the faster one on both shapes measured; 0: step A (k_lz4).
#ifndef PQG_LZ4_BATCH
#define PQG_LZ4_BATCH 1
#endif

namespace pqg {

// A grow-only device buffer; it frees its memory when the context goes.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) hipFree(p);
  }
  int grow(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = std::max(bytes, (size_t)256);
    want = (want + 0xFFFFF) & ~(size_t)0xFFFFF;  // 1 MiB granules
    if (hipMalloc(&p, want) != hipSuccess) {
      p = nullptr;
      return -1;
    }
    cap = want;
    return 0;
  }
};

constexpr int kStages = 10;
// stages timed by pqg_last_timings: scan (K1a-e), list, snappy, setup, walk, levels, nn_scan, values, strings,
// finalize

// Arena capacities of one chunk job (see plan_batch); 0 = use the planner's estimate.
struct Caps {
  int64_t pages = 0, slots = 0, scratch = 0, values = 0, runs = 0, blks = 0, doffs = 0, dchars = 0;
};
// Capacities learned for a chunk (its bytes, size and value count), kept for
// later decodes of the same chunk so a grown arena is planned right away.
// A chunk decoded to keys (PQG_COL_KEEP_DICT) plans other arenas than the same chunk materialised:
// the two learn apart, so neither decode is planned with the other's sizes.
struct JobKey {
  uintptr_t data;
  int64_t tcs, hint;
  int keep;
  bool operator<(const JobKey& o) const {
    return data != o.data ? data < o.data : tcs != o.tcs ? tcs < o.tcs : hint != o.hint ? hint < o.hint : keep < o.keep;
  }
};

// What the in-flight batch holds, worked out once by pqg_decode_chunks_async: plan_batch and launch_pipeline
// neither plan nor launch a stage with no possible work (the host knows each job's codec, type and levels;
// the kernels' own flags stay as the backstop).
struct BatchTraits {
  bool any_var = false;          // variable-length columns
  bool any_fixed_other = false;  // fixed-width columns (k_values<0> pages possible)
  bool any_w4 = false;           // 4-byte columns (the 4-byte dictionary stage: mode 1 pages)
  bool any_levels = false;       // columns with levels (long level runs possible)
  bool any_keep = false;         // keep-dictionary jobs (PQG_COL_KEEP_DICT: k_dict_idx)
  bool any_keep_var = false;     // ... of byte arrays (k_str_dict, then k_dict_export)
  bool any_var_out = false;      // variable-length columns to materialise (the strings stage past k_str_dict)
  bool any_snappy = false, any_gzip = false, any_zstd = false, any_lz4 = false;  // the jobs' codecs
  // jobs with 1-bit levels (maxR = 0, maxD <= 1) for the w = 1 level decoder, others for the general one
  bool any_w1 = false, any_gen = false;
  // some chunk is not known to be left by the K1 prewalk / stride walk (pqg_ctx.many_pages): a batch of only
  // such chunks skips the prewalk launch
  bool prewalk = false;
};

}  // namespace pqg

struct pqg_ctx {
  using DevBuf = pqg::DevBuf;
  int device = 0;
  hipStream_t stream = nullptr;
  int num_cus = 256;
  DevBuf vrecs;          // VRec per page-list entry (k_dict_plan -> k_dict4)
  int dict4_per_cu = 2;  // resident k_dict4 workgroups per CU (LDS-bound), from the occupancy query
  int dict4_threads = 256;
  bool dict4 = true;     // k_dict4 for 4-byte dictionary pages (PQG_DICT4=0: k_values<1>, for A/B runs)
  bool stride = true;     // the K1 stride walk of equal-page chunks (PQG_STRIDE=0: the candidate scan takes them)
  bool dict_big = true;   // k_dict4_big for dictionaries past 4096 entries (PQG_DICT_BIG=0: k_dict4 gathers them)
  bool lev1 = true;       // the whole-page 1-bit level decoder in k_page_levels_w1 (PQG_LEV1=0: the batch decoder alone)
  int seg_waves = 31;     // PQG_SEG_WAVES: k_snap_seg waves per CU (its 5 KiB of LDS allow 31; 16: C4 +10 %)
  int levlong_waves = 28; // PQG_LEVLONG_WAVES: k_level_long waves per CU (66 VGPRs: 7 per SIMD; 8: C5 0.61 ms, 28: 0.32)
  int link_waves = 16;    // PQG_LINK_WAVES: k_snap_link waves per CU (one wave per big page; 4: C4 +50 %)
  int snappy_per_cu = 2;  // resident k_snappy waves per CU (LDS-bound: the output history ring)
  int inflate_per_cu = 8; // resident k_inflate_s waves per CU (LDS / VGPR bound), from the occupancy query
  int zstd_per_cu = 8;    // resident k_zstd waves per CU (LDS-bound: its tables), from the occupancy query
  int lz4_per_cu = 8;     // resident k_lz4 / k_lz4_batch waves per CU, from the occupancy query
  bool lz4_batch = PQG_LZ4_BATCH;  // LZ4_RAW pages by k_lz4_batch (step B), not k_lz4 (step A); PQG_LZ4_BATCH=0/1 in the
                                   // environment overrides the build's choice for a context (tests, tools/lz4_probe.py)
  DevBuf zstd_ws;         // k_zstd: a literal workspace (zstd::kWsBytes) per wave of its grid
  // K1c page checksums (pqg_crc.hip); nothing of it is planned or launched while verify_crc is off
  bool verify_crc = false;  // pqg_set_verify_crc; PQG_VERIFY_CRC=0/1 in the environment sets a context's initial value
  bool crc_ran = false;     // the last decode ran with verification on (pqg_get_page_crcs)
  bool crc_timed = false;   // ... and recorded ev_crc
  int crc_per_cu = 8;       // resident k_page_crc workgroups per CU (LDS-bound: its tables), from the occupancy query
  DevBuf crc_recs, crc_tiles, crc_raws;  // crc::Rec per page-table entry, crc::TileRec / raw register per tile
  int64_t crc_tile_cap = 0;
  int64_t crc_cap_limit = 0;  // PQG_CRC_TILE_CAP (tests): at most this many tile records per region, so that pages find no room
  DevBuf crc_one;           // pqg_crc32: its record, tile table, registers, counter and queue
  DevBuf jobs, pages, list, counters, def_arena, rep_arena, value_arena, scratch;
  DevBuf tile_job;  // K1: tile -> job
  DevBuf tile_count, tile_okc, tile_off, tile_okoff, cand_pos, cands, succ, idx2slot, ok2slot, order;  // K1
  DevBuf streams, runs, blks;  // K3 hybrid run tables
  DevBuf cand_list;
  DevBuf asm_seg;  // K8 per-segment counts + totals
  DevBuf flt_buf;  // K9s: per-segment counts + totals, the literal's bytes, the dictionary-entry bitmap
  float flt_ms = 0.f;    // device time of the last pqg_filter / pqg_select
  bool flt_lds = true;   // entry bitmaps of up to flt::kLdsEntries entries are staged in LDS (PQG_FILTER_LDS=0: read through L2)
  DevBuf conv_buf;       // K10: the count of bad BYTE_ARRAY decimals
  float conv_ms = 0.f;   // device time of the last pqg_convert
  DevBuf offs_arena, doffs_arena;  // K7: value offsets (int64), dictionary record starts
  DevBuf aoffs_arena, dchars_arena;  // K4i: byte-array dictionaries in Arrow layout (k_dict_export): offsets (laid out as
                                     // doffs_arena), chars
  DevBuf page_stage;               // pqg_decode_page: [dictionary page][data page]
  DevBuf blk_src, blk_dst, blk_meta, blk_subs, blk_segpage, blk_F;  // pqg_block_decompress
  DevBuf sn_subs, sn_segpage, sn_F;   // K2 split: sub-block table, segment -> page, segment exits
  int64_t sn_sub_cap = 0, sn_seg_cap = 0;
  DevBuf parts, lev_long, lev_pieces, walk_long;  // big pages: values-stage parts, long level / value-stream runs
  int64_t parts_cap = 0, lev_long_cap = 0, lev_piece_cap = 0, walk_long_cap = 0;
  int64_t total_tiles = 0;
  DevBuf nn_sums, nn_jobs;  // k_nn_scan: block sums [job][block], per-job records
  // grid.y of the per-chunk bookkeeping kernels (pqg_common.h): blocks of kChunkBlock
  // tiles / pages of the batch's largest chunk, the page blocks capped at kChunkBlocks
  int tile_blocks = 1, page_blocks = 1;
  pqg::JobDev* h_jobs = nullptr;  // pinned
  int h_jobs_cap = 0;
  std::vector<pqg_chunk_job> cur;       // jobs of the in-flight batch
  std::vector<pqg::JobDev> plan;        // per-job capacities used
  std::vector<pqg::Caps> force;         // per-job capacities forced for this batch
  std::map<pqg::JobKey, pqg::Caps> learned;  // grown capacities, across calls
  // chunks the K1 prewalk / stride walk did not take (scan_fallback != 2): a batch of only
  // such chunks skips the prewalk launch (performance only: the candidate
  // scan settles any chunk, so a stale entry never changes a result)
  std::map<pqg::JobKey, bool> many_pages;
  pqg::BatchTraits batch;               // the in-flight batch (pqg_decode_chunks_async)
  // located jobs of the in-flight batch (pqg_decode_chunks_located_async): the batch's location table,
  // uploaded once at submit, and each job's entries of it (n_locs 0: the job is scanned).  Such a job
  // neither reads nor feeds `learned` / `many_pages`: their key does not tell a located job from the
  // scanned one of the same chunk, or from another subset of its pages.
  std::vector<pqg::LocDev> h_locs;
  std::vector<int64_t> loc_base;
  std::vector<int32_t> n_locs;
  DevBuf locs;
  int launches = 0;                     // pipeline launches of the last decode
  int n_jobs = 0;
  int64_t list_cap = 0;
  // every event of the context, created and destroyed as one array; the stages' names are views of it
  hipEvent_t events[pqg::kStages + 1 + 4 + 2 + 2 + 4];
  hipEvent_t* const ev = events;                    // [kStages + 1]: the pipeline's stage boundaries
  hipEvent_t* const ev_k8 = ev + pqg::kStages + 1;  // K8: [0,1] assemble / list count, [2,3] list write
  hipEvent_t* const ev_crc = ev_k8 + 4;             // K1c: [0,1] around the checksum kernels
  hipEvent_t* const ev_flt = ev_crc + 2;            // K9s: [0,1] around pqg_filter / pqg_select
  hipEvent_t* const ev_conv = ev_flt + 2;           // K10: [0,1] pqg_convert's count pass, [2,3] its write pass
  float k8_ms = 0.f;     // device time of the last pqg_assemble / pqg_assemble_list
  bool timed = true;
  bool last_timed = false;              // the last pipeline launch recorded the stage events
};

namespace pqg {

inline int hip_ok(hipError_t e) { return e == hipSuccess ? PQG_OK : PQG_ERR_HIP; }

// a copy on the context's stream, waited for
inline int copy_sync(pqg_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (hipMemcpyAsync(dst, src, bytes, kind, c->stream) != hipSuccess) return PQG_ERR_HIP;
  return hip_ok(hipStreamSynchronize(c->stream));
}

// Grid of a queue-driven kernel: shard s of a queue (items s, s + 8, ...) is
// pulled only by blocks with blockIdx & 7 == s (queue_pull, pqg_device.h), so
// every launch needs at least kQShards blocks or a shard's pages are skipped.
inline unsigned qgrid(int64_t blocks) { return (unsigned)std::max<int64_t>(blocks, kQShards); }

inline unsigned zstd_grid(const pqg_ctx* c) { return qgrid((int64_t)c->num_cus * c->zstd_per_cu); }

// K2: the split snappy decode of every compressed page in `list` (pqg_snappy.hip):
// plan -> segment exits -> chain link -> 64 KiB sub-blocks, then the serial
// path for the pages it sent back.  sctr: 2 ints (sub-block / segment totals),
// q_split and q_serial: zeroed sharded queues.  Defined in pqg_runtime.hip.
struct SnapTables {
  SnapSub* subs;
  int sub_cap;
  int* segpage;
  int seg_cap;
  uint2* F;
};
void launch_snappy(pqg_ctx* c, hipStream_t s, JobDev* jobs, PageDev* pages, const int* list, const int* total,
                   int64_t list_cap, int* sctr, int* q_split, int* q_serial, uint8_t* scratch, const SnapTables& T);

}  // namespace pqg
