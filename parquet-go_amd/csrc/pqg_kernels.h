// pqg_kernels.h — the one declaration of everything launched across translation units.
//
// Every __global__ kernel that another file than its own launches, the host *_launch entries of
// pqg_assemble.hip, pqg_filter.hip and pqg_convert.hip, the profile readers, and the launch-shape constants that a
// kernel and its launch site share.  The launching files (pqg_runtime.hip, pqg_ops.hip) and every
// file that defines one of these include it, so a declaration that drifts from its definition is
// an overload nobody defines and the link (-Wl,-z,defs) fails.
#pragma once
#include <hip/hip_runtime.h>

#include "pqgpu.h"
#include "pqg_common.h"

namespace pqg {

namespace crc { struct Rec; struct TileRec; }         // pqg_crc.h
namespace flt { struct Pred; struct Col; struct Sel; }  // pqg_filter.h

// ---- launch shapes: waves per workgroup in the kernel, threads at the launch
constexpr int kCrcWaves = 4;  // k_page_crc: the waves of a workgroup share one copy of the tables
constexpr int kCrcThreads = 64 * kCrcWaves;
constexpr int kBigWaves = 8;  // k_dict4_big: one workgroup per CU around the LDS dictionary prefix
constexpr int kBigDictThreads = 64 * kBigWaves;
constexpr int kExportWaves = 4;  // k_dict_export: grid (jobs, kExportGridY)
constexpr int kExportThreads = 64 * kExportWaves;
constexpr int kExportGridY = 16;
constexpr int kWalkLanes = kWalkThreads;  // k_hybrid_walk: one lane per stream (pqg_common.h)

// ---- pqg_scan.hip (K1)
__global__ void k_tile_jobs(const JobDev* jobs, int* tile_job);
__global__ void k_page_cands(JobDev* jobs, const int* tile_job, int* tile_count, int* tile_okc, int64_t* cand_pos,
                             int* cand_list, int* cand_total, int region);
__global__ void k_cand_parse(JobDev* jobs, const int* tile_job, const int* cand_list, const int* cand_total, int region,
                             int* tile_okc, const int64_t* cand_pos, Cand* cands);
__global__ void k_tile_scan(JobDev* jobs, const int* tile_count, const int* tile_okc, int* tile_off, int* tile_okoff);
__global__ void k_cand_link(JobDev* jobs, const int* tile_job, int64_t total_tiles, const int* tile_count,
                            const int* tile_off, const int* tile_okoff, const Cand* cands, int* succ, int* idx2slot,
                            int* ok2slot);
__global__ void k_page_chain(JobDev* jobs, PageDev* pages, const Cand* cands, const int* succ, const int* idx2slot,
                             const int* ok2slot, int* order);
__global__ void k_scan_pages(JobDev* jobs, PageDev* pages, int n_jobs, int prewalk, int stride);
// located jobs: one lane per listed page, then their chain (cands: the located region of the candidate table)
__global__ void k_scan_located(JobDev* jobs, const LocDev* locs, int n_locs, Cand* cands);
__global__ void k_chain_located(JobDev* jobs, PageDev* pages, const Cand* cands, int* order);
__global__ void k_page_list(JobDev* jobs, PageDev* pages, int n_jobs, int* list, int list_cap, int* total,
                            int* queues);
// ---- pqg_crc.hip (K1c)
__global__ void k_crc_plan(const JobDev* jobs, const PageDev* pages, const int* list, const int* total, int n_recs,
                           crc::Rec* recs, crc::TileRec* tiles, int tile_cap, int* tile_ctr);
__global__ void k_page_crc(const crc::Rec* recs, const crc::TileRec* tiles, const int* tile_ctr, int tile_cap,
                           int* queue, uint32_t* raws);
__global__ void k_crc_fin(PageDev* pages, const int* list, const int* total, int n_recs, crc::Rec* recs,
                          const uint32_t* raws);
// ---- the decompressors (K2): pqg_snappy.hip, pqg_inflate.hip, pqg_zstd.hip, pqg_lz4.hip
__global__ void k_snap_plan(const JobDev* jobs, PageDev* pages, const int* list, const int* total, int* ctr,
                            SnapSub* subs, int sub_cap, int* seg_page, int seg_cap);
__global__ void k_snap_seg(const JobDev* jobs, const PageDev* pages, const int* seg_page, const int* seg_total,
                           int seg_cap, uint2* F);
__global__ void k_snap_link(const JobDev* jobs, PageDev* pages, const int* list, const int* total, SnapSub* subs,
                            const uint2* F);
__global__ void k_snap_decode(const JobDev* jobs, PageDev* pages, const SnapSub* subs, const int* sub_total,
                              int sub_cap, int* queue, uint8_t* scratch);
__global__ void k_snappy(JobDev* jobs, PageDev* pages, const int* list, const int* total, int* queue,
                         uint8_t* scratch);
__global__ void k_inflate(JobDev* jobs, PageDev* pages, const int* list, const int* total, int* queue,
                          uint8_t* scratch, int mode);
__global__ void k_inflate_s(JobDev* jobs, PageDev* pages, const int* list, const int* total, int* queue,
                            uint8_t* scratch);
__global__ void k_zstd(JobDev* jobs, PageDev* pages, const int* list, const int* total, int* queue, uint8_t* scratch,
                       uint8_t* wspace);
__global__ void k_lz4(JobDev* jobs, PageDev* pages, const int* list, const int* total, int* queue, uint8_t* scratch);
__global__ void k_lz4_batch(JobDev* jobs, PageDev* pages, const int* list, const int* total, int* queue,
                            uint8_t* scratch);
// ---- pqg_levels.hip (K3)
__global__ void k_page_levels(JobDev* jobs, PageDev* pages, const int* list, const int* total, int* queue,
                              uint8_t* scratch, HStream* streams, uint8_t* def_arena, uint8_t* rep_arena,
                              LongLev* longs, int long_cap, LevPiece* pieces, int piece_cap, int split);
__global__ void k_page_levels_w1(JobDev* jobs, PageDev* pages, const int* list, const int* total, int* queue,
                                 uint8_t* scratch, HStream* streams, uint8_t* def_arena, uint8_t* rep_arena,
                                 LongLev* longs, int long_cap, LevPiece* pieces, int piece_cap, int split);
__global__ void k_dict_resolve(JobDev* jobs, int n_jobs, PageDev* pages, uint8_t* scratch);
__global__ void k_level_long(PageDev* pages, const int* ctr, const LongLev* longs, int long_cap,
                             const LevPiece* pieces, int piece_cap, int* queue);
__global__ void k_hybrid_walk(const PageDev* pages, const int* list, const int* total, HStream* streams,
                              RunEnt* runs, BlockDesc* blks, LongWalk* longs, int long_cap);
__global__ void k_walk_long(const int* ctr, const LongWalk* longs, int long_cap, BlockDesc* blks);
__global__ void k_nn_scan_sums(JobDev* jobs, PageDev* pages, uint8_t* scratch, const HStream* streams, NnSums* sums,
                               NnJob* njobs, int* ctr, int64_t parts_cap);
__global__ void k_nn_scan(JobDev* jobs, PageDev* pages, uint8_t* scratch, const HStream* streams, const BlockDesc* blks,
                          int* ctr, PartRec* parts, int64_t parts_cap, const NnSums* sums, const NnJob* njobs);
// ---- the values stages (K4): pqg_values.hip, pqg_bss.hip, pqg_dictidx.hip, pqg_dict.hip
// k_values: instantiated for Mode 0, 1 and 3 at the end of pqg_values.hip, and no other Mode links.  The three
// are not declared `extern template` here: a specialisation declared before the definition is seen does
// not get the definition's Mode-dependent launch bounds (k_values<0> then spills registers).
template <int Mode>
__global__ void k_values(JobDev* jobs, PageDev* pages, const PartRec* parts, const int* total, int* queue,
                         uint8_t* value_arena, const HStream* streams, const RunEnt* runs, const BlockDesc* blks);
__global__ void k_finalize(JobDev* jobs, int n_jobs, const PageDev* pages);
__global__ void k_bss(JobDev* jobs, PageDev* pages, const PartRec* parts, const int* total, int* queue,
                      uint8_t* value_arena);
__global__ void k_dict_idx(JobDev* jobs, PageDev* pages, const PartRec* parts, const int* total, int* queue,
                           uint8_t* value_arena, const HStream* streams, const RunEnt* runs, const BlockDesc* blks);
__global__ void k_dict_export(JobDev* jobs, const PageDev* pages, int64_t* aoffs_arena, uint8_t* dchars_arena);
__global__ void k_dict_plan(JobDev* jobs, PageDev* pages, const PartRec* parts, const int* total,
                            uint8_t* value_arena, const HStream* streams, const RunEnt* runs, const BlockDesc* blks,
                            VRec* recs);
__global__ void k_dict4(PageDev* pages, const int* total, int* queue, const VRec* recs, int big);
__global__ void k_dict4_big(PageDev* pages, const int* total, int* queue, const VRec* recs);
// ---- pqg_strings.hip (K7)
__global__ void k_str_dict(JobDev* jobs, PageDev* pages, int64_t* doffs_arena);
__global__ void k_str_count(JobDev* jobs, PageDev* pages, PartRec* parts, const int* total, int* queue,
                            int64_t* offs_arena, const HStream* streams, const RunEnt* runs, const BlockDesc* blks);
__global__ void k_str_plain(JobDev* jobs, PageDev* pages, const int* list, const int* total, int* queue,
                            int64_t* offs_arena);
__global__ void k_char_scan(JobDev* jobs, PageDev* pages, PartRec* parts, int64_t* offs_arena);
__global__ void k_str_delta(JobDev* jobs, PageDev* pages, const int* list, const int* total, int* queue,
                            int64_t* offs_arena);
__global__ void k_str_dba(JobDev* jobs, PageDev* pages, const int* list, const int* total, int* queue,
                          uint8_t* value_arena, int64_t* offs_arena);
__global__ void k_str_copy(JobDev* jobs, PageDev* pages, const PartRec* parts, const int* total, int* queue,
                           uint8_t* value_arena, int64_t* offs_arena);

// ---- host launchers: pqg_assemble.hip (K8), pqg_filter.hip (K9s) and pqg_convert.hip (K10)
int assemble_launch(hipStream_t s, const pqg_assemble_args* a, int64_t* seg_scratch, int64_t* tot);
int list_count_launch(hipStream_t s, const pqg_list_args* a, int64_t* seg_scratch, int64_t* tot);
int list_write_launch(hipStream_t s, const pqg_list_args* a, int64_t* seg_scratch);
int nested_count_launch(hipStream_t s, const pqg_nested_args* a, int64_t* seg_scratch, int64_t* tot);
int nested_write_launch(hipStream_t s, const pqg_nested_args* a, int64_t* seg_scratch, const int64_t* tot);
int struct_count_launch(hipStream_t s, const pqg_struct_args* a, int64_t* seg_scratch, int64_t* tot);
int struct_write_launch(hipStream_t s, const pqg_struct_args* a, const int64_t* seg_scratch);
int pack_levels_launch(hipStream_t s, const uint8_t* levels, int64_t n, int bw, uint8_t* packed);
int filter_launch(hipStream_t s, const flt::Pred& p, const flt::Col& c, const pqg_dictionary* dict, uint32_t* ebits,
                  uint8_t* bitmap, int64_t n, int mode, bool lds, int64_t* seg, int64_t* tot);
int select_launch(hipStream_t s, const flt::Sel& a, int64_t* seg, int64_t* tot);
int range_bitmap_launch(hipStream_t s, const int64_t* ranges, int n, int64_t num_rows, uint8_t* bitmap);
int convert_count_launch(hipStream_t s, const pqg_convert_args* a, int64_t* tot);
int convert_launch(hipStream_t s, const pqg_convert_args* a);

#ifdef PQG_PROFILE
// read + reset a translation unit's in-kernel phase counters (64 slots each; pqg_debug_counters)
int prof_read_values(unsigned long long* out);
int prof_read_levels(unsigned long long* out);
int prof_read_strings(unsigned long long* out);
int prof_read_snappy(unsigned long long* out);
int prof_read_dict(unsigned long long* out);
int prof_read_inflate(unsigned long long* out);
int prof_read_bss(unsigned long long* out);
#endif

}  // namespace pqg
