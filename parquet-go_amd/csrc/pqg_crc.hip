// pqg_crc.hip — K1c: PageHeader.crc (field 4), verified on the GPU before any decoder reads
// the page (parquet-format, "Checksumming": CRC-32 as in gzip over the page's
// compressed_page_size bytes as stored; no such check in the reference).  Launched only
// when verification is on (pqg_set_verify_crc) or by pqg_crc32.
//
//   k_crc_plan   one wave per listed page: walks the top-level fields of the page's header
//                bytes [header_offset, payload_offset) again for field 4 of type i32 (the
//                scan's parser reads and drops it: its records have no room for it), writes
//                the page's crc::Rec and reserves the page's tile records.
//   k_page_crc   one wave per tile of crc::kTile bytes, persistent over a queue of its own, four
//                waves to a workgroup:
//                lane L takes granules L, L + 64, ... straight from its loads with the
//                1008-byte gap folded into the table step (pqg_crc.h), 20 tables of 1 KiB
//                in LDS built in the prologue.  One raw register per tile.
//   k_crc_fin    one wave per page: combines the page's tile registers, compares with the
//                stored value, writes state / computed and, on a mismatch, the page's
//                read_status = kCRC, so every later stage skips the page and k_finalize
//                ranks it with the read-phase errors.
#include <hip/hip_runtime.h>

#include "pqg_common.h"
#include "pqg_kernels.h"
#include "pqg_crc.h"
#include "pqg_device.h"
#include "pqg_thrift.h"

namespace pqg {

namespace {

struct HdrSrc {
  Window w;  // by value: the parser state stays in registers
  __device__ __forceinline__ int get(int64_t i) { return w.get(i); }
};

struct PlanShared {
  uint8_t win[kWin];
  SkipFrame frames[kMaxFrames];
  int16_t last[kMaxLast];
};

struct LdsTab {
  PQG_L uint32_t* t;
  __device__ __forceinline__ uint32_t get(int i) const { return t[i]; }
  __device__ __forceinline__ void put(int i, uint32_t v) const { t[i] = v; }
};

struct GlobalLd {
  __device__ __forceinline__ crc::Q4 operator()(uintptr_t a) const {
    const uint4 v = ldg16(a);
    return crc::Q4{v.x, v.y, v.z, v.w};
  }
};

// the tables, built by the whole workgroup for all of its kCrcWaves waves (pqg_kernels.h); every thread of the
// block calls it
__device__ __forceinline__ void build_tables_block(const LdsTab& tb) {
  for (int r = 0; r < crc::kTabs; r++) {
    crc::build_round(tb, (int)threadIdx.x, r, 64 * kCrcWaves);
    __syncthreads();
  }
}

// xor over the wave: DPP row_shr 1/2/4/8, row_bcast 15/31 (as wave_incl_scan_u64), lane 63 holds it
__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#define PQG_XOR_STEP(ctrl, rm, bc) v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rm, 0xf, bc);
  PQG_XOR_STEP(0x111, 0xf, true) PQG_XOR_STEP(0x112, 0xf, true) PQG_XOR_STEP(0x114, 0xf, true)
  PQG_XOR_STEP(0x118, 0xf, true) PQG_XOR_STEP(0x142, 0xa, false) PQG_XOR_STEP(0x143, 0xc, false)
#undef PQG_XOR_STEP
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// raw register of tile t of [p, p + n); all 64 lanes active
__device__ __forceinline__ uint32_t tile_raw(uintptr_t p, int64_t n, int64_t t, const LdsTab& tb, uint32_t mul) {
  crc::Tile tl;
  tl.init(p, n, t);
  const uint32_t c = crc::lane_tile(tl, lane_id(), GlobalLd{}, tb);
  const uint32_t r = wave_xor(multmodp(c, mul));
  return crc::tile_tail(tl, r, GlobalLd{}, tb);
}

}  // namespace

// pages != nullptr: the listed pages of a decode (recs indexed like the page table).
// pages == nullptr: recs[0, n_recs) come filled by the host (p, n, state = kPending).
__global__ void __launch_bounds__(64) k_crc_plan(const JobDev* jobs, const PageDev* pages, const int* list,
                                                 const int* total, int n_recs, crc::Rec* recs, crc::TileRec* tiles,
                                                 int tile_cap, int* tile_ctr) {
  __shared__ __attribute__((aligned(16))) PlanShared sh;
  const int lane = lane_id();
  const int n_items = pages ? *total : n_recs;
  for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
    const int ridx = pages ? __builtin_amdgcn_readfirstlane(list[it]) : it;
    crc::Rec rc;
    if (pages) {
      const PageDev& pg = pages[ridx];
      const JobDev& job = jobs[pg.job];
      rc.p = job.data + pg.payload_offset;
      rc.n = pg.csize;
      rc.tile_base = 0;
      rc.ntiles = 0;
      rc.state = crc::kNotChecked;
      rc.stored = rc.computed = 0;
      // a page whose own read phase failed keeps that status: its bytes may not be there
      if (pg.read_status == kOK && pg.csize >= 0 && pg.payload_offset >= pg.header_offset &&
          pg.payload_offset + (int64_t)pg.csize <= job.data_len) {
        // the header parsed (read_page_header) and ends at payload_offset: a walk over its
        // top-level fields with the same reader, every other field skipped
        Compact<HdrSrc> c;
        c.src.w = Window{gconst(job.data), pg.payload_offset, kFarAway, lds_ptr(sh.win)};
        c.pos = pg.header_offset;
        c.frames = sh.frames;
        c.last = sh.last;
        c.nlast = 0;
        c.last_id = 0;
        c.bool_set = c.bool_val = false;
        bool present = false;
        uint32_t stored = 0;
        if (c.struct_begin() == 0) {
          for (;;) {
            int t, id;
            if (c.field_begin(&t, &id) || t == T_STOP) break;
            if (id == 4 && t == T_I32) {
              int32_t v;
              if (c.i32(&v)) break;
              stored = (uint32_t)v;  // twice: the last one read, as the parser's slots
              present = true;
            } else if (c.skip(t, 64)) {
              break;
            }
          }
        }
        rc.stored = stored;
        rc.state = present ? crc::kPending : crc::kNoField;
        __builtin_amdgcn_wave_barrier();  // the next page's window fill comes after this page's reads
      }
    } else {
      rc = recs[ridx];
    }
    if (rc.state == crc::kPending) {
      const int64_t nt = crc::num_tiles((uintptr_t)rc.p, rc.n);
      // the counters are sharded like the queues (one word takes ~88 atomics a microsecond: 2 500 pages
      // were 28 us): block b reserves in region b & 7 of the tile table, tile_cap records each
      const int shard = (int)(blockIdx.x & (kQShards - 1));
      int base = tile_cap;
      if (lane == 0 && nt > 0 && nt <= tile_cap) base = atomicAdd(tile_ctr + shard * kQStride, (int)nt);
      base = __builtin_amdgcn_readfirstlane(base);
      const int64_t g0 = (int64_t)shard * tile_cap;
      if (nt > 0 && (base < 0 || (int64_t)base + nt > tile_cap)) {
        // no room (the counter may pass the capacity: consumers read min(counter, cap)): the
        // slots reserved below the capacity are marked empty, k_crc_fin reads the page itself
        rc.ntiles = -1;
        if (base >= 0)
          for (int64_t t = (int64_t)base + lane; t < tile_cap; t += 64) tiles[g0 + t] = crc::TileRec{-1, -1};
      } else {
        rc.tile_base = g0 + base;
        rc.ntiles = (int32_t)nt;
        for (int64_t t = lane; t < nt; t += 64) tiles[g0 + base + t] = crc::TileRec{ridx, (int32_t)t};
      }
    }
    if (lane == 0) recs[ridx] = rc;
  }
}

// Workgroups of kCrcWaves waves share one copy of the tables (20 KiB: 8 workgroups, 32 waves a CU;
// a wave with tables of its own leaves a CU 8 waves, too few to cover the table reads' latency);
// after the build every wave pulls tiles on its own.
__global__ void __launch_bounds__(64 * kCrcWaves) k_page_crc(const crc::Rec* recs, const crc::TileRec* tiles, const int* tile_ctr,
                                                    int tile_cap, int* queue, uint32_t* raws) {
  __shared__ __attribute__((aligned(16))) uint32_t tabs[crc::kTabs * 256];
  // the records reserved in each region of the tile table (k_crc_plan), as one list
  int n_s[kQShards], n_items = 0;
#pragma unroll
  for (int k = 0; k < kQShards; k++) {
    n_s[k] = max(0, min(tile_ctr[k * kQStride], tile_cap));
    n_items += n_s[k];
  }
  if (n_items <= 0) return;
  const LdsTab tb{lds_ptr(tabs)};
  build_tables_block(tb);
  const uint32_t mul = crc::lane_mul(lane_id());
  for (;;) {
    const int q = queue_next(queue);
    if (q >= n_items) return;
    int idx = q, shard = 0;
#pragma unroll
    for (int k = 0; k < kQShards - 1; k++)
      if (shard == k && idx >= n_s[k]) {
        idx -= n_s[k];
        shard = k + 1;
      }
    const int64_t g = (int64_t)shard * tile_cap + idx;
    // wave-uniform: the records are read once, by scalar loads
    const crc::TileRec tr = tiles[g];
    if (tr.rec < 0) continue;  // a reservation that ran past its region: k_crc_fin reads that page itself
    const crc::Rec rc = recs[tr.rec];
    if (rc.state != crc::kPending || tr.t < 0 || tr.t >= rc.ntiles || rc.tile_base + tr.t != g) continue;
    const uint32_t r = tile_raw((uintptr_t)rc.p, rc.n, tr.t, tb, mul);
    if (lane_id() == 0) raws[g] = r;
  }
}

__global__ void __launch_bounds__(64) k_crc_fin(PageDev* pages, const int* list, const int* total, int n_recs,
                                                crc::Rec* recs, const uint32_t* raws) {
  const int lane = lane_id();
  const int n_items = pages ? *total : n_recs;
  for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
    const int ridx = pages ? __builtin_amdgcn_readfirstlane(list[it]) : it;
    const crc::Rec rc = recs[ridx];
    if (rc.state != crc::kPending) continue;
    uint32_t x;
    if (rc.ntiles >= 0) {
      const PQG_G uint32_t* rw = gconst(raws) + rc.tile_base;
      x = crc::lane_combine((uintptr_t)rc.p, rc.n, rc.ntiles, lane, [&](int64_t t) { return rw[t]; });
    } else {
      const gcu8 p = gconst(rc.p);  // no tile records for the page
      x = crc::lane_slice(rc.n, lane, [&](int64_t i) { return (uint32_t)p[i]; });
    }
    const uint32_t got = ~wave_xor(x);
    if (lane == 0) {
      const bool ok = got == rc.stored;
      recs[ridx].computed = got;
      recs[ridx].state = ok ? crc::kVerified : crc::kMismatch;
      if (pages && !ok) pages[ridx].read_status = kCRC;
    }
  }
}

}  // namespace pqg
