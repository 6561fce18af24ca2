// pqg_bss.hip — K6s: values[:notNull] of BYTE_STREAM_SPLIT data pages (encoding 9;
// parquet-format, Encodings, "Byte Stream Split"; no decoder in the reference).
//
//   k_bss   one wave per part of a page (k_part_plan cuts a BSS page like a PLAIN one),
//           persistent over a queue of its own.  A page of nn values of w bytes stores w
//           streams of nn bytes: out[i w + k] = val[k nn + i].  A part [v_lo, v_hi) reads
//           bytes [v_lo, v_hi) of each stream and writes out[v_lo w, v_hi w).
//           w = 2, 4, 8, 16: tiles of 8 KiB; each stream's bytes come in as aligned 16-byte
//           granules, funnel-shifted (the streams are misaligned differently from one
//           another) into an LDS stage where every stream is aligned with the output's
//           granules; each lane then builds whole aligned 16-byte output granules from the
//           stage with byte permutes (pqg_bss.h) and stores them non-temporally, lane L
//           granule L of every KiB.  Every other width: one value per lane, bytewise.
#include <hip/hip_runtime.h>

#include "pqg_bss.h"
#include "pqg_common.h"
#include "pqg_kernels.h"
#include "pqg_device.h"

namespace pqg {

#ifdef PQG_PROFILE
// host reader of this translation unit's phase counters (see pqg_debug_counters):
// 0 part set-up, 1 loads + stage (issue of a tile's loads to its last LDS write),
// 2 transpose (LDS reads + permutes), 3 stores (issue), 4 tiles, 5 parts, 6 whole parts
// of the specialised widths, 7 whole parts of the generic path
int prof_read_bss(unsigned long long* out) {
  unsigned long long z[64] = {0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(pqg_prof), sizeof(z)) != hipSuccess) return -1;
  hipMemcpyToSymbol(HIP_SYMBOL(pqg_prof), z, sizeof(z));
  return 0;
}
#endif

struct LdsStage {
  const PQG_L uint8_t* p;
  __device__ __forceinline__ uint32_t u8(int o) const { return p[o]; }
  __device__ __forceinline__ uint32_t u16(int o) const { return *(const PQG_L uint16_t*)(p + o); }
  __device__ __forceinline__ uint32_t u32(int o) const { return *(const PQG_L uint32_t*)(p + o); }
};

// decoded output: whole granules non-temporal (stg16o), ragged ends as plain dwords / halves
struct GlobalSink {
  __device__ __forceinline__ void st16(uintptr_t a, uint32_t x, uint32_t y, uint32_t z, uint32_t w) const {
    stg16o(a, make_uint4(x, y, z, w));
  }
  __device__ __forceinline__ void st4(uintptr_t a, uint32_t v) const { *(PQG_G uint32_t*)a = v; }
  __device__ __forceinline__ void st2(uintptr_t a, uint32_t v) const { *(PQG_G uint16_t*)a = (uint16_t)v; }
};

// One part of a page of the widths 2, 4, 8, 16.  All 64 lanes active.
template <int W>
__device__ __forceinline__ void bss_part(gcu8 val, int64_t nn, int64_t v_lo, int64_t v_hi, gu8 out, PQG_L uint8_t* st) {
  typedef bss::Part<W> P;
  const int lane = lane_id();
  P pt;
  pt.init((uintptr_t)val, nn, v_lo, v_hi, (uintptr_t)out);
  const LdsStage rd{st};
#ifdef PQG_PROFILE
  uint64_t pf_ld = 0, pf_trs = 0, pf_st = 0, pf_tiles = 0;
#endif
  for (int64_t t0 = 0; t0 < pt.xn; t0 += P::T) {
    PQG_T(ta);
    // half a tile's loads (8 per lane) are issued before its first LDS write
#pragma unroll 1
    for (int h = 0; h < P::NL; h += 4) {
      uint4 A[4], B[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const typename P::Load l = pt.load(t0, lane, h + j);
        A[j] = ldg16(l.base + l.off_a);
        B[j] = ldg16(l.base + l.off_b);
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const typename P::Load l = pt.load(t0, lane, h + j);
        const bss::Q4 o = bss::funnel16(A[j].x, A[j].y, A[j].z, A[j].w, B[j].x, B[j].y, B[j].z, B[j].w, l.s);
        sts16(st + l.st, make_uint4(o.x, o.y, o.z, o.w));
      }
    }
    __builtin_amdgcn_wave_barrier();
    PQG_T(tb);
    const uintptr_t tb_out = pt.out_base(t0);
    uint32_t o_lo, o_hi;
    pt.out_range(t0, &o_lo, &o_hi);
#ifdef PQG_PROFILE
    uint64_t pf_tr = 0;
#endif
#pragma unroll
    for (int j = 0; j < P::NL; j++) {
      PQG_T(tj0);
      uint32_t g[4];
      bss::granule<W>(rd, lane + 64 * j, g);
#ifdef PQG_PROFILE
      if (g[0] == 0x9e3779b9u) __builtin_amdgcn_s_sleep(0);  // the granule is complete before the time is taken
      PQG_T(tj1);
      pf_tr += tj1 - tj0;
#endif
      const uint32_t og = 16u * (uint32_t)(lane + 64 * j);
      bss::store_granule<W>(GlobalSink{}, tb_out + og, og, o_lo, o_hi, g);
    }
    // the next tile's LDS writes come after this tile's reads (one wave: DS operations in order)
    __builtin_amdgcn_wave_barrier();
#ifdef PQG_PROFILE
    PQG_T(td);
    pf_ld += tb - ta;
    pf_trs += pf_tr;
    pf_st += (td - tb) - pf_tr;
    pf_tiles++;
#endif
  }
  // one add per counter and part (an add per tile: the counters' own traffic showed in them)
#ifdef PQG_PROFILE
  PQG_ACC(1, 0, pf_ld);
  PQG_ACC(2, 0, pf_trs);
  PQG_ACC(3, 0, pf_st);
  PQG_ACC(4, 0, pf_tiles);
#endif
}

__global__ void __launch_bounds__(64, 4) k_bss(JobDev* jobs, PageDev* pages, const PartRec* parts, const int* total,
                                               int* queue, uint8_t* value_arena) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[bss::kTileBytes];
  const int lane = lane_id();
  if (total[kModePresentOff + kModeBss] == 0) return;  // no BYTE_STREAM_SPLIT page
  const int n_items = min(total[kCtrItems], total[kCtrPartsCap]);
  PQG_L uint8_t* const st = lds_ptr(stage);
  for (;;) {
    PQG_T(tp0);
    const int t = queue_next(queue);
    if (t >= n_items) return;
    // wave-uniform: part, page and job records are read once, by scalar loads
    const PartRec pr = parts[t];
    if (pr.vmode != kModeBss) continue;
    const int pidx = __builtin_amdgcn_readfirstlane(pr.pidx);
    const PageDev pg = pages[pidx];
    if (pg.read_status != kOK || (pg.page_type != 0 && pg.page_type != 3) || pg.vmode != kModeBss) continue;
    const JobDev job = jobs[pg.job];
    if (job.status == kCAPACITY) continue;
    const bool last = pr.p + 1 >= pr.np;
    const uint32_t nx_v0 = last ? 0u : parts[t + 1].v0;
    const int64_t nn = pg.not_null;
    if (pg.decode_status != kOK || nn == 0) continue;  // no value: nothing is read
    const gcu8 val = gconst(pg.val);
    const int64_t vn = pg.val_n;
    const int w = job.value_width;
    const int64_t v_lo = pr.v0, v_hi = last ? nn : (int64_t)nx_v0;
    const gu8 out = gmut(value_arena) + job.value_base + pg.value_offset * (int64_t)w;
    PQG_T(tpa);
    PQG_ACC(0, tp0, tpa);
    // The streams' stride is the page's notNull, so the value bytes must be exactly
    // nn w (64-bit): fewer is PLAIN's short page, more leaves the stride ambiguous.
    // Checked before any value byte is loaded; every part of a page finds the same.
    int de = kOK;
    const int64_t need = nn * (int64_t)w;
    if (pg.encoding != 9 || w <= 0) de = kUNSUPPORTED;
    else if (vn < need) de = kEOF;
    else if (vn > need) de = kSIZE;
    if (de != kOK) {
      if (lane == 0) atomicMin(&pages[pidx].decode_status, de);
      continue;
    }
    if (v_hi <= v_lo) continue;
    if (w == 4) bss_part<4>(val, nn, v_lo, v_hi, out, st);
    else if (w == 8) bss_part<8>(val, nn, v_lo, v_hi, out, st);
    else if (w == 2) bss_part<2>(val, nn, v_lo, v_hi, out, st);
    else if (w == 16) bss_part<16>(val, nn, v_lo, v_hi, out, st);
    else if (w == 1) wave_copy(out + v_lo, val + v_lo, v_hi - v_lo);
    else {
      // any other width: lane L takes values v_lo + L, + 64, ...; the loads of a stream are
      // consecutive bytes across the lanes
      for (int64_t i = v_lo + lane; i < v_hi; i += 64)
        for (int k = 0; k < w; k++) out[i * w + k] = val[(int64_t)k * nn + i];
    }
    PQG_T(tp1);
    PQG_ACC(w == 2 || w == 4 || w == 8 || w == 16 ? 6 : 7, tpa, tp1);
    PQG_ACC(5, 0, 1);
  }
}

}  // namespace pqg
