// pqg_filter.hip — K9s: row predicates and row selection over decoded flat columns.
//
// pqg_filter evaluates `column op literal` per row into a row bitmap; pqg_select compacts a
// column (def levels, dense values, byte-array offsets and chars) by such a bitmap into the
// chunk-result layout.  What a lane compares, loads and stores is pqg_filter.h (run on the host
// by tools/filter_model.cpp); this file is the wave-level glue, in K8's shape:
//   k_flt_count   one wave per 4096-row segment: the non-null rows (skipped without def levels)
//   k_flt_scan<C> one block: exclusive scan of the C per-segment counters, totals
//   k_flt_dict    kept dictionaries: the comparison once per entry into an entry bitmap
//   k_flt_rows    one wave per segment, 64 rows a round: rank of the valid lanes, load and
//                 compare (or the entry bit of the row's key), ballot, and lanes 0 / 1 combine
//                 and store the two bitmap dwords; a segment owns its dwords, so no atomics
//   k_sel_count   per segment, from the non-null ranks: selected rows, selected non-null rows, their chars
//   k_sel_write   per segment: every selected row's def level, value, rebased offset; chars of
//                 up to 64 bytes by their lane, longer ones by the whole wave (pqg_wavecopy.h)
// All stores are ordinary vector stores.
#include <hip/hip_runtime.h>

#include "pqgpu.h"
#include "pqg_common.h"
#include "pqg_kernels.h"
#include "pqg_device.h"
#include "pqg_filter.h"
#include "pqg_wavecopy.h"

namespace pqg {

using namespace flt;

namespace {

// global-memory IO of pqg_filter.h; LDS: the entry bitmap was staged in `eb`
template <bool LDS>
struct DevIO {
  const PQG_L uint32_t* eb;
  __device__ __forceinline__ uint32_t u8(uintptr_t a) const { return *(const PQG_G uint8_t*)a; }
  __device__ __forceinline__ uint32_t u32(uintptr_t a) const { return *(const PQG_G uint32_t*)a; }
  __device__ __forceinline__ uint64_t u64(uintptr_t a) const { return *(const PQG_G uint64_t*)a; }
  __device__ __forceinline__ void st8(uintptr_t a, uint32_t v) const { *(PQG_G uint8_t*)a = (uint8_t)v; }
  __device__ __forceinline__ void st32(uintptr_t a, uint32_t v) const { *(PQG_G uint32_t*)a = v; }
  __device__ __forceinline__ void st64(uintptr_t a, uint64_t v) const { *(PQG_G uint64_t*)a = v; }
  __device__ __forceinline__ uint32_t eword(uintptr_t base, int64_t j) const {
    return LDS ? eb[j] : ((const PQG_G uint32_t*)base)[j];
  }
};

__device__ __forceinline__ uint64_t lanes_below(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

}  // namespace

__global__ void __launch_bounds__(256) k_flt_count(const uint8_t* def_, int64_t n, int max_def, int64_t nseg,
                                                   int64_t* seg_cnt) {
  const PQG_G uint8_t* def = gconst(def_);
  const int64_t seg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  const int lane = lane_id();
  const int64_t s0 = seg * kSeg, s1 = s0 + kSeg < n ? s0 + kSeg : n;
  int64_t nv = 0;
  for (int64_t b = s0; b < s1; b += 64) {
    const int64_t i = b + lane;
    nv += __popcll(__ballot(i < s1 && def[i] == (uint8_t)max_def));
  }
  if (lane == 0) gmut(seg_cnt)[seg] = nv;
}

// Exclusive scan of the C per-segment counters in place; tot[0..C-1] = totals.  One block,
// 1024 segments a round: a shuffle scan inside each wave, the 16 wave sums through LDS, and a
// carry from round to round (k_nest_scan's shape).
template <int C>
__global__ void __launch_bounds__(1024) k_flt_scan(int64_t* seg_cnt, int64_t nseg, int64_t* tot) {
  __shared__ int64_t wsum[C][16];
  __shared__ int64_t carry[C];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t < C) carry[t] = 0;
  __syncthreads();
  for (int64_t base = 0; base < nseg; base += 1024) {
    const int64_t k = base + t;
    int64_t v[C], inc[C];
#pragma unroll
    for (int j = 0; j < C; j++) {
      v[j] = k < nseg ? seg_cnt[C * k + j] : 0;
      inc[j] = v[j];
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int64_t up = __shfl_up(inc[j], d);
        if (lane >= d) inc[j] += up;
      }
      if (lane == 63) wsum[j][wave] = inc[j];
    }
    __syncthreads();
    if (k < nseg) {
#pragma unroll
      for (int j = 0; j < C; j++) {
        int64_t before = carry[j];
        for (int w = 0; w < wave; w++) before += wsum[j][w];
        seg_cnt[C * k + j] = before + inc[j] - v[j];
      }
    }
    __syncthreads();
    if (t < C) {
      int64_t s = 0;
      for (int w = 0; w < 16; w++) s += wsum[t][w];
      carry[t] += s;
    }
    __syncthreads();
  }
  if (t < C) tot[t] = carry[t];
}

// One lane per dictionary entry; every 64 entries' ballot is two dwords of the entry bitmap
// (4 * ceil(count / 32) bytes), stored by lanes 0 and 1.
__global__ void __launch_bounds__(256) k_flt_dict(Pred p, const uint8_t* values, const int64_t* offsets,
                                                  int64_t values_bytes, int64_t nil_entry, int64_t count,
                                                  uint32_t* ebits) {
  const DevIO<false> io{nullptr};
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = lane_id();
  const bool in = e < count;
  const uint64_t m =
      __ballot(in && entry_pass(io, p, (uintptr_t)values, (uintptr_t)offsets, values_bytes, nil_entry, e));
  const int64_t e0 = e - lane + 32 * lane;  // first entry of this lane's dword
  if (lane < 2 && e0 < count) gmut(ebits)[e0 >> 5] = (uint32_t)(m >> (32 * lane));
}

template <bool LDS>
__global__ void __launch_bounds__(256) k_flt_rows(Pred p, Col c, uint8_t* bitmap, int64_t n, int64_t nseg,
                                                  const int64_t* seg_cnt, int mode, unsigned long long* selected) {
  __shared__ uint32_t eb[LDS ? kLdsEntries / 32 : 1];
  if (LDS) {  // the whole entry bitmap, once per workgroup (4 segments)
    const int64_t words = (c.dict_count + 31) >> 5;
    for (int64_t j = threadIdx.x; j < words; j += 256) eb[j] = ((const PQG_G uint32_t*)c.ebits)[j];
    __syncthreads();
  }
  const DevIO<LDS> io{lds_ptr(&eb[0])};
  const int64_t seg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  const int lane = lane_id();
  const uint64_t lt = lanes_below(lane);
  const int64_t s0 = seg * kSeg, s1 = s0 + kSeg < n ? s0 + kSeg : n;
  int64_t rv = seg_cnt ? gconst(seg_cnt)[seg] : s0;  // non-null rows before this round
  int nsel = 0;
  for (int64_t b = s0; b < s1; b += 64) {
    const int64_t i = b + lane;
    const bool in = i < s1;
    const bool valid = in && row_valid(io, c.def, i, c.max_def);
    const uint64_t mv = __ballot(valid);
    const bool pass = in && row_pass(io, p, c, valid, rv + __popcll(mv & lt));
    const uint64_t mp = __ballot(pass), mi = __ballot(in);
    nsel += store_word(io, (uintptr_t)bitmap, b, n, lane, mp, mi, mode);
    rv += __popcll(mv);
  }
  const int64_t total = wave_sum(nsel);
  if (lane == 0 && total) atomicAdd(selected, (unsigned long long)total);
}

// pqg_select's counters.  seg_v[seg]: non-null rows before the segment (k_flt_count + scan; null
// without def levels: every row is valid).  seg_cnt / tot: [0] selected rows, [1] selected
// non-null rows, [2] their chars (byte arrays).
template <bool VAR>
__global__ void __launch_bounds__(256) k_sel_count(Sel a, int64_t nseg, const int64_t* seg_v, int64_t* seg_cnt) {
  const DevIO<false> io{nullptr};
  const int64_t seg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  const int lane = lane_id();
  const uint64_t lt = lanes_below(lane);
  const int64_t s0 = seg * kSeg, s1 = s0 + kSeg < a.n ? s0 + kSeg : a.n;
  int64_t rv = seg_v ? gconst(seg_v)[seg] : s0;
  int64_t ns = 0, nsv = 0, bytes = 0;
  for (int64_t b = s0; b < s1; b += 64) {
    const int64_t i = b + lane;
    bool sel, valid;
    sel_flags(io, a, i, i < s1, &sel, &valid);
    const uint64_t mv = __ballot(valid);
    const int64_t src = rv + __popcll(mv & lt);
    const bool sv = sel && valid && src < a.num_values;
    if (VAR && sv) {
      int64_t at;
      bytes += sel_len(io, a, src, &at);
    }
    rv += __popcll(mv);
    ns += __popcll(__ballot(sel));
    nsv += __popcll(__ballot(sv));
  }
  if (VAR) bytes = wave_sum(bytes);
  if (lane == 0) {
    PQG_G int64_t* o = gmut(seg_cnt) + 3 * seg;
    o[0] = ns;
    o[1] = nsv;
    o[2] = bytes;
  }
}

template <bool VAR>
__global__ void __launch_bounds__(256) k_sel_write(Sel a, int64_t nseg, const int64_t* seg_v, const int64_t* seg_cnt,
                                                   const int64_t* tot_) {
  const DevIO<false> io{nullptr};
  const int64_t seg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  const int lane = lane_id();
  if (VAR && seg == 0 && lane == 0 && a.out_offsets) {  // the closing offset, from the totals
    const PQG_G int64_t* tot = gconst(tot_);
    io.st64(a.out_offsets + 8 * (uintptr_t)tot[1], (uint64_t)tot[2]);
  }
  const uint64_t lt = lanes_below(lane);
  const int64_t s0 = seg * kSeg, s1 = s0 + kSeg < a.n ? s0 + kSeg : a.n;
  const PQG_G int64_t* sc = gconst(seg_cnt) + 3 * seg;
  int64_t rv = seg_v ? gconst(seg_v)[seg] : s0, rs = sc[0], rsv = sc[1], rc = sc[2];
  WaveCopy wc;
  wc.out = (gu8)a.out_values;
  wc.ln = lane;
  for (int64_t b = s0; b < s1; b += 64) {
    const int64_t i = b + lane;
    bool sel, valid;
    sel_flags(io, a, i, i < s1, &sel, &valid);
    const uint64_t mv = __ballot(valid), ms = __ballot(sel);
    const int64_t src = rv + __popcll(mv & lt);
    const bool sv = sel && valid && src < a.num_values;
    const uint64_t msv = __ballot(sv);
    int64_t at = 0, len = 0, dchar = 0, round_bytes = 0;
    if (VAR) {
      if (sv) len = sel_len(io, a, src, &at);
      dchar = rc + wave_excl_scan_i64(len, &round_bytes);
    }
    sel_store(io, a, i, sel, sv, src, rs + __popcll(ms & lt), rsv + __popcll(msv & lt), dchar, at, len);
    if (VAR && a.out_values) {  // long values, one after another, by the whole wave
      uint64_t ml = __ballot(sv && len > kLongValue);
      while (ml) {
        const int l = __builtin_ctzll(ml);
        ml &= ml - 1;
        const int64_t d = __shfl(dchar, l), s = __shfl(at, l), ln = __shfl(len, l);
        wc.copy<false>((gu8)a.out_values + d, (gcu8)a.values + s, ln);
      }
    }
    rv += __popcll(mv);
    rs += __popcll(ms);
    rsv += __popcll(msv);
    rc += round_bytes;
  }
}

// ---- host launchers (called from pqg_filter / pqg_select in pqg_ops.hip) ------------------------

// seg: nseg int64 (+ tot: [0] non-null rows by the scan, [1] selected rows, zeroed here).  dict:
// the dictionary's device arrays, or null; ebits: 4 * ceil(count / 32) bytes of ctx scratch.
int filter_launch(hipStream_t s, const Pred& p, const Col& c, const pqg_dictionary* dict, uint32_t* ebits,
                  uint8_t* bitmap, int64_t n, int mode, bool lds, int64_t* seg, int64_t* tot) {
  const int64_t nseg = (n + kSeg - 1) / kSeg;
  const unsigned blocks = (unsigned)((nseg + 3) / 4);
  if (nseg == 0) return PQG_OK;
  hipMemsetAsync(tot, 0, 2 * sizeof(int64_t), s);
  const bool ranks = c.def != 0;
  if (ranks) {
    hipLaunchKernelGGL(k_flt_count, dim3(blocks), dim3(256), 0, s, (const uint8_t*)c.def, n, c.max_def, nseg, seg);
    hipLaunchKernelGGL(k_flt_scan<1>, dim3(1), dim3(1024), 0, s, seg, nseg, tot);
  }
  const bool cmp = p.op != OP_IS_NULL && p.op != OP_NOT_NULL;
  if (dict && cmp && dict->count > 0)
    hipLaunchKernelGGL(k_flt_dict, dim3((unsigned)((dict->count + 255) / 256)), dim3(256), 0, s, p, dict->values,
                       dict->offsets, dict->values_bytes, (int64_t)dict->nil_entry, dict->count, ebits);
  unsigned long long* selected = (unsigned long long*)(tot + 1);
  if (dict && cmp && lds && dict->count <= kLdsEntries)
    hipLaunchKernelGGL(k_flt_rows<true>, dim3(blocks), dim3(256), 0, s, p, c, bitmap, n, nseg,
                       ranks ? (const int64_t*)seg : nullptr, mode, selected);
  else
    hipLaunchKernelGGL(k_flt_rows<false>, dim3(blocks), dim3(256), 0, s, p, c, bitmap, n, nseg,
                       ranks ? (const int64_t*)seg : nullptr, mode, selected);
  return hipGetLastError() == hipSuccess ? PQG_OK : PQG_ERR_HIP;
}

// seg: 4 * nseg int64 (the non-null ranks, then the three counters per segment); tot: [0]
// non-null rows, [1..3] k_sel_count's totals.  Counts always; writes when the Sel holds an output.
int select_launch(hipStream_t s, const Sel& a, int64_t* seg, int64_t* tot) {
  const int64_t nseg = (a.n + kSeg - 1) / kSeg;
  const unsigned blocks = (unsigned)((nseg + 3) / 4);
  if (nseg == 0) return PQG_OK;
  const bool var = a.width == 0;
  const int64_t* seg_v = nullptr;
  int64_t* seg3 = seg + nseg;
  if (a.def) {
    hipLaunchKernelGGL(k_flt_count, dim3(blocks), dim3(256), 0, s, (const uint8_t*)a.def, a.n, a.max_def, nseg, seg);
    hipLaunchKernelGGL(k_flt_scan<1>, dim3(1), dim3(1024), 0, s, seg, nseg, tot);
    seg_v = seg;
  }
  if (var)
    hipLaunchKernelGGL(k_sel_count<true>, dim3(blocks), dim3(256), 0, s, a, nseg, seg_v, seg3);
  else
    hipLaunchKernelGGL(k_sel_count<false>, dim3(blocks), dim3(256), 0, s, a, nseg, seg_v, seg3);
  hipLaunchKernelGGL(k_flt_scan<3>, dim3(1), dim3(1024), 0, s, seg3, nseg, tot + 1);
  if (a.out_def || a.out_values || a.out_offsets) {
    if (var)
      hipLaunchKernelGGL(k_sel_write<true>, dim3(blocks), dim3(256), 0, s, a, nseg, seg_v, (const int64_t*)seg3,
                         (const int64_t*)(tot + 1));
    else
      hipLaunchKernelGGL(k_sel_write<false>, dim3(blocks), dim3(256), 0, s, a, nseg, seg_v, (const int64_t*)seg3,
                         (const int64_t*)(tot + 1));
  }
  return hipGetLastError() == hipSuccess ? PQG_OK : PQG_ERR_HIP;
}

// ---- row ranges -> row bitmap (pqg_range_bitmap) ---------------------------------
// One lane per bitmap dword (rows [32 d, 32 d + 32)): a binary search over the ascending, disjoint
// ranges finds the first one that ends past the dword's first row, and the ranges from there on that
// start before its end set their bits.  Every dword is written whole, so bits at and past num_rows
// (no range holds them) are zero.
__global__ void __launch_bounds__(256) k_range_bitmap(const int64_t* ranges, int n, int64_t ndw, uint32_t* bitmap) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= ndw) return;
  const PQG_G int64_t* r = gconst(ranges);
  const int64_t r0 = d * 32, r1 = r0 + 32;
  int lo = 0, hi = n;  // first range with hi > r0
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (r[2 * mid + 1] > r0) hi = mid; else lo = mid + 1;
  }
  uint32_t bits = 0;
  for (int k = lo; k < n; k++) {
    const int64_t a = r[2 * k], b = r[2 * k + 1];
    if (a >= r1) break;
    const int x = (int)((a > r0 ? a : r0) - r0), y = (int)((b < r1 ? b : r1) - r0);  // bits [x, y), 0 <= x, y <= 32
    if (y > x) bits |= (y - x == 32 ? 0xffffffffu : ((1u << (y - x)) - 1u) << x);
  }
  ((PQG_G uint32_t*)bitmap)[d] = bits;
}

// ranges: n pairs [lo, hi) on the device, ascending and disjoint within [0, num_rows]
int range_bitmap_launch(hipStream_t s, const int64_t* ranges, int n, int64_t num_rows, uint8_t* bitmap) {
  const int64_t ndw = (num_rows + 31) / 32;
  if (ndw == 0) return PQG_OK;
  hipLaunchKernelGGL(k_range_bitmap, dim3((unsigned)((ndw + 255) / 256)), dim3(256), 0, s, ranges, n, ndw, (uint32_t*)bitmap);
  return hipGetLastError() == hipSuccess ? PQG_OK : PQG_ERR_HIP;
}

}  // namespace pqg
