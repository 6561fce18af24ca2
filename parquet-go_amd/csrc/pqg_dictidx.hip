// pqg_dictidx.hip — K4i: keep-dictionary jobs (PQG_COL_KEEP_DICT): the chunk's values are the
// int32 keys its RLE_DICTIONARY pages store, the dictionary is handed out as it is.
//
//   k_dict_idx     one wave per part of a page of values stage kModeIdx, persistent over a
//                  queue of its own.  The page's index stream goes through hybrid_expand
//                  (pqg_hybrid.h) into an IndexSink: the keys are bound-checked against the
//                  dictionary's entry count, a group at a time, and stored as they are, as
//                  aligned 16-byte non-temporal stores.  No dictionary byte is read.
//   k_dict_export  byte-array dictionaries: k_str_dict's record starts ([len32][bytes] records)
//                  to Arrow layout: offsets[i] = dict_offs[i] - 4 i, chars back to back.
#include <hip/hip_runtime.h>

#include "pqg_common.h"
#include "pqg_kernels.h"
#include "pqg_device.h"
#include "pqg_hybrid.h"

namespace pqg {

// dictDecoder.decodeValues' bound (type_dict.go:39-59, "dict: invalid index" when key >=
// len(values)) without its gather.  A group whose largest key is below the count (one max,
// one ballot: DictSink<4>::prepare) is stored whole; only a group that fails is checked key
// by key, and its valid keys stored one by one.
struct IndexSink {
  gu8 out;          // keys[0] of the page (4-byte aligned)
  int64_t count;    // dictionary entries
  int64_t bad;      // first index with an invalid key
  bool fast = false;
  __device__ __forceinline__ void prepare(const uint32_t (&v)[kGroup][8], const uint32_t (&i0)[kGroup],
                                          const int (&cnt)[kGroup]) {
    uint32_t mx = 0;
#pragma unroll
    for (int b = 0; b < kGroup; b++)
#pragma unroll
      for (int q = 0; q < 8; q++) mx = q < cnt[b] && v[b][q] > mx ? v[b][q] : mx;
    fast = !__ballot((int64_t)mx >= count);
  }
  __device__ __forceinline__ void group(const uint32_t (&v)[kGroup][8], const uint32_t (&i0)[kGroup],
                                        const int (&cnt)[kGroup]) {
#pragma unroll
    for (int b = 0; b < kGroup; b++) {
      if (!__ballot(cnt[b] > 0)) continue;
      if (fast) {
        // aligned 16-byte stores whatever the page's alignment (store_run_aligned)
        const uint32_t v0 = (uint32_t)__builtin_amdgcn_readfirstlane(i0[b]);
        store_run_aligned<8, true>((uintptr_t)(out + (int64_t)v0 * 4), v[b], cnt[b]);
        continue;
      }
      PQG_G uint32_t* o = (PQG_G uint32_t*)(out + (int64_t)i0[b] * 4);
#pragma unroll
      for (int q = 0; q < 8; q++) {
        if (q >= cnt[b]) continue;
        if ((int64_t)v[b][q] < count) o[q] = v[b][q];
        else if ((int64_t)(i0[b] + q) < bad) bad = (int64_t)(i0[b] + q);
      }
    }
  }
};

__global__ void __launch_bounds__(64) k_dict_idx(JobDev* jobs, PageDev* pages, const PartRec* parts, const int* total,
                                                 int* queue, uint8_t* value_arena, const HStream* streams,
                                                 const RunEnt* runs, const BlockDesc* blks) {
  __shared__ __attribute__((aligned(16))) ExpandShared sh;
  const int lane = lane_id();
  if (total[kModePresentOff + kModeIdx] == 0) return;  // no page of this stage
  const int n_items = min(total[kCtrItems], total[kCtrPartsCap]);
  for (;;) {
    const int t = queue_next(queue);
    if (t >= n_items) return;
    // wave-uniform, as in k_values: part, page and job records by scalar loads
    const PartRec pr = parts[t];
    if (pr.vmode != kModeIdx) continue;
    const int pidx = __builtin_amdgcn_readfirstlane(pr.pidx);
    const PageDev pg = pages[pidx];
    if (pg.read_status != kOK || (pg.page_type != 0 && pg.page_type != 3) || pg.vmode != kModeIdx) continue;
    const JobDev job = jobs[pg.job];
    if (job.status == kCAPACITY) continue;
    const bool last = pr.p + 1 >= pr.np;
    const uint32_t nx_v0 = last ? 0u : parts[t + 1].v0;
    const int nx_b0 = last ? -1 : parts[t + 1].b0;
    const gcu8 val = gconst(pg.val);
    const int64_t vn = pg.val_n;
    const int64_t nn = pg.not_null;
    const int64_t v_lo = pr.v0, v_hi = last ? nn : (int64_t)nx_v0;
    // the job's value_width is 4 (the keys); the arena region holds 4 nn bytes (k_nn_scan's check)
    const gu8 out = gmut(value_arena) + job.value_base + pg.value_offset * 4;
    // ---- valuesDecoder.init (read phase; every part finds the same): the width byte
    int re = kOK;
    int dict_w = 0;
    if (vn < 1) re = kEOF;
    else {
      dict_w = val[0];
      if (dict_w > 32) re = kBIT_WIDTH;
    }
    if (re != kOK) {
      if (lane == 0) pages[pidx].read_status = re;
      continue;
    }
    if (pg.decode_status != kOK || nn == 0) continue;
    // ---- decodeValues(val[:nn]) (decode phase), the keys themselves
    // entries: a fixed-width dictionary is published by k_dict_resolve, a byte-array one by
    // k_str_dict after its walk (dict_offs)
    const int64_t dcount = job.entry_width == 0 ? (job.dict_offs ? job.dict_count : 0)
                                                : (job.dict_data ? job.dict_count : 0);
    int de = kOK;
    if (dict_w == 0) {
      // a zero-width decoder yields key 0 forever, reading nothing (hybrid_decoder.go:84-86)
      if (dcount < 1) de = kDICT_INDEX;
      else
        for (int64_t i = v_lo + lane; i < v_hi; i += 64) ((PQG_G uint32_t*)out)[i] = 0u;
    } else {
      const HStream S = streams[pg.hs_val];
      const int serr = (S.status != kOK && S.produced < nn) ? S.status : kOK;
      IndexSink sk{out, dcount, nn};
      hybrid_expand(S, runs, blks, v_hi, sh, sk, pr.b0, nx_b0);
      const int64_t bad = wave_min(sk.bad);
      // a bad key found lies before the stream's end: "dict: invalid index" wins over the
      // stream's own error, exactly as in k_values
      if (bad < nn && (serr == kOK || bad < S.produced)) de = kDICT_INDEX;
      else de = serr;
    }
    if (lane == 0 && de != kOK) atomicMin(&pages[pidx].decode_status, de);
  }
}

// ---- byte-array dictionaries to Arrow layout --------------------------------------------
// grid (jobs, kExportGridY), kExportWaves waves per block (pqg_kernels.h); a wave takes runs of 64 entries
// (one per lane).  Entries of kExportLong bytes or more are copied by the whole wave, one
// after another (wave_copy: aligned 16-byte destination granules out of funnel-shifted
// source granules); the shorter ones by their own lane, as dwords where the destination is
// aligned.  The export publishes dict_chars / dict_aoffs; every source byte lies inside the
// dictionary page (k_str_dict validated each record), every destination byte below
// dict_offs[count] - 4 count <= dict_len <= dchars_cap (k_dict_resolve's check).
constexpr int kExportLong = 64;

__global__ void __launch_bounds__(64 * kExportWaves) k_dict_export(JobDev* jobs, const PageDev* pages,
                                                                  int64_t* aoffs_arena, uint8_t* dchars_arena) {
  JobDev& job = jobs[blockIdx.x];
  if (!job.keep_dict || job.entry_width != 0 || job.status == kCAPACITY || !job.dict_offs || job.dict_page < 0) return;
  const int lane = lane_id();
  const int64_t cnt = job.dict_count;
  const PQG_G int64_t* doffs = gconst(job.dict_offs);
  PQG_G int64_t* ao = gmut(aoffs_arena) + job.doffs_base;
  const gu8 ch = gmut(dchars_arena) + job.dchars_base;
  const gcu8 src = gconst(job.dict_data);
  const int wave = (int)(blockIdx.y * kExportWaves + (threadIdx.x >> 6)), n_waves = (int)gridDim.y * kExportWaves;
  for (int64_t e0 = (int64_t)wave * 64; e0 <= cnt; e0 += (int64_t)n_waves * 64) {
    const int64_t e = e0 + lane;
    const bool have = e < cnt;
    const int64_t rs = doffs[e <= cnt ? e : cnt];          // record start (entry cnt: the end)
    const int64_t re = doffs[have ? e + 1 : cnt];
    if (e <= cnt) ao[e] = rs - 4 * e;
    const int64_t len = have ? re - rs - 4 : 0;
    const int64_t so = rs + 4, dofs = rs - 4 * e;
    uint64_t longs = __ballot(len >= kExportLong);
    if (len > 0 && len < kExportLong) {
      int64_t k = 0;
      const int64_t head = (int64_t)((4 - ((uintptr_t)(ch + dofs) & 3)) & 3);
      for (; k < head && k < len; k++) ch[dofs + k] = src[so + k];
      for (; k + 4 <= len; k += 4) *(PQG_G uint32_t*)(ch + dofs + k) = rd_u32(src + so + k);
      for (; k < len; k++) ch[dofs + k] = src[so + k];
    }
    while (longs) {
      const int l = __ffsll((long long)longs) - 1;
      longs &= longs - 1;
      const int64_t s_l = __shfl(so, l, 64), d_l = __shfl(dofs, l, 64), n_l = __shfl(len, l, 64);
      wave_copy(ch + d_l, src + s_l, n_l);
    }
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    job.dict_chars = (const uint8_t*)(dchars_arena + job.dchars_base);
    job.dict_aoffs = (const int64_t*)(aoffs_arena + job.doffs_base);
    job.dict_chars_len = doffs[cnt] - 4 * cnt;  // the records' bytes less their length words
  }
}

}  // namespace pqg
