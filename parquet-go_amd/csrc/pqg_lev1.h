// pqg_lev1.h — the whole-page decoder for 1-bit level streams (maxLevel 1:
// optional flat columns, the C2 shape), used by k_page_levels_w1.
//
// The page's def stream (<= kL1MaxN bytes) is staged in LDS with one round of
// loads and decoded with no per-batch loop:
//   1. backward exit table: lane l owns stream positions [l S, l S + S) (S =
//      ceil(n / 64) <= 64, a multiple of 4) and walks them from the last to
//      the first, parsing a run header at every position
//      (hybridDecoder.readRunHeader, hybrid_decoder.go:143-166; RLE value /
//      bit-packed extent :116-141).  Position p's exit — the first header
//      position at or past the segment's end on the chain from p — is the
//      successor's exit when the successor is inside the segment (already
//      known: headers are >= 2 bytes apart), else the successor itself.  One
//      byte per position (offset past the segment's end, "far", or "bad": an
//      error on the way).  Four positions a step, one per byte lane of a
//      dword (l1_quad, pqg_lev1_parse.h): headers of one and two bytes are
//      settled there, every other one is "far"; the positions next to the
//      stream's end, where the checks against it matter, are parsed one at a
//      time with the byte-wise l1_hdr;
//   2. link: the true chain's entry into every segment, 64 dependent table
//      reads (entry(l + 1) = exit(entry(l)) from position 0); a "far" exit is
//      walked header by header with l1_hdr;
//   3. each lane walks its segment's part of the chain twice: the value count
//      (a saturating wave scan gives every lane its first value), then the
//      bits, appended word by word to an LDS bitmap of the page's values in
//      one loop over the lane's words (a step places up to 32 values of the
//      current run and moves on to the next run when that one is used up);
//   4. the wave expands the bitmap 16 values per lane (nibble x 0x00204081)
//      into aligned 16-byte stores of level bytes and counts notNull.
// No global store happens before every check has passed; a page this path
// does not take (longer stream, more values, an error or a 5+ byte header on
// the chain, a chain short of the page's values, a short bit-packed read) is
// decoded by the exact batch decoder (pqg_levdec.h), which reports the
// reference's error (hybridDecoder.next, hybrid_decoder.go:82-114).
#pragma once
#include "pqg_levdec.h"
#include "pqg_lev1_parse.h"

namespace pqg {

constexpr int kL1MaxN = 4096;               // stream bytes
constexpr int kL1MaxCount = 32768 - 16;     // values (+ <= 15 alignment bits: a 4 KiB bitmap)
constexpr int kL1Win = kL1MaxN + 64;        // window: 15 alignment bytes, the stream, zeros for reads past n

struct Lev1Shared {
  uint8_t win[kL1Win];
  uint32_t tab[kL1MaxN / 4 + 2];  // exit codes (one byte per position), then the value bitmap
};

__device__ __forceinline__ L1Hdr l1_parse(const PQG_L uint8_t* win, uint32_t mis, uint32_t q, uint32_t n) {
  const uint32_t wo = mis + q;
  const PQG_L uint32_t* d = (const PQG_L uint32_t*)(win + (wo & ~3u));
  const uint32_t a = d[0], b = d[1], c = d[2];
  const uint32_t sft = (wo & 3) * 8;
  return l1_hdr(__builtin_amdgcn_alignbit(b, a, sft), __builtin_amdgcn_alignbit(c, b, sft), q, n);
}
// A header on the chain (checked by the table walk: <= 4 bytes, no error):
// the fields the value walks need, without the checks.
struct L1Run {
  uint32_t hl, g, vb;  // header bytes, h >> 1, the byte after the header
  bool bp;
};
__device__ __forceinline__ L1Run l1_run(const PQG_L uint8_t* win, uint32_t mis, uint32_t q) {
  const uint32_t wo = mis + q;
  const PQG_L uint32_t* d = (const PQG_L uint32_t*)(win + (wo & ~3u));
  const uint32_t a = d[0], b = d[1], c = d[2];
  const uint32_t sft = (wo & 3) * 8;
  const uint32_t lo = __builtin_amdgcn_alignbit(b, a, sft), hi = __builtin_amdgcn_alignbit(c, b, sft);
  const uint32_t cont = ~lo & 0x80808080u;
  L1Run r;
  r.hl = (cont ? (uint32_t)__builtin_ctz(cont) >> 3 : 3u) + 1;
  const uint32_t hf = (lo & 0x7f) | ((lo >> 1) & 0x3f80) | ((lo >> 2) & 0x1fc000) | ((lo >> 3) & 0xfe00000);
  const uint32_t h = __builtin_amdgcn_ubfe(hf, 0, 7 * r.hl);
  r.g = h >> 1;
  r.bp = (h & 1) != 0;
  r.vb = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * r.hl)) & 0xff;
  return r;
}

// the exit code of a header whose successor lies at or past the segment's end e
__device__ __forceinline__ uint32_t l1_code(const L1Hdr& h, uint32_t e) {
  const uint32_t d = h.nx - e;
  return h.bad ? kL1Bad : (d < kL1Far ? d : kL1Far);
}

// Decode `count` 1-bit levels of stream [p, p + n) into out[0, count) and
// count the ones (notNull for maxLevel 1).  false: not taken (nothing stored;
// the caller runs the exact decoder).
__device__ __forceinline__ bool lev1_page(gcu8 p, uint32_t n, uint32_t count, gu8 out, Lev1Shared& sh, uint32_t* nn_out) {
  const int lane = lane_id();
  if (n == 0 || n > (uint32_t)kL1MaxN || count > (uint32_t)kL1MaxCount) return false;
  PQG_L uint8_t* win = lds_ptr(sh.win);
  PQG_T(t0);
  // ---- 0. stage the stream: 16-byte granules from the aligned base; bytes
  // past the stream read as zero.  Every load is issued (clamped to the base:
  // a guarded load is waited for inside its branch), then masked and stored.
  const uintptr_t pa = (uintptr_t)p;
  const uint32_t mis = (uint32_t)(pa & 15);
  const uintptr_t base = pa - mis;
  const uint32_t lim = mis + n;
  constexpr int kR = (kL1Win + 1023) / 1024;  // 5 rounds of 1 KiB
  uint4 v[kR];
#pragma unroll
  for (int h = 0; h < kR; h++) {
    const uint32_t g = 1024u * h + 16u * lane;
    v[h] = ldg16(g < lim ? base + g : base);
  }
#pragma unroll
  for (int h = 0; h < kR; h++) {
    const uint32_t g = 1024u * h + 16u * lane;
    if (g < (uint32_t)kL1Win) sts16(win + g, g < lim ? mask_tail(v[h], g, lim) : make_uint4(0, 0, 0, 0));
  }
  __builtin_amdgcn_wave_barrier();
  PQG_T(t1);
  PQG_ACC(20, t0, t1);
  // ---- 1. exit codes, each lane over its segment from the end
  PQG_L uint8_t* T = (PQG_L uint8_t*)lds_ptr(sh.tab);
  const uint32_t S = (((n + 63) >> 6) + 3) & ~3u;  // a multiple of 4, <= 64
  const uint32_t a = (uint32_t)lane * S;
  const uint32_t e = a + S < n ? a + S : n;
  // the top (e - a) % 4 positions one at a time with the exact parse, and
  // with them the group that holds positions >= n - 3 (the checks against the
  // stream's end and reads of the padding concern those alone); then groups
  // of four with the bytewise parse.
  int q = (int)e - 1;
  const uint32_t len = e > a ? e - a : 0u;
  uint32_t top = len & 3;
  if (e - top + 3 > n) top += 4;  // a position >= n - 3 below them
  top = top < len ? top : len;
  for (int r = (int)top; r > 0; r--, q--) {
    const L1Hdr h = l1_parse(win, mis, (uint32_t)q, n);
    uint32_t code = l1_code(h, e);
    if (!h.bad && h.nx < e) code = T[h.nx];
    T[q] = (uint8_t)code;
  }
  // Four positions from one 12-byte read: l1_quad settles headers of one and
  // two bytes and calls the rest "far", the code that already sends the link
  // (2.) down the chain with the exact parse.  Calling a position far is
  // therefore always correct (a far position passes its code to every
  // position that leads to it: the link then walks that segment header by
  // header) and costs time only on the true chain.  The codes are selected
  // bytewise as well; the successors' codes are read together (a header's
  // successor is >= 2 positions on: the group's two upper codes are forwarded
  // to its two lower positions in registers).
  for (; q >= (int)a + 3; q -= 4) {
    const uint32_t q0 = (uint32_t)q - 3;  // positions q0 .. q0 + 3
    const uint32_t wo = mis + q0;
    const PQG_L uint32_t* d = (const PQG_L uint32_t*)(win + (wo & ~3u));
    const uint32_t d0 = d[0], d1 = d[1], d2 = d[2];
    const uint32_t sft = (wo & 3) * 8;
    const uint32_t b0 = __builtin_amdgcn_alignbit(d1, d0, sft), b4 = __builtin_amdgcn_alignbit(d2, d1, sft);
    const L1Quad h = l1_quad(b0, __builtin_amdgcn_alignbit(b4, b0, 8), __builtin_amdgcn_alignbit(b4, b0, 16));
    const L1Codes cd = l1_quad_codes(h, e - q0);
    const uint32_t in7 = cd.in, code = cd.code;
    const uint32_t inm = in7 | (in7 - (in7 >> 7));
    uint32_t nx[4], t[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      nx[j] = q0 + j + ((h.len >> (8 * j)) & 0xff);
      t[j] = T[(in7 >> (8 * j + 7)) & 1 ? nx[j] : q0 + 3];  // unconditional (clamped) read
    }
    // successors inside the group come from registers (q0 + 2 / q0 + 3: written below)
    const uint32_t up = (code & ~inm) | ((t[2] << 16 | t[3] << 24) & inm);  // successor >= q0 + 4
    const uint32_t c3 = up >> 24, c2 = (up >> 16) & 0xff;
    const uint32_t t1 = nx[1] == q0 + 3 ? c3 : t[1];
    const uint32_t t0 = nx[0] == q0 + 3 ? c3 : nx[0] == q0 + 2 ? c2 : t[0];
    *(PQG_L uint32_t*)(T + q0) = up | ((t0 | t1 << 8) & inm);  // q0 = a + 4k: aligned
  }
  __builtin_amdgcn_wave_barrier();
  PQG_T(t2);
  PQG_ACC(21, t1, t2);
  // ---- 2. the chain's entry into every segment
  uint32_t E = 0, myE = 0;
  bool ok = true;
  for (int l = 0; l < 64; l++) {
    const uint32_t al = (uint32_t)l * S;
    if (lane == l) myE = E;
    if (al >= n) continue;
    const uint32_t el = al + S < n ? al + S : n;
    if (E >= el) continue;  // a bit-packed payload covers the segment
    const uint32_t code = (uint32_t)__builtin_amdgcn_readfirstlane((int)T[E]);
    if (code == kL1Bad) { ok = false; break; }
    if (code == kL1Far) {  // an exit past the table's reach: walk it
      uint32_t q = E;
      while (q < el) {
        const L1Hdr h = l1_parse(win, mis, q, n);
        if (h.bad) { ok = false; break; }
        q = (uint32_t)__builtin_amdgcn_readfirstlane((int)h.nx);
      }
      if (!ok) break;
      E = q;
    } else {
      E = el + code;
    }
  }
  PQG_T(t3);
  PQG_ACC(22, t2, t3);
  if (!ok) { PQG_ACC(27, 0, 1); return false; }
#ifdef PQG_L1_STOP_AFTER_LINK  // timing experiment only (wrong outputs)
  *nn_out = 0;
  return true;
#endif
  // ---- 3a. values per segment and the segment's chain positions (bit q - a)
  uint32_t C = 0;
  uint64_t cm = 0;
  for (uint32_t q = myE; q < e;) {
    const L1Run r = l1_run(win, mis, q);
    const uint32_t cnt = r.bp ? r.g * 8 : r.g;
    C = C + cnt < (1u << 24) ? C + cnt : (1u << 24);  // > any page count: the scan cannot wrap
    cm |= 1ull << (q - a);
    q += r.hl + (r.bp ? r.g : 1u);
  }
  const uint32_t incl = ldpp_incl_add_sat(C);
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  if (total < count) return false;  // the stream ends early: EOF (the exact decoder reports where)
  const uint32_t B = incl - C;
  PQG_T(t4);
  PQG_ACC(23, t3, t4);
  // ---- 3b. the bits: bitmap bit pre + i = value i.  Each lane appends its
  // runs' bits to a word accumulator in value order; its whole words are
  // plain stores, its first and last (shared with the neighbouring lanes)
  // atomic ORs.  The runs come from the chain mask, so their header reads do
  // not wait for one another.
  const uintptr_t oa = (uintptr_t)out;
  const uintptr_t a0 = oa & ~(uintptr_t)15;
  const uint32_t pre = (uint32_t)(oa - a0);
  const uint32_t end = pre + count;
  PQG_L uint32_t* bm = lds_ptr(sh.tab);
  const uint32_t nw = (end + 31) >> 5;
  __builtin_amdgcn_wave_barrier();
  for (uint32_t k = (uint32_t)lane; k <= nw; k += 64) bm[k] = 0u;
  __builtin_amdgcn_wave_barrier();
  const PQG_L uint32_t* W = (const PQG_L uint32_t*)win;
  bool fail = false;
  uint32_t c = B;
  uint32_t k = (pre + c) >> 5, fill = (pre + c) & 31;
  uint64_t acc = 0;  // bits [32 k, 32 k + fill) of the bitmap (a run of <= 32 values is one step)
  const uint32_t kfirst = k;
  uint32_t nn = 0;
  uint64_t m = c < count ? cm : 0ull;
#ifdef PQG_L1_SKIP_EMIT  // timing experiment only (wrong outputs)
  m = 0;
#endif
  auto flush = [&](uint32_t word) {
    if (k == kfirst) __hip_atomic_fetch_or(bm + k, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    else bm[k] = word;
    nn += __builtin_popcount(word);
    k++;
  };
  // the next run's header is read while the current one's bits are placed
  uint32_t rq = 0;
  L1Run r{};
  bool have = m != 0;  // r: a run to place
  if (have) {
    rq = a + (uint32_t)__builtin_ctzll(m);
    m &= m - 1;
    r = l1_run(win, mis, rq);
  }
  // One loop, a step of which places up to 32 values of the lane's current
  // run; a lane whose run is used up first moves on to its next one in the
  // same step.  The wave takes as many steps as its busiest lane has words,
  // not the longest run of every round of runs.
  uint32_t take = 0, sb = 0, pat = 0;
  bool bp = false;
  while (have | (take != 0)) {
    if (take == 0) {
      const uint32_t cnt = r.bp ? r.g * 8 : r.g;
      take = cnt < count - c ? cnt : count - c;  // >= 1: c < count, and no run on the chain is empty
      const uint32_t pay = rq + r.hl;  // bit-packed payload
      // a short read: the last needed group must start inside the stream (Q5)
      if (r.bp && pay + ((take + 7) >> 3) - 1 >= n) { fail = true; break; }
      c += take;
      have = m != 0 && c < count;
      pat = r.vb ? 0xffffffffu : 0u;  // RLE
      bp = r.bp;
      sb = bp ? (mis + pay) * 8 : 0u;
      // the next run's header, after the last use of this one's: its read is
      // waited for a step later
      if (have) {
        rq = a + (uint32_t)__builtin_ctzll(m);
        m &= m - 1;
        r = l1_run(win, mis, rq);
      }
    }
    const uint32_t nb = take < 32 ? take : 32;
    const uint32_t src = __builtin_amdgcn_alignbit(W[(sb >> 5) + 1], W[sb >> 5], sb & 31);
    const uint32_t bits = (bp ? src : pat) & (nb >= 32 ? 0xffffffffu : ((1u << nb) - 1));
    acc |= (uint64_t)bits << fill;
    fill += nb;
    take -= nb;
    sb += nb;
    if (fill >= 32) {
      flush((uint32_t)acc);
      acc >>= 32;
      fill -= 32;
    }
  }
  // the last, partly filled word, of a lane whose first value lies inside the
  // page: 32 k < pre + c <= pre + count, so k < nw.  (A lane whose first value
  // is at or past `count` placed nothing, and with B saturating at 2^24 its
  // word index lies outside the zeroed words, and can lie outside the table.)
  if (fill && B < count) {
    __hip_atomic_fetch_or(bm + k, (uint32_t)acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    nn += __builtin_popcount((uint32_t)acc);
  }
  if (__ballot(fail)) return false;
  PQG_T(t5);
  PQG_ACC(24, t4, t5);
  __builtin_amdgcn_wave_barrier();
  // ---- 4. level bytes, 16 per lane per step (whole granules: one aligned
  // 1 KiB wave store per step), the ragged first / last granule bytewise
  const PQG_L uint16_t* B16 = (const PQG_L uint16_t*)lds_ptr(sh.tab);
#ifdef PQG_L1_SKIP_EXPAND  // timing experiment only (wrong outputs)
  const uint32_t g0 = 1, g1 = 0;
#else
  const uint32_t g0 = (pre + 15) >> 4, g1 = end >> 4;  // whole granules [g0, g1)
#endif
  for (uint32_t g = g0 + (uint32_t)lane; g < g1; g += 64) {
    const uint32_t b16 = B16[g];
    uint32_t wv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) wv[j] = (((b16 >> (4 * j)) & 0xfu) * 0x00204081u) & 0x01010101u;
    stg16o(a0 + 16 * g, make_uint4(wv[0], wv[1], wv[2], wv[3]));
  }
  if (lane < 32) {
    // the bytes outside whole granules: lanes 0..15 those of the first
    // granule, 16..31 those of the last (the same one for a short page: the
    // same bytes twice)
    const uint32_t gr = lane < 16 ? (pre >> 4) : (end >> 4);
    const uint32_t i = 16 * gr + (uint32_t)(lane & 15);
    if (i >= pre && i < end && (i < 16 * g0 || i >= 16 * g1))
      *(PQG_G uint8_t*)(a0 + i) = (uint8_t)((B16[gr] >> (lane & 15)) & 1);
  }
  *nn_out = (uint32_t)wave_sum((int64_t)nn);
  PQG_T(t6);
  PQG_ACC(25, t5, t6);
  PQG_ACC(26, 0, 1);
  return true;
}

}  // namespace pqg
