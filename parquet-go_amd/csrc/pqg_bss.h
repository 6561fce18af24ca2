// pqg_bss.h — the byte transpose of BYTE_STREAM_SPLIT (parquet-format, Encodings,
// "Byte Stream Split"): out[i * w + k] = val[k * nn + i].  What k_bss (pqg_bss.hip)
// does to registers and to its LDS stage, written so that a host program can run the
// same code on plain memory (tools/bss_model.cpp): byte permutes, the funnel shift of
// two aligned 16-byte granules, and the assembly of one 16-byte output granule from
// the staged streams for the widths 2, 4, 8 and 16.
#pragma once
#include <stdint.h>

#include "pqg_common.h"

namespace pqg {
namespace bss {

constexpr int kTileBytes = 8192;  // value bytes of one tile: the LDS stage of a wave

// v_perm_b32: byte i of the result is byte sel[i] of {a: 4..7, b: 0..3}; 0x0c: zero
__host__ __device__ __forceinline__ uint32_t perm(uint32_t a, uint32_t b, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(a, b, sel);
#else
  const uint64_t v = (uint64_t)a << 32 | b;
  uint32_t r = 0;
  for (int i = 0; i < 4; i++) {
    const uint32_t s = (sel >> (8 * i)) & 0xff;
    r |= (s < 8 ? (uint32_t)(v >> (8 * s)) & 0xff : 0u) << (8 * i);
  }
  return r;
#endif
}
// v_alignbit_b32: the low dword of (hi:lo) >> r, r < 32
__host__ __device__ __forceinline__ uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t r) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, r);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (r & 31));
#endif
}

// Bytes [s, s + 16) of the 32 bytes w0 .. w7 (two consecutive aligned granules), s < 16.
// With s == 0 the second granule is not used (the caller need not have loaded it).
// A barrel shifter over the dwords, by one and then by two, on values passed in
// registers: a select among the elements of an array passed by reference is turned
// into an indexed read of it, which puts the array into scratch memory.
struct Q4 {
  uint32_t x, y, z, w;
};
__host__ __device__ __forceinline__ Q4 funnel16(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4,
                                                uint32_t w5, uint32_t w6, uint32_t w7, uint32_t s) {
  const bool q1 = (s & 4) != 0, q2 = (s & 8) != 0;
  const uint32_t r = (s & 3) * 8;
  const uint32_t t0 = q1 ? w1 : w0, t1 = q1 ? w2 : w1, t2 = q1 ? w3 : w2, t3 = q1 ? w4 : w3, t4 = q1 ? w5 : w4,
                 t5 = q1 ? w6 : w5, t6 = q1 ? w7 : w6;
  const uint32_t e0 = q2 ? t2 : t0, e1 = q2 ? t3 : t1, e2 = q2 ? t4 : t2, e3 = q2 ? t5 : t3, e4 = q2 ? t6 : t4;
  return Q4{alignbit(e1, e0, r), alignbit(e2, e1, r), alignbit(e3, e2, r), alignbit(e4, e3, r)};
}

// Four streams' dwords (byte i of s[k]: byte k of value i) to four values' dwords.
__host__ __device__ __forceinline__ void tr4x4(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t (&o)[4]) {
  const uint32_t lo01 = perm(s1, s0, 0x05010400u), hi01 = perm(s1, s0, 0x07030602u);
  const uint32_t lo23 = perm(s3, s2, 0x05010400u), hi23 = perm(s3, s2, 0x07030602u);
  o[0] = perm(lo23, lo01, 0x05040100u);
  o[1] = perm(lo23, lo01, 0x07060302u);
  o[2] = perm(hi23, hi01, 0x05040100u);
  o[3] = perm(hi23, hi01, 0x07060302u);
}

// Output granule g of a tile (its bytes [16 g, 16 g + 16), 16 / W whole values) from the
// staged streams: stream k's byte of the tile's value x is st[k * (kTileBytes / W) + x].
// R reads the stage: u8 / u16 / u32 (byte offset), every read naturally aligned (LDS on
// the device, plain memory in the host model).
template <int W, class R>
__host__ __device__ __forceinline__ void granule(const R& st, int g, uint32_t (&o)[4]) {
  static_assert(W == 2 || W == 4 || W == 8 || W == 16, "specialised widths");
  constexpr int T = kTileBytes / W;
  if (W == 4) {
    uint32_t s[4];
#pragma unroll
    for (int k = 0; k < 4; k++) s[k] = st.u32(k * T + 4 * g);
    tr4x4(s[0], s[1], s[2], s[3], o);
  } else if (W == 2) {
    uint32_t s[2][2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
      s[k][0] = st.u32(k * T + 8 * g);
      s[k][1] = st.u32(k * T + 8 * g + 4);
    }
    o[0] = perm(s[1][0], s[0][0], 0x05010400u);
    o[1] = perm(s[1][0], s[0][0], 0x07030602u);
    o[2] = perm(s[1][1], s[0][1], 0x05010400u);
    o[3] = perm(s[1][1], s[0][1], 0x07030602u);
  } else if (W == 8) {
    uint32_t s[8];
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = st.u16(k * T + 2 * g);
    const uint32_t p01 = perm(s[1], s[0], 0x05010400u), p23 = perm(s[3], s[2], 0x05010400u);
    const uint32_t p45 = perm(s[5], s[4], 0x05010400u), p67 = perm(s[7], s[6], 0x05010400u);
    o[0] = perm(p23, p01, 0x05040100u);
    o[1] = perm(p67, p45, 0x05040100u);
    o[2] = perm(p23, p01, 0x07060302u);
    o[3] = perm(p67, p45, 0x07060302u);
  } else {
    uint32_t s[16];
#pragma unroll
    for (int k = 0; k < 16; k++) s[k] = st.u8(k * T + g);
#pragma unroll
    for (int d = 0; d < 4; d++) o[d] = s[4 * d] | s[4 * d + 1] << 8 | s[4 * d + 2] << 16 | s[4 * d + 3] << 24;
  }
}

// Output granule g of a tile to memory: the 16 bytes at o = the tile's output base + og,
// of which the part owns the tile's bytes [lo, hi).  A whole granule is one 16-byte
// store; the part's first or last granule stores its dwords (W = 2: halves) inside
// [lo, hi).  S stores: st16 / st4 / st2 (address, value).
template <int W, class S>
__host__ __device__ __forceinline__ void store_granule(const S& sink, uintptr_t o, uint32_t og, uint32_t lo, uint32_t hi,
                                                       const uint32_t (&g)[4]) {
  if (og >= lo && og + 16 <= hi) {
    sink.st16(o, g[0], g[1], g[2], g[3]);
  } else if (og + 16 > lo && og < hi) {
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const uint32_t da = og + 4 * d;
      if (da >= lo && da + 4 <= hi) {
        sink.st4(o + 4 * d, g[d]);
      } else if (W == 2) {
        if (da >= lo && da + 2 <= hi) sink.st2(o + 4 * d, g[d] & 0xffffu);
        if (da + 2 >= lo && da + 4 <= hi) sink.st2(o + 4 * d + 2, g[d] >> 16);
      }
    }
  }
}

// The address arithmetic of one part [v_lo, v_hi) of a page of nn values of W bytes
// (stream k at val + k nn, the page's values at out).  The part's output bytes
// [ob, oe) start W-aligned only, so positions are counted from the 16-byte boundary oa
// at or below ob: position x is value v_lo - a + x, its output bytes oa + x W, and the
// part's values are the positions [a, xn).  A tile is kTileBytes / W positions from a
// multiple t0 of that: every output granule of a tile is 16-byte aligned and holds
// whole values.
template <int W>
struct Part {
  static constexpr int T = kTileBytes / W;   // positions per tile
  static constexpr int GS = T / 16;          // 16-byte granules of one stream per tile
  static constexpr int NL = W * GS / 64;     // granules a lane stages, and output granules it stores, per tile
  static_assert(NL == 8, "kTileBytes is 64 lanes x 8 granules");
  uintptr_t val, ob, oe, oa;
  int64_t nn, a, xn, src0;
  __host__ __device__ __forceinline__ void init(uintptr_t val_, int64_t nn_, int64_t v_lo, int64_t v_hi, uintptr_t out) {
    val = val_;
    nn = nn_;
    ob = out + (uintptr_t)v_lo * W;
    oe = out + (uintptr_t)v_hi * W;
    oa = ob & ~(uintptr_t)15;
    a = (int64_t)(ob - oa) / W;
    xn = a + (v_hi - v_lo);
    src0 = v_lo - a;  // stream offset of position 0 (below 0 only for positions below a, never read)
  }
  // Granule j of a lane in the tile at t0: the stage bytes [st, st + 16) are the stream's
  // bytes of 16 positions, the source bytes [p, p + 16) with p = base + off + s, out of the
  // aligned granules at base + off and base + off + 16.  A granule is loaded only when it
  // holds a byte of the stream that the part reads in this tile; otherwise the load goes
  // to one that does (off_a / off_b say where each load goes; its bytes are then never
  // stored).  base is the same for every lane when GS >= 64 (one stream per load
  // instruction): the lanes differ in 32-bit offsets only.
  struct Load {
    uintptr_t base;
    uint32_t off_a, off_b, s;
    int st;
  };
  __host__ __device__ __forceinline__ Load load(int64_t t0, int lane, int j) const {
    const int gidx = lane + 64 * j, k = GS >= 64 ? (64 * j) / GS : gidx / GS, gi = gidx % GS;
    const int64_t xl = a > t0 ? a : t0, xh = xn < t0 + T ? xn : t0 + T;  // the tile's positions of the part
    const uintptr_t pa = val + (uintptr_t)((int64_t)k * nn + src0 + t0);   // stream k's byte of position t0
    Load r;
    r.base = pa & ~(uintptr_t)15;
    r.s = (uint32_t)(pa & 15);
    r.st = k * T + 16 * gi;
    // the stream bytes read in this tile, relative to base: [lo, hi), 0 <= lo < hi <= T + 15
    const uint32_t lo = r.s + (uint32_t)(xl - t0), hi = r.s + (uint32_t)(xh - t0), off = 16u * (uint32_t)gi;
    const uint32_t safe = lo & ~15u;
    r.off_a = off < hi && off + 16 > lo ? off : safe;
    r.off_b = r.s != 0 && off + 16 < hi && off + 32 > lo ? off + 16 : safe;
    return r;
  }
  // The tile's output bytes start at out_base(t0) (16-byte aligned); the part's bytes of
  // them are [lo, hi) of the tile's kTileBytes.
  __host__ __device__ __forceinline__ uintptr_t out_base(int64_t t0) const { return oa + (uintptr_t)t0 * W; }
  __host__ __device__ __forceinline__ void out_range(int64_t t0, uint32_t* lo, uint32_t* hi) const {
    const uintptr_t tb = out_base(t0);
    *lo = ob > tb ? (uint32_t)(ob - tb) : 0u;
    *hi = oe - tb < (uintptr_t)kTileBytes ? (uint32_t)(oe - tb) : (uint32_t)kTileBytes;
  }
};

}  // namespace bss
}  // namespace pqg
