// pqg_convert.h — K10: what one lane of k_conv_* (pqg_convert.hip) loads, computes and stores,
// written over an IO policy so that a host program runs the same code on plain memory
// (tools/convert_model.cpp): which aligned 16-byte granules of a tile's input are loaded and
// where they are staged, the byte reversal and sign fill of one decimal, the INT96 -> int64
// arithmetic, and the bad-length rule of BYTE_ARRAY decimals.
//
// Fixed-width input (DECIMAL_BE w = 1..32, DECIMAL_INT w = 4 / 8, INT96_TIME w = 12): a wave
// takes a segment of flt::kSeg values in tiles of tile_values(w) of them (at most kTileBytes of
// input).  A tile's input bytes [in + t0 w, in + t1 w) are contiguous but aligned to nothing,
// so the wave loads the aligned granules that hold a byte of them into a stage laid out as the
// input is: stage byte kPad + s is the byte at (in + t0 w rounded down to 16) + s.  A lane
// then reads its value's dwords from the stage (two aligned dwords funnelled by alignbit),
// reverses them, fills the sign and stores whole aligned 16-byte granules.
//
// IO: G  ld16(address) -> Q4: an aligned 16-byte global load;  u8(address): one byte
//     ST put16(offset, Q4), u32(offset), u8(offset): the stage, every access naturally aligned
//     S  st16(address, x, y, z, w), st8(address, lo, hi): aligned global stores
#pragma once
#include <stdint.h>

#include "pqg_bss.h"
#include "pqg_common.h"

namespace pqg {
namespace conv {

// pqg_convert_args.kind / .unit (include/pqgpu.h)
enum : int { K_DECIMAL_BE = 0, K_DECIMAL_INT = 1, K_INT96_TIME = 2 };
enum : int { U_SECONDS = 1, U_MILLIS = 2, U_MICROS = 3, U_NANOS = 4 };

constexpr int kSeg = 4096;        // values per wave segment (flt::kSeg)
constexpr int kTileBytes = 8192;  // input bytes of one tile at most
constexpr int kPad = 16;          // stage bytes before the first granule and after the last
constexpr int kStageBytes = kPad + kTileBytes + 16 + kPad;  // + the input's misalignment
constexpr int64_t kJulianEpoch = 2440588;                   // julian day of 1970-01-01

using bss::Q4;

// values per tile: whole groups of 64 (128 for INT96: a lane stores two int64), at most
// kTileBytes of input, at most a segment
__host__ __device__ __forceinline__ int tile_values(int kind, int w) {
  if (kind == K_INT96_TIME) return 640;  // 5 groups of 128 x 12 bytes
  int g = kTileBytes / (64 * w);         // 4 (w = 32) .. 128
  if (g > kSeg / 64) g = kSeg / 64;
  return 64 * g;
}

// Tile [t0, t1) of the values at `in` (w bytes each): the aligned granules [gbase, gbase + 16 ng)
// are those that hold one of its bytes; its first byte is stage byte kPad + m.
struct Tile {
  uintptr_t gbase;
  uint32_t m;
  int ng;
};
__host__ __device__ __forceinline__ Tile tile_of(uintptr_t in, int w, int64_t t0, int64_t t1) {
  const uintptr_t b = in + (uintptr_t)t0 * (uintptr_t)w, e = in + (uintptr_t)t1 * (uintptr_t)w;
  Tile t;
  t.gbase = b & ~(uintptr_t)15;
  t.m = (uint32_t)(b & 15);
  t.ng = t1 > t0 ? (int)((e - t.gbase + 15) >> 4) : 0;
  return t;
}

// The lane's share of a tile's granules into the stage: granules lane, lane + 64, ..., four
// loads issued before their four stage writes.
template <class G, class ST>
__host__ __device__ __forceinline__ void stage_tile(const G& g, const ST& st, const Tile& t, int lane) {
  for (int j0 = lane; j0 < t.ng; j0 += 256) {
    Q4 q[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int j = j0 + 64 * u;
      q[u] = g.ld16(t.gbase + 16 * (uintptr_t)(j < t.ng ? j : j0));
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int j = j0 + 64 * u;
      if (j < t.ng) st.put16(kPad + 16 * j, q[u]);
    }
  }
}

__host__ __device__ __forceinline__ uint32_t bswap32(uint32_t v) { return bss::perm(0, v, 0x00010203u); }

// the little-endian dword at any stage byte offset: two aligned dwords, funnelled
template <class ST>
__host__ __device__ __forceinline__ uint32_t stage_u32(const ST& st, uint32_t a) {
  const uint32_t al = a & ~3u;
  return bss::alignbit(st.u32(al + 4), st.u32(al), (a & 3) * 8);
}

// One decimal of w bytes at stage offset `off` as OD little-endian dwords, sign-extended.
// be: big-endian input (out byte k = in byte w - 1 - k); else little-endian (DECIMAL_INT).
// Output dword d holds input bytes [w - 4 d - 4, w - 4 d) (be) or [4 d, 4 d + 4): nb of them
// lie inside the value, the rest is sign.  Neighbouring dwords share an aligned stage dword.
template <int OD, class ST>
__host__ __device__ __forceinline__ void decimal_value(const ST& st, uint32_t off, int w, bool be, uint32_t (&o)[OD]) {
  const uint32_t sign = (st.u8(be ? off : off + (uint32_t)w - 1) & 0x80u) ? 0xffffffffu : 0u;
  // dword 0's bytes start at a (be: may lie up to 3 bytes before the value, inside the pad)
  const uint32_t a = be ? off + (uint32_t)w - 4 : off;
  const uint32_t al = a & ~3u, r = (a & 3) * 8;
  uint32_t lo = st.u32(al), hi = st.u32(al + 4);
#pragma unroll
  for (int d = 0; d < OD; d++) {
    const int nb = w - 4 * d >= 4 ? 4 : w - 4 * d > 0 ? w - 4 * d : 0;
    uint32_t v = sign;
    if (nb > 0) {
      const uint32_t u = bss::alignbit(hi, lo, r);
      const uint32_t mask = nb == 4 ? 0xffffffffu : (1u << (8 * nb)) - 1u;
      v = ((be ? bswap32(u) : u) & mask) | (sign & ~mask);
    }
    o[d] = v;
    if (d + 1 < OD && w - 4 * (d + 1) > 0) {  // the next dword lies one aligned dword down (be) or up
      if (be) {
        hi = lo;
        lo = st.u32(al - 4u * (uint32_t)(d + 1));
      } else {
        lo = hi;
        hi = st.u32(al + 4u * (uint32_t)(d + 1) + 4);
      }
    }
  }
}

// INT96 (nanos of the day u64, julian day i32) to int64 in `unit`: the divide is unsigned and
// truncates, the multiply and the add wrap in 64 bits.
__host__ __device__ __forceinline__ uint64_t int96_time(uint32_t n_lo, uint32_t n_hi, uint32_t day, int unit) {
  const uint64_t nanos = (uint64_t)n_hi << 32 | n_lo;
  const uint64_t days = (uint64_t)((int64_t)(int32_t)day - kJulianEpoch);
  switch (unit) {
    case U_SECONDS: return days * 86400ull + nanos / 1000000000ull;
    case U_MILLIS: return days * 86400000ull + nanos / 1000000ull;
    case U_MICROS: return days * 86400000000ull + nanos / 1000ull;
    default: return days * 86400000000000ull + nanos;
  }
}
template <class ST>
__host__ __device__ __forceinline__ uint64_t int96_value(const ST& st, uint32_t off, int unit) {
  return int96_time(stage_u32(st, off), stage_u32(st, off + 4), stage_u32(st, off + 8), unit);
}

// Value v of the tile (lane L takes values L, L + 64, ... of it): OD dwords as OD / 4 aligned
// granules.  16-byte decimals go out non-temporally, a KiB per instruction; a 32-byte
// decimal's two granules are every other granule of two instructions, which write-back
// stores leave to the L2 to merge.
template <int OD, class ST, class S>
__host__ __device__ __forceinline__ void decimal_store(const ST& st, const S& sink, const Tile& t, int w, bool be, int v,
                                                        uintptr_t out_v) {
  uint32_t o[OD];
  decimal_value<OD>(st, kPad + t.m + (uint32_t)v * (uint32_t)w, w, be, o);
  if constexpr (OD == 4) {
    sink.st16(out_v, o[0], o[1], o[2], o[3]);
  } else {
    sink.st16wb(out_v, o[0], o[1], o[2], o[3]);
    sink.st16wb(out_v + 16, o[4], o[5], o[6], o[7]);
  }
}

// Values 2 p and 2 p + 1 of the tile (nv values) as one aligned granule; a last odd value as 8 bytes.
template <class ST, class S>
__host__ __device__ __forceinline__ void int96_store(const ST& st, const S& sink, const Tile& t, int unit, int p, int nv,
                                                      uintptr_t out_p) {
  if (2 * p >= nv) return;
  const uint32_t off = kPad + t.m + 24u * (uint32_t)p;
  const uint64_t a = int96_value(st, off, unit);
  if (2 * p + 1 < nv) {
    const uint64_t b = int96_value(st, off + 12, unit);
    sink.st16(out_p, (uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
  } else {
    sink.st8(out_p, (uint32_t)a, (uint32_t)(a >> 32));
  }
}

// BYTE_ARRAY decimals: the length of value i, or -1 for a bad one: offsets that are negative,
// not ascending or past values_bytes, a length of 0 or above the output width.
__host__ __device__ __forceinline__ int64_t bytes_len(int64_t o0, int64_t o1, int64_t values_bytes, int ow) {
  if (o0 < 0 || o1 < o0 || o1 > values_bytes) return -1;
  const int64_t len = o1 - o0;
  return len >= 1 && len <= ow ? len : -1;
}

// One BYTE_ARRAY decimal of len bytes at address p, read bytewise, as OD dwords.
template <int OD, class G>
__host__ __device__ __forceinline__ void bytes_value(const G& g, uintptr_t p, int len, uint32_t (&o)[OD]) {
  const uint32_t sign = (g.u8(p) & 0x80u) ? 0xffu : 0u;
#pragma unroll
  for (int d = 0; d < OD; d++) {
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int k = 4 * d + b;
      v |= (k < len ? g.u8(p + (uintptr_t)(len - 1 - k)) : sign) << (8 * b);
    }
    o[d] = v;
  }
}

}  // namespace conv
}  // namespace pqg
