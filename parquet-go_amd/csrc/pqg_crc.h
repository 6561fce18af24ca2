// pqg_crc.h — CRC-32 (zlib / gzip: reflected polynomial 0xedb88320) arithmetic shared by
// k_inflate* (the gzip trailer) and K1c k_page_crc (PageHeader.crc), host + device: the tile
// and combine code below is what the kernels run, and tools/crc_model.cpp runs the same code
// with the 64 lanes one after another.
//
// Everything works on the RAW register (initial value 0, no final xor):
//   raw(A || B) = raw(A) x^(8 |B|)  ^  raw(B)          in GF(2)[x] / P, reflected
//   crc32(M)    = ~( 0xffffffff x^(8 |M|)  ^  raw(M) )
// so leading zero bytes leave a raw register of 0 unchanged: a payload that starts anywhere
// in its first 16-byte granule is read as aligned granules with the bytes before it masked
// to zero, and a tile that is no multiple of a wave row is padded IN FRONT with zero granules.
#pragma once
#include "pqg_common.h"

namespace pqg {

constexpr uint32_t kCrcPoly = 0xedb88320u;  // CRC-32 (IEEE, reflected): gzip trailer, PageHeader.crc

// a * b mod P over GF(2), reflected (bit 31 = x^0): zlib's multmodp,
// branch-free (32 fixed steps: the lanes of a CRC combine hold different a)
__host__ __device__ constexpr uint32_t multmodp(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll 4
  for (int i = 0; i < 32; i++) {
    p ^= b & (0u - ((a >> (31 - i)) & 1u));
    b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
  }
  return p;
}
// x^(2^k) mod P, k = 0..31 (zlib's x2n_table; the period is 32)
struct X2n {
  uint32_t v[32];
};
constexpr X2n make_x2n() {
  X2n t{};
  uint32_t p = 1u << 30;  // x^1
  t.v[0] = p;
  for (int k = 1; k < 32; k++) t.v[k] = p = multmodp(p, p);
  return t;
}
#if defined(__HIPCC__)
static __device__ const X2n kX2n = make_x2n();
#endif
constexpr X2n kX2nHost = make_x2n();
// x^(8 n) mod P: one multiply per set bit of n (zlib's x2nmodp(n, 3))
__host__ __device__ __forceinline__ uint32_t x8nmodp(uint64_t n) {
  uint32_t p = 1u << 31;  // x^0
  for (int k = 3; n; k++, n >>= 1)
#if defined(__HIP_DEVICE_COMPILE__)
    if (n & 1) p = multmodp(kX2n.v[k & 31], p);
#else
    if (n & 1) p = multmodp(kX2nHost.v[k & 31], p);
#endif
  return p;
}

namespace crc {

// ---------------------------------------------------------------------------
// K1c.  A page's payload [p, p + n) is read as the aligned granules from p & ~15 on, cut
// into tiles of kTile bytes of that aligned space (the first `p & 15` bytes of tile 0 lie
// before the payload and are masked to zero).  One wave takes a tile: lane L consumes the
// granules L, L + 64, ... straight from its loads (no LDS stage), so its register sees 16
// data bytes, then 1008 bytes of the other lanes, then its next 16 bytes.  That gap is
// folded into the step:
//   c' = G0[c byte 0] ^ .. ^ G3[c byte 3]  ^  T0[data byte 0] ^ .. ^ T15[data byte 15]
//   T_k[b] = raw(b, then 15 - k zero bytes)        (slicing-by-16's tables)
//   G_k[b] = raw(b, then 1023 - k zero bytes)      (the register moved on by one wave row)
// After its last granule lane L is 16 (63 - L) bytes short of the end of the last row: one
// multiply by the per-lane constant x^(8 16 (63 - L)), an xor over the wave, and the whole
// granules are done; the ragged last granule's bytes follow bytewise (T15 is the plain
// byte table).  A tile of nfull whole granules that is no multiple of 64 gets
// (64 - nfull % 64) % 64 zero granules in front, so every lane has the same count and the
// same constant at any length.
// ---------------------------------------------------------------------------
#ifndef PQG_CRC_TILE
#define PQG_CRC_TILE 16384
#endif
constexpr int kTile = PQG_CRC_TILE;
constexpr int kRow = 1024;    // bytes of one wave row: 64 lanes x 16
constexpr int kBatch = 8;     // a lane's loads in flight before its first table read (half a 16 KiB tile)
constexpr int kTabs = 20;     // T0..T15, G0..G3: 256 words each
static_assert(kTile % kRow == 0 && kTile >= kRow, "tiles are whole wave rows");

// page states (pqg_page_crc.state); kPending: to be checked (k_crc_plan -> k_crc_fin)
enum : int32_t { kNoField = 0, kVerified = 1, kMismatch = 2, kNotChecked = 3, kPending = 4 };

struct Rec {            // one per page-table entry
  const uint8_t* p;     // payload
  int64_t n;            // its bytes (compressed_page_size)
  int64_t tile_base;    // first of the page's tile records / raw registers
  int32_t ntiles;       // -1: no room in the tile table, k_crc_fin reads the page itself (lane_slice)
  int32_t state;
  uint32_t stored, computed;
};
struct TileRec {
  int32_t rec;  // Rec index
  int32_t t;    // tile of the page
};

// x^(8 n), usable in constant expressions
constexpr uint32_t xpow8(uint64_t n) {
  const X2n t = make_x2n();
  uint32_t p = 1u << 31;
  for (int k = 3; n; k++, n >>= 1)
    if (n & 1) p = multmodp(t.v[k & 31], p);
  return p;
}
constexpr uint32_t kXGap = xpow8(kRow - 4 - 15);  // T0 (15 zero bytes behind) -> G3 (1020 behind)
constexpr uint32_t kXTile = xpow8(kTile);

__host__ __device__ __forceinline__ uint32_t byte_entry(uint32_t b) {
  for (int i = 0; i < 8; i++) b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
  return b;
}

// Table build, in kTabs rounds with a barrier of the builders between them; lane `lane` of
// `lanes` fills entries lane, lane + lanes, ... of the round's table.  Tab: uint32_t get(int i), void
// put(int i, uint32_t v) over kTabs * 256 words; T_k at 256 k, G_k at 256 (16 + k).
template <class Tab>
__host__ __device__ __forceinline__ void build_round(Tab& tb, int lane, int round, int lanes = 64) {
  for (int b = lane; b < 256; b += lanes) {
    uint32_t v;
    if (round == 0) {
      tb.put(15 * 256 + b, byte_entry((uint32_t)b));
      continue;
    }
    // one more zero byte behind the entry: v' = T15[v & 0xff] ^ (v >> 8)
    const int dst = round <= 15 ? 15 - round : round == 16 ? 19 : 35 - round;  // T14..T0, G3, G2..G0
    const int src = round <= 15 ? dst + 1 : round == 16 ? 0 : dst + 1;
    v = tb.get(src * 256 + b);
    if (round == 16) v = multmodp(v, kXGap);
    else v = tb.get(15 * 256 + (int)(v & 0xff)) ^ (v >> 8);
    tb.put(dst * 256 + b, v);
  }
}

struct Q4 {
  uint32_t x, y, z, w;
};

// the register moved on by one wave row: 4 table reads that wait for the step before
template <class Tab>
__host__ __device__ __forceinline__ uint32_t gap4(const Tab& tb, uint32_t c) {
  return tb.get(16 * 256 + (int)(c & 0xff)) ^ tb.get(17 * 256 + (int)((c >> 8) & 0xff)) ^
         tb.get(18 * 256 + (int)((c >> 16) & 0xff)) ^ tb.get(19 * 256 + (int)(c >> 24));
}
// raw register of one granule: 16 table reads that wait for nothing but the granule's load
template <class Tab>
__host__ __device__ __forceinline__ uint32_t data16(const Tab& tb, const Q4& d) {
  uint32_t r = tb.get(0 * 256 + (int)(d.x & 0xff)) ^ tb.get(1 * 256 + (int)((d.x >> 8) & 0xff)) ^
               tb.get(2 * 256 + (int)((d.x >> 16) & 0xff)) ^ tb.get(3 * 256 + (int)(d.x >> 24));
  r ^= tb.get(4 * 256 + (int)(d.y & 0xff)) ^ tb.get(5 * 256 + (int)((d.y >> 8) & 0xff)) ^
       tb.get(6 * 256 + (int)((d.y >> 16) & 0xff)) ^ tb.get(7 * 256 + (int)(d.y >> 24));
  r ^= tb.get(8 * 256 + (int)(d.z & 0xff)) ^ tb.get(9 * 256 + (int)((d.z >> 8) & 0xff)) ^
       tb.get(10 * 256 + (int)((d.z >> 16) & 0xff)) ^ tb.get(11 * 256 + (int)(d.z >> 24));
  r ^= tb.get(12 * 256 + (int)(d.w & 0xff)) ^ tb.get(13 * 256 + (int)((d.w >> 8) & 0xff)) ^
       tb.get(14 * 256 + (int)((d.w >> 16) & 0xff)) ^ tb.get(15 * 256 + (int)(d.w >> 24));
  return r;
}

// the first `h` (0..16) bytes of a granule to zero
__host__ __device__ __forceinline__ void mask_head(Q4& d, uint32_t h) {
  uint32_t* w[4] = {&d.x, &d.y, &d.z, &d.w};
  for (int j = 0; j < 4; j++) {
    const uint32_t lo = 4u * (uint32_t)j;
    if (h >= lo + 4) *w[j] = 0;
    else if (h > lo) *w[j] &= 0xffffffffu << (8 * (h - lo));
  }
}

__host__ __device__ __forceinline__ int64_t num_tiles(uintptr_t p, int64_t n) {
  return n <= 0 ? 0 : ((int64_t)(p & 15) + n + kTile - 1) / kTile;
}
// payload offset of the end of tile t
__host__ __device__ __forceinline__ int64_t tile_end(uintptr_t p, int64_t n, int64_t t) {
  const int64_t e = (t + 1) * (int64_t)kTile - (int64_t)(p & 15);
  return e < n ? e : n;
}
__host__ __device__ __forceinline__ int64_t tile_bytes(uintptr_t p, int64_t n, int64_t t) {
  return tile_end(p, n, t) - (t > 0 ? tile_end(p, n, t - 1) : 0);
}

struct Tile {
  uintptr_t base;  // aligned address of the tile's first granule
  uint32_t head;   // bytes of granule 0 before the payload (tile 0 only)
  int32_t nfull;   // whole granules
  int32_t m;       // bytes of the ragged last granule (granule nfull), 0: none
  int32_t pad;     // zero granules in front: (nfull + pad) % 64 == 0
  int32_t cnt;     // granules per lane
  __host__ __device__ __forceinline__ void init(uintptr_t p, int64_t n, int64_t t) {
    const uint32_t h = (uint32_t)(p & 15);
    const int64_t N = (int64_t)h + n, lo = t * (int64_t)kTile;
    const int64_t hi = lo + kTile < N ? lo + kTile : N;
    const int32_t r = (int32_t)(hi - lo);
    base = p - h + (uintptr_t)lo;
    head = t == 0 ? h : 0;
    nfull = r >> 4;
    m = r & 15;
    pad = (64 - (nfull & 63)) & 63;
    cnt = (nfull + pad) >> 6;
  }
  // lane's i-th granule (negative: one of the zero granules in front)
  __host__ __device__ __forceinline__ int gran(int lane, int i) const { return lane + 64 * i - pad; }
};

// per-lane constant: the bytes between the end of lane L's granule and the end of its row
__host__ __device__ __forceinline__ uint32_t lane_mul(int lane) { return x8nmodp((uint64_t)(16 * (63 - lane))); }

// One batch of a lane's granules, i0 .. i0 + nb (nb == kBatch when kFull).  Ld: Q4 operator()(uintptr_t
// aligned address).  Every load is issued before the first table read; a load that has no granule
// (a zero granule in front, a slot past nb) reads the tile's last whole granule instead, so no load
// leaves the tile.  A full batch first takes every granule's own register (reads that depend on
// the loads alone), then chains them through the gap step; a short one goes granule by granule.
template <bool kFull, class Ld, class Tab>
__host__ __device__ __forceinline__ uint32_t lane_batch(const Tile& tl, int lane, int i0, int nb, uint32_t c, const Ld& ld,
                                                        const Tab& tb) {
  Q4 g[kBatch];
#pragma unroll
  for (int j = 0; j < kBatch; j++) {
    const int gi = tl.gran(lane, i0 + j);
    const bool ok = (kFull || j < nb) && gi >= 0;
    g[j] = ld(tl.base + 16 * (uintptr_t)(ok ? gi : tl.nfull - 1));
  }
  if (i0 == 0) {  // only a lane's first granule can be a zero granule or hold the payload's first byte
    const int gi = tl.gran(lane, 0);
    if (gi < 0) g[0] = Q4{0, 0, 0, 0};
    else if (gi == 0) mask_head(g[0], tl.head);
  }
  if (kFull) {
    uint32_t t[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; j++) t[j] = data16(tb, g[j]);
#pragma unroll
    for (int j = 0; j < kBatch; j++) c = gap4(tb, c) ^ t[j];
  } else {
#pragma unroll
    for (int j = 0; j < kBatch; j++)
      if (j < nb) c = gap4(tb, c) ^ data16(tb, g[j]);
  }
  return c;
}

// One lane's register over its granules of the tile (before lane_mul): the count's remainder
// first, then full batches.
template <class Ld, class Tab>
__host__ __device__ __forceinline__ uint32_t lane_tile(const Tile& tl, int lane, const Ld& ld, const Tab& tb) {
  uint32_t c = 0;
  int i0 = tl.cnt % kBatch;
  if (i0) c = lane_batch<false>(tl, lane, 0, i0, c, ld, tb);
  for (; i0 < tl.cnt; i0 += kBatch) c = lane_batch<true>(tl, lane, i0, kBatch, c, ld, tb);
  return c;
}

// The tile's raw register from the xor `r` of the lanes' registers (each times lane_mul):
// the ragged last granule's bytes, bytewise.  The same for every lane.
template <class Ld, class Tab>
__host__ __device__ __forceinline__ uint32_t tile_tail(const Tile& tl, uint32_t r, const Ld& ld, const Tab& tb) {
  if (tl.m == 0) return r;
  Q4 d = ld(tl.base + 16 * (uintptr_t)tl.nfull);
  if (tl.nfull == 0) mask_head(d, tl.head);  // leading zeros: r is 0 here
  const uint32_t w[4] = {d.x, d.y, d.z, d.w};
  for (int k = 0; k < tl.m; k++) {
    const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 0xff;
    r = tb.get(15 * 256 + (int)((r ^ b) & 0xff)) ^ (r >> 8);
  }
  return r;
}

// Combine of a page's tile registers into its crc32.  Lane 63 carries the initial value
// (0xffffffff, n bytes before the end), lane 62 the last tile (the ragged one: it ends where the
// payload ends), lanes 0..61 fold the other tiles [L q, (L + 1) q), q = ceil((nt - 1) / 62) -- whole
// tiles all, but for tile 0, which only ever starts a fold -- with one multiply by x^(8 kTile)
// per further tile.  Every lane then moves its register to the payload's end: one x8nmodp and
// one multiply per lane, whatever the page.  The crc32 is the inverted xor of the lanes' returns.
// Raw: uint32_t operator()(int64_t tile).
template <class Raw>
__host__ __device__ __forceinline__ uint32_t lane_combine(uintptr_t p, int64_t n, int64_t nt, int lane, const Raw& raw) {
  uint32_t v = 0;
  int64_t e = 0;
  if (lane == 63) {
    v = 0xffffffffu;
    e = n;
  } else if (lane == 62) {
    if (nt > 0) v = raw(nt - 1);
  } else {
    const int64_t m = nt - 1, q = (m + 61) / 62, t0 = lane * q, t1 = t0 + q < m ? t0 + q : m;
    if (t0 < t1) {
      for (int64_t t = t0; t < t1; t++) v = multmodp(v, kXTile) ^ raw(t);
      e = n - tile_end(p, n, t1 - 1);
    }
  }
  return multmodp(v, x8nmodp((uint64_t)e));
}

// The same for a page that got no tile records (the tile table is sized for pages that do not
// overlap): lane L takes the bytes [L s, (L + 1) s), s = ceil(n / 64), bit by bit, without tables.
// Slow, and never run on a file whose pages follow one another.  Byte: uint32_t operator()(int64_t i).
template <class Byte>
__host__ __device__ __forceinline__ uint32_t lane_slice(int64_t n, int lane, const Byte& byte) {
  const int64_t s = (n + 63) / 64, b0 = lane * s < n ? lane * s : n, b1 = b0 + s < n ? b0 + s : n;
  uint32_t c = 0;
  for (int64_t i = b0; i < b1; i++) {
    c ^= byte(i);
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
  }
  uint32_t r = multmodp(c, x8nmodp((uint64_t)(n - b1)));
  if (lane == 0) r ^= multmodp(0xffffffffu, x8nmodp((uint64_t)n));
  return r;
}

}  // namespace crc
}  // namespace pqg
