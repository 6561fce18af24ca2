// pqg_wavecopy.h — the byte copies of a wave that decodes an LZ77 stream into
// a block of HBM (k_zstd, k_lz4): runs that do not overlap themselves as
// aligned dwords, one per lane, funnel-shifted out of the aligned source
// dwords; overlapping matches bytewise (source start + i % offset).  History
// is the stored output: a match whose source is not known to be stored yet
// first waits for the wave's own stores (s_waitcnt vmcnt(0)) and reads through
// L2.  All stores are ordinary vector stores.  Also where a page's compressed
// block lies (zstd_loc).
#pragma once
#include <hip/hip_runtime.h>

#include "pqg_device.h"

namespace pqg {

struct WaveCopy {
  gu8 out;  // the block being written
  int ln;   // this lane
  int64_t stored = 0;  // output bytes below this are known to be stored

  // the wave's own stores have completed
  __device__ __forceinline__ void drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

  // a byte / the aligned dword at p; L2: through L2 (bytes this wave stored)
  template <bool L2>
  __device__ __forceinline__ uint32_t ldw(uintptr_t a) const {
    const PQG_G uint32_t* q = (const PQG_G uint32_t*)a;
    return L2 ? ld_l2_u32(q) : *q;
  }
  template <bool L2>
  __device__ __forceinline__ uint32_t ldb(gcu8 p) const {
    const uintptr_t a = (uintptr_t)p;
    return (ldw<L2>(a & ~(uintptr_t)3) >> (8 * (a & 3))) & 0xff;
  }
  // dst[0..len) = src[0..len), not overlapping: aligned dwords of dst, one
  // per lane, each out of the one or two aligned source dwords that hold its
  // bytes (a dword holding a source byte lies in mapped memory)
  template <bool L2>
  __device__ __forceinline__ void copy(gu8 dst, gcu8 src, int64_t len) {
    int64_t head = (int64_t)((4 - ((uintptr_t)dst & 3)) & 3);
    if (head > len) head = len;
    if (ln < head) dst[ln] = (uint8_t)ldb<L2>(src + ln);
    const int64_t body = (len - head) & ~(int64_t)3;
    gu8 db = dst + head;
    const uintptr_t sa = (uintptr_t)(src + head);
    const uint32_t sh = (uint32_t)(sa & 3) * 8;
    const uintptr_t sb = sa & ~(uintptr_t)3;
    for (int64_t g = (int64_t)ln * 4; g < body; g += 256) {
      const uint32_t lo = ldw<L2>(sb + g);
      const uint32_t hi = sh ? ldw<L2>(sb + g + 4) : 0u;
      *(PQG_G uint32_t*)(db + g) = __builtin_amdgcn_alignbit(hi, lo, sh);
    }
    const int64_t t0 = head + body;
    if (t0 + ln < len) dst[t0 + ln] = (uint8_t)ldb<L2>(src + t0 + ln);
  }

  __device__ __forceinline__ void out_fill(int64_t d, uint8_t b, int64_t len) {
    gu8 dst = out + d;
    int64_t head = (int64_t)((4 - ((uintptr_t)dst & 3)) & 3);
    if (head > len) head = len;
    if (ln < head) dst[ln] = b;
    const int64_t body = (len - head) & ~(int64_t)3;
    const uint32_t v = 0x01010101u * b;
    for (int64_t g = (int64_t)ln * 4; g < body; g += 256) *(PQG_G uint32_t*)(dst + head + g) = v;
    const int64_t t0 = head + body;
    if (t0 + ln < len) dst[t0 + ln] = b;
  }
  // out[d + i] = out[d - off + i], i < len in order (off <= d, checked by the decoder)
  __device__ __forceinline__ void out_match(int64_t d, int64_t off, int64_t len) {
    const int64_t src_end = d - off + (len < off ? len : off);
    if (src_end > stored) {
      drain();
      stored = d;
    }
    if (off >= len) {
      copy<true>(out + d, out + (d - off), len);
    } else {
      // overlapping: every source byte lies before d (start + i % offset)
      gcu8 s0 = out + (d - off);
      const uint32_t o = (uint32_t)off;
      for (int64_t i = ln; i < len; i += 64) out[d + i] = (uint8_t)ldb<true>(s0 + (uint32_t)i % o);
    }
  }
};

// the compressed bytes of a page and the size they decode to: V2 pages keep
// their level bytes raw in front of the compressed values (page_v2.go:110-123)
__device__ __forceinline__ void zstd_loc(const PageDev& pg, int64_t* src_off, int64_t* clen, int64_t* ulen) {
  int64_t lv = 0;
  if (pg.page_type == 3) lv = (int64_t)(uint32_t)pg.rep_len + (int64_t)(uint32_t)pg.def_len;
  *src_off = pg.payload_offset + lv;
  *clen = (int64_t)pg.csize - lv;
  *ulen = (int64_t)pg.usize - lv;
}

}  // namespace pqg
