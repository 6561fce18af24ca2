// pqg_lz4.hip — LZ4_RAW pages (K2l): the bare LZ4 block of a page's compressed
// bytes, decoded as liblz4's LZ4_decompress_safe decodes it.  The format logic
// and the library's end-of-block rules are pqg_lz4.h's Decoder, shared with
// the host model (tools/lz4_model.cpp); this file is its IO policy on a wave.
//
// One wave per page, persistent over kQueueLz4.  The decoder state is
// wave-uniform and scalar: the compressed bytes are parsed out of a kLz4Win-byte
// LDS window that the 64 lanes refill together, one aligned 16-byte granule
// each, so a token costs an LDS read and not a dependent trip to HBM; a run of
// 0xff extension bytes is skipped a window at a time.
// Two decoders are built on that, both always compiled (the runtime launches
// k_lz4_batch unless built or told otherwise, pqg_ctx.h PQG_LZ4_BATCH):
//  * k_lz4 (step A): sequences are decoded one at a time and executed by the
//    whole wave.  The latest kLz4Ring output bytes are kept in an LDS ring
//    beside the stored output: a match whose source lies in the ring is copied
//    LDS to LDS and stored; literal runs that lie in the window go from there
//    to the output and the ring; longer ones with pqg_wavecopy.h's dword
//    copies.  A match that reaches further back is copied from the stored
//    output through L2 (pqg_wavecopy.h), after waiting for the wave's stores.
//  * k_lz4_batch (step B): the decoder parses up to 64 sequences ahead
//    (Decoder::batch: only sequences far enough from both ends that liblz4's
//    fast loop decodes them plainly), lane k holding sequence k.  A DPP prefix
//    sum of the lanes' lengths places every sequence; all literal runs of the
//    batch are copied at once, each lane its own; the matches then run in
//    order, consecutive ones that do not overlap themselves and read only
//    below the first of them in one pass after a single wait for the wave's
//    stores, the others by the whole wave.  History is the stored output,
//    read through L2.  What the batch does not take (long literal runs, the
//    sequences near the ends, offset 0, errors) goes one at a time as in step
//    A, without the ring.
// The decoder state lives in registers: every helper of the IO policy is
// inlined, since one out-of-line call made the compiler keep the whole policy
// object in scratch memory, and each parsed byte then cost a round trip there.
// A page whose block does not decode to exactly
// its uncompressed size is walked once more without stores, into a buffer no
// block can fill, to tell a well-formed block of another length (PQG_ERR_SIZE)
// from a malformed one (PQG_ERR_LZ4).  Every read is inside the aligned 16-byte
// granules that hold the page's compressed bytes: up to 15 bytes before the
// first and after the last of them, inside the device allocation by its
// granularity (the convention of the other kernels: a granule that holds a byte
// of the input is mapped).  Every write is inside the page's scratch block.
#include <hip/hip_runtime.h>

#include "pqg_common.h"
#include "pqg_kernels.h"
#include "pqg_device.h"
#include "pqg_lz4.h"
#include "pqg_wavecopy.h"

namespace pqg {

namespace {

// The two decoders (DESIGN.md K2l has both measured).  Step A, k_lz4: one sequence at a time, the
// latest output in an LDS ring.  Step B, k_lz4_batch: up to 64 sequences parsed ahead into lanes and
// executed together, history read from the stored output through L2.  Both are always built;
// PQG_LZ4_BATCH (pqg_ctx.h) says which one the runtime launches by default.

constexpr int kLz4Win = 1024;   // the LDS window of compressed bytes: 64 lanes x 16 bytes
constexpr int kLz4Ring = 4096;  // the LDS ring of the latest output bytes (a power of two)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <bool B>
struct Lz4IO : WaveCopy {  // out: the page's scratch block
  static constexpr int kBatch = B ? 64 : 0;
  gcu8 in;
  int64_t n;
  uint32_t* win;            // LDS, kLz4Win bytes
  int64_t wbase = -kLz4Win;    // the window holds in[wbase, wbase + kLz4Win); none yet

  __device__ __forceinline__ void cnt(int) {}

  // the window from the aligned granule that holds byte i (0 <= i < n) on:
  // a granule is loaded when a byte of the block lies in it
  __device__ __forceinline__ void refill(int64_t i) {
    const uintptr_t a = (uintptr_t)(in + i) & ~(uintptr_t)15;
    wbase = (int64_t)a - (int64_t)(uintptr_t)in;
    const uintptr_t g = a + 16u * (uint32_t)ln;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (g < (uintptr_t)(in + n)) v = *(const PQG_G u32x4*)g;
    __builtin_amdgcn_wave_barrier();  // the lanes' reads of the old window are issued
    ((u32x4*)win)[ln] = v;
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ int byte(int64_t i) {
    if ((uint64_t)i >= (uint64_t)n) return 0;  // never: the decoder's checks come first
    if ((uint64_t)(i - wbase) >= (uint64_t)kLz4Win) refill(i);
    const uint32_t k = (uint32_t)(i - wbase);
    return __builtin_amdgcn_readfirstlane((int)((win[k >> 2] >> (8 * (k & 3))) & 0xff));
  }
  // the 0xff bytes at i, i + 1, ... before `end`: bytewise to a granule of the window, then whole
  // granules, one per lane (a run of extension bytes can be megabytes long)
  __device__ __forceinline__ int64_t run255(int64_t i, int64_t end) {
    int64_t p = i;
    for (;;) {
      // through the granule that holds p
      do {
        if (p >= end || byte(p) != 255) return p - i;
        p++;
      } while ((uintptr_t)(in + p) & 15);
      if (p >= end || byte(p) != 255) return p - i;  // (the window now holds p, a granule's first byte)
      const uint32_t g0 = (uint32_t)(p - wbase) >> 4;
      const int64_t limit = end - wbase;  // granules that end at or before it lie wholly before `end`
      const u32x4 v = ((const u32x4*)win)[ln];
      const bool full = (uint32_t)ln >= g0 && 16 * (int64_t)ln + 16 <= limit && (v.x & v.y & v.z & v.w) == 0xffffffffu;
      const uint64_t rest = ~(__ballot(full) >> g0);  // bit j: granule g0 + j is not such a granule
      p += 16 * (int64_t)(rest ? __builtin_ctzll(rest) : 64);
    }
  }
  // Step A.  The last kLz4Ring output bytes also live in LDS, byte x at hist[x % kLz4Ring]: a match whose source
  // lies there is copied LDS to LDS and stored, with no wait for the wave's stores and no trip to L2.
  uint8_t* hist;

  __device__ __forceinline__ void ring_sync() { __builtin_amdgcn_wave_barrier(); }
  // the ring's copy of out[d..d+len), read back through L2 once the wave's stores have completed
  __device__ __forceinline__ void ring_from_out(int64_t d, int64_t len) {
    drain();
    stored = d + len;
    for (int64_t i = (len > kLz4Ring ? len - kLz4Ring : 0) + ln; i < len; i += 64)
      hist[(uint32_t)(d + i) & (kLz4Ring - 1)] = (uint8_t)ldb<true>(out + d + i);
    ring_sync();
  }
  __device__ __forceinline__ void out_from_in(int64_t d, int64_t s, int64_t len) {
    if constexpr (B) {
      copy<false>(out + d, in + s, len);
      return;
    }
    // literals follow their token: a run that lies in the window goes from there to the output and
    // the ring, with no load from memory for the wave to wait on
    const uint64_t k0 = (uint64_t)(s - wbase);
    if (k0 < (uint64_t)kLz4Win && k0 + (uint64_t)len <= (uint64_t)kLz4Win) {
      for (uint32_t i = (uint32_t)ln; i < (uint32_t)len; i += 64) {
        const uint8_t b = ((const uint8_t*)win)[(uint32_t)k0 + i];
        out[d + i] = b;
        hist[((uint32_t)d + i) & (kLz4Ring - 1)] = b;
      }
      ring_sync();
      return;
    }
    copy<false>(out + d, in + s, len);
    // the ring's share, out of the window where it holds the byte
    for (int64_t i = (len > kLz4Ring ? len - kLz4Ring : 0) + ln; i < len; i += 64) {
      const uint64_t k = (uint64_t)(s + i - wbase);
      const uint32_t b = k < (uint64_t)kLz4Win ? ((const uint8_t*)win)[k] : ldb<false>(in + s + i);
      hist[(uint32_t)(d + i) & (kLz4Ring - 1)] = (uint8_t)b;
    }
    ring_sync();
  }
  __device__ __forceinline__ void out_fill(int64_t d, uint8_t b, int64_t len) {
    WaveCopy::out_fill(d, b, len);
    if constexpr (B) return;
    for (int64_t i = (len > kLz4Ring ? len - kLz4Ring : 0) + ln; i < len; i += 64) hist[(uint32_t)(d + i) & (kLz4Ring - 1)] = b;
    ring_sync();
  }
  // out[d + i] = out[d - off + i], i < len in order (0 < off <= d, checked by the decoder)
  __device__ __forceinline__ void out_match(int64_t d, int64_t off, int64_t len) {
    if constexpr (B) {
      WaveCopy::out_match(d, off, len);
      return;
    }
    if (off + len > kLz4Ring) {  // a source the ring has lost, or would lose while the match is written
      WaveCopy::out_match(d, off, len);
      ring_from_out(d, len);
      return;
    }
    // every source byte lies in [d - off, d), in the ring, and no byte written here falls on one
    const uint32_t o = (uint32_t)off, s0 = (uint32_t)(d - off);
    for (uint32_t i = (uint32_t)ln; i < (uint32_t)len; i += 64) {
      const uint8_t b = hist[(s0 + (o >= (uint32_t)len ? i : i % o)) & (kLz4Ring - 1)];
      out[d + i] = b;
      hist[((uint32_t)d + i) & (kLz4Ring - 1)] = b;
    }
    ring_sync();
  }

  // Step B.  Lane k holds sequence k of the batch: where its literals lie in the input, their count,
  // the offset and the match length.
  int64_t q_ls = 0;
  int32_t q_ll = 0, q_off = 0, q_ml = 0;
  __device__ __forceinline__ void put(int k, int64_t ls, int64_t ll, int64_t off, int64_t ml) {
    if (ln == k) {
      q_ls = ls;
      q_ll = (int32_t)ll;   // <= Decoder::kBatchLit
      q_off = (int32_t)off;  // < 65536
      q_ml = (int32_t)ml;   // the output fits the page: < 2^31
    }
  }
  // Execute sequences 0 .. count-1 from out[d] on.  A prefix sum of the lanes' ll + ml gives every
  // sequence its place.  All literal runs are copied first, each lane its own (they read only the
  // input: out of the window where it holds them).  The matches then run in order, in groups: the
  // consecutive sequences whose matches do not overlap themselves, are at most kGroupMatch bytes long
  // and read only bytes below the group's first match go in one pass, each lane its own, after one
  // wait for the wave's stores; any other match is copied by the whole wave (WaveCopy::out_match).
  static constexpr int kGroupMatch = 64;
  __device__ __forceinline__ static int64_t lane64(int64_t v, int k) {
    return (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, k) |
                     (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), k) << 32);
  }
  __device__ __forceinline__ void exec(int count, int64_t d) {
    const bool mine = ln < count;
    const int32_t ll = mine ? q_ll : 0, ml = mine ? q_ml : 0, off = q_off;
    const int64_t end = d + (int64_t)wave_incl_scan_u64((uint64_t)(uint32_t)(ll + ml));
    const int64_t ld = end - ml - ll, md = end - ml;  // this sequence's literals and match in the output
    int maxll = ll;
    for (int sh = 32; sh; sh >>= 1) maxll = max(maxll, __shfl_xor(maxll, sh));
    for (int i = 0; i < maxll; i++) {
      if (i < ll) {
        const uint64_t k = (uint64_t)(q_ls + i - wbase);
        out[ld + i] = (uint8_t)(k < (uint64_t)kLz4Win ? (uint32_t)((const uint8_t*)win)[k] : ldb<false>(in + q_ls + i));
      }
    }
    int g0 = 0;
    while (g0 < count) {
      g0 = __builtin_amdgcn_readfirstlane(g0);
      const int64_t first = lane64(md, g0);  // the first match of the group
      const bool ok = mine && ln >= g0 && off >= ml && ml <= kGroupMatch && md - off + ml <= first;
      const uint64_t rest = ~(__ballot(ok) >> g0);  // bit j: sequence g0 + j cannot go with the group
      const int g = rest ? __builtin_ctzll(rest) : 64;
      if (g < 2) {  // alone: by the whole wave
        const int64_t md0 = first;
        const int32_t off0 = __builtin_amdgcn_readlane(off, g0), ml0 = __builtin_amdgcn_readlane(ml, g0);
        WaveCopy::out_match(md0, off0, ml0);
        g0 += 1;
        continue;
      }
      drain();  // every store so far, the batch's literals among them
      stored = first;
      const bool in_group = ln >= g0 && ln < g0 + g;
      const int32_t m = in_group ? ml : 0;
      int maxml = m;
      for (int sh = 32; sh; sh >>= 1) maxml = max(maxml, __shfl_xor(maxml, sh));
      gcu8 src = out + (md - off);
      for (int base = 0; base < maxml; base += 8) {
        uint32_t b[8];
#pragma unroll
        for (int j = 0; j < 8; j++) b[j] = base + j < m ? ldb<true>(src + base + j) : 0u;
#pragma unroll
        for (int j = 0; j < 8; j++)
          if (base + j < m) out[md + base + j] = (uint8_t)b[j];
      }
      g0 += g;
    }
  }
};

template <bool B>
__device__ __forceinline__ void lz4_pages(JobDev* jobs, PageDev* pages, const int* list, const int* total, int* queue,
                                          uint8_t* scratch, uint32_t* win, uint8_t* hist) {
  const int lane = lane_id();
  for (;;) {
    const int t = queue_next(queue);
    if (t >= *total) return;
    const int pidx = __builtin_amdgcn_readfirstlane(list[t]);
    const PageDev pg = pages[pidx];
    if (pg.read_status != kOK || pg.scratch_offset < 0) continue;
    const JobDev job = jobs[pg.job];
    if (job.codec != kCodecLz4Raw) continue;
    int64_t so, clen, ulen;
    zstd_loc(pg, &so, &clen, &ulen);
    const bool bare = pg.flags & kPageBareBlock;
    Lz4IO<B> io;
    io.in = gconst(job.data) + so;
    io.n = clen;
    io.out = gmut(scratch) + job.scratch_base + pg.scratch_offset;
    io.ln = lane;
    io.win = win;
    io.hist = hist;
    // a page is decoded as LZ4_decompress_safe decodes it into usize bytes; a
    // bare block as into a buffer no block can fill, storing within the length
    // the host walked (usize)
    const bool sane = clen >= 0 && ulen >= 0;
    int64_t r = -1;
    if (sane) {
      lz4::Decoder<Lz4IO<B>> dec(io, clen, bare ? lz4::max_output(clen) : ulen, ulen, true);
      r = dec.run();
    }
    int e = kOK;
    if (bare) {  // pqg_block_decompress: the decoded length, no size check
      if (r < 0) e = kLZ4;
      else if (lane == 0) pages[pidx].gz_len = r;
    } else if (r != ulen) {
      int64_t R = -1;
      if (clen >= 0) {
        lz4::Decoder<Lz4IO<B>> walk(io, clen, lz4::max_output(clen), lz4::max_output(clen), false);
        R = walk.run();
      }
      e = lz4::page_status(r, R, ulen);  // kSIZE: "decompressed data must be %d byte" (compress.go:117)
    }
    // V1: getValuesDecoder runs after the block is decompressed (page_v1.go:91-97)
    if (e == kOK && pg.page_type == 0 && !values_supported(job.type, job.type_length, pg.encoding)) e = kUNSUPPORTED;
    if (lane == 0 && e != kOK) pages[pidx].read_status = e;
  }
}

}  // namespace

__global__ void __launch_bounds__(64) k_lz4(JobDev* jobs, PageDev* pages, const int* list, const int* total, int* queue,
                                            uint8_t* scratch) {
  __shared__ __attribute__((aligned(16))) uint32_t win[kLz4Win / 4];
  __shared__ __attribute__((aligned(16))) uint8_t hist[kLz4Ring];
  lz4_pages<false>(jobs, pages, list, total, queue, scratch, win, hist);
}

__global__ void __launch_bounds__(64) k_lz4_batch(JobDev* jobs, PageDev* pages, const int* list, const int* total,
                                                  int* queue, uint8_t* scratch) {
  __shared__ __attribute__((aligned(16))) uint32_t win[kLz4Win / 4];
  lz4_pages<true>(jobs, pages, list, total, queue, scratch, win, nullptr);
}

}  // namespace pqg
