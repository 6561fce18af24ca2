// pqg_zstd.hip — ZSTD pages (K2z): the Zstandard frames of a page's compressed
// block (RFC 8878, no dictionaries), decoded as libzstd's ZSTD_decompress
// decodes them.  The format logic is pqg_zstd.h's Decoder, shared with the
// host model (tools/zstd_model.cpp); this file is its IO policy on a wave.
//
// One wave per page, persistent over kQueueZstd.  The decoder state is
// wave-uniform; FSE and Huffman tables live in LDS (zstd::Tables, built by
// lane 0); the four Huffman streams of a literals section are decoded by four
// lanes at once into the wave's literal workspace in HBM (kWsBytes per
// resident wave, planned by the runtime from the grid).  Sequences are decoded
// one at a time and executed by the whole wave (pqg_wavecopy.h): literal runs and matches that
// do not overlap themselves as aligned dwords, one per lane; overlapping
// matches bytewise (source start + i % offset).  History is the page's stored
// output: a match whose source is not known to be stored yet first waits for
// the wave's own stores (s_waitcnt vmcnt(0)) and reads through L2.
// A failed decode ends in PQG_ERR_ZSTD, a page that decodes past or short of
// its uncompressed size in PQG_ERR_SIZE; every read is inside the page's
// compressed bytes, every write inside its scratch block.
#include <hip/hip_runtime.h>

#include "pqg_common.h"
#include "pqg_kernels.h"
#include "pqg_device.h"
#include "pqg_wavecopy.h"
#include "pqg_zstd.h"

namespace pqg {

namespace {

struct ZstdIO : WaveCopy {  // out: the page's scratch block
  typedef gcu8 InP;
  gcu8 in;
  int64_t n;
  gu8 ws;   // this wave's literal workspace

  __device__ __forceinline__ int lane() const { return ln; }
  __device__ __forceinline__ bool owns(int k) const { return ln == k; }
  __device__ __forceinline__ void sync() { __builtin_amdgcn_wave_barrier(); }
  __device__ __forceinline__ int bcast(int v) const { return __builtin_amdgcn_readfirstlane(v); }
  __device__ __forceinline__ bool any(bool b) const { return __ballot(b) != 0; }
  __device__ __forceinline__ void cnt(int) {}
  __device__ __forceinline__ void seqs(int) {}

  __device__ __forceinline__ void out_from_in(int64_t d, int64_t s, int64_t len) { copy<false>(out + d, in + s, len); }
  __device__ __forceinline__ void out_from_ws(int64_t d, int64_t s, int64_t len) { copy<true>(out + d, ws + s, len); }
  __device__ __forceinline__ void ws_put(int64_t i, uint8_t b) { ws[i] = b; }
  __device__ __forceinline__ void ws_done() { drain(); }
  __device__ __forceinline__ int out_get(int64_t i) const { return (int)ldb<true>(out + i); }
};

}  // namespace

__global__ void __launch_bounds__(64) k_zstd(JobDev* jobs, PageDev* pages, const int* list, const int* total, int* queue,
                                             uint8_t* scratch, uint8_t* wspace) {
  __shared__ __attribute__((aligned(16))) zstd::Tables T;
  const int lane = lane_id();
  for (;;) {
    const int t = queue_next(queue);
    if (t >= *total) return;
    const int pidx = __builtin_amdgcn_readfirstlane(list[t]);
    const PageDev pg = pages[pidx];
    if (pg.read_status != kOK || pg.scratch_offset < 0) continue;
    const JobDev job = jobs[pg.job];
    if (job.codec != kCodecZstd) continue;
    int64_t so, clen, ulen;
    zstd_loc(pg, &so, &clen, &ulen);
    const bool bare = pg.flags & kPageBareBlock;
    ZstdIO io;
    io.in = gconst(job.data) + so;
    io.n = clen;
    io.out = gmut(scratch) + job.scratch_base + pg.scratch_offset;
    io.ws = gmut(wspace) + (size_t)blockIdx.x * zstd::kWsBytes;
    io.ln = lane;
    // a page may not decode past its uncompressed size (PQG_ERR_SIZE); a bare
    // block's buffer holds all a valid block decodes to
    zstd::Decoder<ZstdIO> dec(io, &T, ulen, bare ? (int)kZSTD : (int)kSIZE);
    int e = clen < 0 ? (int)kZSTD : dec.run();
    __builtin_amdgcn_wave_barrier();
    if (bare) {  // pqg_block_decompress: the decoded length, no size check
      if (lane == 0) pages[pidx].gz_len = dec.d;
    } else if (e == kOK && dec.d != ulen) {
      e = kSIZE;  // "decompressed data must be %d byte" (compress.go:117)
    }
    // V1: getValuesDecoder runs after the block is decompressed (page_v1.go:91-97)
    if (e == kOK && pg.page_type == 0 && !values_supported(job.type, job.type_length, pg.encoding)) e = kUNSUPPORTED;
    if (lane == 0 && e != kOK) pages[pidx].read_status = e;
  }
}

}  // namespace pqg
