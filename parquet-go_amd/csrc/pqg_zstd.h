// pqg_zstd.h — the Zstandard frame format (RFC 8878, no dictionaries) as plain
// __host__ __device__ code: the frame, block, literals and sequences header
// parsers, the normalized-count reader, the FSE and Huffman table builds, the
// baseline tables, the repeat-offset update and XXH64.  k_zstd (pqg_zstd.hip)
// and the host model (tools/zstd_model.cpp) run the same Decoder; they differ
// only in the IO policy, which moves the bytes:
//
//   P in; int64_t n;                     the compressed bytes
//   int lane(); void sync();             this lane, a barrier of the lanes
//   bool owns(k);                        this lane decodes Huffman stream k
//   int bcast(int); bool any(bool);      lane 0's value; true on any lane
//   void out_from_in(d, s, len);         out[d..d+len) = in[s..s+len)
//   void out_fill(d, byte, len);
//   void out_from_ws(d, s, len);         from the literal workspace
//   void out_match(d, off, len);         out[d+i] = out[d-off+i], in order
//   void ws_put(i, byte);                one lane: a decoded literal
//   void ws_done();                      the workspace is written
//   int out_get(i);                      a stored output byte (checksum)
//   void cnt(k);                         feature counter k (the model's)
//   void seqs(n);                        a block's sequence count (the model's)
//
// Every lane runs the Decoder with the same state (wave-uniform control
// flow); tables are built by lane 0, Huffman streams are decoded one per lane.
// What is accepted and rejected follows libzstd's ZSTD_decompress (where it is
// laxer than the RFC, so is this: no block-size limit on raw / RLE blocks, no
// window check on offsets, Huffman codes of 12 bits).  One laxity is this
// decoder's own: a compressed block may regenerate more than the block
// maximum; output stays bounded by `cap`.  (The RFC forbids such a block;
// libzstd takes it up to the block maximum + 67 bytes, an accident of where
// it keeps the block's literals.  No writer emits one.  A buffer sized by
// decoded_bound below, as pqg_block_decompress sizes its own, holds the block
// maximum per compressed block: there the bytes past it are an error.)
#pragma once
#include <stdint.h>

#include "pqg_common.h"

#ifdef __HIPCC__
#include "pqg_device.h"
#endif

namespace pqg {
namespace zstd {

constexpr int kErr = -16;  // kZSTD
constexpr int kBlockMax = 131072;
constexpr int kHufLogMax = 12;
constexpr int kWsBytes = kBlockMax + 64;  // literal workspace of one decoder

// feature counters of the model (tools/zstd_model.cpp prints them by name)
enum Feat : int {
  F_BLK_RAW, F_BLK_RLE, F_BLK_COMP,
  F_FRAME_SINGLE, F_FRAME_WINDOW, F_FCS0, F_FCS1, F_FCS2, F_FCS4, F_FCS8, F_FRAME_ONE_BLOCK, F_FRAME_MULTI_BLOCK,
  F_FRAME_CHECKSUM, F_FRAME_SKIP,
  F_LIT_RAW, F_LIT_RLE, F_LIT_HUF1, F_LIT_HUF4, F_LIT_TREELESS1, F_LIT_TREELESS4,
  F_HUF_DIRECT, F_HUF_FSE,
  F_SEQ_NONE, F_SEQ_SHORT, F_SEQ_MID, F_SEQ_LONG,
  F_LL_PREDEF, F_LL_RLE, F_LL_FSE, F_LL_REPEAT,
  F_OF_PREDEF, F_OF_RLE, F_OF_FSE, F_OF_REPEAT,
  F_ML_PREDEF, F_ML_RLE, F_ML_FSE, F_ML_REPEAT,
  F_REP_OFFSET, F_MATCH_OVERLAP,
  F_COUNT
};

struct FseEnt {
  uint8_t sym, nbits;
  uint16_t base;  // next state = base + nbits stream bits
};
struct FseTable {
  int32_t log;
  FseEnt e[512];
};
struct Tables {
  FseTable ll, of, ml;
  uint16_t huf[1 << kHufLogMax];  // the next huf_log stream bits -> nbits << 8 | symbol
  int32_t huf_log;                // 0: no Huffman table yet (a treeless block is an error)
  int32_t fse_valid;              // a block with sequences has set ll / of / ml (Repeat mode)
  // scratch of the table builds
  int16_t norm[256];
  uint16_t next[256];
  uint8_t weights[256];
  uint32_t rank[16];
  FseTable wfse;  // the Huffman weights' FSE table (log <= 6)
};

__host__ __device__ inline int highbit(uint32_t v) { return 31 - __builtin_clz(v); }

// ---- byte access: bytes outside [0, n) read as zero
inline uint64_t load8(const uint8_t* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}
#ifdef __HIPCC__
typedef uint64_t u64_una __attribute__((aligned(1)));
__device__ __forceinline__ uint64_t load8(gcu8 p) { return *(const PQG_G u64_una*)p; }
#endif
template <class P>
__host__ __device__ inline uint64_t rd64(P p, int64_t n, int64_t i) {
  if (i >= 0 && i + 8 <= n) return load8(p + i);
  uint64_t v = 0;
  for (int k = 0; k < 8; k++)
    if (i + k >= 0 && i + k < n) v |= (uint64_t)p[i + k] << (8 * k);
  return v;
}
template <class P>
__host__ __device__ inline uint32_t rd_le(P p, int64_t i, int bytes) {
  uint32_t v = 0;
  for (int k = 0; k < bytes; k++) v |= (uint32_t)p[i + k] << (8 * k);
  return v;
}

// ---- the backward bit stream (RFC 8878 4.1): read from the end, the last
// byte's highest set bit is the padding marker.  pos counts the bits left and
// may go negative: bits before the start read as zero (libzstd's overflow
// state), and every user then requires pos == 0 at its end.
template <class P>
struct BitR {
  P p;
  int64_t n = 0, pos = 0;
  int64_t wbase = 0;  // the cached 64 bits are stream bits [wbase, wbase + 64)
  uint64_t w = 0;
  bool have = false, wrap = false;
  // no_marker_ok: a last byte of 0 starts the stream at its top bit (libzstd's
  // Huffman fast loop takes it so)
  __host__ __device__ bool init(P p_, int64_t n_, bool no_marker_ok = false) {
    p = p_;
    n = n_;
    have = false;
    if (n < 1) return false;
    const uint32_t last = p[n - 1];
    if (!last) {
      pos = n * 8;
      return no_marker_ok;
    }
    pos = (n - 1) * 8 + highbit(last);
    return true;
  }
  __host__ __device__ uint64_t peek(int k) {  // k <= 56
    if (k == 0) return 0;
    // wrap: past the start, libzstd's Huffman tail goes round the first 8 bytes
    const int64_t ep = wrap && pos <= 0 ? 64 - ((-pos) & 63) : pos;
    const int64_t lo = ep - k;
    if (!have || lo < wbase || ep > wbase + 64) {
      wbase = ((ep + 7) & ~(int64_t)7) - 64;
      w = rd64(p, n, wbase >> 3);
      have = true;
    }
    return (w >> (lo - wbase)) & (((uint64_t)1 << k) - 1);
  }
  __host__ __device__ uint64_t bits(int k) {
    const uint64_t v = peek(k);
    pos -= k;
    return v;
  }
};

// ---- normalized counts (RFC 8878 4.1.1, libzstd's FSE_readNCount): returns
// the header's bytes, or -1.  max_sym: the alphabet's last symbol.
template <class P>
__host__ __device__ inline int read_ncount(P p, int64_t n, int max_sym, int max_log, int16_t* norm, int* log_out,
                                           int* nsym_out) {
  int64_t bit = 0;
  auto rb = [&](int k) -> uint32_t {
    const uint32_t v = (uint32_t)((rd64(p, n, bit >> 3) >> (bit & 7)) & (((uint64_t)1 << k) - 1));
    bit += k;
    return v;
  };
  const int log = 5 + (int)rb(4);
  if (log > 15 || log > max_log) return -1;
  int remaining = 1 << log, symb = 0;
  bool prev0 = false;
  while (remaining > 0 && symb <= max_sym) {
    if (prev0) {
      for (;;) {
        const int rep = (int)rb(2);
        for (int i = 0; i < rep; i++, symb++)
          if (symb <= max_sym) norm[symb] = 0;
        if (rep != 3) break;
        if (bit > 8 * n) return -1;
      }
      prev0 = false;
      if (symb > max_sym) break;
    }
    const int nb = highbit((uint32_t)remaining + 1) + 1;
    uint32_t val = rb(nb);
    const uint32_t lower = (1u << (nb - 1)) - 1;
    const uint32_t threshold = (1u << nb) - 1 - ((uint32_t)remaining + 1);
    if ((val & lower) < threshold) {
      bit--;
      val &= lower;
    } else if (val > lower) {
      val -= threshold;
    }
    const int proba = (int)val - 1;
    remaining -= proba < 0 ? 1 : proba;
    norm[symb++] = (int16_t)proba;
    prev0 = proba == 0;
    if (bit > 8 * n) return -1;
  }
  if (remaining != 0 || symb > max_sym + 1) return -1;
  const int64_t used = (bit + 7) >> 3;
  if (used > n) return -1;
  *log_out = log;
  *nsym_out = symb;
  return (int)used;
}

// ---- FSE decoding table (RFC 8878 4.1.1) from norm[0..nsym)
__host__ __device__ inline void fse_build(FseTable* t, const int16_t* norm, int nsym, int log, uint16_t* next) {
  const int size = 1 << log, mask = size - 1;
  int high = size;
  for (int s = 0; s < nsym; s++)
    if (norm[s] == -1) {
      t->e[--high].sym = (uint8_t)s;
      next[s] = 1;
    }
  const int step = (size >> 1) + (size >> 3) + 3;
  int pos = 0;
  for (int s = 0; s < nsym; s++) {
    if (norm[s] <= 0) continue;
    next[s] = (uint16_t)norm[s];
    for (int i = 0; i < norm[s]; i++) {
      t->e[pos].sym = (uint8_t)s;
      do pos = (pos + step) & mask;
      while (pos >= high);
    }
  }
  for (int i = 0; i < size; i++) {
    const int s = t->e[i].sym;
    const uint32_t nx = next[s]++;
    const int nb = log - highbit(nx);
    t->e[i].nbits = (uint8_t)nb;
    t->e[i].base = (uint16_t)((nx << nb) - (uint32_t)size);
  }
  t->log = log;
}
__host__ __device__ inline void fse_rle(FseTable* t, int sym) {
  t->log = 0;
  t->e[0].sym = (uint8_t)sym;
  t->e[0].nbits = 0;
  t->e[0].base = 0;
}

// ---- baselines (RFC 8878 3.1.1.3.2.1.1) and default distributions (3.1.1.3.2.2)
constexpr int kMaxLL = 35, kMaxML = 52, kMaxOF = 31;
__host__ __device__ inline uint32_t ll_base(int c) { return c < 16 ? (uint32_t)c : c < 18 ? 16u + 2u * (c - 16) : c < 20 ? 20u + 2u * (c - 18) : c < 22 ? 24u + 4u * (c - 20) : c < 24 ? 32u + 8u * (c - 22) : c == 24 ? 48u : 1u << (c - 19); }
__host__ __device__ inline int ll_bits(int c) { return c < 16 ? 0 : c < 20 ? 1 : c < 22 ? 2 : c < 24 ? 3 : c == 24 ? 4 : c - 19; }
__host__ __device__ inline uint32_t ml_base(int c) {
  return c < 32 ? (uint32_t)c + 3 : c < 34 ? 35u + 2u * (c - 32) : c < 36 ? 39u + 2u * (c - 34) : c < 38 ? 43u + 4u * (c - 36) : c < 40 ? 51u + 8u * (c - 38)
         : c < 42 ? 67u + 16u * (c - 40) : c == 42 ? 99u : (1u << (c - 36)) + 3u;
}
__host__ __device__ inline int ml_bits(int c) { return c < 32 ? 0 : c < 36 ? 1 : c < 38 ? 2 : c < 40 ? 3 : c < 42 ? 4 : c == 42 ? 5 : c - 36; }
__host__ __device__ inline int default_norm(int which, int s) {  // 0 LL (log 6), 1 OF (log 5), 2 ML (log 6)
  if (which == 0) return s == 0 ? 4 : s == 1 || s == 25 ? 3 : s >= 32 ? -1 : (s >= 13 && s <= 15) || s >= 27 ? 1 : 2;
  if (which == 1) return s >= 24 ? -1 : s >= 6 && s <= 8 ? 2 : 1;
  return s == 0 ? 1 : s == 1 ? 4 : s == 2 ? 3 : s <= 8 ? 2 : s >= 46 ? -1 : 1;
}

// ---- the repeat offsets (RFC 8878 3.1.1.5, libzstd's ZSTD_decodeSequence):
// of_code 0 / 1 with their one extra bit pick a repeat offset, shifted by one
// when the literal length is 0; anything else is a new offset.  Returns the
// offset, 0: rep1 - 1 == 0 (corrupt).
__host__ __device__ inline uint64_t rep_update(uint64_t rep[3], int of_code, uint64_t of_extra, bool ll0) {
  if (of_code > 1) {
    const uint64_t off = (((uint64_t)1 << of_code) - 3) + of_extra;
    rep[2] = rep[1];
    rep[1] = rep[0];
    rep[0] = off;
    return off;
  }
  if (of_code == 0) {
    const uint64_t off = rep[ll0 ? 1 : 0];
    rep[1] = rep[ll0 ? 0 : 1];
    rep[0] = off;
    return off;
  }
  const int idx = 1 + (ll0 ? 1 : 0) + (int)of_extra;  // 1 rep2, 2 rep3, 3 rep1 - 1
  const uint64_t off = idx == 3 ? rep[0] - 1 : rep[idx];
  if (off == 0) return 0;
  if (idx != 1) rep[2] = rep[1];
  rep[1] = rep[0];
  rep[0] = off;
  return off;
}

// ---- XXH64, seed 0, over bytes get(0..len)
template <class G>
__host__ __device__ inline uint64_t xxh64(G get, int64_t len) {
  const uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull,
                 P4 = 0x85EBCA77C2B2AE63ull, P5 = 0x27D4EB2F165667C5ull;
  auto rotl = [](uint64_t x, int r) { return (x << r) | (x >> (64 - r)); };
  auto rd = [&](int64_t i, int nb) {
    uint64_t v = 0;
    for (int k = 0; k < nb; k++) v |= (uint64_t)(uint8_t)get(i + k) << (8 * k);
    return v;
  };
  auto round = [&](uint64_t acc, uint64_t x) { return rotl(acc + x * P2, 31) * P1; };
  int64_t i = 0;
  uint64_t h;
  if (len >= 32) {
    uint64_t v1 = P1 + P2, v2 = P2, v3 = 0, v4 = 0 - P1;
    for (; i + 32 <= len; i += 32) {
      v1 = round(v1, rd(i, 8));
      v2 = round(v2, rd(i + 8, 8));
      v3 = round(v3, rd(i + 16, 8));
      v4 = round(v4, rd(i + 24, 8));
    }
    h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
    h = (h ^ round(0, v1)) * P1 + P4;
    h = (h ^ round(0, v2)) * P1 + P4;
    h = (h ^ round(0, v3)) * P1 + P4;
    h = (h ^ round(0, v4)) * P1 + P4;
  } else {
    h = P5;
  }
  h += (uint64_t)len;
  for (; i + 8 <= len; i += 8) h = rotl(h ^ round(0, rd(i, 8)), 27) * P1 + P4;
  if (i + 4 <= len) {
    h = rotl(h ^ (rd(i, 4) * P1), 23) * P2 + P3;
    i += 4;
  }
  for (; i < len; i++) h = rotl(h ^ (rd(i, 1) * P5), 11) * P1;
  h ^= h >> 33;
  h *= P2;
  h ^= h >> 29;
  h *= P3;
  h ^= h >> 32;
  return h;
}

// ---- Huffman weights -> decoding table (RFC 8878 4.2.1, libzstd's
// HUF_readStats + HUF_readDTableX1).  p[0..n): the tree description and what
// follows it.  Returns the description's bytes, or -1.
template <class P>
__host__ __device__ inline int huf_read_table(P p, int64_t n, Tables* T, bool* direct) {
  if (n < 1) return -1;
  int hb = p[0], nw, used;
  uint8_t* W = T->weights;
  if (hb >= 128) {
    nw = hb - 127;
    const int bytes = (nw + 1) / 2;
    if (bytes + 1 > n) return -1;
    for (int i = 0; i < nw; i++) W[i] = (i & 1) ? (p[1 + i / 2] & 15) : (p[1 + i / 2] >> 4);
    used = 1 + bytes;
    *direct = true;
  } else {
    if (hb + 1 > n) return -1;
    *direct = false;
    int log, nsym;
    const int h = read_ncount(p + 1, (int64_t)hb, 255, 6, T->norm, &log, &nsym);
    if (h < 0) return -1;
    fse_build(&T->wfse, T->norm, nsym, log, T->next);
    // two interleaved states over the rest of the hb bytes (libzstd's
    // FSE_decompress_usingDTable): ends when a state update runs out of bits
    BitR<P> b;
    if (!b.init(p + 1 + h, (int64_t)hb - h)) return -1;
    uint32_t s1 = (uint32_t)b.bits(log), s2 = (uint32_t)b.bits(log);
    nw = 0;
    for (;;) {
      if (nw > 253) return -1;
      W[nw++] = T->wfse.e[s1].sym;
      s1 = T->wfse.e[s1].base + (uint32_t)b.bits(T->wfse.e[s1].nbits);
      if (b.pos < 0) {
        W[nw++] = T->wfse.e[s2].sym;
        break;
      }
      if (nw > 253) return -1;
      W[nw++] = T->wfse.e[s2].sym;
      s2 = T->wfse.e[s2].base + (uint32_t)b.bits(T->wfse.e[s2].nbits);
      if (b.pos < 0) {
        W[nw++] = T->wfse.e[s1].sym;
        break;
      }
    }
    used = 1 + hb;
  }
  uint32_t* rank = T->rank;
  for (int i = 0; i < 16; i++) rank[i] = 0;
  uint32_t total = 0;
  for (int i = 0; i < nw; i++) {
    if (W[i] > kHufLogMax) return -1;
    rank[W[i]]++;
    total += (1u << W[i]) >> 1;
  }
  if (total == 0) return -1;
  const int log = highbit(total) + 1;
  if (log > kHufLogMax) return -1;
  const uint32_t rest = (1u << log) - total;
  if (rest & (rest - 1)) return -1;  // the last weight must be a power of two
  const int lastw = highbit(rest) + 1;
  W[nw++] = (uint8_t)lastw;
  rank[lastw]++;
  if (rank[1] < 2 || (rank[1] & 1)) return -1;
  // first table slot of each weight, then every symbol's 2^(w-1) slots
  uint32_t start = 0;
  for (int w = 1; w <= log; w++) {
    const uint32_t c = rank[w];
    rank[w] = start;
    start += c << (w - 1);
  }
  for (int s = 0; s < nw; s++) {
    const int w = W[s];
    if (!w) continue;
    const uint32_t len = 1u << (w - 1);
    const uint16_t ent = (uint16_t)((log + 1 - w) << 8 | s);
    for (uint32_t k = 0; k < len; k++) T->huf[rank[w] + k] = ent;
    rank[w] += len;
  }
  T->huf_log = log;
  return used;
}

struct FrameHdr {
  int hsize;  // header bytes (magic included)
  int checksum, single;
  int fcs_bytes;
  uint64_t fcs;     // valid when fcs_bytes != 0
  uint64_t window;  // bytes
};
// the frame header at p (n >= 5 bytes, magic checked): 0, or -1
template <class P>
__host__ __device__ inline int parse_frame_header(P p, int64_t n, FrameHdr* h) {
  const int fhd = p[4];
  const int did = fhd & 3, fid = fhd >> 6;
  h->checksum = (fhd >> 2) & 1;
  h->single = (fhd >> 5) & 1;
  const int didb = did == 3 ? 4 : did;
  h->fcs_bytes = fid == 0 ? h->single : fid == 1 ? 2 : fid == 2 ? 4 : 8;
  h->hsize = 5 + !h->single + didb + h->fcs_bytes;
  if (n < h->hsize) return -1;
  if (fhd & 8) return -1;  // reserved bit
  int64_t q = 5;
  h->window = 0;
  if (!h->single) {
    const int wl = p[q++];
    const int wlog = (wl >> 3) + 10;
    if (wlog > 31) return -1;
    h->window = ((uint64_t)1 << wlog) + (((uint64_t)1 << wlog) >> 3) * (wl & 7);
  }
  if (rd_le(p, q, didb) != 0) return -1;  // a dictionary
  q += didb;
  h->fcs = 0;
  if (h->fcs_bytes == 8) h->fcs = (uint64_t)rd_le(p, q, 4) | (uint64_t)rd_le(p, q + 4, 4) << 32;
  else if (h->fcs_bytes) h->fcs = rd_le(p, q, h->fcs_bytes) + (h->fcs_bytes == 2 ? 256u : 0u);
  if (h->single) h->window = h->fcs;
  return 0;
}

struct LitHdr {
  int type;     // 0 raw, 1 RLE, 2 Huffman, 3 treeless
  int lh;       // header bytes
  int streams;  // Huffman: 1 or 4
  uint32_t size, csize;
};
// literals section header of a compressed block p[0..n): 0, or -1
template <class P>
__host__ __device__ inline int parse_lit_header(P p, int64_t n, LitHdr* h) {
  if (n < 2) return -1;
  const int b0 = p[0], sf = (b0 >> 2) & 3;
  h->type = b0 & 3;
  h->streams = 1;
  if (h->type >= 2) {
    if (n < 5) return -1;
    const uint32_t v = rd_le(p, 0, 4);
    h->streams = sf == 0 ? 1 : 4;
    if (sf <= 1) {
      h->lh = 3;
      h->size = (v >> 4) & 0x3ff;
      h->csize = (v >> 14) & 0x3ff;
    } else if (sf == 2) {
      h->lh = 4;
      h->size = (v >> 4) & 0x3fff;
      h->csize = v >> 18;
    } else {
      h->lh = 5;
      h->size = (v >> 4) & 0x3ffff;
      h->csize = (v >> 22) + ((uint32_t)p[4] << 10);
    }
    return 0;
  }
  if (sf == 1) {
    h->lh = 2;
    h->size = rd_le(p, 0, 2) >> 4;
  } else if (sf == 3) {
    if (n < 3) return -1;
    h->lh = 3;
    h->size = rd_le(p, 0, 3) >> 4;
  } else {
    h->lh = 1;
    h->size = (uint32_t)b0 >> 3;
  }
  h->csize = h->type == 1 ? 1 : h->size;
  return 0;
}

// sequences section header: the count and the modes byte.  Returns the bytes
// used (the modes byte included when nseq > 0), or -1.
template <class P>
__host__ __device__ inline int parse_seq_header(P p, int64_t n, int* nseq, int* modes, int* form) {
  if (n < 1) return -1;
  int q = 1, ns = p[0];
  *form = 0;
  if (ns > 0x7f) {
    if (ns == 0xff) {
      if (n < 3) return -1;
      ns = (int)rd_le(p, 1, 2) + 0x7f00;
      q = 3;
      *form = 2;
    } else {
      if (n < 2) return -1;
      ns = ((ns - 0x80) << 8) + p[1];
      q = 2;
      *form = 1;
    }
  }
  *nseq = ns;
  *modes = 0;
  if (ns == 0) return q == n ? q : -1;  // nothing may follow
  if (q + 1 > n) return -1;
  *modes = p[q++];
  if (*modes & 3) return -1;  // reserved
  return q;
}

template <class IO>
struct Decoder {
  IO& io;
  Tables* T;
  int64_t cap;   // bytes the output holds
  int ovf;       // status when the output would pass cap
  int64_t d = 0; // decoded bytes
  int64_t fstart = 0;  // first output byte of the frame
  uint64_t rep[3];
  uint32_t block_max = kBlockMax;
  typedef typename IO::InP P;

  __host__ __device__ Decoder(IO& io_, Tables* T_, int64_t cap_, int ovf_) : io(io_), T(T_), cap(cap_), ovf(ovf_) {}

  // one sequence table (RFC 8878 3.1.1.3.2.1): bytes used, or -1
  __host__ __device__ int seq_table(int which, int mode, P p, int64_t n) {
    FseTable* t = which == 0 ? &T->ll : which == 1 ? &T->of : &T->ml;
    const int max_sym = which == 0 ? kMaxLL : which == 1 ? kMaxOF : kMaxML;
    io.cnt((which == 0 ? F_LL_PREDEF : which == 1 ? F_OF_PREDEF : F_ML_PREDEF) + mode);
    if (mode == 3) return T->fse_valid ? 0 : -1;
    if (mode == 1) {
      if (n < 1 || p[0] > max_sym) return -1;
      if (io.lane() == 0) fse_rle(t, p[0]);
      return 1;
    }
    int r = 0;
    if (io.lane() == 0) {
      if (mode == 0) {
        const int ns = which == 0 ? 36 : which == 1 ? 29 : 53;
        for (int s = 0; s < ns; s++) T->norm[s] = (int16_t)default_norm(which, s);
        fse_build(t, T->norm, ns, which == 1 ? 5 : 6, T->next);
      } else {
        int log, nsym;
        r = read_ncount(p, n, max_sym, which == 1 ? 8 : 9, T->norm, &log, &nsym);
        if (r >= 0) fse_build(t, T->norm, nsym, log, T->next);
      }
    }
    return io.bcast(r);
  }

  // one Huffman stream p[0..n) into ws[at..at+count): false when it is corrupt
  // libzstd checks that a stream is consumed exactly only where its fast
  // loop does not run: one stream, or four with one shorter than 8 bytes.
  // In the fast loop (below >= 0: the bytes of the jump table and the earlier
  // streams under this one) a stream may end early, or read on into the
  // bytes below its start (checked: by at most 8 of them), and below the jump
  // table round its first 8 bytes; the model follows it.
  __host__ __device__ bool huf_stream(P p, int64_t n, int64_t at, int64_t count, int64_t below = -1) {
    BitR<P> b;
    if (n < 1) return false;
    const bool lax = below >= 0;
    if (!lax) below = 0;
    if (!b.init(p - below, n + below, lax)) return false;
    b.wrap = lax;
    const int log = T->huf_log;
    const uint16_t* H = T->huf;
    for (int64_t i = 0; i < count; i++) {
      const uint32_t e = H[b.peek(log)];
      b.pos -= e >> 8;
      io.ws_put(at + i, (uint8_t)e);
    }
    return lax ? b.pos >= below * 8 - 64 : b.pos == 0;
  }

  // a compressed block p[0..n) (RFC 8878 3.1.1.2)
  __host__ __device__ int block(P p, int64_t n) {
    if (n > (int64_t)block_max) return kErr;
    LitHdr lh;
    if (parse_lit_header(p, n, &lh)) return kErr;
    if (lh.size > block_max) return kErr;
    if ((int64_t)lh.lh + lh.csize > n) return kErr;
    if (d + (int64_t)lh.size > cap) return ovf;
    int lit_kind = lh.type;  // 0: in the input, 1: one byte, 2: the workspace
    int64_t lit_in = 0;
    int lit_byte = 0;
    if (lh.type == 0) {
      io.cnt(F_LIT_RAW);
      lit_in = lh.lh;
    } else if (lh.type == 1) {
      io.cnt(F_LIT_RLE);
      lit_byte = p[lh.lh];
    } else {
      lit_kind = 2;
      if (lh.streams == 4 && lh.size < 6) return kErr;
      if (lh.size == 0 || lh.csize == 0) return kErr;
      P hp = p + lh.lh;
      int64_t hn = lh.csize;
      if (lh.type == 3) {
        if (!T->huf_log) return kErr;
        io.cnt(lh.streams == 1 ? F_LIT_TREELESS1 : F_LIT_TREELESS4);
      } else {
        io.cnt(lh.streams == 1 ? F_LIT_HUF1 : F_LIT_HUF4);
        int used = 0;
        bool direct = false;
        io.sync();
        if (io.lane() == 0) {
          used = huf_read_table(hp, hn, T, &direct);
          if (used < 0) T->huf_log = 0;
        }
        used = io.bcast(used);
        io.sync();
        if (used < 0 || used >= hn) return kErr;
        io.cnt(io.bcast(direct) ? F_HUF_DIRECT : F_HUF_FSE);
        hp = hp + used;
        hn -= used;
      }
      bool ok = true;
      if (lh.streams == 1) {
        if (io.lane() == 0) ok = huf_stream(hp, hn, 0, lh.size);
      } else {
        if (hn < 10) return kErr;
        const int64_t l1 = rd_le(hp, 0, 2), l2 = rd_le(hp, 2, 2), l3 = rd_le(hp, 4, 2);
        if (6 + l1 + l2 + l3 > hn) return kErr;
        const int64_t l4 = hn - 6 - l1 - l2 - l3;
        const int64_t seg = ((int64_t)lh.size + 3) / 4;
        if (3 * seg > (int64_t)lh.size) return kErr;
        for (int k = 0; k < 4; k++) {
          if (!io.owns(k)) continue;
          const int64_t so = 6 + (k > 0 ? l1 : 0) + (k > 1 ? l2 : 0) + (k > 2 ? l3 : 0);
          const int64_t sl = k == 0 ? l1 : k == 1 ? l2 : k == 2 ? l3 : l4;
          const bool fast = l1 >= 8 && l2 >= 8 && l3 >= 8 && l4 >= 8;
          ok = huf_stream(hp + so, sl, seg * k, k < 3 ? seg : (int64_t)lh.size - 3 * seg, fast ? so : -1) && ok;
        }
      }
      io.ws_done();
      if (io.any(!ok)) return kErr;
    }
    // ---- sequences
    P sp = p + lh.lh + lh.csize;
    int64_t sn = n - lh.lh - lh.csize;
    int nseq, modes, form;
    int q = parse_seq_header(sp, sn, &nseq, &modes, &form);
    if (q < 0) return kErr;
    int64_t lp = 0;  // literals used
    auto lits = [&](int64_t len) {
      if (len <= 0) return;
      if (lit_kind == 0) io.out_from_in(d, (p - io.in) + lit_in + lp, len);
      else if (lit_kind == 1) io.out_fill(d, (uint8_t)lit_byte, len);
      else io.out_from_ws(d, lp, len);
      d += len;
      lp += len;
    };
    io.seqs(nseq);
    if (nseq == 0) {
      io.cnt(F_SEQ_NONE);
    } else {
      io.cnt(form == 0 ? F_SEQ_SHORT : form == 1 ? F_SEQ_MID : F_SEQ_LONG);
      io.sync();
      for (int t = 0; t < 3; t++) {
        const int r = seq_table(t, (modes >> (6 - 2 * t)) & 3, sp + q, sn - q);
        if (r < 0) return kErr;
        q += r;
      }
      T->fse_valid = 1;  // every lane stores the same value
      io.sync();
      BitR<P> b;
      if (!b.init(sp + q, sn - q)) return kErr;
      const FseTable *LL = &T->ll, *OF = &T->of, *ML = &T->ml;
      uint32_t sl = (uint32_t)b.bits(LL->log), so = (uint32_t)b.bits(OF->log), sm = (uint32_t)b.bits(ML->log);
      for (int i = 0; i < nseq; i++) {
        const FseEnt el = LL->e[sl], eo = OF->e[so], em = ML->e[sm];
        const uint64_t ofx = b.bits(eo.sym);
        const uint64_t ml = ml_base(em.sym) + b.bits(ml_bits(em.sym));
        const uint64_t ll = ll_base(el.sym) + b.bits(ll_bits(el.sym));
        if (eo.sym <= 1) io.cnt(F_REP_OFFSET);
        const uint64_t off = rep_update(rep, eo.sym, ofx, ll == 0);
        if (off == 0) return kErr;
        if (i + 1 < nseq) {
          sl = el.base + (uint32_t)b.bits(el.nbits);
          sm = em.base + (uint32_t)b.bits(em.nbits);
          so = eo.base + (uint32_t)b.bits(eo.nbits);
        }
        if (b.pos < 0) return kErr;
        if ((int64_t)ll > (int64_t)lh.size - lp) return kErr;
        if (d + (int64_t)(ll + ml) > cap) return ovf;
        lits((int64_t)ll);
        if (off > (uint64_t)(d - fstart)) return kErr;
        if (off < ml) io.cnt(F_MATCH_OVERLAP);
        io.out_match(d, (int64_t)off, (int64_t)ml);
        d += (int64_t)ml;
      }
      if (b.pos != 0) return kErr;
    }
    if (d + ((int64_t)lh.size - lp) > cap) return ovf;
    lits((int64_t)lh.size - lp);
    return kOK;
  }

  // one frame at in[ip..): 0 and *ip past it, or a status
  __host__ __device__ int frame(int64_t* ipp) {
    int64_t ip = *ipp;
    const int64_t n = io.n;
    FrameHdr fh;
    if (parse_frame_header(io.in + ip, n - ip, &fh)) return kErr;
    io.cnt(fh.single ? F_FRAME_SINGLE : F_FRAME_WINDOW);
    io.cnt(fh.fcs_bytes == 0 ? F_FCS0 : fh.fcs_bytes == 1 ? F_FCS1 : fh.fcs_bytes == 2 ? F_FCS2 : fh.fcs_bytes == 4 ? F_FCS4 : F_FCS8);
    ip += fh.hsize;
    block_max = fh.window < (uint64_t)kBlockMax ? (uint32_t)fh.window : (uint32_t)kBlockMax;
    fstart = d;
    rep[0] = 1;
    rep[1] = 4;
    rep[2] = 8;
    io.sync();
    if (io.lane() == 0) {
      T->huf_log = 0;
      T->fse_valid = 0;
    }
    io.sync();
    int nblocks = 0;
    for (;;) {
      if (n - ip < 3) return kErr;
      const uint32_t bh = rd_le(io.in, ip, 3);
      const int last = bh & 1, type = (bh >> 1) & 3;
      const int64_t bsz = bh >> 3;
      ip += 3;
      if (type == 3) return kErr;
      const int64_t csz = type == 1 ? 1 : bsz;
      if (csz > n - ip) return kErr;
      nblocks++;
      if (type == 2) {
        io.cnt(F_BLK_COMP);
        const int e = block(io.in + ip, csz);
        if (e) return e;
      } else {
        io.cnt(type == 0 ? F_BLK_RAW : F_BLK_RLE);
        if (d + bsz > cap) return ovf;
        if (type == 0) io.out_from_in(d, ip, bsz);
        else io.out_fill(d, io.in[ip], bsz);
        d += bsz;
      }
      ip += csz;
      if (last) break;
    }
    io.cnt(nblocks == 1 ? F_FRAME_ONE_BLOCK : F_FRAME_MULTI_BLOCK);
    if (fh.fcs_bytes && (uint64_t)(d - fstart) != fh.fcs) return kErr;
    if (fh.checksum) {
      io.cnt(F_FRAME_CHECKSUM);
      if (n - ip < 4) return kErr;
      const int64_t f0 = fstart;
      IO& o = io;
      const uint64_t h = xxh64([&](int64_t i) { return o.out_get(f0 + i); }, d - fstart);
      if ((uint32_t)h != rd_le(io.in, ip, 4)) return kErr;
      ip += 4;
    }
    *ipp = ip;
    return kOK;
  }

  // frames and skippable frames until the input ends (ZSTD_decompress)
  __host__ __device__ int run() {
    int64_t ip = 0;
    const int64_t n = io.n;
    while (n - ip >= 5) {
      const uint32_t magic = rd_le(io.in, ip, 4);
      if ((magic & 0xfffffff0u) == 0x184d2a50u) {
        if (n - ip < 8) return kErr;
        const int64_t sz = 8 + (int64_t)rd_le(io.in, ip + 4, 4);
        if (sz > n - ip) return kErr;
        ip += sz;
        io.cnt(F_FRAME_SKIP);
        continue;
      }
      if (magic != 0xfd2fb528u) return kErr;
      const int e = frame(&ip);
      if (e) return e;
    }
    return ip == n ? kOK : kErr;
  }
};

// An upper bound of what in[0..n) decodes to (frame content sizes where every
// frame declares one, else per block: its size, or the block maximum), for
// sizing an output buffer before the decode; *exact: every frame declared its
// size.  A malformed input ends the walk: the decoder reports it.
inline int64_t decoded_bound(const uint8_t* in, int64_t n, bool* exact) {
  int64_t ip = 0, total = 0;
  *exact = true;
  while (n - ip >= 5) {
    const uint32_t magic = rd_le(in, ip, 4);
    if ((magic & 0xfffffff0u) == 0x184d2a50u) {
      if (n - ip < 8) break;
      const int64_t sz = 8 + (int64_t)rd_le(in, ip + 4, 4);
      if (sz > n - ip) break;
      ip += sz;
      continue;
    }
    FrameHdr fh;
    if (magic != 0xfd2fb528u || parse_frame_header(in + ip, n - ip, &fh)) break;
    ip += fh.hsize;
    int64_t sum = 0;
    bool ok = false;
    for (;;) {
      if (n - ip < 3) break;
      const uint32_t bh = rd_le(in, ip, 3);
      const int type = (bh >> 1) & 3;
      const int64_t bsz = bh >> 3, csz = type == 1 ? 1 : bsz;
      ip += 3;
      if (type == 3 || csz > n - ip) break;
      sum += type == 2 ? kBlockMax : bsz;
      ip += csz;
      if (bh & 1) {
        ok = true;
        break;
      }
    }
    if (fh.fcs_bytes && fh.fcs < (uint64_t)sum) sum = (int64_t)fh.fcs;
    if (!fh.fcs_bytes) *exact = false;
    total += sum;
    if (!ok) break;
    if (fh.checksum) ip += 4;
  }
  return total;
}

}  // namespace zstd
}  // namespace pqg
