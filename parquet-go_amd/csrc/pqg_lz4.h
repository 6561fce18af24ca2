// pqg_lz4.h — the LZ4 block format (parquet's LZ4_RAW: one bare block, no
// frame, no length prefix, no checksum) as plain __host__ __device__ code.
// k_lz4 (pqg_lz4.hip) and the host model (tools/lz4_model.cpp) run the same
// Decoder; they differ only in the IO policy, which moves the bytes:
//
//   int byte(int64_t i);                 compressed byte i, 0 <= i < n
//   int64_t run255(i, end);              how many bytes of 0xff stand at i, i + 1, ... before `end` (<= n)
//   void out_from_in(d, s, len);         out[d..d+len) = in[s..s+len)
//   void out_fill(d, byte, len);
//   void out_match(d, off, len);         out[d+i] = out[d-off+i], in order
//   void cnt(k);                         feature counter k (the model's)
//   static constexpr int kBatch;         sequences a batch holds (0: one sequence at a time only)
//   void put(k, lit_src, ll, off, ml);   sequence k of the batch being parsed
//   void exec(count, d);                 execute the batch's sequences in order from out[d] on
//
// What is accepted and rejected is what liblz4's LZ4_decompress_safe (1.9.3,
// with its fast decode loop, as built for x86-64) accepts and rejects for an
// output buffer of `cap` bytes; the library has no rule book beyond its code,
// and its verdict depends on which of its loops meets a sequence:
//   * a literal run that ends within 12 bytes of the buffer's end, or within 8
//     bytes of the input's end, must be the last thing in the block and end
//     exactly at the input's end -- but only where the library checks it: a
//     run of < 15 literals whose token lies >= 17 bytes before the input's end
//     (and, in its second loop, >= 32 bytes before the buffer's end) is copied
//     without that check;
//   * a match may not end within the last 5 bytes of the buffer;
//   * an offset beyond the bytes produced so far is an error; an offset of 0
//     is not: the library writes zero bytes for such a match, and so do we;
//   * a literal-length extension whose bytes reach within 15 bytes of the
//     input's end stops there with the length read so far; a match-length
//     extension within 4 bytes of the end is an error;
//   * an empty input is an error; for a buffer of 0 bytes only the block `00`
//     is accepted.
// run() walks the library's own control flow on positions (ip, op), so the
// verdict never depends on the bytes moved, and a walk with store == false
// gives the same verdict and length without touching the output.
//
// All positions and lengths are int64_t: a run of extension bytes can claim
// at most 255 per input byte, and n < 2^31.  (The library sums a length in 32
// bits; the two differ only on inputs with > 16 MiB of 0xff extension bytes.)
#pragma once
#include <stdint.h>

#include "pqg_common.h"

namespace pqg {
namespace lz4 {

constexpr int kErr = -17;  // kLZ4

// the library's constants
constexpr int kMinMatch = 4, kLastLiterals = 5, kMfLimit = 12, kFastSafe = 64;

// the largest output n compressed bytes can decode to, with room to spare
__host__ __device__ inline int64_t max_output(int64_t n) { return 255 * n + 64; }

// feature counters of the model (tools/lz4_model.cpp prints them by name)
enum Feat : int {
  F_LL_0, F_LL_SHORT, F_LL_15, F_LL_EXT1, F_LL_EXT255,
  F_ML_0, F_ML_SHORT, F_ML_15, F_ML_EXT1, F_ML_EXT255,
  F_MATCH_OVERLAP, F_OFF_1, F_OFF_FAR, F_OFF_0, F_LAST_ONLY, F_EMPTY, F_SEQS_GT64,
  F_BATCH,  // a batch of step B executed
  F_GUARD,  // a copy the bounds guard stopped: never, the library's checks come first
  F_COUNT
};

template <class IO>
struct Decoder {
  IO& io;
  const int64_t n;    // compressed bytes
  const int64_t cap;  // the output buffer LZ4_decompress_safe is given: its end sets the end-of-block rules
  const int64_t lim;  // no byte is stored at or past this (<= the real buffer)
  const bool store;
  int64_t ip = 0, op = 0;
  int64_t nseq = 0, lit_bytes = 0, match_bytes = 0;

  __host__ __device__ Decoder(IO& io_, int64_t n_, int64_t cap_, int64_t lim_, bool store_)
      : io(io_), n(n_), cap(cap_), lim(lim_ < cap_ ? lim_ : cap_), store(store_) {}

  __host__ __device__ bool literals(int64_t len) {
    if (len < 0 || ip + len > n || op + len > lim) {
      io.cnt(F_GUARD);
      return false;
    }
    if (store && len) io.out_from_in(op, ip, len);
    lit_bytes += len;
    ip += len;
    op += len;
    return true;
  }
  __host__ __device__ bool match(int64_t off, int64_t len) {
    if (off > op || op + len > lim) {
      io.cnt(F_GUARD);
      return false;
    }
    if (off == 0) {
      io.cnt(F_OFF_0);
      if (store) io.out_fill(op, 0, len);
    } else {
      if (off < len) io.cnt(F_MATCH_OVERLAP);
      if (off == 1) io.cnt(F_OFF_1);
      if (off >= 32768) io.cnt(F_OFF_FAR);
      if (store) io.out_match(op, off, len);
    }
    match_bytes += len;
    op += len;
    nseq++;
    return true;
  }
  __host__ __device__ int64_t rd16(int64_t i) { return (int64_t)io.byte(i) | (int64_t)io.byte(i + 1) << 8; }

  // a literal length's extension: false on the library's "initial" error
  __host__ __device__ bool ll_ext(int64_t* length) {
    // the library reads bytes while they are 255, each at a position before `check`; where the run
    // reaches `check` it stops and goes on with what it has
    const int64_t check = n - 15;
    if (ip >= check) return false;
    const int64_t r = io.run255(ip, check);
    int64_t k = r;
    int s = 255;
    *length += 255 * r;
    ip += r;
    if (ip < check) {
      s = io.byte(ip++);
      *length += s;
      k++;
    }
    io.cnt(k > 1 ? F_LL_EXT255 : s ? F_LL_EXT1 : F_LL_15);
    return true;
  }
  __host__ __device__ bool ml_ext(int64_t* length) {
    // the library reads bytes while they are 255; a byte read at `check` - 1 or past it is an error
    const int64_t check = n - kLastLiterals + 1;
    if (ip >= check - 1) return false;
    const int64_t r = io.run255(ip, check - 1);
    *length += 255 * r;
    ip += r;
    if (ip >= check - 1) return false;
    const int s = io.byte(ip++);
    *length += s;
    io.cnt(r ? F_ML_EXT255 : s ? F_ML_EXT1 : F_ML_15);
    return true;
  }
  __host__ __device__ void cnt_ll(int t) {
    if (t != 15) io.cnt(t ? F_LL_SHORT : F_LL_0);
  }
  __host__ __device__ void cnt_ml(int t) {
    if (t != 15) io.cnt(t ? F_ML_SHORT : F_ML_0);
  }

  __host__ __device__ void cnt_len(int base, int nib, int64_t r, int s) {
    io.cnt(nib != 15 ? base + (nib ? 1 : 0) : base + (r ? 4 : s ? 3 : 2));
  }

  // The batch (step B): parse up to IO::kBatch sequences ahead without executing them, hand them to
  // the IO policy (put) and have it execute them together (exec).  Only sequences that the library's
  // fast loop decodes plainly are taken: far enough from both ends that none of its hand-over or error
  // conditions can fire (the same comparisons as in run(), each one ending the batch instead), with an
  // offset of 1 .. the bytes produced, and literals of at most kBatchLit bytes.  The first sequence
  // that is not such a one ends the batch and is left to run()'s one-at-a-time path, which decides it.
  static constexpr int kBatchLit = 32;
  __host__ __device__ void batch() {
    const int64_t iend = n, oend = cap;
    int k = 0;
    int64_t p = ip, o = op, lits = 0, mats = 0;
    while (k < IO::kBatch) {
      int64_t q = p;
      if (q > iend - 40) break;
      const int t = io.byte(q++);
      int64_t ll = t >> 4, r1 = 0, r2 = 0;
      int s1 = 0, s2 = 0;
      if (ll == 15) {
        if (q >= iend - 15) break;
        r1 = io.run255(q, iend - 15);
        q += r1;
        if (q >= iend - 15) break;
        s1 = io.byte(q++);
        ll += 255 * r1 + s1;
        if (q + ll > iend - 32) break;
      } else if (q > iend - 17) {
        break;
      }
      if (ll > kBatchLit) break;
      const int64_t ls = q;
      q += ll;
      const int64_t off = rd16(q);
      q += 2;
      int64_t ml = t & 15;
      if (ml == 15) {
        if (q >= iend - 5) break;
        r2 = io.run255(q, iend - 5);
        q += r2;
        if (q >= iend - 5) break;
        s2 = io.byte(q++);
        ml += 255 * r2 + s2;
      }
      ml += kMinMatch;
      const int64_t o2 = o + ll;
      if (o2 + ml >= oend - kFastSafe || o2 + ml > lim) break;
      if (off == 0 || off > o2) break;
      cnt_len(F_LL_0, t >> 4, r1, s1);
      cnt_len(F_ML_0, t & 15, r2, s2);
      if (off < ml) io.cnt(F_MATCH_OVERLAP);
      if (off == 1) io.cnt(F_OFF_1);
      if (off >= 32768) io.cnt(F_OFF_FAR);
      io.put(k++, ls, ll, off, ml);
      p = q;
      o = o2 + ml;
      lits += ll;
      mats += ml;
    }
    if (!k) return;
    io.exec(k, op);
    io.cnt(F_BATCH);
    ip = p;
    op = o;
    nseq += k;
    lit_bytes += lits;
    match_bytes += mats;
  }

  // LZ4_decompress_safe(in, out, n, cap): the decoded length, or -1
  __host__ __device__ int64_t run() {
    const int64_t iend = n, oend = cap;
    if (cap == 0) {
      if (n == 1 && io.byte(0) == 0) {
        io.cnt(F_EMPTY);
        return 0;
      }
      return -1;
    }
    if (n == 0) return -1;
    const int64_t shortiend = iend - 14 - 2, shortoend = oend - 14 - 18;
    int64_t length = 0, offset = 0, cpy = 0;
    int token = 0;
    // the steps of one sequence; the library's two loops enter them at different points
    enum { FAST, SAFE, LITERAL, MATCH_EXT, MATCH } at = (oend - op) < kFastSafe ? SAFE : FAST;
    for (;;) {
      if (at == FAST) {
        if (IO::kBatch && store) batch();  // then the next sequence, whatever it is, one at a time
        token = io.byte(ip++);
        length = token >> 4;
        cnt_ll((int)length);
        if (length == 15) {
          if (!ll_ext(&length)) return -1;
          cpy = op + length;
          if (cpy > oend - 32 || ip + length > iend - 32) {
            at = LITERAL;
            continue;
          }
        } else {
          cpy = op + length;
          if (ip > iend - 17) {
            at = LITERAL;
            continue;
          }
        }
        if (!literals(length)) return -1;
        offset = rd16(ip);
        ip += 2;
        length = token & 15;
        cnt_ml((int)length);
        if (length == 15 && !ml_ext(&length)) return -1;
        length += kMinMatch;
        if (op + length >= oend - kFastSafe) {
          at = MATCH;
          continue;
        }
        if (offset > op) return -1;
        if (!match(offset, length)) return -1;
        continue;
      }
      if (at == SAFE) {
        token = io.byte(ip++);
        length = token >> 4;
        cnt_ll((int)length);
        if (length != 15 && ip < shortiend && op <= shortoend) {  // the library's shortcut
          if (!literals(length)) return -1;
          length = token & 15;
          cnt_ml((int)length);
          offset = rd16(ip);
          ip += 2;
          if (length != 15 && offset >= 8 && offset <= op) {
            if (!match(offset, length + kMinMatch)) return -1;
            continue;
          }
          at = MATCH_EXT;
          continue;
        }
        if (length == 15 && !ll_ext(&length)) return -1;
        cpy = op + length;
        at = LITERAL;
      }
      if (at == LITERAL) {
        if (cpy > oend - kMfLimit || ip + length > iend - (2 + 1 + kLastLiterals)) {
          // the last sequence: it consumes the input exactly and fits the buffer
          if (ip + length != iend || cpy > oend) return -1;
          if (!literals(length)) return -1;
          if (nseq == 0) io.cnt(op ? F_LAST_ONLY : F_EMPTY);
          if (nseq > 64) io.cnt(F_SEQS_GT64);
          return op;
        }
        if (!literals(length)) return -1;
        offset = rd16(ip);
        ip += 2;
        length = token & 15;
        cnt_ml((int)length);
        at = MATCH_EXT;
      }
      if (at == MATCH_EXT) {
        if (length == 15 && !ml_ext(&length)) return -1;
        length += kMinMatch;
        at = MATCH;
      }
      // MATCH
      if (offset > op) return -1;
      cpy = op + length;
      if (cpy > oend - kLastLiterals) return -1;  // the last 5 bytes are literals
      if (!match(offset, length)) return -1;
      at = SAFE;
    }
  }
};

// Status of a page whose block should decode to u bytes, by the library's
// verdicts: r = LZ4_decompress_safe into u bytes (the decode), and, when that
// is not u, R = the same into a buffer no block can fill (a walk, nothing
// stored): a well-formed block of another length is kSIZE, all else kErr.
__host__ __device__ inline int page_status(int64_t r, int64_t R, int64_t u) {
  if (r == u) return 0;
  return R >= 0 && R != u ? (int)kSIZE : kErr;
}

// The walk alone over host bytes: the length LZ4_decompress_safe gives into a
// buffer of max_output(n) bytes, or -1.  pqg_block_decompress sizes its device
// buffer with it.
struct WalkIO {
  static constexpr int kBatch = 0;
  void put(int, int64_t, int64_t, int64_t, int64_t) {}
  void exec(int, int64_t) {}
  const uint8_t* in;
  int byte(int64_t i) const { return in[i]; }
  int64_t run255(int64_t i, int64_t end) const {
    int64_t p = i;
    while (p < end && in[p] == 255) p++;
    return p - i;
  }
  void out_from_in(int64_t, int64_t, int64_t) {}
  void out_fill(int64_t, uint8_t, int64_t) {}
  void out_match(int64_t, int64_t, int64_t) {}
  void cnt(int) {}
};
inline int64_t decoded_length(const uint8_t* src, int64_t n) {
  WalkIO io{src};
  Decoder<WalkIO> d(io, n, max_output(n), max_output(n), false);
  return d.run();
}

}  // namespace lz4
}  // namespace pqg
