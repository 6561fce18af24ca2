// pqg_lev1_parse.h — run-header parses of the 1-bit whole-page level decoder
// (pqg_lev1.h), in plain C++ operators so that the host compiler takes them
// too (tools/lev1_quad_check.cpp checks l1_quad against l1_hdr on every
// (b0, b1, b2)).
//   l1_hdr   the byte-wise definition: one header of up to 4 bytes, with the
//            checks against the stream's end;
//   l1_quad  four positions at once, one per byte lane of a dword (SWAR):
//            exact for one- and two-byte headers, "far" for everything else.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PQG_HD __host__ __device__ __forceinline__
#else
#define PQG_HD inline
#endif

namespace pqg {

constexpr uint32_t kL1Far = 254, kL1Bad = 255;

struct L1Hdr {
  uint32_t nx;   // position of the next header
  uint32_t cnt;  // values of the run
  uint32_t pay;  // bit-packed: payload position; RLE: the value
  bool bp, bad;
};

// The run header at stream position q (byte q of the stream = the low byte of
// lo, zeros past n): readUVariant32 (helpers.go:149-165) for headers of <= 4
// bytes; 5+ byte headers, EOF inside the header or the RLE value, empty runs
// and RLE values >= 2 are `bad` (the exact decoder settles them).
// lo / hi: stream bytes q..q+3 / q+4..q+7.
PQG_HD L1Hdr l1_hdr(uint32_t lo, uint32_t hi, uint32_t q, uint32_t n) {
  // branch-free (every position of a segment is parsed: divergent bit-packed
  // / RLE branches would run both sides)
  const uint32_t cont = ~lo & 0x80808080u;
  const uint32_t hl = (cont ? (uint32_t)__builtin_ctz(cont) >> 3 : 4u) + 1;  // 5: no terminating byte in four
  const uint32_t hf = (lo & 0x7f) | ((lo >> 1) & 0x3f80) | ((lo >> 2) & 0x1fc000) | ((lo >> 3) & 0xfe00000);
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t h = __builtin_amdgcn_ubfe(hf, 0, 7 * hl);  // hl 5: garbage, and bad below
#else
  const uint32_t h = hl > 4 ? hf : hf & ((1u << (7 * hl)) - 1);
#endif
  const uint32_t g = h >> 1;
  const bool bp = (h & 1) != 0;
  const uint32_t vb = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * hl)) & 0xff;  // the byte after the header
  const uint32_t ve = q + hl;
  L1Hdr r;
  r.bp = bp;
  // readRLERunValue: the value byte must be there and < 2^w (:116-131)
  r.bad = (hl > 4) | (ve > n) | (g == 0) | ((!bp) & ((ve >= n) | (vb > 1)));  // bitwise: no branches
  r.cnt = bp ? g * 8 : g;  // g < 2^27
  r.pay = bp ? ve : vb;
  r.nx = ve + (bp ? g : 1u);
  return r;
}

// ---- four positions per dword ------------------------------------------------
// Byte lane j of b0 / b1 / b2 holds stream byte q0 + j / q0 + j + 1 / q0 + j + 2:
// the first three bytes of the header at position q0 + j.  Per lane:
//   len  nx - q (1..253) of a header that is neither far nor bad;
//   bad  0x80: l1_hdr's `bad` away from the stream's end (an empty run, an RLE
//        value > 1), for one- and two-byte headers;
//   far  0x80: not settled here (a header of 3+ bytes, a two-byte bit-packed
//        header whose successor is 254 or more positions on); `bad` is clear
//        where `far` is set.
// Exact (neither far, nor wrong) for every one-byte header, every two-byte RLE
// header (counts 64..8191) and two-byte bit-packed headers of up to 251
// groups.  The checks against the stream's end are not made: the caller
// parses positions q >= n - 3 with l1_hdr.
// No carry crosses a byte lane: 0xff masks are m | (m - (m >> 7)) on 0x80 bits
// (0x80 - 1 per set lane, 0 - 0 per clear one) and x * 0xff on 0x01 bits; the
// non-zero tests add 0x7f to 7-bit lanes (<= 0xfe); the length adds 1 or 2 to
// a 7-bit lane (<= 0x81) and restores bit 7 with an XOR.
struct L1Quad {
  uint32_t len, bad, far;
};
PQG_HD uint32_t l1q_nz(uint32_t x) {  // bit 7 of every non-zero byte lane (the other bits: garbage)
  return ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x;
}
PQG_HD L1Quad l1_quad(uint32_t b0, uint32_t b1, uint32_t b2) {
  constexpr uint32_t H = 0x80808080u, L7 = 0x7f7f7f7fu, O = 0x01010101u;
  const uint32_t c0 = b0 & H;              // a continuation bit in the first byte
  const uint32_t two = c0 & ~b1;           // bit 7: a header of exactly two bytes
  const uint32_t far3 = c0 & b1;           // bit 7: three bytes or more
  const uint32_t m2 = two | (two - (two >> 7));  // 0xff: two bytes
  const uint32_t bpm = (b0 & O) * 0xffu;   // 0xff: bit-packed
  const uint32_t low = (b0 >> 1) & 0x3f3f3f3fu;  // g's bits 0..5
  const uint32_t b1m = b1 & m2;            // the second header byte (< 0x80), 0 for one-byte headers
  const uint32_t gm = low | ((b1m & 0x03030303u) << 6);  // g's bits 0..7
  const uint32_t gz = ~l1q_nz(low | b1m);  // bit 7: g == 0
  // g >= 252 (len would be >= 254): bits 8.. of g set, or its bits 2..7 all set
  const uint32_t big = l1q_nz(b1m & 0x7c7c7c7cu) | ~l1q_nz(~gm & 0xfcfcfcfcu);
  const uint32_t vb = (b2 & m2) | (b1 & ~m2);  // the byte after the header
  const uint32_t vbig = l1q_nz(vb & 0xfefefefeu);  // bit 7: an RLE value > 1
  L1Quad r;
  r.far = (far3 | (big & bpm)) & H;
  r.bad = (gz | (vbig & ~bpm)) & ~r.far & H;
  // nx - q = header bytes + (bit-packed: g, RLE: 1)
  const uint32_t x = (gm & bpm) | (O & ~bpm);
  r.len = (((x & L7) + O + (two >> 7)) ^ (x & H));
  return r;
}


// The exit codes of the four positions whose successor is not inside the
// segment, and which ones have it inside.  `ed` = e - q0 (4..64), the
// distance from the quad's first position to the segment's end:
//   in    0x80: settled and nx < e (the position takes its successor's code);
//   code  elsewhere: far 254, bad 255, else nx - e (<= 252).
// Lane j's nx - e is len - (ed - j), subtracted with bit 7 set in the minuend
// so that no lane borrows from the next (ed - j is 1..64: its bit 7 is clear);
// the difference's bit 7 is clear exactly where len < 128 borrowed from it,
// that is where len < ed - j.
struct L1Codes {
  uint32_t code, in;
};
PQG_HD L1Codes l1_quad_codes(const L1Quad& h, uint32_t ed) {
  constexpr uint32_t H = 0x80808080u;
  const uint32_t dist = ed * 0x01010101u - 0x03020100u;
  const uint32_t df = (h.len | H) - dist;
  const uint32_t fb = h.far | h.bad;
  const uint32_t fbm = fb | (fb - (fb >> 7));
  L1Codes r;
  r.in = ~h.len & ~df & ~fb & H;
  r.code = ((df ^ (~h.len & H)) & ~fbm) | (fbm ^ (h.far >> 7));
  return r;
}

}  // namespace pqg
