// lev1_quad_check — host check of the four-positions-per-dword header parse
// (l1_quad, pqg_lev1_parse.h) against the byte-wise l1_hdr on all 2^24 values
// of a header's first three bytes (b0, b1, b2), in each byte lane, with the
// other three lanes holding 0x00, 0xff and random bytes (a carry across a
// lane would show), and on dwords of four random headers.
//   "ok" (neither far nor bad) must give l1_hdr's nx and not-bad;
//   "bad" must be l1_hdr bad;
//   every one-byte header, every two-byte RLE header and every two-byte
//   bit-packed header of up to 251 groups must be settled (not far), and ok
//   exactly when l1_hdr is not bad;
//   the exit codes (l1_quad_codes) at a random distance from the segment's
//   end: far 254, bad 255, else nx - e, and "in" exactly for nx < e.
// Build: c++ -O2 -std=c++17 -I parquet-go_amd/csrc tools/lev1_quad_check.cpp
#include <cstdint>
#include <cstdio>

#include "pqg_lev1_parse.h"

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

long errors = 0;
void fail(const char* what, uint32_t b0, uint32_t b1, uint32_t b2, int lane, uint32_t fill) {
  if (errors++ < 20) std::printf("FAIL %s: b0=%02x b1=%02x b2=%02x lane=%d fill=%08x\n", what, b0, b1, b2, lane, fill);
}

// lane `lane` of the quad parse of (w0, w1, w2) against l1_hdr on (b0, b1, b2, b3..)
void check_lane(const pqg::L1Quad& qd, int lane, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t rest, uint32_t fill) {
  const uint32_t q = 1000, n = 1u << 20;  // far from the stream's end
  const uint32_t lo = b0 | b1 << 8 | b2 << 16 | (rest & 0xff) << 24, hi = rest >> 8;
  const pqg::L1Hdr h = pqg::l1_hdr(lo, hi, q, n);
  const uint32_t len = (qd.len >> (8 * lane)) & 0xff;
  const bool bad = (qd.bad >> (8 * lane)) & 0x80, far = (qd.far >> (8 * lane)) & 0x80;
  if (((qd.bad | qd.far) >> (8 * lane)) & 0x7f) fail("stray flag bits", b0, b1, b2, lane, fill);
  if (bad && far) fail("bad and far", b0, b1, b2, lane, fill);
  if (!bad && !far && (h.bad || h.nx - q != len || len >= pqg::kL1Far)) fail("ok", b0, b1, b2, lane, fill);
  if (bad && !h.bad) fail("bad", b0, b1, b2, lane, fill);
  const bool one = b0 < 0x80, two = b0 >= 0x80 && b1 < 0x80;
  const uint32_t g = ((b0 & 0x7f) | b1 << 7) >> 1;
  const bool settled = one || (two && ((b0 & 1) == 0 || g <= 251));
  if (settled && (far || bad != h.bad)) fail("settled", b0, b1, b2, lane, fill);
  // the exit codes, with the quad's first position `ed` short of the segment's end
  const uint32_t ed = 4 + rest % 61;  // 4..64
  const pqg::L1Codes cd = pqg::l1_quad_codes(qd, ed);
  const uint32_t e = q - lane + ed;  // the header is at q = q0 + lane
  const bool in = (cd.in >> (8 * lane)) & 0x80;
  const uint32_t code = (cd.code >> (8 * lane)) & 0xff;
  if ((cd.in >> (8 * lane)) & 0x7f) fail("stray in bits", b0, b1, b2, lane, fill);
  if (in != (!far && !bad && h.nx < e)) fail("in", b0, b1, b2, lane, fill);
  if (!in) {
    const uint32_t d = h.nx - e;
    const uint32_t want = far ? pqg::kL1Far : h.bad ? pqg::kL1Bad : d < pqg::kL1Far ? d : pqg::kL1Far;
    if (code != want) fail("code", b0, b1, b2, lane, fill);
  }
}

}  // namespace

int main() {
  long checked = 0;
  // every (b0, b1, b2) in every lane, the other lanes 0x00 / 0xff / random
  for (uint32_t v = 0; v < (1u << 24); v++) {
    const uint32_t b0 = v & 0xff, b1 = (v >> 8) & 0xff, b2 = v >> 16;
    const int lane = (int)((v ^ (v >> 8) ^ (v >> 16)) & 3);
    for (int mode = 0; mode < 3; mode++) {
      const uint32_t keep = ~(0xffu << (8 * lane));
      uint32_t w[3];
      const uint32_t fill = mode == 0 ? 0u : mode == 1 ? 0xffffffffu : rnd();
      const uint32_t b[3] = {b0, b1, b2};
      for (int k = 0; k < 3; k++) w[k] = ((mode == 2 ? rnd() : fill) & keep) | b[k] << (8 * lane);
      check_lane(pqg::l1_quad(w[0], w[1], w[2]), lane, b0, b1, b2, rnd(), fill);
      checked++;
    }
  }
  // every lane of the same exhaustive triple (all four lanes alike), and
  // dwords of four random headers
  for (uint32_t v = 0; v < (1u << 24); v++) {
    const bool same = (v & 1) == 0;
    uint32_t w[3];
    if (same) {
      const uint32_t t = (v >> 1) * 2654435761u;
      w[0] = (t & 0xff) * 0x01010101u, w[1] = ((t >> 8) & 0xff) * 0x01010101u, w[2] = ((t >> 16) & 0xff) * 0x01010101u;
    } else {
      for (int k = 0; k < 3; k++) w[k] = rnd();
      if (v & 2) w[0] &= 0x7f7f7f7fu | (rnd() & 0x80808080u);  // more short headers
    }
    const pqg::L1Quad qd = pqg::l1_quad(w[0], w[1], w[2]);
    for (int lane = 0; lane < 4; lane++) {
      check_lane(qd, lane, (w[0] >> (8 * lane)) & 0xff, (w[1] >> (8 * lane)) & 0xff, (w[2] >> (8 * lane)) & 0xff, rnd(),
                 w[0]);
      checked++;
    }
  }
  std::printf("%ld parses checked, %ld errors\n", checked, errors);
  return errors ? 1 : 0;
}
