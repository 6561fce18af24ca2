// crc_model.cpp — k_page_crc's tile and combine code (parquet-go_amd/csrc/pqg_crc.h) on the
// host: the 64 lanes of a wave run one after another over plain memory.  For a sweep of
// lengths and start alignments it checks
//   * that every 16-byte load is aligned and holds a byte of the range [p, p + n) (the only
//     bytes a caller may count on being mapped),
//   * that the result — tables, tiles, the combine over the tiles, the final conditioning —
//     equals a plain bitwise CRC-32 of the range.
// Build: g++ -O1 -std=c++17 -Wno-unknown-pragmas -I parquet-go_amd/csrc tools/crc_model.cpp
// (add -fsanitize=address,undefined for a checked run).  Prints "ok <cases> ..." or the
// first failure; the exit status says which.
//   crc_model            the sweep
//   crc_model combine    lines "crcA crcB lenB" on stdin -> crc32(A || B) per line, by the
//                        shared multmodp / x8nmodp
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pqg_crc.h"

using namespace pqg;

static long g_loads = 0;
static const char* g_fail = nullptr;

struct MemTab {
  uint32_t* t;
  uint32_t get(int i) const {
    if (i < 0 || i >= crc::kTabs * 256) {
      g_fail = "table read out of range";
      return 0;
    }
    return t[i];
  }
  void put(int i, uint32_t v) const {
    if (i < 0 || i >= crc::kTabs * 256) {
      g_fail = "table write out of range";
      return;
    }
    t[i] = v;
  }
};

// one aligned granule; it must hold a byte of [lo, hi)
struct CheckedLd {
  uintptr_t lo, hi;
  crc::Q4 operator()(uintptr_t a) const {
    crc::Q4 q{0, 0, 0, 0};
    if (a & 15) {
      g_fail = "misaligned load";
      return q;
    }
    if (!(a < hi && a + 16 > lo)) {
      g_fail = "load of a granule that holds no byte of the range";
      return q;
    }
    memcpy(&q, (const void*)a, 16);
    g_loads++;
    return q;
  }
};

static uint32_t plain_crc(const uint8_t* p, int64_t n) {
  uint32_t c = 0xffffffffu;
  for (int64_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
  }
  return ~c;
}

// what k_crc_plan / k_page_crc / k_crc_fin do for one page
static uint32_t model_crc(const MemTab& tb, const uint8_t* p, int64_t n, long* tiles_out) {
  const uintptr_t a = (uintptr_t)p;
  const int64_t nt = crc::num_tiles(a, n);
  const CheckedLd ld{a, a + (uintptr_t)n};
  std::vector<uint32_t> raws((size_t)nt);
  int64_t covered = 0;
  for (int64_t t = 0; t < nt; t++) {
    crc::Tile tl;
    tl.init(a, n, t);
    if ((tl.nfull + tl.pad) % 64 || tl.pad < 0 || tl.pad > 63 || tl.m < 0 || tl.m > 15) g_fail = "tile plan";
    uint32_t r = 0;
    for (int lane = 0; lane < 64; lane++) r ^= multmodp(crc::lane_tile(tl, lane, ld, tb), crc::lane_mul(lane));
    raws[(size_t)t] = crc::tile_tail(tl, r, ld, tb);
    covered += crc::tile_bytes(a, n, t);
  }
  if (covered != n) g_fail = "the tiles' bytes do not add up to the range";
  uint32_t x = 0;
  for (int lane = 0; lane < 64; lane++)
    x ^= crc::lane_combine(a, n, nt, lane, [&](int64_t t) { return raws[(size_t)t]; });
  // what k_crc_fin does for a page without tile records (short ranges only: it goes bit by bit)
  if (n <= 70000) {
    uint32_t y = 0;
    for (int lane = 0; lane < 64; lane++) y ^= crc::lane_slice(n, lane, [&](int64_t i) { return (uint32_t)p[i]; });
    if (y != x) g_fail = "the table-free walk differs from the tiles' combine";
  }
  *tiles_out += (long)nt;
  return ~x;
}

static int run_combine() {
  unsigned long a, b;
  unsigned long long len;
  while (scanf("%lu %lu %llu", &a, &b, &len) == 3)
    printf("%u\n", multmodp(x8nmodp((uint64_t)len), (uint32_t)a) ^ (uint32_t)b);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "combine")) return run_combine();
  std::vector<uint32_t> tabs((size_t)crc::kTabs * 256, 0xdeadbeefu);
  const MemTab tb{tabs.data()};
  for (int r = 0; r < crc::kTabs; r++)
    for (int lane = 0; lane < 64; lane++) crc::build_round(tb, lane, r);
  // the tables against their definition: byte b, then z zero bytes
  for (int k = 0; k < crc::kTabs && !g_fail; k++)
    for (int b = 0; b < 256; b += 51) {
      const int z = k < 16 ? 15 - k : crc::kRow - 1 - (k - 16);
      uint32_t c = (uint32_t)b;
      for (int i = 0; i < 8 * (z + 1); i++) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
      if (tb.get(k * 256 + b) != c) g_fail = "table entry";
    }
  if (g_fail) {
    printf("FAIL tables: %s\n", g_fail);
    return 1;
  }
  const int64_t big = (4 << 20) + 5;
  std::vector<uint8_t> buf((size_t)big + 64);
  uint32_t seed = 2463534242u;
  for (auto& x : buf) {
    seed = seed * 1664525u + 1013904223u;
    x = (uint8_t)(seed >> 24);
  }
  uint8_t* base = buf.data() + (16 - ((uintptr_t)buf.data() & 15)) % 16;  // 16-byte aligned, >= 48 bytes of room behind
  long cases = 0, tiles = 0;
  auto check = [&](int64_t n, int al) {
    const uint8_t* p = base + al;
    const uint32_t got = model_crc(tb, p, n, &tiles), want = n == 0 ? 0u : plain_crc(p, n);
    cases++;
    if (!g_fail && got != want) g_fail = "wrong crc";
    if (g_fail) printf("FAIL n=%ld align=%d: %s\n", (long)n, al, g_fail);
    return !g_fail;
  };
  for (int al = 0; al < 16; al++)
    for (int64_t n = 0; n <= 600; n++)
      if (!check(n, al)) return 1;
  const int64_t marks[] = {256, crc::kRow, crc::kTile, 2 * (int64_t)crc::kTile, 3 * (int64_t)crc::kTile};
  const int als[] = {0, 1, 7, 15};
  for (int64_t mk : marks)
    for (int al : als)
      for (int64_t n = mk - 17; n <= mk + 17; n++)
        if (!check(n, al)) return 1;
  const long t0 = tiles;
  if (!check(big, 3)) return 1;
  if (tiles - t0 <= 256) {
    printf("FAIL the big buffer has %ld tiles\n", tiles - t0);
    return 1;
  }
  printf("ok %ld cases, %ld tiles, %ld loads\n", cases, tiles, g_loads);
  return 0;
}
