// convert_model.cpp — the lane code of k_conv_* (parquet-go_amd/csrc/pqg_convert.h) on the host:
// the 64 lanes of a wave run one after another over plain memory, a segment after another.  For
// a sweep of widths, counts, input misalignments and value patterns it checks
//   * that every 16-byte load is aligned and holds a byte of the segment's input bytes (the only
//     bytes a wave may count on being mapped), and every byte load lies inside the chars,
//   * that every stage access is aligned and inside the stage,
//   * that every store is aligned and lies inside the output,
//   * that the output equals a plain byte loop's and nothing around it changed,
//   * the bad-value count of BYTE_ARRAY decimals.
// Build: g++ -O1 -std=c++17 -Wno-unknown-pragmas -I parquet-go_amd/csrc tools/convert_model.cpp
// (add -fsanitize=address,undefined for a checked run).  Prints "ok <cases>" or the first
// failure; the exit status says which.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pqg_convert.h"

using namespace pqg;
using namespace pqg::conv;

static long g_loads = 0, g_stores = 0;
static const char* g_fail = nullptr;
static uint32_t g_seed = 12345;
static uint32_t rnd() {
  g_seed = g_seed * 1664525u + 1013904223u;
  return g_seed >> 8;
}

struct MemIn {
  uintptr_t lo, hi;  // the bytes that may be touched
  Q4 ld16(uintptr_t a) const {
    Q4 q{0, 0, 0, 0};
    if (a & 15) g_fail = "misaligned load";
    if (!(a < hi && a + 16 > lo)) {
      g_fail = "load of a granule that holds no byte of the segment's input";
      return q;
    }
    memcpy(&q, (const void*)a, 16);
    g_loads++;
    return q;
  }
  uint32_t u8(uintptr_t a) const {
    if (a < lo || a >= hi) {
      g_fail = "byte load outside the chars";
      return 0;
    }
    return *(const uint8_t*)a;
  }
};

struct MemStage {
  uint8_t* p;
  bool in(uint32_t o, uint32_t n) const {
    if (o % n) g_fail = "misaligned stage access";
    if (o + n > (uint32_t)kStageBytes) {
      g_fail = "stage access out of bounds";
      return false;
    }
    return true;
  }
  void put16(int o, const Q4& q) const {
    if (o >= 0 && in((uint32_t)o, 16)) memcpy(p + o, &q, 16);
  }
  uint32_t u32(uint32_t o) const {
    uint32_t v = 0;
    if (in(o, 4)) memcpy(&v, p + o, 4);
    return v;
  }
  uint32_t u8(uint32_t o) const { return in(o, 1) ? p[o] : 0; }
};

struct MemSink {
  uintptr_t ob, oe;
  void put(uintptr_t a, const void* v, int n) const {
    if (a % (uintptr_t)n) g_fail = "misaligned store";
    if (a < ob || a + (uintptr_t)n > oe) {
      g_fail = "store outside the output";
      return;
    }
    memcpy((void*)a, v, (size_t)n);
    g_stores++;
  }
  void st16(uintptr_t a, uint32_t x, uint32_t y, uint32_t z, uint32_t w) const {
    const uint32_t v[4] = {x, y, z, w};
    put(a, v, 16);
  }
  void st16wb(uintptr_t a, uint32_t x, uint32_t y, uint32_t z, uint32_t w) const { st16(a, x, y, z, w); }
  void st8(uintptr_t a, uint32_t lo, uint32_t hi) const {
    const uint32_t v[2] = {lo, hi};
    put(a, v, 8);
  }
};

// k_conv_dec / k_conv_int96: one wave per segment, a tile after another
template <int OD>
static void run_fixed(int kind, const uint8_t* in, int64_t n, int w, int unit, uint8_t* out) {
  alignas(16) static uint8_t stage[kStageBytes];
  const int ow = kind == K_INT96_TIME ? 8 : 4 * OD;
  const MemSink sink{(uintptr_t)out, (uintptr_t)out + (uintptr_t)(n * ow)};
  const MemStage st{stage};
  const int T = tile_values(kind, w);
  for (int64_t s0 = 0; s0 < n; s0 += kSeg) {
    const int64_t s1 = s0 + kSeg < n ? s0 + kSeg : n;
    const MemIn g{(uintptr_t)in + (uintptr_t)(s0 * w), (uintptr_t)in + (uintptr_t)(s1 * w)};
    for (int64_t t0 = s0; t0 < s1; t0 += T) {
      const int64_t t1 = t0 + T < s1 ? t0 + T : s1;
      const Tile t = tile_of((uintptr_t)in, w, t0, t1);
      memset(stage, 0xEE, sizeof(stage));
      for (int lane = 0; lane < 64; lane++) stage_tile(g, st, t, lane);
      const int nv = (int)(t1 - t0);
      const uintptr_t ob = (uintptr_t)out + (uintptr_t)(t0 * ow);
      for (int lane = 0; lane < 64; lane++) {
        if (kind == K_INT96_TIME) {
          for (int p = lane; 2 * p < nv; p += 64) int96_store(st, sink, t, unit, p, nv, ob + 16 * (uintptr_t)p);
        } else {
          for (int v = lane; v < nv; v += 64)
            decimal_store<OD>(st, sink, t, w, kind == K_DECIMAL_BE, v, ob + (uintptr_t)v * (4 * OD));
        }
      }
    }
  }
}

// a buffer of n bytes at `mis` past a 16-byte boundary, 48 guard bytes of 0xA5 around it
struct Buf {
  std::vector<uint8_t> store;
  uint8_t* p;
  size_t n;
  Buf(size_t n_, int mis) : store(n_ + 112, 0xA5), n(n_) {
    p = store.data() + 48;
    p += (16 - ((uintptr_t)p & 15)) % 16 + mis;
  }
  bool guards_ok() const {
    for (const uint8_t* q = store.data(); q < p; q++)
      if (*q != 0xA5) return false;
    for (const uint8_t* q = p + n; q < store.data() + store.size(); q++)
      if (*q != 0xA5) return false;
    return true;
  }
};

// value i of a sweep: random, all 0x00, all 0xff, 0x80 00.., 0x7f ff..
static void fill_value(uint8_t* v, int w, int64_t i, bool be) {
  const int pat = (int)(i % 5);
  for (int k = 0; k < w; k++) v[k] = pat == 0 ? (uint8_t)rnd() : pat == 1 || pat == 3 ? 0x00 : 0xff;
  uint8_t* top = be ? v : v + w - 1;
  if (pat == 3) *top = 0x80;
  if (pat == 4) *top = 0x7f;
}

static long g_cases = 0;

static bool decimals(int kind, int w, int ow, int64_t n, int mis) {
  const bool be = kind == K_DECIMAL_BE;
  Buf in((size_t)(n * w), mis), out((size_t)(n * ow), 0);
  for (int64_t i = 0; i < n; i++) fill_value(in.p + i * w, w, i, be);
  if (ow == 16) run_fixed<4>(kind, in.p, n, w, 0, out.p);
  else run_fixed<8>(kind, in.p, n, w, 0, out.p);
  g_cases++;
  for (int64_t i = 0; i < n && !g_fail; i++) {
    const uint8_t top = be ? in.p[i * w] : in.p[i * w + w - 1];
    for (int k = 0; k < ow; k++) {
      const uint8_t want = k < w ? (be ? in.p[i * w + w - 1 - k] : in.p[i * w + k]) : (top & 0x80 ? 0xff : 0x00);
      if (out.p[i * ow + k] != want) g_fail = "wrong output byte";
    }
  }
  if (!g_fail && (!out.guards_ok() || !in.guards_ok())) g_fail = "byte around a buffer changed";
  if (g_fail) printf("FAIL kind=%d w=%d ow=%d n=%ld in+%d: %s\n", kind, w, ow, (long)n, mis, g_fail);
  return !g_fail;
}

static uint64_t int96_plain(const uint8_t* v, int unit) {
  uint64_t nanos = 0;
  for (int k = 7; k >= 0; k--) nanos = nanos << 8 | v[k];
  uint32_t d = 0;
  for (int k = 3; k >= 0; k--) d = d << 8 | v[8 + k];
  static const uint64_t per_day[5] = {0, 86400ull, 86400000ull, 86400000000ull, 86400000000000ull};
  static const uint64_t ns_per[5] = {0, 1000000000ull, 1000000ull, 1000ull, 1ull};
  const __int128 days = (__int128)(int32_t)d - 2440588;
  return (uint64_t)(days * (__int128)per_day[unit] + (__int128)(nanos / ns_per[unit]));
}

static void put_int96(uint8_t* v, uint64_t nanos, int32_t day) {
  memcpy(v, &nanos, 8);
  memcpy(v + 8, &day, 4);
}

static bool int96s(int64_t n, int mis, int unit) {
  Buf in((size_t)(n * 12), mis), out((size_t)(n * 8), 0);
  // ns timestamps 0, -1, 1, -86400000000001, 2^62, -2^62 as (nanos of the day, julian day), the
  // edges of `day`, nanos at and above 2^63, a nil entry's zero bytes, then random values
  static const int64_t ts[6] = {0, -1, 1, -86400000000001ll, (int64_t)1 << 62, -((int64_t)1 << 62)};
  for (int64_t i = 0; i < n; i++) {
    uint8_t* v = in.p + i * 12;
    const int k = (int)(i % 16);
    if (k < 6) {
      const int64_t per = 86400000000000ll;
      int64_t day = ts[k] / per, ns = ts[k] % per;
      if (ns < 0) ns += per, day--;
      put_int96(v, (uint64_t)ns, (int32_t)(day + 2440588));
    } else if (k == 6) put_int96(v, 0, INT32_MAX);
    else if (k == 7) put_int96(v, 86399999999999ull, INT32_MIN);
    else if (k == 8) put_int96(v, (uint64_t)1 << 63, 2440588);
    else if (k == 9) put_int96(v, ~0ull, -1);
    else if (k == 10) put_int96(v, 0, 0);
    else put_int96(v, (uint64_t)rnd() << 40 ^ (uint64_t)rnd() << 20 ^ rnd(), (int32_t)(rnd() << 8 ^ rnd()));
  }
  run_fixed<4>(K_INT96_TIME, in.p, n, 12, unit, out.p);
  g_cases++;
  for (int64_t i = 0; i < n && !g_fail; i++) {
    const uint64_t want = int96_plain(in.p + i * 12, unit);
    if (memcmp(out.p + i * 8, &want, 8) != 0) g_fail = "wrong int64";
  }
  if (!g_fail && (!out.guards_ok() || !in.guards_ok())) g_fail = "byte around a buffer changed";
  if (g_fail) printf("FAIL int96 n=%ld in+%d unit=%d: %s\n", (long)n, mis, unit, g_fail);
  return !g_fail;
}

// BYTE_ARRAY decimals: k_conv_bad's count, and k_conv_bytes when there is no bad value
template <int OD>
static bool byte_arrays(int64_t n, bool with_bad, int mis) {
  const int ow = 4 * OD;
  static const int odd[6] = {0, 1, 16, 17, 32, 33};
  std::vector<int64_t> offs((size_t)n + 1, 0);
  int64_t bad = 0;
  for (int64_t i = 0; i < n; i++) {
    int len = 1 + (int)(rnd() % (uint32_t)ow);
    if (with_bad && i % 3 == 1) len = odd[(i / 3) % 6];
    if (len == 0 || len > ow) bad++;
    offs[(size_t)i + 1] = offs[(size_t)i] + len;
  }
  const int64_t vb = offs[(size_t)n];
  Buf in((size_t)vb, mis), out((size_t)(n * ow), 0);
  for (int64_t i = 0; i < n; i++)
    if (offs[(size_t)i + 1] > offs[(size_t)i]) fill_value(in.p + offs[(size_t)i], (int)(offs[(size_t)i + 1] - offs[(size_t)i]), i, true);
  g_cases++;
  int64_t got = 0;
  for (int64_t i = 0; i < n; i++) got += bytes_len(offs[(size_t)i], offs[(size_t)i + 1], vb, ow) < 0;
  if (got != bad) g_fail = "wrong bad-value count";
  // offsets that do not lie in the chars are bad whatever their difference
  if (bytes_len(-1, 3, 100, ow) >= 0 || bytes_len(8, 4, 100, ow) >= 0 || bytes_len(96, 101, 100, ow) >= 0 ||
      bytes_len(96, 100, 100, ow) != 4)
    g_fail = "wrong offsets rule";
  if (!g_fail && bad == 0) {
    const MemIn g{(uintptr_t)in.p, (uintptr_t)in.p + (uintptr_t)vb};
    const MemSink sink{(uintptr_t)out.p, (uintptr_t)out.p + (uintptr_t)(n * ow)};
    for (int64_t i = 0; i < n; i++) {
      const int64_t len = bytes_len(offs[(size_t)i], offs[(size_t)i + 1], vb, ow);
      uint32_t o[OD];
      bytes_value<OD>(g, (uintptr_t)in.p + (uintptr_t)offs[(size_t)i], (int)len, o);
      const uintptr_t at = (uintptr_t)out.p + (uintptr_t)(i * ow);
      sink.st16(at, o[0], o[1], o[2], o[3]);
      if constexpr (OD == 8) sink.st16(at + 16, o[4], o[5], o[6], o[7]);
    }
    for (int64_t i = 0; i < n && !g_fail; i++) {
      const uint8_t* v = in.p + offs[(size_t)i];
      const int len = (int)(offs[(size_t)i + 1] - offs[(size_t)i]);
      for (int k = 0; k < ow; k++)
        if (out.p[i * ow + k] != (k < len ? v[len - 1 - k] : (v[0] & 0x80 ? 0xff : 0x00))) g_fail = "wrong output byte";
    }
    if (!g_fail && (!out.guards_ok() || !in.guards_ok())) g_fail = "byte around a buffer changed";
  }
  if (g_fail) printf("FAIL byte arrays ow=%d n=%ld bad=%d: %s\n", ow, (long)n, (int)with_bad, g_fail);
  return !g_fail;
}

int main() {
  const int64_t counts[] = {0, 1, 63, 64, 65, 4095, 4096, 4097, 8193};
  for (int ow : {16, 32})
    for (int w = 1; w <= ow; w++)
      for (int64_t n : counts)
        for (int mis = 0; mis < 16; mis++)
          if (!decimals(K_DECIMAL_BE, w, ow, n, mis)) return 1;
  for (int ow : {16, 32})
    for (int w : {4, 8})
      for (int64_t n : counts)
        for (int mis = 0; mis < 16; mis++)
          if (!decimals(K_DECIMAL_INT, w, ow, n, mis)) return 1;
  for (int unit = U_SECONDS; unit <= U_NANOS; unit++)
    for (int64_t n : counts)
      for (int mis = 0; mis < 16; mis++)
        if (!int96s(n, mis, unit)) return 1;
  for (int64_t n : counts)
    for (int bad = 0; bad < 2; bad++)
      for (int mis : {0, 1, 7, 15})
        if (!byte_arrays<4>(n, bad != 0, mis) || !byte_arrays<8>(n, bad != 0, mis)) return 1;
  printf("ok %ld cases, %ld loads, %ld stores\n", g_cases, g_loads, g_stores);
  return 0;
}
