// bss_model.cpp — k_bss's tile code (parquet-go_amd/csrc/pqg_bss.h) on the host: the 64
// lanes of a wave run one after another over plain memory.  It checks, for a sweep of
// widths, page sizes, parts and alignments of both sides,
//   * that every 16-byte load is aligned and holds a byte of the stream range the part
//     reads (the only bytes a part may count on being mapped),
//   * that every store lies inside the part's output bytes,
//   * that the output equals out[i w + k] = val[k nn + i] and nothing around it changed.
// Build: g++ -O1 -std=c++17 -Wno-unknown-pragmas -I parquet-go_amd/csrc tools/bss_model.cpp
// (add -fsanitize=address,undefined for a checked run).  Prints "ok <cases>" or the first
// failure; the exit status says which.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pqg_bss.h"

using namespace pqg;

static long g_loads = 0, g_stores = 0;
static const char* g_fail = nullptr;

struct MemStage {
  const uint8_t* p;
  uint32_t u8(int o) const { return p[o]; }
  uint32_t u16(int o) const {
    if (o & 1) g_fail = "misaligned u16 stage read";
    uint16_t v;
    memcpy(&v, p + o, 2);
    return v;
  }
  uint32_t u32(int o) const {
    if (o & 3) g_fail = "misaligned u32 stage read";
    uint32_t v;
    memcpy(&v, p + o, 4);
    return v;
  }
};

struct MemSink {
  uintptr_t ob, oe;
  void put(uintptr_t a, const void* v, int n) const {
    if (a % (uintptr_t)n) g_fail = "misaligned store";
    if (a < ob || a + (uintptr_t)n > oe) {
      g_fail = "store outside the part's output";
      return;
    }
    memcpy((void*)a, v, (size_t)n);
    g_stores++;
  }
  void st16(uintptr_t a, uint32_t x, uint32_t y, uint32_t z, uint32_t w) const {
    const uint32_t v[4] = {x, y, z, w};
    put(a, v, 16);
  }
  void st4(uintptr_t a, uint32_t v) const { put(a, &v, 4); }
  void st2(uintptr_t a, uint32_t v) const {
    const uint16_t h = (uint16_t)v;
    put(a, &h, 2);
  }
};

// one aligned granule; it must hold a byte of [lo, hi)
static void load16(uintptr_t a, uintptr_t lo, uintptr_t hi, uint32_t (&w)[4]) {
  if (a & 15) g_fail = "misaligned load";
  if (!(a < hi && a + 16 > lo)) {
    g_fail = "load of a granule that holds no byte of the part's stream range";
    memset(w, 0, sizeof(w));
    return;
  }
  memcpy(w, (const void*)a, 16);
  g_loads++;
}

template <int W>
static void run_part(const uint8_t* val, int64_t nn, int64_t v_lo, int64_t v_hi, uint8_t* out) {
  typedef bss::Part<W> P;
  P pt;
  pt.init((uintptr_t)val, nn, v_lo, v_hi, (uintptr_t)out);
  alignas(16) uint8_t st[bss::kTileBytes];
  for (int64_t t0 = 0; t0 < pt.xn; t0 += P::T) {
    memset(st, 0xEE, sizeof(st));
    for (int j = 0; j < P::NL; j++)
      for (int lane = 0; lane < 64; lane++) {
        const typename P::Load l = pt.load(t0, lane, j);
        const int k = l.st / P::T;
        const uintptr_t lo = (uintptr_t)val + (uintptr_t)(k * nn + v_lo), hi = (uintptr_t)val + (uintptr_t)(k * nn + v_hi);
        uint32_t a[4], b[4];
        load16(l.base + l.off_a, lo, hi, a);
        load16(l.base + l.off_b, lo, hi, b);
        const bss::Q4 o = bss::funnel16(a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], l.s);
        if (l.st & 15 || l.st < 0 || l.st + 16 > bss::kTileBytes) g_fail = "stage write out of place";
        memcpy(st + l.st, &o, 16);
      }
    uint32_t o_lo, o_hi;
    pt.out_range(t0, &o_lo, &o_hi);
    const MemSink sink{pt.ob, pt.oe};
    for (int j = 0; j < P::NL; j++)
      for (int lane = 0; lane < 64; lane++) {
        uint32_t g[4];
        bss::granule<W>(MemStage{st}, lane + 64 * j, g);
        const uint32_t og = 16u * (uint32_t)(lane + 64 * j);
        bss::store_granule<W>(sink, pt.out_base(t0) + og, og, o_lo, o_hi, g);
      }
  }
}

static void run(int w, const uint8_t* val, int64_t nn, int64_t v_lo, int64_t v_hi, uint8_t* out) {
  if (w == 2) run_part<2>(val, nn, v_lo, v_hi, out);
  else if (w == 4) run_part<4>(val, nn, v_lo, v_hi, out);
  else if (w == 8) run_part<8>(val, nn, v_lo, v_hi, out);
  else run_part<16>(val, nn, v_lo, v_hi, out);
}

int main() {
  const int widths[] = {2, 4, 8, 16};
  const int64_t nns[] = {1, 2, 15, 16, 17, 63, 64, 65, 255, 511, 512, 513, 1023, 1024, 1025, 2047, 2049, 4095, 4097, 8191, 8193, 70001};
  const int in_mis[] = {0, 1, 3, 4, 7, 8, 13, 15};
  uint32_t seed = 12345;
  long cases = 0;
  for (int w : widths)
    for (int64_t nn : nns)
      for (int im : in_mis)
        for (int om = 0; om < 16; om += w) {
          if (nn > 10000 && (im % 4 != 3 || (om != 0 && om != 16 - w && om != w))) continue;
          // the page's bytes on no boundary, 32 guard bytes around both buffers
          std::vector<uint8_t> src((size_t)(nn * w) + 96), dst((size_t)(nn * w) + 96, 0xA5);
          uint8_t* val = src.data() + 32;
          val += (16 - ((uintptr_t)val & 15)) % 16 + im;
          uint8_t* out = dst.data() + 32;
          out += (16 - ((uintptr_t)out & 15)) % 16 + om;
          for (int64_t i = 0; i < nn * w; i++) {
            seed = seed * 1664525u + 1013904223u;
            val[i] = (uint8_t)(seed >> 24);
          }
          // parts as k_part_plan cuts them: one up to kSplitMin values, above it kPart values each
          if (nn <= kSplitMin) run(w, val, nn, 0, nn, out);
          else
            for (int64_t v = 0; v < nn; v += kPart) run(w, val, nn, v, v + kPart < nn ? v + kPart : nn, out);
          cases++;
          if (!g_fail) {
            for (int64_t i = 0; i < nn && !g_fail; i++)
              for (int k = 0; k < w; k++)
                if (out[i * w + k] != val[k * nn + i]) g_fail = "wrong output byte";
            for (uint8_t* p = dst.data(); p < out; p++)
              if (*p != 0xA5) g_fail = "byte before the output changed";
            for (uint8_t* p = out + nn * w; p < dst.data() + dst.size(); p++)
              if (*p != 0xA5) g_fail = "byte after the output changed";
          }
          if (g_fail) {
            printf("FAIL w=%d nn=%ld in+%d out+%d: %s\n", w, (long)nn, im, om, g_fail);
            return 1;
          }
        }
  printf("ok %ld cases, %ld loads, %ld stores\n", cases, g_loads, g_stores);
  return 0;
}
