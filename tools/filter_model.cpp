// filter_model.cpp — K9s's lane code (parquet-go_amd/csrc/pqg_filter.h) on the host: the 64 lanes of
// a wave run one after another over plain memory, glued the way k_flt_* / k_sel_* (pqg_filter.hip)
// glue them (ballots as loops over the lanes, ranks as popcounts, the per-segment counts and their
// scan).  For every row count at a wave, word and segment edge, every null pattern, type, operator
// and combine mode, with and without a dictionary, and for every select width and bitmap pattern it
// checks
//   * bitmaps, counts and compacted outputs against a plain scalar loop that shares no code with the
//     header,
//   * that every load lies inside an input (or, for AND / OR, the bitmap) and is naturally aligned,
//   * that every store lies inside an output, and that 64 guard bytes on either side of every output
//     are unchanged.
// The wave copy of byte-array values longer than 64 bytes (pqg_wavecopy.h, device builtins) is stood
// in for by a bytewise copy through the same checked IO.
// Build: g++ -O1 -std=c++17 -Wno-unknown-pragmas -I parquet-go_amd/csrc tools/filter_model.cpp
// (add -fsanitize=address,undefined for a checked run).  Prints "ok <cases>" or the first failure;
// the exit status says which.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pqg_filter.h"

using namespace pqg::flt;

static const char* g_fail = nullptr;
static long g_cases = 0;

// ---- checked memory ---------------------------------------------------------------------------
struct Region {
  uintptr_t lo, hi;
  bool writable;
};
static std::vector<Region> g_regions;
static void region(const void* p, size_t n, bool writable) {
  g_regions.push_back(Region{(uintptr_t)p, (uintptr_t)p + n, writable});
}
static bool inside(uintptr_t a, size_t n, bool write) {
  for (const Region& r : g_regions)
    if (a >= r.lo && a + n <= r.hi && (!write || r.writable)) return true;
  return false;
}

struct HostIO {
  template <class T>
  T ld(uintptr_t a) const {
    T v = 0;
    if (a % sizeof(T)) g_fail = "misaligned load";
    if (!inside(a, sizeof(T), false)) {
      g_fail = "load outside the inputs";
      return v;
    }
    memcpy(&v, (const void*)a, sizeof(T));
    return v;
  }
  template <class T>
  void st(uintptr_t a, T v) const {
    if (a % sizeof(T)) g_fail = "misaligned store";
    if (!inside(a, sizeof(T), true)) {
      g_fail = "store outside the outputs";
      return;
    }
    memcpy((void*)a, &v, sizeof(T));
  }
  uint32_t u8(uintptr_t a) const { return ld<uint8_t>(a); }
  uint32_t u32(uintptr_t a) const { return ld<uint32_t>(a); }
  uint64_t u64(uintptr_t a) const { return ld<uint64_t>(a); }
  void st8(uintptr_t a, uint32_t v) const { st<uint8_t>(a, (uint8_t)v); }
  void st32(uintptr_t a, uint32_t v) const { st<uint32_t>(a, v); }
  void st64(uintptr_t a, uint64_t v) const { st<uint64_t>(a, v); }
  uint32_t eword(uintptr_t base, int64_t j) const { return ld<uint32_t>(base + 4 * (uintptr_t)j); }
};

// an output of n bytes between two 64-byte guards
struct Guarded {
  std::vector<uint8_t> buf;
  size_t n;
  explicit Guarded(size_t n_, uint8_t fill = 0xcd) : buf(n_ + 128 + 16, 0xa5), n(n_) { memset(data(), fill, n); }
  uint8_t* data() {
    uintptr_t a = ((uintptr_t)buf.data() + 64 + 15) & ~(uintptr_t)15;
    return (uint8_t*)a;
  }
  bool intact() {
    const uint8_t* d = data();
    for (int k = 1; k <= 64; k++)
      if (d[-k] != 0xa5 || d[n + k - 1] != 0xa5) return false;
    return true;
  }
};

// memcmp / memcpy that take the null pointer of an empty vector
static bool differ(const void* a, const void* b, size_t n) { return n && memcmp(a, b, n); }
static void copy(void* d, const void* s, size_t n) {
  if (n) memcpy(d, s, n);
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 32);
}

// ---- the wave glue of pqg_filter.hip, lanes one after another -------------------------------------
static std::vector<int64_t> valid_ranks(const HostIO& io, uintptr_t def, int64_t n, int max_def, int64_t* total) {
  const int64_t nseg = (n + kSeg - 1) / kSeg;
  std::vector<int64_t> seg((size_t)nseg);
  int64_t run = 0;
  for (int64_t s = 0; s < nseg; s++) {  // k_flt_count + k_flt_scan<1>
    seg[(size_t)s] = run;
    const int64_t s1 = std::min(n, (s + 1) * kSeg);
    for (int64_t i = s * kSeg; i < s1; i++) run += row_valid(io, def, i, max_def);
  }
  *total = run;
  return seg;
}

struct DictIn {
  uintptr_t values = 0, offsets = 0;
  int64_t values_bytes = 0, count = 0, nil_entry = -1;
};

static void model_filter(const Pred& p, Col c, const DictIn* d, uint8_t* bitmap, int64_t n, int mode,
                         int64_t* num_selected, int64_t* num_valid) {
  const HostIO io;
  *num_selected = 0;
  *num_valid = 0;
  if (n == 0) return;
  int64_t nv = n;
  std::vector<int64_t> seg;
  if (c.def) seg = valid_ranks(io, c.def, n, c.max_def, &nv);
  *num_valid = nv;
  const bool cmp = p.op != OP_IS_NULL && p.op != OP_NOT_NULL;
  if (d && cmp)  // k_flt_dict
    for (int64_t e0 = 0; e0 < d->count; e0 += 64) {
      uint64_t m = 0;
      for (int lane = 0; lane < 64; lane++) {
        const int64_t e = e0 + lane;
        if (e < d->count && entry_pass(io, p, d->values, d->offsets, d->values_bytes, d->nil_entry, e)) m |= 1ull << lane;
      }
      for (int lane = 0; lane < 2; lane++)
        if (e0 + 32 * lane < d->count) io.st32(c.ebits + 4 * (uintptr_t)((e0 + 32 * lane) >> 5), (uint32_t)(m >> (32 * lane)));
    }
  const int64_t nseg = (n + kSeg - 1) / kSeg;
  for (int64_t s = 0; s < nseg; s++) {  // k_flt_rows
    const int64_t s0 = s * kSeg, s1 = std::min(n, s0 + kSeg);
    int64_t rv = c.def ? seg[(size_t)s] : s0;
    for (int64_t b = s0; b < s1; b += 64) {
      uint64_t mv = 0, mp = 0, mi = 0;
      bool valid[64];
      for (int lane = 0; lane < 64; lane++) {
        const int64_t i = b + lane;
        valid[lane] = i < s1 && row_valid(io, c.def, i, c.max_def);
        if (valid[lane]) mv |= 1ull << lane;
        if (i < s1) mi |= 1ull << lane;
      }
      for (int lane = 0; lane < 64; lane++) {
        const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
        if (b + lane < s1 && row_pass(io, p, c, valid[lane], rv + __builtin_popcountll(mv & lt))) mp |= 1ull << lane;
      }
      for (int lane = 0; lane < 64; lane++) *num_selected += store_word(io, (uintptr_t)bitmap, b, n, lane, mp, mi, mode);
      rv += __builtin_popcountll(mv);
    }
  }
}

static void model_select(const Sel& a, int64_t* rows_out, int64_t* values_out, int64_t* bytes_out) {
  const HostIO io;
  *rows_out = *values_out = *bytes_out = 0;
  const int64_t n = a.n;
  if (n == 0) return;
  const bool var = a.width == 0;
  int64_t nv;
  std::vector<int64_t> segv;
  if (a.def) segv = valid_ranks(io, a.def, n, a.max_def, &nv);
  const int64_t nseg = (n + kSeg - 1) / kSeg;
  std::vector<int64_t> cnt((size_t)(3 * nseg));
  int64_t tot[3] = {0, 0, 0};
  for (int64_t s = 0; s < nseg; s++) {  // k_sel_count, then k_flt_scan<3>
    const int64_t s0 = s * kSeg, s1 = std::min(n, s0 + kSeg);
    int64_t rv = a.def ? segv[(size_t)s] : s0;
    for (int j = 0; j < 3; j++) cnt[(size_t)(3 * s + j)] = tot[j];
    for (int64_t b = s0; b < s1; b += 64) {
      uint64_t mv = 0;
      bool sel[64], valid[64];
      for (int lane = 0; lane < 64; lane++) {
        sel_flags(io, a, b + lane, b + lane < s1, &sel[lane], &valid[lane]);
        if (valid[lane]) mv |= 1ull << lane;
      }
      for (int lane = 0; lane < 64; lane++) {
        const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
        const int64_t src = rv + __builtin_popcountll(mv & lt);
        const bool sv = sel[lane] && valid[lane] && src < a.num_values;
        tot[0] += sel[lane];
        tot[1] += sv;
        if (var && sv) {
          int64_t at;
          tot[2] += sel_len(io, a, src, &at);
        }
      }
      rv += __builtin_popcountll(mv);
    }
  }
  *rows_out = tot[0];
  *values_out = tot[1];
  *bytes_out = var ? tot[2] : tot[1] * a.width;
  if (!a.out_def && !a.out_values && !a.out_offsets) return;
  if (var && a.out_offsets) io.st64(a.out_offsets + 8 * (uintptr_t)tot[1], (uint64_t)tot[2]);
  for (int64_t s = 0; s < nseg; s++) {  // k_sel_write
    const int64_t s0 = s * kSeg, s1 = std::min(n, s0 + kSeg);
    int64_t rv = a.def ? segv[(size_t)s] : s0, rs = cnt[(size_t)(3 * s)], rsv = cnt[(size_t)(3 * s + 1)],
            rc = cnt[(size_t)(3 * s + 2)];
    for (int64_t b = s0; b < s1; b += 64) {
      uint64_t mv = 0, ms = 0, msv = 0;
      bool sel[64], valid[64], sv[64];
      int64_t src[64], at[64], len[64], dchar[64];
      for (int lane = 0; lane < 64; lane++) {
        sel_flags(io, a, b + lane, b + lane < s1, &sel[lane], &valid[lane]);
        if (valid[lane]) mv |= 1ull << lane;
        if (sel[lane]) ms |= 1ull << lane;
      }
      int64_t round = 0;
      for (int lane = 0; lane < 64; lane++) {
        const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
        src[lane] = rv + __builtin_popcountll(mv & lt);
        sv[lane] = sel[lane] && valid[lane] && src[lane] < a.num_values;
        if (sv[lane]) msv |= 1ull << lane;
        at[lane] = len[lane] = 0;
        if (var && sv[lane]) len[lane] = sel_len(io, a, src[lane], &at[lane]);
        dchar[lane] = rc + round;  // the wave's exclusive scan of len
        round += len[lane];
      }
      for (int lane = 0; lane < 64; lane++) {
        const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
        sel_store(io, a, b + lane, sel[lane], sv[lane], src[lane], rs + __builtin_popcountll(ms & lt),
                  rsv + __builtin_popcountll(msv & lt), dchar[lane], at[lane], len[lane]);
      }
      if (var && a.out_values)
        for (int lane = 0; lane < 64; lane++)
          if (sv[lane] && len[lane] > kLongValue)  // the wave copy's stand-in
            for (int64_t k = 0; k < len[lane]; k++)
              io.st8(a.out_values + (uintptr_t)(dchar[lane] + k), io.u8(a.values + (uintptr_t)(at[lane] + k)));
      rv += __builtin_popcountll(mv);
      rs += __builtin_popcountll(ms);
      rsv += __builtin_popcountll(msv);
      rc += round;
    }
  }
}

// ---- the yardstick: plain scalar loops -----------------------------------------------------------
static int ref_cmp(int kind, const uint8_t* a, size_t alen, const uint8_t* b, size_t blen) {
  switch (kind) {
    case K_I32: { int32_t x, y; memcpy(&x, a, 4); memcpy(&y, b, 4); return x < y ? -1 : x > y ? 1 : 0; }
    case K_U32: { uint32_t x, y; memcpy(&x, a, 4); memcpy(&y, b, 4); return x < y ? -1 : x > y ? 1 : 0; }
    case K_I64: { int64_t x, y; memcpy(&x, a, 8); memcpy(&y, b, 8); return x < y ? -1 : x > y ? 1 : 0; }
    case K_U64: { uint64_t x, y; memcpy(&x, a, 8); memcpy(&y, b, 8); return x < y ? -1 : x > y ? 1 : 0; }
    case K_F32: { float x, y; memcpy(&x, a, 4); memcpy(&y, b, 4); if (isnan(x) || isnan(y)) return 2; return x < y ? -1 : x > y ? 1 : 0; }
    case K_F64: { double x, y; memcpy(&x, a, 8); memcpy(&y, b, 8); if (isnan(x) || isnan(y)) return 2; return x < y ? -1 : x > y ? 1 : 0; }
    case K_U8: return a[0] < b[0] ? -1 : a[0] > b[0] ? 1 : 0;
  }
  const size_t m = std::min(alen, blen);
  const int r = m ? memcmp(a, b, m) : 0;
  if (r) return r < 0 ? -1 : 1;
  return alen < blen ? -1 : alen > blen ? 1 : 0;
}
static bool ref_pass(int op, int c) {
  if (c == 2) return op == OP_NE;
  const bool t[6][3] = {{0, 1, 0}, {1, 0, 1}, {1, 0, 0}, {1, 1, 0}, {0, 0, 1}, {0, 1, 1}};  // [op][c + 1]
  return t[op][c + 1];
}

// a column of n rows: def levels (empty: max_def 0), dense values
struct Column {
  int kind, width, max_def;
  std::vector<uint8_t> def, values;
  std::vector<int64_t> offsets;  // K_BYTES: nv + 1
  int64_t nv = 0;
  const uint8_t* value(int64_t r, size_t* len) const {
    if (kind == K_BYTES) {
      *len = (size_t)(offsets[(size_t)r + 1] - offsets[(size_t)r]);
      return values.data() + offsets[(size_t)r];
    }
    *len = (size_t)width;
    return values.data() + (size_t)r * (size_t)width;
  }
};

static int width_of(int kind, int flba) {
  switch (kind) {
    case K_I32: case K_U32: case K_F32: return 4;
    case K_I64: case K_U64: case K_F64: return 8;
    case K_U8: return 1;
    case K_FLBA: return flba;
  }
  return 0;
}

// the values a column and its literals are drawn from: the type's edges, NaN, infinities, both
// zeros, the empty string, prefixes, 0x7f against 0x80, strings past 64 bytes
static std::vector<std::string> domain(int kind, int width) {
  std::vector<std::string> d;
  auto put = [&](const void* p, size_t n) { d.emplace_back((const char*)p, n); };
  if (kind == K_I32 || kind == K_U32) {
    for (uint32_t v : {0u, 1u, 2u, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xffffffffu, 1000u}) put(&v, 4);
  } else if (kind == K_I64 || kind == K_U64) {
    for (uint64_t v : {0ull, 1ull, 2ull, 0x7fffffffffffffffull, 0x8000000000000000ull, 0x8000000000000001ull, ~0ull, 1ull << 40})
      put(&v, 8);
  } else if (kind == K_F32) {
    for (float v : {0.0f, -0.0f, 1.5f, -1.5f, INFINITY, -INFINITY, NAN, 3.0e38f, 1e-45f}) put(&v, 4);
  } else if (kind == K_F64) {
    for (double v : {0.0, -0.0, 1.5, -1.5, (double)INFINITY, (double)-INFINITY, (double)NAN, 1.7e308, 5e-324}) put(&v, 8);
  } else if (kind == K_U8) {
    for (uint8_t v : {0, 1}) put(&v, 1);
  } else if (kind == K_FLBA) {
    for (int k = 0; k < 6; k++) {
      std::string s((size_t)width, (char)0);
      const uint8_t first[6] = {0x00, 0x7f, 0x80, 0xff, 0x41, 0x41};
      s[0] = (char)first[k];
      if (k == 5) s[(size_t)width - 1] = 1;  // differs from k = 4 in the last byte only
      d.push_back(s);
    }
  } else {
    d = {"", "a", "ab", "abc", std::string("\x7f"), std::string("\x80"), std::string("ab\0", 3), std::string(65, 'x'),
         std::string(65, 'x') + "y", std::string(200, 'x'), std::string(5000, 'q')};
  }
  return d;
}

static Column make_column(int kind, int width, int64_t n, int nullpat, const std::vector<std::string>& dom) {
  Column c;
  c.kind = kind;
  c.width = width;
  c.max_def = nullpat == 0 ? 0 : 1;
  if (c.max_def) c.def.resize((size_t)n);
  if (kind == K_BYTES) c.offsets.push_back(0);
  for (int64_t i = 0; i < n; i++) {
    bool valid = true;
    if (nullpat == 2) valid = false;
    if (nullpat == 3) valid = rnd() % 10 != 0;
    if (nullpat == 4) valid = i != n - 1;
    if (c.max_def) c.def[(size_t)i] = valid;
    if (!valid) continue;
    const std::string& v = dom[rnd() % dom.size()];
    c.values.insert(c.values.end(), v.begin(), v.end());
    if (kind == K_BYTES) c.offsets.push_back((int64_t)c.values.size());
    c.nv++;
  }
  return c;
}

static std::vector<uint32_t> ref_filter(const Column& c, int op, const std::string& lit, const std::vector<uint32_t>& old,
                                        int mode, int64_t n, int64_t* nsel, int64_t* nvalid) {
  std::vector<uint32_t> bm((size_t)((n + 31) / 32), 0u);
  int64_t r = 0;
  *nvalid = 0;
  for (int64_t i = 0; i < n; i++) {
    const bool valid = c.max_def == 0 || c.def[(size_t)i] == 1;
    bool pass;
    if (op == OP_IS_NULL) pass = !valid;
    else if (op == OP_NOT_NULL) pass = valid;
    else if (!valid) pass = false;
    else {
      size_t len;
      const uint8_t* v = c.value(r, &len);
      pass = ref_pass(op, ref_cmp(c.kind, v, len, (const uint8_t*)lit.data(), lit.size()));
    }
    if (valid) r++, (*nvalid)++;
    const bool was = (old[(size_t)(i >> 5)] >> (i & 31)) & 1;
    const bool now = mode == M_SET ? pass : mode == M_AND ? (was && pass) : (was || pass);
    if (now) bm[(size_t)(i >> 5)] |= 1u << (i & 31);
  }
  *nsel = 0;
  for (uint32_t w : bm) *nsel += __builtin_popcount(w);
  return bm;
}

#define FAIL(msg)             \
  do {                        \
    if (!g_fail) g_fail = msg; \
    return;                   \
  } while (0)

static void fill_pred(Pred* p, const Column& c, int op, const std::string& lit, const std::vector<uint8_t>& litbuf) {
  memset(p, 0, sizeof(*p));
  p->kind = c.kind;
  p->op = op;
  p->width = c.width;
  if (c.kind != K_BYTES && c.kind != K_FLBA) copy(&p->lit, lit.data(), lit.size());
  p->lit_bytes = (uintptr_t)litbuf.data();
  p->lit_len = (int64_t)lit.size();
}

static void filter_case(const Column& c, int64_t n, int op, const std::string& lit, int mode, bool use_dict) {
  g_cases++;
  g_regions.clear();
  const size_t words = (size_t)((n + 31) / 32);
  std::vector<uint32_t> old(words);
  for (uint32_t& w : old) w = mode == M_SET ? 0xdeadbeefu : (rnd() % 4 == 0 ? ~0u : rnd());  // tail bits set too
  Guarded bm(4 * words);
  copy(bm.data(), old.data(), 4 * words);
  if (mode == M_SET) std::fill(old.begin(), old.end(), 0u);
  int64_t want_sel, want_valid;
  const std::vector<uint32_t> want = ref_filter(c, op, lit, old, mode, n, &want_sel, &want_valid);
  std::vector<uint8_t> litbuf(lit.begin(), lit.end());
  if (litbuf.empty()) litbuf.push_back(0);  // a non-null address; lit_len says nothing is read
  Pred p;
  fill_pred(&p, c, op, lit, litbuf);
  Col col;
  memset(&col, 0, sizeof(col));
  col.max_def = c.max_def;
  col.def = c.max_def ? (uintptr_t)c.def.data() : 0;
  if (c.max_def) region(c.def.data(), c.def.size(), false);
  if (!lit.empty()) region(litbuf.data(), lit.size(), false);
  region(bm.data(), 4 * words, true);
  // with a dictionary: the column's distinct values plus entries no key uses, and int32 keys
  std::vector<uint8_t> dvals, keys;
  std::vector<int64_t> doffs;
  DictIn d;
  Guarded ebits(0);
  if (use_dict) {
    std::vector<std::string> ent = {c.kind == K_BYTES ? std::string("unused") : std::string((size_t)c.width, (char)0x55)};
    std::vector<int32_t> key((size_t)c.nv);
    for (int64_t r = 0; r < c.nv; r++) {
      size_t len;
      const uint8_t* v = c.value(r, &len);
      const std::string s((const char*)v, len);
      size_t k = 1;
      while (k < ent.size() && ent[k] != s) k++;
      if (k == ent.size()) ent.push_back(s), ent.push_back(s + (c.kind == K_BYTES ? "~" : "")), k = ent.size() - 2;
      key[(size_t)r] = (int32_t)k;
    }
    if (c.kind != K_BYTES) {  // fixed width: the appended duplicates are unused entries too
      for (std::string& s : ent) s.resize((size_t)c.width, (char)0x55);
    }
    dvals.push_back(0);  // the entries start at an odd address, as inside a dictionary page
    doffs.push_back(0);
    for (const std::string& s : ent) {
      dvals.insert(dvals.end(), s.begin(), s.end());
      doffs.push_back((int64_t)dvals.size() - 1);
    }
    keys.resize(4 * key.size());
    copy(keys.data(), key.data(), keys.size());
    d.values = (uintptr_t)dvals.data() + 1;
    d.offsets = c.kind == K_BYTES ? (uintptr_t)doffs.data() : 0;
    d.values_bytes = (int64_t)dvals.size() - 1;
    d.count = (int64_t)ent.size();
    ebits = Guarded(4 * (size_t)((d.count + 31) / 32));
    region(dvals.data() + 1, dvals.size() - 1, false);
    if (c.kind == K_BYTES) region(doffs.data(), 8 * doffs.size(), false);
    if (!keys.empty()) region(keys.data(), keys.size(), false);
    region(ebits.data(), ebits.n, true);
    col.dict = true;
    col.values = (uintptr_t)keys.data();
    col.values_bytes = (int64_t)keys.size();
    col.ebits = (uintptr_t)ebits.data();
    col.dict_count = d.count;
  } else {
    col.values = (uintptr_t)c.values.data();
    col.offsets = c.kind == K_BYTES ? (uintptr_t)c.offsets.data() : 0;
    col.values_bytes = (int64_t)c.values.size();
    if (!c.values.empty()) region(c.values.data(), c.values.size(), false);
    if (c.kind == K_BYTES) region(c.offsets.data(), 8 * c.offsets.size(), false);
  }
  col.num_values = c.nv;
  int64_t got_sel, got_valid;
  model_filter(p, col, use_dict ? &d : nullptr, bm.data(), n, mode, &got_sel, &got_valid);
  if (g_fail) return;
  if (differ(bm.data(), want.data(), 4 * words)) FAIL("bitmap differs from the scalar loop");
  if (n > 0 && (got_sel != want_sel || got_valid != want_valid)) FAIL("num_selected / num_valid differ");
  if (!bm.intact() || !ebits.intact()) FAIL("guard bytes of a filter output changed");
}

static void select_case(const Column& c, int64_t n, int pattern) {
  g_cases++;
  g_regions.clear();
  const size_t words = (size_t)((n + 31) / 32);
  std::vector<uint32_t> bm(words, 0u);
  for (int64_t i = 0; i < n; i++) {
    bool s = false;
    switch (pattern) {
      case 0: s = false; break;
      case 1: s = true; break;
      case 2: s = i & 1; break;
      case 3: s = i % kSeg == 0; break;
      case 4: s = i % kSeg == kSeg - 1 || i == n - 1; break;
      case 5: s = rnd() % 100 == 0; break;
      default: s = rnd() & 1; break;
    }
    if (s) bm[(size_t)(i >> 5)] |= 1u << (i & 31);
  }
  if (words) bm[words - 1] |= n % 32 ? ~0u << (n % 32) : 0u;  // bits past n are ignored
  // the yardstick
  std::vector<uint8_t> wdef, wval;
  std::vector<int64_t> woff = {0};
  int64_t r = 0, wrows = 0, wvals = 0;
  for (int64_t i = 0; i < n; i++) {
    const bool valid = c.max_def == 0 || c.def[(size_t)i] == 1;
    const bool sel = (bm[(size_t)(i >> 5)] >> (i & 31)) & 1;
    if (sel) {
      wrows++;
      if (c.max_def) wdef.push_back(c.def[(size_t)i]);
      if (valid) {
        size_t len;
        const uint8_t* v = c.value(r, &len);
        wval.insert(wval.end(), v, v + len);
        woff.push_back((int64_t)wval.size());
        wvals++;
      }
    }
    if (valid) r++;
  }
  const bool var = c.kind == K_BYTES;
  Guarded odef(wdef.size()), oval(wval.size()), ooff(var ? 8 * woff.size() : 0);
  Sel a;
  memset(&a, 0, sizeof(a));
  a.bitmap = (uintptr_t)bm.data();
  a.def = c.max_def ? (uintptr_t)c.def.data() : 0;
  a.values = (uintptr_t)c.values.data();
  a.offsets = var ? (uintptr_t)c.offsets.data() : 0;
  a.out_def = c.max_def ? (uintptr_t)odef.data() : 0;
  a.out_values = (uintptr_t)oval.data();
  a.out_offsets = var ? (uintptr_t)ooff.data() : 0;
  a.n = n;
  a.num_values = c.nv;
  a.values_bytes = (int64_t)c.values.size();
  a.max_def = c.max_def;
  a.width = var ? 0 : c.width;
  if (words) region(bm.data(), 4 * words, false);
  if (c.max_def && n) region(c.def.data(), c.def.size(), false);
  if (!c.values.empty()) region(c.values.data(), c.values.size(), false);
  if (var) region(c.offsets.data(), 8 * c.offsets.size(), false);
  region(odef.data(), odef.n, true);
  region(oval.data(), oval.n, true);
  region(ooff.data(), ooff.n, true);
  int64_t rows, vals, bytes;
  model_select(a, &rows, &vals, &bytes);
  if (g_fail) return;
  if (n > 0) {
    if (rows != wrows || vals != wvals || bytes != (int64_t)wval.size()) FAIL("select counts differ");
    if (differ(odef.data(), wdef.data(), wdef.size())) FAIL("selected def levels differ");
    if (differ(oval.data(), wval.data(), wval.size())) FAIL("selected values differ");
    if (var && differ(ooff.data(), woff.data(), 8 * woff.size())) FAIL("selected offsets differ");
  }
  if (!odef.intact() || !oval.intact() || !ooff.intact()) FAIL("guard bytes of a select output changed");
  // a counting call writes nothing
  a.out_def = a.out_values = a.out_offsets = 0;
  g_regions.erase(g_regions.end() - 3, g_regions.end());
  int64_t r2, v2, b2;
  model_select(a, &r2, &v2, &b2);
  if (!g_fail && (r2 != rows || v2 != vals || b2 != bytes)) FAIL("the counting call's counts differ");
}

int main() {
  const int64_t ns[] = {0, 1, 33, 63, 64, 65, 4095, 4096, 4097, 8193, 3 * 4096 + 1};
  struct KW {
    int kind, width;
  };
  const KW kinds[] = {{K_I32, 0}, {K_U32, 0}, {K_I64, 0}, {K_U64, 0}, {K_F32, 0}, {K_F64, 0}, {K_U8, 0},
                      {K_FLBA, 3}, {K_FLBA, 16}, {K_FLBA, 17}, {K_BYTES, 0}};
  for (const KW& kw : kinds) {
    const int w = width_of(kw.kind, kw.width);
    const std::vector<std::string> dom = domain(kw.kind, w);
    for (int64_t n : ns)
      for (int nullpat = 0; nullpat < 5; nullpat++) {
        // long strings only in the small columns: a 5000-byte value per row is slow, not different
        std::vector<std::string> use = dom;
        if (kw.kind == K_BYTES && n > 100) use.pop_back();
        const Column c = make_column(kw.kind, w, n, nullpat, use);
        for (int op = 0; op < 8; op++) {
          const bool small = n <= 65;
          for (size_t li = 0; li < (small ? dom.size() : 1); li++) {
            const std::string& lit = dom[small ? li : (size_t)(op + n + nullpat) % dom.size()];
            for (int mode = 0; mode < 3; mode++) {
              if (!small && mode != (op + nullpat) % 3) continue;
              filter_case(c, n, op, lit, mode, false);
              if (!g_fail && (small || (op + n) % 2 == 0)) filter_case(c, n, op, lit, mode, true);
              if (g_fail) {
                printf("FAIL %s: kind %d width %d n %lld nulls %d op %d literal %zu mode %d\n", g_fail, kw.kind, w,
                       (long long)n, nullpat, op, li, mode);
                return 1;
              }
            }
          }
        }
      }
  }
  // select: every width (12: INT96; 3 / 17: FLBA; 4: int32 keys too), byte arrays, every bitmap pattern
  const KW sel_kinds[] = {{K_U8, 0}, {K_I32, 0}, {K_I64, 0}, {K_FLBA, 12}, {K_FLBA, 3}, {K_FLBA, 17}, {K_BYTES, 0}};
  for (const KW& kw : sel_kinds) {
    const int w = width_of(kw.kind, kw.width);
    const std::vector<std::string> dom = domain(kw.kind, w);
    for (int64_t n : ns)
      for (int nullpat = 0; nullpat < 5; nullpat++) {
        std::vector<std::string> use = dom;
        if (kw.kind == K_BYTES && n > 4097) use.pop_back();
        const Column c = make_column(kw.kind, w, n, nullpat, use);
        for (int pattern = 0; pattern < 7; pattern++) {
          select_case(c, n, pattern);
          if (g_fail) {
            printf("FAIL %s: select kind %d width %d n %lld nulls %d bitmap %d\n", g_fail, kw.kind, w, (long long)n,
                   nullpat, pattern);
            return 1;
          }
        }
      }
  }
  printf("ok %ld cases\n", g_cases);
  return 0;
}
