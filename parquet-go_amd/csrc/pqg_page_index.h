// pqg_page_index.h — parsers of the Parquet page index (OffsetIndex, ColumnIndex), host only.
//
// The definitions of pqg_parse_offset_index and pqg_column_index_* (include/pqgpu.h).  The header
// needs no HIP: pqg_file.cpp includes it for libpqgpu, tools/page_index_model.cpp to run the parsers
// on their own (under sanitizers).  Include it in one translation unit of a program.
//
// parquet.thrift: OffsetIndex {1: list<PageLocation>}, PageLocation {1: i64 offset, 2: i32
// compressed_page_size, 3: i64 first_row_index}; ColumnIndex {1: list<bool> null_pages, 2:
// list<binary> min_values, 3: list<binary> max_values, 4: BoundaryOrder, 5: list<i64> null_counts}.
// Nothing is trusted: a list longer than the bytes left, a missing required field, parallel lists of
// different lengths, a size <= 0, a negative or descending offset or first row, overlapping pages,
// a negative null count, an unknown boundary order and bytes left over are all PQG_ERR_METADATA.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pqgpu.h"
#include "pqg_thrift.h"

struct pqg_column_index {
  std::vector<uint8_t> null_pages;
  std::vector<std::string> mins, maxs;
  std::vector<int64_t> null_counts;  // empty: the index has none
  int32_t order = 0;
};

namespace pqg {
namespace pidx {

struct Mem {
  const uint8_t* p;
  int64_t n;
  int get(int64_t i) const { return (i >= 0 && i < n) ? p[i] : -1; }
};

struct Reader {
  Compact<Mem> c;
  SkipFrame frames[kMaxFrames];
  int16_t last[kMaxLast];
  Reader(const uint8_t* p, int64_t n) {
    c.src = Mem{p, n};
    c.pos = 0;
    c.frames = frames;
    c.last = last;
    c.nlast = 0;
    c.last_id = 0;
    c.bool_set = c.bool_val = false;
  }
  int64_t left() const { return c.src.n - c.pos; }
  // a list header; every element takes at least `min_bytes`, so a size past the bytes left is refused
  bool list(int want, int64_t min_bytes, int32_t* size) {
    uint8_t st;
    if (c.byte(&st)) return false;
    int32_t sz = (st >> 4) & 0x0f;
    if (sz == 15) {
      int64_t v;
      if (c.varint64(&v)) return false;
      if (v < 0 || v > INT32_MAX) return false;
      sz = (int32_t)v;
    }
    if (Compact<Mem>::ttype(st) != want) return false;
    if ((int64_t)sz * min_bytes > left()) return false;
    *size = sz;
    return true;
  }
  bool str(std::string* out) {
    int64_t v;
    if (c.varint64(&v)) return false;
    if (v < 0 || v > left()) return false;
    out->assign((const char*)c.src.p + c.pos, (size_t)v);
    c.pos += v;
    return true;
  }
  template <class F>
  bool fields(F&& f) {  // f: 1 handled, 0 skip it, -1 error
    if (c.struct_begin()) return false;
    for (;;) {
      int t, id;
      if (c.field_begin(&t, &id)) return false;
      if (t == T_STOP) break;
      const int r = f(t, id);
      if (r < 0) return false;
      if (r == 0 && c.skip(t, 64)) return false;
    }
    c.struct_end();
    return true;
  }
};

}  // namespace pidx
}  // namespace pqg

extern "C" {

int pqg_parse_offset_index(const uint8_t* buf, int64_t len, pqg_page_loc* out, int cap) {
  using namespace pqg;
  if (!buf || len < 0 || cap < 0 || (cap > 0 && !out)) return PQG_ERR_INVALID_ARG;
  pidx::Reader r(buf, len);
  bool seen = false;
  int32_t n = 0;
  int64_t end = 0, row = 0;  // of the page before
  const bool ok = r.fields([&](int t, int id) -> int {
    if (id != 1 || t != T_LIST || seen) return 0;
    seen = true;
    if (!r.list(T_STRUCT, 4, &n)) return -1;
    for (int32_t k = 0; k < n; k++) {
      pqg_page_loc l;
      memset(&l, 0, sizeof(l));
      int have = 0;
      const bool okl = r.fields([&](int t2, int id2) -> int {
        if (id2 == 1 && t2 == T_I64) { have |= 1; return r.c.i64(&l.offset) ? -1 : 1; }
        if (id2 == 2 && t2 == T_I32) { have |= 2; return r.c.i32(&l.size) ? -1 : 1; }
        if (id2 == 3 && t2 == T_I64) { have |= 4; return r.c.i64(&l.first_row) ? -1 : 1; }
        return 0;
      });
      if (!okl || have != 7) return -1;
      if (l.offset < 0 || l.size <= 0 || l.first_row < 0 || l.offset > INT64_MAX - l.size) return -1;
      if (k > 0 && (l.offset < end || l.first_row < row)) return -1;
      end = l.offset + l.size;
      row = l.first_row;
      if (k < cap) out[k] = l;
    }
    return 1;
  });
  if (!ok || !seen || r.c.pos != len) return PQG_ERR_METADATA;
  return n;
}

int pqg_column_index_parse(const uint8_t* buf, int64_t len, pqg_column_index** out) {
  using namespace pqg;
  if (!out) return PQG_ERR_INVALID_ARG;
  *out = nullptr;
  if (!buf || len < 0) return PQG_ERR_INVALID_ARG;
  pidx::Reader r(buf, len);
  pqg_column_index* ci = new pqg_column_index();
  int have = 0;
  const bool ok = r.fields([&](int t, int id) -> int {
    int32_t n = 0;
    if (id == 1 && t == T_LIST && !(have & 1)) {
      have |= 1;
      if (!r.list(T_BOOL, 1, &n)) return -1;
      for (int32_t k = 0; k < n; k++) {
        uint8_t b;
        if (r.c.byte(&b)) return -1;
        ci->null_pages.push_back(b == 1);
      }
      return 1;
    }
    if ((id == 2 || id == 3) && t == T_LIST && !(have & (id == 2 ? 2 : 4))) {
      have |= id == 2 ? 2 : 4;
      std::vector<std::string>& v = id == 2 ? ci->mins : ci->maxs;
      if (!r.list(T_STRING, 1, &n)) return -1;
      v.resize((size_t)n);
      for (int32_t k = 0; k < n; k++)
        if (!r.str(&v[(size_t)k])) return -1;
      return 1;
    }
    if (id == 4 && t == T_I32 && !(have & 8)) {
      have |= 8;
      return r.c.i32(&ci->order) ? -1 : 1;
    }
    if (id == 5 && t == T_LIST && !(have & 16)) {
      have |= 16;
      if (!r.list(T_I64, 1, &n)) return -1;
      for (int32_t k = 0; k < n; k++) {
        int64_t v;
        if (r.c.i64(&v) || v < 0) return -1;
        ci->null_counts.push_back(v);
      }
      return 1;
    }
    return 0;
  });
  const size_t np = ci->null_pages.size();
  if (!ok || r.c.pos != len || (have & 15) != 15 || ci->mins.size() != np || ci->maxs.size() != np ||
      ((have & 16) && ci->null_counts.size() != np) || ci->order < 0 || ci->order > 2) {
    delete ci;
    return PQG_ERR_METADATA;
  }
  *out = ci;
  return PQG_OK;
}

int pqg_column_index_pages(const pqg_column_index* ci) { return ci ? (int)ci->null_pages.size() : PQG_ERR_INVALID_ARG; }

int pqg_column_index_page(const pqg_column_index* ci, int page, pqg_chunk_stats* out, int32_t* null_page) {
  if (!ci || !out || page < 0 || page >= (int)ci->null_pages.size()) return PQG_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  const bool np = ci->null_pages[(size_t)page] != 0;
  if (null_page) *null_page = np ? 1 : 0;
  out->null_count = ci->null_counts.empty() ? -1 : ci->null_counts[(size_t)page];
  if (!np) {  // a null page has no bounds (its entries are empty strings)
    const std::string &lo = ci->mins[(size_t)page], &hi = ci->maxs[(size_t)page];
    out->min_value = (const uint8_t*)lo.data();
    out->min_len = (int32_t)lo.size();
    out->max_value = (const uint8_t*)hi.data();
    out->max_len = (int32_t)hi.size();
  }
  return PQG_OK;
}

int pqg_column_index_boundary_order(const pqg_column_index* ci) { return ci ? ci->order : PQG_ERR_INVALID_ARG; }

void pqg_column_index_free(pqg_column_index* ci) { delete ci; }

}  // extern "C"
