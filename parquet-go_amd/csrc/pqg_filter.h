// pqg_filter.h — K9s: what one lane of k_flt_* / k_sel_* (pqg_filter.hip) computes, loads and
// stores, written over an IO policy so that a host program runs the same code on plain memory
// (tools/filter_model.cpp): the comparison of one value against a literal for every physical
// type, the pass / fail of a row under the eight operators, the combine of a 32-row bitmap
// dword, and the placement of a selected row's def level, value, offset and short chars.
// Wave-level glue (ballots, ranks = popcount(mask & lanes below), the scan of value lengths,
// the wave copy of long values) is the kernel's and the model's own.
//
// Rows are those of a flat column: row i is null when def[i] < max_def, and dense value r
// belongs to the r-th non-null row.  Comparison orders (include/pqgpu.h, pqg_filter):
// signed / unsigned integers, IEEE floats (a NaN on either side is unordered: it fails every
// operator but NE), BOOLEAN as a byte, byte strings unsigned lexicographic (a proper prefix
// sorts first); K_FLBA_SBE (PQG_COL_SIGNED_BE: a DECIMAL's big-endian two's complement) the same
// with bit 7 of byte 0 flipped on both sides.  A null row passes IS_NULL only.
//
// IO: u8 / u32 / u64 (address) loads and st8 / st32 / st64 (address, value) stores, every
// access naturally aligned; eword(base, j) reads dword j of the dictionary-entry bitmap (the
// device keeps it in LDS or reads it through L2).
#pragma once
#include <stdint.h>
#include <string.h>

#include "pqg_common.h"

namespace pqg {
namespace flt {

constexpr int kSeg = 4096;       // rows per wave segment (64 ballots), as K8
constexpr int kLongValue = 64;   // byte-array values longer than this are copied by the whole wave
constexpr int kLdsEntries = 65536;  // dictionaries up to this many entries may stage their entry bitmap in LDS (8 KiB)

enum : int { OP_EQ = 0, OP_NE = 1, OP_LT = 2, OP_LE = 3, OP_GT = 4, OP_GE = 5, OP_IS_NULL = 6, OP_NOT_NULL = 7 };
enum : int { M_SET = 0, M_AND = 1, M_OR = 2 };
enum : int { K_I32 = 0, K_U32, K_I64, K_U64, K_F32, K_F64, K_U8, K_FLBA, K_BYTES, K_FLBA_SBE };
enum : int { C_LT = -1, C_EQ = 0, C_GT = 1, C_UN = 2 };  // C_UN: unordered (NaN)

// One comparison, as the kernels take it.
struct Pred {
  int kind, op, width;  // width: bytes per fixed-width value (K_FLBA / K_FLBA_SBE: type_length; K_BYTES: 0)
  uint64_t lit;         // numeric kinds: the literal's bits
  uintptr_t lit_bytes;  // byte kinds: the literal's bytes (an address the IO reads)
  int64_t lit_len;
};

// The column a predicate reads.  With `dict` the values are int32 keys and ebits holds one
// bit per dictionary entry (entry_pass).
struct Col {
  uintptr_t def, values, offsets;  // def 0: every row valid; offsets: K_BYTES only
  int64_t num_values, values_bytes;
  int max_def;
  bool dict;
  uintptr_t ebits;
  int64_t dict_count;
};

__host__ __device__ __forceinline__ bool op_pass(int op, int c) {
  switch (op) {
    case OP_EQ: return c == C_EQ;
    case OP_NE: return c != C_EQ;
    case OP_LT: return c == C_LT;
    case OP_LE: return c == C_LT || c == C_EQ;
    case OP_GT: return c == C_GT;
    case OP_GE: return c == C_GT || c == C_EQ;
  }
  return false;
}

template <class T>
__host__ __device__ __forceinline__ int cmp3(T a, T b) {
  return a < b ? C_LT : a > b ? C_GT : a == b ? C_EQ : C_UN;
}
__host__ __device__ __forceinline__ float f32_of(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}
__host__ __device__ __forceinline__ double f64_of(uint64_t b) {
  double f;
  memcpy(&f, &b, 8);
  return f;
}

// value bits `a` of a numeric kind against the literal
__host__ __device__ __forceinline__ int cmp_bits(int kind, uint64_t a, uint64_t lit) {
  switch (kind) {
    case K_I32: return cmp3((int32_t)(uint32_t)a, (int32_t)(uint32_t)lit);
    case K_U32: return cmp3((uint32_t)a, (uint32_t)lit);
    case K_I64: return cmp3((int64_t)a, (int64_t)lit);
    case K_U64: return cmp3(a, lit);
    case K_F32: return cmp3(f32_of((uint32_t)a), f32_of((uint32_t)lit));
    case K_F64: return cmp3(f64_of(a), f64_of(lit));
    default: return cmp3((uint32_t)(a & 0xff), (uint32_t)(lit & 0xff));  // K_U8
  }
}

// bytes [a, a + alen) against [b, b + blen): unsigned lexicographic, a proper prefix first.
// zero_a: a reads as alen zero bytes (a dictionary's nil entry) and is not loaded.  flip0 is
// xor-ed into byte 0 of both sides: 0x80 orders big-endian two's complement (K_FLBA_SBE).
template <class IO>
__host__ __device__ __forceinline__ int cmp_bytes(const IO& io, uintptr_t a, int64_t alen, uintptr_t b, int64_t blen,
                                                  bool zero_a = false, uint32_t flip0 = 0) {
  const int64_t n = alen < blen ? alen : blen;
  for (int64_t i = 0; i < n; i++) {
    const uint32_t f = i == 0 ? flip0 : 0u;
    const uint32_t x = (zero_a ? 0u : io.u8(a + (uintptr_t)i)) ^ f, y = io.u8(b + (uintptr_t)i) ^ f;
    if (x != y) return x < y ? C_LT : C_GT;
  }
  return alen < blen ? C_LT : alen > blen ? C_GT : C_EQ;
}

// the bits of fixed-width value idx of a numeric kind
template <class IO>
__host__ __device__ __forceinline__ uint64_t load_bits(const IO& io, int kind, uintptr_t values, int64_t idx) {
  if (kind == K_I64 || kind == K_U64 || kind == K_F64) return io.u64(values + 8 * (uintptr_t)idx);
  if (kind == K_U8) return io.u8(values + (uintptr_t)idx);
  return io.u32(values + 4 * (uintptr_t)idx);
}

// Value idx of (values, offsets) against the literal.  values_bytes bounds what is read: a
// byte-array value whose offsets do not lie inside it compares unordered (nothing is loaded).
template <class IO>
__host__ __device__ __forceinline__ int cmp_value(const IO& io, const Pred& p, uintptr_t values, uintptr_t offsets,
                                                  int64_t values_bytes, int64_t idx) {
  if (p.kind == K_BYTES) {
    const int64_t o0 = (int64_t)io.u64(offsets + 8 * (uintptr_t)idx), o1 = (int64_t)io.u64(offsets + 8 * (uintptr_t)idx + 8);
    if (o0 < 0 || o1 < o0 || o1 > values_bytes) return C_UN;
    return cmp_bytes(io, values + (uintptr_t)o0, o1 - o0, p.lit_bytes, p.lit_len);
  }
  if (p.kind == K_FLBA) return cmp_bytes(io, values + (uintptr_t)idx * (uintptr_t)p.width, p.width, p.lit_bytes, p.lit_len);
  if (p.kind == K_FLBA_SBE)
    return cmp_bytes(io, values + (uintptr_t)idx * (uintptr_t)p.width, p.width, p.lit_bytes, p.lit_len, false, 0x80u);
  return cmp_bits(p.kind, load_bits(io, p.kind, values, idx), p.lit);
}

// Dictionary entry e under the predicate (one bit of the entry bitmap).  A fixed-width entry
// that is the nil entry, or whose bytes the page does not hold, reads as zero bytes.
template <class IO>
__host__ __device__ __forceinline__ bool entry_pass(const IO& io, const Pred& p, uintptr_t values, uintptr_t offsets,
                                                    int64_t values_bytes, int64_t nil_entry, int64_t e) {
  if (p.kind != K_BYTES) {
    const int64_t w = p.width;
    if (e == nil_entry || (e + 1) * w > values_bytes) {
      if (p.kind == K_FLBA) return op_pass(p.op, cmp_bytes(io, 0, w, p.lit_bytes, p.lit_len, true));
      if (p.kind == K_FLBA_SBE) return op_pass(p.op, cmp_bytes(io, 0, w, p.lit_bytes, p.lit_len, true, 0x80u));
      return op_pass(p.op, cmp_bits(p.kind, 0, p.lit));
    }
  }
  if (p.kind != K_BYTES && p.kind != K_FLBA && p.kind != K_FLBA_SBE) {
    // a dictionary page's entries lie where the file put them: no alignment, so byte loads
    uint64_t bits = 0;
    for (int k = 0; k < p.width; k++) bits |= (uint64_t)io.u8(values + (uintptr_t)(e * p.width + k)) << (8 * k);
    return op_pass(p.op, cmp_bits(p.kind, bits, p.lit));
  }
  return op_pass(p.op, cmp_value(io, p, values, offsets, values_bytes, e));
}

template <class IO>
__host__ __device__ __forceinline__ bool row_valid(const IO& io, uintptr_t def, int64_t i, int max_def) {
  return def == 0 || io.u8(def + (uintptr_t)i) == (uint32_t)(uint8_t)max_def;
}

// Row of the column under the predicate: `valid` from row_valid, rank = non-null rows before
// it.  A rank at or past num_values (levels and values that do not belong together) fails.
template <class IO>
__host__ __device__ __forceinline__ bool row_pass(const IO& io, const Pred& p, const Col& c, bool valid, int64_t rank) {
  if (p.op == OP_IS_NULL) return !valid;
  if (!valid || rank >= c.num_values) return false;
  if (p.op == OP_NOT_NULL) return true;
  if (c.dict) {
    const uint32_t k = io.u32(c.values + 4 * (uintptr_t)rank);
    if ((int64_t)k >= c.dict_count) return false;  // a negative key is a large unsigned one
    return (io.eword(c.ebits, (int64_t)(k >> 5)) >> (k & 31)) & 1u;
  }
  return op_pass(p.op, cmp_value(io, p, c.values, c.offsets, c.values_bytes, rank));
}

__host__ __device__ __forceinline__ int popc32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(v);
#else
  return __builtin_popcount(v);
#endif
}

// The 64 rows from row b (a multiple of 64) own bitmap dwords b / 32 and b / 32 + 1; lane 0
// stores the first, lane 1 the second, when it holds a row below n.  pass / in: the ballots
// of the rows that pass and of the rows below n.  Bits of rows at and past n are stored as
// zero in every mode.  Returns the rows selected in the dword stored (0 for other lanes).
template <class IO>
__host__ __device__ __forceinline__ int store_word(const IO& io, uintptr_t bitmap, int64_t b, int64_t n, int lane,
                                                   uint64_t pass, uint64_t in, int mode) {
  if (lane >= 2) return 0;
  const int64_t r0 = b + 32 * lane;
  if (r0 >= n) return 0;
  const uintptr_t at = bitmap + 4 * (uintptr_t)(r0 >> 5);
  const uint32_t bits = (uint32_t)(pass >> (32 * lane)), inm = (uint32_t)(in >> (32 * lane));
  uint32_t v = bits;
  if (mode == M_AND) v = io.u32(at) & bits;
  if (mode == M_OR) v = io.u32(at) | bits;
  v &= inm;
  io.st32(at, v);
  return popc32(v);
}

// ---- pqg_select: compaction of one column by a row bitmap ---------------------------------------
struct Sel {
  uintptr_t bitmap, def, values, offsets;      // in
  uintptr_t out_def, out_values, out_offsets;  // out; 0: not written
  int64_t n, num_values, values_bytes;
  int max_def, width;  // width 0: byte arrays
};

// row i (in: i < n): selected, and non-null
template <class IO>
__host__ __device__ __forceinline__ void sel_flags(const IO& io, const Sel& a, int64_t i, bool in, bool* sel, bool* valid) {
  *sel = in && ((io.u32(a.bitmap + 4 * (uintptr_t)(i >> 5)) >> (i & 31)) & 1u);
  *valid = in && row_valid(io, a.def, i, a.max_def);
}

// Byte arrays: where dense value src lies in the chars and how long it is (0 when its
// offsets do not lie inside values_bytes: such a value is copied as an empty one).
template <class IO>
__host__ __device__ __forceinline__ int64_t sel_len(const IO& io, const Sel& a, int64_t src, int64_t* at) {
  const int64_t o0 = (int64_t)io.u64(a.offsets + 8 * (uintptr_t)src), o1 = (int64_t)io.u64(a.offsets + 8 * (uintptr_t)src + 8);
  *at = 0;
  if (o0 < 0 || o1 < o0 || o1 > a.values_bytes) return 0;
  *at = o0;
  return o1 - o0;
}

// The stores of one selected row: its def level at out row drow; when it is non-null (sv) its
// value src at out value dval: w bytes, or for byte arrays the offset dchar and, unless the
// value is a long one (the wave copies those), its len chars from chars offset at.
template <class IO>
__host__ __device__ __forceinline__ void sel_store(const IO& io, const Sel& a, int64_t i, bool sel, bool sv, int64_t src,
                                                   int64_t drow, int64_t dval, int64_t dchar, int64_t at, int64_t len) {
  if (sel && a.def && a.out_def) io.st8(a.out_def + (uintptr_t)drow, io.u8(a.def + (uintptr_t)i));
  if (!sv) return;
  if (a.width == 0) {
    if (a.out_offsets) io.st64(a.out_offsets + 8 * (uintptr_t)dval, (uint64_t)dchar);
    if (a.out_values && len <= kLongValue)
      for (int64_t k = 0; k < len; k++) io.st8(a.out_values + (uintptr_t)(dchar + k), io.u8(a.values + (uintptr_t)(at + k)));
    return;
  }
  if (!a.out_values) return;
  const uintptr_t w = (uintptr_t)a.width, s = a.values + (uintptr_t)src * w, d = a.out_values + (uintptr_t)dval * w;
  if (a.width == 8 && ((s | d) & 7) == 0) {
    io.st64(d, io.u64(s));
  } else if ((a.width & 3) == 0 && ((s | d) & 3) == 0) {
    for (uintptr_t k = 0; k < w; k += 4) io.st32(d + k, io.u32(s + k));
  } else {
    for (uintptr_t k = 0; k < w; k++) io.st8(d + k, io.u8(s + k));
  }
}

}  // namespace flt
}  // namespace pqg
