// pqg_file.cpp — host-side planner: footer + schema → column-chunk jobs.
//
// Replaces readFileMetaData (file_meta.go:14-62) and makeSchema / readSchema /
// readGroupSchema / readColumnSchema (schema.go:789-919, 996-1025): PAR1 magic
// at both ends, i32 LE footer length (> 0), thrift FileMetaData, then leaf
// columns in depth-first order with maxD (+1 per non-REQUIRED element) and maxR
// (+1 per REPEATED element).  Row group r's chunk for leaf i is
// RowGroup.columns[i] (readRowGroup chunk_reader.go:404-431).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pqgpu.h"
#include "pqg_thrift.h"
#include "pqg_page_index.h"  // defines pqg_parse_offset_index and pqg_column_index_*

using namespace pqg;

namespace {

struct MemSrc {
  const uint8_t* p;
  int64_t n;
  int get(int64_t i) const { return (i >= 0 && i < n) ? p[i] : -1; }
};

struct Elem {
  bool has_type = false, has_tl = false, has_rep = false, has_nc = false, has_ct = false;
  int32_t type = 0, type_length = 0, rep = 0, num_children = 0, converted = 0;
  bool unsigned_int = false;
  bool has_scale = false, has_precision = false;
  int32_t scale = 0, precision = 0;
  pqg_logical_type lt;  // from the LogicalType union alone; kind PQG_LT_NONE without one that parses
  int32_t group_lt = -1;  // PQG_NODE_* of the LogicalType union's member, -1 without one that parses
  std::string name;
  Elem() { memset(&lt, 0, sizeof(lt)); }
};

struct ChunkM {
  bool has_meta = false, has_path = false, has_dict = false;
  int32_t type = 0, codec = 0;
  int64_t num_values = 0, tus = 0, tcs = 0, data_off = 0, dict_off = 0;
  // Statistics (field 12): null_count, max_value, min_value
  bool has_nulls = false, has_min = false, has_max = false;
  int64_t null_count = 0;
  std::string min_value, max_value;
  // ColumnChunk fields 4-7: where the chunk's OffsetIndex / ColumnIndex lie in the file (length 0: none)
  int64_t oi_off = 0, ci_off = 0;
  int32_t oi_len = 0, ci_len = 0;
};

struct Leaf {
  pqg_column_desc desc;
  pqg_logical_type logical;
  std::string path;
};

struct Parser {
  Compact<MemSrc> c;
  SkipFrame frames[kMaxFrames];
  int16_t last[kMaxLast];
  bool stats_bad = false;  // a Statistics struct that did not parse: the file reports none
  explicit Parser(const uint8_t* p, int64_t n) {
    c.src = MemSrc{p, n};
    c.pos = 0;
    c.frames = frames;
    c.last = last;
    c.nlast = 0;
    c.last_id = 0;
    c.bool_set = c.bool_val = false;
  }
  bool str(std::string* out) {
    int64_t v;
    if (c.varint64(&v)) return false;
    int32_t len = (int32_t)v;
    if (len < 0) return false;
    if (len == 0) {
      out->clear();
      return true;
    }
    if (c.src.get(c.pos + len - 1) < 0) return false;
    out->assign((const char*)c.src.p + c.pos, (size_t)len);
    c.pos += len;
    return true;
  }
  bool list(int* et, int32_t* size) {
    uint8_t st;
    if (c.byte(&st)) return false;
    int32_t sz = (st >> 4) & 0x0f;
    if (sz == 15) {
      int64_t v;
      if (c.varint64(&v)) return false;
      sz = (int32_t)v;
      if (sz < 0) return false;
    }
    int t = Compact<MemSrc>::ttype(st);
    if (t < 0) return false;
    *et = t;
    *size = sz;
    return true;
  }
  // generic field loop
  template <class F>
  bool fields(F&& f) {
    if (c.struct_begin()) return false;
    for (;;) {
      int t, id;
      if (c.field_begin(&t, &id)) return false;
      if (t == T_STOP) break;
      int r = f(t, id);  // 1 handled ok, 0 not handled, -1 error
      if (r < 0) return false;
      if (r == 0 && c.skip(t, 64)) return false;
    }
    c.struct_end();
    return true;
  }
  bool logical_unsigned(bool* uns) {
    // LogicalType union; INTEGER = field 10: IntType{1: bitWidth byte, 2: isSigned bool}
    return fields([&](int t, int id) -> int {
      if (id == 10 && t == T_STRUCT) {
        bool ok = fields([&](int t2, int id2) -> int {
          if (id2 == 2 && t2 == T_BOOL) {
            bool s;
            if (c.read_bool(&s)) return -1;
            *uns = !s;
            return 1;
          }
          return 0;
        });
        return ok ? 1 : -1;
      }
      return 0;
    });
  }
  // LogicalType union: the member set last wins, as in a thrift union read
  static void logical(const uint8_t* p, int64_t n, pqg_logical_type* out) {
    Parser q(p, n);
    pqg_logical_type lt;
    memset(&lt, 0, sizeof(lt));
    const bool ok = q.fields([&](int t, int id) -> int {
      if (t != T_STRUCT) return 0;
      pqg_logical_type m;
      memset(&m, 0, sizeof(m));
      int kind = PQG_LT_OTHER;
      switch (id) {
        case 1: kind = PQG_LT_STRING; break;
        case 4: kind = PQG_LT_ENUM; break;
        case 5: kind = PQG_LT_DECIMAL; break;
        case 6: kind = PQG_LT_DATE; break;
        case 7: kind = PQG_LT_TIME; break;
        case 8: kind = PQG_LT_TIMESTAMP; break;
        case 10: kind = PQG_LT_INTEGER; break;
        case 12: kind = PQG_LT_JSON; break;
        case 13: kind = PQG_LT_BSON; break;
        case 14: kind = PQG_LT_UUID; break;
        case 15: kind = PQG_LT_FLOAT16; break;
      }
      m.kind = kind;
      const bool okm = q.fields([&](int t2, int id2) -> int {
        int32_t v;
        if (kind == PQG_LT_DECIMAL && t2 == T_I32 && (id2 == 1 || id2 == 2)) {
          if (q.c.i32(&v)) return -1;
          (id2 == 1 ? m.scale : m.precision) = v;
          return 1;
        }
        if ((kind == PQG_LT_TIME || kind == PQG_LT_TIMESTAMP) && id2 == 1 && t2 == T_BOOL) {
          bool b;
          if (q.c.read_bool(&b)) return -1;
          m.utc = b ? 1 : 0;
          return 1;
        }
        if ((kind == PQG_LT_TIME || kind == PQG_LT_TIMESTAMP) && id2 == 2 && t2 == T_STRUCT) {
          // TimeUnit union: 1 MILLIS, 2 MICROS, 3 NANOS (empty structs)
          return q.fields([&](int t3, int id3) -> int {
            if (t3 == T_STRUCT && id3 >= 1 && id3 <= 3) m.unit = PQG_UNIT_MILLIS + (id3 - 1);
            return 0;
          }) ? 1 : -1;
        }
        if (kind == PQG_LT_INTEGER && id2 == 1 && t2 == T_BYTE) {
          uint8_t b;
          if (q.c.byte(&b)) return -1;
          m.bit_width = (int8_t)b;
          return 1;
        }
        if (kind == PQG_LT_INTEGER && id2 == 2 && t2 == T_BOOL) {
          bool b;
          if (q.c.read_bool(&b)) return -1;
          m.is_signed = b ? 1 : 0;
          return 1;
        }
        return 0;
      });
      if (!okm) return -1;
      lt = m;
      return 1;
    });
    if (ok && q.c.pos == n) *out = lt;
  }
  // LogicalType union: MAP (2) / LIST (3) or another member, the member set last wins; -1 when it does not parse
  static int32_t group_annotation(const uint8_t* p, int64_t n) {
    Parser q(p, n);
    int32_t kind = -1;
    const bool ok = q.fields([&](int t, int id) -> int {
      if (t == T_STRUCT) kind = id == 2 ? PQG_NODE_MAP : id == 3 ? PQG_NODE_LIST : PQG_NODE_PLAIN;
      return 0;
    });
    return ok && q.c.pos == n ? kind : -1;
  }
  bool elem(Elem* e) {
    return fields([&](int t, int id) -> int {
      int32_t v;
      switch (id) {
        case 1: if (t == T_I32) { if (c.i32(&v)) return -1; e->type = v; e->has_type = true; return 1; } break;
        case 2: if (t == T_I32) { if (c.i32(&v)) return -1; e->type_length = v; e->has_tl = true; return 1; } break;
        case 3: if (t == T_I32) { if (c.i32(&v)) return -1; e->rep = v; e->has_rep = true; return 1; } break;
        case 4: if (t == T_STRING) { return str(&e->name) ? 1 : -1; } break;
        case 5: if (t == T_I32) { if (c.i32(&v)) return -1; e->num_children = v; e->has_nc = true; return 1; } break;
        case 6: if (t == T_I32) { if (c.i32(&v)) return -1; e->converted = v; e->has_ct = true; return 1; } break;
        case 7: if (t == T_I32) { if (c.i32(&v)) return -1; e->scale = v; e->has_scale = true; return 1; } break;
        case 8: if (t == T_I32) { if (c.i32(&v)) return -1; e->precision = v; e->has_precision = true; return 1; } break;
        case 10:
          if (t == T_STRUCT) {
            // read as before (its parse decides whether the footer opens), then once more from its
            // own bytes for the logical type: what that finds or fails on changes nothing else
            const int64_t s0 = c.pos;
            if (!logical_unsigned(&e->unsigned_int)) return -1;
            logical(c.src.p + s0, c.pos - s0, &e->lt);
            e->group_lt = group_annotation(c.src.p + s0, c.pos - s0);
            return 1;
          }
          break;
      }
      return 0;
    });
  }
  bool meta(ChunkM* m) {
    return fields([&](int t, int id) -> int {
      int32_t v;
      int64_t w;
      switch (id) {
        case 1: if (t == T_I32) { if (c.i32(&v)) return -1; m->type = v; return 1; } break;
        case 4: if (t == T_I32) { if (c.i32(&v)) return -1; m->codec = v; return 1; } break;
        case 5: if (t == T_I64) { if (c.i64(&w)) return -1; m->num_values = w; return 1; } break;
        case 6: if (t == T_I64) { if (c.i64(&w)) return -1; m->tus = w; return 1; } break;
        case 7: if (t == T_I64) { if (c.i64(&w)) return -1; m->tcs = w; return 1; } break;
        case 9: if (t == T_I64) { if (c.i64(&w)) return -1; m->data_off = w; return 1; } break;
        case 11: if (t == T_I64) { if (c.i64(&w)) return -1; m->dict_off = w; m->has_dict = true; return 1; } break;
        case 12:
          if (t == T_STRUCT) {
            // skipped exactly as an unknown field is, then read from its own bytes: a
            // statistics struct never changes whether or how the footer parses
            const int64_t s0 = c.pos;
            if (c.skip(t, 64)) return -1;
            if (!stats(c.src.p + s0, c.pos - s0, m)) stats_bad = true;
            return 1;
          }
          break;
      }
      return 0;
    });
  }
  // Statistics: 3 null_count, 5 max_value, 6 min_value; the deprecated max / min (1, 2)
  // and everything else are skipped
  static bool stats(const uint8_t* p, int64_t n, ChunkM* m) {
    Parser q(p, n);
    ChunkM s;
    const bool ok = q.fields([&](int t, int id) -> int {
      if (id == 3 && t == T_I64) {
        if (q.c.i64(&s.null_count)) return -1;
        s.has_nulls = true;
        return 1;
      }
      if (id == 5 && t == T_STRING) {
        s.has_max = true;
        return q.str(&s.max_value) ? 1 : -1;
      }
      if (id == 6 && t == T_STRING) {
        s.has_min = true;
        return q.str(&s.min_value) ? 1 : -1;
      }
      return 0;
    });
    if (!ok || q.c.pos != n) return false;
    m->has_nulls = s.has_nulls;
    m->has_min = s.has_min;
    m->has_max = s.has_max;
    m->null_count = s.null_count;
    m->min_value = s.min_value;
    m->max_value = s.max_value;
    return true;
  }
  bool chunk(ChunkM* m) {
    return fields([&](int t, int id) -> int {
      if (id == 1 && t == T_STRING) {
        std::string s;
        if (!str(&s)) return -1;
        m->has_path = true;
        return 1;
      }
      if (id == 3 && t == T_STRUCT) {
        m->has_meta = true;
        return meta(m) ? 1 : -1;
      }
      if ((id == 4 || id == 6) && t == T_I64) return c.i64(id == 4 ? &m->oi_off : &m->ci_off) ? -1 : 1;
      if ((id == 5 || id == 7) && t == T_I32) return c.i32(id == 5 ? &m->oi_len : &m->ci_len) ? -1 : 1;
      return 0;
    });
  }
};

}  // namespace

struct SNode {
  std::string name;
  int32_t rep, num_children, leaf, max_def, max_rep;
  int32_t kind = PQG_NODE_PLAIN;  // PQG_NODE_*: the group's LIST / MAP annotation
};

struct pqg_file {
  std::vector<Leaf> leaves;
  std::vector<SNode> nodes;  // schema tree below the root, depth first
  std::vector<std::vector<ChunkM>> rgs;
  std::vector<int64_t> rg_rows;
  int64_t num_rows = 0;
  bool stats_bad = false;
};

namespace {

// schema.go:789-894 (readColumnSchema / readGroupSchema), depth-first.
bool read_schema(const std::vector<Elem>& s, size_t& idx, const std::string& name, int d, int r,
                 std::vector<Leaf>& out, int depth, std::vector<SNode>& nodes) {
  if (depth > 256 || idx >= s.size()) return false;
  const Elem& e = s[idx];
  if (!e.has_type) {  // group
    if (!e.has_nc || e.num_children <= 0) return false;
    if (s.size() <= idx + (size_t)e.num_children) return false;
    if (e.has_rep && e.rep != 0) d++;
    if (e.has_rep && e.rep == 2) r++;
    std::string nm = name.empty() ? e.name : name + "." + e.name;
    int32_t kind = PQG_NODE_PLAIN;  // the LogicalType's LIST / MAP, else the converted type's
    if (e.group_lt > PQG_NODE_PLAIN) kind = e.group_lt;
    else if (e.has_ct && e.converted == 3) kind = PQG_NODE_LIST;
    else if (e.has_ct && (e.converted == 1 || e.converted == 2)) kind = PQG_NODE_MAP;
    nodes.push_back(SNode{e.name, e.has_rep ? e.rep : 0, e.num_children, -1, d, r, kind});
    idx++;
    for (int i = 0; i < e.num_children; i++)
      if (!read_schema(s, idx, nm, d, r, out, depth + 1, nodes)) return false;
    return true;
  }
  if (e.name.empty() || !e.has_rep) return false;
  if (e.rep != 0) d++;
  if (e.rep == 2) r++;
  if (e.type == 7 && !e.has_tl) return false;  // getValuesStore: nil type len
  if (e.type < 0 || e.type > 7) return false;
  Leaf l;
  memset(&l.desc, 0, sizeof(l.desc));
  l.desc.physical_type = e.type;
  l.desc.type_length = e.has_tl ? e.type_length : -1;
  l.desc.max_def = d;
  l.desc.max_rep = r;
  bool uns = e.unsigned_int;
  if (e.has_ct && ((e.type == 1 && (e.converted == 11 || e.converted == 12 || e.converted == 13)) ||
                   (e.type == 2 && e.converted == 14)))
    uns = true;
  l.desc.flags = uns ? 1 : 0;
  l.logical = e.lt;
  if (l.logical.kind == PQG_LT_NONE && e.has_ct) {  // a writer of converted types only
    pqg_logical_type& g = l.logical;
    const int ct = e.converted;
    switch (ct) {
      case 0: g.kind = PQG_LT_STRING; break;
      case 4: g.kind = PQG_LT_ENUM; break;
      case 5:
        g.kind = PQG_LT_DECIMAL;
        g.scale = e.has_scale ? e.scale : 0;
        g.precision = e.has_precision ? e.precision : 0;
        break;
      case 6: g.kind = PQG_LT_DATE; break;
      case 7: case 8:
        g.kind = PQG_LT_TIME;
        g.unit = ct == 7 ? PQG_UNIT_MILLIS : PQG_UNIT_MICROS;
        g.utc = 1;
        break;
      case 9: case 10:
        g.kind = PQG_LT_TIMESTAMP;
        g.unit = ct == 9 ? PQG_UNIT_MILLIS : PQG_UNIT_MICROS;
        g.utc = 1;
        break;
      case 11: case 12: case 13: case 14: case 15: case 16: case 17: case 18:
        g.kind = PQG_LT_INTEGER;
        g.bit_width = 8 << ((ct - 11) & 3);
        g.is_signed = ct >= 15;
        break;
      case 19: g.kind = PQG_LT_JSON; break;
      case 20: g.kind = PQG_LT_BSON; break;
    }
  }
  l.logical.converted_type = e.has_ct ? e.converted : -1;
  l.path = name.empty() ? e.name : name + "." + e.name;
  nodes.push_back(SNode{e.name, e.rep, 0, (int32_t)out.size(), d, r});
  out.push_back(l);
  idx++;
  return true;
}

}  // namespace

extern "C" {

static int open_footer(const uint8_t* footer, int32_t fl, pqg_file** out);

int pqg_file_open(const uint8_t* file, int64_t len, pqg_file** out) {
  if (!file || !out || len < 0) return PQG_ERR_INVALID_ARG;
  return pqg_file_open_tail(file, len, file, len, len, out);
}

// readFileMetaData (file_meta.go:14-62) from the file's first bytes and its
// last tail_len bytes only: what a range reader fetches before planning.
int pqg_file_open_tail(const uint8_t* head, int64_t head_len, const uint8_t* tail, int64_t tail_len, int64_t file_len,
                       pqg_file** out) {
  if (!head || !tail || !out || head_len < 0 || tail_len < 0 || file_len < 0 || tail_len > file_len)
    return PQG_ERR_INVALID_ARG;
  *out = nullptr;
  if (head_len < 4 || memcmp(head, "PAR1", 4) != 0) return PQG_ERR_METADATA;
  if (tail_len < 8 || memcmp(tail + tail_len - 4, "PAR1", 4) != 0) return PQG_ERR_METADATA;
  int32_t fl;
  memcpy(&fl, tail + tail_len - 8, 4);
  if (fl <= 0) return PQG_ERR_METADATA;
  if ((int64_t)fl + 8 > file_len) return PQG_ERR_METADATA;
  if ((int64_t)fl + 8 > tail_len) return PQG_ERR_INVALID_ARG;  // fetch the last fl + 8 bytes
  return open_footer(tail + tail_len - 8 - fl, fl, out);
}

static int open_footer(const uint8_t* footer, int32_t fl, pqg_file** out) {
  Parser P(footer, fl);
  std::vector<Elem> schema;
  std::vector<std::vector<ChunkM>> rgs;
  std::vector<int64_t> rg_rows;
  int64_t num_rows = 0;
  bool ok = P.fields([&](int t, int id) -> int {
    if (id == 2 && t == T_LIST) {
      int et;
      int32_t n;
      if (!P.list(&et, &n) || et != T_STRUCT) return -1;
      for (int32_t i = 0; i < n; i++) {
        Elem e;
        if (!P.elem(&e)) return -1;
        schema.push_back(e);
      }
      return 1;
    }
    if (id == 3 && t == T_I64) return P.c.i64(&num_rows) ? -1 : 1;
    if (id == 4 && t == T_LIST) {
      int et;
      int32_t n;
      if (!P.list(&et, &n) || et != T_STRUCT) return -1;
      for (int32_t i = 0; i < n; i++) {
        std::vector<ChunkM> cols;
        int64_t rows = 0;
        bool okr = P.fields([&](int t2, int id2) -> int {
          if (id2 == 1 && t2 == T_LIST) {
            int et2;
            int32_t n2;
            if (!P.list(&et2, &n2) || et2 != T_STRUCT) return -1;
            for (int32_t k = 0; k < n2; k++) {
              ChunkM m;
              if (!P.chunk(&m)) return -1;
              cols.push_back(m);
            }
            return 1;
          }
          if (id2 == 3 && t2 == T_I64) return P.c.i64(&rows) ? -1 : 1;
          return 0;
        });
        if (!okr) return -1;
        rgs.push_back(cols);
        rg_rows.push_back(rows);
      }
      return 1;
    }
    return 0;
  });
  if (!ok || schema.empty()) return PQG_ERR_METADATA;
  pqg_file* f = new pqg_file();
  size_t idx = 1;  // makeSchema: readSchema(meta.Schema[1:])
  while (idx < schema.size()) {
    if (!read_schema(schema, idx, "", 0, 0, f->leaves, 0, f->nodes)) {
      delete f;
      return PQG_ERR_METADATA;
    }
  }
  f->rgs = rgs;
  f->rg_rows = rg_rows;
  f->num_rows = num_rows;
  f->stats_bad = P.stats_bad;
  *out = f;
  return PQG_OK;
}

void pqg_file_close(pqg_file* f) { delete f; }
int pqg_file_num_columns(const pqg_file* f) { return f ? (int)f->leaves.size() : 0; }
int pqg_file_num_row_groups(const pqg_file* f) { return f ? (int)f->rgs.size() : 0; }
int64_t pqg_file_num_rows(const pqg_file* f) { return f ? f->num_rows : 0; }
int64_t pqg_file_row_group_rows(const pqg_file* f, int rg) {
  if (!f || rg < 0 || rg >= (int)f->rgs.size()) return -1;
  return f->rg_rows[(size_t)rg];
}

int pqg_file_num_schema_nodes(const pqg_file* f) { return f ? (int)f->nodes.size() : PQG_ERR_INVALID_ARG; }

int pqg_file_schema_node(const pqg_file* f, int i, pqg_schema_node* out) {
  if (!f || !out || i < 0 || i >= (int)f->nodes.size()) return PQG_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  const SNode& n = f->nodes[(size_t)i];
  // the name is the row's map key (Column.name): never hand out a truncated one
  if (n.name.size() >= sizeof(out->name)) return PQG_ERR_METADATA;
  snprintf(out->name, sizeof(out->name), "%s", n.name.c_str());
  out->repetition = n.rep;
  out->num_children = n.num_children;
  out->leaf = n.leaf;
  out->max_def = n.max_def;
  out->max_rep = n.max_rep;
  return PQG_OK;
}

int pqg_file_schema_node_kind(const pqg_file* f, int i) {
  if (!f || i < 0 || i >= (int)f->nodes.size()) return PQG_ERR_INVALID_ARG;
  return f->nodes[(size_t)i].kind;
}

int pqg_file_column(const pqg_file* f, int col, pqg_column_info* out) {
  if (!f || !out || col < 0 || col >= (int)f->leaves.size()) return PQG_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  if (f->leaves[(size_t)col].path.size() >= sizeof(out->path)) return PQG_ERR_METADATA;  // no truncated paths
  out->desc = f->leaves[(size_t)col].desc;
  strncpy(out->path, f->leaves[(size_t)col].path.c_str(), sizeof(out->path) - 1);
  return PQG_OK;
}

int pqg_file_column_logical(const pqg_file* f, int col, pqg_logical_type* out) {
  if (!f || !out || col < 0 || col >= (int)f->leaves.size()) return PQG_ERR_INVALID_ARG;
  *out = f->leaves[(size_t)col].logical;
  return PQG_OK;
}

// readChunk chunk_reader.go:314-340: FilePath must be nil, MetaData present,
// type must match the schema; start = DictionaryPageOffset if set.
int pqg_file_chunk(const pqg_file* f, int rg, int col, pqg_chunk_meta* out) {
  if (!f || !out || rg < 0 || rg >= (int)f->rgs.size() || col < 0 || col >= (int)f->leaves.size())
    return PQG_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  const std::vector<ChunkM>& cols = f->rgs[(size_t)rg];
  if ((int)cols.size() <= col) return PQG_ERR_METADATA;  // "column index %d is out of bounds"
  const ChunkM& m = cols[(size_t)col];
  if (m.has_path || !m.has_meta) return PQG_ERR_METADATA;
  if (m.type != f->leaves[(size_t)col].desc.physical_type) return PQG_ERR_METADATA;
  out->start = m.has_dict ? m.dict_off : m.data_off;
  out->total_compressed_size = m.tcs;
  out->total_uncompressed_size = m.tus;
  out->data_page_offset = m.data_off;
  out->num_values = m.num_values;
  out->has_dict_page_offset = m.has_dict ? 1 : 0;
  out->codec = m.codec;
  out->type = m.type;
  return PQG_OK;
}

// ColumnMetaData.statistics of the chunk pqg_file_chunk describes.
int pqg_file_chunk_stats(const pqg_file* f, int rg, int col, pqg_chunk_stats* out) {
  if (!f || !out || rg < 0 || rg >= (int)f->rgs.size() || col < 0 || col >= (int)f->leaves.size())
    return PQG_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  out->null_count = -1;
  const std::vector<ChunkM>& cols = f->rgs[(size_t)rg];
  if ((int)cols.size() <= col) return PQG_ERR_METADATA;
  const ChunkM& m = cols[(size_t)col];
  if (m.has_path || !m.has_meta) return PQG_ERR_METADATA;
  if (f->stats_bad) return PQG_OK;
  if (m.has_min) {
    out->min_value = (const uint8_t*)m.min_value.data();
    out->min_len = (int32_t)m.min_value.size();
  }
  if (m.has_max) {
    out->max_value = (const uint8_t*)m.max_value.data();
    out->max_len = (int32_t)m.max_value.size();
  }
  if (m.has_nulls) out->null_count = m.null_count;
  return PQG_OK;
}

// ColumnChunk.offset_index_* / column_index_*: an index with a negative offset or length is reported absent.
int pqg_file_chunk_index(const pqg_file* f, int rg, int col, pqg_index_ranges* out) {
  if (!f || !out || rg < 0 || rg >= (int)f->rgs.size() || col < 0 || col >= (int)f->leaves.size())
    return PQG_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  const std::vector<ChunkM>& cols = f->rgs[(size_t)rg];
  if ((int)cols.size() <= col) return PQG_ERR_METADATA;
  const ChunkM& m = cols[(size_t)col];
  if (m.oi_off > 0 && m.oi_len > 0) {
    out->offset_index_offset = m.oi_off;
    out->offset_index_length = m.oi_len;
  }
  if (m.ci_off > 0 && m.ci_len > 0) {
    out->column_index_offset = m.ci_off;
    out->column_index_length = m.ci_len;
  }
  return PQG_OK;
}

}  // extern "C"
