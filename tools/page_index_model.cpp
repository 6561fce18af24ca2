// page_index_model.cpp — the page-index parsers (pqg_page_index.h) as a stand-alone program.
//
//   page_index_model fuzz <offset|column> <file>
// reads a valid OffsetIndex / ColumnIndex, then parses every prefix of it and every copy with one byte
// flipped (each of 0xff, 0x01, 0x80 xor-ed in) at every position.  Each parse must end in a valid
// result or PQG_ERR_METADATA; every page of a parsed ColumnIndex is read back.  Prints the counts.
// Built plain and with -fsanitize=address,undefined by tests/test_page_index_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../parquet-go_amd/csrc/pqg_page_index.h"

static int run(bool offset, const std::vector<uint8_t>& b, long* ok, long* bad) {
  // an exact-size heap copy: a read past the end is the sanitizer's to find
  uint8_t* p = (uint8_t*)malloc(b.size() ? b.size() : 1);
  if (!b.empty()) memcpy(p, b.data(), b.size());
  int rc;
  if (offset) {
    std::vector<pqg_page_loc> locs(64);
    rc = pqg_parse_offset_index(p, (int64_t)b.size(), locs.data(), (int)locs.size());
    if (rc >= 0) {
      int64_t end = 0;
      for (int k = 0; k < rc && k < (int)locs.size(); k++) {
        if (locs[k].offset < end || locs[k].size <= 0) return 1;
        end = locs[k].offset + locs[k].size;
      }
    }
  } else {
    pqg_column_index* ci = nullptr;
    rc = pqg_column_index_parse(p, (int64_t)b.size(), &ci);
    if (rc == PQG_OK) {
      const int n = pqg_column_index_pages(ci);
      long sum = pqg_column_index_boundary_order(ci);
      for (int k = 0; k < n; k++) {
        pqg_chunk_stats st;
        int32_t np = 0;
        if (pqg_column_index_page(ci, k, &st, &np)) return 1;
        for (int i = 0; i < st.min_len; i++) sum += st.min_value[i];
        for (int i = 0; i < st.max_len; i++) sum += st.max_value[i];
        if (!np && (!st.min_value || !st.max_value)) return 1;
      }
      if (sum == -12345) printf("-");
      pqg_column_index_free(ci);
    } else if (ci) {
      return 1;
    }
  }
  free(p);
  if (rc >= 0) ++*ok;
  else if (rc == PQG_ERR_METADATA) ++*bad;
  else return 1;
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4 || strcmp(argv[1], "fuzz") != 0) return 2;
  const bool offset = strcmp(argv[2], "offset") == 0;
  FILE* f = fopen(argv[3], "rb");
  if (!f) return 2;
  std::vector<uint8_t> b;
  uint8_t buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
  fclose(f);
  long ok = 0, bad = 0;
  if (run(offset, b, &ok, &bad) || ok != 1) return 3;  // the input itself must parse
  for (size_t k = 0; k < b.size(); k++) {
    if (run(offset, std::vector<uint8_t>(b.begin(), b.begin() + (long)k), &ok, &bad)) return 4;
    for (uint8_t x : {0xff, 0x01, 0x80}) {
      std::vector<uint8_t> m = b;
      m[k] ^= x;
      if (run(offset, m, &ok, &bad)) return 5;
    }
  }
  printf("valid %ld metadata %ld\n", ok, bad);
  return 0;
}
