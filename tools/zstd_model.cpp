// zstd_model — the Zstandard decoder of pqg_zstd.h on the host: the same
// parsers, table builds, repeat-offset rule and XXH64 that k_zstd runs, with
// a serial IO policy.  Decodes the frames of a file and prints one line:
//   status <rc> len <n> fnv <hash> <feature>=<count> ...
// With -o FILE the decoded bytes are written there.  With -m the input is a
// mutation corpus (u32 count, then per case u32 cap, u32 len, the bytes), and
// one "rc len fnv" line is printed per case.
// Build: c++ -O2 -std=c++17 -I parquet-go_amd/csrc tools/zstd_model.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pqg_zstd.h"

namespace {

using namespace pqg::zstd;

const char* const kFeatNames[F_COUNT] = {
    "blk_raw", "blk_rle", "blk_comp",
    "frame_single", "frame_window", "fcs0", "fcs1", "fcs2", "fcs4", "fcs8", "frame_one_block", "frame_multi_block",
    "frame_checksum", "frame_skip",
    "lit_raw", "lit_rle", "lit_huf1", "lit_huf4", "lit_treeless1", "lit_treeless4",
    "huf_direct", "huf_fse",
    "seq_none", "seq_short", "seq_mid", "seq_long",
    "ll_predef", "ll_rle", "ll_fse", "ll_repeat",
    "of_predef", "of_rle", "of_fse", "of_repeat",
    "ml_predef", "ml_rle", "ml_fse", "ml_repeat",
    "rep_offset", "match_overlap"};

struct HostIO {
  typedef const uint8_t* InP;
  InP in;
  int64_t n;
  std::vector<uint8_t> out, ws;
  long cnts[F_COUNT] = {0};
  long lit_bytes = 0, match_bytes = 0, max_seq = 0;
  int lane() const { return 0; }
  bool owns(int) const { return true; }
  void sync() {}
  int bcast(int v) const { return v; }
  bool any(bool b) const { return b; }
  void out_from_in(int64_t d, int64_t s, int64_t len) {
    if (len) memcpy(&out[(size_t)d], in + s, (size_t)len);
    lit_bytes += len;
  }
  void out_fill(int64_t d, uint8_t b, int64_t len) {
    if (len) memset(&out[(size_t)d], b, (size_t)len);
    lit_bytes += len;
  }
  void out_from_ws(int64_t d, int64_t s, int64_t len) {
    if (len) memcpy(&out[(size_t)d], &ws[(size_t)s], (size_t)len);
    lit_bytes += len;
  }
  void out_match(int64_t d, int64_t off, int64_t len) {
    for (int64_t i = 0; i < len; i++) out[(size_t)(d + i)] = out[(size_t)(d + i - off)];
    match_bytes += len;
  }
  void ws_put(int64_t i, uint8_t b) { ws[(size_t)i] = b; }
  void ws_done() {}
  int out_get(int64_t i) const { return out[(size_t)i]; }
  void cnt(int k) { cnts[k]++; }
  std::vector<int> seq_counts;
  void seqs(int k) { seq_counts.push_back(k); }
};

uint64_t fnv(const uint8_t* p, int64_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (int64_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}

// decode in[0..n) into at most cap bytes
int decode(const uint8_t* in, int64_t n, int64_t cap, HostIO* io, int64_t* len) {
  io->in = in;
  io->n = n;
  io->out.assign((size_t)cap + 1, 0);
  io->ws.assign(kWsBytes, 0);
  io->seq_counts.clear();
  static Tables T;
  memset(&T, 0, sizeof(T));
  Decoder<HostIO> dec(*io, &T, cap, kErr);
  const int rc = dec.run();
  *len = dec.d;
  return rc;
}

std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  uint8_t buf[65536];
  size_t k;
  while ((k = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  const char *path = nullptr, *outp = nullptr;
  bool corpus = false;
  int64_t cap = -1;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "-m")) corpus = true;
    else if (!strcmp(argv[i], "-o") && i + 1 < argc) outp = argv[++i];
    else if (!strcmp(argv[i], "-c") && i + 1 < argc) cap = atoll(argv[++i]);
    else path = argv[i];
  }
  if (!path) {
    fprintf(stderr, "usage: zstd_model [-m] [-c CAP] [-o OUT] FILE\n");
    return 2;
  }
  const std::vector<uint8_t> f = read_file(path);
  HostIO io;
  if (corpus) {
    if (f.size() < 4) return 2;
    uint32_t cases;
    memcpy(&cases, f.data(), 4);
    size_t at = 4;
    for (uint32_t c = 0; c < cases; c++) {
      uint32_t h[2];
      if (at + 8 > f.size()) return 2;
      memcpy(h, f.data() + at, 8);
      at += 8;
      if (at + h[1] > f.size()) return 2;
      // the case's bytes in a buffer of their own size: a sanitizer sees any read past them
      std::vector<uint8_t> in(f.begin() + (long)at, f.begin() + (long)(at + h[1]));
      at += h[1];
      int64_t len = 0;
      const int rc = decode(in.data(), (int64_t)in.size(), h[0], &io, &len);
      printf("%d %lld %016llx\n", rc, (long long)len, (unsigned long long)fnv(io.out.data(), rc ? 0 : len));
    }
    return 0;
  }
  if (cap < 0) {
    bool exact;
    cap = decoded_bound(f.data(), (int64_t)f.size(), &exact);
  }
  int64_t len = 0;
  const int rc = decode(f.data(), (int64_t)f.size(), cap, &io, &len);
  printf("status %d len %lld fnv %016llx", rc, (long long)len, (unsigned long long)fnv(io.out.data(), rc ? 0 : len));
  for (int k = 0; k < F_COUNT; k++) printf(" %s=%ld", kFeatNames[k], io.cnts[k]);
  printf(" lit_bytes=%ld match_bytes=%ld seqs=", io.lit_bytes, io.match_bytes);
  for (size_t k = 0; k < io.seq_counts.size() && k < 64; k++) printf(k ? ",%d" : "%d", io.seq_counts[k]);
  printf("\n");
  if (outp && rc == 0) {
    FILE* o = fopen(outp, "wb");
    if (!o) return 2;
    fwrite(io.out.data(), 1, (size_t)len, o);
    fclose(o);
  }
  return 0;
}
