// lz4_model — the LZ4 block decoder of pqg_lz4.h on the host: the same walk
// of liblz4's LZ4_decompress_safe that k_lz4 runs, with a serial IO policy.
// Decodes one block and prints one line:
//   status <rc> len <n> fnv <hash> <cell>=<count> ... seqs=<n> lit_bytes=<n> match_bytes=<n>
// With -u U the block is a page's that must decode to U bytes (status 0,
// PQG_ERR_SIZE or PQG_ERR_LZ4 by pqg_lz4.h's page_status); without, it is a
// bare block decoded into a buffer no block can fill.  With -o FILE the decoded
// bytes are written there.  With -m the input is a corpus (u32 count, then per
// case u32 U (0xffffffff: a bare block), u32 len, the bytes), and one
// "rc len fnv" line is printed per case.
// The sequences are decoded in batches (step B's parse; the batch is executed serially here), or with
// -a one at a time (step A).
// Build: c++ -O2 -std=c++17 -I parquet-go_amd/csrc tools/lz4_model.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pqg_lz4.h"

namespace {

using namespace pqg::lz4;

const char* const kFeatNames[F_COUNT] = {
    "ll_0", "ll_short", "ll_15", "ll_ext1", "ll_ext255",
    "ml_0", "ml_short", "ml_15", "ml_ext1", "ml_ext255",
    "match_overlap", "off_1", "off_far", "off_0", "last_only", "empty", "seqs_gt64",
    "batch", "guard"};

// K: sequences per batch (64: step B, the batch executed serially here; 0: step A)
struct Seq {
  int64_t ls, ll, off, ml;
};
template <int K>
struct HostIOT {
  static constexpr int kBatch = K;
  Seq seq[K ? K : 1];
  void put(int k, int64_t ls, int64_t ll, int64_t off, int64_t ml) { seq[k] = Seq{ls, ll, off, ml}; }
  void exec(int count, int64_t d) {
    for (int k = 0; k < count; k++) {
      if (seq[k].ll) out_from_in(d, seq[k].ls, seq[k].ll);
      d += seq[k].ll;
      out_match(d, seq[k].off, seq[k].ml);
      d += seq[k].ml;
    }
  }
  const uint8_t* in;
  std::vector<uint8_t> out;
  long cnts[F_COUNT] = {0};
  int byte(int64_t i) const { return in[i]; }
  int64_t run255(int64_t i, int64_t end) const {
    int64_t p = i;
    while (p < end && in[p] == 255) p++;
    return p - i;
  }
  void out_from_in(int64_t d, int64_t s, int64_t len) { memcpy(&out[(size_t)d], in + s, (size_t)len); }
  void out_fill(int64_t d, uint8_t b, int64_t len) {
    if (len) memset(&out[(size_t)d], b, (size_t)len);
  }
  void out_match(int64_t d, int64_t off, int64_t len) {
    for (int64_t i = 0; i < len; i++) out[(size_t)(d + i)] = out[(size_t)(d + i - off)];
  }
  void cnt(int k) { cnts[k]++; }
};

uint64_t fnv(const uint8_t* p, int64_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (int64_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}

struct Result {
  int rc;
  int64_t len, seqs, lit_bytes, match_bytes;
};

// u >= 0: a page of u bytes; u < 0: a bare block
template <class HostIO>
Result decode(const uint8_t* in, int64_t n, int64_t u, HostIO* io) {
  io->in = in;
  Result r{0, 0, 0, 0, 0};
  if (u < 0) {
    const int64_t len = decoded_length(in, n);
    if (len < 0) {
      r.rc = kErr;
      return r;
    }
    // the buffer is exactly the walked length: the sanitizer sees a store past it
    io->out.assign((size_t)len, 0);
    io->out.shrink_to_fit();
    Decoder<HostIO> dec(*io, n, max_output(n), len, true);
    const int64_t got = dec.run();
    r = Result{got == len ? 0 : kErr, got, dec.nseq, dec.lit_bytes, dec.match_bytes};
    return r;
  }
  io->out.assign((size_t)u, 0);
  io->out.shrink_to_fit();
  Decoder<HostIO> dec(*io, n, u, u, true);
  const int64_t got = dec.run();
  int64_t big = got;
  if (got != u) {
    HostIO walk;
    walk.in = in;
    Decoder<HostIO> w(walk, n, max_output(n), max_output(n), false);
    big = w.run();
  }
  r = Result{page_status(got, big, u), got == u ? u : 0, dec.nseq, dec.lit_bytes, dec.match_bytes};
  return r;
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

template <class HostIO>
int run_model(const char* path, const char* outp, bool corpus, int64_t u) {
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
      in.shrink_to_fit();
      at += h[1];
      const Result r = decode(in.data(), (int64_t)in.size(), h[0] == 0xffffffffu ? -1 : (int64_t)h[0], &io);
      printf("%d %lld %016llx\n", r.rc, (long long)r.len, (unsigned long long)fnv(io.out.data(), r.rc ? 0 : r.len));
    }
    return 0;
  }
  std::vector<uint8_t> in(f);
  in.shrink_to_fit();
  const Result r = decode(in.data(), (int64_t)in.size(), u, &io);
  printf("status %d len %lld fnv %016llx", r.rc, (long long)r.len,
         (unsigned long long)fnv(io.out.data(), r.rc ? 0 : r.len));
  for (int k = 0; k < F_COUNT; k++) printf(" %s=%ld", kFeatNames[k], io.cnts[k]);
  printf(" seqs=%lld lit_bytes=%lld match_bytes=%lld\n", (long long)r.seqs, (long long)r.lit_bytes,
         (long long)r.match_bytes);
  if (outp && r.rc == 0) {
    FILE* o = fopen(outp, "wb");
    if (!o) return 2;
    fwrite(io.out.data(), 1, (size_t)r.len, o);
    fclose(o);
  }
  return 0;
}

int main(int argc, char** argv) {
  const char *path = nullptr, *outp = nullptr;
  bool corpus = false, step_a = false;
  int64_t u = -1;
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "-m")) corpus = true;
    else if (!strcmp(argv[i], "-a")) step_a = true;
    else if (!strcmp(argv[i], "-o") && i + 1 < argc) outp = argv[++i];
    else if (!strcmp(argv[i], "-u") && i + 1 < argc) u = atoll(argv[++i]);
    else path = argv[i];
  }
  if (!path) {
    fprintf(stderr, "usage: lz4_model [-a] [-m] [-u SIZE] [-o OUT] FILE\n");
    return 2;
  }
  return step_a ? run_model<HostIOT<0>>(path, outp, corpus, u) : run_model<HostIOT<64>>(path, outp, corpus, u);
}
