// thrift_model.cpp — the PageHeader reader of K1 (parquet-go_amd/csrc/pqg_thrift.h) on the host,
// twice per header: with the serial walk's full capacity over plain memory, and the way one lane
// of the candidate scan runs it (parse_candidate in pqg_scan.hip): through a byte source with
// CandSrc's limit and `hit` flag, with the kCand* stacks and step budget of pqg_common.h, after the
// same structural pre-check.
// Build: g++ -O1 -std=c++17 -Wno-unknown-pragmas -I parquet-go_amd/csrc tools/thrift_model.cpp
// (add -fsanitize=address,undefined for a checked run).
// stdin: one header per line, "<a> <hex>": the bytes of a chunk from the header's first byte to
// the chunk's end, the header starting `a` bytes into a 16-byte granule (0..15).
// stdout, per line: "F <status> <consumed> <16 fields> B <status> <consumed> <16 fields>
// <overflow> <hit> <pre>"; fields: type usize csize num_values encoding def_enc rep_enc
// dict_num_values dict_encoding v2_num_values v2_encoding v2_def_len v2_rep_len has_dph has_dict
// has_v2 (16 numbers).  `consumed` is where the reader stopped, at most the bytes there are (the
// kernels clamp a failing page's payload offset the same way).  `pre`: the pre-check passed (the
// bounded parse is run either way).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "pqg_thrift.h"

using namespace pqg;

struct MemSrc {
  const uint8_t* p;
  int64_t n;
  int get(int64_t i) const { return i >= 0 && i < n ? p[i] : -1; }
};

// CandSrc of pqg_scan.hip over host memory: bytes [0, limit) of p; a read at or past the limit
// is EOF, and sets `hit` when the chunk has that byte.
struct BoundSrc {
  const uint8_t* p;
  int64_t limit, n;
  bool hit;
  int get(int64_t i) {
    if (i >= limit) {
      hit |= i < n;
      return -1;
    }
    return i >= 0 ? p[i] : -1;
  }
};

static void print_hdr(char tag, int status, int64_t consumed, const PageHdr& h) {
  printf("%c %d %lld %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", tag, status, (long long)consumed, h.type,
         h.usize, h.csize, h.num_values, h.encoding, h.def_enc, h.rep_enc, h.dict_num_values, h.dict_encoding,
         h.v2_num_values, h.v2_encoding, h.v2_def_len, h.v2_rep_len, h.has_dph, h.has_dict, h.has_v2);
}

int main() {
  std::vector<SkipFrame> frames(kMaxFrames);
  std::vector<int16_t> last(kMaxLast);
  // exactly the candidate parse's capacities: a write past them is the sanitizer's to see
  std::vector<SkipFrame> cframes(kCandFrames);
  std::vector<int16_t> clast(kCandLast);
  std::vector<uint8_t> buf;
  std::string line;
  char chunk[1 << 16];
  long lines = 0;
  for (;;) {
    line.clear();
    bool eol = false;
    while (fgets(chunk, sizeof chunk, stdin)) {
      line += chunk;
      if (!line.empty() && line.back() == '\n') {
        eol = true;
        break;
      }
    }
    if (line.empty() && !eol) break;
    int a = 0, used = 0;
    if (sscanf(line.c_str(), "%d %n", &a, &used) < 1 || a < 0 || a > 15) {
      fprintf(stderr, "bad line %ld\n", lines);
      return 2;
    }
    buf.clear();
    auto nib = [](char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; };
    for (size_t i = used; i + 1 < line.size() && nib(line[i]) >= 0 && nib(line[i + 1]) >= 0; i += 2)
      buf.push_back((uint8_t)(nib(line[i]) << 4 | nib(line[i + 1])));
    const int64_t n = (int64_t)buf.size();
    // an exact-size copy: a read past the bytes is the sanitizer's to see
    std::vector<uint8_t> mem(buf.begin(), buf.end());
    {
      Compact<MemSrc> c;
      c.src = MemSrc{mem.data(), n};
      c.pos = 0;
      c.frames = frames.data();
      c.last = last.data();
      c.nlast = 0;
      c.last_id = 0;
      c.bool_set = c.bool_val = false;
      PageHdr h;
      const int e = c.read_page_header(&h);
      print_hdr('F', e, c.pos < n ? c.pos : n, h);
    }
    {
      // the window: kCandWin granules from the header's granule, cut at the chunk's end and at
      // kCandParseBytes past the header
      const int64_t whi = -a + 16 * kCandWin < n ? -a + 16 * kCandWin : n;
      const int64_t lim = kCandParseBytes < whi ? kCandParseBytes : whi;
      Compact<BoundSrc> c;
      c.src = BoundSrc{mem.data(), lim, n, false};
      bool pre = true;
      {
        int64_t q = 3;
        int b = 0x80;
        for (int k = 0; k < 5 && (b & 0x80); k++) b = c.src.get(q++);
        if (b < 0 || (b & 0x80) || c.src.get(q) != 0x15) pre = false;
      }
      c.src.hit = false;  // the kernel does not parse after a failed pre-check; here the parse starts afresh
      c.pos = 0;
      c.frames = cframes.data();
      c.last = clast.data();
      c.nlast = 0;
      c.last_id = 0;
      c.bool_set = c.bool_val = false;
      c.fcap = kCandFrames;
      c.lcap = kCandLast;
      c.budget = kCandSteps;
      PageHdr h;
      const int e = c.read_page_header(&h);
      printf(" ");
      print_hdr('B', e, c.pos < n ? c.pos : n, h);
      printf(" %d %d %d\n", (int)c.overflow, (int)c.src.hit, (int)pre);
    }
    lines++;
  }
  fflush(stdout);
  return 0;
}
