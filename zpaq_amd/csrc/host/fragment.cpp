// The archiver's fragmenting restated (zpaq.cpp `add`: the limits 2194-2201, the scan 2385-2415, the analysis 2436-2471): files
// are cut where a hash of the bytes an order-1 table failed to predict falls below a threshold, so equal content gives equal
// fragments wherever it lies, and the fragments are deduplicated on their SHA-1.  This is the host's serial form, the yardstick
// of device/fragment_kernel.h.
//
// The scan, per fragment: o1[256] = 0, c1 = 0, h = 0, hits = 0.  Byte c: a hit when c == o1[c1]; h = (h + c + 1) * 314159265 on
// a hit, * 271828182 otherwise (mod 2^32); o1[c1] = c; c1 = c.  The fragment ends behind c when it has max_frag bytes, or when
// h < 2^(22 - fragment) (fragment <= 22) and it has min_frag bytes, or at the end of file.  The loop stops only at a fragment
// that ran into the end of file, so an empty file is one empty fragment, and a file whose last byte is a cut ends with one more,
// empty, fragment; the SHA-1 of an empty fragment is the SHA-1 of nothing.
//
// The analysis runs for fragments that did not deduplicate, against the tables of the last four such fragments of the block
// (o1prev[4 * 256], oldest first, all zero at the start of a block).  The caller advances it (zpaq.cpp:2530-2533): only for a
// fragment of at least min_frag bytes, o1prev moves down by 256 bytes (the oldest table leaves) and the fragment's o1 becomes
// the last of the four.  Which fragments deduplicate is the archiver's knowledge, so this part stays on the host.
#include <cstring>

#include "common.hpp"

namespace zpq {

FragLimits fragment_limits(int fragment, U32 blocksize) {
  if (fragment < 0) fragment = 0;
  FragLimits l;
  const U32 room = blocksize - 12u;
  l.max_frag = (fragment > 19 || (8128u << fragment) > room) ? room : 8128u << fragment;
  l.min_frag = (fragment > 25 || (64u << fragment) > l.max_frag) ? l.max_frag : 64u << fragment;
  l.thresh = fragment <= 22 ? 1u << (22 - fragment) : 0u;
  return l;
}

void fragment_scan(const U8* data, U64 n, const FragLimits& lim, bool with_sha1, std::vector<Fragment>& out) {
  U64 p = 0;
  for (;;) {
    Fragment f;
    memset(&f, 0, sizeof f);
    const U64 from = p;
    U32 c1 = 0, h = 0, hits = 0;
    U64 sz = 0;
    bool eof = false;
    for (;;) {
      if (p >= n) { eof = true; break; }
      const U32 c = data[p++];
      if (c == f.o1[c1]) { h = (h + c + 1u) * 314159265u; ++hits; }
      else h = (h + c + 1u) * 271828182u;
      f.o1[c1] = (U8)c;
      c1 = c;
      ++sz;
      if (sz >= lim.max_frag || (h < lim.thresh && sz >= lim.min_frag)) break;
    }
    f.size = (U32)sz;
    f.hits = hits;
    if (with_sha1) {
      Sha1 s;
      if (sz) s.update(data + from, (size_t)sz);
      memcpy(f.sha1, s.result(), 20);
    }
    out.push_back(f);
    if (eof) return;
  }
}

U32 fragment_analyze(const U8 o1[256], U64 sz, U32 hits, const U8 o1prev[1024], int* text1, int* exe1) {
  const int64_t s = (int64_t)sz;
  int text = 0, exe = 0;
  int64_t h1 = s;
  U8 seen[256];                                       // how often a byte occurs in o1, saturating
  memset(seen, 0, sizeof seen);
  for (int i = 0; i < 256; ++i) {
    const U8 v = o1[i];
    if (seen[v] < 255) {
      const int64_t w = 32768 / (((int64_t)seen[v] + 1) * 204);      // the weight of the k-th occurrence, a byte
      h1 -= (s * w) >> 15;
      ++seen[v];
    }
    const bool alnum = (i >= '0' && i <= '9') || (i >= 'A' && i <= 'Z') || (i >= 'a' && i <= 'z');
    if (v == ' ' && (alnum || i == '.' || i == ',')) ++text;
    if (v && (i < 9 || i == 11 || i == 12 || (i >= 14 && i <= 31) || i >= 240)) --text;
    if (i >= 192 && i < 240 && v && (v < 128 || v >= 192)) --text;
    if (v == 139) ++exe;
  }
  if (s > 0) h1 = h1 * h1 / s;                        // test 2: an uneven distribution in o1
  U32 h2 = (U32)h1;
  if (h2 > hits) hits = h2;
  h2 = (U32)((int64_t)seen[0] * s / 256);             // test 3: contexts never seen, or that predict 0
  if (h2 > hits) hits = h2;
  h2 = 0;
  for (int i = 0; i < 1024; ++i) h2 += o1prev[i] == o1[i & 255];
  h2 = (U32)((int64_t)h2 * s / 1024);                 // test 4: agreement with the tables in front
  if (h2 > hits) hits = h2;
  if ((int64_t)hits > s) hits = (U32)s;
  if (text1) *text1 = text >= 3;
  if (exe1) *exe1 = exe >= 5;
  return hits;
}

}  // namespace zpq
