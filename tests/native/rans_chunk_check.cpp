// Stand-alone check of the chunked rANS coder core (csrc/rans_chunk.h) for a sanitizer build:
//   c++ -std=c++17 -fsanitize=address,undefined -I <pkg>/csrc rans_chunk_check.cpp && ./a.out
// tests/test_rans_chunk.py builds and runs it; it is host code only and never runs on a GPU.
//
// Every buffer handed to the core is a heap allocation of exactly the size the core may touch
// (n symbols, n indexes, the chunk's words, the table rows), so a read or write outside them
// is an AddressSanitizer report.  Cases as in tests/rans_chunk_cases.py: K = 64 with n in
// {1, 63, 64, 65, 64*64+1}, two unequal segments, Gaussian-shaped tables and one table of
// length 3, symbols in range / below the offset / at and above max_value / +-2^30, a segment
// of only the most probable symbol (two-word chunks), the short-chunk container, and decoding
// of arbitrary words (every error path).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "rans_chunk.h"

namespace rr = rgbac_rans;

static int g_fail = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      ++g_fail;                                                            \
    }                                                                      \
  } while (0)

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
};

// exact-size heap copy: the sanitizer sees the true extent of what the core may touch
template <typename T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
  std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
  for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
  return p;
}

struct TableSet {
  std::vector<int32_t> cdfs, sizes, offsets;
  int32_t stride = 0;
  std::unique_ptr<int32_t[]> c, s, o;
  rr::Tables view() {
    c = exact(cdfs);
    s = exact(sizes);
    o = exact(offsets);
    return {c.get(), stride, s.get(), o.get(), (int32_t)sizes.size()};
  }
};

// Gaussian-shaped 16-bit CDFs like GaussianConditional.update: row r has scale 0.11 * 1.2^r,
// support +-ceil(6 * scale), every frequency >= 1, the last interval is the escape
static TableSet gaussian_tables(int rows) {
  TableSet t;
  std::vector<std::vector<int32_t>> all;
  for (int r = 0; r < rows; ++r) {
    const double scale = 0.11 * std::pow(1.2, r);
    const int half = (int)std::ceil(6.0 * scale);
    const int nsym = 2 * half + 1;
    std::vector<double> p(nsym + 1);
    double tot = 0;
    for (int i = 0; i < nsym; ++i) {
      const double x = i - half;
      p[i] = 0.5 * (std::erf((x + 0.5) / (scale * std::sqrt(2.0))) -
                    std::erf((x - 0.5) / (scale * std::sqrt(2.0))));
      tot += p[i];
    }
    p[nsym] = 1e-4;
    tot += p[nsym];
    std::vector<int32_t> f(nsym + 1);
    int64_t sum = 0;
    int best = 0;
    for (int i = 0; i <= nsym; ++i) {
      f[i] = (int32_t)(p[i] / tot * 65536.0);
      if (f[i] < 1) f[i] = 1;
      sum += f[i];
      if (f[i] > f[best]) best = i;
    }
    // bring the total to 2^16: the peak takes a deficit, a surplus (the floor of 1 on the
    // tails) comes off the frequencies above 1, largest intervals first in sweeps
    if (sum < 65536) f[best] += (int32_t)(65536 - sum);
    while (sum > 65536) {
      bool any = false;
      for (int i = 0; i <= nsym && sum > 65536; ++i)
        if (f[i] > 1) {
          --f[i];
          --sum;
          any = true;
        }
      if (!any) {
        std::printf("gaussian_tables: row %d cannot be normalised\n", r);
        std::exit(2);
      }
    }
    std::vector<int32_t> cdf(nsym + 2);
    cdf[0] = 0;
    for (int i = 0; i <= nsym; ++i) cdf[i + 1] = cdf[i] + f[i];
    all.push_back(cdf);
    t.sizes.push_back(nsym + 2);
    t.offsets.push_back(-half);
    if (nsym + 2 > t.stride) t.stride = nsym + 2;
  }
  t.cdfs.assign((size_t)rows * t.stride, 0);
  for (int r = 0; r < rows; ++r)
    for (size_t i = 0; i < all[r].size(); ++i) t.cdfs[(size_t)r * t.stride + i] = all[r][i];
  return t;
}

static TableSet tiny_table() {
  TableSet t;
  t.stride = 3;
  t.cdfs = {0, 60000, 65536};
  t.sizes = {3};
  t.offsets = {0};
  return t;
}

struct Stream {
  std::vector<int32_t> sym, idx;
};

static Stream gauss_symbols(const TableSet& t, int64_t n, uint64_t seed) {
  Stream s;
  Rng rng{seed * 977 + 1};
  const int rows = (int)t.sizes.size();
  for (int64_t i = 0; i < n; ++i) {
    const int ci = (int)(rng.next() % rows);
    const int32_t off = t.offsets[ci], mx = t.sizes[ci] - 2;
    int64_t v = off + (int64_t)(rng.next() % (uint32_t)mx);          // in range
    const int64_t pos = i + (int64_t)seed;
    if (pos % 11 == 0) v = off - 1 - (pos % 5);
    if (pos % 13 == 0) v = off + mx;
    if (pos % 17 == 0) v = off + mx + 1 + (pos % 300);
    if (pos % 29 == 0) v = 1 << 30;
    if (pos % 31 == 0) v = -(1 << 30);
    if (pos % 37 == 0) v = INT32_MAX;
    if (pos % 41 == 0) v = INT32_MIN;
    s.sym.push_back((int32_t)v);
    s.idx.push_back(ci);
  }
  return s;
}

struct Container {
  std::vector<int64_t> start, len;     // chunk table
  std::vector<int32_t> counts;
  std::vector<std::vector<uint32_t>> words;   // per chunk, exact size
};

// encodes one chunk into an exact-size buffer (count-only pass, then the stores)
static std::vector<uint32_t> encode_chunk(const int32_t* sym, const int32_t* idx, int64_t n,
                                          const rr::Tables& t) {
  std::vector<int32_t> sv(sym, sym + n), iv(idx, idx + n);
  auto sp = exact(sv), ip = exact(iv);
  int32_t err = 0;
  const int64_t cnt = rr::chunk_encode(sp.get(), ip.get(), n, t, nullptr, 0, &err);
  CHECK(err == 0);
  CHECK(cnt >= 2 && cnt <= rr::chunk_bound(n));
  std::unique_ptr<uint32_t[]> buf(new uint32_t[cnt]);
  const int64_t cnt2 = rr::chunk_encode(sp.get(), ip.get(), n, t, buf.get() + cnt, cnt, &err);
  CHECK(cnt2 == cnt && err == 0);
  // a smaller reservation stores no more than it: the core must stay inside [end - cap, end)
  if (cnt > 2) {
    std::unique_ptr<uint32_t[]> small(new uint32_t[cnt - 1]);
    const int64_t cnt3 =
        rr::chunk_encode(sp.get(), ip.get(), n, t, small.get() + (cnt - 1), cnt - 1, &err);
    CHECK(cnt3 == cnt);
  }
  return std::vector<uint32_t>(buf.get(), buf.get() + cnt);
}

static int32_t decode_chunk(const std::vector<uint32_t>& words, const int32_t* idx, int64_t n,
                            const rr::Tables& t, std::vector<int32_t>* out) {
  auto wp = exact(words);
  std::vector<int32_t> iv(idx, idx + n);
  auto ip = exact(iv);
  std::unique_ptr<int32_t[]> op(new int32_t[n]);
  for (int64_t i = 0; i < n; ++i) op[i] = 0x5A5A5A5A;
  const int32_t e = rr::chunk_decode(wp.get(), (int32_t)words.size(), ip.get(), n, t, op.get());
  out->assign(op.get(), op.get() + n);
  return e;
}

static Container encode_container(const Stream& s, const std::vector<int64_t>& segs, int64_t K,
                                  const rr::Tables& t) {
  Container c;
  int64_t base = 0;
  for (int64_t seg : segs) {
    for (int64_t a = 0; a < seg; a += K) {
      c.start.push_back(base + a);
      c.len.push_back(seg - a < K ? seg - a : K);
    }
    base += seg;
  }
  for (size_t i = 0; i < c.start.size(); ++i) {
    c.words.push_back(encode_chunk(s.sym.data() + c.start[i], s.idx.data() + c.start[i],
                                   c.len[i], t));
    c.counts.push_back((int32_t)c.words.back().size());
  }
  return c;
}

static void round_trip(const char* name, const Stream& s, const std::vector<int64_t>& segs,
                       int64_t K, TableSet& ts, bool want_two_word_chunk = false) {
  const rr::Tables t = ts.view();
  const Container c = encode_container(s, segs, K, t);
  bool two = false;
  for (size_t i = 0; i < c.start.size(); ++i) {
    std::vector<int32_t> out;
    const int32_t e = decode_chunk(c.words[i], s.idx.data() + c.start[i], c.len[i], t, &out);
    CHECK(e == 0);
    for (int64_t j = 0; j < c.len[i]; ++j) CHECK(out[j] == s.sym[c.start[i] + j]);
    two |= c.counts[i] == 2;
  }
  if (want_two_word_chunk) CHECK(two);
  // the short-chunk container: the last chunk loses its last word
  {
    const size_t last = c.start.size() - 1;
    if (c.words[last].size() > 2) {
      std::vector<uint32_t> cut(c.words[last].begin(), c.words[last].end() - 1);
      std::vector<int32_t> out;
      const int32_t e = decode_chunk(cut, s.idx.data() + c.start[last], c.len[last], t, &out);
      CHECK(e == rr::kErrPastEnd);
      CHECK(out[c.len[last] - 1] == 0);            // zero-filled from the error on
    }
  }
  std::printf("  %-14s %zu chunks ok\n", name, c.start.size());
}

// arbitrary words, arbitrary indexes (in and out of range), every length from 0 words up:
// the decoder must stay inside its buffers and return a code, never loop or crash
static void fuzz_decode(TableSet& ts, uint64_t seed) {
  const rr::Tables t = ts.view();
  Rng rng{seed};
  for (int it = 0; it < 400; ++it) {
    const int nwords = (int)(rng.next() % 40);
    const int64_t n = 1 + rng.next() % 80;
    std::vector<uint32_t> words(nwords);
    for (auto& w : words) w = (rng.next() << 16) ^ rng.next();
    if (nwords >= 2 && it % 3 == 0) words[1] = 0x80000000u | (rng.next() & 0xFFFF);  // valid state
    std::vector<int32_t> idx(n);
    for (auto& i : idx) i = (int32_t)(rng.next() % (uint32_t)t.ncdf);
    if (it % 7 == 0) idx[rng.next() % n] = t.ncdf + (int32_t)(rng.next() % 5);
    if (it % 11 == 0) idx[rng.next() % n] = -1 - (int32_t)(rng.next() % 5);
    std::vector<int32_t> out;
    const int32_t e = decode_chunk(words, idx.data(), n, t, &out);
    CHECK(e >= 0 && e <= rr::kErrChunk);
    if (e) CHECK(out[n - 1] == 0);
    if (nwords < 2) CHECK(e == rr::kErrPastEnd);
  }
}

// the encoder's argument guards: an index out of range and a row that is not a CDF
static void encoder_guards(TableSet& ts) {
  const rr::Tables t = ts.view();
  std::vector<int32_t> sym = {0, 1, -1, 5}, idx = {0, t.ncdf, -3, 0};
  auto sp = exact(sym), ip = exact(idx);
  int32_t err = 0;
  const int64_t cnt = rr::chunk_encode(sp.get(), ip.get(), 4, t, nullptr, 0, &err);
  CHECK(err == rr::kErrIndex && cnt >= 2);
  TableSet flat;
  flat.stride = 4;
  flat.cdfs = {0, 0, 0, 65536};       // zero frequencies: must not divide
  flat.sizes = {4};
  flat.offsets = {0};
  const rr::Tables f = flat.view();
  std::vector<int32_t> s2 = {0, 1, 0}, i2 = {0, 0, 0};
  auto s2p = exact(s2), i2p = exact(i2);
  err = 0;
  rr::chunk_encode(s2p.get(), i2p.get(), 3, f, nullptr, 0, &err);
  CHECK(err == rr::kErrCorrupt);
  std::vector<uint32_t> words = {0, 0x80000000u, 1, 2, 3};
  std::vector<int32_t> out;
  const int32_t de = decode_chunk(words, i2.data(), 3, f, &out);   // any code, no crash
  CHECK(de >= 0 && de <= rr::kErrChunk);
}

int main() {
  TableSet g = gaussian_tables(44);       // scales 0.11 .. ~280, rows of up to ~3,400 entries
  TableSet tiny = tiny_table();
  const int64_t K = 64;
  const int64_t ns[] = {1, 63, 64, 65, 64 * 64 + 1};
  uint64_t seed = 29;
  for (int64_t n : ns) {
    char name[32];
    std::snprintf(name, sizeof name, "gauss_n%lld", (long long)n);
    round_trip(name, gauss_symbols(g, n, seed), {n}, K, g);
    seed = seed == 29 ? 1 : seed + 1;
  }
  round_trip("two_segments", gauss_symbols(g, 137, 5), {100, 37}, K, g);
  {
    Stream s;
    Rng rng{6};
    for (int i = 0; i < 130; ++i) {
      s.sym.push_back((int32_t)(rng.next() % 5) - 2);
      s.idx.push_back(0);
    }
    round_trip("tiny_table", s, {130}, K, tiny);
  }
  {
    // only the most probable symbol (0) of the widest row at K = 3, of the narrowest at K = 64
    const int wide = (int)g.sizes.size() - 1;
    Stream s;
    s.sym.assign(211, 0);
    s.idx.assign(211, wide);
    round_trip("peak_wide_k3", s, {211}, 3, g, true);
    Stream m;
    m.sym.assign(133, 0);
    m.idx.assign(133, 0);
    round_trip("peak_narrow", m, {133}, K, g, true);
  }
  fuzz_decode(g, 12345);
  fuzz_decode(tiny, 777);
  encoder_guards(g);
  if (g_fail) {
    std::printf("rans_chunk_check: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("rans_chunk_check: ok\n");
  return 0;
}
