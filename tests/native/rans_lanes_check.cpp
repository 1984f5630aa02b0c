// Stand-alone check of the lane-interleaved rANS coder core (csrc/rans_lanes.h) for a sanitizer
// build:
//   c++ -std=c++17 -fsanitize=address,undefined -I <pkg>/csrc rans_lanes_check.cpp && ./a.out
// tests/test_rans_lanes_host.py builds and runs it; it is host code only and never runs on a GPU.
//
// Every buffer handed to the core is a heap allocation of exactly the size the core may touch
// (n symbols, n indexes, the group's bytes, the table rows).  Cases: W in {8, 16, 32, 64} with
// n around W and W * K, a 3-entry row and a wide row, escapes of every kind, a reservation one
// byte short, every truncation of a group, and arbitrary bytes (every error path).
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "rans_lanes.h"

namespace rr = rgbac_rans;
namespace rl = rgbac_lanes;

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

template <typename T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
  std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
  for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
  return p;
}

int main() {
  // row 0: {0, 60000, 65536}; row 1: 200 symbols of frequency 327 and the escape
  const int32_t stride = 202;
  std::vector<int32_t> cdfs(2 * stride, 0), sizes = {3, 202}, offsets = {0, -100};
  cdfs[1] = 60000;
  cdfs[2] = 65536;
  for (int i = 0; i <= 200; ++i) cdfs[stride + i] = 327 * i;
  cdfs[stride + 201] = 65536;
  auto cp = exact(cdfs), sp = exact(sizes), op = exact(offsets);
  const rr::Tables t = {cp.get(), stride, sp.get(), op.get(), 2};
  Rng rng{17};
  const int K = 4;
  for (int W : {8, 16, 32, 64}) {
    for (int64_t n : {(int64_t)1, (int64_t)W - 1, (int64_t)W, (int64_t)W + 1, (int64_t)W * K}) {
      std::vector<int32_t> sym(n), idx(n);
      for (int64_t i = 0; i < n; ++i) {
        idx[i] = (int32_t)(rng.next() & 1);
        sym[i] = idx[i] ? (int32_t)(rng.next() % 200) - 100 : 0;
        if (i % 7 == 0) sym[i] = 1 << 30;
        if (i % 7 == 1) sym[i] = -(1 << 30);
        if (i % 5 == 2) sym[i] = offsets[idx[i]] - 2;
        if (i % 5 == 3) sym[i] = offsets[idx[i]] + sizes[idx[i]] + 9;
        if (i % 11 == 4) sym[i] = i % 2 ? INT32_MAX : INT32_MIN;
      }
      auto sy = exact(sym), ix = exact(idx);
      int32_t err = 0;
      const int64_t cnt = rl::group_encode(sy.get(), ix.get(), n, W, t, nullptr, 0, &err);
      CHECK(err == 0 && cnt >= 4 * W && cnt <= rl::group_bound(n, W));
      std::unique_ptr<uint8_t[]> buf(new uint8_t[cnt]);
      CHECK(rl::group_encode(sy.get(), ix.get(), n, W, t, buf.get() + cnt, cnt, &err) == cnt);
      std::unique_ptr<uint8_t[]> small(new uint8_t[cnt - 1]);   // stays inside [end - cap, end)
      CHECK(rl::group_encode(sy.get(), ix.get(), n, W, t, small.get() + cnt - 1, cnt - 1, &err) ==
            cnt);
      std::unique_ptr<int32_t[]> out(new int32_t[n]);
      CHECK(rl::group_decode(buf.get(), cnt, ix.get(), n, W, t, out.get()) == 0);
      for (int64_t i = 0; i < n; ++i) CHECK(out[i] == sym[i]);
      // every truncation is an error with a zero tail, and reads nothing past its buffer
      for (int64_t cut = 0; cut < cnt; cut += (cnt > 64 ? 7 : 1)) {
        std::vector<uint8_t> part(buf.get(), buf.get() + cut);
        auto pp = exact(part);
        const int32_t e = rl::group_decode(pp.get(), cut, ix.get(), n, W, t, out.get());
        CHECK(e != 0 && out[n - 1] == 0);
      }
      // arbitrary bytes and indexes: a code or a clean decode, never a crash or a long loop
      for (int it = 0; it < 50; ++it) {
        std::vector<uint8_t> junk(4 * W + rng.next() % 40);
        for (auto& b : junk) b = (uint8_t)rng.next();
        if (it % 2)
          for (int l = 0; l < W; ++l) junk[4 * l + 3] = (uint8_t)(junk[4 * l + 3] & 0x7F) | 1;
        std::vector<int32_t> jidx(idx);
        if (it % 5 == 0) jidx[rng.next() % n] = 2 + (int32_t)(rng.next() % 3);
        if (it % 7 == 0) jidx[rng.next() % n] = -1;
        auto jp = exact(junk);
        auto ji = exact(jidx);
        const int32_t e =
            rl::group_decode(jp.get(), (int64_t)junk.size(), ji.get(), n, W, t, out.get());
        CHECK(e >= 0 && e <= rr::kErrChunk);
      }
    }
  }
  // encoder guards: an index out of range, a row that is not a CDF (no division by zero)
  {
    std::vector<int32_t> sym = {0, 1, -1, 5}, idx = {0, 2, -3, 0};
    auto sy = exact(sym), ix = exact(idx);
    int32_t err = 0;
    rl::group_encode(sy.get(), ix.get(), 4, 8, t, nullptr, 0, &err);
    CHECK(err == rr::kErrIndex);
    std::vector<int32_t> flat = {0, 0, 0, 65536}, fs = {4}, fo = {0}, zi = {0, 0, 0};
    auto fp = exact(flat), fsp = exact(fs), fop = exact(fo), zp = exact(zi);
    const rr::Tables f = {fp.get(), 4, fsp.get(), fop.get(), 1};
    err = 0;
    rl::group_encode(sy.get(), zp.get(), 3, 8, f, nullptr, 0, &err);
    CHECK(err == rr::kErrCorrupt);
  }
  if (g_fail) {
    std::printf("rans_lanes_check: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("rans_lanes_check: ok\n");
  return 0;
}
