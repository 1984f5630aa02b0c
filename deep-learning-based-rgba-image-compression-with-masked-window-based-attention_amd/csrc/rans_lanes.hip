// Device-side lane-interleaved rANS coder (the format and what a lane
// computes are csrc/rans_lanes.h).
//
// Work split: 64-thread workgroups, one wave; a wave codes 64 / W groups at once, one per
// W-wide sub-group of lanes, thread = lane.  Groups come from a table (first symbol, length,
// byte offset), so one launch covers any ranges of a flat symbol sequence.  Control flow is
// uniform inside a sub-group (every loop condition is a ballot masked to the sub-group); sub-
// groups of a wave diverge from each other (escapes, window refills), and nothing after the
// table staging uses a workgroup barrier.
//
// Loads: the symbols / indexes of a step are consecutive across the lanes, one coalesced load
// per array; the next step's symbol, index and that row's length and offset are fetched one
// step ahead of the state machine.
//
// Stream: no lane touches the stream in global memory byte by byte.  Every sub-group owns a
// 16 * W byte window in LDS.  The decoder refills it with four coalesced dword loads per lane
// when fewer than W bytes of it are left, and a lane reads its byte at (position + prefix rank
// of the lane in the round's ballot).  The encoder places its bytes in the window the same way,
// going down, and flushes the window with coalesced dword stores (byte stores only for the up
// to three bytes at either end of a flush that share a dword with other bytes).  LDS rather
// than registers: a round moves one byte per lane to a data-dependent place; in registers that
// is a ds_bpermute plus a dynamic byte extract per lane and a wave-wide shuffle to refill, in
// LDS a single byte access, and the LDS is otherwise idle here.
//
// CDF rows: when ncdf * stride entries fit RGBAC_LANES_LDS_ENTRIES the tables are staged once
// per workgroup as u16 (exclusive sums modulo 2^16; the closing 2^16 of a row is never read as
// a bound), else the int32 rows are read from global memory.  Both go through the same search
// and give the same bytes.
#include <hip/hip_runtime.h>

#include "../../include/rgbac.h"
#include "common.h"
#include "rans_lanes.h"

namespace {

namespace rr = rgbac_rans;
namespace rl = rgbac_lanes;
constexpr int kThreads = 64;
constexpr int kWinPerLane = 16;                 // window bytes per lane: 16 * W per sub-group

struct GroupArgs {
  const int64_t* start;      // first symbol of the group in the container's sequence
  const int64_t* len;        // symbols, 1 .. W * K
  int64_t ngroups;
  int64_t sym_base;
  int64_t nsym;
  int32_t W, K;
};

// symbols of group g relative to the caller's pointers, or -1 if the entry is out of range
__host__ __device__ inline int64_t group_span(const GroupArgs& a, int64_t g, int64_t* len) {
  const int64_t n = a.len[g];
  const int64_t rel = a.start[g] - a.sym_base;
  *len = n;
  if (n < 1 || n > (int64_t)a.W * a.K || rel < 0 || rel > a.nsym - n) return -1;
  return rel;
}

__device__ inline void report(int32_t* err, int32_t code) {
  if (code) atomicCAS(err, 0, code);            // the first non-zero code wins
}

// orders the wave's LDS accesses around a point where lanes exchange window bytes
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a lane's place in its sub-group: the ballot primitive of the format
struct Sub {
  uint64_t mask;             // the lanes of this sub-group
  uint64_t below, above;     // those below / above this lane
  __device__ Sub(int lane, int W) {
    mask = (W == 64 ? ~0ull : ((1ull << W) - 1)) << (lane & ~(W - 1));
    below = mask & ((1ull << lane) - 1);
    above = mask & ~below & ~(1ull << lane);
  }
  __device__ uint64_t ballot(bool p) const { return __ballot(p) & mask; }
};

__device__ inline void stage_tables(const rr::Tables& t, uint16_t* lds) {
  const int32_t total = t.ncdf * t.stride;
  for (int32_t i = threadIdx.x; i < total; i += kThreads) lds[i] = (uint16_t)t.cdfs[i];
  __syncthreads();
}

// the row of the symbol one step ahead: index, then its length and offset (clamped reads; the
// state machine re-validates them when the step comes)
struct Ahead {
  int32_t sym, ci, size, offset;
};
__device__ inline Ahead fetch(const int32_t* sym, const int32_t* idx, int64_t j, bool have,
                              const rr::Tables& t) {
  Ahead a = {0, 0, 3, 0};
  if (!have) return a;
  if (sym) a.sym = sym[j];
  a.ci = idx[j];
  const int32_t c = rr::detail::clamp_i32(a.ci, 0, t.ncdf - 1);
  a.size = t.sizes[c];
  a.offset = t.offsets[c];
  return a;
}

// what row_of does with the prefetched values
__device__ inline bool check_row(const rr::Tables& t, Ahead* a, int32_t* err) {
  bool ok = true;
  if (a->ci < 0 || a->ci >= t.ncdf) {
    if (!*err) *err = rr::kErrIndex;
    a->ci = rr::detail::clamp_i32(a->ci, 0, t.ncdf - 1);
    ok = false;
  }
  if (a->size < 3 || a->size > t.stride) {
    if (!*err) *err = rr::kErrCorrupt;
    a->size = rr::detail::clamp_i32(a->size, 3, t.stride);
    ok = false;
  }
  return ok;
}

// ------------------------------------------------------------------------------------ encoder
// STORE = false: the sizes pass (counts[g] = bytes of group g); true: the bytes go to
// payload[ends[g] - counts[g], ends[g]).
template <bool STORE, class Rows>
__global__ __launch_bounds__(kThreads) void lanes_encode_kernel(
    const int32_t* __restrict__ symbols, const int32_t* __restrict__ indexes, GroupArgs a,
    rr::Tables t, int32_t* __restrict__ counts, const int64_t* __restrict__ ends,
    uint8_t* __restrict__ payload, int64_t payload_bytes, int32_t* err) {
  extern __shared__ uint16_t lds_tab[];
  __shared__ uint32_t win32[kThreads * kWinPerLane / 4];
  Rows rows;
  if constexpr (sizeof(*rows.cdfs) == 2) {
    stage_tables(t, lds_tab);
    rows = {lds_tab, t.stride};
  } else {
    rows = {t.cdfs, t.stride};
  }
  const int W = a.W, lane = threadIdx.x, l = lane & (W - 1), sub_id = lane / W;
  const int64_t g = (int64_t)blockIdx.x * (kThreads / W) + sub_id;
  if (g >= a.ngroups) return;
  const Sub sub(lane, W);
  int64_t n;
  const int64_t rel = group_span(a, g, &n);
  int32_t e = rr::kErrNone;
  const int64_t end = STORE ? ends[g] : 0, cnt = STORE ? counts[g] : 0;
  if (rel < 0 || (STORE && (cnt < 4 * W || cnt > rl::group_bound(n, W) || end - cnt < 0 ||
                            end > payload_bytes))) {
    if (!STORE) counts[g] = 0;
    if (l == 0) report(err, rr::kErrChunk);
    return;
  }
  const int64_t lo_limit = end - cnt;           // no store below it
  const int32_t win = kWinPerLane * W;
  uint32_t* const w32 = win32 + sub_id * (win / 4);
  uint8_t* const w8 = (uint8_t*)w32;
  uint32_t* const pay32 = (uint32_t*)payload;
  // the window holds absolute bytes [wb, wb + win), wb a multiple of 4; [p, hi) is filled
  int64_t p = end, hi = end, wb = ((end + 3) & ~3ll) - win;
  auto flush = [&]() {
    if constexpr (STORE) {
      wave_sync();
      const int64_t lo = p < lo_limit ? lo_limit : p;
      const int64_t d0 = (lo + 3) & ~3ll, d1 = hi & ~3ll;
      for (int64_t k = d0 / 4 + l; k < d1 / 4; k += W) pay32[k] = w32[(k * 4 - wb) / 4];
      const int64_t head_end = d0 < hi ? d0 : hi;
      if (lo + l < head_end) payload[lo + l] = w8[lo + l - wb];
      const int64_t tail = d1 > head_end ? d1 : head_end;
      if (tail + l < hi) payload[tail + l] = w8[tail + l - wb];
      wave_sync();
    }
    hi = p;
    wb = ((p + 3) & ~3ll) - win;
  };
  const int64_t steps = (n + W - 1) / W;
  uint32_t x = rl::kL;
  Ahead next = fetch(symbols + rel, indexes + rel, (steps - 1) * W + l, (steps - 1) * W + l < n, t);
  for (int64_t step = steps - 1; step >= 0; --step) {
    const bool have = step * W + l < n;
    Ahead cur = next;
    if (step > 0) next = fetch(symbols + rel, indexes + rel, (step - 1) * W + l, true, t);
    rl::Rec rec = {0, 0, 0, 0};
    if (have) {
      check_row(t, &cur, &e);
      rec = rl::make_record(cur.sym, cur.ci, cur.size, cur.offset, rows, &e);
    }
    // one record of every lane that has it: two rounds of bytes, then the push
    auto record = [&](int32_t r) {
      const bool part = rec.nrec > r;
      const int32_t c = part ? rl::enc_shifts(x, r, rec.freq) : 0;
      const uint64_t m2 = sub.ballot(c == 2), m1 = sub.ballot(c >= 1);
      const int32_t n2 = __popcll(m2), n1 = __popcll(m1);
      if (STORE && m1) {
        if (p - 2 * W < wb) flush();
        if (c == 2) w8[p - 1 - __popcll(m2 & sub.above) - wb] = (uint8_t)x;
        if (c >= 1)
          w8[p - n2 - 1 - __popcll(m1 & sub.above) - wb] = (uint8_t)(c == 2 ? x >> 8 : x);
      }
      p -= n2 + n1;
      if (part) x = rl::enc_apply(x >> (8 * c), r, rec);
    };
    if (sub.ballot(rec.nrec > 1))               // escapes: rare, and divergent by nature
      for (int32_t r = rl::kMaxRecords - 1; r >= 1; --r)
        if (sub.ballot(rec.nrec > r)) record(r);
    record(0);
  }
  if (STORE) {
    if (p - 4 * W < wb) flush();
    for (int32_t b = 0; b < 4; ++b) w8[p - 4 * W + 4 * l + b - wb] = (uint8_t)(x >> (8 * b));
  }
  p -= 4 * W;
  flush();
  if (!STORE) {
    if (l == 0) counts[g] = (int32_t)(end - p);
  } else if (p != lo_limit && !e) {             // the sizes pass saw other inputs
    e = rr::kErrChunk;
  }
  report(err, e);
}

// ------------------------------------------------------------------------------------ decoder
template <class Rows>
__global__ __launch_bounds__(kThreads) void lanes_decode_kernel(
    const uint8_t* __restrict__ payload, int64_t payload_bytes,
    const int64_t* __restrict__ byte_off, const int32_t* __restrict__ counts,
    const int32_t* __restrict__ indexes, GroupArgs a, rr::Tables t, int32_t* __restrict__ out,
    int32_t* err) {
  extern __shared__ uint16_t lds_tab[];
  __shared__ uint32_t win32[kThreads * kWinPerLane / 4];
  Rows rows;
  if constexpr (sizeof(*rows.cdfs) == 2) {
    stage_tables(t, lds_tab);
    rows = {lds_tab, t.stride};
  } else {
    rows = {t.cdfs, t.stride};
  }
  const int W = a.W, lane = threadIdx.x, l = lane & (W - 1), sub_id = lane / W;
  const int64_t g = (int64_t)blockIdx.x * (kThreads / W) + sub_id;
  if (g >= a.ngroups) return;
  const Sub sub(lane, W);
  int64_t n;
  const int64_t rel = group_span(a, g, &n);
  if (rel < 0) {
    if (l == 0) report(err, rr::kErrChunk);
    return;
  }
  int32_t e = rr::kErrNone;
  int64_t goff = byte_off[g], nbytes = counts[g];
  if (goff < 0 || nbytes < 0 || goff > payload_bytes - nbytes) {   // reads nothing: zeros
    e = rr::kErrChunk;
    goff = 0;
    nbytes = 0;
  }
  const int32_t win = kWinPerLane * W;
  uint32_t* const w32 = win32 + sub_id * (win / 4);
  const uint8_t* const w8 = (const uint8_t*)w32;
  const uint32_t* const pay32 = (const uint32_t*)payload;
  const int64_t pay_dwords = payload_bytes / 4;
  int64_t pos = 0;                              // bytes of the group consumed
  int64_t wb = 0;                               // the window holds absolute bytes [wb, wb + win)
  auto refill = [&]() {
    wave_sync();
    wb = (goff + pos) & ~3ll;
    for (int32_t i = 0; i < kWinPerLane / 4; ++i) {
      const int64_t d = wb / 4 + i * W + l;
      w32[i * W + l] = d < pay_dwords ? pay32[d] : 0u;
    }
    wave_sync();
  };
  // the byte ``rank`` places after pos; past the group's end it is 0 and a code
  auto byte_at = [&](int32_t rank) -> uint32_t {
    if (pos + rank >= nbytes) {
      if (!e) e = rr::kErrPastEnd;
      return 0;
    }
    return w8[goff + pos + rank - wb];
  };
  uint32_t x = 0;
  // two rounds of reads after a record: ``need`` bytes for this lane
  auto rounds = [&](int32_t need) {
#pragma unroll
    for (int32_t round = 1; round <= 2; ++round) {
      const uint64_t m = sub.ballot(need >= round);
      if (!m) break;
      if (goff + pos + W > wb + win) refill();
      if (need >= round) x = (x << 8) | byte_at(__popcll(m & sub.below));
      pos += __popcll(m);
    }
    if (need && x < rl::kL && !e) e = rr::kErrCorrupt;
  };
  refill();
  for (int32_t b = 0; b < 4; ++b) x |= byte_at(4 * l + b) << (8 * b);
  if ((x < rl::kL || x >= rl::kTop) && !e) e = rr::kErrCorrupt;
  pos = 4 * W;
  const int64_t steps = (n + W - 1) / W;
  int64_t step = 0;
  Ahead next = fetch(nullptr, indexes + rel, l, l < n, t);
  bool failed = sub.ballot(e != 0) != 0;
  for (; step < steps && !failed; ++step) {
    const int64_t j = step * W + l;
    const bool have = j < n;
    Ahead cur = next;
    next = fetch(nullptr, indexes + rel, j + W, j + W < n, t);
    int32_t s = 0, need = 0;
    bool esc = false;
    if (have && check_row(t, &cur, &e)) {
      int32_t de = rr::kErrNone;
      x = rl::dec_cdf(x, cur.ci, cur.size, rows, &s, &de);
      if (de) {
        if (!e) e = de;
      } else {
        need = rl::dec_need(x);
        esc = s == cur.size - 2;
      }
    }
    rounds(need);
    uint32_t raw = 0;
    if (sub.ballot(esc) && !sub.ballot(e != 0)) {
      int32_t nd = 0;
      need = 0;
      if (esc) {                                // the digit count
        nd = (int32_t)(x & rr::kMaxBypassVal);
        x >>= rr::kBypassBits;
        need = x < rl::kL;
        if (nd > rr::kMaxBypass) {
          if (!e) e = rr::kErrBypass;
          nd = 0;
        }
      }
      rounds(need);
      for (int32_t d = 0; d < rr::kMaxBypass; ++d) {
        const bool part = esc && d < nd;
        if (!sub.ballot(part) || sub.ballot(e != 0)) break;
        need = 0;
        if (part) {
          raw |= (x & rr::kMaxBypassVal) << (d * rr::kBypassBits);
          x >>= rr::kBypassBits;
          need = x < rl::kL;
        }
        rounds(need);
      }
    }
    if (sub.ballot(e != 0)) {
      failed = true;
      break;
    }
    if (have) {
      const int32_t v = esc ? rl::escape_value(raw, cur.size - 2) : s;
      out[rel + j] = (int32_t)((uint32_t)v + (uint32_t)cur.offset);
    }
  }
  if (failed) {
    for (int64_t j = step * W + l; j < n; j += W) out[rel + j] = 0;
  } else if (x != rl::kL || pos != nbytes) {
    e = rr::kErrCorrupt;
  }
  report(err, e);
}

const char* check_tables(const int32_t* cdfs, int stride, const int32_t* sizes,
                         const int32_t* offsets, int ncdf, bool host) {
  if (!cdfs || !sizes || !offsets || ncdf <= 0 || stride < 3) return "bad CDF table arguments";
  if (host)
    for (int i = 0; i < ncdf; ++i)
      if (sizes[i] < 3 || sizes[i] > stride) return "CDF length out of range";
  return nullptr;
}

inline bool fits_lds(int ncdf, int stride) {
  return (int64_t)ncdf * stride <= RGBAC_LANES_LDS_ENTRIES;
}

inline unsigned grid_of(int64_t ngroups, int W) {
  const int per = kThreads / W;
  return (unsigned)((ngroups + per - 1) / per);
}

}  // namespace

#define RANS_LANES_REQUIRE_COMMON()                                                         \
  RGBAC_REQUIRE(group_start && group_len, "null pointer");                                  \
  RGBAC_REQUIRE(rl::lanes_ok(W), "lane count W must be 8, 16, 32 or 64");                   \
  RGBAC_REQUIRE(K > 0 && K <= (1 << 24), "step count K out of range");                      \
  RGBAC_REQUIRE(ngroups > 0 && ngroups < (1ll << 31), "group count");                       \
  RGBAC_REQUIRE(nsym > 0 && sym_base >= 0, "symbol range")

#define RANS_LANES_LAUNCH(kernel_lds, kernel_global, ...)                                   \
  do {                                                                                      \
    if (fits_lds(ncdf, cdf_stride))                                                         \
      hipLaunchKernelGGL(kernel_lds, dim3(grid_of(ngroups, W)), dim3(kThreads),             \
                         (size_t)ncdf * cdf_stride * sizeof(uint16_t), (hipStream_t)stream, \
                         __VA_ARGS__);                                                      \
    else                                                                                    \
      hipLaunchKernelGGL(kernel_global, dim3(grid_of(ngroups, W)), dim3(kThreads), 0,       \
                         (hipStream_t)stream, __VA_ARGS__);                                 \
  } while (0)

extern "C" int rgbac_rans_lanes_sizes(const int32_t* symbols, const int32_t* indexes,
                                      int64_t nsym, int64_t sym_base,
                                      const int64_t* group_start, const int64_t* group_len,
                                      int64_t ngroups, int W, int K, const int32_t* cdfs,
                                      int cdf_stride, const int32_t* cdf_sizes,
                                      const int32_t* offsets, int ncdf, int32_t* counts,
                                      int32_t* err, void* stream) {
  RGBAC_REQUIRE(symbols && indexes && counts && err, "null pointer");
  RANS_LANES_REQUIRE_COMMON();
  const char* bad = check_tables(cdfs, cdf_stride, cdf_sizes, offsets, ncdf, false);
  RGBAC_REQUIRE(!bad, bad ? bad : "");
  const GroupArgs a = {group_start, group_len, ngroups, sym_base, nsym, W, K};
  const rr::Tables t = {cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
  RANS_LANES_LAUNCH((lanes_encode_kernel<false, rl::RowsU16>),
                    (lanes_encode_kernel<false, rl::RowsI32>), symbols, indexes, a, t, counts,
                    (const int64_t*)nullptr, (uint8_t*)nullptr, (int64_t)0, err);
  return rgbac::check_launch("rgbac_rans_lanes_sizes");
}

extern "C" int rgbac_rans_lanes_encode(const int32_t* symbols, const int32_t* indexes,
                                       int64_t nsym, int64_t sym_base,
                                       const int64_t* group_start, const int64_t* group_len,
                                       int64_t ngroups, int W, int K, const int32_t* cdfs,
                                       int cdf_stride, const int32_t* cdf_sizes,
                                       const int32_t* offsets, int ncdf, const int32_t* counts,
                                       const int64_t* ends, uint8_t* payload,
                                       int64_t payload_bytes, int32_t* err, void* stream) {
  RGBAC_REQUIRE(symbols && indexes && counts && ends && payload && err, "null pointer");
  RANS_LANES_REQUIRE_COMMON();
  RGBAC_REQUIRE(((uintptr_t)payload & 3) == 0, "payload must be 4-byte aligned");
  RGBAC_REQUIRE(payload_bytes >= 4 * (int64_t)W * ngroups, "payload smaller than the states");
  const char* bad = check_tables(cdfs, cdf_stride, cdf_sizes, offsets, ncdf, false);
  RGBAC_REQUIRE(!bad, bad ? bad : "");
  const GroupArgs a = {group_start, group_len, ngroups, sym_base, nsym, W, K};
  const rr::Tables t = {cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
  RANS_LANES_LAUNCH((lanes_encode_kernel<true, rl::RowsU16>),
                    (lanes_encode_kernel<true, rl::RowsI32>), symbols, indexes, a, t,
                    const_cast<int32_t*>(counts), ends, payload, payload_bytes, err);
  return rgbac::check_launch("rgbac_rans_lanes_encode");
}

extern "C" int rgbac_rans_lanes_decode(const uint8_t* payload, int64_t payload_bytes,
                                       const int64_t* byte_off, const int32_t* counts,
                                       const int32_t* indexes, int64_t nsym, int64_t sym_base,
                                       const int64_t* group_start, const int64_t* group_len,
                                       int64_t ngroups, int W, int K, const int32_t* cdfs,
                                       int cdf_stride, const int32_t* cdf_sizes,
                                       const int32_t* offsets, int ncdf, int32_t* out,
                                       int32_t* err, void* stream) {
  RGBAC_REQUIRE(payload && byte_off && counts && indexes && out && err, "null pointer");
  RANS_LANES_REQUIRE_COMMON();
  RGBAC_REQUIRE(((uintptr_t)payload & 3) == 0 && payload_bytes > 0 && payload_bytes % 4 == 0,
                "payload must be 4-byte aligned whole dwords");
  const char* bad = check_tables(cdfs, cdf_stride, cdf_sizes, offsets, ncdf, false);
  RGBAC_REQUIRE(!bad, bad ? bad : "");
  const GroupArgs a = {group_start, group_len, ngroups, sym_base, nsym, W, K};
  const rr::Tables t = {cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
  RANS_LANES_LAUNCH((lanes_decode_kernel<rl::RowsU16>), (lanes_decode_kernel<rl::RowsI32>),
                    payload, payload_bytes, byte_off, counts, indexes, a, t, out, err);
  return rgbac::check_launch("rgbac_rans_lanes_decode");
}

// ------------------------------------------------------------------ host twins
extern "C" int rgbac_rans_lanes_encode_host(const int32_t* symbols, const int32_t* indexes,
                                            int64_t nsym, int64_t sym_base,
                                            const int64_t* group_start,
                                            const int64_t* group_len, int64_t ngroups, int W,
                                            int K, const int32_t* cdfs, int cdf_stride,
                                            const int32_t* cdf_sizes, const int32_t* offsets,
                                            int ncdf, int32_t* counts, uint8_t* payload,
                                            int64_t payload_bytes, int64_t* total_bytes,
                                            int32_t* err) {
  // payload == NULL: counts and *total_bytes only (the sizes pass); otherwise both passes, each
  // group's bytes packed behind the previous group's
  RGBAC_REQUIRE(symbols && indexes && counts && total_bytes && err, "null pointer");
  RANS_LANES_REQUIRE_COMMON();
  const char* bad = check_tables(cdfs, cdf_stride, cdf_sizes, offsets, ncdf, true);
  RGBAC_REQUIRE(!bad, bad ? bad : "");
  const GroupArgs a = {group_start, group_len, ngroups, sym_base, nsym, W, K};
  const rr::Tables t = {cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
  int32_t e = rr::kErrNone;
  int64_t total = 0;
  for (int64_t g = 0; g < ngroups; ++g) {
    int64_t n;
    const int64_t rel = group_span(a, g, &n);
    RGBAC_REQUIRE(rel >= 0, "group table entry outside the symbol range");
    const int64_t b = rl::group_encode(symbols + rel, indexes + rel, n, W, t, nullptr, 0, &e);
    counts[g] = (int32_t)b;
    total += b;
  }
  *total_bytes = total;
  *err = e;
  if (!payload || e) return 0;
  RGBAC_REQUIRE(payload_bytes >= total, "payload buffer smaller than the groups' bytes");
  int64_t end = 0;
  for (int64_t g = 0; g < ngroups; ++g) {
    int64_t n;
    const int64_t rel = group_span(a, g, &n);
    end += counts[g];
    rl::group_encode(symbols + rel, indexes + rel, n, W, t, payload + end, counts[g], &e);
  }
  return 0;
}

extern "C" int rgbac_rans_lanes_decode_host(const uint8_t* payload, int64_t payload_bytes,
                                            const int64_t* byte_off, const int32_t* counts,
                                            const int32_t* indexes, int64_t nsym,
                                            int64_t sym_base, const int64_t* group_start,
                                            const int64_t* group_len, int64_t ngroups, int W,
                                            int K, const int32_t* cdfs, int cdf_stride,
                                            const int32_t* cdf_sizes, const int32_t* offsets,
                                            int ncdf, int32_t* out, int32_t* err) {
  RGBAC_REQUIRE(payload && byte_off && counts && indexes && out && err, "null pointer");
  RANS_LANES_REQUIRE_COMMON();
  RGBAC_REQUIRE(payload_bytes > 0, "empty payload");
  const char* bad = check_tables(cdfs, cdf_stride, cdf_sizes, offsets, ncdf, true);
  RGBAC_REQUIRE(!bad, bad ? bad : "");
  const GroupArgs a = {group_start, group_len, ngroups, sym_base, nsym, W, K};
  const rr::Tables t = {cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
  int32_t first = rr::kErrNone;
  for (int64_t g = 0; g < ngroups; ++g) {
    int64_t n;
    const int64_t rel = group_span(a, g, &n);
    RGBAC_REQUIRE(rel >= 0, "group table entry outside the symbol range");
    const int64_t off = byte_off[g];
    const int32_t cnt = counts[g];
    RGBAC_REQUIRE(off >= 0 && cnt >= 0 && off <= payload_bytes - cnt,
                  "group bytes outside the payload");
    const int32_t e = rl::group_decode(payload + off, cnt, indexes + rel, n, W, t, out + rel);
    if (e && !first) first = e;
  }
  *err = first;
  return 0;
}
