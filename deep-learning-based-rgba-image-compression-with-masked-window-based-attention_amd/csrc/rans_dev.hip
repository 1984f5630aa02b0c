// Device-side chunked rANS coder (DESIGN.md "Device-side chunked rANS coder").
//
// The symbol sequence is cut into chunks of at most K symbols; each chunk is an independent
// rANS stream (csrc/rans_chunk.h, the algorithm of csrc/rans.cpp) coded by one GPU lane.
// Encoding is two passes over the same state machine: rgbac_rans_chunk_sizes runs it without
// stores and writes each chunk's word count, the caller scans the counts, and
// rgbac_rans_chunk_encode runs it again and stores each chunk's words, backwards from the
// chunk's end offset, into the packed payload.  rgbac_rans_chunk_decode reads a chunk's words
// forwards.  The *_host entry points run the same core in a CPU loop on host pointers: the
// CPU-testable twin and the kernels' bit-level reference (not a fallback).
//
// Chunks are described by a table the host builds from the segment lengths: chunk c covers
// symbols [chunk_start[c], chunk_start[c] + chunk_len[c]) of the container's symbol sequence;
// the symbols / indexes / out pointers address symbol ``sym_base`` of that sequence and hold
// ``nsym`` entries, so a call can cover a range of segments.  A table entry that leaves
// [sym_base, sym_base + nsym) or has a length outside [1, K] is skipped with kErrChunk.
//
// Layout: one lane per chunk, 64-thread workgroups (a 640-chunk latent still spreads over 10
// CUs).  The lanes of a wave read symbols K apart; each lane consumes a 64-byte line over 16
// steps, which the vector L1 / L2 hold meanwhile, so there is no LDS stage.  The CDF tables
// (64 rows of up to a few thousand int32) stay in global memory and live in L2.  The state
// machines are data-dependent per lane (refill, escape), so lanes of a wave diverge there by
// nature; the common path (one CDF record, occasional refill) is short.
#include <hip/hip_runtime.h>


#include "common.h"
#include "rans_chunk.h"

namespace {

namespace rr = rgbac_rans;
constexpr int kThreads = 64;

struct ChunkArgs {
  const int64_t* chunk_start;
  const int64_t* chunk_len;
  int64_t nchunks;
  int64_t sym_base;
  int64_t nsym;
  int32_t K;
};

// symbols of chunk c relative to the caller's pointers, or -1 if the entry is out of range
__host__ __device__ inline int64_t chunk_span(const ChunkArgs& a, int64_t c, int64_t* len) {
  const int64_t n = a.chunk_len[c];
  const int64_t rel = a.chunk_start[c] - a.sym_base;
  *len = n;
  if (n < 1 || n > a.K || rel < 0 || rel > a.nsym - n) return -1;
  return rel;
}

__device__ inline void report(int32_t* err, int32_t code) {
  if (code) atomicCAS(err, 0, code);       // the first non-zero code wins
}

__global__ __launch_bounds__(kThreads) void rans_chunk_sizes_kernel(
    const int32_t* __restrict__ symbols, const int32_t* __restrict__ indexes, ChunkArgs a,
    rr::Tables t, int32_t* __restrict__ counts, int32_t* err) {
  const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (c >= a.nchunks) return;
  int64_t n;
  const int64_t rel = chunk_span(a, c, &n);
  int32_t e = rr::kErrNone;
  int64_t words = 0;
  if (rel < 0)
    e = rr::kErrChunk;
  else
    words = rr::chunk_encode(symbols + rel, indexes + rel, n, t, nullptr, 0, &e);
  counts[c] = (int32_t)words;
  report(err, e);
}

__global__ __launch_bounds__(kThreads) void rans_chunk_encode_kernel(
    const int32_t* __restrict__ symbols, const int32_t* __restrict__ indexes, ChunkArgs a,
    rr::Tables t, const int32_t* __restrict__ counts, const int64_t* __restrict__ ends,
    uint32_t* __restrict__ payload, int64_t payload_words, int32_t* err) {
  const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (c >= a.nchunks) return;
  int64_t n;
  const int64_t rel = chunk_span(a, c, &n);
  const int64_t end = ends[c], cnt = counts[c];
  int32_t e = rr::kErrNone;
  // the words land in [end - cnt, end): cnt is what the sizes pass counted for this chunk; the
  // core stores no more than cnt words, and a different count (inputs changed in between) is
  // an error
  if (rel < 0 || cnt < 2 || cnt > rr::chunk_bound(n) || end - cnt < 0 || end > payload_words) {
    e = rr::kErrChunk;
  } else if (rr::chunk_encode(symbols + rel, indexes + rel, n, t, payload + end, cnt, &e) != cnt) {
    e = e ? e : rr::kErrChunk;
  }
  report(err, e);
}

__global__ __launch_bounds__(kThreads) void rans_chunk_decode_kernel(
    const uint32_t* __restrict__ payload, int64_t payload_words,
    const int64_t* __restrict__ word_off, const int32_t* __restrict__ counts,
    const int32_t* __restrict__ indexes, ChunkArgs a, rr::Tables t, int32_t* __restrict__ out,
    int32_t* err) {
  const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (c >= a.nchunks) return;
  int64_t n;
  const int64_t rel = chunk_span(a, c, &n);
  if (rel < 0) {
    report(err, rr::kErrChunk);
    return;
  }
  const int64_t off = word_off[c];
  int32_t cnt = counts[c];
  int32_t e = rr::kErrNone;
  if (off < 0 || cnt < 0 || off > payload_words - cnt) {   // reads nothing: decodes to zeros
    e = rr::kErrChunk;
    cnt = 0;
  }
  const int32_t de = rr::chunk_decode(payload + (cnt ? off : 0), cnt, indexes + rel, n, t,
                                      out + rel);
  report(err, e ? e : de);
}

const char* check_dev_tables(const int32_t* cdfs, int stride, const int32_t* sizes,
                             const int32_t* offsets, int ncdf) {
  if (!cdfs || !sizes || !offsets || ncdf <= 0 || stride < 3) return "bad CDF table arguments";
  return nullptr;
}

const char* check_host_tables(const int32_t* cdfs, int stride, const int32_t* sizes,
                              const int32_t* offsets, int ncdf) {
  if (const char* bad = check_dev_tables(cdfs, stride, sizes, offsets, ncdf)) return bad;
  for (int i = 0; i < ncdf; ++i)
    if (sizes[i] < 3 || sizes[i] > stride) return "CDF length out of range";
  return nullptr;
}

inline unsigned grid_of(int64_t nchunks) { return (unsigned)((nchunks + kThreads - 1) / kThreads); }

}  // namespace

#define RANS_CHUNK_REQUIRE_COMMON()                                                         \
  RGBAC_REQUIRE(chunk_start && chunk_len, "null pointer");                                  \
  RGBAC_REQUIRE(K > 0, "chunk size K must be positive");                                    \
  RGBAC_REQUIRE(nchunks > 0 && nchunks < (1ll << 31) * kThreads, "chunk count");            \
  RGBAC_REQUIRE(nsym > 0 && sym_base >= 0, "symbol range")

extern "C" int rgbac_rans_chunk_sizes(const int32_t* symbols, const int32_t* indexes,
                                      int64_t nsym, int64_t sym_base,
                                      const int64_t* chunk_start, const int64_t* chunk_len,
                                      int64_t nchunks, int K, const int32_t* cdfs,
                                      int cdf_stride, const int32_t* cdf_sizes,
                                      const int32_t* offsets, int ncdf, int32_t* counts,
                                      int32_t* err, void* stream) {
  RGBAC_REQUIRE(symbols && indexes && counts && err, "null pointer");
  RANS_CHUNK_REQUIRE_COMMON();
  const char* bad = check_dev_tables(cdfs, cdf_stride, cdf_sizes, offsets, ncdf);
  RGBAC_REQUIRE(!bad, bad ? bad : "");
  const ChunkArgs a = {chunk_start, chunk_len, nchunks, sym_base, nsym, K};
  const rr::Tables t = {cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
  hipLaunchKernelGGL(rans_chunk_sizes_kernel, dim3(grid_of(nchunks)), dim3(kThreads), 0,
                     (hipStream_t)stream, symbols, indexes, a, t, counts, err);
  return rgbac::check_launch("rgbac_rans_chunk_sizes");
}

extern "C" int rgbac_rans_chunk_encode(const int32_t* symbols, const int32_t* indexes,
                                       int64_t nsym, int64_t sym_base,
                                       const int64_t* chunk_start, const int64_t* chunk_len,
                                       int64_t nchunks, int K, const int32_t* cdfs,
                                       int cdf_stride, const int32_t* cdf_sizes,
                                       const int32_t* offsets, int ncdf, const int32_t* counts,
                                       const int64_t* ends, uint32_t* payload,
                                       int64_t payload_words, int32_t* err, void* stream) {
  RGBAC_REQUIRE(symbols && indexes && counts && ends && payload && err, "null pointer");
  RANS_CHUNK_REQUIRE_COMMON();
  RGBAC_REQUIRE(payload_words >= 2 * nchunks, "payload smaller than the chunks' state words");
  const char* bad = check_dev_tables(cdfs, cdf_stride, cdf_sizes, offsets, ncdf);
  RGBAC_REQUIRE(!bad, bad ? bad : "");
  const ChunkArgs a = {chunk_start, chunk_len, nchunks, sym_base, nsym, K};
  const rr::Tables t = {cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
  hipLaunchKernelGGL(rans_chunk_encode_kernel, dim3(grid_of(nchunks)), dim3(kThreads), 0,
                     (hipStream_t)stream, symbols, indexes, a, t, counts, ends, payload,
                     payload_words, err);
  return rgbac::check_launch("rgbac_rans_chunk_encode");
}

extern "C" int rgbac_rans_chunk_decode(const uint32_t* payload, int64_t payload_words,
                                       const int64_t* word_off, const int32_t* counts,
                                       const int32_t* indexes, int64_t nsym, int64_t sym_base,
                                       const int64_t* chunk_start, const int64_t* chunk_len,
                                       int64_t nchunks, int K, const int32_t* cdfs,
                                       int cdf_stride, const int32_t* cdf_sizes,
                                       const int32_t* offsets, int ncdf, int32_t* out,
                                       int32_t* err, void* stream) {
  RGBAC_REQUIRE(payload && word_off && counts && indexes && out && err, "null pointer");
  RANS_CHUNK_REQUIRE_COMMON();
  RGBAC_REQUIRE(payload_words > 0, "empty payload");
  const char* bad = check_dev_tables(cdfs, cdf_stride, cdf_sizes, offsets, ncdf);
  RGBAC_REQUIRE(!bad, bad ? bad : "");
  const ChunkArgs a = {chunk_start, chunk_len, nchunks, sym_base, nsym, K};
  const rr::Tables t = {cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
  hipLaunchKernelGGL(rans_chunk_decode_kernel, dim3(grid_of(nchunks)), dim3(kThreads), 0,
                     (hipStream_t)stream, payload, payload_words, word_off, counts, indexes, a,
                     t, out, err);
  return rgbac::check_launch("rgbac_rans_chunk_decode");
}

// ------------------------------------------------------------------ host twins
extern "C" int rgbac_rans_chunk_encode_host(const int32_t* symbols, const int32_t* indexes,
                                            int64_t nsym, int64_t sym_base,
                                            const int64_t* chunk_start,
                                            const int64_t* chunk_len, int64_t nchunks, int K,
                                            const int32_t* cdfs, int cdf_stride,
                                            const int32_t* cdf_sizes, const int32_t* offsets,
                                            int ncdf, int32_t* counts, uint32_t* payload,
                                            int64_t payload_words, int64_t* total_words,
                                            int32_t* err) {
  // payload == NULL: counts and *total_words only (the sizes pass); otherwise both passes,
  // each chunk's words packed behind the previous chunk's
  RGBAC_REQUIRE(symbols && indexes && counts && total_words && err, "null pointer");
  RANS_CHUNK_REQUIRE_COMMON();
  const char* bad = check_host_tables(cdfs, cdf_stride, cdf_sizes, offsets, ncdf);
  RGBAC_REQUIRE(!bad, bad ? bad : "");
  const ChunkArgs a = {chunk_start, chunk_len, nchunks, sym_base, nsym, K};
  const rr::Tables t = {cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
  int32_t e = rr::kErrNone;
  int64_t total = 0;
  for (int64_t c = 0; c < nchunks; ++c) {
    int64_t n;
    const int64_t rel = chunk_span(a, c, &n);
    RGBAC_REQUIRE(rel >= 0, "chunk table entry outside the symbol range");
    const int64_t w = rr::chunk_encode(symbols + rel, indexes + rel, n, t, nullptr, 0, &e);
    counts[c] = (int32_t)w;
    total += w;
  }
  *total_words = total;
  *err = e;
  if (!payload || e) return 0;
  RGBAC_REQUIRE(payload_words >= total, "payload buffer smaller than the chunks' words");
  int64_t end = 0;
  for (int64_t c = 0; c < nchunks; ++c) {
    int64_t n;
    const int64_t rel = chunk_span(a, c, &n);
    end += counts[c];
    rr::chunk_encode(symbols + rel, indexes + rel, n, t, payload + end, counts[c], &e);
  }
  return 0;
}

extern "C" int rgbac_rans_chunk_decode_host(const uint32_t* payload, int64_t payload_words,
                                            const int64_t* word_off, const int32_t* counts,
                                            const int32_t* indexes, int64_t nsym,
                                            int64_t sym_base, const int64_t* chunk_start,
                                            const int64_t* chunk_len, int64_t nchunks, int K,
                                            const int32_t* cdfs, int cdf_stride,
                                            const int32_t* cdf_sizes, const int32_t* offsets,
                                            int ncdf, int32_t* out, int32_t* err) {
  RGBAC_REQUIRE(payload && word_off && counts && indexes && out && err, "null pointer");
  RANS_CHUNK_REQUIRE_COMMON();
  RGBAC_REQUIRE(payload_words > 0, "empty payload");
  const char* bad = check_host_tables(cdfs, cdf_stride, cdf_sizes, offsets, ncdf);
  RGBAC_REQUIRE(!bad, bad ? bad : "");
  const ChunkArgs a = {chunk_start, chunk_len, nchunks, sym_base, nsym, K};
  const rr::Tables t = {cdfs, cdf_stride, cdf_sizes, offsets, ncdf};
  int32_t first = rr::kErrNone;
  for (int64_t c = 0; c < nchunks; ++c) {
    int64_t n;
    const int64_t rel = chunk_span(a, c, &n);
    RGBAC_REQUIRE(rel >= 0, "chunk table entry outside the symbol range");
    const int64_t off = word_off[c];
    const int32_t cnt = counts[c];
    RGBAC_REQUIRE(off >= 0 && cnt >= 0 && off <= payload_words - cnt,
                  "chunk words outside the payload");
    const int32_t e = rr::chunk_decode(payload + off, cnt, indexes + rel, n, t, out + rel);
    if (e && !first) first = e;
  }
  *err = first;
  return 0;
}
