// Lossless alpha planes: a static-model, context-conditioned predictive rANS coder that runs on
// the device for a whole ragged batch (rgbac/alphaexact.py).
//
// A plane is cut into 16 x 16 blocks (edge blocks smaller), row-major.  A block is the unit of
// independence: prediction and context never look outside it.  A block whose bytes are all
// equal is CONSTANT (class 1, its value kept in the class word); every other block is CODED
// (class 0) and is one chunk of the chunked rANS format (csrc/rans_chunk.h: the same EncState /
// DecState, state bounds and word stream), its symbols in raster order.
//
// Model, per pixel a at (r, c) of its block, L = left, U = up, D = up-left inside the block:
//   (0, 0): pred = 0, context 4;
//   r == 0: U = D = L;   c == 0: L = D = U   (the one neighbour stands for all three);
//   pred = min(L, U) if D >= max(L, U), max(L, U) if D <= min(L, U), else L + U - D   (MED);
//   context = bin of max(L, U, D) - min(L, U, D): 0 | 1..8 | 9..64 | > 64 -> 0..3;
//   symbol = (a - pred) & 255, coded with table image * 5 + context.
//
// Kernels (one launch each for the whole batch):
//   classify   one wave per block: every lane compares its 4 pixels with the block's first,
//              a wave-wide AND (__all) decides; no scratch, no atomics.
//   histogram  grid (RGBAC_ALPHA_HIST_BLOCKS, images): one wave per coded block, 5 x 256 u32
//              LDS histograms updated with integer LDS atomics, written out as per-workgroup
//              partials.
//   normalise  one workgroup per image: sums the partials in index order and turns every
//              non-empty context into frequencies that sum to 2^16 (rule below), then into the
//              coder's table: 5 x 256 u16 exclusive sums and the last symbol with a frequency.
//   sizes / encode   one workgroup (one wave) per group of 64 consecutive blocks of one image:
//              the wave computes symbol and context of every pixel of its coded blocks
//              cooperatively into LDS, then lane j walks block j's symbols last to first through
//              the rANS state machine: without stores (word counts), then, after the caller's
//              scan, storing backwards from the chunk's end offset.
//   decode     the same split: lane j decodes block j serially into a lane-private 16 x 16
//              block in LDS (symbol by binary search of the LDS table), then the wave writes
//              the 64 blocks to the destination plane row segment by row segment.
//
// LDS layout of the per-lane blocks: byte ``pos`` (= r * 16 + c) of block j lives in word
// (pos / 4) * 64 + ((j + pos / 4) & 63).  In the serial passes the 64 lanes touch the same pos of
// 64 blocks: 64 consecutive words, one per bank.  In the cooperative passes the 64 lanes touch
// 64 consecutive pos of one block: 16 words whose banks (j + pos / 4) & 63 differ, 4 lanes to a
// word.
//
// Frequencies of a context with counts c[0..256), total T > 0:
//   f[s] = 0 where c[s] == 0, else max(1, floor(c[s] * 65536 / T));
//   top = the symbol with the largest count, the lowest such symbol on a tie;
//   one symbol only: f[top] = 65535 and f[(top + 1) & 255] = 1 (no frequency reaches 2^16, which
//   the coder's 16-bit arithmetic could not hold); otherwise f[top] += 65536 - sum f.
// Every symbol that occurs has a frequency >= 1, so there is no bypass path.
//
// The destination / source planes are addressed through rgbac_image_desc (ptr = the plane's
// first byte, h, w, row stride) and one ``pixel_stride`` per call: 1 for a plain plane, 4 with
// ptr at the alpha byte of packed RGBA -- the alpha bytes are coded where they lie.
#include <hip/hip_runtime.h>

#include "common.h"
#include "rans_chunk.h"

namespace {

namespace rr = rgbac_rans;
typedef rgbac_image_desc ImgDesc;
typedef rgbac_alpha_group Group;

constexpr int kEdge = RGBAC_ALPHA_BLOCK;            // 16
constexpr int kPix = kEdge * kEdge;                 // 256
constexpr int kCtx = RGBAC_ALPHA_CONTEXTS;          // 5
constexpr int kBins = kCtx * 256;
constexpr int kLanes = RGBAC_ALPHA_GROUP;           // 64: one wave, one lane per block
constexpr int kHistBlocks = RGBAC_ALPHA_HIST_BLOCKS;
constexpr int kTabU16 = RGBAC_ALPHA_TABLE_U16;      // 5 * 256 starts + 5 last + 3 pad
static_assert(kTabU16 == kBins + 8 && kTabU16 % 2 == 0, "table layout");
static_assert(kEdge == 16 && kLanes == 64, "the index arithmetic below assumes 16 / 64");

struct Plane {
  const uint8_t* p;
  int h, w, ps;
  long long rs;
  int bx, nblk;     // blocks per row, blocks in all
  int base;         // the plane's first entry of the per-block arrays
};

// the plane of image b, or false if its descriptor or its range of the per-block arrays does
// not hold together (nothing of it is touched then)
__device__ inline bool plane_of(const ImgDesc* descs, const int32_t* block_base, int b,
                                int pixel_stride, int total_blocks, Plane& pl) {
  const ImgDesc d = descs[b];
  if (!d.ptr || d.h <= 0 || d.w <= 0) return false;
  pl.p = reinterpret_cast<const uint8_t*>(d.ptr);
  pl.h = d.h;
  pl.w = d.w;
  pl.ps = pixel_stride;
  pl.rs = d.row_stride_bytes;
  pl.bx = (d.w + kEdge - 1) / kEdge;
  const long long n = (long long)pl.bx * ((d.h + kEdge - 1) / kEdge);
  pl.base = block_base[b];
  if (pl.base < 0 || n > total_blocks || pl.base > total_blocks - n) return false;
  pl.nblk = (int)n;
  return true;
}

struct Block {
  const uint8_t* p;   // its first pixel
  int bh, bw;
};

__device__ inline Block block_of(const Plane& pl, int k) {
  const int by = k / pl.bx, bxi = k - by * pl.bx;
  const int r0 = by * kEdge, c0 = bxi * kEdge;
  Block bl;
  bl.p = pl.p + (long long)r0 * pl.rs + (long long)c0 * pl.ps;
  bl.bh = min(kEdge, pl.h - r0);
  bl.bw = min(kEdge, pl.w - c0);
  return bl;
}

__device__ inline int px(const Plane& pl, const Block& bl, int r, int c) {
  return bl.p[(long long)r * pl.rs + (long long)c * pl.ps];
}

// prediction and context from the neighbours inside the block (the file header's rules)
__device__ inline void med_model(int r, int c, int L, int U, int D, int& pred, int& ctx) {
  if (r == 0 && c == 0) {
    pred = 0;
    ctx = 4;
    return;
  }
  if (r == 0) U = D = L;
  if (c == 0) L = D = U;
  const int lo = min(L, U), hi = max(L, U);
  pred = D >= hi ? lo : (D <= lo ? hi : L + U - D);
  const int d = max(hi, D) - min(lo, D);
  ctx = d == 0 ? 0 : (d <= 8 ? 1 : (d <= 64 ? 2 : 3));
}

// symbol and context of pixel (r, c) read from the plane
__device__ inline void pixel_symbol(const Plane& pl, const Block& bl, int r, int c, int& sym,
                                    int& ctx) {
  const int a = px(pl, bl, r, c);
  const int L = c > 0 ? px(pl, bl, r, c - 1) : 0;
  const int U = r > 0 ? px(pl, bl, r - 1, c) : 0;
  const int D = (r > 0 && c > 0) ? px(pl, bl, r - 1, c - 1) : 0;
  int pred;
  med_model(r, c, L, U, D, pred, ctx);
  sym = (a - pred) & 255;
}

// byte address of pos = r * 16 + c of lane-private block j (see the file header)
__device__ inline int swz(int j, int pos) {
  const int w = pos >> 2;
  return (((w << 6) + ((j + w) & 63)) << 2) + (pos & 3);
}

__device__ inline void report(int32_t* err, int32_t code) {
  if (code) atomicCAS(err, 0, code);       // the first non-zero code wins
}

// ------------------------------------------------------------------ classify
// grid: groups; 4 waves, wave v takes blocks block0 + 16 v .. + 16 of the group
__global__ __launch_bounds__(256) void alpha_classify_kernel(
    int batch, const ImgDesc* __restrict__ descs, int pixel_stride,
    const Group* __restrict__ groups, const int32_t* __restrict__ block_base, int total_blocks,
    int32_t* __restrict__ cls) {
  const Group g = groups[blockIdx.x];
  Plane pl;
  if (g.image < 0 || g.image >= batch || g.block0 < 0 ||
      !plane_of(descs, block_base, g.image, pixel_stride, total_blocks, pl))
    return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = 0; i < kLanes / 4; ++i) {
    const int k = g.block0 + wave * (kLanes / 4) + i;
    if (k >= pl.nblk) break;                              // wave-uniform
    const Block bl = block_of(pl, k);
    const int first = px(pl, bl, 0, 0);
    int same = 1;
#pragma unroll
    for (int q = 0; q < kPix / 64; ++q) {
      const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
      if (r < bl.bh && c < bl.bw) same &= px(pl, bl, r, c) == first ? 1 : 0;
    }
    same = __all(same);
    if (lane == 0) cls[pl.base + k] = same ? (1 | (first << 8)) : 0;
  }
}

// ------------------------------------------------------------------ histogram
__global__ __launch_bounds__(256) void alpha_histogram_kernel(
    const ImgDesc* __restrict__ descs, int pixel_stride, const int32_t* __restrict__ block_base,
    int total_blocks, const int32_t* __restrict__ cls, uint32_t* __restrict__ partials) {
  __shared__ uint32_t hist[kBins];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < kBins; i += 256) hist[i] = 0;
  __syncthreads();
  Plane pl;
  if (plane_of(descs, block_base, b, pixel_stride, total_blocks, pl)) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = blockIdx.x * 4 + wave; k < pl.nblk; k += gridDim.x * 4) {
      if (cls[pl.base + k] & 3) continue;                 // constant: not in the histograms
      const Block bl = block_of(pl, k);
#pragma unroll
      for (int q = 0; q < kPix / 64; ++q) {
        const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
        if (r < bl.bh && c < bl.bw) {
          int sym, ctx;
          pixel_symbol(pl, bl, r, c, sym, ctx);
          atomicAdd(&hist[ctx * 256 + sym], 1u);
        }
      }
    }
  }
  __syncthreads();
  uint32_t* out = partials + ((size_t)b * gridDim.x + blockIdx.x) * kBins;
  for (int i = threadIdx.x; i < kBins; i += 256) out[i] = hist[i];
}

// ------------------------------------------------------------------ normalise
template <class Op>
__device__ inline unsigned long long block_reduce(unsigned long long v, unsigned long long* sh,
                                                  Op op) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] = op(sh[threadIdx.x], sh[threadIdx.x + o]);
    __syncthreads();
  }
  return sh[0];
}

// grid: images; thread t owns symbol t of each context in turn
__global__ __launch_bounds__(256) void alpha_normalise_kernel(
    const uint32_t* __restrict__ partials, int nparts, int32_t* __restrict__ freqs,
    uint16_t* __restrict__ tables) {
  __shared__ unsigned long long sh[256];
  __shared__ uint32_t scan[2][256];
  const int b = blockIdx.x, t = threadIdx.x;
  auto add = [](unsigned long long x, unsigned long long y) { return x + y; };
  auto mx = [](unsigned long long x, unsigned long long y) { return x > y ? x : y; };
  for (int ctx = 0; ctx < kCtx; ++ctx) {
    unsigned long long c = 0;
    for (int g = 0; g < nparts; ++g) c += partials[((size_t)b * nparts + g) * kBins + ctx * 256 + t];
    const unsigned long long total = block_reduce(c, sh, add);
    uint32_t f = 0;
    int last = -1;
    if (total > 0) {                                       // block-uniform
      if (c) {
        f = (uint32_t)((c << 16) / total);
        if (f < 1) f = 1;
      }
      const unsigned long long sum = block_reduce(f, sh, add);
      const unsigned long long nz = block_reduce(c ? 1 : 0, sh, add);
      const int top = 255 - (int)(block_reduce((c << 8) | (unsigned)(255 - t), sh, mx) & 255);
      if (nz == 1) {
        if (t == top) f = 65535;
        if (t == ((top + 1) & 255)) f = 1;
      } else if (t == top) {
        f = (uint32_t)((long long)f + 65536 - (long long)sum);
      }
      last = (int)block_reduce(f ? (unsigned)t + 1 : 0, sh, mx) - 1;
    }
    freqs[((size_t)b * kCtx + ctx) * 256 + t] = (int32_t)f;
    // exclusive sums (Hillis-Steele over 256 entries); entries past ``last`` are not read
    int cur = 0;
    __syncthreads();
    scan[0][t] = f;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      scan[cur ^ 1][t] = scan[cur][t] + (t >= o ? scan[cur][t - o] : 0);
      cur ^= 1;
      __syncthreads();
    }
    uint16_t* tab = tables + (size_t)b * kTabU16;
    tab[ctx * 256 + t] = (uint16_t)(scan[cur][t] - f);
    if (t == 0) tab[kBins + ctx] = (uint16_t)(int16_t)last;
  }
  if (t < 3) tables[(size_t)b * kTabU16 + kBins + kCtx + t] = 0;
}

// one image's table in LDS: start[ctx * 256 + s], last[ctx] (int16, -1 = empty context)
__device__ inline void stage_table(const uint16_t* __restrict__ tables, int b, uint16_t* tab) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(tables + (size_t)b * kTabU16);
  uint32_t* dst = reinterpret_cast<uint32_t*>(tab);
  for (int i = threadIdx.x; i < kTabU16 / 2; i += kLanes) dst[i] = src[i];
}

// start and frequency of symbol s in context ctx; freq 0: the symbol has none
__device__ inline void table_entry(const uint16_t* tab, int ctx, int s, uint32_t& start,
                                   uint32_t& freq) {
  const int last = (int16_t)tab[kBins + ctx];
  start = tab[ctx * 256 + s];
  if (s > last)
    freq = 0;
  else if (s == last)
    freq = 65536u - start;
  else
    freq = (uint32_t)tab[ctx * 256 + s + 1] - start;
}

// ------------------------------------------------------------------ sizes / encode
template <bool kStore>
__global__ __launch_bounds__(kLanes) void alpha_code_kernel(
    int batch, const ImgDesc* __restrict__ descs, int pixel_stride,
    const Group* __restrict__ groups, const int32_t* __restrict__ block_base, int total_blocks,
    const int32_t* __restrict__ cls, const uint16_t* __restrict__ tables,
    int32_t* __restrict__ counts, const int64_t* __restrict__ ends,
    uint32_t* __restrict__ payload, int64_t payload_words, int32_t* err) {
  __shared__ uint8_t syms[kLanes * kPix];
  __shared__ uint8_t ctxs[kLanes * kPix];
  __shared__ __attribute__((aligned(4))) uint16_t tab[kTabU16];
  const Group g = groups[blockIdx.x];
  Plane pl;
  if (g.image < 0 || g.image >= batch || g.block0 < 0 ||
      !plane_of(descs, block_base, g.image, pixel_stride, total_blocks, pl)) {
    if (threadIdx.x == 0) report(err, rr::kErrChunk);
    return;
  }
  const int lane = threadIdx.x;
  const int nb = min(kLanes, pl.nblk - g.block0);           // <= 0: a group past the plane
  stage_table(tables, g.image, tab);
  for (int j = 0; j < nb; ++j) {
    if (cls[pl.base + g.block0 + j] & 3) continue;          // wave-uniform
    const Block bl = block_of(pl, g.block0 + j);
#pragma unroll
    for (int q = 0; q < kPix / 64; ++q) {
      const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
      if (r < bl.bh && c < bl.bw) {
        int sym, ctx;
        pixel_symbol(pl, bl, r, c, sym, ctx);
        const int a = swz(j, pos);
        syms[a] = (uint8_t)sym;
        ctxs[a] = (uint8_t)ctx;
      }
    }
  }
  __syncthreads();
  if (lane >= nb) return;
  const int k = pl.base + g.block0 + lane;
  if (cls[k] & 3) {
    if (!kStore) counts[k] = 0;
    return;
  }
  const Block bl = block_of(pl, g.block0 + lane);
  const int64_t n = (int64_t)bl.bh * bl.bw;
  int32_t e = rr::kErrNone;
  int64_t cap = 0;
  uint32_t* end = nullptr;
  if (kStore) {
    // the words land in [end - cnt, end): cnt is what the sizes pass counted for this block
    const int64_t en = ends[k];
    cap = counts[k];
    if (cap < 2 || cap > rr::chunk_bound(n) || en - cap < 0 || en > payload_words) {
      report(err, rr::kErrChunk);
      return;
    }
    end = payload + en;
  }
  rr::detail::EncState s = {rr::kL, end, cap, 0};
  for (int r = bl.bh - 1; r >= 0; --r) {
    for (int c = bl.bw - 1; c >= 0; --c) {
      const int a = swz(lane, r * kEdge + c);
      uint32_t start, freq;
      table_entry(tab, ctxs[a], syms[a], start, freq);
      if (freq == 0 || freq > 65535u) {                     // not this plane's table
        e = rr::kErrCorrupt;
        continue;
      }
      rr::detail::enc_put(s, start, freq);
    }
  }
  rr::detail::emit(s, (uint32_t)(s.x >> 32));
  rr::detail::emit(s, (uint32_t)s.x);
  if (kStore) {
    if (s.nwords != cap && !e) e = rr::kErrChunk;           // inputs changed between the passes
  } else {
    counts[k] = (int32_t)s.nwords;
  }
  report(err, e);
}

// ------------------------------------------------------------------ decode
__global__ __launch_bounds__(kLanes) void alpha_decode_kernel(
    int batch, const ImgDesc* __restrict__ descs, int pixel_stride,
    const Group* __restrict__ groups, const int32_t* __restrict__ block_base, int total_blocks,
    const int32_t* __restrict__ cls, const uint16_t* __restrict__ tables,
    const int64_t* __restrict__ word_off, const int32_t* __restrict__ counts,
    const uint32_t* __restrict__ payload, int64_t payload_words, int32_t* err) {
  __shared__ uint8_t pix[kLanes * kPix];
  __shared__ int32_t fill[kLanes];          // >= 0: the block is that value everywhere
  __shared__ __attribute__((aligned(4))) uint16_t tab[kTabU16];
  const Group g = groups[blockIdx.x];
  Plane pl;
  if (g.image < 0 || g.image >= batch || g.block0 < 0 ||
      !plane_of(descs, block_base, g.image, pixel_stride, total_blocks, pl)) {
    if (threadIdx.x == 0) report(err, rr::kErrChunk);
    return;
  }
  const int lane = threadIdx.x;
  const int nb = min(kLanes, pl.nblk - g.block0);
  stage_table(tables, g.image, tab);
  __syncthreads();
  if (lane < nb) {
    const int k = pl.base + g.block0 + lane;
    const int32_t cl = cls[k];
    int32_t e = rr::kErrNone;
    int32_t value = -1;
    if (cl & 3) {
      value = (cl >> 8) & 255;
    } else {
      const Block bl = block_of(pl, g.block0 + lane);
      const int64_t off = word_off[k];
      const int32_t cnt = counts[k];
      if (off < 0 || cnt < 2 || off > payload_words - cnt) {
        e = rr::kErrChunk;
      } else {
        rr::detail::DecState d = {0, payload + off, cnt, 0, rr::kErrNone};
        const uint32_t lo = rr::detail::dec_word(d), hi = rr::detail::dec_word(d);
        d.x = (uint64_t)lo | ((uint64_t)hi << 32);
        for (int r = 0; r < bl.bh && !d.err; ++r) {
          int L = 0, D = 0;
          for (int c = 0; c < bl.bw; ++c) {
            const int U = r > 0 ? pix[swz(lane, (r - 1) * kEdge + c)] : 0;
            int pred, ctx;
            med_model(r, c, L, U, D, pred, ctx);
            const int last = (int16_t)tab[kBins + ctx];
            if (last < 0) {                                 // a symbol in an empty context
              d.err = rr::kErrCorrupt;
              break;
            }
            const uint32_t cum = (uint32_t)(d.x & 0xFFFFu);
            // the last symbol whose start is <= cum: at most 8 steps
            int slo = 0, shi = last;
            const uint16_t* row = tab + ctx * 256;
            while (slo < shi) {
              const int mid = (slo + shi + 1) >> 1;
              if (row[mid] <= cum) slo = mid; else shi = mid - 1;
            }
            uint32_t start, freq;
            table_entry(tab, ctx, slo, start, freq);
            if (freq == 0 || cum - start >= freq) {         // not a table (the parser's job)
              d.err = rr::kErrCorrupt;
              break;
            }
            uint64_t x = d.x;
            x = freq * (x >> rr::kPrecision) + cum - start;
            if (x < rr::kL) x = (x << 32) | rr::detail::dec_word(d);
            d.x = x;
            const int a = (pred + slo) & 255;
            pix[swz(lane, r * kEdge + c)] = (uint8_t)a;
            L = a;
            D = U;
          }
        }
        // a sound chunk ends where the encoder began: every word read, the state back at kL
        if (!d.err && (d.x != rr::kL || d.pos != d.nwords)) d.err = rr::kErrCorrupt;
        e = d.err;
      }
      if (e) value = 0;                                      // a bad chunk decodes to zeros
    }
    fill[lane] = value;
    report(err, e);
  }
  __syncthreads();
  for (int j = 0; j < nb; ++j) {
    const Block bl = block_of(pl, g.block0 + j);
    const int32_t value = fill[j];
    uint8_t* dst = const_cast<uint8_t*>(bl.p);
#pragma unroll
    for (int q = 0; q < kPix / 64; ++q) {
      const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
      if (r < bl.bh && c < bl.bw)
        dst[(long long)r * pl.rs + (long long)c * pl.ps] =
            value >= 0 ? (uint8_t)value : pix[swz(j, pos)];
    }
  }
}

}  // namespace

#define ALPHA_REQUIRE_COMMON()                                                              \
  RGBAC_REQUIRE(batch > 0 && batch <= 65535, "batch must be in [1, 65535]");                \
  RGBAC_REQUIRE(descs && block_base, "null pointer");                                       \
  RGBAC_REQUIRE(pixel_stride == 1 || pixel_stride == 4, "pixel_stride must be 1 or 4");     \
  RGBAC_REQUIRE(total_blocks > 0, "total_blocks must be positive")
#define ALPHA_REQUIRE_GROUPS() \
  RGBAC_REQUIRE(groups && ngroups > 0, "group table")

extern "C" int rgbac_alpha_exact_classify(int batch, const rgbac_image_desc* descs,
                                          int pixel_stride, int ngroups,
                                          const rgbac_alpha_group* groups,
                                          const int32_t* block_base, int total_blocks,
                                          int32_t* cls, void* stream) {
  ALPHA_REQUIRE_COMMON();
  ALPHA_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls, "null pointer");
  hipLaunchKernelGGL(alpha_classify_kernel, dim3(ngroups), dim3(256), 0, (hipStream_t)stream,
                     batch, descs, pixel_stride, groups, block_base, total_blocks, cls);
  return rgbac::check_launch("rgbac_alpha_exact_classify");
}

extern "C" int rgbac_alpha_exact_tables(int batch, const rgbac_image_desc* descs,
                                        int pixel_stride, const int32_t* block_base,
                                        int total_blocks, const int32_t* cls, uint32_t* partials,
                                        int32_t* freqs, uint16_t* tables, void* stream) {
  ALPHA_REQUIRE_COMMON();
  RGBAC_REQUIRE(cls && partials && freqs && tables, "null pointer");
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned");
  hipLaunchKernelGGL(alpha_histogram_kernel, dim3(kHistBlocks, batch), dim3(256), 0,
                     (hipStream_t)stream, descs, pixel_stride, block_base, total_blocks, cls,
                     partials);
  const int rc = rgbac::check_launch("rgbac_alpha_exact_tables (histogram)");
  if (rc) return rc;
  hipLaunchKernelGGL(alpha_normalise_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream,
                     partials, kHistBlocks, freqs, tables);
  return rgbac::check_launch("rgbac_alpha_exact_tables (normalise)");
}

extern "C" int rgbac_alpha_exact_sizes(int batch, const rgbac_image_desc* descs,
                                       int pixel_stride, int ngroups,
                                       const rgbac_alpha_group* groups,
                                       const int32_t* block_base, int total_blocks,
                                       const int32_t* cls, const uint16_t* tables,
                                       int32_t* counts, int32_t* err, void* stream) {
  ALPHA_REQUIRE_COMMON();
  ALPHA_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls && tables && counts && err, "null pointer");
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned");
  hipLaunchKernelGGL(alpha_code_kernel<false>, dim3(ngroups), dim3(kLanes), 0,
                     (hipStream_t)stream, batch, descs, pixel_stride, groups, block_base,
                     total_blocks, cls, tables, counts, (const int64_t*)nullptr,
                     (uint32_t*)nullptr, (int64_t)0, err);
  return rgbac::check_launch("rgbac_alpha_exact_sizes");
}

extern "C" int rgbac_alpha_exact_encode(int batch, const rgbac_image_desc* descs,
                                        int pixel_stride, int ngroups,
                                        const rgbac_alpha_group* groups,
                                        const int32_t* block_base, int total_blocks,
                                        const int32_t* cls, const uint16_t* tables,
                                        const int32_t* counts, const int64_t* ends,
                                        uint32_t* payload, int64_t payload_words, int32_t* err,
                                        void* stream) {
  ALPHA_REQUIRE_COMMON();
  ALPHA_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls && tables && counts && ends && payload && err, "null pointer");
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned");
  RGBAC_REQUIRE(payload_words >= 2, "payload smaller than one chunk's state words");
  hipLaunchKernelGGL(alpha_code_kernel<true>, dim3(ngroups), dim3(kLanes), 0,
                     (hipStream_t)stream, batch, descs, pixel_stride, groups, block_base,
                     total_blocks, cls, tables, const_cast<int32_t*>(counts), ends, payload,
                     payload_words, err);
  return rgbac::check_launch("rgbac_alpha_exact_encode");
}

extern "C" int rgbac_alpha_exact_decode(int batch, const rgbac_image_desc* descs,
                                        int pixel_stride, int ngroups,
                                        const rgbac_alpha_group* groups,
                                        const int32_t* block_base, int total_blocks,
                                        const int32_t* cls, const uint16_t* tables,
                                        const int64_t* word_off, const int32_t* counts,
                                        const uint32_t* payload, int64_t payload_words,
                                        int32_t* err, void* stream) {
  ALPHA_REQUIRE_COMMON();
  ALPHA_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls && tables && word_off && counts && payload && err, "null pointer");
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned");
  RGBAC_REQUIRE(payload_words >= 0, "payload_words must not be negative");
  hipLaunchKernelGGL(alpha_decode_kernel, dim3(ngroups), dim3(kLanes), 0, (hipStream_t)stream,
                     batch, descs, pixel_stride, groups, block_base, total_blocks, cls, tables,
                     word_off, counts, payload, payload_words, err);
  return rgbac::check_launch("rgbac_alpha_exact_decode");
}
