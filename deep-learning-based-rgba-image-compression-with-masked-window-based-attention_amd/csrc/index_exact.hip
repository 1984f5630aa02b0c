// Palette index planes: a neighbour-match rANS coder that runs on the device for a whole ragged
// batch (rgbac/indexexact.py).
//
// A palette position is a label, not a magnitude, so nothing here predicts a value.  A pixel is
// coded as "which neighbour it equals", with a literal position only where it equals none, and
// the context is how the neighbours equal one another.  Blocks, classes, groups and the chunk
// format are the plane coder's (csrc/alpha_exact.hip): 16 x 16 blocks that decode alone, a block
// of equal bytes is CONSTANT (its class word comes from rgbac_alpha_exact_classify), every other
// block is one chunk of csrc/rans_chunk.h, its pixels in raster order.
//
// Model, for the pixel p at (r, c) of its block, all neighbours inside the block:
//   (0, 0): one literal, no match symbol;
//   W = (r, c-1), N = (r-1, c), NW = (r-1, c-1), NE = (r-1, c+1) if that column is in the block;
//   row 0: N takes W's value, NW and NE are absent; column 0: W takes N's value, NW is absent;
//   candidates: W, N, NE, NW in that order, without the absent ones and without a value that
//   stood earlier in the list;
//   symbol = the rank of the candidate p equals among the kept ones (0..3), else 4 followed by p
//   from the literal table;
//   context = W == N | N == NW << 1 | N == NE << 2 | W == NW << 3 (an absent neighbour equals
//   nothing) | (c >= 2 and (r, c-1) == (r, c-2)) << 4 | (r >= 2 and (r-1, c) == (r-2, c)) << 5.
// The decoder pops the match symbol, then the literal; the encoder walks last to first and puts
// the literal before the match symbol.
//
// Tables per image: 64 match tables over 0..4, one literal table over 0..255, each made by the
// plane coder's rule (a one-symbol match table puts its spare 1 on (top + 1) % 5).  The coder's
// table is their exclusive sums mod 2^16, 64 x 5 + 256 u16; the frequency of a symbol is the
// difference to the next entry (to 0 after a table's last) mod 2^16, which is right because no
// frequency reaches 2^16.  The entries behind a table's last symbol wrap to 0, so the decoder
// does not search a match table: it tests cum - start < freq for the five symbols, of which
// exactly one holds in a table that is not empty.  The literal search is the plane coder's
// 8-step one, bounded by the last literal that has a frequency (found while staging).
//
// Kernels (one launch each for the whole batch):
//   histogram  grid (RGBAC_INDEX_HIST_BLOCKS, images), 4 waves, one coded block per wave and
//              step: the wave stages the block's bytes in LDS, every lane forms context and
//              symbol of 4 pixels branch-free and adds into 576 u32 LDS counters.
//   normalise  one workgroup per image: thread t < 64 owns match table t, then all 256 threads
//              the literal table; writes the file's frequencies and the coder's table.
//   sizes / encode   one wave per group of 64 blocks.  The wave stages one block at a time (256
//              bytes of LDS) and writes one u16 code per pixel into block j's lane-private array:
//              context << 2 | rank for a match, 0x8000 | context << 8 | p for an escape.  The
//              literal rides in the code, so the walk needs no copy of the pixels (64 contexts x
//              5 symbols do not fit a byte; two byte arrays would take the same LDS and two
//              reads).  Lane j then walks block j last to first through enc_put.
//   decode     lane j decodes block j serially into its lane-private block in LDS and reads the
//              neighbours back from it; then the wave writes the 64 blocks as 16-byte rows.
//
// LDS layouts: the u16 code ``pos`` of block j lives in word (pos / 2) * 64 + ((j + pos / 2) &
// 63); the decoder's byte ``pos`` of block j in word (pos / 4) * 64 + ((j + pos / 4) & 63) as in
// alpha_exact.hip.  The serial passes touch 64 consecutive words, the cooperative ones words of
// distinct banks.
#include <hip/hip_runtime.h>

#include "common.h"
#include "rans_chunk.h"

namespace {

namespace rr = rgbac_rans;
typedef rgbac_image_desc ImgDesc;
typedef rgbac_alpha_group Group;

constexpr int kEdge = RGBAC_ALPHA_BLOCK;            // 16
constexpr int kPix = kEdge * kEdge;                 // 256
constexpr int kLanes = RGBAC_ALPHA_GROUP;           // 64: one wave, one lane per block
constexpr int kCtx = RGBAC_INDEX_CONTEXTS;          // 64
constexpr int kSym = RGBAC_INDEX_SYMBOLS;           // 5: four ranks and the escape
constexpr int kEsc = kSym - 1;
constexpr int kMatch = kCtx * kSym;                 // 320 match entries, then 256 literals
constexpr int kBins = RGBAC_INDEX_TABLE_U16;        // 576
constexpr int kHistBlocks = RGBAC_INDEX_HIST_BLOCKS;
static_assert(kBins == kMatch + 256 && kBins % 2 == 0, "table layout");
static_assert(kEdge == 16 && kLanes == 64 && kCtx == 64 && kSym == 5, "index arithmetic below");

struct Plane {
  const uint8_t* p;
  int h, w;
  long long rs;
  int bx, nblk;     // blocks per row, blocks in all
  int base;         // the plane's first entry of the per-block arrays
};

// the plane of image b, or false if its descriptor or its range of the per-block arrays does
// not hold together (nothing of it is touched then)
__device__ inline bool plane_of(const ImgDesc* descs, const int32_t* block_base, int b,
                                int total_blocks, Plane& pl) {
  const ImgDesc d = descs[b];
  if (!d.ptr || d.h <= 0 || d.w <= 0) return false;
  pl.p = reinterpret_cast<const uint8_t*>(d.ptr);
  pl.h = d.h;
  pl.w = d.w;
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
  bl.p = pl.p + (long long)r0 * pl.rs + c0;
  bl.bh = min(kEdge, pl.h - r0);
  bl.bw = min(kEdge, pl.w - c0);
  return bl;
}

// the block's bytes into 256 bytes of LDS, row stride 16; entries outside the block are not
// written and not read
__device__ inline void stage_block(const Plane& pl, const Block& bl, int lane, uint8_t* blk) {
#pragma unroll
  for (int q = 0; q < kPix / 64; ++q) {
    const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
    if (r < bl.bh && c < bl.bw) blk[pos] = bl.p[(long long)r * pl.rs + c];
  }
}

// Context, the 4-bit mask of the candidates kept and the candidates W, N, NE, NW of the pixel
// at (r, c) != (0, 0); get(r, c) reads a pixel of the block.  An absent neighbour is negative,
// NE and NW differently, so that it equals nothing.
struct Model {
  int ctx, keep, cand[4];
};

template <class Get>
__device__ inline Model model_at(Get get, int r, int c, int bw) {
  const int w = c > 0 ? get(r, c - 1) : -1;
  const int n = r > 0 ? get(r - 1, c) : -1;
  const int W = c > 0 ? w : n, N = r > 0 ? n : w;
  const int NE = (r > 0 && c + 1 < bw) ? get(r - 1, c + 1) : -2;
  const int NW = (r > 0 && c > 0) ? get(r - 1, c - 1) : -1;
  const int ww = c >= 2 ? get(r, c - 2) : -3;
  const int nn = r >= 2 ? get(r - 2, c) : -3;
  Model m;
  m.ctx = (W == N ? 1 : 0) | (N == NW ? 2 : 0) | (N == NE ? 4 : 0) | (W == NW ? 8 : 0) |
          (w == ww ? 16 : 0) | (n == nn ? 32 : 0);
  m.keep = 1 | (N != W ? 2 : 0) | ((NE >= 0 && NE != W && NE != N) ? 4 : 0) |
           ((NW >= 0 && NW != W && NW != N && NW != NE) ? 8 : 0);
  m.cand[0] = W;
  m.cand[1] = N;
  m.cand[2] = NE;
  m.cand[3] = NW;
  return m;
}

// the match symbol of p: the kept candidates differ, so at most one bit survives
__device__ inline int symbol_of(const Model& m, int p) {
  const int eq = (p == m.cand[0] ? 1 : 0) | (p == m.cand[1] ? 2 : 0) | (p == m.cand[2] ? 4 : 0) |
                 (p == m.cand[3] ? 8 : 0);
  const int hit = eq & m.keep;
  return hit ? __popc(m.keep & (hit - 1)) : kEsc;
}

// u16 index of code ``pos`` of lane-private block j (see the file header)
__device__ inline int swz16(int j, int pos) {
  const int w = pos >> 1;
  return (((w << 6) + ((j + w) & 63)) << 1) + (pos & 1);
}

// byte address of pos of the decoder's lane-private block j
__device__ inline int swz(int j, int pos) {
  const int w = pos >> 2;
  return (((w << 6) + ((j + w) & 63)) << 2) + (pos & 3);
}

__device__ inline void report(int32_t* err, int32_t code) {
  if (code) atomicCAS(err, 0, code);       // the first non-zero code wins
}

// ------------------------------------------------------------------ histogram
// Every wave of the workgroup runs the same number of steps, so the barriers are uniform.
__global__ __launch_bounds__(256) void index_histogram_kernel(
    const ImgDesc* __restrict__ descs, const int32_t* __restrict__ block_base, int total_blocks,
    const int32_t* __restrict__ cls, uint32_t* __restrict__ partials) {
  __shared__ uint32_t hist[kBins];
  __shared__ uint8_t blk[4][kPix];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < kBins; i += 256) hist[i] = 0;
  Plane pl;
  const bool ok = plane_of(descs, block_base, b, total_blocks, pl);     // block-uniform
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nblk = ok ? pl.nblk : 0;
  for (int k0 = blockIdx.x * 4; k0 < nblk; k0 += gridDim.x * 4) {
    const int k = k0 + wave;
    const bool coded = k < nblk && !(cls[pl.base + k] & 3);             // wave-uniform
    Block bl = {nullptr, 0, 0};
    if (coded) {
      bl = block_of(pl, k);
      stage_block(pl, bl, lane, blk[wave]);
    }
    __syncthreads();
    if (coded) {
      const uint8_t* me = blk[wave];
      auto get = [me](int r, int c) { return (int)me[r * kEdge + c]; };
#pragma unroll
      for (int q = 0; q < kPix / 64; ++q) {
        const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
        if (r >= bl.bh || c >= bl.bw) continue;
        const int p = me[pos];
        int sym = kEsc;
        if (pos) {
          const Model m = model_at(get, r, c, bl.bw);
          sym = symbol_of(m, p);
          atomicAdd(&hist[m.ctx * kSym + sym], 1u);
        }
        if (sym == kEsc) atomicAdd(&hist[kMatch + p], 1u);
      }
    }
    __syncthreads();
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

// grid: images.  The rule is alpha_exact.hip's; a match table's alphabet has 5 symbols.
__global__ __launch_bounds__(256) void index_normalise_kernel(
    const uint32_t* __restrict__ partials, int nparts, int32_t* __restrict__ freqs,
    uint16_t* __restrict__ tables) {
  __shared__ unsigned long long sh[256];
  __shared__ uint32_t scan[2][256];
  const int b = blockIdx.x, t = threadIdx.x;
  const uint32_t* part = partials + (size_t)b * nparts * kBins;
  int32_t* fout = freqs + (size_t)b * kBins;
  uint16_t* tab = tables + (size_t)b * kBins;
  if (t < kCtx) {                                          // match table t, whole, in registers
    unsigned long long c[kSym], total = 0;
#pragma unroll
    for (int s = 0; s < kSym; ++s) c[s] = 0;
    for (int g = 0; g < nparts; ++g) {
#pragma unroll
      for (int s = 0; s < kSym; ++s) c[s] += part[(size_t)g * kBins + t * kSym + s];
    }
    uint32_t f[kSym];
    long long sum = 0;
    int nz = 0, top = 0;
    unsigned long long best = 0;
#pragma unroll
    for (int s = 0; s < kSym; ++s) total += c[s];
#pragma unroll
    for (int s = 0; s < kSym; ++s) {
      f[s] = 0;
      if (c[s]) {
        f[s] = (uint32_t)((c[s] << 16) / total);
        if (f[s] < 1) f[s] = 1;
        ++nz;
      }
      if (c[s] > best) {                                   // the lowest symbol of equal maxima
        best = c[s];
        top = s;
      }
      sum += f[s];
    }
    const int spare = top == kSym - 1 ? 0 : top + 1;
    uint32_t acc = 0;
#pragma unroll
    for (int s = 0; s < kSym; ++s) {
      if (nz == 1) {
        if (s == top) f[s] = 65535;
        if (s == spare) f[s] = 1;
      } else if (nz > 1 && s == top) {
        f[s] = (uint32_t)((long long)f[s] + 65536 - sum);
      }
      fout[t * kSym + s] = (int32_t)f[s];
      tab[t * kSym + s] = (uint16_t)acc;
      acc += f[s];
    }
  }
  // the literal table: thread t owns symbol t
  auto add = [](unsigned long long x, unsigned long long y) { return x + y; };
  auto mx = [](unsigned long long x, unsigned long long y) { return x > y ? x : y; };
  unsigned long long c = 0;
  for (int g = 0; g < nparts; ++g) c += part[(size_t)g * kBins + kMatch + t];
  const unsigned long long total = block_reduce(c, sh, add);
  uint32_t f = 0;
  if (total > 0) {                                         // block-uniform
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
  }
  fout[kMatch + t] = (int32_t)f;
  int cur = 0;                                             // exclusive sums, Hillis-Steele
  __syncthreads();
  scan[0][t] = f;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    scan[cur ^ 1][t] = scan[cur][t] + (t >= o ? scan[cur][t - o] : 0);
    cur ^= 1;
    __syncthreads();
  }
  tab[kMatch + t] = (uint16_t)(scan[cur][t] - f);
}

// one image's table in LDS
__device__ inline void stage_table(const uint16_t* __restrict__ tables, int b, uint16_t* tab) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(tables + (size_t)b * kBins);
  uint32_t* dst = reinterpret_cast<uint32_t*>(tab);
  for (int i = threadIdx.x; i < kBins / 2; i += kLanes) dst[i] = src[i];
}

// start and frequency of entry s of a table of n entries at row; freq 0: the symbol has none
__device__ inline void table_entry(const uint16_t* row, int n, int s, uint32_t& start,
                                   uint32_t& freq) {
  start = row[s];
  freq = ((s + 1 < n ? (uint32_t)row[s + 1] : 0u) - start) & 0xFFFFu;
}

// ------------------------------------------------------------------ sizes / encode
template <bool kStore>
__global__ __launch_bounds__(kLanes) void index_code_kernel(
    int batch, const ImgDesc* __restrict__ descs, const Group* __restrict__ groups,
    const int32_t* __restrict__ block_base, int total_blocks, const int32_t* __restrict__ cls,
    const uint16_t* __restrict__ tables, int32_t* __restrict__ counts,
    const int64_t* __restrict__ ends, uint32_t* __restrict__ payload, int64_t payload_words,
    int32_t* err) {
  __shared__ uint16_t codes[kLanes * kPix];
  __shared__ uint8_t blk[kPix];
  __shared__ __attribute__((aligned(4))) uint16_t tab[kBins];
  const Group g = groups[blockIdx.x];
  Plane pl;
  if (g.image < 0 || g.image >= batch || g.block0 < 0 ||
      !plane_of(descs, block_base, g.image, total_blocks, pl)) {
    if (threadIdx.x == 0) report(err, rr::kErrChunk);
    return;
  }
  const int lane = threadIdx.x;
  const int nb = min(kLanes, pl.nblk - g.block0);           // <= 0: a group past the plane
  stage_table(tables, g.image, tab);
  const uint8_t* staged = blk;
  auto get = [staged](int r, int c) { return (int)staged[r * kEdge + c]; };
  for (int j = 0; j < nb; ++j) {
    if (cls[pl.base + g.block0 + j] & 3) continue;          // wave-uniform
    const Block bl = block_of(pl, g.block0 + j);
    stage_block(pl, bl, lane, blk);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kPix / 64; ++q) {
      const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
      if (r >= bl.bh || c >= bl.bw) continue;
      const int p = blk[pos];
      int code = 0x8000 | p;                                // (0, 0): the literal alone
      if (pos) {
        const Model m = model_at(get, r, c, bl.bw);
        const int sym = symbol_of(m, p);
        code = sym == kEsc ? (0x8000 | (m.ctx << 8) | p) : ((m.ctx << 2) | sym);
      }
      codes[swz16(j, pos)] = (uint16_t)code;
    }
    __syncthreads();
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
    if (cap < 2 || cap > n + 3 || en - cap < 0 || en > payload_words) {
      report(err, rr::kErrChunk);
      return;
    }
    end = payload + en;
  }
  rr::detail::EncState s = {rr::kL, end, cap, 0};
  for (int r = bl.bh - 1; r >= 0; --r) {
    for (int c = bl.bw - 1; c >= 0; --c) {
      const int pos = r * kEdge + c;
      const int code = codes[swz16(lane, pos)];
      uint32_t start, freq;
      if (code & 0x8000) {                                  // the literal goes in first
        table_entry(tab + kMatch, 256, code & 255, start, freq);
        if (freq == 0) {                                    // not this plane's table
          e = rr::kErrCorrupt;
          continue;
        }
        rr::detail::enc_put(s, start, freq);
        if (pos == 0) continue;
        table_entry(tab + ((code >> 8) & 63) * kSym, kSym, kEsc, start, freq);
      } else {
        table_entry(tab + (code >> 2) * kSym, kSym, code & 3, start, freq);
      }
      if (freq == 0) {
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
// one symbol off the state: the caller found (start, freq) with start <= cum < start + freq
__device__ inline void dec_advance(rr::detail::DecState& d, uint32_t cum, uint32_t start,
                                   uint32_t freq) {
  uint64_t x = freq * (d.x >> rr::kPrecision) + cum - start;
  if (x < rr::kL) x = (x << 32) | rr::detail::dec_word(d);
  d.x = x;
}

// a literal: the last symbol whose start is <= cum, at most 8 steps; -1 and d.err if none
__device__ inline int dec_literal(rr::detail::DecState& d, const uint16_t* lit, int last) {
  if (last < 0) {                                           // a literal without a table
    d.err = rr::kErrCorrupt;
    return -1;
  }
  const uint32_t cum = (uint32_t)(d.x & 0xFFFFu);
  int lo = 0, hi = last;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (lit[mid] <= cum) lo = mid; else hi = mid - 1;
  }
  uint32_t start, freq;
  table_entry(lit, 256, lo, start, freq);
  if (freq == 0 || cum - start >= freq) {                   // not a table (the parser's job)
    d.err = rr::kErrCorrupt;
    return -1;
  }
  dec_advance(d, cum, start, freq);
  return lo;
}

__global__ __launch_bounds__(kLanes) void index_decode_kernel(
    int batch, const ImgDesc* __restrict__ descs, const Group* __restrict__ groups,
    const int32_t* __restrict__ block_base, int total_blocks, const int32_t* __restrict__ cls,
    const uint16_t* __restrict__ tables, const int64_t* __restrict__ word_off,
    const int32_t* __restrict__ counts, const uint32_t* __restrict__ payload,
    int64_t payload_words, int32_t* err) {
  __shared__ __attribute__((aligned(16))) uint8_t pix[kLanes * kPix];
  __shared__ int32_t fill[kLanes];          // >= 0: the block is that value everywhere
  __shared__ int32_t lit_last;              // the last literal with a frequency, -1: none
  __shared__ __attribute__((aligned(4))) uint16_t tab[kBins];
  const Group g = groups[blockIdx.x];
  Plane pl;
  if (g.image < 0 || g.image >= batch || g.block0 < 0 ||
      !plane_of(descs, block_base, g.image, total_blocks, pl)) {
    if (threadIdx.x == 0) report(err, rr::kErrChunk);
    return;
  }
  const int lane = threadIdx.x;
  const int nb = min(kLanes, pl.nblk - g.block0);
  stage_table(tables, g.image, tab);
  if (lane == 0) lit_last = -1;
  __syncthreads();
  {
    int mine = -1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t start, freq;
      table_entry(tab + kMatch, 256, lane * 4 + q, start, freq);
      if (freq) mine = lane * 4 + q;
    }
    if (mine >= 0) atomicMax(&lit_last, mine);
  }
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
        const int last = lit_last;
        const uint16_t* lit = tab + kMatch;
        uint8_t* me = pix;
        auto get = [me, lane](int r, int c) { return (int)me[swz(lane, r * kEdge + c)]; };
        rr::detail::DecState d = {0, payload + off, cnt, 0, rr::kErrNone};
        const uint32_t lo = rr::detail::dec_word(d), hi = rr::detail::dec_word(d);
        d.x = (uint64_t)lo | ((uint64_t)hi << 32);
        for (int r = 0; r < bl.bh && !d.err; ++r) {
          for (int c = 0; c < bl.bw && !d.err; ++c) {
            const int pos = r * kEdge + c;
            int a = -1;
            if (pos == 0) {
              a = dec_literal(d, lit, last);
            } else {
              const Model m = model_at(get, r, c, bl.bw);
              const uint16_t* row = tab + m.ctx * kSym;
              const uint32_t cum = (uint32_t)(d.x & 0xFFFFu);
              int sym = -1;
              uint32_t start = 0, freq = 0;
#pragma unroll
              for (int s = 0; s < kSym; ++s) {             // exactly one holds, none if empty
                uint32_t st, fr;
                table_entry(row, kSym, s, st, fr);
                if (((cum - st) & 0xFFFFu) < fr) {
                  sym = s;
                  start = st;
                  freq = fr;
                }
              }
              if (sym < 0) {                                // a symbol in an empty context
                d.err = rr::kErrCorrupt;
                break;
              }
              dec_advance(d, cum, start, freq);
              if (sym == kEsc) {
                a = dec_literal(d, lit, last);
              } else {                                      // the kept candidate of that rank
                int rank = sym;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  if ((m.keep >> i) & 1) {
                    if (rank == 0) a = m.cand[i];
                    --rank;
                  }
                }
                if (a < 0 && !d.err) d.err = rr::kErrCorrupt;   // a rank past the candidates
              }
            }
            if (a < 0) break;
            me[swz(lane, pos)] = (uint8_t)a;
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
  // 4 blocks a step: lane -> block 4 i + lane / 16, row lane % 16, 16 bytes = 4 LDS words
  const uint32_t* words = reinterpret_cast<const uint32_t*>(pix);
  for (int j0 = 0; j0 < nb; j0 += 4) {
    const int j = j0 + (lane >> 4), r = lane & 15;
    if (j >= nb) continue;
    const Block bl = block_of(pl, g.block0 + j);
    if (r >= bl.bh) continue;
    const int32_t value = fill[j];
    uint32_t v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int w = r * 4 + q;
      v[q] = value >= 0 ? (uint32_t)value * 0x01010101u : words[(w << 6) + ((j + w) & 63)];
    }
    uint8_t* dst = const_cast<uint8_t*>(bl.p) + (long long)r * pl.rs;
    if (bl.bw == kEdge && ((uintptr_t)dst & 15) == 0) {
      *reinterpret_cast<uint4*>(dst) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int c = 0; c < kEdge; ++c)
        if (c < bl.bw) dst[c] = (uint8_t)(v[c >> 2] >> (8 * (c & 3)));
    }
  }
}

}  // namespace

#define INDEX_REQUIRE_COMMON()                                                              \
  RGBAC_REQUIRE(batch > 0 && batch <= 65535, "batch must be in [1, 65535]");                \
  RGBAC_REQUIRE(descs && block_base, "null pointer");                                       \
  RGBAC_REQUIRE(total_blocks > 0, "total_blocks must be positive")
#define INDEX_REQUIRE_GROUPS() \
  RGBAC_REQUIRE(groups && ngroups > 0, "group table")
#define INDEX_REQUIRE_TABLES() \
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned")

extern "C" int rgbac_index_exact_tables(int batch, const rgbac_image_desc* descs,
                                        const int32_t* block_base, int total_blocks,
                                        const int32_t* cls, uint32_t* partials, int32_t* freqs,
                                        uint16_t* tables, void* stream) {
  INDEX_REQUIRE_COMMON();
  RGBAC_REQUIRE(cls && partials && freqs && tables, "null pointer");
  INDEX_REQUIRE_TABLES();
  hipLaunchKernelGGL(index_histogram_kernel, dim3(kHistBlocks, batch), dim3(256), 0,
                     (hipStream_t)stream, descs, block_base, total_blocks, cls, partials);
  const int rc = rgbac::check_launch("rgbac_index_exact_tables (histogram)");
  if (rc) return rc;
  hipLaunchKernelGGL(index_normalise_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream,
                     partials, kHistBlocks, freqs, tables);
  return rgbac::check_launch("rgbac_index_exact_tables (normalise)");
}

extern "C" int rgbac_index_exact_sizes(int batch, const rgbac_image_desc* descs, int ngroups,
                                       const rgbac_alpha_group* groups,
                                       const int32_t* block_base, int total_blocks,
                                       const int32_t* cls, const uint16_t* tables,
                                       int32_t* counts, int32_t* err, void* stream) {
  INDEX_REQUIRE_COMMON();
  INDEX_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls && tables && counts && err, "null pointer");
  INDEX_REQUIRE_TABLES();
  hipLaunchKernelGGL(index_code_kernel<false>, dim3(ngroups), dim3(kLanes), 0,
                     (hipStream_t)stream, batch, descs, groups, block_base, total_blocks, cls,
                     tables, counts, (const int64_t*)nullptr, (uint32_t*)nullptr, (int64_t)0,
                     err);
  return rgbac::check_launch("rgbac_index_exact_sizes");
}

extern "C" int rgbac_index_exact_encode(int batch, const rgbac_image_desc* descs, int ngroups,
                                        const rgbac_alpha_group* groups,
                                        const int32_t* block_base, int total_blocks,
                                        const int32_t* cls, const uint16_t* tables,
                                        const int32_t* counts, const int64_t* ends,
                                        uint32_t* payload, int64_t payload_words, int32_t* err,
                                        void* stream) {
  INDEX_REQUIRE_COMMON();
  INDEX_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls && tables && counts && ends && payload && err, "null pointer");
  INDEX_REQUIRE_TABLES();
  RGBAC_REQUIRE(payload_words >= 2, "payload smaller than one chunk's state words");
  hipLaunchKernelGGL(index_code_kernel<true>, dim3(ngroups), dim3(kLanes), 0,
                     (hipStream_t)stream, batch, descs, groups, block_base, total_blocks, cls,
                     tables, const_cast<int32_t*>(counts), ends, payload, payload_words, err);
  return rgbac::check_launch("rgbac_index_exact_encode");
}

extern "C" int rgbac_index_exact_decode(int batch, const rgbac_image_desc* descs, int ngroups,
                                        const rgbac_alpha_group* groups,
                                        const int32_t* block_base, int total_blocks,
                                        const int32_t* cls, const uint16_t* tables,
                                        const int64_t* word_off, const int32_t* counts,
                                        const uint32_t* payload, int64_t payload_words,
                                        int32_t* err, void* stream) {
  INDEX_REQUIRE_COMMON();
  INDEX_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls && tables && word_off && counts && payload && err, "null pointer");
  INDEX_REQUIRE_TABLES();
  RGBAC_REQUIRE(payload_words >= 0, "payload_words must not be negative");
  hipLaunchKernelGGL(index_decode_kernel, dim3(ngroups), dim3(kLanes), 0, (hipStream_t)stream,
                     batch, descs, groups, block_base, total_blocks, cls, tables, word_off,
                     counts, payload, payload_words, err);
  return rgbac::check_launch("rgbac_index_exact_decode");
}
