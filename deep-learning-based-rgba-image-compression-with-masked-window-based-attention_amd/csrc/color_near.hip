// Near-lossless colour of packed RGBA: a closed-loop MED predictor with a uniform quantiser of
// the prediction error and the static-model rANS coder of csrc/color_exact.hip, on the device for
// a whole ragged batch (rgbac/rgbanear.py).  The alpha plane is coded
// exactly by csrc/alpha_exact.hip; this file codes R, G, B of the visible pixels so that every
// byte comes back within +-delta.
//
// Blocks, groups, visibility, which neighbours EXIST, the five contexts and the class word layout
// are color_exact.hip's.  What differs, with step = 2 delta + 1 and
// Q(e) = sgn(e) * ((|e| + delta) div step):
//   * plane 0 is G, planes 1 and 2 are R and B.  Every prediction reads RECONSTRUCTED values (the
//     values the decoder will have): the plane value of a neighbour n is G^(n) for plane 0 and
//     C^(n) - G^(n), signed, for a chroma plane.  color_exact.hip's rule over the plane values of
//     L, U, D gives p and the context; the predicted colour is P = p for G and
//     P = clamp(G^(here) + p, 0, 255) for chroma;
//   * q = Q(C - P), C^ = clamp(P + q * step, 0, 255), symbol q & 255, table channel * 5 + context;
//   * a channel whose values over the block's visible pixels span at most 2 delta is constant:
//     its value, and its reconstruction, is (min + max) >> 1.
// Q(C^ - P) = q even where the clamp acted, so every symbol is a function of the reconstructed
// image alone.  Only the first kernel runs the closed loop; the others read what it settled.
//
// Per-image mode word (modes[image]): bits 0-7 delta in 1..16, bit 8 keep_hidden.
//
// Kernels (one launch each for the whole batch; every image access is one aligned dword):
//   settle     classify and the closed loop.  Grid: groups of 64 blocks, 4 waves, a wave takes 16
//              blocks four at a time: 16 lanes per block.  Staging: lane x loads column x of its
//              block, row by row (16 consecutive dwords per block row), into a 256-dword LDS tile
//              and keeps min / max of the three channels over its visible pixels; four xor
//              shuffles inside the 16 lanes give the block's span: the class word.  Then the
//              anti-diagonal wavefront: at step s = 0..30 lane r owns pixel (r, s - r), whose
//              neighbours (r, c - 1), (r - 1, c), (r - 1, c - 1) were settled at steps s - 1,
//              s - 1, s - 2.  It settles G, then R and B against the new G, and overwrites the
//              tile's dword in place.  The tile goes out as alpha | RGB^ (0 on hidden pixels)
//              into the settled image.  No scratch, no atomics.
//   histogram, normalise, sizes, encode   color_exact.hip's stages over the SETTLED image; the
//              symbol is Q(C^ - P), and a chroma lane reads plane 0 beside its own.
//   decode     wave c = channel, lane j = block.  Green leads by one row: at stage t = 0..16 wave
//              0 decodes row t of G, waves 1 and 2 row t - 1 of R and B, one workgroup barrier per
//              stage.  Along a row the lane carries the last pixel's value and its U (the next
//              pixel's L and D) in registers whenever the mask says the left neighbour exists,
//              so a pixel costs one LDS read per plane it touches plus its own store.
//
// LDS of the coding kernels: color_exact.hip's layout (three swizzled byte planes, masks, the
// image's 15 tables, class words, fills): 59 KiB, two workgroups per CU.
#include <hip/hip_runtime.h>

#include "common.h"
#include "rans_chunk.h"

namespace {

namespace rr = rgbac_rans;
typedef rgbac_image_desc ImgDesc;
typedef rgbac_alpha_group Group;

constexpr int kEdge = RGBAC_ALPHA_BLOCK;            // 16
constexpr int kPix = kEdge * kEdge;                 // 256
constexpr int kCh = RGBAC_COLOR_CHANNELS;           // 3: G, R, B
constexpr int kCtx = RGBAC_ALPHA_CONTEXTS;          // 5 per channel
constexpr int kTabs = kCh * kCtx;                   // 15
constexpr int kBins = kTabs * 256;
constexpr int kLanes = RGBAC_ALPHA_GROUP;           // 64 blocks per group, one lane each
constexpr int kThreads = kCh * kLanes;              // 192: wave c serves channel c
constexpr int kHistBlocks = RGBAC_COLOR_HIST_BLOCKS;
constexpr int kTabU16 = RGBAC_COLOR_TABLE_U16;      // 15 * 256 starts + 15 last + 1 pad
constexpr int kMaxDelta = RGBAC_NEAR_MAX_ERROR;     // 16
static_assert(kTabU16 == kBins + kTabs + 1 && kTabU16 % 2 == 0, "table layout");
static_assert(kEdge == 16 && kLanes == 64 && kCh == 3, "the index arithmetic assumes 16 / 64 / 3");

struct Image {
  const uint8_t* p;
  int h, w;
  long long rs;
  int bx, nblk;     // blocks per row, blocks in all
  int base;         // the image's first entry of the per-block arrays
};

// image b, or false if its descriptor or its range of the per-block arrays does not hold
// together (nothing of it is touched then)
__device__ inline bool image_of(const ImgDesc* descs, const int32_t* block_base, int b,
                                int total_blocks, Image& im) {
  const ImgDesc d = descs[b];
  if (!d.ptr || d.h <= 0 || d.w <= 0) return false;
  if (((uintptr_t)d.ptr & 3) || (d.row_stride_bytes & 3)) return false;    // dword pixels
  im.p = reinterpret_cast<const uint8_t*>(d.ptr);
  im.h = d.h;
  im.w = d.w;
  im.rs = d.row_stride_bytes;
  im.bx = (d.w + kEdge - 1) / kEdge;
  const long long n = (long long)im.bx * ((d.h + kEdge - 1) / kEdge);
  im.base = block_base[b];
  if (im.base < 0 || n > total_blocks || im.base > total_blocks - n) return false;
  im.nblk = (int)n;
  return true;
}

struct Block {
  const uint8_t* p;   // its first pixel
  int bh, bw;
};

__device__ inline Block block_of(const Image& im, int k) {
  const int by = k / im.bx, bxi = k - by * im.bx;
  const int r0 = by * kEdge, c0 = bxi * kEdge;
  Block bl;
  bl.p = im.p + (long long)r0 * im.rs + (long long)c0 * 4;
  bl.bh = min(kEdge, im.h - r0);
  bl.bw = min(kEdge, im.w - c0);
  return bl;
}

__device__ inline uint32_t* pixel_at(const Image& im, const Block& bl, int r, int c) {
  return reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(bl.p) + (long long)r * im.rs + c * 4);
}

// what an image's mode word says
struct Quant {
  int delta, step, qmax;
  uint32_t inv;       // ceil(2^16 / step): n div step = (n * inv) >> 16 for every n <= 255 + 16
  bool keep;
};

__device__ inline bool quant_of(const int32_t* modes, int b, Quant& q) {
  const int m = modes[b];
  q.delta = m & 255;
  q.keep = (m & RGBAC_NEAR_KEEP_HIDDEN) != 0;
  if ((m & ~(255 | RGBAC_NEAR_KEEP_HIDDEN)) || q.delta < 1 || q.delta > kMaxDelta) return false;
  q.step = 2 * q.delta + 1;
  q.inv = (65536u + q.step - 1) / q.step;
  q.qmax = ((255 + q.delta) * q.inv) >> 16;
  return true;
}

__device__ inline int quantise(int e, const Quant& q) {
  const int n = (int)(((uint32_t)(abs(e) + q.delta) * q.inv) >> 16);
  return e < 0 ? -n : n;
}

__device__ inline int clamp255(int v) { return min(max(v, 0), 255); }

// channel ch of a pixel R | G << 8 | B << 16: 0 is G, 1 is R, 2 is B
__device__ inline int colour_of(uint32_t px, int ch) {
  return (px >> (ch == 0 ? 8 : (ch == 1 ? 0 : 16))) & 255;
}

// prediction and context from the neighbours that exist (color_exact.hip's rule; the values may
// be negative here)
__device__ inline void vis_model(bool eL, bool eU, bool eD, int L, int U, int D, int& pred,
                                 int& ctx) {
  if (eL && eU) {
    if (!eD) D = L;
    const int lo = min(L, U), hi = max(L, U);
    pred = D >= hi ? lo : (D <= lo ? hi : L + U - D);
    const int d = max(hi, D) - min(lo, D);
    ctx = d == 0 ? 0 : (d <= 8 ? 1 : (d <= 64 ? 2 : 3));
  } else if (eL || eU || eD) {
    pred = eL ? L : (eU ? U : D);
    ctx = 0;
  } else {
    pred = 0;
    ctx = 4;
  }
}

// predicted colour P and context of channel ch from the settled neighbour pixels L, U, D; g:
// the reconstructed green of the pixel itself
__device__ inline void pixel_model(int ch, int g, bool eL, bool eU, bool eD, uint32_t L,
                                   uint32_t U, uint32_t D, int& P, int& ctx) {
  int p;
  if (ch == 0) {
    vis_model(eL, eU, eD, colour_of(L, 0), colour_of(U, 0), colour_of(D, 0), p, ctx);
    P = p;
  } else {
    vis_model(eL, eU, eD, colour_of(L, ch) - colour_of(L, 0), colour_of(U, ch) - colour_of(U, 0),
              colour_of(D, ch) - colour_of(D, 0), p, ctx);
    P = clamp255(g + p);
  }
}

// byte address of pos = r * 16 + c of lane-private block j (color_exact.hip's swizzle)
__device__ inline int swz(int j, int pos) {
  const int w = pos >> 2;
  return (((w << 6) + ((j + w) & 63)) << 2) + (pos & 3);
}

__device__ inline void report(int32_t* err, int32_t code) {
  if (code) atomicCAS(err, 0, code);       // the first non-zero code wins
}

__device__ inline bool has_chunk(uint32_t cw, int ch) {
  return !(cw & 1u) && !((cw >> (1 + ch)) & 1u);
}
__device__ inline bool has_any_chunk(uint32_t cw) { return !(cw & 1u) && (cw & 14u) != 14u; }

// ------------------------------------------------------------------ settle
constexpr int kSlot = kPix + 8;             // dwords between the tiles of a wave's four blocks

// grid: groups; 4 waves, wave v takes blocks block0 + 16 v .. + 16 of the group, four at a time
__global__ __launch_bounds__(256) void near_settle_kernel(
    int batch, const ImgDesc* __restrict__ src, const ImgDesc* __restrict__ dst,
    const int32_t* __restrict__ modes, const Group* __restrict__ groups,
    const int32_t* __restrict__ block_base, int total_blocks, uint32_t* __restrict__ cls,
    int32_t* err) {
  __shared__ uint32_t tiles[4][4][kSlot];
  const Group g = groups[blockIdx.x];
  Image im, om;
  Quant qu;
  if (g.image < 0 || g.image >= batch || g.block0 < 0 ||
      !image_of(src, block_base, g.image, total_blocks, im) ||
      !image_of(dst, block_base, g.image, total_blocks, om) || om.h != im.h || om.w != im.w ||
      !quant_of(modes, g.image, qu)) {
    if (threadIdx.x == 0) report(err, rr::kErrChunk);
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = lane >> 4, x = lane & 15;   // x: the lane's column while staging, its row after
  uint32_t* t = tiles[wave][slot];
  // every trip count below is the same for all threads: the barriers are workgroup-uniform
  for (int i = 0; i < kLanes / 16; ++i) {
    const int k = g.block0 + wave * (kLanes / 4) + i * 4 + slot;
    const bool have = k < im.nblk;
    Block bl = {nullptr, 0, 0}, ob = {nullptr, 0, 0};
    if (have) {
      bl = block_of(im, k);
      ob = block_of(om, k);
    }
    int lo[kCh] = {255, 255, 255}, hi[kCh] = {0, 0, 0}, any = 0;
#pragma unroll
    for (int y = 0; y < kEdge; ++y) {
      const bool in = y < bl.bh && x < bl.bw;
      const uint32_t p = in ? *pixel_at(im, bl, y, x) : 0u;
      const bool v = in && (qu.keep || (p >> 24));
      t[y * kEdge + x] = v ? p : 0u;           // hidden: alpha 0 already, RGB 0 from here on
      if (v) {
        any = 1;
#pragma unroll
        for (int ch = 0; ch < kCh; ++ch) {
          lo[ch] = min(lo[ch], colour_of(p, ch));
          hi[ch] = max(hi[ch], colour_of(p, ch));
        }
      }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {          // stays inside the block's 16 lanes
      any |= __shfl_xor(any, o);
#pragma unroll
      for (int ch = 0; ch < kCh; ++ch) {
        lo[ch] = min(lo[ch], __shfl_xor(lo[ch], o));
        hi[ch] = max(hi[ch], __shfl_xor(hi[ch], o));
      }
    }
    uint32_t word = 1u;
    if (any) {
      word = 0u;
#pragma unroll
      for (int ch = 0; ch < kCh; ++ch)
        if (hi[ch] - lo[ch] <= 2 * qu.delta)
          word |= (2u << ch) | ((uint32_t)((lo[ch] + hi[ch]) >> 1) << (8 + 8 * ch));
    }
    if (have && x == 0) cls[im.base + k] = word;
    __syncthreads();
    // the wavefront: lane x is row x; a constant channel's reconstruction is its value
    for (int s = 0; s < 2 * kEdge - 1; ++s) {
      const int c = s - x;
      if (any && c >= 0 && c < bl.bw && x < bl.bh) {
        const int pos = x * kEdge + c;
        const uint32_t p = t[pos];
        if (qu.keep || (p >> 24)) {
          const uint32_t L = c ? t[pos - 1] : 0u, U = x ? t[pos - kEdge] : 0u;
          const uint32_t D = (x && c) ? t[pos - kEdge - 1] : 0u;
          const bool eL = c && (qu.keep || (L >> 24)), eU = x && (qu.keep || (U >> 24));
          const bool eD = x && c && (qu.keep || (D >> 24));
          int out[kCh] = {0, 0, 0};
#pragma unroll
          for (int ch = 0; ch < kCh; ++ch) {
            if ((word >> (1 + ch)) & 1u) {
              out[ch] = (word >> (8 + 8 * ch)) & 255;
            } else {
              int P, ctx;
              pixel_model(ch, out[0], eL, eU, eD, L, U, D, P, ctx);
              out[ch] = clamp255(P + quantise(colour_of(p, ch) - P, qu) * qu.step);
            }
          }
          t[pos] = (p & 0xFF000000u) | (uint32_t)out[1] | ((uint32_t)out[0] << 8) |
                   ((uint32_t)out[2] << 16);
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int y = 0; y < kEdge; ++y)
      if (y < ob.bh && x < ob.bw) *pixel_at(om, ob, y, x) = t[y * kEdge + x];
    __syncthreads();
  }
}

// ------------------------------------------------------------------ histogram
// descs: the settled images
__global__ __launch_bounds__(256) void near_histogram_kernel(
    const ImgDesc* __restrict__ descs, const int32_t* __restrict__ modes,
    const int32_t* __restrict__ block_base, int total_blocks, const uint32_t* __restrict__ cls,
    uint32_t* __restrict__ partials) {
  __shared__ uint32_t hist[kBins];
  __shared__ uint32_t tile[4][kPix];        // per wave: R | G << 8 | B << 16 | visible << 24
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < kBins; i += 256) hist[i] = 0;
  __syncthreads();
  Image im;
  Quant qu;
  if (image_of(descs, block_base, b, total_blocks, im) && quant_of(modes, b, qu)) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* tw = tile[wave];
    // the four waves step together so that the barriers around the tile are workgroup-uniform
    for (int k0 = blockIdx.x * 4; k0 < im.nblk; k0 += gridDim.x * 4) {
      const int k = k0 + wave;
      const uint32_t cw = k < im.nblk ? cls[im.base + k] : 1u;
      const bool work = has_any_chunk(cw);                // wave-uniform
      if (work) {
        const Block bl = block_of(im, k);
#pragma unroll
        for (int q = 0; q < kPix / 64; ++q) {
          const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
          const bool in = r < bl.bh && c < bl.bw;
          const uint32_t p = in ? *pixel_at(im, bl, r, c) : 0u;
          const uint32_t v = in && (qu.keep || (p >> 24)) ? 1u : 0u;
          tw[pos] = (p & 0xFFFFFFu) | (v << 24);
        }
      }
      __syncthreads();
      if (work) {
#pragma unroll
        for (int q = 0; q < kPix / 64; ++q) {
          const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
          const uint32_t v = tw[pos];
          if (!(v >> 24)) continue;
          const uint32_t L = c ? tw[pos - 1] : 0u, U = r ? tw[pos - kEdge] : 0u;
          const uint32_t D = (r && c) ? tw[pos - kEdge - 1] : 0u;
#pragma unroll
          for (int ch = 0; ch < kCh; ++ch) {
            if (!has_chunk(cw, ch)) continue;
            int P, ctx;
            pixel_model(ch, colour_of(v, 0), L >> 24, U >> 24, D >> 24, L, U, D, P, ctx);
            const int sym = quantise(colour_of(v, ch) - P, qu) & 255;
            atomicAdd(&hist[(ch * kCtx + ctx) * 256 + sym], 1u);
          }
        }
      }
      __syncthreads();
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

// grid: (15 tables, images); thread t owns symbol t.  The rule is alpha_exact.hip's.
__global__ __launch_bounds__(256) void near_normalise_kernel(
    const uint32_t* __restrict__ partials, int nparts, int32_t* __restrict__ freqs,
    uint16_t* __restrict__ tables) {
  __shared__ unsigned long long sh[256];
  __shared__ uint32_t scan[2][256];
  const int tb = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  auto add = [](unsigned long long x, unsigned long long y) { return x + y; };
  auto mx = [](unsigned long long x, unsigned long long y) { return x > y ? x : y; };
  unsigned long long c = 0;
  for (int g = 0; g < nparts; ++g) c += partials[((size_t)b * nparts + g) * kBins + tb * 256 + t];
  const unsigned long long total = block_reduce(c, sh, add);
  uint32_t f = 0;
  int last = -1;
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
    last = (int)block_reduce(f ? (unsigned)t + 1 : 0, sh, mx) - 1;
  }
  freqs[((size_t)b * kTabs + tb) * 256 + t] = (int32_t)f;
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
  tab[tb * 256 + t] = (uint16_t)(scan[cur][t] - f);
  if (t == 0) tab[kBins + tb] = (uint16_t)(int16_t)last;
  if (t == 0 && tb == 0) tab[kBins + kTabs] = 0;
}

// one image's tables in LDS: start[table * 256 + s], last[table] (int16, -1 = empty)
__device__ inline void stage_table(const uint16_t* __restrict__ tables, int b, uint16_t* tab) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(tables + (size_t)b * kTabU16);
  uint32_t* dst = reinterpret_cast<uint32_t*>(tab);
  for (int i = threadIdx.x; i < kTabU16 / 2; i += kThreads) dst[i] = src[i];
}

// start and frequency of symbol s in table tb; freq 0: the symbol has none
__device__ inline void table_entry(const uint16_t* tab, int tb, int s, uint32_t& start,
                                   uint32_t& freq) {
  const int last = (int16_t)tab[kBins + tb];
  start = tab[tb * 256 + s];
  if (s > last)
    freq = 0;
  else if (s == last)
    freq = 65536u - start;
  else
    freq = (uint32_t)tab[tb * 256 + s + 1] - start;
}

// The LDS of the coding kernels (one struct so that both kernels lay it out alike).
struct Shared {
  uint8_t planes[kCh][kLanes * kPix];                       // 48 KiB, swz layout: G^, R^, B^
  uint16_t vmask[kEdge * kLanes];                           // row r of block j at r * 64 + j
  __attribute__((aligned(4))) uint16_t tab[kTabU16];
  uint32_t cls[kLanes];
  int32_t fill[kCh][kLanes];                                // decode: >= 0 a constant channel
  uint32_t bad[kLanes];                                     // decode: the block decodes to RGB 0
};
static_assert(sizeof(Shared) <= 64 * 1024, "static LDS of one workgroup");

// One wave stages block k of the image as block j of the group: every lane loads 4 pixels as
// dwords; kPlanes: the three colour bytes go to the planes; always: the visibility of the 64
// pixels of a quarter is one ballot, whose four 16-bit rows lanes 0..3 store.
template <bool kPlanes>
__device__ inline void stage_block(const Image& im, int k, bool keep_hidden, int j, int lane,
                                   Shared& sh) {
  const Block bl = block_of(im, k);
#pragma unroll
  for (int q = 0; q < kPix / 64; ++q) {
    const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
    const bool in = r < bl.bh && c < bl.bw;
    const uint32_t p = in ? *pixel_at(im, bl, r, c) : 0u;
    if (kPlanes) {
      const int a = swz(j, pos);
      sh.planes[0][a] = (uint8_t)(p >> 8);
      sh.planes[1][a] = (uint8_t)p;
      sh.planes[2][a] = (uint8_t)(p >> 16);
    }
    const unsigned long long b = __ballot(in && (keep_hidden || (p >> 24)));
    if (lane < 4) sh.vmask[(4 * q + lane) * kLanes + j] = (uint16_t)(b >> (16 * lane));
  }
}

// predicted colour and context of channel ch at (r, c) of block j from the LDS planes; m, mp:
// the visibility masks of row r and of row r - 1 (0 above the block)
__device__ inline void planes_model(const Shared& sh, int ch, int j, int r, int c, uint32_t m,
                                    uint32_t mp, int& P, int& ctx) {
  const bool eL = ((m << 1) >> c) & 1u, eU = (mp >> c) & 1u, eD = ((mp << 1) >> c) & 1u;
  const int pos = r * kEdge + c;
  const int aL = swz(j, pos - 1), aU = swz(j, pos - kEdge), aD = swz(j, pos - kEdge - 1);
  const uint8_t* gp = sh.planes[0];
  int L = eL ? gp[aL] : 0, U = eU ? gp[aU] : 0, D = eD ? gp[aD] : 0, g = 0;
  if (ch) {
    const uint8_t* op = sh.planes[ch];
    g = gp[swz(j, pos)];
    L = eL ? op[aL] - L : 0;
    U = eU ? op[aU] - U : 0;
    D = eD ? op[aD] - D : 0;
  }
  int p;
  vis_model(eL, eU, eD, L, U, D, p, ctx);
  P = ch ? clamp255(g + p) : p;
}

// ------------------------------------------------------------------ sizes / encode
// descs: the settled images
template <bool kStore>
__global__ __launch_bounds__(kThreads) void near_code_kernel(
    int batch, const ImgDesc* __restrict__ descs, const int32_t* __restrict__ modes,
    const Group* __restrict__ groups, const int32_t* __restrict__ block_base, int total_blocks,
    const uint32_t* __restrict__ cls, const uint16_t* __restrict__ tables,
    int32_t* __restrict__ counts, const int64_t* __restrict__ ends,
    uint32_t* __restrict__ payload, int64_t payload_words, int32_t* err) {
  __shared__ Shared sh;
  const Group g = groups[blockIdx.x];
  Image im;
  Quant qu;
  if (g.image < 0 || g.image >= batch || g.block0 < 0 ||
      !image_of(descs, block_base, g.image, total_blocks, im) || !quant_of(modes, g.image, qu)) {
    if (threadIdx.x == 0) report(err, rr::kErrChunk);
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nb = min(kLanes, im.nblk - g.block0);           // <= 0: a group past the image
  if ((int)threadIdx.x < nb) sh.cls[threadIdx.x] = cls[im.base + g.block0 + threadIdx.x];
  stage_table(tables, g.image, sh.tab);
  __syncthreads();
  for (int j = wave; j < nb; j += kCh)
    if (has_any_chunk(sh.cls[j])) stage_block<true>(im, g.block0 + j, qu.keep, j, lane, sh);
  __syncthreads();
  // from here on: wave = channel, lane = block
  if (lane >= nb) return;
  const int64_t ci = (int64_t)(im.base + g.block0 + lane) * kCh + wave;
  if (!has_chunk(sh.cls[lane], wave)) {
    if (!kStore) counts[ci] = 0;
    return;
  }
  int n = 0;
  for (int r = 0; r < kEdge; ++r) n += __popc(sh.vmask[r * kLanes + lane]);
  int32_t e = rr::kErrNone;
  int64_t cap = 0;
  uint32_t* end = nullptr;
  if (kStore) {
    // the words land in [end - cnt, end): cnt is what the sizes pass counted for this chunk
    const int64_t en = ends[ci];
    cap = counts[ci];
    if (cap < 2 || cap > n / 2 + 3 || en - cap < 0 || en > payload_words) {
      report(err, rr::kErrChunk);
      return;
    }
    end = payload + en;
  }
  const uint8_t* pln = sh.planes[wave];
  rr::detail::EncState s = {rr::kL, end, cap, 0};
  for (int r = kEdge - 1; r >= 0; --r) {
    const uint32_t m = sh.vmask[r * kLanes + lane];
    const uint32_t mp = r ? sh.vmask[(r - 1) * kLanes + lane] : 0u;
    uint32_t rest = m;
    while (rest) {
      const int c = 31 - __clz((int)rest);
      rest &= ~(1u << c);
      int P, ctx;
      planes_model(sh, wave, lane, r, c, m, mp, P, ctx);
      const int sym = quantise((int)pln[swz(lane, r * kEdge + c)] - P, qu) & 255;
      uint32_t start, freq;
      table_entry(sh.tab, wave * kCtx + ctx, sym, start, freq);
      if (freq == 0 || freq > 65535u) {                     // not this image's table
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
    counts[ci] = (int32_t)s.nwords;
  }
  report(err, e);
}

// ------------------------------------------------------------------ decode
__global__ __launch_bounds__(kThreads) void near_decode_kernel(
    int batch, const ImgDesc* __restrict__ descs, const int32_t* __restrict__ modes,
    const Group* __restrict__ groups, const int32_t* __restrict__ block_base, int total_blocks,
    const uint32_t* __restrict__ cls, const uint16_t* __restrict__ tables,
    const int64_t* __restrict__ word_off, const int32_t* __restrict__ counts,
    const uint32_t* __restrict__ payload, int64_t payload_words, int32_t* err) {
  __shared__ Shared sh;
  const Group g = groups[blockIdx.x];
  Image im;
  Quant qu;
  if (g.image < 0 || g.image >= batch || g.block0 < 0 ||
      !image_of(descs, block_base, g.image, total_blocks, im) || !quant_of(modes, g.image, qu)) {
    if (threadIdx.x == 0) report(err, rr::kErrChunk);
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nb = min(kLanes, im.nblk - g.block0);
  if ((int)threadIdx.x < nb) sh.cls[threadIdx.x] = cls[im.base + g.block0 + threadIdx.x];
  if (threadIdx.x < kLanes) sh.bad[threadIdx.x] = 0;
  stage_table(tables, g.image, sh.tab);
  // who is visible: the alpha bytes already lie in the destination
  for (int j = wave; j < nb; j += kCh) stage_block<false>(im, g.block0 + j, qu.keep, j, lane, sh);
  __syncthreads();
  // wave = channel, lane = block.  ``run``: the lane has a chunk to decode.
  bool run = false;
  int32_t e = rr::kErrNone, value = -1;
  int gfix = -1;                                            // >= 0: the block's green is constant
  rr::detail::DecState d = {0, payload, 0, 0, rr::kErrNone};
  if (lane < nb) {
    const uint32_t cw = sh.cls[lane];
    int n = 0;
    for (int r = 0; r < kEdge; ++r) n += __popc(sh.vmask[r * kLanes + lane]);
    if (cw & 2u) gfix = (cw >> 8) & 255;
    if (((cw & 1u) != 0) != (n == 0)) {
      e = rr::kErrCorrupt;                                  // the class word is another mask's
    } else if (!has_chunk(cw, wave)) {
      value = (cw >> (8 + 8 * wave)) & 255;                 // (a hidden block writes no colour)
    } else {
      const int64_t ci = (int64_t)(im.base + g.block0 + lane) * kCh + wave;
      const int64_t off = word_off[ci];
      const int32_t cnt = counts[ci];
      if (n < 2 || cnt < 2 || cnt > n / 2 + 3) {
        e = rr::kErrCorrupt;                                // an impossible count
      } else if (off < 0 || off > payload_words - cnt) {
        e = rr::kErrChunk;
      } else {
        d.words = payload + off;
        d.nwords = cnt;
        const uint32_t lo = rr::detail::dec_word(d), hi = rr::detail::dec_word(d);
        d.x = (uint64_t)lo | ((uint64_t)hi << 32);
        run = true;
      }
    }
  }
  uint8_t* pln = sh.planes[wave];
  const uint8_t* gpl = sh.planes[0];
  // stage t: green decodes row t, the chroma waves row t - 1, whose green is complete
  for (int t = 0; t <= kEdge; ++t) {
    const int r = wave == 0 ? t : t - 1;
    if (run && !d.err && r >= 0 && r < kEdge) {
      const uint32_t m = sh.vmask[r * kLanes + lane];
      const uint32_t mp = r ? sh.vmask[(r - 1) * kLanes + lane] : 0u;
      uint32_t rest = m;
      // of the pixel decoded last: its value and its U, and green's; the next pixel's L and D
      // when its left neighbour exists (then that neighbour IS the pixel decoded last)
      int pv = 0, pu = 0, pg = 0, pgu = 0;
      while (rest) {
        const int c = __ffs((int)rest) - 1;
        rest &= rest - 1;
        const bool eL = ((m << 1) >> c) & 1u, eU = (mp >> c) & 1u, eD = ((mp << 1) >> c) & 1u;
        const int pos = r * kEdge + c;
        const int u = eU ? pln[swz(lane, pos - kEdge)] : 0;
        int L = eL ? pv : 0, U = u;
        int D = eD ? (eL ? pu : pln[swz(lane, pos - kEdge - 1)]) : 0;
        int gc = 0, gu = 0;
        if (wave) {
          gc = gfix >= 0 ? gfix : gpl[swz(lane, pos)];
          gu = !eU ? 0 : (gfix >= 0 ? gfix : gpl[swz(lane, pos - kEdge)]);
          const int gd = !eD ? 0 : (eL ? pgu : (gfix >= 0 ? gfix : gpl[swz(lane, pos - kEdge - 1)]));
          L -= eL ? pg : 0;
          U -= gu;
          D -= gd;
        }
        int p, ctx;
        vis_model(eL, eU, eD, L, U, D, p, ctx);
        const int P = wave ? clamp255(gc + p) : p;
        const int tb = wave * kCtx + ctx;
        const int last = (int16_t)sh.tab[kBins + tb];
        if (last < 0) {                                     // a symbol in an empty context
          d.err = rr::kErrCorrupt;
          break;
        }
        const uint32_t cum = (uint32_t)(d.x & 0xFFFFu);
        // the last symbol whose start is <= cum: at most 8 steps
        int slo = 0, shi = last;
        const uint16_t* row = sh.tab + tb * 256;
        while (slo < shi) {
          const int mid = (slo + shi + 1) >> 1;
          if (row[mid] <= cum) slo = mid; else shi = mid - 1;
        }
        uint32_t start, freq;
        table_entry(sh.tab, tb, slo, start, freq);
        const int q = (int8_t)slo;
        if (freq == 0 || cum - start >= freq || abs(q) > qu.qmax) {   // no table / no such error
          d.err = rr::kErrCorrupt;
          break;
        }
        uint64_t x = d.x;
        x = freq * (x >> rr::kPrecision) + cum - start;
        if (x < rr::kL) x = (x << 32) | rr::detail::dec_word(d);
        d.x = x;
        pv = clamp255(P + q * qu.step);
        pu = u;
        pg = gc;
        pgu = gu;
        pln[swz(lane, pos)] = (uint8_t)pv;
      }
    }
    __syncthreads();
  }
  if (lane < nb) {
    if (run) {
      // a sound chunk ends where the encoder began: every word read, the state back at kL
      if (!d.err && (d.x != rr::kL || d.pos != d.nwords)) d.err = rr::kErrCorrupt;
      e = d.err;
    }
    sh.fill[wave][lane] = value;
    if (e) sh.bad[lane] = 1;                                // a bad block decodes to RGB 0
    report(err, e);
  }
  __syncthreads();
  for (int j = wave; j < nb; j += kCh) {
    const Block bl = block_of(im, g.block0 + j);
    const bool zero = sh.bad[j] || (sh.cls[j] & 1u);
    const int32_t fg = sh.fill[0][j], fr = sh.fill[1][j], fb = sh.fill[2][j];
#pragma unroll
    for (int q = 0; q < kPix / 64; ++q) {
      const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
      if (r >= bl.bh || c >= bl.bw) continue;
      uint32_t* dst = pixel_at(im, bl, r, c);
      const uint32_t a = *dst & 0xFF000000u;
      uint32_t rgb = 0;
      if (!zero && ((sh.vmask[r * kLanes + j] >> c) & 1u)) {
        const int at = swz(j, pos);
        rgb = (fr >= 0 ? (uint32_t)fr : sh.planes[1][at]) |
              ((fg >= 0 ? (uint32_t)fg : sh.planes[0][at]) << 8) |
              ((fb >= 0 ? (uint32_t)fb : sh.planes[2][at]) << 16);
      }
      *dst = a | rgb;
    }
  }
}

}  // namespace

#define NEAR_REQUIRE_COMMON()                                                               \
  RGBAC_REQUIRE(batch > 0 && batch <= 65535, "batch must be in [1, 65535]");                \
  RGBAC_REQUIRE(descs && modes && block_base, "null pointer");                              \
  RGBAC_REQUIRE(total_blocks > 0 && total_blocks <= INT32_MAX / 4,                          \
                "total_blocks must be in [1, 2^29)")
#define NEAR_REQUIRE_GROUPS() \
  RGBAC_REQUIRE(groups && ngroups > 0, "group table")

extern "C" int rgbac_color_near_settle(int batch, const rgbac_image_desc* descs,
                                       const rgbac_image_desc* settled, const int32_t* modes,
                                       int ngroups, const rgbac_alpha_group* groups,
                                       const int32_t* block_base, int total_blocks,
                                       uint32_t* cls, int32_t* err, void* stream) {
  NEAR_REQUIRE_COMMON();
  NEAR_REQUIRE_GROUPS();
  RGBAC_REQUIRE(settled && cls && err, "null pointer");
  hipLaunchKernelGGL(near_settle_kernel, dim3(ngroups), dim3(256), 0, (hipStream_t)stream, batch,
                     descs, settled, modes, groups, block_base, total_blocks, cls, err);
  return rgbac::check_launch("rgbac_color_near_settle");
}

extern "C" int rgbac_color_near_tables(int batch, const rgbac_image_desc* descs,
                                       const int32_t* modes, const int32_t* block_base,
                                       int total_blocks, const uint32_t* cls, uint32_t* partials,
                                       int32_t* freqs, uint16_t* tables, void* stream) {
  NEAR_REQUIRE_COMMON();
  RGBAC_REQUIRE(cls && partials && freqs && tables, "null pointer");
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned");
  hipLaunchKernelGGL(near_histogram_kernel, dim3(kHistBlocks, batch), dim3(256), 0,
                     (hipStream_t)stream, descs, modes, block_base, total_blocks, cls, partials);
  const int rc = rgbac::check_launch("rgbac_color_near_tables (histogram)");
  if (rc) return rc;
  hipLaunchKernelGGL(near_normalise_kernel, dim3(kTabs, batch), dim3(256), 0,
                     (hipStream_t)stream, partials, kHistBlocks, freqs, tables);
  return rgbac::check_launch("rgbac_color_near_tables (normalise)");
}

extern "C" int rgbac_color_near_sizes(int batch, const rgbac_image_desc* descs,
                                      const int32_t* modes, int ngroups,
                                      const rgbac_alpha_group* groups, const int32_t* block_base,
                                      int total_blocks, const uint32_t* cls,
                                      const uint16_t* tables, int32_t* counts, int32_t* err,
                                      void* stream) {
  NEAR_REQUIRE_COMMON();
  NEAR_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls && tables && counts && err, "null pointer");
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned");
  hipLaunchKernelGGL(near_code_kernel<false>, dim3(ngroups), dim3(kThreads), 0,
                     (hipStream_t)stream, batch, descs, modes, groups, block_base, total_blocks,
                     cls, tables, counts, (const int64_t*)nullptr, (uint32_t*)nullptr,
                     (int64_t)0, err);
  return rgbac::check_launch("rgbac_color_near_sizes");
}

extern "C" int rgbac_color_near_encode(int batch, const rgbac_image_desc* descs,
                                       const int32_t* modes, int ngroups,
                                       const rgbac_alpha_group* groups, const int32_t* block_base,
                                       int total_blocks, const uint32_t* cls,
                                       const uint16_t* tables, const int32_t* counts,
                                       const int64_t* ends, uint32_t* payload,
                                       int64_t payload_words, int32_t* err, void* stream) {
  NEAR_REQUIRE_COMMON();
  NEAR_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls && tables && counts && ends && payload && err, "null pointer");
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned");
  RGBAC_REQUIRE(payload_words >= 2, "payload smaller than one chunk's state words");
  hipLaunchKernelGGL(near_code_kernel<true>, dim3(ngroups), dim3(kThreads), 0,
                     (hipStream_t)stream, batch, descs, modes, groups, block_base, total_blocks,
                     cls, tables, const_cast<int32_t*>(counts), ends, payload, payload_words, err);
  return rgbac::check_launch("rgbac_color_near_encode");
}

extern "C" int rgbac_color_near_decode(int batch, const rgbac_image_desc* descs,
                                       const int32_t* modes, int ngroups,
                                       const rgbac_alpha_group* groups, const int32_t* block_base,
                                       int total_blocks, const uint32_t* cls,
                                       const uint16_t* tables, const int64_t* word_off,
                                       const int32_t* counts, const uint32_t* payload,
                                       int64_t payload_words, int32_t* err, void* stream) {
  NEAR_REQUIRE_COMMON();
  NEAR_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls && tables && word_off && counts && payload && err, "null pointer");
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned");
  RGBAC_REQUIRE(payload_words >= 0, "payload_words must not be negative");
  hipLaunchKernelGGL(near_decode_kernel, dim3(ngroups), dim3(kThreads), 0, (hipStream_t)stream,
                     batch, descs, modes, groups, block_base, total_blocks, cls, tables, word_off,
                     counts, payload, payload_words, err);
  return rgbac::check_launch("rgbac_color_near_decode");
}
