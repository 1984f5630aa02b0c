// Lossless colour of packed RGBA with the colour transform chosen per block on the device
// (rgbac/rgbalossless.py, version 2 RGAL files).  csrc/color_exact.hip
// subtracts green from red and blue in every block; where the channels do not move together
// that costs bits.  Here each block picks, for red and for blue on their own, between the
// difference and the plain channel.  What is not said here is color_exact.hip's: blocks, groups,
// visibility, which neighbours exist, prediction, contexts, chunk layout and order, the table
// rule; the small addressing helpers are repeated rather than moved.
//
// Five planes: Y = G, Cr = (R - G + 128) & 255, Cb = (B - G + 128) & 255, R, B: kinds 0..4.  A
// block has three SLOTS: 0 carries Y, 1 carries Cr or R, 2 carries Cb or B.  Class word of a
// block: color_exact.hip's, and bit 4: slot 1 holds plain R, bit 5: slot 2 holds plain B; the
// constant flags (bits 1-3) and value bytes refer to the plane the slot holds; bits 6, 7 are
// reserved; a hidden block's word is 1.  The choice of a slot over the block's visible pixels:
//   the difference plane is constant:      the difference (color_exact.hip's outcome);
//   otherwise the plain plane is constant: plain;
//   otherwise:                             plain iff cost(plain) < cost(difference),
// where cost(plane) is the sum over the visible pixels of min(s, 256 - s), s the pixel's symbol
// in that plane (at most 256 x 128 = 32,768: 16 bits).  A chunk is coded with table
// kind * 5 + context of its image, the kind its slot holds: 25 static tables per image.
//
// Kernels:
//   choose     one wave per block (4 per workgroup, 16 blocks each).  The wave puts the block's
//              256 pixels into 1 KiB of LDS as R | G | B | visible, one dword load per pixel, and
//              reads the neighbours from there; a lane forms the symbols of Cr, R, Cb, B of its 4
//              pixels.  Two costs share a dword, 16 bits each, so the four sums are two
//              butterflies of __shfl_xor; "constant" is the first visible pixel (ballot +
//              shuffle) and one __all per plane.  Lane 0 writes the word.  No scratch, no
//              atomics; the choice is a select on wave-uniform values.
//   histogram  grid (RGBAC_COLOR_HIST_BLOCKS, images): color_exact.hip's, with 25 x 256 u32 bins
//              (25,600 bytes) beside the four 1 KiB tiles.  The tile holds the raw pixel; a lane
//              forms only the planes its block's word selects.
//   normalise  grid (25, images).
//   sizes / encode / decode   color_exact.hip's split (192 threads, wave = slot, lane = block).
//              Staging writes the chosen plane's byte into plane `slot` from the class word, so
//              the walk over the masks and the coder calls are unchanged; only the table base
//              depends on the word.  Decode inverts per block from bits 4 and 5.  A word with a
//              reserved bit, or with bit 4 or 5 under the hidden bit, touches nothing of its
//              block and reports code 3.
//
// LDS of the coding kernels: color_exact.hip's struct with 25 tables (25 * 256 + 25 + 1 u16 =
// 12,852 bytes) instead of 15: 65,332 bytes, 204 under the static limit.
#include <hip/hip_runtime.h>

#include "common.h"
#include "rans_chunk.h"

namespace {

namespace rr = rgbac_rans;
typedef rgbac_image_desc ImgDesc;
typedef rgbac_alpha_group Group;

constexpr int kEdge = RGBAC_ALPHA_BLOCK;            // 16
constexpr int kPix = kEdge * kEdge;                 // 256
constexpr int kSlots = RGBAC_COLOR_CHANNELS;        // 3: Y, red, blue
constexpr int kKinds = RGBAC_COLOR_ADAPT_KINDS;     // 5: Y, Cr, Cb, R, B
constexpr int kCtx = RGBAC_ALPHA_CONTEXTS;          // 5 per kind
constexpr int kTabs = kKinds * kCtx;                // 25
constexpr int kBins = kTabs * 256;
constexpr int kLanes = RGBAC_ALPHA_GROUP;           // 64 blocks per group, one lane each
constexpr int kThreads = kSlots * kLanes;           // 192: wave s serves slot s
constexpr int kHistBlocks = RGBAC_COLOR_HIST_BLOCKS;
constexpr int kTabU16 = RGBAC_COLOR_ADAPT_TABLE_U16;  // 25 * 256 starts + 25 last + 1 pad
constexpr uint32_t kPlainR = 16u, kPlainB = 32u, kReserved = 0xC0u;
static_assert(kTabU16 == kBins + kTabs + 1 && kTabU16 % 2 == 0, "table layout");
static_assert(kEdge == 16 && kLanes == 64 && kSlots == 3 && kKinds == 5,
              "the index arithmetic assumes 16 / 64 / 3 / 5");

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

// R | G << 8 | B << 16 (| anything << 24) -> slot 0 | slot 1 << 8 | slot 2 << 16 under class
// word cw.  A plain slot subtracts 128 where the difference subtracts green, so that the centring
// +128 cancels: one expression for both, no branch.
__device__ inline uint32_t chosen(uint32_t p, uint32_t cw) {
  const uint32_t g = (p >> 8) & 255u;
  const uint32_t sr = (cw & kPlainR) ? 128u : g, sb = (cw & kPlainB) ? 128u : g;
  return g | (((p - sr + 128u) & 255u) << 8) | ((((p >> 16) - sb + 128u) & 255u) << 16);
}

// the three slots of a pixel under class word cw -> R | G << 8 | B << 16
__device__ inline uint32_t unchosen(uint32_t y, uint32_t s1, uint32_t s2, uint32_t cw) {
  const uint32_t ar = (cw & kPlainR) ? 128u : y, ab = (cw & kPlainB) ? 128u : y;
  return ((s1 + ar - 128u) & 255u) | (y << 8) | (((s2 + ab - 128u) & 255u) << 16);
}

// the kind (table group) that slot s of a block with class word cw holds
__device__ inline int kind_of(uint32_t cw, int s) {
  return s == 0 ? 0 : (s == 1 ? ((cw & kPlainR) ? 3 : 1) : ((cw & kPlainB) ? 4 : 2));
}

// a word the format allows: no reserved bit, no choice under the hidden bit
__device__ inline bool word_ok(uint32_t cw) {
  return !(cw & kReserved) && !((cw & 1u) && (cw & (kPlainR | kPlainB)));
}

// prediction and context from the neighbours that exist (color_exact.hip's rules)
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

// byte address of pos = r * 16 + c of lane-private block j (color_exact.hip's swizzle)
__device__ inline int swz(int j, int pos) {
  const int w = pos >> 2;
  return (((w << 6) + ((j + w) & 63)) << 2) + (pos & 3);
}

// the model of pixel (r, c) of block j from its LDS plane; m, mp: the visibility masks of row r
// and of row r - 1 (0 above the block)
__device__ inline void plane_model(const uint8_t* pln, int j, int r, int c, uint32_t m,
                                   uint32_t mp, int& pred, int& ctx) {
  const bool eL = ((m << 1) >> c) & 1u, eU = (mp >> c) & 1u, eD = ((mp << 1) >> c) & 1u;
  const int pos = r * kEdge + c;
  const int L = eL ? pln[swz(j, pos - 1)] : 0;
  const int U = eU ? pln[swz(j, pos - kEdge)] : 0;
  const int D = eD ? pln[swz(j, pos - kEdge - 1)] : 0;
  vis_model(eL, eU, eD, L, U, D, pred, ctx);
}

__device__ inline void report(int32_t* err, int32_t code) {
  if (code) atomicCAS(err, 0, code);       // the first non-zero code wins
}

__device__ inline bool has_chunk(uint32_t cw, int s) {
  return !(cw & 1u) && !((cw >> (1 + s)) & 1u);
}
__device__ inline bool has_any_chunk(uint32_t cw) { return !(cw & 1u) && (cw & 14u) != 14u; }

// one wave's tile entry of pixel pos of a block: R | G << 8 | B << 16 | visible << 24
__device__ inline uint32_t tile_pixel(const Image& im, const Block& bl, int pos, int keep_hidden) {
  const int r = pos >> 4, c = pos & 15;
  const bool in = r < bl.bh && c < bl.bw;
  const uint32_t p = in ? *pixel_at(im, bl, r, c) : 0u;
  const uint32_t v = in && (keep_hidden || (p >> 24)) ? 1u : 0u;
  return (p & 0xFFFFFFu) | (v << 24);
}

// ------------------------------------------------------------------ choose
// the cost min(s, 256 - s) of byte `shift` of v against the same byte of its neighbours
__device__ inline uint32_t cost_of(uint32_t v, uint32_t L, uint32_t U, uint32_t D, bool eL,
                                   bool eU, bool eD, int shift) {
  int pred, ctx;
  vis_model(eL, eU, eD, (L >> shift) & 255, (U >> shift) & 255, (D >> shift) & 255, pred, ctx);
  const int s = ((int)((v >> shift) & 255) - pred) & 255;
  return (uint32_t)min(s, 256 - s);
}

// grid: groups; 4 waves, wave v takes blocks block0 + 16 v .. + 16 of the group.  The waves step
// together so that the barriers around the tiles are workgroup-uniform.
__global__ __launch_bounds__(256) void adapt_choose_kernel(
    int batch, const ImgDesc* __restrict__ descs, int keep_hidden,
    const Group* __restrict__ groups, const int32_t* __restrict__ block_base, int total_blocks,
    uint32_t* __restrict__ cls) {
  __shared__ uint32_t tile[4][kPix];        // per wave: R | G << 8 | B << 16 | visible << 24
  const Group g = groups[blockIdx.x];
  Image im;
  if (g.image < 0 || g.image >= batch || g.block0 < 0 ||
      !image_of(descs, block_base, g.image, total_blocks, im))
    return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t* tw = tile[wave];
  const uint32_t diff = ~(kPlainR | kPlainB), plain = kPlainR | kPlainB;
  for (int i = 0; i < kLanes / 4; ++i) {
    if (g.block0 + i >= im.nblk) break;                   // wave 0 is done, so are the others
    const int k = g.block0 + wave * (kLanes / 4) + i;
    const bool work = k < im.nblk;                        // wave-uniform
    uint32_t px[kPix / 64];
    if (work) {
      const Block bl = block_of(im, k);
#pragma unroll
      for (int q = 0; q < kPix / 64; ++q) {
        px[q] = tile_pixel(im, bl, lane + 64 * q, keep_hidden);
        tw[lane + 64 * q] = px[q];
      }
    }
    __syncthreads();
    if (work) {
      uint32_t first = 0, cost_r = 0, cost_b = 0;         // Cr | R << 16, Cb | B << 16
      bool found = false;
#pragma unroll
      for (int q = 0; q < kPix / 64; ++q) {
        const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
        const uint32_t v = px[q];
        const unsigned long long b = __ballot(v >> 24);   // raster order: q, then lane
        if (!found && b) {                                // wave-uniform
          first = __shfl(v, __ffsll(b) - 1);
          found = true;
        }
        if (!(v >> 24)) continue;
        const uint32_t L = c ? tw[pos - 1] : 0u, U = r ? tw[pos - kEdge] : 0u;
        const uint32_t D = (r && c) ? tw[pos - kEdge - 1] : 0u;
        const bool eL = L >> 24, eU = U >> 24, eD = D >> 24;
        const uint32_t dv = chosen(v, diff), dL = chosen(L, diff), dU = chosen(U, diff),
                       dD = chosen(D, diff);
        cost_r += cost_of(dv, dL, dU, dD, eL, eU, eD, 8) |
                  (cost_of(v, L, U, D, eL, eU, eD, 0) << 16);
        cost_b += cost_of(dv, dL, dU, dD, eL, eU, eD, 16) |
                  (cost_of(v, L, U, D, eL, eU, eD, 16) << 16);
      }
      // a block's cost is at most 32,768 per field: the low sums never carry into the high ones
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        cost_r += __shfl_xor(cost_r, o);
        cost_b += __shfl_xor(cost_b, o);
      }
      // which of Y | Cr | Cb (bytes of d) and R | . | B (bytes of p) equal the first visible
      // pixel's over all visible pixels
      const uint32_t fd = chosen(first, diff), fp = chosen(first, plain);
      uint32_t dd = 0, dp = 0;
#pragma unroll
      for (int q = 0; q < kPix / 64; ++q) {
        if (!(px[q] >> 24)) continue;
        dd |= chosen(px[q], diff) ^ fd;
        dp |= chosen(px[q], plain) ^ fp;
      }
      const bool cy = __all(!(dd & 0xFFu));
      const bool ccr = __all(!(dd & 0xFF00u)), ccb = __all(!(dd & 0xFF0000u));
      const bool cr = __all(!(dp & 0xFF00u)), cb = __all(!(dp & 0xFF0000u));
      const bool pr = !ccr && (cr || (cost_r >> 16) < (cost_r & 0xFFFFu));
      const bool pb = !ccb && (cb || (cost_b >> 16) < (cost_b & 0xFFFFu));
      const uint32_t sel = (pr ? kPlainR : 0u) | (pb ? kPlainB : 0u);
      const uint32_t fs = chosen(first, sel);
      const uint32_t flags = (cy ? 1u : 0u) | ((ccr || cr) ? 2u : 0u) | ((ccb || cb) ? 4u : 0u);
      const uint32_t keep = ((flags & 1u) ? 0xFFu : 0u) | ((flags & 2u) ? 0xFF00u : 0u) |
                            ((flags & 4u) ? 0xFF0000u : 0u);
      const uint32_t word = found ? (sel | (flags << 1) | ((fs & keep) << 8)) : 1u;
      if (lane == 0) cls[im.base + k] = word;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ histogram
__global__ __launch_bounds__(256) void adapt_histogram_kernel(
    const ImgDesc* __restrict__ descs, int keep_hidden, const int32_t* __restrict__ block_base,
    int total_blocks, const uint32_t* __restrict__ cls, uint32_t* __restrict__ partials) {
  __shared__ uint32_t hist[kBins];
  __shared__ uint32_t tile[4][kPix];        // per wave: R | G << 8 | B << 16 | visible << 24
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < kBins; i += 256) hist[i] = 0;
  __syncthreads();
  Image im;
  if (image_of(descs, block_base, b, total_blocks, im)) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* tw = tile[wave];
    // the four waves step together so that the barriers around the tile are workgroup-uniform
    for (int k0 = blockIdx.x * 4; k0 < im.nblk; k0 += gridDim.x * 4) {
      const int k = k0 + wave;
      const uint32_t cw = k < im.nblk ? cls[im.base + k] : 1u;
      const bool work = word_ok(cw) && has_any_chunk(cw);  // wave-uniform
      if (work) {
        const Block bl = block_of(im, k);
#pragma unroll
        for (int q = 0; q < kPix / 64; ++q)
          tw[lane + 64 * q] = tile_pixel(im, bl, lane + 64 * q, keep_hidden);
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
          const uint32_t sv = chosen(v, cw), sL = chosen(L, cw), sU = chosen(U, cw),
                         sD = chosen(D, cw);
#pragma unroll
          for (int s = 0; s < kSlots; ++s) {
            if (!has_chunk(cw, s)) continue;
            const int sh = 8 * s;
            int pred, ctx;
            vis_model(L >> 24, U >> 24, D >> 24, (sL >> sh) & 255, (sU >> sh) & 255,
                      (sD >> sh) & 255, pred, ctx);
            const int sym = ((int)((sv >> sh) & 255) - pred) & 255;
            atomicAdd(&hist[(kind_of(cw, s) * kCtx + ctx) * 256 + sym], 1u);
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

// grid: (25 tables, images); thread t owns symbol t.  The rule is alpha_exact.hip's.
__global__ __launch_bounds__(256) void adapt_normalise_kernel(
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
  uint8_t planes[kSlots][kLanes * kPix];                    // 48 KiB, swz layout
  uint16_t vmask[kEdge * kLanes];                           // row r of block j at r * 64 + j
  __attribute__((aligned(4))) uint16_t tab[kTabU16];
  uint32_t cls[kLanes];
  int32_t fill[kSlots][kLanes];                             // decode: >= 0 a constant slot
  uint32_t bad[kLanes];                                     // decode: the block decodes to RGB 0
};
static_assert(sizeof(Shared) == 65332, "the LDS arithmetic of the file header");
static_assert(sizeof(Shared) <= 64 * 1024, "static LDS of one workgroup");

// One wave stages block k of the image as block j of the group: every lane loads 4 pixels as
// dwords; kPlanes: the bytes of the three slots, as class word cw chooses them, go to the
// planes; always: the visibility of the 64 pixels of a quarter is one ballot, whose four 16-bit
// rows lanes 0..3 store.
template <bool kPlanes>
__device__ inline void stage_block(const Image& im, int k, int keep_hidden, int j, int lane,
                                   uint32_t cw, Shared& sh) {
  const Block bl = block_of(im, k);
#pragma unroll
  for (int q = 0; q < kPix / 64; ++q) {
    const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
    const bool in = r < bl.bh && c < bl.bw;
    const uint32_t p = in ? *pixel_at(im, bl, r, c) : 0u;
    if (kPlanes) {
      const uint32_t t = chosen(p, cw);
      const int a = swz(j, pos);
      sh.planes[0][a] = (uint8_t)t;
      sh.planes[1][a] = (uint8_t)(t >> 8);
      sh.planes[2][a] = (uint8_t)(t >> 16);
    }
    const unsigned long long b = __ballot(in && (keep_hidden || (p >> 24)));
    if (lane < 4) sh.vmask[(4 * q + lane) * kLanes + j] = (uint16_t)(b >> (16 * lane));
  }
}

// ------------------------------------------------------------------ sizes / encode
template <bool kStore>
__global__ __launch_bounds__(kThreads) void adapt_code_kernel(
    int batch, const ImgDesc* __restrict__ descs, int keep_hidden,
    const Group* __restrict__ groups, const int32_t* __restrict__ block_base, int total_blocks,
    const uint32_t* __restrict__ cls, const uint16_t* __restrict__ tables,
    int32_t* __restrict__ counts, const int64_t* __restrict__ ends,
    uint32_t* __restrict__ payload, int64_t payload_words, int32_t* err) {
  __shared__ Shared sh;
  const Group g = groups[blockIdx.x];
  Image im;
  if (g.image < 0 || g.image >= batch || g.block0 < 0 ||
      !image_of(descs, block_base, g.image, total_blocks, im)) {
    if (threadIdx.x == 0) report(err, rr::kErrChunk);
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nb = min(kLanes, im.nblk - g.block0);           // <= 0: a group past the image
  if ((int)threadIdx.x < nb) sh.cls[threadIdx.x] = cls[im.base + g.block0 + threadIdx.x];
  stage_table(tables, g.image, sh.tab);
  __syncthreads();
  for (int j = wave; j < nb; j += kSlots) {
    const uint32_t cw = sh.cls[j];
    if (word_ok(cw) && has_any_chunk(cw))
      stage_block<true>(im, g.block0 + j, keep_hidden, j, lane, cw, sh);
  }
  __syncthreads();
  // from here on: wave = slot, lane = block
  if (lane >= nb) return;
  const uint32_t cw = sh.cls[lane];
  const int64_t ci = (int64_t)(im.base + g.block0 + lane) * kSlots + wave;
  if (!word_ok(cw) || !has_chunk(cw, wave)) {
    if (!kStore) counts[ci] = 0;
    if (!word_ok(cw)) report(err, rr::kErrCorrupt);         // not a word choose writes
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
  const int tb0 = kind_of(cw, wave) * kCtx;
  rr::detail::EncState s = {rr::kL, end, cap, 0};
  for (int r = kEdge - 1; r >= 0; --r) {
    const uint32_t m = sh.vmask[r * kLanes + lane];
    const uint32_t mp = r ? sh.vmask[(r - 1) * kLanes + lane] : 0u;
    uint32_t rest = m;
    while (rest) {
      const int c = 31 - __clz((int)rest);
      rest &= ~(1u << c);
      int pred, ctx;
      plane_model(pln, lane, r, c, m, mp, pred, ctx);
      const int sym = ((int)pln[swz(lane, r * kEdge + c)] - pred) & 255;
      uint32_t start, freq;
      table_entry(sh.tab, tb0 + ctx, sym, start, freq);
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
__global__ __launch_bounds__(kThreads) void adapt_decode_kernel(
    int batch, const ImgDesc* __restrict__ descs, int keep_hidden,
    const Group* __restrict__ groups, const int32_t* __restrict__ block_base, int total_blocks,
    const uint32_t* __restrict__ cls, const uint16_t* __restrict__ tables,
    const int64_t* __restrict__ word_off, const int32_t* __restrict__ counts,
    const uint32_t* __restrict__ payload, int64_t payload_words, int32_t* err) {
  __shared__ Shared sh;
  const Group g = groups[blockIdx.x];
  Image im;
  if (g.image < 0 || g.image >= batch || g.block0 < 0 ||
      !image_of(descs, block_base, g.image, total_blocks, im)) {
    if (threadIdx.x == 0) report(err, rr::kErrChunk);
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nb = min(kLanes, im.nblk - g.block0);
  if ((int)threadIdx.x < nb) sh.cls[threadIdx.x] = cls[im.base + g.block0 + threadIdx.x];
  if (threadIdx.x < kLanes) sh.bad[threadIdx.x] = 0;
  stage_table(tables, g.image, sh.tab);
  // who is visible: the alpha bytes already lie in the destination
  for (int j = wave; j < nb; j += kSlots)
    stage_block<false>(im, g.block0 + j, keep_hidden, j, lane, 0u, sh);
  __syncthreads();
  if (lane < nb) {                                          // wave = slot, lane = block
    const uint32_t cw = sh.cls[lane];
    int n = 0;
    for (int r = 0; r < kEdge; ++r) n += __popc(sh.vmask[r * kLanes + lane]);
    int32_t e = rr::kErrNone;
    int32_t value = -1;
    if (!word_ok(cw)) {
      e = rr::kErrCorrupt;                                  // the block is left as it is
    } else if (((cw & 1u) != 0) != (n == 0)) {
      e = rr::kErrCorrupt;                                  // the class word is another mask's
    } else if (!has_chunk(cw, wave)) {
      value = (cw >> (8 + 8 * wave)) & 255;                 // (a hidden block writes no colour)
    } else {
      const int64_t ci = (int64_t)(im.base + g.block0 + lane) * kSlots + wave;
      const int64_t off = word_off[ci];
      const int32_t cnt = counts[ci];
      if (n < 2 || cnt < 2 || cnt > n / 2 + 3) {
        e = rr::kErrCorrupt;                                // an impossible count
      } else if (off < 0 || off > payload_words - cnt) {
        e = rr::kErrChunk;
      } else {
        uint8_t* pln = sh.planes[wave];
        const int tb0 = kind_of(cw, wave) * kCtx;
        rr::detail::DecState d = {0, payload + off, cnt, 0, rr::kErrNone};
        const uint32_t lo = rr::detail::dec_word(d), hi = rr::detail::dec_word(d);
        d.x = (uint64_t)lo | ((uint64_t)hi << 32);
        for (int r = 0; r < kEdge && !d.err; ++r) {
          const uint32_t m = sh.vmask[r * kLanes + lane];
          const uint32_t mp = r ? sh.vmask[(r - 1) * kLanes + lane] : 0u;
          uint32_t rest = m;
          while (rest) {
            const int c = __ffs((int)rest) - 1;
            rest &= rest - 1;
            int pred, ctx;
            plane_model(pln, lane, r, c, m, mp, pred, ctx);
            const int tb = tb0 + ctx;
            const int last = (int16_t)sh.tab[kBins + tb];
            if (last < 0) {                                 // a symbol in an empty context
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
            if (freq == 0 || cum - start >= freq) {         // not a table (the parser's job)
              d.err = rr::kErrCorrupt;
              break;
            }
            uint64_t x = d.x;
            x = freq * (x >> rr::kPrecision) + cum - start;
            if (x < rr::kL) x = (x << 32) | rr::detail::dec_word(d);
            d.x = x;
            pln[swz(lane, r * kEdge + c)] = (uint8_t)((pred + slo) & 255);
          }
        }
        // a sound chunk ends where the encoder began: every word read, the state back at kL
        if (!d.err && (d.x != rr::kL || d.pos != d.nwords)) d.err = rr::kErrCorrupt;
        e = d.err;
      }
    }
    sh.fill[wave][lane] = value;
    if (e) sh.bad[lane] = 1;                                // a bad block decodes to RGB 0
    report(err, e);
  }
  __syncthreads();
  for (int j = wave; j < nb; j += kSlots) {
    const uint32_t cw = sh.cls[j];
    if (!word_ok(cw)) continue;                             // nothing of this block is touched
    const Block bl = block_of(im, g.block0 + j);
    const bool zero = sh.bad[j] || (cw & 1u);
    const int32_t f0 = sh.fill[0][j], f1 = sh.fill[1][j], f2 = sh.fill[2][j];
#pragma unroll
    for (int q = 0; q < kPix / 64; ++q) {
      const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
      if (r >= bl.bh || c >= bl.bw) continue;
      uint32_t* dst = pixel_at(im, bl, r, c);
      const uint32_t a = *dst & 0xFF000000u;
      uint32_t rgb = 0;
      if (!zero && ((sh.vmask[r * kLanes + j] >> c) & 1u)) {
        const int at = swz(j, pos);
        rgb = unchosen(f0 >= 0 ? (uint32_t)f0 : sh.planes[0][at],
                       f1 >= 0 ? (uint32_t)f1 : sh.planes[1][at],
                       f2 >= 0 ? (uint32_t)f2 : sh.planes[2][at], cw);
      }
      *dst = a | rgb;
    }
  }
}

}  // namespace

#define ADAPT_REQUIRE_COMMON()                                                              \
  RGBAC_REQUIRE(batch > 0 && batch <= 65535, "batch must be in [1, 65535]");                \
  RGBAC_REQUIRE(descs && block_base, "null pointer");                                       \
  RGBAC_REQUIRE(keep_hidden == 0 || keep_hidden == 1, "keep_hidden must be 0 or 1");        \
  RGBAC_REQUIRE(total_blocks > 0 && total_blocks <= INT32_MAX / 4,                          \
                "total_blocks must be in [1, 2^29)")
#define ADAPT_REQUIRE_GROUPS() \
  RGBAC_REQUIRE(groups && ngroups > 0, "group table")

extern "C" int rgbac_color_adapt_choose(int batch, const rgbac_image_desc* descs,
                                        int keep_hidden, int ngroups,
                                        const rgbac_alpha_group* groups,
                                        const int32_t* block_base, int total_blocks,
                                        uint32_t* cls, void* stream) {
  ADAPT_REQUIRE_COMMON();
  ADAPT_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls, "null pointer");
  hipLaunchKernelGGL(adapt_choose_kernel, dim3(ngroups), dim3(256), 0, (hipStream_t)stream,
                     batch, descs, keep_hidden, groups, block_base, total_blocks, cls);
  return rgbac::check_launch("rgbac_color_adapt_choose");
}

extern "C" int rgbac_color_adapt_tables(int batch, const rgbac_image_desc* descs,
                                        int keep_hidden, const int32_t* block_base,
                                        int total_blocks, const uint32_t* cls,
                                        uint32_t* partials, int32_t* freqs, uint16_t* tables,
                                        void* stream) {
  ADAPT_REQUIRE_COMMON();
  RGBAC_REQUIRE(cls && partials && freqs && tables, "null pointer");
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned");
  hipLaunchKernelGGL(adapt_histogram_kernel, dim3(kHistBlocks, batch), dim3(256), 0,
                     (hipStream_t)stream, descs, keep_hidden, block_base, total_blocks, cls,
                     partials);
  const int rc = rgbac::check_launch("rgbac_color_adapt_tables (histogram)");
  if (rc) return rc;
  hipLaunchKernelGGL(adapt_normalise_kernel, dim3(kTabs, batch), dim3(256), 0,
                     (hipStream_t)stream, partials, kHistBlocks, freqs, tables);
  return rgbac::check_launch("rgbac_color_adapt_tables (normalise)");
}

extern "C" int rgbac_color_adapt_sizes(int batch, const rgbac_image_desc* descs, int keep_hidden,
                                       int ngroups, const rgbac_alpha_group* groups,
                                       const int32_t* block_base, int total_blocks,
                                       const uint32_t* cls, const uint16_t* tables,
                                       int32_t* counts, int32_t* err, void* stream) {
  ADAPT_REQUIRE_COMMON();
  ADAPT_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls && tables && counts && err, "null pointer");
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned");
  hipLaunchKernelGGL(adapt_code_kernel<false>, dim3(ngroups), dim3(kThreads), 0,
                     (hipStream_t)stream, batch, descs, keep_hidden, groups, block_base,
                     total_blocks, cls, tables, counts, (const int64_t*)nullptr,
                     (uint32_t*)nullptr, (int64_t)0, err);
  return rgbac::check_launch("rgbac_color_adapt_sizes");
}

extern "C" int rgbac_color_adapt_encode(int batch, const rgbac_image_desc* descs,
                                        int keep_hidden, int ngroups,
                                        const rgbac_alpha_group* groups,
                                        const int32_t* block_base, int total_blocks,
                                        const uint32_t* cls, const uint16_t* tables,
                                        const int32_t* counts, const int64_t* ends,
                                        uint32_t* payload, int64_t payload_words, int32_t* err,
                                        void* stream) {
  ADAPT_REQUIRE_COMMON();
  ADAPT_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls && tables && counts && ends && payload && err, "null pointer");
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned");
  RGBAC_REQUIRE(payload_words >= 2, "payload smaller than one chunk's state words");
  hipLaunchKernelGGL(adapt_code_kernel<true>, dim3(ngroups), dim3(kThreads), 0,
                     (hipStream_t)stream, batch, descs, keep_hidden, groups, block_base,
                     total_blocks, cls, tables, const_cast<int32_t*>(counts), ends, payload,
                     payload_words, err);
  return rgbac::check_launch("rgbac_color_adapt_encode");
}

extern "C" int rgbac_color_adapt_decode(int batch, const rgbac_image_desc* descs,
                                        int keep_hidden, int ngroups,
                                        const rgbac_alpha_group* groups,
                                        const int32_t* block_base, int total_blocks,
                                        const uint32_t* cls, const uint16_t* tables,
                                        const int64_t* word_off, const int32_t* counts,
                                        const uint32_t* payload, int64_t payload_words,
                                        int32_t* err, void* stream) {
  ADAPT_REQUIRE_COMMON();
  ADAPT_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls && tables && word_off && counts && payload && err, "null pointer");
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned");
  RGBAC_REQUIRE(payload_words >= 0, "payload_words must not be negative");
  hipLaunchKernelGGL(adapt_decode_kernel, dim3(ngroups), dim3(kThreads), 0, (hipStream_t)stream,
                     batch, descs, keep_hidden, groups, block_base, total_blocks, cls, tables,
                     word_off, counts, payload, payload_words, err);
  return rgbac::check_launch("rgbac_color_adapt_decode");
}
