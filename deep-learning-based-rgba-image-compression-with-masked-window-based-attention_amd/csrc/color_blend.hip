// Composite-bounded near-lossless colour of packed RGBA: csrc/color_near.hip's coder with a
// tolerance that follows the pixel's alpha (rgbac/rgbanear.py).  A colour
// error dC of a pixel of alpha a shows in the composite over any background as a |dC| / 255, so
// with delta = max_error the pixel may be off by
//     e(a) = min(255, (255 delta) div a),   a in 1..255   (e(255) = delta),
// and its quantiser is step = 2 e(a) + 1, Q_a(x) = sgn(x) * ((|x| + e(a)) div step).
//
// Blocks, groups, visibility, neighbours, the prediction over reconstructed plane values, the
// contexts, the 15 tables, the class word layout and the chunk rule are color_near.hip's.  What
// differs:
//   * q = Q_a(C - P), C^ = clamp(P + q * step, 0, 255) with the step of the pixel's own alpha.
//     The alpha plane is exact and decoded first, so both sides know e at every pixel;
//   * a channel is constant in a block iff lo = max(C_i - e_i) <= hi = min(C_i + e_i) over the
//     block's visible pixels, at clamp((lo + hi) >> 1, 0, 255).
// Q_a(C^ - P) = q still holds, so only the settle kernel runs the closed loop.
//
// Per-image mode word (modes[image]): bits 0-7 delta in 1..16, bit 8 keep_hidden, bit 9
// (RGBAC_BLEND_COMPOSITE) the composite bound.  Bits 8 and 9 together mean nothing: code 5.
//
// The tolerance table.  A group belongs to one image, so every workgroup builds, before its first
// barrier, one 256-entry LDS table alpha -> e | ceil(2^18 / step) << 8 from its image's mode
// word.  n div step = (n * ceil(2^18 / step)) >> 18 is exact for every n <= 255 + e and every
// step that occurs (2^16 is not).  With bit 9 clear the table is flat (e = delta) and every
// kernel here produces what color_near.hip produces.  Every quantise and dequantise is one LDS
// dword and a multiply; the table itself is built from a float reciprocal and an integer
// correction, so the device never divides integers.
//
// Kernels (one launch each for the whole batch):
//   settle     classify and the closed loop, as a REGISTER wavefront.  Staging is
//              color_near.hip's: 16 lanes per block, lane x loads column x row by row into a
//              256-dword LDS tile and reduces max(C - e) and min(C + e) of the three channels;
//              four xor shuffles give the class word.  Then lane r owns pixel (r, s - r) at step
//              s = 0..30.  Its L is what it settled itself at step s - 1, its U is what lane
//              r - 1 settled at step s - 1 (one 16-lane shuffle), its D is the U of the step
//              before.  So a step reads one tile dword (the lane's own pixel, stride 15: no bank
//              conflict), one table dword, and no barrier separates the 31 steps: the tile only
//              transposes columns to rows and back.  No scratch, no atomics.
//   histogram, normalise   color_near.hip's over the settled image; the tile keeps the alpha
//              byte, the symbol is Q_a(C^ - P).
//   sizes, encode   wave = channel, lane = block, rows from the last to the first.  The LDS has
//              no room for a fourth plane, so under the composite bound a lane carries the 16
//              alpha bytes of its row in four registers, loaded from the settled image one row
//              ahead of their use.
//   decode     color_near.hip's order (green leads by one row, register carry).  Staging writes
//              every pixel's alpha into the byte of each plane that the decoded value will
//              replace: a lane reads its pixel's alpha from its own plane just before it stores
//              there.  A symbol with |q| > (255 + e) div (2 e + 1) at its pixel is corrupt.
//
// LDS of the coding kernels: color_near.hip's struct plus the table: 61,216 bytes.
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
constexpr int kInvBits = 18;                        // the reciprocal's fixed point
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
struct Mode {
  int delta;
  bool keep, blend;
};

__device__ inline bool mode_of(const int32_t* modes, int b, Mode& m) {
  const int w = modes[b];
  m.delta = w & 255;
  m.keep = (w & RGBAC_NEAR_KEEP_HIDDEN) != 0;
  m.blend = (w & RGBAC_BLEND_COMPOSITE) != 0;
  return !(w & ~(255 | RGBAC_NEAR_KEEP_HIDDEN | RGBAC_BLEND_COMPOSITE)) && !(m.keep && m.blend) &&
         m.delta >= 1 && m.delta <= kMaxDelta;
}

// floor(n / d) for 0 <= n < 2^19, 1 <= d <= 511: a float estimate (off by one at the most, next
// to a multiple of d) and an integer correction
__device__ inline int small_div(int n, int d) {
  int q = (int)((float)n * __builtin_amdgcn_rcpf((float)d));
  q += (q + 1) * d <= n;
  q -= q * d > n;
  return q;
}

// the table entry of alpha a: e | ceil(2^18 / (2 e + 1)) << 8.  Alpha 0 is hidden under the
// composite bound: its entry is the limit, e = 255, and is never used.
__device__ inline uint32_t tol_entry(int a, const Mode& m) {
  int e = m.delta;
  if (m.blend) e = a ? min(255, small_div(255 * m.delta, a)) : 255;
  const int step = 2 * e + 1;
  return (uint32_t)e | ((uint32_t)small_div((1 << kInvBits) + step - 1, step) << 8);
}

__device__ inline void build_tol(uint32_t* tol, const Mode& m) {
  for (int a = threadIdx.x; a < 256; a += blockDim.x) tol[a] = tol_entry(a, m);
}

__device__ inline int tol_e(uint32_t tw) { return (int)(tw & 255u); }
__device__ inline int tol_step(uint32_t tw) { return 2 * (int)(tw & 255u) + 1; }

// Q_a(x) with a's table entry tw
__device__ inline int quantise(int x, uint32_t tw) {
  const int n = (int)(((uint32_t)(abs(x) + tol_e(tw)) * (tw >> 8)) >> kInvBits);
  return x < 0 ? -n : n;
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
__global__ __launch_bounds__(256) void blend_settle_kernel(
    int batch, const ImgDesc* __restrict__ src, const ImgDesc* __restrict__ dst,
    const int32_t* __restrict__ modes, const Group* __restrict__ groups,
    const int32_t* __restrict__ block_base, int total_blocks, uint32_t* __restrict__ cls,
    int32_t* err) {
  __shared__ uint32_t tiles[4][4][kSlot];
  __shared__ uint32_t tol[256];
  const Group g = groups[blockIdx.x];
  Image im, om;
  Mode mo;
  if (g.image < 0 || g.image >= batch || g.block0 < 0 ||
      !image_of(src, block_base, g.image, total_blocks, im) ||
      !image_of(dst, block_base, g.image, total_blocks, om) || om.h != im.h || om.w != im.w ||
      !mode_of(modes, g.image, mo)) {
    if (threadIdx.x == 0) report(err, rr::kErrChunk);
    return;
  }
  build_tol(tol, mo);
  __syncthreads();
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
    // lo: max(C - e), hi: min(C + e) over the lane's visible pixels
    int lo[kCh] = {-512, -512, -512}, hi[kCh] = {512, 512, 512}, any = 0;
#pragma unroll
    for (int y = 0; y < kEdge; ++y) {
      const bool in = y < bl.bh && x < bl.bw;
      const uint32_t p = in ? *pixel_at(im, bl, y, x) : 0u;
      const bool v = in && (mo.keep || (p >> 24));
      t[y * kEdge + x] = v ? p : 0u;           // hidden: alpha 0 already, RGB 0 from here on
      if (v) {
        any = 1;
        const int e = tol_e(tol[p >> 24]);
#pragma unroll
        for (int ch = 0; ch < kCh; ++ch) {
          lo[ch] = max(lo[ch], colour_of(p, ch) - e);
          hi[ch] = min(hi[ch], colour_of(p, ch) + e);
        }
      }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {          // stays inside the block's 16 lanes
      any |= __shfl_xor(any, o);
#pragma unroll
      for (int ch = 0; ch < kCh; ++ch) {
        lo[ch] = max(lo[ch], __shfl_xor(lo[ch], o));
        hi[ch] = min(hi[ch], __shfl_xor(hi[ch], o));
      }
    }
    uint32_t word = 1u;
    if (any) {
      word = 0u;
#pragma unroll
      for (int ch = 0; ch < kCh; ++ch)
        if (lo[ch] <= hi[ch])
          word |= (2u << ch) | ((uint32_t)clamp255((lo[ch] + hi[ch]) >> 1) << (8 + 8 * ch));
    }
    if (have && x == 0) cls[im.base + k] = word;
    __syncthreads();
    // the wavefront: lane x is row x.  me: what the lane settled at the step before (0: nothing
    // visible there), up: its U of the step before.  Every lane takes part in the shuffle.
    uint32_t me = 0u, up = 0u;
    for (int s = 0; s < 2 * kEdge - 1; ++s) {
      const uint32_t above = __shfl_up(me, 1, 16);
      const uint32_t L = me, U = x ? above : 0u, D = up;
      const int c = s - x;
      uint32_t now = 0u;
      if (any && c >= 0 && c < bl.bw && x < bl.bh) {
        const int pos = x * kEdge + c;
        const uint32_t p = t[pos];
        if (mo.keep || (p >> 24)) {
          const uint32_t tw = tol[p >> 24];
          const bool eL = c && (mo.keep || (L >> 24)), eU = x && (mo.keep || (U >> 24));
          const bool eD = x && c && (mo.keep || (D >> 24));
          int out[kCh] = {0, 0, 0};
#pragma unroll
          for (int ch = 0; ch < kCh; ++ch) {
            if ((word >> (1 + ch)) & 1u) {
              out[ch] = (word >> (8 + 8 * ch)) & 255;   // a constant channel: its value
            } else {
              int P, ctx;
              pixel_model(ch, out[0], eL, eU, eD, L, U, D, P, ctx);
              out[ch] = clamp255(P + quantise(colour_of(p, ch) - P, tw) * tol_step(tw));
            }
          }
          now = (p & 0xFF000000u) | (uint32_t)out[1] | ((uint32_t)out[0] << 8) |
                ((uint32_t)out[2] << 16);
          t[pos] = now;
        }
      }
      up = U;
      me = now;
    }
    __syncthreads();
#pragma unroll
    for (int y = 0; y < kEdge; ++y)
      if (y < ob.bh && x < ob.bw) *pixel_at(om, ob, y, x) = t[y * kEdge + x];
    __syncthreads();
  }
}

// ------------------------------------------------------------------ histogram
// descs: the settled images
__global__ __launch_bounds__(256) void blend_histogram_kernel(
    const ImgDesc* __restrict__ descs, const int32_t* __restrict__ modes,
    const int32_t* __restrict__ block_base, int total_blocks, const uint32_t* __restrict__ cls,
    uint32_t* __restrict__ partials) {
  __shared__ uint32_t hist[kBins];
  __shared__ uint32_t tile[4][kPix];        // per wave: the settled dwords, 0 outside the image
  __shared__ uint32_t tol[256];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < kBins; i += 256) hist[i] = 0;
  Image im;
  Mode mo;
  const bool ok = image_of(descs, block_base, b, total_blocks, im) && mode_of(modes, b, mo);
  if (ok) build_tol(tol, mo);
  __syncthreads();
  if (ok) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* tw = tile[wave];
    // the four waves step together so that the barriers around the tile are workgroup-uniform
    for (int k0 = blockIdx.x * 4; k0 < im.nblk; k0 += gridDim.x * 4) {
      const int k = k0 + wave;
      const uint32_t cw = k < im.nblk ? cls[im.base + k] : 1u;
      const bool work = has_any_chunk(cw);                // wave-uniform
      Block bl = {nullptr, 0, 0};
      if (work) {
        bl = block_of(im, k);
#pragma unroll
        for (int q = 0; q < kPix / 64; ++q) {
          const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
          tw[pos] = r < bl.bh && c < bl.bw ? *pixel_at(im, bl, r, c) : 0u;
        }
      }
      __syncthreads();
      if (work) {
#pragma unroll
        for (int q = 0; q < kPix / 64; ++q) {
          const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
          const uint32_t v = tw[pos];
          // a neighbour inside the block's 16 x 16 is inside the image when the pixel is
          if (r >= bl.bh || c >= bl.bw || !(mo.keep || (v >> 24))) continue;
          const uint32_t L = c ? tw[pos - 1] : 0u, U = r ? tw[pos - kEdge] : 0u;
          const uint32_t D = (r && c) ? tw[pos - kEdge - 1] : 0u;
          const bool eL = c && (mo.keep || (L >> 24)), eU = r && (mo.keep || (U >> 24));
          const bool eD = r && c && (mo.keep || (D >> 24));
          const uint32_t te = tol[v >> 24];
#pragma unroll
          for (int ch = 0; ch < kCh; ++ch) {
            if (!has_chunk(cw, ch)) continue;
            int P, ctx;
            pixel_model(ch, colour_of(v, 0), eL, eU, eD, L, U, D, P, ctx);
            const int sym = quantise(colour_of(v, ch) - P, te) & 255;
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
__global__ __launch_bounds__(256) void blend_normalise_kernel(
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
  uint32_t tol[256];                                        // alpha -> e | reciprocal << 8
  uint32_t cls[kLanes];
  int32_t fill[kCh][kLanes];                                // decode: >= 0 a constant channel
  uint32_t bad[kLanes];                                     // decode: the block decodes to RGB 0
};
static_assert(sizeof(Shared) <= 64 * 1024, "static LDS of one workgroup");

// what stage_block puts into the three planes
enum Planes { kNone, kColour, kAlpha };

// One wave stages block k of the image as block j of the group: every lane loads 4 pixels as
// dwords.  kColour: the three colour bytes go to the planes; kAlpha: the alpha byte goes to all
// three; always: the visibility of the 64 pixels of a quarter is one ballot, whose four 16-bit
// rows lanes 0..3 store.
template <Planes kFill>
__device__ inline void stage_block(const Image& im, int k, bool keep_hidden, int j, int lane,
                                   Shared& sh) {
  const Block bl = block_of(im, k);
#pragma unroll
  for (int q = 0; q < kPix / 64; ++q) {
    const int pos = lane + 64 * q, r = pos >> 4, c = pos & 15;
    const bool in = r < bl.bh && c < bl.bw;
    const uint32_t p = in ? *pixel_at(im, bl, r, c) : 0u;
    if (kFill != kNone) {
      const int a = swz(j, pos);
      sh.planes[0][a] = (uint8_t)(kFill == kAlpha ? p >> 24 : p >> 8);
      sh.planes[1][a] = (uint8_t)(kFill == kAlpha ? p >> 24 : p);
      sh.planes[2][a] = (uint8_t)(kFill == kAlpha ? p >> 24 : p >> 16);
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

// The alpha bytes of columns c0 .. c0 + 7 of row r of a block, byte i for column c0 + i: half a
// row in one register pair.  Only the columns that row mask m marks are read (a marked pixel lies
// inside the image); nothing for r < 0.
__device__ inline uint64_t alpha_half(const Image& im, const Block& bl, int r, uint32_t m,
                                      int c0) {
  uint64_t w = 0;
  if (r < 0) return w;
  const uint8_t* row = bl.p + (long long)r * im.rs + 3;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if ((m >> (c0 + i)) & 1u) w |= (uint64_t)row[(c0 + i) * 4] << (8 * i);
  return w;
}

// column c of the row whose halves are lo and hi
__device__ inline int alpha_at(uint64_t lo, uint64_t hi, int c) {
  return (int)((((c & 8) ? hi : lo) >> (8 * (c & 7))) & 255u);
}

// ------------------------------------------------------------------ sizes / encode
// descs: the settled images
template <bool kStore>
__global__ __launch_bounds__(kThreads) void blend_code_kernel(
    int batch, const ImgDesc* __restrict__ descs, const int32_t* __restrict__ modes,
    const Group* __restrict__ groups, const int32_t* __restrict__ block_base, int total_blocks,
    const uint32_t* __restrict__ cls, const uint16_t* __restrict__ tables,
    int32_t* __restrict__ counts, const int64_t* __restrict__ ends,
    uint32_t* __restrict__ payload, int64_t payload_words, int32_t* err) {
  __shared__ Shared sh;
  const Group g = groups[blockIdx.x];
  Image im;
  Mode mo;
  if (g.image < 0 || g.image >= batch || g.block0 < 0 ||
      !image_of(descs, block_base, g.image, total_blocks, im) || !mode_of(modes, g.image, mo)) {
    if (threadIdx.x == 0) report(err, rr::kErrChunk);
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nb = min(kLanes, im.nblk - g.block0);           // <= 0: a group past the image
  if ((int)threadIdx.x < nb) sh.cls[threadIdx.x] = cls[im.base + g.block0 + threadIdx.x];
  stage_table(tables, g.image, sh.tab);
  build_tol(sh.tol, mo);
  __syncthreads();
  for (int j = wave; j < nb; j += kCh)
    if (has_any_chunk(sh.cls[j])) stage_block<kColour>(im, g.block0 + j, mo.keep, j, lane, sh);
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
  const Block bl = block_of(im, g.block0 + lane);
  const uint32_t flat = sh.tol[255];                        // every entry, without the bound
  // the row's alpha bytes travel one row ahead of their use (a flat table needs none)
  uint64_t alo = 0, ahi = 0;
  if (mo.blend) {
    const uint32_t m15 = sh.vmask[(kEdge - 1) * kLanes + lane];
    alo = alpha_half(im, bl, kEdge - 1, m15, 0);
    ahi = alpha_half(im, bl, kEdge - 1, m15, 8);
  }
  rr::detail::EncState s = {rr::kL, end, cap, 0};
  for (int r = kEdge - 1; r >= 0; --r) {
    const uint32_t m = sh.vmask[r * kLanes + lane];
    const uint32_t mp = r ? sh.vmask[(r - 1) * kLanes + lane] : 0u;
    uint64_t nlo = 0, nhi = 0;
    if (mo.blend) {
      nlo = alpha_half(im, bl, r - 1, mp, 0);
      nhi = alpha_half(im, bl, r - 1, mp, 8);
    }
    uint32_t rest = m;
    while (rest) {
      const int c = 31 - __clz((int)rest);
      rest &= ~(1u << c);
      int P, ctx;
      planes_model(sh, wave, lane, r, c, m, mp, P, ctx);
      const uint32_t tw = mo.blend ? sh.tol[alpha_at(alo, ahi, c)] : flat;
      const int sym = quantise((int)pln[swz(lane, r * kEdge + c)] - P, tw) & 255;
      uint32_t start, freq;
      table_entry(sh.tab, wave * kCtx + ctx, sym, start, freq);
      if (freq == 0 || freq > 65535u) {                     // not this image's table
        e = rr::kErrCorrupt;
        continue;
      }
      rr::detail::enc_put(s, start, freq);
    }
    alo = nlo;
    ahi = nhi;
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
__global__ __launch_bounds__(kThreads) void blend_decode_kernel(
    int batch, const ImgDesc* __restrict__ descs, const int32_t* __restrict__ modes,
    const Group* __restrict__ groups, const int32_t* __restrict__ block_base, int total_blocks,
    const uint32_t* __restrict__ cls, const uint16_t* __restrict__ tables,
    const int64_t* __restrict__ word_off, const int32_t* __restrict__ counts,
    const uint32_t* __restrict__ payload, int64_t payload_words, int32_t* err) {
  __shared__ Shared sh;
  const Group g = groups[blockIdx.x];
  Image im;
  Mode mo;
  if (g.image < 0 || g.image >= batch || g.block0 < 0 ||
      !image_of(descs, block_base, g.image, total_blocks, im) || !mode_of(modes, g.image, mo)) {
    if (threadIdx.x == 0) report(err, rr::kErrChunk);
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nb = min(kLanes, im.nblk - g.block0);
  if ((int)threadIdx.x < nb) sh.cls[threadIdx.x] = cls[im.base + g.block0 + threadIdx.x];
  if (threadIdx.x < kLanes) sh.bad[threadIdx.x] = 0;
  stage_table(tables, g.image, sh.tab);
  build_tol(sh.tol, mo);
  // who is visible, and under the composite bound how much: the alpha bytes already lie in the
  // destination
  for (int j = wave; j < nb; j += kCh) {
    if (mo.blend)
      stage_block<kAlpha>(im, g.block0 + j, false, j, lane, sh);
    else
      stage_block<kNone>(im, g.block0 + j, mo.keep, j, lane, sh);
  }
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
  const uint32_t flat = sh.tol[255];
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
        const int at = swz(lane, pos);
        // the byte about to be replaced still holds the pixel's alpha
        const uint32_t tw = mo.blend ? sh.tol[pln[at]] : flat;
        const int u = eU ? pln[swz(lane, pos - kEdge)] : 0;
        int L = eL ? pv : 0, U = u;
        int D = eD ? (eL ? pu : pln[swz(lane, pos - kEdge - 1)]) : 0;
        int gc = 0, gu = 0;
        if (wave) {
          gc = gfix >= 0 ? gfix : gpl[at];
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
        const int qmax = (int)(((uint32_t)(255 + tol_e(tw)) * (tw >> 8)) >> kInvBits);
        if (freq == 0 || cum - start >= freq || abs(q) > qmax) {      // no table / no such error
          d.err = rr::kErrCorrupt;
          break;
        }
        uint64_t x = d.x;
        x = freq * (x >> rr::kPrecision) + cum - start;
        if (x < rr::kL) x = (x << 32) | rr::detail::dec_word(d);
        d.x = x;
        pv = clamp255(P + q * tol_step(tw));
        pu = u;
        pg = gc;
        pgu = gu;
        pln[at] = (uint8_t)pv;
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

#define BLEND_REQUIRE_COMMON()                                                              \
  RGBAC_REQUIRE(batch > 0 && batch <= 65535, "batch must be in [1, 65535]");                \
  RGBAC_REQUIRE(descs && modes && block_base, "null pointer");                              \
  RGBAC_REQUIRE(total_blocks > 0 && total_blocks <= INT32_MAX / 4,                          \
                "total_blocks must be in [1, 2^29)")
#define BLEND_REQUIRE_GROUPS() \
  RGBAC_REQUIRE(groups && ngroups > 0, "group table")

extern "C" int rgbac_color_blend_settle(int batch, const rgbac_image_desc* descs,
                                        const rgbac_image_desc* settled, const int32_t* modes,
                                        int ngroups, const rgbac_alpha_group* groups,
                                        const int32_t* block_base, int total_blocks,
                                        uint32_t* cls, int32_t* err, void* stream) {
  BLEND_REQUIRE_COMMON();
  BLEND_REQUIRE_GROUPS();
  RGBAC_REQUIRE(settled && cls && err, "null pointer");
  hipLaunchKernelGGL(blend_settle_kernel, dim3(ngroups), dim3(256), 0, (hipStream_t)stream,
                     batch, descs, settled, modes, groups, block_base, total_blocks, cls, err);
  return rgbac::check_launch("rgbac_color_blend_settle");
}

extern "C" int rgbac_color_blend_tables(int batch, const rgbac_image_desc* descs,
                                        const int32_t* modes, const int32_t* block_base,
                                        int total_blocks, const uint32_t* cls, uint32_t* partials,
                                        int32_t* freqs, uint16_t* tables, void* stream) {
  BLEND_REQUIRE_COMMON();
  RGBAC_REQUIRE(cls && partials && freqs && tables, "null pointer");
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned");
  hipLaunchKernelGGL(blend_histogram_kernel, dim3(kHistBlocks, batch), dim3(256), 0,
                     (hipStream_t)stream, descs, modes, block_base, total_blocks, cls, partials);
  const int rc = rgbac::check_launch("rgbac_color_blend_tables (histogram)");
  if (rc) return rc;
  hipLaunchKernelGGL(blend_normalise_kernel, dim3(kTabs, batch), dim3(256), 0,
                     (hipStream_t)stream, partials, kHistBlocks, freqs, tables);
  return rgbac::check_launch("rgbac_color_blend_tables (normalise)");
}

extern "C" int rgbac_color_blend_sizes(int batch, const rgbac_image_desc* descs,
                                       const int32_t* modes, int ngroups,
                                       const rgbac_alpha_group* groups, const int32_t* block_base,
                                       int total_blocks, const uint32_t* cls,
                                       const uint16_t* tables, int32_t* counts, int32_t* err,
                                       void* stream) {
  BLEND_REQUIRE_COMMON();
  BLEND_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls && tables && counts && err, "null pointer");
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned");
  hipLaunchKernelGGL(blend_code_kernel<false>, dim3(ngroups), dim3(kThreads), 0,
                     (hipStream_t)stream, batch, descs, modes, groups, block_base, total_blocks,
                     cls, tables, counts, (const int64_t*)nullptr, (uint32_t*)nullptr,
                     (int64_t)0, err);
  return rgbac::check_launch("rgbac_color_blend_sizes");
}

extern "C" int rgbac_color_blend_encode(int batch, const rgbac_image_desc* descs,
                                        const int32_t* modes, int ngroups,
                                        const rgbac_alpha_group* groups,
                                        const int32_t* block_base, int total_blocks,
                                        const uint32_t* cls, const uint16_t* tables,
                                        const int32_t* counts, const int64_t* ends,
                                        uint32_t* payload, int64_t payload_words, int32_t* err,
                                        void* stream) {
  BLEND_REQUIRE_COMMON();
  BLEND_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls && tables && counts && ends && payload && err, "null pointer");
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned");
  RGBAC_REQUIRE(payload_words >= 2, "payload smaller than one chunk's state words");
  hipLaunchKernelGGL(blend_code_kernel<true>, dim3(ngroups), dim3(kThreads), 0,
                     (hipStream_t)stream, batch, descs, modes, groups, block_base, total_blocks,
                     cls, tables, const_cast<int32_t*>(counts), ends, payload, payload_words, err);
  return rgbac::check_launch("rgbac_color_blend_encode");
}

extern "C" int rgbac_color_blend_decode(int batch, const rgbac_image_desc* descs,
                                        const int32_t* modes, int ngroups,
                                        const rgbac_alpha_group* groups,
                                        const int32_t* block_base, int total_blocks,
                                        const uint32_t* cls, const uint16_t* tables,
                                        const int64_t* word_off, const int32_t* counts,
                                        const uint32_t* payload, int64_t payload_words,
                                        int32_t* err, void* stream) {
  BLEND_REQUIRE_COMMON();
  BLEND_REQUIRE_GROUPS();
  RGBAC_REQUIRE(cls && tables && word_off && counts && payload && err, "null pointer");
  RGBAC_REQUIRE(((uintptr_t)tables & 3) == 0, "tables must be 4-byte aligned");
  RGBAC_REQUIRE(payload_words >= 0, "payload_words must not be negative");
  hipLaunchKernelGGL(blend_decode_kernel, dim3(ngroups), dim3(kThreads), 0, (hipStream_t)stream,
                     batch, descs, modes, groups, block_base, total_blocks, cls, tables, word_off,
                     counts, payload, payload_words, err);
  return rgbac::check_launch("rgbac_color_blend_decode");
}
