// Images of any size: the geometry layer in front of / behind the two codecs, which only take
// heights and widths that are multiples of 64 (check_geometry, AutoEncoderRGB_Journal.py:242).
// A batch of B images (h_b, w_b) shares one canvas hp x wp = round_up(max h_b, 64) x
// round_up(max w_b, 64); every image sits at its top-left corner.  Outside an image's
// rectangle the canvas holds 0 (RGBAC_PAD_TRANSPARENT: alpha 0 there, so the masked window
// attention drops those windows and the masked MSE never counts them) or the image's nearest
// edge pixel (RGBAC_PAD_REPLICATE: an opaque image stays all-ones in alpha).
//   * rgba_pack_kernel:    ragged uint8 RGBA (h_b, w_b, 4) -> padded fp32 NCHW alpha / rgb /
//                          masked = where(alpha > 0, rgb, alpha) (MYdataset.py:113), /255 by
//                          IEEE division (ToTensor);
//   * rgba_opaque_*:       per image, whether every alpha byte of its rectangle is 255 (what
//                          decides replicate padding and "no alpha stream" per image); the
//                          pack kernel takes one pad mode per image for that;
//   * pad_nchw_kernel:     fp32 (B,C,h,w) -> (B,C,hp,wp), either mode;
//   * rgba_unpack_kernel:  padded fp32 x_hat (+ alpha) -> ragged uint8 RGBA cropped to
//                          (h_b, w_b): u8 = (uint8) clamp(x*255 + 0.5, 0, 255), the multiply and
//                          the add rounded separately (torchvision save_image after the clamp
//                          of trainRGB.py:290,295-297);
//   * region_error_*:      reconstruct_error (AutoEncoderRGB_Journal.py:36-64) restricted to each
//                          image's rectangle: fp64 squared error over mask > 0, per image.
// All HBM-bound element work: one thread per 4 canvas columns (16-byte fp32 loads / stores,
// canvas rows are 256-byte aligned since wp % 64 == 0; the uint8 side is only 4-byte aligned
// and is moved one pixel = one dword at a time, adjacent lanes 16 bytes apart), one launch per
// batch, a capped grid with a grid-stride loop.
#include "common.h"

namespace rgbac {

typedef rgbac_image_desc ImgDesc;

inline int any_grid(long long items) {
  long long b = (items + 255) / 256;
  const long long cap = (long long)device_cus() * 16;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

__device__ __forceinline__ void st_f4(float* p, const float (&v)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void ld_f4(const float* p, float (&v)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}

__global__ void __launch_bounds__(256)
rgba_pack_kernel(const ImgDesc* __restrict__ descs, int hp, int wp, long long items, int mode,
                 const int32_t* __restrict__ modes, float* __restrict__ alpha,
                 float* __restrict__ rgb, float* __restrict__ masked) {
  const int wq = wp >> 2;
  const size_t plane = (size_t)hp * wp;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items;
       i += (long long)gridDim.x * 256) {
    const int q = (int)(i % wq);
    const long long t = i / wq;
    const int r = (int)(t % hp);
    const int b = (int)(t / hp);
    const ImgDesc d = descs[b];
    const int c0 = q << 2;
    float v[4][4];  // [channel R,G,B,A][column]
    // an empty descriptor reads nothing and yields zeros (the host builds them checked)
    const bool ok = d.ptr && d.h > 0 && d.w > 0;
    // one mode for the batch, or one per image (rgbac_rgba_pack_modes)
    const bool rep = (modes ? modes[b] : mode) == RGBAC_PAD_REPLICATE;
    const int sr = r < d.h ? r : d.h - 1;
    const bool row_in = ok && (rep || r < d.h);
    const uint8_t* row = reinterpret_cast<const uint8_t*>(d.ptr) + (long long)sr * d.row_stride_bytes;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + j;
      const int sc = c < d.w ? c : d.w - 1;
      uchar4 p = make_uchar4(0, 0, 0, 0);
      if (row_in && (rep || c < d.w)) p = *reinterpret_cast<const uchar4*>(row + 4 * (size_t)sc);
      v[0][j] = (float)p.x / 255.0f;
      v[1][j] = (float)p.y / 255.0f;
      v[2][j] = (float)p.z / 255.0f;
      v[3][j] = (float)p.w / 255.0f;
    }
    const size_t o = (size_t)r * wp + c0;
    if (alpha) st_f4(alpha + (size_t)b * plane + o, v[3]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (rgb) st_f4(rgb + ((size_t)b * 3 + c) * plane + o, v[c]);
      if (masked) {
        float m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = v[3][j] > 0.f ? v[c][j] : v[3][j];
        st_f4(masked + ((size_t)b * 3 + c) * plane + o, m);
      }
    }
  }
}

// grid (RGBAC_OPAQUE_BLOCKS, B): block k of image b looks at its share of the rectangle's
// pixels (one dword per lane, adjacent lanes adjacent pixels of a row) and writes
// scratch[b * RGBAC_OPAQUE_BLOCKS + k] = 1 if every alpha byte it saw is 255 (a block without
// pixels writes 1; an empty descriptor 0).  An integer AND: no order to fix.
__global__ void __launch_bounds__(256)
rgba_opaque_kernel(const ImgDesc* __restrict__ descs, int32_t* __restrict__ scratch) {
  const int b = blockIdx.y;
  const ImgDesc d = descs[b];
  const bool ok = d.ptr && d.h > 0 && d.w > 0;
  int all = ok ? 1 : 0;
  if (ok) {
    const long long items = (long long)d.h * d.w;
    const uint8_t* base = reinterpret_cast<const uint8_t*>(d.ptr);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items;
         i += (long long)gridDim.x * 256) {
      const int r = (int)(i / d.w), c = (int)(i - (long long)r * d.w);
      const uchar4 p =
          *reinterpret_cast<const uchar4*>(base + (long long)r * d.row_stride_bytes + 4 * (size_t)c);
      all &= p.w == 255 ? 1 : 0;
    }
  }
  all = __syncthreads_and(all);
  if (threadIdx.x == 0) scratch[(size_t)b * gridDim.x + blockIdx.x] = all ? 1 : 0;
}

// one thread per image: the AND of its block flags
__global__ void __launch_bounds__(256)
rgba_opaque_final_kernel(int batch, const int32_t* __restrict__ scratch,
                         int32_t* __restrict__ flags) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  int all = 1;
  for (int k = 0; k < RGBAC_OPAQUE_BLOCKS; ++k) all &= scratch[(size_t)b * RGBAC_OPAQUE_BLOCKS + k];
  flags[b] = all;
}

__global__ void __launch_bounds__(256)
pad_nchw_kernel(int h, int w, int hp, int wp, long long items, int mode,
                const float* __restrict__ x, float* __restrict__ out) {
  const int wq = wp >> 2;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items;
       i += (long long)gridDim.x * 256) {
    const int q = (int)(i % wq);
    const long long t = i / wq;
    const int r = (int)(t % hp);
    const long long pl = t / hp;
    const bool rep = mode == RGBAC_PAD_REPLICATE;
    const int sr = r < h ? r : h - 1;
    const float* row = x + ((size_t)pl * h + sr) * w;
    const bool row_in = rep || r < h;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = (q << 2) + j;
      const int sc = c < w ? c : w - 1;
      v[j] = (row_in && (rep || c < w)) ? row[sc] : 0.f;
    }
    st_f4(out + ((size_t)pl * hp + r) * wp + (q << 2), v);
  }
}

// (uint8) clamp(x*255 + 0.5, 0, 255): two separately rounded fp32 operations -- a fused
// multiply-add rounds once and lands on the other byte next to a tie
__device__ __forceinline__ uint8_t quant_u8(float x) {
  float v = __fadd_rn(__fmul_rn(x, 255.0f), 0.5f);
  v = fminf(fmaxf(v, 0.0f), 255.0f);
  return (uint8_t)v;
}

__global__ void __launch_bounds__(256)
rgba_unpack_kernel(const ImgDesc* __restrict__ descs, int hp, int wp, long long items,
                   const float* __restrict__ x_hat, const float* __restrict__ alpha,
                   int zero_transparent) {
  const int wq = wp >> 2;
  const size_t plane = (size_t)hp * wp;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items;
       i += (long long)gridDim.x * 256) {
    const int q = (int)(i % wq);
    const long long t = i / wq;
    const int r = (int)(t % hp);
    const int b = (int)(t / hp);
    const ImgDesc d = descs[b];
    const int c0 = q << 2;
    if (!d.ptr || r >= d.h || c0 >= d.w) continue;     // nothing of this quad is in the crop
    const size_t o = (size_t)r * wp + c0;
    float v[4][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) ld_f4(x_hat + ((size_t)b * 3 + c) * plane + o, v[c]);
    if (alpha) ld_f4(alpha + (size_t)b * plane + o, v[3]);
    uint8_t* row = reinterpret_cast<uint8_t*>(d.ptr) + (long long)r * d.row_stride_bytes;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (c0 + j >= d.w) continue;
      uchar4 p;
      p.w = alpha ? quant_u8(v[3][j]) : (uint8_t)255;
      const bool zero = zero_transparent && p.w == 0;
      p.x = zero ? (uint8_t)0 : quant_u8(v[0][j]);
      p.y = zero ? (uint8_t)0 : quant_u8(v[1][j]);
      p.z = zero ? (uint8_t)0 : quant_u8(v[2][j]);
      *reinterpret_cast<uchar4*>(row + 4 * (size_t)(c0 + j)) = p;
    }
  }
}

// rgba_opaque_kernel with a second flag: scratch[(b * RGBAC_OPAQUE_BLOCKS + k) * 2 + {0, 1}] =
// {every alpha byte block k saw is 255, every one is 0} (a block without pixels writes 1, 1; an
// empty descriptor 0, 0)
__global__ void __launch_bounds__(256)
rgba_alpha_class_kernel(const ImgDesc* __restrict__ descs, int32_t* __restrict__ scratch) {
  const int b = blockIdx.y;
  const ImgDesc d = descs[b];
  const bool ok = d.ptr && d.h > 0 && d.w > 0;
  int full = ok ? 1 : 0, none = ok ? 1 : 0;
  if (ok) {
    const long long items = (long long)d.h * d.w;
    const uint8_t* base = reinterpret_cast<const uint8_t*>(d.ptr);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items;
         i += (long long)gridDim.x * 256) {
      const int r = (int)(i / d.w), c = (int)(i - (long long)r * d.w);
      const uchar4 p =
          *reinterpret_cast<const uchar4*>(base + (long long)r * d.row_stride_bytes + 4 * (size_t)c);
      full &= p.w == 255 ? 1 : 0;
      none &= p.w == 0 ? 1 : 0;
    }
  }
  full = __syncthreads_and(full);
  none = __syncthreads_and(none);
  if (threadIdx.x == 0) {
    int32_t* o = scratch + ((size_t)b * gridDim.x + blockIdx.x) * 2;
    o[0] = full ? 1 : 0;
    o[1] = none ? 1 : 0;
  }
}

// one thread per rectangle: the ANDs of its block flags -> 1 opaque, 2 transparent, 0 mixed
__global__ void __launch_bounds__(256)
rgba_alpha_class_final_kernel(int batch, const int32_t* __restrict__ scratch,
                              int32_t* __restrict__ cls) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  int full = 1, none = 1;
  for (int k = 0; k < RGBAC_OPAQUE_BLOCKS; ++k) {
    full &= scratch[((size_t)b * RGBAC_OPAQUE_BLOCKS + k) * 2];
    none &= scratch[((size_t)b * RGBAC_OPAQUE_BLOCKS + k) * 2 + 1];
  }
  cls[b] = full ? 1 : (none ? 2 : 0);
}

// One fp32 multiply / add, rounded on its own.  The header's __fmul_rn / __fadd_rn are plain
// operators under the default contraction mode: once inlined, a product feeding a sum becomes one
// FMA, which rounds once.  The blend's sums of products must match their numpy twin bit for bit
// (alpha is k/255 and the weights are dyadic, so sums land on the quantiser's ties), hence
// operators compiled with contraction off.
__device__ __forceinline__ float mul_rn(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ float add_rn(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}

// Seam blend of decoded tiles (include/rgbac.h has the rule).  One axis of one pixel: the later
// tile j that holds p, whether the tile before it holds p too, and the weight of each.
struct BlendAxis {
  int j;          // last tile whose origin is <= p
  bool two;       // tile j - 1 covers p as well
  float w0, w1;   // weights of tile j - 1 (when two) and of tile j
};
__device__ __forceinline__ BlendAxis blend_axis(int p, int k, int stride, int overlap) {
  BlendAxis a;
  int j = p / stride;
  a.j = j < k - 1 ? j : k - 1;
  const int d = p - a.j * stride;
  a.two = a.j >= 1 && d < overlap;
  a.w1 = 1.0f;
  a.w0 = 0.0f;
  if (a.two) {
    a.w1 = __fdiv_rn(add_rn((float)d, 0.5f), (float)overlap);
    a.w0 = add_rn(1.0f, -a.w1);
  }
  return a;
}

// grid (capped, nout): the blocks of output k walk its dst.h x dst.w pixels, one dword per lane,
// adjacent lanes adjacent pixels of a row (the fp32 planes are read 4 bytes per lane from
// consecutive addresses: a region may start at any column, so nothing wider is aligned)
__global__ void __launch_bounds__(256)
rgba_blend_tiles_kernel(const rgbac_blend_desc* __restrict__ outs, int ntiles,
                        const rgbac_tile_desc* __restrict__ tiles) {
  const rgbac_blend_desc o = outs[blockIdx.y];
  const ImgDesc d = o.dst;
  // a descriptor that does not hold together writes nothing (the host builds them checked)
  if (!d.ptr || d.h <= 0 || d.w <= 0 || o.tile <= 0 || o.overlap < 0 ||
      o.overlap > o.tile / 2 || o.ky <= 0 || o.kx <= 0 || o.y0 < 0 || o.x0 < 0 || o.tile0 < 0 ||
      (long long)o.ky * o.kx > (long long)ntiles - o.tile0)
    return;
  const int stride = o.tile - o.overlap;
  const long long items = (long long)d.h * d.w;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items;
       i += (long long)gridDim.x * 256) {
    const int r = (int)(i / d.w), c = (int)(i - (long long)r * d.w);
    const int py = o.y0 + r, px = o.x0 + c;
    const BlendAxis ay = blend_axis(py, o.ky, stride, o.overlap);
    const BlendAxis ax = blend_axis(px, o.kx, stride, o.overlap);
    float A = 0.0f, Wp = 0.0f, C[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < 4; ++s) {                    // row-major over the 2 x 2 candidates
      const bool hy = s >> 1, hx = s & 1;            // 0: the earlier tile, 1: tile j
      if ((!hy && !ay.two) || (!hx && !ax.two)) continue;
      const int ty = hy ? ay.j : ay.j - 1, tx = hx ? ax.j : ax.j - 1;
      const rgbac_tile_desc t = tiles[o.tile0 + ty * o.kx + tx];
      const int ly = py - t.oy, lx = px - t.ox;
      if (!t.x_hat || ly < 0 || lx < 0 || ly >= t.ey || lx >= t.ex || t.ey > t.hp || t.ex > t.wp)
        continue;
      const float w = mul_rn(hy ? ay.w1 : ay.w0, hx ? ax.w1 : ax.w0);
      const size_t plane = (size_t)t.hp * t.wp, at = (size_t)ly * t.wp + lx;
      const float a = t.alpha ? t.alpha[at] : 1.0f;
      A = add_rn(A, mul_rn(w, a));
      if (a > 0.0f) {
        Wp = add_rn(Wp, w);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
          C[ch] = add_rn(C[ch], mul_rn(w, t.x_hat[ch * plane + at]));
      }
    }
    uchar4 p;
    p.w = quant_u8(A);
    const bool zero = p.w == 0 || !(Wp > 0.0f);
    p.x = zero ? (uint8_t)0 : quant_u8(__fdiv_rn(C[0], Wp));
    p.y = zero ? (uint8_t)0 : quant_u8(__fdiv_rn(C[1], Wp));
    p.z = zero ? (uint8_t)0 : quant_u8(__fdiv_rn(C[2], Wp));
    *reinterpret_cast<uchar4*>(reinterpret_cast<uint8_t*>(d.ptr) +
                               (long long)r * d.row_stride_bytes + 4 * (size_t)c) = p;
  }
}

constexpr int kRegionMaxBlocks = 64;     // per image
inline int region_blocks(int hp, int wp) {
  long long b = ((long long)hp * (wp >> 2) + kReduceThreads - 1) / kReduceThreads;
  if (b > kRegionMaxBlocks) b = kRegionMaxBlocks;
  if (b < 1) b = 1;
  return (int)b;
}

// grid (nblk, B): block k of image b sums its share of the rectangle's quads in a fixed
// order and writes scratch[(b*nblk + k)*2 + {0, 1}] = {sse partial, counted pixels}
__global__ void __launch_bounds__(kReduceThreads)
region_error_kernel(const ImgDesc* __restrict__ descs, int channels, int hp, int wp,
                    const float* __restrict__ x, const float* __restrict__ y,
                    const float* __restrict__ mask, double* __restrict__ scratch) {
  __shared__ double smem[kReduceThreads / 64];
  const int b = blockIdx.y;
  const ImgDesc d = descs[b];
  const int h = d.h < hp ? d.h : hp, w = d.w < wp ? d.w : wp;
  const size_t plane = (size_t)hp * wp;
  double sse = 0.0, cnt = 0.0;
  if (h > 0 && w > 0) {
    const int wq = (w + 3) >> 2;
    const long long items = (long long)h * wq;
    for (long long i = (long long)blockIdx.x * kReduceThreads + threadIdx.x; i < items;
         i += (long long)gridDim.x * kReduceThreads) {
      const int r = (int)(i / wq), c0 = (int)(i - (long long)r * wq) << 2;
      const size_t o = (size_t)r * wp + c0;
      // padding columns of a quad that straddles the edge are loaded but never selected
      bool on[4];
      float m[4] = {1.f, 1.f, 1.f, 1.f};
      if (mask) ld_f4(mask + (size_t)b * plane + o, m);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        on[j] = c0 + j < w && m[j] > 0.f;
        if (on[j]) cnt += 1.0;
      }
      for (int c = 0; c < channels; ++c) {
        float xv[4], yv[4];
        ld_f4(x + ((size_t)b * channels + c) * plane + o, xv);
        ld_f4(y + ((size_t)b * channels + c) * plane + o, yv);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (on[j]) {
            const double e = (double)xv[j] - (double)yv[j];
            sse += e * e;
          }
        }
      }
    }
  }
  const double s = block_sum_f64(sse, smem);
  const double n = block_sum_f64(cnt, smem);     // integers below 2^53: exact
  if (threadIdx.x == 0) {
    double* o = scratch + ((size_t)b * gridDim.x + blockIdx.x) * 2;
    o[0] = s;
    o[1] = n;
  }
}

// one thread per image: the block partials in index order, then the scalars
__global__ void __launch_bounds__(256)
region_error_final_kernel(int batch, int channels, int nblk, const double* __restrict__ scratch,
                          double* __restrict__ sse, int64_t* __restrict__ n,
                          float* __restrict__ mse, float* __restrict__ psnr) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  double s = 0.0, c = 0.0;
  for (int k = 0; k < nblk; ++k) {
    s += scratch[((size_t)b * nblk + k) * 2];
    c += scratch[((size_t)b * nblk + k) * 2 + 1];
  }
  const double terms = c * (double)channels;
  const double m = s / (terms > 1.0 ? terms : 1.0);
  if (sse) sse[b] = s;
  if (n) n[b] = (int64_t)terms;
  if (mse) mse[b] = (float)m;
  if (psnr) psnr[b] = s > 0.0 ? (float)(10.0 * log10(1.0 / m)) : 100.0f;   // trainRGB.py:202-206
}

}  // namespace rgbac

using namespace rgbac;

#define RGBAC_REQUIRE_CANVAS(batch, hp, wp)                                                   \
  RGBAC_REQUIRE((batch) > 0 && (batch) < 65536, "batch");                                     \
  RGBAC_REQUIRE((hp) > 0 && (wp) > 0 && (hp) % 64 == 0 && (wp) % 64 == 0,                     \
                "the canvas height and width must be positive multiples of 64")

extern "C" int rgbac_rgba_pack(int batch, const rgbac_image_desc* descs, int hp, int wp,
                               int mode, float* alpha, float* rgb, float* masked, void* stream) {
  RGBAC_REQUIRE_CANVAS(batch, hp, wp);
  RGBAC_REQUIRE(descs, "null descriptor pointer");
  RGBAC_REQUIRE(mode == RGBAC_PAD_TRANSPARENT || mode == RGBAC_PAD_REPLICATE, "pad mode");
  RGBAC_REQUIRE(alpha || rgb || masked, "no output");
  const long long items = (long long)batch * hp * (wp >> 2);
  hipLaunchKernelGGL(rgba_pack_kernel, dim3(any_grid(items)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), descs, hp, wp, items, mode,
                     (const int32_t*)nullptr, alpha, rgb, masked);
  return check_launch("rgba_pack_kernel");
}

extern "C" int rgbac_rgba_pack_modes(int batch, const rgbac_image_desc* descs, int hp, int wp,
                                     const int32_t* modes, float* alpha, float* rgb,
                                     float* masked, void* stream) {
  RGBAC_REQUIRE_CANVAS(batch, hp, wp);
  RGBAC_REQUIRE(descs && modes, "null descriptor or mode pointer");
  RGBAC_REQUIRE(alpha || rgb || masked, "no output");
  const long long items = (long long)batch * hp * (wp >> 2);
  hipLaunchKernelGGL(rgba_pack_kernel, dim3(any_grid(items)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), descs, hp, wp, items,
                     (int)RGBAC_PAD_TRANSPARENT, modes, alpha, rgb, masked);
  return check_launch("rgba_pack_kernel");
}

extern "C" int rgbac_rgba_opaque(int batch, const rgbac_image_desc* descs, int32_t* scratch,
                                 int32_t* flags, void* stream) {
  RGBAC_REQUIRE(batch > 0 && batch < 65536, "batch");
  RGBAC_REQUIRE(descs && scratch && flags, "null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rgba_opaque_kernel, dim3(RGBAC_OPAQUE_BLOCKS, batch), dim3(256), 0, st,
                     descs, scratch);
  int rc = check_launch("rgba_opaque_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(rgba_opaque_final_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, batch,
                     scratch, flags);
  return check_launch("rgba_opaque_final_kernel");
}

extern "C" int rgbac_rgba_alpha_class(int batch, const rgbac_image_desc* descs, int32_t* scratch,
                                      int32_t* cls, void* stream) {
  RGBAC_REQUIRE(batch > 0 && batch < 65536, "batch");
  RGBAC_REQUIRE(descs && scratch && cls, "null pointer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rgba_alpha_class_kernel, dim3(RGBAC_OPAQUE_BLOCKS, batch), dim3(256), 0, st,
                     descs, scratch);
  int rc = check_launch("rgba_alpha_class_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(rgba_alpha_class_final_kernel, dim3((batch + 255) / 256), dim3(256), 0, st,
                     batch, scratch, cls);
  return check_launch("rgba_alpha_class_final_kernel");
}

extern "C" int rgbac_rgba_blend_tiles(int nout, const rgbac_blend_desc* outs, int ntiles,
                                      const rgbac_tile_desc* tiles, int64_t max_pixels,
                                      void* stream) {
  RGBAC_REQUIRE(nout > 0 && nout < 65536, "output count");
  RGBAC_REQUIRE(ntiles > 0, "tile count");
  RGBAC_REQUIRE(outs && tiles, "null descriptor pointer");
  RGBAC_REQUIRE(max_pixels > 0, "max_pixels");
  // the capped grid is shared among the outputs
  int gx = any_grid((long long)max_pixels);
  const int per = (device_cus() * 16 + nout - 1) / nout;
  if (gx > per) gx = per;
  hipLaunchKernelGGL(rgba_blend_tiles_kernel, dim3(gx, nout), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), outs, ntiles, tiles);
  return check_launch("rgba_blend_tiles_kernel");
}

extern "C" int rgbac_pad_nchw(int batch, int channels, int h, int w, int hp, int wp, int mode,
                              const float* x, float* out, void* stream) {
  RGBAC_REQUIRE_CANVAS(batch, hp, wp);
  RGBAC_REQUIRE(channels > 0 && h > 0 && w > 0 && h <= hp && w <= wp, "shape");
  RGBAC_REQUIRE(mode == RGBAC_PAD_TRANSPARENT || mode == RGBAC_PAD_REPLICATE, "pad mode");
  RGBAC_REQUIRE(x && out, "null pointer");
  const long long n_in = (long long)batch * channels * h * w;
  const long long n_out = (long long)batch * channels * hp * wp;
  RGBAC_REQUIRE(out + n_out <= x || x + n_in <= out, "the output must not alias the input");
  const long long items = n_out >> 2;
  hipLaunchKernelGGL(pad_nchw_kernel, dim3(any_grid(items)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), h, w, hp, wp, items, mode, x, out);
  return check_launch("pad_nchw_kernel");
}

extern "C" int rgbac_rgba_unpack(int batch, const rgbac_image_desc* descs, int hp, int wp,
                                 const float* x_hat, const float* alpha, int zero_transparent,
                                 void* stream) {
  RGBAC_REQUIRE_CANVAS(batch, hp, wp);
  RGBAC_REQUIRE(descs, "null descriptor pointer");
  RGBAC_REQUIRE(x_hat, "null pointer");
  const long long items = (long long)batch * hp * (wp >> 2);
  hipLaunchKernelGGL(rgba_unpack_kernel, dim3(any_grid(items)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), descs, hp, wp, items, x_hat, alpha,
                     zero_transparent);
  return check_launch("rgba_unpack_kernel");
}

extern "C" int rgbac_region_error_blocks(int hp, int wp) {
  if (hp <= 0 || wp <= 0) return 0;
  return region_blocks(hp, wp);
}

extern "C" int rgbac_region_error(int batch, int channels, const rgbac_image_desc* descs, int hp,
                                  int wp, const float* x, const float* y, const float* mask,
                                  double* scratch, double* sse, int64_t* n, float* mse,
                                  float* psnr, void* stream) {
  RGBAC_REQUIRE_CANVAS(batch, hp, wp);
  RGBAC_REQUIRE(channels > 0, "channels");
  RGBAC_REQUIRE(descs, "null descriptor pointer");
  RGBAC_REQUIRE(x && y && scratch, "null pointer");
  const int nblk = region_blocks(hp, wp);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(region_error_kernel, dim3(nblk, batch), dim3(kReduceThreads), 0, st, descs,
                     channels, hp, wp, x, y, mask, scratch);
  int rc = check_launch("region_error_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(region_error_final_kernel, dim3((batch + 255) / 256), dim3(256), 0, st,
                     batch, channels, nblk, scratch, sse, n, mse, psnr);
  return check_launch("region_error_final_kernel");
}
