// Palette mode of the lossless RGBA files (rgbac/rgbalossless.py, version 3
// RGAL files): an image with at most 256 distinct pixels becomes a sorted palette and one uint8
// plane of palette positions, which csrc/alpha_exact.hip codes as it codes any plane.  Deciding
// that, building the palette in the format's order and turning pixels into indices and back is
// done here, for a ragged batch, without a host round trip in between.
//
// A pixel is its little-endian dword R | G << 8 | B << 16 | A << 24; its CANONICAL form is the
// dword itself, or 0 where alpha is 0 and keep_hidden is not set.  The palette of an image is
// the set of its canonical pixels, ascending by the 48-bit key A << 40 | ((R + 2 G + B) >> 2) <<
// 32 | dword: one order per image, whatever order the workgroups met the colours in.
//
// An image is FLAT where its rows lie back to back (row stride = 4 w); pixel i of a flat image
// is at byte 4 i, and where its first byte is 16-byte aligned as well a lane moves its four
// consecutive pixels 4 q .. 4 q + 3 (a QUAD) as one 16-byte access.  The last quad of an image
// may be short and any image may be a view with longer rows: those go pixel by pixel, always as
// whole dwords.  A workgroup of 256 lanes covers a SLICE of 4,096 pixels: four rounds, lane t
// taking quad 256 round + t of the slice, so that a wave reads 1 KiB at a stretch.
//
// The sets are open-addressing tables of 512 dwords with linear probing from a multiplicative
// hash; 0 marks an empty slot, so the pixel 0 is kept as a flag beside the table.  At most 256
// colours ever count, so a table that matters is never more than half full; every probe loop is
// bounded by the table's size all the same.
//
// Kernels:
//   collect  grid (slices, images).  Lanes canonicalise their pixels, skip one that equals the
//            lane's previous pixel, and put the others into the workgroup's LDS set with LDS
//            compare-and-swap; the 257th colour raises the image's overflow word and ends the
//            workgroup.  Otherwise lane t merges slots t and t + 256 into the image's set in
//            global memory with global compare-and-swap; a colour that is new there bumps the
//            image's count, and the bump that finds 256 already raises the overflow word.
//            Workgroups that find the word raised when they start leave at once.
//   order    one workgroup per image: the image's set becomes up to 256 keys in LDS, padded with
//            an all-ones sentinel, sorted by a bitonic network (36 compare-exchange steps, lane t
//            owning element t), and written out as overflow, n, palette[256].
//   map      grid (slices, images).  The palette goes into an LDS table of 512 (dword, position);
//            a lane looks up the four pixels of a quad and stores the four positions as one
//            dword of the index plane.  A pixel that is not in the palette reports code 3.
//   unmap    grid (slices, images), after the plane decoder on the same stream.  The palette
//            lies in 1 KiB of LDS; a lane reads one dword of four positions and writes a quad.
//            A position >= n reports code 3 and writes the dword 0.
// A descriptor that does not hold together (null, misaligned, a side outside [1, 32767], rows
// that overlap, an index plane of another shape) reports code 5 and nothing of its image is
// touched.  No kernel reads or writes outside h x w pixels of an image, h x w bytes of a plane
// and the image's own entries of the per-image arrays.
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

typedef rgbac_image_desc ImgDesc;

constexpr int kThreads = 256;
constexpr int kRounds = 4;                          // quads per lane
constexpr int kSlicePix = RGBAC_PALETTE_SLICE;      // 4,096 pixels per workgroup
constexpr int kMax = RGBAC_PALETTE_MAX;             // 256 colours
constexpr int kSlots = RGBAC_PALETTE_SLOTS;         // 512
constexpr int kState = RGBAC_PALETTE_STATE_U32;     // slots, count, overflow, zero flag, pad
constexpr int kCount = kSlots, kOverflow = kSlots + 1, kZero = kSlots + 2;
constexpr int kResult = RGBAC_PALETTE_RESULT_U32;   // overflow, n, palette[256]
constexpr int kMaxSide = 32767;                     // h * w < 2^30: pixel numbers fit an int
constexpr int32_t kErrCorrupt = 3, kErrDesc = 5;
static_assert(kSlicePix == kThreads * kRounds * 4 && kSlots == 2 * kThreads && kMax == kThreads &&
                  kState == kSlots + 4 && kResult == kMax + 2,
              "the index arithmetic assumes 256 lanes, 512 slots, 256 colours");

struct Image {
  uint8_t* p;
  int w, npix;
  long long rs;
  bool flat, vec;   // rows back to back; and 16-byte aligned
};

__device__ inline bool image_of(const ImgDesc& d, Image& im) {
  if (!d.ptr || d.h <= 0 || d.w <= 0 || d.h > kMaxSide || d.w > kMaxSide) return false;
  if (((uintptr_t)d.ptr & 3) || (d.row_stride_bytes & 3) || d.row_stride_bytes < 4LL * d.w)
    return false;
  im.p = reinterpret_cast<uint8_t*>(d.ptr);
  im.w = d.w;
  im.npix = d.h * d.w;
  im.rs = d.row_stride_bytes;
  im.flat = d.h == 1 || d.row_stride_bytes == 4LL * d.w;
  im.vec = im.flat && ((uintptr_t)d.ptr & 15) == 0;
  return true;
}

// the dense uint8 index plane that belongs to image d, or nullptr
__device__ inline uint8_t* plane_of(const ImgDesc& pl, const ImgDesc& d) {
  if (!pl.ptr || ((uintptr_t)pl.ptr & 3) || pl.h != d.h || pl.w != d.w ||
      (pl.h > 1 && pl.row_stride_bytes != pl.w))
    return nullptr;
  return reinterpret_cast<uint8_t*>(pl.ptr);
}

__device__ inline uint32_t* pixel_at(const Image& im, int i) {
  if (im.flat) return reinterpret_cast<uint32_t*>(im.p + 4LL * i);
  const int r = i / im.w;
  return reinterpret_cast<uint32_t*>(im.p + r * im.rs + 4LL * (i - r * im.w));
}

// pixels i0 .. i0 + n - 1 (n in 1..4) of the image
__device__ inline void load_quad(const Image& im, int i0, int n, uint32_t (&px)[4]) {
  if (im.vec && n == 4) {
    const uint4 v = *reinterpret_cast<const uint4*>(im.p + 4LL * i0);
    px[0] = v.x, px[1] = v.y, px[2] = v.z, px[3] = v.w;
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) px[k] = k < n ? *pixel_at(im, i0 + k) : 0u;
}

__device__ inline void store_quad(const Image& im, int i0, int n, const uint32_t (&px)[4]) {
  if (im.vec && n == 4) {
    *reinterpret_cast<uint4*>(im.p + 4LL * i0) = make_uint4(px[0], px[1], px[2], px[3]);
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < n) *pixel_at(im, i0 + k) = px[k];
}

// the first pixel and the length of the quad that lane t takes in round `round` of slice `slice`;
// false past the image's end (then every later round of the lane is past it too)
__device__ inline bool quad_of(const Image& im, int slice, int round, int t, int& i0, int& n) {
  const long long at = (long long)slice * kSlicePix + 4LL * (round * kThreads + t);
  if (at >= im.npix) return false;
  i0 = (int)at;
  n = min(4, im.npix - i0);
  return true;
}

__device__ inline uint32_t canonical(uint32_t p, int keep_hidden) {
  return (keep_hidden || (p >> 24)) ? p : 0u;
}

__device__ inline int slot_of(uint32_t v) { return (int)((v * 2654435761u) >> 23); }   // 9 bits

__device__ inline uint32_t peek(const uint32_t* word) {
  return __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// v != 0 into a 512-slot set, LDS or global: 1 it is new, 0 it was there, 2 the set is full.
// (Reading the slot before the compare-and-swap made collect slower on the device, 207 us
// against 148 us over section 31's images, and was taken out again.)
__device__ inline int set_insert(uint32_t* set, uint32_t v) {
  int s = slot_of(v);
  for (int i = 0; i < kSlots; ++i) {
    const uint32_t have = atomicCAS(&set[s], 0u, v);
    if (have == 0u) return 1;
    if (have == v) return 0;
    s = (s + 1) & (kSlots - 1);
  }
  return 2;
}

__device__ inline void report(int32_t* err, int32_t code) {
  atomicCAS(err, 0, code);                 // the first non-zero code wins
}

// ------------------------------------------------------------------ collect
__global__ __launch_bounds__(kThreads) void palette_collect_kernel(
    const ImgDesc* __restrict__ descs, int keep_hidden, uint32_t* __restrict__ state,
    int32_t* __restrict__ err) {
  __shared__ uint32_t set[kSlots];
  __shared__ uint32_t count, zero, over;    // non-zero colours, the pixel 0 was met, give up
  const int b = blockIdx.y, t = threadIdx.x;
  Image im;
  if (!image_of(descs[b], im)) {
    if (blockIdx.x == 0 && t == 0) report(err, kErrDesc);
    return;
  }
  if ((long long)blockIdx.x * kSlicePix >= im.npix) return;
  uint32_t* st = state + (size_t)b * kState;
  set[t] = 0u;
  set[t + kThreads] = 0u;
  if (t == 0) {
    count = 0u;
    zero = 0u;
    over = peek(&st[kOverflow]);            // another workgroup has settled the image already
  }
  __syncthreads();
  if (over) return;
  volatile uint32_t* vover = &over;
  uint32_t prev = 0u;
  bool have = false;
  for (int round = 0; round < kRounds; ++round) {
    int i0, n;
    if (!quad_of(im, blockIdx.x, round, t, i0, n) || *vover) break;
    uint32_t px[4];
    load_quad(im, i0, n, px);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= n) break;
      const uint32_t v = canonical(px[k], keep_hidden);
      if (have && v == prev) continue;
      prev = v;
      have = true;
      if (v == 0u) {
        zero = 1u;
        continue;
      }
      const int r = set_insert(set, v);
      if (r == 2 || (r == 1 && atomicAdd(&count, 1u) >= (uint32_t)kMax)) *vover = 1u;
    }
  }
  __syncthreads();
  if (over || count + zero > (uint32_t)kMax) {
    if (t == 0) atomicExch(&st[kOverflow], 1u);
    return;
  }
  // merge: every colour that is new to the image counts once
  int fresh = 0, full = 0;
  if (t == 0 && zero) fresh += atomicExch(&st[kZero], 1u) == 0u;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const uint32_t v = set[t + q * kThreads];
    if (v == 0u) continue;
    const int r = set_insert(st, v);
    fresh += r == 1;
    full |= r == 2;
  }
  for (int i = 0; i < fresh; ++i)
    if (atomicAdd(&st[kCount], 1u) >= (uint32_t)kMax) full = 1;
  if (full) atomicExch(&st[kOverflow], 1u);
}

// ------------------------------------------------------------------ order
__device__ inline unsigned long long key_of(uint32_t v) {
  const uint32_t luma = ((v & 255u) + 2u * ((v >> 8) & 255u) + ((v >> 16) & 255u)) >> 2;
  return ((unsigned long long)(v >> 24) << 40) | ((unsigned long long)luma << 32) | v;
}

__global__ __launch_bounds__(kThreads) void palette_order_kernel(
    const uint32_t* __restrict__ state, uint32_t* __restrict__ result) {
  __shared__ unsigned long long key[kMax];
  __shared__ uint32_t found;
  const int b = blockIdx.x, t = threadIdx.x;
  const uint32_t* st = state + (size_t)b * kState;
  uint32_t* res = result + (size_t)b * kResult;
  key[t] = ~0ull;                            // the sentinel: above every key, which has 48 bits
  if (t == 0) found = 0u;
  __syncthreads();
  const bool over = st[kOverflow] != 0u;     // workgroup-uniform
  if (!over) {
    // the count is taken from the set itself; the order of arrival does not matter, the sort
    // settles it
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const uint32_t v = st[t + q * kThreads];
      if (v == 0u) continue;
      const uint32_t at = atomicAdd(&found, 1u);
      if (at < (uint32_t)kMax) key[at] = key_of(v);
    }
    if (t == 0 && st[kZero]) {
      const uint32_t at = atomicAdd(&found, 1u);
      if (at < (uint32_t)kMax) key[at] = 0ull;
    }
  }
  __syncthreads();
  const uint32_t n = found;
  if (over || n == 0u || n > (uint32_t)kMax) {   // n == 0: collect did not touch the image
    if (t == 0) res[0] = 1u, res[1] = 0u;
    res[2 + t] = 0u;
    return;
  }
  for (int k = 2; k <= kMax; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int p = t ^ j;
      if (p > t) {
        const unsigned long long a = key[t], c = key[p];
        if ((a > c) == ((t & k) == 0)) key[t] = c, key[p] = a;
      }
      __syncthreads();
    }
  }
  if (t == 0) res[0] = 0u, res[1] = n;
  res[2 + t] = (uint32_t)t < n ? (uint32_t)key[t] : 0u;
}

// ------------------------------------------------------------------ map
__global__ __launch_bounds__(kThreads) void palette_map_kernel(
    const ImgDesc* __restrict__ descs, const ImgDesc* __restrict__ planes, int keep_hidden,
    const uint32_t* __restrict__ result, int32_t* __restrict__ err) {
  __shared__ uint32_t lkey[kSlots];
  __shared__ uint8_t lpos[kSlots];
  __shared__ int zero_pos;                   // the palette position of the pixel 0, or -1
  const int b = blockIdx.y, t = threadIdx.x;
  const uint32_t* res = result + (size_t)b * kResult;
  if (res[0]) return;                        // more than 256 colours: the image goes another way
  Image im;
  uint8_t* plane = nullptr;
  const uint32_t n = res[1];
  if (!image_of(descs[b], im) || !(plane = plane_of(planes[b], descs[b])) || n == 0u ||
      n > (uint32_t)kMax) {
    if (blockIdx.x == 0 && t == 0) report(err, kErrDesc);
    return;
  }
  if ((long long)blockIdx.x * kSlicePix >= im.npix) return;
  lkey[t] = 0u;
  lkey[t + kThreads] = 0u;
  if (t == 0) zero_pos = -1;
  __syncthreads();
  if ((uint32_t)t < n) {
    const uint32_t v = res[2 + t];
    if (v == 0u) {
      zero_pos = t;
    } else {
      int s = slot_of(v);
      for (int i = 0; i < kSlots; ++i) {     // palette entries differ: every one finds a slot
        if (atomicCAS(&lkey[s], 0u, v) == 0u) {
          lpos[s] = (uint8_t)t;
          break;
        }
        s = (s + 1) & (kSlots - 1);
      }
    }
  }
  __syncthreads();
  bool missing = false;
  for (int round = 0; round < kRounds; ++round) {
    int i0, cnt;
    if (!quad_of(im, blockIdx.x, round, t, i0, cnt)) break;
    uint32_t px[4], packed = 0u;
    load_quad(im, i0, cnt, px);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= cnt) break;
      const uint32_t v = canonical(px[k], keep_hidden);
      int pos = -1;
      if (v == 0u) {
        pos = zero_pos;
      } else {
        int s = slot_of(v);
        for (int i = 0; i < kSlots; ++i) {
          const uint32_t have = lkey[s];
          if (have == v) pos = lpos[s];
          if (have == v || have == 0u) break;
          s = (s + 1) & (kSlots - 1);
        }
      }
      if (pos < 0) missing = true, pos = 0;
      packed |= (uint32_t)pos << (8 * k);
    }
    if (cnt == 4) {
      *reinterpret_cast<uint32_t*>(plane + i0) = packed;   // i0 is a multiple of 4
    } else {
      for (int k = 0; k < cnt; ++k) plane[i0 + k] = (uint8_t)(packed >> (8 * k));
    }
  }
  if (missing) report(err, kErrCorrupt);
}

// ------------------------------------------------------------------ unmap
__global__ __launch_bounds__(kThreads) void palette_unmap_kernel(
    const ImgDesc* __restrict__ descs, const ImgDesc* __restrict__ planes,
    const uint32_t* __restrict__ palettes, const int32_t* __restrict__ counts,
    int32_t* __restrict__ err) {
  __shared__ uint32_t pal[kMax];
  const int b = blockIdx.y, t = threadIdx.x;
  Image im;
  const uint8_t* plane = nullptr;
  const int n = counts[b];
  if (!image_of(descs[b], im) || !(plane = plane_of(planes[b], descs[b])) || n < 1 || n > kMax) {
    if (blockIdx.x == 0 && t == 0) report(err, kErrDesc);
    return;
  }
  if ((long long)blockIdx.x * kSlicePix >= im.npix) return;
  pal[t] = t < n ? palettes[(size_t)b * kMax + t] : 0u;
  __syncthreads();
  bool beyond = false;
  for (int round = 0; round < kRounds; ++round) {
    int i0, cnt;
    if (!quad_of(im, blockIdx.x, round, t, i0, cnt)) break;
    uint32_t packed = 0u;
    if (cnt == 4) {
      packed = *reinterpret_cast<const uint32_t*>(plane + i0);
    } else {
      for (int k = 0; k < cnt; ++k) packed |= (uint32_t)plane[i0 + k] << (8 * k);
    }
    uint32_t px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int pos = (packed >> (8 * k)) & 255u;
      if (k < cnt && pos >= n) beyond = true;
      px[k] = pal[pos];                      // 0 from n on
    }
    store_quad(im, i0, cnt, px);
  }
  if (beyond) report(err, kErrCorrupt);
}

}  // namespace

#define PALETTE_REQUIRE_COMMON()                                                            \
  RGBAC_REQUIRE(batch > 0 && batch <= 65535, "batch must be in [1, 65535]");                \
  RGBAC_REQUIRE(slices > 0 && slices <= (1 << 18), "slices must be in [1, 2^18]");          \
  RGBAC_REQUIRE(descs && err, "null pointer")

extern "C" int rgbac_color_palette_collect(int batch, const rgbac_image_desc* descs,
                                           int keep_hidden, int slices, uint32_t* state,
                                           int32_t* err, void* stream) {
  PALETTE_REQUIRE_COMMON();
  RGBAC_REQUIRE(keep_hidden == 0 || keep_hidden == 1, "keep_hidden must be 0 or 1");
  RGBAC_REQUIRE(state, "null pointer");
  hipLaunchKernelGGL(palette_collect_kernel, dim3(slices, batch), dim3(kThreads), 0,
                     (hipStream_t)stream, descs, keep_hidden, state, err);
  return rgbac::check_launch("rgbac_color_palette_collect");
}

extern "C" int rgbac_color_palette_order(int batch, const uint32_t* state, uint32_t* result,
                                         void* stream) {
  RGBAC_REQUIRE(batch > 0 && batch <= 65535, "batch must be in [1, 65535]");
  RGBAC_REQUIRE(state && result, "null pointer");
  hipLaunchKernelGGL(palette_order_kernel, dim3(batch), dim3(kThreads), 0, (hipStream_t)stream,
                     state, result);
  return rgbac::check_launch("rgbac_color_palette_order");
}

extern "C" int rgbac_color_palette_map(int batch, const rgbac_image_desc* descs,
                                       const rgbac_image_desc* planes, int keep_hidden,
                                       int slices, const uint32_t* result, int32_t* err,
                                       void* stream) {
  PALETTE_REQUIRE_COMMON();
  RGBAC_REQUIRE(keep_hidden == 0 || keep_hidden == 1, "keep_hidden must be 0 or 1");
  RGBAC_REQUIRE(planes && result, "null pointer");
  hipLaunchKernelGGL(palette_map_kernel, dim3(slices, batch), dim3(kThreads), 0,
                     (hipStream_t)stream, descs, planes, keep_hidden, result, err);
  return rgbac::check_launch("rgbac_color_palette_map");
}

extern "C" int rgbac_color_palette_unmap(int batch, const rgbac_image_desc* descs,
                                         const rgbac_image_desc* planes, int slices,
                                         const uint32_t* palettes, const int32_t* counts,
                                         int32_t* err, void* stream) {
  PALETTE_REQUIRE_COMMON();
  RGBAC_REQUIRE(planes && palettes && counts, "null pointer");
  hipLaunchKernelGGL(palette_unmap_kernel, dim3(slices, batch), dim3(kThreads), 0,
                     (hipStream_t)stream, descs, planes, palettes, counts, err);
  return rgbac::check_launch("rgbac_color_palette_unmap");
}
