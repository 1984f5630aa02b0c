// Per-image rate of a batch (evaluation): the forward's bits partials are indexed by the GAUSS
// conv's M-tile block and cannot be split by image afterwards, but every GAUSS epilogue and both
// eb_forward kernels can store the fp32 likelihood they computed (aux1 / lik), and their bits
// term is bits_of() of exactly that float (conv_common.h, entropy.hip).  This file sums
// (double) bits_of(lik) per image over likelihood tensors laid out [segments][B][n_per_image]
// (the slices of one model side by side, or z alone with segments = 1).
//   * bits_image_kernel: grid (nblk, B); block k of image b walks its share of the image's
//     segments * n elements in a fixed order, one fp64 partial per block;
//   * bits_image_final_kernel: one thread per image adds its block partials in index order.
// No atomics: bit-reproducible, and an image's sum depends on its own likelihoods only.
#include "common.h"

namespace rgbac {

// the same fp32 expression as bits_of (AutoEncoderRGB_Journal.py:280):
// clamp(-1.0 * log(lik + 1e-10) / log(2.0), 0, 50)
__device__ __forceinline__ float image_bits_of(float lik) {
  float b = (-1.0f * logf(lik + 1e-10f)) / 0.69314718055994530942f;
  return fminf(fmaxf(b, 0.0f), 50.0f);
}

constexpr int kBitsMaxBlocks = 64;     // per image
inline int bits_blocks(long long per_image) {
  long long b = (per_image + kReduceThreads - 1) / kReduceThreads;
  if (b > kBitsMaxBlocks) b = kBitsMaxBlocks;
  if (b < 1) b = 1;
  return (int)b;
}

__global__ void __launch_bounds__(kReduceThreads)
bits_image_kernel(int batch, long long n, int segments, const float* __restrict__ lik,
                  double* __restrict__ scratch) {
  __shared__ double smem[kReduceThreads / 64];
  const int b = blockIdx.y;
  const long long items = n * segments;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * kReduceThreads + threadIdx.x; i < items;
       i += (long long)gridDim.x * kReduceThreads) {
    const long long seg = i / n, j = i - seg * n;
    acc += (double)image_bits_of(lik[(seg * batch + b) * n + j]);
  }
  const double s = block_sum_f64(acc, smem);
  if (threadIdx.x == 0) scratch[(size_t)b * gridDim.x + blockIdx.x] = s;
}

__global__ void __launch_bounds__(256)
bits_image_final_kernel(int batch, int nblk, const double* __restrict__ scratch,
                        double* __restrict__ bits) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  double s = 0.0;
  for (int k = 0; k < nblk; ++k) s += scratch[(size_t)b * nblk + k];
  bits[b] = s;
}

}  // namespace rgbac

using namespace rgbac;

extern "C" int rgbac_image_bits_blocks(int64_t n_per_image, int segments) {
  if (n_per_image <= 0 || segments <= 0) return 0;
  return bits_blocks((long long)n_per_image * segments);
}

extern "C" int rgbac_image_bits(int batch, int64_t n_per_image, int segments, const float* lik,
                                double* scratch, double* bits, void* stream) {
  RGBAC_REQUIRE(batch > 0 && batch < 65536, "batch");
  RGBAC_REQUIRE(n_per_image > 0 && segments > 0 && segments <= 4096, "shape");
  RGBAC_REQUIRE(lik && scratch && bits, "null pointer");
  const int nblk = bits_blocks((long long)n_per_image * segments);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(bits_image_kernel, dim3(nblk, batch), dim3(kReduceThreads), 0, st, batch,
                     (long long)n_per_image, segments, lik, scratch);
  int rc = check_launch("bits_image_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(bits_image_final_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, batch,
                     nblk, scratch, bits);
  return check_launch("bits_image_final_kernel");
}
