// Backward of the MS-SSIM / SSIM metric kernels of msssim.hip (plain and masked), so that
// 1 - ms_ssim(x, x_hat) can be the training distortion (trainRGB.py:183).  fp32, no atomics,
// fixed summation order: the gradient is bit-reproducible from run to run.
//   * ssim_bwd_tile_kernel: one workgroup owns a 16x16 tile of INPUT pixels q of one
//     (image, channel) plane and writes dY there (and dX when asked).  Gather form:
//       1. the X / Y patch with a halo of 2*(ws-1) is staged in LDS (zero outside the image);
//       2. the five separable-gaussian statistics m1, m2, e11, e22, e12 are recomputed at every
//          valid-map position p whose window touches the tile ((T+ws-1)^2 of them);
//       3. the upstream scalars become adjoint maps at p.  With
//            l = (2 m1 m2 + C1) / B1,  B1 = m1^2 + m2^2 + C1,
//            cs = (2 s12 + C2) / B2,   B2 = s11 + s22 + C2,   ssim = l * cs,
//            D_cs = u_cs + u_ssim * l,  D_l = u_ssim * cs:
//            a_e12 = 2 D_cs / B2,   a_e11 = a_e22 = -D_cs cs / B2  (one plane, a_e),
//            a_m2 = D_l (2 m1 - 2 l m2) / B1 - m1 a_e12 - 2 m2 a_e,   a_m1 symmetric;
//          positions outside [0, Ho) x [0, Wo) contribute nothing;
//       4. the transposed separable gaussian carries the adjoint maps back onto the tile;
//       5. dY(q) = Gt a_m2 + 2 Y(q) Gt a_e + X(q) Gt a_e12  (dX symmetric).
//     Upstream scalars: plain, per image, u = g[b] / (C Ho Wo); masked, per plane,
//     u = keep(p) g[b, c] / (count[b, c] + 1e-10) with the forward's NEAREST-resized level mask
//     (the index rule of masked_ssim_tile_kernel) and the count summed from the forward's tile
//     partials (integers, summed in double: the forward's value in any order).
//     The adjoint of avgpool2_kernel is fused in: with the next-coarser level's gradient gc,
//     dY(q) += gc[(qy + ph) / 2][(qx + pw) / 2] / 4 (ph = H % 2, pw = W % 2 -- every input
//     pixel feeds exactly one pooled pixel), so the backward is one launch per level, coarse to
//     fine, and no pooled-gradient plane makes a round trip through HBM.  In the masked
//     ms_ssim the sum is multiplied by the level's binary mask (adjoint of masked_apply_kernel).
//   * msssim_combine_bwd_kernel / masked_msssim_combine_bwd_kernel: d(value) / d(cs_l, ssim_last)
//     times the incoming gradient -> u[l][.] (rows l < L-1: u_cs of level l; row L-1: u_ssim of
//     the last level).  The plain form differentiates exactly prod_{l<L-1} (cs_l^w_l *
//     ssim^w_last), the reference's broadcast included.  The masked form carries the relu
//     gates: where a clamped factor is 0 the whole plane's gradient is 0 (torch autograd gives
//     0 * inf = NaN there; that is not reproduced).
// LDS per workgroup, sized for the launch's window (dynamic): at ws = 15 with dX, 2 patch planes
// 44x45, 5 horizontal planes 44x31, 4 adjoint planes 30x31 = 58000 B; at ws = 11, dY only,
// 38520 B (the transposed-pass planes reuse the horizontal ones).
#include "common.h"

namespace rgbac {

constexpr int SB_T = 16;                          // input tile edge
constexpr int SB_MAXWS = 15;                      // as the forward's SS_MAXWS
constexpr int SB_TS = SB_T + 1;                   // padded row stride of the tile-wide planes
// LDS floats of one workgroup at window ws with na adjoint planes (3: dY only, 4: dX too).  The
// planes are laid out for the launch's own ws (row strides edge + 1), not for SB_MAXWS: at
// ws = 11 / dY only that is 38.5 KB instead of 58 KB, so four workgroups share a CU's LDS.
constexpr int sb_lds_floats(int ws, int na) {
  const int pa = SB_T + 2 * (ws - 1), ra = SB_T + ws - 1;
  return 2 * pa * (pa + 1) + 5 * pa * (ra + 1) + na * ra * (ra + 1);
}
static_assert(sb_lds_floats(SB_MAXWS, 4) * 4 + 256 <= 65536, "LDS above 64 KiB");
// the transposed-pass planes (na x ra x SB_TS) reuse the horizontal ones (5 x pa x (ra + 1)):
// na * SB_TS = 68 <= 5 * pa for every pa >= SB_T
static_assert(4 * SB_TS <= 5 * SB_T, "transposed-pass planes must fit the reuse");

template <bool MASKED, bool DX>
__global__ void __launch_bounds__(256)
ssim_bwd_tile_kernel(int C, int Cm, int H, int W, int ws, const float* __restrict__ X,
                     const float* __restrict__ Y, const float* __restrict__ M,
                     const float* __restrict__ win, float C1, float C2,
                     const float* __restrict__ u_cs, const float* __restrict__ u_ssim,
                     float inv_n, const float* __restrict__ partials, int fwd_ntiles,
                     float scale_h, float scale_w, int apply_mask,
                     const float* __restrict__ gcx, const float* __restrict__ gcy, int Hc, int Wc,
                     int tiles_x, float* __restrict__ dX, float* __restrict__ dY) {
  extern __shared__ float lds[];         // sb_lds_floats(ws, DX ? 4 : 3)
  __shared__ float sw[SB_MAXWS + 1];
  __shared__ double dsm[4];
  __shared__ float sden;
  const int tile = blockIdx.x;
  const long long plane = blockIdx.y;    // b * C + c
  const long long b = plane / C;
  const int c = (int)(plane - b * C);
  const int qy0 = (tile / tiles_x) * SB_T, qx0 = (tile % tiles_x) * SB_T;
  const int Pa = SB_T + 2 * (ws - 1), Ra = SB_T + ws - 1;
  const int PS = Pa + 1, RS = Ra + 1;    // padded row strides
  const int HP = Pa * RS, AP = Ra * RS, TP = Ra * SB_TS;   // plane strides of sh, sa, st
  float* sx = lds;                       // [Pa][PS]
  float* sy = sx + Pa * PS;              // [Pa][PS]
  float* sh = sy + Pa * PS;              // [5][Pa][RS]
  float* sa = sh + 5 * HP;               // [3 or 4][Ra][RS]: a_m2, a_e, a_e12, a_m1
  float* st = sh;                        // [3 or 4][Ra][SB_TS], after the statistics are consumed
  const int Ho = H - ws + 1, Wo = W - ws + 1;
  const int oy = qy0 - (ws - 1), ox = qx0 - (ws - 1);     // image position of patch (0, 0)
  const float* xp = X + plane * H * W;
  const float* yp = Y + plane * H * W;
  const float* mp = MASKED ? M + (b * Cm + (Cm == 1 ? 0 : c)) * (long long)H * W : nullptr;
  const int tid = threadIdx.x;

  if (tid < ws) sw[tid] = win[tid];
  for (int i = tid; i < Pa * Pa; i += 256) {
    const int r = i / Pa, cc = i - r * Pa;
    const int gy = oy + r, gx = ox + cc;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    sx[r * PS + cc] = in ? xp[(long long)gy * W + gx] : 0.f;
    sy[r * PS + cc] = in ? yp[(long long)gy * W + gx] : 0.f;
  }
  // upstream scalars of this plane
  float ucs, uss;
  if (MASKED) {
    double n = 0.0;
    const float* pp = partials + plane * fwd_ntiles * 3 + 2;
    for (int i = tid; i < fwd_ntiles; i += 256) n += (double)pp[3 * i];
    n = block_sum_f64(n, dsm);                       // exact: integer counts
    if (tid == 0) sden = (float)n + 1e-10f;
    __syncthreads();
    const float den = sden;
    ucs = u_cs ? u_cs[plane] / den : 0.f;
    uss = u_ssim ? u_ssim[plane] / den : 0.f;
  } else {
    __syncthreads();
    ucs = u_cs ? u_cs[b] * inv_n : 0.f;
    uss = u_ssim ? u_ssim[b] * inv_n : 0.f;
  }
  // horizontal pass of the statistics: patch rows 0..Pa-1, positions 0..Ra-1
  for (int i = tid; i < Pa * Ra; i += 256) {
    const int r = i / Ra, j = i - r * Ra;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
    for (int k = 0; k < ws; ++k) {
      const float w = sw[k];
      const float xv = sx[r * PS + j + k], yv = sy[r * PS + j + k];
      a0 += w * xv;
      a1 += w * yv;
      a2 += w * (xv * xv);
      a3 += w * (yv * yv);
      a4 += w * (xv * yv);
    }
    float* o = sh + r * RS + j;
    o[0] = a0; o[HP] = a1; o[2 * HP] = a2; o[3 * HP] = a3;
    o[4 * HP] = a4;
  }
  __syncthreads();
  // vertical pass -> statistics at position (pi, pj) -> adjoint maps
  for (int i = tid; i < Ra * Ra; i += 256) {
    const int pi = i / Ra, pj = i - pi * Ra;
    const int py = oy + pi, px = ox + pj;
    float am1 = 0.f, am2 = 0.f, ae = 0.f, ae12 = 0.f;
    if (py >= 0 && py < Ho && px >= 0 && px < Wo) {
      float keep = 1.f;
      if (MASKED) {
        const int sy_ = min((int)floorf((float)py * scale_h), H - 1);
        const int sx_ = min((int)floorf((float)px * scale_w), W - 1);
        keep = mp[(long long)sy_ * W + sx_] != 0.f ? 1.f : 0.f;
      }
      if (keep != 0.f) {
        float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
        const float* h = sh + pi * RS + pj;
        for (int k = 0; k < ws; ++k) {
          const float w = sw[k];
          m1 += w * h[k * RS];
          m2 += w * h[HP + k * RS];
          e11 += w * h[2 * HP + k * RS];
          e22 += w * h[3 * HP + k * RS];
          e12 += w * h[4 * HP + k * RS];
        }
        const float mu1_sq = m1 * m1, mu2_sq = m2 * m2, mu1_mu2 = m1 * m2;
        const float s11 = e11 - mu1_sq, s22 = e22 - mu2_sq, s12 = e12 - mu1_mu2;
        const float B1 = mu1_sq + mu2_sq + C1, B2 = s11 + s22 + C2;
        const float l = (2.f * mu1_mu2 + C1) / B1;
        const float cs = (2.f * s12 + C2) / B2;
        const float Dcs = ucs + uss * l, Dl = uss * cs;
        ae12 = 2.f * Dcs / B2;
        ae = -Dcs * cs / B2;
        am2 = Dl * (2.f * m1 - 2.f * l * m2) / B1 - m1 * ae12 - 2.f * m2 * ae;
        if (DX) am1 = Dl * (2.f * m2 - 2.f * l * m1) / B1 - m2 * ae12 - 2.f * m1 * ae;
      }
    }
    float* o = sa + pi * RS + pj;
    o[0] = am2; o[AP] = ae; o[2 * AP] = ae12;
    if (DX) o[3 * AP] = am1;
  }
  __syncthreads();
  // transposed horizontal pass: position rows 0..Ra-1, tile columns 0..T-1 (p = q - k)
  for (int i = tid; i < Ra * SB_T; i += 256) {
    const int pi = i / SB_T, t = i - pi * SB_T;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    const float* a = sa + pi * RS + t + ws - 1;
    for (int k = 0; k < ws; ++k) {
      const float w = sw[k];
      a0 += w * a[-k];
      a1 += w * a[AP - k];
      a2 += w * a[2 * AP - k];
      if (DX) a3 += w * a[3 * AP - k];
    }
    float* o = st + pi * SB_TS + t;
    o[0] = a0; o[TP] = a1; o[2 * TP] = a2;
    if (DX) o[3 * TP] = a3;
  }
  __syncthreads();
  const int ty = tid / SB_T, tx = tid - ty * SB_T;
  const int qy = qy0 + ty, qx = qx0 + tx;
  if (qy >= H || qx >= W) return;
  float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
  const float* a = st + (ty + ws - 1) * SB_TS + tx;
  for (int k = 0; k < ws; ++k) {
    const float w = sw[k];
    g0 += w * a[-k * SB_TS];
    g1 += w * a[TP - k * SB_TS];
    g2 += w * a[2 * TP - k * SB_TS];
    if (DX) g3 += w * a[3 * TP - k * SB_TS];
  }
  const float xv = sx[(ty + ws - 1) * PS + tx + ws - 1];
  const float yv = sy[(ty + ws - 1) * PS + tx + ws - 1];
  const long long q = plane * H * W + (long long)qy * W + qx;
  const long long qc = plane * Hc * Wc + (long long)((qy + (H & 1)) >> 1) * Wc + ((qx + (W & 1)) >> 1);
  bool on = true;
  if (MASKED && apply_mask) on = mp[(long long)qy * W + qx] != 0.f;
  if (dY) {
    float v = g0 + 2.f * yv * g1 + xv * g2;
    if (gcy) v += gcy[qc] * 0.25f;
    dY[q] = on ? v : 0.f;
  }
  if (DX) {
    float v = g3 + 2.f * xv * g1 + yv * g2;
    if (gcx) v += gcx[qc] * 0.25f;
    dX[q] = on ? v : 0.f;
  }
}

// u[l][b], l < L-1: d/d cs_l;  u[L-1][b]: d/d ssim_last, of
// val[b] = prod_{l<L-1} cs_l^w_l * ssim^(w_last (L-1)), times the incoming gradient.
__global__ void __launch_bounds__(64)
msssim_combine_bwd_kernel(int levels, int B, const float* __restrict__ mcs,
                          const float* __restrict__ ssim_last, const float* __restrict__ weights,
                          const float* __restrict__ grad, int grad_is_mean,
                          float* __restrict__ u) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const float g = grad_is_mean ? grad[0] / (float)B : grad[b];
  const int n = levels - 1;
  const float wl = weights[n], s = ssim_last[b];
  float tail = 1.f;                                  // ssim^(w_last (L-1))
  const float t1 = powf(s, wl);
  for (int l = 0; l < n; ++l) tail *= t1;
  float all = 1.f;
  for (int l = 0; l < n; ++l) all *= powf(mcs[(long long)l * B + b], weights[l]);
  for (int l = 0; l < n; ++l) {
    float v = weights[l] * powf(mcs[(long long)l * B + b], weights[l] - 1.f);
    for (int j = 0; j < n; ++j)
      if (j != l) v *= powf(mcs[(long long)j * B + b], weights[j]);
    u[(long long)l * B + b] = g * v * tail;
  }
  // d tail / d s = (L-1) t1^(L-2) * w_last s^(w_last - 1)
  float dt = 0.f;
  if (n > 0) {
    dt = (float)n * wl * powf(s, wl - 1.f);
    for (int l = 0; l < n - 1; ++l) dt *= t1;
  }
  u[(long long)n * B + b] = g * all * dt;
}

// per plane k = (b, c): val = prod_l relu(v_l)^w_l with v_l = cs_l (l < L-1), ssim_last (L-1).
__global__ void __launch_bounds__(64)
masked_msssim_combine_bwd_kernel(int levels, int B, int C, const float* __restrict__ mcs,
                                 const float* __restrict__ ssim_last,
                                 const float* __restrict__ weights,
                                 const float* __restrict__ grad, int grad_is_mean,
                                 float* __restrict__ u) {
  const long long BC = (long long)B * C;
  const long long k = (long long)blockIdx.x * 64 + threadIdx.x;
  if (k >= BC) return;
  const float g = grad_is_mean ? grad[0] / (float)BC : grad[k / C] / (float)C;
  bool dead = false;                                 // a factor clamped to 0 with a weight > 0
  for (int l = 0; l < levels; ++l) {
    const float v = l < levels - 1 ? mcs[l * BC + k] : ssim_last[k];
    if (!(v > 0.f) && weights[l] > 0.f) dead = true;
  }
  for (int l = 0; l < levels; ++l) {
    const float vl = l < levels - 1 ? mcs[l * BC + k] : ssim_last[k];
    float d = 0.f;
    if (!dead && vl > 0.f) {
      d = weights[l] * powf(vl, weights[l] - 1.f);
      for (int j = 0; j < levels; ++j) {
        if (j == l) continue;
        const float vj = j < levels - 1 ? mcs[j * BC + k] : ssim_last[k];
        d *= powf(fmaxf(vj, 0.f), weights[j]);
      }
    }
    u[l * BC + k] = g * d;
  }
}

}  // namespace rgbac

using namespace rgbac;

namespace {

template <bool MASKED>
int launch_level_bwd(int batch, int channels, int mask_channels, int h, int w, int win_size,
                     const float* x, const float* y, const float* mask, const float* win,
                     float c1, float c2, const float* partials, const float* u_cs,
                     const float* u_ssim, int apply_mask, const float* gc_x, const float* gc_y,
                     float* dx, float* dy, void* stream) {
  const int ho = h - win_size + 1, wo = w - win_size + 1;
  const int tiles_x = (w + SB_T - 1) / SB_T, tiles_y = (h + SB_T - 1) / SB_T;
  const int ntiles = tiles_x * tiles_y;
  const int fwd_ntiles = ((wo + SB_T - 1) / SB_T) * ((ho + SB_T - 1) / SB_T);
  const int ph = h % 2, pw = w % 2;
  const int hc = (h + 2 * ph - 2) / 2 + 1, wc = (w + 2 * pw - 2) / 2 + 1;
  const float inv_n = (float)(1.0 / ((double)channels * (double)ho * (double)wo));
  const float scale_h = (float)h / (float)ho, scale_w = (float)w / (float)wo;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(ntiles, batch * channels), block(256);
  const size_t lds = sizeof(float) * sb_lds_floats(win_size, dx ? 4 : 3);
  if (dx)
    hipLaunchKernelGGL((ssim_bwd_tile_kernel<MASKED, true>), grid, block, lds, st, channels,
                       mask_channels, h, w, win_size, x, y, mask, win, c1, c2, u_cs, u_ssim,
                       inv_n, partials, fwd_ntiles, scale_h, scale_w, apply_mask, gc_x, gc_y, hc,
                       wc, tiles_x, dx, dy);
  else
    hipLaunchKernelGGL((ssim_bwd_tile_kernel<MASKED, false>), grid, block, lds, st, channels,
                       mask_channels, h, w, win_size, x, y, mask, win, c1, c2, u_cs, u_ssim,
                       inv_n, partials, fwd_ntiles, scale_h, scale_w, apply_mask, gc_x, gc_y, hc,
                       wc, tiles_x, dx, dy);
  return check_launch("ssim_bwd_tile_kernel");
}

}  // namespace

extern "C" int rgbac_ssim_level_bwd(int batch, int channels, int h, int w, int win_size,
                                    const float* x, const float* y, const float* win, float c1,
                                    float c2, const float* u_cs, const float* u_ssim,
                                    const float* gc_x, const float* gc_y, float* dx, float* dy,
                                    void* stream) {
  RGBAC_REQUIRE(batch > 0 && channels > 0, "shape");
  RGBAC_REQUIRE(win_size >= 1 && win_size <= SB_MAXWS && (win_size & 1), "window size");
  RGBAC_REQUIRE(h >= win_size && w >= win_size, "image smaller than the window");
  RGBAC_REQUIRE(x && y && win && (dx || dy), "null pointer");
  RGBAC_REQUIRE((long long)batch * channels <= 65535, "too many planes for one launch");
  return launch_level_bwd<false>(batch, channels, 1, h, w, win_size, x, y, nullptr, win, c1, c2,
                                 nullptr, u_cs, u_ssim, 0, gc_x, gc_y, dx, dy, stream);
}

extern "C" int rgbac_masked_ssim_level_bwd(int batch, int channels, int mask_channels, int h,
                                           int w, int win_size, const float* x, const float* y,
                                           const float* mask, const float* win, float c1,
                                           float c2, const float* partials, const float* u_cs,
                                           const float* u_ssim, int apply_mask,
                                           const float* gc_x, const float* gc_y, float* dx,
                                           float* dy, void* stream) {
  RGBAC_REQUIRE(batch > 0 && channels > 0, "shape");
  RGBAC_REQUIRE(mask_channels == 1 || mask_channels == channels, "mask channels: 1 or C");
  RGBAC_REQUIRE(win_size >= 1 && win_size <= SB_MAXWS && (win_size & 1), "window size");
  RGBAC_REQUIRE(h >= win_size && w >= win_size, "image smaller than the window");
  RGBAC_REQUIRE(x && y && mask && win && partials && (dx || dy), "null pointer");
  RGBAC_REQUIRE((long long)batch * channels <= 65535, "too many planes for one launch");
  return launch_level_bwd<true>(batch, channels, mask_channels, h, w, win_size, x, y, mask, win,
                                c1, c2, partials, u_cs, u_ssim, apply_mask, gc_x, gc_y, dx, dy,
                                stream);
}

extern "C" int rgbac_msssim_combine_bwd(int levels, int batch, const float* mcs,
                                        const float* ssim_last, const float* weights,
                                        const float* grad, int grad_is_mean, float* u,
                                        void* stream) {
  RGBAC_REQUIRE(levels >= 1 && batch > 0, "arguments");
  RGBAC_REQUIRE(mcs && ssim_last && weights && grad && u, "null pointer");
  hipLaunchKernelGGL(msssim_combine_bwd_kernel, dim3((batch + 63) / 64), dim3(64), 0,
                     reinterpret_cast<hipStream_t>(stream), levels, batch, mcs, ssim_last,
                     weights, grad, grad_is_mean, u);
  return check_launch("msssim_combine_bwd_kernel");
}

extern "C" int rgbac_masked_msssim_combine_bwd(int levels, int batch, int channels,
                                               const float* mcs, const float* ssim_last,
                                               const float* weights, const float* grad,
                                               int grad_is_mean, float* u, void* stream) {
  RGBAC_REQUIRE(levels >= 1 && batch > 0 && channels > 0, "arguments");
  RGBAC_REQUIRE((levels == 1 || mcs) && ssim_last && weights && grad && u, "null pointer");
  const long long planes = (long long)batch * channels;
  hipLaunchKernelGGL(masked_msssim_combine_bwd_kernel, dim3((unsigned)((planes + 63) / 64)),
                     dim3(64), 0, reinterpret_cast<hipStream_t>(stream), levels, batch, channels,
                     mcs, ssim_last, weights, grad, grad_is_mean, u);
  return check_launch("masked_msssim_combine_bwd_kernel");
}
