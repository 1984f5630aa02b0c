// Ragged MS-SSIM / masked MS-SSIM: the metric of msssim.hip for a batch of images of different
// sizes that share one canvas (rgbac.anysize: image b is the top-left h_b x w_b of its planes).
// Evaluation only.  Every image is scored as the reference scores it alone
// (metrics/ms_ssim_torch.py:135-194, metrics/masked_ms_ssim_torch.py:181-265): nothing outside
// its rectangle enters its value, whatever the canvas holds there.
//   * per image and level the size is its own: level 0 (h_b, w_b), level l+1 =
//     ((h + 2(h%2) - 2)/2 + 1, (w + 2(w%2) - 2)/2 + 1), F.avg_pool2d(kernel 2, padding (h%2, w%2))
//     of that image (:183-185).  Level l's planes are (B, C, Hc_l, Wc_l), the largest image's
//     size; the host computes all of it and uploads one table of rgbac_ssim_any_desc
//     (levels x B);
//   * ssim_any_tile_kernel: ssim_tile_kernel / masked_ssim_tile_kernel of msssim.hip, the same
//     arithmetic in the same order, with the image's own valid map (h - ws + 1) x (w - ws + 1)
//     as output bound and the plane's row length as stride.  The grid is the largest image's
//     tile count; a block past its image's tiles writes nothing.  Masked: the level's
//     binarisation (mask > 0) and X*m, Y*m (masked_apply_kernel) happen in the patch load;
//   * avgpool2_any_kernel: one launch pools all planes of X and Y (and the mask) of a level.  A
//     tap outside the IMAGE's rectangle contributes 0 -- the bound is the image's, not the
//     plane's: for an odd h the last output row reads row h, padding in the reference, while the
//     plane holds replicated pixels or a taller neighbour's data there.  Outputs outside the
//     image's next-level rectangle are written 0, so every plane is fully defined;
//   * ssim_any_reduce_kernel: one launch for all levels; per (level, image) -- masked: per
//     (level, image, channel) -- that image's own tile partials in tile order, in double
//     (ssim_reduce_kernel / masked_ssim_reduce_kernel).
// The combine step is msssim.hip's (rgbac_msssim_combine / rgbac_masked_msssim_combine).
// No atomics, fixed order: an image's value depends on its own pixels and size only.
#include "common.h"

namespace rgbac {

typedef rgbac_ssim_any_desc AnyDesc;

constexpr int SA_T = 16;         // output tile edge (msssim.hip SS_T)
constexpr int SA_MAXWS = 15;     // largest odd window the LDS patch holds
constexpr int SA_R = SA_T + SA_MAXWS - 1;
constexpr int SA_MAXLEVELS = 8;

template <bool MASKED>
__global__ void __launch_bounds__(256)
ssim_any_tile_kernel(const AnyDesc* __restrict__ descs, int C, int Hc, int Wc, int ws,
                     const float* __restrict__ X, const float* __restrict__ Y,
                     const float* __restrict__ M, const float* __restrict__ win, float C1,
                     float C2, float* __restrict__ partials) {
  __shared__ float sx[SA_R][SA_R + 1];
  __shared__ float sy[SA_R][SA_R + 1];
  __shared__ float sh[5][SA_R][SA_T + 1];
  __shared__ float red[3][4];
  constexpr int NP = MASKED ? 3 : 2;
  const int tile = blockIdx.x;
  const long long plane = blockIdx.y;                 // b * C + c
  const long long b = plane / C;
  const AnyDesc d = descs[b];
  // the image's rectangle, never larger than the plane whatever the table says
  const int H = min(d.h, Hc), W = min(d.w, Wc);
  const int Ho = H - ws + 1, Wo = W - ws + 1;
  if (Ho < 1 || Wo < 1) return;
  const int tiles_x = (Wo + SA_T - 1) / SA_T, tiles_y = (Ho + SA_T - 1) / SA_T;
  if (tile >= tiles_x * tiles_y) return;              // outside this image's tile grid
  const int ty0 = (tile / tiles_x) * SA_T, tx0 = (tile % tiles_x) * SA_T;
  const int R = SA_T + ws - 1;
  const float* xp = X + plane * Hc * Wc;
  const float* yp = Y + plane * Hc * Wc;
  const float* mp = MASKED ? M + b * (long long)Hc * Wc : nullptr;
  const int tid = threadIdx.x;
  for (int i = tid; i < R * R; i += 256) {
    const int r = i / R, c = i - r * R;
    const int gy = ty0 + r, gx = tx0 + c;
    const bool in = gy < H && gx < W;
    float xv = 0.f, yv = 0.f;
    if (in) {
      const long long o = (long long)gy * Wc + gx;
      xv = xp[o];
      yv = yp[o];
      if (MASKED) {
        const float m = mp[o] > 0.f ? 1.f : 0.f;
        xv = xv * m;
        yv = yv * m;
      }
    }
    sx[r][c] = xv;
    sy[r][c] = yv;
  }
  __syncthreads();
  // horizontal pass (conv with win of shape (1, ws)): rows 0..R-1, output columns 0..T-1
  for (int i = tid; i < R * SA_T; i += 256) {
    const int r = i / SA_T, c = i - r * SA_T;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
    for (int k = 0; k < ws; ++k) {
      const float w = win[k];
      const float xv = sx[r][c + k], yv = sy[r][c + k];
      a0 += w * xv;
      a1 += w * yv;
      a2 += w * (xv * xv);
      a3 += w * (yv * yv);
      a4 += w * (xv * yv);
    }
    sh[0][r][c] = a0; sh[1][r][c] = a1; sh[2][r][c] = a2; sh[3][r][c] = a3; sh[4][r][c] = a4;
  }
  __syncthreads();
  const int ty = tid / SA_T, tx = tid - (tid / SA_T) * SA_T;
  float ssim_v = 0.f, cs_v = 0.f, keep = 0.f;
  const int oy = ty0 + ty, ox = tx0 + tx;
  if (oy < Ho && ox < Wo) {
    float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
    for (int k = 0; k < ws; ++k) {
      const float w = win[k];
      m1 += w * sh[0][ty + k][tx];
      m2 += w * sh[1][ty + k][tx];
      e11 += w * sh[2][ty + k][tx];
      e22 += w * sh[3][ty + k][tx];
      e12 += w * sh[4][ty + k][tx];
    }
    const float mu1_sq = m1 * m1, mu2_sq = m2 * m2, mu1_mu2 = m1 * m2;
    const float s11 = e11 - mu1_sq, s22 = e22 - mu2_sq, s12 = e12 - mu1_mu2;
    cs_v = (2.f * s12 + C2) / (s11 + s22 + C2);
    ssim_v = ((2.f * mu1_mu2 + C1) / (mu1_sq + mu2_sq + C1)) * cs_v;
    if (MASKED) {
      // NEAREST resize of the image's (H, W) level mask to its valid map: torch's scale is
      // (float)in / out, source index min(floor(dst * scale), in - 1)
      const float scale_h = (float)H / (float)Ho, scale_w = (float)W / (float)Wo;
      const int sy_ = min((int)floorf((float)oy * scale_h), H - 1);
      const int sx_ = min((int)floorf((float)ox * scale_w), W - 1);
      keep = mp[(long long)sy_ * Wc + sx_] > 0.f ? 1.f : 0.f;
      ssim_v = ssim_v * keep;
      cs_v = cs_v * keep;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    ssim_v += __shfl_xor(ssim_v, o);
    cs_v += __shfl_xor(cs_v, o);
    if (MASKED) keep += __shfl_xor(keep, o);
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = ssim_v; red[1][tid >> 6] = cs_v; red[2][tid >> 6] = keep;
  }
  __syncthreads();
  if (tid == 0) {
    float* out = partials + (plane * gridDim.x + tile) * NP;
    out[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    out[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    if (MASKED) out[2] = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);   // exact: <= 256 ones
  }
}

// One thread per output element of the next level's planes: first the B*C planes of X, then
// those of Y, then (masked) the B mask planes.  din: this level's descriptors (the input
// rectangles); the output rectangle follows from them.
template <bool MASKED>
__global__ void __launch_bounds__(256)
avgpool2_any_kernel(const AnyDesc* __restrict__ din, int B, int C, int Hc, int Wc, int Hco,
                    int Wco, long long nout, const float* __restrict__ x,
                    const float* __restrict__ y, const float* __restrict__ m,
                    float* __restrict__ xo, float* __restrict__ yo, float* __restrict__ mo) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nout) return;
  const long long per = (long long)Hco * Wco;
  const long long BC = (long long)B * C;
  long long plane = i / per;                           // over X planes | Y planes | mask planes
  const int s = (int)(i - plane * per);
  const int oy = s / Wco, ox = s - (s / Wco) * Wco;
  const float* src;
  float* dst;
  long long b;
  bool is_mask = false;
  if (plane < BC) {
    src = x + plane * Hc * Wc; dst = xo + plane * per; b = plane / C;
  } else if (plane < 2 * BC) {
    plane -= BC;
    src = y + plane * Hc * Wc; dst = yo + plane * per; b = plane / C;
  } else {
    plane -= 2 * BC;
    src = m + plane * Hc * Wc; dst = mo + plane * per; b = plane; is_mask = true;
  }
  const AnyDesc d = din[b];
  const int H = min(d.h, Hc), W = min(d.w, Wc);
  const int ph = H % 2, pw = W % 2;
  const int Ho = (H + 2 * ph - 2) / 2 + 1, Wo = (W + 2 * pw - 2) / 2 + 1;
  float acc = 0.f;
  if (oy < Ho && ox < Wo) {
    const float* mp = MASKED ? m + b * (long long)Hc * Wc : nullptr;
    for (int dy = 0; dy < 2; ++dy) {
      const int iy = oy * 2 - ph + dy;
      for (int dx = 0; dx < 2; ++dx) {
        const int ix = ox * 2 - pw + dx;
        // the image's own rectangle: what lies beyond it in the plane is not this image
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
          const long long o = (long long)iy * Wc + ix;
          if (MASKED) {
            const float mv = mp[o] > 0.f ? 1.f : 0.f;
            acc += is_mask ? mv : src[o] * mv;
          } else {
            acc += src[o];
          }
        }
      }
    }
    acc = acc / 4.f;  // count_include_pad: the 2x2 window always lies inside the padded image
  }
  dst[s] = acc;
}

struct AnyLevels {
  long long part_off[SA_MAXLEVELS];   // floats, from the start of the partials scratch
  int max_tiles[SA_MAXLEVELS];        // the level's tile-grid size (largest image)
  int hc[SA_MAXLEVELS], wc[SA_MAXLEVELS];
};

// grid (ceil(units / 64), levels); unit = image (unmasked: sums its C planes, c major as
// ssim_reduce_kernel does) or (image, channel) plane (masked).  out[(level * units) + unit].
template <bool MASKED>
__global__ void __launch_bounds__(64)
ssim_any_reduce_kernel(const AnyDesc* __restrict__ descs, int B, int C, int ws, AnyLevels lv,
                       const float* __restrict__ partials, float* __restrict__ ssim_out,
                       float* __restrict__ cs_out) {
  const int level = blockIdx.y;
  const long long units = MASKED ? (long long)B * C : B;
  const long long u = (long long)blockIdx.x * 64 + threadIdx.x;
  if (u >= units) return;
  const long long b = MASKED ? u / C : u;
  const AnyDesc d = descs[(long long)level * B + b];
  const int H = min(d.h, lv.hc[level]), W = min(d.w, lv.wc[level]);
  const int Ho = H - ws + 1, Wo = W - ws + 1;
  const int mt = lv.max_tiles[level];
  int nt = 0;
  if (Ho >= 1 && Wo >= 1) nt = ((Wo + SA_T - 1) / SA_T) * ((Ho + SA_T - 1) / SA_T);
  if (nt > mt) nt = mt;
  const float* base = partials + lv.part_off[level];
  const long long o = level * units + u;
  if (MASKED) {
    double s = 0.0, c = 0.0, n = 0.0;
    const float* p = base + u * mt * 3;
    for (int i = 0; i < nt; ++i) {
      s += p[3 * i];
      c += p[3 * i + 1];
      n += p[3 * i + 2];
    }
    const float den = (float)n + 1e-10f;
    ssim_out[o] = (float)s / den;
    cs_out[o] = (float)c / den;
  } else {
    double s = 0.0, c = 0.0;
    for (int ch = 0; ch < C; ++ch) {
      const float* p = base + (b * C + ch) * mt * 2;
      for (int i = 0; i < nt; ++i) {
        s += p[2 * i];
        c += p[2 * i + 1];
      }
    }
    const double n = (double)C * ((double)Ho * (double)Wo);
    ssim_out[o] = (float)(s / n);
    cs_out[o] = (float)(c / n);
  }
}

inline int any_tiles(int h, int w, int ws) {
  const int ho = h - ws + 1, wo = w - ws + 1;
  if (ho < 1 || wo < 1) return 0;
  return ((ho + SA_T - 1) / SA_T) * ((wo + SA_T - 1) / SA_T);
}

}  // namespace rgbac

using namespace rgbac;

extern "C" int rgbac_ssim_any_tiles(int h, int w, int win_size) {
  if (win_size < 1) return 0;
  return any_tiles(h, w, win_size);
}

extern "C" int64_t rgbac_ssim_any_partial_floats(int batch, int channels, int max_tiles,
                                                 int masked) {
  if (batch <= 0 || channels <= 0 || max_tiles <= 0) return 0;
  return (int64_t)batch * channels * max_tiles * (masked ? 3 : 2);
}

extern "C" int rgbac_ssim_any_level(int batch, int channels, int hc, int wc, int win_size,
                                    const rgbac_ssim_any_desc* descs, int max_tiles,
                                    const float* x, const float* y, const float* mask,
                                    const float* win, float c1, float c2, float* partials,
                                    void* stream) {
  RGBAC_REQUIRE(batch > 0 && channels > 0 && hc > 0 && wc > 0, "shape");
  RGBAC_REQUIRE(win_size >= 1 && win_size <= SA_MAXWS && (win_size & 1), "window size");
  RGBAC_REQUIRE(hc >= win_size && wc >= win_size, "plane smaller than the window");
  RGBAC_REQUIRE(descs && x && y && win && partials, "null pointer");
  RGBAC_REQUIRE(max_tiles >= 1 && max_tiles <= any_tiles(hc, wc, win_size),
                "max_tiles: 1 .. the plane's own tile count");
  RGBAC_REQUIRE((long long)batch * channels <= 65535, "too many planes for one launch");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (mask) {
    hipLaunchKernelGGL(ssim_any_tile_kernel<true>, dim3(max_tiles, batch * channels), dim3(256),
                       0, st, descs, channels, hc, wc, win_size, x, y, mask, win, c1, c2,
                       partials);
  } else {
    hipLaunchKernelGGL(ssim_any_tile_kernel<false>, dim3(max_tiles, batch * channels), dim3(256),
                       0, st, descs, channels, hc, wc, win_size, x, y, mask, win, c1, c2,
                       partials);
  }
  return check_launch("ssim_any_tile_kernel");
}

extern "C" int rgbac_avgpool2_any(int batch, int channels, int hc, int wc, int hc_out, int wc_out,
                                  const rgbac_ssim_any_desc* descs, const float* x,
                                  const float* y, const float* mask, float* x_out, float* y_out,
                                  float* mask_out, void* stream) {
  RGBAC_REQUIRE(batch > 0 && channels > 0 && hc > 0 && wc > 0, "shape");
  // the largest image decides the next level's planes; none of its outputs may fall outside
  RGBAC_REQUIRE(hc_out >= 1 && wc_out >= 1 && hc_out <= (hc + 2 * (hc % 2) - 2) / 2 + 1 &&
                    wc_out <= (wc + 2 * (wc % 2) - 2) / 2 + 1,
                "output plane larger than the pooled input plane");
  RGBAC_REQUIRE(descs && x && y && x_out && y_out, "null pointer");
  RGBAC_REQUIRE((mask == nullptr) == (mask_out == nullptr), "mask and mask_out go together");
  const long long planes = 2LL * batch * channels + (mask ? batch : 0);
  const long long n = planes * hc_out * wc_out;
  RGBAC_REQUIRE((n + 255) / 256 <= 0x7fffffffLL, "too many elements for one launch");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (mask) {
    hipLaunchKernelGGL(avgpool2_any_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       st, descs, batch, channels, hc, wc, hc_out, wc_out, n, x, y, mask, x_out,
                       y_out, mask_out);
  } else {
    hipLaunchKernelGGL(avgpool2_any_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       st, descs, batch, channels, hc, wc, hc_out, wc_out, n, x, y, mask, x_out,
                       y_out, mask_out);
  }
  return check_launch("avgpool2_any_kernel");
}

extern "C" int rgbac_ssim_any_reduce(int levels, int batch, int channels, int win_size, int masked,
                                     const rgbac_ssim_any_desc* descs, const int32_t* plane_h,
                                     const int32_t* plane_w, const int32_t* max_tiles,
                                     const int64_t* partial_offsets, int64_t partial_floats,
                                     const float* partials, float* ssim_out, float* cs_out,
                                     void* stream) {
  RGBAC_REQUIRE(levels >= 1 && levels <= SA_MAXLEVELS, "levels: 1 .. 8");
  RGBAC_REQUIRE(batch > 0 && channels > 0, "shape");
  RGBAC_REQUIRE(win_size >= 1 && win_size <= SA_MAXWS && (win_size & 1), "window size");
  RGBAC_REQUIRE(descs && plane_h && plane_w && max_tiles && partial_offsets && partials &&
                    ssim_out && cs_out, "null pointer");
  AnyLevels lv = {};
  const int np = masked ? 3 : 2;
  for (int l = 0; l < levels; ++l) {
    RGBAC_REQUIRE(plane_h[l] > 0 && plane_w[l] > 0 && max_tiles[l] >= 1, "level geometry");
    const int64_t need = (int64_t)batch * channels * max_tiles[l] * np;
    RGBAC_REQUIRE(partial_offsets[l] >= 0 && partial_offsets[l] + need <= partial_floats,
                  "a level's partials lie outside the scratch");
    lv.part_off[l] = partial_offsets[l];
    lv.max_tiles[l] = max_tiles[l];
    lv.hc[l] = plane_h[l];
    lv.wc[l] = plane_w[l];
  }
  const long long units = masked ? (long long)batch * channels : batch;
  const dim3 grid((unsigned)((units + 63) / 64), levels);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (masked) {
    hipLaunchKernelGGL(ssim_any_reduce_kernel<true>, grid, dim3(64), 0, st, descs, batch, channels,
                       win_size, lv, partials, ssim_out, cs_out);
  } else {
    hipLaunchKernelGGL(ssim_any_reduce_kernel<false>, grid, dim3(64), 0, st, descs, batch,
                       channels, win_size, lv, partials, ssim_out, cs_out);
  }
  return check_launch("ssim_any_reduce_kernel");
}
