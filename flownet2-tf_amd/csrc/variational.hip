// EpicFlow variational refinement (the reference's src/SrcVariational, called through utils.py:542-555
// calc_variational_inference_map): one pyramid level of energy minimisation started from a given flow.
//   variational()            variational.c:101-142   -> fn2_variational_refine
//   compute_one_level()      variational.c:19-82     -> the outer / inner loop in fn2_variational_refine
//   color_image_convolve_hv  image.c:461-491 with gaussian_filter (image.c:116-154)  -> var_smooth_h / var_smooth_v
//   compute_dpsis_weight     variational_aux.c:237-266  -> var_dpsis
//   image_warp               variational_aux.c:18-48    -> var_warp (with the mean / difference of get_derivatives)
//   get_derivatives          variational_aux.c:51-74    -> var_deriv1 (Ix, Iy) + var_system (second order)
//   compute_smoothness, compute_data_and_match, sub_laplacian (variational_aux.c:81-318)  -> var_system
//   sor_coupled              solver.c:57-399            -> var_sor (wavefront form of the lexicographic sweep)
//
// Every image is planar fp32 of the pair's own size (no stride padding: the reference's padding never reaches a
// real pixel).  The SOR system lives in a SKEWED layout, element (row j, column i) at [(i + j) * H + j]: at each
// wavefront step the lanes of a wave (consecutive rows) touch consecutive addresses.  Arithmetic is written in the
// reference's operation order with contraction off, so the per-pixel terms round as the SSE code does.
#include "fn2_common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace fn2 {
namespace {

constexpr int VAR_MAX_ORDER = 32;   // Gaussian half-width bound (the entry point takes sigma < 31 / 3)
constexpr int VAR_BLOCK = 256;

struct GaussTaps {
  int order;
  float c[2 * VAR_MAX_ORDER + 1];   // full filter, centre at [order]
  float a[2 * VAR_MAX_ORDER + 1];   // accumulated coefficients (convolve_extract_coeffs, image.c:157-179)
};

// 5-tap derivative (variational.c:117-118) and flow derivative (:119-120) as convolution_new lays them out
// (anti-symmetric: coeffs[order - i] = half[i], then coeffs[order + i] = -half[i], so the centre tap is -0).
__constant__ float kD5[5] = {1.0f / 12.0f, -8.0f / 12.0f, -0.0f, 8.0f / 12.0f, -(1.0f / 12.0f)};
__constant__ float kD3[3] = {-0.5f, -0.0f, 0.5f};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Horizontal convolve_horiz_fast_3/5 (image.c:266-332): replicated borders, taps summed left to right.
template <int O, class F>
__device__ __forceinline__ float hconv_fast(F f, int x, int W, const float* c) {
  float s = c[0] * f(clampi(x - O, 0, W - 1));
#pragma unroll
  for (int k = 1; k <= 2 * O; ++k) s = s + c[k] * f(clampi(x - O + k, 0, W - 1));
  return s;
}

// Vertical convolve_vert_fast_3/5 (image.c:206-264): the taps that fall on the same (clamped) border row are summed
// first, then each row's product is added top to bottom.
template <int O, class F>
__device__ __forceinline__ float vconv_fast(F f, int y, int H, const float* c) {
  int r = clampi(y - O, 0, H - 1);
  float cc = c[0], s = 0.0f;
  bool first = true;
#pragma unroll
  for (int k = 1; k <= 2 * O; ++k) {
    const int rk = clampi(y - O + k, 0, H - 1);
    if (rk == r) {
      cc = cc + c[k];
    } else {
      const float p = cc * f(r);
      s = first ? p : s + p;
      first = false;
      r = rk;
      cc = c[k];
    }
  }
  const float p = cc * f(r);
  return first ? p : s + p;
}

// Generic convolve_horiz (image.c:343-381) for a Gaussian of order >= 3 and W >= 2 * order + 1, in its summation
// order; other sizes fall back to the replicated-border sum.
template <class F>
__device__ float hconv_gauss(F f, int x, int W, const GaussTaps& g) {
  const int o = g.order;
  const float* c = g.c + o;
  const float* a = g.a + o;
  if (o <= 2 || W < 2 * o + 1) {
    float s = 0.0f;
    for (int k = -o; k <= o; ++k) s = s + c[k] * f(clampi(x + k, 0, W - 1));
    return s;
  }
  float s;
  if (x < o) {
    s = a[-x - 1] * f(0);
    for (int ii = o + x; ii >= 0; --ii) s = s + c[ii - x] * f(ii);
  } else if (x < W - o) {
    s = 0.0f;
    for (int ii = 2 * o; ii >= 0; --ii) s = s + c[ii - o] * f(x - o + ii);
  } else {
    s = a[W - x] * f(W - 1);
    for (int ii = W + o - 1 - x; ii >= 0; --ii) s = s + c[ii - o] * f(x - o + ii);
  }
  return s;
}

// Generic convolve_vert (image.c:393-448), same conditions.
template <class F>
__device__ float vconv_gauss(F f, int y, int H, const GaussTaps& g) {
  const int o = g.order;
  const float* c = g.c + o;
  const float* a = g.a + o;
  if (o <= 2 || H < 2 * o + 1) {
    float s = 0.0f;
    for (int k = -o; k <= o; ++k) s = s + c[k] * f(clampi(y + k, 0, H - 1));
    return s;
  }
  float s;
  if (y < o) {
    s = a[-y - 1] * f(0);
    for (int ii = -y; ii <= o; ++ii) s = s + c[ii] * f(y + ii);
  } else if (y < H - o) {
    s = 0.0f;
    for (int ii = 0; ii <= 2 * o; ++ii) s = s + c[ii - o] * f(y - o + ii);
  } else {
    s = a[H - y] * f(H - 1);
    for (int ii = -o; ii <= H - 1 - y; ++ii) s = s + c[ii] * f(y + ii);
  }
  return s;
}

// ---------------------------------------------------------------------------------------------- presmoothing
// Horizontal Gaussian pass of both frames (uint8 NHWC with row pitch / batch stride, read in place) into planar fp32.
// grid (pixels / VAR_BLOCK, n, 2): z selects the frame.
__global__ void __launch_bounds__(VAR_BLOCK) var_smooth_h(const uint8_t* __restrict__ img_a,
                                                          const uint8_t* __restrict__ img_b, int64_t pitch,
                                                          int64_t bstride, float* __restrict__ tmp, int H, int W,
                                                          GaussTaps g) {
  const int64_t P = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * VAR_BLOCK + threadIdx.x;
  if (p >= P) return;
  const int y = (int)(p / W), x = (int)(p % W);
  const int n = blockIdx.y, img = blockIdx.z;
  const uint8_t* row = (img ? img_b : img_a) + n * bstride + y * pitch;
  float* out = tmp + ((int64_t)(2 * n + img) * 3) * P + p;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    auto f = [&](int xx) { return (float)row[3 * xx + ch]; };
    out[ch * P] = hconv_gauss(f, x, W, g);
  }
}

// Vertical Gaussian pass: tmp -> smoothed frames sm[n][img][3][P].
__global__ void __launch_bounds__(VAR_BLOCK) var_smooth_v(const float* __restrict__ tmp, float* __restrict__ sm,
                                                          int H, int W, GaussTaps g) {
  const int64_t P = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * VAR_BLOCK + threadIdx.x;
  if (p >= P) return;
  const int y = (int)(p / W), x = (int)(p % W);
  const int64_t plane = (int64_t)(2 * blockIdx.y + blockIdx.z) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float* col = tmp + (plane + ch) * P + x;
    auto f = [&](int yy) { return col[(int64_t)yy * W]; };
    sm[(plane + ch) * P + p] = vconv_gauss(f, y, H, g);
  }
}

// compute_dpsis_weight (variational_aux.c:237-266) on the smoothed first frame: 0.5 exp(-5 |grad lum|).
__global__ void __launch_bounds__(VAR_BLOCK) var_dpsis(const float* __restrict__ sm, float* __restrict__ dpsis,
                                                       int H, int W) {
  const int64_t P = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * VAR_BLOCK + threadIdx.x;
  if (p >= P) return;
  const int y = (int)(p / W), x = (int)(p % W);
  const float* im = sm + (int64_t)blockIdx.y * 6 * P;
  auto lum = [&](int yy, int xx) {
    const int64_t q = (int64_t)yy * W + xx;
    return (0.299f * im[q] + 0.587f * im[P + q] + 0.114f * im[2 * P + q]) / 255.0f;
  };
  const float lx = hconv_fast<2>([&](int xx) { return lum(y, xx); }, x, W, kD5);
  const float ly = vconv_fast<2>([&](int yy) { return lum(yy, x); }, y, H, kD5);
  const float e = -5.0f * sqrtf(lx * lx + ly * ly);
  dpsis[(int64_t)blockIdx.y * P + p] = 0.5f * expf(e);
}

// ---------------------------------------------------------------------------------------------- per outer iteration
// image_warp of the smoothed second frame by the current flow (RECTIFY clamp, in-image mask), then the mean with the
// first frame and the temporal difference of get_derivatives.  ws planes per pair: avg[3], dt[3], mask.
__global__ void __launch_bounds__(VAR_BLOCK) var_warp(const float* __restrict__ flow, int64_t fpitch,
                                                      int64_t fbstride, const float* __restrict__ sm,
                                                      float* __restrict__ avg, float* __restrict__ dt,
                                                      float* __restrict__ mask, int H, int W) {
  const int64_t P = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * VAR_BLOCK + threadIdx.x;
  if (p >= P) return;
  const int j = (int)(p / W), i = (int)(p % W);
  const int n = blockIdx.y;
  const float* fl = flow + n * fbstride + j * fpitch + 2 * i;
  const float* im1 = sm + (int64_t)n * 6 * P;
  const float* im2 = im1 + 3 * P;
  const float xx = i + fl[0], yy = j + fl[1];
  const int x = (int)floorf(xx), y = (int)floorf(yy);
  const float dx = xx - x, dy = yy - y;
  mask[n * P + p] = (xx >= 0 && xx <= W - 1 && yy >= 0 && yy <= H - 1) ? 1.0f : 0.0f;
  const int x1 = clampi(x, 0, W - 1), x2 = clampi(x + 1, 0, W - 1);
  const int y1 = clampi(y, 0, H - 1), y2 = clampi(y + 1, 0, H - 1);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float* s = im2 + ch * P;
    const float w2 = s[(int64_t)y1 * W + x1] * (1.0f - dx) * (1.0f - dy) + s[(int64_t)y1 * W + x2] * dx * (1.0f - dy) +
                     s[(int64_t)y2 * W + x1] * (1.0f - dx) * dy + s[(int64_t)y2 * W + x2] * dx * dy;
    const float v1 = im1[ch * P + p];
    avg[(n * 3 + ch) * P + p] = 0.5f * (w2 + v1);
    dt[(n * 3 + ch) * P + p] = w2 - v1;
  }
}

// First spatial derivatives of the mean image: Ix = horizontal, Iy = vertical 5-tap derivative (get_derivatives).
__global__ void __launch_bounds__(VAR_BLOCK) var_deriv1(const float* __restrict__ avg, float* __restrict__ ix,
                                                        float* __restrict__ iy, int H, int W) {
  const int64_t P = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * VAR_BLOCK + threadIdx.x;
  if (p >= P) return;
  const int j = (int)(p / W), i = (int)(p % W);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int64_t pl = ((int64_t)blockIdx.y * 3 + ch) * P;
    const float* a = avg + pl;
    ix[pl + p] = hconv_fast<2>([&](int xx) { return a[(int64_t)j * W + xx]; }, i, W, kD5);
    iy[pl + p] = vconv_fast<2>([&](int yy) { return a[(int64_t)yy * W + i]; }, j, H, kD5);
  }
}

struct SysArgs {
  const float* flow;
  int64_t fpitch, fbstride;
  const float* dpsis;
  const float* dt;
  const float* mask;
  const float* ix;
  const float* iy;
  const float2* X;   // du, dv (skewed)
  float4* P0;        // (inv11, inv12, inv22, b1), or (a11, a12, a22, b1) on the slow path
  float4* P1;        // (b2, h_left, h_right, v_down)
  float* P2;         // v_up
  int H, W;
  float half_alpha, half_delta_over3, half_gamma_over3;
  int slow;
};

// compute_smoothness + compute_data_and_match + sub_laplacian for one pixel, written as the solver reads it.
// The four diffusivities around the pixel are recomputed here (those of the left and upper neighbours too), so
// one launch builds the whole system from the flow, du and the derivative planes.
__global__ void __launch_bounds__(VAR_BLOCK) var_system(SysArgs A) {
  const int H = A.H, W = A.W;
  const int64_t P = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * VAR_BLOCK + threadIdx.x;
  if (p >= P) return;
  const int j = (int)(p / W), i = (int)(p % W);
  const int n = blockIdx.y;
  const int64_t S = (int64_t)(W + H - 1) * H;
  const float* fl = A.flow + n * A.fbstride;
  const float2* X = A.X + n * S;
  const float* dp = A.dpsis + n * P;
  constexpr float eps_smooth = 0.001f * 0.001f;
  constexpr float dnorm = 0.1f * 0.1f;
  constexpr float eps_color = 0.001f * 0.001f;
  constexpr float eps_grad = 0.001f * 0.001f;

  // uu = wx + du, vv = wy + dv (compute_one_level's flow plus increment)
  auto uu = [&](int yy, int xx) { return fl[yy * A.fpitch + 2 * xx] + X[(int64_t)(xx + yy) * H + yy].x; };
  auto vv = [&](int yy, int xx) { return fl[yy * A.fpitch + 2 * xx + 1] + X[(int64_t)(xx + yy) * H + yy].y; };
  // ux2 / uy2 of compute_smoothness: [-0.5 0 0.5] with replicated borders
  auto dx3 = [&](bool u, int yy, int xx) {
    return u ? hconv_fast<1>([&](int q) { return uu(yy, q); }, xx, W, kD3)
             : hconv_fast<1>([&](int q) { return vv(yy, q); }, xx, W, kD3);
  };
  auto dy3 = [&](bool u, int yy, int xx) {
    return u ? vconv_fast<1>([&](int q) { return uu(q, xx); }, yy, H, kD3)
             : vconv_fast<1>([&](int q) { return vv(q, xx); }, yy, H, kD3);
  };
  // diffusivity between (yy, xx) and (yy, xx + 1); zero in the last column
  auto horiz = [&](int yy, int xx) -> float {
    if (xx >= W - 1) return 0.0f;
    const float ux1 = uu(yy, xx + 1) - uu(yy, xx), vx1 = vv(yy, xx + 1) - vv(yy, xx);
    float tmp = 0.5f * (dy3(true, yy, xx) + dy3(true, yy, xx + 1));
    const float uxsq = ux1 * ux1 + tmp * tmp;
    tmp = 0.5f * (dy3(false, yy, xx) + dy3(false, yy, xx + 1));
    const float vxsq = vx1 * vx1 + tmp * tmp;
    tmp = uxsq + vxsq;
    const float num = (dp[(int64_t)yy * W + xx] + dp[(int64_t)yy * W + xx + 1]) * A.half_alpha;
    return (float)((double)num / sqrt((double)(tmp + eps_smooth)));
  };
  // diffusivity between (yy, xx) and (yy + 1, xx); zero in the last row
  auto vert = [&](int yy, int xx) -> float {
    if (yy >= H - 1) return 0.0f;
    const float uy1 = uu(yy + 1, xx) - uu(yy, xx), vy1 = vv(yy + 1, xx) - vv(yy, xx);
    float tmp = 0.5f * (dx3(true, yy, xx) + dx3(true, yy + 1, xx));
    const float uysq = uy1 * uy1 + tmp * tmp;
    tmp = 0.5f * (dx3(false, yy, xx) + dx3(false, yy + 1, xx));
    const float vysq = vy1 * vy1 + tmp * tmp;
    tmp = uysq + vysq;
    const float num = (dp[(int64_t)yy * W + xx] + dp[(int64_t)(yy + 1) * W + xx]) * A.half_alpha;
    return (float)((double)num / sqrt((double)(tmp + eps_smooth)));
  };

  const int64_t sk = (int64_t)(i + j) * H + j;
  const float du = X[sk].x, dv = X[sk].y;
  const float msk = A.mask[n * P + p];

  float ix[3], iy[3], iz[3], ixx[3], ixy[3], iyy[3], ixz[3], iyz[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int64_t pl = ((int64_t)n * 3 + ch) * P;
    const float* X_ = A.ix + pl;
    const float* Y_ = A.iy + pl;
    const float* Z_ = A.dt + pl;
    ix[ch] = X_[p];
    iy[ch] = Y_[p];
    iz[ch] = Z_[p];
    ixx[ch] = hconv_fast<2>([&](int q) { return X_[(int64_t)j * W + q]; }, i, W, kD5);
    ixy[ch] = vconv_fast<2>([&](int q) { return X_[(int64_t)q * W + i]; }, j, H, kD5);
    iyy[ch] = vconv_fast<2>([&](int q) { return Y_[(int64_t)q * W + i]; }, j, H, kD5);
    ixz[ch] = hconv_fast<2>([&](int q) { return Z_[(int64_t)j * W + q]; }, i, W, kD5);
    iyz[ch] = vconv_fast<2>([&](int q) { return Z_[(int64_t)q * W + i]; }, j, H, kD5);
  }

  // compute_data_and_match
  float a11 = 0.0f, a12 = 0.0f, a22 = 0.0f, b1 = 0.0f, b2 = 0.0f;
  if (A.half_delta_over3 != 0.0f) {
    float t[3], nn[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      t[ch] = iz[ch] + ix[ch] * du + iy[ch] * dv;
      nn[ch] = ix[ch] * ix[ch] + iy[ch] * iy[ch] + dnorm;
    }
    float tmp = msk * A.half_delta_over3 /
                sqrtf(t[0] * t[0] / nn[0] + t[1] * t[1] / nn[1] + t[2] * t[2] / nn[2] + eps_color);
    const float w[3] = {tmp / nn[0], tmp / nn[1], tmp / nn[2]};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      a11 = a11 + w[ch] * ix[ch] * ix[ch];
      a12 = a12 + w[ch] * ix[ch] * iy[ch];
      a22 = a22 + w[ch] * iy[ch] * iy[ch];
      b1 = b1 - w[ch] * iz[ch] * ix[ch];
      b2 = b2 - w[ch] * iz[ch] * iy[ch];
    }
  }
  {
    float nx[3], ny[3], tx[3], ty[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      nx[ch] = ixx[ch] * ixx[ch] + ixy[ch] * ixy[ch] + dnorm;
      ny[ch] = iyy[ch] * iyy[ch] + ixy[ch] * ixy[ch] + dnorm;
      tx[ch] = ixz[ch] + ixx[ch] * du + ixy[ch] * dv;
      ty[ch] = iyz[ch] + ixy[ch] * du + iyy[ch] * dv;
    }
    const float tmp = msk * A.half_gamma_over3 /
                      sqrtf(tx[0] * tx[0] / nx[0] + ty[0] * ty[0] / ny[0] + tx[1] * tx[1] / nx[1] +
                            ty[1] * ty[1] / ny[1] + tx[2] * tx[2] / nx[2] + ty[2] * ty[2] / ny[2] + eps_grad);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float wx = tmp / nx[ch], wy = tmp / ny[ch];
      a11 = a11 + (wx * ixx[ch] * ixx[ch] + wy * ixy[ch] * ixy[ch]);
      a12 = a12 + (wx * ixx[ch] * ixy[ch] + wy * ixy[ch] * iyy[ch]);
      a22 = a22 + (wy * iyy[ch] * iyy[ch] + wx * ixy[ch] * ixy[ch]);
      b1 = b1 - (wx * ixx[ch] * ixz[ch] + wy * ixy[ch] * iyz[ch]);
      b2 = b2 - (wy * iyy[ch] * iyz[ch] + wx * ixy[ch] * ixz[ch]);
    }
  }

  // the four diffusivities around the pixel
  const float hr = horiz(j, i);
  const float hl = i > 0 ? horiz(j, i - 1) : 0.0f;
  const float vd = vert(j, i);
  const float vu = j > 0 ? vert(j - 1, i) : 0.0f;

  // sub_laplacian of the current flow (not uu): left edge, right edge, upper edge, lower edge
  {
    auto wxa = [&](int yy, int xx) { return fl[yy * A.fpitch + 2 * xx]; };
    auto wya = [&](int yy, int xx) { return fl[yy * A.fpitch + 2 * xx + 1]; };
    const float cx = wxa(j, i), cy = wya(j, i);
    if (i > 0) {
      b1 = b1 - hl * (cx - wxa(j, i - 1));
      b2 = b2 - hl * (cy - wya(j, i - 1));
    }
    if (i < W - 1) {
      b1 = b1 + hr * (wxa(j, i + 1) - cx);
      b2 = b2 + hr * (wya(j, i + 1) - cy);
    }
    if (j > 0) {
      b1 = b1 - vu * (cx - wxa(j - 1, i));
      b2 = b2 - vu * (cy - wya(j - 1, i));
    }
    if (j < H - 1) {
      b1 = b1 + vd * (wxa(j + 1, i) - cx);
      b2 = b2 + vd * (wya(j + 1, i) - cy);
    }
  }

  float4 q0;
  if (A.slow) {
    q0 = make_float4(a11, a12, a22, b1);
  } else {
    // inverse of the 2x2 diagonal block, once per solve (sor_coupled's first iteration)
    const float dpsis = hl + hr + vu + vd;
    const float A11 = a22 + dpsis, A22 = a11 + dpsis;
    const float det = A11 * A22 - a12 * a12;
    q0 = make_float4(A11 / det, a12 / -det, A22 / det, b1);
  }
  A.P0[n * S + sk] = q0;
  A.P1[n * S + sk] = make_float4(b2, hl, hr, vd);
  A.P2[n * S + sk] = vu;
}

// ---------------------------------------------------------------------------------------------- SOR
// sor_coupled as a wavefront: at step s, row j updates column i = s - j - 2t for every sweep t in [0, T) with
// 0 <= i < W.  Left and upper neighbours then hold sweep t, right and lower ones sweep t - 1 (all written one step
// earlier, none overwritten yet): exactly the lexicographic order.  One workgroup per pair; the barrier orders the
// steps (workgroup-scope visibility: every wave runs on the same CU and its L1).  No pixel a step reads is written
// in that step, so the updates of a step are independent: `k` threads share a row (thread g takes the sweeps
// t = g mod k), and each issues the loads of SOR_U updates before it computes and stores them, so that a step costs
// a few memory latencies instead of one per sweep.
constexpr int SOR_U = 4;

__global__ void __launch_bounds__(1024) var_sor(float2* __restrict__ Xall, const float4* __restrict__ P0all,
                                                const float4* __restrict__ P1all, const float* __restrict__ P2all,
                                                int H, int W, int T, int k, float omega, int slow) {
  const int64_t S = (int64_t)(W + H - 1) * H;
  float2* X = Xall + blockIdx.x * S;
  const float4* P0 = P0all + blockIdx.x * S;
  const float4* P1 = P1all + blockIdx.x * S;
  const float* P2 = P2all + blockIdx.x * S;
  const int nsteps = W + H + 2 * T - 2;
  const float2 zero = make_float2(0.0f, 0.0f);
  for (int s = 0; s < nsteps; ++s) {
    for (int jj = threadIdx.x; jj < H * k; jj += blockDim.x) {
      const int j = jj % H, g = jj / H;
      const int r = s - j;  // column of sweep 0
      if (r < 0) continue;
      int t_lo = r > W - 1 ? (r - W + 2) / 2 : 0;
      const int t_hi = min(T - 1, r / 2);
      t_lo += ((g - t_lo) % k + k) % k;  // first sweep of this thread's residue class
      for (int t0 = t_lo; t0 <= t_hi; t0 += SOR_U * k) {
        float2 c[SOR_U], l[SOR_U], rt[SOR_U], u[SOR_U], d[SOR_U];
        float4 q0[SOR_U], q1[SOR_U];
        float vu[SOR_U];
        int64_t idx[SOR_U];
        bool ok[SOR_U];
#pragma unroll
        for (int q = 0; q < SOR_U; ++q) {
          const int t = t0 + q * k;
          const int i = r - 2 * t;
          ok[q] = t <= t_hi;
          idx[q] = (int64_t)(i + j) * H + j;
          if (ok[q]) {
            c[q] = X[idx[q]];
            l[q] = i > 0 ? X[idx[q] - H] : zero;
            rt[q] = i < W - 1 ? X[idx[q] + H] : zero;
            u[q] = j > 0 ? X[idx[q] - H - 1] : zero;
            d[q] = j < H - 1 ? X[idx[q] + H + 1] : zero;
            q0[q] = P0[idx[q]];
            q1[q] = P1[idx[q]];
            vu[q] = P2[idx[q]];
          }
        }
#pragma unroll
        for (int q = 0; q < SOR_U; ++q) {
          if (!ok[q]) continue;
          const int i = r - 2 * (t0 + q * k);
          const float hl = q1[q].y, hr = q1[q].z, vd = q1[q].w;
          float2 o;
          if (!slow) {
            const float s1 = hr * rt[q].x + vu[q] * u[q].x + vd * d[q].x + q0[q].w;
            const float s2 = hr * rt[q].y + vu[q] * u[q].y + vd * d[q].y + q1[q].x;
            const float B1 = hl * l[q].x + s1, B2 = hl * l[q].y + s2;
            o.x = c[q].x + omega * (q0[q].x * B1 + q0[q].y * B2 - c[q].x);
            o.y = c[q].y + omega * (q0[q].y * B1 + q0[q].z * B2 - c[q].y);
          } else {
            // sor_coupled_slow_but_readable (solver.c:19-52): w < 2 or h < 2
            float su = 0.0f, sv = 0.0f, sd = 0.0f;
            if (j > 0) { su -= vu[q] * u[q].x; sv -= vu[q] * u[q].y; sd += vu[q]; }
            if (i > 0) { su -= hl * l[q].x; sv -= hl * l[q].y; sd += hl; }
            if (j < H - 1) { su -= vd * d[q].x; sv -= vd * d[q].y; sd += vd; }
            if (i < W - 1) { su -= hr * rt[q].x; sv -= hr * rt[q].y; sd += hr; }
            const float A11 = q0[q].x + sd, A12 = q0[q].y, A22 = q0[q].z + sd;
            const float det = A11 * A22 - A12 * A12;
            const float B1 = q0[q].w - su, B2 = q1[q].x - sv;
            o.x = (1.0f - omega) * c[q].x + omega * (A22 * B1 - A12 * B2) / det;
            o.y = (1.0f - omega) * c[q].y + omega * (-A12 * B1 + A11 * B2) / det;
          }
          X[idx[q]] = o;
        }
      }
    }
    __syncthreads();
  }
}

// wx += du, wy += dv (compute_one_level's copy of uu / vv into wx / wy)
__global__ void __launch_bounds__(VAR_BLOCK) var_update(float* __restrict__ flow, int64_t fpitch, int64_t fbstride,
                                                        const float2* __restrict__ Xall, int H, int W) {
  const int64_t P = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * VAR_BLOCK + threadIdx.x;
  if (p >= P) return;
  const int j = (int)(p / W), i = (int)(p % W);
  const int64_t S = (int64_t)(W + H - 1) * H;
  const float2 d = Xall[blockIdx.y * S + (int64_t)(i + j) * H + j];
  float* fl = flow + blockIdx.y * fbstride + j * fpitch + 2 * i;
  fl[0] = fl[0] + d.x;
  fl[1] = fl[1] + d.y;
}

// gaussian_filter (image.c:116-154) + convolution_new(order, half, even = 1) (image.c:157-204), in the same float
// arithmetic, so that the taps are the reference's bits.
GaussTaps gauss_taps(float sigma) {
  GaussTaps g{};
  int order = (int)std::floor(3 * sigma) + 1;
  if (order == 0) order = 1;
  g.order = order;
  float data[2 * VAR_MAX_ORDER + 1];
  const float alpha = 1.0f / (2.0f * sigma * sigma);
  float sum = 0.0f;
  for (int i = -order; i <= order; ++i) {
    data[i + order] = (float)std::exp((double)(-i * i * alpha));
    sum += data[i + order];
  }
  for (int i = -order; i <= order; ++i) data[i + order] /= sum;
  const float* half = data + order;  // centre .. border
  for (int i = 0; i <= order; ++i) g.c[order - i] = g.c[order + i] = half[i];
  float accu = 0.0f;
  for (int i = 0; i <= order; ++i) {
    accu += g.c[i];
    g.a[2 * order - i] = g.a[i] = accu;
  }
  return g;
}

struct WsLayout {
  int64_t tmp_sm, sm, dpsis, avg, dt, mask, ix, iy, X, P0, P1, P2, total;  // byte offsets
};

int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

WsLayout ws_layout(int n, int h, int w) {
  const int64_t P = (int64_t)h * w, S = (int64_t)(w + h - 1) * h, f = sizeof(float);
  WsLayout L{};
  int64_t o = 0;
  auto take = [&](int64_t bytes) { const int64_t at = o; o = align256(o + bytes); return at; };
  L.sm = take(n * 6 * P * f);
  L.dpsis = take(n * P * f);
  L.avg = take(n * 3 * P * f);
  L.dt = take(n * 3 * P * f);
  L.tmp_sm = L.avg;  // the horizontal presmoothing pass (6 planes) runs before avg / dt are used
  L.mask = take(n * P * f);
  L.ix = take(n * 3 * P * f);
  L.iy = take(n * 3 * P * f);
  L.X = take(n * S * 2 * f);
  L.P0 = take(n * S * 4 * f);
  L.P1 = take(n * S * 4 * f);
  L.P2 = take(n * S * f);
  L.total = o;
  return L;
}

}  // namespace
}  // namespace fn2

using namespace fn2;

extern "C" int64_t fn2_variational_workspace_bytes(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1) return -1;
  return ws_layout(n, h, w).total;
}

extern "C" int fn2_variational_refine(const uint8_t* img_a, const uint8_t* img_b, int64_t img_pitch,
                                      int64_t img_bstride, float* flow, int64_t flow_pitch, int64_t flow_bstride,
                                      int n, int h, int w, float alpha, float gamma, float delta, float sigma,
                                      int niter_outer, int niter_inner, int niter_solver, float sor_omega,
                                      void* workspace, int64_t ws_bytes, void* stream) {
  FN2_REQUIRE(img_a && img_b && flow && workspace, "variational_refine: null pointer");
  FN2_REQUIRE(n >= 1 && n <= 65535 && h >= 1 && w >= 1, "variational_refine: bad size n=%d h=%d w=%d", n, h, w);
  FN2_REQUIRE((int64_t)h * w <= (1LL << 30), "variational_refine: image too large (%d x %d)", h, w);
  FN2_REQUIRE(img_pitch >= 3LL * w, "variational_refine: img_pitch %lld < 3 * w", (long long)img_pitch);
  FN2_REQUIRE(n == 1 || img_bstride >= img_pitch * h, "variational_refine: img_bstride %lld < img_pitch * h",
              (long long)img_bstride);
  FN2_REQUIRE(flow_pitch >= 2LL * w, "variational_refine: flow_pitch %lld < 2 * w", (long long)flow_pitch);
  FN2_REQUIRE(n == 1 || flow_bstride >= flow_pitch * h, "variational_refine: flow_bstride %lld < flow_pitch * h",
              (long long)flow_bstride);
  FN2_REQUIRE(niter_outer >= 0 && niter_inner >= 0 && niter_solver >= 0,
              "variational_refine: iteration counts must be >= 0 (%d, %d, %d)", niter_outer, niter_inner, niter_solver);
  FN2_REQUIRE(sigma > 0.0f && 3.0f * sigma < (float)(VAR_MAX_ORDER - 1),
              "variational_refine: sigma must be in (0, %g), got %g", (VAR_MAX_ORDER - 1) / 3.0, (double)sigma);
  FN2_REQUIRE(std::isfinite(alpha) && std::isfinite(gamma) && std::isfinite(delta) && std::isfinite(sor_omega),
              "variational_refine: non-finite parameter");
  const WsLayout L = ws_layout(n, h, w);
  FN2_REQUIRE(ws_bytes >= L.total, "variational_refine: workspace %lld bytes < %lld", (long long)ws_bytes,
              (long long)L.total);
  hipStream_t st = (hipStream_t)stream;
  if (niter_outer == 0 || niter_inner == 0) return FN2_OK;  // compute_one_level leaves the flow as it is

  char* ws = (char*)workspace;
  float* sm = (float*)(ws + L.sm);
  float* dps = (float*)(ws + L.dpsis);
  float* avg = (float*)(ws + L.avg);
  float* dt = (float*)(ws + L.dt);
  float* mask = (float*)(ws + L.mask);
  float* ix = (float*)(ws + L.ix);
  float* iy = (float*)(ws + L.iy);
  float2* X = (float2*)(ws + L.X);
  const int64_t P = (int64_t)h * w, S = (int64_t)(w + h - 1) * h;
  const dim3 pix((unsigned)((P + VAR_BLOCK - 1) / VAR_BLOCK), (unsigned)n);

  const GaussTaps g = gauss_taps(sigma);
  var_smooth_h<<<dim3(pix.x, n, 2), VAR_BLOCK, 0, st>>>(img_a, img_b, img_pitch, img_bstride, (float*)(ws + L.tmp_sm),
                                                         h, w, g);
  var_smooth_v<<<dim3(pix.x, n, 2), VAR_BLOCK, 0, st>>>((const float*)(ws + L.tmp_sm), sm, h, w, g);
  var_dpsis<<<pix, VAR_BLOCK, 0, st>>>(sm, dps, h, w);
  FN2_CHECK_LAUNCH("variational presmoothing");

  SysArgs A{};
  A.flow = flow; A.fpitch = flow_pitch; A.fbstride = flow_bstride;
  A.dpsis = dps; A.dt = dt; A.mask = mask; A.ix = ix; A.iy = iy; A.X = X;
  A.P0 = (float4*)(ws + L.P0); A.P1 = (float4*)(ws + L.P1); A.P2 = (float*)(ws + L.P2);
  A.H = h; A.W = w;
  // the globals variational() sets (variational.c:114-116)
  A.half_alpha = 0.5f * alpha;
  A.half_gamma_over3 = gamma * 0.5f / 3.0f;
  A.half_delta_over3 = delta * 0.5f / 3.0f;
  A.slow = (w < 2 || h < 2) ? 1 : 0;
  // threads per row: as many as fit one 1024-thread workgroup (and no more than there are sweeps)
  const int rows64 = (int)std::min<int64_t>(1024, (h + 63) / 64 * 64);
  const int sor_k = std::max(1, std::min(std::max(niter_solver, 1), 1024 / rows64));
  const int sor_threads = (int)std::min<int64_t>(1024, ((int64_t)h * sor_k + 63) / 64 * 64);

  for (int it = 0; it < niter_outer; ++it) {
    FN2_HIP(hipMemsetAsync(X, 0, (size_t)n * S * sizeof(float2), st));
    var_warp<<<pix, VAR_BLOCK, 0, st>>>(flow, flow_pitch, flow_bstride, sm, avg, dt, mask, h, w);
    var_deriv1<<<pix, VAR_BLOCK, 0, st>>>(avg, ix, iy, h, w);
    for (int in = 0; in < niter_inner; ++in) {
      var_system<<<pix, VAR_BLOCK, 0, st>>>(A);
      if (niter_solver > 0)
        var_sor<<<n, sor_threads, 0, st>>>(X, A.P0, A.P1, A.P2, h, w, niter_solver, sor_k, sor_omega, A.slow);
    }
    var_update<<<pix, VAR_BLOCK, 0, st>>>(flow, flow_pitch, flow_bstride, X, h, w);
    FN2_CHECK_LAUNCH("variational outer iteration");
  }
  return FN2_OK;
}
