// Occlusion-aware photometric loss of the unsupervised trainer: SelFlow's abs_robust_loss (src/utils.py:378-395) of
// the difference between a frame and its partner warped by tf_warp (:453-515), on the pixels that are neither occluded
// by the forward-backward test (occlusion, :523-538) nor sampled from outside the partner frame.  The reference carries
// these pieces (:354-538) and never joins them into a training graph.
//
// Slots: image j of the batch is a frame, image j ^ 1 its partner (pair k fills slots 2k and 2k + 1 with the two
// directions).  Per loss scale, with f = scale * pred rounded once and (X, Y) = (x + f.u, y + f.v) rounded once (never
// a fused multiply-add: the truncation in tf_warp is discontinuous and the float64 twin of the tests has to land on the
// same coordinate):
//   masks      m = valid & ~occ;  occ = |f + tf_warp(f', f)|^2 > alpha (|f|^2 + |tf_warp(f', f)|^2) + beta with f' the
//              partner's flow;  valid = 0 <= X < w - 1 and 0 <= Y < h - 1 (tf_warp returns exactly 0 from w - 1 on: such
//              a pixel would contribute its own brightness as a residual);  mask_sum += sum m
//   loss_grad  d_c = img[j] - tf_warp(img[j ^ 1], f)_c;  psi = (|d| + 0.01)^q;  L = weight * sum m psi / (2 M + 1e-6);
//              dpred = grad_mult * weight * scale / (2 M + 1e-6) * m * sum_c psi'(d_c) * (-d warp_c / d(X, Y)), the masks
//              and M constants.  The gradient is local to its pixel: plain stores.
//
// Both kernels take the table of levels by value and walk the levels one after another; within a level a wave owns 64
// consecutive pixels of a row and the waves stride the (image, row, segment) units, as in occlusion.hip.  The scalars
// are reduced by wave shuffles, then per level in LDS, and leave the block as one atomic per level.
#include "photo_levels.h"

namespace fn2 {
namespace {

__global__ void __launch_bounds__(PHOTO_BLOCK) photometric_masks_kernel(const PhotoArgs a, float alpha, float beta) {
  __shared__ float sums[PHOTO_MAX_LEVELS];
  LevelSums acc{sums};
  acc.clear();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (int l = 0; l < a.n_levels; ++l) {
    const fn2_photometric_level& L = a.lv[l];
    const int H = L.h, W = L.w, segs = (W + 63) / 64;
    const int64_t units = (int64_t)a.n * H * segs, pitch = 2LL * W, bstride = pitch * H;
    const float s = L.scale;
    float count = 0.f;
    for (int64_t u = (int64_t)blockIdx.x * PHOTO_WAVES + wave; u < units; u += (int64_t)gridDim.x * PHOTO_WAVES) {
      const Unit p = unit_at(u, H, segs);
      if (p.x >= W) continue;
      const float* own = L.pred + p.n * bstride;
      const float* par = L.pred + (p.n ^ 1) * bstride;
      const float2 f = scaled_flow(ld2(own + (int64_t)p.y * pitch + 2 * p.x), s);
      const float X = coord(p.x, f.x), Y = coord(p.y, f.y);
      const TfTaps t = tf_taps_at(X, Y, W, H);
      const float* r0 = par + (int64_t)t.y0 * pitch;
      const float* r1 = par + (int64_t)t.y1 * pitch;
      const float2 ta = scaled_flow(ld2(r0 + 2 * t.x0), s), tb = scaled_flow(ld2(r1 + 2 * t.x0), s);
      const float2 tc = scaled_flow(ld2(r0 + 2 * t.x1), s), td = scaled_flow(ld2(r1 + 2 * t.x1), s);
      const float bx = tf_blend(t, ta.x, tb.x, tc.x, td.x), by = tf_blend(t, ta.y, tb.y, tc.y, td.y);  // :527
      const float sx = f.x + bx, sy = f.y + by;                                                       // :529
      const float d = sx * sx + sy * sy;
      const float mag = (f.x * f.x + f.y * f.y) + (bx * bx + by * by);                                // :531
      const bool occ = d > alpha * mag + beta;                                    // :533-535; a NaN compares false
      const bool valid = X >= 0.f && X < (float)(W - 1) && Y >= 0.f && Y < (float)(H - 1);            // a NaN fails
      const float m = valid && !occ ? 1.f : 0.f;
      L.mask[(p.n * H + p.y) * W + p.x] = m;
      count += m;
    }
    acc.add(l, count);
  }
  __syncthreads();
  if (threadIdx.x < a.n_levels && sums[threadIdx.x] != 0.f) atomicAdd(a.lv[threadIdx.x].mask_sum, sums[threadIdx.x]);
}

__global__ void __launch_bounds__(PHOTO_BLOCK) photometric_loss_grad_kernel(const PhotoArgs a, float q, float grad_mult,
                                                                            float* __restrict__ loss_accum) {
  __shared__ float sums[PHOTO_MAX_LEVELS];
  LevelSums acc{sums};
  acc.clear();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (int l = 0; l < a.n_levels; ++l) {
    const fn2_photometric_level& L = a.lv[l];
    const int H = L.h, W = L.w, segs = (W + 63) / 64;
    const int64_t units = (int64_t)a.n * H * segs, ipitch = 3LL * W, ibstride = ipitch * H;
    const float s = L.scale;
    // (one division per level and wave, in double: 2 M + 1e-6 is not an fp32 number)
    const float gcoef = (float)((double)grad_mult * (double)L.weight * (double)s / (2.0 * (double)*L.mask_sum + 1e-6));
    float part = 0.f;
    for (int64_t u = (int64_t)blockIdx.x * PHOTO_WAVES + wave; u < units; u += (int64_t)gridDim.x * PHOTO_WAVES) {
      const Unit p = unit_at(u, H, segs);
      if (p.x >= W) continue;
      const int64_t o = (p.n * H + p.y) * W + p.x;
      float gu = 0.f, gv = 0.f;
      if (L.mask[o] != 0.f) {
        const float2 f = scaled_flow(ld2(L.pred + 2 * o), s);
        const float X = coord(p.x, f.x), Y = coord(p.y, f.y);
        const TfTaps t = tf_taps_at(X, Y, W, H);
        const float* par = L.img + (p.n ^ 1) * ibstride;
        const float* r0 = par + (int64_t)t.y0 * ipitch;
        const float* r1 = par + (int64_t)t.y1 * ipitch;
        const rgb3_t me = load_rgb(L.img + 3 * o);
        const rgb3_t ia = load_rgb(r0 + 3 * t.x0), ib = load_rgb(r1 + 3 * t.x0);
        const rgb3_t ic = load_rgb(r0 + 3 * t.x1), id = load_rgb(r1 + 3 * t.x1);
        // d warp / dX = (y1 - Y)(Ic - Ia) + (Y - y0)(Id - Ib), d warp / dY = (x1 - X)(Ib - Ia) + (X - x0)(Id - Ic): what
        // autodiff of :502-514 gives, the integer casts carrying no gradient
        const float wy1 = (float)t.y1 - Y, wy0 = Y - (float)t.y0, wx1 = (float)t.x1 - X, wx0 = X - (float)t.x0;
        auto channel = [&](float mine, float va, float vb, float vc, float vd) {
          const float d = mine - tf_blend(t, va, vb, vc, vd);
          const float mag = fabsf(d) + 0.01f;
          const float psi = powf(mag, q);                                         // :389
          const float dpsi = d == 0.f ? 0.f : copysignf(q * psi / mag, d);        // q (|d| + 0.01)^(q - 1) sign(d), sign(0) = 0
          part += psi;
          gu -= dpsi * (wy1 * (vc - va) + wy0 * (vd - vb));
          gv -= dpsi * (wx1 * (vb - va) + wx0 * (vd - vc));
        };
        channel(me.r, ia.r, ib.r, ic.r, id.r);
        channel(me.g, ia.g, ib.g, ic.g, id.g);
        channel(me.b, ia.b, ib.b, ic.b, id.b);
      }
      *reinterpret_cast<float2*>(L.dpred + 2 * o) = make_float2(gcoef * gu, gcoef * gv);
    }
    acc.add(l, part);
  }
  __syncthreads();
  if (threadIdx.x < a.n_levels && sums[threadIdx.x] != 0.f) {
    const fn2_photometric_level& L = a.lv[threadIdx.x];
    atomicAdd(loss_accum, (float)((double)sums[threadIdx.x] * (double)L.weight / (2.0 * (double)*L.mask_sum + 1e-6)));
  }
}

// the table checked and copied into the kernel argument; the grid covers the largest level
int photo_args(const char* what, const fn2_photometric_level* levels, int n_levels, int n, PhotoArgs& a, int& grid) {
  FN2_REQUIRE(levels, "%s: null level table", what);
  FN2_REQUIRE(n_levels >= 1 && n_levels <= PHOTO_MAX_LEVELS, "%s: n_levels must be 1..%d, got %d", what,
              PHOTO_MAX_LEVELS, n_levels);
  FN2_REQUIRE(n >= 2 && n % 2 == 0, "%s: n must be even (two slots per pair), got %d", what, n);
  a = PhotoArgs{};
  a.n_levels = n_levels;
  a.n = n;
  int64_t blocks = 1;
  for (int i = 0; i < n_levels; ++i) {
    const fn2_photometric_level& l = levels[i];
    FN2_REQUIRE(l.pred && l.img && l.mask && l.mask_sum && l.dpred, "%s: null pointer in level %d", what, i);
    FN2_REQUIRE(l.h >= 1 && l.w >= 1, "%s: level %d: bad size h=%d w=%d", what, i, l.h, l.w);
    FN2_REQUIRE((int64_t)l.h * l.w <= (1LL << 30), "%s: level %d: image too large (%d x %d)", what, i, l.h, l.w);
    FN2_REQUIRE(((reinterpret_cast<uintptr_t>(l.pred) | reinterpret_cast<uintptr_t>(l.dpred)) & 7) == 0,
                "%s: level %d: pred and dpred must be 8-byte aligned", what, i);
    a.lv[i] = l;
    blocks = max(blocks, level_blocks(n, l));
  }
  grid = (int)min(blocks, (int64_t)PHOTO_MAX_BLOCKS);
  return FN2_OK;
}

}  // namespace
}  // namespace fn2

using namespace fn2;

extern "C" {

int fn2_photometric_masks(const fn2_photometric_level* levels, int n_levels, int n, float alpha, float beta,
                          void* stream) {
  PhotoArgs a;
  int grid;
  if (int rc = photo_args("photometric_masks", levels, n_levels, n, a, grid)) return rc;
  hipLaunchKernelGGL(photometric_masks_kernel, dim3(grid), dim3(PHOTO_BLOCK), 0, (hipStream_t)stream, a, alpha, beta);
  FN2_CHECK_LAUNCH("photometric_masks");
  return FN2_OK;
}

int fn2_photometric_loss_grad(const fn2_photometric_level* levels, int n_levels, int n, float q, float grad_mult,
                              float* loss_accum, void* stream) {
  PhotoArgs a;
  int grid;
  if (int rc = photo_args("photometric_loss_grad", levels, n_levels, n, a, grid)) return rc;
  FN2_REQUIRE(loss_accum, "photometric_loss_grad: null loss_accum");
  FN2_REQUIRE(q > 0.f && q <= 1.f, "photometric_loss_grad: q must lie in (0, 1], got %g", (double)q);
  hipLaunchKernelGGL(photometric_loss_grad_kernel, dim3(grid), dim3(PHOTO_BLOCK), 0, (hipStream_t)stream, a, q,
                     grad_mult, loss_accum);
  FN2_CHECK_LAUNCH("photometric_loss_grad");
  return FN2_OK;
}

}  // extern "C"
