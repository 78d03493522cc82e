// Edge-aware smoothness term of the unsupervised trainer: a first- or second-order flow regulariser whose terms are
// weighted down across image edges.  An addition to the reference, which has no such term; its definition is the one in
// include/flownet2_hip.h and its float64 twin is tests/smoothness_twin.py.
//
// Per loss scale, with f = scale * pred rounded once (scaled_flow of photo_levels.h, as the photometric loss forms it),
// I the level's frames, rho(d) = sqrt(d^2 + eps^2), k the flow component:
//   order 1   a term sits between x and x + 1, x in [0, w - 2]:  D_k = f_k(x + 1) - f_k(x),
//             g = exp(-lambda * mean_c |I(x + 1) - I(x)|)
//   order 2   a term sits on x in [1, w - 2]:  D_k = f_k(x - 1) - 2 f_k(x) + f_k(x + 1),
//             g = exp(-lambda * mean_c |I(x + 1) - I(x - 1)| / 2)
//   L = weight * smooth_weight * 0.5 * (sum g rho(D_k) / Cx + the same along y), Cx = n h (w - order) the number of x terms
// The gradient is a GATHER: a pixel takes part in the order + 1 terms of an axis that touch it and recomputes each of them
// from its own loads (2 order + 1 flows and frames per axis, the centre shared), so every dpred element is written by one
// lane, with a plain store (accumulate: a plain load and store of that element), and two runs agree bit for bit.
//
// Safety: every address is formed from (image, row, column) and the level's sizes alone, and a tap is loaded only when its
// row / column lies inside the image.  No index is computed from data, so whatever pred holds (NaN, inf, 1e30) moves no
// load and no store; such a value reaches the terms it takes part in -- the pixels within `order` of it along a row or a
// column, and the loss -- and nothing else.
//
// The second difference is formed in double and rounded once: in fp32 the intermediate f(x - 1) - 2 f(x) rounds at the
// size of f, not of D, and rho' has slope 1 / eps at 0 (an ulp of a 3-pixel flow is 2.4e-4 eps at eps = 1e-3).  A first
// difference is one correctly rounded subtraction already.
//
// Work split of photometric.hip: levels one after another, a wave owns 64 consecutive pixels of a row, the waves stride
// the (image, row, segment) units; the loss goes through wave shuffles and LDS into one atomic per block and level.
#include "photo_levels.h"

#include <cmath>

namespace fn2 {
namespace {

struct SmoothConst {
  float lambda, eps2;
};

// one term from its taps: the edge weight g, g * rho'(D_k) for both components, and g * (rho(D_u) + rho(D_v))
struct SmoothTerm {
  float tu, tv, loss;
};

__device__ __forceinline__ float second_diff(float m, float c, float p) {
  return (float)(((double)m - 2.0 * (double)c) + (double)p);
}

__device__ __forceinline__ SmoothTerm smooth_term(float du, float dv, const rgb3_t& a, const rgb3_t& b, float half,
                                                  const SmoothConst& k) {
  const float diff = (fabsf(b.r - a.r) + fabsf(b.g - a.g) + fabsf(b.b - a.b)) * (half * (1.f / 3.f));
  const float g = expf(-k.lambda * diff);
  const float ru = sqrtf(du * du + k.eps2), rv = sqrtf(dv * dv + k.eps2);
  return SmoothTerm{g * (du / ru), g * (dv / rv), g * (ru + rv)};
}

// The part of one axis: `fp` / `ip` point at the pixel's own flow and frame, `step` is the distance of neighbours along
// the axis in pixels (1 or w), `p` the pixel's position on the axis and `len` the axis length.  Adds c * dS/df to (gu, gv)
// and c * (the term the pixel owns) to `part`.
template <int ORDER>
__device__ __forceinline__ void smooth_axis(const float* fp, const float* ip, int64_t step, int p, int len, float s,
                                            float c, const SmoothConst& k, float& gu, float& gv, float& part) {
  float2 f[2 * ORDER + 1];
  rgb3_t I[2 * ORDER + 1];
#pragma unroll
  for (int d = -ORDER; d <= ORDER; ++d) {
    f[d + ORDER] = make_float2(0.f, 0.f);
    I[d + ORDER] = rgb3_t{0.f, 0.f, 0.f};
    if (p + d >= 0 && p + d < len) {  // the only condition a load depends on
      f[d + ORDER] = scaled_flow(ld2(fp + 2 * d * step), s);
      I[d + ORDER] = load_rgb(ip + 3 * d * step);
    }
  }
  float su = 0.f, sv = 0.f;
  if constexpr (ORDER == 1) {
    if (p >= 1) {  // the term between p - 1 and p
      const SmoothTerm t = smooth_term(f[1].x - f[0].x, f[1].y - f[0].y, I[0], I[1], 1.f, k);
      su += t.tu, sv += t.tv;
    }
    if (p <= len - 2) {  // the term between p and p + 1: the one this pixel owns
      const SmoothTerm t = smooth_term(f[2].x - f[1].x, f[2].y - f[1].y, I[1], I[2], 1.f, k);
      su -= t.tu, sv -= t.tv;
      part += c * t.loss;
    }
  } else {
    auto term = [&](int i) {  // centred on tap i
      return smooth_term(second_diff(f[i - 1].x, f[i].x, f[i + 1].x), second_diff(f[i - 1].y, f[i].y, f[i + 1].y),
                         I[i - 1], I[i + 1], 0.5f, k);
    };
    if (p >= 2) {  // centred on p - 1 (p - 1 <= len - 2 always)
      const SmoothTerm t = term(1);
      su += t.tu, sv += t.tv;
    }
    if (p >= 1 && p <= len - 2) {  // centred on p: owned
      const SmoothTerm t = term(2);
      su -= 2.f * t.tu, sv -= 2.f * t.tv;
      part += c * t.loss;
    }
    if (p <= len - 3) {  // centred on p + 1
      const SmoothTerm t = term(3);
      su += t.tu, sv += t.tv;
    }
  }
  gu += c * su;
  gv += c * sv;
}

template <int ORDER>
__global__ void __launch_bounds__(PHOTO_BLOCK) smoothness_loss_grad_kernel(const PhotoArgs a, float edge_lambda, float eps,
                                                                           float smooth_weight, float grad_mult,
                                                                           int accumulate, float* __restrict__ loss_accum) {
  __shared__ float sums[PHOTO_MAX_LEVELS];
  LevelSums acc{sums};
  acc.clear();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const SmoothConst k{edge_lambda, eps * eps};
  for (int l = 0; l < a.n_levels; ++l) {
    const fn2_photometric_level& L = a.lv[l];
    const int H = L.h, W = L.w, segs = (W + 63) / 64;
    const int64_t units = (int64_t)a.n * H * segs;
    const float s = L.scale;
    // an axis too short for one term is absent; a 1-high or 1-wide level has neither
    const bool has_x = W > ORDER && H > 1, has_y = H > ORDER && W > 1;
    if (!has_x && !has_y && accumulate) continue;  // loss 0, gradient 0: nothing to add
    // 0.5 / C per axis, one division per level and wave, in double
    const float cx = has_x ? (float)(0.5 / ((double)a.n * H * (W - ORDER))) : 0.f;
    const float cy = has_y ? (float)(0.5 / ((double)a.n * W * (H - ORDER))) : 0.f;
    const float gcoef = (float)((double)grad_mult * (double)L.weight * (double)smooth_weight * (double)s);
    float part = 0.f;
    for (int64_t u = (int64_t)blockIdx.x * PHOTO_WAVES + wave; u < units; u += (int64_t)gridDim.x * PHOTO_WAVES) {
      const Unit p = unit_at(u, H, segs);
      if (p.x >= W) continue;
      const int64_t o = (p.n * H + p.y) * W + p.x;
      float gu = 0.f, gv = 0.f;
      if (has_x) smooth_axis<ORDER>(L.pred + 2 * o, L.img + 3 * o, 1, p.x, W, s, cx, k, gu, gv, part);
      if (has_y) smooth_axis<ORDER>(L.pred + 2 * o, L.img + 3 * o, W, p.y, H, s, cy, k, gu, gv, part);
      float2 out = make_float2(gcoef * gu, gcoef * gv);
      float2* dst = reinterpret_cast<float2*>(L.dpred + 2 * o);
      if (accumulate) {
        const float2 old = *dst;
        out = make_float2(old.x + out.x, old.y + out.y);
      }
      *dst = out;
    }
    acc.add(l, part);
  }
  __syncthreads();
  if (threadIdx.x < a.n_levels && sums[threadIdx.x] != 0.f)
    atomicAdd(loss_accum, (float)((double)sums[threadIdx.x] * (double)a.lv[threadIdx.x].weight * (double)smooth_weight));
}

}  // namespace
}  // namespace fn2

using namespace fn2;

extern "C" {

int fn2_smoothness_loss_grad(const fn2_photometric_level* levels, int n_levels, int n, int order, float edge_lambda,
                             float eps, float smooth_weight, float grad_mult, int accumulate, float* loss_accum,
                             void* stream) {
  const char* what = "smoothness_loss_grad";
  FN2_REQUIRE(levels, "%s: null level table", what);
  FN2_REQUIRE(n_levels >= 1 && n_levels <= PHOTO_MAX_LEVELS, "%s: n_levels must be 1..%d, got %d", what,
              PHOTO_MAX_LEVELS, n_levels);
  FN2_REQUIRE(n >= 1, "%s: n must be >= 1, got %d", what, n);
  FN2_REQUIRE(loss_accum, "%s: null loss_accum", what);
  FN2_REQUIRE(order == 1 || order == 2, "%s: order must be 1 or 2, got %d", what, order);
  FN2_REQUIRE(std::isfinite(edge_lambda) && edge_lambda >= 0.f, "%s: edge_lambda must be finite and >= 0, got %g", what,
              (double)edge_lambda);
  FN2_REQUIRE(std::isfinite(eps) && eps > 0.f, "%s: eps must be finite and > 0, got %g", what, (double)eps);
  FN2_REQUIRE(std::isfinite(smooth_weight) && smooth_weight >= 0.f, "%s: smooth_weight must be finite and >= 0, got %g",
              what, (double)smooth_weight);
  FN2_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate must be 0 or 1, got %d", what, accumulate);
  PhotoArgs a{};
  a.n_levels = n_levels;
  a.n = n;
  int64_t blocks = 1;
  for (int i = 0; i < n_levels; ++i) {
    const fn2_photometric_level& l = levels[i];
    FN2_REQUIRE(l.pred && l.img && l.dpred, "%s: null pointer in level %d", what, i);  // (mask, mask_sum: not read)
    FN2_REQUIRE(l.h >= 1 && l.w >= 1, "%s: level %d: bad size h=%d w=%d", what, i, l.h, l.w);
    FN2_REQUIRE((int64_t)l.h * l.w <= (1LL << 30), "%s: level %d: image too large (%d x %d)", what, i, l.h, l.w);
    FN2_REQUIRE(((reinterpret_cast<uintptr_t>(l.pred) | reinterpret_cast<uintptr_t>(l.dpred)) & 7) == 0,
                "%s: level %d: pred and dpred must be 8-byte aligned", what, i);
    a.lv[i] = l;
    blocks = max(blocks, level_blocks(n, l));
  }
  const int grid = (int)min(blocks, (int64_t)PHOTO_MAX_BLOCKS);
  if (order == 1)
    hipLaunchKernelGGL(smoothness_loss_grad_kernel<1>, dim3(grid), dim3(PHOTO_BLOCK), 0, (hipStream_t)stream, a,
                       edge_lambda, eps, smooth_weight, grad_mult, accumulate, loss_accum);
  else
    hipLaunchKernelGGL(smoothness_loss_grad_kernel<2>, dim3(grid), dim3(PHOTO_BLOCK), 0, (hipStream_t)stream, a,
                       edge_lambda, eps, smooth_weight, grad_mult, accumulate, loss_accum);
  FN2_CHECK_LAUNCH(what);
  return FN2_OK;
}

}  // extern "C"
