// Multi-scale endpoint error over SPARSE ground truth (KITTI, HD1K, Middlebury): a label pixel whose u or v is not finite
// carries no ground truth, takes no part in the loss and receives a gradient of exactly +0.  The labels come from the
// NaN-aware Downsample op (ops.hip: it skips NaN samples and returns NaN where more than half of the weight was NaN), which
// is what the Caffe FlowNet2 convention for sparse ground truth hands on; this file is what honours it.  The definition is
// the one in include/flownet2_hip.h and its float64 twin is tests/sparse_epe_twin.py.
//
// Per loss scale, valid(p) = both label components finite, M = #valid over the batch, e = ||pred - label||_2 in fp32 as
// epe_loss_grad_kernel (train.hip) forms it:
//   L     = weight * (h w) * sum_valid e / M                                   added to *loss_accum
//   dpred = grad_mult * weight * (h w) / M * (pred - label) / e                on valid pixels with e > 0
//   dpred = +0 in both components everywhere else: invalid pixels, e == 0, and e NaN (which fails e > 0 as it does in the
//           dense kernel);  M = 0: loss 0, dpred all zero
// With every label finite M = n h w and this is average_endpoint_error (weight / n * sum e): the dense loss.
//
// Two launches, each ONE launch for all levels: fn2_sparse_epe_count adds M into the level's counter (an integer: atomics
// are exact in any order), fn2_sparse_epe_loss_grad reads it.  weight * h * w / M is formed in double once per wave and
// level and rounded once, as the coefficient of the photometric loss is.
//
// Safety: both kernels are element-wise.  Every address is base + 2 * i with i from the block, the thread and the level's
// n * h * w alone, i < n * h * w checked by the loop; no index is computed from data.  So whatever pred and label hold
// (NaN, inf, 1e30) moves no load and no store: a non-finite label makes its pixel invalid, a non-finite prediction at an
// invalid pixel is loaded, discarded by a select and reaches nothing, and one at a valid pixel reaches that pixel's dpred
// (0 for NaN) and the loss, as in the dense kernel.  The counter is read, never used as an index.
//
// Work split: levels one after another, a grid-stride walk over the level's pixels with float2 accesses; the count and
// the loss go through a wave shuffle sum, one LDS add per wave and one global atomic per block and level.
#include "photo_levels.h"

#include <cmath>

namespace fn2 {
namespace {

struct SparseArgs {
  fn2_sparse_epe_level lv[PHOTO_MAX_LEVELS];
  int n_levels, n;
};

// one test for NaN and +-inf
__device__ __forceinline__ bool finite2(float2 l) { return fabsf(l.x) < INFINITY && fabsf(l.y) < INFINITY; }

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_xor((int)v, off, 64);
  return v;
}

__global__ void __launch_bounds__(PHOTO_BLOCK) sparse_epe_count_kernel(const SparseArgs a) {
  __shared__ unsigned cnt[PHOTO_MAX_LEVELS];
  if (threadIdx.x < PHOTO_MAX_LEVELS) cnt[threadIdx.x] = 0u;
  __syncthreads();
  for (int l = 0; l < a.n_levels; ++l) {
    const fn2_sparse_epe_level& L = a.lv[l];
    const int64_t npix = (int64_t)a.n * L.h * L.w;
    unsigned mine = 0u;
    for (int64_t i = (int64_t)blockIdx.x * PHOTO_BLOCK + threadIdx.x; i < npix; i += (int64_t)gridDim.x * PHOTO_BLOCK)
      mine += finite2(ld2(L.label + 2 * i)) ? 1u : 0u;
    const unsigned v = wave_sum_u32(mine);
    if ((threadIdx.x & 63) == 0 && v != 0u) atomicAdd(&cnt[l], v);
  }
  __syncthreads();
  if (threadIdx.x < a.n_levels && cnt[threadIdx.x] != 0u) atomicAdd(a.lv[threadIdx.x].count, cnt[threadIdx.x]);
}

__global__ void __launch_bounds__(PHOTO_BLOCK) sparse_epe_loss_grad_kernel(const SparseArgs a, float grad_mult,
                                                                           float* __restrict__ loss_accum) {
  __shared__ float sums[PHOTO_MAX_LEVELS];
  LevelSums acc{sums};
  acc.clear();
  for (int l = 0; l < a.n_levels; ++l) {
    const fn2_sparse_epe_level& L = a.lv[l];
    const int64_t npix = (int64_t)a.n * L.h * L.w;
    const unsigned M = *L.count;  // written by the launch in front; a value, never an index
    // weight * h * w / M once per wave and level, in double, rounded once; 0 for a level without ground truth
    const double cd = M > 0u ? (double)L.weight * (double)L.h * (double)L.w / (double)M : 0.0;
    const float gcoef = (float)((double)grad_mult * cd);
    float part = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * PHOTO_BLOCK + threadIdx.x; i < npix; i += (int64_t)gridDim.x * PHOTO_BLOCK) {
      const float2 p = ld2(L.pred + 2 * i);
      const float2 g = ld2(L.label + 2 * i);
      const bool valid = finite2(g);
      const float du = p.x - g.x, dv = p.y - g.y;
      const float e = sqrtf(du * du + dv * dv);
      part += valid ? e : 0.f;
      float2 out = make_float2(0.f, 0.f);
      if (valid && e > 0.f) {
        const float inv = gcoef / e;
        out = make_float2(du * inv, dv * inv);
      }
      *reinterpret_cast<float2*>(L.dpred + 2 * i) = out;
    }
    acc.add(l, part);
  }
  __syncthreads();
  if (threadIdx.x < a.n_levels && sums[threadIdx.x] != 0.f) {
    const fn2_sparse_epe_level& L = a.lv[threadIdx.x];
    const unsigned M = *L.count;
    if (M > 0u)
      atomicAdd(loss_accum, sums[threadIdx.x] * (float)((double)L.weight * (double)L.h * (double)L.w / (double)M));
  }
}

// the rules both entry points share; fills the by-value table and the grid
int sparse_table(const char* what, const fn2_sparse_epe_level* levels, int n_levels, int n, SparseArgs& a, int& grid) {
  FN2_REQUIRE(levels, "%s: null level table", what);
  FN2_REQUIRE(n_levels >= 1 && n_levels <= PHOTO_MAX_LEVELS, "%s: n_levels must be 1..%d, got %d", what,
              PHOTO_MAX_LEVELS, n_levels);
  FN2_REQUIRE(n >= 1, "%s: n must be >= 1, got %d", what, n);
  a.n_levels = n_levels;
  a.n = n;
  int64_t blocks = 1;
  for (int i = 0; i < n_levels; ++i) {
    const fn2_sparse_epe_level& l = levels[i];
    FN2_REQUIRE(l.pred && l.label && l.dpred && l.count, "%s: null pointer in level %d", what, i);
    FN2_REQUIRE(l.h >= 1 && l.w >= 1, "%s: level %d: bad size h=%d w=%d", what, i, l.h, l.w);
    FN2_REQUIRE((int64_t)n * l.h * l.w < (1LL << 31), "%s: level %d: n*h*w must be below 2^31 (%d x %d x %d)", what, i,
                n, l.h, l.w);
    FN2_REQUIRE(((reinterpret_cast<uintptr_t>(l.pred) | reinterpret_cast<uintptr_t>(l.label) |
                  reinterpret_cast<uintptr_t>(l.dpred)) & 7) == 0,
                "%s: level %d: pred, label and dpred must be 8-byte aligned", what, i);
    FN2_REQUIRE((reinterpret_cast<uintptr_t>(l.count) & 3) == 0, "%s: level %d: count must be 4-byte aligned", what, i);
    FN2_REQUIRE(std::isfinite(l.weight) && l.weight >= 0.f, "%s: level %d: weight must be finite and >= 0, got %g", what,
                i, (double)l.weight);
    a.lv[i] = l;
    blocks = max(blocks, ((int64_t)n * l.h * l.w + PHOTO_BLOCK - 1) / PHOTO_BLOCK);
  }
  grid = (int)min(blocks, (int64_t)PHOTO_MAX_BLOCKS);
  return FN2_OK;
}

}  // namespace
}  // namespace fn2

using namespace fn2;

extern "C" {

int fn2_sparse_epe_count(const fn2_sparse_epe_level* levels, int n_levels, int n, void* stream) {
  const char* what = "sparse_epe_count";
  SparseArgs a{};
  int grid = 1;
  if (const int rc = sparse_table(what, levels, n_levels, n, a, grid)) return rc;
  hipLaunchKernelGGL(sparse_epe_count_kernel, dim3(grid), dim3(PHOTO_BLOCK), 0, (hipStream_t)stream, a);
  FN2_CHECK_LAUNCH(what);
  return FN2_OK;
}

int fn2_sparse_epe_loss_grad(const fn2_sparse_epe_level* levels, int n_levels, int n, float grad_mult, float* loss_accum,
                             void* stream) {
  const char* what = "sparse_epe_loss_grad";
  SparseArgs a{};
  int grid = 1;
  if (const int rc = sparse_table(what, levels, n_levels, n, a, grid)) return rc;
  FN2_REQUIRE(loss_accum, "%s: null loss_accum", what);
  FN2_REQUIRE(std::isfinite(grad_mult) && grad_mult > 0.f, "%s: grad_mult must be finite and > 0, got %g", what,
              (double)grad_mult);
  hipLaunchKernelGGL(sparse_epe_loss_grad_kernel, dim3(grid), dim3(PHOTO_BLOCK), 0, (hipStream_t)stream, a, grad_mult,
                     loss_accum);
  FN2_CHECK_LAUNCH(what);
  return FN2_OK;
}

}  // extern "C"
