// What the kernels over a by-value table of loss levels share (photometric.hip, smoothness.hip): the kernel argument, the
// contraction-free f = scale * pred, and the per-level partial sums of a block.  The walk itself (a wave owns 64
// consecutive pixels of a row, the waves stride the (image, row, segment) units) is unit_at of tf_warp.h.
#pragma once
#include "tf_warp.h"

namespace fn2 {
namespace {

constexpr int PHOTO_BLOCK = 256;  // four waves, each on its own unit
constexpr int PHOTO_WAVES = PHOTO_BLOCK / 64;
constexpr int PHOTO_MAX_BLOCKS = 4096;
constexpr int PHOTO_MAX_LEVELS = 8;

struct PhotoArgs {
  fn2_photometric_level lv[PHOTO_MAX_LEVELS];
  int n_levels, n;
};

// f = scale * pred and the sample position, every product and every sum rounded on its own
__device__ __forceinline__ float2 scaled_flow(float2 p, float s) {
#pragma clang fp contract(off)
  return make_float2(s * p.x, s * p.y);
}
__device__ __forceinline__ float coord(int p, float f) {
#pragma clang fp contract(off)
  return (float)p + f;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the per-level partial sums of a block: every wave adds its own, then one global atomic per level that got something
struct LevelSums {
  float* s;
  __device__ __forceinline__ void clear() {
    if (threadIdx.x < PHOTO_MAX_LEVELS) s[threadIdx.x] = 0.f;
    __syncthreads();
  }
  __device__ __forceinline__ void add(int level, float lane_part) {
    const float v = wave_sum(lane_part);
    if ((threadIdx.x & 63) == 0 && v != 0.f) atomicAdd(&s[level], v);
  }
};

// blocks that give every (image, row, segment) unit of a level its own wave
inline int64_t level_blocks(int n, const fn2_photometric_level& l) {
  const int64_t units = (int64_t)n * l.h * ((l.w + 63) / 64);
  return (units + PHOTO_WAVES - 1) / PHOTO_WAVES;
}

}  // namespace
}  // namespace fn2
