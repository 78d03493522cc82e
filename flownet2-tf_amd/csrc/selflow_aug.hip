// The augmentation the reference's live loader trains with (the SelFlow-style functions of src/data_augmentation.py,
// called from src/dataloader.py:35-113), as two launches over a batch:
//   fn2_selflow_stats  -> what has to be known about a whole sample before any of its pixels can be written: the number
//                         of pixels the re-sampled match mask sets (sample_from_distribution's "almost empty" test,
//                         data_augmentation.py:513-521) and the per-channel sums adjust_contrast needs (the mean of the
//                         image as it stands in front of the contrast op of that sample's chain)
//   fn2_selflow_apply  -> every output pixel from its source pixel: re-sampled mask and sparse flow
//                         (sample_sparse_uniform :435-445, sample_sparse_invalid_like :449-479), flips with their flow
//                         signs (:107-140), channel permutation (:162-175), colour chain (:30-91)
// Every random decision is made on the host (src/data_augmentation.py draw_*_params) and arrives in the per-sample
// parameter table (include/flownet2_hip.h FN2_SF_*); the kernels are deterministic functions of their inputs and
// that table.  Both passes are HBM-bound small-channel passes: a lane per pixel, the image as one 12-byte access, flows
// as float2, blockIdx.y = sample so that everything per-sample is wave-uniform (scalar loads, uniform branches).
#include "fn2_common.h"

namespace fn2 {

constexpr int SF_STATS_BLOCK = 512;
constexpr int SF_APPLY_BLOCK = 256;
constexpr int SF_MAX_PARTIALS = 64;
constexpr int SF_STATS_PIXELS = 2048;  // pixels per partial until SF_MAX_PARTIALS caps the count

// partials per sample: a function of (h, w) only, so the reduction order is too
static inline int sf_partials(int h, int w) {
  const long p = ((long)h * w + SF_STATS_PIXELS - 1) / SF_STATS_PIXELS;
  return (int)(p < 1 ? 1 : (p > SF_MAX_PARTIALS ? SF_MAX_PARTIALS : p));
}
static inline int64_t sf_align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

__device__ __forceinline__ uint32_t fmix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}
// the per-pixel uniform draw: i = source pixel index y * w + x
__device__ __forceinline__ uint32_t sf_hash(uint32_t i, uint32_t key0, uint32_t key1) {
  return fmix32(fmix32(i ^ key0) + key1);
}

// one sample's record, read through a wave-uniform pointer (scalar loads)
struct sf_sample {
  uint32_t distrib, threshold, key0, key1;
  int n_rect, rect[3][4];
  bool flip_lr, flip_ud;
  int perm;
};
struct sf_colour {
  int order;  // 0..3, anything else: no colour distortion
  float d_brightness, f_saturation, d_hue, f_contrast;
};

__device__ __forceinline__ sf_sample sf_load_sample(const uint32_t* __restrict__ p) {
  sf_sample s;
  s.distrib = p[FN2_SF_DISTRIB];
  s.threshold = p[FN2_SF_THRESHOLD];
  s.key0 = p[FN2_SF_KEY0];
  s.key1 = p[FN2_SF_KEY1];
  const int nr = (int)p[FN2_SF_N_RECT];
  s.n_rect = nr < 0 ? 0 : (nr > 3 ? 3 : nr);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) s.rect[r][k] = (int)p[FN2_SF_RECTS + 4 * r + k];
  s.flip_lr = p[FN2_SF_FLIP_LR] != 0;
  s.flip_ud = p[FN2_SF_FLIP_UD] != 0;
  s.perm = (int)p[FN2_SF_PERM];
  return s;
}
__device__ __forceinline__ sf_colour sf_load_colour(const uint32_t* __restrict__ p) {
  sf_colour c;
  c.order = (int)p[FN2_SF_COLOUR_ORDER];
  c.d_brightness = __uint_as_float(p[FN2_SF_D_BRIGHTNESS]);
  c.f_saturation = __uint_as_float(p[FN2_SF_F_SATURATION]);
  c.d_hue = __uint_as_float(p[FN2_SF_D_HUE]);
  c.f_contrast = __uint_as_float(p[FN2_SF_F_CONTRAST]);
  return c;
}
__device__ __forceinline__ bool sf_has_colour(const sf_colour& c) { return c.order >= 0 && c.order <= 3; }

// the re-sampled mask at source pixel (y, x) for distrib 1 / 2 (anything else: 0, never asked for)
__device__ __forceinline__ bool sf_mask(const sf_sample& s, int y, int x, int W) {
  if (s.distrib == 1u) return sf_hash((uint32_t)(y * W + x), s.key0, s.key1) < s.threshold;
  bool inside = false;
#pragma unroll
  for (int r = 0; r < 3; ++r)
    inside |= r < s.n_rect && y >= s.rect[r][0] && y < s.rect[r][0] + s.rect[r][2] && x >= s.rect[r][1] &&
              x < s.rect[r][1] + s.rect[r][3];
  return s.distrib == 2u && !inside;
}

// rows of the table at data_augmentation.py:163-168: out channel k = in channel perm[k]
__device__ __forceinline__ void sf_permute(int perm, float& r, float& g, float& b) {
  const float i0 = r, i1 = g, i2 = b;
  switch (perm) {
    case 1: r = i0; g = i2; b = i1; break;
    case 2: r = i1; g = i0; b = i2; break;
    case 3: r = i1; g = i2; b = i0; break;
    case 4: r = i2; g = i0; b = i1; break;
    case 5: r = i2; g = i1; b = i0; break;
    default: break;
  }
}

// TensorFlow's rgb_to_hsv / hsv_to_rgb (adjust_saturation / adjust_hue go through them), stated in the header
__device__ __forceinline__ void sf_rgb_to_hsv(float r, float g, float b, float& h, float& s, float& v) {
  v = fmaxf(r, fmaxf(g, b));
  const float range = v - fminf(r, fminf(g, b));
  s = v > 0.0f ? range / v : 0.0f;
  if (range <= 0.0f) {
    h = 0.0f;
  } else if (r == v) {
    h = (g - b) / (6.0f * range);
  } else if (g == v) {
    h = (b - r) / (6.0f * range) + 2.0f / 6.0f;
  } else {
    h = (r - g) / (6.0f * range) + 4.0f / 6.0f;
  }
  if (h < 0.0f) h += 1.0f;
}
__device__ __forceinline__ void sf_hsv_to_rgb(float h, float s, float v, float& r, float& g, float& b) {
  const float c = s * v, m = v - c, dh = 6.0f * h;
  const float x = c * (1.0f - fabsf(fmodf(dh, 2.0f) - 1.0f));
  switch ((int)dh) {
    case 1: r = x; g = c; b = 0.0f; break;
    case 2: r = 0.0f; g = c; b = x; break;
    case 3: r = 0.0f; g = x; b = c; break;
    case 4: r = x; g = 0.0f; b = c; break;
    case 5: r = c; g = 0.0f; b = x; break;
    default: r = c; g = x; b = 0.0f; break;  // case 0, and a dh that rounded to exactly 6
  }
  r += m; g += m; b += m;
}

// The four chains of distort_colour_zero..three (data_augmentation.py:30-63) as four 2-bit op codes each, first op in
// the low bits: 0 brightness, 1 saturation, 2 hue, 3 contrast.
//   zero: B S H C   one: S B C H   two: C H B S   three: H S C B
constexpr uint32_t SF_CHAINS = 228u | (177u << 8) | (75u << 16) | (54u << 24);

// Runs the chain of `c.order` on one pixel; with until_contrast it stops in front of the contrast op (what the stats
// pass sums).  mean: the per-channel means of the sample at that point.  No clipping between the ops.
__device__ __forceinline__ void sf_chain(const sf_colour& c, const float* mean, bool until_contrast, float& r, float& g,
                                         float& b) {
  const uint32_t code = (SF_CHAINS >> (8 * c.order)) & 255u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t op = (code >> (2 * k)) & 3u;
    if (op == 3u) {
      if (until_contrast) return;
      r = (r - mean[0]) * c.f_contrast + mean[0];
      g = (g - mean[1]) * c.f_contrast + mean[1];
      b = (b - mean[2]) * c.f_contrast + mean[2];
    } else if (op == 0u) {
      r += c.d_brightness; g += c.d_brightness; b += c.d_brightness;
    } else {
      float h, s, v;
      sf_rgb_to_hsv(r, g, b, h, s, v);
      if (op == 1u) {
        s = fminf(fmaxf(s * c.f_saturation, 0.0f), 1.0f);
      } else {
        h += c.d_hue;
        h -= floorf(h);
      }
      sf_hsv_to_rgb(h, s, v, r, g, b);
    }
  }
}

// Sum over the block, valid in thread 0.  Lanes -> wave by shuffles, waves -> block through LDS in wave order: the
// same tree every run.  Call from block-uniform control flow only.
template <typename T, int BLOCK>
__device__ __forceinline__ T sf_block_sum(T v, T* lds) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  const int wave = threadIdx.x >> 6;
  __syncthreads();  // lds may still be read from the previous call
  if ((threadIdx.x & 63) == 0) lds[wave] = v;
  __syncthreads();
  T t = 0;
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < BLOCK / 64; ++k) t += lds[k];
  return t;
}

// grid (P, N): block p of sample n owns the source pixels [p * chunk, (p + 1) * chunk) of that sample
__global__ void __launch_bounds__(SF_STATS_BLOCK)
    selflow_stats_kernel(const float* __restrict__ img_a, const float* __restrict__ img_b,
                         const uint32_t* __restrict__ params, const uint32_t* __restrict__ params_b,
                         uint32_t* __restrict__ counts, float* __restrict__ part_a, float* __restrict__ part_b, int H, int W,
                         int P) {
  __shared__ float lds_f[SF_STATS_BLOCK / 64];
  __shared__ uint32_t lds_u[SF_STATS_BLOCK / 64];
  const int n = blockIdx.y, p = blockIdx.x, hw = H * W;
  const int chunk = (hw + P - 1) / P;
  const int i0 = p * chunk, i1 = min(hw, i0 + chunk);
  const uint32_t* pr = params + (size_t)n * FN2_SELFLOW_PARAM_WORDS;
  const sf_sample s = sf_load_sample(pr);
  if (s.distrib == 1u || s.distrib == 2u) {  // (a) block counts, added with integer atomics: exact in any order
    uint32_t c = 0;
    for (int i = i0 + (int)threadIdx.x; i < i1; i += SF_STATS_BLOCK) c += sf_mask(s, i / W, i % W, W) ? 1u : 0u;
    c = sf_block_sum<uint32_t, SF_STATS_BLOCK>(c, lds_u);
    if (threadIdx.x == 0 && c != 0u) atomicAdd(counts + n, c);
  }
  // (b) one fp32 partial per block and channel; the consumer adds the P partials of a sample in index order
  for (int which = 0; which < 2; ++which) {
    const float* img = which ? img_b : img_a;
    if (img == nullptr) continue;
    const sf_colour col = sf_load_colour(which ? params_b + (size_t)n * FN2_SELFLOW_PARAM_WORDS : pr);
    if (!sf_has_colour(col)) continue;
    const float* base = img + (size_t)n * hw * 3;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f;
    for (int i = i0 + (int)threadIdx.x; i < i1; i += SF_STATS_BLOCK) {
      const rgb3_t px = load_rgb(base + (size_t)i * 3);
      float r = px.r, g = px.g, b = px.b;
      sf_permute(s.perm, r, g, b);
      sf_chain(col, nullptr, true, r, g, b);
      sr += r; sg += g; sb += b;
    }
    sr = sf_block_sum<float, SF_STATS_BLOCK>(sr, lds_f);
    sg = sf_block_sum<float, SF_STATS_BLOCK>(sg, lds_f);
    sb = sf_block_sum<float, SF_STATS_BLOCK>(sb, lds_f);
    if (threadIdx.x == 0) {
      float* o = (which ? part_b : part_a) + ((size_t)n * P + p) * 3;
      o[0] = sr; o[1] = sg; o[2] = sb;
    }
  }
}

struct sf_apply_args {
  const float *img_a, *img_b, *matches, *sparse, *edges, *flow;
  float *o_img_a, *o_img_b, *o_matches, *o_sparse, *o_edges, *o_flow;
  const uint32_t *params, *params_b, *counts;
  const float *part_a, *part_b;
  int H, W, P;
};

__device__ __forceinline__ void sf_image(const float* __restrict__ src, float* __restrict__ dst, const sf_sample& s,
                                         const sf_colour& col, const float* mean) {
  const rgb3_t px = load_rgb(src);
  float r = px.r, g = px.g, b = px.b;
  sf_permute(s.perm, r, g, b);
  if (sf_has_colour(col)) {
    sf_chain(col, mean, false, r, g, b);
    r = fminf(fmaxf(r, 0.0f), 1.0f);  // tf.clip_by_value once, after the chain (data_augmentation.py:91)
    g = fminf(fmaxf(g, 0.0f), 1.0f);
    b = fminf(fmaxf(b, 0.0f), 1.0f);
  }
  store_rgb(dst, r, g, b);
}

// grid (gx, N), a grid-stride walk over the output pixels of sample blockIdx.y
__global__ void __launch_bounds__(SF_APPLY_BLOCK) selflow_apply_kernel(const sf_apply_args a) {
  __shared__ float s_mean[6];
  const int n = blockIdx.y, H = a.H, W = a.W, hw = H * W;
  const uint32_t* pr = a.params + (size_t)n * FN2_SELFLOW_PARAM_WORDS;
  const sf_sample s = sf_load_sample(pr);
  sf_colour col_a = sf_load_colour(pr), col_b = col_a;
  if (a.o_img_b != nullptr) col_b = sf_load_colour(a.params_b + (size_t)n * FN2_SELFLOW_PARAM_WORDS);
  const bool colour_a = a.o_img_a != nullptr && sf_has_colour(col_a), colour_b = a.o_img_b != nullptr && sf_has_colour(col_b);
  if (colour_a || colour_b) {  // block-uniform
    if (threadIdx.x < 6) {
      const int which = threadIdx.x / 3, c = threadIdx.x % 3;
      float sum = 0.0f;
      if (which ? colour_b : colour_a) {
        const float* part = (which ? a.part_b : a.part_a) + (size_t)n * a.P * 3 + c;
        for (int k = 0; k < a.P; ++k) sum += part[k * 3];  // index order
      }
      s_mean[threadIdx.x] = sum / (float)hw;
    }
    __syncthreads();
  }
  // sample_from_distribution's guard (data_augmentation.py:513-521), in float32 as there: an almost empty re-sampled mask
  // gives the DeepMatching inputs back.  Without the ground-truth flow nothing can be re-sampled.
  bool resample = (s.distrib == 1u || s.distrib == 2u) && a.flow != nullptr;
  if (resample) resample = 100.0f * ((float)a.counts[n] / (float)hw) >= 0.01f;

  const size_t base = (size_t)n * hw;
  for (int o = blockIdx.x * SF_APPLY_BLOCK + threadIdx.x; o < hw; o += gridDim.x * SF_APPLY_BLOCK) {
    const int y = o / W, x = o - y * W;
    const int ys = s.flip_ud ? H - 1 - y : y, xs = s.flip_lr ? W - 1 - x : x;
    const size_t src = base + (size_t)ys * W + xs, dst = base + o;
    const bool m = resample && sf_mask(s, ys, xs, W);
    float2 gt = make_float2(0.0f, 0.0f);
    if (a.flow != nullptr) gt = *reinterpret_cast<const float2*>(a.flow + src * 2);
    if (a.o_matches != nullptr) a.o_matches[dst] = resample ? (m ? 1.0f : 0.0f) : a.matches[src];
    if (a.o_sparse != nullptr) {
      float2 sf = resample ? (m ? gt : make_float2(0.0f, 0.0f)) : *reinterpret_cast<const float2*>(a.sparse + src * 2);
      if (s.flip_lr) sf.x = -sf.x;
      if (s.flip_ud) sf.y = -sf.y;
      *reinterpret_cast<float2*>(a.o_sparse + dst * 2) = sf;
    }
    if (a.o_flow != nullptr) {
      if (s.flip_lr) gt.x = -gt.x;
      if (s.flip_ud) gt.y = -gt.y;
      *reinterpret_cast<float2*>(a.o_flow + dst * 2) = gt;
    }
    if (a.o_edges != nullptr) a.o_edges[dst] = a.edges[src];
    if (a.o_img_a != nullptr) sf_image(a.img_a + src * 3, a.o_img_a + dst * 3, s, col_a, s_mean);
    if (a.o_img_b != nullptr) sf_image(a.img_b + src * 3, a.o_img_b + dst * 3, s, col_b, s_mean + 3);
  }
}

struct sf_workspace {
  uint32_t* counts;
  float *part_a, *part_b;
};
static inline int64_t sf_workspace_bytes(int n, int h, int w) {
  return sf_align16((int64_t)n * 4) + 2 * sf_align16((int64_t)n * sf_partials(h, w) * 3 * 4);
}
static inline sf_workspace sf_carve(void* ws, int n, int h, int w) {
  char* p = (char*)ws;
  sf_workspace r;
  r.counts = (uint32_t*)p;
  p += sf_align16((int64_t)n * 4);
  r.part_a = (float*)p;
  p += sf_align16((int64_t)n * sf_partials(h, w) * 3 * 4);
  r.part_b = (float*)p;
  return r;
}
static inline bool sf_dims_ok(int n, int h, int w) {
  return n >= 1 && n <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w <= (1LL << 30);
}

}  // namespace fn2

using namespace fn2;

extern "C" {

int64_t fn2_selflow_workspace_bytes(int n, int h, int w) { return sf_dims_ok(n, h, w) ? sf_workspace_bytes(n, h, w) : -1; }

int fn2_selflow_stats(const float* image_a, const float* image_b, const uint32_t* params, const uint32_t* params_b,
                      void* workspace, int64_t ws_bytes, int n, int h, int w, void* stream) {
  FN2_REQUIRE(params && workspace, "selflow_stats: null pointer");
  FN2_REQUIRE(sf_dims_ok(n, h, w), "selflow_stats: bad size n=%d h=%d w=%d", n, h, w);
  FN2_REQUIRE(image_b == nullptr || params_b != nullptr, "selflow_stats: image_b needs its own colour records (params_b)");
  FN2_REQUIRE(((uintptr_t)workspace & 15) == 0, "selflow_stats: workspace must be 16-byte aligned");
  FN2_REQUIRE(ws_bytes >= sf_workspace_bytes(n, h, w), "selflow_stats: workspace of %lld bytes, need %lld",
              (long long)ws_bytes, (long long)sf_workspace_bytes(n, h, w));
  const sf_workspace ws = sf_carve(workspace, n, h, w);
  hipStream_t s = (hipStream_t)stream;
  FN2_HIP(hipMemsetAsync(ws.counts, 0, (size_t)n * 4, s));
  const int P = sf_partials(h, w);
  hipLaunchKernelGGL(selflow_stats_kernel, dim3(P, n), dim3(SF_STATS_BLOCK), 0, s, image_a, image_b, params, params_b,
                     ws.counts, ws.part_a, ws.part_b, h, w, P);
  FN2_CHECK_LAUNCH("selflow_stats");
  return FN2_OK;
}

int fn2_selflow_apply(const float* image_a, const float* image_b, const float* matches, const float* sparse_flow,
                      const float* edges, const float* flow, float* out_image_a, float* out_image_b, float* out_matches,
                      float* out_sparse_flow, float* out_edges, float* out_flow, const uint32_t* params,
                      const uint32_t* params_b, const void* workspace, int64_t ws_bytes, int n, int h, int w,
                      void* stream) {
  FN2_REQUIRE(params && workspace, "selflow_apply: null pointer");
  FN2_REQUIRE(sf_dims_ok(n, h, w), "selflow_apply: bad size n=%d h=%d w=%d", n, h, w);
  FN2_REQUIRE(out_image_a || out_image_b || out_matches || out_sparse_flow || out_edges || out_flow,
              "selflow_apply: no output");
  FN2_REQUIRE((!out_image_a || image_a) && (!out_image_b || image_b) && (!out_matches || matches) &&
                  (!out_sparse_flow || sparse_flow) && (!out_edges || edges) && (!out_flow || flow),
              "selflow_apply: an output without its input");
  FN2_REQUIRE(out_image_b == nullptr || params_b != nullptr, "selflow_apply: image_b needs its own colour records (params_b)");
  FN2_REQUIRE((((uintptr_t)sparse_flow | (uintptr_t)flow | (uintptr_t)out_sparse_flow | (uintptr_t)out_flow) & 7) == 0,
              "selflow_apply: flows must be 8-byte aligned");
  FN2_REQUIRE(((uintptr_t)workspace & 15) == 0, "selflow_apply: workspace must be 16-byte aligned");
  FN2_REQUIRE(ws_bytes >= sf_workspace_bytes(n, h, w), "selflow_apply: workspace of %lld bytes, need %lld",
              (long long)ws_bytes, (long long)sf_workspace_bytes(n, h, w));
  const sf_workspace ws = sf_carve(const_cast<void*>(workspace), n, h, w);
  sf_apply_args a;
  a.img_a = image_a; a.img_b = image_b; a.matches = matches; a.sparse = sparse_flow; a.edges = edges; a.flow = flow;
  a.o_img_a = out_image_a; a.o_img_b = out_image_b; a.o_matches = out_matches; a.o_sparse = out_sparse_flow;
  a.o_edges = out_edges; a.o_flow = out_flow;
  a.params = params; a.params_b = params_b; a.counts = ws.counts; a.part_a = ws.part_a; a.part_b = ws.part_b;
  a.H = h; a.W = w; a.P = sf_partials(h, w);
  // four pixels a lane until the grid cap (aug.hip aug_grid: 256 * 32 blocks) is reached, so that the per-block
  // prologue (the record, the ordered sum of the partials) is paid once per 1024 pixels
  long gx = ((long)h * w + 4 * SF_APPLY_BLOCK - 1) / (4 * SF_APPLY_BLOCK);
  const long cap = 256L * 32 / n;
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(selflow_apply_kernel, dim3((unsigned)gx, n), dim3(SF_APPLY_BLOCK), 0, (hipStream_t)stream, a);
  FN2_CHECK_LAUNCH("selflow_apply");
  return FN2_OK;
}

}  // extern "C"
