// Forward-backward occlusion check of the reference (src/utils.py:426-538: get_pixel_value, tf_warp, length_sq,
// occlusion -- the SelFlow consistency test), which the reference never ran: its comment at :424 says the check was
// not adapted to the warping operator the networks use.
//
// tf_warp is NOT flow_warp (ops.hip): there is no in-range test.  The coordinate is truncated toward zero, the two
// taps of an axis are clamped to the image AFTER the +1, and the weights are formed from the clamped tap positions and
// the UNCLAMPED coordinate.  So x = -0.25 reads columns 0 and 1 with weights 1.25 and -0.25 (it extrapolates), and
// wherever both taps of an axis clamp to one index the two weights cancel: the result is exactly 0 for x <= -1, for
// x >= W - 1 and everywhere in a 1-wide image.
//
// One pixel per lane, a wave along x: a wave owns 64 consecutive pixels of one row, so its own flows are one coalesced
// 512-byte run and, for a smooth flow, the taps of neighbouring lanes are neighbours too (served from L2).  Waves walk
// the (image, row, 64-pixel segment) units with a grid-stride loop: the block count is bounded for any size.
#include "tf_warp.h"

namespace fn2 {
namespace {

constexpr int OCC_BLOCK = 256;                  // four waves, each on its own unit
constexpr int OCC_WAVES = OCC_BLOCK / 64;
constexpr int OCC_MAX_BLOCKS = 4096;

// tf_warp of a two-channel map `src` (one image: row pitch in floats) at pixel (px, py) displaced by (u, v)
__device__ __forceinline__ float2 tf_warp_c2(const float* __restrict__ src, int64_t pitch, int px, int py, float u,
                                             float v, int W, int H) {
  const TfTaps t = tf_taps(px, py, u, v, W, H);
  const float* r0 = src + (int64_t)t.y0 * pitch;
  const float* r1 = src + (int64_t)t.y1 * pitch;
  const float2 a = ld2(r0 + 2 * t.x0), b = ld2(r1 + 2 * t.x0), c = ld2(r0 + 2 * t.x1), d = ld2(r1 + 2 * t.x1);
  return make_float2(tf_blend(t, a.x, b.x, c.x, d.x), tf_blend(t, a.y, b.y, c.y, d.y));
}

__global__ void __launch_bounds__(OCC_BLOCK) tf_warp_kernel(const float* __restrict__ img, int64_t img_pitch,
                                                            int64_t img_bstride, const float* __restrict__ flow,
                                                            int64_t flow_pitch, int64_t flow_bstride,
                                                            float* __restrict__ out, int N, int H, int W, int C) {
  const int segs = (W + 63) / 64;
  const int64_t units = (int64_t)N * H * segs;
  for (int64_t u = (int64_t)blockIdx.x * OCC_WAVES + (threadIdx.x >> 6); u < units; u += (int64_t)gridDim.x * OCC_WAVES) {
    const Unit p = unit_at(u, H, segs);
    if (p.x >= W) continue;
    const float2 f = ld2(flow + p.n * flow_bstride + (int64_t)p.y * flow_pitch + 2 * p.x);
    const TfTaps t = tf_taps(p.x, p.y, f.x, f.y, W, H);
    const float* base = img + p.n * img_bstride;
    const float* pa = base + (int64_t)t.y0 * img_pitch + (int64_t)t.x0 * C;
    const float* pb = base + (int64_t)t.y1 * img_pitch + (int64_t)t.x0 * C;
    const float* pc = base + (int64_t)t.y0 * img_pitch + (int64_t)t.x1 * C;
    const float* pd = base + (int64_t)t.y1 * img_pitch + (int64_t)t.x1 * C;
    float* po = out + ((p.n * H + p.y) * W + p.x) * C;
    for (int c = 0; c < C; ++c) po[c] = tf_blend(t, pa[c], pb[c], pc[c], pd[c]);
  }
}

__device__ __forceinline__ void store_mask(float* p, bool v) { *p = v ? 1.0f : 0.0f; }
__device__ __forceinline__ void store_mask(uint8_t* p, bool v) { *p = v ? (uint8_t)255 : (uint8_t)0; }

// occlusion() (:523-538) for both directions: per pixel 2 coalesced + 8 gathered 8-byte loads and 2 mask stores; the
// warped flows live in registers only.
template <typename M>
__global__ void __launch_bounds__(OCC_BLOCK) fb_occlusion_kernel(const float* __restrict__ fw, const float* __restrict__ bw,
                                                                 int64_t pitch, int64_t bstride, M* __restrict__ occ_fw,
                                                                 M* __restrict__ occ_bw, int N, int H, int W, float alpha,
                                                                 float beta) {
  const int segs = (W + 63) / 64;
  const int64_t units = (int64_t)N * H * segs;
  for (int64_t u = (int64_t)blockIdx.x * OCC_WAVES + (threadIdx.x >> 6); u < units; u += (int64_t)gridDim.x * OCC_WAVES) {
    const Unit p = unit_at(u, H, segs);
    if (p.x >= W) continue;
    const float* fw_n = fw + p.n * bstride;
    const float* bw_n = bw + p.n * bstride;
    const int64_t own = (int64_t)p.y * pitch + 2 * p.x;
    const float2 f = ld2(fw_n + own), b = ld2(bw_n + own);
    const float2 bww = tf_warp_c2(bw_n, pitch, p.x, p.y, f.x, f.y, W, H);  // flow_bw_warped, :527
    const float2 fww = tf_warp_c2(fw_n, pitch, p.x, p.y, b.x, b.y, W, H);  // flow_fw_warped, :528
    const float sfx = f.x + bww.x, sfy = f.y + bww.y, sbx = b.x + fww.x, sby = b.y + fww.y;  // :529-530
    const float d_fw = sfx * sfx + sfy * sfy, d_bw = sbx * sbx + sby * sby;
    const float m_fw = (f.x * f.x + f.y * f.y) + (bww.x * bww.x + bww.y * bww.y);  // :531-532
    const float m_bw = (b.x * b.x + b.y * b.y) + (fww.x * fww.x + fww.y * fww.y);
    const int64_t o = (p.n * H + p.y) * W + p.x;
    store_mask(occ_fw + o, d_fw > alpha * m_fw + beta);  // :533-536; a NaN compares false
    store_mask(occ_bw + o, d_bw > alpha * m_bw + beta);
  }
}

int occ_grid(int n, int h, int w) {
  const int64_t units = (int64_t)n * h * ((w + 63) / 64);
  const int64_t blocks = (units + OCC_WAVES - 1) / OCC_WAVES;
  return (int)(blocks < OCC_MAX_BLOCKS ? blocks : OCC_MAX_BLOCKS);
}

// float2 loads: the flow base 8-byte aligned, pitch and batch stride even
bool flow_aligned(const float* p, int64_t pitch, int64_t bstride) {
  return (reinterpret_cast<uintptr_t>(p) & 7) == 0 && (pitch & 1) == 0 && (bstride & 1) == 0;
}

}  // namespace
}  // namespace fn2

using namespace fn2;

extern "C" int fn2_tf_warp_f32(const float* img, int64_t img_pitch, int64_t img_bstride, const float* flow,
                               int64_t flow_pitch, int64_t flow_bstride, float* out, int n, int h, int w, int c,
                               void* stream) {
  FN2_REQUIRE(img && flow && out, "tf_warp: null pointer");
  FN2_REQUIRE(n >= 1 && h >= 1 && w >= 1 && c >= 1, "tf_warp: bad size n=%d h=%d w=%d c=%d", n, h, w, c);
  FN2_REQUIRE((int64_t)h * w <= (1LL << 30), "tf_warp: image too large (%d x %d)", h, w);
  FN2_REQUIRE(img_pitch >= (int64_t)c * w, "tf_warp: img_pitch %lld < c * w", (long long)img_pitch);
  FN2_REQUIRE(n == 1 || img_bstride >= img_pitch * h, "tf_warp: img_bstride %lld < img_pitch * h",
              (long long)img_bstride);
  FN2_REQUIRE(flow_pitch >= 2LL * w, "tf_warp: flow_pitch %lld < 2 * w", (long long)flow_pitch);
  FN2_REQUIRE(n == 1 || flow_bstride >= flow_pitch * h, "tf_warp: flow_bstride %lld < flow_pitch * h",
              (long long)flow_bstride);
  FN2_REQUIRE(flow_aligned(flow, flow_pitch, flow_bstride),
              "tf_warp: flow must be 8-byte aligned with an even pitch and batch stride");
  hipLaunchKernelGGL(tf_warp_kernel, dim3(occ_grid(n, h, w)), dim3(OCC_BLOCK), 0, (hipStream_t)stream, img, img_pitch,
                     img_bstride, flow, flow_pitch, flow_bstride, out, n, h, w, c);
  FN2_CHECK_LAUNCH("tf_warp");
  return FN2_OK;
}

extern "C" int fn2_fb_occlusion(const float* flow_fw, const float* flow_bw, int64_t flow_pitch, int64_t flow_bstride,
                                void* occ_fw, void* occ_bw, int mask_dtype, int n, int h, int w, float alpha,
                                float beta, void* stream) {
  FN2_REQUIRE(flow_fw && flow_bw && occ_fw && occ_bw, "fb_occlusion: null pointer");
  FN2_REQUIRE(n >= 1 && h >= 1 && w >= 1, "fb_occlusion: bad size n=%d h=%d w=%d", n, h, w);
  FN2_REQUIRE((int64_t)h * w <= (1LL << 30), "fb_occlusion: image too large (%d x %d)", h, w);
  FN2_REQUIRE(flow_pitch >= 2LL * w, "fb_occlusion: flow_pitch %lld < 2 * w", (long long)flow_pitch);
  FN2_REQUIRE(n == 1 || flow_bstride >= flow_pitch * h, "fb_occlusion: flow_bstride %lld < flow_pitch * h",
              (long long)flow_bstride);
  FN2_REQUIRE(flow_aligned(flow_fw, flow_pitch, flow_bstride) && flow_aligned(flow_bw, flow_pitch, flow_bstride),
              "fb_occlusion: flows must be 8-byte aligned with an even pitch and batch stride");
  FN2_REQUIRE(mask_dtype == FN2_MASK_F32 || mask_dtype == FN2_MASK_U8, "fb_occlusion: unknown mask_dtype %d", mask_dtype);
  const dim3 grid(occ_grid(n, h, w)), block(OCC_BLOCK);
  if (mask_dtype == FN2_MASK_F32)
    hipLaunchKernelGGL(fb_occlusion_kernel<float>, grid, block, 0, (hipStream_t)stream, flow_fw, flow_bw, flow_pitch,
                       flow_bstride, (float*)occ_fw, (float*)occ_bw, n, h, w, alpha, beta);
  else
    hipLaunchKernelGGL(fb_occlusion_kernel<uint8_t>, grid, block, 0, (hipStream_t)stream, flow_fw, flow_bw, flow_pitch,
                       flow_bstride, (uint8_t*)occ_fw, (uint8_t*)occ_bw, n, h, w, alpha, beta);
  FN2_CHECK_LAUNCH("fb_occlusion");
  return FN2_OK;
}
