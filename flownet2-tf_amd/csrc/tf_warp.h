// tf_warp's index rules (src/utils.py:453-515) and the wave-per-row-segment walk, shared by occlusion.hip and
// photometric.hip.
//
// tf_warp is NOT flow_warp (ops.hip): there is no in-range test.  The coordinate is truncated toward zero, the two
// taps of an axis are clamped to the image AFTER the +1, and the weights are formed from the clamped tap positions and
// the UNCLAMPED coordinate.  So x = -0.25 reads columns 0 and 1 with weights 1.25 and -0.25 (it extrapolates), and
// wherever both taps of an axis clamp to one index the two weights cancel: the result is exactly 0 for x <= -1, for
// x >= W - 1 and everywhere in a 1-wide image.
#pragma once
#include "fn2_common.h"

namespace fn2 {
namespace {

// tf.cast(float -> int32) made safe for every input: NaN -> 0, anything else saturates.  The bounds -2 and size + 1
// already lie outside what the clamp below can tell apart, and truncation commutes with a clamp to integer bounds, so
// every coordinate the reference defines gets the reference's index.
__device__ __forceinline__ int trunc_sat(float v, int size) {
  if (!(v == v)) return 0;
  return (int)fminf(fmaxf(v, -2.0f), (float)size + 1.0f);
}

struct TfTaps {
  int x0, x1, y0, y1;
  float wa, wb, wc, wd;
};

// taps and weights of the sample position (x, y)
__device__ __forceinline__ TfTaps tf_taps_at(float x, float y, int W, int H) {
  TfTaps t;
  const int tx = trunc_sat(x, W), ty = trunc_sat(y, H);  // :477-480
  t.x0 = min(max(tx, 0), W - 1);                      // :483-486
  t.x1 = min(max(tx + 1, 0), W - 1);
  t.y0 = min(max(ty, 0), H - 1);
  t.y1 = min(max(ty + 1, 0), H - 1);
  const float x0f = (float)t.x0, x1f = (float)t.x1, y0f = (float)t.y0, y1f = (float)t.y1;  // :495-498
  t.wa = (x1f - x) * (y1f - y);                       // :502-505
  t.wb = (x1f - x) * (y - y0f);
  t.wc = (x - x0f) * (y1f - y);
  t.wd = (x - x0f) * (y - y0f);
  return t;
}

__device__ __forceinline__ TfTaps tf_taps(int px, int py, float u, float v, int W, int H) {
  return tf_taps_at((float)px + u, (float)py + v, W, H);  // :467, :473-474
}

// tf.add_n([wa*Ia, wb*Ib, wc*Ic, wd*Id]) (:514), left to right
__device__ __forceinline__ float tf_blend(const TfTaps& t, float a, float b, float c, float d) {
  return ((t.wa * a + t.wb * b) + t.wc * c) + t.wd * d;
}

__device__ __forceinline__ float2 ld2(const float* p) { return *reinterpret_cast<const float2*>(p); }

// (image, row, first column) of the unit a wave works on
struct Unit {
  int64_t n;
  int y, x;
};
__device__ __forceinline__ Unit unit_at(int64_t u, int H, int segs) {
  Unit r;
  const int64_t row = u / segs;
  r.x = (int)(u - row * segs) * 64 + (int)(threadIdx.x & 63);
  r.n = row / H;
  r.y = (int)(row - r.n * H);
  return r;
}

}  // namespace
}  // namespace fn2
