// HBM-bound fused elementwise kernels between the sub-networks of the stacked models.
// One lane per pixel; the 16-channel (padded) input row of the next network is assembled in
// registers and written with 16-byte stores, so flow_warp + brightness error + concat
// (flownet_cs.py:21-36) and ChannelNorm x4 + flow_warp x2 + concat (flownet2.py:25-47) are one
// pass over the images instead of 6-10 TF nodes.
#include "fn2_common.h"

namespace fn2 {

// bilinear warp of a 3-channel fp32 image, exact reference rules (flow_warp.cu.cc:44-95)
__device__ __forceinline__ void warp3(const float* __restrict__ img, long nb, int x, int y, float u, float v,
                                      int W, int H, float o[3]) {
  const float x2 = (float)x + u, y2 = (float)y + v;
  o[0] = o[1] = o[2] = 0.f;
  if (!((x2 >= 0.f) && (y2 >= 0.f) && (x2 < (float)W) && (y2 < (float)H))) return;
  const int xL = (int)x2, yT = (int)y2;
  const int xR = min(xL + 1, W - 1), yB = min(yT + 1, H - 1);
  const float al = x2 - (float)xL, be = y2 - (float)yT;
  const float cTL = (1.f - al) * (1.f - be), cTR = al * (1.f - be), cBL = (1.f - al) * be, cBR = al * be;
  // 12-byte tap loads (fn2_common.h rgb3_t); same expression per channel as flow_warp_kernel
  const rgb3_t tl = load_rgb(img + (nb + (long)yT * W + xL) * 3), tr = load_rgb(img + (nb + (long)yT * W + xR) * 3);
  const rgb3_t bl = load_rgb(img + (nb + (long)yB * W + xL) * 3), br = load_rgb(img + (nb + (long)yB * W + xR) * 3);
  o[0] = cTL * tl.r + cTR * tr.r + cBL * bl.r + cBR * br.r;
  o[1] = cTL * tl.g + cTR * tr.g + cBL * bl.g + cBR * br.g;
  o[2] = cTL * tl.b + cTR * tr.b + cBL * bl.b + cBR * br.b;
}

// ChannelNorm of a flow vector (flownet2.py:25-31).  The squares of a finite vector overflow fp32 beyond |v| ~ 1.8e19
// although its norm is representable: only then is it taken again on the vector scaled by 2^-70 (exact), so every
// other input -- NaN and infinite flows included -- gives the bits of the plain expression.
__device__ __forceinline__ float norm2(float x, float y) {
  float r = sqrtf(x * x + y * y);
  if (r == INFINITY && fabsf(x) < INFINITY && fabsf(y) < INFINITY) {
    x *= 0x1p-70f;
    y *= 0x1p-70f;
    r = sqrtf(x * x + y * y) * 0x1p70f;
  }
  return r;
}

// A full-resolution flow field given either as itself (ph == 0: `p` is [N,H,W,2]) or as the quarter-resolution
// predict_flow2 it is resized from (`flow = resize_bilinear(scale * predict_flow2)`, align_corners, flownet_s.py:105-109):
// then the consumer interpolates its pixel itself -- resize_bilinear_c2_kernel's arithmetic, operation for operation --
// and, when `keep` is set, stores it there as the resize launch would have.
struct FlowSrc { const float* p; int ph, pw; float sy, sx, scale; float* keep; };

__device__ __forceinline__ float2 flow_at(const FlowSrc& f, int n, int y, int x, long pix) {
  if (f.ph == 0) return *reinterpret_cast<const float2*>(f.p + pix * 2);
  int y0, y1, x0, x1;
  float ly, lx;
  resize_coord(y, f.sy, f.ph, y0, y1, ly);
  resize_coord(x, f.sx, f.pw, x0, x1, lx);
  const float2* r0 = reinterpret_cast<const float2*>(f.p) + ((long)n * f.ph + y0) * f.pw;
  const float2* r1 = reinterpret_cast<const float2*>(f.p) + ((long)n * f.ph + y1) * f.pw;
  float2 r = bilerp_c2(r0[x0], r0[x1], r1[x0], r1[x1], lx, ly, f.scale);
  // the vector is used as the resize launch would have STORED it: without this the final multiply by `scale` contracts
  // with the consumer's first addition (x + u in the warp) and the results differ in the last bit
  asm volatile("" : "+v"(r.x), "+v"(r.y));
  if (f.keep != nullptr) *reinterpret_cast<float2*>(f.keep + pix * 2) = r;
  return r;
}

template <typename OutT>
__global__ void __launch_bounds__(256) stack_input_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          const FlowSrc flow, OutT* __restrict__ out,
                                                          int N, int H, int W, int out_cs, int out_c0, int pad) {
  const long npix = (long)N * H * W;
  for (long pix = (long)blockIdx.x * blockDim.x + threadIdx.x; pix < npix; pix += (long)gridDim.x * blockDim.x) {
    const int x = (int)(pix % W), y = (int)((pix / W) % H);
    const long nb = (pix / W / H) * (long)H * W;
    const float2 f = flow_at(flow, (int)(pix / W / H), y, x, pix);
    float wv[3];
    warp3(b, nb, x, y, f.x, f.y, W, H, wv);
    float v[16];
    float e = 0.f;
    const rgb3_t pa = load_rgb(a + pix * 3), pb = load_rgb(b + pix * 3);
    const float av3[3] = {pa.r, pa.g, pa.b}, bv3[3] = {pb.r, pb.g, pb.b};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float av = av3[c];
      v[c] = av;
      v[3 + c] = bv3[c];
      v[6 + c] = wv[c];
      const float d = av - wv[c];
      e += d * d;
    }
    {
      // the ROUNDED fp32 product in every storage format: left contractable, the split-fp16 store's `v - hi` fused with
      // this multiply (in channel 9 only) and its lo part came from the unrounded product, not from the value f32 stores
#pragma clang fp contract(off)
      v[9] = f.x * 0.05f;   // flownet_cs.py:34
      v[10] = f.y * 0.05f;
    }
    v[11] = sqrtf(e);     // brightness error, flownet_cs.py:24-27
    v[12] = v[13] = v[14] = v[15] = 0.f;
    const size_t opix = ((size_t)(pix / W / H) * (H + 2 * pad) + y + pad) * (W + 2 * pad) + x + pad;
    store16<OutT>(out + opix * out_cs + out_c0, v);
  }
}

template <typename OutT>
__global__ void __launch_bounds__(256) fusion_input_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           const FlowSrc fsd, const FlowSrc fcss, OutT* __restrict__ out,
                                                           int N, int H, int W, int out_cs, int out_c0, int pad) {
  const long npix = (long)N * H * W;
  for (long pix = (long)blockIdx.x * blockDim.x + threadIdx.x; pix < npix; pix += (long)gridDim.x * blockDim.x) {
    const int x = (int)(pix % W), y = (int)((pix / W) % H);
    const long nb = (pix / W / H) * (long)H * W;
    const float2 sd = flow_at(fsd, (int)(pix / W / H), y, x, pix);
    const float2 cs = flow_at(fcss, (int)(pix / W / H), y, x, pix);
    float wsd[3], wcs[3];
    warp3(b, nb, x, y, sd.x, sd.y, W, H, wsd);  // flownet2.py:33
    warp3(b, nb, x, y, cs.x, cs.y, W, H, wcs);  // flownet2.py:37
    float v[16];
    float esd = 0.f, ecs = 0.f;
    const rgb3_t pa = load_rgb(a + pix * 3);
    const float av3[3] = {pa.r, pa.g, pa.b};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float av = av3[c];
      v[c] = av;
      const float d1 = av - wsd[c], d2 = av - wcs[c];
      esd += d1 * d1;
      ecs += d2 * d2;
    }
    v[3] = sd.x; v[4] = sd.y; v[5] = cs.x; v[6] = cs.y;           // flownet2.py:41-43
    v[7] = norm2(sd.x, sd.y);                                      // ChannelNorm(flow_sd), :30
    v[8] = norm2(cs.x, cs.y);                                      // ChannelNorm(flow_css), :31
    v[9] = sqrtf(esd);                                             // :35
    v[10] = sqrtf(ecs);                                            // :39
    v[11] = v[12] = v[13] = v[14] = v[15] = 0.f;
    const size_t opix = ((size_t)(pix / W / H) * (H + 2 * pad) + y + pad) * (W + 2 * pad) + x + pad;
    store16<OutT>(out + opix * out_cs + out_c0, v);
  }
}

static inline int grid_for(long work_items, int block) {
  long g = (work_items + block - 1) / block;
  if (g > 256L * 16) g = 256L * 16;
  if (g < 1) g = 1;
  return (int)g;
}

static int check_out16(const fn2_tensor* out, int c, int pad, const char* what) {
  FN2_REQUIRE(out && out->data, "%s: null output", what);
  FN2_REQUIRE(out->n >= 1 && out->c == c, "%s: output view must have %d channels and n >= 1", what, c);
  FN2_REQUIRE(out->c0 >= 0 && out->cs % 8 == 0 && out->c0 % 8 == 0 && out->c0 + 16 <= out->cs,
              "%s: output needs a 16-channel, 8-aligned slot", what);
  FN2_REQUIRE(out->dtype >= FN2_F32 && out->dtype <= FN2_F16X2, "%s: bad dtype", what);
  FN2_REQUIRE(pad >= 0 && out->h > 2 * pad && out->w > 2 * pad, "%s: bad border", what);
  FN2_REQUIRE(((size_t)out->data & 15) == 0, "%s: output must be 16-byte aligned", what);  // the 16-byte group stores
  return FN2_OK;
}

// the 12-byte rgb loads need 4-byte alignment, the float2 flow loads and stores 8-byte (a null flow_out passes)
static int check_in_align(const float* a, const float* b, const float* f0, const float* f1, const float* f2, const float* f3,
                          const char* what) {
  FN2_REQUIRE((((size_t)a | (size_t)b) & 3) == 0, "%s: images must be 4-byte aligned", what);
  FN2_REQUIRE((((size_t)f0 | (size_t)f1 | (size_t)f2 | (size_t)f3) & 7) == 0, "%s: flows must be 8-byte aligned", what);
  return FN2_OK;
}

}  // namespace fn2

using namespace fn2;

// FlowNetS_interp stem input from the bytes the files decode to: [image rgb | 0.05 * sparse_flow uv | matches | 0 0]
// (flownet_s_interp.py:34-38) in the interior of the padded 8-channel stem view -- the view, border and storage formats
// of pack_image_kernel<OutT, 2> (conv.hip).  The byte -> float step is the table of u8_to_f32_lut_kernel
// (float32(float64(i) / 255.0)): adapt_x's `/ 255.0` (net.py:334-345) per input whose max exceeds 1, which the
// per-sample flags carry (flags[2n]: image, flags[2n+1]: mask; cleared = the byte as it is, float32(i)).  The flags are
// read from device memory, so one captured launch serves any mix of samples.  HBM-bound: 12 bytes in, one 8-channel
// group out per lane (one 16-byte store for the 16-bit formats, two for the 4-byte ones); the 64 lanes of a wave read
// 192 + 64 contiguous image / mask bytes and 512 contiguous bytes of sparse flow.
template <typename OutT>
__global__ void __launch_bounds__(256) pack_interp_u8_kernel(const unsigned char* __restrict__ img,
                                                             const unsigned char* __restrict__ mask,
                                                             const float* __restrict__ sparse,
                                                             const float* __restrict__ lut,
                                                             const unsigned char* __restrict__ flags,
                                                             OutT* __restrict__ out, int n, int h, int w, int pad,
                                                             int out_cs, int c0) {
  __shared__ float t[512];  // [0, 256): the byte as it is; [256, 512): the byte / 255 -- a flag is an offset, not a branch
  t[threadIdx.x] = (float)threadIdx.x;
  t[256 + threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const unsigned npix = (unsigned)n * h * w;  // < 2^31 (checked by the caller): 32-bit index arithmetic
  const int hp = h + 2 * pad, wp = w + 2 * pad;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
    const unsigned row = i / (unsigned)w;
    const int x = (int)(i - row * w), nn = (int)(row / (unsigned)h), y = (int)(row - nn * h);
    const unsigned char* p = img + (size_t)i * 3;
    const unsigned r = p[0], g = p[1], b = p[2], m = mask[i];
    const float2 sf = *reinterpret_cast<const float2*>(sparse + (size_t)i * 2);
    const unsigned ti = flags[2 * nn] ? 256u : 0u, tm = flags[2 * nn + 1] ? 256u : 0u;
    float v[8];
    v[0] = t[ti + r];
    v[1] = t[ti + g];
    v[2] = t[ti + b];
    v[3] = sf.x * 0.05f;  // flownet_s_interp.py:36
    v[4] = sf.y * 0.05f;
    v[5] = t[tm + m];
    v[6] = v[7] = 0.f;
    OutT* d = out + (((size_t)nn * hp + y + pad) * wp + x + pad) * out_cs + c0;
    if constexpr (is_x2<OutT>::value) {
      uint4* q = reinterpret_cast<uint4*>(d);
      split8(v, q[0], q[1]);
    } else if constexpr (sizeof(OutT) == 2) {
      store_vec<OutT, 8>(d, v);
    } else {
      store_vec<OutT, 4>(d, v);
      store_vec<OutT, 4>(d + 4, v + 4);
    }
  }
}

// uint8 image bytes -> fp32 through a 256-entry table: what Net.adapt_x does on the host (src/net.py:338-345:
// `x / 255.0` in float64 when the image's max exceeds 1, else the values as they are, then the float32 feed) done
// after the copy, so the host link carries one byte per channel instead of four.  The table IS the host arithmetic
// (lut[i] = float32(float64(i) / 255.0) or float32(i)), hence the result is byte-identical to the fp32 path.
// HBM-bound: 16 bytes in, 64 bytes out per lane.
__global__ void __launch_bounds__(256) u8_to_f32_lut_kernel(const unsigned char* __restrict__ src,
                                                            const float* __restrict__ lut, float* __restrict__ dst,
                                                            long count) {
  __shared__ float t[256];
  t[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const long n16 = count >> 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x) {
    const uint4 v = reinterpret_cast<const uint4*>(src)[i];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    float4* o = reinterpret_cast<float4*>(dst) + i * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      o[j] = make_float4(t[w[j] & 255u], t[(w[j] >> 8) & 255u], t[(w[j] >> 16) & 255u], t[w[j] >> 24]);
  }
  if (blockIdx.x == 0)  // ragged tail (counts that are not multiples of 16)
    for (long i = (n16 << 4) + threadIdx.x; i < count; i += blockDim.x) dst[i] = t[src[i]];
}

extern "C" {

int fn2_u8_to_f32_lut(const unsigned char* src, const float* lut256, float* dst, long count, void* stream) {
  FN2_REQUIRE(src && lut256 && dst && count >= 0, "u8_to_f32_lut: null pointer / negative count");
  FN2_REQUIRE(((size_t)src & 15) == 0 && ((size_t)dst & 15) == 0, "u8_to_f32_lut: src and dst must be 16-byte aligned");
  if (count == 0) return FN2_OK;
  hipLaunchKernelGGL(u8_to_f32_lut_kernel, dim3(grid_for(count >> 4, 256)), dim3(256), 0, (hipStream_t)stream, src,
                     lut256, dst, count);
  FN2_CHECK_LAUNCH("u8_to_f32_lut");
  return FN2_OK;
}

int fn2_pack_interp_u8(const unsigned char* img, const unsigned char* mask, const float* sparse, const float* lut256,
                       const unsigned char* flags, const fn2_tensor* out, int pad, void* stream) {
  FN2_REQUIRE(img && mask && sparse && lut256 && flags, "pack_interp_u8: null pointer");
  FN2_REQUIRE(out && out->data, "pack_interp_u8: null output");
  FN2_REQUIRE(out->dtype >= FN2_F32 && out->dtype <= FN2_F16X2, "pack_interp_u8: bad dtype");
  FN2_REQUIRE(out->n >= 1 && out->c == 6, "pack_interp_u8: output view must have 6 channels");
  FN2_REQUIRE(out->c0 >= 0 && out->c0 % 8 == 0 && out->cs % 8 == 0 && out->c0 + 8 <= out->cs,
              "pack_interp_u8: needs an 8-channel aligned slot");
  FN2_REQUIRE(pad >= 0 && out->h > 2 * pad && out->w > 2 * pad, "pack_interp_u8: bad border");
  // the 8-byte sparse-flow load and the 16-byte group stores
  FN2_REQUIRE(((size_t)sparse & 7) == 0 && ((size_t)lut256 & 3) == 0, "pack_interp_u8: sparse must be 8-byte aligned");
  FN2_REQUIRE(((size_t)out->data & 15) == 0, "pack_interp_u8: output must be 16-byte aligned");
  const int h = out->h - 2 * pad, w = out->w - 2 * pad;
  const long npix = (long)out->n * h * w;
  FN2_REQUIRE(npix < (1L << 31), "pack_interp_u8: more than 2^31 pixels");
  const dim3 g(grid_for(npix, 256)), b(256);
  hipStream_t s = (hipStream_t)stream;
  if (out->dtype == FN2_F32)
    hipLaunchKernelGGL(pack_interp_u8_kernel<float>, g, b, 0, s, img, mask, sparse, lut256, flags, (float*)out->data,
                       out->n, h, w, pad, out->cs, out->c0);
  else if (out->dtype == FN2_F16X2)
    hipLaunchKernelGGL(pack_interp_u8_kernel<x2_t>, g, b, 0, s, img, mask, sparse, lut256, flags, (x2_t*)out->data,
                       out->n, h, w, pad, out->cs, out->c0);
  else if (out->dtype == FN2_BF16)
    hipLaunchKernelGGL(pack_interp_u8_kernel<bf16_t>, g, b, 0, s, img, mask, sparse, lut256, flags, (bf16_t*)out->data,
                       out->n, h, w, pad, out->cs, out->c0);
  else
    hipLaunchKernelGGL(pack_interp_u8_kernel<f16_t>, g, b, 0, s, img, mask, sparse, lut256, flags, (f16_t*)out->data,
                       out->n, h, w, pad, out->cs, out->c0);
  FN2_CHECK_LAUNCH("pack_interp_u8");
  return FN2_OK;
}

static FlowSrc flow_src(const float* p, int ph, int pw, float scale, float* keep, int out_h, int out_w) {
  FlowSrc f{p, ph, pw, 0.f, 0.f, scale, keep};
  if (ph > 0) {   // fn2_resize_bilinear_f32's scales
    f.sy = out_h > 1 ? (float)(ph - 1) / (float)(out_h - 1) : 0.f;
    f.sx = out_w > 1 ? (float)(pw - 1) / (float)(out_w - 1) : 0.f;
  }
  return f;
}

static int stack_input_launch(const float* a, const float* b, const FlowSrc& f, const fn2_tensor* out, int pad, void* stream) {
  const long npix = (long)out->n * (out->h - 2 * pad) * (out->w - 2 * pad);
  if (out->dtype == FN2_F32)
    hipLaunchKernelGGL(stack_input_kernel<float>, dim3(grid_for(npix, 256)), dim3(256), 0, (hipStream_t)stream, a,
                       b, f, (float*)out->data, out->n, out->h - 2 * pad, out->w - 2 * pad, out->cs, out->c0, pad);
  else if (out->dtype == FN2_F16X2)
    hipLaunchKernelGGL(stack_input_kernel<x2_t>, dim3(grid_for(npix, 256)), dim3(256), 0, (hipStream_t)stream, a,
                       b, f, (x2_t*)out->data, out->n, out->h - 2 * pad, out->w - 2 * pad, out->cs, out->c0, pad);
  else if (out->dtype == FN2_BF16)
    hipLaunchKernelGGL(stack_input_kernel<bf16_t>, dim3(grid_for(npix, 256)), dim3(256), 0, (hipStream_t)stream, a,
                       b, f, (bf16_t*)out->data, out->n, out->h - 2 * pad, out->w - 2 * pad, out->cs, out->c0, pad);
  else
    hipLaunchKernelGGL(stack_input_kernel<f16_t>, dim3(grid_for(npix, 256)), dim3(256), 0, (hipStream_t)stream, a,
                       b, f, (f16_t*)out->data, out->n, out->h - 2 * pad, out->w - 2 * pad, out->cs, out->c0, pad);
  FN2_CHECK_LAUNCH("stack_input");
  return FN2_OK;
}

int fn2_stack_input(const float* a, const float* b, const float* flow, const fn2_tensor* out, int pad, void* stream) {
  FN2_REQUIRE(a && b && flow, "stack_input: null pointer");
  int rc = check_out16(out, 12, pad, "stack_input");
  if (rc) return rc;
  rc = check_in_align(a, b, flow, nullptr, nullptr, nullptr, "stack_input");
  if (rc) return rc;
  return stack_input_launch(a, b, flow_src(flow, 0, 0, 1.f, nullptr, 0, 0), out, pad, stream);
}

int fn2_stack_input_pf(const float* a, const float* b, const float* pf, int pf_h, int pf_w, float scale, float* flow_out,
                       const fn2_tensor* out, int pad, void* stream) {
  FN2_REQUIRE(a && b && pf && pf_h >= 1 && pf_w >= 1, "stack_input_pf: null pointer / bad size");
  int rc = check_out16(out, 12, pad, "stack_input_pf");
  if (rc) return rc;
  rc = check_in_align(a, b, pf, flow_out, nullptr, nullptr, "stack_input_pf");
  if (rc) return rc;
  return stack_input_launch(a, b, flow_src(pf, pf_h, pf_w, scale, flow_out, out->h - 2 * pad, out->w - 2 * pad), out, pad, stream);
}

static int fusion_input_launch(const float* a, const float* b, const FlowSrc& fs, const FlowSrc& fc, const fn2_tensor* out,
                               int pad, void* stream) {
  const long npix = (long)out->n * (out->h - 2 * pad) * (out->w - 2 * pad);
  if (out->dtype == FN2_F32)
    hipLaunchKernelGGL(fusion_input_kernel<float>, dim3(grid_for(npix, 256)), dim3(256), 0, (hipStream_t)stream, a,
                       b, fs, fc, (float*)out->data, out->n, out->h - 2 * pad, out->w - 2 * pad, out->cs, out->c0, pad);
  else if (out->dtype == FN2_F16X2)
    hipLaunchKernelGGL(fusion_input_kernel<x2_t>, dim3(grid_for(npix, 256)), dim3(256), 0, (hipStream_t)stream,
                       a, b, fs, fc, (x2_t*)out->data, out->n, out->h - 2 * pad, out->w - 2 * pad, out->cs, out->c0, pad);
  else if (out->dtype == FN2_BF16)
    hipLaunchKernelGGL(fusion_input_kernel<bf16_t>, dim3(grid_for(npix, 256)), dim3(256), 0, (hipStream_t)stream,
                       a, b, fs, fc, (bf16_t*)out->data, out->n, out->h - 2 * pad, out->w - 2 * pad, out->cs, out->c0, pad);
  else
    hipLaunchKernelGGL(fusion_input_kernel<f16_t>, dim3(grid_for(npix, 256)), dim3(256), 0, (hipStream_t)stream,
                       a, b, fs, fc, (f16_t*)out->data, out->n, out->h - 2 * pad, out->w - 2 * pad, out->cs, out->c0, pad);
  FN2_CHECK_LAUNCH("fusion_input");
  return FN2_OK;
}

int fn2_fusion_input(const float* a, const float* b, const float* flow_sd, const float* flow_css,
                     const fn2_tensor* out, int pad, void* stream) {
  FN2_REQUIRE(a && b && flow_sd && flow_css, "fusion_input: null pointer");
  int rc = check_out16(out, 11, pad, "fusion_input");
  if (rc) return rc;
  rc = check_in_align(a, b, flow_sd, flow_css, nullptr, nullptr, "fusion_input");
  if (rc) return rc;
  return fusion_input_launch(a, b, flow_src(flow_sd, 0, 0, 1.f, nullptr, 0, 0), flow_src(flow_css, 0, 0, 1.f, nullptr, 0, 0),
                             out, pad, stream);
}

int fn2_fusion_input_pf(const float* a, const float* b, const float* pf_sd, float scale_sd, float* flow_sd_out,
                        const float* pf_css, float scale_css, float* flow_css_out, int pf_h, int pf_w,
                        const fn2_tensor* out, int pad, void* stream) {
  FN2_REQUIRE(a && b && pf_sd && pf_css && pf_h >= 1 && pf_w >= 1, "fusion_input_pf: null pointer / bad size");
  int rc = check_out16(out, 11, pad, "fusion_input_pf");
  if (rc) return rc;
  rc = check_in_align(a, b, pf_sd, pf_css, flow_sd_out, flow_css_out, "fusion_input_pf");
  if (rc) return rc;
  const int oh = out->h - 2 * pad, ow = out->w - 2 * pad;
  return fusion_input_launch(a, b, flow_src(pf_sd, pf_h, pf_w, scale_sd, flow_sd_out, oh, ow),
                             flow_src(pf_css, pf_h, pf_w, scale_css, flow_css_out, oh, ow), out, pad, stream);
}

}  // extern "C"
