// Ternary census data term of the unsupervised trainer: UnFlow's soft Hamming distance between the
// 7 x 7 census descriptors of a frame's grey values and of its partner's grey values warped by tf_warp, under
// abs_robust_loss in its loss_mean form (src/utils.py:378-395), as DDFlow and SelFlow train their final stages.  The slot
// layout, f = scale * pred, (X, Y), the taps and `valid` are those of photometric.hip.
//
// Per level (h x w), R = 3:
//   warp   G = ((r + g) + b) * 85 (each operation rounded on its own);  W = tf_blend(taps, G[j ^ 1] at the four taps),
//          DX = d W / dX, DY = d W / dY on the clamped taps;  V = 0 <= X < w - 1 and 0 <= Y < h - 1 (NaN fails);  where
//          V = 0 the three are stored as 0 (tf_warp extrapolates or cancels there, and a poisoned flow would leave NaN);
//          count += sum mask * V * [Omega],  Omega = {R <= x < w - R, R <= y < h - R}
//   cost   S(q) = sum_d V(q + d) e / (0.1 + e),  e = (n(G(q + d) - G(q)) - n(W(q + d) - W(q)))^2,  n(t) = t / sqrt(0.81 + t^2),
//          q in Omega (0 elsewhere);  psi = (S + 0.01)^q;  c = mc * q * psi / (S + 0.01);  L = weight * sum mc psi / (2 Mc + 1e-6)
//   grad   dW(p) = sum_d c(p - d) k(p - d, d) - c(p) sum_d k(p, d) with k of the header.  k is odd in its pair of
//          differences, so both sums run over the same 49 neighbours r of p with ONE k each:
//          dW(p) = sum_r k(G(p) - G(r), W(p) - W(r)) * (c(r) V(p) + c(p) V(r));  dpred = gcoef * dW * (DX, DY).  A gather:
//          plain stores, deterministic.
//
// warp walks the levels as photometric.hip does (a wave owns 64 consecutive pixels of a row).  cost and grad work on tiles
// of 8 rows x 32 columns, one pixel per thread, staged with their 3-pixel halo (14 x 38) in LDS: G, W, V (and c for grad),
// 6.4 / 8.5 KB per block.  A wave reads two tile rows of 32 consecutive floats per ds_read_b32 -- the banks of a lane
// group of 32 are all different at any row pitch -- and the 49 offsets are immediates.  Small tiles on purpose: the largest
// level of a 384 x 512 batch of 8 is 96 x 128, which 8 x 32 tiles cut into 384 blocks (2.1 x halo traffic from L2) where
// 16 x 64 tiles would leave 96 blocks for 256 CUs.  Outside the level a tile holds G = W = V = c = 0.
#include "photo_levels.h"

namespace fn2 {
namespace {

constexpr int CR = 3;                         // census radius: 7 x 7 descriptors
constexpr int CTH = 8, CTW = 32;              // pixels of a tile: one per thread
constexpr int CPH = CTH + 2 * CR, CPW = CTW + 2 * CR;
static_assert(CTH * CTW == PHOTO_BLOCK, "one pixel per thread");

struct CensusArgs {
  fn2_census_level lv[PHOTO_MAX_LEVELS];
  int64_t tile_end[PHOTO_MAX_LEVELS];  // tiles of the levels 0..l together: cost and grad walk all levels as ONE list of tiles
  int n_levels, n;
};

__device__ __forceinline__ float grey_of(const rgb3_t v) {
#pragma clang fp contract(off)
  return ((v.r + v.g) + v.b) * 85.0f;
}

// n(t) = t / sqrt(0.81 + t^2)
__device__ __forceinline__ float census_norm(float t) { return t / sqrtf(0.81f + t * t); }

// d/dtw of e / (0.1 + e) at the differences (tg, tw) of the grey values and of the warped ones
__device__ __forceinline__ float census_k(float tg, float tw) {
  const float s = 0.81f + tw * tw;
  const float r = sqrtf(s);
  const float ab = census_norm(tg) - tw / r;
  const float den = 0.1f + ab * ab;
  return (-0.2f * ab / (den * den)) * (0.81f / (s * r));
}

__device__ __forceinline__ bool in_omega(int y, int x, int H, int W) {
  return x >= CR && x < W - CR && y >= CR && y < H - CR;
}

__global__ void __launch_bounds__(PHOTO_BLOCK) census_warp_kernel(const CensusArgs a) {
  __shared__ float sums[PHOTO_MAX_LEVELS];
  LevelSums acc{sums};
  acc.clear();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (int l = 0; l < a.n_levels; ++l) {
    const fn2_census_level& L = a.lv[l];
    const int H = L.h, W = L.w, segs = (W + 63) / 64;
    const int64_t units = (int64_t)a.n * H * segs, ipitch = 3LL * W, ibstride = ipitch * H, npix = (int64_t)a.n * H * W;
    const float s = L.scale;
    float count = 0.f;
    for (int64_t u = (int64_t)blockIdx.x * PHOTO_WAVES + wave; u < units; u += (int64_t)gridDim.x * PHOTO_WAVES) {
      const Unit p = unit_at(u, H, segs);
      if (p.x >= W) continue;
      const int64_t o = (p.n * H + p.y) * W + p.x;
      const float2 f = scaled_flow(ld2(L.pred + 2 * o), s);
      const float X = coord(p.x, f.x), Y = coord(p.y, f.y);
      const bool valid = X >= 0.f && X < (float)(W - 1) && Y >= 0.f && Y < (float)(H - 1);  // a NaN fails
      float wv = 0.f, dx = 0.f, dy = 0.f;
      if (valid) {
        const TfTaps t = tf_taps_at(X, Y, W, H);
        const float* par = L.img + (p.n ^ 1) * ibstride;
        const float* r0 = par + (int64_t)t.y0 * ipitch;
        const float* r1 = par + (int64_t)t.y1 * ipitch;
        const float ga = grey_of(load_rgb(r0 + 3 * t.x0)), gb = grey_of(load_rgb(r1 + 3 * t.x0));
        const float gc = grey_of(load_rgb(r0 + 3 * t.x1)), gd = grey_of(load_rgb(r1 + 3 * t.x1));
        wv = tf_blend(t, ga, gb, gc, gd);
        dx = ((float)t.y1 - Y) * (gc - ga) + (Y - (float)t.y0) * (gd - gb);
        dy = ((float)t.x1 - X) * (gb - ga) + (X - (float)t.x0) * (gd - gc);
      }
      L.grey[o] = grey_of(load_rgb(L.img + 3 * o));
      L.warp[o] = wv;
      L.warp[npix + o] = dx;
      L.warp[2 * npix + o] = dy;
      L.valid[o] = valid ? 1.f : 0.f;
      if (valid && in_omega(p.y, p.x, H, W)) count += L.mask[o];
    }
    acc.add(l, count);
  }
  __syncthreads();
  if (threadIdx.x < a.n_levels && sums[threadIdx.x] != 0.f) atomicAdd(a.lv[threadIdx.x].count, sums[threadIdx.x]);
}

// the tile walk of cost and grad: (level, image, first row, first column) of tile t of the list over all levels.  With a
// loop over the levels around a loop over each level's tiles, block 0 would work through one tile of EVERY level in turn;
// over the one list a block of a 384 x 512 batch of 8 (528 tiles) has one tile.
struct Tile {
  int64_t n;
  int level, y0, x0;
};
__device__ __forceinline__ Tile tile_at(const CensusArgs& a, int64_t t) {
  Tile r;
  r.level = 0;
  while (t >= a.tile_end[r.level]) ++r.level;
  if (r.level > 0) t -= a.tile_end[r.level - 1];
  const int tiles_y = (a.lv[r.level].h + CTH - 1) / CTH, tiles_x = (a.lv[r.level].w + CTW - 1) / CTW;
  const int64_t row = t / tiles_x;
  r.x0 = (int)(t - row * tiles_x) * CTW;
  r.n = row / tiles_y;
  r.y0 = (int)(row - r.n * tiles_y) * CTH;
  return r;
}

// a [CPH][CPW] tile with its halo from the plane `src` of image n; 0 outside the level
__device__ __forceinline__ void stage(float* dst, const float* __restrict__ src, const Tile& t, int H, int W) {
  const float* img = src + t.n * H * W;
  for (int i = threadIdx.x; i < CPH * CPW; i += PHOTO_BLOCK) {
    const int ty = i / CPW, tx = i - ty * CPW;
    const int y = t.y0 - CR + ty, x = t.x0 - CR + tx;
    dst[i] = (y >= 0 && y < H && x >= 0 && x < W) ? img[(int64_t)y * W + x] : 0.f;
  }
}

__global__ void __launch_bounds__(PHOTO_BLOCK) census_cost_kernel(const CensusArgs a, float q,
                                                                  float* __restrict__ loss_accum) {
  __shared__ float sums[PHOTO_MAX_LEVELS];
  __shared__ float sg[CPH * CPW], sw[CPH * CPW], sv[CPH * CPW];
  LevelSums acc{sums};
  acc.clear();
  const int lx = threadIdx.x & (CTW - 1), ly = threadIdx.x / CTW;
  const int centre = (ly + CR) * CPW + lx + CR;
  const int64_t tiles = a.tile_end[a.n_levels - 1];
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const Tile T = tile_at(a, t);
    const fn2_census_level& L = a.lv[T.level];
    const int H = L.h, W = L.w;
    const int64_t npix = (int64_t)a.n * H * W;
    __syncthreads();  // the previous tile has been read
    stage(sg, L.grey, T, H, W);
    stage(sw, L.warp, T, H, W);
    stage(sv, L.valid, T, H, W);
    __syncthreads();
    const int y = T.y0 + ly, x = T.x0 + lx;
    float part = 0.f;
    if (y < H && x < W) {
      const int64_t o = (T.n * H + y) * W + x;
      float S = 0.f, c = 0.f;
      if (in_omega(y, x, H, W)) {
        const float g0 = sg[centre], w0 = sw[centre];
#pragma unroll 1  // (a descriptor row at a time; all 49 neighbours in flight cost 93 VGPRs)
        for (int dy = -CR; dy <= CR; ++dy) {
#pragma unroll
          for (int dx = -CR; dx <= CR; ++dx) {
            const int k = centre + dy * CPW + dx;
            const float ab = census_norm(sg[k] - g0) - census_norm(sw[k] - w0);
            const float e = ab * ab;
            const float term = e / (0.1f + e);
            S += sv[k] != 0.f ? term : 0.f;
          }
        }
        if (sv[centre] != 0.f && L.mask[o] != 0.f) {
          const float mag = S + 0.01f;
          part = powf(mag, q);
          c = q * part / mag;
        }
      }
      L.coef[o] = S;
      L.coef[npix + o] = c;
    }
    acc.add(T.level, part);  // (the level is the block's: every wave is here)
  }
  __syncthreads();
  if (threadIdx.x < a.n_levels && sums[threadIdx.x] != 0.f) {
    const fn2_census_level& L = a.lv[threadIdx.x];
    atomicAdd(loss_accum, (float)((double)sums[threadIdx.x] * (double)L.weight / (2.0 * (double)*L.count + 1e-6)));
  }
}

__global__ void __launch_bounds__(PHOTO_BLOCK) census_grad_kernel(const CensusArgs a, float grad_mult) {
  __shared__ float sg[CPH * CPW], sw[CPH * CPW], sv[CPH * CPW], sc[CPH * CPW];
  const int lx = threadIdx.x & (CTW - 1), ly = threadIdx.x / CTW;
  const int centre = (ly + CR) * CPW + lx + CR;
  const int64_t tiles = a.tile_end[a.n_levels - 1];
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const Tile T = tile_at(a, t);
    const fn2_census_level& L = a.lv[T.level];
    const int H = L.h, W = L.w;
    const int64_t npix = (int64_t)a.n * H * W;
    __syncthreads();
    stage(sg, L.grey, T, H, W);
    stage(sw, L.warp, T, H, W);
    stage(sv, L.valid, T, H, W);
    stage(sc, L.coef + npix, T, H, W);
    __syncthreads();
    const int y = T.y0 + ly, x = T.x0 + lx;
    if (y >= H || x >= W) continue;  // (no barrier behind this point of the iteration)
    // (one division per tile and thread, in double: 2 Mc + 1e-6 is not an fp32 number)
    const float gcoef =
        (float)((double)grad_mult * (double)L.weight * (double)L.scale / (2.0 * (double)*L.count + 1e-6));
    const int64_t o = (T.n * H + y) * W + x;
    const float g0 = sg[centre], w0 = sw[centre], v0 = sv[centre], c0 = sc[centre];
    float dw = 0.f;
#pragma unroll 1  // (all 49 neighbours in flight cost 162 VGPRs; a row at a time: 7 ds_reads x 4 per batch)
    for (int dy = -CR; dy <= CR; ++dy) {
#pragma unroll
      for (int dx = -CR; dx <= CR; ++dx) {
        const int k = centre + dy * CPW + dx;
        const float wgt = sc[k] * v0 + c0 * sv[k];  // c(r) V(p) + c(p) V(r): both 0 wherever V(p) = 0
        const float kk = census_k(g0 - sg[k], w0 - sw[k]);
        dw += wgt != 0.f ? wgt * kk : 0.f;
      }
    }
    const float gd = gcoef * dw;
    *reinterpret_cast<float2*>(L.dpred + 2 * o) = make_float2(gd * L.warp[npix + o], gd * L.warp[2 * npix + o]);
  }
}

// the table checked and copied into the kernel argument; `tiled`: the grid covers the tiles of all levels, else the
// (image, row, segment) units of the largest level
int census_args(const char* what, const fn2_census_level* levels, int n_levels, int n, bool tiled, CensusArgs& a,
                int& grid) {
  FN2_REQUIRE(levels, "%s: null level table", what);
  FN2_REQUIRE(n_levels >= 1 && n_levels <= PHOTO_MAX_LEVELS, "%s: n_levels must be 1..%d, got %d", what,
              PHOTO_MAX_LEVELS, n_levels);
  FN2_REQUIRE(n >= 2 && n % 2 == 0, "%s: n must be even (two slots per pair), got %d", what, n);
  a = CensusArgs{};
  a.n_levels = n_levels;
  a.n = n;
  int64_t blocks = 1, tiles = 0;
  for (int i = 0; i < n_levels; ++i) {
    const fn2_census_level& l = levels[i];
    FN2_REQUIRE(l.pred && l.img && l.mask && l.dpred && l.grey && l.warp && l.valid && l.coef && l.count,
                "%s: null pointer in level %d", what, i);
    FN2_REQUIRE(l.h >= 1 && l.w >= 1, "%s: level %d: bad size h=%d w=%d", what, i, l.h, l.w);
    FN2_REQUIRE((int64_t)l.h * l.w <= (1LL << 30), "%s: level %d: image too large (%d x %d)", what, i, l.h, l.w);
    FN2_REQUIRE(((reinterpret_cast<uintptr_t>(l.pred) | reinterpret_cast<uintptr_t>(l.dpred)) & 7) == 0,
                "%s: level %d: pred and dpred must be 8-byte aligned", what, i);
    FN2_REQUIRE(((reinterpret_cast<uintptr_t>(l.img) | reinterpret_cast<uintptr_t>(l.mask) |
                  reinterpret_cast<uintptr_t>(l.grey) | reinterpret_cast<uintptr_t>(l.warp) |
                  reinterpret_cast<uintptr_t>(l.valid) | reinterpret_cast<uintptr_t>(l.coef) |
                  reinterpret_cast<uintptr_t>(l.count)) & 3) == 0,
                "%s: level %d: every float buffer must be 4-byte aligned", what, i);
    a.lv[i] = l;
    const int64_t units = (int64_t)n * l.h * ((l.w + 63) / 64);
    blocks = max(blocks, (units + PHOTO_WAVES - 1) / PHOTO_WAVES);
    a.tile_end[i] = tiles += (int64_t)n * cdiv(l.h, CTH) * cdiv(l.w, CTW);
  }
  if (tiled) blocks = tiles;
  grid = (int)min(blocks, (int64_t)PHOTO_MAX_BLOCKS);
  return FN2_OK;
}

}  // namespace
}  // namespace fn2

using namespace fn2;

extern "C" {

int fn2_census_warp(const fn2_census_level* levels, int n_levels, int n, void* stream) {
  CensusArgs a;
  int grid;
  if (int rc = census_args("census_warp", levels, n_levels, n, false, a, grid)) return rc;
  hipLaunchKernelGGL(census_warp_kernel, dim3(grid), dim3(PHOTO_BLOCK), 0, (hipStream_t)stream, a);
  FN2_CHECK_LAUNCH("census_warp");
  return FN2_OK;
}

int fn2_census_cost(const fn2_census_level* levels, int n_levels, int n, float q, float* loss_accum, void* stream) {
  CensusArgs a;
  int grid;
  if (int rc = census_args("census_cost", levels, n_levels, n, true, a, grid)) return rc;
  FN2_REQUIRE(loss_accum, "census_cost: null loss_accum");
  FN2_REQUIRE(q > 0.f && q <= 1.f, "census_cost: q must lie in (0, 1], got %g", (double)q);
  hipLaunchKernelGGL(census_cost_kernel, dim3(grid), dim3(PHOTO_BLOCK), 0, (hipStream_t)stream, a, q, loss_accum);
  FN2_CHECK_LAUNCH("census_cost");
  return FN2_OK;
}

int fn2_census_grad(const fn2_census_level* levels, int n_levels, int n, float grad_mult, void* stream) {
  CensusArgs a;
  int grid;
  if (int rc = census_args("census_grad", levels, n_levels, n, true, a, grid)) return rc;
  hipLaunchKernelGGL(census_grad_kernel, dim3(grid), dim3(PHOTO_BLOCK), 0, (hipStream_t)stream, a, grad_mult);
  FN2_CHECK_LAUNCH("census_grad");
  return FN2_OK;
}

}  // extern "C"
