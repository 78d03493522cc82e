// Hard-flow-example mining of FlowNetS_interp.loss (src/utils.py:227-339): the per-pixel loss weights of the 'hard'
// and 'edges' modes, without a sort and without an allocation, so that the train step can be captured.
//
// 'hard': weight = hard_weight on the k pixels of the batch with the largest endpoint error and 0 elsewhere, ties
// taken in index order (tf.nn.top_k is a stable descending sort: among equal values the lower index comes first).
// One launch for all loss scales: one workgroup of 1024 threads per level, the levels side by side.
//
//   pass 0   epe[i] = ||pred[i] - label[i]||_2
//   select   the k-th largest key T by an 8-bit x 4-pass radix select, the most significant byte first.  A key is
//            the fp32 bit pattern of the EPE (>= 0, so unsigned order is float order; any NaN -> all ones).  Every
//            pass re-reads epe (the maps do not fit in LDS), counts the keys that match the prefix found so far into
//            per-wave LDS histograms, sums the 16 histograms, and wave 0 scans the 256 bins from the top.
//   write    c = #keys > T are all selected; of the keys == T the first k - c in flat-index order.  The map is walked
//            in tiles of 1024 consecutive pixels with a carried count, ranks inside a tile from a ballot per wave and
//            the per-wave totals in LDS.
//
// Thread t owns pixels t, t + 1024, ... in every pass, so a thread only ever re-reads epe values it wrote itself.
#include "fn2_common.h"

namespace fn2 {

constexpr int HFEM_THREADS = 1024;
constexpr int HFEM_WAVES = HFEM_THREADS / 64;
constexpr int HFEM_MAX_LEVELS = 8;

struct HfemArgs {
  fn2_hfem_level lv[HFEM_MAX_LEVELS];
};

__device__ __forceinline__ unsigned hfem_key(float e) {
  return e != e ? 0xffffffffu : (__float_as_uint(e) & 0x7fffffffu);
}

__global__ void __launch_bounds__(HFEM_THREADS) hfem_hard_weights_kernel(const HfemArgs args) {
  __shared__ unsigned hist[HFEM_WAVES][256];
  __shared__ unsigned tot[256];
  __shared__ unsigned wave_eq[2][HFEM_WAVES];
  __shared__ unsigned sel_digit, sel_k;

  const fn2_hfem_level& L = args.lv[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long npix = L.npix;
  const float2* __restrict__ pred = reinterpret_cast<const float2*>(L.pred);
  const float2* __restrict__ label = reinterpret_cast<const float2*>(L.label);
  float* __restrict__ epe = L.epe;
  float* __restrict__ weight = L.weight;
  const float hw = L.hard_weight;
  const long kl = L.k < 0 ? 0 : (L.k > npix ? npix : L.k);  // (the entry point has checked it; a graph replays it blindly)

  for (long i = tid; i < npix; i += HFEM_THREADS) {
    const float2 p = pred[i], l = label[i];
    const float dx = p.x - l.x, dy = p.y - l.y;
    epe[i] = sqrtf(dx * dx + dy * dy);  // (correctly rounded: the library is built without fast-math)
  }
  if (kl == 0) {  // (uniform over the block)
    for (long i = tid; i < npix; i += HFEM_THREADS) weight[i] = 0.f;
    return;
  }

  // ---- radix select of the k-th largest key
  unsigned prefix = 0, mask = 0, kk = (unsigned)kl;  // kk: rank (1-based, from the top) among the keys matching prefix
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int b = tid; b < HFEM_WAVES * 256; b += HFEM_THREADS) (&hist[0][0])[b] = 0;
    __syncthreads();
    unsigned* h = hist[wave];
    for (long base = 0; base < npix; base += HFEM_THREADS) {  // (uniform trip count: the ballots below need whole waves)
      const long i = base + tid;
      unsigned key = 0;
      bool valid = i < npix;
      if (valid) {
        key = hfem_key(epe[i]);
        valid = (key & mask) == prefix;
      }
      const unsigned digit = (key >> shift) & 255u;
      // few bins are populated (exponents of one map, tie groups): the two most frequent-looking digits of the wave go
      // in as one add each, the rest as plain LDS atomics
      unsigned long long act = __ballot(valid);
      for (int r = 0; r < 2 && act; ++r) {
        const int leader = __ffsll((long long)act) - 1;
        const unsigned d0 = __shfl(digit, leader);
        const unsigned long long m = __ballot(valid && digit == d0);
        if (lane == leader) atomicAdd(&h[d0], (unsigned)__popcll(m));
        valid = valid && digit != d0;
        act &= ~m;
      }
      if (valid) atomicAdd(&h[digit], 1u);
    }
    __syncthreads();
    if (tid < 256) {
      unsigned s = 0;
#pragma unroll
      for (int w = 0; w < HFEM_WAVES; ++w) s += hist[w][tid];
      tot[tid] = s;
    }
    __syncthreads();
    if (wave == 0) {
      // lane l holds bins 255 - 4l .. 252 - 4l: an inclusive scan over the lanes walks the bins from the top
      unsigned c[4], s = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        c[j] = tot[255 - 4 * lane - j];
        s += c[j];
      }
      unsigned incl = s;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
      }
      unsigned run = incl - s;
      const bool found = run < kk && kk <= incl;
      if (found) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (run < kk && kk <= run + c[j]) {
            sel_digit = 255 - 4 * lane - j;
            sel_k = kk - run;
          }
          run += c[j];
        }
      }
      if (__ballot(found) == 0 && lane == 0) {  // cannot happen while #matching keys >= kk; keeps the state defined
        sel_digit = 0;
        sel_k = kk;
      }
    }
    __syncthreads();
    prefix |= sel_digit << shift;
    mask |= 255u << shift;
    kk = sel_k;
  }

  // ---- weights: every key above T, and the first kk keys equal to T in index order
  const unsigned T = prefix;
  unsigned taken = 0;  // keys == T in the tiles before this one (uniform over the block)
  int par = 0;
  for (long base = 0; base < npix; base += HFEM_THREADS, par ^= 1) {
    const long i = base + tid;
    const bool inb = i < npix;
    const unsigned key = inb ? hfem_key(epe[i]) : 0u;
    const bool eq = inb && key == T, gt = inb && key > T;
    const unsigned long long m = __ballot(eq);
    const unsigned below = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_eq[par][wave] = (unsigned)__popcll(m);
    __syncthreads();  // (one barrier per tile: the other half of wave_eq is rewritten only behind the next one)
    unsigned off = 0, all = 0;
#pragma unroll
    for (int w = 0; w < HFEM_WAVES; ++w) {
      const unsigned c = wave_eq[par][w];
      off += w < wave ? c : 0u;
      all += c;
    }
    if (inb) weight[i] = (gt || (eq && taken + off + below < kk)) ? hw : 0.f;
    taken += all;
  }
}

__global__ void __launch_bounds__(256) hfem_edge_weights_kernel(const float* __restrict__ edges, float lambda_w,
                                                                float* __restrict__ weight, long npix) {
#pragma clang fp contract(off)  // product and sum rounded separately: no fma (__fmul_rn / __fadd_rn inline to contractable operators)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < npix) {
    const float prod = lambda_w * edges[i];
    weight[i] = 1.0f + prod;
  }
}

}  // namespace fn2

using namespace fn2;

extern "C" {

int fn2_hfem_hard_weights(const fn2_hfem_level* levels, int n_levels, void* stream) {
  FN2_REQUIRE(levels, "hfem_hard_weights: null level table");
  FN2_REQUIRE(n_levels >= 1 && n_levels <= HFEM_MAX_LEVELS, "hfem_hard_weights: n_levels must be 1..%d, got %d",
              HFEM_MAX_LEVELS, n_levels);
  HfemArgs a = {};
  for (int i = 0; i < n_levels; ++i) {
    const fn2_hfem_level& l = levels[i];
    FN2_REQUIRE(l.pred && l.label && l.epe && l.weight, "hfem_hard_weights: null pointer in level %d", i);
    FN2_REQUIRE(l.npix >= 1 && l.npix <= 0x7fffffffL, "hfem_hard_weights: level %d: npix must be 1..2^31-1, got %ld", i,
                (long)l.npix);
    FN2_REQUIRE(l.k >= 0 && l.k <= l.npix, "hfem_hard_weights: level %d: k = %ld outside [0, npix = %ld]", i, (long)l.k,
                (long)l.npix);
    a.lv[i] = l;
  }
  hipLaunchKernelGGL(hfem_hard_weights_kernel, dim3(n_levels), dim3(HFEM_THREADS), 0, (hipStream_t)stream, a);
  FN2_CHECK_LAUNCH("hfem_hard_weights");
  return FN2_OK;
}

int fn2_hfem_edge_weights(const float* edges, float lambda_w, float* weight, int64_t npix, void* stream) {
  FN2_REQUIRE(edges && weight, "hfem_edge_weights: null pointer");
  FN2_REQUIRE(npix >= 1 && npix <= 0x7fffffffL, "hfem_edge_weights: npix must be 1..2^31-1, got %ld", (long)npix);
  hipLaunchKernelGGL(hfem_edge_weights_kernel, dim3(cdiv(npix, 256)), dim3(256), 0, (hipStream_t)stream, edges, lambda_w,
                     weight, (long)npix);
  FN2_CHECK_LAUNCH("hfem_edge_weights");
  return FN2_OK;
}

}  // extern "C"
