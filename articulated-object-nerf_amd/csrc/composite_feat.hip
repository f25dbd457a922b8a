// Feature compositing: out[b, c] = sum_s weights[b, s] * feat[b, s, c] -- the reference's
// comp_nocs = (weights[..., None] * nocs).sum(dim=-2) (models/vanilla_nerf/helper.py:191-193) for
// any per-sample feature of up to 8 channels (the articulated render's x' and deformation maps).
// HBM-bound: one 64-lane wave per ray, lane i owns samples i, i + 64, ...; every weight and every
// feat row is read once (one 16-B load per row when the rows are 16-B rows), the products go to
// planar LDS arrays and each channel is summed over S terms in torch's CPU order by the whole
// wave (wave_row_sums) -- the sum k_composite_fwd forms for comp_rgb, so a 3-channel call on the
// same weights gives its comp_rgb (no background) bit for bit.
#include "composite_core.hpp"

namespace aon {

// NB = ceil(S / 64); CM: channel capacity (4 or 8); ROW4: feat rows of 4 floats, 16-B aligned
template <int NB, int CM, bool ROW4>
__global__ __launch_bounds__(64 * kCompWaves) void k_composite_feat(
    const float* __restrict__ wts, const float* __restrict__ feat, int64_t feat_stride, int C,
    int64_t B, int S, float* __restrict__ out) {
  constexpr int SM = 64 * NB;
  // wave_row_sums task partials: C sums over S terms, 4 ((S / 4) / 16 + 1) each
  constexpr int kScratch = CM * 4 * ((SM >> 2 >> 4) + 1);
  __shared__ float lds_all[kCompWaves][CM * SM + kScratch + CM];
  float* P = lds_all[threadIdx.x >> 6];  // P[c * SM + i] = w_i * feat[i][c]
  float* scratch = P + CM * SM;
  float* sums = scratch + kScratch;
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * kCompWaves;
  for (int64_t ray = (int64_t)blockIdx.x * kCompWaves + (threadIdx.x >> 6); ray < B;
       ray += nwaves) {
    const int64_t row0 = ray * S;
    float w[NB], f[NB][CM];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int i = 64 * b + lane;
      w[b] = 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c) f[b][c] = 0.f;
      if (i < S) {
        w[b] = wts[row0 + i];
        if (ROW4) {
          const f4 v = *reinterpret_cast<const f4*>(feat + (row0 + i) * 4);
#pragma unroll
          for (int c = 0; c < 4; ++c) f[b][c] = v[c];
        } else {
          const float* r = feat + (row0 + i) * feat_stride;
#pragma unroll
          for (int c = 0; c < CM; ++c)
            if (c < C) f[b][c] = r[c];
        }
      }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int i = 64 * b + lane;
      if (i < S) {
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c < C) P[c * SM + i] = __fmul_rn(w[b], f[b][c]);
      }
    }
    wave_sync_c();
    wave_row_sums(
        [&](int sp, const float*& base, int& str) {
          base = P + sp * SM;
          str = 1;
        },
        C, S, 0, 0, scratch, sums, lane, wave_sync_c);
    if (lane < C) out[ray * C + lane] = sums[lane];
    wave_sync_c();  // LDS reuse by this wave's next ray
  }
}

template <int NB>
static void launch_composite_feat(int grid, hipStream_t st, const float* w, const float* feat,
                                  int64_t feat_stride, int C, int64_t B, int S, float* out) {
  const bool row4 = feat_stride == 4 && C <= 4 && aligned16(feat);
  if (row4)
    hipLaunchKernelGGL((k_composite_feat<NB, 4, true>), grid, 64 * kCompWaves, 0, st, w, feat,
                       feat_stride, C, B, S, out);
  else if (C <= 4)
    hipLaunchKernelGGL((k_composite_feat<NB, 4, false>), grid, 64 * kCompWaves, 0, st, w, feat,
                       feat_stride, C, B, S, out);
  else
    hipLaunchKernelGGL((k_composite_feat<NB, 8, false>), grid, 64 * kCompWaves, 0, st, w, feat,
                       feat_stride, C, B, S, out);
}

}  // namespace aon

using namespace aon;

extern "C" int aon_composite_feat(const float* weights, const float* feat, int64_t feat_stride,
                                  int C, int64_t B, int S, float* out, aon_stream_t stream) {
  AON_REQUIRE(weights && feat && out, "null pointer");
  AON_REQUIRE(C >= 1 && C <= 8, "bad channel count (1 <= C <= 8)");
  AON_REQUIRE(B >= 0 && S >= 1 && S <= kCompMaxS, "bad shape (1 <= S <= 512)");
  AON_REQUIRE(feat_stride >= C, "feat_stride must be >= C");
  AON_REQUIRE(((reinterpret_cast<uintptr_t>(weights) | reinterpret_cast<uintptr_t>(feat) |
                reinterpret_cast<uintptr_t>(out)) & 3) == 0,
              "weights / feat / out must be 4-byte aligned");
  if (B == 0) return 0;
  const int grid = grid_for(B, kCompWaves, 1 << 16);
  hipStream_t st = (hipStream_t)stream;
  switch ((S + 63) / 64) {
#define AON_FEAT_CASE(nb)                                                              \
  case nb:                                                                             \
    launch_composite_feat<nb>(grid, st, weights, feat, feat_stride, C, B, S, out);     \
    break;
    AON_FEAT_CASE(1)
    AON_FEAT_CASE(2)
    AON_FEAT_CASE(3)
    AON_FEAT_CASE(4)
    AON_FEAT_CASE(5)
    AON_FEAT_CASE(6)
    AON_FEAT_CASE(7)
    AON_FEAT_CASE(8)
#undef AON_FEAT_CASE
  }
  return launch_status(__func__);
}
