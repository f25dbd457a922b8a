// The articulated NeRFMLP's deformation MLP alone (reference models/vanilla_nerf/
// model_autodecoder.py:196-205), on the fp16x3 MFMA path of mlp_art.hip:
//
//   xyz = o + t d                                     (helper.py:25-26; or given points)
//   h = relu(D3 relu(D2 relu(D1 relu(D0 [xyz | shape, art]))))          :196-203
//   delta = deformation_layer(h);  x' = delta + xyz                     :205
//
// -- the canonical coordinate x' and the deformation of every sample, which the full kernel
// (k_mlp_art_f16x3) keeps on chip.  The pass reads the deformation PREFIX of an aon_mlp_art_pack
// stream in place (mlp_layout.hpp NetArtDeformH: kBlocks of NetArtH's blocks, kBiasFloats of its
// bias rows, its status word), with the full kernel's arithmetic for xyz, the four layers, the head and the
// fp32 add, so x' is the full kernel's x' bit for bit.
//
// Budget.  No trunk, no pos_enc, no view branch: the widest layer is 128, so a wave's two
// activation fragments are Frag<4, NCOL> (64 NCOL VGPRs, a quarter of the full kernel's), nothing
// is stashed in LDS, and the weight ring is 3 chunks of 16 blocks (48 KB + 2 KB of biases, a
// third of the full kernel's LDS).  A wave reads the whole 216-KB prefix from LDS per 16 NCOL
// samples: at NCOL = 1 that is 13.5 KB of ds_read per sample against 324 MFMAs per 16 samples,
// LDS-read-bound; NCOL = 2 halves the reads per sample and its 128 + 32 fragment and
// accumulator VGPRs still leave two workgroups of 4 waves per CU (2 waves per SIMD, 2 x 50 KB
// LDS) -- the instantiation of every launch past one workgroup per CU.  At or below
// kDeformSmallRows (128 rows x 256 CUs) each CU holds at most one workgroup and NCOL = 1 puts 8
// waves on it instead of 4.  Both cover 128 rows per workgroup.
#include "mlp_f16x3_core.hpp"

namespace aon {
namespace mlp {

constexpr int kDeformLdsWeights = kRing * NetArtDeformH::kChunk * 64;                   // f4
constexpr int kDeformLdsF4 = kDeformLdsWeights + NetArtDeformH::kBiasFloats / 4;
static_assert(2 * kDeformLdsF4 * 16 <= 160 * 1024, "two workgroups per CU");
constexpr int64_t kDeformSmallRows = 128 * 256;  // one 128-row workgroup per CU of an MI355X

// MODE 0: (rays_o, rays_d, t) inputs; MODE 1: points (N, 3).  xp / delta: (N, 4) rows, either
// may be null.
template <int MODE, int NCOL>
__global__ __launch_bounds__(GeomH<NCOL>::kThreads, 2) void k_mlp_art_deform_f16x3(
    const f4* __restrict__ wstream, const float* __restrict__ bias_g, const float* __restrict__ in0,
    const float* __restrict__ in1, const float* __restrict__ in3, int64_t N, int S,
    float* __restrict__ xp, float* __restrict__ delta) {
  using G = GeomH<NCOL>;
  using Net = NetArtDeformH;
  __shared__ f4 smem[kDeformLdsF4];  // weight ring | bias rows of the prefix
  float* bias_s = reinterpret_cast<float*>(smem + kDeformLdsWeights);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, j = lane & 15;

  using WP = DmaPipe<G::kThreads, kRing, Net::kChunk, Net::kStreamBlocks, Net::kBlocks, kRingLead>;
  WP p;
  start_chain<Net, G::kThreads>(p, smem, wstream, tid, lane, bias_s, bias_g);

  // deformation input (xyz, natural order: lane group 0 elements 0..2), as k_mlp_art_f16x3
  Frag<1, NCOL> din;
  int64_t rows[NCOL];
  float px[NCOL][3];
#pragma unroll
  for (int c = 0; c < NCOL; ++c) {
    const int64_t row = (int64_t)blockIdx.x * G::kRowsPerBlock + wave * G::kRowsPerWave + 16 * c + j;
    rows[c] = row;
    const int64_t rr = row < N ? row : N - 1;
    if (MODE == 0) {
      const int64_t ray = rr / S;
      const float* ro = in0 + 3 * ray;
      const float* rd = in1 + 3 * ray;
      const float tt = in3[rr];
#pragma unroll
      for (int q = 0; q < 3; ++q) px[c][q] = __fadd_rn(ro[q], __fmul_rn(tt, rd[q]));
    } else {
      const float* x = in0 + rr * 3;
#pragma unroll
      for (int q = 0; q < 3; ++q) px[c][q] = x[q];
    }
    float dv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) dv[e] = (g == 0 && e < 3) ? px[c][e < 3 ? e : 0] * kActS : 0.f;
    split8(dv, din.hi[0][c], din.lo[0][c], din.ovf);
  }

  FragPipe<WP, AON_PREFETCH> fp(p);
  fp.start();  // begin(0): chunk 0 landed; the barrier also publishes bias_s
  lds_float* bias_l = opaque_lds(bias_s + 4 * g);

  Frag<4, NCOL> x, y;
  Frag<1, NCOL> none;
  layer_h<Net, A_D0, true>(fp, none, din, x, bias_l, g);
  layer_h<Net, A_D1, true>(fp, x, none, y, bias_l, g);
  layer_h<Net, A_D2, true>(fp, y, none, x, bias_l, g);
  layer_h<Net, A_D3, true>(fp, x, none, y, bias_l, g);
  f4 dlt[NCOL];
  head_h<Net, A_DOUT>(fp, y, dlt, bias_l, g);

  // the head's tile holds delta in lane group 0 (rows 0..2, column = sample): those 16 lanes
  // write the sample's two 16-B rows; x' = delta + xyz in fp32, as the full kernel adds it
  if (g == 0) {
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
      if (rows[c] < N) {
        const float d0 = dlt[c][0], d1 = dlt[c][1], d2 = dlt[c][2];
        if (xp) {
          const f4 o = {__fadd_rn(d0, px[c][0]), __fadd_rn(d1, px[c][1]), __fadd_rn(d2, px[c][2]), 0.0f};
          *reinterpret_cast<f4*>(xp + 4 * rows[c]) = o;
        }
        if (delta) {
          const float n2 = __fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2));
          const f4 o = {d0, d1, d2, sqrtf(n2)};  // (correctly rounded: the build's sqrt flag)
          *reinterpret_cast<f4*>(delta + 4 * rows[c]) = o;
        }
      }
    }
  }
  // the status word of the whole pack, behind the whole stream's bias table
  range_report(bias_g + NetArtH::kBiasFloats, ovf_of(x) | ovf_of(y) | din.ovf);
}

template <int MODE, int NCOL>
static void launch_deform(const void* packed, const float* a0, const float* a1, const float* a3,
                          int64_t N, int S, float* xp, float* delta, hipStream_t stream) {
  using G = GeomH<NCOL>;
  static_assert(kRowsOkCovers<G>, "deform_launch's rows_ok covers this grid");
  hipLaunchKernelGGL((k_mlp_art_deform_f16x3<MODE, NCOL>), chain_grid<G>(N), G::kThreads, 0, stream,
                     static_cast<const f4*>(packed), stream_bias<NetArtH>(packed), a0, a1, a3, N, S,
                     xp, delta);
}

}  // namespace mlp
}  // namespace aon

using namespace aon;
using namespace aon::mlp;

static int deform_launch(int mode, const char* fn, const void* packed, const float* a0,
                         const float* a1, const float* a3, int64_t B, int S, float* xp,
                         float* delta, aon_stream_t stream) {
  AON_REQUIRE_AS(fn, packed && a0 && (mode == 1 || (a1 && a3)), "null pointer");
  AON_REQUIRE_AS(fn, xp || delta, "xp and delta are both null");
  AON_REQUIRE_AS(fn, B >= 0 && S >= 1, "bad shape");
  AON_REQUIRE_AS(fn, aligned16(packed) && aligned16(xp) && aligned16(delta),
                 "packed / xp / delta must be 16-byte aligned");
  AON_REQUIRE_AS(fn, B <= INT64_MAX / S, "too many rows");
  const int64_t N = B * S;
  if (N == 0) return 0;
  AON_REQUIRE_AS(fn, rows_ok(N), "too many rows");
  hipStream_t st = (hipStream_t)stream;
  const bool small = N <= kDeformSmallRows;
  if (mode == 0)
    (small ? launch_deform<0, 1> : launch_deform<0, 2>)(packed, a0, a1, a3, N, S, xp, delta, st);
  else
    (small ? launch_deform<1, 1> : launch_deform<1, 2>)(packed, a0, a1, a3, N, S, xp, delta, st);
  return launch_status(fn);
}

extern "C" int aon_mlp_art_fwd_deform(const void* packed, const float* rays_o, const float* rays_d,
                                      const float* t, int64_t B, int S, float* xp, float* delta,
                                      aon_stream_t stream) {
  return deform_launch(0, __func__, packed, rays_o, rays_d, t, B, S, xp, delta, stream);
}

extern "C" int aon_mlp_art_fwd_deform_points(const void* packed, const float* pos, int64_t N,
                                             float* xp, float* delta, aon_stream_t stream) {
  return deform_launch(1, __func__, packed, pos, nullptr, nullptr, N, 1, xp, delta, stream);
}
