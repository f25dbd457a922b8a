// The articulated NeRFMLP's density alone (reference models/vanilla_nerf/model_autodecoder.py:
// 196-223), on the fp16x3 MFMA path of mlp_art.hip:
//
//   xyz = o + t d                                     (helper.py:25-26; or given points)
//   h = relu(D3 relu(D2 relu(D1 relu(D0 [xyz | shape, art]))))          :196-203
//   x' = deformation_layer(h) + xyz;  enc = pos_enc(x', 0, 10)          :205-212
//   trunk on [enc | shape] with the skip concat, density_layer          :214-223
//
// -- everything k_mlp_art_f16x3 does up to and including its density head, operation for
// operation, and nothing after it: no view encoding, no bottleneck_layer, no views_linear.0-3, no
// rgb_layer.  The pass reads the density PREFIX of an aon_mlp_art_pack stream in place
// (mlp_layout.hpp NetArtSigmaH: kBlocks of NetArtH's blocks, kBiasFloats of its bias rows, its
// status word), so sigma is the full kernel's sigma bit for bit.  Two callers: the coarse level
// of a render that keeps only the fine level (its colour reaches nothing, its sigma the fine
// level's samples), and density queries at given points.
//
// Budget.  The trunk is 256 wide, so a wave's two activation fragments are the full kernel's
// Frag<8, 1> pair (128 VGPRs): 2 waves per SIMD, one 8-wave workgroup per CU, as there -- whatever
// the LDS holds.  The ring keeps the full kernel's cadence (3 chunks of kChunkH blocks, 96 KB);
// behind it sit the prefix's 2,592 bias floats and 4 stash slots per lane (enc hi / lo of two
// k-steps; the full kernel's two venc slots are gone).
#include "mlp_f16x3_core.hpp"

namespace aon {
namespace mlp {

static_assert(NetArtSigmaH::kChunk == kChunkH, "density prefix: cut for the chain ring");

// MODE 0: (rays_o, rays_d, t) inputs; MODE 1: points (N, 3).  raw: (N, 4) rows {0, 0, 0, sigma}.
template <int MODE>
__global__ __launch_bounds__(GeomH<1>::kThreads, 2) void k_mlp_art_sigma_f16x3(
    const f4* __restrict__ wstream, const float* __restrict__ bias_g, const float* __restrict__ in0,
    const float* __restrict__ in1, const float* __restrict__ in3, int64_t N, int S, int act,
    float* __restrict__ raw) {
  constexpr int NCOL = 1;
  using G = GeomH<NCOL>;
  using Net = NetArtSigmaH;
  using Lds = ChainLds<Net, G, 4 * NCOL>;  // per lane: enc 2 k-steps, hi & lo
  __shared__ f4 smem[Lds::kF4];
  float* bias_s = Lds::bias(smem);
  f4* stash = Lds::stash(smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, j = lane & 15;

  using WP = WeightPipe<Net, G::kThreads>;
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

  Frag<8, NCOL> x, y;
  Frag<1, NCOL> none;
  // deformation MLP (model_autodecoder.py:196-205)
  layer_h<Net, A_D0, true>(fp, none, din, x, bias_l, g);
  layer_h<Net, A_D1, true>(fp, x, none, y, bias_l, g);
  layer_h<Net, A_D2, true>(fp, y, none, x, bias_l, g);
  layer_h<Net, A_D3, true>(fp, x, none, y, bias_l, g);
  f4 dlt[NCOL];
  head_h<Net, A_DOUT>(fp, y, dlt, bias_l, g);

  // x' = deformation + xyz, pos_enc(x') (enc_after, :205-212)
  Frag<2, NCOL> enc;
#pragma unroll
  for (int c = 0; c < NCOL; ++c) {
    float q3[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) q3[q] = __fadd_rn(__shfl(dlt[c][q], j, 64), px[c][q]);
    float ev[2][8];
    auto enc_fn = [&](auto fast) {
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float f =
              pos_enc_feature_fast(q3[0], q3[1], q3[2], 32 * k + 8 * g + e, 0, 10, fast.value);
          ev[k][e] = f * kActS;
          __builtin_amdgcn_sched_barrier(0);  // one feature's fp64 temporaries live at a time
        }
    };
    if (pos_enc_fast_ok(q3[0], q3[1], q3[2], 10))
      enc_fn(std::true_type{});
    else
      enc_fn(std::false_type{});
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      split8(ev[k], enc.hi[k][c], enc.lo[k][c], enc.ovf);
      stash[64 * (4 * c + 2 * k)] = __builtin_bit_cast(f4, enc.hi[k][c]);
      stash[64 * (4 * c + 2 * k + 1)] = __builtin_bit_cast(f4, enc.lo[k][c]);
    }
  }

  // trunk on cat[enc, shape] (:214-220), shape folded into the pts_linears.0 / .5 biases
  layer_h<Net, A_P0, true>(fp, none, enc, x, bias_l, g);
  layer_h<Net, A_P1, true>(fp, x, none, y, bias_l, g);
  layer_h<Net, A_P2, true>(fp, y, none, x, bias_l, g);
  layer_h<Net, A_P3, true>(fp, x, none, y, bias_l, g);
  layer_h<Net, A_P4, true>(fp, y, none, x, bias_l, g);
#pragma unroll
  for (int c = 0; c < NCOL; ++c)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      enc.hi[k][c] = __builtin_bit_cast(h8, stash[64 * (4 * c + 2 * k)]);
      enc.lo[k][c] = __builtin_bit_cast(h8, stash[64 * (4 * c + 2 * k + 1)]);
    }
  // skip: cat[h, enc, shape]
  layer_h<Net, A_P5, true>(fp, x, enc, y, bias_l, g);
  layer_h<Net, A_P6, true>(fp, y, none, x, bias_l, g);
  layer_h<Net, A_P7, true>(fp, x, none, y, bias_l, g);
  f4 dens[NCOL];
  head_h<Net, A_DEN>(fp, y, dens, bias_l, g);  // :221-223

  // the head's tile holds sigma in lane group 0 (row 0, column = sample): density only, no colour
  if (g == 0) {
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
      if (rows[c] < N) {
        const f4 o = {0.0f, 0.0f, 0.0f, act_sigma(dens[c][0], act)};
        *reinterpret_cast<f4*>(raw + 4 * rows[c]) = o;
      }
    }
  }
  // the status word of the whole pack, behind the whole stream's bias table
  range_report(bias_g + NetArtH::kBiasFloats, ovf_of(x) | ovf_of(y) | enc.ovf | din.ovf);
}

}  // namespace mlp
}  // namespace aon

using namespace aon;
using namespace aon::mlp;

static int sigma_launch(int mode, const char* fn, const void* packed, const float* a0,
                        const float* a1, const float* a3, int64_t B, int S, int act, float* out,
                        aon_stream_t stream) {
  AON_REQUIRE_AS(fn, packed && out && a0 && (mode == 1 || (a1 && a3)), "null pointer");
  if (check_fwd_args(fn, packed, out, B, S, act)) return -1;
  AON_REQUIRE_AS(fn, B <= INT64_MAX / S, "too many rows");
  const int64_t N = B * S;
  if (N == 0) return 0;
  using G = GeomH<1>;
  AON_REQUIRE_AS(fn, rows_ok(N), "too many rows");
  static_assert(kRowsOkCovers<G>, "rows_ok covers this grid");
  hipLaunchKernelGGL((mode == 0 ? k_mlp_art_sigma_f16x3<0> : k_mlp_art_sigma_f16x3<1>),
                     chain_grid<G>(N), G::kThreads, 0, (hipStream_t)stream,
                     static_cast<const f4*>(packed), stream_bias<NetArtH>(packed), a0, a1, a3, N, S,
                     act, out);
  return launch_status(fn);
}

extern "C" int aon_mlp_art_fwd_sigma(const void* packed, const float* rays_o, const float* rays_d,
                                     const float* t, int64_t B, int S, int act, float* out,
                                     aon_stream_t stream) {
  return sigma_launch(0, __func__, packed, rays_o, rays_d, t, B, S, act, out, stream);
}

extern "C" int aon_mlp_art_fwd_sigma_points(const void* packed, const float* pos, int64_t N, int act,
                                            float* out, aon_stream_t stream) {
  return sigma_launch(1, __func__, packed, pos, nullptr, nullptr, N, 1, act, out, stream);
}
