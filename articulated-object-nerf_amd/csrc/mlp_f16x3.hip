// Fused NeRFMLP forward on fp16 MFMA with a 3-product hi/lo split ("fp16x3").
//
// Every operand x is carried as x_hi = fp16(x) and x_lo = fp16(x - x_hi) (x - x_hi is exact in
// fp32): together ~22 significant bits.  A weight-activation product is
// w_hi*x_hi + w_hi*x_lo + w_lo*x_hi (the dropped w_lo*x_lo term is 2^-22 relative), three
// v_mfma_f32_16x16x32_f16 into ONE fp32 accumulator.  That is 3 fp16 MFMAs per 32-deep k-step
// where the fp32 path needs 8 v_mfma_f32_16x16x4_f32 of twice the cycles: 16/3 = 5.3x the
// arithmetic rate at fp32-class accuracy (measured against the reference in
// tests/test_gpu_parity.py).  Scales (exact powers of two, mlp_layout.hpp kActS / kWS):
// activations ride at 2^3 (kActS) and weights at 2^6 (kWS), so the unscaled lo parts stay
// normal in fp16 for |activation| >= 2^-6 and the products share the accumulator at 2^9; the
// epilogue folds 2^-6 and the bias into one fma.  fp16 then bounds a hidden activation at
// |x| < 65504 / 2^3 ~ 8188: every split value is range-tested and a wave that meets one sets
// the pack's status word (range guard, mlp_f16x3_core.hpp or_ballot; aon_mlp_read_status),
// and the callers fall back to the fp32 path or refuse the training step.
//
// Structure (mlp_layout.hpp kShapeH): feature-major tiles as in mlp.hip; a wave owns 16*NCOL
// samples; output tiles are produced in pairs (u, u+1) whose accumulators, converted in the
// epilogue, ARE the next layer's B operand for one 32-feature k-step (lane group g holds rows
// 4g..4g+3 of both tiles) -- no LDS round trip; the epilogue of pair p overlaps the MFMAs of
// pair p+1.  Weights stream through the same chunked LDS pipeline (mlp_pipe.hpp).
#include "mlp_f16x3_core.hpp"

namespace aon {
namespace mlp {

// per-lane LDS stash of the encodings: enc k-steps 0, 1 and venc, hi and lo (fp16x3) or hi only
// (bf16: no lo part); slot (c, i) at stash[64 (kStashPer c + i)].  SIG (the density-only pass):
// no venc slots
template <bool BF, bool SIG = false>
__host__ __device__ constexpr int stash_per() { return BF ? 3 : (SIG ? 4 : 6); }
template <bool BF, bool SIG = false>
__device__ __forceinline__ int enc_slot(int c, int k, int lo) {
  return BF ? 3 * c + k : stash_per<BF, SIG>() * c + 2 * k + lo;
}
template <bool BF>
__device__ __forceinline__ int venc_slot(int c, int lo) { return BF ? 3 * c + 2 : 6 * c + 4 + lo; }

// the density-only pass (mlp_layout.hpp NetVanillaSigmaH): the trunk and the density head
template <typename Net>
constexpr bool kSigmaOnly = std::is_same<Net, NetVanillaSigmaH>::value;
// the ring chunks of the prefix: whole chunks, and the last one holds a block the pass reads, so
// every copy the ring issues is waited for (DmaPipe::begin) before the kernel ends
static_assert(NetVanillaSigmaH::kChunk == kChunkH, "density-only stream: cut for this ring");

// The layer sequence of k_mlp_fwd_f16x3 (model.py:95-120)
template <typename Net, int NCOL, bool STORE, typename T, typename FP>
__device__ __forceinline__ void vanilla_layers(FP& fp, Frag<2, NCOL>& enc, Frag<1, NCOL>& venc,
                                               Frag<8, NCOL>& x, Frag<8, NCOL>& y, f4* stash,
                                               float* bias_s, int g,
                                               const int64_t (&rows)[NCOL], int64_t N, int act,
                                               float* __restrict__ raw, const TrainStore& ts) {
  constexpr bool BF = std::is_same<T, __bf16>::value;
  constexpr bool SIG = kSigmaOnly<Net>;
  static_assert(!SIG || (!STORE && !BF), "the density-only pass is a render pass");
  fp.start();  // begin(0): chunk 0 landed; the barrier also publishes bias_s
  lds_float* bias_l = opaque_lds(bias_s + 4 * g);  // this lane group's rows of the bias table

  Frag<1, NCOL> none;
  using SP = StorePick<STORE, NCOL, T>;
  // the kept activations (training forward): fp32, or bf16 in the bf16 training mode
  T* const th = reinterpret_cast<T*>(ts.h);
  T* const tbot = reinterpret_cast<T*>(ts.bot);
  T* const thv = reinterpret_cast<T*>(ts.hv);
  const int64_t hs = act_rows(N) * 256;  // one pts_linears output in ts.h
  const int64_t ms = act_rows(N) * 4;    // one layer's ReLU' bits in ts.masks
  layer_h<Net, L0, true>(fp, none, enc, x, bias_l, g, SP::make(th, 256, rows, N, g, ts.masks));
  layer_h<Net, L1, true>(fp, x, none, y, bias_l, g, SP::make(th + 1 * hs, 256, rows, N, g, ts.masks + 1 * ms));
  layer_h<Net, L2, true>(fp, y, none, x, bias_l, g, SP::make(th + 2 * hs, 256, rows, N, g, ts.masks + 2 * ms));
  layer_h<Net, L3, true>(fp, x, none, y, bias_l, g, SP::make(th + 3 * hs, 256, rows, N, g, ts.masks + 3 * ms));
  layer_h<Net, L4, true>(fp, y, none, x, bias_l, g, SP::make(th + 4 * hs, 256, rows, N, g, ts.masks + 4 * ms));
#pragma unroll
  for (int c = 0; c < NCOL; ++c)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      enc.hi[k][c] = __builtin_bit_cast(h8, stash[64 * enc_slot<BF, SIG>(c, k, 0)]);
      if (!BF) enc.lo[k][c] = __builtin_bit_cast(h8, stash[64 * enc_slot<BF, SIG>(c, k, 1)]);
    }
  // skip: cat[h, enc] (model.py:102-103)
  layer_h<Net, L5, true>(fp, x, enc, y, bias_l, g, SP::make(th + 5 * hs, 256, rows, N, g, ts.masks + 5 * ms));
  layer_h<Net, L6, true>(fp, y, none, x, bias_l, g, SP::make(th + 6 * hs, 256, rows, N, g, ts.masks + 6 * ms));
  layer_h<Net, L7, true>(fp, x, none, y, bias_l, g, SP::make(th + 7 * hs, 256, rows, N, g, ts.masks + 7 * ms));
  f4 dens[NCOL], rgb[NCOL];
  head_h<Net, LDEN>(fp, y, dens, bias_l, g);             // model.py:105-107
  constexpr bool FOLD = std::is_same<Net, NetVanillaFoldH>::value;
  static_assert(!FOLD || !STORE, "the training forwards keep the bottleneck activation");
  if constexpr (!SIG) {  // (the density-only pass: its stream ends with the density head)
    // bottleneck, no activation (model.py:109) -- the render stream has none: it is folded into
    // the view layer's weights (mlp_layout.hpp kLayoutHFold), which then reads h7 (y) itself
    if constexpr (!FOLD)
      layer_h<Net, LBOT, false>(fp, y, none, x, bias_l, g, SP::make(tbot, 256, rows, N, g));
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
      venc.hi[0][c] = __builtin_bit_cast(h8, stash[64 * venc_slot<BF>(c, 0)]);
      if (!BF) venc.lo[0][c] = __builtin_bit_cast(h8, stash[64 * venc_slot<BF>(c, 1)]);
    }
    // cat[bottleneck, enc_dir] + ReLU (:110-116), rgb head (:118)
    if constexpr (FOLD) {
      layer_h<Net, LF_VIEW, true>(fp, y, venc, x, bias_l, g);
      head_h<Net, LF_RGB>(fp, x, rgb, bias_l, g);
    } else {
      layer_h<Net, LVIEW, true>(fp, x, venc, y, bias_l, g, SP::make(thv, 128, rows, N, g, ts.masks + 8 * ms));
      head_h<Net, LRGB>(fp, y, rgb, bias_l, g);
    }
  }

  if (g == 0) {
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
      if (rows[c] < N) {
        float sig = dens[c][0];  // the heads are at true scale
        if (STORE && ts.noise) sig = __fadd_rn(sig, ts.noise[rows[c]]);  // raw_sigma + noise
        f4 o = {0.0f, 0.0f, 0.0f, act_sigma(sig, act)};  // density-only: no colour
        if constexpr (!SIG) {
          o[0] = act_rgb(rgb[c][0], act);
          o[1] = act_rgb(rgb[c][1], act);
          o[2] = act_rgb(rgb[c][2], act);
        }
        *reinterpret_cast<f4*>(raw + 4 * rows[c]) = o;
      }
    }
  }
}

// MODE 0: (rays_o, rays_d, viewdirs, t) inputs; MODE 1: encoded x (N, 63), condition (B, 27);
// MODE 2: (rays_o, rays_d, condition (B, 27), t) -- the position encoding in registers as in
// MODE 0, the per-ray view encoding read as in MODE 1 instead of 8 sines per lane and tile.
// BF: bf16 numerics (one bf16 MFMA per k-step; the kept activations stored as bf16) -- the
// bf16 training mode; the stream then carries bf16 weights in its hi blocks (k_pack_h bf16).
// Net: the stream's layer table -- NetVanillaFoldH for the render (no bottleneck layer),
// NetVanillaH for the training forwards (STORE), NetVanillaSigmaH for the density-only render
// pass (MODE 0 inputs without viewdirs: no view encoding is formed, split or stashed; the bias
// table and the status word are the whole render stream's, bias_g / status).
template <int MODE, int NCOL, bool STORE = false, bool BF = false, typename Net = NetVanillaH>
__global__ __launch_bounds__((GeomH<NCOL, BF>::kThreads), (GeomH<NCOL, BF>::kWavesPerSimd)) void k_mlp_fwd_f16x3(
    const f4* __restrict__ wstream, const float* __restrict__ bias_g, const float* __restrict__ in0,
    const float* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ in3,
    int64_t B, int S, int act, float* __restrict__ raw, TrainStore ts = {}) {
  using G = GeomH<NCOL, BF>;
  constexpr bool SIG = kSigmaOnly<Net>;
  static_assert(!SIG || MODE == 0, "the density-only pass takes MODE 0 inputs");
  // the per-lane stash of the encodings: enc 2 k-steps + venc 1, hi (& lo)
  using Lds = ChainLds<Net, G, stash_per<BF, SIG>() * NCOL>;
  __shared__ f4 smem[Lds::kF4];
  float* bias_s = Lds::bias(smem);
  f4* stash = Lds::stash(smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, j = lane & 15;
  const int64_t N = B * S;

  WeightPipeP<Net, G::kThreads, BF> p;
  start_chain<Net, G::kThreads>(p, smem, wstream, tid, lane, bias_s, bias_g);

  // layer-0 (enc) and view-layer (enc_dir) fragments: k-step k, lane group g, element e
  // <-> feature 32k + 8g + e of the encoding
  Frag<2, NCOL> enc;
  Frag<1, NCOL> venc;
  int64_t rows[NCOL];
#pragma unroll
  for (int c = 0; c < NCOL; ++c) {
    const int64_t row = (int64_t)blockIdx.x * G::kRowsPerBlock + wave * G::kRowsPerWave + 16 * c + j;
    rows[c] = row;
    const int64_t rr = row < N ? row : N - 1;
    const int64_t ray = rr / S;
    float ev[2][8], vv[8];
    if constexpr (MODE == 0 && !SIG) {
      const float* ro = in0 + 3 * ray;
      const float* rd = in1 + 3 * ray;
      const float* vd = in2 + 3 * ray;
      const float tt = in3[rr];
      const float x0 = __fadd_rn(ro[0], __fmul_rn(tt, rd[0]));
      const float x1 = __fadd_rn(ro[1], __fmul_rn(tt, rd[1]));
      const float x2 = __fadd_rn(ro[2], __fmul_rn(tt, rd[2]));
      const float v0 = vd[0], v1 = vd[1], v2 = vd[2];
      auto encode = [&](auto fast) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
          for (int e = 0; e < 8; ++e)
          {
            ev[k][e] = pos_enc_feature_fast(x0, x1, x2, 32 * k + 8 * g + e, 0, 10, fast.value);
            __builtin_amdgcn_sched_barrier(0);  // one feature's fp64 temporaries live at a time
          }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          vv[e] = pos_enc_feature_fast(v0, v1, v2, 8 * g + e, 0, 4, fast.value);
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      // every argument of the wave below kSinCrMax (aon_common.hpp): no per-value range branch
      if (pos_enc_fast_ok(x0, x1, x2, 10) && pos_enc_fast_ok(v0, v1, v2, 4))
        encode(std::true_type{});
      else
        encode(std::false_type{});
    } else if constexpr (MODE == 0 || MODE == 2) {
      // the density-only pass, or MODE 2: pos_enc(x) as above, no sine of the view direction
      const float* ro = in0 + 3 * ray;
      const float* rd = in1 + 3 * ray;
      const float tt = in3[rr];
      const float x0 = __fadd_rn(ro[0], __fmul_rn(tt, rd[0]));
      const float x1 = __fadd_rn(ro[1], __fmul_rn(tt, rd[1]));
      const float x2 = __fadd_rn(ro[2], __fmul_rn(tt, rd[2]));
      auto encode = [&](auto fast) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
          for (int e = 0; e < 8; ++e)
          {
            ev[k][e] = pos_enc_feature_fast(x0, x1, x2, 32 * k + 8 * g + e, 0, 10, fast.value);
            __builtin_amdgcn_sched_barrier(0);  // one feature's fp64 temporaries live at a time
          }
      };
      // (fast or not, a feature is the same value bit for bit: aon_common.hpp)
      if (pos_enc_fast_ok(x0, x1, x2, 10))
        encode(std::true_type{});
      else
        encode(std::false_type{});
      if constexpr (MODE == 2) {
        const float* cd = in2 + ray * 27;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int f = 8 * g + e;
          vv[e] = f < 27 ? cd[f] : 0.f;
        }
      }
    } else {
      const float* x = in0 + rr * 63;
      const float* cd = in1 + ray * 27;
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int f = 32 * k + 8 * g + e;
          ev[k][e] = f < 63 ? x[f] : 0.f;
        }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int f = 8 * g + e;
        vv[e] = f < 27 ? cd[f] : 0.f;
      }
    }
    if (STORE && BF && ts.enc_bf && keep_row(rows[c], N)) store_enc_bf(ts.enc_bf, rows[c], g, ev);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
      for (int e = 0; e < 8; ++e) ev[k][e] *= act_scale<BF>();
      split8<BF>(ev[k], enc.hi[k][c], enc.lo[k][c], enc.ovf);
    }
    if constexpr (!SIG) {
#pragma unroll
      for (int e = 0; e < 8; ++e) vv[e] *= act_scale<BF>();
      split8<BF>(vv, venc.hi[0][c], venc.lo[0][c], venc.ovf);
    }
  }

  // park the encodings in LDS until the skip / view layers need them (frees 24 VGPRs for the
  // fragment prefetch); only the owning lane ever touches its slots
#pragma unroll
  for (int c = 0; c < NCOL; ++c) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      stash[64 * enc_slot<BF, SIG>(c, k, 0)] = __builtin_bit_cast(f4, enc.hi[k][c]);
      if (!BF) stash[64 * enc_slot<BF, SIG>(c, k, 1)] = __builtin_bit_cast(f4, enc.lo[k][c]);
    }
    if constexpr (!SIG) {
      stash[64 * venc_slot<BF>(c, 0)] = __builtin_bit_cast(f4, venc.hi[0][c]);
      if (!BF) stash[64 * venc_slot<BF>(c, 1)] = __builtin_bit_cast(f4, venc.lo[0][c]);
    }
  }

  Frag<8, NCOL> x, y;
  using WP = WeightPipeP<Net, G::kThreads, BF>;
  using T = typename std::conditional<BF, __bf16, float>::type;
  FragPipe<WP, AON_PREFETCH, BF> fp(p);
  vanilla_layers<Net, NCOL, STORE, T>(fp, enc, venc, x, y, stash, bias_s, g, rows, N, act, raw, ts);
  // every split of this launch: the layers' (x, y) and the encodings' (venc.ovf stays 0 in the
  // density-only pass, which splits none); the status word sits behind the WHOLE bias table
  constexpr int kStatusAt = SIG ? NetVanillaFoldH::kBiasFloats : Net::kBiasFloats;
  range_report(bias_g + kStatusAt, ovf_of(x) | ovf_of(y) | enc.ovf | venc.ovf);
}

// ---- packing: torch [out][ldw] fp32 -> hi/lo fp16 blocks (+ biases at activation scale), for
// any NetH layer table (passed by value with each layer's weight row stride)
__global__ void k_pack_h(PackArgsH a, float* __restrict__ out_f) {
  const int64_t nhalf = (int64_t)a.stream_blocks * 512;  // fp16 elements of the stream
  _Float16* out = reinterpret_cast<_Float16*>(out_f);
  float* bias_out = out_f + (int64_t)a.stream_blocks * 256;
  const int64_t total = nhalf + a.bias_floats;
  const LayerDesc& last = a.layers[a.n_layers - 1];
  const int used_blocks = last.blk0 + (last.ka + last.kb) * last.u * 2;
  const StreamMap map{a.bf16, a.mx_lo, a.mx_hi};
  // an all-bf16 stream never reports (no weight is range-tested): the status words are cleared
  // here instead of by a memset launch ahead of the pack (pack_h)
  if (a.bf16 == 1 && !a.f16w && blockIdx.x == 0 && threadIdx.x < kStatusBytes / 4)
    reinterpret_cast<uint32_t*>(bias_out + a.bias_floats)[threadIdx.x] = 0u;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    if (e < nhalf) {
      // element e of stream block m is element e of fp16x3 block map.unmap(m) (StreamMap):
      // past the used blocks (the compact modes' tail of the stream region) it maps past the
      // weights and is zero
      const int blk = map.unmap(static_cast<int>(e >> 9));
      const bool bf = !map.f16(blk);  // a bf16 (hi-only) block
      const int l = static_cast<int>((e >> 3) & 63), jj = static_cast<int>(e & 7);
      float w = 0.f;
      bool lo_part = false;
      if (blk < used_blocks) {
        int li = 0;
        while (li + 1 < a.n_layers && a.layers[li + 1].blk0 <= blk) ++li;
        const LayerDesc d = a.layers[li];
        const int K = d.ka + d.kb;
        const int q = (blk - d.blk0) >> 1;
        lo_part = ((blk - d.blk0) & 1) != 0;
        int u, k;
        if (d.u == 1) {
          u = 0;
          k = q;
        } else {
          u = 2 * ((q >> 1) / K) + (q & 1);
          k = (q >> 1) % K;
        }
        const int o = 16 * u + (l & 15), gg = l >> 4;
        int col = -1;
        const float* src = a.w[li];
        int64_t ld = a.ldw[li];
        if (k < d.ka) {  // previous-layer output fragment order
          const int f = 32 * k + 16 * (jj >> 2) + 4 * gg + (jj & 3);
          col = f < d.len_a ? f : -1;
        } else {  // in-register encodings: natural order
          const int f = 32 * (k - d.ka) + 8 * gg + jj;
          col = f < d.len_b ? (a.w2[li] ? f : d.len_a + f) : -1;
          if (a.w2[li]) {
            src = a.w2[li];
            ld = a.ldw2[li];
          }
        }
        if (o < d.out_real && col >= 0) {
          if (a.fold_w && li == a.fold_layer && k < d.ka) {
            // folded segment A (PackArgsH fold_w): fp64 in index order, one rounding to fp32
            double acc = 0.0;
            for (int j = 0; j < a.fold_k; ++j)
              acc = fma(static_cast<double>(src[(int64_t)o * ld + j]),
                        static_cast<double>(a.fold_w[(int64_t)j * d.len_a + col]), acc);
            w = static_cast<float>(acc);
          } else {
            w = a.tr[li] ? src[(int64_t)col * ld + o] : src[(int64_t)o * ld + col];
          }
        }
      }
      if (bf && !a.f16w) {  // bf16 layer: bf16(w), unscaled, in the compact (hi-only) stream
        out[e] = bf_bits(w);
        continue;
      }
      w *= kWS;  // exact (power of two)
      const _Float16 h = static_cast<_Float16>(w);
      out[e] = lo_part ? static_cast<_Float16>(w - static_cast<float>(h)) : h;
      // range guard (mlp_f16x3_core.hpp): a weight whose scaled hi part is not a finite fp16
      // makes every kernel reading this stream invalid -- status 2 (the word was cleared by
      // pack_h before this launch; many lanes may store the same value)
      if (!lo_part && !(fabsf(w) <= kF16Max))
        *reinterpret_cast<uint32_t*>(bias_out + a.bias_floats) = 2u;
    } else {
      const int i = static_cast<int>(e - nhalf);
      int li = 0;
      while (li + 1 < a.n_layers && a.layers[li + 1].bias0 <= i) ++li;
      const int o = i - a.layers[li].bias0;
      // hidden layers add the bias at activation scale; the 1-tile heads at true scale
      // (bf16 layers: at true scale, their activations are unscaled)
      const StreamMap map{a.bf16, a.mx_lo, a.mx_hi};
      const float bs =
          a.layers[li].u == 1 || !(map.f16(a.layers[li].blk0) || a.f16w) ? 1.0f : kActS;
      float b = (o < a.layers[li].out_real && a.b[li]) ? a.b[li][o] : 0.f;
      if (a.fold_w && li == a.fold_layer && o < a.layers[li].out_real) {
        // folded bias: b[o] + sum_j w[o][j] fold_b[j], fp64 in index order, rounded once
        double acc = 0.0;
        for (int j = 0; j < a.fold_k; ++j)
          acc = fma(static_cast<double>(a.w[li][(int64_t)o * a.ldw[li] + j]),
                    static_cast<double>(a.fold_b[j]), acc);
        b = static_cast<float>(static_cast<double>(b) + acc);
      }
      bias_out[i] = b * bs;
    }
  }
}

int pack_h(PackArgsH a, void* packed, hipStream_t stream) {
  const int64_t total = (int64_t)a.stream_blocks * 512 + a.bias_floats;
  // the range-status word behind the bias table: cleared (stream-ordered) before the pack, which
  // sets it for an unrepresentable weight; the kernels reading the stream set it on overflow
  // (an all-bf16 stream: k_pack_h clears it itself, one launch fewer)
  if (a.bf16 != 1 || a.f16w) {
    const hipError_t e = hipMemsetAsync(
        static_cast<char*>(packed) + (size_t)a.stream_blocks * 1024 + (size_t)a.bias_floats * 4, 0,
        kStatusBytes, stream);
    if (e != hipSuccess) return static_cast<int>(e);
  }
  hipLaunchKernelGGL(k_pack_h, grid_for(total, 256, 4096), 256, 0, stream, a,
                     static_cast<float*>(packed));
  return launch_status("aon_mlp_pack");
}

int pack_f16x3(const PackArgs& a, void* packed, hipStream_t stream, bool bf16, bool fold) {
  PackArgsH h{};
  h.bf16 = bf16 ? 1 : 0;
  if (fold) {
    // the render stream: kShapeH without the bottleneck, folded into the view layer
    fill_net<NetVanillaFoldH>(h);
    h.fold_w = a.w[LBOT];
    h.fold_b = a.b[LBOT];
    h.fold_layer = LF_VIEW;
    h.fold_k = NetVanillaH::layer(LBOT).out_real;
  } else {
    fill_net<NetVanillaH>(h);
  }
  for (int i = 0; i < h.n_layers; ++i) {
    const int src = fold && i >= LBOT ? i + 1 : i;
    h.w[i] = a.w[src];
    h.b[i] = a.b[src];
  }
  return pack_h(h, packed, stream);
}

// one launch of k_mlp_fwd_f16x3<MODE, NCOL, STORE, BF, Net>, reported as fn (the density-only
// pass reads a prefix of the render pack: its bias table sits behind the whole folded stream)
template <int MODE, int NCOL, bool STORE, bool BF, typename Net>
static int launch_fwd(const char* fn, const void* packed, const float* a0, const float* a1,
                      const float* a2, const float* a3, int64_t B, int S, int act, float* raw,
                      hipStream_t stream, const TrainStore& ts = {}) {
  using G = GeomH<NCOL, BF>;
  using Packed = typename std::conditional<kSigmaOnly<Net>, NetVanillaFoldH, Net>::type;
  static_assert(kRowsOkCovers<G>, "the callers' rows_ok covers this grid");
  hipLaunchKernelGGL((k_mlp_fwd_f16x3<MODE, NCOL, STORE, BF, Net>), chain_grid<G>(B * S),
                     G::kThreads, 0, stream, static_cast<const f4*>(packed),
                     stream_bias<Packed>(packed), a0, a1, a2, a3, B, S, act, raw, ts);
  return launch_status(fn);
}

int launch_f16x3_train(bool bf16, const TrainStore& ts, const void* packed, const float* rays_o,
                       const float* rays_d, const float* viewdirs, const float* t, int64_t B,
                       int S, float* raw, hipStream_t stream) {
  // (the bf16 training mode: 16 kBfNcolFwd samples per wave)
  const auto launch = bf16 ? launch_fwd<0, kBfNcolFwd, true, true, NetVanillaH>
                           : launch_fwd<0, 1, true, false, NetVanillaH>;
  return launch("aon_mlp_fwd_train", packed, rays_o, rays_d, viewdirs, t, B, S, AON_ACT_NONE, raw,
                stream, ts);
}

int launch_f16x3_render(bool encoded, int ncol, const void* packed, const float* a0,
                        const float* a1, const float* a2, const float* a3, int64_t B, int S,
                        int act, float* raw, hipStream_t stream) {
  using Net = NetVanillaFoldH;
  const auto launch =
      !encoded ? (ncol == 1 ? launch_fwd<0, 1, false, false, Net> : launch_fwd<0, 2, false, false, Net>)
               : (ncol == 1 ? launch_fwd<1, 1, false, false, Net> : launch_fwd<1, 2, false, false, Net>);
  return launch("aon_mlp_fwd", packed, a0, a1, a2, a3, B, S, act, raw, stream, TrainStore{});
}

int launch_f16x3_sigma(const void* packed, const float* rays_o, const float* rays_d,
                       const float* t, int64_t B, int S, int act, float* raw, hipStream_t stream) {
  return launch_fwd<0, 1, false, false, NetVanillaSigmaH>("aon_mlp_fwd_sigma", packed, rays_o,
                                                          rays_d, nullptr, t, B, S, act, raw, stream);
}

int launch_f16x3_cond(const void* packed, const float* rays_o, const float* rays_d,
                      const float* cond, const float* t, int64_t B, int S, int act, float* raw,
                      hipStream_t stream) {
  return launch_fwd<2, 1, false, false, NetVanillaFoldH>("aon_mlp_fwd_cond", packed, rays_o, rays_d,
                                                         cond, t, B, S, act, raw, stream);
}

}  // namespace mlp
}  // namespace aon
