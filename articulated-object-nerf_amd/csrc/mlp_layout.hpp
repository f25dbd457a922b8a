// Compile-time layout of the packed NeRFMLP weight stream (shared by pack and forward).
//
// The MLP runs "feature-major": a layer computes D[out][sample] = W[out][in] . H[in][sample]
// with 16x16 MFMA tiles, samples on the MFMA column (lane & 15) and features on the rows.
// The accumulator of one layer is then already the B operand of the next (no LDS round
// trip): k-step (t, r) of the next layer takes register r of feature tile t, whose lane group
// g = lane >> 4 holds input feature 16t + 4g + r.
//
// Weight stream = the A operands in consumption order.  One 1-KB "block" (t, u) holds, for lane
// l, the float4 W[16u + (l & 15)][16t + 4(l >> 4) + 0..3] -> one conflict-free ds_read_b128 per
// lane feeds 4 MFMAs.  Blocks are ordered layer by layer, t-major, u-minor, and padded to whole
// LDS chunks.  Inputs with two concatenated segments (the skip layer cat[h, enc], the view
// layer cat[bottleneck, enc_dir]; reference model.py:102-103, 113) are two K ranges of the same
// layer; padded features (63 -> 64, 27 -> 32) carry zero weights.
#pragma once

namespace aon {
namespace mlp {

struct LayerDesc {
  int ka, kb;        // 16-feature input tiles of segment A / B
  int u;             // 16-row output tiles
  int len_a, len_b;  // real columns of segment A / B in the torch weight ([out][len_a+len_b])
  int out_real;      // real output rows
  int blk0;          // first 1-KB block in the stream
  int bias0;         // first float in the bias table (u*16 floats per layer)
};

// A network is STATED as a shape table, one LayerShape per layer in consumption order; where
// each layer sits in the stream is derived (build_layout): blk0 and bias0 are running sums.
struct LayerShape {
  int ka, kb, u, len_a, len_b, out_real;  // as in LayerDesc
};
template <int N>
struct Layout {
  static constexpr int kNumLayers = N;
  LayerDesc layer[N];
  int blocks;       // blocks carrying weights
  int bias_floats;  // 16 per output tile
};
// blocks_per_step: 1-KB blocks per (output tile, k-step) -- 1 on the fp32 grid, 2 (hi, lo) on
// the fp16x3 grid.  DROP >= 0: the table without that row.
template <int DROP = -1, int N>
constexpr Layout<(DROP < 0 ? N : N - 1)> build_layout(const LayerShape (&s)[N],
                                                      int blocks_per_step) {
  Layout<(DROP < 0 ? N : N - 1)> l{};
  for (int i = 0, o = 0; i < N; ++i) {
    if (i == DROP) continue;
    const LayerShape& r = s[i];
    l.layer[o++] = {r.ka, r.kb, r.u, r.len_a, r.len_b, r.out_real, l.blocks, l.bias_floats};
    l.blocks += (r.ka + r.kb) * r.u * blocks_per_step;
    l.bias_floats += 16 * r.u;
  }
  return l;
}
constexpr int round_up(int x, int m) { return (x + m - 1) / m * m; }
// (The built layouts below are plain namespace-scope constexpr objects, one per translation unit,
// not `inline`: making them so is a change with its own assembly diff)

enum { L0 = 0, L1, L2, L3, L4, L5, L6, L7, LDEN, LBOT, LVIEW, LRGB, kNumLayers };

constexpr int kChunk = 16;  // 1-KB blocks per LDS pipeline stage

// the exact-fp32 kernel (mlp.hip): ka/kb count 16-feature tiles
constexpr LayerShape kShape32[kNumLayers] = {
    {4, 0, 16, 63, 0, 256},     // pts_linears.0   256 x 63
    {16, 0, 16, 256, 0, 256},   // pts_linears.1
    {16, 0, 16, 256, 0, 256},   // pts_linears.2
    {16, 0, 16, 256, 0, 256},   // pts_linears.3
    {16, 0, 16, 256, 0, 256},   // pts_linears.4
    {16, 4, 16, 256, 63, 256},  // pts_linears.5   256 x (256 + 63)
    {16, 0, 16, 256, 0, 256},   // pts_linears.6
    {16, 0, 16, 256, 0, 256},   // pts_linears.7
    {16, 0, 1, 256, 0, 1},      // density_layer     1 x 256
    {16, 0, 16, 256, 0, 256},   // bottleneck_layer 256 x 256
    {16, 2, 8, 256, 27, 128},   // views_linear.0  128 x (256 + 27)
    {8, 0, 1, 128, 0, 3},       // rgb_layer         3 x 128
};
constexpr auto kLayout32 = build_layout(kShape32, 1);

// The fp16x3 kernel (mlp_f16x3.hip) walks the SAME block grid with 32-feature k-steps and
// two 1-KB blocks (hi, lo) per (u, k-step): ka/kb count 32-feature k-steps, and segment B
// (enc / enc_dir, computed in-register) uses the natural feature order.
constexpr LayerShape kShapeH[kNumLayers] = {
    {0, 2, 16, 0, 63, 256},     // pts_linears.0: enc only (segment B)
    {8, 0, 16, 256, 0, 256},
    {8, 0, 16, 256, 0, 256},
    {8, 0, 16, 256, 0, 256},
    {8, 0, 16, 256, 0, 256},
    {8, 2, 16, 256, 63, 256},
    {8, 0, 16, 256, 0, 256},
    {8, 0, 16, 256, 0, 256},
    {8, 0, 1, 256, 0, 1},       // density_layer
    {8, 0, 16, 256, 0, 256},    // bottleneck_layer
    {8, 1, 8, 256, 27, 128},    // views_linear.0
    {4, 0, 1, 128, 0, 3},       // rgb_layer
};
constexpr auto kLayoutH = build_layout(kShapeH, 2);

// The fp16x3 RENDER stream (inference: aon_mlp_fwd / aon_mlp_fwd_encoded): bottleneck_layer has
// no activation (model.py:109) and feeds only views_linear.0, so the two linear maps are one --
//   z_view = (Wv[:, :256] Wb) h7 + Wv[:, 256:] enc_dir + (bv + Wv[:, :256] bb)
// -- and the stream is kShapeH without LBOT: the view layer's segment A is h7 with the folded
// 128 x 256 weight, formed by the pack (k_pack_h fold_w).  65,536 of the 593,408 MAC per sample
// (11%) and the bottleneck's 256 blocks go.  The training forwards keep the unfolded stream
// (they store the bottleneck activation for the backward).
enum { LF_VIEW = LDEN + 1, LF_RGB, kNumLayersFold };
constexpr auto kLayoutHFold = build_layout<LBOT>(kShapeH, 2);
static_assert(kLayoutHFold.layer[LF_VIEW].len_a == kLayoutH.layer[LBOT].out_real,
              "the folded view layer reads what the bottleneck read");

// fp16x3 numerics: activations carried at 2^3, weights at 2^6, so the lo parts (x - fp16(x))
// stay in fp16's normal range unscaled and hi*hi, hi*lo, lo*hi share ONE fp32 accumulator at
// scale 2^9; the epilogue folds the 2^-6 and the bias into one fma.  A hidden activation past
// 65504 / 2^3 overflows the hi part: the range guard reports it.
constexpr float kActS = 8.0f;
constexpr float kWS = 64.0f;

// the fp32 stream: whole chunks of 16/32/64
constexpr int kBlocks = kLayout32.blocks;
constexpr int kStreamBlocks = round_up(kBlocks, 64);
constexpr int kNumChunks = kStreamBlocks / kChunk;
constexpr int kBiasFloats = kLayout32.bias_floats;
constexpr size_t kStreamBytesF32 = (size_t)kStreamBlocks * 1024;
// every packed buffer ends in a 16-B status block (word 0: the fp16x3 range guard,
// mlp_f16x3_core.hpp range_report; zeroed by the pack, read by aon_mlp_status)
constexpr size_t kStatusBytes = 16;
constexpr size_t kPackedBytesF32 = kStreamBytesF32 + kBiasFloats * 4 + kStatusBytes;

constexpr bool layout_ok() {
  for (const LayerDesc& d : kLayout32.layer) {
    if (d.blk0 % kChunk) return false;  // every layer starts on a chunk boundary
    if (!(d.u == 1 || d.u % 4 == 0)) return false;
  }
  return true;
}
static_assert(layout_ok(), "inconsistent MLP stream layout");

constexpr bool layout_h_ok() {
  for (int i = 0; i < kNumLayers; ++i) {
    const LayerDesc& a = kLayout32.layer[i];
    const LayerDesc& h = kLayoutH.layer[i];
    if (a.blk0 != h.blk0 || a.bias0 != h.bias0 || a.u != h.u) return false;
    if ((h.ka + h.kb) * h.u * 2 != (a.ka + a.kb) * a.u) return false;
  }
  return true;
}
static_assert(layout_h_ok(), "fp16x3 layout must share the block grid");

// ---- the articulated NeRFMLP (reference model_autodecoder.py:60-239, default geometry) on the
// fp16x3 path, after latent folding: the latent columns of deformations_linear.0,
// pts_linears.0 / .5 and views_linear.0 meet the same (1, C) code on every sample, so their
// products are per-call biases (NeRFMLP.folded_biases) and the stream holds only the
// per-sample columns.  Same block grid rules as kShapeH; ka/kb in 32-feature k-steps.
enum {
  A_D0 = 0, A_D1, A_D2, A_D3, A_DOUT,
  A_P0, A_P1, A_P2, A_P3, A_P4, A_P5, A_P6, A_P7,
  A_DEN, A_BOT, A_V0, A_V1, A_V2, A_V3, A_RGB, kNumLayersArt
};

constexpr LayerShape kShapeArt[kNumLayersArt] = {
    {0, 1, 8, 0, 3, 128},       // deformations_linear.0  128 x 3 (xyz columns)
    {4, 0, 8, 128, 0, 128},     // deformations_linear.1
    {4, 0, 8, 128, 0, 128},     // deformations_linear.2
    {4, 0, 8, 128, 0, 128},     // deformations_linear.3
    {4, 0, 1, 128, 0, 3},       // deformation_layer        3 x 128
    {0, 2, 16, 0, 63, 256},     // pts_linears.0   256 x 63 (enc columns)
    {8, 0, 16, 256, 0, 256},    // pts_linears.1
    {8, 0, 16, 256, 0, 256},    // pts_linears.2
    {8, 0, 16, 256, 0, 256},    // pts_linears.3
    {8, 0, 16, 256, 0, 256},    // pts_linears.4
    {8, 2, 16, 256, 63, 256},   // pts_linears.5   256 x (256 + 63)
    {8, 0, 16, 256, 0, 256},    // pts_linears.6
    {8, 0, 16, 256, 0, 256},    // pts_linears.7
    {8, 0, 1, 256, 0, 1},       // density_layer    1 x 256
    {8, 0, 16, 256, 0, 256},    // bottleneck_layer 256 x 256
    {8, 1, 8, 256, 27, 128},    // views_linear.0   128 x (256 + 27)
    {4, 0, 8, 128, 0, 128},     // views_linear.1
    {4, 0, 8, 128, 0, 128},     // views_linear.2
    {4, 0, 8, 128, 0, 128},     // views_linear.3
    {4, 0, 1, 128, 0, 3},       // rgb_layer        3 x 128
};
constexpr auto kLayoutArt = build_layout(kShapeArt, 2);

// ---- backward chain of the vanilla NeRFMLP (training, model.py:95-120 under autograd): the
// input gradients dL/dX = dZ W (W^T applied feature-major), last layer first, each masked by
// ReLU' of the forward output it flows into.  Row o of a layer = an INPUT feature of the forward
// layer, columns = its outputs; packed from the forward weights with tr = 1.
enum { B_RGB = 0, B_VIEW, B_BOTDEN, B_7, B_6, B_5, B_4, B_3, B_2, B_1, kNumLayersBwd };

constexpr LayerShape kShapeBwd[kNumLayersBwd] = {
    {0, 1, 8, 0, 3, 128},       // rgb_layer^T: d hv = W_rgb^T d rgb (3 -> 128)
    {4, 0, 16, 128, 0, 256},    // views_linear.0^T, bottleneck columns only
    {8, 1, 16, 256, 1, 256},    // [bottleneck^T | density^T]: d h7
    {8, 0, 16, 256, 0, 256},    // pts_linears.7^T: d h6
    {8, 0, 16, 256, 0, 256},    // pts_linears.6^T: d h5
    {8, 0, 16, 256, 0, 256},    // pts_linears.5^T, h4 columns only (not enc)
    {8, 0, 16, 256, 0, 256},    // pts_linears.4^T: d h3
    {8, 0, 16, 256, 0, 256},    // pts_linears.3^T: d h2
    {8, 0, 16, 256, 0, 256},    // pts_linears.2^T: d h1
    {8, 0, 16, 256, 0, 256},    // pts_linears.1^T: d h0
};
constexpr auto kLayoutBwd = build_layout(kShapeBwd, 2);

// ---- backward chain of the articulated NeRFMLP (training, model_autodecoder.py:168-239 under
// autograd), same conventions as kShapeBwd: the view branch, the bottleneck / density heads,
// the trunk, the enc columns of pts_linears.5 (the skip) and of pts_linears.0 (256 -> 63: the
// gradient w.r.t. pos_enc(x'), reduced in registers through pos_enc's backward to dL/dx'), the
// deformation head and the deformation MLP.  Latent columns carry no per-sample gradient (their
// codes' gradients come from the bias gradients, train_art.py).
enum {
  AB_RGB = 0, AB_V3, AB_V2, AB_V1, AB_V0, AB_BOTDEN, AB_P7, AB_P6, AB_P5, AB_P5E, AB_P4, AB_P3,
  AB_P2, AB_P1, AB_P0E, AB_DL, AB_D3, AB_D2, AB_D1, kNumLayersArtBwd
};

constexpr LayerShape kShapeArtBwd[kNumLayersArtBwd] = {
    {0, 1, 8, 0, 3, 128},       // rgb_layer^T: d hv3 (3 -> 128)
    {4, 0, 8, 128, 0, 128},     // views_linear.3^T: d hv2
    {4, 0, 8, 128, 0, 128},     // views_linear.2^T: d hv1
    {4, 0, 8, 128, 0, 128},     // views_linear.1^T: d hv0
    {4, 0, 16, 128, 0, 256},    // views_linear.0^T, bottleneck columns: d bottleneck
    {8, 1, 16, 256, 1, 256},    // [bottleneck^T | density^T]: d h7
    {8, 0, 16, 256, 0, 256},    // pts_linears.7^T: d h6
    {8, 0, 16, 256, 0, 256},    // pts_linears.6^T: d h5
    {8, 0, 16, 256, 0, 256},    // pts_linears.5^T, h4 columns: d h4
    {8, 0, 4, 256, 0, 63},      // pts_linears.5^T, enc columns: d enc (skip)
    {8, 0, 16, 256, 0, 256},    // pts_linears.4^T: d h3
    {8, 0, 16, 256, 0, 256},    // pts_linears.3^T: d h2
    {8, 0, 16, 256, 0, 256},    // pts_linears.2^T: d h1
    {8, 0, 16, 256, 0, 256},    // pts_linears.1^T: d h0
    {8, 0, 4, 256, 0, 63},      // pts_linears.0^T, enc columns: d enc
    {0, 1, 8, 0, 3, 128},       // deformation_layer^T: d hd3 (3 -> 128)
    {4, 0, 8, 128, 0, 128},     // deformations_linear.3^T: d hd2
    {4, 0, 8, 128, 0, 128},     // deformations_linear.2^T: d hd1
    {4, 0, 8, 128, 0, 128},     // deformations_linear.1^T: d hd0
};
constexpr auto kLayoutArtBwd = build_layout(kShapeArtBwd, 2);

// compile-time description of one fp16x3 network: its built layout and stream geometry
template <const auto& LAYOUT, bool ZERO_BIAS = false>
struct NetH {
  static constexpr bool kZeroBias = ZERO_BIAS;  // the backward chains: an all-zero bias table
  static constexpr int kNumLayers = LAYOUT.kNumLayers;
  static constexpr int kBlocks = LAYOUT.blocks;                  // blocks carrying weights
  static constexpr int kStreamBlocks = round_up(kBlocks, 64);    // padded to whole LDS chunks
  static constexpr int kBiasFloats = LAYOUT.bias_floats;
  static constexpr size_t kStreamBytes = (size_t)kStreamBlocks * 1024;
  static constexpr size_t kPackedBytes = kStreamBytes + (size_t)kBiasFloats * 4 + kStatusBytes;
  static constexpr LayerDesc layer(int i) { return LAYOUT.layer[i]; }
  static constexpr bool ok() {
    for (const LayerDesc& d : LAYOUT.layer) {
      if (d.blk0 % 2) return false;  // a (hi, lo) pair never straddles a chunk
      if (!(d.u == 1 || d.u % 2 == 0)) return false;
      if (d.len_a > 32 * d.ka || d.len_b > 32 * d.kb || d.out_real > 16 * d.u) return false;
    }
    return kStreamBlocks % 64 == 0;
  }
};

using NetVanillaH = NetH<kLayoutH>;
using NetVanillaFoldH = NetH<kLayoutHFold>;
using NetArtH = NetH<kLayoutArt>;
using NetBwdH = NetH<kLayoutBwd, true>;
using NetArtBwdH = NetH<kLayoutArtBwd, true>;
static_assert(NetVanillaH::ok() && NetVanillaFoldH::ok() && NetArtH::ok() && NetBwdH::ok() &&
                  NetArtBwdH::ok(),
              "inconsistent fp16x3 layout");

// A pass that stops after the first N_LAYERS layers of Net reads a PREFIX of Net's packed stream
// in place: same buffer, same bias table and status word (behind the WHOLE stream's
// Net::kStreamBytes, not behind the prefix).  The prefix ends where layer N_LAYERS of the parent
// begins and rounds up to whole ring chunks of CHUNK blocks (the ring then copies some of that
// layer's blocks, never read); only the prefix's rows of the bias table are staged in LDS.
template <typename Net, int N_LAYERS, int CHUNK>
struct Prefix {
  static_assert(N_LAYERS >= 1 && N_LAYERS < Net::kNumLayers, "a proper prefix");
  static constexpr bool kZeroBias = Net::kZeroBias;
  static constexpr int kNumLayers = N_LAYERS;
  static constexpr int kChunk = CHUNK;  // 1-KB blocks per ring chunk of the pass
  static constexpr int kBlocks = Net::layer(N_LAYERS).blk0;
  static constexpr int kStreamBlocks = round_up(kBlocks, CHUNK);
  static constexpr int kBiasFloats = Net::layer(N_LAYERS).bias0;
  static constexpr LayerDesc layer(int i) { return Net::layer(i); }
  static_assert(kBiasFloats % 4 == 0, "the bias rows are staged as float4");
  // whole ring chunks inside the parent's buffer, the last one holding a block the pass reads:
  // every copy the ring issues is waited for (DmaPipe::begin) before the kernel ends
  static_assert(kStreamBlocks % CHUNK == 0 && kStreamBlocks <= Net::kStreamBlocks &&
                    (kBlocks - 1) / CHUNK == kStreamBlocks / CHUNK - 1,
                "prefix stream: whole ring chunks, none unused");
};
// The density-only render pass (aon_mlp_fwd_sigma: the coarse level of a render that keeps only
// the fine level's colour -- its rgb reaches nothing, its sigma the fine level's samples): the
// trunk and the density head of the render stream, in ring chunks of 32 (mlp_f16x3.hip).
using NetVanillaSigmaH = Prefix<NetVanillaFoldH, LDEN + 1, 32>;
// The deformation-only pass (aon_mlp_art_fwd_deform: x' and the deformation of a render's
// samples, without the trunk and the view branch): deformations_linear.0-3 and
// deformation_layer, in ring chunks of 16 (mlp_art_deform.hip's ring).
using NetArtDeformH = Prefix<NetArtH, A_DOUT + 1, 16>;
// The articulated density-only pass (aon_mlp_art_fwd_sigma: the coarse level of a render that
// keeps only the fine level, and density queries at points): everything through density_layer
// -- the deformation MLP and head, the trunk, the density head -- without bottleneck_layer and
// the view branch, in the chain ring's chunks of 32 (mlp_art_sigma.hip).  Two workgroups per CU
// are out of reach at any chunk size: the 256-wide trunk's two Frag<8> fragments alone are 128
// VGPRs, so a SIMD holds 2 waves = one 8-wave workgroup per CU, and at 16-block chunks the ring
// (48 KB), the prefix's bias rows (10 KB) and the enc stash (32 KB) would still pass 80 KB.
using NetArtSigmaH = Prefix<NetArtH, A_DEN + 1, 32>;

// pack-kernel arguments: per-layer torch parameter pointers + the layout table by value
struct PackArgs {
  const float* w[kNumLayers];
  const float* b[kNumLayers];
  LayerDesc layers[kNumLayers];
};

// fp16x3 pack: any NetH; ldw = row stride of each torch weight ([out][ldw], the real columns
// first: latent columns past len_a + len_b are folded into the biases)
constexpr int kMaxLayersH = 24;
// tr: the layer applies W^T (the backward chain): stream element (row o, column c) = w[c][o].
// w2 / ldw2: segment B from its own matrix (else columns len_a.. of w); b may be null (0).
struct PackArgsH {
  const float* w[kMaxLayersH];
  const float* w2[kMaxLayersH];
  const float* b[kMaxLayersH];
  int ldw[kMaxLayersH];
  int ldw2[kMaxLayersH];
  int tr[kMaxLayersH];
  LayerDesc layers[kMaxLayersH];
  int n_layers, stream_blocks, bias_floats;
  // 0: fp16x3; 1: bf16 (compact, StreamMap mode 1); 2: mixed -- fp16x3 pairs for the blocks
  // [mx_lo, mx_hi) of the fp16x3 numbering, compact bf16 for the rest (the articulated bf16
  // training mode keeps the deformation MLP in fp16x3, StreamMap mode 2)
  int bf16;
  int mx_lo, mx_hi;
  // compact blocks (modes 1, 2) hold fp16(w 2^6) instead of bf16(w), range-guarded like the
  // fp16x3 hi blocks, and their layers' biases are at activation scale (FragPipe W1)
  int f16w;
  // fold_w set: layer fold_layer's segment A is the product of its own first fold_k columns
  // with the linear layer in front of it (fold_w [fold_k][len_a], fold_b [fold_k]; no
  // activation between them): stream element (o, col) = fp32(sum_j w[o][j] fold_w[j][col]),
  // bias fp32(b[o] + sum_j w[o][j] fold_b[j]), both summed in fp64 in index order -- then
  // scaled, split and range-tested like any other weight (the render stream's view layer)
  const float* fold_w;
  const float* fold_b;
  int fold_layer, fold_k;
};

// Where the weight stream holds fp16x3 block b (even b: the hi block of a (hi, lo) pair, b + 1
// its lo block) -- shared by k_pack_h and FragPipe.  mode 0: fp16x3, in place; 1: bf16 compact,
// only hi blocks, block 2c at c; 2: mixed, [lo, hi) kept as fp16x3 pairs (lo even), every other
// hi block compact bf16, all in consumption order (the ring's chunk starts are still met: a
// chunk boundary is even, so it falls on a pair's hi block or a bf16 block).
struct StreamMap {
  int mode, lo, hi;
  __host__ __device__ constexpr bool f16(int b) const {
    return mode == 0 || (mode == 2 && b >= lo && b < hi);
  }
  __host__ __device__ constexpr int map(int b) const {
    return mode == 0 ? b
         : mode == 1 ? b >> 1
         : b < lo    ? b >> 1
         : b < hi    ? (lo >> 1) + b - lo
                     : (lo >> 1) + (hi - lo) + ((b - hi) >> 1);
  }
  // stream block m -> its fp16x3 block
  __host__ __device__ constexpr int unmap(int m) const {
    return mode == 0 ? m
         : mode == 1 ? 2 * m
         : m < (lo >> 1)            ? 2 * m
         : m < (lo >> 1) + hi - lo  ? lo + m - (lo >> 1)
                                    : hi + 2 * (m - (lo >> 1) - (hi - lo));
  }
  // stream blocks carrying the `blocks` weight blocks of the fp16x3 numbering
  __host__ __device__ constexpr int used(int blocks) const {
    return mode == 0 ? blocks : mode == 1 ? blocks / 2 : (lo >> 1) + (hi - lo) + ((blocks - hi) >> 1);
  }
};
// the articulated forward's mixed stream: the deformation MLP (the blocks before pts_linears.0)
// fp16x3 -- x' feeds pos_enc's sin(2^9 x'), where bf16's 2^-9 would cost whole radians -- the
// trunk, heads and view branch compact bf16
constexpr StreamMap kArtMix{2, 0, NetArtH::layer(A_P0).blk0};
constexpr int kArtMixUsed = kArtMix.used(NetArtH::kBlocks);
constexpr int kArtMixStream = round_up(kArtMixUsed, 64);
// the articulated bf16 mode's view-branch stream (train_art.BF16_VIEW): the deformation MLP, the
// trunk, density and bottleneck fp16x3 (the blocks before views_linear.0 -- everything the
// deformation gradients are ill-conditioned in), views_linear.0-3 and rgb_layer compact bf16
constexpr StreamMap kArtMixV{2, 0, NetArtH::layer(A_V0).blk0};
constexpr int kArtMixVUsed = kArtMixV.used(NetArtH::kBlocks);
constexpr int kArtMixVStream = round_up(kArtMixVUsed, 64);
static_assert(kArtMixVStream <= NetArtH::kStreamBlocks, "the mixed streams fit the fp16x3 buffer");
// round trip: the last pair, the last pair before and the first two hi blocks past the fp16x3 range
constexpr bool stream_map_ok(StreamMap m, int blocks) {
  return m.unmap(m.map(blocks - 2)) == blocks - 2 && m.unmap(m.map(m.hi - 2)) == m.hi - 2 &&
         m.map(m.hi) == m.hi && m.map(m.hi + 2) == m.hi + 1;
}
static_assert(stream_map_ok(kArtMix, NetArtH::kBlocks) && stream_map_ok(kArtMixV, NetArtH::kBlocks),
              "stream map round trip");

// ---- the packed sizes are visible through the C ABI (aon_*_packed_bytes; packs live in
// checkpointed buffers): the derived totals, pinned.  The only literals of this file.
template <typename Net>
constexpr bool net_is(int blocks, int stream_blocks, int bias_floats) {
  return Net::kBlocks == blocks && Net::kStreamBlocks == stream_blocks &&
         Net::kBiasFloats == bias_floats;
}
static_assert(kBlocks == 2344 && kStreamBlocks == 2368 && kBiasFloats == 2464, "fp32 stream");
static_assert(net_is<NetVanillaH>(2344, 2368, 2464), "unfolded vanilla stream");
static_assert(net_is<NetVanillaFoldH>(2088, 2112, 2208), "folded render stream");
static_assert(net_is<NetVanillaSigmaH>(1936, 1952, 2064), "density-only prefix");
static_assert(net_is<NetArtH>(2752, 2752, 3376), "articulated stream");
static_assert(net_is<NetBwdH>(2224, 2240, 2432), "vanilla backward stream");
static_assert(net_is<NetArtBwdH>(2752, 2752, 3456), "articulated backward stream");
static_assert(net_is<NetArtDeformH>(216, 224, 528), "deformation-only prefix");
static_assert(net_is<NetArtSigmaH>(2152, 2176, 2592), "articulated density-only prefix");
static_assert(kArtMix.hi == 216 && kArtMixUsed == 1484 && kArtMixStream == 1536,
              "mixed articulated stream");
static_assert(kArtMixV.hi == 2408 && kArtMixVUsed == 2580 && kArtMixVStream == 2624,
              "view-branch mixed articulated stream");

// Training forward of the fused kernel (launch_f16x3_train): every hidden activation goes to
// HBM for the backward, as the layer-by-layer path keeps them: h (8, N, 256) post-ReLU
// pts_linears outputs, bot (N, 256), hv (N, 128) post-ReLU views_linear.0; raw_sigma gets
// + noise[row] when noise is set (model.py:183-184).
struct TrainStore {
  float* h;
  float* bot;
  float* hv;
  const float* noise;
  uint2* masks;  // (9, N, 4) ReLU' bits of h0..h7, hv (RowStoreBits)
  __bf16* enc_bf;  // bf16 mode, optional: pos_enc(x) tiled (N, 128), columns 63.. zero
};

// activations the articulated training forward keeps (aon_mlp_art_fwd_train)
struct TrainStoreArt {
  float* hd;    // (4, N, 128) deformation layers
  float* h;     // (8, N, 256) pts_linears
  float* bot;   // (N, 256)
  float* hv;    // (4, N, 128) views_linear
  float* enc;   // (N, 63) pos_enc(x'); enc[:, :3] = x'
  float* xyz;   // (N, 3) the sample points (deformation input)
  const float* noise;  // (N) added to raw_sigma, or nullptr
  uint2* masks;        // (16, N, 4) ReLU' bits of hd0..3, h0..7, hv0..3 (RowStoreBits)
  __bf16* enc_bf;      // bf16 modes, optional: pos_enc(x') tiled (N, 128), columns 63.. zero
};

// ---- workgroup geometry of the chain kernels
#ifndef AON_WAVES_H
#define AON_WAVES_H 8  // waves per workgroup at 16 samples per wave (2 waves per SIMD either way)
#endif

// BF: the bf16 training kernels -- at 32 samples per wave (NCOL = 2) they keep 8 waves (2 per
// SIMD): bf16 activations carry no lo part, so a wave's input and output fragments take 64 + 64
// VGPRs where fp16x3 needs 256 (its NCOL = 2 runs 4 waves, one per SIMD)
#ifndef AON_BF_NCOL_FWD
#define AON_BF_NCOL_FWD 1  // samples per wave / 16 of the bf16 training forward
#endif
#ifndef AON_BF_NCOL_BWD
#define AON_BF_NCOL_BWD 2  // ... and of the bf16 backward chain
#endif
constexpr int kBfNcolFwd = AON_BF_NCOL_FWD, kBfNcolBwd = AON_BF_NCOL_BWD;
template <int NCOL, bool BF = false>
struct GeomH {
  static constexpr int kWaves = (NCOL == 1 || BF) ? AON_WAVES_H : 4;
  static constexpr int kThreads = 64 * kWaves;
  static constexpr int kRowsPerWave = 16 * NCOL;
  static constexpr int kRowsPerBlock = kRowsPerWave * kWaves;
  static constexpr int kWavesPerSimd = kWaves / 4;  // __launch_bounds__' occupancy request
};

// ---- host side of every chain launch (G: a geometry with kRowsPerBlock; Net: the stream read)
template <typename G>
inline int64_t chain_grid(int64_t N) { return (N + G::kRowsPerBlock - 1) / G::kRowsPerBlock; }
// the "too many rows" guard: the grid fits 31 bits.  The forwards test GeomH<1> whatever they
// launch; static_assert(kRowsOkCovers<G>) beside a launch says that its grid is no larger.
template <typename G = GeomH<1>>
inline bool rows_ok(int64_t N) { return chain_grid<G>(N) < (1ll << 31); }
template <typename G>
constexpr bool kRowsOkCovers = G::kRowsPerBlock >= GeomH<1>::kRowsPerBlock;
// the bias table (and, behind it, the status word) of a packed Net stream
template <typename Net>
inline const float* stream_bias(const void* packed) {
  return reinterpret_cast<const float*>(static_cast<const char*>(packed) + Net::kStreamBytes);
}
// the shape / activation / alignment checks of the render and training forwards, reported as fn
inline int check_fwd_args(const char* fn, const void* packed, const void* raw, int64_t B, int S,
                          int act) {
  AON_REQUIRE_AS(fn, B >= 0 && S >= 1, "bad shape");
  AON_REQUIRE_AS(fn, act >= AON_ACT_NONE && act <= AON_ACT_ARTIC, "bad activation");
  AON_REQUIRE_AS(fn, aligned16(packed) && aligned16(raw), "packed / raw must be 16-byte aligned");
  return 0;
}
// a Net's layer table, stream geometry and default row strides (len_a + len_b) into pack args
template <typename Net>
inline void fill_net(PackArgsH& a) {
  for (int i = 0; i < Net::kNumLayers; ++i) {
    a.layers[i] = Net::layer(i);
    a.ldw[i] = Net::layer(i).len_a + Net::layer(i).len_b;
  }
  a.n_layers = Net::kNumLayers;
  a.stream_blocks = Net::kStreamBlocks;
  a.bias_floats = Net::kBiasFloats;
}

// fp16x3 path (mlp_f16x3.hip)
// fold: the render stream (NetVanillaFoldH), else the training forwards' (NetVanillaH)
int pack_f16x3(const PackArgs& a, void* packed, hipStream_t stream, bool bf16 = false,
               bool fold = false);
int pack_h(PackArgsH a, void* packed, hipStream_t stream);
// *out = bits of max |x| over n floats (memset + k_absmax, mlp_bwd.hip): the backward chains'
// per-call gradient scale
int absmax(const float* x, int64_t n, uint32_t* out, hipStream_t stream);
// the render forward (folded stream): kernel MODE 0, or MODE 1 (encoded); 16 ncol samples per wave
int launch_f16x3_render(bool encoded, int ncol, const void* packed, const float* a0,
                        const float* a1, const float* a2, const float* a3, int64_t B, int S,
                        int act, float* raw, hipStream_t stream);
// the training forward (MODE 0 inputs, AON_ACT_NONE, activations kept in ts): fp16x3 or bf16
int launch_f16x3_train(bool bf16, const TrainStore& ts, const void* packed, const float* rays_o,
                       const float* rays_d, const float* viewdirs, const float* t, int64_t B,
                       int S, float* raw, hipStream_t stream);
// the render stream's two-pass entry points (16 samples per wave): the density-only pass
// (NetVanillaSigmaH: raw rows {0, 0, 0, sigma}) and the conditioned forward (kernel MODE 2: the
// view encodings from a (B, 27) table) -- column 3 / all of launch_f16x3_render's MODE 0, bit
// for bit
int launch_f16x3_sigma(const void* packed, const float* rays_o, const float* rays_d,
                       const float* t, int64_t B, int S, int act, float* raw, hipStream_t stream);
int launch_f16x3_cond(const void* packed, const float* rays_o, const float* rays_d,
                      const float* cond, const float* t, int64_t B, int S, int act, float* raw,
                      hipStream_t stream);

}  // namespace mlp
}  // namespace aon
