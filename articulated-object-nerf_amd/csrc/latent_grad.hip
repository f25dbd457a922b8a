// Latent-code gradients of one articulated level with the MLPs frozen (the reference's
// --is_optimize fit, utils.get_optimizer_latent_opt): a layer z = W [x; l] + b with the code l on
// every row has dL/dl = (sum_rows dZ)^T W[:, latent columns], so the three code gradients need
// only the column sums of four of the backward chain's gradient tensors (aon_mlp_art_bwd[_bf16]:
// dzv[0], dz[5], dz[0], dzd[0] -- 768 of its 3,328 columns) and four weight slices; no
// activation is read and no weight gradient is formed.
//
//   stage (a)  k_tiled_colsum: column sums over the rows of the four tiled tensors.  A fixed
//              number of workgroups (a function of N only) each take a contiguous range of 16-row
//              blocks; every lane owns the same 16-byte pieces of every block -- one tile row and
//              4 (fp32) / 8 (bf16) columns each, 48 fp32 accumulators -- so the loop is loads and
//              adds only; the 16 lanes that share a column set (one per tile row) are combined by a
//              fixed xor butterfly and each workgroup leaves 768 partial sums in `work`.  The rows
//              N .. NR-1 of the last block are never loaded (the chain does not write them).
//   stage (b)  k_partial_sum: the partials summed per column in a fixed order;
//              k_latent_products: dl[c] = sum_o s[o] W[o, col0 + c], one fmaf chain per eighth of
//              the rows, the eighths and then the shape code's three terms added in a fixed order.
// No atomics, no allocation, no synchronisation: bit-identical from run to run, capturable.
#include "aon_common.hpp"
#include "param_check.hpp"

namespace aon {
namespace latent {

constexpr int kThreads = 256;
constexpr int kMaxGroups = 1024;  // stage (a) workgroups: four per CU keep every CU streaming
// the 768 summed columns: views_linear.0 (128), pts_linears.5 (256), pts_linears.0 (256),
// deformations_linear.0 (128)
constexpr int kWidth[4] = {128, 256, 256, 128};
constexpr int kOff[4] = {0, 128, 384, 640};
constexpr int kCols = 768;
// first latent column of each weight and the latent widths (model_autodecoder.py:186-235)
constexpr int kColApp = 256 + 27, kColShape5 = 256 + 63, kColShape0 = 63, kColShapeD = 3;
constexpr int kColArt = 3 + 128, kNShape = 128, kNApp = 128, kNArt = 32;

inline int groups_for(int64_t N) {
  const int64_t nblk = (N + 15) / 16;
  return (int)(nblk < kMaxGroups ? nblk : kMaxGroups);
}

struct SumArgs {
  const void* t[4];  // dzv[0], dz[5], dz[0], dzd[0], tiled (include/aonerf.h "Kept tensors")
  int64_t N;
  float* part;  // (gridDim.x, 768)
};

// One tensor's share of a 16-row block: W / 16 tiles of 16 x 16, i.e. 16 W / E pieces of 16
// bytes (E = 4 fp32 or 8 bf16 elements of one tile row); thread t takes pieces t, t + 256, ...
// -- all in tile row (t % (256 / E)) / (16 / E), so one row test covers the thread's loads.
template <bool BF, int W>
__device__ __forceinline__ void add_block(const void* base, int64_t blk, int tid,
                                          float (*acc)[BF ? 8 : 4]) {
  constexpr int E = BF ? 8 : 4;
  constexpr int K = W / (16 * E);  // pieces per thread
  const f4* p = static_cast<const f4*>(base) + blk * (16 * W / E) + tid;
  f4 v[K];
#pragma unroll
  for (int j = 0; j < K; ++j) v[j] = p[kThreads * j];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if constexpr (BF) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {  // a bf16 is the high half of its fp32
        const uint32_t u = __float_as_uint(v[j][e]);
        acc[j][2 * e] = __fadd_rn(acc[j][2 * e], __uint_as_float(u << 16));
        acc[j][2 * e + 1] = __fadd_rn(acc[j][2 * e + 1], __uint_as_float(u & 0xffff0000u));
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[j][e] = __fadd_rn(acc[j][e], v[j][e]);
    }
  }
}

template <bool BF>
__global__ __launch_bounds__(kThreads) void k_tiled_colsum(SumArgs a) {
  constexpr int E = BF ? 8 : 4;
  constexpr int kPieces = 256 / E;    // 16-byte pieces per 16 x 16 tile
  constexpr int kPerRow = 16 / E;     // ... per tile row
  constexpr int kSlots = kCols / (16 * E);  // pieces per thread and block: 12 fp32, 6 bf16
  const int tid = threadIdx.x;
  const int row = (tid % kPieces) / kPerRow;  // the tile row of every piece of this thread
  const int64_t nblk = (a.N + 15) / 16;
  const int64_t b0 = nblk * blockIdx.x / gridDim.x, b1 = nblk * (blockIdx.x + 1) / gridDim.x;

  float acc[kSlots][E];
#pragma unroll
  for (int j = 0; j < kSlots; ++j)
#pragma unroll
    for (int e = 0; e < E; ++e) acc[j][e] = 0.f;
  // slots of the four tensors in acc: widths / (16 E)
  constexpr int s1 = 128 / (16 * E), s2 = s1 + 256 / (16 * E), s3 = s2 + 256 / (16 * E);
  for (int64_t blk = b0; blk < b1; ++blk) {
    if (16 * blk + row < a.N) {  // false only in the padding rows of the last block
      add_block<BF, 128>(a.t[0], blk, tid, acc);
      add_block<BF, 256>(a.t[1], blk, tid, acc + s1);
      add_block<BF, 256>(a.t[2], blk, tid, acc + s2);
      add_block<BF, 128>(a.t[3], blk, tid, acc + s3);
    }
  }
  // the 16 lanes holding one column set differ in the tile row: lane bits kPerRow .. 8 kPerRow
#pragma unroll
  for (int m = kPerRow; m < 16 * kPerRow; m <<= 1)
#pragma unroll
    for (int j = 0; j < kSlots; ++j)
#pragma unroll
      for (int e = 0; e < E; ++e) acc[j][e] = __fadd_rn(acc[j][e], __shfl_xor(acc[j][e], m, 64));
  if (row != 0) return;
  float* out = a.part + (int64_t)blockIdx.x * kCols;
  const int slot0[5] = {0, s1, s2, s3, kSlots};
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int j = slot0[t]; j < slot0[t + 1]; ++j) {
      const int q = tid + kThreads * (j - slot0[t]);  // the piece: tile q / kPieces, columns below
      float* o = out + kOff[t] + 16 * (q / kPieces) + E * (q % kPerRow);
#pragma unroll
      for (int e = 0; e < E; e += 4)
        *reinterpret_cast<f4*>(o + e) = f4{acc[j][e], acc[j][e + 1], acc[j][e + 2], acc[j][e + 3]};
    }
}

// colsum[c] = sum_g part[g][c]: 32 columns per workgroup, eight lanes per column each summing
// g = s, s + 8, ... in order, the eight combined in order.
__global__ __launch_bounds__(kThreads) void k_partial_sum(const float* __restrict__ part, int G,
                                                          float* __restrict__ colsum) {
  __shared__ float red[8][32];
  const int s = threadIdx.x >> 5, c = threadIdx.x & 31, col = 32 * blockIdx.x + c;
  float v = 0.f;
#pragma unroll 8
  for (int g = s; g < G; g += 8) v = __fadd_rn(v, part[(int64_t)g * kCols + col]);
  red[s][c] = v;
  __syncthreads();
  if (s == 0) {
    float t = red[0][c];
#pragma unroll
    for (int i = 1; i < 8; ++i) t = __fadd_rn(t, red[i][c]);
    colsum[col] = t;
  }
}

struct Term {
  const float* w;  // the weight, [out][in]
  int64_t ld;      // its row stride
  int sum0, n_out, col0;  // first column sum, rows, first latent column
};
struct ProdArgs {
  Term term[5];  // the shape code's three (pts_linears.5, .0, deformations_linear.0), app, art
  const float* colsum;
  float *dshape, *dapp, *dart;
};

// sum_o s[o] W[o, col]: this thread's eighth of the rows as one fmaf chain
__device__ __forceinline__ float term_slice(const Term& t, const float* __restrict__ colsum, int s,
                                            int c) {
  const int n = t.n_out / 8;
  const float* sv = colsum + t.sum0 + s * n;
  const float* w = t.w + (int64_t)(s * n) * t.ld + t.col0 + c;
  float v = 0.f;
  for (int o = 0; o < n; ++o) v = fmaf(sv[o], w[(int64_t)o * t.ld], v);
  return v;
}

// workgroups 0..3: dshape columns 32 b .. 32 b + 31; 4..7: dapp; 8: dart
__global__ __launch_bounds__(kThreads) void k_latent_products(ProdArgs a) {
  __shared__ float red[3][8][32];
  const int s = threadIdx.x >> 5, c = threadIdx.x & 31, b = blockIdx.x;
  const int nterm = b < 4 ? 3 : 1, first = b < 4 ? 0 : (b < 8 ? 3 : 4);
  const int col = 32 * (b & 3) + c;
  for (int t = 0; t < nterm; ++t) red[t][s][c] = term_slice(a.term[first + t], a.colsum, s, col);
  __syncthreads();
  if (s != 0) return;
  float v = 0.f;
  for (int t = 0; t < nterm; ++t) {
    float x = red[t][0][c];
#pragma unroll
    for (int i = 1; i < 8; ++i) x = __fadd_rn(x, red[t][i][c]);
    v = t == 0 ? x : __fadd_rn(v, x);  // pts_linears.5, + pts_linears.0, + deformations_linear.0
  }
  (b < 4 ? a.dshape : (b < 8 ? a.dapp : a.dart))[col] = v;
}

}  // namespace latent
}  // namespace aon

using namespace aon;
using namespace aon::latent;

extern "C" size_t aon_art_latent_grad_workspace_bytes(int64_t N) {
  if (N <= 0 || N > ((int64_t)1 << 40)) return 0;
  return ((size_t)groups_for(N) + 1) * kCols * sizeof(float);
}

extern "C" int aon_art_latent_grad(const aon_mlp_art_params* prm, const void* dzv0,
                                   const void* dz5, const void* dz0, const void* dzd0, int bf16,
                                   int64_t N, float* dshape, float* dapp, float* dart, void* work,
                                   aon_stream_t stream) {
  AON_REQUIRE(prm && dzv0 && dz5 && dz0 && dzd0 && dshape && dapp && dart && work, "null pointer");
  AON_REQUIRE(N > 0, "bad shape: N must be positive");
  AON_REQUIRE(N <= ((int64_t)1 << 40), "too many rows");
  AON_REQUIRE(bf16 == 0 || bf16 == 1, "bf16: 0 fp32 gradient tensors, 1 bf16");
  AON_REQUIRE(aligned16(dzv0) && aligned16(dz5) && aligned16(dz0) && aligned16(dzd0) &&
                  aligned16(work),
              "gradient tensors and work must be 16-byte aligned");
  if (mlp::check_mlp_art_params(prm, __func__)) return -1;
  // the four latent-carrying layers with their latent columns present (the packs need only the
  // per-sample ones)
  const int layer[4] = {mlp::kArtView0, mlp::kArtPts5, mlp::kArtPts0, mlp::kArtDef0};
  const int need[4] = {kColApp + kNApp, kColShape5 + kNShape, kColShape0 + kNShape,
                       kColArt + kNArt};
  const float* w[4] = {prm->views_w[0], prm->pts_w[5], prm->pts_w[0], prm->def_w[0]};
  for (int i = 0; i < 4; ++i) {
    const mlp::ArtShape& s = mlp::kArtShape[layer[i]];
    if (prm->w_cols[layer[i]] < need[i]) {
      set_error(std::string(__func__) + ": " + s.name + ": weight " +
                std::to_string(prm->w_rows[layer[i]]) + " x " +
                std::to_string(prm->w_cols[layer[i]]) + " has no latent columns; expected " +
                std::to_string(s.out) + " x >= " + std::to_string(need[i]));
      return -1;
    }
    AON_REQUIRE(w[i], std::string(s.name) + ": null layer weight");
  }
  const int64_t ld[4] = {prm->w_cols[layer[0]], prm->w_cols[layer[1]], prm->w_cols[layer[2]],
                         prm->w_cols[layer[3]]};

  hipStream_t st = (hipStream_t)stream;
  const int G = groups_for(N);
  float* part = static_cast<float*>(work);
  float* colsum = part + (size_t)G * kCols;
  const SumArgs sa{{dzv0, dz5, dz0, dzd0}, N, part};
  if (bf16)
    hipLaunchKernelGGL(k_tiled_colsum<true>, G, kThreads, 0, st, sa);
  else
    hipLaunchKernelGGL(k_tiled_colsum<false>, G, kThreads, 0, st, sa);
  hipLaunchKernelGGL(k_partial_sum, kCols / 32, kThreads, 0, st, part, G, colsum);
  ProdArgs pa{};
  pa.term[0] = Term{w[1], ld[1], kOff[1], kWidth[1], kColShape5};
  pa.term[1] = Term{w[2], ld[2], kOff[2], kWidth[2], kColShape0};
  pa.term[2] = Term{w[3], ld[3], kOff[3], kWidth[3], kColShapeD};
  pa.term[3] = Term{w[0], ld[0], kOff[0], kWidth[0], kColApp};
  pa.term[4] = Term{w[3], ld[3], kOff[3], kWidth[3], kColArt};
  pa.colsum = colsum;
  pa.dshape = dshape;
  pa.dapp = dapp;
  pa.dart = dart;
  hipLaunchKernelGGL(k_latent_products, 9, kThreads, 0, st, pa);
  return launch_status(__func__);
}
