// What every aon_gemm kernel shares (gemm_f16x3.hip): the kernel arguments, the XCD-aware tile
// and K-chunk order, the fp16 hi / lo split, and the deterministic split-K reduce kernels.
#pragma once
#include "aon_common.hpp"

#include <type_traits>

namespace aon {
namespace gemm {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

constexpr int BM = 128, BN = 128, BK = 32, THREADS = 256;
constexpr int ROWH = BK + 8;                 // halves per LDS row: 80 B, 16-B aligned
constexpr int PLANE = BM * ROWH;             // halves per plane (BM == BN)
constexpr int STAGE = 4 * PLANE;             // A hi, A lo, B hi, B lo
constexpr float kLo = 2048.0f;               // lo planes carry (x - hi) * 2^11
constexpr float kInvLo = 1.0f / 2048.0f;

struct Params {
  int64_t M, N, K;
  const float* A;
  int64_t lda;
  const float* A2;  // a_kc only: columns [K1, K) from A2[(m / a2_rdiv) * lda2 + (k - K1)]
  int64_t lda2, K1, a2_rdiv;
  const float* B;
  int64_t ldb, b_rdiv;  // !b_kc: element (k, n) = B[(k / b_rdiv) * ldb + n]
  float* C;
  int64_t ldc;
  const float* bias;  // per column n
  const float* mask;  // v *= (mask[m * ldm + n] > 0)
  int64_t ldm;
  int relu, accumulate;
  float sa, sb, inv_s;  // operand prescales (powers of two); result * inv_s
  const uint32_t* sa_bits;  // optional: A's scale also times grad_scale(*sa_bits) (per call)
  int64_t kchunk;       // K rows per blockIdx.z (split-K); == K when not split
  float* part;          // split-K partials [z][M][N] (unscaled epilogue-free sums * inv_s)
  float* rowsum;        // !a_kc: rowsum[m] = sum_k A(m, k) (bias gradient of a dW product)
  float* rowsum_part;   // split-K partials [z][M]
  int tiles_m, tiles_n, gm;  // XCD-aware tile order over a 1-D grid.x (see tile_of)
  int zsplit;                // split-K: number of K chunks (1 = not split), see split_of
  int tblocks;               // blocks of one K chunk's tile grid (tile_of's ids, with padding)
  int a_tiled, b_tiled;      // reduction-major operand in the fused training kernels' 16-row
                             // tiled layout (mlp_f16x3_core.hpp act_base; rdiv 1)
  int64_t nstore;            // columns of C written: n < nstore (a zero-padded B, bf16 mode)
  int c_trans;               // C[n * ldc + m]; rowsum = column sums of B (skinny path, aon_gemm_args)
};

// start of the 4-element run (k, row .. row + 3) of a reduction-major operand (row % 4 == 0):
// row-major storage row k / rdiv, or the 16-row tiled layout of the fused training kernels
__device__ __forceinline__ int64_t km_off(int64_t k, int64_t row, int64_t ld, int64_t rdiv,
                                          bool tiled) {
  if (tiled) return (k & ~int64_t(15)) * ld + 256 * (row >> 4) + 16 * (k & 15) + (row & 15);
  // 32-bit division (aon_gemm checks K < 2^32): a 64-bit one is a ~40-instruction sequence
  const int64_t kr = rdiv == 1 ? k : (int64_t)((uint32_t)k / (uint32_t)rdiv);
  return kr * ld + row;
}

// Workgroups are dispatched round-robin over the 8 XCDs (block L -> XCD L mod 8), each with
// its own L2.  The tiles (m, 0..tiles_n-1) that share one A row-block are given block ids
// gm apart -- with gm = 8 the same XCD, dispatched together -- so the A tile is fetched from
// HBM once per XCD: group g of gm m-tiles x tiles_n n-tiles, L = gm tiles_n g + gm n + (m mod gm).
// Grids of fewer than 8 m-tiles (weight gradients) use gm = tiles_m: no padding blocks, which
// would otherwise pile the real tiles onto a few XCDs (measured: 3.5x slower).
// Split-K grids: the tile count T is small (a weight gradient is 2 x 2 tiles) and every K chunk
// is read by the T tiles that share it.  Chunk z's tiles get block ids 8 apart (L = 8 q + x,
// z = 8 (q / T) + x, tile = q mod T): one XCD, dispatched together, so each chunk of both
// operands comes from HBM once and the other tiles hit that XCD's L2.
__device__ __forceinline__ bool split_of(const Params& p, int& tile, int& z) {
  if (p.zsplit <= 1) {
    tile = blockIdx.x;
    z = 0;
    return true;
  }
  const int T = p.tblocks;
  const int L = blockIdx.x, x = L & 7, q = L >> 3;
  z = 8 * (q / T) + x;
  tile = q - (q / T) * T;
  return z < p.zsplit;
}

__device__ __forceinline__ bool tile_of(const Params& p, int L, int& tm, int& tn) {
  const int gsz = p.gm * p.tiles_n;
  const int g = L / gsz, r = L - g * gsz;
  tn = r / p.gm;
  tm = p.gm * g + (r - tn * p.gm);
  return tm < p.tiles_m;
}

__device__ __forceinline__ f4 mfma16(h8 a, h8 b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// 4 consecutive k values of one row -> hi / lo halves
__device__ __forceinline__ void split4(f4 v, float s, h4& hi, h4& lo) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float x = v[j] * s;  // power-of-two prescale: exact
    const _Float16 h = static_cast<_Float16>(x);
    hi[j] = h;
    lo[j] = static_cast<_Float16>(__fmul_rn(__fsub_rn(x, static_cast<float>(h)), kLo));
  }
}

// split-K: C = epilogue(sum_z part[z]) in z order (deterministic); rowsum likewise.  The loads
// of 8 consecutive z are issued before their (in-order) adds: a thread walks up to 256 partials
// spaced M*N apart, and one load at a time left this kernel latency-bound (~50 us at any size).
__device__ __forceinline__ float sum_z(const float* src, int64_t stride, int splits) {
  float v = src[0];
  int z = 1;
  for (; z + 8 <= splits; z += 8) {
    float t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = src[(int64_t)(z + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) v = __fadd_rn(v, t[u]);
  }
  for (; z < splits; ++z) v = __fadd_rn(v, src[(int64_t)z * stride]);
  return v;
}

// Four lanes per output: lane q sums the partials of the q-th quarter of the chunks in z order,
// then the quarters combine as (q0 + q1) + (q2 + q3) -- a fixed order (deterministic), a quarter
// of the dependent load rounds per thread and 4x the threads of a one-lane-per-output reduce
// (whose 256 workgroups of sequential partial loads took ~11 us per weight gradient).
__device__ __forceinline__ float sum_z4(const float* src, int64_t stride, int splits, int q) {
  const int zq = (splits + 3) / 4;
  const int z0 = q * zq, z1 = z0 + zq < splits ? z0 + zq : splits;
  float v = 0.f;
  if (z0 < z1) v = sum_z(src + (int64_t)z0 * stride, stride, z1 - z0);
  const float w = __shfl_xor(v, 1, 64);  // lanes 4e + q: q0 + q1 and q2 + q3
  const float pair = (q & 1) ? __fadd_rn(w, v) : __fadd_rn(v, w);
  const float other = __shfl_xor(pair, 2, 64);
  return (q & 2) ? __fadd_rn(other, pair) : __fadd_rn(pair, other);
}

// Sixteen lanes per output (the small products -- heads, segment sums -- whose few hundred
// outputs each sum 256-512 chunks: at 4 lanes they ran on ~6 workgroups in 16 dependent load
// rounds, ~8-11 us): lane q sums the q-th sixteenth in z order, then a fixed xor tree combines
// them, lower lane first at every level (deterministic).
__device__ __forceinline__ float sum_z16(const float* src, int64_t stride, int splits, int q) {
  const int zq = (splits + 15) / 16;
  const int z0 = q * zq, z1 = z0 + zq < splits ? z0 + zq : splits;
  float v = 0.f;
  if (z0 < z1) v = sum_z(src + (int64_t)z0 * stride, stride, z1 - z0);
#pragma unroll
  for (int b = 1; b < 16; b <<= 1) {
    const float w = __shfl_xor(v, b, 64);
    v = (q & b) ? __fadd_rn(w, v) : __fadd_rn(v, w);
  }
  return v;
}

template <int L>
__device__ __forceinline__ void reduce_body(const Params& p, int splits) {
  static_assert(L == 4 || L == 16, "lanes per output");
  constexpr int kSh = L == 4 ? 2 : 4;
  const int64_t total = p.M * p.N;
  const int64_t nrs = p.c_trans ? p.N : p.M;  // rowsum entries: row sums of A, or B's column sums
  const int64_t extra = p.rowsum ? nrs : 0;   // they ride along as e >= total
  const int q = threadIdx.x & (L - 1);
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  auto sum = [&](const float* src, int64_t stride) {
    return L == 4 ? sum_z4(src, stride, splits, q) : sum_z16(src, stride, splits, q);
  };
  // every lane of a wave takes part in the shuffles: the loop bound is per group of L lanes and
  // the grid stride a multiple of L, so a group's lanes run the same iterations
  for (int64_t eL = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; (eL >> kSh) < total + extra;
       eL += nthreads) {
    const int64_t e = eL >> kSh;
    if (e >= total) {
      const int64_t m = e - total;
      const float v = sum(p.rowsum_part + m, nrs);
      if (q == 0) p.rowsum[m] = v;
      continue;
    }
    const int64_t m = e / p.N, n = e - m * p.N;
    float v = sum(p.part + e, total);
    if (q != 0 || n >= p.nstore) continue;
    float* c = p.C + (p.c_trans ? n * p.ldc + m : m * p.ldc + n);
    if (p.accumulate) v = __fadd_rn(*c, v);
    if (p.bias) v = __fadd_rn(v, p.bias[n]);
    if (p.relu) v = fmaxf(v, 0.0f);
    if (p.mask && !(p.mask[m * p.ldm + n] > 0.0f)) v = 0.0f;
    *c = v;
  }
}

template <int L>
__global__ void k_gemm_reduce(Params p, int splits) { reduce_body<L>(p, splits); }

// aon_gemm_batch: up to AON_GEMM_BATCH_MAX products in one launch, selected by a wave-uniform
// index into the kernel-argument table
struct ParamsBatch {
  Params p[AON_GEMM_BATCH_MAX];
  int count, zsplit;
  int tile0[AON_GEMM_BATCH_MAX + 1];  // 128 x 128-tile batch: first tile of each product
};

static_assert(sizeof(ParamsBatch) <= 4096, "aon_gemm_batch's table must fit the kernel arguments");

// the batch's split-K reduce: grid.y = product
__global__ void k_gemm_reduce_batch(ParamsBatch pb) { reduce_body<4>(pb.p[blockIdx.y], pb.zsplit); }

}  // namespace gemm
}  // namespace aon
