// k_gemm_skinny_bf16 / k_gemm_segsum_bf16: the streaming weight gradients (M <= 4 rows; a
// per-ray B operand), bf16-staged or exact fp32.
#pragma once
#include "gemm_params.hpp"

namespace aon {
namespace gemm {

// ---- bf16 weight gradients with M <= 4 rows (the rgb / density heads: dW = d raw^T X with
// X = hv3 / h7): a 128 x 128 MFMA tile would run 97% empty and the km kernel's transposing
// loads held these at ~130 us for 0.2-0.4 GB, so the product streams instead.  Thread (r, cg):
// row phase r of every 16-row block of its K chunk, columns 8 cg .. 8 cg + 7 (one 16-B run of B:
// a wave reads two whole 16 x 16 tiles, 1 KB contiguous, of the tiled layout); A's M values of
// the row rounded to bf16 as the MFMA paths stage them, products exact in fp32, fp32 sums in
// row order, then a fixed xor tree over the 16 row phases; one chunk's partial per workgroup
// (k_gemm_reduce sums the chunks in z order: deterministic).  TB = float: the parity mode's
// heads (fp32 A and B, the fused forward's tiled fp32 h7 / hv3), the same kernel with nothing
// rounded -- fp32 products and sums, more accurate than the fp16x3 split it replaces for M <= 4
// (a 128 x 128 tile 97-99% empty, 0.23-0.28 ms per fine-level head).
constexpr int kSkinnyRows = 16;
#ifndef AON_GEMM_SKINNY_SK
#define AON_GEMM_SKINNY_SK 4  // rows in flight per thread of the skinny kernel; 1: A/B
#endif
#ifndef AON_GEMM_SEGSUM_SK
#define AON_GEMM_SEGSUM_SK 16  // ... of the segment-sum kernel (one workgroup of 4 waves per CU;
                               // 16 vs 4: 60.4 vs 62.4 us fine level, neutral)
#endif
#ifndef AON_GEMM_SKINNY_SK2
#define AON_GEMM_SKINNY_SK2 4  // ... of the skinny kernel on B of <= 128 columns (A/B knob: 8 measured
                               // 81 -> 108 us on the fine level's rgb head, profiles/r04/final2)
#endif
template <int M, typename TA, bool BT, int SK = AON_GEMM_SKINNY_SK, typename TB = __bf16>
__global__ __launch_bounds__(512) void k_gemm_skinny_bf16(Params p) {
  constexpr bool RND = std::is_same<TB, __bf16>::value;  // the bf16 mode: A staged as bf16
  constexpr int NB = sizeof(TB) / 2;                      // 16-B loads per 8-column run of B
  const int tid = threadIdx.x, r = tid & 15, cg = tid >> 4;
  const int64_t n0 = 8 * (int64_t)cg;
  const int64_t kbeg = (int64_t)blockIdx.x * p.kchunk;
  const int64_t kend = kbeg + p.kchunk < p.K ? kbeg + p.kchunk : p.K;
  const TA* A = reinterpret_cast<const TA*>(p.A);
  const TB* B = reinterpret_cast<const TB*>(p.B);
  float acc[M][8], rs[M], cs[8];  // cs: B's column sums (c_trans)
  const bool ct = p.c_trans != 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) cs[j] = 0.f;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    rs[m] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[m][j] = 0.f;
  }
  auto boff = [&](int64_t k) {
    return BT ? (k & ~int64_t(15)) * p.ldb + 256 * (n0 >> 4) + 16 * (k & 15) + (n0 & 15)
              : k * p.ldb + n0;
  };
  auto row = [&](const uint4 (&bv)[NB], const TA* ar) {
    float b[8];
    if (RND) {
      const uint32_t bw[4] = {bv[0].x, bv[0].y, bv[0].z, bv[0].w};
#pragma unroll
      for (int j = 0; j < 8; ++j) b[j] = __uint_as_float((j & 1) ? (bw[j >> 1] & 0xffff0000u) : (bw[j >> 1] << 16));
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint4& q = bv[(j >> 2) & (NB - 1)];
        const uint32_t w = (j & 3) == 0 ? q.x : (j & 3) == 1 ? q.y : (j & 3) == 2 ? q.z : q.w;
        b[j] = __uint_as_float(w);
      }
    }
    if (ct) {
#pragma unroll
      for (int j = 0; j < 8; ++j) cs[j] = __fadd_rn(cs[j], b[j]);
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float a = RND ? static_cast<float>(static_cast<__bf16>(static_cast<float>(ar[m])))
                          : static_cast<float>(ar[m]);
      rs[m] = __fadd_rn(rs[m], a);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[m][j] = fmaf(a, b[j], acc[m][j]);  // bf16: a * b exact
    }
  };
  auto load_b = [&](int64_t kk, uint4 (&bv)[NB]) {
    const uint4* src = reinterpret_cast<const uint4*>(B + boff(kk));
#pragma unroll
    for (int h = 0; h < NB; ++h) bv[h] = src[h];
  };
  // SK rows per thread in flight: their loads are issued before the first is consumed (one
  // dependent load per row left this kernel latency-bound: rgb's 0.27 GB at ~2.2 TB/s); the
  // rows are still summed in k order (bit-identical); SK2 for B of <= 128 columns (half the waves
  // per workgroup)
  int64_t k = kbeg + r;
  for (; k + (SK - 1) * kSkinnyRows < kend; k += SK * kSkinnyRows) {
    uint4 bv[SK][NB];
    TA av[SK][M];
#pragma unroll
    for (int u = 0; u < SK; ++u) {
      load_b(k + u * kSkinnyRows, bv[u]);
#pragma unroll
      for (int m = 0; m < M; ++m) av[u][m] = A[(k + u * kSkinnyRows) * p.lda + m];
    }
#pragma unroll
    for (int u = 0; u < SK; ++u) row(bv[u], av[u]);
  }
  for (; k < kend; k += kSkinnyRows) {
    TA av[M];
#pragma unroll
    for (int m = 0; m < M; ++m) av[m] = A[k * p.lda + m];
    uint4 bv[NB];
    load_b(k, bv);
    row(bv, av);
  }
  // the 16 row phases of a column group are lanes 16 q .. 16 q + 15 of one wave
#pragma unroll
  for (int sh = 1; sh < 16; sh <<= 1) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      rs[m] = __fadd_rn(rs[m], __shfl_xor(rs[m], sh, 64));
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[m][j] = __fadd_rn(acc[m][j], __shfl_xor(acc[m][j], sh, 64));
    }
    if (ct) {
#pragma unroll
      for (int j = 0; j < 8; ++j) cs[j] = __fadd_rn(cs[j], __shfl_xor(cs[j], sh, 64));
    }
  }
  if (r != 0) return;
  const bool split = p.zsplit > 1;
  const int z = blockIdx.x;
  if (ct && p.rowsum) {  // B's column sums: columns n0 .. n0 + 7 of this column group
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (split) p.rowsum_part[(int64_t)z * p.N + n0 + j] = cs[j];
      else p.rowsum[n0 + j] = cs[j];
    }
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    if (!ct && p.rowsum && cg == 0) {
      if (split) p.rowsum_part[(int64_t)z * p.M + m] = rs[m];
      else p.rowsum[m] = rs[m];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = acc[m][j];
      if (split) {
        p.part[((int64_t)z * p.M + m) * p.N + n0 + j] = v;
        continue;
      }
      float* c = p.C + (ct ? (n0 + j) * p.ldc + m : m * p.ldc + n0 + j);
      if (p.accumulate) v = __fadd_rn(*c, v);
      *c = v;
    }
  }
}

// ---- bf16 weight gradient against a per-ray operand: C = A^T B with row k of B at k / rdiv
// (views_linear.0's enc_dir columns: B = pos_enc(viewdirs), one row per ray, rdiv = S).  Every
// B row meets rdiv consecutive A rows, so C = sum_ray (sum_{s<rdiv} A[ray rdiv + s]) B[ray]:
// thread (ray, cg) sums its ray's rdiv rows of columns 8 cg .. 8 cg + 7 in row order (A's
// values rounded to bf16 as staged; fp32 sums, kept unrounded), the workgroup's RB rays' sums go
// to LDS, and their outer products with bf16(B) make the chunk's partial of C (and of A's
// column sums).  The km kernel read A with the reduction-major transposing loads at ~130 us for
// the fine level's 0.2 GB; this reads A once, in 16-B runs, and does 1/rdiv of the products.
// RND = false: the parity mode's (fp32 A and B), nothing rounded -- fp32 sums and products.
template <typename TA, typename TB, bool AT, bool RND = true>
__global__ __launch_bounds__(256) void k_gemm_segsum_bf16(Params p) {
  __shared__ float seg[256 * 8];  // [RB rays][M]: RB * M = 8 * 256
  const int M = static_cast<int>(p.M), N = static_cast<int>(p.N);
  const int cgs = M / 8, rb = 256 / cgs;
  const int tid = threadIdx.x, cg = tid % cgs, rl = tid / cgs;
  const int64_t rdiv = p.b_rdiv;
  const int64_t ray = (int64_t)blockIdx.x * rb + rl;
  const TA* A = reinterpret_cast<const TA*>(p.A);
  const int64_t n0 = 8 * (int64_t)cg;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int64_t kb = ray * rdiv, ke = kb + rdiv < p.K ? kb + rdiv : p.K;
  auto aoff = [&](int64_t k) {
    return AT ? (k & ~int64_t(15)) * p.lda + 256 * (n0 >> 4) + 16 * (k & 15) + (n0 & 15)
              : k * p.lda + n0;
  };
  auto add_row = [&](int64_t o, const uint4& w) {
    float v[8];
    if (std::is_same<TA, __bf16>::value) {
      const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = __uint_as_float((j & 1) ? (ww[j >> 1] & 0xffff0000u) : (ww[j >> 1] << 16));
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = static_cast<float>(static_cast<__bf16>(static_cast<float>(A[o + j])));
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = __fadd_rn(acc[j], v[j]);
  };
  // fp32 A unrounded: one row's 8 columns as two 16-B loads
  auto add_row32 = [&](const uint4 (&w)[2]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint4& q = w[j >> 2];
      const uint32_t u = (j & 3) == 0 ? q.x : (j & 3) == 1 ? q.y : (j & 3) == 2 ? q.z : q.w;
      acc[j] = __fadd_rn(acc[j], __uint_as_float(u));
    }
  };
  int64_t k = kb;
  if (!RND && std::is_same<TA, float>::value) {
    constexpr int SK = AON_GEMM_SEGSUM_SK / 2;
    for (; k + SK - 1 < ke; k += SK) {
      uint4 w[SK][2];
#pragma unroll
      for (int u = 0; u < SK; ++u) {
        const uint4* src = reinterpret_cast<const uint4*>(A + aoff(k + u));
        w[u][0] = src[0];
        w[u][1] = src[1];
      }
#pragma unroll
      for (int u = 0; u < SK; ++u) add_row32(w[u]);
    }
    for (; k < ke; ++k) {
      const uint4* src = reinterpret_cast<const uint4*>(A + aoff(k));
      const uint4 w[2] = {src[0], src[1]};
      add_row32(w);
    }
  }
  if (std::is_same<TA, __bf16>::value) {
    // AON_GEMM_SEGSUM_SK rows' 16-B loads in flight per thread before the first is summed (one
    // dependent load per row left one workgroup of 4 waves per CU latency-bound; 4 rows still
    // held the fine level's 0.2 GB at ~3.3 TB/s); the rows are still summed in k order
    // (bit-identical)
    constexpr int SK = AON_GEMM_SEGSUM_SK;
    for (; k + SK - 1 < ke; k += SK) {
      uint4 w[SK];
#pragma unroll
      for (int u = 0; u < SK; ++u) w[u] = *reinterpret_cast<const uint4*>(A + aoff(k + u));
#pragma unroll
      for (int u = 0; u < SK; ++u) add_row(0, w[u]);
    }
  }
  for (; k < ke; ++k) {
    const int64_t o = aoff(k);
    uint4 w = {0u, 0u, 0u, 0u};
    if (std::is_same<TA, __bf16>::value) w = *reinterpret_cast<const uint4*>(A + o);
    add_row(o, w);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) seg[rl * M + n0 + j] = acc[j];
  __syncthreads();
  const int64_t ray0 = (int64_t)blockIdx.x * rb;
  const int64_t nray = (p.K + rdiv - 1) / rdiv;
  const int nr = static_cast<int>(nray - ray0 < rb ? nray - ray0 : rb);
  const TB* Bm = reinterpret_cast<const TB*>(p.B);
  const bool split = p.zsplit > 1;
  const int z = blockIdx.x;
  for (int e = tid; e < M * N + M; e += 256) {
    float v = 0.f;
    if (e < M * N) {
      const int m = e / N, n = e - m * N;
      for (int q = 0; q < nr; ++q) {
        const float b = RND ? static_cast<float>(static_cast<__bf16>(static_cast<float>(Bm[(ray0 + q) * p.ldb + n])))
                            : static_cast<float>(Bm[(ray0 + q) * p.ldb + n]);
        v = fmaf(seg[q * M + m], b, v);
      }
      if (split) {
        p.part[((int64_t)z * M + m) * N + n] = v;
        continue;
      }
      float* c = p.C + m * p.ldc + n;
      if (p.accumulate) v = __fadd_rn(*c, v);
      *c = v;
    } else if (p.rowsum) {
      const int m = e - M * N;
      for (int q = 0; q < nr; ++q) v = __fadd_rn(v, seg[q * M + m]);
      if (split) p.rowsum_part[(int64_t)z * M + m] = v;
      else p.rowsum[m] = v;
    }
  }
}

}  // namespace gemm
}  // namespace aon
