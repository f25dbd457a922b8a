// k_gemm_small_f32 / k_gemm_small_batch: tiny exact-fp32 products.
#pragma once
#include "gemm_params.hpp"

namespace aon {
namespace gemm {

// ---- tiny fp32 products (the latent-code terms of the articulated step: per-call folded biases
// b + W_l l, dW_l = db l^T, dl = db^T W_l -- M x N <= 64K outputs, K <= 1024): the 128 x 128
// tiled kernel spent 17-27 us on each (a K pass one or two k-tiles deep, PF register sets and
// split epilogues for a few hundred outputs).  Exact fp32 fmaf (the operand scales are powers
// of two and cancel exactly).  K <= 16: one thread per output, k in order; longer K: one wave
// per output, lane l summing k = l, l + 64, ... in order, then a fixed xor tree (deterministic).
__device__ __forceinline__ void small_store(const Params& p, int64_t m, int64_t n, float v) {
  float* c = p.C + m * p.ldc + n;
  if (p.accumulate) v = __fadd_rn(*c, v);
  if (p.bias) v = __fadd_rn(v, p.bias[n]);
  *c = v;
}
__global__ __launch_bounds__(256) void k_gemm_small_f32(Params p, int a_kc, int b_kc) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= p.M * p.N) return;
  const int64_t m = e / p.N, n = e - m * p.N;
  float v = 0.f;
  for (int64_t k = 0; k < p.K; ++k) {
    const float a = a_kc ? p.A[m * p.lda + k] : p.A[k * p.lda + m];
    const float b = b_kc ? p.B[n * p.ldb + k] : p.B[k * p.ldb + n];
    v = fmaf(a, b, v);
  }
  small_store(p, m, n, v);
}
__global__ __launch_bounds__(256) void k_gemm_small_f32_wave(Params p, int a_kc, int b_kc) {
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // one wave per output
  const int lane = threadIdx.x & 63;
  if (e >= p.M * p.N) return;  // wave-uniform
  const int64_t m = e / p.N, n = e - m * p.N;
  float v = 0.f;
  for (int64_t k = lane; k < p.K; k += 64) {
    const float a = a_kc ? p.A[m * p.lda + k] : p.A[k * p.lda + m];
    const float b = b_kc ? p.B[n * p.ldb + k] : p.B[k * p.ldb + n];
    v = fmaf(a, b, v);
  }
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) v = __fadd_rn(v, __shfl_xor(v, sh, 64));
  if (lane == 0) small_store(p, m, n, v);
}

// aon_gemm_small_batch: up to AON_GEMM_SMALL_BATCH_MAX exact-fp32 tiny products in ONE launch,
// each computed exactly as its own aon_gemm launch would (k_gemm_small_f32 for K <= 16: one
// lane per output, a k-ordered fma chain; k_gemm_small_f32_wave above: one wave per output,
// lane-strided chains and the same xor butterfly), and products writing the same C applied in
// argument order in registers (c = accumulate ? c + v : v; + bias), so the result is bit for bit
// that of the launches in sequence.  Work units: 64 outputs (lane kind) or 1 output (wave kind)
// per wave; group g (one C) owns units unit0[g] .. unit0[g + 1] - 1.
struct SmallItem {
  const float* A;
  const float* B;
  float* C;
  const float* bias;
  int64_t lda, ldb, ldc, M, N, K;
  int a_kc, b_kc, accumulate, pad;
};
struct SmallBatch {
  SmallItem it[AON_GEMM_SMALL_BATCH_MAX];   // in group order (a group's items consecutive)
  int gfirst[AON_GEMM_SMALL_BATCH_MAX + 1];  // first item of each group
  int64_t unit0[AON_GEMM_SMALL_BATCH_MAX + 1];
  int ngroups;
};
static_assert(sizeof(SmallBatch) <= 4096, "aon_gemm_small_batch's table must fit the kernel arguments");

__device__ __forceinline__ float small_dot_lane(const SmallItem& f, int64_t m, int64_t n) {
  float v = 0.f;
  for (int64_t k = 0; k < f.K; ++k) {
    const float a = f.a_kc ? f.A[m * f.lda + k] : f.A[k * f.lda + m];
    const float b = f.b_kc ? f.B[n * f.ldb + k] : f.B[k * f.ldb + n];
    v = fmaf(a, b, v);
  }
  return v;
}
__device__ __forceinline__ float small_dot_wave(const SmallItem& f, int64_t m, int64_t n, int lane) {
  float v = 0.f;
  for (int64_t k = lane; k < f.K; k += 64) {
    const float a = f.a_kc ? f.A[m * f.lda + k] : f.A[k * f.lda + m];
    const float b = f.b_kc ? f.B[n * f.ldb + k] : f.B[k * f.ldb + n];
    v = fmaf(a, b, v);
  }
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) v = __fadd_rn(v, __shfl_xor(v, sh, 64));
  return v;
}
__global__ __launch_bounds__(256) void k_gemm_small_batch(SmallBatch sb) {
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
  const int lane = threadIdx.x & 63;
  if (u >= sb.unit0[sb.ngroups]) return;
  int g = 0;
  while (g + 1 < sb.ngroups && u >= sb.unit0[g + 1]) ++g;
  const SmallItem& f0 = sb.it[sb.gfirst[g]];
  const bool wave = f0.K > 16;
  const int64_t e = wave ? u - sb.unit0[g] : (u - sb.unit0[g]) * 64 + lane;
  if (e >= f0.M * f0.N) return;
  const int64_t m = e / f0.N, n = e - m * f0.N;
  float* c = f0.C + m * f0.ldc + n;
  float acc = f0.accumulate ? *c : 0.f;
  for (int i = sb.gfirst[g]; i < sb.gfirst[g + 1]; ++i) {
    const SmallItem& f = sb.it[i];
    const float v = wave ? small_dot_wave(f, m, n, lane) : small_dot_lane(f, m, n);
    acc = f.accumulate ? __fadd_rn(acc, v) : v;
    if (f.bias) acc = __fadd_rn(acc, f.bias[n]);
  }
  if (!wave || lane == 0) *c = acc;
}

}  // namespace gemm
}  // namespace aon
