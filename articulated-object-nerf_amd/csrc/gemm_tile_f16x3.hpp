// k_gemm_f16x3: the generic 128 x 128-tile fp16x3 product (any operand layout, every epilogue)
// and its weight-gradient batch (gemm_f16x3.hip has the numerics and the routing).
#pragma once
#include "gemm_params.hpp"

namespace aon {
namespace gemm {

#ifndef AON_GEMM_PF
#define AON_GEMM_PF 1
#endif
constexpr int PF = AON_GEMM_PF;              // k-tiles loaded ahead (register sets)

// ---- tile loaders: 128 rows x 32 k of one operand into 4 f4 registers per thread -------------
// KC (k-contiguous rows): thread t -> rows (t >> 3) + 32 i, k quad 4 (t & 7).
// KM (k-major storage, rows contiguous): thread t -> rows 16 (t >> 5) + 4 (t & 3) + 0..3, k quad
//     4 ((t >> 2) & 7); register i holds k = kq + i for those 4 rows (transposed when stored).
//     Four lanes cover 64 contiguous bytes of a k row; the stores of a 32-lane half hit rows
//     4 apart in two 16-row groups at 8 k offsets: at most 2-way bank conflicts (80-B rows).
template <bool KC, bool VEC>
struct TileLoad {
  f4 r[4];

  // rows/k outside [0,R) x [k0, kend) read as 0.  KC: k >= K1 from p2 (row / rdiv);
  // KM: storage row k / rdiv.
  __device__ __forceinline__ void load(const float* p, int64_t ld, const float* p2, int64_t ld2,
                                       int64_t K1, int64_t rdiv, int64_t row0, int64_t R,
                                       int64_t k0, int64_t kend, int tid, bool tiled = false) {
    if (KC) {
      const int kq = 4 * (tid & 7);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = row0 + (tid >> 3) + 32 * i;
        const int64_t k = k0 + kq;
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < R) {
          if (VEC && k + 3 < kend && k + 3 < K1) {
            v = *reinterpret_cast<const f4*>(p + row * ld + k);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int64_t kk = k + j;
              if (kk < kend) v[j] = kk < K1 ? p[row * ld + kk] : p2[(row / rdiv) * ld2 + (kk - K1)];
            }
          }
        }
        r[i] = v;
      }
    } else {
      const int kq = 4 * ((tid >> 2) & 7), rq = 16 * (tid >> 5) + 4 * (tid & 3);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t k = k0 + kq + i;
        const int64_t row = row0 + rq;
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (k < kend) {
          const float* src = p + km_off(k, row, ld, rdiv, tiled);
          if (VEC && row + 3 < R) {
            v = *reinterpret_cast<const f4*>(src);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (row + j < R) v[j] = src[j];
          }
        }
        r[i] = v;
      }
    }
  }

  // KM only: per-row sums of this thread's 4 k values (rows rq..rq+3), in k order
  __device__ __forceinline__ void add_rows(float (&rs)[4]) const {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      rs[j] = __fadd_rn(rs[j], __fadd_rn(__fadd_rn(__fadd_rn(r[0][j], r[1][j]), r[2][j]), r[3][j]));
  }

  // split and store into the [row][k] hi / lo planes
  __device__ __forceinline__ void store(_Float16* hi, _Float16* lo, float s, int tid) const {
    if (KC) {
      const int kq = 4 * (tid & 7);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = (tid >> 3) + 32 * i;
        h4 h, l;
        split4(r[i], s, h, l);
        *reinterpret_cast<h4*>(hi + row * ROWH + kq) = h;
        *reinterpret_cast<h4*>(lo + row * ROWH + kq) = l;
      }
    } else {
      const int kq = 4 * ((tid >> 2) & 7), rq = 16 * (tid >> 5) + 4 * (tid & 3);
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // row rq + j: k = kq .. kq + 3 from r[0..3][j]
        const f4 v = {r[0][j], r[1][j], r[2][j], r[3][j]};
        h4 h, l;
        split4(v, s, h, l);
        *reinterpret_cast<h4*>(hi + (rq + j) * ROWH + kq) = h;
        *reinterpret_cast<h4*>(lo + (rq + j) * ROWH + kq) = l;
      }
    }
  }
};

template <bool AKC, bool BKC, bool VA, bool VB>
__device__ __forceinline__ void f16x3_body(const Params& p, int tm, int tn, int z, _Float16* smem) {
  // A's prescale: a constant, or per call from the gradient's max |x| (exact powers of two)
  float sa = p.sa, inv_s = p.inv_s;
  if (p.sa_bits) {
    const float gs = grad_scale(*p.sa_bits);
    sa = __fmul_rn(sa, gs);
    inv_s = __fdiv_rn(inv_s, gs);
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
  const int64_t kbeg = (int64_t)z * p.kchunk;
  const int64_t kend = kbeg + p.kchunk < p.K ? kbeg + p.kchunk : p.K;
  const int nk = static_cast<int>((kend - kbeg + BK - 1) / BK);

  // PF register sets: tile kt + 1 waits in one while later tiles' loads fly into the others
  TileLoad<AKC, VA> ta[PF];
  TileLoad<BKC, VB> tb[PF];
  f4 acc_h[4][4], acc_x[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc_h[i][j] = f4{0.f, 0.f, 0.f, 0.f};
      acc_x[i][j] = f4{0.f, 0.f, 0.f, 0.f};
    }

  auto load = [&](int kt, auto set) {
    constexpr int S = decltype(set)::value;
    const int64_t k0 = kbeg + (int64_t)kt * BK;
    ta[S].load(p.A, p.lda, p.A2, p.lda2, p.K1, p.a2_rdiv, m0, p.M, k0, kend, tid, p.a_tiled);
    tb[S].load(p.B, p.ldb, nullptr, 0, INT64_MAX, p.b_rdiv, n0, p.N, k0, kend, tid, p.b_tiled);
  };
  const bool want_rows = !AKC && p.rowsum && tn == 0;
  float rs[4] = {0.f, 0.f, 0.f, 0.f};
  // publish a landed register set to LDS stage `stage` (and add its rows to the row sums, in
  // k-tile order)
  auto store = [&](int stage, auto set) {
    constexpr int S = decltype(set)::value;
    if (!AKC && want_rows) ta[S].add_rows(rs);
    _Float16* s = smem + stage * STAGE;
    ta[S].store(s, s + PLANE, sa, tid);
    tb[S].store(s + 2 * PLANE, s + 3 * PLANE, p.sb, tid);
  };
  using Set0 = std::integral_constant<int, 0>;
  using Set1 = std::integral_constant<int, 1>;

  using SetN = std::integral_constant<int, PF - 1>;
  if (nk > 0) {
    load(0, Set0{});
    if (PF == 2 && nk > 1) load(1, SetN{});
    store(0, Set0{});
  }
  __syncthreads();
  const int g = lane >> 4, r16 = lane & 15;
  // step kt: tile kt is in LDS stage kt & 1 and tile kt + 1 in register set (kt + 1) % PF
  // (PF = 2: loaded last step; PF = 1: loaded now, under this step's MFMAs); tile kt + PF goes
  // into set kt % PF, free since tile kt was published
  auto step = [&](int kt, auto par) {
    constexpr int P = decltype(par)::value;
    using Cur = std::integral_constant<int, P % PF>;
    using Nxt = std::integral_constant<int, (P + 1) % PF>;
    if (kt + PF < nk) load(kt + PF, Cur{});  // global loads in flight under PF steps of MFMAs
    const _Float16* s = smem + P * STAGE;
    h8 bh[4], bl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = wn * 64 + 16 * j + r16;
      bh[j] = *reinterpret_cast<const h8*>(s + 2 * PLANE + row * ROWH + 8 * g);
      bl[j] = *reinterpret_cast<const h8*>(s + 3 * PLANE + row * ROWH + 8 * g);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = wm * 64 + 16 * i + r16;
      const h8 ah = *reinterpret_cast<const h8*>(s + row * ROWH + 8 * g);
      const h8 al = *reinterpret_cast<const h8*>(s + PLANE + row * ROWH + 8 * g);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc_h[i][j] = mfma16(ah, bh[j], acc_h[i][j]);
        acc_x[i][j] = mfma16(ah, bl[j], acc_x[i][j]);
        acc_x[i][j] = mfma16(al, bh[j], acc_x[i][j]);
      }
    }
    if (kt + 1 < nk) store(1 - P, Nxt{});
    __syncthreads();
  };
  for (int kt = 0; kt < nk; kt += 2) {
    step(kt, Set0{});
    if (kt + 1 < nk) step(kt + 1, Set1{});
  }

  const bool split = p.zsplit > 1;
  if (!AKC && want_rows) {
    // combine the 8 k-quad lanes of every row in k order (LDS free after the last barrier)
    float* red = reinterpret_cast<float*>(smem);  // [8 k quads][128 rows]
    const int kqi = (tid >> 2) & 7, rq = 16 * (tid >> 5) + 4 * (tid & 3);
#pragma unroll
    for (int j = 0; j < 4; ++j) red[kqi * BM + rq + j] = rs[j];
    __syncthreads();
    if (tid < BM && m0 + tid < p.M) {
      float v = red[tid];
#pragma unroll
      for (int q = 1; q < 8; ++q) v = __fadd_rn(v, red[q * BM + tid]);
      if (split) p.rowsum_part[(int64_t)z * p.M + m0 + tid] = v;
      else p.rowsum[m0 + tid] = v;
    }
  }

  // ---- epilogue: D lane layout col = lane & 15, rows 4 (lane >> 4) + r
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t n = n0 + wn * 64 + 16 * j + r16;
      if (n >= p.N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + wm * 64 + 16 * i + 4 * g + r;
        if (m >= p.M) continue;
        float v = __fmul_rn(__fadd_rn(acc_h[i][j][r], __fmul_rn(acc_x[i][j][r], kInvLo)), inv_s);
        if (split) {
          p.part[((int64_t)z * p.M + m) * p.N + n] = v;
          continue;
        }
        if (n >= p.nstore) continue;
        float* c = p.C + m * p.ldc + n;
        if (p.accumulate) v = __fadd_rn(*c, v);
        if (p.bias) v = __fadd_rn(v, p.bias[n]);
        if (p.relu) v = fmaxf(v, 0.0f);
        if (p.mask && !(p.mask[m * p.ldm + n] > 0.0f)) v = 0.0f;
        *c = v;
      }
    }
}

template <bool AKC, bool BKC, bool VA, bool VB>
__global__ __launch_bounds__(THREADS, 2) void k_gemm_f16x3(Params p) {
  __shared__ __align__(16) _Float16 smem[2 * STAGE];  // 2 stages x (A hi, A lo, B hi, B lo)
  int tm, tn, tile, z;
  if (!split_of(p, tile, z)) return;      // padding block of the last chunk group
  if (!tile_of(p, tile, tm, tn)) return;  // padding block of the last XCD group (uniform exit)
  f16x3_body<AKC, BKC, VA, VB>(p, tm, tn, z, smem);
}

// fp16x3 weight gradients of one level (aon_gemm_batch): every product's 128 x 128 tiles, chunk z
// of all of them on one XCD (split_of's order), product b owning tiles tile0[b] .. tile0[b+1]-1
__global__ __launch_bounds__(THREADS, 2) void k_gemm_f16x3_batch(ParamsBatch pb) {
  __shared__ __align__(16) _Float16 smem[2 * STAGE];
  const int T = pb.tile0[pb.count], L = blockIdx.x, x = L & 7, q = L >> 3;
  const int z = 8 * (q / T) + x, t = q - (q / T) * T;
  if (z >= pb.zsplit) return;  // padding block of the last chunk group (uniform exit)
  int b = 0;
  while (b + 1 < pb.count && t >= pb.tile0[b + 1]) ++b;
  const Params& p = pb.p[b];
  const int lt = t - pb.tile0[b];
  f16x3_body<false, false, true, true>(p, lt % p.tiles_m, lt / p.tiles_m, z, smem);
}

}  // namespace gemm
}  // namespace aon
