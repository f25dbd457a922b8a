// k_gemm_f1 / k_gemm_f1h_batch: the parity mode's single-accumulator fp16x3 weight gradients.
#pragma once
#include "gemm_bf16_dma.hpp"

namespace aon {
namespace gemm {

// ---- fp16x3 weight gradients in one 256 x 256 tile per workgroup, ONE fp32 accumulator
// (aon_gemm_args.f16_single): the parity mode's 256 x 256 products dW = dY^T X of the fused
// training kernels' tiled fp32 tensors (pts_linears, bottleneck).  k_gemm_f16x3 runs them as a
// 2 x 2 grid of 128 x 128 tiles with two accumulators per tile (hi*hi and the 2^11-scaled cross
// terms), each operand byte staged into two workgroups; at 0.57 ms per fine-level product it was
// at 0.21 of the MFMA peak.  Here the operands carry the fused kernels' own scales -- A (dY) at
// the backward chain's per-call gradient scale, B (the activations) at 2^3 -- where the lo parts
// x s - fp16(x s) stay normal fp16 for |x s| >= 2^-3 (below it they keep an absolute 2^-25), so
// hi*hi + hi*lo + lo*hi share one accumulator (the fused MLP kernels' V2 numerics) and a wave's
// 64 x 128 sub-tile fits in 128 accumulator VGPRs.  The caller guarantees |x s| < 65504 for both
// operands (the chain and the forward range-guard their own splits at exactly these scales).
// 512 threads = 8 waves in 4 (m) x 2 (n), one workgroup per CU.  Per 32-row k-tile each thread
// loads two 32-B runs of each operand (a wave reads 2 KB contiguous of the tiled layout), splits
// them once into fp16 hi / lo and writes them (16-B stores) into [32 k][256 col] planes with
// the bf16 kernels' XOR swizzle, from which the MFMA fragments come by ds_read_b64_tr_b16; two
// LDS stages (128 KB), the split of tile kt + 1 and the loads of tile kt + 2 ride between the
// MFMAs of tile kt, one barrier per k-tile.  rowsum: A's fp32 values in row order per thread,
// then a fixed order over the 16 threads of a column run.
// Shapes (MW x NW, the operands' widths): 256 x 256 (pts_linears, bottleneck), 128 x 256
// (views_linear.0's bottleneck columns) and 256 x 64 (pts_linears.0's and the skip layer's
// pos_enc columns, B the tiled 64-column encodings of aon_cast_rays_tiled).  Waves in MW / 64
// (m) x 8 / (MW / 64) (n): every wave 64 rows x NW / WN columns.  An operand of width W < 128
// is staged into a 128-column image (the 128-column swizzle of the bf16 kernels).
template <int W>
struct F1Img {
  static constexpr int kCols = W < 128 ? 128 : W;  // image columns
  static constexpr int kPlane = BK * kCols * 2;    // bytes of one [32 k][kCols] fp16 plane
  static constexpr int kRuns = (4 * W + THREADS2 - 1) / THREADS2;  // 8-float runs per thread
  __device__ __forceinline__ static int off(int row, int ch) {
    return kCols == 256 ? tt_off2(row, ch) : tt_off(row, ch);
  }
  __device__ __forceinline__ static h8 frag(const char* plane, int c0, int lane) {
    return __builtin_bit_cast(h8, kCols == 256 ? tt_frag2(plane, c0, lane) : tt_frag(plane, c0, lane));
  }
};

// one thread's runs of a k-tile of a tiled fp32 operand of width W: run u = tid + 512 i (< 4 W)
// is floats 8 u .. 8 u + 7 of the k-tile's contiguous 32 W floats -- k row 16 (8 u / 16 W) +
// (8 u % 256) / 16, columns 16 ((8 u % 16 W) / 256) + (8 u % 16) .. + 7 (a wave reads 2 KB
// contiguous)
template <int W>
struct F1Run {
  static constexpr int NR = F1Img<W>::kRuns;
  f4 v[NR][2];
  __device__ __forceinline__ static bool valid(int tid, int i) {
    return (4 * W) % THREADS2 == 0 || tid + THREADS2 * i < 4 * W;  // every thread's: no branch
  }
  __device__ __forceinline__ static int row(int tid, int i) {
    const int u = tid + THREADS2 * i;
    return 16 * (8 * u / (16 * W)) + (8 * u % 256) / 16;
  }
  __device__ __forceinline__ static int col(int tid, int i) {
    const int u = tid + THREADS2 * i;
    return 16 * ((8 * u % (16 * W)) / 256) + (8 * u % 16);
  }
  __device__ __forceinline__ void load(const float* base, int64_t k0, int64_t kend, int tid, int i) {
    if (!valid(tid, i)) return;
    const f4* src = reinterpret_cast<const f4*>(base + k0 * W + 8 * (tid + THREADS2 * i));
    if (k0 + row(tid, i) < kend) {
      v[i][0] = src[0];
      v[i][1] = src[1];
    } else {
      v[i][0] = f4{0.f, 0.f, 0.f, 0.f};
      v[i][1] = f4{0.f, 0.f, 0.f, 0.f};
    }
  }
  // split run i at scale s into the hi / lo planes (16-B stores)
  __device__ __forceinline__ void store(char* hi, char* lo, float s, int tid, int i) const {
    if (!valid(tid, i)) return;
    h8 h, l;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = v[i][e >> 2][e & 3] * s;  // power of two: exact
      const _Float16 hh = static_cast<_Float16>(x);
      h[e] = hh;
      l[e] = static_cast<_Float16>(__fsub_rn(x, static_cast<float>(hh)));  // exact in fp32
    }
    const int off = F1Img<W>::off(row(tid, i), col(tid, i) >> 3);
    *reinterpret_cast<h8*>(hi + off) = h;
    *reinterpret_cast<h8*>(lo + off) = l;
  }
  // run i added to the thread's 8 running column sums, in row order
  __device__ __forceinline__ void add_rows(float (&rs)[8], int i) const {
#pragma unroll
    for (int e = 0; e < 8; ++e) rs[e] = __fadd_rn(rs[e], v[i][e >> 2][e & 3]);
  }
};


template <int MW, int NW>
struct F1Shape {
  static constexpr int kWM = MW / 64, kWN = 8 / kWM;  // waves in m / n
  static constexpr int kTJ = NW / kWN / 16;           // 16-column tiles per wave
  static constexpr int kStage = 2 * F1Img<MW>::kPlane + 2 * F1Img<NW>::kPlane;  // A hi, lo, B hi, lo
  static constexpr int kLds = 2 * kStage;
  // row sums: a thread's A runs share their columns when it has two (rows r, 16 + r: 16 slots
  // per column), else its one run is row 16 h + r (32 slots)
  static constexpr int kSlots = F1Img<MW>::kRuns == 2 ? 16 : 32;
  static_assert(MW % 64 == 0 && 8 % kWM == 0 && kTJ >= 1 && kSlots * MW * 4 <= kLds, "f1 shape");
};

// split-K by interleaved k-tiles (p.kchunk only sets the number of workgroups, p.zsplit)
template <int MW, int NW>
__device__ __forceinline__ void f1_body(const Params& p, int z, char* smem) {
  using S = F1Shape<MW, NW>;
  using IA = F1Img<MW>;
  using IB = F1Img<NW>;
  float sa = p.sa, inv_s = p.inv_s;
  if (p.sa_bits) {
    const float gs = grad_scale(*p.sa_bits);
    sa = __fmul_rn(sa, gs);
    inv_s = __fdiv_rn(inv_s, gs);
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / S::kWN, wn = wave % S::kWN;
  // workgroup z takes k-tiles z, z + zsplit, z + 2 zsplit, ... so a lone product's
  // workgroups read one contiguous run of zsplit k-tiles at a time (its contiguous chunks put
  // 256 read streams a fixed multiple of 3 MB apart: 0.51-0.54 ms against 0.45-0.48 interleaved;
  // a batch's 8 products x 32 chunks measured the other way round, 3.08-3.17 ms contiguous
  // against 3.57-3.71 interleaved, profiles/r05/f1_ab: f1h_body below)
  const int64_t ntiles = (p.K + BK - 1) / BK, zs = p.zsplit;
  const int64_t kend = p.K;
  const int64_t t0 = z;  // first k-tile; then every zs-th
  const int nk = z < ntiles ? static_cast<int>((ntiles - 1 - z) / zs + 1) : 0;
  const bool want_rows = p.rowsum != nullptr;
  float rs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  F1Run<MW> ra;
  F1Run<NW> rb;
  constexpr int NRUN = IA::kRuns > IB::kRuns ? IA::kRuns : IB::kRuns;
  auto load = [&](int kt, int i) {
    const int64_t k0 = (t0 + (int64_t)kt * zs) * BK;
    if (i < IA::kRuns) ra.load(p.A, k0, kend, tid, i);
    if (i < IB::kRuns) rb.load(p.B, k0, kend, tid, i);
  };
  // publish run i of both operands to stage st (and A's values to the row sums, in row order)
  auto publish = [&](int st, int i) {
    char* s = smem + st * S::kStage;
    if (i < IA::kRuns) {
      if (want_rows && ra.valid(tid, i)) ra.add_rows(rs, i);
      ra.store(s, s + IA::kPlane, sa, tid, i);
    }
    if (i < IB::kRuns) rb.store(s + 2 * IA::kPlane, s + 2 * IA::kPlane + IB::kPlane, p.sb, tid, i);
  };
  f4 acc[4][S::kTJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < S::kTJ; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
  if (nk > 0) {
#pragma unroll
    for (int i = 0; i < NRUN; ++i) load(0, i);
#pragma unroll
    for (int i = 0; i < NRUN; ++i) publish(0, i);
    if (nk > 1) {
#pragma unroll
      for (int i = 0; i < NRUN; ++i) load(1, i);
    }
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const char* s = smem + (kt & 1) * S::kStage;
    const char* sb = s + 2 * IA::kPlane;
    const bool more = kt + 1 < nk;
    h8 ah[4], al[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ah[i] = IA::frag(s, 8 * wm + 2 * i, lane);
      al[i] = IA::frag(s + IA::kPlane, 8 * wm + 2 * i, lane);
    }
#pragma unroll
    for (int j = 0; j < S::kTJ; ++j) {
      const int c0 = 2 * (S::kTJ * wn + j);
      const h8 bh = IB::frag(sb, c0, lane);
      const h8 bl = IB::frag(sb + IB::kPlane, c0, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[i][j] = mfma16(ah[i], bh, acc[i][j]);
        acc[i][j] = mfma16(ah[i], bl, acc[i][j]);
        acc[i][j] = mfma16(al[i], bh, acc[i][j]);
      }
      // tile kt + 1 (in registers) into the other stage between the MFMAs, each run's
      // registers refilled with tile kt + 2's at once: its loads fly under a whole k-tile
      if (more && j < NRUN) {
        publish((kt + 1) & 1, j);
        if (kt + 2 < nk) load(kt + 2, j);
      }
    }
    if (more && S::kTJ < NRUN) {  // narrow B: the runs left after the MFMAs
#pragma unroll
      for (int i = S::kTJ; i < NRUN; ++i) {
        publish((kt + 1) & 1, i);
        if (kt + 2 < nk) load(kt + 2, i);
      }
    }
    __syncthreads();
  }
  const bool split = p.zsplit > 1;
  if (want_rows) {
    // combine the slots of every column in slot order (LDS free after the last barrier)
    float* red = reinterpret_cast<float*>(smem);  // [kSlots][MW]
    if (ra.valid(tid, 0)) {
      const int slot = S::kSlots == 16 ? ra.row(tid, 0) : ra.row(tid, 0) & 31;
      const int c = ra.col(tid, 0);
#pragma unroll
      for (int e = 0; e < 8; ++e) red[slot * MW + c + e] = rs[e];
    }
    __syncthreads();
    if (tid < MW) {
      float v = red[tid];
#pragma unroll
      for (int q = 1; q < S::kSlots; ++q) v = __fadd_rn(v, red[q * MW + tid]);
      if (split) p.rowsum_part[(int64_t)z * p.M + tid] = v;
      else p.rowsum[tid] = v;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < S::kTJ; ++j) {
      const int64_t n = (NW / S::kWN) * wn + 16 * j + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t m = 64 * wm + 16 * i + 4 * (lane >> 4) + r;
        float v = __fmul_rn(acc[i][j][r], inv_s);
        if (split) {
          p.part[((int64_t)z * p.M + m) * p.N + n] = v;
          continue;
        }
        if (n >= p.nstore) continue;
        float* c = p.C + m * p.ldc + n;
        if (p.accumulate) v = __fadd_rn(*c, v);
        *c = v;
      }
    }
}

template <int MW, int NW>
__global__ __launch_bounds__(THREADS2, 1) void k_gemm_f1(Params p) {
  __shared__ __align__(16) char smem[F1Shape<MW, NW>::kLds];
  int tile, z;
  if (!split_of(p, tile, z)) return;
  f1_body<MW, NW>(p, z, smem);
}

// The batch's 256 x 256 products as two 256 x 128 half tiles each (k_gemm_f1h_batch): a
// workgroup keeps 64 accumulator VGPRs per wave instead of 128, which buys AON_F1H_SETS
// register sets of staged runs -- that many k-tiles of loads in flight instead of one -- for
// twice the A reads, the second from L2 (the two halves of a chunk are dispatched together on
// one XCD: block ids 8 apart).
#ifndef AON_F1H_SETS
#define AON_F1H_SETS 2  // 3 spills (22 VGPRs): 5.13 ms against 3.62-3.71 for 2, 4.08-4.12 whole tiles
#endif

constexpr int F1H_SETS = AON_F1H_SETS;

// one thread's run of a k-tile of the 128-column half h of a tiled fp32 operand of width 256:
// run u = tid: k row 16 (u / 256) + (u % 32) / 2, columns 16 ((u % 256) / 32) + 8 (u % 2) of
// the half (a wave reads two 1-KB runs of the tiled layout)
struct F1HalfRun {
  f4 v[2];
  __device__ __forceinline__ static int row(int tid) { return 16 * (tid >> 8) + ((tid & 31) >> 1); }
  __device__ __forceinline__ static int col(int tid) { return 16 * ((tid & 255) >> 5) + 8 * (tid & 1); }
  __device__ __forceinline__ void load(const float* base, int h, int64_t k0, int64_t kend, int tid) {
    const int rr = row(tid);
    const f4* src = reinterpret_cast<const f4*>(base + (k0 + 16 * (tid >> 8)) * 256 +
                                                256 * (8 * h + ((tid & 255) >> 5)) +
                                                16 * ((tid & 31) >> 1) + 8 * (tid & 1));
    if (k0 + rr < kend) {
      v[0] = src[0];
      v[1] = src[1];
    } else {
      v[0] = f4{0.f, 0.f, 0.f, 0.f};
      v[1] = f4{0.f, 0.f, 0.f, 0.f};
    }
  }
  __device__ __forceinline__ void store(char* hi, char* lo, float s, int tid) const {
    h8 hh, ll;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = v[e >> 2][e & 3] * s;
      const _Float16 q = static_cast<_Float16>(x);
      hh[e] = q;
      ll[e] = static_cast<_Float16>(__fsub_rn(x, static_cast<float>(q)));
    }
    const int off = tt_off(row(tid), col(tid) >> 3);
    *reinterpret_cast<h8*>(hi + off) = hh;
    *reinterpret_cast<h8*>(lo + off) = ll;
  }
};

struct F1HSet {
  F1Run<256> a;
  F1HalfRun b;
};

constexpr int F1H_STAGE = 2 * F1Img<256>::kPlane + 2 * F1Img<128>::kPlane;  // 48 KB

// product p's half h (columns 128 h ..) of K chunk z
__device__ __forceinline__ void f1h_body(const Params& p, int h, int z, char* smem) {
  float sa = p.sa, inv_s = p.inv_s;
  if (p.sa_bits) {
    const float gs = grad_scale(*p.sa_bits);
    sa = __fmul_rn(sa, gs);
    inv_s = __fdiv_rn(inv_s, gs);
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;  // 4 x 2 waves of 64 x 64
  const int64_t kbeg = (int64_t)z * p.kchunk;
  const int64_t kend = kbeg + p.kchunk < p.K ? kbeg + p.kchunk : p.K;
  const int nk = static_cast<int>((kend - kbeg + BK - 1) / BK);
  const bool want_rows = p.rowsum != nullptr && h == 0;
  float rs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  F1HSet set[F1H_SETS];
  auto load = [&](F1HSet& st, int kt) {
    const int64_t k0 = kbeg + (int64_t)kt * BK;
    st.a.load(p.A, k0, kend, tid, 0);
    st.a.load(p.A, k0, kend, tid, 1);
    st.b.load(p.B, h, k0, kend, tid);
  };
  auto publish = [&](const F1HSet& st, int stage) {
    char* s = smem + stage * F1H_STAGE;
    if (want_rows) {
      st.a.add_rows(rs, 0);
      st.a.add_rows(rs, 1);
    }
    st.a.store(s, s + F1Img<256>::kPlane, sa, tid, 0);
    st.a.store(s, s + F1Img<256>::kPlane, sa, tid, 1);
    char* sb = s + 2 * F1Img<256>::kPlane;
    st.b.store(sb, sb + F1Img<128>::kPlane, p.sb, tid);
  };
  f4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
  // tiles 0 .. SETS-1 into the sets, tile 0 to stage 0, its set refilled with tile SETS
#pragma unroll
  for (int q = 0; q < F1H_SETS; ++q)
    if (q < nk) load(set[q], q);
  if (nk > 0) {
    publish(set[0], 0);
    if (F1H_SETS < nk) load(set[0], F1H_SETS);
  }
  __syncthreads();
  // step kt: tile kt in stage kt & 1; tile kt + 1 in set (kt + 1) % SETS, published between
  // this step's MFMAs and that set refilled with tile kt + 1 + SETS (loaded SETS steps ahead)
  auto step = [&](int kt, auto cur) {
    constexpr int NXT = (decltype(cur)::value + 1) % F1H_SETS;
    const char* s = smem + (kt & 1) * F1H_STAGE;
    const char* sb = s + 2 * F1Img<256>::kPlane;
    h8 ah[4], al[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ah[i] = F1Img<256>::frag(s, 8 * wm + 2 * i, lane);
      al[i] = F1Img<256>::frag(s + F1Img<256>::kPlane, 8 * wm + 2 * i, lane);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c0 = 2 * (4 * wn + j);
      const h8 bh = F1Img<128>::frag(sb, c0, lane);
      const h8 bl = F1Img<128>::frag(sb + F1Img<128>::kPlane, c0, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[i][j] = mfma16(ah[i], bh, acc[i][j]);
        acc[i][j] = mfma16(ah[i], bl, acc[i][j]);
        acc[i][j] = mfma16(al[i], bh, acc[i][j]);
      }
      if (j == 0 && kt + 1 < nk) {
        publish(set[NXT], (kt + 1) & 1);
        if (kt + 1 + F1H_SETS < nk) load(set[NXT], kt + 1 + F1H_SETS);
      }
    }
    __syncthreads();
  };
  for (int kt = 0; kt < nk; kt += F1H_SETS) {
    step(kt, std::integral_constant<int, 0>{});
    if (F1H_SETS > 1 && kt + 1 < nk) step(kt + 1, std::integral_constant<int, 1 % F1H_SETS>{});
    if (F1H_SETS > 2 && kt + 2 < nk) step(kt + 2, std::integral_constant<int, 2 % F1H_SETS>{});
    if (F1H_SETS > 3 && kt + 3 < nk) step(kt + 3, std::integral_constant<int, 3 % F1H_SETS>{});
  }
  const bool split = p.zsplit > 1;
  if (want_rows) {
    float* red = reinterpret_cast<float*>(smem);  // [16 r][256]
    const int r = (tid & 31) >> 1, c = 16 * (tid >> 5) + 8 * (tid & 1);
#pragma unroll
    for (int e = 0; e < 8; ++e) red[r * 256 + c + e] = rs[e];
    __syncthreads();
    if (tid < 256) {
      float v = red[tid];
#pragma unroll
      for (int q = 1; q < 16; ++q) v = __fadd_rn(v, red[q * 256 + tid]);
      if (split) p.rowsum_part[(int64_t)z * p.M + tid] = v;
      else p.rowsum[tid] = v;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t n = 128 * h + 64 * wn + 16 * j + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t m = 64 * wm + 16 * i + 4 * (lane >> 4) + r;
        float v = __fmul_rn(acc[i][j][r], inv_s);
        if (split) {
          p.part[((int64_t)z * p.M + m) * p.N + n] = v;
          continue;
        }
        float* c = p.C + m * p.ldc + n;
        if (p.accumulate) v = __fadd_rn(*c, v);
        *c = v;
      }
    }
}

// T = 2 count half tiles: chunk z of every half of every product on one XCD, the two halves of
// a (product, chunk) 8 block ids apart
__global__ __launch_bounds__(THREADS2, 1) void k_gemm_f1h_batch(ParamsBatch pb) {
  __shared__ __align__(16) char smem[2 * F1H_STAGE];
  const int T = 2 * pb.count, L = blockIdx.x, x = L & 7, q = L >> 3;
  const int z = 8 * (q / T) + x, t = q - (q / T) * T;
  if (z >= pb.zsplit) return;  // padding block of the last chunk group (uniform exit)
  f1h_body(pb.p[t >> 1], t & 1, z, smem);
}

}  // namespace gemm
}  // namespace aon
