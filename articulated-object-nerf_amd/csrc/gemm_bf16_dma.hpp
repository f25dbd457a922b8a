// k_gemm_bf16_dma / k_gemm_bf16_dma256 and their batches: bf16 x bf16 weight gradients with
// the operand tiles copied HBM/L2 -> LDS by global_load_lds_dwordx4.
#pragma once
#include "gemm_bf16_km.hpp"

namespace aon {
namespace gemm {

// ---- bf16 x bf16 weight gradients with both operands bf16 and reduction-major (the bf16
// training mode's dW = dZ^T H on the fused kernels' tiled tensors, or row-major), M and N
// multiples of 128.  The k-tile of each operand is copied, not transposed, into a
// [k][128 columns] LDS image (XOR-swizzled 16-B chunks, cdna_hip_programming.md T10 (b)); the
// MFMA fragments, 8 consecutive k of one column, come out of ds_read_b64_tr_b16 (the hardware
// transpose read).  The transposing loader of k_gemm_bf16_km (4 x 8-B loads scattered over 32-B
// pieces per thread) held it at 0.34 ms per fine-level product: global loads, not MFMA or LDS,
// set its pace.
typedef short tt_v4s __attribute__((ext_vector_type(4)));
constexpr int TT_PLANE = BK * 256;  // bytes of one operand's [32 k][128 col] bf16 image

__device__ __forceinline__ int tt_off(int row, int ch) {  // byte offset of 16-B chunk ch of row
  return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

// 8 consecutive k (rows 8 g .. 8 g + 7 of the image) of column c0 * 8 + (lane & 15): two
// transposed reads of 4 rows x 16 columns each (lane 4 q + p addresses row q, columns 4 p..)
__device__ __forceinline__ bf8 tt_frag(const char* plane, int c0, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  tt_v4s h[2];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    const char* a = plane + tt_off(8 * g + 4 * hh + q, c0 + (p >> 1)) + 8 * (p & 1);
    h[hh] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        reinterpret_cast<__attribute__((address_space(3))) tt_v4s*>(
            reinterpret_cast<uintptr_t>(a)));
  }
  typedef short v8s __attribute__((ext_vector_type(8)));
  const v8s w = {h[0][0], h[0][1], h[0][2], h[0][3], h[1][0], h[1][1], h[1][2], h[1][3]};
  return __builtin_bit_cast(bf8, w);
}

// ---- the copies are global_load_lds_dwordx4 (no register staging): a DNB-deep ring of
// [32 k][128 col] image pairs, DNB - 1 k-tiles in flight ahead of the one in use.  A
// register-staged copy kernel (retired GEMM kernels) kept ~2 MB in flight chip-wide
// (PMC: 1,363-cycle HBM queue latency, 3.2 TB/s); the ring keeps DNB - 1 tiles of 16 KB per
// workgroup in flight.  The LDS image is lane-linear per copy (lane i of a wave's copy lands at
// 16 i), so the XOR swizzle is applied on the global side: lane i fetches the logical chunk
// that belongs at its physical slot.  A k-tile past the end of the reduction (only the last
// one of the last chunk) goes through registers with zero fill.
#ifndef AON_GEMM_DMA_NBUF
#define AON_GEMM_DMA_NBUF 3  // 2 / 4: within 2-10%, 6: 50% slower (profiles/r02/ab_gemm)
#endif
constexpr int DNB = AON_GEMM_DMA_NBUF;

// s_waitcnt vmcnt(n) (lgkmcnt, expcnt untouched); n a small constant after unrolling
__device__ __forceinline__ void dma_wait_vm(int n) {
#define AON_DW(n_) __builtin_amdgcn_s_waitcnt(((n_) & 0xF) | (((n_) >> 4) << 14) | (0x7 << 4) | (0xF << 8))
  switch (n) {
    case 0: AON_DW(0); break;
    case 1: AON_DW(1); break;
    case 2: AON_DW(2); break;
    case 3: AON_DW(3); break;
    case 4: AON_DW(4); break;
    case 5: AON_DW(5); break;
    case 6: AON_DW(6); break;
    case 7: AON_DW(7); break;
    case 8: AON_DW(8); break;
    case 9: AON_DW(9); break;
    case 10: AON_DW(10); break;
    case 11: AON_DW(11); break;
    default: AON_DW(12); break;
  }
#undef AON_DW
}

// one operand's copies: lane `lane` of wave w, copy c (0, 1) fills image row r = 8 w + 4 c +
// lane / 16, physical chunk lane % 16 <- logical chunk (lane % 16) ^ swz(r)
struct DmaOperand {
  const char* gbase;  // byte address of k-tile 0's (row 0, column col0) origin, kbeg applied
  int64_t tstep;      // bytes between k-tiles
  uint32_t voff[2];   // per-lane byte offset of copy c within a k-tile
  __device__ __forceinline__ DmaOperand(const __bf16* p, int64_t ld, int64_t col0, int64_t kbeg,
                                        int wave, int lane, bool tiled) {
    gbase = reinterpret_cast<const char*>(p) + 2 * (kbeg * ld + (tiled ? 16 * col0 : col0));
    tstep = 2 * BK * ld;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int r = 8 * wave + 4 * c + (lane >> 4);
      const int ch = (lane & 15) ^ (((r & 3) << 2) | ((r >> 2) & 3));
      const int64_t e = tiled ? (int64_t)(r & 16) * ld + 256 * (ch >> 1) + 16 * (r & 15) + 8 * (ch & 1)
                              : (int64_t)r * ld + 8 * ch;
      voff[c] = static_cast<uint32_t>(2 * e);
    }
  }
  // copy k-tile kt into the image at LDS byte address `plane` (this wave's rows)
  __device__ __forceinline__ void issue(uint32_t plane, int wave, int kt) const {
    const char* g = gbase + kt * tstep;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const uint32_t m0 = __builtin_amdgcn_readfirstlane(plane + 256u * (8 * wave + 4 * c));
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
      asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2"
                   :
                   : "s"(m0), "v"(voff[c]), "s"(g)
                   : "memory", "m0");
#pragma clang diagnostic pop
    }
  }
  // the same copies through registers, rows at or past `rows_left` zero (the ragged last tile)
  __device__ __forceinline__ void issue_ragged(char* plane, int wave, int lane, int kt,
                                               int64_t rows_left) const {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int r = 8 * wave + 4 * c + (lane >> 4);
      uint4 v = {0u, 0u, 0u, 0u};
      if (r < rows_left) v = *reinterpret_cast<const uint4*>(gbase + kt * tstep + voff[c]);
      *reinterpret_cast<uint4*>(plane + 256 * (8 * wave + 4 * c) + 16 * lane) = v;
    }
    // s_barrier does not wait for LDS writes: land them before the tile's barrier
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
};

__device__ __forceinline__ void dma128_body(const Params& p, int tm, int tn, int z, char* smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
  const int64_t kbeg = (int64_t)z * p.kchunk;
  const int64_t kend = kbeg + p.kchunk < p.K ? kbeg + p.kchunk : p.K;
  const int nk = static_cast<int>((kend - kbeg + BK - 1) / BK);
  const DmaOperand da(reinterpret_cast<const __bf16*>(p.A), p.lda, m0, kbeg, wave, lane, p.a_tiled);
  const DmaOperand db(reinterpret_cast<const __bf16*>(p.B), p.ldb, n0, kbeg, wave, lane, p.b_tiled);
  const uint32_t lds0 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(smem));
  // copies of k-tile kt into stage kt % DNB (4 per wave: 2 per operand)
  auto issue = [&](int kt) {
    const int st = kt % DNB;
    const int64_t left = kend - (kbeg + (int64_t)kt * BK);
    if (left >= BK) {
      da.issue(lds0 + st * 2 * TT_PLANE, wave, kt);
      db.issue(lds0 + st * 2 * TT_PLANE + TT_PLANE, wave, kt);
    } else {
      dma_wait_vm(0);
      da.issue_ragged(smem + st * 2 * TT_PLANE, wave, lane, kt, left);
      db.issue_ragged(smem + st * 2 * TT_PLANE + TT_PLANE, wave, lane, kt, left);
    }
  };
  f4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
  const bool want_rows = p.rowsum && tn == 0;
  float rs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // this thread's column-sum runs in the A image: rows kl0, kl0 + 16, columns cl .. cl + 7
  const int kl0 = tid >> 4, cl = 8 * (tid & 15);
  for (int kt = 0; kt < DNB - 1 && kt < nk; ++kt) issue(kt);
  for (int kt = 0; kt < nk; ++kt) {
    // this wave's copies of tile kt have landed once only the later tiles' may be pending
    const int later = (kt + DNB - 2 < nk - 1 ? kt + DNB - 2 : nk - 1) - kt;
    dma_wait_vm(4 * later);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // every wave is past tile kt - 1's reads: its stage takes tile kt + DNB - 1
    if (kt + DNB - 1 < nk) issue(kt + DNB - 1);
    const char* s = smem + (kt % DNB) * 2 * TT_PLANE;
    if (want_rows) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint4 v = *reinterpret_cast<const uint4*>(s + tt_off(kl0 + 16 * j, cl >> 3));
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t d = w[e >> 1];
          rs[e] = __fadd_rn(rs[e], __uint_as_float((e & 1) ? (d & 0xffff0000u) : (d << 16)));
        }
      }
    }
    bf8 b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = tt_frag(s + TT_PLANE, 8 * wn + 2 * j, lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bf8 a = tt_frag(s, 8 * wm + 2 * i, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[j], acc[i][j], 0, 0, 0);
    }
  }
  dma_wait_vm(0);
  __syncthreads();  // LDS free for the row-sum reduction
  const bool split = p.zsplit > 1;
  if (want_rows) {
    float* red = reinterpret_cast<float*>(smem);  // [16][128]
#pragma unroll
    for (int e = 0; e < 8; ++e) red[kl0 * BM + cl + e] = rs[e];
    __syncthreads();
    if (tid < BM) {
      float v = red[tid];
#pragma unroll
      for (int q = 1; q < 16; ++q) v = __fadd_rn(v, red[q * BM + tid]);
      if (split) p.rowsum_part[(int64_t)z * p.M + m0 + tid] = v;
      else p.rowsum[m0 + tid] = v;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t n = n0 + wn * 64 + 16 * j + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + wm * 64 + 16 * i + 4 * (lane >> 4) + r;
        float v = acc[i][j][r];
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

__global__ __launch_bounds__(THREADS, 2) void k_gemm_bf16_dma(Params p) {
  __shared__ __align__(16) char smem[DNB * 2 * TT_PLANE];  // DNB stages x (A, B) images
  int tm, tn, tile, z;
  if (!split_of(p, tile, z)) return;
  if (!tile_of(p, tile, tm, tn)) return;
  dma128_body(p, tm, tn, z, smem);
}

// A batch of products in whole 128 x 128 tiles over the same K (aon_gemm_batch): T = all the
// products' tiles, chunk z of every tile on one XCD (split_of's order), product b owning tiles
// tile0[b] .. tile0[b + 1] - 1 (its own grid, m fastest)
__global__ __launch_bounds__(THREADS, 2) void k_gemm_bf16_dma_batch(ParamsBatch pb) {
  __shared__ __align__(16) char smem[DNB * 2 * TT_PLANE];
  const int T = pb.tile0[pb.count], L = blockIdx.x, x = L & 7, q = L >> 3;
  const int z = 8 * (q / T) + x, t = q - (q / T) * T;
  if (z >= pb.zsplit) return;  // padding block of the last chunk group (uniform exit)
  int b = 0;
  while (b + 1 < pb.count && t >= pb.tile0[b + 1]) ++b;
  const Params& p = pb.p[b];
  const int lt = t - pb.tile0[b];
  dma128_body(p, lt % p.tiles_m, lt / p.tiles_m, z, smem);
}

// ---- the same product with a 256 x 256 C tile per workgroup (k_gemm_bf16_dma256): the
// training step's 256 x 256 weight gradients (pts_linears, bottleneck) are ONE tile, so every
// workgroup is a K chunk and each operand byte crosses into a CU once -- the 128 x 128 kernel
// reads every k-tile of both operands into two workgroups (the 2 x 2 tile grid), twice the
// bytes per CU for the same product (0.195 ms per fine-level product at ~15 B/cycle/CU).
// 512 threads = 8 waves in 4 (m) x 2 (n), each wave 64 x 128 = 4 x 8 MFMA tiles (128 fp32
// accumulator VGPRs), one workgroup per CU: DNB2 stages of a [32 k][256 col] image pair
// (32 KB), the same XOR swizzle on the low four 16-B chunks of each 512-B image row
// (ds_read_b64_tr_b16 banks repeat every 256 B, so the 128-column analysis holds).

#ifndef AON_GEMM_DMA256_NBUF
#define AON_GEMM_DMA256_NBUF 3
#endif
constexpr int DNB2 = AON_GEMM_DMA256_NBUF;
constexpr int BM2 = 256, THREADS2 = 512;
constexpr int TT_PLANE2 = BK * 512;  // bytes of one operand's [32 k][256 col] bf16 image

__device__ __forceinline__ int tt_off2(int row, int ch) {  // byte offset of 16-B chunk ch of row
  return 512 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

__device__ __forceinline__ bf8 tt_frag2(const char* plane, int c0, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  tt_v4s h[2];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    const char* a = plane + tt_off2(8 * g + 4 * hh + q, c0 + (p >> 1)) + 8 * (p & 1);
    h[hh] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        reinterpret_cast<__attribute__((address_space(3))) tt_v4s*>(
            reinterpret_cast<uintptr_t>(a)));
  }
  typedef short v8s __attribute__((ext_vector_type(8)));
  const v8s w = {h[0][0], h[0][1], h[0][2], h[0][3], h[1][0], h[1][1], h[1][2], h[1][3]};
  return __builtin_bit_cast(bf8, w);
}

// one operand's copies into a 256-column image: copy c of wave w fills image rows
// 2 (2 w + c) + lane / 32, physical chunk lane % 32 <- logical chunk (lane % 32) ^ swz(row)
struct DmaOperand2 {
  const char* gbase;
  int64_t tstep;
  uint32_t voff[2];
  __device__ __forceinline__ DmaOperand2(const __bf16* p, int64_t ld, int64_t col0, int64_t kbeg,
                                         int wave, int lane, bool tiled) {
    gbase = reinterpret_cast<const char*>(p) + 2 * (kbeg * ld + (tiled ? 16 * col0 : col0));
    tstep = 2 * BK * ld;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int r = 2 * (2 * wave + c) + (lane >> 5);
      const int ch = (lane & 31) ^ (((r & 3) << 2) | ((r >> 2) & 3));
      const int64_t e = tiled ? (int64_t)(r & 16) * ld + 256 * (ch >> 1) + 16 * (r & 15) + 8 * (ch & 1)
                              : (int64_t)r * ld + 8 * ch;
      voff[c] = static_cast<uint32_t>(2 * e);
    }
  }
  __device__ __forceinline__ void issue(uint32_t plane, int wave, int kt) const {
    const char* g = gbase + kt * tstep;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const uint32_t m0 = __builtin_amdgcn_readfirstlane(plane + 1024u * (2 * wave + c));
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
      asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2"
                   :
                   : "s"(m0), "v"(voff[c]), "s"(g)
                   : "memory", "m0");
#pragma clang diagnostic pop
    }
  }
  __device__ __forceinline__ void issue_ragged(char* plane, int wave, int lane, int kt,
                                               int64_t rows_left) const {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int r = 2 * (2 * wave + c) + (lane >> 5);
      uint4 v = {0u, 0u, 0u, 0u};
      if (r < rows_left) v = *reinterpret_cast<const uint4*>(gbase + kt * tstep + voff[c]);
      *reinterpret_cast<uint4*>(plane + 1024 * (2 * wave + c) + 16 * lane) = v;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
};

__device__ __forceinline__ void dma256_body(const Params& p, int tm, int tn, int z, char* smem) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = (int64_t)tm * BM2, n0 = (int64_t)tn * BM2;
  const int64_t kbeg = (int64_t)z * p.kchunk;
  const int64_t kend = kbeg + p.kchunk < p.K ? kbeg + p.kchunk : p.K;
  const int nk = static_cast<int>((kend - kbeg + BK - 1) / BK);
  const DmaOperand2 da(reinterpret_cast<const __bf16*>(p.A), p.lda, m0, kbeg, wave, lane, p.a_tiled);
  const DmaOperand2 db(reinterpret_cast<const __bf16*>(p.B), p.ldb, n0, kbeg, wave, lane, p.b_tiled);
  const uint32_t lds0 = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(smem));
  auto issue = [&](int kt) {
    const int st = kt % DNB2;
    const int64_t left = kend - (kbeg + (int64_t)kt * BK);
    if (left >= BK) {
      da.issue(lds0 + st * 2 * TT_PLANE2, wave, kt);
      db.issue(lds0 + st * 2 * TT_PLANE2 + TT_PLANE2, wave, kt);
    } else {
      dma_wait_vm(0);
      da.issue_ragged(smem + st * 2 * TT_PLANE2, wave, lane, kt, left);
      db.issue_ragged(smem + st * 2 * TT_PLANE2 + TT_PLANE2, wave, lane, kt, left);
    }
  };
  f4 acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
  const bool want_rows = p.rowsum && tn == 0;
  float rs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // this thread's column-sum runs in the A image: rows kl0, kl0 + 16, columns cl .. cl + 7
  const int kl0 = tid >> 5, cl = 8 * (tid & 31);
  for (int kt = 0; kt < DNB2 - 1 && kt < nk; ++kt) issue(kt);
  for (int kt = 0; kt < nk; ++kt) {
    const int later = (kt + DNB2 - 2 < nk - 1 ? kt + DNB2 - 2 : nk - 1) - kt;
    dma_wait_vm(4 * later);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (kt + DNB2 - 1 < nk) issue(kt + DNB2 - 1);
    const char* s = smem + (kt % DNB2) * 2 * TT_PLANE2;
    if (want_rows) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint4 v = *reinterpret_cast<const uint4*>(s + tt_off2(kl0 + 16 * j, cl >> 3));
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t d = w[e >> 1];
          rs[e] = __fadd_rn(rs[e], __uint_as_float((e & 1) ? (d & 0xffff0000u) : (d << 16)));
        }
      }
    }
    bf8 b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = tt_frag2(s + TT_PLANE2, 16 * wn + 2 * j, lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bf8 a = tt_frag2(s, 8 * wm + 2 * i, lane);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[j], acc[i][j], 0, 0, 0);
    }
  }
  dma_wait_vm(0);
  __syncthreads();  // LDS free for the row-sum reduction
  const bool split = p.zsplit > 1;
  if (want_rows) {
    float* red = reinterpret_cast<float*>(smem);  // [16][256]
#pragma unroll
    for (int e = 0; e < 8; ++e) red[kl0 * BM2 + cl + e] = rs[e];
    __syncthreads();
    if (tid < BM2) {
      float v = red[tid];
#pragma unroll
      for (int q = 1; q < 16; ++q) v = __fadd_rn(v, red[q * BM2 + tid]);
      if (split) p.rowsum_part[(int64_t)z * p.M + m0 + tid] = v;
      else p.rowsum[m0 + tid] = v;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t n = n0 + wn * 128 + 16 * j + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + wm * 64 + 16 * i + 4 * (lane >> 4) + r;
        float v = acc[i][j][r];
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

__global__ __launch_bounds__(THREADS2, 2) void k_gemm_bf16_dma256(Params p) {
  __shared__ __align__(16) char smem[DNB2 * 2 * TT_PLANE2];  // DNB2 stages x (A, B) images
  int tm, tn, tile, z;
  if (!split_of(p, tile, z)) return;
  if (!tile_of(p, tile, tm, tn)) return;
  dma256_body(p, tm, tn, z, smem);
}

// A batch of one-tile (256 x 256) products over the same K (one level's weight gradients): the
// 256 workgroups are count products x zsplit K chunks -- chunk z of every product on one XCD
// (split_of's order, the product index in place of the tile) -- so each product's chunks are
// count times longer than in its own launch: count times fewer fp32 partials written and summed
// (each launch of a lone product wrote 256 x 257 KB = 67 MB of partials for 0.27-0.81 GB of
// operands), and one launch + one reduce per level instead of count of each.
__global__ __launch_bounds__(THREADS2, 2) void k_gemm_bf16_dma256_batch(ParamsBatch pb) {
  __shared__ __align__(16) char smem[DNB2 * 2 * TT_PLANE2];
  const int T = pb.count, L = blockIdx.x, x = L & 7, q = L >> 3;
  const int z = 8 * (q / T) + x, b = q - (q / T) * T;
  if (z >= pb.zsplit) return;  // padding block of the last chunk group (uniform exit)
  dma256_body(pb.p[b], 0, 0, z, smem);
}

}  // namespace gemm
}  // namespace aon
