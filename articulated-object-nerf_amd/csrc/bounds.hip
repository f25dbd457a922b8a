// Box-bounded rendering: the ray / box slab test and the batch fill of the reference's
// get_ray_limits_box / get_ray_limits (models/vanilla_nerf/helper.py:42-102, :29-39), its
// stratified sampler on per-ray bounds (helper.py:116-129), and this project's own extension:
// an order-preserving compaction of the rays that hit the box and the scatter of their rendered
// rows back into the frame.  All HBM-bound, one lane per ray (or per sample); every reference
// op is one correctly rounded fp32 op (no contraction), so the limits and the sample positions
// equal the reference's torch CPU values bit for bit.
#include <climits>

#include "aon_common.hpp"

namespace aon {

constexpr int kBlock = 256;            // threads per workgroup of the per-ray kernels
constexpr int kWaves = kBlock / 64;
constexpr int kScanBlock = 1024;       // the single workgroup that scans the block counts

// torch.max / torch.min of two tensors (helper.py:85-86, :97-98): NaN if either is NaN (fmaxf /
// fminf would drop it); of two equal values the second, as ATen's vectorised kernels return it
__device__ __forceinline__ float max_nan(float a, float b) {
  if (a != a || b != b) return __builtin_nanf("");
  return a > b ? a : b;
}
__device__ __forceinline__ float min_nan(float a, float b) {
  if (a != a || b != b) return __builtin_nanf("");
  return a < b ? a : b;
}

// helper.py:66-81 for one axis: invdir = 1 / d; sign = invdir < 0 (so d = -0.0 -> -inf selects
// the upper bound first); t0 = (bounds[sign] - o) * invdir, t1 = (bounds[1 - sign] - o) * invdir
__device__ __forceinline__ void slab(float o, float d, float half, float& t0, float& t1) {
  const float inv = __fdiv_rn(1.0f, d);
  const bool neg = inv < 0.0f;
  t0 = __fmul_rn(__fsub_rn(neg ? half : -half, o), inv);
  t1 = __fmul_rn(__fsub_rn(neg ? -half : half, o), inv);
}

// helper.py:42-102 for one ray: misses get (-1, -2)
__device__ __forceinline__ void box_limits(const float* __restrict__ ro,
                                           const float* __restrict__ rd, int64_t b, float half,
                                           float& tmin, float& tmax) {
  float tymin, tymax, tzmin, tzmax;
  slab(ro[3 * b], rd[3 * b], half, tmin, tmax);
  slab(ro[3 * b + 1], rd[3 * b + 1], half, tymin, tymax);
  bool valid = true;
  if (tmin > tymax || tymin > tmax) valid = false;  // (a NaN compares false: stays valid)
  tmin = max_nan(tmin, tymin);
  tmax = min_nan(tmax, tymax);
  slab(ro[3 * b + 2], rd[3 * b + 2], half, tzmin, tzmax);
  if (tmin > tzmax || tzmin > tmax) valid = false;
  tmin = max_nan(tmin, tzmin);
  tmax = min_nan(tmax, tzmax);
  if (!valid) {
    tmin = -1.0f;
    tmax = -2.0f;
  }
}

// One lane per ray.  part != NULL (aon_ray_limits): also this workgroup's minimum near and
// maximum far over its valid rays (far > near, helper.py:33) and their count, at
// part[3 * block + 0 / 1 / 2] (the count as int32 bits).
__global__ void __launch_bounds__(kBlock)
k_ray_limits_box(const float* __restrict__ ro, const float* __restrict__ rd, int64_t B, float half,
                 float* __restrict__ tmin_out, float* __restrict__ tmax_out,
                 float* __restrict__ part) {
  const int64_t b = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  float tmin = 0.0f, tmax = 0.0f;
  if (b < B) {
    box_limits(ro, rd, b, half, tmin, tmax);
    tmin_out[b] = tmin;
    tmax_out[b] = tmax;
  }
  if (!part) return;  // (uniform over the grid)
  const bool valid = b < B && tmax > tmin;
  float mn = valid ? tmin : __builtin_inff(), mx = valid ? tmax : -__builtin_inff();
#pragma unroll
  for (int off = 32; off; off >>= 1) {  // valid values are never NaN: fminf / fmaxf are exact
    mn = fminf(mn, __shfl_xor(mn, off));
    mx = fmaxf(mx, __shfl_xor(mx, off));
  }
  const int cnt = __popcll(__ballot(valid));
  __shared__ float s_mn[kWaves], s_mx[kWaves];
  __shared__ int s_cnt[kWaves];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_mn[wave] = mn;
    s_mx[wave] = mx;
    s_cnt[wave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      mn = fminf(mn, s_mn[w]);
      mx = fmaxf(mx, s_mx[w]);
      c += s_cnt[w];
    }
    part[3 * (int64_t)blockIdx.x] = mn;
    part[3 * (int64_t)blockIdx.x + 1] = mx;
    part[3 * (int64_t)blockIdx.x + 2] = __int_as_float(c > 0 ? 1 : 0);
  }
}

// one workgroup: the batch's (min near, max far, any valid) from the per-workgroup partials,
// written to part[3 * nblocks ..] (a min / max reduction: exact in any order)
__global__ void __launch_bounds__(kScanBlock)
k_limits_reduce(float* __restrict__ part, int64_t nblocks) {
  float mn = __builtin_inff(), mx = -__builtin_inff();
  int any = 0;
  for (int64_t i = threadIdx.x; i < nblocks; i += kScanBlock) {
    mn = fminf(mn, part[3 * i]);
    mx = fmaxf(mx, part[3 * i + 1]);
    any |= __float_as_int(part[3 * i + 2]);
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, off));
    mx = fmaxf(mx, __shfl_xor(mx, off));
    any |= __shfl_xor(any, off);
  }
  __shared__ float s_mn[kScanBlock / 64], s_mx[kScanBlock / 64];
  __shared__ int s_any[kScanBlock / 64];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_mn[wave] = mn;
    s_mx[wave] = mx;
    s_any[wave] = any;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < kScanBlock / 64; ++w) {
      mn = fminf(mn, s_mn[w]);
      mx = fmaxf(mx, s_mx[w]);
      any |= s_any[w];
    }
    part[3 * nblocks] = mn;
    part[3 * nblocks + 1] = mx;
    part[3 * nblocks + 2] = __int_as_float(any);
  }
}

// helper.py:33-38: invalid rays take the batch's minimum near / maximum far (if any ray is
// valid), then negatives become 0 (a NaN stays)
__global__ void __launch_bounds__(kBlock)
k_limits_fill(float* __restrict__ near, float* __restrict__ far, int64_t B,
              const float* __restrict__ total) {
  const int64_t b = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  if (b >= B) return;
  float n = near[b], f = far[b];
  if (__float_as_int(total[2]) && !(f > n)) {
    n = total[0];
    f = total[1];
  }
  if (n < 0.0f) n = 0.0f;
  if (f < 0.0f) f = 0.0f;
  near[b] = n;
  far[b] = f;
}

// helper.py:117-120 for entry j of ray (near, far): one rounding per reference op
__device__ __forceinline__ float sched_at(const float* __restrict__ s_tab, int j, float near,
                                          float far, bool lindisp) {
  const float s = s_tab[j], c = __fsub_rn(1.0f, s);
  if (lindisp)
    return __fdiv_rn(1.0f, __fadd_rn(__fmul_rn(__fdiv_rn(1.0f, near), c),
                                     __fmul_rn(__fdiv_rn(1.0f, far), s)));
  return __fadd_rn(__fmul_rn(near, c), __fmul_rn(far, s));
}

// helper.py:116-131 on per-ray bounds, one lane per (ray, sample): the schedule entry, and when
// randomized its strata bounds from the two neighbouring entries (mids = 0.5 * (t[j+1] + t[j]);
// lower = [t[0], mids], upper = [mids, t[S-1]]), t = lower + (upper - lower) * u
__global__ void k_sample_along_rays_bounds(const float* __restrict__ ro,
                                           const float* __restrict__ rd, int64_t B, int S,
                                           const float* __restrict__ s_tab,
                                           const float* __restrict__ near,
                                           const float* __restrict__ far, bool lindisp,
                                           const float* __restrict__ u, float* __restrict__ t_out,
                                           float* __restrict__ xyz) {
  const int64_t n = B * S;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / S;
    const int s = static_cast<int>(i - b * S);
    const float nr = near[b], fr = far[b];
    float t = sched_at(s_tab, s, nr, fr, lindisp);
    if (u) {
      float lower = t, upper = t;
      if (s > 0) lower = __fmul_rn(0.5f, __fadd_rn(t, sched_at(s_tab, s - 1, nr, fr, lindisp)));
      if (s < S - 1) upper = __fmul_rn(0.5f, __fadd_rn(sched_at(s_tab, s + 1, nr, fr, lindisp), t));
      t = __fadd_rn(lower, __fmul_rn(__fsub_rn(upper, lower), u[i]));
    }
    t_out[i] = t;
    if (xyz) {
#pragma unroll
      for (int c = 0; c < 3; ++c) xyz[3 * i + c] = __fadd_rn(ro[3 * b + c], __fmul_rn(t, rd[3 * b + c]));
    }
  }
}

// ---------------------------------------------------------------------------- culling
// a ray hits the box iff tmax > max(tmin, 0); a NaN limit compares false: a miss
__device__ __forceinline__ bool ray_hits(float tmin, float tmax) {
  return tmax > tmin && tmax > 0.0f;
}

// pass 1: hits per workgroup, from the wave ballots
__global__ void __launch_bounds__(kBlock)
k_hit_counts(const float* __restrict__ tmin, const float* __restrict__ tmax, int64_t B,
             int32_t* __restrict__ counts) {
  const int64_t b = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  const bool hit = b < B && ray_hits(tmin[b], tmax[b]);
  const int cnt = __popcll(__ballot(hit));
  __shared__ int s_cnt[kWaves];
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) c += s_cnt[w];
    counts[blockIdx.x] = c;
  }
}

// pass 2: one workgroup turns the counts into exclusive offsets in place (kScanBlock at a time,
// carrying the running total) and writes the total
__global__ void __launch_bounds__(kScanBlock)
k_scan_counts(int32_t* __restrict__ counts, int64_t nblocks, int32_t* __restrict__ total) {
  __shared__ int s_wave[kScanBlock / 64];
  __shared__ int s_carry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < nblocks; base += kScanBlock) {
    const int64_t i = base + threadIdx.x;
    const int v = i < nblocks ? counts[i] : 0;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(incl, off);
      if (lane >= off) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = s_carry;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    if (i < nblocks) counts[i] = before + incl - v;
    __syncthreads();  // every lane has read s_carry / s_wave
    if (threadIdx.x == kScanBlock - 1) s_carry = before + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = s_carry;
}

// pass 3: rank = workgroup offset + the earlier waves' hits + the ballot's lower lanes; writes
// slot[b] for every ray and, for a hit, its index and its gathered row
__global__ void __launch_bounds__(kBlock)
k_compact(const float* __restrict__ tmin, const float* __restrict__ tmax,
          const float* __restrict__ ro, const float* __restrict__ rd,
          const float* __restrict__ vd, int64_t B, const int32_t* __restrict__ offsets,
          int32_t* __restrict__ slot, int32_t* __restrict__ idx, float* __restrict__ o_out,
          float* __restrict__ d_out, float* __restrict__ v_out, float* __restrict__ near_out,
          float* __restrict__ far_out) {
  const int64_t b = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  float lo = 0.0f, hi = 0.0f;
  bool hit = false;
  if (b < B) {
    lo = tmin[b];
    hi = tmax[b];
    hit = ray_hits(lo, hi);
  }
  const unsigned long long ballot = __ballot(hit);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ int s_cnt[kWaves];
  if (lane == 0) s_cnt[wave] = __popcll(ballot);
  __syncthreads();
  if (b >= B) return;
  if (!hit) {
    slot[b] = -1;
    return;
  }
  int r = offsets[blockIdx.x] + __popcll(ballot & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) r += s_cnt[w];
  // r < total hits <= B: the outputs hold B rows
  slot[b] = r;
  idx[r] = static_cast<int32_t>(b);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    o_out[3 * (int64_t)r + c] = ro[3 * b + c];
    d_out[3 * (int64_t)r + c] = rd[3 * b + c];
    if (v_out) v_out[3 * (int64_t)r + c] = vd[3 * b + c];
  }
  near_out[r] = lo > 0.0f ? lo : 0.0f;
  far_out[r] = hi;
}

// one lane per frame ray: its compact row, or the background row
__global__ void __launch_bounds__(kBlock)
k_scatter_payload(const float* __restrict__ comp, const float* __restrict__ acc,
                  const float* __restrict__ depth, int64_t n_comp,
                  const int32_t* __restrict__ slot, int64_t B, float bg, float* __restrict__ out) {
  const int64_t b = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  if (b >= B) return;
  const int64_t s = slot[b];
  float* o = out + 5 * b;
  if (s >= 0 && s < n_comp) {
    o[0] = comp[3 * s];
    o[1] = comp[3 * s + 1];
    o[2] = comp[3 * s + 2];
    o[3] = depth[s];
    o[4] = acc[s];
  } else {
    o[0] = o[1] = o[2] = bg;
    o[3] = o[4] = 0.0f;
  }
}

static inline int64_t ray_blocks(int64_t B) { return (B + kBlock - 1) / kBlock; }

}  // namespace aon

using namespace aon;

extern "C" int aon_ray_limits_box(const float* rays_o, const float* rays_d, int64_t B,
                                  float half_side, float* tmin, float* tmax,
                                  aon_stream_t stream) {
  AON_REQUIRE(rays_o && rays_d && tmin && tmax, "null pointer");
  AON_REQUIRE(B >= 0 && B <= INT32_MAX, "B outside [0, 2^31)");
  AON_REQUIRE(half_side > 0.0f, "half_side must be positive");
  if (B == 0) return 0;
  hipLaunchKernelGGL(k_ray_limits_box, dim3((unsigned)ray_blocks(B)), kBlock, 0,
                     (hipStream_t)stream, rays_o, rays_d, B, half_side, tmin, tmax,
                     (float*)nullptr);
  return launch_status(__func__);
}

extern "C" size_t aon_ray_limits_workspace_bytes(int64_t B) {
  if (B < 0 || B > INT32_MAX) return 0;
  return static_cast<size_t>(3 * (ray_blocks(B) + 1)) * sizeof(float);
}

extern "C" int aon_ray_limits(const float* rays_o, const float* rays_d, int64_t B,
                              float half_side, float* near, float* far, void* work,
                              size_t work_bytes, aon_stream_t stream) {
  AON_REQUIRE(rays_o && rays_d && near && far && work, "null pointer");
  AON_REQUIRE(B >= 0 && B <= INT32_MAX, "B outside [0, 2^31)");
  AON_REQUIRE(half_side > 0.0f, "half_side must be positive");
  AON_REQUIRE(work_bytes >= aon_ray_limits_workspace_bytes(B), "work_bytes too small");
  if (B == 0) return 0;
  const int64_t nb = ray_blocks(B);
  float* part = static_cast<float*>(work);
  hipLaunchKernelGGL(k_ray_limits_box, dim3((unsigned)nb), kBlock, 0, (hipStream_t)stream, rays_o,
                     rays_d, B, half_side, near, far, part);
  hipLaunchKernelGGL(k_limits_reduce, 1, kScanBlock, 0, (hipStream_t)stream, part, nb);
  hipLaunchKernelGGL(k_limits_fill, dim3((unsigned)nb), kBlock, 0, (hipStream_t)stream, near, far,
                     B, part + 3 * nb);
  return launch_status(__func__);
}

extern "C" int aon_sample_along_rays_bounds(const float* rays_o, const float* rays_d, int64_t B,
                                            int S, const float* s_tab, const float* near,
                                            const float* far, int lindisp, const float* u,
                                            float* t_out, float* xyz_out, aon_stream_t stream) {
  AON_REQUIRE(s_tab && near && far && t_out, "null pointer");
  AON_REQUIRE(B >= 0, "B < 0");
  AON_REQUIRE(S >= 2, "S < 2");
  AON_REQUIRE(!xyz_out || (rays_o && rays_d), "xyz needs rays_o/rays_d");
  if (B == 0) return 0;
  hipLaunchKernelGGL(k_sample_along_rays_bounds, grid_for(B * S, 256, 65536), 256, 0,
                     (hipStream_t)stream, rays_o, rays_d, B, S, s_tab, near, far, lindisp != 0, u,
                     t_out, xyz_out);
  return launch_status(__func__);
}

extern "C" size_t aon_compact_rays_workspace_bytes(int64_t B) {
  if (B < 0 || B > INT32_MAX) return 0;
  return static_cast<size_t>(ray_blocks(B) + 1) * sizeof(int32_t);
}

extern "C" int aon_compact_rays(const float* tmin, const float* tmax, const float* rays_o,
                                const float* rays_d, const float* viewdirs, int64_t B,
                                int32_t* slot, int32_t* idx, float* o_out, float* d_out,
                                float* v_out, float* near_out, float* far_out, int32_t* n_hit,
                                void* work, size_t work_bytes, aon_stream_t stream) {
  AON_REQUIRE(tmin && tmax && rays_o && rays_d && slot && idx && o_out && d_out && near_out &&
                  far_out && n_hit && work,
              "null pointer");
  AON_REQUIRE(!viewdirs == !v_out, "viewdirs and v_out go together");
  AON_REQUIRE(B >= 0 && B <= INT32_MAX, "B outside [0, 2^31)");
  AON_REQUIRE(work_bytes >= aon_compact_rays_workspace_bytes(B), "work_bytes too small");
  const int64_t nb = ray_blocks(B);
  int32_t* counts = static_cast<int32_t*>(work);
  if (B > 0)
    hipLaunchKernelGGL(k_hit_counts, dim3((unsigned)nb), kBlock, 0, (hipStream_t)stream, tmin,
                       tmax, B, counts);
  hipLaunchKernelGGL(k_scan_counts, 1, kScanBlock, 0, (hipStream_t)stream, counts, nb, n_hit);
  if (B > 0)
    hipLaunchKernelGGL(k_compact, dim3((unsigned)nb), kBlock, 0, (hipStream_t)stream, tmin, tmax,
                       rays_o, rays_d, viewdirs, B, counts, slot, idx, o_out, d_out, v_out,
                       near_out, far_out);
  return launch_status(__func__);
}

extern "C" int aon_scatter_payload(const float* comp, const float* acc, const float* depth,
                                   int64_t n_comp, const int32_t* slot, int64_t B, int white_bkgd,
                                   float* out, aon_stream_t stream) {
  AON_REQUIRE(slot && out, "null pointer");
  AON_REQUIRE(n_comp >= 0 && (n_comp == 0 || (comp && acc && depth)), "null pointer");
  AON_REQUIRE(B >= 0 && B <= INT32_MAX, "B outside [0, 2^31)");
  if (B == 0) return 0;
  hipLaunchKernelGGL(k_scatter_payload, dim3((unsigned)ray_blocks(B)), kBlock, 0,
                     (hipStream_t)stream, comp, acc, depth, n_comp, slot, B,
                     white_bkgd ? 1.0f : 0.0f, out);
  return launch_status(__func__);
}
