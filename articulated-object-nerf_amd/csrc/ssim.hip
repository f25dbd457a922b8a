// SSIM of the reference's test epoch (models/interface.py:101-111, 141-155: piqa.ssim.SSIM()
// with its defaults -- 11-tap Gaussian window of sigma 1.5, no padding, value range 1, mean over
// channels and window positions), evaluated in fp64: in fp32 the variance terms E[x^2] - mx^2
// cancel against c2 = 9e-4 and near-flat images drift by up to ~7e-5 (DESIGN.md "Metrics").
#include "aon_common.hpp"

namespace aon {

constexpr int kSsimTH = 21, kSsimTW = 32;    // one workgroup's output tile
constexpr int kSsimWin = 11;                 // window taps
constexpr int kSsimRows = kSsimTH + kSsimWin - 1;  // input rows of a tile (31)
constexpr int kSsimCols = kSsimTW + kSsimWin - 1;  // input columns of a tile (42)
constexpr int kSsimPitch = 44;               // LDS row pitch in floats: 16-byte rows that hold
                                             // the last column group's 16-float read
constexpr int kSsimHX = 4;                   // horizontal pass: outputs per thread (one row)
constexpr int kSsimHGroups = kSsimTW / kSsimHX;
constexpr int kSsimVR = 3;                   // vertical pass: output rows per thread (one column)
constexpr int kSsimVGroups = kSsimTH / kSsimVR;
constexpr int kSsimThreads = 256;
static_assert(kSsimTW % kSsimHX == 0 && kSsimTH % kSsimVR == 0, "tile / blocking mismatch");
static_assert(kSsimVGroups * kSsimTW <= kSsimThreads, "vertical pass: one thread per column strip");
static_assert(kSsimPitch % 4 == 0 && kSsimPitch >= (kSsimHGroups - 1) * kSsimHX + 16, "LDS pitch");
static_assert(kSsimPitch >= kSsimCols, "LDS pitch");

// g[i] = exp(-(i - 5)^2 / (2 1.5^2)) / sum, rounded to fp64
static __device__ const double kSsimG[kSsimWin] = {
    0.00102838008447911,  0.007598758135239185, 0.03600077212843083, 0.10936068950970002,
    0.2130055377112537,   0.26601172486179436,  0.2130055377112537,  0.10936068950970002,
    0.03600077212843083,  0.007598758135239185, 0.00102838008447911};

// One workgroup per (tile, image); the three channels one after another through the same LDS:
//   stage   the (TH+10) x (TW+10) input tile of both images, clipped, fp32 (out of the image: 0,
//           feeding only outputs that are masked below);
//   rows    11-tap horizontal sums of x, y, x^2, y^2, x y in fp64 -> s_h, 4 adjacent outputs per
//           thread from one 14-value register window (16-byte LDS reads);
//   columns 11-tap vertical sums, 3 output rows per thread from one 13-value window (8-byte LDS
//           reads, consecutive lanes on consecutive columns), then ss;
// and the tile's sum of ss (fp64, fixed order) -> partial[image][tile].
__global__ __launch_bounds__(kSsimThreads) void k_ssim_tiles(const float* __restrict__ pred,
                                                             const float* __restrict__ gt,
                                                             int64_t H, int64_t W,
                                                             float* __restrict__ ss_map,
                                                             double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float s_x[kSsimRows * kSsimPitch];
  __shared__ __attribute__((aligned(16))) float s_y[kSsimRows * kSsimPitch];
  __shared__ __attribute__((aligned(16))) double s_h[5][kSsimRows][kSsimTW];
  __shared__ double s_red[kSsimThreads];
  const int tid = threadIdx.x;
  const int64_t img = blockIdx.z;
  const int64_t ox = (int64_t)blockIdx.x * kSsimTW, oy = (int64_t)blockIdx.y * kSsimTH;
  const int64_t OH = H - (kSsimWin - 1), OW = W - (kSsimWin - 1);
  const float* p = pred + img * H * W * 3;
  const float* g = gt + img * H * W * 3;
  constexpr double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
  double acc = 0.0;

  for (int ch = 0; ch < 3; ++ch) {
    for (int i = tid; i < kSsimRows * kSsimPitch; i += kSsimThreads) {
      const int r = i / kSsimPitch, c = i - r * kSsimPitch;
      const int64_t gy = oy + r, gx = ox + c;
      float a = 0.0f, b = 0.0f;
      if (c < kSsimCols && gy < H && gx < W) {
        const int64_t e = (gy * W + gx) * 3 + ch;
        a = fminf(fmaxf(p[e], 0.0f), 1.0f);
        b = fminf(fmaxf(g[e], 0.0f), 1.0f);
      }
      s_x[i] = a;
      s_y[i] = b;
    }
    __syncthreads();

    for (int it = tid; it < kSsimRows * kSsimHGroups; it += kSsimThreads) {
      const int r = it / kSsimHGroups, cg = it - r * kSsimHGroups;
      const f4* px = reinterpret_cast<const f4*>(&s_x[r * kSsimPitch + cg * kSsimHX]);
      const f4* py = reinterpret_cast<const f4*>(&s_y[r * kSsimPitch + cg * kSsimHX]);
      double x[16], y[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f4 vx = px[q], vy = py[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          x[4 * q + j] = (double)vx[j];
          y[4 * q + j] = (double)vy[j];
        }
      }
      double sx[kSsimHX], sy[kSsimHX], sxx[kSsimHX], syy[kSsimHX], sxy[kSsimHX];
#pragma unroll
      for (int o = 0; o < kSsimHX; ++o) sx[o] = sy[o] = sxx[o] = syy[o] = sxy[o] = 0.0;
#pragma unroll
      for (int k = 0; k < kSsimWin; ++k) {
#pragma unroll
        for (int o = 0; o < kSsimHX; ++o) {
          // x y and x x are the same operations on the same numbers when the images are equal
          const double wx = kSsimG[k] * x[o + k], wy = kSsimG[k] * y[o + k];
          sx[o] += wx;
          sy[o] += wy;
          sxx[o] = fma(wx, x[o + k], sxx[o]);
          syy[o] = fma(wy, y[o + k], syy[o]);
          sxy[o] = fma(wx, y[o + k], sxy[o]);
        }
      }
#pragma unroll
      for (int o = 0; o < kSsimHX; ++o) {
        s_h[0][r][cg * kSsimHX + o] = sx[o];
        s_h[1][r][cg * kSsimHX + o] = sy[o];
        s_h[2][r][cg * kSsimHX + o] = sxx[o];
        s_h[3][r][cg * kSsimHX + o] = syy[o];
        s_h[4][r][cg * kSsimHX + o] = sxy[o];
      }
    }
    __syncthreads();

    if (tid < kSsimVGroups * kSsimTW) {
      const int col = tid % kSsimTW, r0 = (tid / kSsimTW) * kSsimVR;
      double m[5][kSsimVR];
#pragma unroll
      for (int mo = 0; mo < 5; ++mo) {
        double h[kSsimVR + kSsimWin - 1];
#pragma unroll
        for (int j = 0; j < kSsimVR + kSsimWin - 1; ++j) h[j] = s_h[mo][r0 + j][col];
#pragma unroll
        for (int i = 0; i < kSsimVR; ++i) {
          double a = 0.0;
#pragma unroll
          for (int k = 0; k < kSsimWin; ++k) a = fma(kSsimG[k], h[i + k], a);
          m[mo][i] = a;
        }
      }
#pragma unroll
      for (int i = 0; i < kSsimVR; ++i) {
        const double mxx = m[0][i] * m[0][i], myy = m[1][i] * m[1][i], mxy = m[0][i] * m[1][i];
        const double vxx = m[2][i] - mxx, vyy = m[3][i] - myy, vxy = m[4][i] - mxy;
        // l cs as one quotient; numerator and denominator are bit-identical for equal images
        const double num = (2.0 * mxy + c1) * (2.0 * vxy + c2);
        const double den = (mxx + myy + c1) * (vxx + vyy + c2);
        const double ss = num / den;
        const int64_t orow = oy + r0 + i, ocol = ox + col;
        if (orow < OH && ocol < OW) {
          acc += ss;
          if (ss_map) ss_map[((img * 3 + ch) * OH + orow) * OW + ocol] = (float)ss;
        }
      }
    }
    // (the next channel's staging writes s_x / s_y only, which nobody reads after the barrier
    // above; its barrier orders this channel's s_h reads before the next row pass)
  }

  s_red[tid] = acc;
  __syncthreads();
  for (int o = kSsimThreads / 2; o > 0; o >>= 1) {
    if (tid < o) s_red[tid] += s_red[tid + o];
    __syncthreads();
  }
  if (tid == 0)
    partial[(img * gridDim.y + blockIdx.y) * (int64_t)gridDim.x + blockIdx.x] = s_red[0];
}

// One workgroup per image: the tiles' partial sums in a fixed order / (3 (H-10) (W-10)).
__global__ __launch_bounds__(kSsimThreads) void k_ssim_finish(const double* __restrict__ partial,
                                                              int64_t tiles, double count,
                                                              float* __restrict__ ssim) {
  __shared__ double s_red[kSsimThreads];
  const int tid = threadIdx.x;
  const double* q = partial + (int64_t)blockIdx.x * tiles;
  double acc = 0.0;
  for (int64_t t = tid; t < tiles; t += kSsimThreads) acc += q[t];
  s_red[tid] = acc;
  __syncthreads();
  for (int o = kSsimThreads / 2; o > 0; o >>= 1) {
    if (tid < o) s_red[tid] += s_red[tid + o];
    __syncthreads();
  }
  if (tid == 0) ssim[blockIdx.x] = (float)(s_red[0] / count);
}

// tiles along x / y; false when the shape is invalid or a grid dimension would overflow
static bool ssim_grid(int64_t n, int64_t h, int64_t w, int64_t* tx, int64_t* ty) {
  if (n < 0 || h < kSsimWin || w < kSsimWin) return false;
  *tx = (w - (kSsimWin - 1) + kSsimTW - 1) / kSsimTW;
  *ty = (h - (kSsimWin - 1) + kSsimTH - 1) / kSsimTH;
  return n <= 65535 && *ty <= 65535 && *tx <= 0x7fffffffll &&
         w <= (1ll << 40) / h / 3;  // element offsets of one image stay far inside int64
}

}  // namespace aon

using namespace aon;

extern "C" const int aon_ssim_tile[2] = {kSsimTH, kSsimTW};

extern "C" size_t aon_ssim_workspace_bytes(int64_t n_images, int64_t height, int64_t width) {
  int64_t tx = 0, ty = 0;
  if (!ssim_grid(n_images, height, width, &tx, &ty)) return 0;
  return (size_t)(n_images > 0 ? n_images : 1) * (size_t)tx * (size_t)ty * sizeof(double);
}

extern "C" int aon_image_ssim(const float* pred, const float* gt, int64_t n_images,
                              int64_t height, int64_t width, float* ssim, float* ss_map,
                              void* work, size_t work_bytes, aon_stream_t stream) {
  AON_REQUIRE(n_images >= 0, "negative image count");
  if (n_images == 0) return 0;
  AON_REQUIRE(pred && gt && ssim && work, "bad arguments (null pred, gt, ssim or work)");
  AON_REQUIRE(height >= kSsimWin && width >= kSsimWin, "height and width must be at least 11");
  int64_t tx = 0, ty = 0;
  AON_REQUIRE(ssim_grid(n_images, height, width, &tx, &ty),
              "too large for one call: at most 65535 images, 65535 tile rows, 2^40 values per image");
  AON_REQUIRE(work_bytes >= aon_ssim_workspace_bytes(n_images, height, width),
              "work_bytes below aon_ssim_workspace_bytes()");
  AON_REQUIRE((reinterpret_cast<uintptr_t>(work) & 7u) == 0, "work must be 8-byte aligned");
  double* partial = static_cast<double*>(work);
  hipLaunchKernelGGL(k_ssim_tiles, dim3((unsigned)tx, (unsigned)ty, (unsigned)n_images),
                     kSsimThreads, 0, (hipStream_t)stream, pred, gt, height, width, ss_map,
                     partial);
  const int st = launch_status(__func__);
  if (st) return st;
  const double count = 3.0 * (double)(height - (kSsimWin - 1)) * (double)(width - (kSsimWin - 1));
  hipLaunchKernelGGL(k_ssim_finish, (unsigned)n_images, kSsimThreads, 0, (hipStream_t)stream,
                     partial, tx * ty, count, ssim);
  return launch_status(__func__);
}
