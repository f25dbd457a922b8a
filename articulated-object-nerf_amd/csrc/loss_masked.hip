// The loss of a mask-supervised training step in one launch: the two levels' img2mse (over every
// ray, or over the foreground rays only: model_autodecoder.py:423-426, model_ae_art.py:380), the
// latent regulariser's add, and one of the reference's three opacity losses on the levels'
// accumulated opacity against the instance mask (model_autodecoder.py:703-766,
// model_ae_art.py:630-690), with the gradients of every term.
//
// opacity_loss_autorf is reproduced as the reference writes it, including what looks like a slip
// there: the FINE level's foreground term reads the COARSE opacity (model_autodecoder.py:761-763),
// so the coarse foreground opacity carries twice the weight and the fine one gets no gradient.
// Parity with the reference is the contract.
#include "aon_common.hpp"

#include <cmath>

namespace aon {

// One 256-thread workgroup (the inputs are a few thousand rays).  Pass 1 counts the foreground
// rays; pass 2 is k_loss_pair's sweep over the 3B colour values (train.hip: the same per-thread
// element order, fp64 accumulation, reduction tree and rounding when mask_rgb == 0); pass 3
// sweeps the B opacities, every term and gradient formed in fp64 and rounded to fp32 once.
// pred0 == NULL skips the colour terms (loss0 = loss1 = 0).
__global__ __launch_bounds__(256) void k_loss_masked(
    const float* __restrict__ pred0, const float* __restrict__ pred1,
    const float* __restrict__ acc0, const float* __restrict__ acc1,
    const float* __restrict__ target, const uint8_t* __restrict__ mask, int64_t B,
    const float* __restrict__ extra, int kind, double lambda, int mask_rgb,
    float* __restrict__ out, float* __restrict__ grad_rgb0, float* __restrict__ grad_rgb1,
    float* __restrict__ grad_acc0, float* __restrict__ grad_acc1) {
  __shared__ double part[5][256];
  __shared__ long long cnt[256];
  const int tid = threadIdx.x;
  constexpr int kU = 8;

  // pass 1: n_fg
  long long c = 0;
  for (int64_t i = tid; i < B; i += 256) c += mask[i] != 0;
  cnt[tid] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) cnt[tid] += cnt[tid + o];
    __syncthreads();
  }
  const int64_t n_fg = cnt[0], n_bg = B - n_fg;

  // pass 2: the colour terms
  double s0 = 0.0, s1 = 0.0;
  const int64_t n = 3 * B;
  if (pred0) {
    const int64_t n_rgb = mask_rgb ? 3 * n_fg : n;
    const float gscale = __fdiv_rn(2.0f, (float)n_rgb);
    for (int64_t i0 = tid; i0 < n; i0 += 256 * kU) {
      float p0[kU], p1[kU], q[kU];
      bool fg[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t i = i0 + 256 * u;
        p0[u] = i < n ? pred0[i] : 0.f;
        p1[u] = i < n ? pred1[i] : 0.f;
        q[u] = i < n ? target[i] : 0.f;
        fg[u] = !mask_rgb || (i < n && mask[i / 3] != 0);
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t i = i0 + 256 * u;
        if (i < n) {
          if (fg[u]) {
            const float d0 = __fsub_rn(p0[u], q[u]), d1 = __fsub_rn(p1[u], q[u]);
            s0 += (double)d0 * (double)d0;
            s1 += (double)d1 * (double)d1;
            grad_rgb0[i] = __fmul_rn(gscale, d0);
            grad_rgb1[i] = __fmul_rn(gscale, d1);
          } else {
            grad_rgb0[i] = 0.f;
            grad_rgb1[i] = 0.f;
          }
        }
      }
    }
  }

  // pass 3: the opacity term.  MSE / CE: t0, t1 = the levels' sums.  AutoRF: t0, t1 = the
  // background sums of acc0, acc1 and t2 = the foreground sum of 1 - acc0.
  double t0 = 0.0, t1 = 0.0, t2 = 0.0;
  if (kind != AON_OPACITY_NONE) {
    const double invB = 1.0 / (double)B;
    const double bg_ratio = (double)n_bg / (double)B, fg_ratio = (double)n_fg / (double)B;
    // AutoRF's constant gradients (n_bg, n_fg > 0 wherever they are stored)
    const float g_bg = (float)(bg_ratio / (double)n_bg);
    const float g_fg = (float)(-2.0 * fg_ratio / (double)n_fg);
    for (int64_t i0 = tid; i0 < B; i0 += 256 * kU) {
      float a0[kU], a1[kU];
      bool fg[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t i = i0 + 256 * u;
        a0[u] = i < B ? acc0[i] : 0.f;
        a1[u] = i < B ? acc1[i] : 0.f;
        fg[u] = i < B && mask[i] != 0;
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t i = i0 + 256 * u;
        if (i >= B) continue;
        const double m = fg[u] ? 1.0 : 0.0;
        if (kind == AON_OPACITY_MSE) {
          // (clamp(acc, 0, 1) - m)^2; the clamp passes the gradient on 0 <= acc <= 1
          const float x0 = a0[u], x1 = a1[u];
          const double d0 = (double)fminf(fmaxf(x0, 0.f), 1.f) - m;
          const double d1 = (double)fminf(fmaxf(x1, 0.f), 1.f) - m;
          t0 += d0 * d0;
          t1 += d1 * d1;
          grad_acc0[i] = (x0 >= 0.f && x0 <= 1.f) ? (float)(2.0 * d0 * invB) : 0.f;
          grad_acc1[i] = (x1 >= 0.f && x1 <= 1.f) ? (float)(2.0 * d1 * invB) : 0.f;
        } else if (kind == AON_OPACITY_CE) {
          // BCE with logits: max(x, 0) - x m + log1p(exp(-|x|)); d/dx = sigmoid(x) - m
          const double x0 = (double)a0[u], x1 = (double)a1[u];
          t0 += fmax(x0, 0.0) - x0 * m + log1p(exp(-fabs(x0)));
          t1 += fmax(x1, 0.0) - x1 * m + log1p(exp(-fabs(x1)));
          grad_acc0[i] = (float)(lambda * (1.0 / (1.0 + exp(-x0)) - m) * invB);
          grad_acc1[i] = (float)(lambda * (1.0 / (1.0 + exp(-x1)) - m) * invB);
        } else {  // AON_OPACITY_AUTORF
          if (fg[u]) {
            t2 += 1.0 - (double)a0[u];
            grad_acc0[i] = g_fg;
            grad_acc1[i] = 0.f;  // the reference's fine foreground term reads the coarse opacity
          } else {
            t0 += (double)a0[u];
            t1 += (double)a1[u];
            grad_acc0[i] = g_bg;
            grad_acc1[i] = g_bg;
          }
        }
      }
    }
  }

  part[0][tid] = s0;
  part[1][tid] = s1;
  part[2][tid] = t0;
  part[3][tid] = t1;
  part[4][tid] = t2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int k = 0; k < 5; ++k) part[k][tid] += part[k][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    float l0 = 0.f, l1 = 0.f;
    if (pred0) {
      // mask_rgb with no foreground ray: 0 / 0 = NaN, torch's mean of an empty selection
      const double n_rgb = (double)(mask_rgb ? 3 * n_fg : n);
      l0 = (float)(part[0][0] / n_rgb);
      l1 = (float)(part[1][0] / n_rgb);
    }
    double op = 0.0;
    if (kind == AON_OPACITY_MSE) {
      op = part[2][0] / (double)B + part[3][0] / (double)B;
    } else if (kind == AON_OPACITY_CE) {
      op = lambda * (part[2][0] / (double)B + part[3][0] / (double)B);
    } else if (kind == AON_OPACITY_AUTORF) {
      const double bg_ratio = (double)n_bg / (double)B, fg_ratio = (double)n_fg / (double)B;
      if (n_bg > 0)
        op += bg_ratio * (part[2][0] / (double)n_bg) + bg_ratio * (part[3][0] / (double)n_bg);
      if (n_fg > 0) op += 2.0 * fg_ratio * (part[4][0] / (double)n_fg);
    }
    const float lop = (float)op;
    float l = __fadd_rn(l1, l0);
    if (extra) l = __fadd_rn(l, *extra);
    if (kind != AON_OPACITY_NONE) l = __fadd_rn(l, lop);
    out[0] = l;
    out[1] = l0;
    out[2] = l1;
    out[3] = lop;
  }
}

// its backward: k_loss_pair_bwd's rule extended -- the colour gradients take g_loss + g_loss_i,
// the opacity gradients g_loss + g_opacity; absent (NULL) scalars count as 0, absent buffer
// pairs (no colour terms / no opacity term) are skipped
__global__ __launch_bounds__(256) void k_loss_masked_bwd(
    const float* __restrict__ grad_rgb0, const float* __restrict__ grad_rgb1,
    const float* __restrict__ grad_acc0, const float* __restrict__ grad_acc1, int64_t B,
    const float* __restrict__ g_loss, const float* __restrict__ g_loss0,
    const float* __restrict__ g_loss1, const float* __restrict__ g_opacity,
    float* __restrict__ d_rgb0, float* __restrict__ d_rgb1, float* __restrict__ d_acc0,
    float* __restrict__ d_acc1) {
  const float g = g_loss ? *g_loss : 0.f;
  const float a = g_loss0 ? (g_loss ? __fadd_rn(g, *g_loss0) : *g_loss0) : g;
  const float b = g_loss1 ? (g_loss ? __fadd_rn(g, *g_loss1) : *g_loss1) : g;
  const float c = g_opacity ? (g_loss ? __fadd_rn(g, *g_opacity) : *g_opacity) : g;
  const int64_t n = grad_rgb0 ? 3 * B : B;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (grad_rgb0) {
      d_rgb0[i] = __fmul_rn(grad_rgb0[i], a);
      d_rgb1[i] = __fmul_rn(grad_rgb1[i], b);
    }
    if (grad_acc0 && i < B) {
      d_acc0[i] = __fmul_rn(grad_acc0[i], c);
      d_acc1[i] = __fmul_rn(grad_acc1[i], c);
    }
  }
}

}  // namespace aon

using namespace aon;

extern "C" int aon_loss_masked(const float* pred0, const float* pred1, const float* acc0,
                               const float* acc1, const float* target, const uint8_t* mask,
                               int64_t B, const float* extra, int kind, double lambda,
                               int mask_rgb, float* out, float* grad_rgb0, float* grad_rgb1,
                               float* grad_acc0, float* grad_acc1, aon_stream_t stream) {
  AON_REQUIRE(acc0 && acc1 && mask && out, "null pointer");
  const bool rgb = pred0 || pred1 || target || grad_rgb0 || grad_rgb1;
  AON_REQUIRE(!rgb || (pred0 && pred1 && target && grad_rgb0 && grad_rgb1),
              "null pointer (the colour terms are skipped only when pred0, pred1, target, "
              "grad_rgb0 and grad_rgb1 are all NULL)");
  AON_REQUIRE(B >= 1 && B <= (int64_t)1 << 40, "bad ray count (B >= 1)");
  AON_REQUIRE(kind >= AON_OPACITY_NONE && kind <= AON_OPACITY_AUTORF, "bad opacity kind");
  AON_REQUIRE(kind == AON_OPACITY_NONE || (grad_acc0 && grad_acc1),
              "an opacity term needs grad_acc0 and grad_acc1");
  AON_REQUIRE(rgb || kind != AON_OPACITY_NONE, "nothing to compute");
  AON_REQUIRE(rgb || !mask_rgb, "mask_rgb without colour terms");
  hipLaunchKernelGGL(k_loss_masked, 1, 256, 0, (hipStream_t)stream, pred0, pred1, acc0, acc1,
                     target, mask, B, extra, kind, lambda, mask_rgb ? 1 : 0, out, grad_rgb0,
                     grad_rgb1, grad_acc0, grad_acc1);
  return launch_status(__func__);
}

extern "C" int aon_loss_masked_bwd(const float* grad_rgb0, const float* grad_rgb1,
                                   const float* grad_acc0, const float* grad_acc1, int64_t B,
                                   const float* g_loss, const float* g_loss0,
                                   const float* g_loss1, const float* g_opacity, float* d_rgb0,
                                   float* d_rgb1, float* d_acc0, float* d_acc1,
                                   aon_stream_t stream) {
  const bool rgb = grad_rgb0 || grad_rgb1 || d_rgb0 || d_rgb1;
  const bool acc = grad_acc0 || grad_acc1 || d_acc0 || d_acc1;
  AON_REQUIRE(!rgb || (grad_rgb0 && grad_rgb1 && d_rgb0 && d_rgb1),
              "null pointer (colour buffers: all four or none)");
  AON_REQUIRE(!acc || (grad_acc0 && grad_acc1 && d_acc0 && d_acc1),
              "null pointer (opacity buffers: all four or none)");
  AON_REQUIRE(rgb || acc, "null pointer");
  AON_REQUIRE(B >= 1 && B <= (int64_t)1 << 40, "bad ray count (B >= 1)");
  hipLaunchKernelGGL(k_loss_masked_bwd, grid_for(rgb ? 3 * B : B, 256, 1024), 256, 0,
                     (hipStream_t)stream, grad_rgb0, grad_rgb1, grad_acc0, grad_acc1, B, g_loss,
                     g_loss0, g_loss1, g_opacity, d_rgb0, d_rgb1, d_acc0, d_acc1);
  return launch_status(__func__);
}
