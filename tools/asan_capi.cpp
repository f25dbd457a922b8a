// Host-side AddressSanitizer driver for the C ABI (the "-fsanitize=address
// debug build" of the host code).  Built by `make asan` (csrc/Makefile) against
// lib/asan/libaonerf_asan.so, whose host code -- argument validation, size queries, the error
// plumbing, packing tables -- is compiled with -fsanitize=address (host-only objects: no device
// code, so nothing here may launch a kernel).  Every call below must fail argument validation
// BEFORE touching the GPU and report it through aon_last_error(); ASan aborts the process on
// any out-of-bounds or use-after-free on the way.
#include <cstdio>
#include <cstring>

#include "aonerf.h"

static int failures = 0;

static void expect_invalid(int rc, const char* what) {
  const char* msg = aon_last_error();
  if (rc >= 0 || !msg || !msg[0]) {
    std::printf("FAIL %s: rc=%d msg=%s\n", what, rc, msg ? msg : "(null)");
    ++failures;
  } else {
    std::printf("ok   %s -> %s\n", what, msg);
  }
}

int main() {
  if (aon_abi_version() != AON_ABI_VERSION) {
    std::printf("FAIL abi version\n");
    return 1;
  }
  float c2w[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4};
  float dummy[16];
  void* p = dummy;
  expect_invalid(aon_ray_directions(0, 4, 1.f, dummy, nullptr), "ray_directions H=0");
  expect_invalid(aon_get_rays(nullptr, 4, c2w, dummy, dummy, nullptr, 0, 0, nullptr, nullptr),
                 "get_rays null dirs");
  expect_invalid(aon_get_rays(dummy, 4, c2w, dummy, dummy, nullptr, 2, 2, dummy, nullptr),
                 "get_rays radii H=2");
  expect_invalid(aon_frame_rays(4, 4, 1.f, nullptr, 0, 16, dummy, dummy, nullptr, nullptr),
                 "frame_rays null c2w");
  expect_invalid(aon_sample_pdf(nullptr, 0, dummy, 4, 4, 1000, 128, dummy, 0, nullptr, 0, nullptr,
                                nullptr, dummy, nullptr, nullptr),
                 "sample_pdf nb > 256");
  expect_invalid(aon_composite_march(dummy + 1, dummy, dummy, 4, 65, 1, 0, dummy, 0, 128, dummy,
                                     dummy, nullptr, dummy, dummy, nullptr),
                 "composite_march misaligned raw");
  expect_invalid(aon_composite_march(dummy, dummy, dummy, 4, 300, 1, 0, dummy, 0, 128, dummy,
                                     dummy, nullptr, dummy, dummy, nullptr),
                 "composite_march S > 256");
  expect_invalid(aon_composite_fwd(dummy, 2, dummy, 1, dummy, dummy, 4, 8, 1, 0, dummy, dummy,
                                   nullptr, dummy, nullptr),
                 "composite_fwd rgb_stride < 3");
  expect_invalid(aon_composite_feat(dummy, dummy, 4, 9, 4, 8, dummy, nullptr), "composite_feat C = 9");
  expect_invalid(aon_composite_feat(dummy, dummy, 4, 3, 4, 513, dummy, nullptr),
                 "composite_feat S = 513");
  expect_invalid(aon_composite_feat(dummy, dummy, 2, 3, 4, 8, dummy, nullptr),
                 "composite_feat feat_stride < C");
  expect_invalid(aon_composite_feat(dummy, nullptr, 4, 3, 4, 8, dummy, nullptr),
                 "composite_feat null feat");
  expect_invalid(aon_mlp_art_fwd_deform(p, dummy, dummy, dummy, 4, 8, nullptr, nullptr, nullptr),
                 "art_fwd_deform no output");
  expect_invalid(aon_mlp_art_fwd_deform(p, dummy, dummy, dummy, 4, 0, dummy, dummy, nullptr),
                 "art_fwd_deform S = 0");
  expect_invalid(aon_mlp_art_fwd_deform(p, dummy, nullptr, dummy, 4, 8, dummy, dummy, nullptr),
                 "art_fwd_deform null rays_d");
  expect_invalid(aon_mlp_art_fwd_deform_points(p, nullptr, 4, dummy, dummy, nullptr),
                 "art_fwd_deform_points null pos");
  expect_invalid(aon_mlp_art_fwd_deform_points(p, dummy, -1, dummy, dummy, nullptr),
                 "art_fwd_deform_points N < 0");
  expect_invalid(aon_mlp_art_fwd_sigma(p, dummy, dummy, dummy, 4, 8, 0, nullptr, nullptr),
                 "art_fwd_sigma null out");
  expect_invalid(aon_mlp_art_fwd_sigma(p, dummy, dummy, dummy, 4, 0, 0, dummy, nullptr),
                 "art_fwd_sigma S = 0");
  expect_invalid(aon_mlp_art_fwd_sigma(p, dummy, dummy, dummy, 4, 8, 3, dummy, nullptr),
                 "art_fwd_sigma bad act");
  expect_invalid(aon_mlp_art_fwd_sigma_points(p, nullptr, 4, 0, dummy, nullptr),
                 "art_fwd_sigma_points null pos");
  expect_invalid(aon_mlp_art_fwd_sigma_points(p, dummy, -1, 0, dummy, nullptr),
                 "art_fwd_sigma_points N < 0");
  expect_invalid(aon_mlp_pack(nullptr, AON_PREC_F16X3, p, nullptr), "mlp_pack null params");
  aon_mlp_params prm;
  std::memset(&prm, 0, sizeof(prm));
  expect_invalid(aon_mlp_pack(&prm, 7, p, nullptr), "mlp_pack bad precision");
  expect_invalid(aon_mlp_pack(&prm, AON_PREC_F16X3, p, nullptr), "mlp_pack no shapes");
  // the default geometry's shapes (ABI 9), null tensors: refused by the null check, no launch
  const int64_t shp[12][2] = {{256, 63},  {256, 256}, {256, 256}, {256, 256}, {256, 256}, {256, 319},
                              {256, 256}, {256, 256}, {1, 256},   {256, 256}, {128, 283}, {3, 128}};
  for (int i = 0; i < 12; ++i) {
    prm.w_rows[i] = shp[i][0];
    prm.w_cols[i] = shp[i][1];
    prm.b_len[i] = shp[i][0];
  }
  expect_invalid(aon_mlp_pack(&prm, AON_PREC_F16X3, p, nullptr), "mlp_pack null layer");
  // registration order (views_linear.0 in the density slot): refused by the shape check
  prm.w_rows[8] = 128;
  prm.w_cols[8] = 283;
  prm.b_len[8] = 128;
  expect_invalid(aon_mlp_pack(&prm, AON_PREC_F16X3, p, nullptr), "mlp_pack registration order");
  expect_invalid(aon_mlp_bwd_pack(&prm, p, nullptr), "mlp_bwd_pack registration order");
  aon_mlp_art_params aprm;
  std::memset(&aprm, 0, sizeof(aprm));
  expect_invalid(aon_mlp_art_pack(&aprm, p, nullptr), "mlp_art_pack no shapes");
  expect_invalid(aon_mlp_art_bwd_pack(&aprm, p, nullptr), "mlp_art_bwd_pack no shapes");
  uint32_t st = 0;
  expect_invalid(aon_mlp_read_status(p, 3, &st, nullptr), "read_status bad size");
  aon_gemm_args g;
  std::memset(&g, 0, sizeof(g));
  g.M = g.N = g.K = 16;
  g.A = g.B = dummy;
  g.C = dummy;
  g.lda = g.ldb = 16;
  g.a_kc = g.b_kc = 1;
  g.ldc = 8;  // < N
  g.a_scale = g.b_scale = 1.f;
  expect_invalid(aon_gemm(&g, nullptr, 0, nullptr), "gemm ldc < N");
  g.ldc = 16;
  g.a_scale = 0.f;
  expect_invalid(aon_gemm(&g, nullptr, 0, nullptr), "gemm zero scale");
  aon_adam_tensor t;
  std::memset(&t, 0, sizeof(t));
  expect_invalid(aon_adam_step(&t, 0, 1e-3, 0.9, 0.999, 1e-8, 1, nullptr), "adam count 0");
  // aon_image_ssim: every refusal happens before the first launch; zero images is a no-op that
  // does not look at the pointers
  const size_t ssim_ws = aon_ssim_workspace_bytes(2, 24, 32);
  expect_invalid(aon_image_ssim(nullptr, dummy, 2, 24, 32, dummy, nullptr, p, ssim_ws, nullptr),
                 "image_ssim null pred");
  expect_invalid(aon_image_ssim(dummy, nullptr, 2, 24, 32, dummy, nullptr, p, ssim_ws, nullptr),
                 "image_ssim null gt");
  expect_invalid(aon_image_ssim(dummy, dummy, 2, 24, 32, nullptr, nullptr, p, ssim_ws, nullptr),
                 "image_ssim null ssim");
  expect_invalid(aon_image_ssim(dummy, dummy, 2, 24, 32, dummy, nullptr, nullptr, ssim_ws, nullptr),
                 "image_ssim null work");
  expect_invalid(aon_image_ssim(dummy, dummy, 2, 10, 32, dummy, nullptr, p, ssim_ws, nullptr),
                 "image_ssim height < 11");
  expect_invalid(aon_image_ssim(dummy, dummy, 2, 24, 10, dummy, nullptr, p, ssim_ws, nullptr),
                 "image_ssim width < 11");
  expect_invalid(aon_image_ssim(dummy, dummy, -1, 24, 32, dummy, nullptr, p, ssim_ws, nullptr),
                 "image_ssim negative count");
  expect_invalid(aon_image_ssim(dummy, dummy, 2, -24, 32, dummy, nullptr, p, ssim_ws, nullptr),
                 "image_ssim negative height");
  expect_invalid(aon_image_ssim(dummy, dummy, 2, 24, 32, dummy, nullptr, p, ssim_ws - 1, nullptr),
                 "image_ssim work_bytes too small");
  expect_invalid(aon_image_ssim(dummy, dummy, 70000, 24, 32, dummy, nullptr, p, ~(size_t)0, nullptr),
                 "image_ssim image count past the grid");
  expect_invalid(aon_image_ssim(dummy, dummy, 1, 4000000, 32, dummy, nullptr, p, ~(size_t)0, nullptr),
                 "image_ssim tile rows past the grid");
  if (aon_image_ssim(nullptr, nullptr, 0, 24, 32, nullptr, nullptr, nullptr, 0, nullptr) != 0) {
    std::printf("FAIL image_ssim zero images\n");
    ++failures;
  }
  if (ssim_ws == 0 || aon_ssim_workspace_bytes(3, 24, 32) < ssim_ws ||
      aon_ssim_workspace_bytes(0, 24, 32) == 0 || aon_ssim_workspace_bytes(2, 10, 32) != 0 ||
      aon_ssim_workspace_bytes(-1, 24, 32) != 0 || aon_ssim_tile[0] < 1 || aon_ssim_tile[1] < 1) {
    std::printf("FAIL ssim workspace query\n");
    ++failures;
  }
  // aon_loss_masked / aon_loss_masked_bwd: null pointers, B, kind and the buffers a kind needs
  const uint8_t* mk = reinterpret_cast<const uint8_t*>(dummy);
  expect_invalid(aon_loss_masked(dummy, dummy, nullptr, dummy, dummy, mk, 4, nullptr,
                                 AON_OPACITY_MSE, 0.05, 0, dummy, dummy, dummy, dummy, dummy, nullptr),
                 "loss_masked null acc0");
  expect_invalid(aon_loss_masked(dummy, dummy, dummy, dummy, dummy, nullptr, 4, nullptr,
                                 AON_OPACITY_MSE, 0.05, 0, dummy, dummy, dummy, dummy, dummy, nullptr),
                 "loss_masked null mask");
  expect_invalid(aon_loss_masked(dummy, nullptr, dummy, dummy, dummy, mk, 4, nullptr,
                                 AON_OPACITY_MSE, 0.05, 0, dummy, dummy, dummy, dummy, dummy, nullptr),
                 "loss_masked null pred1 alone");
  expect_invalid(aon_loss_masked(dummy, dummy, dummy, dummy, dummy, mk, 0, nullptr,
                                 AON_OPACITY_MSE, 0.05, 0, dummy, dummy, dummy, dummy, dummy, nullptr),
                 "loss_masked B=0");
  expect_invalid(aon_loss_masked(dummy, dummy, dummy, dummy, dummy, mk, 4, nullptr, 4, 0.05, 0,
                                 dummy, dummy, dummy, dummy, dummy, nullptr),
                 "loss_masked kind out of range");
  expect_invalid(aon_loss_masked(dummy, dummy, dummy, dummy, dummy, mk, 4, nullptr,
                                 AON_OPACITY_CE, 0.05, 0, dummy, dummy, dummy, nullptr, dummy, nullptr),
                 "loss_masked CE without grad_acc0");
  expect_invalid(aon_loss_masked(nullptr, nullptr, dummy, dummy, nullptr, mk, 4, nullptr,
                                 AON_OPACITY_NONE, 0.05, 0, dummy, nullptr, nullptr, nullptr, nullptr,
                                 nullptr),
                 "loss_masked nothing to compute");
  expect_invalid(aon_loss_masked_bwd(dummy, dummy, dummy, dummy, 4, dummy, nullptr, nullptr, nullptr,
                                     dummy, nullptr, dummy, dummy, nullptr),
                 "loss_masked_bwd null d_rgb1");
  expect_invalid(aon_loss_masked_bwd(nullptr, nullptr, nullptr, nullptr, 4, dummy, nullptr, nullptr,
                                     nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
                 "loss_masked_bwd no buffers");
  expect_invalid(aon_loss_masked_bwd(dummy, dummy, dummy, dummy, 0, dummy, nullptr, nullptr, nullptr,
                                     dummy, dummy, dummy, dummy, nullptr),
                 "loss_masked_bwd B=0");
  // box bounds: null pointers, B < 0, S < 2 and a non-positive half_side, all before any launch
  int32_t* ip = reinterpret_cast<int32_t*>(dummy);
  const size_t lim_ws = aon_ray_limits_workspace_bytes(4), cmp_ws = aon_compact_rays_workspace_bytes(4);
  expect_invalid(aon_ray_limits_box(nullptr, dummy, 4, 1.f, dummy, dummy, nullptr),
                 "ray_limits_box null rays_o");
  expect_invalid(aon_ray_limits_box(dummy, dummy, 4, 1.f, dummy, nullptr, nullptr),
                 "ray_limits_box null tmax");
  expect_invalid(aon_ray_limits_box(dummy, dummy, -1, 1.f, dummy, dummy, nullptr),
                 "ray_limits_box B < 0");
  expect_invalid(aon_ray_limits_box(dummy, dummy, 4, 0.f, dummy, dummy, nullptr),
                 "ray_limits_box half_side 0");
  expect_invalid(aon_ray_limits(dummy, nullptr, 4, 1.f, dummy, dummy, p, lim_ws, nullptr),
                 "ray_limits null rays_d");
  expect_invalid(aon_ray_limits(dummy, dummy, 4, 1.f, dummy, dummy, nullptr, lim_ws, nullptr),
                 "ray_limits null work");
  expect_invalid(aon_ray_limits(dummy, dummy, -1, 1.f, dummy, dummy, p, lim_ws, nullptr),
                 "ray_limits B < 0");
  expect_invalid(aon_ray_limits(dummy, dummy, 4, -1.f, dummy, dummy, p, lim_ws, nullptr),
                 "ray_limits half_side < 0");
  expect_invalid(aon_ray_limits(dummy, dummy, 4, 1.f, dummy, dummy, p, lim_ws - 1, nullptr),
                 "ray_limits work_bytes too small");
  expect_invalid(aon_sample_along_rays_bounds(dummy, dummy, 4, 8, nullptr, dummy, dummy, 0, nullptr,
                                              dummy, nullptr, nullptr),
                 "sample_along_rays_bounds null s_tab");
  expect_invalid(aon_sample_along_rays_bounds(dummy, dummy, 4, 8, dummy, nullptr, dummy, 0, nullptr,
                                              dummy, nullptr, nullptr),
                 "sample_along_rays_bounds null near");
  expect_invalid(aon_sample_along_rays_bounds(dummy, dummy, -1, 8, dummy, dummy, dummy, 0, nullptr,
                                              dummy, nullptr, nullptr),
                 "sample_along_rays_bounds B < 0");
  expect_invalid(aon_sample_along_rays_bounds(dummy, dummy, 4, 1, dummy, dummy, dummy, 0, nullptr,
                                              dummy, nullptr, nullptr),
                 "sample_along_rays_bounds S < 2");
  expect_invalid(aon_sample_along_rays_bounds(nullptr, dummy, 4, 8, dummy, dummy, dummy, 0, nullptr,
                                              dummy, dummy, nullptr),
                 "sample_along_rays_bounds xyz without rays_o");
  expect_invalid(aon_compact_rays(nullptr, dummy, dummy, dummy, dummy, 4, ip, ip, dummy, dummy, dummy,
                                  dummy, dummy, ip, p, cmp_ws, nullptr),
                 "compact_rays null tmin");
  expect_invalid(aon_compact_rays(dummy, dummy, dummy, dummy, dummy, 4, ip, ip, dummy, dummy, dummy,
                                  dummy, dummy, nullptr, p, cmp_ws, nullptr),
                 "compact_rays null n_hit");
  expect_invalid(aon_compact_rays(dummy, dummy, dummy, dummy, dummy, 4, ip, ip, dummy, dummy, nullptr,
                                  dummy, dummy, ip, p, cmp_ws, nullptr),
                 "compact_rays viewdirs without v_out");
  expect_invalid(aon_compact_rays(dummy, dummy, dummy, dummy, dummy, -1, ip, ip, dummy, dummy, dummy,
                                  dummy, dummy, ip, p, cmp_ws, nullptr),
                 "compact_rays B < 0");
  expect_invalid(aon_compact_rays(dummy, dummy, dummy, dummy, dummy, 4, ip, ip, dummy, dummy, dummy,
                                  dummy, dummy, ip, p, cmp_ws - 1, nullptr),
                 "compact_rays work_bytes too small");
  expect_invalid(aon_scatter_payload(dummy, dummy, dummy, 2, nullptr, 4, 1, dummy, nullptr),
                 "scatter_payload null slot");
  expect_invalid(aon_scatter_payload(nullptr, dummy, dummy, 2, ip, 4, 1, dummy, nullptr),
                 "scatter_payload null comp");
  expect_invalid(aon_scatter_payload(dummy, dummy, dummy, 2, ip, -1, 1, dummy, nullptr),
                 "scatter_payload B < 0");
  if (lim_ws == 0 || cmp_ws == 0 || aon_ray_limits_workspace_bytes(-1) != 0 ||
      aon_compact_rays_workspace_bytes(-1) != 0 ||
      aon_ray_limits_workspace_bytes(257) <= aon_ray_limits_workspace_bytes(256) ||
      aon_compact_rays_workspace_bytes(257) <= aon_compact_rays_workspace_bytes(256)) {
    std::printf("FAIL box bounds workspace queries\n");
    ++failures;
  }
  // size queries: pure host arithmetic
  if (aon_mlp_packed_bytes(AON_PREC_F16X3) == 0 || aon_mlp_bwd_packed_bytes() == 0 ||
      aon_mlp_art_packed_bytes() == 0 || aon_colsum_workspace_bytes(1024, 256) == 0) {
    std::printf("FAIL size queries\n");
    ++failures;
  }
  std::printf("%s: %d failures\n", failures ? "FAILED" : "ASAN_CAPI_OK", failures);
  return failures ? 1 : 0;
}
