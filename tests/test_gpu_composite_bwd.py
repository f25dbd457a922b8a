"""The compositing backward (aon_composite_bwd, k_composite_bwd<NB> in csrc/train.hip) on its
own against autograd through the CPU oracle's volumetric_rendering (reference helper.py:157-195)
on the activations (model.py:186-187, model_autodecoder.py:321-323), evaluated in fp64 on the
same fp32 inputs: every 64-sample block count NB = 1..8 and both sides of each block boundary,
the three activations, both backgrounds, every presence pattern of g_acc / g_depth, both operand
layouts, rays that take the kernel's edge paths, the ray loop and determinism.

Error measure (as test_gpu_train.test_composite_backward): max |got - want| over a ray divided
by that ray's max |want|, separately for d raw_rgb and d raw_sigma, worst ray.  Gate:
err <= max(1e-5, 2 x env) with env the fp32 oracle's own distance from the fp64 oracle on the
same case, and env <= 1e-4 asserted so the gate cannot go slack.
"""
import functools

import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

B = 48
# every NB = ceil(S / 64) from 1 to 8, both sides of each block boundary
S_LIST = (1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 512)
ACT = {"none": 0, "vanilla": 1, "artic": 2}  # AON_ACT_*
SENTINEL = 7.0


@functools.lru_cache(maxsize=None)
def _inputs(S, act, n_rays=B, seed=1000):
    """fp32 inputs of one case (CPU).  dirs are not unit length (|d| in [0.2, 3]: the dnorm
    factor of D = dist * |d|).  With S >= 8 the first 24 rays take the kernel's edge paths:
      0..3   dirs = 0 (D = 0 everywhere, the last sample's 1e10 included);
      4..7   one duplicated t (dist 0);
      8..15  one opaque sample (raw sigma 400: f = 1e-10, the suffix recurrence keeps R finite)
             next to the ray's ends, mid-ray and on both sides of the first block boundary;
      16..19 raw sigma all -5 (relu: no density at all; softplus: a faint haze) -- not under
             ACT_NONE, where a negative density times the last sample's 1e10 is infinite in the
             reference too (the densities there are |randn|: already activated);
      20..23 one raw sigma of 25 (softplus's z > 20 branch under ACT_ARTIC)."""
    g = torch.Generator().manual_seed(seed + S)
    # t spans [2, 6] as in training; shorter for S < 40 so that one random sample's optical depth
    # sigma D stays below ~8: past that 1 - alpha cancels in fp32 and the reference's own fp32
    # evaluation leaves the envelope (opaque samples are the rays 8..15 below)
    t = torch.sort(2.0 + min(4.0, 0.1 * S) * torch.rand((n_rays, S), generator=g), -1).values
    raw_rgb = torch.randn((n_rays, S, 3), generator=g)
    raw_sig = torch.randn((n_rays, S, 1), generator=g) * 2
    dirs = torch.nn.functional.normalize(torch.randn((n_rays, 3), generator=g), dim=-1)
    dirs = dirs * (0.2 + 2.8 * torch.rand((n_rays, 1), generator=g))
    g_rgb = torch.randn((n_rays, 3), generator=g) * 1e-2
    g_acc = torch.randn((n_rays,), generator=g) * 1e-2
    g_depth = torch.randn((n_rays,), generator=g) * 1e-2
    if act == "none":
        raw_sig = raw_sig.abs()
    if S >= 8 and n_rays >= 24:
        dirs[0:4] = 0.0
        for r in range(4, 8):
            k = S // 3 + r - 4
            t[r, k + 1] = t[r, k]
        opaque = (1, S // 4, S // 2 - 1, S // 2, 63 if S > 65 else S // 3,
                  64 if S > 66 else 2 * S // 3, S - 3, S - 2)
        for r, k in zip(range(8, 16), opaque):
            raw_sig[r, k] = 400.0
            # a true wall: D >= 0.15, so exp(-400 D) is far below the 1e-10 of f in fp64 too
            t[r, k + 1:] += 0.3
            dirs[r] *= max(1.0, 0.5 / dirs[r].norm().item())
        if act != "none":
            raw_sig[16:20] = -5.0
        for r in range(20, 24):
            raw_sig[r, S // 2 + r - 20] = 25.0
    return dict(t=t, raw_rgb=raw_rgb, raw_sig=raw_sig, dirs=dirs, g_rgb=g_rgb, g_acc=g_acc,
                g_depth=g_depth)


def _reference(inp, act, white, use_acc, use_depth, dtype):
    """(d raw_rgb, d raw_sigma) of sum(comp g_rgb) + sum(acc g_acc) + sum(depth g_depth) by
    autograd through the oracle in ``dtype``."""
    c = {k: v.to(dtype) for k, v in inp.items()}
    rr = c["raw_rgb"].clone().requires_grad_(True)
    rs = c["raw_sig"].clone().requires_grad_(True)
    if act == "none":
        rgb, sigma = rr, rs
    elif act == "vanilla":
        rgb, sigma = torch.sigmoid(rr), torch.relu(rs)
    else:
        rgb, sigma = O.art_activations(rr, rs)
    comp, acc, _, depth = O.volumetric_rendering(rgb, sigma, c["t"], c["dirs"], white)
    loss = (comp * c["g_rgb"]).sum()
    if use_acc:
        loss = loss + (acc * c["g_acc"]).sum()
    if use_depth:
        loss = loss + (depth * c["g_depth"]).sum()
    loss.backward()
    return rr.grad.double(), rs.grad.double()


def _ray_err(got, want):
    scale = want.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-12)
    return ((got.double() - want).abs() / scale).max().item()


@functools.lru_cache(maxsize=None)
def _case(S, act, white, use_acc, use_depth, n_rays=B):
    """The fp64 gradients of one case and the fp32 oracle's distance from them (the envelope),
    (want_rgb, want_sigma, env_rgb, env_sigma); the condition env <= 1e-4 is checked here."""
    inp = _inputs(S, act, n_rays)
    w_rgb, w_sig = _reference(inp, act, white, use_acc, use_depth, torch.float64)
    f_rgb, f_sig = _reference(inp, act, white, use_acc, use_depth, torch.float32)
    assert torch.isfinite(w_rgb).all() and torch.isfinite(w_sig).all(), (S, act)
    env = (_ray_err(f_rgb, w_rgb), _ray_err(f_sig, w_sig))
    assert max(env) <= 1e-4, (S, act, white, use_acc, use_depth, env)
    return w_rgb, w_sig, env[0], env[1]


@functools.lru_cache(maxsize=None)
def _device_inputs(S, act, n_rays=B, seed=1000):
    return {k: v.cuda().contiguous() for k, v in _inputs(S, act, n_rays, seed).items()}


def _launch(d_in, n_rays, S, act, white, use_acc, use_depth, layout, r0=0, r1=None):
    """aon_composite_bwd on rays r0..r1 of the device inputs -> (d raw_rgb (n, S, 3), d raw_sigma
    (n, S, 1)).  layout "raw4": [r, g, b, sigma] rows in, d_stride 4 out (pre-filled with NaN:
    every element must be written); "split": rgb (stride 3) and sigma (stride 1) apart, the
    output padded to d_stride 6 with columns 4, 5 holding a sentinel that must survive."""
    from aonerf import _lib as L

    r1 = n_rays if r1 is None else r1
    n = r1 - r0
    rgb = d_in["raw_rgb"][r0:r1].reshape(-1, 3)
    sig = d_in["raw_sig"][r0:r1].reshape(-1, 1)
    if layout == "raw4":
        raw = torch.cat([rgb, sig], -1).contiguous()
        p_rgb, s_rgb, p_sig, s_sig = raw, 4, raw[:, 3:], 4
        d = torch.full((n * S, 4), float("nan"), device="cuda")
    else:
        rgb, sig = rgb.contiguous(), sig.contiguous()
        p_rgb, s_rgb, p_sig, s_sig = rgb, 3, sig, 1
        d = torch.full((n * S, 6), SENTINEL, device="cuda")
    ga = d_in["g_acc"][r0:r1] if use_acc else None
    gd = d_in["g_depth"][r0:r1] if use_depth else None
    L.call("aon_composite_bwd", L.ptr(p_rgb), s_rgb, L.ptr(p_sig), s_sig, L.ptr(d_in["t"][r0:r1]),
           L.ptr(d_in["dirs"][r0:r1]), n, S, int(white), ACT[act], L.ptr(d_in["g_rgb"][r0:r1]),
           L.ptr(ga), L.ptr(gd), L.ptr(d), L.ptr(d[:, 3:]), d.shape[1], L.stream())
    torch.cuda.synchronize()
    if layout == "split":
        assert bool((d[:, 4:] == SENTINEL).all()), "padding columns of d were written"
    return d[:, :3].reshape(n, S, 3), d[:, 3:4].reshape(n, S, 1)


@pytest.mark.parametrize("use_acc,use_depth", [(False, False), (True, False), (False, True),
                                               (True, True)],
                         ids=["rgb_only", "g_acc", "g_depth", "g_acc_g_depth"])
@pytest.mark.parametrize("white", [0, 1])
@pytest.mark.parametrize("act", ["none", "vanilla", "artic"])
def test_composite_backward_sample_counts(act, white, use_acc, use_depth):
    """Every S of S_LIST, both layouts, 48 rays with the edge rays of _inputs: the kernel within
    max(1e-5, 2 x env) of the fp64 oracle per ray, env <= 1e-4, the padded output's sentinel
    columns untouched, a second launch bit-equal.

    Measured worst kernel error over all S, backgrounds and g patterns (MI355X), rgb / sigma,
    with the fp32 oracle's own envelope on the same cases:
      ACT_NONE     9.4e-07 / 1.9e-06   (envelope 9.4e-07 / 2.7e-06)
      ACT_VANILLA  1.9e-06 / 5.2e-06   (envelope 1.9e-06 / 3.8e-06)
      ACT_ARTIC    1.1e-06 / 7.0e-06   (envelope 1.1e-06 / 6.0e-06)
    The rgb error is the fp32 rounding of the inputs' own products (kernel and fp32 oracle
    agree); the envelope's worst case is S = 2.
    """
    worst = [0.0, 0.0, 0.0, 0.0]
    for S in S_LIST:
        w_rgb, w_sig, env_rgb, env_sig = _case(S, act, bool(white), use_acc, use_depth)
        d_in = _device_inputs(S, act)
        for layout in ("raw4", "split"):
            g_rgb, g_sig = _launch(d_in, B, S, act, white, use_acc, use_depth, layout)
            g_rgb2, g_sig2 = _launch(d_in, B, S, act, white, use_acc, use_depth, layout)
            assert torch.equal(g_rgb, g_rgb2) and torch.equal(g_sig, g_sig2), (S, layout)
            e_rgb, e_sig = _ray_err(g_rgb.cpu(), w_rgb), _ray_err(g_sig.cpu(), w_sig)
            print(f"composite bwd act={act} white={white} acc={int(use_acc)} depth={int(use_depth)} "
                  f"S={S} {layout}: rgb {e_rgb:.2e} (env {env_rgb:.2e}) sigma {e_sig:.2e} "
                  f"(env {env_sig:.2e})")
            worst = [max(a, b) for a, b in zip(worst, (e_rgb, e_sig, env_rgb, env_sig))]
            assert e_rgb <= max(1e-5, 2 * env_rgb), (S, layout, "rgb", e_rgb, env_rgb)
            assert e_sig <= max(1e-5, 2 * env_sig), (S, layout, "sigma", e_sig, env_sig)
    print(f"composite bwd act={act} white={white} acc={int(use_acc)} depth={int(use_depth)} worst: "
          f"rgb {worst[0]:.2e} sigma {worst[1]:.2e} (env rgb {worst[2]:.2e} sigma {worst[3]:.2e})")


@pytest.mark.parametrize("act", ["none", "vanilla", "artic"])
def test_composite_backward_ray_loop(act):
    """270,000 rays at S = 3: the grid caps at 65,536 workgroups of 4 waves, so 7,856 waves take
    a second ray.  The one launch equals launches of 900-ray chunks bit for bit, every output is
    finite, and its first 256 rays pass the gate of the sample-count test (white background,
    g_acc and g_depth present).

    Measured (MI355X), rgb / sigma:
      ACT_NONE     1.6e-07 / 2.6e-06   (envelope 1.6e-07 / 2.7e-06)
      ACT_VANILLA  6.2e-06 / 8.2e-06   (envelope 6.2e-06 / 8.3e-06)
      ACT_ARTIC    5.3e-07 / 3.2e-05   (envelope 4.4e-07 / 4.0e-05)
    """
    n, S, chunk = 270000, 3, 900
    # a seed at which the reference's own fp32 evaluation of the first 256 rays meets the 1e-4
    # condition (at S = 3 a ray whose only lit sample sits in front of a like-coloured last
    # sample cancels in q_i - R_{i+1}: one such ray in 256 puts the fp32 oracle at 1.6e-4)
    seed = 3000
    d_in = _device_inputs(S, act, n, seed)
    full_rgb, full_sig = _launch(d_in, n, S, act, 1, True, True, "raw4")
    assert torch.isfinite(full_rgb).all() and torch.isfinite(full_sig).all()
    for layout in ("raw4", "split"):
        parts = [_launch(d_in, n, S, act, 1, True, True, layout, r0, r0 + chunk)
                 for r0 in range(0, n, chunk)]
        assert torch.equal(full_rgb, torch.cat([p[0] for p in parts])), layout
        assert torch.equal(full_sig, torch.cat([p[1] for p in parts])), layout
    head = {k: v[:256] for k, v in _inputs(S, act, n, seed).items()}
    w_rgb, w_sig = _reference(head, act, True, True, True, torch.float64)
    f_rgb, f_sig = _reference(head, act, True, True, True, torch.float32)
    env_rgb, env_sig = _ray_err(f_rgb, w_rgb), _ray_err(f_sig, w_sig)
    assert max(env_rgb, env_sig) <= 1e-4, (env_rgb, env_sig)
    e_rgb, e_sig = _ray_err(full_rgb[:256].cpu(), w_rgb), _ray_err(full_sig[:256].cpu(), w_sig)
    print(f"composite bwd ray loop act={act}: rgb {e_rgb:.2e} (env {env_rgb:.2e}) "
          f"sigma {e_sig:.2e} (env {env_sig:.2e})")
    assert e_rgb <= max(1e-5, 2 * env_rgb) and e_sig <= max(1e-5, 2 * env_sig)
