"""The articulated density-only pass (include/aonerf.h aon_mlp_art_fwd_sigma[_points],
csrc/mlp_art_sigma.hip) and what is built on it: NeRFMLP.forward_sigma / density,
NeRF_AE_Art.forward(fine_only=True), ``latents=`` on aonerf.render, the vanilla NeRFMLP.density
and aonerf.geometry.density_grid.

The pass is a prefix of the full kernel (k_mlp_art_f16x3) on a prefix of the same packed stream:
it removes work and leaves every kept bit where it was.  So every check here is ``torch.equal``
against the full kernel or the one-pass forward: there is no tolerance anywhere."""
import functools
import warnings

import numpy as np
import pytest
import torch

from oracle import weights as W

pytestmark = pytest.mark.gpu

# tests/test_gpu_sigma_only.py's: one row; tiles spanning several rays; one row short of / past a
# 128-row workgroup; several workgroups with a ragged last tile
SHAPES = [(1, 1), (13, 5), (1, 127), (1, 129), (3, 65), (7, 193)]
GUARD = 256       # rows behind the output that no launch may touch
SENTINEL = -777.0


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def load(net, sd):
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.requires_grad_(False)


def make_net(sd=None, **kw):
    from aonerf.model_autodecoder import NeRF_AE_Art

    return load(NeRF_AE_Art(**kw).cuda(), W.art_state_dict(0) if sd is None else sd)


@functools.lru_cache(maxsize=None)
def _golden():
    """NeRF_AE_Art on the golden weights and latent codes; never edited (the range tests build
    their own)."""
    return make_net(), {k: cuda(v) for k, v in W.art_latents(1).items()}


def rays_of(B, S, seed=7):
    """(o, d, v, t) on the GPU: |o| <= 0.5, unit d, view directions independent of d, sorted t in
    [2, 6]."""
    gen = torch.Generator().manual_seed(seed + 131 * B + S)
    o = torch.rand(B, 3, generator=gen) - 0.5
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1)
    v = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1)
    t = (2.0 + 4.0 * torch.rand(B, S, generator=gen)).sort(-1).values
    return o.cuda(), d.cuda(), v.cuda(), t.cuda()


def guarded(N):
    buf = torch.full((N + GUARD, 4), SENTINEL, device="cuda")
    return buf, buf[:N]


def status(pack):
    from aonerf import _lib as L

    return int(L.status_word(pack))


def full_rays(pack, o, d, v, t, act):
    from aonerf import _lib as L

    B, S = t.shape
    raw = torch.empty((B * S, 4), device="cuda")
    L.call("aon_mlp_art_fwd", L.ptr(pack), L.ptr(o), L.ptr(d), L.ptr(v), L.ptr(t), B, S, act,
           L.ptr(raw), L.stream(t.device))
    return raw


def sigma_rays(pack, o, d, t, act, out):
    from aonerf import _lib as L

    B, S = t.shape
    L.call("aon_mlp_art_fwd_sigma", L.ptr(pack), L.ptr(o), L.ptr(d), L.ptr(t), B, S, act,
           L.ptr(out), L.stream(t.device))


# ---------------------------------------------------------------------------- 1. rays, bitwise
@pytest.mark.parametrize("level", ["coarse", "fine"])
@pytest.mark.parametrize("act", [0, 2], ids=["act_none", "act_artic"])
@pytest.mark.parametrize("B,S", SHAPES)
def test_sigma_equals_the_full_kernels_sigma(B, S, act, level):
    from aonerf import _lib as L

    assert (L.ACT_NONE, L.ACT_ARTIC) == (0, 2)
    net, lat = _golden()
    mlp = getattr(net, f"{level}_mlp")
    o, d, v, t = rays_of(B, S)
    N = B * S
    pack = mlp.packed_weights(lat)
    ref = full_rays(pack, o, d, v, t, act)
    assert torch.isfinite(ref).all()
    buf, out = guarded(N)
    sigma_rays(pack, o, d, t, act, buf)
    torch.cuda.synchronize()
    assert torch.equal(out[:, 3], ref[:, 3])
    assert torch.equal(out[:, :3], torch.zeros((N, 3), device="cuda"))
    assert torch.equal(buf[N:], torch.full((GUARD, 4), SENTINEL, device="cuda")), "rows past B*S written"
    assert status(pack) == 0
    # NeRFMLP.forward_sigma is this entry point (on its own pack of the same weights and codes)
    assert torch.equal(mlp.forward_sigma(o, d, t, lat, act=act), out)


# ---------------------------------------------------------------------------- 2. points, bitwise
@pytest.mark.parametrize("act", [0, 2], ids=["act_none", "act_artic"])
@pytest.mark.parametrize("N", [1, 127, 129, 1351])
def test_sigma_points_equals_the_full_kernels_sigma(N, act):
    from aonerf import _lib as L

    net, lat = _golden()
    mlp = net.fine_mlp
    gen = torch.Generator().manual_seed(17 + N)
    pos = (3.0 * (torch.rand(N, 3, generator=gen) - 0.5)).cuda()
    cond = torch.randn(N, 27, generator=gen).cuda()  # arbitrary: sigma does not read it
    pack = mlp.packed_weights(lat)
    ref = torch.empty((N, 4), device="cuda")
    L.call("aon_mlp_art_fwd_points", L.ptr(pack), L.ptr(pos), L.ptr(cond), N, 1, act, L.ptr(ref),
           L.stream(pos.device))
    buf, out = guarded(N)
    L.call("aon_mlp_art_fwd_sigma_points", L.ptr(pack), L.ptr(pos), N, act, L.ptr(buf),
           L.stream(pos.device))
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all()
    assert torch.equal(out[:, 3], ref[:, 3])
    assert torch.equal(out[:, :3], torch.zeros((N, 3), device="cuda"))
    assert torch.equal(buf[N:], torch.full((GUARD, 4), SENTINEL, device="cuda")), "rows past N written"
    assert status(pack) == 0


# ---------------------------------------------------------------------------- 3. in place
def test_the_prefix_is_read_in_place():
    """One pack; sigma pass, full kernel, sigma pass again with no re-pack: the pass neither needs
    a stream of its own nor disturbs the one it reads."""
    net, lat = _golden()
    o, d, v, t = rays_of(7, 193)
    N = t.numel()
    pack = net.coarse_mlp.packed_weights(lat)
    before = pack.clone()
    a, b = torch.empty((N, 4), device="cuda"), torch.empty((N, 4), device="cuda")
    sigma_rays(pack, o, d, t, 0, a)
    full = full_rays(pack, o, d, v, t, 0)
    sigma_rays(pack, o, d, t, 0, b)
    assert torch.equal(a[:, 3], full[:, 3]) and torch.equal(b[:, 3], full[:, 3])
    assert torch.equal(a, b)
    assert torch.equal(pack, before) and status(pack) == 0


# ---------------------------------------------------------------------------- 4. range word
def test_trunk_overflow_is_reported_and_density_falls_back():
    """tests/test_gpu_art_range.py's recipe on a trunk layer: pts_linears.3's unit 0 at 12000,
    disconnected from pts_linears.4 (the network function does not depend on it).  The trunk is
    part of the density-only pass: it must report; density() then warns and returns the
    layer-by-layer values."""
    from aonerf import two_level
    from aonerf.model_autodecoder import RANGE_WARNING
    from test_gpu_art_range import VALUES, hot_sd

    net = make_net(hot_sd("h3", VALUES["outside"]))
    _, lat = _golden()
    mlp = net.fine_mlp
    o, d, v, t = rays_of(3, 43)
    pack = mlp.packed_weights(lat)
    assert status(pack) == 0
    out = torch.empty((t.numel(), 4), device="cuda")
    sigma_rays(pack, o, d, t, 0, out)
    assert status(pack) == 1
    mlp.forward_sigma(o, d, t, lat)  # the Python entry: its own pack, the same report
    assert status(mlp._art_packed) == 1

    pos = (o[:, None, :] + t[..., None] * d[:, None, :]).contiguous()  # (3, 43, 3)
    for activated in (True, False):
        with pytest.warns(RuntimeWarning, match="fp16x3 range") as seen:
            got = mlp.density(pos, lat, activated=activated)
        assert [str(w.message) for w in seen] == [RANGE_WARNING]
        with two_level.switched([mlp], "fused", False), warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*fp16x3 range.*")
            want = mlp.density(pos, lat, activated=activated)
        assert got.shape == (3, 43) and torch.isfinite(got).all() and torch.equal(got, want)
    # inside the range the same network stays on the fused pass, silently
    load(net, hot_sd("h3", VALUES["inside"]))
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*fp16x3 range.*")
        mlp.density(pos, lat)
    assert status(mlp._art_packed) == 0


def test_view_branch_overflow_is_not_the_sigma_passs():
    """The same edit on views_linear.1 only: the full kernel splits that layer's output and
    reports; the density-only pass never forms it and leaves the word at 0 -- with the same
    sigma, which never depended on the view branch."""
    from test_gpu_art_range import VALUES, hot_sd

    net = make_net(hot_sd("hv1", VALUES["outside"]))
    _, lat = _golden()
    mlp = net.coarse_mlp
    o, d, v, t = rays_of(3, 43)
    pack = mlp.packed_weights(lat)
    full = full_rays(pack, o, d, v, t, 0)
    assert status(pack) == 1  # the recipe does overflow the view branch
    pack = mlp.packed_weights(lat)  # re-pack: the word is cleared
    assert status(pack) == 0
    out = torch.empty((t.numel(), 4), device="cuda")
    sigma_rays(pack, o, d, t, 0, out)
    assert status(pack) == 0
    assert torch.equal(out[:, 3], full[:, 3])


# ---------------------------------------------------------------------------- 5. fine_only
B5 = 37


def rays5():
    o, d, v, _ = rays_of(B5, 1)
    return {"rays_o": o, "rays_d": d, "viewdirs": v}


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def both(net, lat, randomized, near=2.0, far=6.0, seed=None, **kw):
    """(one-pass forward, fine_only forward) on the same rays; ``seed``: the generator re-seeded
    before each, and left in the same state by both."""
    outs, states = [], []
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*fp16x3 range.*")  # none at these parameters
        for fine_only in (False, True):
            if seed is not None:
                torch.manual_seed(seed)
            with torch.no_grad():
                outs.append(net(rays5(), randomized, True, near, far, lat, fine_only=fine_only,
                                **kw))
            states.append(torch.cuda.get_rng_state("cuda"))
    if seed is not None:
        assert torch.equal(states[0], states[1]), "the two forwards drew differently"
    return outs


def check_fine_only(one, two):
    assert one[0] is not None and len(one[0]) == 3
    assert two[0] is None
    assert len(two[1]) == 3 and same(one[1], two[1])


def test_fine_only_eval_and_injected_uniforms():
    net, lat = _golden()
    assert (net.num_coarse_samples, net.num_fine_samples) == (64, 128)
    check_fine_only(*both(net, lat, False))
    gen = torch.Generator().manual_seed(3)
    u_c, u_f = torch.rand(B5, 65, generator=gen).cuda(), torch.rand(B5, 128, generator=gen).cuda()
    one, two = both(net, lat, True, u_coarse=u_c, u_fine=u_f)
    check_fine_only(one, two)
    assert not torch.equal(one[1][0], both(net, lat, False)[0][1][0])  # the uniforms matter


def test_fine_only_per_ray_bounds_and_two_kernel_march():
    net, lat = _golden()
    gen = torch.Generator().manual_seed(4)
    near = (1.5 + torch.rand(B5, 1, generator=gen)).cuda()
    far = (5.0 + torch.rand(B5, 1, generator=gen)).cuda()
    check_fine_only(*both(net, lat, False, near=near, far=far))
    net2 = make_net(fused_march=False)
    one, two = both(net2, lat, False)
    check_fine_only(one, two)
    assert same(one[1], both(net, lat, False)[0][1])  # (the march kernels agree, as ever)


def test_fine_only_density_noise_keeps_the_rng_order():
    net = make_net(noise_std=0.1)
    _, lat = _golden()
    one, two = both(net, lat, True, seed=5)
    check_fine_only(one, two)
    other = both(net, lat, True, seed=6)[1]
    assert not torch.equal(other[1][0], two[1][0])  # and the draws matter


def test_fine_only_with_weights_maps_and_timers():
    net, lat = _golden()
    with torch.no_grad():
        one = net(rays5(), False, True, 2.0, 6.0, lat, return_weights=True)
        two = net(rays5(), False, True, 2.0, 6.0, lat, return_weights=True, fine_only=True)
        assert two[0] is not None and len(two[0]) == 4 and same(one[0], two[0]) and same(one[1], two[1])
        two = net(rays5(), False, True, 2.0, 6.0, lat, return_intermediates=True, fine_only=True)
        assert two[0] is not None and two[0][3]["raw"][:, :3].any()  # the coarse colours: computed
        one = net(rays5(), False, True, 2.0, 6.0, lat, maps=True)
        two = net(rays5(), False, True, 2.0, 6.0, lat, maps=True, fine_only=True)
        assert two[0] is None and len(two[1]) == 4 and same(one[1][:3], two[1][:3])
        assert set(two[1][3]) == {"canonical", "motion", "motion_mag"}
        assert all(torch.equal(one[1][3][k], two[1][3][k]) for k in one[1][3])
        timers = {}
        net(rays5(), False, True, 2.0, 6.0, lat, fine_only=True, timers=timers)
    assert sorted(timers) == ["comp1", "march0", "mlp0", "mlp1"]


def test_fine_only_is_ignored_on_the_training_path():
    """As NeRF.forward: with autograd on and trainable parameters the keyword changes nothing."""
    from aonerf import _lib as L
    from aonerf.model_autodecoder import NeRF_AE_Art

    net = NeRF_AE_Art().cuda()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in W.art_state_dict(0).items()})
    _, lat = _golden()
    o, d, v, _ = rays_of(4, 1)
    rays = {"rays_o": o, "rays_d": d, "viewdirs": v}
    assert torch.is_grad_enabled() and any(p.requires_grad for p in net.parameters())
    one = net(rays, False, True, 2.0, 6.0, lat)
    two = net(rays, False, True, 2.0, 6.0, lat, fine_only=True)
    assert two[0] is not None and two[1][0].requires_grad
    assert same(one[0], two[0]) and same(one[1], two[1])
    L.check_pending()  # the training forwards' packs: consumed here (no overflow to inherit)


# ---------------------------------------------------------------------------- 6. aonerf.render
def test_render_with_latents_equals_the_closure_form():
    from aonerf import helper
    from aonerf.ray_utils import frame_rays
    from aonerf.render import (create_spheric_poses, render_frame, render_rays, render_rays_test,
                               sapien_focal)

    net, lat = _golden()

    def model(sub, randomized, white_bkgd, near, far, maps=False, **_):  # the closure form
        return net(sub, randomized, white_bkgd, near, far, lat, maps=maps)

    batch = rays5()
    for chunk in (None, 13):
        want = render_rays(model, batch, chunk, True, 2.0, 6.0, maps=True)
        got = render_rays(net, batch, chunk, True, 2.0, 6.0, maps=True, latents=lat)
        assert set(got) == set(want) == {"comp_rgb", "acc", "depth", "canonical", "motion",
                                         "motion_mag"}
        assert all(torch.equal(got[k], want[k]) for k in want), chunk
    assert torch.equal(render_rays_test(net, batch, 13, True, 2.0, 6.0, latents=lat)["rgb"],
                       want["comp_rgb"])

    H, WD = 24, 32
    c2w, focal = torch.as_tensor(create_spheric_poses(4.0)[11]), sapien_focal(H)
    rays = frame_rays(c2w, H, WD, focal)
    tmin, tmax = helper.get_ray_limits_box(rays["rays_o"], rays["rays_d"], 2)
    hit = ((tmax > tmin) & (tmax > 0)).reshape(-1)
    assert 0 < int(hit.sum()) < H * WD  # some rays miss the box of side 2
    cases = [dict()] + [dict(box_side_length=2, cull=c) for c in (True, False)]
    for kw in cases:
        want = render_frame(model, c2w, H, WD, focal, chunk=200, maps=True, **kw)
        got = render_frame(net, c2w, H, WD, focal, chunk=200, maps=True, latents=lat, **kw)
        assert tuple(got.shape) == (H * WD, 12) and torch.equal(got, want), kw
        want = render_rays(model, rays, 200, True, 2.0, 6.0, **kw)
        got = render_rays(net, rays, 200, True, 2.0, 6.0, latents=lat, **kw)
        assert all(torch.equal(got[k], want[k]) for k in want), kw


# ---------------------------------------------------------------------------- 7. density
def test_density_articulated():
    from aonerf import _lib as L
    from aonerf import two_level

    net, lat = _golden()
    mlp = net.fine_mlp
    gen = torch.Generator().manual_seed(23)
    pos = (2.0 * (torch.rand(5, 7, 3, generator=gen) - 0.5)).cuda()
    flat = pos.reshape(-1, 3).contiguous()
    want = {}
    for act in (L.ACT_ARTIC, L.ACT_NONE):
        out = torch.empty((35, 4), device="cuda")
        L.call("aon_mlp_art_fwd_sigma_points", L.ptr(mlp.packed_weights(lat)), L.ptr(flat), 35, act,
               L.ptr(out), L.stream(flat.device))
        want[act] = out[:, 3].view(5, 7)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*fp16x3 range.*")
        got = mlp.density(pos, lat)
        raw = mlp.density(pos, lat, activated=False)
    assert got.shape == (5, 7) and raw.shape == (5, 7)
    assert torch.equal(got, want[L.ACT_ARTIC]) and torch.equal(raw, want[L.ACT_NONE])
    assert torch.equal(got, mlp.density(pos, lat, activated=True))
    assert (got > 0).all() and not torch.equal(got, raw)
    assert mlp.density(pos[0, 0], lat).shape == ()  # one point
    # layer by layer: column 3 of _mlp
    venc = torch.zeros((35, 27), device="cuda")
    with two_level.switched([mlp], "fused", False):
        slow = mlp.density(pos, lat, activated=False)
        assert torch.equal(slow, mlp._mlp(flat, venc, 1, lat)[:, 3].view(5, 7))
        t = torch.zeros((35, 1), device="cuda")
        fs = mlp.forward_sigma(flat, torch.zeros_like(flat), t, lat)
        assert torch.equal(fs[:, 3], slow.reshape(-1)) and not fs[:, :3].any()
    with pytest.raises(ValueError, match=r"\(\.\.\., 3\)"):
        mlp.density(torch.zeros(4, 2, device="cuda"), lat)


# ---------------------------------------------------------------------------- 8. density (vanilla)
def test_density_vanilla():
    from aonerf import _lib as L
    from aonerf.model import NeRFMLP
    from oracle import nerf_oracle as O

    mlp = NeRFMLP(0, 10, 4).cuda()
    mlp.load_state_dict({k: torch.as_tensor(v)
                         for k, v in O.split_state_dict(W.nerf_state_dict(0))[1].items()})
    mlp.requires_grad_(False)
    gen = torch.Generator().manual_seed(29)
    pos = (2.0 * (torch.rand(5, 7, 3, generator=gen) - 0.5)).cuda()
    flat = pos.reshape(-1, 3).contiguous()
    d = torch.nn.functional.normalize(torch.randn(35, 3, generator=gen), dim=-1).cuda()
    t = torch.zeros((35, 1), device="cuda")
    ref = {}
    for act in (L.ACT_NONE, L.ACT_VANILLA):
        out = torch.empty((35, 4), device="cuda")
        L.call("aon_mlp_fwd", L.ptr(mlp.packed_weights()), L.PREC["f16x3"], L.ptr(flat), L.ptr(d),
               L.ptr(d), L.ptr(t), 35, 1, act, L.ptr(out), L.stream(flat.device))
        ref[act] = out[:, 3].view(5, 7)
    raw = mlp.density(pos, activated=False)
    assert raw.shape == (5, 7) and torch.equal(raw, ref[L.ACT_NONE])
    assert torch.equal(mlp.density(pos), ref[L.ACT_VANILLA])
    assert torch.equal(mlp.density(pos), torch.relu(raw))  # not the articulated softplus
    assert int(L.status_word(mlp._packed)) == 0


# ---------------------------------------------------------------------------- 9. density_grid
def test_density_grid():
    from aonerf import geometry

    net, lat = _golden()
    mlp = net.fine_mlp
    R, side = 5, 2.0
    grid = geometry.density_grid(mlp, R, side, latents=lat)
    assert tuple(grid.shape) == (R, R, R)
    c = (torch.arange(R, dtype=torch.float32) + 0.5) * (side / R) - side / 2
    pts = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), -1).cuda()
    assert torch.equal(geometry.grid_points(R, side), pts)
    assert torch.equal(grid, mlp.density(pts, lat))
    assert torch.equal(geometry.density_grid(mlp, R, side, latents=lat, chunk=50), grid)
    raw = geometry.density_grid(mlp, R, side, latents=lat, activated=False)
    assert torch.equal(raw, mlp.density(pts, lat, activated=False))
    # grid[i, j, k] is the point (x_i, y_j, z_k): x slowest
    for i, j, k in ((0, 0, 0), (1, 2, 3), (4, 0, 2)):
        p = torch.tensor([c[i], c[j], c[k]]).cuda()
        assert torch.equal(grid[i, j, k], mlp.density(p, lat)), (i, j, k)
    assert not torch.equal(grid, grid.transpose(0, 2))  # and the order is observable
