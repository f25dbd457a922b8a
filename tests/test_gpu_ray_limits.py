"""GPU tests of box-bounded rendering: the ray / box limits and the per-ray stratified sampler
against the reference's recorded values (tests/golden/ray_limits.npz, bit for bit), both models
end to end on per-ray bounds against the CPU oracle (the chain of tests/test_gpu_parity.py,
every link at its 1e-4), the order-preserving compaction, and the culled render against the
unculled one.  Everything here needs an MI355X (marker `gpu`)."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from oracle import weights as W

from test_gpu_parity import E2E_ATOL, cuda, make_nerf, npy, report

pytestmark = pytest.mark.gpu

SIDES = (("2", 2), ("1p2", 1.2))
H, WD = 24, 32


@pytest.fixture(scope="module")
def g(golden):
    return golden("ray_limits.npz")


def assert_bits(got, want, what=""):
    """Equal bit patterns wherever the reference is not NaN (so every inf too), NaN where it is."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{what}: NaN positions")
    np.testing.assert_array_equal(np.isinf(got), np.isinf(want), err_msg=f"{what}: inf positions")
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32), err_msg=what)


# ----------------------------------------------------------------------------- 1: limits
@pytest.mark.parametrize("key,side", SIDES)
@pytest.mark.parametrize("batch", ["frame", "hand", "none"])
def test_limits_bit_equal_to_the_reference(g, batch, key, side):
    from aonerf import helper

    o, d = cuda(g[f"{batch}_rays_o"]), cuda(g[f"{batch}_rays_d"])
    tmin, tmax = helper.get_ray_limits_box(o, d, side)
    assert tuple(tmin.shape) == tuple(tmax.shape) == (o.shape[0], 1)
    assert_bits(npy(tmin), g[f"{batch}_box_tmin_{key}"], f"{batch} tmin")
    assert_bits(npy(tmax), g[f"{batch}_box_tmax_{key}"], f"{batch} tmax")
    near, far = helper.get_ray_limits(o, d, side)
    assert_bits(npy(near), g[f"{batch}_near_{key}"], f"{batch} near")
    assert_bits(npy(far), g[f"{batch}_far_{key}"], f"{batch} far")


def test_limits_shapes_and_default_side(g):
    """The reference's shapes: (..., 3) in, (..., 1) out; box_side_length defaults to 2."""
    from aonerf import helper

    o, d = cuda(g["frame_rays_o"]).reshape(H, WD, 3), cuda(g["frame_rays_d"]).reshape(H, WD, 3)
    near, far = helper.get_ray_limits(o, d)
    assert tuple(near.shape) == tuple(far.shape) == (H, WD, 1)
    assert_bits(npy(near).reshape(-1, 1), g["frame_near_2"])
    tmin, _ = helper.get_ray_limits_box(o[:, :5], d[:, :5], 2)  # strided input
    assert_bits(npy(tmin).reshape(-1), g["frame_box_tmin_2"].reshape(H, WD)[:, :5].reshape(-1))


# ----------------------------------------------------------------------------- 2: sampler
@pytest.mark.parametrize("N", [64, 8])
@pytest.mark.parametrize("mode", ["eval", "lindisp", "rand", "rand_lindisp"])
def test_per_ray_sampler_bit_equal_to_the_reference(g, mode, N):
    from aonerf import helper

    o, d = cuda(g["samp_rays_o"]), cuda(g["samp_rays_d"])
    near, far = cuda(g["samp_near"]), cuda(g["samp_far"])
    randomized, lindisp = mode.startswith("rand"), mode.endswith("lindisp")
    u = cuda(g[f"samp_u_{N}"]) if randomized else None
    want = g[f"samp_t_{mode}_{N}"]
    t, xyz = helper.sample_along_rays(o, d, N, near, far, randomized, lindisp, u=u)
    assert tuple(t.shape) == (77, N + 1)
    assert_bits(npy(t), want, mode)
    ref_xyz = O.cast_rays(torch.from_numpy(want), torch.from_numpy(g["samp_rays_o"]),
                          torch.from_numpy(g["samp_rays_d"])).numpy()
    assert_bits(npy(xyz), ref_xyz, f"{mode} xyz")
    t2, none = helper.sample_along_rays(o, d, N, near[:, 0], far, randomized, lindisp, u=u,
                                        want_coords=False)  # (B,) beside (B, 1); no xyz
    assert none is None and torch.equal(t2, t)


# ----------------------------------------------------------------------------- 3: scalar path
@pytest.mark.parametrize("randomized", [False, True])
@pytest.mark.parametrize("lindisp", [False, True])
def test_scalar_path_untouched(g, monkeypatch, randomized, lindisp):
    from aonerf import _lib as L
    from aonerf import helper

    names = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    o, d = cuda(g["samp_rays_o"]), cuda(g["samp_rays_d"])
    B = o.shape[0]
    u = cuda(g["samp_u_64"]) if randomized else None
    t_s, xyz_s = helper.sample_along_rays(o, d, 64, 2.0, 6.0, randomized, lindisp, u=u)
    assert names == ["aon_sample_along_rays"]  # two python numbers: today's kernel
    del names[:]
    near, far = torch.full((B, 1), 2.0, device="cuda"), torch.full((B,), 6.0, device="cuda")
    for nr, fr in ((near, far), (2.0, far), (near, 6.0)):  # tensors, and a scalar beside one
        t, xyz = helper.sample_along_rays(o, d, 64, nr, fr, randomized, lindisp, u=u)
        assert_bits(npy(t), npy(t_s))
        assert_bits(npy(xyz), npy(xyz_s))
    assert names == ["aon_sample_along_rays_bounds"] * 3
    with pytest.raises(ValueError, match="near must be"):
        helper.sample_along_rays(o, d, 64, near[:5], far, randomized, lindisp, u=u)


# ----------------------------------------------------------------------------- 4, 5: end to end
@pytest.fixture(scope="module")
def frame(g):
    rays = {k: cuda(g[f"frame_{k}"]) for k in ("rays_o", "rays_d", "viewdirs")}
    rc = {k: torch.from_numpy(g[f"frame_{k}"]) for k in ("rays_o", "rays_d", "viewdirs")}
    return rays, rc, torch.from_numpy(g["frame_near_2"]), torch.from_numpy(g["frame_far_2"])


@pytest.fixture(scope="module")
def vanilla_ref(frame):
    """The oracle's two-level forward given the reference's (B, 1) bounds (its sampler
    broadcasts them as the reference's does); computed once for both precisions."""
    _, rc, near, far = frame
    params = O.split_state_dict(W.nerf_state_dict(0))
    ret, inter = O.nerf_forward(params, rc, False, True, near, far, return_intermediates=True)
    return params, ret, inter


def chain(ret, coarse, coarse_inter, rc, fine_level, what):
    """Links (1)-(3) of tests/test_gpu_parity.py on per-ray bounds, each at 1e-4 on every ray."""
    want = (coarse[0], coarse[1], coarse[2], coarse_inter["weights"])
    assert_bits(npy(ret[0][4]["t_vals"]), coarse_inter["t_vals"].numpy(), f"{what} coarse t")
    for j, k in enumerate(("rgb", "acc", "depth", "weights")):
        err = report(f"{what} coarse {k}", npy(ret[0][j]), want[j].detach().numpy(), E2E_ATOL)
        assert err.max() <= E2E_ATOL, f"coarse {k}: {err.max():.3e}"
    t_c, w_c = ret[0][4]["t_vals"].cpu(), ret[0][3].cpu()
    t_f, _ = O.sample_pdf(0.5 * (t_c[..., 1:] + t_c[..., :-1]), w_c[..., 1:-1], rc["rays_o"],
                          rc["rays_d"], t_c, 128, False)
    np.testing.assert_array_equal(npy(ret[1][4]["t_vals"]), t_f.numpy())
    fine = fine_level(t_f)  # (rgb, acc, weights, depth)
    for j, k, jj in ((0, "rgb", 0), (1, "acc", 1), (3, "depth", 2), (2, "weights", 3)):
        err = report(f"{what} fine {k}", npy(ret[1][jj]), fine[j].detach().numpy(), E2E_ATOL)
        assert err.max() <= E2E_ATOL, f"fine {k}: {err.max():.3e}"


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_vanilla_end_to_end_on_box_bounds(g, frame, vanilla_ref, precision):
    from aonerf import helper

    rays, rc, _, _ = frame
    params, ref, inter = vanilla_ref
    net = make_nerf(precision)
    near, far = helper.get_ray_limits(rays["rays_o"], rays["rays_d"], 2)
    assert_bits(npy(near), g["frame_near_2"])
    ret = net(rays, False, True, near, far, return_weights=True, return_intermediates=True)
    chain(ret, ref[0], inter[0], rc, lambda t_f: O.render_level(params, rc, t_f, 1, True),
          f"box {precision}")


def test_articulated_end_to_end_on_box_bounds(g, golden, frame):
    from aonerf import helper
    from aonerf.model_autodecoder import NeRF_AE_Art

    rays, rc, near_ref, far_ref = frame
    ga = golden("articulated.npz")
    sd = W.art_state_dict(0)
    net = NeRF_AE_Art().cuda()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    lat = {k: cuda(ga[f"latent_{k}"]) for k in ("density", "color", "articulation")}
    lat_cpu = {k: torch.from_numpy(ga[f"latent_{k}"]) for k in ("density", "color", "articulation")}
    params = O.split_state_dict(sd)
    with torch.no_grad():
        ref, inter = O.art_nerf_forward(params, rc, False, True, near_ref, far_ref, lat_cpu,
                                        return_intermediates=True)
        near, far = helper.get_ray_limits(rays["rays_o"], rays["rays_d"], 2)
        ret = net(rays, False, True, near, far, lat, return_weights=True,
                  return_intermediates=True)
        chain(ret, ref[0], inter[0], rc,
              lambda t_f: O.art_render_level(params, rc, t_f, 1, True, lat_cpu), "box art")


# ----------------------------------------------------------------------------- 6: compaction
@pytest.mark.parametrize("mask", ["all", "none", "alternating"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257, 768])
def test_compaction(B, mask):
    from aonerf import helper

    gen = torch.Generator().manual_seed(100 + B)
    hit = {"all": torch.ones(B, dtype=torch.bool), "none": torch.zeros(B, dtype=torch.bool),
           "alternating": torch.arange(B) % 2 == 0}[mask]
    tmin = torch.where(hit, 4.0 * torch.rand(B, generator=gen) - 1.0, torch.tensor(-1.0))
    tmax = torch.where(hit, tmin.clamp(min=0) + 0.5 + torch.rand(B, generator=gen),
                       torch.tensor(-2.0))
    if mask == "none" and B > 4:  # the other ways to miss: NaN limits, tmin == tmax, all behind
        tmin[0], tmax[0] = float("nan"), 3.0
        tmin[1], tmax[1] = 1.0, float("nan")
        tmin[2], tmax[2] = 2.0, 2.0
        tmin[3], tmax[3] = -3.0, -1.0
    o, d, v = (torch.randn(B, 3, generator=gen) for _ in range(3))
    c = helper.compact_rays(tmin.cuda().reshape(B, 1), tmax.cuda().reshape(B, 1), o.cuda(),
                            d.cuda(), v.cuda())
    want = torch.nonzero(hit).reshape(-1)
    n = int(c["n_hit"].item())
    assert n == len(want)
    idx = c["idx"][:n].cpu().long()
    assert torch.equal(idx, want)
    assert n < 2 or bool((idx[1:] > idx[:-1]).all())  # strictly increasing: order kept
    slot = torch.full((B,), -1, dtype=torch.int32)
    slot[want] = torch.arange(n, dtype=torch.int32)
    assert torch.equal(c["slot"].cpu(), slot)
    for k, src in (("rays_o", o), ("rays_d", d), ("viewdirs", v)):
        assert torch.equal(c[k][:n].cpu(), src[want]), k
    assert torch.equal(c["near"][:n].cpu(), tmin[want].clamp(min=0))
    assert torch.equal(c["far"][:n].cpu(), tmax[want])
    # the payload: compact rows where they came from, the background row elsewhere
    comp, acc, depth = torch.rand(n, 3, generator=gen), torch.rand(n, generator=gen), \
        torch.rand(n, generator=gen)
    for white in (True, False):
        out = helper.scatter_payload(comp.cuda(), acc.cuda(), depth.cuda(), c["slot"], white).cpu()
        exp = torch.zeros(B, 5)
        exp[:, :3] = 1.0 if white else 0.0
        exp[want] = torch.cat([comp, depth[:, None], acc[:, None]], -1)
        assert torch.equal(out, exp)


# ----------------------------------------------------------------------------- 7: culling
@pytest.fixture(scope="module")
def net():
    return make_nerf("f16x3")


@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("cam", [0, 1, 2], ids=["frame", "away", "narrow"])
def test_culled_render_equals_the_unculled_one(g, net, monkeypatch, cam, white):
    from aonerf import _lib as L
    from aonerf import helper
    from aonerf.ray_utils import frame_rays
    from aonerf.render import render_frame

    c2w, focal = torch.from_numpy(g["cam_c2w"][cam]), float(g["cam_focal"][cam])
    n_ref = int(g["cam_hits"][cam])
    assert 0.2 < int(g["cam_hits"][0]) / (H * WD) < 0.8 and int(g["cam_hits"][0]) % 16 != 0
    assert int(g["cam_hits"][1]) == 0 and int(g["cam_hits"][2]) == H * WD
    rays = frame_rays(c2w, H, WD, focal)
    tmin, tmax = helper.get_ray_limits_box(rays["rays_o"], rays["rays_d"], 2)
    hit = ((tmax > tmin) & (tmax > 0)).reshape(-1)
    assert int(hit.sum()) == n_ref  # the reference's count on the reference's rays
    kw = dict(white_bkgd=white, chunk=200, box_side_length=2)  # 768 = 3 x 200 + 168: ragged
    full = render_frame(net, c2w, H, WD, focal, cull=False, **kw)
    names = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    culled = render_frame(net, c2w, H, WD, focal, cull=True, **kw)
    monkeypatch.undo()
    assert tuple(culled.shape) == tuple(full.shape) == (H * WD, 5)
    mlp_calls = [s for s in names if s.startswith("aon_mlp")]
    if n_ref == 0:
        assert not mlp_calls, mlp_calls  # zero hits launch no MLP
    else:
        assert mlp_calls
    assert torch.equal(culled[hit], full[hit])  # hit rows: bit-equal in all five columns
    bg = torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0] if white else [0.0] * 5, device="cuda")
    assert torch.equal(culled[~hit], bg.expand(int((~hit).sum()), 5))


def test_render_rays_box_keeps_its_keys(g, net, frame):
    from aonerf.render import render_frame, render_rays

    rays, _, _, _ = frame
    batch = dict(rays, target=torch.rand(H * WD, 3, device="cuda"))
    plain = render_rays(net, batch, 300, True, 2.0, 6.0)
    c2w, focal = torch.from_numpy(g["frame_c2w"]), float(g["frame_hwf"][2])
    for cull in (False, True):
        out = render_rays(net, batch, 300, True, 2.0, 6.0, box_side_length=2, cull=cull)
        assert set(out) == set(plain)
        for k in plain:
            assert out[k].shape == plain[k].shape, k
        want = render_frame(net, c2w, H, WD, focal, chunk=300, box_side_length=2, cull=cull)
        assert torch.equal(out["comp_rgb"], want[:, :3])
        assert torch.equal(out["depth"], want[:, 3]) and torch.equal(out["acc"], want[:, 4])


# ----------------------------------------------------------------------------- 8: capture
def test_box_render_under_stream_capture(g, net):
    from aonerf.render import render_frame

    c2w, focal = torch.from_numpy(g["frame_c2w"]), float(g["frame_hwf"][2])

    def render(cull):
        return render_frame(net, c2w, H, WD, focal, box_side_length=2, cull=cull)

    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):  # warm-up: schedules cached, weights packed
        eager = render(False)
        render(False)
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = render(False)
        with pytest.raises(ValueError, match="cull=False"):
            render(True)
    for _ in range(2):
        captured.zero_()
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)
