"""The articulated render's canonical-coordinate and deformation maps: the deformation-only pass
(aon_mlp_art_fwd_deform[_points], csrc/mlp_art_deform.hip), the feature compositor
(aon_composite_feat, csrc/composite_feat.hip) and what is built on them (NeRFMLP.deform_rays /
deform, helper.composite_features, ``maps=True`` on NeRF_AE_Art.forward and aonerf.render).

Gates.  x' of the pass == the x' the fused training forward keeps (enc columns 0..2), bit for
bit: the same arithmetic on the same packed stream.  x' vs the CPU oracle: 1e-5 on every row
(the MLP-stage gate of tests/test_gpu_articulated.py).  ||delta||: relative 3e-7 of the fp64
norm of the returned delta -- three products, two sums of non-negatives and a square root, each
correctly rounded, bound the error by 2.5 * 2^-24 = 1.5e-7; the gate is twice that.  The feature
compositor == aon_composite_fwd's comp_rgb on the same weights, bit for bit, channel by channel.
The composited maps vs the oracle chain on the GPU's own fine samples: 1e-4 (ATOL of
tests/test_gpu_articulated.py: sums of the same kind and magnitude as depth)."""
import warnings

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu
ATOL = 1e-4
NAMES = ("density", "color", "articulation")
PAD, SENTINEL = 64, -7.25  # guard rows behind every output buffer and what they must still hold


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def report(name, got, want, atol):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    print(f"{name}: max|err|={err.max():.3e}  within {atol:g}: {(err <= atol).mean() * 100:.3f}%")
    return err


def load(net, sd):
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net


@pytest.fixture()
def art():
    """NeRF_AE_Art on the oracle's seeded weights and latent codes (reloaded per test: the range
    test edits them)."""
    from aonerf.model_autodecoder import NeRF_AE_Art

    sd = W.art_state_dict(0)
    net = load(NeRF_AE_Art().cuda(), sd)
    lat_np = W.art_latents(1)
    lat = {k: cuda(v) for k, v in lat_np.items()}
    lat_cpu = {k: torch.from_numpy(v) for k, v in lat_np.items()}
    return net, lat, lat_cpu, O.split_state_dict(sd)


def rays_of(B, S, seed=5):
    """(o, d, t) on the CPU: |o| <= 0.5, unit d, sorted t in [2, 6]."""
    gen = torch.Generator().manual_seed(seed + 131 * B + S)
    o = torch.rand(B, 3, generator=gen) - 0.5
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1)
    t = (2.0 + 4.0 * torch.rand(B, S, generator=gen)).sort(-1).values
    return o, d, t


def padded(N):
    return torch.full((N + PAD, 4), SENTINEL, device="cuda")


def deform_call(L, pack, o, d, t, xp, delta, points=None):
    """The C entry points on caller-owned (N + PAD, 4) buffers (None: that output not asked for)."""
    B, S = t.shape
    if points is None:
        L.call("aon_mlp_art_fwd_deform", L.ptr(pack), L.ptr(o), L.ptr(d), L.ptr(t), B, S,
               L.ptr(xp), L.ptr(delta), L.stream(t.device))
    else:
        L.call("aon_mlp_art_fwd_deform_points", L.ptr(pack), L.ptr(points), B * S, L.ptr(xp),
               L.ptr(delta), L.stream(t.device))


# ---------------------------------------------------------------------------- 1. the pass, bitwise
# (1, 1) .. (37, 193): the issue's shapes; (7, 19) = 133 rows: no multiple of 16 or of the 128
# rows of a workgroup; (257, 129) = 33,153 rows: past the launcher's 32,768-row threshold, so the
# 32-samples-per-wave instantiation (the smaller ones take 16), ragged in its last tile too
SHAPES = [(1, 1), (3, 5), (37, 65), (37, 193), (7, 19), (257, 129)]


@pytest.mark.parametrize("B,S", SHAPES)
def test_deform_pass_equals_the_training_forward_bit_for_bit(art, B, S):
    from aonerf import _lib as L
    from aonerf import tiles, train_art

    net, lat, _, _ = art
    mlp = net.fine_mlp
    o, d, t = (x.cuda() for x in rays_of(B, S))
    N = B * S
    geo = train_art._Geo(mlp)
    P = [(m.weight.detach(), m.bias.detach()) for m in train_art.art_layers(mlp)]
    lat_t = tuple(lat[k] for k in NAMES)
    raw = torch.empty((N, 4), device="cuda")
    xyz_kept, _, enc, _, _, _ = train_art._forward_level_fused(geo, P, lat_t, o, d, d, t, raw)
    xp_train = tiles.untile(enc, N)[:, :3].contiguous()
    pack = train_art._pack(geo, P, lat_t, S)  # the stream that forward read, packed again

    xp, delta = padded(N), padded(N)
    deform_call(L, pack, o, d, t, xp, delta)
    assert int(L.status_word(pack)) == 0
    assert torch.equal(xp[:N, :3], xp_train), "x' differs from the training forward's"
    assert torch.equal(xp[:N, 3], torch.zeros(N, device="cuda"))
    for buf in (xp, delta):  # rows past N are never written
        assert torch.equal(buf[N:], torch.full((PAD, 4), SENTINEL, device="cuda"))

    # delta + xyz == x' in fp32 (xyz from aon_cast_rays; torch's add rounds to nearest)
    xyz = torch.empty((N, 3), device="cuda")
    L.call("aon_cast_rays", L.ptr(o), L.ptr(d), L.ptr(t), B, S, None, 0, L.ptr(xyz), 0, 0, None,
           L.stream(o.device))
    assert torch.equal(xyz, xyz_kept)
    assert torch.equal(delta[:N, :3] + xyz, xp[:N, :3])

    # ||delta||: relative 3e-7 of the fp64 norm of the returned delta
    want = delta[:N, :3].double().norm(dim=-1)
    rel = ((delta[:N, 3].double() - want).abs() / want.clamp_min(1e-300)).max().item()
    print(f"({B}, {S}): max relative error of ||delta|| = {rel:.3e}")
    assert rel <= 3e-7

    # points mode on the same positions; one output alone
    xp_p, delta_p = padded(N), padded(N)
    deform_call(L, pack, o, d, t, xp_p, delta_p, points=xyz)
    assert torch.equal(xp_p, xp) and torch.equal(delta_p, delta)
    for points in (None, xyz):
        xp_1, delta_1 = padded(N), padded(N)
        deform_call(L, pack, o, d, t, xp_1, None, points=points)
        deform_call(L, pack, o, d, t, None, delta_1, points=points)
        assert torch.equal(xp_1, xp) and torch.equal(delta_1, delta)

    # the Python surface (its own pack of the same weights and codes)
    a, b, m = mlp.deform_rays(o, d, t, lat)
    assert a.shape == (B, S, 3) and b.shape == (B, S, 3) and m.shape == (B, S)
    assert torch.equal(a.reshape(N, 3), xp[:N, :3]) and torch.equal(b.reshape(N, 3), delta[:N, :3])
    assert torch.equal(m.reshape(N), delta[:N, 3])
    a, b, m = mlp.deform(xyz.view(B, S, 3), lat)
    assert torch.equal(a.reshape(N, 3), xp[:N, :3]) and torch.equal(m.reshape(N), delta[:N, 3])


# ---------------------------------------------------------------------------- 2. vs the oracle
def test_deform_pass_against_the_oracle(art):
    net, lat, lat_cpu, params = art
    B, S = 37, 65
    o, d, t = rays_of(B, S)
    pos = O.cast_rays(t, o, d)
    with torch.no_grad():
        xp_ref = O.art_mlp_forward(params[1], pos, O.pos_enc(d, 0, 4), lat_cpu, return_xp=True)[2]
    xp, delta, _ = net.fine_mlp.deform_rays(o.cuda(), d.cuda(), t.cuda(), lat)
    err = report("x' vs oracle", xp.reshape(-1, 3).cpu().numpy(), xp_ref.numpy(), 1e-5)
    assert err.max() <= 1e-5
    err = report("delta vs oracle", delta.reshape(-1, 3).cpu().numpy(),
                 (xp_ref.double() - pos.reshape(-1, 3).double()).numpy(), 1e-5)
    assert err.max() <= 1e-5


# ---------------------------------------------------------------------------- 3. feature compositor
@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("S", [1, 2, 65, 193, 512])
def test_composite_feat_equals_comp_rgb_channel_by_channel(B, S):
    from aonerf import _lib as L

    gen = torch.Generator().manual_seed(11 + 7 * B + S)
    N, dev = B * S, "cuda"
    feat = torch.rand(N, 4, generator=gen).cuda()  # activated colours: AON_ACT_NONE below
    sigma = (3.0 * torch.rand(N, generator=gen)).cuda()
    _, d, t = rays_of(B, S)
    d, t = d.cuda(), t.cuda()

    def comp_rgb(rgb, stride, w_out):
        comp, acc, depth = (torch.empty(s, device=dev) for s in ((B, 3), (B,), (B,)))
        L.call("aon_composite_fwd", L.ptr(rgb), stride, L.ptr(sigma), 1, L.ptr(t), L.ptr(d), B, S,
               0, L.ACT_NONE, L.ptr(comp), L.ptr(acc), L.ptr(w_out), L.ptr(depth), L.stream(dev))
        return comp

    def comp_feat(f, stride, C):
        out = torch.full((B + 1, C), SENTINEL, device=dev)
        L.call("aon_composite_feat", L.ptr(w), L.ptr(f), stride, C, B, S, L.ptr(out), L.stream(dev))
        assert torch.equal(out[B], torch.full((C,), SENTINEL, device=dev))
        return out[:B]

    w = torch.empty((B, S), device=dev)
    want = comp_rgb(feat, 4, w)
    assert torch.equal(comp_feat(feat, 4, 3), want)  # the 16-byte-row path
    assert torch.equal(comp_feat(feat[:, :3].contiguous(), 3, 3), want)
    for C in (1, 4, 8):
        for stride in (C, C + 3):
            f = torch.rand(N, stride, generator=gen).cuda()
            got = comp_feat(f, stride, C)
            for k in range(0, C, 3):  # channels k..k+2 through a 3-channel compositor call
                f3 = torch.zeros((N, 3), device=dev)
                n = min(3, C - k)
                f3[:, :n] = f[:, k:k + n]
                assert torch.equal(got[:, k:k + n], comp_rgb(f3, 3, None)[:, :n]), (C, stride, k)
    # the Python surface: (B, S, C), flat rows, and a column slice read in place
    from aonerf import helper

    assert torch.equal(helper.composite_features(w, feat[:, :3]), want)
    assert torch.equal(helper.composite_features(w, feat[:, :3].reshape(B, S, 3)), want)


# ---------------------------------------------------------------------------- 4. end to end
def oracle_maps(params, rc, t_f, lat_cpu):
    """The oracle chain: the oracle's x' and delta on the given fine samples, composited with its
    own weights as volumetric_rendering(nocs=) does (reference helper.py:191-193)."""
    with torch.no_grad():
        fine = O.art_render_level(params, rc, t_f, 1, True, lat_cpu, return_xp=True)
    w, xp = fine[2], fine[4].reshape(t_f.shape + (3,))
    delta = (xp.double() - O.cast_rays(t_f, rc["rays_o"], rc["rays_d"]).double()).float()

    def nocs(f):
        return (w[..., None] * f).sum(dim=-2)

    return {"canonical": nocs(xp), "motion": nocs(delta),
            "motion_mag": nocs(delta.norm(dim=-1, keepdim=True))[:, 0]}


@pytest.mark.parametrize("white", [True, False])
def test_forward_maps_end_to_end(art, white):
    net, lat, lat_cpu, params = art
    B = 37
    o, d, _ = rays_of(B, 1)
    rays = {"rays_o": o.cuda(), "rays_d": d.cuda(), "viewdirs": d.cuda()}
    with torch.no_grad():
        plain = net(rays, False, white, 2.0, 6.0, lat)
        ret = net(rays, False, white, 2.0, 6.0, lat, maps=True, return_weights=True,
                  return_intermediates=True)
        short = net(rays, False, white, 2.0, 6.0, lat, maps=True)
    assert len(plain[1]) == 3 and len(short[1]) == 4 and len(ret[1]) == 6 and len(ret[0]) == 5
    maps = ret[1][-1]
    assert set(maps) == {"canonical", "motion", "motion_mag"} and set(short[1][-1]) == set(maps)
    for j in range(3):  # every other output: the same bits
        assert torch.equal(ret[1][j], plain[1][j]) and torch.equal(short[1][j], plain[1][j])
        assert torch.equal(ret[0][j], plain[0][j])
    for k, shape in (("canonical", (B, 3)), ("motion", (B, 3)), ("motion_mag", (B,))):
        assert tuple(maps[k].shape) == shape and torch.equal(short[1][-1][k], maps[k])
    assert ret[1][4]["t_vals"].shape == (B, 65 + 128)
    want = oracle_maps(params, {k: v.cpu() for k, v in rays.items()}, ret[1][4]["t_vals"].cpu(),
                       lat_cpu)
    for k in maps:
        err = report(f"maps {k} (white={white})", maps[k].cpu().numpy(), want[k].numpy(), ATOL)
        assert err.max() <= ATOL


def test_maps_have_no_backward(art):
    net, lat, _, _ = art
    o, d, _ = rays_of(5, 1)
    rays = {"rays_o": o.cuda(), "rays_d": d.cuda(), "viewdirs": d.cuda()}
    assert torch.is_grad_enabled() and any(p.requires_grad for p in net.parameters())
    with pytest.raises(ValueError, match="maps"):
        net(rays, False, True, 2.0, 6.0, lat, maps=True)


def test_render_rays_maps_chunks_and_culling(art):
    from aonerf import helper
    from aonerf.ray_utils import frame_rays
    from aonerf.render import create_spheric_poses, render_frame, render_rays, sapien_focal

    net, lat, _, _ = art

    def model(sub, randomized, white_bkgd, near, far, maps=False, **_):  # render's model call
        return net(sub, randomized, white_bkgd, near, far, lat, maps=maps)

    o, d, _ = rays_of(37, 1)
    batch = {"rays_o": o.cuda(), "rays_d": d.cuda(), "viewdirs": d.cuda()}
    one = render_rays(model, batch, None, True, 2.0, 6.0, maps=True)
    assert set(one) == {"comp_rgb", "acc", "depth", "canonical", "motion", "motion_mag"}
    ragged = render_rays(model, batch, 13, True, 2.0, 6.0, maps=True)  # 13 + 13 + 11
    off = render_rays(model, batch, 13, True, 2.0, 6.0)
    assert set(off) == {"comp_rgb", "acc", "depth"}
    for k in one:
        assert torch.equal(one[k], ragged[k]), k
    for k in off:
        assert torch.equal(one[k], off[k]), k

    # a frame some of whose rays miss the box of side 2
    H, WD = 24, 32
    c2w, focal = torch.as_tensor(create_spheric_poses(4.0)[11]), sapien_focal(H)
    rays = frame_rays(c2w, H, WD, focal)
    tmin, tmax = helper.get_ray_limits_box(rays["rays_o"], rays["rays_d"], 2)
    hit = ((tmax > tmin) & (tmax > 0)).reshape(-1)
    assert 0 < int(hit.sum()) < H * WD
    culled = render_rays(model, rays, 200, True, 2.0, 6.0, box_side_length=2, cull=True, maps=True)
    full = render_rays(model, rays, 200, True, 2.0, 6.0, box_side_length=2, cull=False, maps=True)
    for k in ("canonical", "motion", "motion_mag"):
        assert torch.equal(culled[k][hit], full[k][hit]), k
        assert not culled[k][~hit].any(), k  # a ray that misses the box: zeros
        assert culled[k][hit].abs().sum() > 0
    frame = render_frame(model, c2w, H, WD, focal, chunk=200, box_side_length=2, cull=True,
                         maps=True)
    assert tuple(frame.shape) == (H * WD, 12)
    assert torch.equal(frame[:, 5:8], culled["canonical"])
    assert torch.equal(frame[:, 8:11], culled["motion"])
    assert torch.equal(frame[:, 11], culled["motion_mag"])
    assert torch.equal(frame[:, 0:3], culled["comp_rgb"])
    unb = render_frame(model, c2w, H, WD, focal, chunk=200, maps=True)
    assert tuple(unb.shape) == (H * WD, 12)
    assert torch.equal(unb[:, :5], render_frame(model, c2w, H, WD, focal, chunk=200))


# ---------------------------------------------------------------------------- 5. range fallback
SCALE = 6000.0  # of deformations_linear.1.weight: as far as the pack's own weight limit allows
# (65504 / 64 = 1023 after the scale; xavier's bound for 128 x 128 is 0.153).  On samples 20 to
# 60 units out (hd0 up to ~13) that puts hd1 far past 65504 / 8 = 8188 (the oracle: ~55,000).
FAR = 10.0


def test_range_flag_falls_back_to_the_layer_by_layer_path(art):
    from aonerf import _lib as L
    from aonerf import level as _level
    from aonerf import two_level
    from aonerf.model_autodecoder import RANGE_WARNING

    net, lat, lat_cpu, _ = art
    sd = dict(W.art_state_dict(0))
    for pre in ("coarse_mlp.", "fine_mlp."):
        sd[f"{pre}deformations_linear.1.weight"] = sd[f"{pre}deformations_linear.1.weight"] * SCALE
    assert np.abs(sd["fine_mlp.deformations_linear.1.weight"]).max() < 1000.0
    load(net, sd)
    mlp = net.fine_mlp
    B, S = 9, 21
    o, d, t = rays_of(B, S)
    t = FAR * t
    rec = {}
    with torch.no_grad():  # the recipe's condition, from the oracle: a hidden activation is out
        O.art_mlp_forward(O.split_state_dict(sd)[1], O.cast_rays(t, o, d), O.pos_enc(d, 0, 4),
                          lat_cpu, record=rec)
    assert float(rec["hd"][1].max()) > 2 * 8188.0
    o, d, t = o.cuda(), d.cuda(), t.cuda()
    with pytest.warns(RuntimeWarning, match="fp16x3 range") as seen:
        xp, delta, mag = mlp.deform_rays(o, d, t, lat)
    assert [str(w.message) for w in seen] == [RANGE_WARNING]
    assert L.range_overflow([mlp._art_packed])  # the pack's status word reports it
    with two_level.switched([mlp], "fused", False), warnings.catch_warnings():
        warnings.simplefilter("error")
        xp2, delta2, mag2 = mlp.deform_rays(o, d, t, lat)
        # ... and the x' of the layer-by-layer forward itself (pos_enc(x') columns 0..2)
        N = B * S
        xyz = torch.empty((N, 3), device="cuda")
        L.call("aon_cast_rays", L.ptr(o), L.ptr(d), L.ptr(t), B, S, None, 0, L.ptr(xyz), 0, 0,
               None, L.stream(o.device))
        geo, P = _level.geo_of(mlp), mlp._pairs()
        fb = mlp._folded(P, lat)
        venc = torch.zeros((B, geo.nv), device="cuda")
        enc, _ = _level.art_forward(geo, P, fb.__getitem__, xyz, venc, S,
                                    _level.LayerBuffers(geo, N, xyz.device))
    assert torch.isfinite(xp).all() and torch.equal(xp, xp2)
    assert torch.equal(delta, delta2) and torch.equal(mag, mag2)
    assert torch.equal(xp.reshape(N, 3), enc[:, :3])

    # the render: one warning, and the maps of the layer-by-layer render
    rays = {"rays_o": o, "rays_d": d, "viewdirs": d}
    with torch.no_grad():
        with pytest.warns(RuntimeWarning, match="fp16x3 range") as seen:
            got = net(rays, False, True, 2.0 * FAR, 6.0 * FAR, lat, maps=True)[1][-1]
        assert len(seen) == 1
        with two_level.switched([net.coarse_mlp, mlp], "fused", False):
            want = net(rays, False, True, 2.0 * FAR, 6.0 * FAR, lat, maps=True)[1][-1]
    for k in want:
        assert torch.isfinite(got[k]).all() and torch.equal(got[k], want[k]), k


def test_canonical_to_rgb_feeds_to8b(art):
    from aonerf import interface

    net, lat, _, _ = art
    o, d, _ = rays_of(12, 1)
    rays = {"rays_o": o.cuda(), "rays_d": d.cuda(), "viewdirs": d.cuda()}
    with torch.no_grad():
        fine = net(rays, False, True, 2.0, 6.0, lat, maps=True)[1]
    img = interface.canonical_to_rgb(fine[-1]["canonical"], fine[1], box_side_length=2)
    assert tuple(img.shape) == (12, 3) and float(img.min()) >= 0.0 and float(img.max()) <= 1.0
    assert interface.to8b(img.reshape(3, 4, 3)).dtype == torch.uint8
