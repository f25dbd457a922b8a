"""The two-pass f16x3 render (include/aonerf.h aon_mlp_fwd_sigma / aon_mlp_fwd_cond;
NeRF.forward(fine_only=True), which render_frame and render_rays pass).

A render that keeps only the fine level needs the coarse level's sigma alone -- its colour reaches
nothing -- and the per-ray view encodings once per ray, not once per sample.  Both changes remove
work and leave every kept bit where it was, so every check here is equality with the one-pass
kernels: no tolerance anywhere.
"""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu

# every way a 16-row tile and a 128-row workgroup can be cut: one row; tiles spanning several rays
# ((13, 5): four rays with different view directions per tile); one row short of / past a
# workgroup; several workgroups with a partial last tile
SHAPES = [(1, 1), (13, 5), (1, 127), (1, 129), (3, 65), (7, 193)]
GUARD = 256       # rows behind the output that no launch may touch
SENTINEL = -777.0


@functools.lru_cache(maxsize=None)
def _golden_sd():
    return W.nerf_state_dict(0)


def _mlp(p):
    from aonerf.model import NeRFMLP

    m = NeRFMLP(0, 10, 4).cuda()
    m.load_state_dict({k: torch.as_tensor(v) for k, v in p.items()})
    return m.requires_grad_(False)


def _nerf(sd, **kw):
    from aonerf.model import NeRF

    net = NeRF(**kw).cuda()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return net.requires_grad_(False).eval()


@functools.lru_cache(maxsize=None)
def _fine_mlp():
    return _mlp(O.split_state_dict(_golden_sd())[1])


def _status(mlp):
    from aonerf import _lib as L

    packed = mlp._packed
    st = ctypes.c_uint32(7)
    L.call("aon_mlp_read_status", L.ptr(packed), packed.numel() * 4, ctypes.byref(st),
           L.stream(packed.device))
    return st.value


def _guarded(N):
    buf = torch.full((N + GUARD, 4), SENTINEL, device="cuda")
    return buf, buf[:N]


@functools.lru_cache(maxsize=None)
def _case(B, S, act):
    """Inputs of one shape (view directions independent of the ray directions, so neighbouring
    rays of a tile differ in both) and aon_mlp_fwd's output on them: the reference, computed once
    and never written again."""
    from aonerf import _lib as L

    gen = torch.Generator().manual_seed(1000 * B + S)
    o = ((torch.rand(B, 3, generator=gen) - 0.5) * 2.0).cuda()
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1).cuda()
    v = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1).cuda()
    t = (2.0 + 4.0 * torch.rand(B, S, generator=gen)).sort(-1).values.cuda()
    packed = _fine_mlp().packed_weights()
    ref = torch.empty((B * S, 4), device="cuda")
    L.call("aon_mlp_fwd", L.ptr(packed), L.PREC["f16x3"], L.ptr(o), L.ptr(d), L.ptr(v), L.ptr(t),
           B, S, act, L.ptr(ref), L.stream(ref.device))
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all()
    return o, d, v, t, ref


@pytest.mark.parametrize("act", [0, 1], ids=["act_none", "act_vanilla"])
@pytest.mark.parametrize("B,S", SHAPES)
def test_sigma_equals_the_full_kernels_sigma(B, S, act):
    from aonerf import _lib as L

    o, d, v, t, ref = _case(B, S, act)
    packed = _fine_mlp().packed_weights()
    buf, out = _guarded(B * S)
    L.call("aon_mlp_fwd_sigma", L.ptr(packed), L.PREC["f16x3"], L.ptr(o), L.ptr(d), L.ptr(t), B, S,
           act, L.ptr(buf), L.stream(buf.device))
    torch.cuda.synchronize()
    assert torch.equal(out[:, 3], ref[:, 3])
    assert torch.equal(out[:, :3], torch.zeros_like(out[:, :3]))
    assert torch.equal(buf[B * S:], torch.full_like(buf[B * S:], SENTINEL)), "rows past B*S written"
    assert _status(_fine_mlp()) == 0
    # NeRFMLP.forward_sigma is this entry point
    assert torch.equal(_fine_mlp().forward_sigma(o, d, t, act=act), out)


@pytest.mark.parametrize("act", [0, 1], ids=["act_none", "act_vanilla"])
@pytest.mark.parametrize("B,S", SHAPES)
def test_cond_equals_the_full_kernel(B, S, act):
    from aonerf import _lib as L
    from aonerf import helper

    o, d, v, t, ref = _case(B, S, act)
    packed = _fine_mlp().packed_weights()
    cond = helper.pos_enc(v, 0, 4)
    assert cond.shape == (B, 27)
    buf, out = _guarded(B * S)
    L.call("aon_mlp_fwd_cond", L.ptr(packed), L.PREC["f16x3"], L.ptr(o), L.ptr(d), L.ptr(cond),
           L.ptr(t), B, S, act, L.ptr(buf), L.stream(buf.device))
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert torch.equal(buf[B * S:], torch.full_like(buf[B * S:], SENTINEL)), "rows past B*S written"
    assert _status(_fine_mlp()) == 0
    assert torch.equal(_fine_mlp().forward_rays(o, d, v, t, act=act, cond=cond), ref)


# ------------------------------------------------------------------ range guard
def _golden_rays(golden):
    g = golden("forward_eval.npz")
    rays = {k: torch.from_numpy(g[k]).cuda() for k in ("rays_o", "rays_d", "viewdirs")}
    return rays, torch.from_numpy(np.ascontiguousarray(g["coarse_t"])).cuda()


def test_trunk_overflow_reported_by_the_sigma_pass(golden):
    """tests/test_gpu_range.py's recipe: pts_linears.0 scaled until the largest hidden activation
    is ~1.2e4 > 8188.  The trunk is all of the density-only pass: it must report."""
    from test_gpu_range import _scaled

    _, sd, _, m = _scaled(golden, 1.2e4)
    assert m > 1.0e4
    net = _nerf(sd)
    rays, t = _golden_rays(golden)
    net.coarse_mlp.packed_weights()
    assert _status(net.coarse_mlp) == 0
    net.coarse_mlp.forward_sigma(rays["rays_o"], rays["rays_d"], t)
    assert _status(net.coarse_mlp) == 1


def test_view_layer_overflow_is_not_the_sigma_passs(golden):
    """views_linear.0.bias = 1e4: the view layer's ReLU outputs sit near 1e4, past the range, and
    nothing else moves (the trunk and the density head do not read that bias).  aon_mlp_fwd splits
    those outputs for the rgb head and reports; the density-only pass never forms them."""
    sd = dict(_golden_sd())
    for lv in ("coarse_mlp", "fine_mlp"):
        sd[f"{lv}.views_linear.0.bias"] = np.full((128,), 1.0e4, np.float32)
    net = _nerf(sd)
    rays, t = _golden_rays(golden)
    o, d, v = rays["rays_o"], rays["rays_d"], rays["viewdirs"]
    full = net.coarse_mlp.forward_rays(o, d, v, t)
    assert _status(net.coarse_mlp) == 1  # the recipe does overflow the view layer
    net.coarse_mlp._packed_key = None    # repack: the status word is cleared
    net.coarse_mlp.packed_weights()
    assert _status(net.coarse_mlp) == 0
    sig = net.coarse_mlp.forward_sigma(o, d, t)
    assert _status(net.coarse_mlp) == 0
    assert torch.equal(sig[:, 3], full[:, 3])  # sigma never depended on the view layer


# ------------------------------------------------------------------ end to end
H, WD = 12, 16


def _frame_rays():
    from aonerf.ray_utils import frame_rays
    from aonerf.render import create_spheric_poses, sapien_focal

    c2w = create_spheric_poses(4.0)[5]
    return c2w, sapien_focal(H), frame_rays(c2w, H, WD, sapien_focal(H))


def test_render_frame_equals_the_one_pass_forward():
    from aonerf.render import render_frame, render_rays

    net = _nerf(_golden_sd())
    c2w, focal, rays = _frame_rays()
    fine = net(rays, False, True, 2.0, 6.0)[1]
    frame = render_frame(net, c2w, H, WD, focal)
    assert frame.shape == (H * WD, 5)
    assert torch.equal(frame[:, 0:3], fine[0])
    assert torch.equal(frame[:, 3], fine[2])
    assert torch.equal(frame[:, 4], fine[1])
    out = render_rays(net, rays, None, True, 2.0, 6.0)
    assert all(torch.equal(out[k], x) for k, x in zip(("comp_rgb", "acc", "depth"), fine))
    # the forward itself: the coarse level is not returned, the fine level is the same
    ret = net(rays, False, True, 2.0, 6.0, fine_only=True)
    assert ret[0] is None and all(torch.equal(a, b) for a, b in zip(ret[1], fine))
    # asking for weights or intermediates is the one-pass forward, whatever fine_only says
    ret = net(rays, False, True, 2.0, 6.0, fine_only=True, return_weights=True)
    assert ret[0] is not None and len(ret[0]) == 4 and torch.equal(ret[1][0], fine[0])
    # the timers keep their keys
    timers = {}
    net(rays, False, True, 2.0, 6.0, fine_only=True, timers=timers)
    assert sorted(timers) == ["comp1", "march0", "mlp0", "mlp1"]


def test_seeded_randomized_forward_keeps_its_draws():
    """Density noise (noise_std > 0) and stratified / inverse-CDF uniforms: the same bits with and
    without fine_only, and the generator left in the same state (the reference's draw order:
    coarse t, coarse noise, fine u, fine noise)."""
    net = _nerf(_golden_sd(), noise_std=1.0)
    _, _, rays = _frame_rays()
    outs, states = [], []
    for fine_only in (False, True):
        torch.manual_seed(5)
        outs.append(net(rays, True, False, 2.0, 6.0, fine_only=fine_only)[1])
        states.append(torch.cuda.get_rng_state(rays["rays_o"].device))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert torch.equal(states[0], states[1])
    torch.manual_seed(6)  # and the draws matter: another seed is another frame
    assert not torch.equal(net(rays, True, False, 2.0, 6.0, fine_only=True)[1][0], outs[0][0])


def test_fp32_fallback_is_the_same_on_both_paths(golden):
    """A trunk overflow (tests/test_gpu_range.py's recipe) on the golden rays: both paths warn
    with the same text, re-render on the fp32 kernels and return the same fine level."""
    from test_gpu_range import _scaled

    _, sd, _, _ = _scaled(golden, 1.2e4)
    net = _nerf(sd)
    rays, _ = _golden_rays(golden)
    outs, texts = [], []
    for fine_only in (False, True):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            outs.append(net(rays, False, True, 2.0, 6.0, fine_only=fine_only)[1])
        texts.append([str(x.message) for x in w])
        assert net.coarse_mlp.precision == net.fine_mlp.precision == "f16x3"  # restored
    assert texts[0] == texts[1] and any("fp16x3 range" in s for s in texts[0])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    # and it is the fp32 render
    fp32 = _nerf(sd, precision="fp32")(rays, False, True, 2.0, 6.0)[1]
    assert all(torch.equal(a, b) for a, b in zip(outs[1], fp32))


def test_two_pass_render_replays_from_a_graph():
    """sample -> density-only MLP -> march -> view encodings -> conditioned MLP -> composite on
    one stream (a single chain) captured into a HIP graph, as the one-pass render is in
    tests/test_gpu_parity.py: the replay equals the eager launches bit for bit."""
    net = _nerf(_golden_sd())
    _, _, rays = _frame_rays()

    def render():
        out = net(rays, False, True, 2.0, 6.0, fine_only=True)[1]
        return torch.cat([out[0], out[1][:, None], out[2][:, None]], -1)

    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):  # warm-up: code objects loaded, weights packed
        eager = render()
        render()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = render()
    for _ in range(2):
        captured.zero_()
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)
