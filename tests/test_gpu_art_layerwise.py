"""The articulated network layer by layer has two callers -- the render's fallback
(NeRFMLP(fused=False): forward_rays / forward, two alternating buffers per width) and the
training path's layer-by-layer forward (train_art._forward_level, one kept tensor per layer).
Both walk aonerf.level.art_forward; this pins them to each other bit for bit in the f16x3 mode,
on the golden weights with non-zero latent codes, at 3 rays x 7 samples (21 rows: one full
16-row tile and a ragged one)."""
import numpy as np
import pytest
import torch

from oracle import weights as W

pytestmark = pytest.mark.gpu


def test_render_fallback_equals_training_forward(golden):
    from aonerf import _lib as L
    from aonerf import train_art
    from aonerf.model_autodecoder import NeRF_AE_Art

    g = golden("articulated.npz")
    net = NeRF_AE_Art().cuda()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in W.art_state_dict(0).items()})
    mlp = net.fine_mlp
    mlp.fused = False
    lat = {k: torch.from_numpy(np.ascontiguousarray(g[f"latent_{k}"])).cuda()
           for k in ("density", "color", "articulation")}
    assert all(float(v.abs().max()) > 0 for v in lat.values())
    B, S = 3, 7
    gen = torch.Generator().manual_seed(11)
    o = (torch.rand(B, 3, generator=gen) - 0.5).cuda()
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1).cuda()
    t = (2.0 + 4.0 * torch.rand(B, S, generator=gen)).sort(-1).values.cuda()
    with torch.no_grad():
        raw_rays = mlp.forward_rays(o, d, d, t, lat)
        # the same sample points and view encodings, from the kernels forward_rays runs
        xyz = torch.empty((B * S, 3), device="cuda")
        L.call("aon_cast_rays", L.ptr(o), L.ptr(d), L.ptr(t), B, S, None, 0, L.ptr(xyz), 0, 0, None,
               L.stream(xyz.device))
        venc = torch.empty((B, 27), device="cuda")
        L.call("aon_pos_enc", L.ptr(d), B, 0, 4, L.ptr(venc), L.stream(xyz.device))
        rgb, sigma = mlp(xyz.view(B, S, 3), venc, lat)
        P = [(m.weight.detach(), m.bias.detach()) for m in train_art.art_layers(mlp)]
        codes = tuple(lat[k].reshape(1, -1) for k in ("density", "color", "articulation"))
        raw_train = torch.empty((B * S, 4), device="cuda")
        train_art._forward_level(train_art._Geo(mlp), P, codes, xyz, venc, S, raw_train)
    torch.cuda.synchronize()
    assert torch.isfinite(raw_rays).all() and float(raw_rays.abs().max()) > 0
    assert torch.equal(raw_rays, raw_train)
    assert torch.equal(torch.cat([rgb, sigma], -1).reshape(-1, 4), raw_rays)
