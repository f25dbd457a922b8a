"""The f16x3 render stream folds bottleneck_layer into views_linear.0 (csrc/mlp_layout.hpp
kLayoutHFold): bottleneck_layer has no activation and feeds only the view layer, so

    z_view = (Wv[:, :256] Wb) h7 + Wv[:, 256:] enc_dir + (bv + Wv[:, :256] bb)

and the pack forms W' and b' (fp64 sums, one rounding to fp32).  The render kernels then run no
bottleneck layer; the training forwards keep the unfolded stream.

``exact`` below is the network (reference model.py:95-120, oracle.mlp_forward) in fp64 torch on
the CPU from the same fp32 parameters and the kernel's own inputs: the fp32 sample points
o + t d, pos_enc with its sin arguments rounded as fp32 arithmetic rounds them and the sin
rounded to fp32 (the kernels' sin is correctly rounded), then every GEMM in fp64.  The gate is
the project's raw gate of tests/test_gpu_parity.py, 1e-5 absolute on the pre-activation outputs
(scaled by the largest |raw| where that exceeds 1).

Measured on MI355X (golden weights, the 256 rays of forward_eval.npz, S = 65), max |raw - exact|:
coarse MLP folded 2.98e-07 / unfolded training forward 2.98e-07, fine MLP 2.72e-07 / 2.72e-07
(folded and unfolded rgb differ by at most 1.8e-07).  Before
the fold the render's raw was bit-equal to the training forward's on these inputs; the sigma
column still is.
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

GATE = 1e-5  # tests/test_gpu_parity.py: the MLP raw outputs


def _enc64(xyz, lo, hi):
    """pos_enc at fp32 points as the kernels form it: fp32 sin arguments, sin correctly rounded
    to fp32 -- as fp64 values."""
    return O.pos_enc_at(xyz, xyz.double(), lo, hi).float().double()


def _exact_encoded(p, enc, venc):
    """(B*S, 4) fp64 [raw_rgb, raw_sigma] from encoded inputs enc (B, S, 63), venc (B, 27)."""
    p64 = {k: v.double() for k, v in p.items()}
    rgb, sig = O.mlp_forward(p64, enc.double(), venc.double())
    return torch.cat([rgb.reshape(-1, 3), sig.reshape(-1, 1)], -1)


def _exact_rays(p, o, d, v, t):
    xyz = O.cast_rays(t, o, d)  # fp32: one multiply, one add, as the kernel's
    return _exact_encoded(p, _enc64(xyz, 0, 10), _enc64(v, 0, 4))


def _mlp(p):
    from aonerf.model import NeRFMLP

    m = NeRFMLP(0, 10, 4).cuda()
    m.load_state_dict({k: torch.as_tensor(v) for k, v in p.items()})
    return m.requires_grad_(False)


def _status(mlp):
    from aonerf import _lib as L

    packed = mlp._packed
    st = ctypes.c_uint32(7)
    L.call("aon_mlp_read_status", L.ptr(packed), packed.numel() * 4, ctypes.byref(st),
           L.stream(packed.device))
    return st.value


def _err(raw, exact):
    return float((raw.double().cpu() - exact).abs().max())


@functools.lru_cache(maxsize=None)
def _golden_params():
    return O.split_state_dict(W.nerf_state_dict(0))


# ------------------------------------------------------------------ parity at the golden weights
@pytest.mark.parametrize("level", [0, 1], ids=["coarse", "fine"])
def test_parity_golden(golden, level):
    """Folded render raw and the unfolded training forward's raw against exact: 256 rays x 65
    samples.  The density head does not see the fold, and on the parent commit the render's raw
    was bit-equal to the training forward's (checked there on these inputs): sigma stays so."""
    from aonerf import train

    g = golden("forward_eval.npz")
    p = _golden_params()[level]
    o, d, v = (torch.from_numpy(g[k]) for k in ("rays_o", "rays_d", "viewdirs"))
    t = torch.from_numpy(np.ascontiguousarray(g["coarse_t"]))
    assert t.shape == (256, 65)
    exact = _exact_rays(p, o, d, v, t)
    mlp = _mlp(p)
    og, dg, vg, tg = (x.cuda() for x in (o, d, v, t))
    raw = mlp.forward_rays(og, dg, vg, tg)
    P = [(m.weight.detach(), m.bias.detach()) for m in mlp._layers()]
    raw_t = torch.empty_like(raw)
    train._forward_level_fused(P, og, dg, vg, tg, raw_t)
    torch.cuda.synchronize()
    e_fold, e_train = _err(raw, exact), _err(raw_t, exact)
    print(f"level {level}: max |raw - exact| folded render {e_fold:.3e}, unfolded training "
          f"forward {e_train:.3e}; folded vs unfolded rgb {float((raw - raw_t)[:, :3].abs().max()):.3e}")
    assert _status(mlp) == 0
    assert torch.isfinite(raw).all()
    assert e_fold <= GATE
    assert e_train <= GATE
    assert torch.equal(raw[:, 3], raw_t[:, 3]), "the density head must not see the fold"


# ------------------------------------------------------------------ ragged shapes, modes, acts
SHAPES = [(1, 1), (1, 129), (3, 193), (1237, 65)]


@functools.lru_cache(maxsize=None)
def _ragged(B, S):
    gen = torch.Generator().manual_seed(1000 * B + S)
    o = (torch.rand(B, 3, generator=gen) - 0.5) * 2.0
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1)
    t = (2.0 + 4.0 * torch.rand(B, S, generator=gen)).sort(-1).values
    p = _golden_params()[1]
    xyz = O.cast_rays(t, o, d)
    enc, venc = _enc64(xyz, 0, 10).float(), _enc64(d, 0, 4).float()
    return o, d, t, enc, venc, _exact_encoded(p, enc, venc)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("B,S", SHAPES)
def test_ragged_shapes_modes_acts(B, S, act):
    """1 sample, one sample past a 128-row workgroup, several workgroups with a partial last one,
    and 80,405 rows; through aon_mlp_fwd (rays + t) and aon_mlp_fwd_encoded."""
    from aonerf import _lib as L

    o, d, t, enc, venc, exact = _ragged(B, S)
    mlp = _mlp(_golden_params()[1])
    packed = mlp.packed_weights()
    og, dg, tg, eg, vg = (x.cuda().contiguous() for x in (o, d, t, enc, venc))
    outs = {}
    for name in ("aon_mlp_fwd", "aon_mlp_fwd_encoded"):
        raw = torch.full((B * S, 4), float("nan"), device="cuda")
        if name == "aon_mlp_fwd":
            L.call(name, L.ptr(packed), L.PREC["f16x3"], L.ptr(og), L.ptr(dg), L.ptr(dg), L.ptr(tg),
                   B, S, act, L.ptr(raw), L.stream(raw.device))
        else:
            L.call(name, L.ptr(packed), L.PREC["f16x3"], L.ptr(eg), L.ptr(vg), B, S, act,
                   L.ptr(raw), L.stream(raw.device))
        outs[name] = raw
    torch.cuda.synchronize()
    assert _status(mlp) == 0
    for name, raw in outs.items():
        assert torch.isfinite(raw).all(), name
        if act == 0:
            e = _err(raw, exact)
            print(f"{name} ({B}, {S}): max |raw - exact| {e:.3e}")
            assert e <= GATE, name
    if act == 0:  # NeRFMLP.forward is aon_mlp_fwd_encoded with no activation
        rgb, sig = mlp(eg.view(B, S, 63), vg)
        assert torch.equal(torch.cat([rgb, sig], -1).view(-1, 4), outs["aon_mlp_fwd_encoded"])


# ------------------------------------------------------------------ the fold itself
def test_fold_terms_cannot_hide(golden):
    """Weights under which a wrong fold shows: the bottleneck bias x 50 (b' must carry
    Wv[:, :256] bb), different magnitudes on the bottleneck and enc_dir column blocks of
    views_linear.0 (a fold applied to the wrong columns, or to all of them), a non-zero view bias."""
    g = golden("forward_eval.npz")
    p = dict(_golden_params()[1])
    gen = torch.Generator().manual_seed(7)
    p["bottleneck_layer.bias"] = (p["bottleneck_layer.bias"] + 0.02 * torch.randn(256, generator=gen)) * 50.0
    wv = p["views_linear.0.weight"].clone()
    wv[:, :256] *= 3.7
    wv[:, 256:] *= 0.31
    p["views_linear.0.weight"] = wv
    p["views_linear.0.bias"] = 0.5 * torch.randn(128, generator=gen)
    o, d, v = (torch.from_numpy(g[k])[:64] for k in ("rays_o", "rays_d", "viewdirs"))
    t = torch.from_numpy(np.ascontiguousarray(g["coarse_t"]))[:64]
    exact = _exact_rays(p, o, d, v, t)
    mlp = _mlp(p)
    raw = mlp.forward_rays(o.cuda(), d.cuda(), v.cuda(), t.cuda())
    scale = max(1.0, float(exact.abs().max()))
    e = _err(raw, exact)
    # an unfolded bias or a mis-scaled column block moves raw rgb by far more than the gate
    print(f"fold terms: max |raw - exact| {e:.3e}, largest |raw| {scale:.3f}")
    assert _status(mlp) == 0
    assert e <= GATE * scale


# ------------------------------------------------------------------ range guard
def _ok(err, acc):
    """tests/test_gpu_range.py _ok: within 1e-4 of the fp32 reference, or no farther from a more
    accurate evaluation of the reference than 2x the reference's own fp32 result is."""
    ours, theirs = acc
    return err <= 1e-4 or ours <= max(1e-4, 2.0 * theirs)


def _coarse_vs_oracle(net, g, params):
    """As tests/test_gpu_range.py: the coarse rgb / acc / weights of NeRF.forward against the
    oracle, the warnings raised, and both distances from the oracle's more accurate evaluation."""
    from oracle import attribution as A

    rays = {k: torch.from_numpy(g[k]).cuda() for k in ("rays_o", "rays_d", "viewdirs")}
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ret = net(rays, False, True, 2.0, 6.0, return_weights=True, return_intermediates=True)
    rc = {k: v.cpu() for k, v in rays.items()}
    t = ret[0][4]["t_vals"].cpu()
    gpu = [ret[0][0].cpu(), ret[0][1].cpu(), ret[0][3].cpu()]

    def dist(a, b):
        return max(float((x - y).abs().max()) for x, y in zip(a, b))

    ref = O.render_level(params, rc, t, 0, True)[:3]
    v = A.oracle_variants()
    with v["fp64_gemm"](), v["sin_cr"](), v["exp_cr"]():
        acc = O.render_level(params, rc, t, 0, True)[:3]
    return dist(gpu, ref), [str(x.message) for x in w], (dist(gpu, acc), dist(ref, acc))


def _nerf(sd):
    from aonerf.model import NeRF

    net = NeRF().cuda()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.requires_grad_(False)


def test_guard_tests_the_folded_weight(golden):
    """Wb and Wv[:, :256] constant 30: each holds at the 2^6 weight scale (30 * 64 = 1920), their
    product 256 * 900 = 230,400 does not (1.5e7 > 65504) -- the pack reports 2, and NeRF.forward
    warns and renders on the fp32 kernels."""
    g = golden("forward_eval.npz")
    sd = dict(W.nerf_state_dict(0))
    for lv in ("coarse_mlp", "fine_mlp"):
        sd[f"{lv}.bottleneck_layer.weight"] = np.full((256, 256), 30.0, np.float32)
        wv = sd[f"{lv}.views_linear.0.weight"].copy()
        wv[:, :256] = 30.0
        sd[f"{lv}.views_linear.0.weight"] = wv
    net = _nerf(sd)
    net.coarse_mlp.packed_weights()
    torch.cuda.synchronize()
    assert _status(net.coarse_mlp) == 2
    params = O.split_state_dict(sd)
    err, warns, acc = _coarse_vs_oracle(net, g, params)
    print(f"fallback render: max |gpu - oracle| {err:.2e}; from the accurate evaluation: gpu "
          f"{acc[0]:.2e}, reference fp32 {acc[1]:.2e}; warnings {warns}")
    assert any("fp16x3 range" in w for w in warns)
    assert net.coarse_mlp.precision == "f16x3"  # restored after the fallback
    assert _ok(err, acc)


def _max_bottleneck(p, enc):
    x = enc.reshape(-1, enc.shape[-1])
    inputs = x
    for i in range(8):
        x = torch.relu(x @ p[f"pts_linears.{i}.weight"].T + p[f"pts_linears.{i}.bias"])
        if i == 4:
            x = torch.cat([x, inputs], -1)
    return float((x @ p["bottleneck_layer.weight"].T + p["bottleneck_layer.bias"]).abs().max())


def test_large_bottleneck_no_longer_matters(golden):
    """Wb, bb x F and Wv[:, :256] / F: the bottleneck activation leaves the fp16x3 range
    (|x| > 8188) while W' and b' are unchanged -- F is a power of two, so they are the same
    bits.  The render has no bottleneck activation to split: status 0, raw within the gate.
    F: the smallest power of two that takes the oracle's largest |bottleneck| past 1e4."""
    g = golden("forward_eval.npz")
    sd = dict(W.nerf_state_dict(0))
    p0 = _golden_params()[0]
    o, d, v = (torch.from_numpy(g[k]) for k in ("rays_o", "rays_d", "viewdirs"))
    t = torch.from_numpy(np.ascontiguousarray(g["coarse_t"]))
    enc = O.pos_enc(O.cast_rays(t, o, d), 0, 10)
    m = _max_bottleneck(p0, enc)
    F = np.float32(2.0 ** int(np.ceil(np.log2(1.0e4 / m))))
    for lv in ("coarse_mlp", "fine_mlp"):
        sd[f"{lv}.bottleneck_layer.weight"] = sd[f"{lv}.bottleneck_layer.weight"] * F
        sd[f"{lv}.bottleneck_layer.bias"] = sd[f"{lv}.bottleneck_layer.bias"] * F
        wv = sd[f"{lv}.views_linear.0.weight"].copy()
        wv[:, :256] /= F
        sd[f"{lv}.views_linear.0.weight"] = wv
    params = O.split_state_dict(sd)
    big = _max_bottleneck(params[0], enc)
    print(f"largest |bottleneck| {m:.2f} -> {big:.1f} (F = {F:g})")
    assert big > 8188.0
    exact = _exact_rays(params[0], o, d, v, t)
    net = _nerf(sd)
    raw = net.coarse_mlp.forward_rays(o.cuda(), d.cuda(), v.cuda(), t.cuda())
    torch.cuda.synchronize()
    e = _err(raw, exact)
    print(f"max |raw - exact| {e:.3e}")
    assert _status(net.coarse_mlp) == 0
    assert e <= GATE
    # the same bits as the unscaled weights give: W' and b' did not change
    raw0 = _mlp(p0).forward_rays(o.cuda(), d.cuda(), v.cuda(), t.cuda())
    assert torch.equal(raw, raw0)
    err, warns, acc = _coarse_vs_oracle(net, g, params)
    assert not warns and err <= 1e-4


# ------------------------------------------------------------------ determinism
def test_pack_is_deterministic():
    mlp = _mlp(_golden_params()[1])
    a = mlp.packed_weights().view(torch.int32).clone()
    mlp._packed_key = None
    b = mlp.packed_weights().view(torch.int32)
    torch.cuda.synchronize()
    assert a.data_ptr() != b.data_ptr()
    assert torch.equal(a, b)
    from aonerf import _lib as L

    assert a.numel() * 4 == L.lib().aon_mlp_packed_bytes(L.PREC["f16x3"])
