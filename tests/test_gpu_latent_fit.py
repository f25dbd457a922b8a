"""Fitting latent codes with the MLPs frozen (aonerf/latent_fit.py; NeRF_AE_Art.forward(...,
latent_only=True)): the code gradients of the latent-only backward against the full backward on
the same frozen model (unchanged code) and against the fp32 oracle, the MLPs untouched by a fit,
and no GEMM launched.

A NeRF_AE_Art of the default widths (the fused kernels' geometry is fixed) on the first 5 rays of
the golden training batch: coarse 5 x 65 = 325 rows, fine 5 x 193 = 965, neither a multiple of
16; injected uniforms."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from oracle import weights as W
from test_gpu_art_train import _batch, _make, cuda, rel_err

pytestmark = pytest.mark.gpu

B = 5
KEYS = ("density", "color", "articulation")


def _small(g):
    """The golden batch's first B rays and their uniforms."""
    b = _batch(g)
    for k in ("rays_o", "rays_d", "viewdirs", "target"):
        b[k] = b[k][:B].contiguous()
    return b, cuda(g["u_coarse"][:B]), cuda(g["u_fine"][:B])


def _frozen(precision):
    from aonerf import latent_fit

    net, lib = _make(0, precision=precision)
    return latent_fit.freeze(net), lib


def _recorded(monkeypatch):
    """Every C entry point launched from here on, by name."""
    from aonerf import _lib as L

    names, call = [], L.call

    def spy(name, *args):
        names.append(name)
        return call(name, *args)

    monkeypatch.setattr(L, "call", spy)
    return names


@pytest.mark.parametrize("precision", ["f16x3", "bf16"])
def test_code_gradients_match_the_full_backward(golden, precision):
    """fit_step's code gradients vs training_step's on the same frozen model with
    latent_only=False (each level's 40 weight gradients computed and dropped): within 1e-4 of
    each tensor's max; same loss bit for bit (the forward is the same launches); the MLPs get
    no gradient at all."""
    from aonerf import latent_fit, train_art

    g = golden("art_train_step.npz")
    net, lib = _frozen(precision)
    batch, uc, uf = _small(g)
    start = lib(batch)
    grads, losses = {}, {}
    for arm in ("latent_only", "full"):
        codes = latent_fit.LatentCodes(init=start).cuda()
        if arm == "latent_only":
            loss, logs = latent_fit.fit_step(net, codes, batch, True, True, 2.0, 6.0, u_coarse=uc,
                                             u_fine=uf)
        else:
            loss, logs = train_art.training_step(net, lambda b: codes(), batch, True, True, 2.0,
                                                 6.0, u_coarse=uc, u_fine=uf)
        loss.backward()
        torch.cuda.synchronize()
        assert all(p.grad is None for p in net.parameters())
        grads[arm] = {k: v.grad.cpu().numpy() for k, v in codes().items()}
        losses[arm] = (loss.item(), logs["loss0"].item(), logs["loss1"].item(), logs["reg"].item())
    assert losses["latent_only"] == losses["full"]
    for k in KEYS:
        e = rel_err(grads["latent_only"][k], grads["full"][k])
        print(f"{precision} {k}: latent-only vs full backward {e:.2e} of max "
              f"{np.abs(grads['full'][k]).max():.3e}")
        assert np.abs(grads["full"][k]).max() > 0
        assert e <= 1e-4, (k, e)


def test_code_gradients_match_the_fp32_oracle(golden):
    """The f16x3 mode, teacher-forced as test_gpu_art_train.test_art_train_step_chain gates the
    latent gradients: the oracle's autograd at OUR sample positions, each code gradient within
    max(2 x the fp32 oracle's own distance from fp64, 1e-3) of the tensor's max."""
    from aonerf import latent_fit, train_art

    g = golden("art_train_step.npz")
    net, lib = _frozen("f16x3")
    batch, uc, uf = _small(g)
    codes = latent_fit.LatentCodes(init=lib(batch)).cuda()
    latents = codes()
    ret = net(batch, True, True, 2.0, 6.0, latents, u_coarse=uc, u_fine=uf,
              return_intermediates=True, latent_only=True)
    target = batch["target"]
    (train_art.img2mse(ret[1][0], target) + train_art.img2mse(ret[0][0], target)).backward()
    ref = {}
    for dtype in (torch.float32, torch.float64):
        rays = {k: torch.from_numpy(g[k][:B]).to(dtype) for k in ("rays_o", "rays_d", "viewdirs")}
        params = [{k: v.to(dtype) for k, v in p.items()}
                  for p in O.split_state_dict(W.art_state_dict(0))]
        lat = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in latents.items()}
        tgt = torch.from_numpy(g["target"][:B]).to(dtype)
        ref_loss = 0.0
        for level in range(2):
            t = ret[level][3]["t_vals"].cpu().to(dtype)
            comp = O.art_render_level(params, rays, t, level, True, lat)[0]
            ref_loss = ref_loss + O.img2mse(comp, tgt)
            np.testing.assert_allclose(ret[level][0].detach().cpu().numpy(), comp.detach().numpy(),
                                       rtol=0, atol=1e-5)
        ref_loss.backward()
        ref[dtype] = {k: v.grad.double().numpy() for k, v in lat.items()}
    for k in KEYS:
        env = rel_err(ref[torch.float32][k], ref[torch.float64][k])
        e = rel_err(latents[k].grad.cpu().numpy(), ref[torch.float32][k])
        print(f"latent {k}: ours {e:.2e}  oracle fp32-vs-fp64 {env:.2e}")
        assert e <= max(2 * env, 1e-3), (k, e, env)


def test_no_gemm_in_the_latent_only_backward(golden, monkeypatch):
    """The latent-only backward of both levels: the chain once and aon_art_latent_grad once per
    level, and no aon_gemm* / aon_colsum launch -- linalg's entry points raise while it runs.
    The full backward of the same step does launch them (so the spy would have seen one)."""
    from aonerf import latent_fit, level, linalg, train_art

    g = golden("art_train_step.npz")
    net, lib = _frozen("f16x3")
    batch, uc, uf = _small(g)
    start = lib(batch)

    def step(latent_only):
        codes = latent_fit.LatentCodes(init=start).cuda()
        timers = {}
        loss, _ = train_art.step_on_latents(net, codes, batch, True, True, 2.0, 6.0, u_coarse=uc,
                                            u_fine=uf, timers=timers, latent_only=latent_only)
        return loss, timers

    loss, timers = step(False)
    with monkeypatch.context() as m:
        names = _recorded(m)
        loss.backward()
    assert any(n.startswith("aon_gemm") for n in names)
    assert "aon_art_latent_grad" not in names and "art_dlatent65" not in timers

    def refuse(*a, **k):
        raise AssertionError("a GEMM entry point ran in a latent_only backward")

    loss, timers = step(True)
    with monkeypatch.context() as m:
        for mod, name in ((linalg, "gemm"), (level, "gemm"), (train_art, "gemm"),
                          (linalg, "_flush"), (linalg, "_flush_small"), (linalg, "colsum")):
            m.setattr(mod, name, refuse)
        names = _recorded(m)
        loss.backward()
        torch.cuda.synchronize()
    assert not [n for n in names if n.startswith("aon_gemm") or n == "aon_colsum"], names
    assert names.count("aon_art_latent_grad") == 2 and names.count("aon_mlp_art_bwd") == 2
    assert {"art_dlatent65", "art_dlatent193", "art_bwd_chain65", "art_bwd_chain193"} <= set(timers)
    assert not [k for k in timers if k.startswith("art_dweight")]


LR, STEPS = 1e-2, 10


def test_fit_moves_the_codes_and_nothing_else(golden):
    """10 fit steps (lr 1e-2, randomized=False) on one fixed batch whose target is the model's
    own render under OTHER codes (instance 11 / articulation 5 of the seed library), starting from
    the batch's own row: a zero-colour-loss solution exists.  Every MLP parameter stays bit for
    bit, all three codes move, and the randomized=False loss falls.
    lr and the step count were chosen on the MI355X, first try: lr 1e-2 is a tenth of the seed
    codes' spread (xavier, |x| <= 0.15) per Adam step; the loss went 8.817936e-04 -> 3.882997e-04,
    falling at every step (8.82, 8.24, 7.70, 7.09, 6.55, 6.02, 5.49, 4.99, 4.59, 4.26 e-04)."""
    from aonerf import latent_fit

    g = golden("art_train_step.npz")
    net, lib = _frozen("f16x3")
    batch, _, _ = _small(g)
    other = dict(batch, instance_id=torch.tensor([11], device="cuda"),
                 articulation_id=torch.tensor([5], device="cuda"))
    assert int(g["instance_id"]) != 11 and int(g["articulation_id"]) != 5
    with torch.no_grad():
        batch["target"] = net(batch, False, True, 2.0, 6.0, lib(other))[1][0].clone()
    codes = latent_fit.LatentCodes(init=lib(batch)).cuda()
    start = {k: v.detach().clone() for k, v in codes().items()}
    before = [p.detach().clone() for p in net.parameters()]

    def eval_loss():
        loss, _ = latent_fit.fit_step(net, codes, batch, False, True, 2.0, 6.0)
        return loss.item()

    loss0 = eval_loss()
    losses = latent_fit.fit(net, codes, [batch] * STEPS, LR, False, True, 2.0, 6.0)
    loss1 = eval_loss()
    print(f"fit: lr {LR}, {STEPS} steps: loss {loss0:.6e} -> {loss1:.6e}; per step "
          f"{[round(x.item(), 8) for x in losses]}")
    assert len(losses) == STEPS and losses[0].item() == loss0
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), before))
    assert all(p.grad is None for p in net.parameters())
    for k, v in codes().items():
        assert not torch.equal(v.detach(), start[k]), f"{k} did not move"
        assert torch.isfinite(v).all()
    assert loss1 < loss0, (loss0, loss1)
