"""CPU-side checks of the mask-supervision losses (include/aonerf.h aon_loss_masked): a float64
torch restatement of the four formulas -- opacity_loss, opacity_loss_CE, opacity_loss_autorf
(reference model_autodecoder.py:703-766) and img2mse(rgb[mask], target[mask]) (:423-426) --
reproduces the losses and autograd gradients the REFERENCE gave in fp32
(tests/golden/opacity_loss.npz, written by tests/golden/make_golden_opacity.py), which pins the
fixture and the restatement to each other; and the C ABI declares, exports, binds and guards the
two new entry points.  No GPU needed.

The restatement and d_ref = |reference fp32 - fp64 restatement| per case are what the GPU gates
(tests/test_gpu_opacity_loss.py) use."""
import ctypes

import numpy as np
import pytest
import torch

KINDS = ("mse", "ce", "autorf")
LAMBDA = 0.05  # the reference autodecoder's opacity_lambda (model_autodecoder.py:720)
ULP = 2.0 ** -24  # one fp32 rounding, relative


def opacity_term(kind, acc0, acc1, m, lam=LAMBDA):
    """The opacity term on torch tensors of any float dtype (float64: the restatement); ``m`` is
    the 0 / 1 mask in the same dtype.  kind None -> 0."""
    if kind is None:
        return acc0.new_zeros(())
    if kind == "mse":
        return sum(((a.clamp(0, 1) - m) ** 2).mean() for a in (acc0, acc1))
    if kind == "ce":
        return lam * sum((a.clamp(min=0) - a * m + torch.log1p(torch.exp(-a.abs()))).mean()
                         for a in (acc0, acc1))
    assert kind == "autorf"
    fg = m != 0
    n, n_fg = m.numel(), int(fg.sum())
    n_bg = n - n_fg
    loss = acc0.new_zeros(())
    if n_bg > 0:
        loss = loss + acc0[~fg].mean() * (n_bg / n) + acc1[~fg].mean() * (n_bg / n)
    if n_fg > 0:  # the reference's fine term reads the COARSE opacity (model_autodecoder.py:761-763)
        loss = loss + 2 * ((n_fg / n) * (1 - acc0[fg]).mean())
    return loss


def masked_mse(pred, target, m):
    """img2mse(pred[mask], target[mask]) with the mask repeated over the 3 channels."""
    fg = m != 0
    return ((pred[fg] - target[fg]) ** 2).mean()


def restate(kind, acc0, acc1, mask, lam=LAMBDA):
    """float64 loss and gradients (numpy) of the opacity term on fp32 / uint8 numpy inputs."""
    a0, a1 = (torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True) for a in (acc0, acc1))
    m = torch.from_numpy(np.asarray(mask != 0, np.float64))
    if kind is None:
        return 0.0, np.zeros(len(mask)), np.zeros(len(mask))
    loss = opacity_term(kind, a0, a1, m, lam)
    g0, g1 = torch.autograd.grad(loss, (a0, a1), allow_unused=True)
    z = lambda g, a: (g if g is not None else torch.zeros_like(a)).numpy()  # noqa: E731
    return float(loss.detach()), z(g0, a0), z(g1, a1)


def restate_rgb(pred, target, mask, masked=True):
    """float64 loss and gradient of one level's colour loss (all rays when not ``masked``)."""
    p = torch.from_numpy(np.asarray(pred, np.float64)).requires_grad_(True)
    t = torch.from_numpy(np.asarray(target, np.float64))
    m = torch.from_numpy(np.asarray(mask != 0, np.float64)) if masked else torch.ones(len(pred))
    loss = masked_mse(p, t, m)
    (g,) = torch.autograd.grad(loss, (p,))
    return float(loss.detach()), g.numpy()


def case_inputs(G, name):
    return G[f"{name}__acc0"], G[f"{name}__acc1"], G[f"{name}__mask"]


def cases(G):
    return [str(c) for c in G["cases"]], [str(c) for c in G["rgb_cases"]]


def d_ref(G, name, kind):
    """(|d loss|, |d g0|, |d g1|) between the reference's fp32 values and the restatement."""
    loss, g0, g1 = restate(kind, *case_inputs(G, name))
    return (abs(float(G[f"{name}__{kind}_loss"]) - loss),
            np.abs(G[f"{name}__{kind}_g0"].astype(np.float64) - g0),
            np.abs(G[f"{name}__{kind}_g1"].astype(np.float64) - g1))


def d_ref_rgb(G, name, level):
    loss, g = restate_rgb(G[f"{name}__pred{level}"], G[f"{name}__target"], G[f"{name}__mask"])
    return (abs(float(G[f"{name}__rgb_loss{level}"]) - loss),
            np.abs(G[f"{name}__rgb_g{level}"].astype(np.float64) - g))


@pytest.fixture(scope="module")
def G(golden):
    return golden("opacity_loss.npz")


def test_fixture_has_the_cases(G):
    names, rgb = cases(G)
    sizes = {n: len(G[f"{n}__mask"]) for n in names}
    assert sorted(sizes.values()) == sorted([1, 255, 256, 257, 2047, 2049, 300, 300, 300, 64])
    assert not G["b300_bg__mask"].any() and G["b300_fg__mask"].all()
    assert 0 < G["b300_rgb__mask"].sum() < 300 and not G["b64_rgb_bg__mask"].any()
    assert rgb == ["b300_rgb", "b64_rgb_bg"]
    for n in names:
        a = np.concatenate([G[f"{n}__acc0"], G[f"{n}__acc1"]])
        assert a.min() >= -0.1 and a.max() <= 1.1
        if sizes[n] >= 255:  # the clamp has work to do on both sides
            assert (a < 0).any() and (a > 1).any()


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_reproduces_the_reference(G, kind):
    """d_ref <= B 2^-24 relative: an fp32 mean's worst-case bound (the reference's own rounding,
    not our code), for the loss and for every gradient element."""
    for name in cases(G)[0]:
        B = len(G[f"{name}__mask"])
        loss, g0, g1 = restate(kind, *case_inputs(G, name))
        dl, d0, d1 = d_ref(G, name, kind)
        print(f"{name} {kind}: loss {loss:.9g} d_ref {dl:.3e} ({dl / max(abs(loss), 1e-300) / ULP:.2f} ulp), "
              f"grad d_ref max {max(d0.max(), d1.max()):.3e}")
        assert dl <= B * ULP * abs(loss), (name, dl, loss)
        assert (d0 <= B * ULP * np.abs(g0)).all() and (d1 <= B * ULP * np.abs(g1)).all(), name


def test_restatement_reproduces_the_reference_masked_rgb(G):
    for level in range(2):
        loss, g = restate_rgb(G[f"b300_rgb__pred{level}"], G["b300_rgb__target"], G["b300_rgb__mask"])
        dl, dg = d_ref_rgb(G, "b300_rgb", level)
        n = 3 * int(G["b300_rgb__mask"].sum())
        assert dl <= n * ULP * abs(loss) and (dg <= n * ULP * np.abs(g)).all()
        bg = G["b300_rgb__mask"] == 0
        assert (G[f"b300_rgb__rgb_g{level}"][bg] == 0).all() and (g[bg] == 0).all()
        # no foreground ray: NaN loss, zero gradients -- in the reference and in the restatement
        loss, g = restate_rgb(G[f"b64_rgb_bg__pred{level}"], G["b64_rgb_bg__target"], G["b64_rgb_bg__mask"])
        assert np.isnan(loss) and np.isnan(G[f"b64_rgb_bg__rgb_loss{level}"])
        assert (g == 0).all() and (G[f"b64_rgb_bg__rgb_g{level}"] == 0).all()


def test_autorf_reads_the_coarse_opacity_twice(G):
    """The reference's slip, kept: no gradient reaches the fine level's foreground opacity."""
    fg = G["b300_rgb__mask"] != 0
    assert (G["b300_rgb__autorf_g1"][fg] == 0).all() and (G["b300_rgb__autorf_g1"][~fg] != 0).all()
    assert (G["b300_fg__autorf_g1"] == 0).all()


# ------------------------------------------------------------------------------ the C ABI
@pytest.fixture(scope="module")
def L():
    from aonerf import _lib

    return _lib


def test_symbols_declared_exported_and_bound(L):
    from test_capi import declared_symbols

    lib = L.lib()
    for s in ("aon_loss_masked", "aon_loss_masked_bwd"):
        assert s in declared_symbols(), f"{s} not declared in aonerf.h"
        assert hasattr(lib, s) and s in L._SIGNATURES, s
    assert lib.aon_abi_version() == L.ABI_VERSION == 13  # purely additive: no version change
    assert L.OPACITY == {None: 0, "mse": 1, "ce": 2, "autorf": 3}


def test_bad_arguments_refused_before_any_launch(L):
    p = ctypes.c_void_p(16)
    #        pred0 pred1 acc0 acc1 target mask B extra kind lambda mask_rgb out g0 g1 a0 a1 stream
    good = [p, p, p, p, p, p, 4, None, 1, 0.05, 0, p, p, p, p, p, None]
    bad = {"null acc0": {2: None}, "null acc1": {3: None}, "null mask": {5: None},
           "null out": {11: None}, "null pred1 alone": {1: None}, "null target alone": {4: None},
           "null grad_rgb0 alone": {12: None}, "B = 0": {6: 0}, "B < 0": {6: -3},
           "kind < 0": {8: -1}, "kind > 3": {8: 4}, "mse without grad_acc0": {14: None},
           "autorf without grad_acc1": {8: 3, 15: None},
           "nothing to compute": {0: None, 1: None, 4: None, 12: None, 13: None, 8: 0},
           "mask_rgb without colours": {0: None, 1: None, 4: None, 12: None, 13: None, 10: 1}}
    for what, change in bad.items():
        args = list(good)
        for i, v in change.items():
            args[i] = v
        with pytest.raises(ValueError, match="aon_loss_masked"):
            L.call("aon_loss_masked", *args)
    #         g0 g1 a0 a1 B g gl0 gl1 gop d0 d1 e0 e1 stream
    good = [p, p, p, p, 4, p, None, None, None, p, p, p, p, None]
    bad = {"null d_rgb1": {10: None}, "null grad_acc0": {2: None}, "B = 0": {4: 0},
           "no buffers": {0: None, 1: None, 2: None, 3: None, 9: None, 10: None, 11: None, 12: None}}
    for what, change in bad.items():
        args = list(good)
        for i, v in change.items():
            args[i] = v
        with pytest.raises(ValueError, match="aon_loss_masked_bwd"):
            L.call("aon_loss_masked_bwd", *args)


def test_python_surface_refuses_bad_requests():
    from aonerf import train, train_art

    with pytest.raises(ValueError, match="opacity"):
        train.masked_loss(None, None, None, None, None, None, opacity="l1")
    for fn in ("opacity_loss", "opacity_loss_CE", "opacity_loss_autorf"):
        assert callable(getattr(train_art, fn))
    with pytest.raises(ValueError, match="instance_mask"):
        train_art.training_step(None, None, {"target": None}, False, True, 2.0, 6.0, opacity="ce")
    with pytest.raises(ValueError, match="instance_mask"):
        train_art.training_step(None, None, {"target": None}, False, True, 2.0, 6.0, mask_rgb=True)
