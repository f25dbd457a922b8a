"""GPU gates of mask-supervised training: aon_loss_masked / aon_loss_masked_bwd
(include/aonerf.h; reference opacity_loss / opacity_loss_CE / opacity_loss_autorf,
model_autodecoder.py:703-766, and img2mse(rgb[mask], target[mask]), :423-426) and the
`opacity` / `mask_rgb` arguments of train_art.training_step.

Tolerances (fixed before any GPU run):
  kernel vs the float64 restatement (tests/test_opacity_loss_golden.py): every loss scalar and
    every gradient element within 4 fp32 ulps (4 x 2^-24 relative) -- by construction at most
    three fp32 roundings separate them (the fp32 subtract or scale, the product, the final
    store), plus one spare;
  kernel vs the reference's fp32 fixture: |ours - reference| <= d_ref + 4 ulps, d_ref the
    reference's own distance to the restatement (the triangle inequality, no free constant);
  end to end (articulated, f16x3): per tensor, relative L2 distance to the fp32 CPU reference's
    gradient <= max(F16X3_FACTOR x the fp64 re-evaluation's, F16X3_FLOOR), the constants of
    tests/test_gpu_teacher_forced.py, unchanged.

Worst end-to-end ratio per kind on the first GPU run with these gates: see DESIGN.md section 2.
"""
import numpy as np
import pytest
import torch

from test_opacity_loss_golden import (KINDS, LAMBDA, ULP, case_inputs, cases, d_ref, d_ref_rgb,
                                      masked_mse, opacity_term, restate, restate_rgb)

pytestmark = pytest.mark.gpu

TOL = 4 * ULP


@pytest.fixture(scope="module")
def G(golden):
    return golden("opacity_loss.npz")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_RGB = {}


def _rgb_inputs(G, name):
    """pred0, pred1, target (B,3) fp32 numpy: the fixture's for the masked-colour cases, seeded
    uniforms otherwise."""
    if name not in _RGB:
        if f"{name}__target" in G:
            _RGB[name] = tuple(G[f"{name}__{k}"] for k in ("pred0", "pred1", "target"))
        else:
            B = len(G[f"{name}__mask"])
            rng = np.random.Generator(np.random.PCG64(77 + B))
            _RGB[name] = tuple(rng.random((B, 3), dtype=np.float32) for _ in range(3))
    return _RGB[name]


def _run(G, name, kind, mask_rgb=False, extra=None, lam=LAMBDA, rgb=True):
    """One aon_loss_masked launch -> (out (4,), grad_rgb0, grad_rgb1, grad_acc0, grad_acc1) as
    numpy (the absent ones None)."""
    from aonerf import _lib as L

    acc0, acc1, mask = (_cuda(x) for x in case_inputs(G, name))
    B = acc0.numel()
    p0 = p1 = tg = g0 = g1 = a0 = a1 = None
    if rgb:
        p0, p1, tg = (_cuda(x) for x in _rgb_inputs(G, name))
        g0, g1 = torch.full_like(p0, 7.0), torch.full_like(p1, 7.0)
    if kind is not None:
        a0, a1 = torch.full_like(acc0, 7.0), torch.full_like(acc1, 7.0)
    ex = torch.tensor(extra, device="cuda") if extra is not None else None
    out = torch.full((4,), 7.0, device="cuda")
    L.call("aon_loss_masked", L.ptr(p0), L.ptr(p1), L.ptr(acc0), L.ptr(acc1), L.ptr(tg),
           L.ptr(mask), B, L.ptr(ex), L.OPACITY[kind], lam, int(mask_rgb), L.ptr(out), L.ptr(g0),
           L.ptr(g1), L.ptr(a0), L.ptr(a1), L.stream(acc0.device))
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (out, g0, g1, a0, a1))


def _within(ours, ref64, slack=0.0):
    """|ours - ref64| <= slack + 4 ulps of ref64, elementwise; returns the worst error in ulps
    of ref64 beyond the slack."""
    ours, ref64 = np.asarray(ours, np.float64), np.asarray(ref64, np.float64)
    err = np.abs(ours - ref64) - slack
    ok = err <= TOL * np.abs(ref64)
    worst = float(np.max(np.where(ref64 != 0, err / np.maximum(np.abs(ref64), 1e-300) / ULP,
                                  np.where(err > 0, np.inf, 0.0)), initial=0.0))
    return bool(np.all(ok)), worst


@pytest.mark.parametrize("kind", (None,) + KINDS)
def test_kernel_vs_fp64_restatement(G, kind):
    names, rgb_names = cases(G)
    worst = 0.0
    for name in names:
        acc0, acc1, mask = case_inputs(G, name)
        p0, p1, tg = _rgb_inputs(G, name)
        for mask_rgb in ((False, True) if name in rgb_names else (False,)):
            extra = 0.03125 if name in ("b257", "b300_rgb") else None
            out, g0, g1, a0, a1 = _run(G, name, kind, mask_rgb, extra)
            l0, r0 = restate_rgb(p0, tg, mask, masked=mask_rgb)
            l1, r1 = restate_rgb(p1, tg, mask, masked=mask_rgb)
            op, o0, o1 = restate(kind, acc0, acc1, mask)
            print(f"{name} {kind} mask_rgb={mask_rgb}: out {out} fp64 {l0:.9g} {l1:.9g} {op:.9g}")
            if np.isnan(l0):  # masked colours, no foreground ray
                assert np.isnan(out[0]) and np.isnan(out[1]) and np.isnan(out[2])
                assert (g0 == 0).all() and (g1 == 0).all()
            else:
                checks = [(out[1], l0), (out[2], l1), (g0, r0), (g1, r1),
                          (out[0], l1 + l0 + (extra or 0.0) + op)]
                for ours, ref in checks:
                    ok, w = _within(ours, ref)
                    worst = max(worst, w)
                    assert ok, (name, kind, mask_rgb, w)
                # the total is the fp32 sum of the rounded terms, in k_loss_pair's order
                tot = np.float32(out[2]) + np.float32(out[1])
                if extra is not None:
                    tot = tot + np.float32(extra)
                if kind is not None:
                    tot = tot + np.float32(out[3])
                assert out[0] == tot
            ok, w = _within(out[3], op)
            worst = max(worst, w)
            assert ok, (name, kind, w)
            if kind is None:
                assert out[3] == 0 and a0 is None
                continue
            for ours, ref in ((a0, o0), (a1, o1)):
                ok, w = _within(ours, ref)
                worst = max(worst, w)
                assert ok, (name, kind, w)
                assert (ours[ref == 0] == 0).all()  # exact zeros stay exact
            fg = mask != 0
            if kind == "mse":  # the clamp stops the gradient outside [0, 1]
                for a, g in ((acc0, a0), (acc1, a1)):
                    assert (g[(a < 0) | (a > 1)] == 0).all()
            if kind == "autorf":
                assert (a1[fg] == 0).all()
            if mask_rgb:
                assert (g0[~fg] == 0).all() and (g1[~fg] == 0).all()
    print(f"kind {kind}: worst {worst:.2f} ulp of the 4 allowed")


def test_plain_mode_is_bit_equal_to_loss_pair(G):
    """mask_rgb = 0, kind = NONE: out[0:3] and both colour gradients are aon_loss_pair's bits."""
    from aonerf import _lib as L

    for name in cases(G)[0]:
        for extra in (None, 0.0123):
            out, g0, g1, _, _ = _run(G, name, None, False, extra)
            p0, p1, tg = (_cuda(x) for x in _rgb_inputs(G, name))
            ex = torch.tensor(extra, device="cuda") if extra is not None else None
            ref = torch.empty((3,), device="cuda")
            r0, r1 = torch.empty_like(p0), torch.empty_like(p1)
            L.call("aon_loss_pair", L.ptr(p0), L.ptr(p1), L.ptr(tg), p0.numel(), L.ptr(ex),
                   L.ptr(ref), L.ptr(r0), L.ptr(r1), L.stream(p0.device))
            assert np.array_equal(out[:3], ref.cpu().numpy()), name
            assert np.array_equal(g0, r0.cpu().numpy()) and np.array_equal(g1, r1.cpu().numpy())


@pytest.mark.parametrize("kind", KINDS)
def test_kernel_vs_reference_fixture(G, kind):
    """|ours - reference fp32| <= d_ref + 4 ulps, with the colour terms skipped (the reference's
    stand-alone opacity losses) -- losses and every gradient element."""
    for name in cases(G)[0]:
        out, _, _, a0, a1 = _run(G, name, kind, rgb=False)
        op, o0, o1 = restate(kind, *case_inputs(G, name))
        dl, d0, d1 = d_ref(G, name, kind)
        assert out[1] == 0 and out[2] == 0 and out[0] == out[3]
        for ours, ref, r64, d in ((out[3], G[f"{name}__{kind}_loss"], op, dl),
                                  (a0, G[f"{name}__{kind}_g0"], o0, d0),
                                  (a1, G[f"{name}__{kind}_g1"], o1, d1)):
            err = np.abs(np.asarray(ours, np.float64) - np.asarray(ref, np.float64))
            assert (err <= d + TOL * np.abs(r64)).all(), (name, kind, float(np.max(err)))


def test_masked_rgb_vs_reference_fixture(G):
    out, g0, g1, _, _ = _run(G, "b300_rgb", None, mask_rgb=True)
    mask = G["b300_rgb__mask"]
    for level, (loss, g) in enumerate(((out[1], g0), (out[2], g1))):
        l64, g64 = restate_rgb(G[f"b300_rgb__pred{level}"], G["b300_rgb__target"], mask)
        dl, dg = d_ref_rgb(G, "b300_rgb", level)
        assert abs(float(loss) - float(G[f"b300_rgb__rgb_loss{level}"])) <= dl + TOL * abs(l64)
        err = np.abs(g.astype(np.float64) - G[f"b300_rgb__rgb_g{level}"].astype(np.float64))
        assert (err <= dg + TOL * np.abs(g64)).all()
    # no foreground ray: the loss is NaN and the gradients are all zero, as the reference's
    for kind in (None, "mse"):
        out, g0, g1, a0, _ = _run(G, "b64_rgb_bg", kind, mask_rgb=True)
        assert np.isnan(G["b64_rgb_bg__rgb_loss0"]) and np.isnan(out[:3]).all()
        assert (g0 == 0).all() and (g1 == 0).all()
        assert (G["b64_rgb_bg__rgb_g0"] == 0).all() and (G["b64_rgb_bg__rgb_g1"] == 0).all()
        if kind:
            assert np.isfinite(out[3]) and np.isfinite(a0).all()


def test_loss_masked_bwd_every_scalar_combination():
    from aonerf import _lib as L

    B = 301
    rng = np.random.Generator(np.random.PCG64(5))
    grads = [_cuda(rng.standard_normal(s, dtype=np.float32)) for s in ((B, 3), (B, 3), (B,), (B,))]
    vals = (1.0, 0.37, -2.5, 0.611)  # g_loss, g_loss0, g_loss1, g_opacity
    for combo in range(16):
        present = [bool(combo >> k & 1) for k in range(4)]
        sc = [torch.tensor(v, device="cuda") if p else None for v, p in zip(vals, present)]
        outs = [torch.full_like(g, 7.0) for g in grads]
        L.call("aon_loss_masked_bwd", *(L.ptr(g) for g in grads), B, *(L.ptr(s) for s in sc),
               *(L.ptr(o) for o in outs), L.stream(grads[0].device))
        torch.cuda.synchronize()
        g = np.float32(vals[0]) if present[0] else np.float32(0)
        factors = [g + (np.float32(vals[k]) if present[k] else np.float32(0)) for k in (1, 2, 3, 3)]
        for grad, out, f in zip(grads, outs, factors):
            grad, out = grad.cpu().numpy(), out.cpu().numpy()
            if combo == 1:  # g_loss = 1 alone
                assert np.array_equal(out, grad)
            want = grad.astype(np.float64) * float(f)
            assert (np.abs(out - want) <= ULP * np.abs(want)).all(), (combo, f)
    # one pair of buffers absent: the other is scaled, nothing else is touched
    one = torch.tensor(2.0, device="cuda")
    outs = [torch.full_like(g, 7.0) for g in grads]
    L.call("aon_loss_masked_bwd", None, None, L.ptr(grads[2]), L.ptr(grads[3]), B, L.ptr(one), None,
           None, None, None, None, L.ptr(outs[2]), L.ptr(outs[3]), L.stream(one.device))
    L.call("aon_loss_masked_bwd", L.ptr(grads[0]), L.ptr(grads[1]), None, None, B, L.ptr(one), None,
           None, None, L.ptr(outs[0]), L.ptr(outs[1]), None, None, L.stream(one.device))
    for grad, out in zip(grads, outs):
        assert torch.equal(out, grad * 2.0)


def test_graph_replay_is_bit_equal(G):
    """The B = 257 CE case captured into a hip graph (one kernel node) and replayed: the same
    bits as the eager call -- nothing in the entry point reads the device from the host."""
    from aonerf import _lib as L

    eager = _run(G, "b257", "ce", extra=0.25)
    acc0, acc1, mask = (_cuda(x) for x in case_inputs(G, "b257"))
    p0, p1, tg = (_cuda(x) for x in _rgb_inputs(G, "b257"))
    ex = torch.tensor(0.25, device="cuda")
    bufs = [torch.empty((4,), device="cuda"), torch.empty_like(p0), torch.empty_like(p1),
            torch.empty_like(acc0), torch.empty_like(acc1)]

    def launch():
        L.call("aon_loss_masked", L.ptr(p0), L.ptr(p1), L.ptr(acc0), L.ptr(acc1), L.ptr(tg),
               L.ptr(mask), 257, L.ptr(ex), L.OPACITY["ce"], LAMBDA, 0, *(L.ptr(b) for b in bufs),
               L.stream(acc0.device))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for b in bufs:
        b.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for b, e in zip(bufs, eager):
        assert np.array_equal(b.cpu().numpy(), e)


# ------------------------------------------------------------------------------ end to end
CONFIGS = [("mse", False), ("ce", False), ("autorf", False), ("mse", True)]
_E2E = {}


def _mask_of(target):
    """The deterministic synthetic mask: target.mean(-1) < 0.99, or every third ray where that
    is degenerate (all or none)."""
    m = target.mean(-1) < 0.99
    if m.all() or not m.any():
        m = torch.arange(target.shape[0], device=target.device) % 3 == 0
    return m


def _reference_grads(cpu, mask, dtype):
    """The reference's gradients per config from ONE forward in ``dtype`` on the CPU:
    art_nerf_forward + latent_reg_loss (oracle), the mask terms in torch."""
    from oracle import nerf_oracle as O
    from oracle import trajectory as T

    leaves = {n: v.to(dtype).clone().requires_grad_(True)
              for n, v in T.initial_state("art")["theta"].items()}
    params = [{k[len(pre):]: v for k, v in leaves.items() if k.startswith(pre)}
              for pre in ("coarse_mlp.", "fine_mlp.")]
    tables = {k[len("code_library."):]: v for k, v in leaves.items() if k.startswith("code_library.")}
    rays = {k: cpu[k].to(dtype) for k in ("rays_o", "rays_d", "viewdirs")}
    target = cpu["target"].to(dtype)
    latents = O.code_library_latents(tables, int(cpu["instance_id"]), int(cpu["articulation_id"]))
    ret = O.art_nerf_forward(params, rays, False, True, 2.0, 6.0, latents)
    reg = O.latent_reg_loss(latents)
    m = mask.to(dtype)
    out = {}
    for kind, mask_rgb in [(None, False)] + CONFIGS:
        if mask_rgb:
            loss0, loss1 = masked_mse(ret[0][0], target, m), masked_mse(ret[1][0], target, m)
        else:
            loss0, loss1 = O.img2mse(ret[0][0], target), O.img2mse(ret[1][0], target)
        loss = loss1 + loss0
        loss = loss + reg
        if kind is not None:
            loss = loss + opacity_term(kind, ret[0][1], ret[1][1], m, LAMBDA)
        grads = torch.autograd.grad(loss, list(leaves.values()), retain_graph=True, allow_unused=True)
        out[(kind, mask_rgb)] = {n: (g if g is not None else torch.zeros_like(v)).detach().double()
                                 for (n, v), g in zip(leaves.items(), grads)}
    return out


def _e2e():
    if not _E2E:
        from test_gpu_teacher_forced import _gpu_batch

        cpu, gpu = _gpu_batch("art")
        mask = _mask_of(gpu["target"])
        gpu = dict(gpu, instance_mask=mask)
        _E2E.update(cpu=cpu, gpu=gpu, mask=mask.cpu(),
                    ref32=_reference_grads(cpu, mask.cpu(), torch.float32),
                    ref64=_reference_grads(cpu, mask.cpu(), torch.float64))
    return _E2E


def _gpu_grads(net, lib, batch, monkeypatch, **kw):
    """One training_step + backward -> (loss, logs, grads per name (float64 numpy), the acc the
    loss saw per level)."""
    from test_gpu_teacher_forced import _named

    from aonerf import train_art

    seen = {}
    real = train_art.masked_loss

    def spy(p0, p1, a0, a1, *a, **k):
        seen["acc"] = (a0.detach().clone(), a1.detach().clone())
        return real(p0, p1, a0, a1, *a, **k)

    monkeypatch.setattr(train_art, "masked_loss", spy)
    named = _named(net, lib)
    for p in named.values():
        p.grad = None
    loss, logs = train_art.training_step(net, lib, batch, False, True, 2.0, 6.0, **kw)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().double().cpu().numpy() for n, p in named.items()}
    return loss, logs, grads, seen.get("acc")


def _check_opacity_log(logs, acc, mask, kind, lam=LAMBDA):
    op64, _, _ = restate(kind, acc[0].cpu().numpy(), acc[1].cpu().numpy(), mask.numpy(), lam)
    ours = float(logs["opacity"].detach())
    ok, w = _within(ours, op64)
    assert ok, (kind, ours, op64, w)


def test_end_to_end_f16x3(monkeypatch):
    """One training_step + backward per kind on the teacher-forced articulated batch (128 rays,
    eval sampling, seed 0) against the fp32 CPU reference, gated as the teacher-forced f16x3
    gradients are."""
    from oracle import trajectory as T
    from test_gpu_teacher_forced import F16X3_FACTOR, F16X3_FLOOR, _model

    E = _e2e()
    net, lib, _ = _model("art", "f16x3")
    _, _, plain, _ = _gpu_grads(net, lib, E["gpu"], monkeypatch)
    for n, g in plain.items():  # the default path is the reference's unmasked step
        assert np.isfinite(g).all(), n
    bad = []
    for kind, mask_rgb in CONFIGS:
        loss, logs, grads, acc = _gpu_grads(net, lib, E["gpu"], monkeypatch, opacity=kind,
                                            opacity_lambda=LAMBDA, mask_rgb=mask_rgb)
        assert torch.isfinite(loss) and all(torch.isfinite(v).all() for v in logs.values())
        assert all(np.isfinite(g).all() for g in grads.values())
        _check_opacity_log(logs, acc, E["mask"], kind)
        ref32, ref64 = E["ref32"][(kind, mask_rgb)], E["ref64"][(kind, mask_rgb)]
        ours = T.compare(grads, ref32)
        self_ = T.compare({n: g.numpy() for n, g in ref64.items()}, ref32)
        worst = (0.0, None, 0.0)
        for n, (e, _cos) in ours.items():
            allow = max(F16X3_FACTOR * self_[n][0], F16X3_FLOOR)
            if e / allow > worst[0]:
                worst = (e / allow, n, e)
            if e > allow:
                bad.append((kind, mask_rgb, n, e, allow))
        print(f"f16x3 opacity={kind} mask_rgb={mask_rgb}: loss {float(loss.detach()):.6f} opacity "
              f"{float(logs['opacity'].detach()):.6f}; worst gradient {worst[1]} rel {worst[2]:.2e} "
              f"({worst[0]:.2f} of gate)")
        # g_acc reaches the compositor's backward at both levels
        for level in ("coarse_mlp.", "fine_mlp."):
            assert any(not np.array_equal(grads[n], plain[n]) for n in grads if n.startswith(level))
    assert not bad, bad[:10]


def test_end_to_end_bf16(monkeypatch):
    """bf16 mode on the same batch: the loss kernel is fp32 in either mode, so finiteness and the
    opacity log against the step's own acc -- fused and layer-by-layer kernels alike."""
    from test_gpu_art_train import _make

    E = _e2e()
    for numerics in (dict(precision="bf16"),
                     dict(precision="bf16", fused_forward=False, fused_backward=False)):
        net, lib = _make(0, **numerics)
        for kind in KINDS:
            loss, logs, grads, acc = _gpu_grads(net, lib, E["gpu"], monkeypatch, opacity=kind)
            assert torch.isfinite(loss) and all(torch.isfinite(v).all() for v in logs.values())
            assert all(np.isfinite(g).all() for g in grads.values())
            _check_opacity_log(logs, acc, E["mask"], kind)
            print(f"bf16 {numerics} opacity={kind}: loss {float(loss.detach()):.6f} opacity "
                  f"{float(logs['opacity'].detach()):.6f}")


def test_opacity_wrappers_match_training_step(monkeypatch):
    """train_art.opacity_loss / opacity_loss_CE / opacity_loss_autorf (the reference's names and
    arguments) give the step's opacity term, and their backward the kernel's acc gradients."""
    from aonerf import train_art

    rng = np.random.Generator(np.random.PCG64(9))
    acc = [_cuda(rng.random(300, dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).requires_grad_(True)
           for _ in range(2)]
    mask = _cuda(rng.random(300) < 0.4)
    ret = [(None, acc[0], None), (None, acc[1], None)]
    for kind, fn in zip(KINDS, (train_art.opacity_loss, train_art.opacity_loss_CE,
                                train_art.opacity_loss_autorf)):
        for a in acc:
            a.grad = None
        loss = fn(ret, mask.float())  # the reference passes instance_mask as it comes
        (loss * 1.0).backward()
        op, g0, g1 = restate(kind, acc[0].detach().cpu().numpy(), acc[1].detach().cpu().numpy(),
                             mask.cpu().numpy())
        assert loss.dim() == 0 and _within(float(loss.detach()), op)[0]
        assert _within(acc[0].grad.cpu().numpy(), g0)[0] and _within(acc[1].grad.cpu().numpy(), g1)[0]


def test_defaults_are_todays_loss_pair_path():
    """No new kwargs: loss and gradients bit-equal to the loss_pair composition, no `opacity`
    log; asking for a mask term without a mask raises."""
    from test_gpu_teacher_forced import _model, _named

    from aonerf import train_art

    E = _e2e()
    batch = {k: v for k, v in E["gpu"].items() if k != "instance_mask"}
    net, lib, _ = _model("art", "f16x3")
    named = _named(net, lib)

    def grads():
        out = {n: p.grad.detach().clone() for n, p in named.items()}
        for p in named.values():
            p.grad = None
        return out

    loss, logs = train_art.training_step(net, lib, batch, False, True, 2.0, 6.0)
    loss.backward()
    ours = grads()
    latents = lib(batch)
    ret = net(batch, False, True, 2.0, 6.0, latents)
    reg = train_art.LatentReg.apply(latents["density"], latents["color"], latents["articulation"])
    ref, *_ = train_art.loss_pair(ret[0][0], ret[1][0], batch["target"], reg)
    ref.backward()
    want = grads()
    assert torch.equal(loss, ref) and "opacity" not in logs
    for n in want:
        assert torch.equal(ours[n], want[n]), n
    with pytest.raises(ValueError, match="instance_mask"):
        train_art.training_step(net, lib, batch, False, True, 2.0, 6.0, opacity="ce")
    # the key SapienMultiImage.ray_batch uses
    loss, logs = train_art.training_step(net, lib, dict(batch, mask=E["gpu"]["instance_mask"]),
                                         False, True, 2.0, 6.0, opacity="ce")
    assert torch.isfinite(loss) and "opacity" in logs
