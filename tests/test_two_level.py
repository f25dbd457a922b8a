"""aonerf.two_level, the coarse/fine driver NeRF and NeRF_AE_Art share.  Host logic on CPU
tensors with stub spec callables and stubbed launches (as tests/test_level.py: no kernel runs):
the output tuples, fine_only, the per-level call and draw order, the range-fallback protocol.
On the GPU, for both models at B = 37 (no multiple of 16 or 64), 8 coarse + 16 fine samples:
the forced fallback against a direct render on the fallback path, and fused_march on / off."""
import contextlib
import warnings
from types import SimpleNamespace

import pytest
import torch

B, NC, NF = 37, 8, 16


# ---------------------------------------------------------------------------- stubs (CPU)
@pytest.fixture
def drv(monkeypatch):
    """two_level with every launch and draw replaced by a recorder -> (module, log, state)."""
    from aonerf import _lib as L
    from aonerf import two_level as T

    log, state = [], SimpleNamespace(overflow=False, rng=0)

    def level_t_vals(level, o, d, t_prev, w_prev, randomized, near, far, nc, nf, lindisp,
                     u_coarse=None, u_fine=None):
        log.append(("sample", level))
        if level == 1:
            assert w_prev is not None, "the two-kernel path resamples the coarse weights"
        return torch.zeros(o.shape[0], nc if level == 0 else t_prev.shape[1] + nf)

    def fine_uniforms(b, nf, randomized, dev, u_fine=None):
        log.append(("fine_u",))
        return torch.zeros(b, nf), nf

    def outputs(t_vals, keep):
        b, s = t_vals.shape
        return torch.zeros(b, 3), torch.zeros(b), torch.zeros(b), torch.ones(b, s) if keep else None

    def composite_march(raw, t_vals, d, white_bkgd, act, u, u_stride, nf, keep_weights):
        log.append(("march", act, bool(keep_weights)))
        return outputs(t_vals, keep_weights), torch.zeros(t_vals.shape[0], t_vals.shape[1] + nf)

    def composite_fwd(raw, t_vals, d, white_bkgd, act, keep_weights=True):
        log.append(("comp", act, bool(keep_weights)))
        return outputs(t_vals, keep_weights)

    for name, fn in (("level_t_vals", level_t_vals), ("fine_uniforms", fine_uniforms),
                     ("composite_march", composite_march), ("composite_fwd", composite_fwd)):
        monkeypatch.setattr(T, name, fn)
    rand_like, rand = torch.rand_like, torch.rand
    monkeypatch.setattr(torch, "rand_like", lambda x: (log.append(("noise",)), rand_like(x))[1])
    monkeypatch.setattr(torch, "rand", lambda *a, **k: (log.append(("noise",)), rand(*a, **k))[1])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(torch.cuda, "get_rng_state",
                        lambda dev=None: (log.append(("rng_save",)), "saved")[1])
    monkeypatch.setattr(torch.cuda, "set_rng_state", lambda s, dev=None: log.append(("rng_set", s)))
    monkeypatch.setattr(L, "range_overflow",
                        lambda packs: (log.append(("overflow?", packs)), state.overflow)[1])
    return T, log, state


def make_spec(log, *, noise_std=1.0, fused_march=True, keep_fine_weights=False, key="rgb_sigma",
              range_checked=False, mlp_raw=None):
    model = SimpleNamespace(num_coarse_samples=NC, num_fine_samples=NF, lindisp=False,
                            noise_std=noise_std, fused_march=fused_march, coarse_mlp="coarse",
                            fine_mlp="fine")

    def raw_of(level, mlp, o, d, v, t_vals, act):
        log.append(("mlp", level, mlp, act))
        return torch.zeros(t_vals.numel(), 4)

    def train_level(level, mlp, o, d, v, t_vals, white_bkgd, noise, timers):
        log.append(("train_level", level, mlp, noise is not None))
        b, s = t_vals.shape
        return torch.zeros(b, 3), torch.zeros(b), torch.zeros(b), torch.ones(b, s)

    @contextlib.contextmanager
    def fallback():
        log.append(("fallback_enter",))
        try:
            yield
        finally:
            log.append(("fallback_exit",))

    return SimpleNamespace(
        model=model, mlp_raw=mlp_raw or raw_of, train_level=train_level,
        acts=lambda noisy: ("mlp_raw_act", "comp_all_act") if noisy else ("mlp_all_act", "comp_no_act"),
        keep_fine_weights=keep_fine_weights, extras_key=key, range_checked=lambda: range_checked,
        packs=lambda: "packs", fallback=fallback, warning="MODEL: left the range")


def rays_cpu():
    return torch.zeros(B, 3), torch.ones(B, 3), torch.ones(B, 3)


# ---------------------------------------------------------------------------- output tuples
@pytest.mark.parametrize("key", ["rgb_sigma", "raw"])
@pytest.mark.parametrize("rw", [False, True])
@pytest.mark.parametrize("ri", [False, True])
def test_shape_output(rw, ri, key):
    from aonerf.two_level import shape_output

    comp, acc, depth, w = object(), object(), object(), object()
    extras = {"t_vals": 1, "weights": w, key: 2}
    out = shape_output(comp, acc, depth, w, extras, rw, ri)
    want = (comp, acc, depth) + ((w,) if rw else ()) + ((extras,) if ri else ())
    assert isinstance(out, tuple) and len(out) == len(want)
    assert all(a is b for a, b in zip(out, want))


@pytest.mark.parametrize("key", ["rgb_sigma", "raw"])
def test_render_extras_carry_the_models_key(drv, key):
    T, log, _ = drv
    ret = T.render(make_spec(log, key=key), *rays_cpu(), False, True, 2.0, 6.0,
                   return_intermediates=True)
    for lv, s in zip(ret, (NC, NC + NF)):
        assert len(lv) == 4 and set(lv[3]) == {"t_vals", "weights", key}
        assert lv[3][key].shape == (B * s, 4) and lv[3]["t_vals"].shape == (B, s)
        assert lv[3]["weights"].shape == (B, s)
    ret = T.train(make_spec(log, key=key), *rays_cpu(), False, True, 2.0, 6.0, return_weights=True,
                  return_intermediates=True)
    assert all(len(lv) == 5 and set(lv[4]) == {"t_vals", "weights"} and lv[3] is lv[4]["weights"]
               for lv in ret)


# ---------------------------------------------------------------------------- fine_only
def test_fine_only_drops_the_coarse_entry(drv):
    T, log, _ = drv
    ret = T.render(make_spec(log), *rays_cpu(), False, True, 2.0, 6.0, fine_only=True)
    assert ret[0] is None and len(ret[1]) == 3
    for kw in (dict(return_weights=True), dict(return_intermediates=True)):
        ret = T.render(make_spec(log), *rays_cpu(), False, True, 2.0, 6.0, fine_only=True, **kw)
        assert ret[0] is not None and len(ret[0]) == len(ret[1]) == 4


def test_fine_only_is_ignored_when_training(monkeypatch):
    """NeRF.forward under autograd takes two_level.train, which has no fine_only, and builds no
    view encodings; without autograd fine_only reaches two_level.render (resolved: off when
    extras are asked for)."""
    from aonerf import _lib as L
    from aonerf import helper, model, two_level

    calls = []
    monkeypatch.setattr(L, "require_gpu", lambda *t: None)
    monkeypatch.setattr(helper, "pos_enc", lambda v, lo, hi: calls.append("pos_enc") or "cond")
    monkeypatch.setattr(two_level, "train", lambda spec, *a, **kw: calls.append(("train", kw)))
    monkeypatch.setattr(two_level, "render", lambda spec, *a, **kw: calls.append(("render", kw)))
    net = model.NeRF(num_coarse_samples=NC, num_fine_samples=NF)
    o, d, v = rays_cpu()
    rays = {"rays_o": o, "rays_d": d, "viewdirs": v}
    net(rays, False, True, 2.0, 6.0, fine_only=True)
    assert calls[0][0] == "train" and "fine_only" not in calls[0][1]
    del calls[:]
    with torch.no_grad():
        net(rays, False, True, 2.0, 6.0, fine_only=True)
        assert calls == ["pos_enc", ("render", calls[1][1])] and calls[1][1]["fine_only"] is True
        del calls[:]
        net(rays, False, True, 2.0, 6.0, fine_only=True, return_weights=True)
        assert [c[0] for c in calls] == ["render"] and calls[0][1]["fine_only"] is False
        del calls[:]
        net.coarse_mlp.precision = "fp32"  # no density-only / cond kernels in fp32
        net(rays, False, True, 2.0, 6.0, fine_only=True)
        assert [c[0] for c in calls] == ["render"] and calls[0][1]["fine_only"] is True


# ---------------------------------------------------------------------------- order
def test_render_order_fused_march(drv):
    """Per level: sampling, MLP, density noise, [fine u,] compositor -- the level's noise is
    drawn before the fine level's u; the march hands its t over (no level-1 sampling)."""
    T, log, _ = drv
    T.render(make_spec(log), *rays_cpu(), True, True, 2.0, 6.0)
    assert log == [("rng_save",), ("sample", 0), ("mlp", 0, "coarse", "mlp_raw_act"), ("noise",),
                   ("fine_u",), ("march", "comp_all_act", False),
                   ("mlp", 1, "fine", "mlp_raw_act"), ("noise",), ("comp", "comp_all_act", False)]


def test_render_order_two_kernels(drv):
    T, log, _ = drv
    T.render(make_spec(log, fused_march=False), *rays_cpu(), True, True, 2.0, 6.0)
    assert log == [("rng_save",), ("sample", 0), ("mlp", 0, "coarse", "mlp_raw_act"), ("noise",),
                   ("comp", "comp_all_act", True), ("sample", 1),
                   ("mlp", 1, "fine", "mlp_raw_act"), ("noise",), ("comp", "comp_all_act", False)]


@pytest.mark.parametrize("randomized,noise_std", [(False, 1.0), (True, 0.0), (False, 0.0)])
def test_no_noise_no_draw(drv, randomized, noise_std):
    T, log, _ = drv
    T.render(make_spec(log, noise_std=noise_std), *rays_cpu(), randomized, True, 2.0, 6.0)
    assert ("noise",) not in log and (("rng_save",) in log) == randomized
    assert [e for e in log if e[0] in ("mlp", "march", "comp")] == [
        ("mlp", 0, "coarse", "mlp_all_act"), ("march", "comp_no_act", False),
        ("mlp", 1, "fine", "mlp_all_act"), ("comp", "comp_no_act", False)]


@pytest.mark.parametrize("fused_march", [True, False])
@pytest.mark.parametrize("keep_fine", [False, True])
@pytest.mark.parametrize("rw,ri", [(False, False), (True, False), (False, True)])
def test_keep_weights_rule(drv, fused_march, keep_fine, rw, ri):
    """The march keeps the coarse weights on chip unless asked for; the two-kernel coarse level
    always writes them (the resampler reads them); the fine level's are written when asked for
    or when the model always keeps them."""
    T, log, _ = drv
    T.render(make_spec(log, fused_march=fused_march, keep_fine_weights=keep_fine), *rays_cpu(),
             False, True, 2.0, 6.0, return_weights=rw, return_intermediates=ri)
    kept = [e[2] for e in log if e[0] in ("march", "comp")]
    assert kept == [(rw or ri) if fused_march else True, rw or ri or keep_fine]


def test_train_order(drv):
    T, log, _ = drv
    ret = T.train(make_spec(log), *rays_cpu(), True, True, 2.0, 6.0)
    assert log == [("sample", 0), ("noise",), ("train_level", 0, "coarse", True),
                   ("sample", 1), ("noise",), ("train_level", 1, "fine", True)]
    assert [len(lv) for lv in ret] == [3, 3]
    del log[:]
    T.train(make_spec(log), *rays_cpu(), False, True, 2.0, 6.0)
    assert log == [("sample", 0), ("train_level", 0, "coarse", False),
                   ("sample", 1), ("train_level", 1, "fine", False)]


# ---------------------------------------------------------------------------- range fallback
def test_no_overflow_check_without_range_check(drv):
    T, log, state = drv
    state.overflow = True
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        T.render(make_spec(log, range_checked=False), *rays_cpu(), True, True, 2.0, 6.0)
    assert not [e for e in log if e[0] in ("overflow?", "fallback_enter", "rng_set")]


def test_no_fallback_without_overflow(drv):
    T, log, _ = drv
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        T.render(make_spec(log, range_checked=True), *rays_cpu(), True, True, 2.0, 6.0)
    assert log[-1] == ("overflow?", "packs") and ("fallback_enter",) not in log


def test_fallback_entered_once_with_the_saved_rng(drv):
    T, log, state = drv
    state.overflow = True
    with pytest.warns(RuntimeWarning, match="MODEL: left the range") as w:
        ret = T.render(make_spec(log, range_checked=True), *rays_cpu(), True, True, 2.0, 6.0)
    assert len(w) == 1 and len(ret) == 2
    one_pass = [("sample", 0), ("mlp", 0, "coarse", "mlp_raw_act"), ("noise",), ("fine_u",),
                ("march", "comp_all_act", False), ("mlp", 1, "fine", "mlp_raw_act"), ("noise",),
                ("comp", "comp_all_act", False)]
    assert log == ([("rng_save",)] + one_pass + [("overflow?", "packs"), ("rng_set", "saved"),
                                                 ("fallback_enter",)] + one_pass
                   + [("fallback_exit",)])  # one check: the fallback's outputs are not re-checked


def test_fallback_left_when_the_second_render_raises(drv):
    T, log, state = drv
    state.overflow = True
    n = []

    def mlp_raw(level, mlp, o, d, v, t_vals, act):
        n.append(level)
        if len(n) > 2:
            raise RuntimeError("second pass")
        return torch.zeros(t_vals.numel(), 4)

    spec = make_spec(log, range_checked=True, mlp_raw=mlp_raw)
    with pytest.warns(RuntimeWarning), pytest.raises(RuntimeError, match="second pass"):
        T.render(spec, *rays_cpu(), False, True, 2.0, 6.0)
    assert log.count(("fallback_enter",)) == 1 and log[-1] == ("fallback_exit",)
    assert not [e for e in log if e[0].startswith("rng")]  # not randomized: nothing to replay


def test_switched_restores_each_value():
    from aonerf.two_level import switched

    a, b = SimpleNamespace(fused=True), SimpleNamespace(fused="other")
    with pytest.raises(KeyError):
        with switched((a, b), "fused", False):
            assert a.fused is False and b.fused is False
            raise KeyError
    assert a.fused is True and b.fused == "other"


def test_helpers_stay_importable_from_model():
    from aonerf import model, two_level

    for name in ("fine_uniforms", "composite_march", "march_ok", "level_t_vals"):
        assert getattr(model, name) is getattr(two_level, name)


# ---------------------------------------------------------------------------- GPU
def _rays():
    g = torch.Generator().manual_seed(5 + B)
    o = torch.rand(B, 3, generator=g) - 0.5
    o[:, 2] += 4.0
    d = torch.randn(B, 3, generator=g) * 0.2 - torch.tensor([0.0, 0.0, 1.0])
    d = torch.nn.functional.normalize(d, dim=-1)
    return {"rays_o": o.cuda(), "rays_d": d.cuda(), "viewdirs": d.clone().cuda()}


def _model(kind, **kw):
    """(net with the oracle's seed weights, extra forward arguments) at 8 + 16 samples."""
    from oracle import weights as W

    if kind == "vanilla":
        from aonerf.model import NeRF as Net
        sd, extra = W.nerf_state_dict(0), ()
    else:
        from aonerf.model_autodecoder import NeRF_AE_Art as Net
        sd = W.art_state_dict(0)
        extra = ({k: torch.from_numpy(v).cuda() for k, v in W.art_latents(1).items()},)
    net = Net(num_coarse_samples=NC, num_fine_samples=NF, noise_std=1.0, **kw).cuda()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.requires_grad_(False), extra


def _render(net, extra, seed=77):
    torch.cuda.manual_seed(seed)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            ret = net(_rays(), True, True, 2.0, 6.0, *extra, return_weights=True,
                      return_intermediates=True)
    torch.cuda.synchronize()
    return ret, torch.cuda.get_rng_state("cuda"), [x for x in w if "fp16x3 range" in str(x.message)]


def _assert_same_bits(a, b):
    for lv in range(2):
        for j in range(4):
            assert torch.isfinite(a[lv][j]).all() and torch.equal(a[lv][j], b[lv][j]), (lv, j)
        assert a[lv][4].keys() == b[lv][4].keys()
        for k in a[lv][4]:
            assert torch.equal(a[lv][4][k], b[lv][4][k]), (lv, k)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["vanilla", "art"])
def test_forced_fallback_equals_direct_render_on_the_fallback_path(kind):
    """A hidden unit at 12000 in both levels (outside the fp16x3 range, 8188: the kernels set
    the pack's status word), randomized, noise_std 1: the render warns once, returns the bits of
    a render made directly on the fallback path (fp32 / layer by layer) from the same seed, and
    leaves the generator where that single render leaves it; the model's switch is put back."""
    from aonerf.two_level import switched

    net, extra = _model(kind)
    mlps = (net.coarse_mlp, net.fine_mlp)
    with torch.no_grad():
        for m in mlps:
            m.pts_linears[3].bias[0] = 12000.0
    attr, exact = ("precision", "fp32") if kind == "vanilla" else ("fused", False)
    before = [getattr(m, attr) for m in mlps]
    a, rng_a, warns = _render(net, extra)
    assert len(warns) == 1 and [getattr(m, attr) for m in mlps] == before
    with switched(mlps, attr, exact):
        b, rng_b, warns = _render(net, extra)
    assert not warns
    _assert_same_bits(a, b)
    assert torch.equal(rng_a, rng_b)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["vanilla", "art"])
def test_fused_march_on_and_off_give_the_same_bits(kind):
    """aon_composite_march against aon_composite_fwd + aon_sample_pdf under the same driver,
    randomized with density noise: the same draws in the same order, the same bits out."""
    out = []
    for fm in (True, False):
        net, extra = _model(kind, fused_march=fm)
        ret, rng, warns = _render(net, extra)
        assert not warns
        out.append((ret, rng))
    _assert_same_bits(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
