"""The coarse/fine loop above a level (level.py is what happens inside one), once for NeRF and
NeRF_AE_Art: the sampling hand-over (the fused march's t_next, else level_t_vals), the density
noise and its place in the RNG order (after the level's MLP, before the fine level's u), the
march-or-composite choice with its timers, the output tuples and the fp16x3 range fallback.
Each model describes itself per forward with a ``spec``, a plain object of what differs:

    model              the sample counts, lindisp, noise_std, fused_march and the two MLPs
    mlp_raw(level, mlp, o, d, v, t_vals, act) -> raw (B*S, 4)
    acts(noisy)        -> (activation code of the MLP epilogue, of the compositor)
    keep_fine_weights  the fine compositor writes its weights even when nobody asked for them
    extras_key         the name of raw in the return_intermediates dict
    train_level(level, mlp, o, d, v, t_vals, white_bkgd, noise, timers) -> comp, acc, depth, w
    range_checked(), packs(), fallback(), warning   the range guard: whether to look, the packs
        with the status words, a context manager onto the model's exact path, the warning's text
    maps(mlp, o, d, t_vals, weights, timers) -> dict   (render(maps=True) only) per-ray maps of
        the fine level from its samples and weights, appended to the fine level's tuple

Both models launch what they launched before they shared this: same entry points, arguments,
order, allocations and random draws."""
import contextlib
import warnings

import torch

from . import _lib as L
from . import helper
from .level import composite_fwd, events, record


def fine_uniforms(B, num_fine_samples, randomized, dev, u_fine=None):
    """The u of the fine level's inverse-CDF sampling (helper.py:227-231) and its row stride:
    per-ray draws in randomized mode (or the injected ``u_fine``), else one shared linspace."""
    if randomized:
        u = torch.rand((B, num_fine_samples), device=dev) if u_fine is None else L.contig(u_fine)
        return u, num_fine_samples
    return helper.eval_u(num_fine_samples, dev), 0


def composite_march(raw, t_vals, d, white_bkgd, act, u, u_stride, num_fine_samples,
                    keep_weights):
    """Coarse compositing + the fine level's resampling in one kernel (aon_composite_march):
    (comp, acc, depth, weights or None), t_fine (B, S + Nf) -- helper.py:157-252 and
    model.py:163-172, the coarse weights kept on chip unless asked for."""
    B, S = t_vals.shape
    dev = t_vals.device
    comp = torch.empty((B, 3), device=dev)
    acc = torch.empty((B,), device=dev)
    depth = torch.empty((B,), device=dev)
    weights = torch.empty((B, S), device=dev) if keep_weights else None
    t_fine = torch.empty((B, S + num_fine_samples), device=dev)
    L.call("aon_composite_march", L.ptr(raw), L.ptr(t_vals), L.ptr(d), B, S, int(bool(white_bkgd)),
           act, L.ptr(u), u_stride, num_fine_samples, L.ptr(comp), L.ptr(acc), L.ptr(weights),
           L.ptr(depth), L.ptr(t_fine), L.stream(dev))
    return (comp, acc, depth, weights), t_fine


def march_ok(S, num_fine_samples, fused=True):
    """The fused march kernel's limits (include/aonerf.h: 3 <= S <= 256, 1 <= Ns <= 256); larger
    N_importance (up to aon_sample_pdf's 512) takes the two-kernel path, as does a model whose
    ``fused_march`` is False (aon_composite_fwd + aon_sample_pdf, bit-identical outputs)."""
    return fused and 3 <= S <= 256 and 1 <= num_fine_samples <= 256


def level_t_vals(level, o, d, t_prev, w_prev, randomized, near, far, num_coarse_samples,
                 num_fine_samples, lindisp, u_coarse=None, u_fine=None):
    """Sample positions of a level: stratified (helper.py:106-133) or inverse-CDF resampling
    of the previous level's weights merged with its samples (model.py:163-172)."""
    dev = o.device
    B = o.shape[0]
    if level == 0:
        t_vals, _ = helper.sample_along_rays(o, d, num_coarse_samples, near, far, randomized,
                                             lindisp, u=u_coarse, want_coords=False)
        return t_vals
    Sc = t_prev.shape[1]
    u, u_stride = fine_uniforms(B, num_fine_samples, randomized, dev, u_fine)
    w_prev = L.contig(w_prev.detach())
    t_new = torch.empty((B, Sc + num_fine_samples), device=dev)
    # bins = mids of t (model.py:163), weights[..., 1:-1] as a strided view
    L.call("aon_sample_pdf", None, 0, L.ptr(w_prev[:, 1:]), Sc, B, Sc - 1, num_fine_samples,
           L.ptr(u), u_stride, L.ptr(t_prev), Sc, None, None, L.ptr(t_new), None, L.stream(dev))
    return t_new


def shape_output(comp, acc, depth, weights, extras, return_weights, return_intermediates):
    """A level's tuple: (comp, acc, depth[, weights][, extras])."""
    out = (comp, acc, depth, weights) if return_weights else (comp, acc, depth)
    return out + (extras,) if return_intermediates else out


@contextlib.contextmanager
def switched(mlps, attr, value):
    """``attr`` of both MLPs set to ``value`` inside the block (a spec's fallback)."""
    old = [getattr(m, attr) for m in mlps]
    for m in mlps:
        setattr(m, attr, value)
    try:
        yield
    finally:
        for m, x in zip(mlps, old):
            setattr(m, attr, x)


def train(spec, o, d, v, randomized, white_bkgd, near, far, *, u_coarse=None, u_fine=None,
          return_weights=False, return_intermediates=False, timers=None):
    """Both levels under autograd (spec.train_level); no gradient reaches the sampling
    (helper.py:246-252)."""
    m = spec.model
    ret = []
    t_vals = weights = None
    for level, mlp in enumerate((m.coarse_mlp, m.fine_mlp)):
        with torch.no_grad():
            t_vals = level_t_vals(level, o, d, t_vals, weights, randomized, near, far,
                                  m.num_coarse_samples, m.num_fine_samples, m.lindisp, u_coarse,
                                  u_fine)
        noise = None
        if m.noise_std > 0 and randomized:  # model.py:183-184, model_autodecoder.py:318-319
            noise = torch.rand((t_vals.numel(),), device=o.device) * m.noise_std
        comp, acc, depth, weights = spec.train_level(level, mlp, o, d, v, t_vals, white_bkgd,
                                                     noise, timers)
        ret.append(shape_output(comp, acc, depth, weights, dict(t_vals=t_vals, weights=weights),
                                return_weights, return_intermediates))
    return ret


def _render_pass(spec, o, d, v, randomized, white_bkgd, near, far, u_coarse, u_fine,
                 return_weights, return_intermediates, timers, fine_only, maps=False):
    m = spec.model
    B, dev = o.shape[0], o.device
    want_w = return_weights or return_intermediates
    noisy = m.noise_std > 0 and randomized
    act_mlp, act_comp = spec.acts(noisy)
    ret = []
    t_vals = weights = t_next = None
    for level, mlp in enumerate((m.coarse_mlp, m.fine_mlp)):
        t_vals = t_next if t_next is not None else level_t_vals(
            level, o, d, t_vals, weights, randomized, near, far, m.num_coarse_samples,
            m.num_fine_samples, m.lindisp, u_coarse, u_fine)
        S = t_vals.shape[1]
        ev = events(timers)
        raw = spec.mlp_raw(level, mlp, o, d, v, t_vals, act_mlp)
        record(timers, ev, f"mlp{level}", B * S)
        if noisy:  # model.py:183-184, model_autodecoder.py:318-319
            raw[:, 3] += torch.rand_like(raw[:, 3]) * m.noise_std
        ev = events(timers)
        if level == 0 and march_ok(S, m.num_fine_samples, m.fused_march):
            # + the fine level's resampling, its u drawn after the level's density noise (the
            # reference's RNG order); the coarse weights reach HBM only when asked for
            u, u_stride = fine_uniforms(B, m.num_fine_samples, randomized, dev, u_fine)
            (comp, acc, depth, weights), t_next = composite_march(
                raw, t_vals, d, white_bkgd, act_comp, u, u_stride, m.num_fine_samples, want_w)
            record(timers, ev, f"march{level}", B * S)
        else:
            # the coarse weights feed level_t_vals; the fine level's are an output
            comp, acc, depth, weights = composite_fwd(
                raw, t_vals, d, white_bkgd, act_comp, want_w or level == 0 or spec.keep_fine_weights)
            record(timers, ev, f"comp{level}", B * S)
        extras = {"t_vals": t_vals, "weights": weights, spec.extras_key: raw}
        ret.append(None if fine_only and level == 0 else shape_output(
            comp, acc, depth, weights, extras, return_weights, return_intermediates))
        if maps and level == 1:
            ret[1] = ret[1] + (spec.maps(mlp, o, d, t_vals, weights, timers),)
    return ret


@torch.no_grad()
def render(spec, o, d, v, randomized, white_bkgd, near, far, *, u_coarse=None, u_fine=None,
           return_weights=False, return_intermediates=False, timers=None, fine_only=False,
           maps=False):
    """Both levels on the inference kernels.  ``maps``: the fine level's tuple ends with
    spec.maps' dict (inside the range fallback too, so on the exact path when it is taken).  ``fine_only`` (ignored when weights or
    intermediates are asked for): the coarse entry is None.  If the range guard reports an
    activation outside the fp16x3 range (one sync per forward, skipped under HIP-graph capture)
    the outputs are invalid: render again inside spec.fallback(), with the same random draws,
    which leaves the generator where one forward leaves it."""
    fine_only = bool(fine_only) and not (return_weights or return_intermediates)
    args = (spec, o, d, v, randomized, white_bkgd, near, far, u_coarse, u_fine, return_weights,
            return_intermediates, timers, fine_only, bool(maps))
    rng = torch.cuda.get_rng_state(o.device) if randomized else None
    ret = _render_pass(*args)
    if (spec.range_checked() and not torch.cuda.is_current_stream_capturing()
            and L.range_overflow(spec.packs())):
        warnings.warn(spec.warning, RuntimeWarning)
        if rng is not None:
            torch.cuda.set_rng_state(rng, o.device)
        with spec.fallback():
            ret = _render_pass(*args)
    return ret
