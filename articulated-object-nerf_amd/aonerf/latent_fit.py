"""Fitting latent codes to a trained NeRF_AE_Art with the MLPs frozen: the auto-decoder's
test-time use (the reference's --is_optimize, utils.get_optimizer_latent_opt: only the shape,
appearance and articulation codes are optimised against a few views of a new object or joint
state).

    model = freeze(model)                        # the MLPs take no gradient
    codes = LatentCodes(init=code_library(batch)).cuda()   # or a random start
    opt = configure_optimizer(codes, lr=1e-2)
    loss, logs = fit_step(model, codes, batch, False, True, near, far)
    loss.backward(); opt.step()                  # or fit(model, codes, batches, lr, ...)

fit_step calls the model with ``latent_only=True`` (train_art.render_level): each level runs the
training forward and the fused backward chain as a training step does, then ONE
aon_art_latent_grad launch instead of the level's 40 weight and bias gradients -- the code
gradients are (sum_rows dZ)^T W[:, latent columns] of four layers, which reads four of the
chain's sixteen gradient tensors and no activation.  The loss is training_step's own."""
import torch
import torch.nn as nn

from . import train, train_art

KEYS = ("density", "color", "articulation")  # CodeLibraryArticulated.forward's keys


class LatentCodes(nn.Module):
    """The three codes being fitted, (1, C) parameters named as the code library's dict:
    density = shape (n_shape), color = appearance (n_app), articulation (n_art).  Calling it
    returns that dict.  ``init``: such a dict to start from -- CodeLibraryArticulated's forward,
    or e.g. {..., "articulation": get_interpolated_articulations()[k]} (copied; any shape with
    C elements) -- else xavier_uniform_, the library's own init."""

    def __init__(self, n_shape=128, n_app=128, n_art=32, init=None):
        super().__init__()
        for key, n in zip(KEYS, (n_shape, n_app, n_art)):
            if init is None:
                code = nn.init.xavier_uniform_(torch.empty(1, n))
            else:
                code = init[key].detach().to(torch.float32).reshape(1, -1).clone()
                if code.shape[1] != n:
                    raise ValueError(f"LatentCodes: init[{key!r}] has {code.shape[1]} values, "
                                     f"expected {n}")
            setattr(self, key, nn.Parameter(code))

    def forward(self):
        return {key: getattr(self, key) for key in KEYS}


def freeze(model):
    """requires_grad_(False) on every MLP parameter of ``model``; returns the model."""
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def configure_optimizer(codes, lr):
    """Adam over the codes (train.Adam: the fused aon_adam_step, betas (0.9, 0.999)).  The
    reference's get_optimizer_latent_opt uses AdamW; the fused Adam has no decay term, so this
    is AdamW with weight_decay = 0 (the codes' only shrinkage is the loss's own regulariser)."""
    return train.Adam(codes.parameters(), lr=lr)


def fit_step(model, codes, batch, randomized, white_bkgd, near, far, *, opacity=None,
             opacity_lambda=0.05, mask_rgb=False, u_coarse=None, u_fine=None, timers=None):
    """One step of the fit -> (loss, logs): train_art.training_step with ``codes`` (a
    LatentCodes) in the code library's place and the model called with latent_only=True, so
    loss.backward() leaves gradients on the three codes only.  The MLPs must be frozen
    (freeze(model); ValueError otherwise).  Same loss assembly, keywords and logs as
    training_step; ``timers`` also receives ``art_dlatent{S}`` per level."""
    return train_art.step_on_latents(model, codes, batch, randomized, white_bkgd, near, far,
                                     u_coarse=u_coarse, u_fine=u_fine, timers=timers,
                                     opacity=opacity, opacity_lambda=opacity_lambda,
                                     mask_rgb=mask_rgb, latent_only=True)


def fit(model, codes, batches, lr, randomized, white_bkgd, near, far, *, opt=None, **step_kw):
    """The plain loop over ``batches`` (an iterable of ray batches): fit_step, backward,
    opt.step -> the list of per-step losses (device scalars, no host read).  ``opt``: an
    optimizer to continue with (default configure_optimizer(codes, lr)); ``step_kw``: fit_step's
    keywords.  The codes' optimizer packs no MLP weight, so the fp16x3 range guard of the frozen
    MLPs' kernels is checked here before each step (train.check_range: FloatingPointError, the
    step not applied)."""
    opt = configure_optimizer(codes, lr) if opt is None else opt
    mlp_params = list(model.parameters())
    devices = {str(p.device) for p in mlp_params}
    losses = []
    for batch in batches:
        opt.zero_grad()
        loss, _ = fit_step(model, codes, batch, randomized, white_bkgd, near, far, **step_kw)
        loss.backward()
        train.check_range(devices, mlp_params)
        opt.step()
        losses.append(loss.detach())
    return losses
