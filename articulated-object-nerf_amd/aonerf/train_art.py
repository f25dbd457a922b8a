"""Training step of the articulated auto-decoder (reference LitNeRF_AutoDecoder.training_step,
models/vanilla_nerf/model_autodecoder.py:395-477; configure_optimizers / optimizer_step :599-633)
on the HIP kernels.

One NeRF_AE_Art level under autograd is ``ArtRenderLevel`` (a torch.autograd.Function) with
gradients for the level's 40 MLP parameters AND the three latent codes:

  forward   one fused kernel per level (aon_mlp_art_fwd_train, the inference kernel with
            activation stores): cast_rays -> deformation MLP on cat[xyz, shape, articulation] ->
            x' = delta + xyz, pos_enc(x') -> trunk on cat[pos_enc(x'), shape] with the skip
            concat -> density, bottleneck -> view branch on cat[bottleneck, enc_dir tiled over
            samples, appearance] -> rgb, every activation, pos_enc(x') and the points kept
            (model_autodecoder.py:168-239); or the same layer by layer on aon_gemm
            (TrainNumerics.fused_forward False) -> compositing with the padded sigmoid / softplus
            (aon_composite_fwd, AON_ACT_ARTIC; :321-333)
  backward  aon_composite_bwd -> every input gradient dX = (dZ W) * relu'(X) in one fused
            kernel (aon_mlp_art_bwd): view branch, heads, trunk, the gradient w.r.t.
            pos_enc(x') (skip + first layer) through pos_enc's backward into the deformation
            head and MLP -> per layer dW = dZ^T X with db = sum_rows dZ from the same pass
            (aon_gemm); or the whole chain as GEMMs + aon_pos_enc_bwd (fused_backward False).
            latent_only (the MLPs frozen, latent_fit.py): the chain, then the three code
            gradients from four of its tensors in one call (aon_art_latent_grad), no dW.

The latent codes are the same row for every sample (repeated over B*S rows,
model_autodecoder.py:186-194), so their columns are folded into per-call biases in the
forward, and in the backward a layer z = W [x; l] + b gives dL/dl = W_l^T db and
dL/dW_l = db l^T from the bias gradient db alone (aon_gemm with K = 1 / M = 1); the shape code
collects three such terms (deformation input, trunk input, skip), appearance one, articulation
one, both levels add through autograd.  The regulariser 1e-4 * sum of mean code norms
(:456-466) is aon_latent_reg.  All arithmetic is in HIP kernels; torch allocates, routes
autograd and looks up / scatters the code-library rows (nn.Embedding).  The plumbing shared
with train.py, the latent folds and the layer-by-layer walker (also the render's fallback,
model_autodecoder.NeRFMLP._mlp) are level.py.
"""
import functools

import torch

from . import _lib as L
from . import level, tiles
from .level import BOT, DEF0, DENS, DL, PTS0, RGB, VIEW0, art_layers  # noqa: F401 (layer order)
from .level import Geo as _Geo
from .linalg import batched, gemm, small_batched
from .numerics import ART_FORWARD, DEFAULT
from .train import (Adam, _amax_word, img2mse, learning_rate, loss_pair, masked_loss,  # noqa: F401 (shared)
                    mse2psnr, relu_masks)


def _forward_level(geo, P, lat, xyz, venc, S, raw, noise=None, exact_folds=False):
    """NeRFMLP.forward layer by layer (level.art_forward), keeping activations; each latent fold
    runs just before its layer (exact_folds: exact fp32, as the bf16 mode computes them)."""
    bufs = level.LayerBuffers(geo, xyz.shape[0], xyz.device, raw)
    enc, _ = level.art_forward(
        geo, P, lambda i: level.fold(*P[i], *level.fold_args(geo, lat, i), exact_folds), xyz, venc,
        S, bufs, noise)
    return bufs.t["hd"], enc, bufs.t["h"], bufs.t["bot"][0], bufs.t["hv"]


# Which kernels, precision and (bf16 mode) forward numerics a level trains with is the MODEL's
# TrainNumerics (aonerf/numerics.py; NeRF_AE_Art(train_precision=...)), passed into
# ArtRenderLevel per call -- no module-level switch.  The bf16 mode: the whole backward chain and
# the weight-gradient GEMMs bf16 (aon_mlp_art_bwd_bf16, aon_gemm mma_bf16), kept activations and
# gradients bf16 (aon_mlp_art_fwd_train_bf16); compositing, the loss, their backward, the latent
# terms and Adam fp32 on fp32 master weights (tests/test_gpu_art_train_bf16.py).  Its forward
# past the deformation MLP (TrainNumerics.art_forward): "f16_acts" (default) two fp16 MFMAs per
# product, the weights' exact hi / lo split kept, the activations rounded once to fp16 per sample
# (the backward already reads bf16 copies, 8x coarser; C5 gradients cosine 0.99919 / max-rel
# 0.049 against the fp32 oracle at the 0.999 / 0.05 gates); "f16x3" fp16x3 throughout, only the
# stores bf16; held off by their measured gates: "f16_weights" (weights rounded to fp16: 0.99886
# / 0.074), "bf16_view" (view branch bf16: deformation gradients cosine 0.9968 for 2% of the
# step) and "bf16_trunk" (trunk, heads and view branch bf16: 0.987 -- the articulated gradients
# are ill-conditioned in the forward values).

def _params_struct(P, fb=None):
    """AonMlpArtParams of one level's parameters (``fb``: folded biases by layer index), checked
    against the layer table (ValueError) before any pointer reaches a pack kernel."""
    return L.mlp_art_params(level.folded_pairs(P, fb or {}))


def _pack(geo, P, lat, tag="", mixed=0, exact_folds=False):
    """The fused kernel's fp16x3 weight stream (aon_mlp_art_pack) of one level's parameters with
    this call's latent codes folded into the biases; re-packed on every call (the optimizer
    updates the parameters in place).  mixed: the bf16 mode's mixed streams
    (aon_mlp_art_pack_mixed: 1 trunk bf16, 2 view branch bf16, 3 fp16 weights; range-guarded,
    their deformation part is fp16x3).  exact_folds (the bf16 mode): the folds on the exact-fp32
    path."""
    dev = lat[0].device
    with small_batched():  # bf16: the four folds as one launch (exact-fp32 path, same bits)
        fb = level.folded_biases(geo, P, lat, exact_folds)
    buf = level.buffer("train_art", f"fwd{'bf' if mixed else ''}{tag}",
                       L.lib().aon_mlp_art_packed_bytes(), dev, guard=True,
                       params=[t for wb in P for t in wb])
    if mixed:
        L.call("aon_mlp_art_pack_mixed", L.ctypes.byref(_params_struct(P, fb)), mixed, L.ptr(buf),
               L.stream(dev))
    else:
        L.call("aon_mlp_art_pack", L.ctypes.byref(_params_struct(P, fb)), L.ptr(buf), L.stream(dev))
    return buf


def _pack_bwd(P, dev, tag="", bf16=False):
    """The transposed weight stream of the fused backward chain (aon_mlp_art_bwd_pack[_bf16])."""
    return level.pack_bwd("train_art", "aon_mlp_art_bwd_pack",
                          L.lib().aon_mlp_art_bwd_packed_bytes, _params_struct, P, dev, tag, bf16)


def _forward_level_fused(geo, P, lat, rays_o, rays_d, viewdirs, t_vals, raw, noise=None,
                         masks=None, bf16=False, enc_bf=None, return_enc_bf=False,
                         art_forward="f16_acts", timers=None, exact_folds=None):
    """_forward_level on the fused kernel (aon_mlp_art_fwd_train): raw (R x 4) and the kept
    activations (tiled, tiles.rows(R) rows each), the sample points (row-major) and pos_enc(x')
    (tiled, (tiles.rows(R), 64), column 63 zero); ``masks`` ((16, tiles.rows(R), 8) int32)
    receives the ReLU' bits of hd0..3, h0..7, hv0..3 for the backward chain.  bf16: the bf16
    mode (aon_mlp_art_fwd_train_bf16; hd / h / bot / hv kept as torch.bfloat16; enc keeps
    columns 0..15 only, (tiles.rows(R), 16) -- the chain reads x' = columns 0..2 -- and
    ``enc_bf`` ((tiles.rows(R), 128) bfloat16, allocated when None) receives pos_enc(x') tiled,
    columns 63.. zero: the enc-column weight gradients' operand; ``art_forward``: its forward numerics past
    the deformation MLP, TrainNumerics.art_forward).  enc_rows() converts enc for the all-GEMM
    backward.  ``timers``: hip events (bench.py); ``exact_folds``: the latent folds on the
    exact-fp32 path (None: as the mode computes them -- exact in bf16, fp16x3 otherwise)."""
    B, S = t_vals.shape
    R, dev = B * S, t_vals.device
    NR = tiles.rows(R)
    if masks is None:
        masks = torch.empty((16, NR, 8), dtype=torch.int32, device=dev)
    dt = torch.bfloat16 if bf16 else torch.float32
    hd = torch.empty((4, NR, geo.wd), device=dev, dtype=dt)
    h = torch.empty((8, NR, geo.nw), device=dev, dtype=dt)
    bot = torch.empty((NR, geo.nw), device=dev, dtype=dt)
    hv = torch.empty((4, NR, geo.wc), device=dev, dtype=dt)
    enc = torch.empty((NR, 16 if bf16 else 64), device=dev)
    if bf16 and enc_bf is None:
        enc_bf = torch.empty((NR, 128), device=dev, dtype=torch.bfloat16)
    xyz = torch.empty((R, 3), device=dev)
    mixed, mixed_stream = ART_FORWARD[art_forward] if bf16 else (0, False)
    # (f16_acts, 4, and f16x3, 0, read the plain fp16x3 stream)
    packed = _pack(geo, P, lat, S, mixed if mixed_stream else 0,
                   exact_folds=bf16 if exact_folds is None else exact_folds)
    ev = level.events(timers)
    args = (L.ptr(packed), L.ptr(rays_o), L.ptr(rays_d), L.ptr(viewdirs), L.ptr(t_vals), B, S,
            L.ptr(noise) if noise is not None else None, L.ptr(hd), L.ptr(h), L.ptr(bot),
            L.ptr(hv), L.ptr(enc), L.ptr(xyz), L.ptr(raw), L.ptr(masks))
    if bf16:
        L.call("aon_mlp_art_fwd_train_bf16", *args, L.ptr(enc_bf), mixed, L.stream(dev))
    else:
        L.call("aon_mlp_art_fwd_train", *args, L.stream(dev))
    L.snapshot_pack(packed)  # the forward was the pack's last reader (range guard, _lib)
    level.record(timers, ev, f"art_fwd_train{S}", R)
    return (xyz, hd, enc, h, bot, hv) + ((enc_bf,) if return_enc_bf else ())


def enc_rows(geo, enc, R):
    """pos_enc(x') row-major (R, 63) fp32 from what a level's forward kept: as is (the
    layer-by-layer forward), untiled (the fused fp16x3 forward's (NR, 64)), or recomputed from
    x' (the fused bf16 forward keeps columns 0..15 only) by aon_pos_enc -- the kernel's own
    pos_enc_feature, bit-identical."""
    if enc.shape[1] == geo.ne:
        return enc
    if enc.shape[1] == 64:
        return tiles.untile(enc, R)[:, :geo.ne].contiguous()
    xp = tiles.untile(enc, R)[:, :3].contiguous()
    out = torch.empty((R, geo.ne), device=enc.device)
    L.call("aon_pos_enc", L.ptr(xp), R, geo.min_deg, geo.max_deg, L.ptr(out), L.stream(enc.device))
    return out


def _enc_tiled(enc, width):
    """The chain's enc operand (tiled, ``width`` columns) from a row-major (R, 63) pos_enc(x')."""
    if enc.shape[1] == width:
        return enc
    pad = torch.zeros((enc.shape[0], width), device=enc.device)
    n = min(width, enc.shape[1])
    pad[:, :n] = enc[:, :n]
    return tiles.tile(pad)


def _backward_level(geo, P, G, lat, dlat, xyz, enc, venc, S, hd, h, bot, hv, draw):
    """Autograd of _forward_level from dL/draw (R x 4): G[i] = (dW, db) of layer i; dlat =
    (dshape, dapp, dart) (1 x n each) receive the latent-code gradients.  Every dY enters the
    f16x3 split at a per-call power-of-two scale from max |dY| (aon_absmax -> a_amax; for the
    density column of d raw, from all of d raw), as the fused chain scales its gradients."""
    R, dev = xyz.shape[0], xyz.device
    wd, nw, wc, ne, nv = geo.wd, geo.nw, geo.wc, geo.ne, geo.nv
    enc = enc_rows(geo, enc, R)
    shape, app, art = lat
    dshape, dapp, dart = dlat
    word = torch.zeros((1,), dtype=torch.int32, device=dev)  # stream-ordered: reused per call

    def dweight(i, dY, ldy, X, ldx, n_in, col0=0, rdiv=1, bias=True, of=None):
        # ``of``: the tensor whose max scales dY (default dY itself)
        level.gemm_dweight(G[i][0], G[i][1] if bias else None, dY, ldy, X, ldx, n_in, R,
                           col0=col0, rdiv=rdiv, amax=_amax_word(dY if of is None else of, word))

    def dinput(dX, dY, ldy, i, col0, n_in, mask=None, accumulate=False, of=None):
        level.gemm_dinput(dX, dY, ldy, P[i][0], n_in, R, col0=col0, mask=mask,
                          accumulate=accumulate, amax=_amax_word(dY if of is None else of, word))

    def dlatent(i, col0, l, dl, accumulate):
        level.dlatent(*G[i], P[i][0], col0, l, dl, accumulate)

    # rgb head and the view branch
    dweight(RGB, draw, 4, hv[3], wc, wc)
    dz = torch.empty((R, wc), device=dev)
    dz2 = torch.empty((R, wc), device=dev)
    dinput(dz, draw, 4, RGB, 0, wc, mask=hv[3])
    for i in range(3, 0, -1):
        dweight(VIEW0 + i, dz, wc, hv[i - 1], wc, wc)
        dinput(dz2, dz, wc, VIEW0 + i, 0, wc, mask=hv[i - 1])
        dz, dz2 = dz2, dz
    dweight(VIEW0, dz, wc, bot, nw, nw)
    dweight(VIEW0, dz, wc, venc, nv, nv, col0=nw, rdiv=S, bias=False)
    dlatent(VIEW0, nw + nv, app, dapp, False)
    dbot = torch.empty((R, nw), device=dev)
    dinput(dbot, dz, wc, VIEW0, 0, nw)  # the bottleneck has no activation
    del dz, dz2
    # bottleneck + density heads on h7
    dweight(BOT, dbot, nw, h[7], nw, nw)
    dweight(DENS, draw[:, 3:], 4, h[7], nw, nw, of=draw)  # the sigma column at d raw's scale
    dy = torch.empty((R, nw), device=dev)
    dinput(dy, dbot, nw, BOT, 0, nw)
    dinput(dy, draw[:, 3:], 4, DENS, 0, nw, mask=h[7], accumulate=True, of=draw)
    del dbot
    # trunk; the gradient w.r.t. enc = pos_enc(x') collects the skip and the first layer
    denc = torch.empty((R, ne), device=dev)
    dx = torch.empty((R, nw), device=dev)
    for i in range(7, -1, -1):  # dy = dL/d(pre-activation of pts_linears.i)
        if i == 5:
            dweight(PTS0 + 5, dy, nw, h[4], nw, nw)
            dweight(PTS0 + 5, dy, nw, enc, ne, ne, col0=nw, bias=False)
            dlatent(PTS0 + 5, nw + ne, shape, dshape, False)
            dinput(denc, dy, nw, PTS0 + 5, nw, ne)
        elif i == 0:
            dweight(PTS0, dy, nw, enc, ne, ne)
            dlatent(PTS0, ne, shape, dshape, True)
            dinput(denc, dy, nw, PTS0, 0, ne, accumulate=True)
        else:
            dweight(PTS0 + i, dy, nw, h[i - 1], nw, nw)
        if i > 0:
            dinput(dx, dy, nw, PTS0 + i, 0, nw, mask=h[i - 1])
            dx, dy = dy, dx
    del dx, dy
    # x' = deformation_layer(hd3) + xyz, enc = pos_enc(x') (:205-212)
    dxp = torch.empty((R, 3), device=dev)
    L.call("aon_pos_enc_bwd", L.ptr(enc), ne, L.ptr(denc), ne, R, geo.min_deg, geo.max_deg, 0,
           L.ptr(dxp), 3, L.stream(dev))
    del denc
    dweight(DL, dxp, 3, hd[3], wd, wd)
    dz = torch.empty((R, wd), device=dev)
    dz2 = torch.empty((R, wd), device=dev)
    dinput(dz, dxp, 3, DL, 0, wd, mask=hd[3])
    for i in range(3, 0, -1):
        dweight(DEF0 + i, dz, wd, hd[i - 1], wd, wd)
        dinput(dz2, dz, wd, DEF0 + i, 0, wd, mask=hd[i - 1])
        dz, dz2 = dz2, dz
    # deformations_linear.0 on cat[xyz, shape, art]
    dweight(DEF0, dz, wd, xyz, 3, 3)
    dlatent(DEF0, 3, shape, dshape, True)
    dlatent(DEF0, 3 + geo.n_shape, art, dart, False)


def _chain(geo, P, enc, S, draw, masks, bf16, timers=None):
    """The fused backward chain of one level (aon_mlp_art_bwd[_bf16]) from dL/d raw (R, 4) ->
    (dzv, dbot, dz, dxp, dzd, work): every layer's dL/d pre-activation, tiled (dxp row-major), and
    the word with the chain's per-call gradient scale.  ``enc``: the forward's pos_enc(x'), tiled
    or row-major (R, 63)."""
    R, dev = draw.shape[0], draw.device
    NR = tiles.rows(R)
    dt = torch.bfloat16 if bf16 else torch.float32
    dzv = torch.empty((4, NR, geo.wc), device=dev, dtype=dt)
    dbot = torch.empty((NR, geo.nw), device=dev, dtype=dt)
    dz = torch.empty((8, NR, geo.nw), device=dev, dtype=dt)
    dxp = torch.empty((R, 3), device=dev)
    dzd = torch.empty((4, NR, geo.wd), device=dev, dtype=dt)
    work = level.buffer("train_art", "work", 4, dev)
    packed = _pack_bwd(P, dev, S, bf16)
    enc_chain = enc if enc.shape[1] != geo.ne else _enc_tiled(enc, 16 if bf16 else 64)
    ev = level.events(timers)
    L.call("aon_mlp_art_bwd_bf16" if bf16 else "aon_mlp_art_bwd", L.ptr(packed), L.ptr(draw),
           L.ptr(masks), L.ptr(enc_chain), R, L.ptr(dzv), L.ptr(dbot), L.ptr(dz), L.ptr(dxp),
           L.ptr(dzd), L.ptr(work), L.stream(dev))
    L.snapshot_pack(packed)  # the chain was the pack's last reader
    level.record(timers, ev, f"art_bwd_chain{S}", R)
    return dzv, dbot, dz, dxp, dzd, work


def _backward_level_latent(geo, P, dlat, enc, S, draw, masks, bf16, timers=None):
    """The latent-code gradients alone (``latent_only``: the MLPs are frozen): the chain as
    _backward_level_fused launches it, then ONE aon_art_latent_grad on four of its tensors --
    dl = (sum_rows dZ)^T W[:, latent columns] needs the column sums of dzv[0], dz[5], dz[0] and
    dzd[0] (768 of the chain's 3,328 columns) and no activation; no weight gradient is formed
    and no aon_gemm runs.  dlat = (dshape, dapp, dart), (1, n) each, overwritten."""
    R, dev = draw.shape[0], draw.device
    dzv, _, dz, _, dzd, _ = _chain(geo, P, enc, S, draw, masks, bf16, timers)
    nbytes = L.lib().aon_art_latent_grad_workspace_bytes(R)
    work = level.buffer("train_art", f"latent{nbytes}", nbytes, dev)  # sized by R: one per size
    ev = level.events(timers)
    L.call("aon_art_latent_grad", L.ctypes.byref(_params_struct(P)), L.ptr(dzv[0]), L.ptr(dz[5]),
           L.ptr(dz[0]), L.ptr(dzd[0]), int(bf16), R, *(L.ptr(d) for d in dlat), L.ptr(work),
           L.stream(dev))
    level.record(timers, ev, f"art_dlatent{S}", R)


def _backward_level_fused(geo, P, G, lat, dlat, xyz, enc, venc, S, hd, h, bot, hv, draw,
                          masks=None, h_tiled=True, enc_bf=None, timers=None, cfg=DEFAULT):
    """_backward_level with every input-gradient product (and pos_enc's backward) in one fused
    kernel (aon_mlp_art_bwd); the weight gradients dW = dZ^T X, db = sum_rows dZ and the latent
    terms stay GEMMs.  ``masks``: the fused forward's ReLU' bits (built from the activations
    when None); h_tiled: hd / h / bot / hv in the fused forward's tiled layout (else
    row-major); the chain's dzv / dbot / dz / dzd are tiled.  enc: the fused forward's tiled
    pos_enc(x') ((NR, 64) fp16x3, (NR, 16) bf16) or the layer-by-layer forward's row-major
    (R, 63).  enc_bf: the bf16 forward's tiled 128-column pos_enc(x') (the enc-column weight
    gradients then run on the LDS-DMA kernel).  ``timers``: hip events (bench.py); ``cfg``: the
    model's TrainNumerics (the weight-gradient batching)."""
    R, dev = xyz.shape[0], xyz.device
    bf16 = h[0].dtype == torch.bfloat16  # activations kept by the bf16 training forward
    if masks is None:
        acts = list(hd) + list(h) + list(hv)
        masks = relu_masks([tiles.untile(a, R).float() for a in acts] if h_tiled else acts, R)
    wd, nw, wc, ne, nv = geo.wd, geo.nw, geo.wc, geo.ne, geo.nv
    shape, app, art = lat
    dshape, dapp, dart = dlat
    enc_t = enc.shape[1] != ne  # the fused forward's tiled copy
    dzv, dbot, dz, dxp, dzd, work = _chain(geo, P, enc, S, draw, masks, bf16, timers)
    ev = level.events(timers)

    # the operands (level.Operand): d raw and dL/dx' row-major, the chain's gradients tiled (the
    # deformation branch's at the fixed 2^10), the kept activations tiled after the fused forward
    (d_raw, d_sigma), d_xp = level.draw_operands(draw), level.Operand(dxp, 3, False, level.DXP)
    d_bot, *d_z = level.operands((dbot, *dz.unbind(0)), nw, True, level.CHAIN)
    d_zv = level.operands(dzv.unbind(0), wc, True, level.CHAIN)
    d_zd = level.operands(dzd.unbind(0), wd, True, level.CHAIN_DEF)
    x_hd, x_hv = level.operands(hd, wd, h_tiled, level.ACT), level.operands(hv, wc, h_tiled, level.ACT)
    x_bot, *x_h = level.operands((bot, *h), nw, h_tiled, level.ACT)
    if bf16 and enc_bf is not None:
        x_enc = level.enc_operand(enc_bf)
    elif enc_t and enc.shape[1] != 64:
        raise ValueError("the bf16 forward keeps 16 enc columns: pass its enc_bf")
    else:
        x_enc = level.enc_operand(enc)
    x_venc, x_xyz = level.Operand(venc, nv, False, level.VENC), level.Operand(xyz, 3, False, level.XYZ)

    dweight = functools.partial(level.dweight, G, R, bf16, work)

    def dlatent(i, col0, l, dl, accumulate):
        # (bf16 mode: the exact-fp32 tiny-product path)
        level.dlatent(*G[i], P[i][0], col0, l, dl, accumulate, exact=bf16)

    # every whole-tile product of the level deferred to aon_gemm_batch launches (bf16: the eight
    # 256 x 256 ones -- bottleneck, pts_linears.1-7 -- and the 128-wide view / deformation / enc
    # column ones; fp16x3: all as the fp16x3 class), flushed before the latent terms read the
    # bias gradients; the latent terms then run in the same order as before (bit-identical)
    with batched(cfg.batch_dweights, cfg.batch_128):
        dweight(RGB, d_raw, x_hv[3])                                      # rgb_layer
        for i in range(3, 0, -1):                                         # views_linear.i
            dweight(VIEW0 + i, d_zv[i], x_hv[i - 1])
        dweight(VIEW0, d_zv[0], x_bot)                                    # views_linear.0
        dweight(VIEW0, d_zv[0], x_venc, col0=nw, rdiv=S, bias=False)
        dweight(BOT, d_bot, x_h[7])                                       # bottleneck
        dweight(DENS, d_sigma, x_h[7])                                    # density
        for i in range(7, 0, -1):                                         # pts_linears.i
            dweight(PTS0 + i, d_z[i], x_h[i - 1])
        dweight(PTS0 + 5, d_z[5], x_enc, col0=nw, bias=False)
        dweight(PTS0, d_z[0], x_enc)                                      # pts_linears.0
        dweight(DL, d_xp, x_hd[3])                                        # deformation_layer
        for i in range(3, 0, -1):                                         # deformations_linear.i
            dweight(DEF0 + i, d_zd[i], x_hd[i - 1])
        if bf16:  # deformations_linear.0's xyz columns: (xyz^T dZ)^T on the skinny kernel, the
            # bias gradient as dZ's column sums (a 128-wide tile for 3 columns took 0.12 ms)
            gemm(G[DEF0][0], xyz, dzd[0], 3, wd, R, lda=3, a_kc=False, ldb=wd, b_kc=False,
                 ldc=G[DEF0][0].stride(0), rowsum=G[DEF0][1], mma_bf16=True, b_tiled=True,
                 c_trans=True)
        else:
            dweight(DEF0, d_zd[0], x_xyz)                                 # deformations_linear.0
    # the latent terms read the bias gradients just flushed; bf16 (exact-fp32 tiny products): all
    # ten as ONE aon_gemm_small_batch launch, bit-identical to ten launches in this order
    with small_batched():
        dlatent(VIEW0, nw + nv, app, dapp, False)
        dlatent(PTS0 + 5, nw + ne, shape, dshape, False)
        dlatent(PTS0, ne, shape, dshape, True)
        dlatent(DEF0, 3, shape, dshape, True)
        dlatent(DEF0, 3 + geo.n_shape, art, dart, False)
    level.record(timers, ev, f"art_dweight{S}", R)


class ArtRenderLevel(torch.autograd.Function):
    """cast_rays + articulated NeRFMLP + activations + volumetric_rendering of one level
    (model_autodecoder.py:296-333) with gradients for the level's 40 MLP parameters and the
    three latent codes (density = shape, color = appearance, articulation).  ``latent_only``
    (render_level): gradients for the codes alone -- the same forward and chain, then
    _backward_level_latent instead of the weight gradients; no activation is kept."""

    @staticmethod
    def forward(ctx, geo, cfg, timers, latent_only, rays_o, rays_d, viewdirs, t_vals, white_bkgd,
                noise, shape, app, art, *params):
        # cfg: the model's TrainNumerics; timers: a dict of hip events (bench.py) or None
        B, S = t_vals.shape
        R, dev = B * S, t_vals.device
        lat = tuple(L.contig(x.detach().reshape(1, -1)) for x in (shape, app, art))
        L.require_gpu(rays_o, rays_d, viewdirs, t_vals, *lat)
        if lat[0].shape[1] != geo.n_shape or lat[1].shape[1] != geo.n_app or lat[2].shape[1] != geo.n_art:
            raise ValueError("latent code sizes do not match the MLP")
        for p in params:
            if not p.is_contiguous():
                raise ValueError("MLP parameters must be contiguous")
        venc = torch.empty((B, geo.nv), device=dev)
        L.call("aon_pos_enc", L.ptr(viewdirs), B, 0, geo.deg_view, L.ptr(venc), L.stream(dev))
        P = [(params[2 * i], params[2 * i + 1]) for i in range(20)]
        # the kernels' layer order, shapes, dtype and device (ValueError, before any launch)
        L.check_mlp_art_layers(P)
        raw = torch.empty((R, 4), device=dev)
        noise = L.contig(noise) if noise is not None else None
        masks = None  # ReLU' bits for the fused backward chain (built there when None)
        enc_bf = None  # the bf16 forward's tiled pos_enc(x') copy
        if cfg.fused_forward and geo.fused_ok:
            masks = torch.empty((16, tiles.rows(R), 8), dtype=torch.int32, device=dev)
            xyz, hd, enc, h, bot, hv, enc_bf = _forward_level_fused(
                geo, P, lat, L.contig(rays_o), L.contig(rays_d), L.contig(viewdirs),
                L.contig(t_vals), raw, noise, masks, bf16=cfg.bf16, return_enc_bf=True,
                art_forward=cfg.art_forward, timers=timers)
        else:
            xyz = torch.empty((R, 3), device=dev)
            L.call("aon_cast_rays", L.ptr(rays_o), L.ptr(rays_d), L.ptr(t_vals), B, S, None, 0,
                   L.ptr(xyz), 0, 0, None, L.stream(dev))
            hd, enc, h, bot, hv = _forward_level(geo, P, lat, xyz, venc, S, raw, noise,
                                                 exact_folds=cfg.bf16)
        comp, acc, depth, weights = level.composite_fwd(raw, t_vals, rays_d, white_bkgd,
                                                        L.ACT_ARTIC)
        ctx.enc_bf = enc_bf if masks is not None else None
        ctx.h_tiled = masks is not None  # the fused forward keeps its tensors tiled
        ctx.latent_only = latent_only
        if latent_only:  # only what the chain and aon_art_latent_grad read
            if masks is None:  # (the layer-by-layer forward: row-major activations)
                masks = relu_masks(list(hd) + list(h) + list(hv), R)
            ctx.bf16 = hd.dtype == torch.bfloat16  # as the kept activations, like the full backward
            ctx.enc_bf = None
            ctx.save_for_backward(rays_d, t_vals, enc, raw, *params)
        else:
            ctx.save_for_backward(rays_d, t_vals, xyz, enc, venc, raw, hd, h, bot, hv, *lat,
                                  *params)
        ctx.masks = masks
        ctx.meta = (geo, B, S, bool(white_bkgd), tuple(x.shape for x in (shape, app, art)))
        ctx.cfg, ctx.timers = cfg, timers
        ctx.mark_non_differentiable(weights)
        # unused outputs (acc, depth, weights in training_step) get no zero-filled gradients
        ctx.set_materialize_grads(False)
        return comp, acc, depth, weights

    @staticmethod
    def backward(ctx, g_rgb, g_acc, g_depth, _g_w):
        geo, B, S, white, lat_shapes = ctx.meta
        saved = ctx.saved_tensors
        if ctx.latent_only:
            rays_d, t_vals, enc, raw = saved[:4]
            params = saved[4:]
            draw = level.composite_bwd(raw, t_vals, rays_d, B, S, white, L.ACT_ARTIC, g_rgb,
                                       g_acc, g_depth)
            P = [(params[2 * i], params[2 * i + 1]) for i in range(20)]
            dlat = tuple(torch.empty((1, n), device=raw.device)
                         for n in (geo.n_shape, geo.n_app, geo.n_art))
            _backward_level_latent(geo, P, dlat, enc, S, draw, ctx.masks, ctx.bf16, ctx.timers)
            dlat = [d.reshape(s) for d, s in zip(dlat, lat_shapes)]
            return (None,) * 10 + (*dlat,) + (None,) * 40
        rays_d, t_vals, xyz, enc, venc, raw, hd, h, bot, hv = saved[:10]
        lat = saved[10:13]
        params = saved[13:]
        R = B * S
        draw = level.composite_bwd(raw, t_vals, rays_d, B, S, white, L.ACT_ARTIC, g_rgb, g_acc,
                                   g_depth)
        P = [(params[2 * i], params[2 * i + 1]) for i in range(20)]
        G = [(torch.empty_like(w), torch.empty_like(b)) for w, b in P]
        dlat = tuple(torch.empty_like(x) for x in lat)
        if ctx.cfg.fused_backward and geo.fused_ok:
            _backward_level_fused(geo, P, G, lat, dlat, xyz, enc, venc, S, hd, h, bot, hv, draw,
                                  ctx.masks, ctx.h_tiled, ctx.enc_bf, timers=ctx.timers,
                                  cfg=ctx.cfg)
        else:
            if ctx.h_tiled:  # the all-GEMM backward reads row-major fp32 activations
                hd, h, hv = (torch.stack([tiles.untile(x, R).float() for x in t]) for t in (hd, h, hv))
                bot = tiles.untile(bot, R).float()
            _backward_level(geo, P, G, lat, dlat, xyz, enc, venc, S, hd, h, bot, hv, draw)
        grads = [g for pair in G for g in pair]
        dlat = [d.reshape(s) for d, s in zip(dlat, lat_shapes)]
        return (None, None, None, None, None, None, None, None, None, None, *dlat, *grads)


def render_level(mlp, rays_o, rays_d, viewdirs, t_vals, white_bkgd, latents, noise=None,
                 cfg=DEFAULT, timers=None, latent_only=False):
    """One NeRF_AE_Art level under autograd -> (comp_rgb, acc, depth, weights); ``cfg``: the
    model's TrainNumerics.  ``latent_only``: the backward computes the latent codes' gradients
    alone (aon_art_latent_grad after the fused chain: no weight gradient, no kept activation)
    and returns None for every MLP parameter -- for fitting codes with the MLPs frozen
    (latent_fit.py).  It needs every MLP parameter frozen and the fused backward (ValueError
    otherwise, before any launch)."""
    params = [p for m in art_layers(mlp) for p in (m.weight, m.bias)]
    geo = level.geo_of(mlp)
    if not geo.default_depths:
        raise ValueError("the articulated training path implements the reference's default layer "
                         "counts (netdepth 8, skip 4, 4 deformation / 4 condition layers)")
    if latent_only:
        if any(p.requires_grad for p in params):
            raise ValueError("latent_only: an MLP parameter requires grad -- freeze the MLPs "
                             "(latent_fit.freeze) or take the full backward (latent_only=False)")
        if not (cfg.fused_backward and geo.fused_ok):
            raise ValueError("latent_only needs the fused backward chain (TrainNumerics."
                             "fused_backward and the default MLP geometry)")
    return ArtRenderLevel.apply(geo, cfg, timers, bool(latent_only), rays_o, rays_d, viewdirs,
                                t_vals, bool(white_bkgd), noise,
                                latents["density"], latents["color"], latents["articulation"],
                                *params)


class LatentReg(torch.autograd.Function):
    """The latent regulariser of training_step (model_autodecoder.py:456-466):
    1e-4 * (mean ||shape||_0 + mean ||appearance||_0 + mean ||articulation||_0), norms over
    dim 0 (aon_latent_reg)."""

    @staticmethod
    def forward(ctx, shape, app, art):
        codes = [L.contig(x.detach()) for x in (shape, app, art)]
        L.require_gpu(*codes)
        loss = torch.empty((), device=shape.device)
        grads = []
        for i, c in enumerate(codes):
            c2 = c.reshape(c.shape[0], -1)  # norm over dim 0: (1, C) -> |x|, (C,) -> ||x||
            g = torch.empty_like(c)
            L.call("aon_latent_reg", L.ptr(c2), c2.shape[0], c2.shape[1], 1e-4, int(i > 0),
                   L.ptr(loss), L.ptr(g), L.stream(shape.device))
            grads.append(g)
        ctx.save_for_backward(*grads)
        return loss

    @staticmethod
    def backward(ctx, g):
        # the regulariser is a leaf term of the loss: g is dL/dreg = 1 (a scalar multiply by
        # a non-unit g would be the only torch arithmetic; training_step always passes 1)
        return tuple(x * g for x in ctx.saved_tensors)


def opacity_loss(rendered_results, instance_mask):
    """LitNeRF_AutoDecoder.opacity_loss (model_autodecoder.py:703-717): sum over the two levels
    of mean((clamp(acc, 0, 1) - mask)^2) -> a scalar under autograd (train.MaskedLoss, its
    colour terms skipped).  ``rendered_results`` = the model's [(rgb, acc, depth)] per level."""
    return masked_loss(None, None, rendered_results[0][1], rendered_results[1][1], None,
                       instance_mask, opacity="mse")[3]


def opacity_loss_CE(rendered_results, instance_mask, opacity_lambda=0.05):
    """LitNeRF_AutoDecoder.opacity_loss_CE (model_autodecoder.py:719-736): opacity_lambda * the
    levels' BCEWithLogitsLoss(acc, mask); the reference hard-codes opacity_lambda 0.05 here and
    0.5 in model_ae_art.py:646-663."""
    return masked_loss(None, None, rendered_results[0][1], rendered_results[1][1], None,
                       instance_mask, opacity="ce", opacity_lambda=opacity_lambda)[3]


def opacity_loss_autorf(rendered_results, instance_mask):
    """LitNeRF_AutoDecoder.opacity_loss_autorf (model_autodecoder.py:738-766) as the reference
    writes it: its fine foreground term reads the coarse opacity (:761-763), kept for parity."""
    return masked_loss(None, None, rendered_results[0][1], rendered_results[1][1], None,
                       instance_mask, opacity="autorf")[3]


def training_step(model, code_library, batch, randomized, white_bkgd, near, far, *,
                  u_coarse=None, u_fine=None, timers=None, opacity=None, opacity_lambda=0.05,
                  mask_rgb=False):
    """LitNeRF_AutoDecoder.training_step (model_autodecoder.py:395-477) ->
    (loss, logs{loss0, loss1, reg, psnr0, psnr1}).  ``batch`` holds rays_o / rays_d / viewdirs /
    target (B, 3) and instance_id / articulation_id (1,) as the reference's loader gives them
    after its squeeze (model_autodecoder.py:396-399).  The kernels and precision are the model's
    own (model.train_numerics).

    Mask supervision (the reference's commented-out terms, model_autodecoder.py:423-426 and
    :441-454; live in model_ae_art.py:380-408): ``opacity`` = "mse" / "ce" / "autorf" adds
    opacity_loss / opacity_loss_CE (weighted by ``opacity_lambda``) / opacity_loss_autorf of the
    two levels' acc against batch["instance_mask"] (or batch["mask"]); ``mask_rgb`` takes the
    colour losses over the foreground rays only.  The whole loss is then one aon_loss_masked
    launch and ``logs`` gains ``opacity``.  With the defaults nothing changes."""
    return step_on_latents(model, lambda: code_library(batch), batch, randomized, white_bkgd, near,
                           far, u_coarse=u_coarse, u_fine=u_fine, timers=timers, opacity=opacity,
                           opacity_lambda=opacity_lambda, mask_rgb=mask_rgb)


def step_on_latents(model, lookup, batch, randomized, white_bkgd, near, far, *, u_coarse=None,
                    u_fine=None, timers=None, opacity=None, opacity_lambda=0.05, mask_rgb=False,
                    latent_only=False):
    """training_step's forward and loss assembly on the latent dict ``lookup()`` returns (looked
    up after the mask check, as training_step always did): shared with latent_fit.fit_step, which
    passes ``latent_only`` on to the model."""
    masked = opacity is not None or mask_rgb
    if masked:
        mask = batch.get("instance_mask", batch.get("mask"))
        if mask is None:
            raise ValueError("training_step: opacity / mask_rgb need batch['instance_mask'] "
                             "(or batch['mask'])")
    latents = lookup()
    ret = model(batch, randomized, white_bkgd, near, far, latents, u_coarse=u_coarse,
                u_fine=u_fine, timers=timers, **({"latent_only": True} if latent_only else {}))
    reg = LatentReg.apply(latents["density"], latents["color"], latents["articulation"])
    if masked:
        loss, loss0, loss1, op, psnr0, psnr1 = masked_loss(
            ret[0][0], ret[1][0], ret[0][1], ret[1][1], batch["target"], mask, reg,
            opacity=opacity, opacity_lambda=opacity_lambda, mask_rgb=mask_rgb)
        return loss, dict(loss0=loss0, loss1=loss1, reg=reg, psnr0=psnr0, psnr1=psnr1, opacity=op)
    # loss1 + loss0 + reg and the psnrs in one launch (train.LossPair)
    loss, loss0, loss1, psnr0, psnr1 = loss_pair(ret[0][0], ret[1][0], batch["target"], reg)
    return loss, dict(loss0=loss0, loss1=loss1, reg=reg, psnr0=psnr0, psnr1=psnr1)


def configure_optimizers(model, code_library, lr_init=5.0e-4):
    """configure_optimizers (model_autodecoder.py:599-601): Adam over the MLPs and the code
    library (the fused aon_adam_step, betas (0.9, 0.999))."""
    return Adam(list(model.parameters()) + list(code_library.parameters()), lr=lr_init,
                betas=(0.9, 0.999))
