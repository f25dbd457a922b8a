"""What the vanilla and the articulated render level share (train.py / train_art.py,
model_autodecoder.py, and two_level.py, the coarse/fine driver of both models, which holds what
happens above a level), once: the event timers; the cache of packed weight streams, whose
namespace ("train", "train_art") is also the name the fp16x3 range guard keeps a pack under;
the compositor calls with their allocations; the weight gradients dW = dZ^T X of the fused
backward chains' kept tensors, each operand an ``Operand`` record that dweight_kwargs turns into
aon_gemm's layout / scale / kernel-licence keywords; the all-GEMM backward products; and the
articulated network layer by layer -- Geo, the latent folds, and art_forward, the one walker
over its layers (training keeps one tensor per layer, inference alternates two buffers per
width: LayerBuffers).  Callers launch what they launched before they shared this, and so does
two_level.py above them: same entry points, arguments, order and allocations (there also the
same random draws in the same order)."""
import collections

import torch

from . import _lib as L
from .linalg import ACT_SCALE, GRAD_SCALE, W_SCALE, gemm, linear_fwd


# ---------------------------------------------------------------------------- timers
def events(timers):
    """HIP events bracketing launches on the current stream (the stream the C ABI uses)."""
    if timers is None:
        return None
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    return ev


def record(timers, ev, key, rows):
    if ev is not None:
        ev[1].record()
        timers.setdefault(key, []).append((ev[0], ev[1], rows))


# ---------------------------------------------------------------------------- pack cache
_packed = {}


def buffer(ns, key, nbytes, dev, guard=False, params=()):
    """One buffer per namespace, kind and device (pack and reader are stream-ordered).  guard: a
    packed weight stream whose status word the next optimizer step over ``params`` checks."""
    buf = _packed.get((ns, key, str(dev)))
    if buf is None:
        buf = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)
        _packed[(ns, key, str(dev))] = buf
    if guard:
        L.register_pack((ns, key), buf, params)
    return buf


def pack_bwd(ns, entry, packed_bytes, params_struct, P, dev, tag="", bf16=False):
    """A fused backward chain's transposed weight stream, packed by ``entry``[_bf16]."""
    buf = buffer(ns, f"bwd{'bf' if bf16 else ''}{tag}", packed_bytes(), dev, guard=not bf16,
                 params=[t for wb in P for t in wb])
    L.call(entry + "_bf16" if bf16 else entry, L.ctypes.byref(params_struct(P)), L.ptr(buf),
           L.stream(dev))
    return buf


# ---------------------------------------------------------------------------- compositor
def composite_fwd(raw, t_vals, rays_d, white_bkgd, act, keep_weights=True):
    """volumetric_rendering of raw (B*S, 4) = [rgb, sigma] (aon_composite_fwd; ``act``: the
    activations still to apply) -> (comp, acc, depth, weights or None)."""
    B, S = t_vals.shape
    dev = t_vals.device
    comp = torch.empty((B, 3), device=dev)
    acc = torch.empty((B,), device=dev)
    weights = torch.empty((B, S), device=dev) if keep_weights else None
    depth = torch.empty((B,), device=dev)
    L.call("aon_composite_fwd", L.ptr(raw), 4, L.ptr(raw[:, 3:]), 4, L.ptr(t_vals), L.ptr(rays_d),
           B, S, int(bool(white_bkgd)), act, L.ptr(comp), L.ptr(acc), L.ptr(weights), L.ptr(depth),
           L.stream(dev))
    return comp, acc, depth, weights


def composite_bwd(raw, t_vals, rays_d, B, S, white, act, g_rgb, g_acc, g_depth):
    """dL/draw (B*S, 4) from the gradients of comp / acc / depth (None: an unused output)."""
    dev = raw.device
    draw = torch.empty((B * S, 4), device=dev)
    g_rgb = L.contig(g_rgb) if g_rgb is not None else torch.zeros((B, 3), device=dev)
    L.call("aon_composite_bwd", L.ptr(raw), 4, L.ptr(raw[:, 3:]), 4, L.ptr(t_vals), L.ptr(rays_d),
           B, S, int(white), act, L.ptr(g_rgb),
           L.ptr(L.contig(g_acc)) if g_acc is not None else None,
           L.ptr(L.contig(g_depth)) if g_depth is not None else None,
           L.ptr(draw), L.ptr(draw[:, 3:]), 4, L.stream(dev))
    return draw


# ---------------------------------------------------------------------------- dW of kept tensors
# One operand of dW = dY^T X: tensor, leading dimension, tiled (tiles.py) or not, and its kind
Operand = collections.namedtuple("Operand", "t ld tiled kind")

# dY kinds.  CHAIN / DRAW / DRAW_SIGMA ride at the chain's per-call scale from max |d raw| (its
# work word); the deformation branch (DXP = dL/dx', CHAIN_DEF the chain below it) at a fixed 2^10
CHAIN, CHAIN_DEF, DRAW, DRAW_SIGMA, DXP = "chain", "chain_def", "draw", "draw_sigma", "dxp"
# X kinds: a kept activation, pos_enc(x) row-major (R, 63) / tiled fp32 (NR, 64) / tiled bf16
# (NR, 128), the per-ray view encodings (read with b_rdiv = S) and the sample points
ACT, ENC63, ENC_T64, ENC_T128_BF, VENC, XYZ = "act", "enc63", "enc_t64", "enc_t128_bf", "venc", "xyz"


def operands(ts, ld, tiled, kind):
    return [Operand(t, ld, tiled, kind) for t in ts]


def draw_operands(draw):
    """(d raw, its sigma column): row-major, ld 4."""
    return Operand(draw, 4, False, DRAW), Operand(draw[:, 3:], 4, False, DRAW_SIGMA)


def enc_operand(enc):
    """pos_enc(x) as a forward kept it: row-major (R, 63), tiled (NR, 64) or bf16 (NR, 128)."""
    n = enc.shape[1]
    return Operand(enc, n, n != 63, ENC63 if n == 63 else ENC_T64 if n == 64 else ENC_T128_BF)


def dweight_kwargs(a, b, n_out, bf16, work=None):
    """aon_gemm's keywords for dW (n_out x n_in) = a^T b over the rows, a / b Operands.  f16x3:
    dY at the chain's per-call scale (a_amax = ``work``) or the fixed 2^10, X at 2^-8 -- except
    the 256 x 256 / 128 x 256 / 256 x 64 products of the fused kernels' tiled tensors: one
    accumulator (f16_single), dY at the chain's scale and X at the forward's 2^3, the scales
    both kernels range-guard their own splits at (pos_enc(x) and x: far inside the range).
    bf16: one bf16 MFMA per product, no scales (bf16 has fp32's exponent range).  A tiled
    pos_enc(x) is read in whole 16-column tiles (n_in = its width), 63 columns of dW stored."""
    chain = a.kind not in (DXP, CHAIN_DEF)
    single = (not bf16 and chain and a.tiled and b.tiled
              and (n_out, b.ld) in ((256, 256), (128, 256), (256, 64)))
    return dict(n_in=b.ld, ldb=b.ld, a_tiled=a.tiled, b_tiled=b.tiled,
                n_store=63 if b.kind in (ENC_T64, ENC_T128_BF) else 0, f16_single=single,
                a_scale=1.0 if (chain or bf16) else GRAD_SCALE,
                b_scale=1.0 if bf16 else (8.0 if single else ACT_SCALE),
                a_amax=work if (chain and not bf16) else None, mma_bf16=bf16)


def dweight(G, R, bf16, work, i, a, b, col0=0, rdiv=1, bias=True):
    """Layer i's dW[:, col0:col0+n_in] = a^T b (K = R rows, split-K), db = sum_rows a.  (Bound
    by functools.partial in the callers: ~40 calls per step, whose host time shows in it.)"""
    dW, db = G[i]
    n_out, ldc = dW.shape  # (contiguous: empty_like of a checked parameter)
    kw = dweight_kwargs(a, b, n_out, bf16, work)
    gemm(dW[:, col0:] if col0 else dW, a[0], b[0], n_out, kw.pop("n_in"), R, lda=a[1], a_kc=False,
         b_kc=False, b_rdiv=rdiv, ldc=ldc, rowsum=db if bias else None, **kw)


# ---------------------------------------------------------------------------- all-GEMM backward
def gemm_dweight(dW, db, dY, ldy, X, ldx, n_in, R, *, col0=0, rdiv=1, amax=None):
    """dW[:, col0:col0+n_in] = dY^T X (K = R rows, split-K); db (or None) = sum_rows dY;
    ``amax``: the word with max |dY| (aon_absmax), dY's per-call f16x3 scale."""
    gemm(dW[:, col0:] if col0 else dW, dY, X, dW.shape[0], n_in, R, lda=ldy, a_kc=False, ldb=ldx,
         b_kc=False, b_rdiv=rdiv, ldc=dW.stride(0), a_scale=1.0, b_scale=ACT_SCALE, rowsum=db,
         a_amax=amax)


def gemm_dinput(dX, dY, ldy, W, n_in, R, *, col0=0, mask=None, accumulate=False, amax=None):
    """dX (R x n_in) (+)= dY W[:, col0:col0+n_in] (* relu'(mask))."""
    gemm(dX, dY, W[:, col0:] if col0 else W, R, n_in, W.shape[0], lda=ldy, a_kc=True,
         ldb=W.stride(0), b_kc=False, ldc=dX.stride(0), mask=mask,
         ldm=mask.stride(0) if mask is not None else 0, accumulate=accumulate, a_scale=1.0,
         b_scale=W_SCALE, a_amax=amax)


def dlatent(dW, db, W, col0, l, dl, accumulate, exact=False):
    """z = W [x; l] + b with the code l on every row: dW[:, col0:col0+n] = db l^T and dl (+)=
    db^T W[:, col0:col0+n] from the bias gradient alone (exact: bf16's exact-fp32 tiny path)."""
    n_out, n = W.shape[0], l.shape[1]
    gemm(dW[:, col0:], db, l, n_out, n, 1, lda=1, a_kc=True, ldb=n, b_kc=False, ldc=dW.stride(0),
         a_scale=GRAD_SCALE, b_scale=1.0, exact_fp32=exact)
    gemm(dl, db, W[:, col0:], 1, n, n_out, lda=n_out, a_kc=True, ldb=W.stride(0), b_kc=False,
         ldc=n, accumulate=accumulate, a_scale=GRAD_SCALE, b_scale=W_SCALE, exact_fp32=exact)


# ---------------------------------------------------------------------------- articulated network
# parameter layout of one articulated NeRFMLP of the default depths: 20 layers x (weight, bias)
DEF0, DL, PTS0, DENS, BOT, VIEW0, RGB = 0, 4, 5, 13, 14, 15, 19


def art_layers(mlp):
    """The nn.Linear layers of an articulated NeRFMLP in the kernels' order."""
    return (list(mlp.deformations_linear) + [mlp.deformation_layer] + list(mlp.pts_linears)
            + [mlp.density_layer, mlp.bottleneck_layer] + list(mlp.views_linear) + [mlp.rgb_layer])


class Geo:
    """Widths, depths and layer indices (art_layers order) of one articulated NeRFMLP."""

    def __init__(self, mlp):
        self.wd, self.nw, self.wc = mlp.netwidth_deformation, mlp.netwidth, mlp.netwidth_condition
        self.ne = mlp.pos_size_enc  # 3 + 6 (max_deg - min_deg)
        self.min_deg, self.max_deg, self.deg_view = mlp.min_deg_point, mlp.max_deg_point, mlp.deg_view
        self.nv = (mlp.deg_view * 2 + 1) * mlp.input_ch_view
        self.n_shape, self.n_app = mlp.shape_latent_dim, mlp.appearance_latent_dim
        self.n_art = mlp.articulation_latent_dim
        self.nd, self.depth, self.nc = mlp.netdepth_deformation, mlp.netdepth, mlp.netdepth_condition
        self.skip = mlp.skip_layer + 1  # the trunk layer that reads cat[h, enc, shape]
        self.DEF0, self.DL, self.PTS0, self.DENS = 0, self.nd, self.nd + 1, self.nd + 1 + self.depth
        self.BOT, self.VIEW0, self.RGB = self.DENS + 1, self.DENS + 2, self.DENS + 2 + self.nc
        # the training path and the fused kernels implement the reference's default layer counts
        self.default_depths = (mlp.netdepth == 8 and mlp.skip_layer == 4
                               and mlp.netdepth_deformation == 4 and mlp.netdepth_condition == 4
                               and mlp.input_ch == 3 and mlp.input_ch_view == 3
                               and mlp.num_rgb_channels == 3 and mlp.num_density_channels == 1)
        # the fused kernels are compiled for the default geometry (mlp_layout.hpp kShapeArt)
        self.fused_ok = (self.default_depths and mlp.netwidth == 256
                         and mlp.netwidth_deformation == 128 and mlp.netwidth_condition == 128
                         and mlp.min_deg_point == 0 and mlp.max_deg_point == 10
                         and mlp.deg_view == 4)


def geo_of(mlp):
    if getattr(mlp, "_geo", None) is None:
        mlp._geo = Geo(mlp)
    return mlp._geo


def fold(W, b, c0, lat, exact=False):
    """b + W[:, c0:c0+n] . lat (the latent columns of a layer as a per-call bias: one M = 1 GEMM
    with bias epilogue); exact (the bf16 mode): on aon_gemm's exact-fp32 tiny-product path."""
    N, n = W.shape[0], lat.shape[1]
    out = torch.empty((1, N), device=W.device)
    gemm(out, lat, W[:, c0:], 1, N, n, lda=n, a_kc=True, ldb=W.stride(0), b_kc=True, ldc=N,
         bias=b, a_scale=1.0, b_scale=W_SCALE, exact_fp32=exact)
    return out.reshape(-1)


def fold_args(geo, lat, i, lat_def=None):
    """(first latent column, latent row) of one of the four layers that read a code: DEF0 on
    cat[xyz, shape, art] (``lat_def``: that cat[shape, art] where the caller holds one), PTS0 on
    cat[enc, shape], the skip layer on cat[h, enc, shape], VIEW0 on cat[bottleneck, enc_dir, app]."""
    shape, app, art = lat
    if i == geo.DEF0:
        return 3, torch.cat([shape, art], -1) if lat_def is None else lat_def
    if i == geo.VIEW0:
        return geo.nw + geo.nv, app
    return (geo.ne if i == geo.PTS0 else geo.nw + geo.ne), shape


def folded_biases(geo, P, lat, exact=False, lat_def=None):
    """layer index -> folded bias of the four layers that read a latent code."""
    return {i: fold(*P[i], *fold_args(geo, lat, i, lat_def), exact)
            for i in (geo.DEF0, geo.PTS0, geo.PTS0 + geo.skip, geo.VIEW0)}


def folded_pairs(P, fb):
    """(weight, bias) in the kernels' layer order with the folded biases substituted."""
    return [(w, fb.get(i, b)) for i, (w, b) in enumerate(P)]


class LayerBuffers:
    """Where art_forward writes each layer's output.  ``raw`` given (training): one kept tensor
    per layer, stacked per branch in t["hd"], t["h"], t["bot"], t["hv"].  raw None (inference):
    two alternating buffers per branch (the bottleneck in the trunk's idle one), raw allocated
    when the heads write it: a full frame keeps no activation."""

    def __init__(self, geo, R, dev, raw=None):
        self.n = dict(hd=(geo.nd, geo.wd), h=(geo.depth, geo.nw), bot=(1, geo.nw), hv=(geo.nc, geo.wc))
        self.R, self.dev, self.kept, self.raw, self.t = R, dev, raw is not None, raw, {}

    def out(self, g, i=0):
        if g == "bot" and not self.kept:
            g, i = "h", self.n["h"][0]
        t = self.t.get(g)
        if t is None:
            n, w = self.n[g]
            t = self.t[g] = (torch.empty((n, self.R, w), device=self.dev) if self.kept else
                             tuple(torch.empty((self.R, w), device=self.dev) for _ in range(2)))
        return t[i] if self.kept else t[i & 1]


def art_deformation(geo, P, bias, xyz, bufs):
    """The deformation MLP of art_forward alone (model_autodecoder.py:196-205) -> delta (R, 3):
    also what NeRFMLP.deform computes when the fused deformation pass is off or out of range."""
    R, dev = xyz.shape[0], xyz.device
    # deformation MLP on cat[xyz, shape, art] (:196-203), the latent columns folded
    x = bufs.out("hd", 0)
    linear_fwd(x, xyz, 3, P[geo.DEF0][0], bias(geo.DEF0), relu=True)
    for i in range(1, geo.nd):
        y = bufs.out("hd", i)
        linear_fwd(y, x, geo.wd, *P[geo.DEF0 + i], relu=True)
        x = y
    delta = torch.empty((R, 3), device=dev)
    linear_fwd(delta, x, geo.wd, *P[geo.DL])  # deformation_layer (:205)
    x = y = None
    if not bufs.kept:
        del bufs.t["hd"]
    return delta


def art_forward(geo, P, bias, xyz, venc, S, bufs, noise=None):
    """The articulated NeRFMLP.forward (model_autodecoder.py:168-239) layer by layer on aon_gemm,
    on sample positions xyz (R, 3) and view encodings venc (R / S, nv): P the (weight, bias)
    pairs in art_layers order, ``bias(i)`` the folded bias of a layer that reads a latent code,
    ``bufs`` (LayerBuffers) the outputs' buffers -> (enc = pos_enc(x'), raw)."""
    R, dev = xyz.shape[0], xyz.device
    nw, wc, ne, nv = geo.nw, geo.wc, geo.ne, geo.nv
    delta = art_deformation(geo, P, bias, xyz, bufs)
    # x' = delta + xyz -> pos_enc (enc_after, :205-212); enc[:, :3] is x' itself
    enc = torch.empty((R, ne), device=dev)
    L.call("aon_cast_rays", L.ptr(xyz), None, None, R, 1, L.ptr(delta), 3, None, geo.min_deg,
           geo.max_deg, L.ptr(enc), L.stream(dev))
    # trunk on cat[enc, shape] with the skip concat cat[h, enc, shape] (:214-220)
    x = bufs.out("h", 0)
    linear_fwd(x, enc, ne, P[geo.PTS0][0], bias(geo.PTS0), relu=True)
    for i in range(1, geo.depth):
        y = bufs.out("h", i)
        if i == geo.skip:
            linear_fwd(y, x, nw, P[geo.PTS0 + i][0], bias(geo.PTS0 + i), relu=True, X2=enc, K2=ne,
                       ld2=ne)
        else:
            linear_fwd(y, x, nw, *P[geo.PTS0 + i], relu=True)
        x = y
    raw = bufs.raw if bufs.kept else torch.empty((R, 4), device=dev)
    if noise is not None:  # raw_sigma + noise (:318-319), added in the GEMM epilogue
        raw[:, 3].copy_(noise)
    linear_fwd(raw[:, 3:], x, nw, *P[geo.DENS], ldo=4, accumulate=noise is not None)
    bot = bufs.out("bot")
    linear_fwd(bot, x, nw, *P[geo.BOT])  # bottleneck, no activation (:225)
    # view branch on cat[bottleneck, enc_dir tiled over samples, appearance] (:226-235)
    x = bufs.out("hv", 0)
    linear_fwd(x, bot, nw, P[geo.VIEW0][0], bias(geo.VIEW0), relu=True, X2=venc, K2=nv, ld2=nv,
               rdiv2=S)
    for i in range(1, geo.nc):
        y = bufs.out("hv", i)
        linear_fwd(y, x, wc, *P[geo.VIEW0 + i], relu=True)
        x = y
    linear_fwd(raw, x, wc, *P[geo.RGB], ldo=4)  # rgb_layer (:237)
    return enc, raw
