"""Drop-in for the articulated ``NeRFMLP`` / ``NeRF_AE_Art`` of the reference
(models/vanilla_nerf/model_autodecoder.py:60-337; config C3).

Identical constructor keywords, forward signatures and parameter (state_dict) names.  One
inference level runs ONE fused kernel (aon_mlp_art_fwd, k_mlp_art_f16x3; NeRFMLP.fused, the
default):

    cast_rays                                                              helper.py:25-26
    deformation MLP on cat[xyz, shape, articulation]: 4 x (MFMA + ReLU),   model_autodecoder.py:
      deformation_layer                                                    196-205
    x' = deformation + xyz, pos_enc(x') in registers                       :205-212
    trunk on cat[pos_enc(x'), shape] with the skip concat, density,        :214-223
      bottleneck
    view branch on cat[bottleneck, enc_dir, appearance]: 4 x (MFMA + ReLU) :224-235
    rgb head; padded sigmoid / softplus(raw - 1) in the epilogue           :321-323

then the coarse compositor fused with the fine level's resampling (aon_composite_march) or, for
the fine level, aon_composite_fwd (AON_ACT_ARTIC; :324-333).  The latent codes are the same for
every sample (the reference repeats (1, C) rows over all B*S rows, :186-194), so their products
with the weight columns they meet are folded into per-call biases (b' = b + W[:, latent cols] .
latent, one tiny GEMM each).  ``NeRFMLP.fused = False`` selects the layer-by-layer path
(level.art_forward, the walker the training path shares), every product on the f16x3 MFMA GEMM
(aon_gemm): also the fallback when an activation leaves the fused kernel's fp16x3 range.
"""
import warnings
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.init as init

from . import _lib as L
from . import helper
from . import level as _level
from . import two_level
from .numerics import resolve as _resolve_numerics

# what a render (two_level.render) and a deformation pass say when they leave the fused path
RANGE_WARNING = ("NeRF_AE_Art: an MLP activation exceeded the fused fp16x3 range; "
                 "re-rendered on the layer-by-layer path")


class NeRFMLP(nn.Module):
    """reference model_autodecoder.py:60-166 (same nn.Linear layout and init)."""

    def __init__(self, min_deg_point, max_deg_point, deg_view, netdepth: int = 8,
                 netwidth: int = 256, netdepth_deformation=4, netwidth_deformation: int = 128,
                 netdepth_condition: int = 4, netwidth_condition: int = 128,
                 shape_latent_dim=128, appearance_latent_dim=128, articulation_latent_dim=32,
                 skip_layer: int = 4, input_ch: int = 3, input_ch_view: int = 3,
                 num_rgb_channels: int = 3, num_density_channels: int = 1,
                 deformation_mlp: bool = True, enc_after: bool = True, embed_deg: bool = False,
                 fused: bool = True):
        super().__init__()
        self.fused = fused  # one fused kernel per level (aon_mlp_art_fwd) vs GEMM per layer
        cfg = dict(netdepth=netdepth, netwidth=netwidth, netdepth_deformation=netdepth_deformation,
                   netwidth_deformation=netwidth_deformation, netdepth_condition=netdepth_condition,
                   netwidth_condition=netwidth_condition, shape_latent_dim=shape_latent_dim,
                   appearance_latent_dim=appearance_latent_dim,
                   articulation_latent_dim=articulation_latent_dim, skip_layer=skip_layer,
                   input_ch=input_ch, input_ch_view=input_ch_view,
                   num_rgb_channels=num_rgb_channels, num_density_channels=num_density_channels,
                   deformation_mlp=deformation_mlp, enc_after=enc_after, embed_deg=embed_deg)
        for k, v in cfg.items():
            setattr(self, k, v)
        self.min_deg_point, self.max_deg_point, self.deg_view = min_deg_point, max_deg_point, deg_view
        if not (deformation_mlp and enc_after and not embed_deg):
            raise ValueError("aonerf implements the reference's default articulated MLP "
                             "(deformation_mlp=True, enc_after=True, embed_deg=False)")
        view_pos_size = (deg_view * 2 + 1) * input_ch_view
        pos_size_deformation = input_ch + shape_latent_dim + articulation_latent_dim
        deformations = [nn.Linear(pos_size_deformation, netwidth_deformation)]
        for _ in range(netdepth_deformation - 1):
            deformations.append(nn.Linear(netwidth_deformation, netwidth_deformation))
        for m in deformations:
            init.xavier_uniform_(m.weight)
        self.deformations_linear = nn.ModuleList(deformations)
        self.deformation_layer = nn.Linear(netwidth_deformation, 3)
        init.xavier_uniform_(self.deformation_layer.weight)
        pos_size = ((max_deg_point - min_deg_point) * 2 + 1) * input_ch + shape_latent_dim
        pts = [nn.Linear(pos_size, netwidth)]
        for idx in range(netdepth - 1):
            k = netwidth + pos_size if (idx % skip_layer == 0 and idx > 0) else netwidth
            pts.append(nn.Linear(k, netwidth))
        for m in pts:
            init.xavier_uniform_(m.weight)
        self.pts_linears = nn.ModuleList(pts)
        views = [nn.Linear(netwidth + view_pos_size + appearance_latent_dim, netwidth_condition)]
        for _ in range(netdepth_condition - 1):
            layer = nn.Linear(netwidth_condition, netwidth_condition)
            init.xavier_uniform_(layer.weight)
            views.append(layer)
        self.views_linear = nn.ModuleList(views)
        self.bottleneck_layer = nn.Linear(netwidth, netwidth)
        self.density_layer = nn.Linear(netwidth, num_density_channels)
        self.rgb_layer = nn.Linear(netwidth_condition, num_rgb_channels)
        for m in (self.bottleneck_layer, self.density_layer, self.rgb_layer):
            init.xavier_uniform_(m.weight)
        self.pos_size_enc = pos_size - shape_latent_dim  # 63

    # -- latent folding: b' = b + W[:, c0:c0+n] . latent (_level.fold)
    def _pairs(self):
        """(weight, bias) in the kernels' layer order (contiguous copies, if any, live here)."""
        return [(L.contig(m.weight.detach()), L.contig(m.bias.detach()))
                for m in _level.art_layers(self)]

    def _folded(self, P, latents):
        shape = L.contig(latents["density"].detach().reshape(1, -1))
        app = L.contig(latents["color"].detach().reshape(1, -1))
        art = L.contig(latents["articulation"].detach().reshape(1, -1))
        L.require_gpu(shape, app, art)
        if shape.shape[1] != self.shape_latent_dim or art.shape[1] != self.articulation_latent_dim:
            raise ValueError("latent code sizes do not match the MLP")
        # lat_def: the 160 latent columns of cat[pos, shape, art], held over the four folds
        return _level.folded_biases(_level.geo_of(self), P, (shape, app, art),
                                   lat_def=torch.cat([shape, art], -1))

    def folded_biases(self, latents):
        geo = _level.geo_of(self)
        fb = self._folded(self._pairs(), latents)
        return {"def0": fb[geo.DEF0], "pts0": fb[geo.PTS0], "pts_skip": fb[geo.PTS0 + geo.skip],
                "view0": fb[geo.VIEW0]}

    @torch.no_grad()
    def packed_weights(self, latents):
        """The fused kernel's fp16x3 weight stream with this call's folded biases
        (aon_mlp_art_pack; re-packed per call: the folded biases follow the latent codes)."""
        P = self._pairs()
        # the folded biases live in `pairs` until the pack is enqueued (the struct holds plain
        # pointers); shape-checked (ValueError) before the pack
        pairs = _level.folded_pairs(P, self._folded(P, latents))
        prm = L.mlp_art_params(pairs)
        dev = self.rgb_layer.weight.device
        nbytes = L.lib().aon_mlp_art_packed_bytes()
        buf = getattr(self, "_art_packed", None)
        if buf is None or buf.device != dev:
            buf = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
            self._art_packed = buf
        L.call("aon_mlp_art_pack", L.ctypes.byref(prm), L.ptr(buf), L.stream(dev))
        return buf

    def _fused_ok(self):
        # the fused kernel is compiled for the default geometry (_level.Geo.fused_ok)
        return self.fused and _level.geo_of(self).fused_ok

    @torch.no_grad()
    def forward_rays(self, rays_o, rays_d, viewdirs, t_vals, latents, act=L.ACT_NONE):
        """One level's MLP on samples o + t d -> raw (B*S, 4) = [raw_rgb, raw_sigma]: one fused
        kernel (aon_mlp_art_fwd: cast_rays, deformation, both pos_encs, trunk, view branch;
        ``act=L.ACT_ARTIC`` also applies model_autodecoder.py:321-323), or the layer-by-layer
        GEMM path when ``fused`` is off."""
        L.require_gpu(rays_o, rays_d, viewdirs, t_vals)
        B, S = t_vals.shape
        if self._fused_ok():
            raw = torch.empty((B * S, 4), device=t_vals.device)
            L.call("aon_mlp_art_fwd", L.ptr(self.packed_weights(latents)), L.ptr(L.contig(rays_o)),
                   L.ptr(L.contig(rays_d)), L.ptr(L.contig(viewdirs)), L.ptr(L.contig(t_vals)), B,
                   S, act, L.ptr(raw), L.stream(t_vals.device))
            return raw
        if act != L.ACT_NONE:
            raise ValueError("the layer-by-layer path returns raw outputs only")
        R, dev = B * S, t_vals.device
        xyz = torch.empty((R, 3), device=dev)
        L.call("aon_cast_rays", L.ptr(rays_o), L.ptr(rays_d), L.ptr(t_vals), B, S, None, 0,
               L.ptr(xyz), 0, 0, None, L.stream(dev))
        venc = torch.empty((B, (self.deg_view * 2 + 1) * self.input_ch_view), device=dev)
        L.call("aon_pos_enc", L.ptr(viewdirs), B, 0, self.deg_view, L.ptr(venc), L.stream(dev))
        return self._mlp(xyz, venc, S, latents)

    @torch.no_grad()
    def _mlp(self, xyz, venc, S, latents):
        """The MLP on sample positions xyz (R, 3), view encodings venc (R / S, 27) -> (R, 4):
        _level.art_forward on two alternating buffers per width."""
        geo = _level.geo_of(self)
        P = self._pairs()
        fb = self._folded(P, latents)
        bufs = _level.LayerBuffers(geo, xyz.shape[0], xyz.device)
        return _level.art_forward(geo, P, fb.__getitem__, xyz, venc, S, bufs)[1]

    # -- the density alone (:196-223): no bottleneck, view branch or rgb head
    def _sigma_layerwise(self, xyz, latents):
        """(R, 4) = [0, 0, 0, raw sigma] of the layer-by-layer path: column 3 of _mlp (the
        density head reads the trunk alone, so any view encoding gives these bits)."""
        R = xyz.shape[0]
        venc = torch.zeros((1, (self.deg_view * 2 + 1) * self.input_ch_view), device=xyz.device)
        raw = self._mlp(xyz, venc, max(R, 1), latents)
        raw[:, :3] = 0.0
        return raw

    @torch.no_grad()
    def forward_sigma(self, rays_o, rays_d, t_vals, latents, act=L.ACT_NONE):
        """The density-only pass on samples o + t d (aon_mlp_art_fwd_sigma): (B*S, 4) =
        [0, 0, 0, sigma], column 3 as forward_rays returns it bit for bit; no bottleneck, view
        branch, rgb head or view encoding runs.  With ``fused`` off: column 3 of the
        layer-by-layer forward_rays (raw only), zeros in columns 0..2."""
        L.require_gpu(rays_o, rays_d, t_vals)
        B, S = t_vals.shape
        dev = t_vals.device
        if self._fused_ok():
            raw = torch.empty((B * S, 4), device=dev)
            L.call("aon_mlp_art_fwd_sigma", L.ptr(self.packed_weights(latents)),
                   L.ptr(L.contig(rays_o)), L.ptr(L.contig(rays_d)), L.ptr(L.contig(t_vals)), B, S,
                   act, L.ptr(raw), L.stream(dev))
            return raw
        if act != L.ACT_NONE:
            raise ValueError("the layer-by-layer path returns raw outputs only")
        xyz = torch.empty((B * S, 3), device=dev)
        L.call("aon_cast_rays", L.ptr(L.contig(rays_o)), L.ptr(L.contig(rays_d)),
               L.ptr(L.contig(t_vals)), B, S, None, 0, L.ptr(xyz), 0, 0, None, L.stream(dev))
        return self._sigma_layerwise(xyz, latents)

    @torch.no_grad()
    def density(self, pos, latents, activated=True):
        """The density field at points pos (..., 3) under these latent codes -> (...):
        softplus(raw - 1) (``activated``, model_autodecoder.py:323: what the compositor reads) or
        the raw density_layer output.  One density-only launch (aon_mlp_art_fwd_sigma_points), or
        layer by layer on aon_gemm when ``fused`` is off -- or when the pass raised the pack's
        range flag (one sync, skipped under stream capture; RANGE_WARNING).  No backward."""
        if pos.shape[-1] != 3:
            raise ValueError("density expects (..., 3) points")
        L.require_gpu(pos)
        lead = tuple(pos.shape[:-1])
        pos = L.contig(pos.reshape(-1, 3))
        N, dev = pos.shape[0], pos.device
        if self._fused_ok():
            buf = self.packed_weights(latents)
            raw = torch.empty((N, 4), device=dev)
            L.call("aon_mlp_art_fwd_sigma_points", L.ptr(buf), L.ptr(pos), N,
                   L.ACT_ARTIC if activated else L.ACT_NONE, L.ptr(raw), L.stream(dev))
            if torch.cuda.is_current_stream_capturing() or not L.range_overflow([buf]):
                return raw[:, 3].view(lead)
            warnings.warn(RANGE_WARNING, RuntimeWarning)
        sigma = self._sigma_layerwise(pos, latents)[:, 3]
        if activated:
            sigma = torch.nn.functional.softplus(sigma - 1.0)
        return sigma.view(lead)

    # -- the deformation MLP alone (:196-205): x' = x + delta(x, shape, articulation)
    @torch.no_grad()
    def _deform_rows(self, latents, *, rays=None, pos=None, packed=None, range_check=True):
        """(xp4 (N, 4) = [x', 0], d4 (N, 4) = [delta, ||delta||]) of the samples o + t d of
        ``rays`` = (rays_o, rays_d, t_vals (B, S)) or of the points ``pos`` (N, 3): the fused
        deformation pass (aon_mlp_art_fwd_deform[_points]) on ``packed`` (this MLP's stream
        already packed with these latents; None: pack it), or layer by layer on aon_gemm
        (_level.art_deformation) when ``fused`` is off -- or, with ``range_check`` (one sync, not
        under stream capture), when the pass raised the pack's range flag."""
        if rays is not None:
            o, d, t = (L.contig(x) for x in rays)
            L.require_gpu(o, d, t)
            B, S = t.shape
            N, dev = B * S, t.device
        else:
            L.require_gpu(pos)
            pos = L.contig(pos)
            N, dev = pos.shape[0], pos.device
        if self._fused_ok():
            buf = self.packed_weights(latents) if packed is None else packed
            xp4, d4 = torch.empty((N, 4), device=dev), torch.empty((N, 4), device=dev)
            if rays is not None:
                L.call("aon_mlp_art_fwd_deform", L.ptr(buf), L.ptr(o), L.ptr(d), L.ptr(t), B, S,
                       L.ptr(xp4), L.ptr(d4), L.stream(dev))
            else:
                L.call("aon_mlp_art_fwd_deform_points", L.ptr(buf), L.ptr(pos), N, L.ptr(xp4),
                       L.ptr(d4), L.stream(dev))
            if not (range_check and not torch.cuda.is_current_stream_capturing()
                    and L.range_overflow([buf])):
                return xp4, d4
            warnings.warn(RANGE_WARNING, RuntimeWarning)
        if rays is not None:
            xyz = torch.empty((N, 3), device=dev)
            L.call("aon_cast_rays", L.ptr(o), L.ptr(d), L.ptr(t), B, S, None, 0, L.ptr(xyz), 0, 0,
                   None, L.stream(dev))
        else:
            xyz = pos
        geo = _level.geo_of(self)
        P = self._pairs()
        fb = self._folded(P, latents)
        delta = _level.art_deformation(geo, P, fb.__getitem__, xyz,
                                       _level.LayerBuffers(geo, N, dev))
        xp4, d4 = torch.zeros((N, 4), device=dev), torch.empty((N, 4), device=dev)
        torch.add(delta, xyz, out=xp4[:, :3])
        d4[:, :3] = delta
        d4[:, 3] = (delta * delta).sum(-1).sqrt()
        return xp4, d4

    def deform_rays(self, rays_o, rays_d, t_vals, latents):
        """The deformation field on the samples o + t d of one level: (xp (B, S, 3) the canonical
        coordinate x' = x + delta the trunk encodes, delta (B, S, 3), mag (B, S) = ||delta||),
        through the fused deformation pass (aon_mlp_art_fwd_deform); x' is the x' of
        forward_rays' fused kernel bit for bit.  No backward."""
        B, S = t_vals.shape
        xp4, d4 = self._deform_rows(latents, rays=(rays_o, rays_d, t_vals))
        return xp4[:, :3].view(B, S, 3), d4[:, :3].view(B, S, 3), d4[:, 3].view(B, S)

    def deform(self, pos, latents):
        """The same on given sample points pos (..., 3) -> (xp (..., 3), delta (..., 3), mag (...))."""
        if pos.shape[-1] != 3:
            raise ValueError("deform expects (..., 3) points")
        lead = tuple(pos.shape[:-1])
        xp4, d4 = self._deform_rows(latents, pos=pos.reshape(-1, 3))
        return xp4[:, :3].view(lead + (3,)), d4[:, :3].view(lead + (3,)), d4[:, 3].view(lead)

    def forward(self, pos, condition, latents):
        """reference model_autodecoder.py:168-239: pos (B, S, 3) sample positions (enc_after),
        condition (B, 27) encoded view directions -> (raw_rgb (B, S, 3), raw_density (B, S, 1))."""
        L.require_gpu(pos, condition)
        B, S, _ = pos.shape
        if self._fused_ok():
            raw = torch.empty((B * S, 4), device=pos.device)
            L.call("aon_mlp_art_fwd_points", L.ptr(self.packed_weights(latents)),
                   L.ptr(L.contig(pos.reshape(-1, 3))), L.ptr(L.contig(condition)), B, S,
                   L.ACT_NONE, L.ptr(raw), L.stream(pos.device))
            raw = raw.view(B, S, 4)
            return raw[..., :3], raw[..., 3:]
        raw = self._mlp(L.contig(pos.reshape(-1, 3)), L.contig(condition), S, latents).view(B, S, 4)
        return raw[..., :3], raw[..., 3:]


class NeRF_AE_Art(nn.Module):  # noqa: N801 (reference name)
    """reference model_autodecoder.py:242-337 (two-level render with latent codes)."""

    def __init__(self, num_levels: int = 2, min_deg_point: int = 0, max_deg_point: int = 10,
                 deg_view: int = 4, num_coarse_samples: int = 64, num_fine_samples: int = 128,
                 use_viewdirs: bool = True, noise_std: float = 0.0, lindisp: bool = False,
                 rgb_padding: float = 0.001, density_bias: float = -1.0, enc_after=True,
                 embed_deg=False, train_precision: str = "f16x3", train_numerics=None,
                 fused_march: bool = True, range_check: bool = True):
        """The reference's kwargs (model_autodecoder.py:243-276) plus the per-model settings of
        aonerf.model.NeRF: ``train_precision`` / ``train_numerics`` (aonerf/numerics.py),
        ``fused_march`` and ``range_check``."""
        super().__init__()
        self.train_numerics = _resolve_numerics(train_precision, train_numerics)
        self.fused_march, self.range_check = bool(fused_march), bool(range_check)
        if num_levels != 2:
            raise ValueError("the reference NeRF_AE_Art is two-level (coarse + fine)")
        if rgb_padding != 0.001 or density_bias != -1.0:
            raise ValueError("the fused epilogue implements rgb_padding=0.001, density_bias=-1")
        self.num_levels, self.min_deg_point, self.max_deg_point = num_levels, min_deg_point, max_deg_point
        self.deg_view, self.num_coarse_samples, self.num_fine_samples = deg_view, num_coarse_samples, num_fine_samples
        self.use_viewdirs, self.noise_std, self.lindisp = use_viewdirs, noise_std, lindisp
        self.rgb_padding, self.density_bias = rgb_padding, density_bias
        self.enc_after, self.embed_deg = enc_after, embed_deg
        self.coarse_mlp = NeRFMLP(min_deg_point, max_deg_point, deg_view, enc_after=enc_after,
                                  embed_deg=embed_deg)
        self.fine_mlp = NeRFMLP(min_deg_point, max_deg_point, deg_view, enc_after=enc_after,
                                embed_deg=embed_deg)

    def forward(self, rays, randomized, white_bkgd, near, far, latents, train=True, *,
                u_coarse=None, u_fine=None, return_weights=False, return_intermediates=False,
                timers=None, latent_only=False, maps=False, fine_only=False):
        """reference model_autodecoder.py:278-337 -> [(comp_rgb, acc, depth)_coarse, (...)_fine]
        (``u_coarse`` / ``u_fine`` inject randomized-mode uniforms; the extras as NeRF.forward;
        ``timers`` (dict) records hip events around each level's MLP / composite launches).

        With autograd enabled and trainable parameters or latent codes, each level runs the
        training path (train_art.ArtRenderLevel: the fused training forward
        aon_mlp_art_fwd_train, which also stores the activations, then the HIP backward into the
        MLP parameters and the latent codes); otherwise the fused inference kernel (two_level.py
        drives the two levels either way).  ``latent_only`` (the training path only): gradients
        for the latent codes alone, the MLPs frozen (train_art.render_level; latent_fit.py).

        ``maps`` (inference only; ValueError on the training path, there is no backward): the
        fine level's tuple ends with a dict of the deformation field composited with the fine
        weights (helper.py:191-193's nocs hook) -- ``canonical`` (B, 3) = sum w x',
        ``motion`` (B, 3) = sum w delta, ``motion_mag`` (B,) = sum w ||delta|| -- from one
        deformation pass over the fine samples (aon_mlp_art_fwd_deform) and two
        aon_composite_feat launches; every other output is unchanged.

        ``fine_only`` (inference path, without ``return_weights`` / ``return_intermediates``; as
        NeRF.forward, and what aonerf.render asks for): the caller keeps only the fine level, so
        the first element is None and, with both MLPs on the fused path, the coarse MLP runs the
        density-only kernel (aon_mlp_art_fwd_sigma): no bottleneck, view branch or rgb head for
        colours that reach nothing.  The fine level is the same, bit for bit -- the coarse level
        reaches it through its weights alone, which read sigma and t.  An activation out of the
        fp16x3 range in the coarse VIEW branch alone is then no longer reported (nothing kept
        read it); the fine level still reports its own."""
        o, d, v = rays["rays_o"], rays["rays_d"], rays["viewdirs"]
        L.require_gpu(o, d, v)
        o, d, v = L.contig(o), L.contig(d), L.contig(v)
        training = torch.is_grad_enabled() and (
            any(p.requires_grad for p in self.parameters())
            or any(x.requires_grad for x in latents.values()))
        if maps and training:
            raise ValueError("maps=True has no backward: call under torch.no_grad() or with "
                             "frozen parameters and latent codes")
        run = two_level.train if training else two_level.render
        kw = dict(maps=True) if maps else {}
        fine_only = bool(fine_only) and not (training or return_weights or return_intermediates)
        if fine_only:
            kw["fine_only"] = True
        return run(self._spec(latents, latent_only, fine_only), o, d, v, randomized, white_bkgd,
                   near, far, u_coarse=u_coarse, u_fine=u_fine, return_weights=return_weights,
                   return_intermediates=return_intermediates, timers=timers, **kw)

    def _spec(self, latents, latent_only=False, fine_only=False):
        mlps = (self.coarse_mlp, self.fine_mlp)

        def mlp_raw(level, mlp, o, d, v, t_vals, act):
            # fine_only: the coarse colour reaches nothing -- density only, while both MLPs are on
            # the fused path (inside the range fallback: the layer-by-layer forward, as before)
            if fine_only and level == 0 and all(m._fused_ok() for m in mlps):
                return mlp.forward_sigma(o, d, t_vals, latents, act=act)
            return mlp.forward_rays(o, d, v, t_vals, latents, act=act)

        def train_level(level, mlp, o, d, v, t_vals, white_bkgd, noise, timers):
            from .train_art import render_level
            return render_level(mlp, o, d, v, t_vals, white_bkgd, latents, noise,
                                self.train_numerics, timers, latent_only)

        def level_maps(mlp, o, d, t_vals, weights, timers):
            # the level's MLP has just packed mlp._art_packed with these latents: the pass reads
            # its prefix in place (a re-pack would clear the status word the render checks)
            ev = _level.events(timers)
            xp4, d4 = mlp._deform_rows(
                latents, rays=(o, d, t_vals), range_check=False,
                packed=getattr(mlp, "_art_packed", None) if mlp._fused_ok() else None)
            _level.record(timers, ev, "deform1", t_vals.numel())
            ev = _level.events(timers)
            motion = helper.composite_features(weights, d4)
            canonical = helper.composite_features(weights, xp4[:, :3])
            _level.record(timers, ev, "maps1", t_vals.numel())
            return {"canonical": canonical, "motion": motion[:, :3], "motion_mag": motion[:, 3]}

        return SimpleNamespace(
            model=self, train_level=train_level, maps=level_maps,
            mlp_raw=mlp_raw,
            # model_autodecoder.py:321-323 always in the compositor (AON_ACT_ARTIC)
            acts=lambda noisy: (L.ACT_NONE, L.ACT_ARTIC),
            keep_fine_weights=True, extras_key="raw",
            range_checked=lambda: self.range_check and all(m._fused_ok() for m in mlps),
            packs=lambda: [getattr(m, "_art_packed", None) for m in mlps],
            # (the layer-by-layer path's aon_gemm operands carry 2^-8: range 1.6e7, not 8188)
            fallback=lambda: two_level.switched(mlps, "fused", False),
            warning=RANGE_WARNING)
