"""Drop-in for ``NeRFMLP`` / ``NeRF`` of the reference (models/vanilla_nerf/model.py:39-199).

Identical constructor keywords, forward signatures, return tuples and parameter (state_dict)
names, so a reference Lightning checkpoint (``model.coarse_mlp.pts_linears.0.weight`` ...)
loads unchanged.  The forward pass runs on the fused HIP kernels:

    level 0: aon_sample_along_rays (t only) -> aon_mlp_fwd (xyz + pos_enc + MLP + sigmoid/relu
             fused) -> aon_composite_march (alpha compositing fused with the fine level's
             sample_pdf: the coarse weights stay on chip; NeRF.fused_march / march_ok)
    level 1: aon_mlp_fwd on the merged t -> aon_composite_fwd
    (fused_march False, or N_importance > 256: aon_composite_fwd + aon_sample_pdf, bit-identical)
    fine_only (what aonerf.render asks for), f16x3: level 0's MLP is the density-only pass
    aon_mlp_fwd_sigma, level 1's reads per-ray view encodings (aon_pos_enc once per forward,
    aon_mlp_fwd_cond) -- the fine level's outputs are the same bits

Per-model configuration only (no mutable globals): the render precision
(``precision``), the training numerics (``train_precision`` / ``train_numerics``,
aonerf/numerics.py), ``fused_march`` and ``range_check`` are attributes of each NeRF.

Intermediates live in HBM (a 640x480 frame needs ~1.6 GB), so a whole frame is one launch
per stage instead of the reference's 80 chunk iterations.
"""
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.init as init

from . import _lib as L
from . import helper, two_level
from .two_level import composite_march, fine_uniforms, level_t_vals, march_ok  # noqa: F401 (re-exported)
from .numerics import resolve as _resolve_numerics

_DEFAULT_GEOMETRY = dict(min_deg_point=0, max_deg_point=10, deg_view=4, netdepth=8, netwidth=256,
                         netdepth_condition=1, netwidth_condition=128, skip_layer=4, input_ch=3,
                         input_ch_view=3, num_rgb_channels=3, num_density_channels=1)


class NeRFMLP(nn.Module):
    """reference model.py:39-120 (same nn.Linear layout and init)."""

    def __init__(self, min_deg_point, max_deg_point, deg_view, netdepth: int = 8,
                 netwidth: int = 256, netdepth_condition: int = 1, netwidth_condition: int = 128,
                 skip_layer: int = 4, input_ch: int = 3, input_ch_view: int = 3,
                 num_rgb_channels: int = 3, num_density_channels: int = 1,
                 precision: str = "f16x3"):
        super().__init__()
        self.min_deg_point, self.max_deg_point, self.deg_view = min_deg_point, max_deg_point, deg_view
        self.netdepth, self.netwidth, self.skip_layer = netdepth, netwidth, skip_layer
        self.netdepth_condition, self.netwidth_condition = netdepth_condition, netwidth_condition
        self.input_ch, self.input_ch_view = input_ch, input_ch_view
        self.num_rgb_channels, self.num_density_channels = num_rgb_channels, num_density_channels
        geometry = dict(min_deg_point=min_deg_point, max_deg_point=max_deg_point, deg_view=deg_view,
                        netdepth=netdepth, netwidth=netwidth, netdepth_condition=netdepth_condition,
                        netwidth_condition=netwidth_condition, skip_layer=skip_layer,
                        input_ch=input_ch, input_ch_view=input_ch_view,
                        num_rgb_channels=num_rgb_channels, num_density_channels=num_density_channels)
        if geometry != _DEFAULT_GEOMETRY:
            raise ValueError("aonerf's fused MLP kernel implements the reference's default NeRFMLP "
                             f"geometry {_DEFAULT_GEOMETRY}; got {geometry}")
        if precision not in L.PREC:
            raise ValueError(f"precision must be one of {sorted(L.PREC)}")
        self.precision = precision

        pos_size = ((max_deg_point - min_deg_point) * 2 + 1) * input_ch
        view_pos_size = (deg_view * 2 + 1) * input_ch_view
        init_layer = nn.Linear(pos_size, netwidth)
        init.xavier_uniform_(init_layer.weight)
        pts = [init_layer]
        for idx in range(netdepth - 1):
            k = netwidth + pos_size if (idx % skip_layer == 0 and idx > 0) else netwidth
            layer = nn.Linear(k, netwidth)
            init.xavier_uniform_(layer.weight)
            pts.append(layer)
        self.pts_linears = nn.ModuleList(pts)
        views = [nn.Linear(netwidth + view_pos_size, netwidth_condition)]  # default init (model.py:79)
        for idx in range(netdepth_condition - 1):
            layer = nn.Linear(netwidth_condition, netwidth_condition)
            init.xavier_uniform_(layer.weight)
            views.append(layer)
        self.views_linear = nn.ModuleList(views)
        self.bottleneck_layer = nn.Linear(netwidth, netwidth)
        self.density_layer = nn.Linear(netwidth, num_density_channels)
        self.rgb_layer = nn.Linear(netwidth_condition, num_rgb_channels)
        for m in (self.bottleneck_layer, self.density_layer, self.rgb_layer):
            init.xavier_uniform_(m.weight)
        self._packed = None
        self._packed_key = None

    # -- weight packing (cached; repacked whenever a parameter is replaced or updated in place)
    def _layers(self):
        return list(self.pts_linears) + [self.density_layer, self.bottleneck_layer,
                                         self.views_linear[0], self.rgb_layer]

    def packed_weights(self):
        params = [p for m in self._layers() for p in (m.weight, m.bias)]
        L.require_gpu(*params)
        key = (self.precision,) + tuple((p.data_ptr(), p._version) for p in params)
        if key != self._packed_key:
            params = [L.contig(p.detach()) for p in params]
            prm = L.mlp_params(zip(params[0::2], params[1::2]))  # shape-checked (ValueError)
            prec = L.PREC[self.precision]
            nbytes = L.lib().aon_mlp_packed_bytes(prec)
            if nbytes == 0:
                raise NotImplementedError(f"precision {self.precision!r} is not built yet")
            buf = torch.empty(nbytes // 4, dtype=torch.float32, device=params[0].device)
            L.call("aon_mlp_pack", L.ctypes.byref(prm), prec, L.ptr(buf), L.stream(buf.device))
            self._packed, self._packed_key = buf, key
        return self._packed

    def forward_rays(self, rays_o, rays_d, viewdirs, t_vals, act=L.ACT_NONE, cond=None):
        """Fused cast_rays + pos_enc + forward: (B*S, 4) = [raw_rgb, raw_sigma]; with
        ``act=L.ACT_VANILLA`` the rgb/sigma activations of model.py:186-187 are applied too.
        ``cond`` (B, 27) = pos_enc(viewdirs, 0, deg_view), f16x3 only: the view encodings are read
        from it (aon_mlp_fwd_cond) instead of recomputed per sample -- the same bits."""
        L.require_gpu(rays_o, rays_d, viewdirs, t_vals, cond)
        B, S = t_vals.shape
        raw = torch.empty((B * S, 4), device=t_vals.device)
        if cond is not None:
            if tuple(cond.shape) != (B, 27):
                raise ValueError("forward_rays expects cond (B, 27)")
            L.call("aon_mlp_fwd_cond", L.ptr(self.packed_weights()), L.PREC[self.precision],
                   L.ptr(L.contig(rays_o)), L.ptr(L.contig(rays_d)), L.ptr(L.contig(cond)),
                   L.ptr(L.contig(t_vals)), B, S, act, L.ptr(raw), L.stream(t_vals.device))
            return raw
        L.call("aon_mlp_fwd", L.ptr(self.packed_weights()), L.PREC[self.precision],
               L.ptr(L.contig(rays_o)), L.ptr(L.contig(rays_d)), L.ptr(L.contig(viewdirs)),
               L.ptr(L.contig(t_vals)), B, S, act, L.ptr(raw), L.stream(t_vals.device))
        return raw

    def forward_sigma(self, rays_o, rays_d, t_vals, act=L.ACT_NONE):
        """The density-only pass (aon_mlp_fwd_sigma, f16x3 only): (B*S, 4) = [0, 0, 0, sigma],
        column 3 as forward_rays returns it; no view layer, rgb head or view encoding runs."""
        L.require_gpu(rays_o, rays_d, t_vals)
        B, S = t_vals.shape
        raw = torch.empty((B * S, 4), device=t_vals.device)
        L.call("aon_mlp_fwd_sigma", L.ptr(self.packed_weights()), L.PREC[self.precision],
               L.ptr(L.contig(rays_o)), L.ptr(L.contig(rays_d)), L.ptr(L.contig(t_vals)), B, S, act,
               L.ptr(raw), L.stream(t_vals.device))
        return raw

    @torch.no_grad()
    def density(self, pos, activated=True):
        """The density field at points pos (..., 3) -> (...): relu(raw) (``activated``,
        model.py:187: AON_ACT_VANILLA's sigma) or the raw density_layer output.  One density-only
        launch (aon_mlp_fwd_sigma with rays_o = pos, rays_d = 0, t = 0, S = 1), so f16x3 only: a
        fp32 model has no such kernel (aon_mlp_fwd's column 3 is its density).  The range guard
        reports through the pack's status word, as forward_sigma's.  No backward."""
        if pos.shape[-1] != 3:
            raise ValueError("density expects (..., 3) points")
        if self.precision != "f16x3":
            raise ValueError("density runs the f16x3 density-only kernel; with precision='fp32' "
                             "take column 3 of forward_rays (aon_mlp_fwd)")
        lead = tuple(pos.shape[:-1])
        pos = L.contig(pos.reshape(-1, 3))
        N = pos.shape[0]
        raw = self.forward_sigma(pos, torch.zeros_like(pos), torch.zeros((N, 1), device=pos.device),
                                 act=L.ACT_VANILLA if activated else L.ACT_NONE)
        return raw[:, 3].view(lead)

    def forward(self, x, condition):
        """reference model.py:95-120: x (B, S, 63) encoded points, condition (B, 27)."""
        L.require_gpu(x, condition)
        B, S, C = x.shape
        if C != 63 or tuple(condition.shape) != (B, 27):
            raise ValueError("NeRFMLP.forward expects x (B, S, 63) and condition (B, 27)")
        raw = torch.empty((B * S, 4), device=x.device)
        L.call("aon_mlp_fwd_encoded", L.ptr(self.packed_weights()), L.PREC[self.precision],
               L.ptr(L.contig(x)), L.ptr(L.contig(condition)), B, S, L.ACT_NONE, L.ptr(raw),
               L.stream(x.device))
        raw = raw.view(B, S, 4)
        return raw[..., :3], raw[..., 3:]


class NeRF(nn.Module):
    """reference model.py:123-199 (two-level coarse/fine render)."""

    def __init__(self, num_levels: int = 2, min_deg_point: int = 0, max_deg_point: int = 10,
                 deg_view: int = 4, num_coarse_samples: int = 64, num_fine_samples: int = 128,
                 use_viewdirs: bool = True, noise_std: float = 0.0, lindisp: bool = False,
                 precision: str = "f16x3", train_precision: str = "f16x3", train_numerics=None,
                 fused_march: bool = True, range_check: bool = True):
        """The reference's kwargs (model.py:124-145) plus, per model: ``precision`` (render MLP:
        "f16x3" or exact "fp32"), ``train_precision`` / ``train_numerics`` (the training step's
        kernels, aonerf/numerics.py), ``fused_march`` (the coarse compositor fused with the fine
        level's resampling) and ``range_check`` (after a f16x3 render, read the packs'
        range-status words -- one sync per forward, skipped under HIP-graph capture -- and
        re-render on the fp32 kernels on overflow)."""
        super().__init__()
        if num_levels != 2:
            raise ValueError("the reference NeRF is two-level (coarse + fine)")
        self.train_numerics = _resolve_numerics(train_precision, train_numerics)
        self.fused_march, self.range_check = bool(fused_march), bool(range_check)
        self.num_levels, self.min_deg_point, self.max_deg_point = num_levels, min_deg_point, max_deg_point
        self.deg_view, self.num_coarse_samples, self.num_fine_samples = deg_view, num_coarse_samples, num_fine_samples
        self.use_viewdirs, self.noise_std, self.lindisp = use_viewdirs, noise_std, lindisp
        self.coarse_mlp = NeRFMLP(min_deg_point, max_deg_point, deg_view, precision=precision)
        self.fine_mlp = NeRFMLP(min_deg_point, max_deg_point, deg_view, precision=precision)

    def set_precision(self, precision):
        for m in (self.coarse_mlp, self.fine_mlp):
            if precision not in L.PREC:
                raise ValueError(precision)
            m.precision = precision
        return self

    def forward(self, rays, randomized, white_bkgd, near, far, *, u_coarse=None, u_fine=None,
                return_weights=False, return_intermediates=False, timers=None, fine_only=False):
        """reference model.py:147-199 -> [(comp_rgb, acc, depth)_coarse, (...)_fine].

        ``u_coarse`` (B, Sc+1) / ``u_fine`` (B, Nf) inject the uniforms of randomized mode;
        ``return_weights`` adds each level's weights (B, S) as a 4th element;
        ``return_intermediates`` adds a dict(t_vals, weights[, rgb_sigma]) as the last element
        (rgb_sigma (B*S, 4), inference path only: the activated MLP outputs the compositor
        consumed);
        ``timers`` (dict) records hip events around each level's MLP / composite launches (the
        training path: around its fused training kernels);
        ``fine_only`` (inference path, without ``return_weights`` / ``return_intermediates``): the
        caller keeps only the fine level, so the coarse level's colour is not computed and the
        first element is None.  The fine level is the same, bit for bit: the coarse level reaches
        it through its weights alone, which read sigma and t.  On f16x3 the coarse MLP then runs
        the density-only kernel (aon_mlp_fwd_sigma) and the fine MLP reads the per-ray view
        encodings, formed once per forward (aon_pos_enc), instead of recomputing them per sample
        (aon_mlp_fwd_cond); fp32 has no such kernels and runs aon_mlp_fwd.

        With autograd enabled and trainable parameters, each level runs the training path
        (train.RenderLevel: the fused training forward aon_mlp_fwd_train, which also stores the
        activations and their ReLU' bits, then the HIP backward); otherwise the fused inference
        kernels (two_level.py drives the two levels either way).
        """
        o, d, v = rays["rays_o"], rays["rays_d"], rays["viewdirs"]
        L.require_gpu(o, d, v)
        o, d, v = L.contig(o), L.contig(d), L.contig(v)
        kw = dict(u_coarse=u_coarse, u_fine=u_fine, return_weights=return_weights,
                  return_intermediates=return_intermediates, timers=timers)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            spec = SimpleNamespace(model=self, train_level=self._train_level(timers))
            return two_level.train(spec, o, d, v, randomized, white_bkgd, near, far, **kw)
        fine_only = bool(fine_only) and not (return_weights or return_intermediates)
        return two_level.render(self._render_spec(v, fine_only), o, d, v, randomized, white_bkgd,
                                near, far, fine_only=fine_only, **kw)

    def _train_level(self, timers):
        from . import train
        cfg = self.train_numerics
        token, joined = None, {}
        if cfg.overlap_dweight and cfg.fused_backward and timers is None:
            # both levels' parameters through one Join: its backward, after both levels',
            # joins the fine level's weight-gradient stream (overlap_dweight)
            token = train.JoinToken()
            ps = [p for m in (self.coarse_mlp, self.fine_mlp) for l in m._layers()
                  for p in (l.weight, l.bias)]
            joined = dict(zip(map(id, ps), train.Join.apply(token, *ps)))

        def train_level(level, mlp, o, d, v, t_vals, white_bkgd, noise, timers):
            params = [joined.get(id(p), p) for m in mlp._layers() for p in (m.weight, m.bias)]
            return train.RenderLevel.apply(o, d, v, t_vals, bool(white_bkgd), noise, token, cfg,
                                           timers, *params)
        return train_level

    def _render_spec(self, v, fine_only):
        mlps = (self.coarse_mlp, self.fine_mlp)
        two_pass = fine_only and mlps[0].precision == mlps[1].precision == "f16x3"
        cond = helper.pos_enc(v, 0, self.deg_view) if two_pass else None  # once per forward

        def mlp_raw(level, mlp, o, d, v, t_vals, act):
            if not (two_pass and mlp.precision == "f16x3"):  # (the fallback's fp32: aon_mlp_fwd)
                return mlp.forward_rays(o, d, v, t_vals, act=act)
            if level == 0:  # density only: the compositor's colour of a zero rgb means nothing
                return mlp.forward_sigma(o, d, t_vals, act=act)
            return mlp.forward_rays(o, d, v, t_vals, act=act, cond=cond)

        return SimpleNamespace(
            model=self, mlp_raw=mlp_raw, keep_fine_weights=False, extras_key="rgb_sigma",
            # the activations (model.py:186-187) run in the MLP epilogue, unless density noise
            # must be added to the raw sigma first (model.py:183-184)
            acts=lambda noisy: (L.ACT_NONE, L.ACT_VANILLA) if noisy else (L.ACT_VANILLA, L.ACT_NONE),
            range_checked=lambda: self.range_check and mlps[0].precision.startswith("f16x3"),
            packs=lambda: [m._packed for m in mlps],
            # (past |x| = 8188 the fp16x3 split cannot hold an activation; fp32 has no limit)
            fallback=lambda: two_level.switched(mlps, "precision", "fp32"),
            warning="NeRF: an MLP activation exceeded the fp16x3 range; re-rendered with "
                    "precision='fp32'")
