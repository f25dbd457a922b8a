"""Drop-in for ``models/vanilla_nerf/helper.py`` of the reference, running on the MI355X.

Same function names, argument meaning and return tuples as the reference; the work happens in
the HIP kernels of libaonerf.so (include/aonerf.h).  Extensions over the reference signatures
are keyword-only extras (``u=...``) that inject the uniforms the reference draws with
torch.rand (helper.py:126, :227) so randomized mode is testable.

The only host-side arithmetic is the 1-D sample schedule (S floats): it is built with the very
torch CPU ops the reference uses (helper.py:116-125, :229) because torch's CPU linspace is not a
closed formula (vectorised blocks round differently), then cached on the device.
"""
import numpy as np
import torch

from . import _lib as L


# ----------------------------------------------------------------------------- metrics
def img2mse(x, y):
    """reference helper.py:17-18."""
    return torch.mean((x - y) ** 2)


def mse2psnr(x):
    """reference helper.py:21-22."""
    return -10.0 * torch.log(x) / np.log(10)


def cast_rays(t_vals, origins, directions):
    """reference helper.py:25-26 (elementwise; fused into every kernel that needs xyz)."""
    return origins[..., None, :] + t_vals[..., None] * directions[..., None, :]


# ----------------------------------------------------------------------------- schedules
_sched_cache = {}


def coarse_schedule(num_samples, near, far, lindisp, device):
    """(t, lower, upper) of helper.py:116-125 as device tensors, built with torch CPU ops."""
    key = (int(num_samples), float(near), float(far), bool(lindisp), str(device))
    if key not in _sched_cache:
        t = torch.linspace(0.0, 1.0, num_samples + 1)
        if lindisp:
            t = 1.0 / (1.0 / near * (1.0 - t) + 1.0 / far * t)
        else:
            t = near * (1.0 - t) + far * t
        mids = 0.5 * (t[..., 1:] + t[..., :-1])
        upper = torch.cat([mids, t[..., -1:]], -1)
        lower = torch.cat([t[..., :1], mids], -1)
        _sched_cache[key] = tuple(x.to(device) for x in (t, lower, upper))
    return _sched_cache[key]


def eval_u(num_samples, device, float_min_eps=2 ** -32):
    """u of helper.py:229 (its last entry rounds to exactly 1.0 in fp32)."""
    key = ("u", int(num_samples), float(float_min_eps), str(device))
    if key not in _sched_cache:
        _sched_cache[key] = torch.linspace(0.0, 1.0 - float_min_eps, num_samples).to(device)
    return _sched_cache[key]


def unit_schedule(num_samples, device):
    """torch.linspace(0, 1, num_samples + 1) of helper.py:116 as a device tensor (built on the
    CPU, as the reference's values are)."""
    key = ("s", int(num_samples), str(device))
    if key not in _sched_cache:
        _sched_cache[key] = torch.linspace(0.0, 1.0, num_samples + 1).to(device)
    return _sched_cache[key]


# ----------------------------------------------------------------------------- box bounds
def _flat_rays(rays_o, rays_d, box_side_length):
    L.require_gpu(rays_o, rays_d)
    if rays_o.shape[-1] != 3 or rays_o.shape != rays_d.shape:
        raise ValueError("ray limits expect rays_o and rays_d of one shape (..., 3)")
    half = float(box_side_length / 2)
    o = L.contig(rays_o.detach().reshape(-1, 3))
    d = L.contig(rays_d.detach().reshape(-1, 3))
    return o, d, half, tuple(rays_o.shape[:-1]) + (1,)


def get_ray_limits_box(rays_o, rays_d, box_side_length):
    """reference helper.py:42-102 -> (tmin, tmax), each (..., 1); misses hold (-1, -2)."""
    o, d, half, shape = _flat_rays(rays_o, rays_d, box_side_length)
    B = o.shape[0]
    tmin, tmax = torch.empty((B,), device=o.device), torch.empty((B,), device=o.device)
    L.call("aon_ray_limits_box", L.ptr(o), L.ptr(d), B, half, L.ptr(tmin), L.ptr(tmax),
           L.stream(o.device))
    return tmin.reshape(shape), tmax.reshape(shape)


def get_ray_limits(rays_o, rays_d, box_side_length=2):
    """reference helper.py:29-39 -> (near, far), each (..., 1): the box limits, the rays that
    miss filled with the batch's smallest near / largest far, negatives clamped to 0."""
    o, d, half, shape = _flat_rays(rays_o, rays_d, box_side_length)
    B = o.shape[0]
    near, far = torch.empty((B,), device=o.device), torch.empty((B,), device=o.device)
    nbytes = L.lib().aon_ray_limits_workspace_bytes(B)
    work = torch.empty((nbytes // 4,), dtype=torch.int32, device=o.device)
    L.call("aon_ray_limits", L.ptr(o), L.ptr(d), B, half, L.ptr(near), L.ptr(far), L.ptr(work),
           nbytes, L.stream(o.device))
    return near.reshape(shape), far.reshape(shape)


def compact_rays(tmin, tmax, rays_o, rays_d, viewdirs=None):
    """The rays that hit the box (tmax > max(tmin, 0); NaN: a miss), in order, from the box
    limits of get_ray_limits_box.  Returns a dict: ``slot`` (B,) int32 -- the rank of each ray
    among the hits or -1; ``n_hit`` -- a 0-dim int32 DEVICE tensor (reading it is the caller's
    one sync); and, B rows each of which the first n_hit are written, ``idx`` (int32),
    ``rays_o`` / ``rays_d`` / ``viewdirs`` (B, 3), ``near`` = max(tmin, 0) and ``far`` (B,)."""
    L.require_gpu(tmin, tmax, rays_o, rays_d, viewdirs)
    B = rays_o.shape[0]
    dev = rays_o.device
    if tmin.numel() != B or tmax.numel() != B:
        raise ValueError(f"tmin / tmax must hold {B} limits")
    tmin, tmax = L.contig(tmin.reshape(B)), L.contig(tmax.reshape(B))
    rays_o, rays_d = L.contig(rays_o), L.contig(rays_d)
    viewdirs = None if viewdirs is None else L.contig(viewdirs)
    out = {"slot": torch.empty((B,), dtype=torch.int32, device=dev),
           "idx": torch.empty((B,), dtype=torch.int32, device=dev),
           "rays_o": torch.empty((B, 3), device=dev), "rays_d": torch.empty((B, 3), device=dev),
           "viewdirs": None if viewdirs is None else torch.empty((B, 3), device=dev),
           "near": torch.empty((B,), device=dev), "far": torch.empty((B,), device=dev),
           "n_hit": torch.empty((), dtype=torch.int32, device=dev)}
    nbytes = L.lib().aon_compact_rays_workspace_bytes(B)
    work = torch.empty((nbytes // 4,), dtype=torch.int32, device=dev)
    L.call("aon_compact_rays", L.ptr(tmin), L.ptr(tmax), L.ptr(rays_o), L.ptr(rays_d),
           L.ptr(viewdirs), B, L.ptr(out["slot"]), L.ptr(out["idx"]), L.ptr(out["rays_o"]),
           L.ptr(out["rays_d"]), L.ptr(out["viewdirs"]), L.ptr(out["near"]), L.ptr(out["far"]),
           L.ptr(out["n_hit"]), L.ptr(work), nbytes, L.stream(dev))
    return out


def scatter_payload(comp, acc, depth, slot, white_bkgd):
    """(B, 5) = [rgb(3), depth, acc] per frame ray from the rendered compact rows (comp (n, 3),
    acc / depth (n,)): row slot[b], or the background row (rgb 1 or 0, depth 0, acc 0)."""
    L.require_gpu(comp, acc, depth)
    B, n = slot.shape[0], comp.shape[0]
    if slot.dtype != torch.int32 or tuple(comp.shape) != (n, 3) or acc.numel() != n \
            or depth.numel() != n:
        raise ValueError("scatter_payload: slot must be int32, comp (n, 3), acc / depth (n,)")
    comp, acc, depth, slot = (L.contig(x) for x in (comp, acc, depth, slot))
    out = torch.empty((B, 5), device=slot.device)
    L.call("aon_scatter_payload", L.ptr(comp), L.ptr(acc), L.ptr(depth), n, L.ptr(slot), B,
           int(bool(white_bkgd)), L.ptr(out), L.stream(slot.device))
    return out


# ----------------------------------------------------------------------------- sampling
def _ray_bound(x, B, dev, name):
    """A per-ray bound as a contiguous (B,) device tensor: (B,), (B, 1), or a python number."""
    if not isinstance(x, torch.Tensor):
        return torch.full((B,), x, dtype=torch.float32, device=dev)
    L.require_gpu(x)
    if tuple(x.shape) not in ((B,), (B, 1)):
        raise ValueError(f"{name} must be a number or a ({B},) / ({B}, 1) tensor, got "
                         f"{tuple(x.shape)}")
    return L.contig(x.detach().reshape(B))


def sample_along_rays(rays_o, rays_d, num_samples, near, far, randomized, lindisp, *, u=None,
                      want_coords=True):
    """reference helper.py:106-133 -> (t_vals (B, S+1), coords (B, S+1, 3)).  ``near`` / ``far``:
    two python numbers (one cached schedule for the batch), or per-ray bounds -- a (B,) or
    (B, 1) tensor for either, the other a tensor or a number (helper.py:117-120 broadcasting)."""
    L.require_gpu(rays_o, rays_d, u)
    rays_o, rays_d = L.contig(rays_o), L.contig(rays_d)
    B, S = rays_o.shape[0], num_samples + 1
    dev = rays_o.device
    per_ray = isinstance(near, torch.Tensor) or isinstance(far, torch.Tensor)
    if per_ray:
        near, far = _ray_bound(near, B, dev, "near"), _ray_bound(far, B, dev, "far")
        s_tab = unit_schedule(num_samples, dev)
    else:
        t_sched, lower, upper = coarse_schedule(num_samples, near, far, lindisp, dev)
    if randomized and u is None:
        u = torch.rand((B, S), device=dev)
    u = L.contig(u) if randomized else None
    if u is not None and tuple(u.shape) != (B, S):
        raise ValueError(f"u must be ({B}, {S})")
    t_vals = torch.empty((B, S), device=dev)
    coords = torch.empty((B, S, 3), device=dev) if want_coords else None
    if per_ray:
        L.call("aon_sample_along_rays_bounds", L.ptr(rays_o), L.ptr(rays_d), B, S, L.ptr(s_tab),
               L.ptr(near), L.ptr(far), int(bool(lindisp)), L.ptr(u), L.ptr(t_vals),
               L.ptr(coords), L.stream(dev))
        return t_vals, coords
    base = lower if randomized else t_sched  # eval mode: the schedule itself (helper.py:129)
    L.call("aon_sample_along_rays", L.ptr(rays_o), L.ptr(rays_d), B, S, L.ptr(base), L.ptr(upper),
           L.ptr(u), L.ptr(t_vals), L.ptr(coords), L.stream(dev))
    return t_vals, coords


def pos_enc(x, min_deg, max_deg):
    """reference helper.py:136-140 -> (..., 3 + 6*(max_deg-min_deg))."""
    L.require_gpu(x)
    if x.shape[-1] != 3:
        raise ValueError("pos_enc expects (..., 3) inputs")
    x = L.contig(x)
    n = x.numel() // 3
    out = torch.empty(list(x.shape[:-1]) + [3 + 6 * (max_deg - min_deg)], device=x.device)
    L.call("aon_pos_enc", L.ptr(x), n, min_deg, max_deg, L.ptr(out), L.stream(x.device))
    return out


# ----------------------------------------------------------------------------- composite
def volumetric_rendering(rgb, density, t_vals, dirs, white_bkgd, nocs=None):
    """reference helper.py:157-195 -> (comp_rgb, acc, weights, depth | comp_nocs)."""
    L.require_gpu(rgb, density, t_vals, dirs)
    B, S = t_vals.shape
    if tuple(rgb.shape) != (B, S, 3) or tuple(density.shape) != (B, S, 1) or dirs.shape[-1] != 3:
        raise ValueError("volumetric_rendering: shape mismatch")
    rgb, density, t_vals, dirs = (L.contig(x) for x in (rgb, density, t_vals, dirs))
    comp = torch.empty((B, 3), device=rgb.device)
    acc = torch.empty((B,), device=rgb.device)
    w = torch.empty((B, S), device=rgb.device)
    depth = torch.empty((B,), device=rgb.device)
    L.call("aon_composite_fwd", L.ptr(rgb), 3, L.ptr(density), 1, L.ptr(t_vals), L.ptr(dirs), B, S,
           int(bool(white_bkgd)), L.ACT_NONE, L.ptr(comp), L.ptr(acc), L.ptr(w), L.ptr(depth),
           L.stream(rgb.device))
    if nocs is not None:
        return comp, acc, w, (w[..., None] * nocs).sum(dim=-2)
    return comp, acc, w, depth


def composite_features(weights, feat):
    """A per-sample feature composited with a render's weights (reference helper.py:191-193,
    comp_nocs): weights (B, S), feat (B, S, C) or (B*S, C), 1 <= C <= 8 -> (B, C) =
    sum_s weights[b, s] feat[b, s, :], on aon_composite_feat (summed in the order
    aon_composite_fwd sums comp_rgb).  A 2-D ``feat`` may be a column slice of wider rows (unit
    column stride): it is read in place."""
    L.require_gpu(weights, feat)
    if weights.dim() != 2:
        raise ValueError("composite_features: weights must be (B, S)")
    B, S = weights.shape
    C = feat.shape[-1]
    if feat.dim() not in (2, 3) or feat.numel() != B * S * C or not 1 <= C <= 8:
        raise ValueError(f"composite_features: feat must be ({B}, {S}, C) or ({B * S}, C), "
                         f"1 <= C <= 8, got {tuple(feat.shape)}")
    if not 1 <= S <= 512:
        raise ValueError("composite_features: 1 <= S <= 512")
    weights = L.contig(weights.detach())
    feat = feat.detach()
    if not (feat.dim() == 2 and feat.stride(1) == 1 and feat.stride(0) >= C):
        feat = L.contig(feat).reshape(B * S, C)
    out = torch.empty((B, C), device=weights.device)
    L.call("aon_composite_feat", L.ptr(weights), L.ptr(feat), feat.stride(0) if B * S > 1 else C,
           C, B, S, L.ptr(out), L.stream(weights.device))
    return out


# ----------------------------------------------------------------------------- pdf sampling
def _pdf_call(bins, weights, num_samples, randomized, u, t_merge, origins, directions,
              float_min_eps=2 ** -32):
    L.require_gpu(bins, weights, u, t_merge, origins, directions)
    B, nb = bins.shape
    if tuple(weights.shape) != (B, nb - 1):
        raise ValueError("weights must be (B, nbins - 1)")
    dev = bins.device
    bins = L.contig(bins)
    if weights.stride(-1) != 1:
        weights = weights.contiguous()
    if randomized:
        u = torch.rand((B, num_samples), device=dev) if u is None else L.contig(u)
        if tuple(u.shape) != (B, num_samples):
            raise ValueError(f"u must be ({B}, {num_samples})")
        u_stride = num_samples
    else:
        u, u_stride = eval_u(num_samples, dev, float_min_eps), 0
    Nt = 0
    if t_merge is not None:
        t_merge = L.contig(t_merge)
        Nt = t_merge.shape[-1]
    out = torch.empty((B, Nt + num_samples), device=dev)
    xyz = None
    if origins is not None:
        origins, directions = L.contig(origins), L.contig(directions)
        xyz = torch.empty((B, Nt + num_samples, 3), device=dev)
    L.call("aon_sample_pdf", L.ptr(bins), bins.stride(0), L.ptr(weights), weights.stride(0), B, nb,
           num_samples, L.ptr(u), u_stride, L.ptr(t_merge), Nt, L.ptr(origins), L.ptr(directions),
           L.ptr(out), L.ptr(xyz), L.stream(dev))
    return out, xyz


def sorted_piecewise_constant_pdf(bins, weights, num_samples, randomized, float_min_eps=2 ** -32,
                                  *, u=None):
    """reference helper.py:203-243 -> samples (B, num_samples) (unsorted when randomized)."""
    if randomized:
        # the reference returns the samples in u order; sort indices come from the kernel's
        # sorted output, so recover u-order by evaluating without a merge on sorted u
        L.require_gpu(u)
        B = bins.shape[0]
        if u is None:
            u = torch.rand((B, num_samples), device=bins.device)
        us, order = torch.sort(L.contig(u), dim=-1)
        s, _ = _pdf_call(bins, weights, num_samples, True, us, None, None, None)
        out = torch.empty_like(s)
        out.scatter_(-1, order, s)  # samples are monotone in u: sorted u <-> sorted samples
        return out
    s, _ = _pdf_call(bins, weights, num_samples, False, None, None, None, None, float_min_eps)
    return s


def sample_pdf(bins, weights, origins, directions, t_vals, num_samples, randomized, *, u=None):
    """reference helper.py:246-252 -> (sorted t_vals (B, Nt+Ns), coords (B, Nt+Ns, 3))."""
    return _pdf_call(bins.detach(), weights.detach(), num_samples, randomized, u, t_vals.detach(),
                     origins, directions)
