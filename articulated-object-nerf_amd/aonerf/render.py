"""Render-batch API of the reference's Lightning system (models/vanilla_nerf/model.py:295-348)
and the synthetic SAPIEN cameras used by the benches (datasets/sapien_multi.py:29-72)."""
import math
from collections import defaultdict

import numpy as np
import torch

from . import helper, interface
from .ray_utils import frame_rays

# The reference splits every image into hparams.chunk = 3840-ray pieces (opt.py:103) only to
# bound activation memory on a 11 GB card; on a 288 GB MI355X a whole 640x480 frame is one
# launch per stage.  Outputs do not depend on the chunking (the per-chunk depth clamp of
# helper.py:183 is an identity), so `chunk` only bounds the rays per launch.
DEFAULT_CHUNK = 1 << 21


def _chunks(B, chunk):
    chunk = max(int(chunk or DEFAULT_CHUNK), 1)
    for i in range(0, B, chunk):
        yield i, min(i + chunk, B)


MAP_KEYS = ("canonical", "motion", "motion_mag")  # columns 5:8, 8:11, 11 of a maps payload


def _maps_kw(maps):
    # only a model asked for maps sees the keyword (NeRF_AE_Art.forward; the vanilla model has
    # no deformation and refuses it)
    return {"maps": True} if maps else {}


def _model_args(white_bkgd, near, far, latents):
    # the model call's positional arguments: a model with latent codes (NeRF_AE_Art) takes them
    # after ``far``; None: a vanilla model, or a closure that binds them itself
    return (False, white_bkgd, near, far) + (() if latents is None else (latents,))


def _put_maps(out, i, j, m):
    out[i:j, 5:8], out[i:j, 8:11], out[i:j, 11] = m["canonical"], m["motion"], m["motion_mag"]


def _render_box(model, rays, chunk, white_bkgd, box_side_length, cull, timers=None, maps=False,
                latents=None):
    """(B, 5) payload [rgb(3), depth, acc] of ``rays`` bounded by the box of side
    ``box_side_length`` around the origin.  The bounds are formed once over all the rays (the
    fill of get_ray_limits depends on the batch), not per chunk.  ``cull``: only the rays that
    hit the box reach the MLPs (zero hits: no MLP launch); the others are background rows.
    ``maps``: (B, 12), the payload followed by canonical (3), motion (3), motion_mag -- zero on
    a culled ray."""
    o, d, v = rays["rays_o"], rays["rays_d"], rays["viewdirs"]
    B, dev = o.shape[0], o.device
    kw = _maps_kw(maps)
    if not cull:
        near, far = helper.get_ray_limits(o, d, box_side_length)
        out = torch.empty((B, 12 if maps else 5), device=dev)
        for i, j in _chunks(B, chunk):
            sub = {k: x[i:j] for k, x in rays.items()}
            fine = model(sub, *_model_args(white_bkgd, near[i:j], far[i:j], latents),
                         timers=timers, fine_only=True, **kw)[1]
            out[i:j, 0:3] = fine[0]
            out[i:j, 3] = fine[2]
            out[i:j, 4] = fine[1]
            if maps:
                _put_maps(out, i, j, fine[-1])
        return out
    if torch.cuda.is_current_stream_capturing():
        raise ValueError("box culling reads the hit count on the host, which a stream capture "
                         "cannot record: render with cull=False under capture")
    tmin, tmax = helper.get_ray_limits_box(o, d, box_side_length)
    c = helper.compact_rays(tmin, tmax, o, d, v)
    n = int(c["n_hit"].item())  # the one 4-byte read-back of the call
    comp = torch.empty((n, 3), device=dev)
    acc, depth = torch.empty((n,), device=dev), torch.empty((n,), device=dev)
    hit = torch.empty((n, 12), device=dev) if maps else None  # columns 5.. : the hit rays' maps
    for i, j in _chunks(n, chunk):
        sub = {k: c[k][i:j] for k in ("rays_o", "rays_d", "viewdirs")}
        fine = model(sub, *_model_args(white_bkgd, c["near"][i:j], c["far"][i:j], latents),
                     timers=timers, fine_only=True, **kw)[1]
        comp[i:j], acc[i:j], depth[i:j] = fine[0], fine[1], fine[2]
        if maps:
            _put_maps(hit, i, j, fine[-1])
    out = helper.scatter_payload(comp, acc, depth, c["slot"], white_bkgd)
    if not maps:
        return out
    # the maps through the same scatter kernel, on a black background: a miss is a zero row
    a = helper.scatter_payload(hit[:, 5:8], hit[:, 11], hit[:, 8], c["slot"], False)
    b = helper.scatter_payload(hit[:, 8:11], hit[:, 11], hit[:, 8], c["slot"], False)
    return torch.cat([out, a[:, 0:3], b[:, 0:3], a[:, 4:5]], 1)


@torch.no_grad()
def render_rays(model, batch, chunk, white_bkgd, near, far, box_side_length=None, cull=True,
                maps=False, latents=None):
    """LitNeRF.render_rays (model.py:295-321): fine-level comp_rgb/acc/depth over all rays and
    psnr_legacy against batch['target'] (returned as 'psnr' instead of being logged).

    ``maps`` (a model with a deformation field: NeRF_AE_Art.forward(maps=True)): also
    'canonical' (B, 3), 'motion' (B, 3) and 'motion_mag' (B,), concatenated over the chunks like
    comp_rgb; zero on a ray that box culling dropped.

    ``latents`` (NeRF_AE_Art: the dict of latent codes): passed to the model after ``far``, so
    the articulated model renders without a closure and gets ``fine_only=True`` -- its coarse
    level then runs the density-only pass.  None: the model is called as before.

    ``box_side_length`` (default None: ``near`` / ``far`` as given): bound every ray by the box
    of that side around the origin instead (helper.get_ray_limits; ``near`` / ``far`` are then
    unused).  With ``cull`` the rays that miss the box skip both MLPs and come out as background
    (rgb 1 or 0 by ``white_bkgd``, acc 0, depth 0): one 4-byte read-back per call, so not under
    stream capture (``cull=False`` there)."""
    B = batch["rays_o"].shape[0]
    if box_side_length is not None:
        rays = {k: batch[k] for k in ("rays_o", "rays_d", "viewdirs")}
        p = _render_box(model, rays, chunk, white_bkgd, box_side_length, cull, maps=maps,
                        latents=latents)
        out = {"comp_rgb": p[:, 0:3].contiguous(), "acc": p[:, 4].contiguous(),
               "depth": p[:, 3].contiguous()}
        if maps:
            out.update(canonical=p[:, 5:8].contiguous(), motion=p[:, 8:11].contiguous(),
                       motion_mag=p[:, 11].contiguous())
        if "target" in batch:
            out["psnr"] = interface.psnr_legacy(out["comp_rgb"], batch["target"]).mean()
        return out
    ret = defaultdict(list)
    for i, j in _chunks(B, chunk):
        sub = {k: batch[k][i:j] for k in ("rays_o", "rays_d", "viewdirs")}
        fine = model(sub, *_model_args(white_bkgd, near, far, latents), fine_only=True,
                     **_maps_kw(maps))[1]
        ret["comp_rgb"].append(fine[0])
        ret["acc"].append(fine[1])
        ret["depth"].append(fine[2])
        for k in MAP_KEYS if maps else ():
            ret[k].append(fine[-1][k])
    out = {k: torch.cat(v, 0) for k, v in ret.items()}
    if "target" in batch:
        out["psnr"] = interface.psnr_legacy(out["comp_rgb"], batch["target"]).mean()
    return out


@torch.no_grad()
def render_rays_test(model, batch, chunk, white_bkgd, near, far, latents=None):
    """LitNeRF.render_rays_test (model.py:323-348) -> {target, instance_mask, rgb}
    (``latents``: as render_rays)."""
    out = render_rays(model, {k: v for k, v in batch.items() if k != "target"}, chunk, white_bkgd,
                      near, far, latents=latents)
    test_output = {"rgb": out["comp_rgb"]}
    for k in ("target", "instance_mask"):
        if k in batch:
            test_output[k] = batch[k]
    return test_output


@torch.no_grad()
def render_frame(model, c2w, H, W, focal, near=2.0, far=6.0, white_bkgd=True, p0=0, n=None,
                 chunk=None, timers=None, box_side_length=None, cull=True, maps=False,
                 latents=None):
    """Fused ray generation + two-level render of pixels [p0, p0+n) of an H x W frame.
    Returns (n, 5) = [rgb(3), depth, acc] per pixel (the payload of the frame gather).
    ``box_side_length`` / ``cull``: as render_rays (the bounds are formed over the n pixels).
    ``maps`` (as render_rays): (n, 12), the payload followed by canonical (3), motion (3) and
    motion_mag.  ``latents``: as render_rays."""
    n = H * W - p0 if n is None else n
    rays = frame_rays(c2w, H, W, focal, p0, n)
    if box_side_length is not None:
        return _render_box(model, rays, chunk, white_bkgd, box_side_length, cull, timers, maps,
                           latents)
    out = torch.empty((n, 12 if maps else 5), device=rays["rays_o"].device)
    for i, j in _chunks(n, chunk):
        sub = {k: v[i:j] for k, v in rays.items()}
        fine = model(sub, *_model_args(white_bkgd, near, far, latents), timers=timers,
                     fine_only=True, **_maps_kw(maps))[1]
        out[i:j, 0:3] = fine[0]
        out[i:j, 3] = fine[2]
        out[i:j, 4] = fine[1]
        if maps:
            _put_maps(out, i, j, fine[-1])
    return out


# ----------------------------------------------------------------------------- cameras
def create_spheric_poses(radius=4.0, n=40, phi=-30.0):
    """datasets/sapien_multi.py:29-72 -> (n, 4, 4) float32 camera-to-world matrices."""

    def trans_t(t):
        return np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, t], [0, 0, 0, 1]], np.float32)

    def rot_phi(p):
        c, s = np.cos(p), np.sin(p)
        return np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]], np.float32)

    def rot_theta(th):
        c, s = np.cos(th), np.sin(th)
        return np.array([[c, 0, -s, 0], [0, 1, 0, 0], [s, 0, c, 0], [0, 0, 0, 1]], np.float32)

    flip = np.array([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.float32)
    out = []
    for angle in np.linspace(-180, 180, n + 1)[:-1]:
        m = torch.from_numpy(trans_t(radius))
        m = torch.from_numpy(rot_phi(phi / 180.0 * np.pi)) @ m
        m = torch.from_numpy(rot_theta(angle / 180.0 * np.pi)) @ m
        out.append(torch.from_numpy(flip) @ m)
    return torch.stack(out, 0)


def sapien_focal(H, fovy_deg=35.0):
    """SAPIEN pinhole (datagen/data_gen.py:60-67): focal = 0.5*H / tan(0.5*fovy)."""
    return 0.5 * H / math.tan(0.5 * math.radians(fovy_deg))
