"""Geometry queries on a trained density field: occupancy, extraction and collision tests start
from the density at points, which both models' NeRFMLP answer with one density-only launch
(``NeRFMLP.density``: aon_mlp_art_fwd_sigma_points for the articulated model at a given
articulation, aon_mlp_fwd_sigma for the vanilla one)."""
import torch

from . import _lib as L

# points per density launch when ``chunk`` is not given (a 256^3 grid is 16.8 M points: 8 launches)
DEFAULT_CHUNK = 1 << 21


def grid_points(resolution, box_side_length=2.0, device="cuda"):
    """(R, R, R, 3) voxel centres of the box of side ``box_side_length`` around the origin, built
    on the GPU with ``ij`` indexing: [i, j, k] = (x_i, y_j, z_k), x slowest."""
    R = int(resolution)
    if R < 1:
        raise ValueError("resolution must be >= 1")
    half = 0.5 * float(box_side_length)
    c = (torch.arange(R, device=device, dtype=torch.float32) + 0.5) * (2.0 * half / R) - half
    return torch.stack(torch.meshgrid(c, c, c, indexing="ij"), -1)


@torch.no_grad()
def density_grid(mlp, resolution, box_side_length=2.0, latents=None, chunk=None, activated=True):
    """(R, R, R) sigma at the voxel centres of the box (grid_points), through ``mlp.density`` in
    chunks of ``chunk`` points.  ``mlp``: either model's NeRFMLP; ``latents`` (the dict of latent
    codes) is required for the articulated one and refused by the vanilla one.  ``activated``: as
    ``density`` (the sigma the compositor reads, else the raw head output)."""
    from .model_autodecoder import NeRFMLP as ArtMLP

    art = isinstance(mlp, ArtMLP)
    if art and latents is None:
        raise ValueError("density_grid: the articulated NeRFMLP needs latents")
    if not art and latents is not None:
        raise ValueError("density_grid: the vanilla NeRFMLP takes no latents")
    dev = next(mlp.parameters()).device
    L.require_gpu(next(mlp.parameters()))
    pts = grid_points(resolution, box_side_length, dev).reshape(-1, 3)
    N = pts.shape[0]
    step = max(int(chunk or DEFAULT_CHUNK), 1)
    out = torch.empty((N,), device=dev)
    for i in range(0, N, step):
        p = pts[i:i + step]
        out[i:i + step] = (mlp.density(p, latents, activated=activated) if art
                           else mlp.density(p, activated=activated))
    R = int(resolution)
    return out.view(R, R, R)
