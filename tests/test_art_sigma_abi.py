"""CPU-side checks of the articulated density-only pass (include/aonerf.h aon_mlp_art_fwd_sigma,
aon_mlp_art_fwd_sigma_points), in the pattern of tests/test_sigma_abi.py: declared, exported and
bound, additive in ABI 13, and every refusal happens in argument validation -- the pointers below
are not device memory, so a launch that got past it would not return -1.  Also the stream layout
the pass relies on, restated from the shape table, and the Python surface's argument checks that
need no GPU."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT
from test_capi import declared_symbols

NEW = ("aon_mlp_art_fwd_sigma", "aon_mlp_art_fwd_sigma_points")
P = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced
ODD = ctypes.c_void_p(24)


@pytest.fixture(scope="module")
def L():
    from aonerf import _lib

    return _lib


def _args(name, packed=P, o=P, d=P, t=P, B=4, S=8, act=0, out=P):
    """aon_mlp_art_fwd_sigma(packed, rays_o, rays_d, t, B, S, act, out, stream) /
    aon_mlp_art_fwd_sigma_points(packed, pos, N, act, out, stream): ``o`` is pos, ``B`` is N."""
    if name == "aon_mlp_art_fwd_sigma":
        return (packed, o, d, t, B, S, act, out, None)
    return (packed, o, B, act, out, None)


def test_symbols_declared_exported_and_bound(L):
    lib = L.lib()
    for s in NEW:
        assert s in declared_symbols(), f"{s} not declared in aonerf.h"
        assert hasattr(lib, s) and s in L._SIGNATURES, s
    assert len(L._SIGNATURES["aon_mlp_art_fwd_sigma"][1]) == 9
    assert len(L._SIGNATURES["aon_mlp_art_fwd_sigma_points"][1]) == 6


def test_abi_version_stays_13(L):
    assert L.lib().aon_abi_version() == 13 and L.ABI_VERSION == 13


@pytest.mark.parametrize("name", NEW)
def test_refuses_null_and_misaligned_pointers(L, name):
    keys = ["packed", "o", "out"] + (["d", "t"] if name == "aon_mlp_art_fwd_sigma" else [])
    for k in keys:
        with pytest.raises(ValueError, match=f"{name}: null pointer"):
            L.call(name, *_args(name, **{k: None}))
    for k in ("packed", "out"):
        with pytest.raises(ValueError, match=f"{name}: .*16-byte aligned"):
            L.call(name, *_args(name, **{k: ODD}))


@pytest.mark.parametrize("name", NEW)
def test_refuses_bad_shapes_and_activations(L, name):
    if name == "aon_mlp_art_fwd_sigma":
        with pytest.raises(ValueError, match=f"{name}: bad shape"):
            L.call(name, *_args(name, S=0))
        with pytest.raises(ValueError, match=f"{name}: too many rows"):
            L.call(name, *_args(name, B=1 << 62, S=4))  # B * S past int64
    with pytest.raises(ValueError, match=f"{name}: bad shape"):
        L.call(name, *_args(name, B=-1))
    for act in (3, -1):
        with pytest.raises(ValueError, match=f"{name}: bad activation"):
            L.call(name, *_args(name, act=act))
    with pytest.raises(ValueError, match=f"{name}: too many rows"):
        L.call(name, *_args(name, B=1 << 38, S=1))  # 128-row workgroups past 2^31
    L.call(name, *_args(name, B=0))  # nothing to do: no launch, no error
    for act in (L.ACT_NONE, L.ACT_VANILLA, L.ACT_ARTIC):  # what aon_mlp_art_fwd accepts
        L.call(name, *_args(name, B=0, act=act))


def test_density_prefix_of_the_articulated_stream():
    """The numbers mlp_layout.hpp pins for the density-only prefix, restated from the shape table
    as build_layout sums them: everything through density_layer is the first 2,152 blocks (2,176
    in whole 32-block ring chunks, inside the stream's 2,752) and 2,592 bias rows, where
    bottleneck_layer begins; and the MACs the pass issues against the full kernel's."""
    text = open(os.path.join(ROOT, "articulated-object-nerf_amd", "csrc", "mlp_layout.hpp")).read()
    body = text[text.index("constexpr LayerShape kShapeArt[kNumLayersArt]"):]
    rows = [tuple(map(int, r))
            for r in re.findall(r"\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\}", body)[:20]]
    assert len(rows) == 20

    def totals(rs):
        blk = sum((ka + kb) * u * 2 for ka, kb, u, _, _, _ in rs)
        return blk, sum(16 * u for _, _, u, _, _, _ in rs), blk // 2 * 512  # 16 x 32 MACs / pair

    assert totals(rows) == (2752, 3376, 704512)
    assert totals(rows[:14]) == (2152, 2592, 550912)
    assert 2152 <= 2176 <= 2752 and 2176 % 32 == 0 and (2152 - 1) // 32 == 2176 // 32 - 1
    assert "using NetArtSigmaH = Prefix<NetArtH, A_DEN + 1, 32>;" in text
    assert "static_assert(net_is<NetArtSigmaH>(2152, 2176, 2592)" in text


def test_python_surface_signatures():
    from aonerf import geometry, render
    from aonerf.model import NeRFMLP as VanillaMLP
    from aonerf.model_autodecoder import NeRF_AE_Art, NeRFMLP

    assert inspect.signature(NeRF_AE_Art.forward).parameters["fine_only"].default is False
    for fn in (render.render_rays, render.render_rays_test, render.render_frame,
               render._render_box):
        assert inspect.signature(fn).parameters["latents"].default is None, fn.__name__
    assert list(inspect.signature(NeRFMLP.forward_sigma).parameters)[1:] == [
        "rays_o", "rays_d", "t_vals", "latents", "act"]
    assert inspect.signature(NeRFMLP.density).parameters["activated"].default is True
    assert inspect.signature(VanillaMLP.density).parameters["activated"].default is True
    sig = inspect.signature(geometry.density_grid).parameters
    assert [sig[k].default for k in ("box_side_length", "latents", "chunk", "activated")] == [
        2.0, None, None, True]


def test_density_refuses_bad_points_before_any_launch():
    from aonerf import geometry
    from aonerf.model import NeRFMLP as VanillaMLP
    from aonerf.model_autodecoder import NeRFMLP

    art, van = NeRFMLP(0, 10, 4), VanillaMLP(0, 10, 4)
    with pytest.raises(ValueError, match=r"\(\.\.\., 3\)"):
        art.density(torch.zeros(4, 2), {})
    with pytest.raises(ValueError, match=r"\(\.\.\., 3\)"):
        van.density(torch.zeros(4, 2))
    with pytest.raises(ValueError, match="MI355X only"):
        art.density(torch.zeros(4, 3), {})
    with pytest.raises(ValueError, match="fp32"):
        VanillaMLP(0, 10, 4, precision="fp32").density(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="needs latents"):
        geometry.density_grid(art, 4)
    with pytest.raises(ValueError, match="takes no latents"):
        geometry.density_grid(van, 4, latents={})
    with pytest.raises(ValueError, match="resolution"):
        geometry.grid_points(0, device="cpu")
    g = geometry.grid_points(4, 2.0, device="cpu")  # voxel centres, x slowest
    assert tuple(g.shape) == (4, 4, 4, 3)
    assert torch.equal(g[1, 2, 3], torch.tensor([-0.25, 0.25, 0.75]))
