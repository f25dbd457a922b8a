"""CPU-side checks of the latent-code fit (include/aonerf.h aon_art_latent_grad and its workspace
query; aonerf/latent_fit.py; train_art.render_level(latent_only=True)): the symbols are declared,
exported and bound, additive in ABI 13; every refusal happens in argument validation -- the
pointers below are not device memory, so a launch that got past it would not return -1 -- and the
Python layers refuse a trainable MLP before anything touches the GPU."""
import ctypes

import pytest
import torch

from test_capi import _struct_with, declared_symbols

F = "aon_art_latent_grad"
NEW = (F, "aon_art_latent_grad_workspace_bytes")
P, ODD = ctypes.c_void_p(16), ctypes.c_void_p(24)  # non-null, never dereferenced
# the articulated layer table with the latent columns present (the real parameter shapes)
FULL = {0: (128, 163), 5: (256, 191), 10: (256, 447), 15: (128, 411)}


@pytest.fixture(scope="module")
def L():
    from aonerf import _lib

    return _lib


def _params(L, **cols):
    shapes = [FULL.get(i, s) for i, s in enumerate(L.ART_SHAPES)]
    for i, c in cols.items():
        shapes[int(i[1:])] = (shapes[int(i[1:])][0], c)
    return _struct_with(L, L.AonMlpArtParams, 20, shapes)


def _args(L, prm="default", dzv0=P, dz5=P, dz0=P, dzd0=P, bf16=0, N=325, dshape=P, dapp=P,
          dart=P, work=P):
    prm = ctypes.byref(_params(L)) if prm == "default" else prm
    return (prm, dzv0, dz5, dz0, dzd0, bf16, N, dshape, dapp, dart, work, None)


def test_symbols_declared_exported_and_bound(L):
    lib = L.lib()
    for s in NEW:
        assert s in declared_symbols(), f"{s} not declared in aonerf.h"
        assert hasattr(lib, s) and s in L._SIGNATURES, s
    assert len(L._SIGNATURES[F][1]) == 12
    assert len(L._SIGNATURES[NEW[1]][1]) == 1


def test_abi_version_stays_13(L):
    assert L.lib().aon_abi_version() == 13 and L.ABI_VERSION == 13


def test_refuses_null_pointers(L):
    for k in ("prm", "dzv0", "dz5", "dz0", "dzd0", "dshape", "dapp", "dart", "work"):
        with pytest.raises(ValueError, match=f"{F}.*null pointer"):
            L.call(F, *_args(L, **{k: None}))


@pytest.mark.parametrize("N", [0, -1, -(1 << 40)])
def test_refuses_non_positive_rows(L, N):
    with pytest.raises(ValueError, match=f"{F}.*bad shape"):
        L.call(F, *_args(L, N=N))


@pytest.mark.parametrize("k", ["dzv0", "dz5", "dz0", "dzd0", "work"])
def test_refuses_misaligned_tensors(L, k):
    with pytest.raises(ValueError, match=f"{F}.*16-byte aligned"):
        L.call(F, *_args(L, **{k: ODD}))


@pytest.mark.parametrize("bf16", [-1, 2, 7])
def test_refuses_bf16_flag_outside_0_1(L, bf16):
    with pytest.raises(ValueError, match=f"{F}.*bf16"):
        L.call(F, *_args(L, bf16=bf16))


def test_refuses_wrong_geometry_naming_the_layer(L):
    # registration order is not the kernels' layer order: the packs' own check, under this name
    reg = ([(128, 163)] + [(128, 128)] * 3 + [(3, 128), (256, 191)] + [(256, 256)] * 4 +
           [(256, 447), (256, 256), (256, 256), (128, 411)] + [(128, 128)] * 3 +
           [(256, 256), (1, 256), (3, 128)])
    prm = _struct_with(L, L.AonMlpArtParams, 20, reg)
    with pytest.raises(ValueError, match=f"{F}: density_layer: weight 128 x 411"):
        L.call(F, *_args(L, prm=ctypes.byref(prm)))
    # a table the packs accept (per-sample columns only) has no latent columns to read
    for key, name, need in (("c0", "deformations_linear.0", 163), ("c5", "pts_linears.0", 191),
                            ("c10", "pts_linears.5", 447), ("c15", "views_linear.0", 411)):
        prm = _params(L, **{key: need - 1})
        with pytest.raises(ValueError, match=f"{F}: {name}: .*no latent columns.*>= {need}"):
            L.call(F, *_args(L, prm=ctypes.byref(prm)))
    prm = _struct_with(L, L.AonMlpArtParams, 20, L.ART_SHAPES)
    with pytest.raises(ValueError, match=f"{F}: .*no latent columns"):
        L.call(F, *_args(L, prm=ctypes.byref(prm)))
    # a null weight among the four that are read
    prm = _params(L)
    prm.pts_w[5] = None
    with pytest.raises(ValueError, match=f"{F}: pts_linears.5: null layer weight"):
        L.call(F, *_args(L, prm=ctypes.byref(prm)))


def test_workspace_bytes_positive_and_monotone(L):
    q = L.lib().aon_art_latent_grad_workspace_bytes
    sizes = [q(n) for n in (1, 15, 16, 17, 325, 4099, 16384, 16385, 100000, 1 << 22)]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert sizes[-1] == q(1 << 30)  # the group count is capped: so is the workspace
    assert q(0) == 0 and q(-5) == 0


def test_latent_codes_shapes_keys_and_init_round_trip():
    from aonerf import latent_fit

    codes = latent_fit.LatentCodes()
    out = codes()
    assert list(out) == ["density", "color", "articulation"]
    assert [tuple(out[k].shape) for k in out] == [(1, 128), (1, 128), (1, 32)]
    assert all(isinstance(out[k], torch.nn.Parameter) and out[k].requires_grad for k in out)
    assert len(list(codes.parameters())) == 3
    init = {"density": torch.randn(1, 128), "color": torch.randn(128),
            "articulation": torch.randn(1, 1, 32)}
    again = latent_fit.LatentCodes(init=init)()
    for k in init:
        assert again[k].shape[0] == 1 and torch.equal(again[k].detach().reshape(-1), init[k].reshape(-1))
        assert again[k].data_ptr() != init[k].data_ptr()  # copied: fitting leaves the library alone
    small = latent_fit.LatentCodes(n_shape=8, n_app=4, n_art=2)()
    assert [small[k].shape[1] for k in small] == [8, 4, 2]
    with pytest.raises(ValueError, match="articulation.*expected 32"):
        latent_fit.LatentCodes(init=dict(init, articulation=torch.zeros(1, 16)))


def test_init_from_code_library_row():
    from types import SimpleNamespace

    from aonerf import latent_fit
    from aonerf.code_library import CodeLibraryArticulated

    lib = CodeLibraryArticulated(SimpleNamespace(N_max_objs=4, N_obj_code_length=128))
    batch = {"instance_id": torch.tensor([2]), "articulation_id": torch.tensor([3])}
    row = lib(batch)
    codes = latent_fit.LatentCodes(init=row)()
    for k in row:
        assert torch.equal(codes[k].detach(), row[k].detach())
    table = lib.get_interpolated_articulations(2, "cpu")
    codes = latent_fit.LatentCodes(init=dict(row, articulation=table[5]))()
    assert torch.equal(codes["articulation"].detach()[0], table[5].detach())


def test_freeze_and_optimizer_cover_the_codes_only():
    from aonerf import latent_fit
    from aonerf.model_autodecoder import NeRF_AE_Art

    model = NeRF_AE_Art()
    assert latent_fit.freeze(model) is model
    assert not any(p.requires_grad for p in model.parameters())


def test_latent_only_refuses_a_trainable_mlp_before_the_gpu():
    """CPU tensors throughout: reaching any launch would raise 'MI355X only', not these."""
    from aonerf import latent_fit, train_art
    from aonerf.model_autodecoder import NeRFMLP
    from aonerf.numerics import TrainNumerics

    mlp = NeRFMLP(0, 10, 4)
    lat = latent_fit.LatentCodes()()
    rays = (torch.zeros(5, 3), torch.ones(5, 3), torch.ones(5, 3), torch.ones(5, 65))
    with pytest.raises(ValueError, match="latent_only.*requires grad"):
        train_art.render_level(mlp, *rays, True, lat, latent_only=True)
    next(mlp.parameters()).requires_grad_(False)  # one frozen tensor is not enough
    with pytest.raises(ValueError, match="latent_only.*requires grad"):
        train_art.render_level(mlp, *rays, True, lat, latent_only=True)
    latent_fit.freeze(mlp)
    with pytest.raises(ValueError, match="latent_only needs the fused backward"):
        train_art.render_level(mlp, *rays, True, lat, cfg=TrainNumerics(fused_backward=False),
                               latent_only=True)
    narrow = latent_fit.freeze(NeRFMLP(0, 10, 4, netwidth=128))
    with pytest.raises(ValueError, match="latent_only needs the fused backward"):
        train_art.render_level(narrow, *rays, True, lat, latent_only=True)
    # frozen and fused: the flag is accepted, and the first thing to object is the device
    with pytest.raises(ValueError, match="MI355X only"):
        train_art.render_level(mlp, *rays, True, lat, latent_only=True)
