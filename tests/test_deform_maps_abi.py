"""CPU-side checks of the deformation-only pass and the feature compositor (include/aonerf.h
aon_mlp_art_fwd_deform, aon_mlp_art_fwd_deform_points, aon_composite_feat), in the pattern of
tests/test_capi.py: every call is refused, or has no rows, before any HIP call -- no GPU needed.
Every pointer is a fake non-null address (16; 20 = misaligned); a call wrong in two ways pins
which check comes first.  Also the stream layout the pass relies on and the two pure-torch
helpers (interface.canonical_to_rgb, helper.composite_features' shape checks)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

_P, _ODD = ctypes.c_void_p(16), ctypes.c_void_p(20)
_BIG = 1 << 38  # rows whose 128-row blocks reach 2^31
_AL = "packed / xp / delta must be 16-byte aligned"


@pytest.fixture(scope="module")
def L():
    from aonerf import _lib

    return _lib


def _run_cases(L, fn, base, cases):
    lib, wrong = L.lib(), []
    for over, want in cases:
        args = list(base)
        for i, v in over.items():
            args[i] = v
        st = getattr(lib, fn)(*args)
        msg = lib.aon_last_error().decode() if st else None
        if (st, msg) != ((-1, f"{fn}: {want}") if want is not None else (0, None)):
            wrong.append((over, st, msg, want))
    assert not wrong, f"{fn} (overrides, status, message, expected): {wrong}"


def test_symbols_declared_exported_and_bound(L):
    text = open(os.path.join(ROOT, "include", "aonerf.h")).read()
    for s in ("aon_mlp_art_fwd_deform", "aon_mlp_art_fwd_deform_points", "aon_composite_feat"):
        assert re.search(rf"\b{s}\s*\(", text), s
        assert hasattr(L.lib(), s) and s in L._SIGNATURES, s
    assert L.lib().aon_abi_version() == 13  # added without a version change


def test_deform_rays_refusals(L):
    # aon_mlp_art_fwd_deform(packed, rays_o, rays_d, t, B, S, xp, delta, stream)
    _run_cases(L, "aon_mlp_art_fwd_deform", [_P, _P, _P, _P, 4, 8, _P, _P, None], [
        ({0: None}, "null pointer"), ({1: None}, "null pointer"), ({2: None}, "null pointer"),
        ({3: None}, "null pointer"),
        ({6: None, 7: None}, "xp and delta are both null"),
        ({6: None, 4: 0}, None), ({7: None, 4: 0}, None),  # one output alone is a valid call
        ({5: 0}, "bad shape"), ({4: -1}, "bad shape"),
        ({0: _ODD}, _AL), ({6: _ODD}, _AL), ({7: _ODD}, _AL), ({6: None, 7: _ODD}, _AL),
        ({4: 0}, None), ({4: 0, 5: 193}, None),  # B * S == 0: nothing to do, nothing launched
        ({4: _BIG, 5: 1}, "too many rows"), ({4: 1 << 62, 5: 4}, "too many rows"),
        ({0: None, 6: None, 7: None}, "null pointer"),
        ({6: None, 7: None, 5: 0}, "xp and delta are both null"),
        ({5: 0, 0: _ODD}, "bad shape"), ({0: _ODD, 4: _BIG, 5: 1}, _AL)])


def test_deform_points_refusals(L):
    # aon_mlp_art_fwd_deform_points(packed, pos, N, xp, delta, stream)
    _run_cases(L, "aon_mlp_art_fwd_deform_points", [_P, _P, 5, _P, _P, None], [
        ({0: None}, "null pointer"), ({1: None}, "null pointer"),
        ({3: None, 4: None}, "xp and delta are both null"),
        ({2: -1}, "bad shape"), ({0: _ODD}, _AL), ({3: _ODD}, _AL), ({4: _ODD}, _AL),
        ({2: 0}, None), ({2: 0, 3: None}, None), ({2: 0, 4: None}, None),
        ({2: _BIG}, "too many rows"), ({2: -1, 3: _ODD}, "bad shape"),
        ({3: _ODD, 2: _BIG}, _AL)])


def test_composite_feat_refusals(L):
    # aon_composite_feat(weights, feat, feat_stride, C, B, S, out, stream)
    shape = "bad shape (1 <= S <= 512)"
    chan = "bad channel count (1 <= C <= 8)"
    _run_cases(L, "aon_composite_feat", [_P, _P, 4, 3, 4, 8, _P, None], [
        ({0: None}, "null pointer"), ({1: None}, "null pointer"), ({6: None}, "null pointer"),
        ({3: 0}, chan), ({3: 9}, chan), ({3: -1}, chan),
        ({5: 513}, shape), ({5: 0}, shape), ({4: -1}, shape),
        ({2: 2}, "feat_stride must be >= C"), ({2: 7, 3: 8}, "feat_stride must be >= C"),
        ({1: ctypes.c_void_p(18)}, "weights / feat / out must be 4-byte aligned"),
        ({4: 0}, None), ({4: 0, 5: 512, 3: 8, 2: 8}, None),
        ({3: 9, 5: 513}, chan), ({5: 513, 2: 2}, shape), ({0: None, 3: 0}, "null pointer")])


def test_deformation_prefix_of_the_articulated_stream():
    """The numbers mlp_layout.hpp pins for the deformation-only prefix, restated from the shape
    table as build_layout sums them: the deformation MLP is the first 216 blocks (224 with the
    16-block ring's padding) and 528 bias rows of the stream, where pts_linears.0 begins."""
    text = open(os.path.join(ROOT, "articulated-object-nerf_amd", "csrc", "mlp_layout.hpp")).read()
    body = text[text.index("constexpr LayerShape kShapeArt[kNumLayersArt]"):]
    rows = re.findall(r"\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\}", body)[:5]
    assert len(rows) == 5
    blk = bias = 0
    for ka, kb, u, _, _, _ in (tuple(map(int, r)) for r in rows):
        blk, bias = blk + (ka + kb) * u * 2, bias + 16 * u
    assert (blk, bias) == (216, 528)
    assert "using NetArtDeformH = Prefix<NetArtH, A_DOUT + 1, 16>;" in text
    assert "static_assert(net_is<NetArtDeformH>(216, 224, 528)" in text
    assert "constexpr StreamMap kArtMix{2, 0, NetArtH::layer(A_P0).blk0};" in text
    assert "kArtMix.hi == 216" in text


def test_canonical_to_rgb():
    from aonerf import interface

    canon = torch.tensor([[0.5, -0.5, 0.0], [4.0, -4.0, 0.2], [0.0, 0.0, 0.0], [0.3, 0.0, 0.0]])
    acc = torch.tensor([1.0, 0.5, 0.0, 0.5])
    white = interface.canonical_to_rgb(canon, acc, box_side_length=2, white_bkgd=True)
    black = interface.canonical_to_rgb(canon, acc, box_side_length=2, white_bkgd=False)
    assert torch.allclose(white[0], torch.tensor([0.75, 0.25, 0.5]))
    # normalised by acc, clipped to the box, blended by acc
    assert torch.allclose(black[1], torch.tensor([0.5, 0.0, 0.35]))
    assert torch.allclose(white[1], torch.tensor([1.0, 0.5, 0.85]))
    assert torch.equal(white[2], torch.ones(3)) and torch.equal(black[2], torch.zeros(3))
    assert torch.allclose(black[3], torch.tensor([0.4, 0.25, 0.25]))
    assert float(white.min()) >= 0.0 and float(white.max()) <= 1.0
    img = interface.canonical_to_rgb(torch.zeros(2, 3, 3), torch.ones(2, 3))
    assert tuple(img.shape) == (2, 3, 3)


def test_composite_features_refuses_cpu_tensors():
    from aonerf import helper

    with pytest.raises(ValueError, match="MI355X only"):
        helper.composite_features(torch.zeros(2, 5), torch.zeros(2, 5, 3))
