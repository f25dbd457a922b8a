"""CPU-side checks of the box-bound entry points (include/aonerf.h: aon_ray_limits_box,
aon_ray_limits, aon_sample_along_rays_bounds, aon_compact_rays, aon_scatter_payload and the two
workspace queries): declared, exported and bound, additive in ABI 13, and every refusal -- a
null pointer, B < 0, S < 2, a non-positive half_side -- happens in argument validation: the
pointers below are not device memory, so a launch that got past it would not return -1."""
import ctypes

import pytest

from test_capi import declared_symbols

NEW = ("aon_ray_limits_box", "aon_ray_limits_workspace_bytes", "aon_ray_limits",
       "aon_sample_along_rays_bounds", "aon_compact_rays_workspace_bytes", "aon_compact_rays",
       "aon_scatter_payload")
P = ctypes.c_void_p(16)  # non-null, aligned, never dereferenced


@pytest.fixture(scope="module")
def L():
    from aonerf import _lib

    return _lib


def box_args(o=P, d=P, B=4, half=1.0, tmin=P, tmax=P):
    return (o, d, B, half, tmin, tmax, None)


def limits_args(L, o=P, d=P, B=4, half=1.0, near=P, far=P, work=P, nbytes=None):
    nbytes = L.lib().aon_ray_limits_workspace_bytes(4) if nbytes is None else nbytes
    return (o, d, B, half, near, far, work, nbytes, None)


def sample_args(o=P, d=P, B=4, S=9, s_tab=P, near=P, far=P, lindisp=0, u=None, t=P, xyz=None):
    return (o, d, B, S, s_tab, near, far, lindisp, u, t, xyz, None)


def compact_args(L, B=4, nbytes=None, **kw):
    names = ("tmin", "tmax", "rays_o", "rays_d", "viewdirs")
    outs = ("slot", "idx", "o_out", "d_out", "v_out", "near_out", "far_out", "n_hit", "work")
    nbytes = L.lib().aon_compact_rays_workspace_bytes(4) if nbytes is None else nbytes
    return (tuple(kw.get(k, P) for k in names) + (B,) + tuple(kw.get(k, P) for k in outs)
            + (nbytes, None))


def scatter_args(comp=P, acc=P, depth=P, n=2, slot=P, B=4, white=1, out=P):
    return (comp, acc, depth, n, slot, B, white, out, None)


def test_symbols_declared_exported_and_bound(L):
    lib = L.lib()
    for s in NEW:
        assert s in declared_symbols(), f"{s} not declared in aonerf.h"
        assert hasattr(lib, s) and s in L._SIGNATURES, s
    assert len(L._SIGNATURES["aon_ray_limits_box"][1]) == 7
    assert len(L._SIGNATURES["aon_sample_along_rays_bounds"][1]) == 12
    assert len(L._SIGNATURES["aon_compact_rays"][1]) == 17


def test_abi_version_stays_13(L):
    assert L.lib().aon_abi_version() == 13 and L.ABI_VERSION == 13


def test_header_cites_the_reference_lines():
    from test_capi import HEADER

    text = open(HEADER).read()
    for cite in ("helper.py:42-102", "helper.py:29-39", "helper.py:116-129"):
        assert cite in text, cite


def test_ray_limits_box_refusals(L):
    name = "aon_ray_limits_box"
    for k in ("o", "d", "tmin", "tmax"):
        with pytest.raises(ValueError, match=f"{name}.*null pointer"):
            L.call(name, *box_args(**{k: None}))
    with pytest.raises(ValueError, match=f"{name}.*B outside"):
        L.call(name, *box_args(B=-1))
    for half in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match=f"{name}.*half_side"):
            L.call(name, *box_args(half=half))
    L.call(name, *box_args(B=0))  # nothing to do: no launch, no error


def test_ray_limits_refusals(L):
    name = "aon_ray_limits"
    for k in ("o", "d", "near", "far", "work"):
        with pytest.raises(ValueError, match=f"{name}.*null pointer"):
            L.call(name, *limits_args(L, **{k: None}))
    with pytest.raises(ValueError, match=f"{name}.*B outside"):
        L.call(name, *limits_args(L, B=-1))
    with pytest.raises(ValueError, match=f"{name}.*half_side"):
        L.call(name, *limits_args(L, half=0.0))
    with pytest.raises(ValueError, match=f"{name}.*work_bytes"):
        L.call(name, *limits_args(L, nbytes=L.lib().aon_ray_limits_workspace_bytes(4) - 1))
    L.call(name, *limits_args(L, B=0))


def test_sampler_refusals(L):
    name = "aon_sample_along_rays_bounds"
    for k in ("s_tab", "near", "far", "t"):
        with pytest.raises(ValueError, match=f"{name}.*null pointer"):
            L.call(name, *sample_args(**{k: None}))
    with pytest.raises(ValueError, match=f"{name}.*B < 0"):
        L.call(name, *sample_args(B=-1))
    for S in (1, 0, -3):
        with pytest.raises(ValueError, match=f"{name}.*S < 2"):
            L.call(name, *sample_args(S=S))
    with pytest.raises(ValueError, match=f"{name}.*xyz needs"):
        L.call(name, *sample_args(o=None, xyz=P))
    L.call(name, *sample_args(B=0))


def test_compact_and_scatter_refusals(L):
    name = "aon_compact_rays"
    for k in ("tmin", "tmax", "rays_o", "rays_d", "slot", "idx", "o_out", "d_out", "near_out",
              "far_out", "n_hit", "work"):
        with pytest.raises(ValueError, match=f"{name}.*null pointer"):
            L.call(name, *compact_args(L, **{k: None}))
    with pytest.raises(ValueError, match=f"{name}.*go together"):
        L.call(name, *compact_args(L, v_out=None))
    with pytest.raises(ValueError, match=f"{name}.*B outside"):
        L.call(name, *compact_args(L, B=-1))
    with pytest.raises(ValueError, match=f"{name}.*work_bytes"):
        L.call(name, *compact_args(L, nbytes=0))
    name = "aon_scatter_payload"
    for k in ("comp", "acc", "depth", "slot", "out"):
        with pytest.raises(ValueError, match=f"{name}.*null pointer"):
            L.call(name, *scatter_args(**{k: None}))
    with pytest.raises(ValueError, match=f"{name}.*B outside"):
        L.call(name, *scatter_args(B=-1))
    L.call(name, *scatter_args(B=0))


def test_workspace_queries(L):
    lib = L.lib()
    for q in (lib.aon_ray_limits_workspace_bytes, lib.aon_compact_rays_workspace_bytes):
        assert q(-1) == 0 and q(1 << 31) == 0
        assert 0 < q(0) <= q(1) == q(256) < q(257) <= q(307200)
        assert q(307200) < 64 * 1024  # a few bytes per 256-ray workgroup


def test_python_layer_refuses_before_the_library():
    import torch
    from aonerf import helper

    o = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="MI355X only"):
        helper.get_ray_limits_box(o, o, 2)
    with pytest.raises(ValueError, match="MI355X only"):
        helper.get_ray_limits(o, o)
