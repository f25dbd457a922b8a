"""CPU-side checks of the two-pass render entry points (include/aonerf.h aon_mlp_fwd_sigma, the
density-only pass, and aon_mlp_fwd_cond, the forward on given per-ray view encodings): declared,
exported and bound, additive in ABI 13, and every refusal happens in argument validation -- the
pointers below are not device memory, so a launch that got past it would not return -1."""
import ctypes

import pytest

from test_capi import declared_symbols

NEW = ("aon_mlp_fwd_sigma", "aon_mlp_fwd_cond")
P = ctypes.c_void_p(16)  # non-null, 16-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def L():
    from aonerf import _lib

    return _lib


def _args(name, packed=P, prec=1, o=P, d=P, cond=P, t=P, B=4, S=8, act=0, out=P):
    mid = (o, d, t) if name == "aon_mlp_fwd_sigma" else (o, d, cond, t)
    return (packed, prec) + mid + (B, S, act, out, None)


def test_symbols_declared_exported_and_bound(L):
    lib = L.lib()
    for s in NEW:
        assert s in declared_symbols(), f"{s} not declared in aonerf.h"
        assert hasattr(lib, s) and s in L._SIGNATURES, s
    assert len(L._SIGNATURES["aon_mlp_fwd_sigma"][1]) == 10
    assert len(L._SIGNATURES["aon_mlp_fwd_cond"][1]) == 11


def test_abi_version_stays_13(L):
    assert L.lib().aon_abi_version() == 13 and L.ABI_VERSION == 13


@pytest.mark.parametrize("name", NEW)
def test_refuses_other_streams(L, name):
    with pytest.raises(ValueError, match=f"{name}.*AON_PREC_F16X3_TRAIN"):
        L.call(name, *_args(name, prec=L.PREC_F16X3_TRAIN))
    with pytest.raises(ValueError, match=f"{name}.*AON_PREC_BF16"):
        L.call(name, *_args(name, prec=L.PREC_BF16))
    # fp32 has no two-pass kernels: refused with a pointer to aon_mlp_fwd (NeRF.forward takes it)
    with pytest.raises(ValueError, match=f"{name}.*AON_PREC_FP32.*aon_mlp_fwd"):
        L.call(name, *_args(name, prec=L.PREC["fp32"]))
    with pytest.raises(ValueError, match=f"{name}.*unsupported precision"):
        L.call(name, *_args(name, prec=3))


@pytest.mark.parametrize("name", NEW)
def test_refuses_null_and_misaligned_pointers(L, name):
    keys = ["packed", "o", "d", "t", "out"] + (["cond"] if name == "aon_mlp_fwd_cond" else [])
    for k in keys:
        with pytest.raises(ValueError, match=f"{name}.*null pointer"):
            L.call(name, *_args(name, **{k: None}))
    for k in ("packed", "out"):
        with pytest.raises(ValueError, match=f"{name}.*16-byte aligned"):
            L.call(name, *_args(name, **{k: ctypes.c_void_p(24)}))


@pytest.mark.parametrize("name", NEW)
def test_refuses_bad_shapes_and_activations(L, name):
    with pytest.raises(ValueError, match=f"{name}.*bad shape"):
        L.call(name, *_args(name, S=0))
    with pytest.raises(ValueError, match=f"{name}.*bad shape"):
        L.call(name, *_args(name, B=-1))
    with pytest.raises(ValueError, match=f"{name}.*bad activation"):
        L.call(name, *_args(name, act=3))
    L.call(name, *_args(name, B=0))  # nothing to do: no launch, no error


def test_existing_precision_table_untouched(L):
    assert L.PREC == {"fp32": 0, "f16x3": 1}
    assert L.lib().aon_mlp_packed_bytes(L.PREC["f16x3"]) == 2112 * 1024 + 2208 * 4 + 16
