"""CPU-side checks of the SSIM entry points (include/aonerf.h "evaluation"): both symbols are
exported and bound, the workspace query is pure host arithmetic, and aon_image_ssim refuses
every bad argument before any launch -- no GPU needed."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    from aonerf import _lib

    return _lib


def test_symbols_exported(L):
    lib = L.lib()
    for s in ("aon_ssim_workspace_bytes", "aon_image_ssim"):
        assert hasattr(lib, s) and s in L._SIGNATURES, s
    assert lib.aon_abi_version() == 13  # purely additive: no version change
    th, tw = L.ssim_tile()
    assert th >= 1 and tw >= 1


def test_workspace_query(L):
    ws = L.lib().aon_ssim_workspace_bytes
    th, tw = L.ssim_tile()
    shapes = [(11, 11), (11, 37), (37, 11), (24, 32), (2 * th + 13, 2 * tw + 17), (480, 640)]
    for h, w in shapes:
        sizes = [ws(n, h, w) for n in (1, 2, 3, 64)]
        assert sizes[0] > 0, (h, w)
        assert sizes == sorted(sizes), (h, w, sizes)
        # one fp64 partial per (image, tile) at least
        tiles = -(-(h - 10) // th) * -(-(w - 10) // tw)
        assert sizes[2] >= 3 * tiles * 8
    assert ws(1, 10, 32) == 0 and ws(1, 32, 10) == 0 and ws(-1, 24, 32) == 0


def test_bad_arguments_refused_before_any_launch(L):
    p = ctypes.c_void_p(16)
    ws = L.lib().aon_ssim_workspace_bytes(2, 24, 32)
    huge = ctypes.c_size_t(-1).value
    cases = {
        "null pred": (None, p, 2, 24, 32, p, None, p, ws, None),
        "null gt": (p, None, 2, 24, 32, p, None, p, ws, None),
        "null ssim": (p, p, 2, 24, 32, None, None, p, ws, None),
        "null work": (p, p, 2, 24, 32, p, None, None, ws, None),
        "height < 11": (p, p, 2, 10, 32, p, None, p, ws, None),
        "width < 11": (p, p, 2, 24, 10, p, None, p, ws, None),
        "negative count": (p, p, -1, 24, 32, p, None, p, ws, None),
        "negative height": (p, p, 2, -24, 32, p, None, p, ws, None),
        "negative width": (p, p, 2, 24, -32, p, None, p, ws, None),
        "work_bytes too small": (p, p, 2, 24, 32, p, None, p, ws - 1, None),
        "work_bytes zero": (p, p, 2, 24, 32, p, None, p, 0, None),
        "image count past the grid": (p, p, 1 << 20, 24, 32, p, None, p, huge, None),
        "tile rows past the grid": (p, p, 1, 1 << 26, 32, p, None, p, huge, None),
        "tile columns past the grid": (p, p, 1, 11, 1 << 50, p, None, p, huge, None),
    }
    lib = L.lib()
    for what, args in cases.items():
        rc = lib.aon_image_ssim(*args)
        msg = lib.aon_last_error().decode()
        assert rc < 0 and msg, (what, rc, msg)
        with pytest.raises(ValueError, match="aon_image_ssim"):
            L.call("aon_image_ssim", *args)


def test_zero_images_is_a_noop(L):
    """n_images == 0 is checked before the pointers: NULL everywhere returns 0, nothing runs."""
    assert L.lib().aon_image_ssim(None, None, 0, 24, 32, None, None, None, 0, None) == 0
    L.call("aon_image_ssim", None, None, 0, 0, 0, None, None, None, 0, None)
