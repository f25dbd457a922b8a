"""CPU-side checks of the folded render stream's ABI (include/aonerf.h AON_PREC_F16X3 /
AON_PREC_F16X3_TRAIN): sizes per precision and the render entry points' refusal of the training
stream -- argument validation only, no GPU."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "aonerf.h")


@pytest.fixture(scope="module")
def L():
    from aonerf import _lib

    return _lib


def test_precision_values_match_the_header(L):
    text = open(HEADER).read()
    vals = {k: int(v) for k, v in re.findall(r"#define (AON_PREC_\w+) (\d+)", text)}
    assert vals == {"AON_PREC_FP32": 0, "AON_PREC_F16X3": 1, "AON_PREC_BF16": 2,
                    "AON_PREC_F16X3_TRAIN": 4}
    assert L.PREC == {"fp32": 0, "f16x3": 1}
    assert L.PREC_F16X3_TRAIN == 4 and L.PREC_BF16 == 2


def test_packed_sizes(L):
    """1-KB blocks padded to 64, 16 floats of bias per output tile, a 16-B status block: the
    unfolded streams 2,344 -> 2,368 blocks and 2,464 bias floats; the render stream without the
    bottleneck's 256 blocks and 256 bias floats, 2,088 -> 2,112 and 2,208."""
    lib = L.lib()
    unfolded = 2368 * 1024 + 2464 * 4 + 16
    assert lib.aon_mlp_packed_bytes(0) == unfolded
    assert lib.aon_mlp_packed_bytes(L.PREC_F16X3_TRAIN) == unfolded
    assert lib.aon_mlp_packed_bytes(L.PREC_BF16) == unfolded
    assert lib.aon_mlp_packed_bytes(L.PREC["f16x3"]) == 2112 * 1024 + 2208 * 4 + 16


@pytest.mark.parametrize("name,tail", [
    ("aon_mlp_fwd", (ctypes.c_void_p(16),) * 4),
    ("aon_mlp_fwd_encoded", (ctypes.c_void_p(16),) * 2),
])
def test_render_refuses_the_training_stream(L, name, tail):
    p = ctypes.c_void_p(16)
    with pytest.raises(ValueError, match=f"{name}.*AON_PREC_F16X3_TRAIN"):
        L.call(name, p, L.PREC_F16X3_TRAIN, *tail, 4, 8, 0, p, None)
