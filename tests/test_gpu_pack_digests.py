"""Every packed weight stream, byte for byte: the SHA-256 of each pack entry point's whole buffer
(stream, bias table and status block) against tests/golden/pack_digests.json, recorded from the
library as it stood before csrc/mlp_layout.hpp derived its layer tables from shape tables.  The
packs place every weight by the tables' blk0 / bias0, so one moved offset changes a digest.

The parameters come from a closed integer formula (no RNG, no library version in the values):
element i of tensor k is ((i * 2654435761 + k * 40503) mod 2^32) / 2^32 - 0.5, times 0.2, formed
in float64 and rounded to float32; k = the layer's index for its weight, 100 + that for its bias.
The four latent-carrying articulated layers are 17 / 33 / 33 / 9 columns wider than their
per-sample inputs.  Buffers start zeroed: the compact (bf16, mixed) streams leave their tail
unwritten.

AONERF_RECORD_PACK_DIGESTS=<file> writes the digests there instead of comparing them.
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "pack_digests.json")
ART_LATENT_COLS = {0: 17, 5: 33, 10: 33, 15: 9}


def _tensor(k, *shape):
    i = np.arange(int(np.prod(shape)), dtype=np.uint64)
    v = (i * np.uint64(2654435761) + np.uint64(k * 40503)) & np.uint64(0xFFFFFFFF)
    x = (v.astype(np.float64) / 2.0 ** 32 - 0.5) * 0.2
    return torch.from_numpy(x.astype(np.float32).reshape(shape)).cuda()


def _pairs(shapes, wider=None):
    return [(_tensor(k, out, inp + (wider or {}).get(k, 0)), _tensor(100 + k, out))
            for k, (out, inp) in enumerate(shapes)]


def _digest(L, size, fn, *args):
    buf = torch.zeros(size, dtype=torch.uint8, device="cuda")
    L.call(fn, *args, L.ptr(buf), L.stream())
    torch.cuda.synchronize()
    return hashlib.sha256(buf.cpu().numpy().tobytes()).hexdigest()


def test_pack_digests():
    from aonerf import _lib as L

    lib = L.lib()
    van, art = _pairs(L.MLP_SHAPES), _pairs(L.ART_SHAPES, ART_LATENT_COLS)
    pv, pa = L.ctypes.byref(L.mlp_params(van)), L.ctypes.byref(L.mlp_art_params(art))
    got = {}
    for prec in (0, 1, 2, 4):
        got[f"aon_mlp_pack/{prec}"] = _digest(L, lib.aon_mlp_packed_bytes(prec), "aon_mlp_pack",
                                              pv, prec)
    for fn in ("aon_mlp_bwd_pack", "aon_mlp_bwd_pack_bf16"):
        got[fn] = _digest(L, lib.aon_mlp_bwd_packed_bytes(), fn, pv)
    got["aon_mlp_art_pack"] = _digest(L, lib.aon_mlp_art_packed_bytes(), "aon_mlp_art_pack", pa)
    for mixed in (1, 2, 3):
        got[f"aon_mlp_art_pack_mixed/{mixed}"] = _digest(L, lib.aon_mlp_art_packed_bytes(),
                                                         "aon_mlp_art_pack_mixed", pa, mixed)
    for fn in ("aon_mlp_art_bwd_pack", "aon_mlp_art_bwd_pack_bf16"):
        got[fn] = _digest(L, lib.aon_mlp_art_bwd_packed_bytes(), fn, pa)
    assert len(set(got.values())) == len(got), "two packs gave the same bytes"

    record = os.environ.get("AONERF_RECORD_PACK_DIGESTS")
    if record:
        with open(record, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    with open(FIXTURE) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    wrong = [k for k in sorted(got) if got[k] != want[k]]
    assert not wrong, f"packed bytes changed: {wrong}"
