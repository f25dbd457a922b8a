"""Packed sizes of every weight stream, as the C ABI reports them (no GPU): csrc/mlp_layout.hpp
derives each stream's block and bias counts from its shape table, and a caller allocates by
these queries -- so the derived totals are pinned here to the values of ABI 13."""
import pytest


def _bytes(stream_blocks, bias_floats):
    """1-KB blocks, the bias table, the 16-B status block."""
    return stream_blocks * 1024 + bias_floats * 4 + 16


UNFOLDED = _bytes(2368, 2464)  # 2,344 blocks carry weights


@pytest.mark.parametrize("precision,want", [
    (0, UNFOLDED), (2, UNFOLDED), (4, UNFOLDED),
    (1, _bytes(2112, 2208)),  # the folded render stream: 2,088 blocks
])
def test_vanilla_packed_bytes(precision, want):
    from aonerf import _lib as L

    assert L.lib().aon_mlp_packed_bytes(precision) == want


@pytest.mark.parametrize("query,want", [
    ("aon_mlp_bwd_packed_bytes", _bytes(2240, 2432)),      # 2,224 blocks
    ("aon_mlp_art_packed_bytes", _bytes(2752, 3376)),      # 2,752 blocks
    ("aon_mlp_art_bwd_packed_bytes", _bytes(2752, 3456)),  # 2,752 blocks
])
def test_chain_packed_bytes(query, want):
    from aonerf import _lib as L

    assert getattr(L.lib(), query)() == want
