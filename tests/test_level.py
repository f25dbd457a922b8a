"""Host logic of aonerf.level, what the vanilla and the articulated training paths share: the
pack-buffer cache (on CPU stand-in buffers, as tests/test_range_bookkeeping.py: no kernel runs,
the status words are set by hand) and the table from weight-gradient operands to aon_gemm
keywords (written out from a launch trace of the two paths before they shared it)."""
import ctypes

import pytest
import torch


@pytest.fixture
def env(monkeypatch):
    from aonerf import _lib as L
    from aonerf import level

    dicts = (L.PENDING_PACKS, L._STICKY, L.PACK_PARAMS, L.SNAPSHOTS)
    for d in dicts:
        d.clear()
    monkeypatch.setattr(level, "_packed", {})
    seen = []
    register = L.register_pack
    monkeypatch.setattr(L, "register_pack", lambda key, buf, params=(): (
        seen.append((key, buf)), register(key, buf, params))[1])
    yield L, level, seen
    for d in dicts:
        d.clear()


def test_namespaces_keep_their_own_buffers(env):
    """The same key and device in the two namespaces: two buffers of their own sizes (vanilla
    "fwd64" and articulated "fwd64" are different streams); a second request returns the same
    buffer; the range guard sees ("train", key) / ("train_art", key)."""
    L, level, seen = env
    a = level.buffer("train", "fwd64", 256, "cpu", guard=True)
    b = level.buffer("train_art", "fwd64", 1024, "cpu", guard=True)
    assert a is not b and a.numel() == 64 and b.numel() == 256
    assert a.dtype == torch.float32
    assert [k for k, _ in seen] == [("train", "fwd64"), ("train_art", "fwd64")]
    assert seen[0][1] is a and seen[1][1] is b
    assert set(L.PENDING_PACKS) == {("train", "fwd64", "cpu"), ("train_art", "fwd64", "cpu")}
    assert level.buffer("train", "fwd64", 256, "cpu", guard=True) is a
    assert level.buffer("train_art", "fwd64", 1024, "cpu", guard=True) is b
    # the scale word: one per namespace and device, never registered with the guard
    n = len(seen)
    w = level.buffer("train", "work", 4, "cpu")
    assert w.numel() == 1 and level.buffer("train", "work", 4, "cpu") is w
    assert level.buffer("train_art", "work", 4, "cpu") is not w
    assert len(seen) == n and not any(k[1] == "work" for k in L.PENDING_PACKS)


def test_repack_of_pending_buffer_goes_sticky(env):
    """A buffer requested again before an optimizer step looked at it: its status word is kept
    (the sticky path of register_pack), whatever the re-pack then writes."""
    L, level, _ = env
    p = torch.nn.Parameter(torch.ones(3))
    buf = level.buffer("train_art", "bwd65", 64, "cpu", guard=True, params=[p])
    buf.view(torch.int32)[-4] = 1                 # a kernel met an overflow
    assert level.buffer("train_art", "bwd65", 64, "cpu", guard=True, params=[p]) is buf
    buf.view(torch.int32)[-4] = 0                 # what the re-pack does to the status word
    assert any(sk[0] == "cpu" for sk in L._STICKY)
    assert L.check_pending({"cpu"}, {p.data_ptr()}) is True
    assert not L._STICKY and not L.PENDING_PACKS


def test_pack_bwd_names(env, monkeypatch):
    """pack_bwd: the namespace's "bwd[bf]<tag>" buffer of the queried size, guarded in f16x3
    only, packed by ``entry`` / ``entry``_bf16."""
    L, level, seen = env
    calls = []
    monkeypatch.setattr(L, "call", lambda name, *a: calls.append(name))
    monkeypatch.setattr(L, "stream", lambda dev=None: None)
    P = [(torch.ones(2, 2), torch.ones(2))]
    struct = lambda P: ctypes.c_int(0)  # noqa: E731
    a = level.pack_bwd("train", "aon_mlp_bwd_pack", lambda: 512, struct, P, "cpu", 64)
    b = level.pack_bwd("train_art", "aon_mlp_art_bwd_pack", lambda: 2048, struct, P, "cpu", 64,
                       bf16=True)
    assert calls == ["aon_mlp_bwd_pack", "aon_mlp_art_bwd_pack_bf16"]
    assert a.numel() == 128 and b.numel() == 512
    assert [k for k, _ in seen] == [("train", "bwd64")]  # bf16 streams carry no range guard
    assert L.PACK_PARAMS[("train", "bwd64", "cpu")] == {t.data_ptr() for t in P[0]}
    assert set(level._packed) == {("train", "bwd64", "cpu"), ("train_art", "bwdbf64", "cpu")}


# (bf16, dY kind, dY tiled, dY ld, X kind, X tiled, X ld, n_out) ->
# (n_in, n_store, a_scale, b_scale, a_amax is the chain's word, f16_single): every pair the
# launch trace of the two training paths shows (fused backward after the fused f16x3 forward,
# after the bf16 forward, and after the layer-by-layer forward), before they shared this table
A, G = 2.0 ** -8, 2.0 ** 10
TABLE = [
    # fused f16x3 forward: kept tensors tiled
    (False, "draw", False, 4, "act", True, 128, 3, (128, 0, 1.0, A, True, False)),
    (False, "draw_sigma", False, 4, "act", True, 256, 1, (256, 0, 1.0, A, True, False)),
    (False, "chain", True, 128, "act", True, 256, 128, (256, 0, 1.0, 8.0, True, True)),
    (False, "chain", True, 256, "act", True, 256, 256, (256, 0, 1.0, 8.0, True, True)),
    (False, "chain", True, 128, "act", True, 128, 128, (128, 0, 1.0, A, True, False)),
    (False, "chain", True, 256, "enc_t64", True, 64, 256, (64, 63, 1.0, 8.0, True, True)),
    (False, "chain", True, 128, "venc", False, 27, 128, (27, 0, 1.0, A, True, False)),
    (False, "dxp", False, 3, "act", True, 128, 3, (128, 0, G, A, False, False)),
    (False, "chain_def", True, 128, "act", True, 128, 128, (128, 0, G, A, False, False)),
    (False, "chain_def", True, 128, "xyz", False, 3, 128, (3, 0, G, A, False, False)),
    # layer-by-layer forward: kept tensors and pos_enc(x) row-major
    (False, "draw", False, 4, "act", False, 128, 3, (128, 0, 1.0, A, True, False)),
    (False, "draw_sigma", False, 4, "act", False, 256, 1, (256, 0, 1.0, A, True, False)),
    (False, "chain", True, 128, "act", False, 256, 128, (256, 0, 1.0, A, True, False)),
    (False, "chain", True, 256, "act", False, 256, 256, (256, 0, 1.0, A, True, False)),
    (False, "chain", True, 128, "act", False, 128, 128, (128, 0, 1.0, A, True, False)),
    (False, "chain", True, 256, "enc63", False, 63, 256, (63, 0, 1.0, A, True, False)),
    (False, "dxp", False, 3, "act", False, 128, 3, (128, 0, G, A, False, False)),
    (False, "chain_def", True, 128, "act", False, 128, 128, (128, 0, G, A, False, False)),
    # bf16 forward: one bf16 MFMA per product, no scales
    (True, "draw", False, 4, "act", True, 128, 3, (128, 0, 1.0, 1.0, False, False)),
    (True, "draw_sigma", False, 4, "act", True, 256, 1, (256, 0, 1.0, 1.0, False, False)),
    (True, "chain", True, 128, "act", True, 256, 128, (256, 0, 1.0, 1.0, False, False)),
    (True, "chain", True, 256, "act", True, 256, 256, (256, 0, 1.0, 1.0, False, False)),
    (True, "chain", True, 128, "act", True, 128, 128, (128, 0, 1.0, 1.0, False, False)),
    (True, "chain", True, 256, "enc_t128_bf", True, 128, 256, (128, 63, 1.0, 1.0, False, False)),
    (True, "chain", True, 128, "venc", False, 27, 128, (27, 0, 1.0, 1.0, False, False)),
    (True, "dxp", False, 3, "act", True, 128, 3, (128, 0, 1.0, 1.0, False, False)),
    (True, "chain_def", True, 128, "act", True, 128, 128, (128, 0, 1.0, 1.0, False, False)),
]


@pytest.mark.parametrize("row", TABLE, ids=lambda r: f"{'bf16' if r[0] else 'f16x3'}-{r[1]}-"
                         f"{r[4]}{'T' if r[5] else ''}-{r[7]}x{r[6]}")
def test_dweight_keywords(row):
    from aonerf import level

    bf16, ak, at, ald, bk, bt, bld, n_out, want = row
    a, b = level.Operand(None, ald, at, ak), level.Operand(None, bld, bt, bk)
    assert {ak, bk} <= {level.CHAIN, level.CHAIN_DEF, level.DRAW, level.DRAW_SIGMA, level.DXP,
                        level.ACT, level.ENC63, level.ENC_T64, level.ENC_T128_BF, level.VENC,
                        level.XYZ}
    work = object()
    kw = level.dweight_kwargs(a, b, n_out, bf16, work)
    n_in, n_store, a_scale, b_scale, amax, single = want
    assert kw == dict(n_in=n_in, ldb=bld, a_tiled=at, b_tiled=bt, n_store=n_store,
                      f16_single=single, a_scale=a_scale, b_scale=b_scale,
                      a_amax=work if amax else None, mma_bf16=bf16)
