"""CPU-side checks of the C ABI: the library loads, exports every symbol include/aonerf.h
declares, and rejects invalid arguments with the documented status/message -- all without
touching a GPU (argument validation happens before any HIP call)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "aonerf.h")


def declared_symbols():
    text = open(HEADER).read()
    return sorted(set(re.findall(r"\b(aon_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def L():
    from aonerf import _lib

    return _lib


def test_header_symbols_exported(L):
    lib = L.lib()
    syms = declared_symbols()
    assert len(syms) >= 12
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in aonerf.h but not exported"
    assert set(syms) <= set(L._SIGNATURES), "ctypes binding misses a declared entry point"


def test_abi_version_and_sizes(L):
    lib = L.lib()
    assert lib.aon_abi_version() == L.ABI_VERSION == 13
    # precision 3 (ABI 12's 32x32x16 render stream) is withdrawn: no packed size
    assert lib.aon_mlp_packed_bytes(3) == 0
    assert lib.aon_mlp_packed_bytes(99) == 0


@pytest.mark.parametrize("name,args", [
    ("aon_composite_fwd", (None, 3, None, 1, None, None, 4, 8, 1, 1, None, None, None, None, None)),
    ("aon_sample_pdf", (None, 0, None, 0, 4, 1, 128, None, 0, None, 0, None, None, None, None, None)),
    ("aon_mlp_fwd", (None, 0, None, None, None, None, 4, 8, 0, None, None)),
    ("aon_pos_enc", (None, 4, 0, 10, None, None)),
    ("aon_frame_rays", (0, 4, 1.0, None, 0, 0, None, None, None, None)),
])
def test_invalid_arguments_raise(L, name, args):
    with pytest.raises(ValueError, match=name):
        L.call(name, *args)


def test_abi10_argument_checks(L):
    """ABI 10's new entry points refuse bad arguments before any launch (no GPU needed):
    aon_cast_rays_tiled's width (a multiple of 16 holding every encoding), the articulated bf16
    forward's `mixed` range and aon_gemm's n_store on an exact-fp32 tiny product."""
    p = ctypes.c_void_p(16)
    with pytest.raises(ValueError, match="width"):
        L.call("aon_cast_rays_tiled", p, p, p, 4, 8, 0, 10, 48, p, None)  # 63 encodings > 48
    with pytest.raises(ValueError, match="width"):
        L.call("aon_cast_rays_tiled", p, p, p, 4, 8, 0, 10, 72, p, None)  # not a multiple of 16
    with pytest.raises(ValueError, match="bad arguments"):
        L.call("aon_cast_rays_tiled", None, p, p, 4, 8, 0, 10, 64, p, None)
    with pytest.raises(ValueError, match="mixed"):
        L.call("aon_mlp_art_fwd_train_bf16", p, p, p, p, p, 1, 1, None, p, p, p, p, p, p, p, p, p,
               5, None)
    with pytest.raises(ValueError, match="mixed"):
        L.call("aon_mlp_art_pack_mixed", None, 4, p, None)
    a = L.AonGemmArgs(M=2, N=4, K=3, A=16, lda=3, a_kc=1, B=16, ldb=4, b_kc=0, b_rdiv=1, C=16,
                      ldc=4, a_scale=1.0, b_scale=1.0, exact_fp32=1, n_store=2)
    with pytest.raises(ValueError, match="n_store"):
        L.call("aon_gemm", ctypes.byref(a), None, 0, None)


def test_abi11_argument_checks(L):
    """ABI 11: the articulated training forward keeps pos_enc(x') tiled with 16-byte stores, so
    enc must be 16-byte aligned, and the bf16 entry requires enc_bf (its fp32 enc keeps x' only)."""
    p, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    with pytest.raises(ValueError, match="enc_bf"):
        L.call("aon_mlp_art_fwd_train_bf16", p, p, p, p, p, 1, 1, None, p, p, p, p, p, p, p, p,
               None, 4, None)
    with pytest.raises(ValueError, match="enc must be 16-byte aligned"):
        L.call("aon_mlp_art_fwd_train", p, p, p, p, p, 1, 1, None, p, p, p, p, odd, p, p, p, None)
    with pytest.raises(ValueError, match="16-byte aligned"):
        L.call("aon_mlp_art_bwd", p, p, p, odd, 1, p, p, p, p, p, p, None)


def test_pdf_shape_limits(L):
    with pytest.raises(ValueError, match="bad shape"):
        L.call("aon_sample_pdf", ctypes.c_void_p(16), 0, ctypes.c_void_p(16), 0, 4, 1000, 128,
               ctypes.c_void_p(16), 0, None, 0, None, None, ctypes.c_void_p(16), None, None)


def test_cpu_tensors_rejected():
    import torch
    from aonerf import helper

    with pytest.raises(ValueError, match="MI355X only"):
        helper.pos_enc(torch.zeros(4, 3), 0, 10)


def _fake_pairs(shapes):
    """(weight, bias) stand-ins with the given shapes: the C side only reads the shape fields
    before it refuses, so the pointers are never dereferenced."""
    import torch

    return [(torch.empty(o, i), torch.empty(o)) for o, i in shapes]


def _struct_with(L, cls, n, shapes):
    prm = cls()
    for i, (o, k) in enumerate(shapes):
        prm.w_rows[i], prm.w_cols[i], prm.b_len[i] = o, k, o
    # every pointer non-null: only the shape check stands between the struct and a launch
    for name, typ in cls._fields_:
        if name.endswith(("_w", "_b")):
            v = getattr(prm, name)
            if isinstance(v, int) or v is None:
                setattr(prm, name, 16)
            else:
                for j in range(len(v)):
                    v[j] = 16
    return prm


def _registration_order(mlp):
    ps = list(mlp.parameters())
    return [(ps[2 * i], ps[2 * i + 1]) for i in range(len(ps) // 2)]


def test_registration_order_rejected_python(L):
    """nn.Module.parameters() in registration order (pts_linears, views_linear,
    bottleneck, density, rgb) is not the kernels' layer order.  The Python builders refuse it
    with ValueError naming the layer -- before any pointer exists -- for both MLPs, and the
    training path's _params_struct (train.py / train_art.py) goes through them."""
    from aonerf import train, train_art
    from aonerf.model import NeRFMLP
    from aonerf.model_autodecoder import NeRFMLP as ArtMLP

    mlp = NeRFMLP(0, 10, 4)
    reg = _registration_order(mlp)
    with pytest.raises(ValueError, match="density_layer.*layer order"):
        L.mlp_params(reg)
    with pytest.raises(ValueError, match="density_layer.*layer order"):
        train._params_struct(reg)
    # the kernels' order passes the shape check (and then needs GPU tensors)
    good = [(m.weight, m.bias) for m in mlp._layers()]
    with pytest.raises(ValueError, match="GPU tensor"):
        L.mlp_params(good)
    with pytest.raises(ValueError, match="12 \\(weight, bias\\) pairs"):
        L.mlp_params(good[:11])
    art = ArtMLP(0, 10, 4)
    reg = _registration_order(art)
    with pytest.raises(ValueError, match="density_layer.*layer order"):
        L.mlp_art_params(reg)
    with pytest.raises(ValueError, match="density_layer.*layer order"):
        train_art._params_struct(reg)
    good = [(m.weight, m.bias) for m in train_art.art_layers(art)]
    with pytest.raises(ValueError, match="GPU tensor"):
        L.mlp_art_params(good)


def test_registration_order_rejected_c(L):
    """The same refusal on the C side (aon_mlp_params / aon_mlp_art_params carry the shapes,
    ABI 9): every pack returns < 0 naming the layer before any launch -- no GPU needed."""
    reg = [(256, 63)] + [(256, 256)] * 4 + [(256, 319), (256, 256), (256, 256), (128, 283),
                                             (256, 256), (1, 256), (3, 128)]
    prm = _struct_with(L, L.AonMlpParams, 12, reg)
    for fn, args in (("aon_mlp_pack", (1, ctypes.c_void_p(16), None)),
                     ("aon_mlp_bwd_pack", (ctypes.c_void_p(16), None)),
                     ("aon_mlp_bwd_pack_bf16", (ctypes.c_void_p(16), None))):
        with pytest.raises(ValueError, match=f"{fn}: density_layer: weight 128 x 283"):
            L.call(fn, ctypes.byref(prm), *args)
    art_reg = ([(128, 163)] + [(128, 128)] * 3 + [(3, 128), (256, 191)] + [(256, 256)] * 4 +
               [(256, 447), (256, 256), (256, 256), (128, 411)] + [(128, 128)] * 3 +
               [(256, 256), (1, 256), (3, 128)])
    prm = _struct_with(L, L.AonMlpArtParams, 20, art_reg)
    for fn in ("aon_mlp_art_pack", "aon_mlp_art_pack_bf16", "aon_mlp_art_bwd_pack",
               "aon_mlp_art_bwd_pack_bf16"):
        with pytest.raises(ValueError, match=f"{fn}: density_layer: weight 128 x 411"):
            L.call(fn, ctypes.byref(prm), ctypes.c_void_p(16), None)
    # a latent-carrying layer narrower than its per-sample columns
    ok = list(L.ART_SHAPES)
    ok[10] = (256, 300)
    prm = _struct_with(L, L.AonMlpArtParams, 20, ok)
    with pytest.raises(ValueError, match="pts_linears.5: weight 256 x 300.*>= 319"):
        L.call("aon_mlp_art_pack", ctypes.byref(prm), ctypes.c_void_p(16), None)


def test_gemm_small_batch_validation(L):
    """aon_gemm_small_batch refuses, before any launch: a product off the exact-fp32 tiny path,
    two products on one C that differ in shape or do not accumulate, and overlapping outputs
    (column slices of one matrix at the same row stride do not overlap)."""
    def args(C, M, N, K, ldc, acc=0, exact=1):
        return L.AonGemmArgs(M=M, N=N, K=K, A=16, lda=K, a_kc=1, B=16, ldb=K, b_kc=1, C=C,
                             ldc=ldc, accumulate=acc, a_scale=1.0, b_scale=1.0, exact_fp32=exact)

    def run(*items):
        arr = (L.AonGemmArgs * len(items))(*items)
        L.call("aon_gemm_small_batch", arr, len(items), None)

    with pytest.raises(ValueError, match="exact_fp32 tiny products only"):
        run(args(4096, 4, 4, 4, 4, exact=0))
    with pytest.raises(ValueError, match="match in shape and accumulate"):
        run(args(4096, 4, 4, 4, 4), args(4096, 4, 4, 4, 4, acc=0))
    with pytest.raises(ValueError, match="outputs overlap"):
        run(args(1 << 20, 8, 8, 4, 16), args((1 << 20) + 4 * 4, 8, 8, 4, 16))


def test_gemm_workspace_bytes_pinned(L):
    """The GEMM's split policy, read out through its two pure host functions, equals the table
    recorded from the library before kernel selection moved to route_of
    (tests/golden/gemm_workspace.json, tools/gemm_workspace_table.py): every route at a short
    and two long K, both sides of each routing condition, and every batch class.  The workspace
    is splits x (M N + rowsum entries) floats, so any change of route or split count shows."""
    import json

    table = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_workspace.json")))
    lib = L.lib()

    def args(case):
        f = dict(table["defaults"], lda=case["M"], ldb=case["N"], ldc=case["N"])
        f.update(case)
        return L.AonGemmArgs(**f)

    assert len(table["single"]) >= 150 and len(table["batch"]) >= 40
    wrong = []
    for row in table["single"]:
        a = args(row["args"])
        got = lib.aon_gemm_workspace_bytes(ctypes.byref(a))
        if got != row["bytes"]:
            wrong.append((row["name"], got, row["bytes"]))
    for row in table["batch"]:
        arr = (L.AonGemmArgs * len(row["args"]))(*[args(c) for c in row["args"]])
        got = lib.aon_gemm_batch_workspace_bytes(arr, len(arr))
        if got != row["bytes"]:
            wrong.append((row["name"], got, row["bytes"]))
    assert not wrong, f"(case, bytes, recorded): {wrong}"


# ---- every MLP entry point's refusals, message for message -------------------------------------
# The texts and the order in which checks fire were recorded from the library before the launch /
# argument-check helpers of the fused MLP files were shared (mlp_layout.hpp check_fwd_args,
# rows_ok, ...): a call wrong in two ways pins which check comes first.  Every pointer is a fake
# non-null address (16; 20 = misaligned) and every call is refused, or has N = 0, before any HIP
# call -- no GPU needed.
_P, _ODD = ctypes.c_void_p(16), ctypes.c_void_p(20)
_BIG = 1 << 38  # rows whose 128-row blocks reach 2^31: refused; one block fewer passes the guard
_TRAIN_MSG = ("AON_PREC_F16X3_TRAIN is the training forward's stream (aon_mlp_fwd_train): render "
              "with an AON_PREC_F16X3 pack")
_BF16_MSG = "unsupported precision (AON_PREC_BF16 is the training forward's: aon_mlp_fwd_train_bf16)"
_FP32_MSG = "AON_PREC_FP32 has no two-pass kernels: render a fp32 pack with aon_mlp_fwd"
_PR = "packed / raw must be 16-byte aligned"
_MIXED_FWD = "mixed: 0 fp16x3, 1 trunk bf16, 2 view branch bf16, 3 fp16 weights, 4 fp16 activations"
_MIXED_PACK = "mixed: 1 trunk bf16, 2 view branch bf16, 3 fp16 weights past the deformation MLP"


def _render_cases(fn, inner, own_null, inner_null, prec, B, S, act, packed, raw, two_pass):
    """Refusals of a render forward whose shared checks run in `inner` (mlp_launch /
    two_pass_check / art_launch); own_null: pointers the entry point tests itself (first);
    prec: index of the precision argument or None."""
    c = [({i: None}, f"{fn}: null pointer") for i in own_null]
    c += [({i: None}, f"{inner}: null pointer") for i in inner_null]
    if own_null:
        c.append(({own_null[0]: None, packed: None}, f"{fn}: null pointer"))
    c += [({S: 0}, f"{inner}: bad shape"), ({B: -1}, f"{inner}: bad shape"),
          ({act: 3}, f"{inner}: bad activation"), ({act: -1}, f"{inner}: bad activation"),
          ({packed: _ODD}, f"{inner}: {_PR}"), ({raw: _ODD}, f"{inner}: {_PR}"),
          ({B: 0}, None), ({B: _BIG, S: 1}, f"{inner}: too many rows"),
          ({B: _BIG - 128, S: 1, act: 3}, f"{inner}: bad activation"),
          ({packed: None, S: 0}, f"{inner}: null pointer"),
          ({S: 0, act: 3}, f"{inner}: bad shape"),
          ({act: 3, raw: _ODD}, f"{inner}: bad activation"),
          ({raw: _ODD, B: _BIG, S: 1}, f"{inner}: {_PR}")]
    if prec is not None:
        c += [({prec: 4}, f"{inner}: {_TRAIN_MSG}"), ({prec: 2}, f"{inner}: {_BF16_MSG}"),
              ({prec: 3}, f"{inner}: {_BF16_MSG}"), ({prec: 99}, f"{inner}: {_BF16_MSG}"),
              ({prec: 4, packed: None}, f"{inner}: null pointer"),
              ({prec: 4, S: 0}, f"{inner}: {_TRAIN_MSG}"), ({prec: 2, S: 0}, f"{inner}: {_BF16_MSG}")]
        if two_pass:
            c += [({prec: 0}, f"{inner}: {_FP32_MSG}"), ({prec: 0, S: 0}, f"{inner}: {_FP32_MSG}")]
        else:
            c += [({prec: 0, B: 0}, None), ({prec: 0, B: _BIG, S: 1}, f"{inner}: too many rows")]
    return c


def _mlp_refusal_table():
    P = _P
    t = {}
    # aon_mlp_fwd(packed, precision, rays_o, rays_d, viewdirs, t, B, S, act, raw, stream)
    t["aon_mlp_fwd"] = ([P, 1, P, P, P, P, 4, 8, 0, P, None], _render_cases(
        "aon_mlp_fwd", "mlp_launch", [4, 5], [0, 2, 3, 9], 1, 6, 7, 8, 0, 9, False))
    # aon_mlp_fwd_encoded(packed, precision, x, condition, B, S, act, raw, stream)
    t["aon_mlp_fwd_encoded"] = ([P, 1, P, P, 4, 8, 0, P, None], _render_cases(
        "aon_mlp_fwd_encoded", "mlp_launch", [], [0, 2, 3, 7], 1, 4, 5, 6, 0, 7, False))
    # aon_mlp_fwd_sigma(packed, precision, rays_o, rays_d, t, B, S, act, raw, stream)
    t["aon_mlp_fwd_sigma"] = ([P, 1, P, P, P, 4, 8, 0, P, None], _render_cases(
        "aon_mlp_fwd_sigma", "two_pass_check", [], [0, 2, 3, 4, 8], 1, 5, 6, 7, 0, 8, True))
    # aon_mlp_fwd_cond(packed, precision, rays_o, rays_d, cond, t, B, S, act, raw, stream)
    t["aon_mlp_fwd_cond"] = ([P, 1, P, P, P, P, 4, 8, 0, P, None], _render_cases(
        "aon_mlp_fwd_cond", "two_pass_check", [4], [0, 2, 3, 5, 9], 1, 6, 7, 8, 0, 9, True))
    # aon_mlp_art_fwd(packed, rays_o, rays_d, viewdirs, t, B, S, act, out, stream)
    t["aon_mlp_art_fwd"] = ([P, P, P, P, P, 4, 8, 0, P, None], _render_cases(
        "aon_mlp_art_fwd", "art_launch", [3, 4], [0, 1, 2, 8], None, 5, 6, 7, 0, 8, False))
    # aon_mlp_art_fwd_points(packed, pos, condition, B, S, act, out, stream)
    t["aon_mlp_art_fwd_points"] = ([P, P, P, 4, 8, 0, P, None], _render_cases(
        "aon_mlp_art_fwd_points", "art_launch", [], [0, 1, 2, 6], None, 3, 4, 5, 0, 6, False))

    # aon_mlp_fwd_train(packed, rays_o, rays_d, viewdirs, t, B, S, noise, h, bot, hv, raw, masks,
    #                   stream): noise may be null
    f, al = "aon_mlp_fwd_train", "packed / output buffers must be 16-byte aligned"
    t[f] = ([P, P, P, P, P, 4, 8, None, P, P, P, P, P, None],
            [({i: None}, f"{f}: null pointer") for i in (0, 1, 2, 3, 4, 8, 9, 10, 11, 12)] +
            [({12: _ODD}, f"{f}: masks must be 16-byte aligned"), ({6: 0}, f"{f}: bad shape"),
             ({5: -1}, f"{f}: bad shape")] +
            [({i: _ODD}, f"{f}: {al}") for i in (0, 8, 9, 10, 11)] +
            [({5: 0}, None), ({5: _BIG, 6: 1}, f"{f}: too many rows"),
             ({5: _BIG - 128, 6: 1, 11: _ODD}, f"{f}: {al}"),
             ({12: _ODD, 6: 0}, f"{f}: masks must be 16-byte aligned"),
             ({6: 0, 0: _ODD}, f"{f}: bad shape"), ({0: None, 12: _ODD}, f"{f}: null pointer"),
             ({0: _ODD, 5: _BIG, 6: 1}, f"{f}: {al}")])
    # aon_mlp_fwd_train_bf16(..., raw, masks, enc, stream): enc may be null
    f = "aon_mlp_fwd_train_bf16"
    t[f] = ([P, P, P, P, P, 4, 8, None, P, P, P, P, P, P, None],
            [({i: None}, f"{f}: null pointer") for i in (0, 1, 2, 3, 4, 8, 9, 10, 11, 12)] +
            [({6: 0}, f"{f}: bad shape"), ({5: -1}, f"{f}: bad shape")] +
            [({i: _ODD}, f"{f}: {al}") for i in (0, 8, 9, 10, 11, 12, 13)] +
            [({5: 0}, None), ({5: 0, 13: None}, None), ({5: _BIG, 6: 1}, f"{f}: too many rows"),
             ({5: _BIG - 128, 6: 1, 13: _ODD}, f"{f}: {al}"),
             ({12: _ODD, 6: 0}, f"{f}: bad shape"), ({0: None, 6: 0}, f"{f}: null pointer"),
             ({0: _ODD, 5: _BIG, 6: 1}, f"{f}: {al}")])

    # aon_mlp_art_fwd_train(packed, rays_o, rays_d, viewdirs, t, B, S, noise, hd, h, bot, hv, enc,
    #                       xyz, raw, masks, stream); _bf16: ..., masks, enc_bf, mixed, stream
    a8 = "activation buffers must be 8-byte aligned"
    for f, tail in (("aon_mlp_art_fwd_train", [None]), ("aon_mlp_art_fwd_train_bf16", [P, 1, None])):
        c = ([({i: None}, "art_fwd_train: null pointer") for i in (0, 1, 2, 3, 4, 14)] +
             [({i: None}, "art_fwd_train: null activation buffer") for i in (8, 9, 10, 11, 12, 13, 15)] +
             [({i: _ODD}, "art_fwd_train: masks / enc must be 16-byte aligned") for i in (12, 15)] +
             [({6: 0}, "art_fwd_train: bad shape"), ({5: -1}, "art_fwd_train: bad shape"),
              ({0: _ODD}, f"art_fwd_train: {_PR}"), ({14: _ODD}, f"art_fwd_train: {_PR}")] +
             [({i: _ODD}, f"art_fwd_train: {a8}") for i in (8, 9, 10, 11)] +
             [({i: ctypes.c_void_p(24)}, "art_fwd_train: too many rows", {5: _BIG, 6: 1})
              for i in (8, 9, 10, 11)] +
             [({5: 0}, None), ({5: _BIG, 6: 1}, "art_fwd_train: too many rows"),
              ({5: _BIG - 128, 6: 1, 8: _ODD}, f"art_fwd_train: {a8}"),
              ({0: None, 8: None}, "art_fwd_train: null pointer"),
              ({8: None, 12: _ODD}, "art_fwd_train: null activation buffer"),
              ({12: _ODD, 6: 0}, "art_fwd_train: masks / enc must be 16-byte aligned"),
              ({6: 0, 0: _ODD}, "art_fwd_train: bad shape"),
              ({0: _ODD, 8: _ODD}, f"art_fwd_train: {_PR}"),
              ({8: _ODD, 5: _BIG, 6: 1}, f"art_fwd_train: {a8}")])
        if len(tail) == 3:
            eb = "art_fwd_train: enc_bf: a 16-byte aligned buffer"
            c += [({17: 5}, f"{f}: {_MIXED_FWD}"), ({17: -1}, f"{f}: {_MIXED_FWD}"),
                  ({17: 5, 0: None}, f"{f}: {_MIXED_FWD}"),
                  ({16: None}, eb), ({16: _ODD}, eb), ({16: None, 17: 0}, eb),
                  ({16: None, 12: _ODD}, "art_fwd_train: masks / enc must be 16-byte aligned"),
                  ({16: None, 6: 0}, eb)]
            c += [({17: m, 5: 0}, None) for m in range(5)]
            c += [({17: m, 5: _BIG, 6: 1}, "art_fwd_train: too many rows") for m in range(5)]
        t[f] = ([P, P, P, P, P, 4, 8, None, P, P, P, P, P, P, P, P] + tail, c)

    # aon_mlp_bwd(packed, draw, masks, N, dzv, dzb, dz, work, stream) and its bf16 twin (whose
    # 256-row blocks move the row guard to 2^39)
    al = "buffers must be 16-byte aligned"
    for f, big, rpb in (("aon_mlp_bwd", _BIG, 128), ("aon_mlp_bwd_bf16", 2 * _BIG, 256)):
        t[f] = ([P, P, P, 5, P, P, P, P, None],
                [({i: None}, "bwd_launch: null pointer") for i in (0, 1, 2, 4, 5, 6, 7)] +
                [({3: -1}, "bwd_launch: bad shape")] +
                [({i: _ODD}, f"bwd_launch: {al}") for i in (0, 1, 2, 4, 5, 6)] +
                [({3: 0}, None), ({3: 0, 7: _ODD}, None), ({3: big}, "bwd_launch: too many rows"),
                 ({3: big - rpb, 6: _ODD}, f"bwd_launch: {al}"),
                 ({0: None, 3: -1}, "bwd_launch: null pointer"),
                 ({3: -1, 0: _ODD}, "bwd_launch: bad shape"),
                 ({0: _ODD, 3: big}, f"bwd_launch: {al}")])
    # aon_mlp_art_bwd(packed, draw, masks, enc, N, dzv, dbot, dz, dxp, dzd, work, stream)
    for f, big, rpb in (("aon_mlp_art_bwd", _BIG, 128), ("aon_mlp_art_bwd_bf16", 2 * _BIG, 256)):
        t[f] = ([P, P, P, P, 5, P, P, P, P, P, P, None],
                [({i: None}, "art_bwd: null pointer") for i in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10)] +
                [({4: -1}, "art_bwd: bad shape")] +
                [({i: _ODD}, f"art_bwd: {al}") for i in (0, 1, 2, 3, 5, 6, 7, 9)] +
                [({4: 0}, None), ({4: 0, 8: _ODD}, None), ({4: big}, "art_bwd: too many rows"),
                 ({4: big - rpb, 9: _ODD}, f"art_bwd: {al}"),
                 ({0: None, 4: -1}, "art_bwd: null pointer"),
                 ({4: -1, 0: _ODD}, "art_bwd: bad shape"),
                 ({0: _ODD, 4: big}, f"art_bwd: {al}")])
    return t


_MLP_REFUSALS = _mlp_refusal_table()


def _run_cases(L, fn, base, cases):
    lib, wrong = L.lib(), []
    for case in cases:
        args = list(base)
        for d in case[2:] + (case[0],):
            for i, v in d.items():
                args[i] = v
        st = getattr(lib, fn)(*args)
        msg = lib.aon_last_error().decode() if st else None
        if (st, msg) != ((-1, case[1]) if case[1] is not None else (0, None)):
            wrong.append((case[0], st, msg, case[1]))
    assert not wrong, f"{fn} (overrides, status, message, expected): {wrong}"


@pytest.mark.parametrize("fn", sorted(_MLP_REFUSALS))
def test_mlp_entry_point_refusals(L, fn):
    base, cases = _MLP_REFUSALS[fn]
    assert len(cases) >= 12
    _run_cases(L, fn, base, cases)


def test_mlp_pack_refusals(L):
    """The same for the seven pack entry points: null / misaligned buffers, a refused precision or
    `mixed`, a null layer pointer -- each with well-shaped parameter tables, so only the check
    under test stands between the call and a launch."""
    P = _P
    al = "packed buffer must be 16-byte aligned"

    def vanilla(**null):
        prm = _struct_with(L, L.AonMlpParams, 12, L.MLP_SHAPES)
        for k in null:
            setattr(prm, k, None)
        return ctypes.byref(prm)

    def art(**null):
        prm = _struct_with(L, L.AonMlpArtParams, 20, L.ART_SHAPES)
        for k in null:
            setattr(prm, k, None)
        return ctypes.byref(prm)

    f = "aon_mlp_pack"
    _run_cases(L, f, [vanilla(), 1, P, None], [
        ({0: None}, f"{f}: null pointer"), ({2: None}, f"{f}: null pointer"),
        ({1: 3}, f"{f}: unsupported precision"), ({1: -1}, f"{f}: unsupported precision"),
        ({2: _ODD}, f"{f}: {al}"), ({1: 3, 2: None}, f"{f}: null pointer"),
        ({1: 3, 2: _ODD}, f"{f}: unsupported precision"),
        ({0: vanilla(density_w=None)}, f"{f}: null layer parameter"),
        ({0: vanilla(rgb_b=None), 1: 0}, f"{f}: null layer parameter"),
        ({0: vanilla(rgb_b=None), 2: _ODD}, f"{f}: {al}")])
    for f in ("aon_mlp_bwd_pack", "aon_mlp_bwd_pack_bf16"):
        _run_cases(L, f, [vanilla(), P, None], [
            ({0: None}, "bwd_pack: null pointer"), ({1: None}, "bwd_pack: null pointer"),
            ({1: _ODD}, f"bwd_pack: {al}"),
            ({0: vanilla(rgb_w=None)}, "bwd_pack: null layer weight"),
            ({0: vanilla(density_w=None)}, "bwd_pack: null layer weight"),
            ({0: vanilla(density_w=None), 1: _ODD}, f"bwd_pack: {al}")])
    for f in ("aon_mlp_art_pack", "aon_mlp_art_pack_bf16"):
        _run_cases(L, f, [art(), P, None], [
            ({0: None}, "art_pack: null pointer"), ({1: None}, "art_pack: null pointer"),
            ({1: _ODD}, f"art_pack: {al}"),
            ({0: art(deformation_b=None)}, "art_pack: null layer parameter"),
            ({0: art(rgb_w=None), 1: _ODD}, f"art_pack: {al}")])
    f = "aon_mlp_art_pack_mixed"
    _run_cases(L, f, [art(), 1, P, None], [
        ({1: 0}, f"{f}: {_MIXED_PACK}"), ({1: 4}, f"{f}: {_MIXED_PACK}"),
        ({1: 4, 0: None}, f"{f}: {_MIXED_PACK}"),
        ({0: None}, "art_pack: null pointer"), ({1: 3, 2: None}, "art_pack: null pointer"),
        ({1: 2, 2: _ODD}, f"art_pack: {al}"),
        ({1: 3, 0: art(density_w=None)}, "art_pack: null layer parameter")])
    for f in ("aon_mlp_art_bwd_pack", "aon_mlp_art_bwd_pack_bf16"):
        _run_cases(L, f, [art(), P, None], [
            ({0: None}, "art_bwd_pack: null pointer"), ({1: None}, "art_bwd_pack: null pointer"),
            ({1: _ODD}, f"art_bwd_pack: {al}"),
            ({0: art(deformation_w=None)}, "art_bwd_pack: null layer weight"),
            ({0: art(density_w=None)}, "art_bwd_pack: null layer weight"),
            ({0: art(density_w=None), 1: _ODD}, f"art_bwd_pack: {al}")])
