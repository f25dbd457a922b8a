"""GPU parity of the training path (reference LitNeRF.training_step, model.py:256-282, and
optimizer_step, model.py:386-419): the f16x3 GEMM (aon_gemm) against an fp64 matmul of the same
operands (a floating-point kernel: the plain-torch reference is the oracle of record), the
compositing backward against autograd through the CPU oracle, the whole training step against
the reference's golden loss / gradients, and the fused Adam against torch.optim.Adam.

Tolerances: GEMM 2e-6 of the row-scaled magnitude (fp32-class: 22-bit operands, fp32
accumulation); compositing backward 1e-5 relative to each ray's gradient scale; training-step
gradients rtol 2e-3 / atol 1e-6 against the reference (the reference's own fp32 autograd and
ours differ by summation order; the teacher-forced chain checks the fine level at the same
sample positions, like the forward gate in test_gpu_parity.py); loss rtol 1e-5.
"""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max() if want.size else 1.0
    return float(np.abs(got - want).max() / max(scale, 1e-30)) if want.size else 0.0


# ----------------------------------------------------------------------------- GEMM
def _ref_gemm(A, B, a_kc, b_kc, M, N, K, A2=None, K1=None, a2_rdiv=1, b_rdiv=1):
    Ad = A.double()
    if a_kc:
        Am = Ad[:M, :K if A2 is None else K1]
        if A2 is not None:
            A2m = A2.double()[torch.arange(M, device=A.device) // a2_rdiv][:, :K - K1]
            Am = torch.cat([Am, A2m], 1)
    else:
        Am = Ad[:K, :M].t()
    Bd = B.double()
    if b_kc:
        Bm = Bd[:N, :K].t()
    else:
        Bm = Bd[torch.arange(K, device=B.device) // b_rdiv][:, :N]
    return Am @ Bm


@pytest.mark.parametrize("a_kc,b_kc", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (300, 200, 70), (257, 3, 63), (5, 129, 283), (1, 256, 1)])
def test_gemm_layouts(a_kc, b_kc, M, N, K):
    from aonerf.train import gemm

    g = torch.Generator(device="cuda").manual_seed(M * 7 + N * 3 + K)
    A = torch.randn((M, K) if a_kc else (K, M), device="cuda", generator=g)
    B = torch.randn((N, K) if b_kc else (K, N), device="cuda", generator=g)
    C = torch.empty((M, N), device="cuda")
    gemm(C, A, B, M, N, K, lda=A.shape[1], a_kc=a_kc, ldb=B.shape[1], b_kc=b_kc, ldc=N)
    ref = _ref_gemm(A, B, a_kc, b_kc, M, N, K)
    err = (C.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
    assert err < 2e-6, err


def test_gemm_epilogues_segments_split():
    """bias + relu, accumulate-then-mask, the K-concat A2 segment with a per-ray row divisor, a
    broadcast B (b_rdiv), operand prescales and the split-K reduction."""
    from aonerf.train import gemm

    g = torch.Generator(device="cuda").manual_seed(11)
    R, S = 640, 10
    X = torch.randn((R, 256), device="cuda", generator=g) * 3
    E = torch.randn((R // S, 27), device="cuda", generator=g)
    Wt = torch.randn((128, 283), device="cuda", generator=g) * 0.1
    b = torch.randn((128,), device="cuda", generator=g)
    Y = torch.empty((R, 128), device="cuda")
    gemm(Y, X, Wt, R, 128, 283, lda=256, a_kc=True, ldb=283, b_kc=True, ldc=128, A2=E, lda2=27,
         K1=256, a2_rdiv=S, bias=b, relu=True, a_scale=2.0 ** -8)
    ref = torch.relu(_ref_gemm(X, Wt, True, True, R, 128, 283, A2=E, K1=256, a2_rdiv=S) + b.double())
    assert (Y.double() - ref).abs().max().item() < 2e-6 * ref.abs().max().item()
    # accumulate then mask
    C0 = torch.randn((R, 128), device="cuda", generator=g)
    mask = torch.relu(torch.randn((R, 128), device="cuda", generator=g))
    C = C0.clone()
    D = torch.randn((R, 64), device="cuda", generator=g)
    Wd = torch.randn((64, 128), device="cuda", generator=g)
    gemm(C, D, Wd, R, 128, 64, lda=64, a_kc=True, ldb=128, b_kc=False, ldc=128, mask=mask, ldm=128,
         accumulate=True, a_scale=2.0 ** 10)
    ref = (C0.double() + D.double() @ Wd.double()) * (mask > 0)
    assert (C.double() - ref).abs().max().item() < 2e-6 * ref.abs().max().item()
    # weight-gradient shape: K = rows (split-K), A reduction-major, broadcast B
    Rb = 20000
    dY = torch.randn((Rb, 128), device="cuda", generator=g) * 1e-3
    V = torch.randn((Rb // 40, 27), device="cuda", generator=g)
    dW = torch.empty((128, 27), device="cuda")
    db = torch.empty((128,), device="cuda")
    gemm(dW, dY, V, 128, 27, Rb, lda=128, a_kc=False, ldb=27, b_kc=False, b_rdiv=40, ldc=27,
         a_scale=2.0 ** 10, b_scale=2.0 ** -8, k_splits=7, rowsum=db)
    ref = dY.double().t() @ V.double()[torch.arange(Rb, device="cuda") // 40]
    assert (dW.double() - ref).abs().max().item() < 2e-6 * ref.abs().max().item()
    ref_b = dY.double().sum(0)
    assert (db.double() - ref_b).abs().max().item() < 1e-5 * ref_b.abs().max().item()
    # unsplit rowsum, ragged M
    dW2, db2 = torch.empty((3, 27), device="cuda"), torch.empty((3,), device="cuda")
    gemm(dW2, dY[:, 5:], V, 3, 27, 200, lda=128, a_kc=False, ldb=27, b_kc=False, b_rdiv=40, ldc=27,
         k_splits=1, rowsum=db2)
    ref_b2 = dY[:200, 5:8].double().sum(0)
    assert (db2.double() - ref_b2).abs().max().item() < 1e-5 * ref_b2.abs().max().item()


def _single_operands(K, seed):
    """dY-like A (rows spread over six decades, a per-call scale word) and activation-like B
    (ReLU outputs from 1e-6 to ~100, under the forward's 8188 range guard), tiled."""
    from aonerf import _lib as L
    from aonerf import tiles

    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn((K, 256), device="cuda", generator=g) * 1e-3
    A *= 10.0 ** (-6 * torch.rand((K, 1), device="cuda", generator=g))
    B = torch.relu(torch.randn((K, 256), device="cuda", generator=g))
    B *= 10.0 ** (2 - 8 * torch.rand((K, 256), device="cuda", generator=g))
    word = torch.zeros((1,), dtype=torch.int32, device="cuda")
    L.call("aon_absmax", L.ptr(A), A.numel(), L.ptr(word), L.stream())

    def tile_nan(x):  # the padding rows of the last tile NaN: never read
        p = torch.full((tiles.rows(K), 256), float("nan"), device="cuda")
        p[:K] = x
        return tiles.tile(p)
    return A, B, tile_nan(A), tile_nan(B), word


def _single_dw(At, Bt, word, K, single, C=None, accumulate=False, rowsum=None):
    from aonerf.linalg import ACT_SCALE, gemm

    C = torch.zeros((256, 256), device="cuda") if C is None else C
    gemm(C, At, Bt, 256, 256, K, lda=256, a_kc=False, ldb=256, b_kc=False, ldc=256,
         a_scale=1.0, b_scale=8.0 if single else ACT_SCALE, a_amax=word, rowsum=rowsum,
         accumulate=accumulate, a_tiled=True, b_tiled=True, f16_single=single)
    return C


@pytest.mark.parametrize("K", [8192 + 5, 70003, 266240])
def test_f16_single_weight_gradient(K):
    """aon_gemm f16_single (k_gemm_f1_256: one 256 x 256 tile per workgroup, hi*hi + hi*lo +
    lo*hi in ONE accumulator with dY at its per-call scale and X at 2^3): the parity mode's
    256 x 256 weight gradients against fp64 at the GEMM gate (2e-6 of the magnitude), the bias
    gradient (rowsum) within 1e-6, within 2e-6 of the two-accumulator kernel (f16_single = 0),
    accumulate, ragged K (rows past K in the tiles' padding ignored), deterministic."""
    A, B, At, Bt, word = _single_operands(K, K)
    db, db0 = torch.empty((256,), device="cuda"), torch.empty((256,), device="cuda")
    C1 = _single_dw(At, Bt, word, K, True, rowsum=db)
    C1b = _single_dw(At, Bt, word, K, True)
    C0 = _single_dw(At, Bt, word, K, False, rowsum=db0)
    C_init = torch.randn((256, 256), device="cuda")
    Cacc = _single_dw(At, Bt, word, K, True, C=C_init.clone(), accumulate=True)
    torch.cuda.synchronize()
    want = (A.double().T @ B.double()).cpu().numpy()
    e1, e0 = rel_err(C1.cpu().numpy(), want), rel_err(C0.cpu().numpy(), want)
    eb = rel_err(db.cpu().numpy(), A.double().sum(0).cpu().numpy())
    e10 = rel_err(C1.cpu().numpy(), C0.cpu().numpy())
    ea = rel_err(Cacc.cpu().numpy(), want + C_init.double().cpu().numpy())
    print(f"f16_single dW K={K}: max-rel {e1:.2e} (two accumulators {e0:.2e}, between {e10:.2e}),"
          f" rowsum {eb:.2e}, accumulate {ea:.2e}")
    assert torch.equal(C1, C1b), "deterministic"
    assert e1 < 2e-6 and e10 < 2e-6 and eb < 1e-6 and ea < 2e-6


@pytest.mark.parametrize("M,N,n_store", [(128, 256, 256), (256, 64, 63)])
def test_f16_single_other_shapes(M, N, n_store):
    """k_gemm_f1's 128 x 256 (views_linear.0's bottleneck columns) and 256 x 64 (the pos_enc
    columns against aon_cast_rays_tiled's 64-column copy, n_store 63) shapes: against fp64 at
    the GEMM gate, rowsum, only n_store columns written, deterministic; and the tiled
    encodings equal the row-major aon_cast_rays ones bit for bit."""
    from aonerf import _lib as L
    from aonerf import tiles
    from aonerf.linalg import ACT_SCALE, gemm

    K = 70003
    g = torch.Generator(device="cuda").manual_seed(M + N)
    A = torch.randn((K, M), device="cuda", generator=g) * 1e-3
    if N == 64:  # pos_enc(o + t d) tiled, as the f16x3 training step keeps it
        B_, S = 61, K // 61 + 1
        ro = torch.randn((B_, 3), device="cuda", generator=g)
        rd = torch.randn((B_, 3), device="cuda", generator=g)
        t = torch.rand((B_, S), device="cuda", generator=g) * 4 + 2
        Bt = torch.full((tiles.rows(B_ * S), 64), float("nan"), device="cuda")
        L.call("aon_cast_rays_tiled", L.ptr(ro), L.ptr(rd), L.ptr(t), B_, S, 0, 10, 64, L.ptr(Bt),
               L.stream())
        enc = torch.empty((B_ * S, 63), device="cuda")
        L.call("aon_cast_rays", L.ptr(ro), L.ptr(rd), L.ptr(t), B_, S, None, 0, None, 0, 10,
               L.ptr(enc), L.stream())
        un = tiles.untile(Bt, B_ * S)
        assert torch.equal(un[:, :63], enc) and not un[:, 63].any()
        B = un[:K]  # the product's K rows of the (longer) tiled copy
    else:
        B = torch.relu(torch.randn((K, N), device="cuda", generator=g)) * 3
        Bt = tiles.tile(B)
    At = tiles.tile(A)
    word = torch.zeros((1,), dtype=torch.int32, device="cuda")
    L.call("aon_absmax", L.ptr(A), A.numel(), L.ptr(word), L.stream())
    outs = []
    for single in (True, True, False):
        C = torch.full((M, N), 7.0, device="cuda")
        db = torch.empty((M,), device="cuda")
        gemm(C, At, Bt, M, N, K, lda=M, a_kc=False, ldb=N, b_kc=False, ldc=N, rowsum=db,
             a_scale=1.0, b_scale=8.0 if single else ACT_SCALE, a_amax=word, a_tiled=True,
             b_tiled=True, n_store=n_store if single else 0, f16_single=single)
        outs.append((C, db))
    torch.cuda.synchronize()
    (C1, db1), (C2, db2), (C0, _) = outs
    assert torch.equal(C1, C2) and torch.equal(db1, db2)
    want = (A.double().T @ B.double()).cpu().numpy()
    e = rel_err(C1[:, :n_store].cpu().numpy(), want[:, :n_store])
    e0 = rel_err(C1[:, :n_store].cpu().numpy(), C0[:, :n_store].cpu().numpy())
    eb = rel_err(db1.cpu().numpy(), A.double().sum(0).cpu().numpy())
    print(f"f16_single dW {M}x{N} K={K}: max-rel {e:.2e} (vs two accumulators {e0:.2e}), rowsum {eb:.2e}")
    assert e < 2e-6 and e0 < 2e-6 and eb < 1e-6
    if n_store < N:
        assert (C1[:, n_store:] == 7.0).all()


@pytest.mark.parametrize("M,N,K,tiled", [(3, 128, 790528, True), (1, 256, 790528, True),
                                         (4, 256, 70003, False), (2, 16, 5, False)])
def test_f32_skinny_weight_gradient(M, N, K, tiled):
    """The parity mode's head weight gradients (M <= 4: dW = d raw^T X with X = hv3 / h7, the
    fused forward's tiled fp32 tensors) on the streaming skinny kernel without rounding: fp32
    products and sums against fp64 within 1e-6 of the magnitude (the fp16x3 GEMM gate is 2e-6),
    the bias gradient likewise; a_amax and the operand scales cancel; deterministic."""
    from aonerf import _lib as L
    from aonerf import tiles
    from aonerf.linalg import gemm

    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    draw = torch.randn((K, 4), device="cuda", generator=g) * 1e-3
    X = torch.relu(torch.randn((K, N), device="cuda", generator=g)) * 3
    Xs = tiles.tile(X) if tiled else X
    word = torch.zeros((1,), dtype=torch.int32, device="cuda")
    L.call("aon_absmax", L.ptr(draw), draw.numel(), L.ptr(word), L.stream())
    out = []
    for _ in range(2):
        C, db = torch.empty((M, N), device="cuda"), torch.empty((M,), device="cuda")
        gemm(C, draw, Xs, M, N, K, lda=4, a_kc=False, ldb=N, b_kc=False, ldc=N, rowsum=db,
             a_scale=1.0, b_scale=2.0 ** -8, a_amax=word, b_tiled=tiled)
        out.append((C, db))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    want = draw[:, :M].double().T @ X.double()
    e = rel_err(out[0][0].cpu().numpy(), want.cpu().numpy())
    eb = rel_err(out[0][1].cpu().numpy(), draw[:, :M].double().sum(0).cpu().numpy())
    print(f"fp32 skinny dW M={M} N={N} K={K}: max-rel {e:.2e}, rowsum {eb:.2e}")
    assert e < 1e-6 and eb < 1e-6


@pytest.mark.parametrize("K,rdiv", [(790528, 193), (266240, 65), (1885, 65)])
def test_f32_segsum_weight_gradient(K, rdiv):
    """views_linear.0's enc_dir columns in the parity mode (dW = dZv^T venc[row / S], dZv the
    chain's tiled fp32 gradient) on the segment-sum kernel without rounding: against fp64 within
    1e-6, the bias gradient likewise, deterministic."""
    from aonerf import tiles
    from aonerf.linalg import gemm

    g = torch.Generator(device="cuda").manual_seed(K)
    dz = torch.randn((K, 128), device="cuda", generator=g) * 1e-3
    V = torch.randn(((K + rdiv - 1) // rdiv, 27), device="cuda", generator=g)
    dzt = tiles.tile(dz)
    out = []
    for _ in range(2):
        C, db = torch.empty((128, 27), device="cuda"), torch.empty((128,), device="cuda")
        gemm(C, dzt, V, 128, 27, K, lda=128, a_kc=False, ldb=27, b_kc=False, b_rdiv=rdiv, ldc=27,
             rowsum=db, a_scale=1.0, b_scale=2.0 ** -8, a_tiled=True)
        out.append((C, db))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    Vr = V.double()[torch.arange(K, device="cuda") // rdiv]
    e = rel_err(out[0][0].cpu().numpy(), (dz.double().T @ Vr).cpu().numpy())
    eb = rel_err(out[0][1].cpu().numpy(), dz.double().sum(0).cpu().numpy())
    print(f"fp32 segsum dW K={K} rdiv={rdiv}: max-rel {e:.2e}, rowsum {eb:.2e}")
    assert e < 1e-6 and eb < 1e-6


@pytest.mark.parametrize("K", [790528, 70003])
def test_f16_single_weight_gradient_batch_full_level(K):
    """The fine level's 790,528-row products (and a ragged 70,003-row level) as aon_gemm_batch's
    f16_single class (k_gemm_f1h_batch: 256 x 128 half tiles, chunk z of every half on one XCD)
    plus a two-accumulator product in the same batch, the third accumulating: each within 2e-6
    of its own f16_single launch and of the two-accumulator kernel (fp64 at this size is the
    single-size test above); deterministic."""
    from aonerf.linalg import batched

    A, B, At, Bt, word = _single_operands(K, 5)
    del A, B
    C_init = torch.randn((256, 256), device="cuda")

    def run():
        Cs = [torch.zeros((256, 256), device="cuda") for _ in range(2)] + [C_init.clone()]
        rs = [torch.empty((256,), device="cuda") for _ in range(3)]
        with batched():
            for i in range(3):
                _single_dw(At, Bt, word, K, i != 1, C=Cs[i], rowsum=rs[i], accumulate=i == 2)
        torch.cuda.synchronize()
        return Cs, rs

    (Cb, rb), (Cb2, rb2) = run(), run()
    own = _single_dw(At, Bt, word, K, True)
    v1 = _single_dw(At, Bt, word, K, False)
    torch.cuda.synchronize()
    for i in range(3):
        assert torch.equal(Cb[i], Cb2[i]) and torch.equal(rb[i], rb2[i])
    e_own = rel_err(Cb[0].cpu().numpy(), own.cpu().numpy())
    e_v1 = rel_err(Cb[0].cpu().numpy(), v1.cpu().numpy())
    print(f"f16_single dW batch K={K}: vs own launch {e_own:.2e}, vs two accumulators {e_v1:.2e}")
    assert torch.equal(Cb[0] + C_init, Cb[2])  # accumulate: C_init + the same product
    assert torch.equal(rb[0], rb[2]) and e_own < 2e-6 and e_v1 < 2e-6
    assert rel_err(Cb[1].cpu().numpy(), v1.cpu().numpy()) < 1e-6


# ----------------------------------------------------------------------------- compositing bwd
@pytest.mark.parametrize("S,white", [(65, True), (193, False), (7, True), (130, True)])
def test_composite_backward(S, white):
    from aonerf import _lib as L

    g = torch.Generator().manual_seed(S)
    B = 48
    t = torch.sort(2.0 + 4.0 * torch.rand((B, S), generator=g), -1).values
    raw_rgb = torch.randn((B, S, 3), generator=g)
    raw_sig = torch.randn((B, S, 1), generator=g) * 2
    dirs = torch.nn.functional.normalize(torch.randn((B, 3), generator=g), dim=-1)
    g_rgb = torch.randn((B, 3), generator=g) * 1e-2
    # oracle: autograd through the CPU restatement (model.py:186-187 + helper.py:157-195)
    rr, rs = raw_rgb.clone().requires_grad_(True), raw_sig.clone().requires_grad_(True)
    comp, acc, w, depth = O.volumetric_rendering(torch.sigmoid(rr), torch.relu(rs), t, dirs, white)
    (comp * g_rgb).sum().backward()
    raw = cuda(torch.cat([raw_rgb, raw_sig], -1).reshape(-1, 4))
    t_d, dirs_d, g_d = cuda(t), cuda(dirs), cuda(g_rgb)
    d = torch.empty_like(raw)
    L.call("aon_composite_bwd", L.ptr(raw), 4, L.ptr(raw[:, 3:]), 4, L.ptr(t_d), L.ptr(dirs_d), B, S,
           int(white), L.ACT_VANILLA, L.ptr(g_d), None, None, L.ptr(d), L.ptr(d[:, 3:]), 4, L.stream())
    torch.cuda.synchronize()
    got = d.cpu().reshape(B, S, 4)
    for name, gg, want in (("rgb", got[..., :3], rr.grad), ("sigma", got[..., 3:], rs.grad)):
        scale = want.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-12)
        err = ((gg - want).abs() / scale).max().item()
        print(f"composite bwd S={S} {name}: max rel err {err:.2e}")
        assert err < 1e-5, (name, err)


# ----------------------------------------------------------------------------- training step
@pytest.fixture(params=[(True, True), (False, False), (False, True)],
                ids=["fused", "gemm", "gemm_fwd_fused_bwd"])
def fwd_mode(request):
    """Training forward on the fused kernel with activation stores (aon_mlp_fwd_train) or on
    the layer-by-layer GEMMs; backward input gradients in the fused chain (aon_mlp_bwd) or as
    GEMMs.  Every training test runs on each combination (the model's
    TrainNumerics)."""
    fwd, bwd = request.param
    return dict(fused_forward=fwd, fused_backward=bwd)


def test_fused_train_forward_activations():
    """aon_mlp_fwd_train's kept activations and raw outputs (with noise) against the
    layer-by-layer GEMM forward on a ragged batch: the two f16x3 evaluations agree to ~1e-6
    relative of each tensor's range.  The kept tensors are tiled (aonerf/tiles.py; 2,405 rows:
    a partial last 16-row block) and compared through tiles.untile."""
    from aonerf import tiles, train

    net = _make_trainable(0)
    gen = torch.Generator().manual_seed(3)
    B, S = 37, 65
    o = (torch.rand(B, 3, generator=gen) - 0.5).cuda()
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1).cuda()
    t = (2.0 + 4.0 * torch.rand(B, S, generator=gen)).sort(-1).values.cuda()
    noise = torch.rand(B * S, generator=gen).cuda()
    P = [(m.weight.detach(), m.bias.detach()) for m in net.fine_mlp._layers()]
    raw_f = torch.empty((B * S, 4), device="cuda")
    R = B * S
    masks = torch.empty((9, tiles.rows(R), 8), dtype=torch.int32, device="cuda")
    h_t, bot_t, hv_t = train._forward_level_fused(P, o, d, d, t, raw_f, noise, masks)
    h_f = [tiles.untile(x, R) for x in h_t]
    bot_f, hv_f = tiles.untile(bot_t, R), tiles.untile(hv_t, R)
    # the ReLU' bits written by the forward == those built from its stored activations
    rebuilt = train.relu_masks(list(h_f) + [hv_f], R)
    for i in range(9):
        assert torch.equal(tiles.untile_masks(masks[i], R), tiles.untile_masks(rebuilt[i], R)), i
    enc = torch.empty((B * S, 63), device="cuda")
    L = train.L
    L.call("aon_cast_rays", L.ptr(o), L.ptr(d), L.ptr(t), B, S, None, 0, None, 0, 10, L.ptr(enc),
           L.stream(o.device))
    venc = torch.empty((B, 27), device="cuda")
    L.call("aon_pos_enc", L.ptr(d), B, 0, 4, L.ptr(venc), L.stream(o.device))
    raw_g = torch.empty((B * S, 4), device="cuda")
    h_g, bot_g, hv_g = train._forward_level(P, enc, venc, S, raw_g, noise)
    for name, a, b in [(f"h{i}", h_f[i], h_g[i]) for i in range(8)] + [
            ("bot", bot_f, bot_g), ("hv", hv_f, hv_g), ("raw", raw_f, raw_g)]:
        e = rel_err(a.cpu().numpy(), b.cpu().numpy())
        print(f"  fused vs gemm forward {name}: max rel err {e:.2e}")
        assert e < 2e-5, name
    # relu masks agree wherever the value is not within rounding of zero
    for i in range(8):
        a, b = h_f[i].cpu().numpy(), h_g[i].cpu().numpy()
        tol = 1e-5 * np.abs(b).max()
        assert np.all(((a > 0) == (b > 0)) | (np.abs(b) < tol))


def _make_trainable(seed, **numerics):
    """A NeRF with the oracle's seed-``seed`` weights; ``numerics``: TrainNumerics fields."""
    from aonerf.model import NeRF
    from aonerf.numerics import TrainNumerics

    net = NeRF(train_numerics=TrainNumerics(**numerics)).cuda()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in W.nerf_state_dict(seed).items()})
    return net


def _oracle_params(seed, requires_grad=True):
    params = O.split_state_dict(W.nerf_state_dict(seed))
    for p in params:
        for v in p.values():
            v.requires_grad_(requires_grad)
    return params


def _oracle_grads(g, dtype):
    params = [{k: v.to(dtype).requires_grad_(True) for k, v in p.items()}
              for p in O.split_state_dict(W.nerf_state_dict(0))]
    rays = {k: torch.from_numpy(g[k]).to(dtype) for k in ("rays_o", "rays_d", "viewdirs")}
    ret, inter = O.nerf_forward(params, rays, True, True, 2.0, 6.0,
                                u_coarse=torch.from_numpy(g["u_coarse"]).to(dtype),
                                u_fine=torch.from_numpy(g["u_fine"]).to(dtype),
                                return_intermediates=True)
    tgt = torch.from_numpy(g["target"]).to(dtype)
    (O.img2mse(ret[1][0], tgt) + O.img2mse(ret[0][0], tgt)).backward()
    grads = {f"{lv}.{k}": v.grad.double().numpy() for lv, p in zip(("coarse_mlp", "fine_mlp"), params)
             for k, v in p.items()}
    return grads, inter


def test_train_step_golden(golden, fwd_mode):
    """Loss and the recorded gradients of one LitNeRF.training_step (randomized, injected
    uniforms) against the reference.  Gradients w.r.t. the first layer see the encodings'
    sin(2^9 x) features, so a 1e-7 change of a coarse weight, amplified by the inverse CDF into
    a ~1e-5 move of a fine sample, moves them by ~1e-2 of their maximum: the reference itself
    evaluated in fp64 instead of fp32 differs that much (its re-association envelope, computed
    here by the oracle).  Gate per tensor: max|ours - ref| <= max(4 x envelope, 1e-4) x max|ref|.
    The strict gate is the teacher-forced chain below (same sample positions: ~1e-5)."""
    from aonerf import train

    g = golden("train_step.npz")
    net = _make_trainable(0, **fwd_mode)
    assert W.digest(W.nerf_state_dict(0)) == str(g["digest"])
    batch = {k: cuda(g[k]) for k in ("rays_o", "rays_d", "viewdirs", "target")}
    loss, logs = train.training_step(net, batch, True, True, 2.0, 6.0, u_coarse=cuda(g["u_coarse"]),
                                     u_fine=cuda(g["u_fine"]))
    loss.backward()
    torch.cuda.synchronize()
    print(f"loss gpu {loss.item():.8f} ref {float(g['loss']):.8f}")
    np.testing.assert_allclose(loss.item(), g["loss"], rtol=1e-5)
    np.testing.assert_allclose(logs["loss0"].item(), g["loss0"], rtol=1e-5)
    g64, _ = _oracle_grads(g, torch.float64)
    named = dict(net.named_parameters())
    worst = 0.0
    for key in g:
        if not key.startswith("grad::"):
            continue
        ref = g[key]
        env = rel_err(ref, g64[key[6:]])
        e = rel_err(named[key[6:]].grad.cpu().numpy(), ref)
        print(f"  {key[6:]:40s} ours {e:.2e}  reference fp32-vs-fp64 envelope {env:.2e}")
        worst = max(worst, e / max(4 * env, 1e-4))
        assert e <= max(4 * env, 1e-4), (key, e, env)
    print(f"train-step grads vs reference: worst error / allowance {worst:.2f}")


@pytest.mark.parametrize("loss_scale", [1.0, 1.0 / 64], ids=["64rays", "grad_mag_4096rays"])
def test_train_step_chain(golden, fwd_mode, loss_scale):
    """Teacher-forced per-level gradients: our level-l t_vals through the oracle's autograd
    (fp32, the reference's arithmetic), each tensor within max(1e-3, 2 x the fp32 oracle's own
    distance from the fp64 oracle) of its max.  ``loss_scale`` 1/64 gives the per-row gradient
    magnitudes of a 4096-ray batch."""
    from aonerf import train

    g = golden("train_step.npz")
    net = _make_trainable(0, **fwd_mode)
    batch = {k: cuda(g[k]) for k in ("rays_o", "rays_d", "viewdirs", "target")}
    ret = net(batch, True, True, 2.0, 6.0, u_coarse=cuda(g["u_coarse"]), u_fine=cuda(g["u_fine"]),
              return_weights=True, return_intermediates=True)
    target = batch["target"]
    loss = (train.img2mse(ret[1][0], target) + train.img2mse(ret[0][0], target)) * loss_scale
    loss.backward()
    ref = {}
    for dtype in (torch.float32, torch.float64):  # the oracle at our sample positions
        rays = {k: torch.from_numpy(g[k]).to(dtype) for k in ("rays_o", "rays_d", "viewdirs")}
        params = [{k: v.to(dtype).requires_grad_(True) for k, v in p.items()}
                  for p in O.split_state_dict(W.nerf_state_dict(0))]
        tgt = torch.from_numpy(g["target"]).to(dtype)
        ref_loss = 0.0
        for level in range(2):
            t = ret[level][4]["t_vals"].cpu().to(dtype)
            comp, acc, w, depth = O.render_level(params, rays, t, level, True)
            ref_loss = ref_loss + O.img2mse(comp, tgt)
            np.testing.assert_allclose(ret[level][0].detach().cpu().numpy(), comp.detach().numpy(),
                                       rtol=0, atol=1e-5)
        (ref_loss * loss_scale).backward()
        ref[dtype] = {f"{pre}{n}": v.grad.double().numpy()
                      for lv, pre in ((0, "coarse_mlp."), (1, "fine_mlp.")) for n, v in params[lv].items()}
    named = dict(net.named_parameters())
    worst = worst32 = 0.0
    for name, want in ref[torch.float32].items():
        e = rel_err(named[name].grad.cpu().numpy(), want)
        env = rel_err(want, ref[torch.float64][name])
        if e > 1e-4:
            print(f"  {name}: max-rel err {e:.2e} (fp32 vs fp64 oracle {env:.2e})")
        worst, worst32 = max(worst, e), max(worst32, env)
        assert e < max(1e-3, 2 * env), (name, e, env)
    print(f"teacher-forced grads: worst max-rel err {worst:.2e} vs the fp32 oracle "
          f"(fp32 vs fp64 oracle: {worst32:.2e})")


@pytest.mark.parametrize("n_rays,with_reg", [(4096, False), (1000, True), (1, False)])
def test_loss_pair_equals_unfused(n_rays, with_reg):
    """train.loss_pair (aon_loss_pair: both img2mse, their sum, the psnrs in one launch) gives
    the unfused training_step's values bit for bit -- img2mse per level (aon_mse), loss1 + loss0
    (+ reg) and mse2psnr as torch computes it on the device -- and its backward (one
    aon_loss_pair_bwd launch) the same rgb gradients as img2mse's, for a non-unit dL/dloss and
    with the per-level losses also used downstream."""
    from aonerf import train

    g = torch.Generator(device="cuda").manual_seed(n_rays)
    p0 = torch.rand((n_rays, 3), device="cuda", generator=g)
    p1 = torch.rand((n_rays, 3), device="cuda", generator=g)
    tgt = torch.rand((n_rays, 3), device="cuda", generator=g)
    reg = torch.rand((), device="cuda", generator=g) * 1e-3 if with_reg else None
    a0, a1 = p0.clone().requires_grad_(True), p1.clone().requires_grad_(True)
    b0, b1 = p0.clone().requires_grad_(True), p1.clone().requires_grad_(True)
    ra = reg.clone().requires_grad_(True) if with_reg else None
    rb = reg.clone().requires_grad_(True) if with_reg else None

    loss, l0, l1, s0, s1 = train.loss_pair(a0, a1, tgt, ra)
    u0, u1 = train.img2mse(b0, tgt), train.img2mse(b1, tgt)
    uloss = u1 + u0 + rb if with_reg else u1 + u0
    for got, want in ((loss, uloss), (l0, u0), (l1, u1), (s0, train.mse2psnr(u0.detach())),
                      (s1, train.mse2psnr(u1.detach()))):
        assert torch.equal(got.detach(), want.detach()), (got.item(), want.item())
    assert not s0.requires_grad and not s1.requires_grad
    (3.0 * loss + 0.5 * l0).backward()
    (3.0 * uloss + 0.5 * u0).backward()
    assert torch.equal(a0.grad, b0.grad) and torch.equal(a1.grad, b1.grad)
    if with_reg:
        assert torch.equal(ra.grad, rb.grad)


def test_adam_matches_torch():
    """aon_adam_step against torch.optim.Adam (model.py:386-389) as the reference builds it on a
    GPU: foreach=None -> the multi-tensor path (_foreach_div_ by the Python-float sqrt(bc2) is a
    true division; the single-tensor path multiplies by its fp32 reciprocal instead, 1 ulp
    apart).  The parameters start at zero so the update is not lost in the ulps of p: the first
    step's update must agree to 1e-6 relative (fp32 hyperparameters rounded before 1 - beta
    would be 1.3e-5 off), and every later step to 2e-6 of the update's size."""
    from aonerf import train

    g = torch.Generator(device="cuda").manual_seed(5)
    ps = [torch.zeros(s, device="cuda") for s in ((256, 63), (256,), (3, 128), (1,))]
    mine = [p.clone().requires_grad_(True) for p in ps]
    ref = [p.clone().requires_grad_(True) for p in ps]
    opt_m = train.Adam(mine, lr=5e-4)
    opt_r = torch.optim.Adam(ref, lr=5e-4, betas=(0.9, 0.999))
    for step in range(1, 6):
        grads = [torch.randn(p.shape, device="cuda", generator=g) * 10 ** -step for p in ps]
        lr = train.learning_rate(step, 1000)
        before = [q.detach().clone() for q in ref]
        for p, q, gr in zip(mine, ref, grads):
            p.grad = gr.clone()
            q.grad = gr.clone()
        v0 = [p._version for p in mine]
        opt_m.step(lr=lr)
        assert all(p._version > v for p, v in zip(mine, v0)), "Adam.step must bump versions"
        for pg in opt_r.param_groups:
            pg["lr"] = lr
        opt_r.step()
        for p, q, q0 in zip(mine, ref, before):
            upd = (q.detach() - q0).abs().max().item()
            assert upd > 1e-6  # the parameters did move
            d = (p.detach() - q.detach()).abs().max().item()
            tol = (1e-6 if step == 1 else 2e-6) * upd
            assert d <= tol, (step, d, upd)


def test_adam_vector_path_equals_scalar_path():
    """aon_adam_step's 4-wide kernel (every tensor 16-B aligned) and its one-element kernel (any
    misaligned tensor) give the same bits, ragged tails (numel % 4 != 0) included."""
    from aonerf import train

    g = torch.Generator(device="cuda").manual_seed(9)
    shapes = ((256, 63), (3,), (1,), (7, 5), (128,))
    base = [torch.randn(s, device="cuda", generator=g) for s in shapes]
    grads = [torch.randn(s, device="cuda", generator=g) for s in shapes]
    aligned = [b.clone().requires_grad_(True) for b in base]
    # the same values at a 4-B offset inside a larger buffer: not 16-B aligned
    store = [torch.empty(b.numel() + 1, device="cuda") for b in base]
    shifted = []
    for st, b in zip(store, base):
        st[1:].copy_(b.reshape(-1))
        shifted.append(st[1:].view(b.shape).requires_grad_(True))
    assert shifted[0].data_ptr() % 16 != 0
    oa, os_ = train.Adam(aligned, lr=1e-3), train.Adam(shifted, lr=1e-3)
    for step in range(3):
        for p, q, gr in zip(aligned, shifted, grads):
            p.grad = gr * (step + 1)
            q.grad = gr * (step + 1)
        oa.step()
        os_.step()
        for p, q in zip(aligned, shifted):
            assert torch.equal(p.detach(), q.detach())
        for (m1, v1), (m2, v2) in zip(oa.state, os_.state):
            assert torch.equal(m1, m2) and torch.equal(v1, v2)


def test_render_after_adam_uses_new_weights():
    """A no_grad render packs the weights once and caches the pack by (pointer, version); the
    fused Adam updates parameters in place through raw pointers, so it must bump the versions or
    the next render would draw the stale pack.  Render, train one step, render
    again: the result equals a freshly built model holding the trained weights, bit for bit."""
    from aonerf import train
    from aonerf.model import NeRF
    from aonerf.ray_utils import frame_rays
    from aonerf.render import create_spheric_poses, sapien_focal

    net = _make_trainable(0)
    H, Wd = 16, 20
    rays = frame_rays(create_spheric_poses(4.0)[3], H, Wd, sapien_focal(H))
    with torch.no_grad():
        before = net(rays, False, True, 2.0, 6.0)[1][0].clone()
    opt = train.Adam(net.parameters(), lr=5e-3)
    batch = dict(rays, target=torch.full((H * Wd, 3), 0.25, device="cuda"))
    loss, _ = train.training_step(net, batch, False, True, 2.0, 6.0)
    loss.backward()
    opt.step()
    with torch.no_grad():
        after = net(rays, False, True, 2.0, 6.0)[1][0]
        fresh = NeRF().cuda()
        fresh.load_state_dict({k: v.detach().clone() for k, v in net.state_dict().items()})
        want = fresh(rays, False, True, 2.0, 6.0)[1][0]
    torch.cuda.synchronize()
    assert not torch.equal(before, after), "the render did not see the trained weights"
    assert torch.equal(after, want)


def c5_batch(n=4096, seed=11):
    """Config C5's batch: n pixels of a synthetic 640x480 view (distinct, PCG64), a synthetic
    target, and the randomized-mode uniforms (injected so the oracle sees the same draws)."""
    from aonerf.ray_utils import frame_rays
    from aonerf.render import create_spheric_poses, sapien_focal

    H, Wd = 480, 640
    rays = frame_rays(torch.as_tensor(create_spheric_poses(4.0)[5]), H, Wd, sapien_focal(H))
    rng = np.random.Generator(np.random.PCG64(seed))
    idx = torch.from_numpy(rng.choice(H * Wd, n, replace=False)).cuda()
    batch = {k: v[idx].contiguous() for k, v in rays.items()}
    batch["target"] = cuda(rng.uniform(0, 1, (n, 3)).astype(np.float32))
    u_c = cuda(rng.uniform(0, 1, (n, 65)).astype(np.float32))
    u_f = cuda(rng.uniform(0, 1, (n, 128)).astype(np.float32))
    return batch, u_c, u_f


def test_train_step_c5_4096_rays():
    """Config C5 at its stated size: one training step on a 4096-ray batch (1,056,768 MLP
    samples).  The loss against the oracle's end-to-end loss on the same rays and uniforms
    (rtol 1e-4: a CDF-bin flip of a few rays' fine samples moves the mean by ~1e-6), the loss of
    our sample positions to 1e-5, and every parameter's gradient teacher-forced against the fp32
    oracle's autograd at our sample positions within max(2 x the oracle's own fp32-vs-fp64
    distance, 1e-3) of the tensor's max, as the 64-ray test above."""
    from aonerf import train

    net = _make_trainable(0)
    batch, u_c, u_f = c5_batch()
    ret = net(batch, True, True, 2.0, 6.0, u_coarse=u_c, u_fine=u_f, return_weights=True,
              return_intermediates=True)
    target = batch["target"]
    loss = train.img2mse(ret[1][0], target) + train.img2mse(ret[0][0], target)
    loss.backward()
    torch.cuda.synchronize()
    with torch.no_grad():
        rays = {k: batch[k].cpu() for k in ("rays_o", "rays_d", "viewdirs")}
        e2e = O.nerf_forward(_oracle_params(0, False), rays, True, True, 2.0, 6.0,
                             u_coarse=u_c.cpu(), u_fine=u_f.cpu())
        tgt = target.cpu()
        ref_e2e = (O.img2mse(e2e[1][0], tgt) + O.img2mse(e2e[0][0], tgt)).item()
    ref, ref_loss = {}, None
    for dtype in (torch.float32, torch.float64):  # the oracle at our sample positions
        rays = {k: batch[k].cpu().to(dtype) for k in ("rays_o", "rays_d", "viewdirs")}
        params = [{k: v.to(dtype).requires_grad_(True) for k, v in p.items()}
                  for p in O.split_state_dict(W.nerf_state_dict(0))]
        tgt = target.cpu().to(dtype)
        lv_loss = 0.0
        for level in range(2):
            t = ret[level][4]["t_vals"].cpu().to(dtype)
            comp, acc, w, depth = O.render_level(params, rays, t, level, True)
            lv_loss = lv_loss + O.img2mse(comp, tgt)
        lv_loss.backward()
        if dtype == torch.float32:
            ref_loss = lv_loss.item()
        ref[dtype] = {f"{pre}{n}": v.grad.double().numpy()
                      for lv, pre in ((0, "coarse_mlp."), (1, "fine_mlp.")) for n, v in params[lv].items()}
        del params, lv_loss
    print(f"C5 loss gpu {loss.item():.8f}  oracle on our t {ref_loss:.8f}  "
          f"oracle end to end {ref_e2e:.8f}")
    np.testing.assert_allclose(loss.item(), ref_loss, rtol=1e-5)
    np.testing.assert_allclose(loss.item(), ref_e2e, rtol=1e-4)
    named = dict(net.named_parameters())
    worst = 0.0
    for name, want in ref[torch.float32].items():
        e = rel_err(named[name].grad.cpu().numpy(), want)
        env = rel_err(want, ref[torch.float64][name])
        allow = max(2 * env, 1e-3)
        if e > 1e-4:
            print(f"  {name:40s} ours {e:.2e}  oracle fp32-vs-fp64 {env:.2e}")
        worst = max(worst, e / allow)
        assert e <= allow, (name, e, env)
    print(f"C5 teacher-forced grads (4096 rays): worst error / allowance {worst:.2f}")


@pytest.mark.parametrize("fused", [False, True], ids=["gemm_backward", "fused_chain"])
def test_backward_gradient_scale_invariance(fused):
    """Late-training gradient magnitudes (a fixed 2^10 prescale of dY before the
    fp16 hi/lo split would push small dL/dz into fp16's subnormals).  Both backward paths scale
    every gradient operand per call by a power of two from its own max |dY| (aon_absmax /
    k_absmax -> a_amax), so d raw x 2^-24 -- a loss ~1.7e7 times smaller than the 64-ray
    golden's -- must give every weight and bias gradient x 2^-24 BIT FOR BIT; d raw x 2^20
    likewise."""
    from aonerf import train

    net = _make_trainable(0)
    gen = torch.Generator().manual_seed(5)
    B, S = 61, 65
    R = B * S
    o = (torch.rand(B, 3, generator=gen) - 0.5).cuda()
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1).cuda()
    t = (2.0 + 4.0 * torch.rand(B, S, generator=gen)).sort(-1).values.cuda()
    P = [(m.weight.detach(), m.bias.detach()) for m in net.fine_mlp._layers()]
    L = train.L
    enc = torch.empty((R, 63), device="cuda")
    L.call("aon_cast_rays", L.ptr(o), L.ptr(d), L.ptr(t), B, S, None, 0, None, 0, 10, L.ptr(enc),
           L.stream(o.device))
    venc = torch.empty((B, 27), device="cuda")
    L.call("aon_pos_enc", L.ptr(d), B, 0, 4, L.ptr(venc), L.stream(o.device))
    raw = torch.empty((R, 4), device="cuda")
    h, bot, hv = train._forward_level(P, enc, venc, S, raw)
    draw = (torch.randn(R, 4, generator=gen) * 1e-4).cuda()
    out = {}
    for k in (0, -24, 20):
        G = [(torch.empty_like(w), torch.empty_like(b)) for w, b in P]
        dr = draw * 2.0 ** k
        if fused:
            train._backward_level_fused(P, G, enc, venc, S, h, bot, hv, dr, h_tiled=False)
        else:
            train._backward_level(P, G, enc, venc, S, h, bot, hv, dr)
        out[k] = [g for pair in G for g in pair]
    torch.cuda.synchronize()
    for k in (-24, 20):
        for i, (a, b) in enumerate(zip(out[k], out[0])):
            assert torch.equal(a * 2.0 ** -k, b), (k, i, float((a * 2.0 ** -k - b).abs().max()))


_LAYER_NAMES = ([f"pts_linears.{i}" for i in range(8)]
                + ["density_layer", "bottleneck_layer", "views_linear.0", "rgb_layer"])  # _layers()
_DZ_NAMES = [f"dz{i}" for i in range(8)] + ["dzb", "dzv"]


def _nan_padding(x, R):
    """A tiled kept tensor with the padding rows of its last 16-row tile NaN: never read."""
    from aonerf import tiles

    rm = tiles.untile(x, x.shape[0])
    rm[R:] = float("nan")
    return tiles.tile(rm)


def stage_level(B, S, bf16=False):
    """One fine level's fused training forward on a ragged batch (train._forward_level_fused:
    the kept activations, tiled, and their ReLU' bits) with everything the stage-isolated
    backward gates need: the row-major encodings (aon_cast_rays, aon_pos_enc), the tiled copy
    the fused backward reads in production (aon_cast_rays_tiled, 64 fp32 columns; bf16: the
    forward's own 128-column bf16 copy), both pre-filled with NaN past row R, the kept tensors
    row-major (for the fp64 oracle and the all-GEMM backward) and tiled with NaN padding rows
    (for the fused backward)."""
    from aonerf import tiles, train

    L = train.L
    net = _make_trainable(0)
    gen = torch.Generator().manual_seed(B + S)
    R, NR = B * S, tiles.rows(B * S)
    o = (torch.rand(B, 3, generator=gen) - 0.5).cuda()
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1).cuda()
    t = (2.0 + 4.0 * torch.rand(B, S, generator=gen)).sort(-1).values.cuda()
    P = [(m.weight.detach(), m.bias.detach()) for m in net.fine_mlp._layers()]
    raw = torch.empty((R, 4), device="cuda")
    masks = torch.empty((9, NR, 8), dtype=torch.int32, device="cuda")
    if bf16:
        enc_t = torch.full((NR, 128), float("nan"), device="cuda", dtype=torch.bfloat16)
    else:
        enc_t = torch.full((NR, 64), float("nan"), device="cuda")
        L.call("aon_cast_rays_tiled", L.ptr(o), L.ptr(d), L.ptr(t), B, S, 0, 10, 64, L.ptr(enc_t),
               L.stream())
    h_t, bot_t, hv_t = train._forward_level_fused(P, o, d, d, t, raw, None, masks, bf16=bf16,
                                                  enc=enc_t if bf16 else None)
    enc = torch.empty((R, 63), device="cuda")
    L.call("aon_cast_rays", L.ptr(o), L.ptr(d), L.ptr(t), B, S, None, 0, None, 0, 10, L.ptr(enc),
           L.stream())
    venc = torch.empty((B, 27), device="cuda")
    L.call("aon_pos_enc", L.ptr(d), B, 0, 4, L.ptr(venc), L.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(raw).all()
    return dict(P=P, R=R, NR=NR, S=S, gen=gen, rays_d=d, t=t, raw=raw, masks=masks, enc=enc,
                enc_t=enc_t, venc=venc,
                h_rm=[tiles.untile(x, R).float() for x in h_t],
                bot_rm=tiles.untile(bot_t, R).float(), hv_rm=tiles.untile(hv_t, R).float(),
                h_t=[_nan_padding(x, R) for x in h_t], bot_t=_nan_padding(bot_t, R),
                hv_t=_nan_padding(hv_t, R))


def stage_reference(lv, draw):
    """The fp64 oracle backward at the GPU forward's own kept values (oracle.mlp_forward_kept)
    from ``draw`` (R, 4): ({parameter name: gradient}, [dL/dZ of pts_linears.0..7,
    bottleneck_layer, views_linear.0]) as fp64 numpy arrays."""
    p64 = {k[len("fine_mlp."):]: torch.from_numpy(v).double().requires_grad_(True)
           for k, v in W.nerf_state_dict(0).items() if k.startswith("fine_mlp.")}
    kept = {"enc": lv["enc"].cpu(), "h": [x.cpu() for x in lv["h_rm"]], "bot": lv["bot_rm"].cpu(),
            "hv": [lv["hv_rm"].cpu()]}
    pre = {}
    r_rgb, r_sig = O.mlp_forward_kept(p64, kept, lv["venc"].cpu(), lv["S"], record=pre)
    zs = pre["z"] + [pre["zb"]] + pre["zv"]
    for z in zs:
        z.retain_grad()
    d64 = draw.cpu().double()
    torch.autograd.backward([r_rgb, r_sig], [d64[:, :3], d64[:, 3:]])
    return {k: v.grad.numpy() for k, v in p64.items()}, [z.grad.numpy() for z in zs]


def stage_chain(lv, draw, bf16=False):
    """aon_mlp_bwd[_bf16] alone on the level's ReLU' bits and ``draw``: the untiled dz[0..7],
    dzb, dzv (outputs pre-filled with NaN: every row below R must be written)."""
    from aonerf import tiles, train

    L = train.L
    R, NR = lv["R"], lv["NR"]
    dt = torch.bfloat16 if bf16 else torch.float32
    dzv = torch.full((NR, 128), float("nan"), device="cuda", dtype=dt)
    dzb = torch.full((NR, 256), float("nan"), device="cuda", dtype=dt)
    dz = torch.full((8, NR, 256), float("nan"), device="cuda", dtype=dt)
    work = torch.zeros((4,), dtype=torch.int32, device="cuda")
    packed = train._pack_bwd(lv["P"], draw.device, "stage", bf16)
    L.call("aon_mlp_bwd_bf16" if bf16 else "aon_mlp_bwd", L.ptr(packed), L.ptr(draw),
           L.ptr(lv["masks"]), R, L.ptr(dzv), L.ptr(dzb), L.ptr(dz), L.ptr(work), L.stream())
    L.snapshot_pack(packed)
    torch.cuda.synchronize()
    return [tiles.untile(dz[i], R).float() for i in range(8)] + [
        tiles.untile(dzb, R).float(), tiles.untile(dzv, R).float()]


@pytest.mark.parametrize("B,S,scale", [(1, 1, 1e-3), (29, 65, 1e-3), (37, 193, 1e-4),
                                       (128, 193, 1e-4)],
                         ids=["one_row", "ragged_13_of_16", "fine193_ragged", "fine193"])
def test_backward_stage_isolated(B, S, scale):
    """Stage isolation of the vanilla backward (model.py:95-120), the counterpart of
    test_gpu_art_train.test_art_backward_stage_isolated: the fused forward's own kept tensors
    and ReLU' bits and a fixed random d raw go through (a) aon_mlp_bwd + the weight-gradient
    aon_gemm's on the tiled tensors (train._backward_level_fused, the padding rows of the last
    tile NaN), (b) the all-GEMM backward on their row-major copies (train._backward_level) and
    (c) the oracle's fp64 autograd evaluated at exactly those forward values
    (oracle.mlp_forward_kept).  Every weight and bias gradient of (a) and (b) within 1e-4 of
    its tensor's max of (c); and aon_mlp_bwd alone: dz[0..7], dzb, dzv against the fp64 dL/dZ
    of each layer (retain_grad on the pre-activation sums), same gate, every row below R
    finite.  R = 1885 leaves 13 rows in the last 16-row tile, R = 7141 five, R = 1 one.

    Measured worst tensor (MI355X), fused / GEMM / chain:
      (1, 1)      8.4e-07 / 4.9e-07 / 8.4e-07
      (29, 65)    2.4e-06 / 9.6e-07 / 5.7e-07
      (37, 193)   2.4e-06 / 9.9e-07 / 5.8e-07
      (128, 193)  9.9e-06 / 9.0e-07 / 6.1e-07   (fused: pts_linears.1.bias, a column sum of dz1)
    """
    from aonerf import train

    lv = stage_level(B, S)
    P, venc = lv["P"], lv["venc"]
    draw = (torch.randn(lv["R"], 4, generator=lv["gen"]) * scale).cuda()
    Gf = [(torch.empty_like(w), torch.empty_like(b)) for w, b in P]
    Gg = [(torch.empty_like(w), torch.empty_like(b)) for w, b in P]
    train._backward_level_fused(P, Gf, lv["enc_t"], venc, S, lv["h_t"], lv["bot_t"], lv["hv_t"],
                                draw, lv["masks"], True)
    train._backward_level(P, Gg, lv["enc"], venc, S, lv["h_rm"], lv["bot_rm"], lv["hv_rm"], draw)
    dzs = stage_chain(lv, draw)
    torch.cuda.synchronize()
    want, want_dz = stage_reference(lv, draw)
    report, bad = [], []
    for mode, G in (("fused", Gf), ("gemm", Gg)):
        worst, worst_name = 0.0, ""
        for (dw, db), name in zip(G, _LAYER_NAMES):
            for got, key in ((dw, f"{name}.weight"), (db, f"{name}.bias")):
                e = rel_err(got.cpu().numpy(), want[key])
                if not e <= worst:  # (a NaN is the worst)
                    worst, worst_name = e, key
                if not e <= 1e-4:
                    bad.append((mode, key, e))
        report.append(f"{mode} {worst:.2e} ({worst_name})")
    worst, worst_name = 0.0, ""
    for got, w, name in zip(dzs, want_dz, _DZ_NAMES):
        assert torch.isfinite(got).all(), name
        e = rel_err(got.cpu().numpy(), w)
        if e > worst:
            worst, worst_name = e, name
        if not e <= 1e-4:
            bad.append(("chain", name, e))
    report.append(f"chain {worst:.2e} ({worst_name})")
    print(f"vanilla backward (B={B}, S={S}) vs fp64 at the GPU's forward values: worst "
          + ", ".join(report))
    assert not bad, bad


def _step_state(net, opt, train_mod, batch, u_c, u_f, lib=None):
    """One training step + Adam: (loss, grads, params after) as host copies."""
    opt.zero_grad()
    if lib is None:
        loss, _ = train_mod.training_step(net, batch, True, True, 2.0, 6.0, u_coarse=u_c, u_fine=u_f)
    else:
        loss, _ = train_mod.training_step(net, lib, batch, True, True, 2.0, 6.0, u_coarse=u_c,
                                          u_fine=u_f)
    loss.backward()
    params = list(net.parameters()) + (list(lib.parameters()) if lib is not None else [])
    grads = [p.grad.detach().cpu().clone() for p in params]
    opt.step()
    return loss.detach().cpu(), grads, [p.detach().cpu().clone() for p in params]


def test_two_precisions_in_one_process():
    """Verdict r05 #5 (reentrant, no mutable globals): a bf16 model and an f16x3
    model of the same weights train in ONE process, their forwards, backward and Adam steps
    interleaved, and each is bit-equal to its solo run -- the training numerics are the model's
    own (TrainNumerics), not a module switch."""
    from aonerf import train

    batch, u_c, u_f = c5_batch(n=512, seed=5)
    solo = {}
    for prec in ("f16x3", "bf16"):
        net = _make_trainable(0, precision=prec)
        opt = train.Adam(net.parameters())
        solo[prec] = [_step_state(net, opt, train, batch, u_c, u_f) for _ in range(2)]
    a, b = _make_trainable(0, precision="f16x3"), _make_trainable(0, precision="bf16")
    oa, ob = train.Adam(a.parameters()), train.Adam(b.parameters())
    for step in range(2):
        oa.zero_grad()
        ob.zero_grad()
        la, _ = train.training_step(a, batch, True, True, 2.0, 6.0, u_coarse=u_c, u_fine=u_f)
        lb, _ = train.training_step(b, batch, True, True, 2.0, 6.0, u_coarse=u_c, u_fine=u_f)
        (la + lb).backward()  # one backward through both graphs: autograd interleaves them
        ga = [p.grad.detach().cpu().clone() for p in a.parameters()]
        gb = [p.grad.detach().cpu().clone() for p in b.parameters()]
        ob.step()
        oa.step()
        for (loss, grads, params), l2, g2, net in ((solo["f16x3"][step], la, ga, a),
                                                  (solo["bf16"][step], lb, gb, b)):
            assert torch.equal(loss, l2.detach().cpu())
            assert all(torch.equal(x, y) for x, y in zip(grads, g2))
            assert all(torch.equal(x, p.detach().cpu()) for x, p in zip(params, net.parameters()))
    # and the two precisions really differ
    assert not torch.equal(solo["f16x3"][0][1][0], solo["bf16"][0][1][0])
