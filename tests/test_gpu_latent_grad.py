"""aon_art_latent_grad alone (csrc/latent_grad.hip): the latent-code gradients from four tiled
gradient tensors and the weights' latent columns, against fp64 torch on the CPU.

Sizes: N = 1, 15, 16, 17 (one 16-row block, with and without padding rows), 325 (5 rays x 65
samples), 4099 (257 blocks = 257 workgroups' partials, a padded last block) and 20003: stage (a)
runs min(blocks, 1024) workgroups, so only past 16,384 rows does a workgroup sum more than one
block -- 20003 rows are 1,251 blocks in uneven ranges of one and two, the last one padded.  Both
element types.  The padding rows N .. NR-1 of every tensor hold NaN: the kernel must not read
them.

Bound per output element: |got - ref| <= (N + n_out + 2) 2^-24 (sum_rows |dZ|)^T |W[:, cols]|,
both sides in fp64 (for dshape the sum of its three terms' bounds; bf16: the bf16-rounded inputs
on both sides) -- the fp32 summation bound of N row terms, n_out products and the final adds, in
any order; nothing measured enters it."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 15, 16, 17, 325, 4099, 20003]
WIDTHS = (128, 256, 256, 128)  # dzv[0], dz[5], dz[0], dzd[0]
# (tensor index, layer index in the kernels' order, first latent column, columns) per output
TERMS = {"dshape": [(1, 10, 256 + 63, 128), (2, 5, 63, 128), (3, 0, 3, 128)],
         "dapp": [(0, 15, 256 + 27, 128)],
         "dart": [(3, 0, 3 + 128, 32)]}
FULL = {0: 163, 5: 191, 10: 447, 15: 411}  # in-features of the four latent-carrying layers


@pytest.fixture(scope="module")
def weights():
    """Random parameters in the real shapes -> (pairs on the GPU, the weights in fp64 on the CPU)."""
    from aonerf import _lib as L

    g = torch.Generator().manual_seed(7)
    pairs = [(torch.randn((o, FULL.get(i, k)), generator=g) * 0.3, torch.randn((o,), generator=g))
             for i, (o, k) in enumerate(L.ART_SHAPES)]
    return [(w.cuda(), b.cuda()) for w, b in pairs], [w.double() for w, _ in pairs]


def _inputs(N, bf16):
    """Row-major (N, W) values (as the kernel's element type rounds them) and their tiled GPU
    copies with NaN in the padding rows."""
    from aonerf import tiles

    g = torch.Generator().manual_seed(1000 + N)
    dt = torch.bfloat16 if bf16 else torch.float32
    rows, tiled = [], []
    for i, W in enumerate(WIDTHS):
        x = (torch.randn((N, W), generator=g) * (0.5 + i)).to(dt)
        pad = torch.full((tiles.rows(N), W), float("nan"), dtype=dt)
        pad[:N] = x
        rows.append(x.double())
        tiled.append(tiles.tile(pad).cuda())
    return rows, tiled


def _call(L, prm, tiled, bf16, N, outs, work):
    L.call("aon_art_latent_grad", ctypes.byref(prm), *(L.ptr(t) for t in tiled), int(bf16), N,
           *(L.ptr(o) for o in outs), L.ptr(work), L.stream(work.device))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", SIZES)
def test_latent_grad_against_fp64(weights, N, bf16):
    from aonerf import _lib as L

    pairs, w64 = weights
    prm = L.mlp_art_params(pairs)
    rows, tiled = _inputs(N, bf16)
    nbytes = L.lib().aon_art_latent_grad_workspace_bytes(N)
    assert nbytes > 0

    def run(fill):
        outs = [torch.full((n,), fill, device="cuda") for n in (128, 128, 32)]  # garbage first
        work = torch.full((nbytes // 4,), float("nan"), device="cuda")
        _call(L, prm, tiled, bf16, N, outs, work)
        torch.cuda.synchronize()
        return dict(zip(("dshape", "dapp", "dart"), (o.cpu() for o in outs)))

    got, again = run(float("nan")), run(1e30)
    worst = 0.0
    for name, terms in TERMS.items():
        ref = torch.zeros(terms[0][3], dtype=torch.float64)
        bound = torch.zeros_like(ref)
        for t, layer, c0, n in terms:
            Wl = w64[layer][:, c0:c0 + n]
            ref += rows[t].sum(0) @ Wl
            bound += (N + Wl.shape[0] + 2) * 2.0 ** -24 * (rows[t].abs().sum(0) @ Wl.abs())
        assert torch.isfinite(got[name]).all(), f"{name}: not finite (padding rows read?)"
        err = (got[name].double() - ref).abs()
        ratio = float((err / bound).max())
        print(f"N={N} {'bf16' if bf16 else 'fp32'} {name}: max |err| {float(err.max()):.3e}, "
              f"max err/bound {ratio:.3f}")
        worst = max(worst, ratio)
        assert (err <= bound).all(), (name, ratio)
        # overwritten, not accumulated, and bit-identical from call to call
        assert torch.equal(got[name], again[name]), f"{name}: two calls differ"
    print(f"N={N}: worst err/bound {worst:.3f}")
