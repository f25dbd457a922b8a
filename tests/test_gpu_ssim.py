"""SSIM (aon_image_ssim, aonerf.interface.ssim*) against the definition of piqa.ssim.SSIM()
with its defaults, as the reference's LitModel.ssim_each uses it (models/interface.py:101-111):
clip to [0, 1]; window g x g, g[i] ~ exp(-(i-5)^2 / (2 1.5^2)) normalised to sum 1, applied
without padding per channel; c1 = 0.01^2, c2 = 0.03^2; ss = (2 mx my + c1) / (mx^2 + my^2 + c1)
* (2 sxy + c2) / (sxx + syy + c2); plain mean over channels and positions.

The reference here is that definition in fp64 on the CPU (separable grouped conv2d).  Gate: 1e-6
absolute on every per-image value and every map element -- the outputs are fp32 of magnitude at
most 1 (rounding ~6e-8) and the kernel's fp64 window sums on fp32 inputs contribute ~1e-12, so
the bound leaves ~16x headroom; it is not fitted to a run.  (An fp32 evaluation of the same
definition misses it by ~50x on the near-flat case: E[x^2] - mx^2 cancels against c2.)"""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 1e-6
SHAPES = ("11x11", "11x37", "37x11", "24x32", "tiles")
CONTENTS = ("noise", "smooth+noise", "smooth+small", "flat", "white_bg")


def _shape(name):
    if name == "tiles":  # several tiles with ragged remainders both ways
        from aonerf import interface as I

        th, tw = I.SSIM_TILE
        return 2 * th + 13, 2 * tw + 17
    h, w = name.split("x")
    return int(h), int(w)


def ref_ssim_map(pred, gt):
    """(h, w, 3) CPU tensors -> (3, h-10, w-10) fp64 map of the definition above."""
    x = pred.float().clip(0, 1).permute(2, 0, 1)[None].double()
    y = gt.float().clip(0, 1).permute(2, 0, 1)[None].double()
    g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / (2 * 1.5 ** 2))
    g = g / g.sum()

    def blur(t):
        t = F.conv2d(t, g.view(1, 1, 1, 11).repeat(3, 1, 1, 1), groups=3)
        return F.conv2d(t, g.view(1, 1, 11, 1).repeat(3, 1, 1, 1), groups=3)

    c1, c2 = 0.01 ** 2, 0.03 ** 2
    mx, my = blur(x), blur(y)
    sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    return ((2 * mx * my + c1) / (mx * mx + my * my + c1) * cs)[0]


def _smooth(h, w):
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    return torch.stack([0.5 + 0.5 * torch.sin(6 * xx + 3 * yy), xx * yy,
                        (xx > 0.5).float() * 0.8 + 0.1], -1)


@functools.lru_cache(maxsize=None)
def _case(shape, content):
    """Seeded (pred, gt) CPU images and their fp64 reference map, built once per case."""
    h, w = _shape(shape)
    gen = torch.Generator().manual_seed(1000 * SHAPES.index(shape) + CONTENTS.index(content))
    if content == "noise":  # pred leaves [0, 1]: the clip
        gt = torch.rand((h, w, 3), generator=gen)
        pred = torch.rand((h, w, 3), generator=gen) * 1.2 - 0.1
    elif content == "smooth+noise":
        gt = _smooth(h, w)
        pred = gt + 0.1 * torch.randn((h, w, 3), generator=gen)
    elif content == "smooth+small":
        gt = _smooth(h, w)
        pred = gt + 0.003 * torch.randn((h, w, 3), generator=gen)
    elif content == "flat":  # the cancellation case
        gt = torch.full((h, w, 3), 0.7)
        pred = gt + 1e-3 * torch.randn((h, w, 3), generator=gen)
    else:  # white background (exactly 1.0) with a noisy textured rectangle
        r0, r1, c0, c1 = h // 4, h - h // 4, w // 4, w - w // 4
        gt = torch.ones((h, w, 3))
        gt[r0:r1, c0:c1] = _smooth(r1 - r0, c1 - c0)
        pred = gt.clone()
        pred[r0:r1, c0:c1] += 0.05 * torch.randn((r1 - r0, c1 - c0, 3), generator=gen)
    return pred, gt, ref_ssim_map(pred, gt)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_accuracy(shape, content):
    from aonerf import interface as I

    pred, gt, ref = _case(shape, content)
    h, w = _shape(shape)
    got = I.ssim_each([pred.cuda()], [gt.cuda()])
    assert got.shape == (1,) and got.dtype == torch.float32 and got.is_cuda
    err = abs(float(got[0].double().cpu()) - float(ref.mean()))
    m = I.ssim_map(pred.cuda(), gt.cuda())
    assert m.shape == (3, h - 10, w - 10) and m.dtype == torch.float32
    d = (m.double().cpu() - ref).abs()
    c, r, q = np.unravel_index(int(d.argmax()), d.shape)
    print(f"ssim {shape} {content}: value {float(ref.mean()):.8f} |err| {err:.3e}; "
          f"map max |err| {float(d.max()):.3e} at channel {c} row {r} col {q}")
    assert err <= TOL
    assert float(d.max()) <= TOL, (c, r, q)


@pytest.mark.parametrize("shape", ("24x32", "tiles"))
def test_batch_equals_single_calls(shape):
    """Three images of different content in one launch == three single-image launches, bit for
    bit (per-tile partial sums, summed per image in tile order)."""
    from aonerf import interface as I

    cases = [_case(shape, c) for c in ("noise", "flat", "white_bg")]
    preds, gts = [c[0].cuda() for c in cases], [c[1].cuda() for c in cases]
    batch = I.ssim_each(preds, gts)
    single = torch.cat([I.ssim_each([p], [g]) for p, g in zip(preds, gts)])
    assert batch.shape == (3,) and torch.equal(batch, single)
    for b, c in zip(batch.cpu(), cases):
        assert abs(float(b) - float(c[2].mean())) <= TOL


def test_inputs_as_stack_takes_them():
    """Non-contiguous and non-fp32 images are accepted (made contiguous fp32 first)."""
    from aonerf import interface as I

    pred, gt, ref = _case("24x32", "smooth+noise")
    p_t = pred.cuda().permute(1, 0, 2).contiguous().permute(1, 0, 2)  # strided view
    assert not p_t.is_contiguous()
    a = I.ssim_each([p_t], [gt.cuda().double()])
    assert torch.equal(a, I.ssim_each([pred.cuda()], [gt.cuda()]))


@pytest.mark.parametrize("shape", SHAPES)
def test_identity_is_exactly_one(shape):
    """x y and x x are then the same numbers, so numerator and denominator are bit-identical."""
    from aonerf import interface as I

    for content in ("noise", "flat"):
        x = _case(shape, content)[0].cuda()
        assert I.ssim_each([x], [x]).cpu().tolist() == [1.0]
        m = I.ssim_map(x, x)
        assert torch.equal(m, torch.ones_like(m))


def test_deterministic():
    from aonerf import interface as I

    pred, gt, _ = _case("tiles", "smooth+noise")
    p, g = [pred.cuda()] * 2, [gt.cuda(), pred.cuda()]
    a, b = I.ssim_each(p, g), I.ssim_each(p, g)
    assert torch.equal(a, b)
    with_map, m = I._image_ssim(p, g, want_map=True)  # the same launch, map requested
    assert torch.equal(with_map, a)
    assert torch.equal(m[0], I.ssim_map(p[0], g[0]))


def test_reference_dict_and_errors():
    from aonerf import interface as I

    cases = [_case("24x32", c) for c in ("noise", "smooth+small")]
    preds, gts = [c[0].cuda() for c in cases], [c[1].cuda() for c in cases]
    d = I.ssim(preds, gts)
    m = float(I.ssim_each(preds, gts).mean())
    assert d == {"name": "SSIM", "mean": m, "test": m}
    assert I.ssim(preds, gts, [0], [1], [1]) == d
    leg = I.ssim_legacy(preds[0], gts[0])
    assert leg.shape == (1,) and torch.equal(leg, I.ssim_each(preds[:1], gts[:1]))
    small = torch.rand(10, 40, 3).cuda()
    with pytest.raises(ValueError):
        I.ssim_each([small], [small])
    with pytest.raises(ValueError):
        I.ssim_each([small.permute(1, 0, 2)], [small.permute(1, 0, 2)])
    other = torch.rand(24, 33, 3).cuda()
    with pytest.raises(ValueError):  # shapes disagree within one list
        I.ssim_each([preds[0], other], [gts[0], other])
    with pytest.raises(ValueError):  # ... and between the lists
        I.ssim_each([preds[0]], [other])
    with pytest.raises(ValueError):
        I.ssim_each(preds, gts[:1])


def test_replays_from_a_graph():
    """aon_image_ssim neither allocates nor synchronises: with caller-owned outputs and
    workspace its two launches capture into one HIP graph (a single chain), and the replay
    equals the eager call."""
    from aonerf import _lib as L

    cases = [_case("tiles", c) for c in ("noise", "white_bg")]
    h, w = _shape("tiles")
    p = torch.stack([c[0] for c in cases]).cuda()
    g = torch.stack([c[1] for c in cases]).cuda()
    n = p.shape[0]
    nbytes = L.lib().aon_ssim_workspace_bytes(n, h, w)
    work = torch.empty((nbytes // 8,), dtype=torch.float64, device="cuda")
    out = torch.empty((n,), device="cuda")
    ss_map = torch.empty((n, 3, h - 10, w - 10), device="cuda")

    def run():
        L.call("aon_image_ssim", L.ptr(p), L.ptr(g), n, h, w, L.ptr(out), L.ptr(ss_map),
               L.ptr(work), nbytes, L.stream(p.device))

    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):  # warm-up: code objects loaded before the capture
        run()
        eager, eager_map = out.clone(), ss_map.clone()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    out.zero_()
    ss_map.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(ss_map, eager_map)
    for v, c in zip(out.cpu(), cases):
        assert abs(float(v) - float(c[2].mean())) <= TOL


def test_epoch_reports_ssim(tmp_path):
    """test_epoch(ssim=True) adds the SSIM dict and results.json entry; the default is unchanged."""
    from aonerf import interface as I
    from aonerf.datasets import SapienDataset
    from aonerf.model import NeRF
    from aonerf.parallel import render_frame_sharded
    from conftest import ROOT
    from oracle import weights as W

    root = os.path.join(ROOT, "tests", "golden", "data", "sapien_mini")
    ds = SapienDataset(root, "test" if os.path.isdir(os.path.join(root, "test")) else "val",
                       img_wh=(32, 24), white_back=True)
    net = NeRF().cuda().requires_grad_(False)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in W.nerf_state_dict(0).items()})

    with_dir, without_dir = tmp_path / "with", tmp_path / "without"
    stats = I.test_epoch(net, ds, out_dir=str(with_dir), ssim=True)
    assert len(stats) == 3 and [s["name"] for s in stats] == ["PSNR", "PSNR", "SSIM"]
    res = json.load(open(with_dir / "results.json"))
    assert sorted(res) == ["PSNR", "PSNR_obj", "SSIM"]
    assert res["SSIM"] == {"mean": stats[2]["mean"], "test": stats[2]["test"]}

    # the render is deterministic: the same views again give the epoch's SSIM exactly
    w, h = ds.img_wh
    rgbs, targets = [], []
    with torch.no_grad():
        for i, f in enumerate(ds.img_files_val):
            c2w = torch.FloatTensor(np.array(ds.meta["frames"][f.split(".")[0]]))[:3, :4]
            frame, _ = render_frame_sharded(net, c2w, h, w, ds.focal, ds.near, ds.far, True)
            rgbs.append(frame[:, :3].reshape(h, w, 3))
            targets.append(ds[i]["target"].reshape(h, w, 3))
    again = I.ssim(rgbs, targets)
    assert again["test"] == stats[2]["test"] and -1.0 <= again["test"] <= 1.0
    ref = np.mean([float(ref_ssim_map(a.cpu(), b.cpu()).mean()) for a, b in zip(rgbs, targets)])
    assert abs(again["test"] - ref) <= TOL

    plain = I.test_epoch(net, ds, out_dir=str(without_dir))
    assert isinstance(plain, tuple) and len(plain) == 2
    assert sorted(json.load(open(without_dir / "results.json"))) == ["PSNR", "PSNR_obj"]
    assert plain[0] == stats[0] and plain[1] == stats[1]
