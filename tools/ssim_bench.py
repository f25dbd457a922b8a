#!/usr/bin/env python3
"""Time aon_image_ssim (without the map) on a batch of random image pairs -- default 64 pairs of
640x480 -- against the reference's own path on the same GPU: piqa's SSIM as torch runs it, five
separable grouped torch.nn.functional.conv2d blurs (x, y, x^2, y^2, x y) in fp32 plus the
pointwise arithmetic, here on the whole batch at once (the reference loops over the images, which
only adds launches).  HIP events on the launch stream after warm-up; the two paths alternate
inside one process, `--inner` calls per event pair so a timed window is not a single short
launch; median and minimum over `--reps` windows.  Prints one JSON line: ms per batch for both,
the kernel's algorithmic GB/s counting the input bytes once (2 n H W 3 floats) and its fraction
of the 8 TB/s HBM peak, and the largest difference between the two paths' per-image values (the
torch path is the fp32 evaluation, so up to ~1e-4 is its own drift).  Hand-run; not part of
bench.py."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "articulated-object-nerf_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from aonerf import _lib as L  # noqa: E402

HBM_PEAK_GBS = 8000.0


def torch_ssim(pred, gt, win):
    """(n, H, W, 3) fp32 -> (n,): the definition as piqa evaluates it (fp32, valid convolutions)."""
    x = pred.clip(0, 1).permute(0, 3, 1, 2)
    y = gt.clip(0, 1).permute(0, 3, 1, 2)
    kh, kv = win.view(1, 1, 1, -1).repeat(3, 1, 1, 1), win.view(1, 1, -1, 1).repeat(3, 1, 1, 1)

    def blur(t):
        return F.conv2d(F.conv2d(t, kh, groups=3), kv, groups=3)

    c1, c2 = 0.01 ** 2, 0.03 ** 2
    mx, my = blur(x), blur(y)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, syy, sxy = blur(x * x) - mxx, blur(y * y) - myy, blur(x * y) - mxy
    ss = (2 * mxy + c1) / (mxx + myy + c1) * ((2 * sxy + c2) / (sxx + syy + c2))
    return ss.mean((1, 2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ssim_bench.py needs a GPU"
    n, h, w = args.images, args.height, args.width
    gen = torch.Generator(device="cuda").manual_seed(0)
    gt = torch.rand((n, h, w, 3), device="cuda", generator=gen)
    pred = (gt + 0.1 * torch.randn((n, h, w, 3), device="cuda", generator=gen)).contiguous()
    win = torch.exp(-(torch.arange(11, device="cuda", dtype=torch.float32) - 5) ** 2 / (2 * 1.5 ** 2))
    win = win / win.sum()
    nbytes = L.lib().aon_ssim_workspace_bytes(n, h, w)
    work = torch.empty((nbytes // 8,), dtype=torch.float64, device="cuda")
    out = torch.empty((n,), device="cuda")
    st = torch.cuda.current_stream()

    def run_kernel():
        L.call("aon_image_ssim", L.ptr(pred), L.ptr(gt), n, h, w, L.ptr(out), None, L.ptr(work),
               nbytes, L.stream())

    ref = [None]

    def run_torch():
        with torch.no_grad():
            ref[0] = torch_ssim(pred, gt, win)

    paths = {"aon_image_ssim": run_kernel, "torch_conv2d_fp32": run_torch}
    for fn in paths.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(args.reps):  # alternate the two paths
        for k, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            for _ in range(args.inner):
                fn()
            b.record(st)
            b.synchronize()
            times[k].append(a.elapsed_time(b) / args.inner)
    res = {"images": n, "height": h, "width": w, "reps": args.reps, "inner": args.inner}
    for k, ts in times.items():
        ts = sorted(ts)
        res[k] = {"ms_median": ts[len(ts) // 2], "ms_min": ts[0], "ms_max": ts[-1]}
    in_bytes = 2 * n * h * w * 3 * 4
    gbs = in_bytes / (res["aon_image_ssim"]["ms_median"] * 1e-3) / 1e9
    res["input_bytes"] = in_bytes
    res["kernel_GB/s"] = gbs
    res["kernel_frac_hbm_peak"] = gbs / HBM_PEAK_GBS
    res["speedup_vs_torch"] = res["torch_conv2d_fp32"]["ms_median"] / res["aon_image_ssim"]["ms_median"]
    res["max_abs_diff_vs_torch_fp32"] = float((out - ref[0]).abs().max())
    res["ssim_mean"] = float(out.mean())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
