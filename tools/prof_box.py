"""Frame time of box-bounded rendering (aonerf.render: box_side_length / cull) on the two bench
frames: the vanilla 640x480 frame and the articulated 320x240 frame, both from the bench's
create_spheric_poses(4.0)[7] camera at the SAPIEN focal length, box_side_length = 2.

Three variants -- unbounded (near 2, far 6), box with cull=False, box with cull=True -- in three
interleaved runs each (variant A, B, C, A, B, C, ...), warmed up as bench.py warms up (untimed
frames, synchronize, then K frames between two synchronizes).  Prints the hit fraction and the
ms per frame of every run, and writes the record to profiles/box/prof_box.json.

    python tools/prof_box.py [--steps 5] [--warmup 3] [--runs 3] [--out profiles/box]

The expectation the numbers are read against: culled time ~ unbounded time x hit fraction + a
fixed overhead (three small kernels and one 4-byte read-back).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "articulated-object-nerf_amd"))

BOX = 2
VARIANTS = ("unbounded", "box", "box_cull")


def frame_ms(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def measure(name, steps_of, hit_fraction, args):
    for v in VARIANTS:  # warm-up: schedules cached, weights packed, allocator pools grown
        for _ in range(args.warmup):
            steps_of[v]()
    runs = {v: [] for v in VARIANTS}
    for _ in range(args.runs):
        for v in VARIANTS:
            runs[v].append(frame_ms(steps_of[v], args.steps))
    rec = {"frame": name, "box_side_length": BOX, "hit_fraction": hit_fraction,
           "steps": args.steps, "warmup": args.warmup, "ms_per_frame": runs,
           "median_ms": {v: sorted(r)[len(r) // 2] for v, r in runs.items()}}
    m = rec["median_ms"]
    rec["culled_over_unbounded"] = m["box_cull"] / m["unbounded"]
    rec["overhead_ms_vs_model"] = m["box_cull"] - m["unbounded"] * hit_fraction
    print(f"{name}: hit fraction {hit_fraction:.4f}")
    for v in VARIANTS:
        print(f"  {v:10s} " + "  ".join(f"{x:8.3f}" for x in runs[v]) + "  ms/frame")
    print(f"  culled / unbounded = {rec['culled_over_unbounded']:.3f}; culled - unbounded x hit "
          f"fraction = {rec['overhead_ms_vs_model']:.3f} ms")
    return rec


def hit_fraction_of(rays):
    from aonerf import helper

    tmin, tmax = helper.get_ray_limits_box(rays["rays_o"], rays["rays_d"], BOX)
    return float(((tmax > tmin) & (tmax > 0)).float().mean().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box"))
    args = ap.parse_args()

    from aonerf.model import NeRF
    from aonerf.model_autodecoder import NeRF_AE_Art
    from aonerf.ray_utils import frame_rays
    from aonerf.render import create_spheric_poses, render_frame, render_rays, sapien_focal
    from aonerf.synthetic import art_latents, init_like_reference

    c2w = create_spheric_poses(4.0)[7]
    records = []

    H, W = 480, 640
    net = init_like_reference(NeRF()).cuda()

    def vanilla(name, focal):
        records.append(measure(name, {
            "unbounded": lambda: render_frame(net, c2w, H, W, focal, 2.0, 6.0, True),
            "box": lambda: render_frame(net, c2w, H, W, focal, white_bkgd=True,
                                        box_side_length=BOX, cull=False),
            "box_cull": lambda: render_frame(net, c2w, H, W, focal, white_bkgd=True,
                                             box_side_length=BOX, cull=True),
        }, hit_fraction_of(frame_rays(c2w, H, W, focal)), args))

    vanilla("vanilla 640x480", sapien_focal(H))
    # every ray hits: what compaction, the read-back and the scatter cost when they save nothing
    vanilla("vanilla 640x480, narrow field of view", 4.0 * sapien_focal(H))

    h, w = 240, 320
    art = init_like_reference(NeRF_AE_Art()).cuda()
    lat = art_latents(0, device="cuda")
    rays = frame_rays(c2w, h, w, sapien_focal(h))

    def art_model(sub, randomized, white_bkgd, near, far, **_):  # render_rays' model call
        return art(sub, randomized, white_bkgd, near, far, lat)

    records.append(measure("articulated 320x240", {
        "unbounded": lambda: render_rays(art_model, rays, None, True, 2.0, 6.0),
        "box": lambda: render_rays(art_model, rays, None, True, 2.0, 6.0, box_side_length=BOX,
                                   cull=False),
        "box_cull": lambda: render_rays(art_model, rays, None, True, 2.0, 6.0,
                                        box_side_length=BOX, cull=True),
    }, hit_fraction_of(rays), args))

    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "prof_box.json")
    with open(path, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "records": records}, fh, indent=1)
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
