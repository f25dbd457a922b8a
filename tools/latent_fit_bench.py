#!/usr/bin/env python3
"""Step time of the latent-code fit (aonerf/latent_fit.py) on 4,096 rays of the C5 articulated
workload (bench.py's views, model and code library), MLPs frozen, codes under Adam:

    latent  fit_step + backward + opt.step            (latent_only=True: aon_art_latent_grad)
    full    the same step with latent_only=False      (each level's 40 weight gradients formed and
                                                       dropped: what a frozen model cost before)

One process measures one arm at one precision: W warm-up steps, K steps on the host clock between
synchronises with no timers, then K more steps with the stage timers (HIP events) on.  --all runs
the arms interleaved, each in a fresh child process, `--repeats` times per precision, and writes
one JSON line per run.  Stage (a)'s algorithmic bytes are 768 columns x NR rows x the element
size; its share of HBM peak is reported over the whole aon_art_latent_grad call (three launches),
a lower bound for the column-sum kernel itself."""
import argparse
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "articulated-object-nerf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

NC, NF, NRAYS, H, W = 64, 128, 4096, 480, 640
PEAK_HBM_GBS = 8000.0  # bench.py's figure (spec)


def run_arm(arm, precision, steps, warmup):
    import numpy as np
    import torch

    from aonerf import latent_fit, tiles, train, train_art
    from aonerf.code_library import CodeLibraryArticulated
    from aonerf.model_autodecoder import NeRF_AE_Art
    from aonerf.ray_utils import frame_rays
    from aonerf.render import create_spheric_poses, sapien_focal
    from aonerf.synthetic import init_code_library, init_like_reference

    dev = torch.device("cuda", 0)
    net = latent_fit.freeze(init_like_reference(NeRF_AE_Art(train_precision=precision)).to(dev))
    lib = init_code_library(CodeLibraryArticulated(
        types.SimpleNamespace(N_max_objs=151, N_obj_code_length=128))).to(dev)
    ids = {"instance_id": torch.tensor([7], device=dev),
           "articulation_id": torch.tensor([3], device=dev)}
    codes = latent_fit.LatentCodes(init=lib(ids)).to(dev)
    opt = latent_fit.configure_optimizer(codes, 1e-3)
    poses = create_spheric_poses(4.0)
    focal = sapien_focal(H)
    views = [frame_rays(torch.as_tensor(poses[(5 * k) % len(poses)]), H, W, focal) for k in range(8)]
    rays_all = {k: torch.cat([v[k] for v in views], 0) for k in ("rays_o", "rays_d", "viewdirs")}
    rng = np.random.Generator(np.random.PCG64(3))
    target_all = torch.from_numpy(rng.uniform(0, 1, size=(8 * H * W, 3)).astype(np.float32)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1000)
    mlp_params = list(net.parameters())

    def step(timers=None):
        idx = torch.randint(0, 8 * H * W, (NRAYS,), device=dev, generator=gen)
        batch = {k: v[idx] for k, v in rays_all.items()}
        batch["target"] = target_all[idx]
        opt.zero_grad()
        loss, _ = train_art.step_on_latents(net, codes, batch, True, True, 2.0, 6.0, timers=timers,
                                            latent_only=arm == "latent")
        loss.backward()
        train.check_range({str(dev)}, mlp_params)
        opt.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    timers = {}
    for _ in range(steps):
        step(timers)
    torch.cuda.synchronize()
    stages = {k: float(np.mean([a.elapsed_time(b) for a, b, _ in v])) for k, v in sorted(timers.items())}
    rec = {"arm": arm, "precision": precision, "rays": NRAYS, "steps": steps, "warmup": warmup,
           "ms_per_step": ms, "stage_ms": stages}
    esize = 2 if precision == "bf16" else 4
    for S in (NC + 1, NC + 1 + NF):
        t = stages.get(f"art_dlatent{S}")
        if t:
            nbytes = 768 * tiles.rows(NRAYS * S) * esize
            rec[f"dlatent{S}"] = {"algorithmic_bytes": nbytes, "GB/s": nbytes / (t * 1e-3) / 1e9,
                                  "hbm_frac_of_8TBs": nbytes / (t * 1e-3) / 1e9 / PEAK_HBM_GBS}
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--arm", choices=("latent", "full"))
    ap.add_argument("--precision", choices=("f16x3", "bf16"), default="f16x3")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--all", action="store_true", help="every arm and precision, interleaved")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="JSONL file (--all)")
    args = ap.parse_args()
    if not args.all:
        print(json.dumps(run_arm(args.arm, args.precision, args.steps, args.warmup)), flush=True)
        return 0
    lines = []
    for precision in ("f16x3", "bf16"):
        for _ in range(args.repeats):
            for arm in ("full", "latent"):
                cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--precision",
                       precision, "--steps", str(args.steps), "--warmup", str(args.warmup)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                if r.returncode != 0:  # stop at the first failure: nothing more runs on the GPU
                    sys.stderr.write(r.stdout + r.stderr)
                    return r.returncode
                line = r.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                lines.append(line)
                if args.out:
                    with open(args.out, "w") as f:
                        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
