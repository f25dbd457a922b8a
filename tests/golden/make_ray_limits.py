"""Generate tests/golden/ray_limits.npz by running the REFERENCE's box-bound helpers
(models/vanilla_nerf/helper.py): get_ray_limits_box (:42-102), get_ray_limits (:29-39) and
sample_along_rays with (B, 1) near / far (:106-133), in fp32 on the CPU.

Runs only where the reference tree is present (see _refimport.py); the fixture is data only.

    python tests/golden/make_ray_limits.py

Contents (SIDES = box_side_length 2 and 1.2, keyed "2" and "1p2"):
  frame_c2w (3, 4), frame_hwf; frame_rays_o / _rays_d / _viewdirs (768, 3): the 24 x 32 frame
      of create_spheric_poses(4.0)[0], its focal length chosen so that the box of side 2 is hit
      by a fraction of the rays strictly between 0.2 and 0.8 and by a count that is no multiple
      of 16 (asserted below);
  hand_rays_o / hand_rays_d (n, 3), hand_names, hand_degenerate (n,): hand-made rays; the
      degenerate ones (a zero direction component, a NaN limit, a graze with tmin == tmax) are
      the ones a float64 restatement need not agree on;
  none_rays_o / none_rays_d: a batch in which no ray is valid (get_ray_limits fills nothing);
  for SET in frame / hand / none and every side: SET_box_tmin_SIDE, SET_box_tmax_SIDE,
      SET_near_SIDE, SET_far_SIDE, each (n, 1);
  cam_c2w (3, 3, 4), cam_focal (3,), cam_hits (3,): the cameras of the culling test on the
      24 x 32 frame and box side 2 -- the fixture frame, the same camera turned away from the
      box (0 hits) and a narrow field of view (every ray hits) -- with the number of rays that
      hit (tmax > max(tmin, 0)) by the reference's limits on the reference's rays;
  samp_rays_o / samp_rays_d (77, 3), samp_near / samp_far (77, 1); for num_samples N in 64, 8:
      samp_t_eval_N, samp_t_lindisp_N, samp_u_N (the one torch.rand((B, N + 1)) the reference
      draws, drawn again from the same seed), samp_t_rand_N, samp_t_rand_lindisp_N.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _refimport  # noqa: E402

SIDES = (("2", 2), ("1p2", 1.2))
H, W = 24, 32
SEED = 20240607


def hits(tmin, tmax):
    return ((tmax > tmin) & (tmax > 0)).reshape(-1)


def hand_rays():
    """(name, origin, direction, degenerate)."""
    p6 = float(np.float32(0.6))
    n = np.array([0.3, 0.5, 0.8], np.float32)
    n /= np.linalg.norm(n)
    b = np.array([0.1, 0.05, 1.0], np.float32)
    b /= np.linalg.norm(b)
    return [
        ("parallel_inside_pos0", (0.5, 0.3, -4.0), (0.0, 0.0, 1.0), True),
        ("parallel_inside_neg0", (0.5, 0.3, -4.0), (-0.0, -0.0, 1.0), True),
        ("parallel_inside_mixed0", (-0.25, 0.3, 4.0), (-0.0, 0.0, -1.0), True),
        ("parallel_outside_pos0", (1.5, 0.0, -4.0), (0.0, 0.0, 1.0), True),
        ("parallel_outside_neg0", (1.5, 0.0, -4.0), (-0.0, 0.0, 1.0), True),
        ("parallel_outside_small_box", (0.8, 0.0, -4.0), (0.0, -0.0, 1.0), True),
        ("on_plane_side2_nan", (1.0, 0.0, -4.0), (0.0, 0.0, 1.0), True),
        ("on_plane_side2_nan_neg0", (-1.0, 0.0, -4.0), (-0.0, 0.0, 1.0), True),
        ("on_plane_side1p2_nan", (p6, 0.0, -4.0), (0.0, 0.0, 1.0), True),
        ("on_plane_y_nan", (0.2, 1.0, 3.0), (0.6, 0.0, -0.8), True),
        ("inside_box", (0.1, 0.2, -0.3), tuple(n), False),
        ("inside_box_negative_dir", (-0.2, 0.1, 0.25), tuple(-n), False),
        ("box_behind_axis", (0.0, 0.0, 4.0), (0.0, 0.0, 1.0), True),
        ("box_behind", (0.1, 0.2, 4.0), tuple(b), False),
        ("edge_graze_tmin_eq_tmax", (-3.0, -1.0, 0.0), (1.0, 1.0, 0.0), True),
        ("corner_graze_tmin_eq_tmax", (-3.0, -1.0, -1.0), (1.0, 1.0, 1.0), True),
        ("through_centre", (0.0, 0.0, -4.0), (0.0, 0.0, 1.0), True),
        ("zero_direction_inside", (0.1, -0.2, 0.3), (0.0, -0.0, 0.0), True),  # limits -inf, +inf
        ("oblique_hit",(-3.0, 0.4, 0.3), (1.0, -0.1, -0.05), False),
        ("oblique_miss", (-3.0, 0.4, 0.3), (1.0, 0.9, -0.05), False),
    ]


def main():
    helper, _, ray_utils, sapien_multi = _refimport.load()
    torch.set_num_threads(1)
    out = {}

    def limits(prefix, o, d):
        for key, side in SIDES:
            tmin, tmax = helper.get_ray_limits_box(o, d, side)
            near, far = helper.get_ray_limits(o, d, side)
            for name, v in (("box_tmin", tmin), ("box_tmax", tmax), ("near", near), ("far", far)):
                out[f"{prefix}_{name}_{key}"] = v.numpy().copy()

    def camera(c2w, focal):
        dirs = ray_utils.get_ray_directions(H, W, focal)
        o, v, d = ray_utils.get_rays(dirs, c2w, output_view_dirs=True)
        return o.contiguous(), d.contiguous(), v.contiguous()

    # ---- the frame: the focal length is the SAPIEN one (fovy 35 degrees) unless the box of
    # side 2 then fills too much of the frame; each candidate widens the field of view
    c2w = sapien_multi.create_spheric_poses(4.0)[0][:3, :4].contiguous()
    base = 0.5 * H / np.tan(0.5 * np.deg2rad(35.0))
    for focal in (base, base / 1.5, base / 2.0, base / 2.5, base / 3.0):
        o, d, v = camera(c2w, focal)
        n_hit = int(hits(*helper.get_ray_limits_box(o, d, 2)).sum())
        if 0.2 < n_hit / (H * W) < 0.8 and n_hit % 16 != 0:
            break
    else:
        raise SystemExit("no candidate focal length meets the hit-fraction conditions")
    print(f"frame: focal {focal:.4f}, {n_hit} of {H * W} rays hit ({n_hit / (H * W):.3f})")
    out.update(frame_c2w=c2w.numpy(), frame_hwf=np.array([H, W, focal]), frame_rays_o=o.numpy(),
               frame_rays_d=d.numpy(), frame_viewdirs=v.numpy())
    limits("frame", o, d)

    # ---- the cameras of the culling test
    away = c2w.clone()
    away[:, 0] = -away[:, 0]  # half a turn about the camera's y axis: the box is behind it
    away[:, 2] = -away[:, 2]
    cams = [(c2w, focal), (away, focal), (c2w, base * 8.0)]
    counts = []
    for m, f in cams:
        co, cd, _ = camera(m, f)
        counts.append(int(hits(*helper.get_ray_limits_box(co, cd, 2)).sum()))
    print("culling cameras: hits", counts)
    assert counts[0] == n_hit and counts[1] == 0 and counts[2] == H * W, counts
    out.update(cam_c2w=np.stack([m.numpy() for m, _ in cams]),
               cam_focal=np.array([f for _, f in cams], np.float64), cam_hits=np.array(counts))

    # ---- hand-made rays
    hr = hand_rays()
    ho = torch.tensor([r[1] for r in hr], dtype=torch.float32)
    hd = torch.tensor([r[2] for r in hr], dtype=torch.float32)
    out.update(hand_rays_o=ho.numpy(), hand_rays_d=hd.numpy(),
               hand_names=np.array([r[0] for r in hr]),
               hand_degenerate=np.array([r[3] for r in hr]))
    limits("hand", ho, hd)
    assert np.isnan(out["hand_box_tmax_2"]).any() and np.isnan(out["hand_box_tmax_1p2"]).any()
    g = [r[0] for r in hr].index("edge_graze_tmin_eq_tmax")
    assert out["hand_box_tmin_2"][g, 0] == out["hand_box_tmax_2"][g, 0] == 2.0

    # ---- a batch with no valid ray: nothing is filled, (-1, -2) clamp to (0, 0)
    no = torch.tensor([(3.0, 3.0, 4.0), (0.0, 2.5, 4.0), (-3.0, 0.5, 0.0), (1.5, 0.0, -4.0)])
    nd = torch.tensor([(0.0, 0.1, 1.0), (0.2, 1.0, 0.1), (-1.0, 2.0, 0.3), (0.0, 0.0, 1.0)])
    out.update(none_rays_o=no.numpy(), none_rays_d=nd.numpy())
    limits("none", no, nd)
    for key, _ in SIDES:
        assert not (out[f"none_box_tmax_{key}"] > out[f"none_box_tmin_{key}"]).any()
        assert (out[f"none_near_{key}"] == 0).all() and (out[f"none_far_{key}"] == 0).all()

    # ---- the fixture guards itself: a float64 slab test agrees on every non-degenerate ray
    for prefix, ro, rd, skip in (("frame", o, d, np.zeros(H * W, bool)),
                                 ("hand", ho, hd, out["hand_degenerate"])):
        for key, side in SIDES:
            want = slab_valid64(ro.numpy(), rd.numpy(), side)
            got = out[f"{prefix}_box_tmax_{key}"][:, 0] != -2
            assert (want == got)[~skip].all(), (prefix, key)

    # ---- the sampler on (B, 1) bounds
    B = 77
    rng = np.random.Generator(np.random.PCG64(77))
    so = torch.from_numpy((rng.random((B, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(4))
    sd = torch.from_numpy(rng.standard_normal((B, 3), dtype=np.float32))
    sd = sd / sd.norm(dim=-1, keepdim=True)
    near = torch.from_numpy(rng.random((B, 1), dtype=np.float32) * np.float32(2.5) + np.float32(0.5))
    far = near + torch.from_numpy(rng.random((B, 1), dtype=np.float32) * np.float32(3.5) + np.float32(0.5))
    out.update(samp_rays_o=so.numpy(), samp_rays_d=sd.numpy(), samp_near=near.numpy(),
               samp_far=far.numpy())
    for N in (64, 8):
        for name, lindisp in (("eval", False), ("lindisp", True)):
            t, _ = helper.sample_along_rays(so, sd, N, near, far, False, lindisp)
            out[f"samp_t_{name}_{N}"] = t.numpy().copy()
        for name, lindisp in (("rand", False), ("rand_lindisp", True)):
            torch.manual_seed(SEED + N)
            t, _ = helper.sample_along_rays(so, sd, N, near, far, True, lindisp)
            torch.manual_seed(SEED + N)
            u = torch.rand((B, N + 1))
            out[f"samp_t_{name}_{N}"] = t.numpy().copy()
            out[f"samp_u_{N}"] = u.numpy().copy()
    path = os.path.join(HERE, "ray_limits.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


def slab_valid64(o, d, side):
    """Whether each ray meets the box, by a float64 slab test (no NaN handling: callers skip the
    degenerate rays)."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (-side / 2 - o) / d, (side / 2 - o) / d
    lo, hi = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
    return lo <= hi


if __name__ == "__main__":
    main()
