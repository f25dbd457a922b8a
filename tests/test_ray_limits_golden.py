"""The ray-limits fixture (tests/golden/ray_limits.npz, recorded from the reference by
tests/golden/make_ray_limits.py) guarded on the CPU: a float64 numpy slab test agrees with the
validity the reference recorded on every ray that is not one of the hand-made degenerate cases
(a zero direction component, a NaN limit, a graze with tmin == tmax), and the fixture holds the
cases and meets the conditions the GPU tests rely on."""
import numpy as np
import pytest

SIDES = (("2", 2.0), ("1p2", 1.2))


@pytest.fixture(scope="module")
def g(golden):
    return golden("ray_limits.npz")


def slab_valid64(o, d, side):
    o, d = o.astype(np.float64), d.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (-side / 2 - o) / d, (side / 2 - o) / d
    lo, hi = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
    return lo <= hi, lo, hi


@pytest.mark.parametrize("key,side", SIDES)
def test_float64_slab_test_agrees_on_validity(g, key, side):
    n_frame = len(g["frame_rays_o"])
    for prefix, skip in (("frame", np.zeros(n_frame, bool)), ("hand", g["hand_degenerate"])):
        want, lo, hi = slab_valid64(g[f"{prefix}_rays_o"], g[f"{prefix}_rays_d"], side)
        tmin, tmax = g[f"{prefix}_box_tmin_{key}"][:, 0], g[f"{prefix}_box_tmax_{key}"][:, 0]
        got = ~((tmin == -1) & (tmax == -2))
        keep = ~skip
        assert keep.sum() >= 5
        np.testing.assert_array_equal(got[keep], want[keep])
        ok = keep & want
        # and on the values, to fp32 accuracy of a few operations
        np.testing.assert_allclose(tmin[ok], lo[ok], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(tmax[ok], hi[ok], rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("key", [k for k, _ in SIDES])
def test_get_ray_limits_follows_from_the_box_limits(g, key):
    """helper.py:29-39 restated in numpy on the recorded box limits."""
    for prefix in ("frame", "hand", "none"):
        near, far = g[f"{prefix}_box_tmin_{key}"].copy(), g[f"{prefix}_box_tmax_{key}"].copy()
        valid = far > near
        if valid.any():
            near[~valid], far[~valid] = near[valid].min(), far[valid].max()
        near[near < 0] = 0
        far[far < 0] = 0
        np.testing.assert_array_equal(near, g[f"{prefix}_near_{key}"])
        np.testing.assert_array_equal(far, g[f"{prefix}_far_{key}"])


def test_fixture_holds_the_cases(g):
    names = set(g["hand_names"].tolist())
    for want in ("parallel_inside_pos0", "parallel_inside_neg0", "parallel_outside_pos0",
                 "parallel_outside_neg0", "on_plane_side2_nan", "on_plane_side1p2_nan",
                 "inside_box", "box_behind", "edge_graze_tmin_eq_tmax"):
        assert want in names
    d = g["hand_rays_d"]
    assert (np.signbit(d) & (d == 0)).any() and (~np.signbit(d) & (d == 0)).any()  # -0.0 and +0.0
    for key, _ in SIDES:
        assert np.isnan(g[f"hand_box_tmax_{key}"]).any()  # the 0 * inf of an origin on a plane
        assert np.isinf(g[f"hand_box_tmin_{key}"]).any()
        assert not (g[f"none_box_tmax_{key}"] > g[f"none_box_tmin_{key}"]).any()
        assert (g[f"none_near_{key}"] == 0).all() and (g[f"none_far_{key}"] == 0).all()
    i = g["hand_names"].tolist().index("edge_graze_tmin_eq_tmax")
    assert g["hand_box_tmin_2"][i, 0] == g["hand_box_tmax_2"][i, 0] == 2.0
    i = g["hand_names"].tolist().index("inside_box")
    assert g["hand_box_tmin_2"][i, 0] < 0 < g["hand_box_tmax_2"][i, 0] and g["hand_near_2"][i, 0] == 0
    i = g["hand_names"].tolist().index("box_behind")
    assert g["hand_box_tmin_2"][i, 0] < g["hand_box_tmax_2"][i, 0] < 0
    assert g["samp_near"].shape == (77, 1) and g["samp_t_eval_64"].shape == (77, 65)
    assert g["samp_t_rand_8"].shape == g["samp_u_8"].shape == (77, 9)


def test_culling_conditions(g):
    """The conditions of the culling test, on the reference's limits of the reference's rays."""
    tmin, tmax = g["frame_box_tmin_2"][:, 0], g["frame_box_tmax_2"][:, 0]
    n = int(((tmax > tmin) & (tmax > 0)).sum())
    hits = g["cam_hits"].tolist()
    assert hits[0] == n
    assert 0.2 < n / len(tmin) < 0.8
    assert n % 16 != 0
    assert hits[1] == 0 and hits[2] == len(tmin)
    np.testing.assert_array_equal(g["cam_c2w"][0], g["frame_c2w"])
    assert g["cam_focal"][0] == g["frame_hwf"][2]
