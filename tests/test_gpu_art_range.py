"""The fp16x3 range guard of the ARTICULATED kernels, site by site (include/aonerf.h
aon_mlp_read_status; tests/test_gpu_range.py pins the vanilla model's).

k_mlp_art_f16x3 (csrc/mlp_art.hip) ORs five sources into its one report -- ovf_of(x), ovf_of(y)
(the layer outputs hd0-3, h0-7, bot, hv0-3, alternating between the two fragments), enc.ovf
(pos_enc(x'), whose first three columns are x' itself), venc.ovf and din.ovf (the sample points)
-- and k_mlp_art_bwd adds d raw's splits and dL/dx'.  Each test here makes ONE of those tensors
leave the range and nothing else, so a term dropped from the OR, or tested one step late, fails.

The recipe (one hot unit).  For a layer, bias[0] = V on the golden weights: unit 0 of its output
is V (+ a remainder below 2, asserted) on every row.  The SILENT variant also zeroes column 0 of
every weight that reads that output, so unit 0 is disconnected: the network function no longer
depends on V at all.  Its reference is therefore the same network with unit 0 disconnected and
the bias left alone (``V=None``) -- not the unmodified network, whose unit 0 does feed the next
layer.  The kernels multiply the hot unit's hi / lo parts by exact zeros, so at every in-range V
the fused output is BIT-EQUAL to that reference's fused output (held on the MI355X; asserted).
x' is reached through deformation_layer.bias[0] = V (detection only: sin(2^9 12000) is not a
conditioned quantity), the points through a far origin.  The isolation conditions -- target
within 0.1% of V, remainder below 2, every other recorded tensor below 4000 -- are asserted on the
CPU from the oracle's record; they are conditions of the recipe, not measurements.

V: inside 6000, outside 12000, and the two edges 8150 / 8230 around the limit 65504 / 8 = 8188
(the layer epilogues test the fp16 hi part for inf, i.e. from 65520 / 8 = 8190 on: both edges
sit clear of either reading).
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu

VALUES = {"inside": 6000.0, "edge_inside": 8150.0, "edge_outside": 8230.0, "outside": 12000.0}
EXPECT = {"inside": 0, "edge_inside": 0, "edge_outside": 1, "outside": 1}
LAYER = {**{f"hd{i}": f"deformations_linear.{i}" for i in range(4)},
         **{f"h{i}": f"pts_linears.{i}" for i in range(8)},
         "bot": "bottleneck_layer",
         **{f"hv{i}": f"views_linear.{i}" for i in range(4)}}
# who reads a layer's output (its unit 0 is their input column 0: the skip layer's input is
# cat[h4, enc, shape], the view layer's cat[bottleneck, enc_dir, appearance])
READERS = {**{f"deformations_linear.{i}": [f"deformations_linear.{i + 1}"] for i in range(3)},
           "deformations_linear.3": ["deformation_layer"],
           **{f"pts_linears.{i}": [f"pts_linears.{i + 1}"] for i in range(7)},
           "pts_linears.7": ["density_layer", "bottleneck_layer"],
           "bottleneck_layer": ["views_linear.0"],
           **{f"views_linear.{i}": [f"views_linear.{i + 1}"] for i in range(3)},
           "views_linear.3": ["rgb_layer"]}
LAYER_SITES = list(LAYER)  # 17
SITES = LAYER_SITES + ["xp", "xyz", "xyz_only"]
PRE = ("coarse_mlp.", "fine_mlp.")
NAMES = ("density", "color", "articulation")


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------- the recipe
def hot_sd(site, V, silent=True):
    """The golden state dict with ``site``'s unit 0 at V in both levels (V None: bias kept) and,
    silent, that unit disconnected from its readers.  xp: deformation_layer.bias[0] = V (loud by
    nature).  xyz / xyz_only: the points are given by the caller; deformations_linear.0's xyz
    columns are zeroed (the deformation no longer reads the far point) and, xyz_only,
    deformation_layer.bias[0] = -V brings x' = delta + xyz back in range, so the points are the
    ONLY split tensor out of range."""
    sd = dict(W.art_state_dict(0))

    def edit(key):
        sd[key] = sd[key].copy()
        return sd[key]

    for pre in PRE:
        if site in LAYER:
            name = LAYER[site]
            if V is not None:
                edit(f"{pre}{name}.bias")[0] = V
            if silent:
                for r in READERS[name]:
                    edit(f"{pre}{r}.weight")[:, 0] = 0.0
        elif site == "xp":
            if V is not None:
                edit(f"{pre}deformation_layer.bias")[0] = V
        else:
            edit(f"{pre}deformations_linear.0.weight")[:, :3] = 0.0
            if site == "xyz_only" and V is not None:
                edit(f"{pre}deformation_layer.bias")[0] = -V
    return sd


def load(net, sd):
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net


def rays_of(B, S, seed=3):
    """(o, d, t) on the CPU: |o| <= 0.5, unit d, t in [2, 5] -- |o + t d| <= 5.5, below 0.1% of
    the smallest V, so a far point's coordinate stays within the condition."""
    gen = torch.Generator().manual_seed(seed + 131 * B + S)
    o = torch.rand(B, 3, generator=gen) - 0.5
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1)
    t = (2.0 + 3.0 * torch.rand(B, S, generator=gen)).sort(-1).values
    return o, d, t


def far(site, V, o, which):
    """The ray set with a far origin (V, 0, 0) + o: on ray ``which`` (xyz), on every ray
    (xyz_only: the bias -V shifts every row's x')."""
    o = o.clone()
    if site == "xyz":
        o[which, 0] += V
    elif site == "xyz_only":
        o[:, 0] += V
    return o


def lat_cpu():
    return {k: torch.from_numpy(v) for k, v in W.art_latents(1).items()}


def record(sd, level, o, d, v, t, dtype=torch.float32):
    """The oracle's intermediates of one level on these rays -> {name: (R, n) tensor}."""
    p = {k: x.to(dtype) for k, x in O.split_state_dict(sd)[level].items()}
    rec = {}
    with torch.no_grad():
        O.art_mlp_forward(p, O.cast_rays(t.to(dtype), o.to(dtype), d.to(dtype)),
                          O.pos_enc(v.to(dtype), 0, 4), {k: x.to(dtype) for k, x in lat_cpu().items()},
                          record=rec)
    out = {"xyz": rec["xyz"], "xp": rec["xp"], "bot": rec["bot"]}
    for grp, n in (("hd", 4), ("h", 8), ("hv", 4)):
        out.update({f"{grp}{i}": rec[grp][i] for i in range(n)})
    return out


def check_isolation(site, V, rec, far_rows=None):
    """The recipe's conditions, from the oracle's record: the target within 0.1% of V (a hot
    unit: on every row, its remainder below 2), every other recorded tensor below 4000.
    -> the target's maximum."""
    if site in LAYER:
        col = rec[site][:, 0]
        assert float((col - V).abs().max()) < 2.0, (site, V)
        target = float(col.abs().max())
        others = {k: float(x.abs().max()) for k, x in rec.items() if k not in (site, "xyz")}
        others[site + "[1:]"] = float(rec[site][:, 1:].abs().max())
    elif site == "xp":
        target = float(rec["xp"][:, 0].abs().max())
        assert float((rec["xp"][:, 0] - V).abs().max()) <= 1e-3 * V
        others = {k: float(x.abs().max()) for k, x in rec.items() if k not in ("xp", "xyz")}
        others["xp[1:]"] = float(rec["xp"][:, 1:].abs().max())
    else:
        rows = far_rows if far_rows is not None else slice(None)
        target = float(rec["xyz"][rows, 0].abs().max())
        assert float((rec["xyz"][rows, 0] - V).abs().max()) <= 1e-3 * V
        # (xyz: x' = delta + xyz follows the far point, the one tensor that cannot be isolated
        # from it without moving every row -- xyz_only does that)
        others = {k: float(x.abs().max()) for k, x in rec.items()
                  if k != "xyz" and not (site == "xyz" and k == "xp")}
    assert abs(target - V) <= 1e-3 * V, (site, V, target)
    worst = max(others, key=others.get)
    assert others[worst] < 4000.0, (site, V, worst, others[worst])
    return target


def status(buf):
    from aonerf import _lib as L

    st = ctypes.c_uint32(7)
    L.call("aon_mlp_read_status", L.ptr(buf), buf.numel() * 4, ctypes.byref(st),
           L.stream(buf.device))
    return st.value


@pytest.fixture(scope="module")
def art():
    from test_gpu_art_train import _make

    net, lib = _make(0)
    net.requires_grad_(False)
    return net, {k: cuda(v) for k, v in W.art_latents(1).items()}


@pytest.fixture(autouse=True)
def _consume_pending():
    """The training tests leave packs pending (some with an overflow on purpose): consumed
    here, so no later optimizer step in the session inherits them."""
    yield
    from aonerf import _lib as L

    L.check_pending()


def run_entry(mlp, entry, o, d, v, t, lat):
    """One launch of the fine MLP through ``entry`` -> (status after the pack, raw (R, 4),
    status after the launch)."""
    from aonerf import _lib as L

    B, S = t.shape
    packed0 = status(mlp.packed_weights(lat))
    if entry == "rays":
        raw = mlp.forward_rays(o, d, v, t, lat)
    else:
        pos = o[:, None, :] + t[..., None] * d[:, None, :]  # any points: the entry takes them as given
        cond = torch.empty((B, 27), device="cuda")
        L.call("aon_pos_enc", L.ptr(v), B, 0, 4, L.ptr(cond), L.stream())
        rgb, sig = mlp(pos.contiguous(), cond, lat)
        raw = torch.cat([rgb, sig], -1).reshape(-1, 4)
    return packed0, raw, status(mlp._art_packed)


SHAPES = [(1, 1), (3, 43)]  # 129 rows: one past a 128-row workgroup, a ragged 16-row tile


def detect(art, site, vname, entries=("rays", "points")):
    net, lat = art
    V = VALUES[vname]
    mlp = net.fine_mlp
    geom = {}
    for B, S in SHAPES:
        o, d, t = rays_of(B, S)
        of = far(site, V, o, 0)
        target = check_isolation(site, V, record(hot_sd(site, V), 1, of, d, d, t),
                                 far_rows=slice(0, S) if site == "xyz" else None)
        geom[(B, S)] = (o.cuda(), of.cuda(), d.cuda(), t.cuda(), target)
    base = {}
    if site in LAYER and EXPECT[vname] == 0:
        load(net, hot_sd(site, None))  # unit 0 disconnected, its bias kept: the reference
        for entry in entries:
            for shape, (o, of, d, t, _) in geom.items():
                p0, raw, st = run_entry(mlp, entry, o, d, d, t, lat)
                assert (p0, st) == (0, 0), (entry, shape, p0, st)
                base[(entry, shape)] = raw
    load(net, hot_sd(site, V))
    for entry in entries:
        for shape, (o, of, d, t, target) in geom.items():
            p0, raw, st = run_entry(mlp, entry, of, d, d, t, lat)
            print(f"{site} {vname} {entry} {shape}: oracle target max {target:.1f}, status after "
                  f"the pack {p0}, after the launch {st}")
            assert p0 == 0, "the pack itself must not report (biases are not range-limited)"
            assert st == EXPECT[vname], (site, vname, entry, shape, st)
            if st == 0:
                assert torch.isfinite(raw).all()
                if (entry, shape) in base:
                    ref = base[(entry, shape)]
                    assert torch.equal(raw, ref), (site, entry, shape,
                                                   float((raw - ref).abs().max()))


# ---------------------------------------------------------------------------- 1. detection
@pytest.mark.parametrize("vname", list(VALUES))
@pytest.mark.parametrize("site", SITES)
def test_detected_at_every_site(art, site, vname):
    """Every guarded tensor of aon_mlp_art_fwd (forward_rays) and aon_mlp_art_fwd_points
    (NeRFMLP.forward), at (B, S) = (1, 1) and (3, 43): the pack reports 0; the launch reports 0
    at 6000 and 8150, 1 at 8230 and 12000.  At every status-0 case of a layer site the raw output
    is bit-equal to the fused output of the network with unit 0 disconnected at its own bias
    (bit-equality held; no fp64 fall-back gate was needed)."""
    detect(art, site, vname)


# ---------------------------------------------------------------------------- 2. selectivity
W_SEL = 1000.0  # the largest round weight the fp16x3 stream holds (|w| <= 1023 at its 2^6 scale)


def selective_sd(w):
    """views_linear.0's unit 0 = ReLU(w * viewdir_x): row 0 zero but for column 256 (the first
    cond column, the raw direction's x), bias 0 zero, unit 0 disconnected from views_linear.1."""
    sd = hot_sd("hv0", None)
    for pre in PRE:
        sd[f"{pre}views_linear.0.weight"] = sd[f"{pre}views_linear.0.weight"].copy()
        sd[f"{pre}views_linear.0.bias"] = sd[f"{pre}views_linear.0.bias"].copy()
        sd[f"{pre}views_linear.0.weight"][0, :] = 0.0
        sd[f"{pre}views_linear.0.weight"][0, 256] = w
        sd[f"{pre}views_linear.0.bias"][0] = 0.0
    return sd


def selective_rays():
    """129 single-sample rays, |d_x| <= 0.3 on all but the last, whose d = (1, 0, 0): the last
    ray is row 128, the one live row of the second, partial workgroup."""
    o, d, t = rays_of(129, 1)
    gen = torch.Generator().manual_seed(11)
    dx = 0.29 * (2.0 * torch.rand(129, generator=gen) - 1.0)
    phi = 6.2831853 * torch.rand(129, generator=gen)
    r = torch.sqrt(1.0 - dx * dx)
    d = torch.stack([dx, r * torch.cos(phi), r * torch.sin(phi)], -1)
    d[-1] = torch.tensor([1.0, 0.0, 0.0])
    assert float(d[:-1, 0].abs().max()) <= 0.3
    return o, d, t


@pytest.mark.parametrize("entry", ["rays", "points"])
@pytest.mark.parametrize("K,want", [(12000.0, 1), (6000.0, 0)])
def test_only_the_last_row_overflows(art, K, want, entry):
    """Unit 0 of views_linear.0 is ReLU(K d_x), a per-ray value: K = 12000 puts ONLY the last
    ray's row (row 128: the second workgroup's single live row) out of range and must report 1;
    K = 6000 reports 0.  K is the product of the weight 1000 and view directions scaled by
    K / 1000: a weight of K itself is beyond what the fp16x3 stream holds (|w| <= 1023), which the
    pack reports as 2 whatever the inputs (test_pack_refuses_a_weight_beyond_the_stream)."""
    net, lat = art
    o, d, t = selective_rays()
    v = d * (K / W_SEL)
    sd = selective_sd(W_SEL)
    rec = record(sd, 1, o, d, v, t)
    u0 = rec["hv0"][:, 0]
    assert abs(float(u0[-1]) - K) <= 1e-3 * K and float(u0[:-1].max()) <= 0.3 * K + 1e-3 < 4000.0
    others = {k: float(x.abs().max()) for k, x in rec.items() if k != "hv0"}
    assert max(others.values()) < 4000.0 and float(rec["hv0"][:, 1:].abs().max()) < 4000.0
    load(net, sd)
    p0, raw, st = run_entry(net.fine_mlp, entry, o.cuda(), d.cuda(), v.cuda(), t.cuda(), lat)
    print(f"hv0 = ReLU({K:.0f} d_x) {entry}: oracle unit 0 last row {float(u0[-1]):.1f}, others <= "
          f"{float(u0[:-1].max()):.1f}; status after the pack {p0}, after the launch {st}")
    assert (p0, st) == (0, want)


def test_pack_refuses_a_weight_beyond_the_stream(art):
    """The same unit written with the weight 12000 (or 6000) never reaches the activation guard:
    aon_mlp_art_pack reports 2 (a weight whose scaled fp16 hi part is not finite)."""
    net, lat = art
    for K in (12000.0, 6000.0):
        load(net, selective_sd(K))
        assert status(net.fine_mlp.packed_weights(lat)) == 2


@pytest.mark.parametrize("entry", ["rays", "points"])
def test_far_origin_on_the_last_ray_only(art, entry):
    """The far point on the last of 129 single-sample rays (row 128 alone): reports 1."""
    net, lat = art
    o, d, t = rays_of(129, 1)
    V = VALUES["outside"]
    of = far("xyz", V, o, 128)
    sd = hot_sd("xyz", V)
    target = check_isolation("xyz", V, record(sd, 1, of, d, d, t), far_rows=slice(128, 129))
    load(net, sd)
    p0, raw, st = run_entry(net.fine_mlp, entry, of.cuda(), d.cuda(), d.cuda(), t.cuda(), lat)
    print(f"xyz last ray {entry}: oracle target max {target:.1f}, status {p0} -> {st}")
    assert (p0, st) == (0, 1)
    assert torch.isfinite(raw[:128]).all()  # the other rows are unaffected


@pytest.mark.parametrize("entry", ["rays", "points"])
@pytest.mark.parametrize("B,S", [(1, 1), (3, 43), (77, 65)])
def test_padded_rows_never_report(art, B, S, entry):
    """All-normal rays on the golden weights: status 0 -- the rows a partial workgroup pads its
    last tile with never trip the guard."""
    net, lat = art
    load(net, dict(W.art_state_dict(0)))
    o, d, t = rays_of(B, S)
    p0, raw, st = run_entry(net.fine_mlp, entry, o.cuda(), d.cuda(), d.cuda(), t.cuda(), lat)
    assert (p0, st) == (0, 0) and torch.isfinite(raw).all()


# ---------------------------------------------------------------------------- 3. loud, in range
def fused_train_forward(mlp, o, d, v, t, lat):
    """aon_mlp_art_fwd_train on one level -> (raw, x' (R, 3), the pack)."""
    from aonerf import tiles, train_art

    geo = train_art._Geo(mlp)
    P = [(m.weight.detach(), m.bias.detach()) for m in train_art.art_layers(mlp)]
    raw = torch.empty((t.numel(), 4), device="cuda")
    xyz, hd, enc, h, bot, hv = train_art._forward_level_fused(
        geo, P, tuple(lat[k] for k in NAMES), o, d, v, t, raw)
    return raw, tiles.untile(enc, t.numel())[:, :3].contiguous(), (geo, P, xyz, hd, enc, h, bot, hv)


def test_large_in_range_value_is_carried_accurately(art):
    """pts_linears.3's unit 0 at 6000 with its outgoing column KEPT (loud): h4.. and the raw
    outputs now depend on a value 73% of the way to the limit.  The fused f16x3 raw (inference
    and training forward) against the fp64 evaluation at the kernel's own x' (as
    test_art_c5_level_stage_isolated), at test_gpu_fold.py's raw gate 1e-5 max(1, max |raw|).
    Measured on the MI355X, (3, 43) rays: max |f16x3 - fp64| 1.6e-4 at max |raw| 178 (9e-7
    relative, gate 1.8e-3), the inference kernel and the training forward alike."""
    from aonerf import _lib as L

    net, lat = art
    V = VALUES["inside"]
    sd = hot_sd("h3", V, silent=False)
    B, S = SHAPES[1]
    o, d, t = rays_of(B, S)
    rec = record(sd, 1, o, d, d, t)
    col = rec["h3"][:, 0]
    assert float((col - V).abs().max()) < 2.0
    assert max(float(x.abs().max()) for k, x in rec.items() if k != "h3") < 4000.0
    load(net, sd)
    mlp = net.fine_mlp
    oc, dc, tc = o.cuda(), d.cuda(), t.cuda()
    raw_t, xp, _ = fused_train_forward(mlp, oc, dc, dc, tc, lat)
    raw_i = mlp.forward_rays(oc, dc, dc, tc, lat)
    assert status(mlp._art_packed) == 0
    venc = torch.empty((B, 27), device="cuda")
    L.call("aon_pos_enc", L.ptr(dc), B, 0, 4, L.ptr(venc), L.stream())
    p64 = {k: x.double() for k, x in O.split_state_dict(sd)[1].items()}
    with torch.no_grad():
        rgb64, sig64 = O.art_mlp_forward(
            p64, O.cast_rays(t.double(), o.double(), d.double()), venc.cpu().double(),
            {k: x.double() for k, x in lat_cpu().items()}, xp_fixed=xp.cpu())
    want = torch.cat([rgb64.reshape(-1, 3), sig64.reshape(-1, 1)], -1)
    gate = 1e-5 * max(1.0, float(want.abs().max()))
    for name, raw in (("inference", raw_i), ("training forward", raw_t)):
        err = float((raw.cpu().double() - want).abs().max())
        print(f"h3 unit 0 = {V:.0f}, loud, {name}: max |raw| {float(want.abs().max()):.1f}, "
              f"max |f16x3 - fp64| {err:.3e}, gate {gate:.3e}")
        assert err <= gate, (name, err, gate)


# ---------------------------------------------------------------------------- 4. render fallback
def eval_rays(golden, n=24):
    g = golden("articulated.npz")
    return {k: torch.from_numpy(g[f"eval_{k}"][:n]) for k in ("rays_o", "rays_d", "viewdirs")}


def render(net, rays, lat, randomized=False):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            ret = net(rays, randomized, True, 2.0, 6.0, lat, return_weights=True,
                      return_intermediates=True)
    return ret, [x for x in w if issubclass(x.category, RuntimeWarning)
                 and "exceeded the fused fp16x3 range" in str(x.message)]


def check_chain(ret, rc, params):
    """tests/test_gpu_articulated.py's chain at 1e-4 against the oracle: coarse level; fine t ==
    sample_pdf of OUR coarse weights, bit for bit; fine level at those t."""
    worst = 0.0
    t_c, w_c = ret[0][4]["t_vals"].cpu(), ret[0][3].cpu()
    coarse = O.art_render_level(params, rc, t_c, 0, True, lat_cpu())
    t_f, _ = O.sample_pdf(0.5 * (t_c[..., 1:] + t_c[..., :-1]), w_c[..., 1:-1], rc["rays_o"],
                          rc["rays_d"], t_c, 128, False)
    np.testing.assert_array_equal(ret[1][4]["t_vals"].cpu().numpy(), t_f.numpy())
    fine = O.art_render_level(params, rc, t_f, 1, True, lat_cpu())
    for lv, ref in ((0, coarse), (1, fine)):
        for j, jj in ((0, 0), (1, 1), (3, 2), (2, 3)):  # comp, acc, depth, weights
            assert torch.isfinite(ret[lv][jj]).all()
            err = float((ret[lv][jj].cpu().double() - ref[j].double()).abs().max())
            worst = max(worst, err)
            assert err <= 1e-4, (lv, jj, err)
    return worst


@pytest.mark.parametrize("site", ["h3", "hd1", "hv2"])
def test_render_falls_back_and_matches_the_oracle(art, golden, site):
    """NeRF_AE_Art under no_grad on 24 golden eval rays with a silent hot unit in both levels'
    MLPs.  Outside: exactly one "exceeded the fused fp16x3 range" RuntimeWarning, both fused
    flags restored, every tensor finite, every link within the 1e-4 chain gates against the
    oracle (on the network with unit 0 disconnected: the same function); the randomized render
    equals, bit for bit, a hand-made layer-by-layer render from the same RNG state (the saved-state
    replay).  Inside: no warning, the same gates on the fused path.  ``range_check=False`` turns
    the guarantee OFF: no warning is raised and the outputs are whatever the overflow made."""
    net, lat = art
    rc = eval_rays(golden)
    rays = {k: v.cuda() for k, v in rc.items()}
    params = O.split_state_dict(hot_sd(site, None))
    mlps = (net.coarse_mlp, net.fine_mlp)
    # inside: the fused path stays
    load(net, hot_sd(site, VALUES["inside"]))
    ret, warns = render(net, rays, lat)
    assert not warns
    print(f"{site} inside, fused: worst chain link {check_chain(ret, rc, params):.2e}")
    # outside: one warning, the fallback matches
    load(net, hot_sd(site, VALUES["outside"]))
    ret, warns = render(net, rays, lat)
    assert len(warns) == 1, [str(x.message) for x in warns]
    assert all(m.fused for m in mlps)
    print(f"{site} outside, fallback: worst chain link {check_chain(ret, rc, params):.2e}")
    # randomized: the fallback replays the first attempt's random draws
    state = torch.cuda.get_rng_state("cuda")
    a, warns = render(net, rays, lat, randomized=True)
    assert len(warns) == 1 and all(m.fused for m in mlps)
    for m in mlps:
        m.fused = False
    try:
        torch.cuda.set_rng_state(state, "cuda")
        b, warns = render(net, rays, lat, randomized=True)
    finally:
        for m in mlps:
            m.fused = True
    assert not warns
    for lv in range(2):
        for j in range(4):
            assert torch.isfinite(a[lv][j]).all() and torch.equal(a[lv][j], b[lv][j]), (lv, j)
        assert torch.equal(a[lv][4]["t_vals"], b[lv][4]["t_vals"])
    # range_check off: the guard is not consulted
    net.range_check = False
    try:
        _, warns = render(net, rays, lat)
    finally:
        net.range_check = True
    assert not warns and all(m.fused for m in mlps)


# ---------------------------------------------------------------------------- 5. training
def train_batch(golden, n=4):
    g = golden("art_train_step.npz")
    b = {k: cuda(g[k][:n]) for k in ("rays_o", "rays_d", "viewdirs", "target")}
    b["instance_id"] = torch.tensor([int(g["instance_id"])], device="cuda")
    b["articulation_id"] = torch.tensor([int(g["articulation_id"])], device="cuda")
    return b


def make_trainable(numerics):
    from test_gpu_art_train import _make

    return _make(0, **numerics)


def step_once(net, lib, opt, batch):
    from aonerf import train_art

    opt.zero_grad()
    loss, logs = train_art.training_step(net, lib, batch, False, True, 2.0, 6.0)
    loss.backward()
    return loss, logs


def make_opt(kind, net, lib):
    from aonerf import train_art

    if kind == "aon_adam":
        return train_art.configure_optimizers(net, lib)
    return torch.optim.Adam(list(net.parameters()) + list(lib.parameters()), lr=5e-4)


MODES = {"f16x3": {}, "bf16": dict(precision="bf16"),
         "bf16_trunk": dict(precision="bf16", art_forward="bf16_trunk")}
# what each training forward splits into fp16 (csrc/mlp_art.hip, PREC): the deformation MLP in
# every mode; the trunk, bottleneck and view branch in f16x3 and in bf16's default forward
# (f16_acts: fp16 activations, the layer epilogue's test as in fp16x3); in bf16_trunk they are
# bf16 values with fp32's exponent range -- nothing to overflow, nothing reported
REPORTS = {("f16x3", "hd1"): True, ("f16x3", "h3"): True, ("bf16", "hd1"): True,
           ("bf16", "h3"): True, ("bf16_trunk", "hd1"): True, ("bf16_trunk", "h3"): False}


@pytest.mark.parametrize("opt_kind", ["aon_adam", "torch_adam"])
@pytest.mark.parametrize("mode,site", list(REPORTS), ids=[f"{m}-{s}" for m, s in REPORTS])
def test_training_step_refused(golden, mode, site, opt_kind):
    """One train_art.training_step + backward with a silent hot unit at 12000 in both levels,
    then the optimizer's step (train_art.configure_optimizers' Adam, and torch.optim.Adam over
    the same parameters through the global pre-hook): FloatingPointError, every MLP parameter and
    every code-library table bit-equal to before; a step at 6000 afterwards goes through.
    "Range-guarded likewise" (include/aonerf.h) holds for what a mode splits into fp16: the
    deformation MLP always, the trunk in f16x3 and in bf16's default forward.  bf16_trunk keeps
    the trunk as bf16 values (no fp16 split, no range limit): there h3 at 12000 cannot overflow,
    so instead the forward must be finite and equal, bit for bit, to the 6000 run's rendered
    tensors (unit 0 is disconnected: only the kept h3 differs), and the step goes through."""
    batch = train_batch(golden)
    net, lib = make_trainable(MODES[mode])
    opt = make_opt(opt_kind, net, lib)
    tensors = list(net.parameters()) + list(lib.parameters())
    load(net, hot_sd(site, VALUES["outside"]))
    if REPORTS[(mode, site)]:
        step_once(net, lib, opt, batch)
        before = [p.detach().clone() for p in tensors]
        with pytest.raises(FloatingPointError):
            opt.step()
        assert all(torch.equal(a, p.detach()) for a, p in zip(before, tensors))
    else:
        outs = {}
        for vname in ("outside", "inside"):
            load(net, hot_sd(site, VALUES[vname]))
            ret = net(batch, False, True, 2.0, 6.0, lib(batch))
            outs[vname] = [x.detach().clone() for lv in ret for x in lv]
        assert all(torch.isfinite(x).all() for x in outs["outside"])
        assert all(torch.equal(a, b) for a, b in zip(outs["outside"], outs["inside"]))
        load(net, hot_sd(site, VALUES["outside"]))
        step_once(net, lib, opt, batch)
        opt.step()
    # inside the range the same step goes through
    load(net, hot_sd(site, VALUES["inside"]))
    loss, _ = step_once(net, lib, opt, batch)
    opt.step()
    assert torch.isfinite(loss)
    assert all(torch.isfinite(p).all() for p in tensors)


def test_backward_chain_reports_an_overflowing_gradient(art):
    """aon_mlp_art_bwd (train_art._backward_level_fused) on in-range weights and a ragged batch
    (129 rows).  d raw is split at a per-call power-of-two scale from its own maximum
    (grad_scale, csrc/aon_common.hpp: |x s| < 2^8), so every FINITE d raw is representable in
    that split -- 1e30 included; an inf (the scale then falls back to 1) in the last row must set
    the backward pack's status word, a normal d raw must leave it 0."""
    from aonerf import _lib as L
    from aonerf import level, train_art

    net, lat = art
    load(net, dict(W.art_state_dict(0)))
    B, S = SHAPES[1]
    o, d, t = rays_of(B, S)
    oc, dc, tc = o.cuda(), d.cuda(), t.cuda()
    raw, _, (geo, P, xyz, hd, enc, h, bot, hv) = fused_train_forward(net.fine_mlp, oc, dc, dc, tc, lat)
    venc = torch.empty((B, 27), device="cuda")
    L.call("aon_pos_enc", L.ptr(dc), B, 0, 4, L.ptr(venc), L.stream())
    lat_t = tuple(lat[k] for k in NAMES)
    gen = torch.Generator().manual_seed(5)
    base = torch.randn(B * S, 4, generator=gen) * 1e-3
    for name, last, want in (("normal", None, 0), ("inf", float("inf"), 1)):
        draw = base.clone()
        if last is not None:
            draw[-1, 1] = last
        G = [(torch.empty_like(w), torch.empty_like(b)) for w, b in P]
        dlat = tuple(torch.empty_like(x) for x in lat_t)
        train_art._backward_level_fused(geo, P, G, lat_t, dlat, xyz, enc, venc, S, hd, h, bot, hv,
                                        draw.cuda())
        buf = level.buffer("train_art", f"bwd{S}", L.lib().aon_mlp_art_bwd_packed_bytes(), "cuda:0")
        st = status(buf)
        print(f"backward chain, d raw {name}: status {st}")
        assert st == want, (name, st)
        if want == 0:
            assert all(torch.isfinite(g).all() for pair in G for g in pair)
