"""Median depth of stage-3 and human-only rays from the composite launch (`hos_merge_composite_median_fwd`,
`hos_raw2outputs_median_fwd`) against its definition (tests/_median_expect.py: stage 1's `sorted_interp(0.5, integrate_weights(w), t)` on
the weights of `_raw2outputs`, knots [z_0 .. z_{S-1}, z_{S-1}]), hand cases with exact weights, the same-launch guarantees, the module
and frame surface (`median=True`) and the launcher's `run.render_median`.

Bound of the kernel test, the rule of tests/test_gpu_bkgd_maps.py: with F the fp64 CDF of the ray (knots t, values integrate_weights of
the fp64 weights, linear in between) evaluated at the kernel's depth,
    |F - 0.5| <= 2 * max_rays |F(fp32 definition) - 0.5| + S * 2^-23 + 2 * ulp32(t) * slope,
S the number of samples the ray composites; in a zero-width interval (the last sample, coinciding depths) every value between its knots
counts.  No ray is excluded."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle.human as oh
from hosnerf_amd import synth
from tests import _bkgd_maps_expect as X
from tests import _median_expect as ME
from tests import test_gpu_maps as TM
from tests.test_gpu_maps import dev, hos  # noqa: F401  (fixtures of the stage-3 parity tests, read-only)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -23
ALL_KEYS = TM.MAPS + ("depth_median",)
RANDOM_CASES = [("r1x1", 1, 1, 51), ("r32x33", 32, 33, 52), ("r128x128", 128, 128, 53)]       # S = 2; 65: per = 2, ragged last lane; 256 = MAXS, per = 4


# ------------------------------------------------------------------------------------------ the definition on one batch
def merged_rows(td, bden, hum_sigma, mask, d, z_h):
    """The samples each ray composites, in sorted order, as the kernel's C2 / C3 take them (oracle/human.py:339-349): per group of rays
    (foreground: the stable z-sort of Sb background + Sh human samples; background-only: the Sb background samples, all-ones mask)
    a tuple (selector [B] bool, z [n,S], sigma [n,S], mask [n,S], d [n,3], order [n,S] or None).  CPU tensors."""
    z_b = td[..., :-1]
    fg = mask.sum(-1) > 5e-3
    groups = []
    if int(fg.sum()) > 0:
        zz, order = torch.sort(torch.cat([z_b[fg], z_h[fg]], -1), dim=-1, stable=True)
        sig = torch.gather(torch.cat([bden[fg], hum_sigma[fg]], -1), 1, order)
        m = torch.gather(torch.cat([torch.ones_like(z_b[fg]), mask[fg]], -1), 1, order)
        groups.append((fg, zz, sig, m, d[fg], order))
    if int((~fg).sum()) > 0:
        bg = ~fg
        groups.append((bg, z_b[bg], bden[bg], torch.ones_like(z_b[bg]), d[bg], None))
    return groups


def definition(z, sigma, m, d, dtype, last_dist=1e10):
    """(median [n], knots [n,S+1], cw [n,S+1]) of the definition in `dtype` on one group's rows."""
    c = lambda t: t.to(dtype)
    if z.shape[1] == 1:             # one sample: its interval is last_dist (M:77-81), T = 1; the oracle's concatenation needs two samples
        w = (1.0 - torch.exp(-c(sigma) * (last_dist * torch.norm(c(d), dim=-1, keepdim=True)))) * c(m)
    else:
        w = oh.raw2outputs(torch.zeros(z.shape + (3,), dtype=dtype), c(sigma), c(z), c(d), c(m), None, last_dist)[2]
    return ME.median_definition(w, c(z))


RERUN_UNIT, RERUN_DEPTH = 1e-6, 1.1e-5     # the project's bounds for another chunking of a frame (tests/test_gpu_maps.py:277-287)


def cdf_distance(t_hip, z, sigma, m, d, last_dist=1e10, foreign_knots=False, rerun=False):
    """Per ray of one group: (|F(t_hip) - 0.5| [n], the bound's ray-dependent part S * 2^-23 + 2 ulp32(t) slope [n], |F(fp32 definition)
    - 0.5| [n], the fp32 and fp64 medians).  `foreign_knots`: the knots come from another evaluation of the ray's human depths (the
    oracle's z_h on the CPU), so a kernel depth a rounding outside [t_0, t_S] is moved to the nearer end (`cdf_at(clamp=True)`).
    `rerun`: `t_hip` comes from ANOTHER run of the same rays (other chunks, other ranks) than the rows: unit-scale quantities of the
    two runs -- the CDF's values -- differ by up to RERUN_UNIT and depths by RERUN_DEPTH * max(1, |t|), which the slope maps into CDF space."""
    S = z.shape[1]
    med32, _, _ = definition(z, sigma, m, d, torch.float32, last_dist)
    med64, t64, cw64 = definition(z, sigma, m, d, torch.float64, last_dist)
    t_hip = t_hip.cpu().numpy().astype(np.float32)
    F, slope = X.cdf_at(t_hip, t64.numpy(), cw64.numpy(), clamp=foreign_knots or rerun)
    # the fp32 definition has no final min: its last addition may round one ulp past the last knot
    F32, _ = X.cdf_at(med32.numpy(), t64.numpy(), cw64.numpy(), clamp=True)
    own = S * ULP + 2.0 * np.spacing(np.abs(t_hip)).astype(np.float64) * slope
    if rerun:
        own = own + RERUN_UNIT + RERUN_DEPTH * np.maximum(1.0, np.abs(t_hip).astype(np.float64)) * slope
    return np.abs(F - 0.5), own, np.abs(F32 - 0.5), med32, med64


def judge(tag, t_hip, groups, foreign_knots, rerun=False):
    """Assert the bound over all rays of a case and record the distances."""
    from tests._record import record
    parts = [(sel, cdf_distance(t_hip[sel.to(t_hip.device)], z, sig, m, d, foreign_knots=foreign_knots and order is not None, rerun=rerun))
             for sel, z, sig, m, d, order in groups]
    ref = max(float(p[2].max()) for _, p in parts)                       # max over the rays of the case
    dist = {"fp32_definition_cdf": ref, "hip_cdf": max(float(p[0].max()) for _, p in parts), "rays": int(sum(int(s.sum()) for s, _ in parts)),
            "hip_t_rel": max(float(((t_hip[s.to(t_hip.device)].double().cpu() - p[4]).abs() / p[4].abs().clamp_min(1e-30)).max()) for s, p in parts),
            "fp32_definition_t_rel": max(float(((p[3].double() - p[4]).abs() / p[4].abs().clamp_min(1e-30)).max()) for _, p in parts)}
    slack = min(float((2.0 * ref + p[1] - p[0]).min()) for _, p in parts)
    dist["smallest_margin"] = slack
    record(f"median.kernel_vs_fp64_definition[{tag}]", dist)
    print(f"median parity [{tag}]:", json.dumps(dist))
    for _, (err, own, _, _, _) in parts:
        assert bool(np.all(err <= 2.0 * ref + own)), (tag, dist)


@pytest.mark.parametrize("tag,B,seed", TM.CASES)
def test_median_kernel_vs_definition_on_the_reference_cases(dev, tag, B, seed):
    """The three cases of the maps test (per = 3 on foreground rays, per = 1 on background-only rays, tiny directions): merged rows
    from the oracle's z_h and order, as tests/test_gpu_maps.expected_maps rebuilds them; idx_fg / total_order bit-exact."""
    from hosnerf_amd import ops
    b, last, human, want_order, want_fg = TM.case_inputs(tag, B, seed)
    got = ops.merge_composite_maps(*TM.kernel_args(b, last, human, dev), want=("depth_median",))
    assert set(got) == {"rgb", "idx_fg", "total_order", "depth_median"} and tuple(got["depth_median"].shape) == (B,)
    with torch.no_grad():
        _, idx_fg, total_order, _, z_h = oh.stage3_composite(last["tdist"], last["rgb"], last["density"], human, b["rays_o_bkg"],
                                                             b["rays_d_bkg"], b["newsmpl_to_scale_world"])
    fg = got["idx_fg"].cpu().numpy().astype(bool)
    assert np.array_equal(fg, want_fg) and np.array_equal(fg, idx_fg.numpy())
    order = got["total_order"].cpu().numpy().astype(np.int64)
    assert np.array_equal(order[fg], want_order) and np.array_equal(order[fg], total_order.numpy()) and np.all(order[~fg] == -1)
    groups = merged_rows(last["tdist"], last["density"], human["human_density"], human["pts_mask"], b["rays_d_bkg"], z_h)
    assert all(np.array_equal(g[0].numpy(), fg if g[5] is not None else ~fg) for g in groups)
    assert all(g[5] is None or torch.equal(g[5], total_order) for g in groups)
    judge(tag, got["depth_median"], groups, foreign_knots=True)


@pytest.mark.parametrize("tag,Sb,Sh,seed", RANDOM_CASES)
def test_median_kernel_vs_definition_on_random_batches(dev, tag, Sb, Sh, seed):
    """Sample counts at which the chunked scan takes another shape.  The human depths are the kernel's own z_human (the rgb-only
    entry's output, checked against the oracle elsewhere), so the stable sort on the CPU must reproduce total_order bit for bit."""
    from hosnerf_amd import ops
    B = 16
    args = TM._random_batch(B, Sb, Sh, seed, dev)
    got = ops.merge_composite_maps(*args, want=("depth_median",))
    _, _, idx_fg, order_rgb, z_h = ops.merge_composite(*args)
    td, _, bden, hum, _, mask, _, d, _ = [t.cpu() for t in args]
    groups = merged_rows(td, bden, hum[..., 3], mask, d, z_h.cpu())
    fg = got["idx_fg"].cpu().bool()
    assert torch.equal(got["idx_fg"], idx_fg) and torch.equal(got["total_order"], order_rgb)
    assert 0 < int(fg.sum()) < B and torch.equal(groups[0][0], fg) and torch.equal(groups[1][0], ~fg)
    assert torch.equal(got["total_order"].cpu()[fg].long(), groups[0][5]) and bool((got["total_order"].cpu()[~fg] == -1).all())
    judge(tag, got["depth_median"], groups, foreign_knots=False)


def test_raw2outputs_median_vs_definition(dev):
    """The `_raw2outputs` kernel on the reference's own inputs (tests/golden/human_parts.npz), with and without mask / background colour."""
    from hosnerf_amd import ops
    hp = TM.load("human_parts.npz")
    raw, z, d, mask = (TM.T(hp[k]) for k in ("r2o_raw", "r2o_z", "r2o_d", "r2o_mask"))
    for name, mk, bg in (("mask", mask, None), ("nomask_bg", None, torch.tensor([10.0, 120.0, 250.0]))):
        got = ops.raw2outputs_median(raw.to(dev), z.to(dev), d.to(dev), None if mk is None else mk.to(dev), None if bg is None else bg.to(dev))
        m = torch.ones_like(z) if mk is None else mk
        judge(f"raw2outputs_{name}", got["depth_median"], [(torch.ones(z.shape[0], dtype=torch.bool), z, raw[..., 3], m, d, None)], foreign_knots=False)


# ------------------------------------------------------------------------------------------ hand cases, exact
@pytest.mark.parametrize("S", [150, 32, 256])
def test_hand_cases_raw2outputs(dev, S):
    """Weights exact in fp32 (tests/test_median_cpu.py shows it): equality in t.  S = 150: per = 3, the crossing in the last sample of
    lane 0 and in the first sample of lane 1; S = 32 / 256: per = 1 / 4."""
    from hosnerf_amd import ops
    cases = ME.hand_cases(S)
    names = list(cases)
    B = len(names)
    z = ME.hand_depths(S).float()[None].expand(B, S).contiguous()
    mask = torch.stack([cases[n][0] for n in names]).float()
    rgbsigma = torch.zeros(B, S, 4)
    rgbsigma[..., 3] = ME.SIGMA_OPAQUE
    d = torch.tensor([[0.0, 0.0, 1.0]]).expand(B, 3).contiguous()
    got = ops.raw2outputs_median(rgbsigma.to(dev), z.to(dev), d.to(dev), mask.to(dev), None, last_dist=1.0)
    want_acc = [float(cases[n][1].sum()) for n in names]
    assert got["acc"].cpu().tolist() == want_acc                                                            # the weights arrived exact
    assert got["depth_median"].cpu().tolist() == [ME.as_f32(cases[n][2]) for n in names], names
    assert got["depth_median"].cpu().tolist()[names.index("nowhere")] == float(z[0, -1]) and want_acc[names.index("nowhere")] == 0.25


def test_hand_cases_merge(dev):
    """All-background rays (no human sample is masked in) through the merge entry, Sb = 150 (per = 3): densities 0 / 1e30."""
    from hosnerf_amd import ops
    Sb, Sh = 150, 1
    cases = ME.merge_hand_cases(Sb)
    names = list(cases)
    B = len(names)
    td = ME.hand_depths(Sb + 1).float()[None].expand(B, Sb + 1).contiguous()
    bden = torch.stack([cases[n][0] for n in names]).float()
    d = torch.tensor([[0.0, 0.0, 1.0]]).expand(B, 3).contiguous()
    args = [t.to(dev) for t in (td, torch.rand(B, Sb, 3), bden, torch.zeros(B, Sh, 4), torch.zeros(B, Sh, 3), torch.zeros(B, Sh),
                                torch.zeros(B, 3), d, torch.eye(4))]
    got = ops.merge_composite_maps(*args, want=("acc", "depth_median"))
    assert int(got["idx_fg"].sum()) == 0
    assert got["acc"].cpu().tolist() == [0.0 if n == "nowhere" else 1.0 for n in names]
    assert got["depth_median"].cpu().tolist() == [ME.as_f32(cases[n][1]) for n in names], names


# ------------------------------------------------------------------------------------------ same launch, same colours
def test_median_shares_the_launch_of_the_maps(dev):
    from hosnerf_amd import _lib, ops
    batches = [TM.kernel_args(*TM.case_inputs(*c)[:3], dev) for c in TM.CASES] + [TM._random_batch(16, Sb, Sh, seed, dev) for _, Sb, Sh, seed in RANDOM_CASES]
    batches.append(TM._random_batch(4096, 32, 128, 17, dev))
    for n, args in enumerate(batches):
        base = ops.merge_composite_maps(*args)
        full = ops.merge_composite_maps(*args, want=ALL_KEYS)
        assert set(base) == {"rgb", "idx_fg", "total_order", *TM.MAPS} and set(full) == set(base) | {"depth_median"}
        for k, v in base.items():
            assert torch.equal(full[k], v), (n, k)
        med = full["depth_median"]
        assert med.dtype == torch.float32 and tuple(med.shape) == (args[0].shape[0],) and not med.requires_grad and bool(torch.isfinite(med).all())
        # every subset of `want` (NULL for the other pointers) gives the values of the full call; all 128 on one batch, a few elsewhere
        subsets = [w for r in range(len(ALL_KEYS) + 1) for w in itertools.combinations(ALL_KEYS, r)] if n == 4 else \
            [(), ("depth_median",), ("depth", "depth_median"), ("acc_human", "rgb_bkg", "depth_median"), ("acc",)]
        for want in subsets:
            s = ops.merge_composite_maps(*args, want=want)
            assert set(s) == {"rgb", "idx_fg", "total_order", *want}
            for k, v in s.items():
                assert torch.equal(v, full[k]), (n, want, k)
    with pytest.raises(ValueError):
        ops.merge_composite_maps(*batches[0], want=("depth_median", "weights"))
    with pytest.raises(_lib.HosLibraryError):
        ops.merge_composite_maps(*TM._random_batch(4, 200, 128, 3, dev), want=("depth_median",))          # Sb + Sh > 256
    req = [t.clone().requires_grad_(True) for t in batches[0][1:4]]                                          # inputs are detached
    assert not ops.merge_composite_maps(batches[0][0], *req, *batches[0][4:], want=("depth_median",))["depth_median"].requires_grad


def test_raw2outputs_median_shares_the_launch(dev):
    from hosnerf_amd import _lib, ops
    hp = TM.load("human_parts.npz")
    cases = [(TM.T(hp["r2o_raw"], dev), TM.T(hp["r2o_z"], dev), TM.T(hp["r2o_d"], dev), TM.T(hp["r2o_mask"], dev))]
    g = torch.Generator().manual_seed(8)
    for S in (1, 65, 256):
        z = torch.sort(torch.rand(9, S, generator=g) * 3 + 0.2, -1).values
        raw = torch.rand(9, S, 4, generator=g) * torch.tensor([1.0, 1.0, 1.0, 4.0])
        cases.append(tuple(t.to(dev) for t in (raw, z, torch.randn(9, 3, generator=g), torch.rand(9, S, generator=g))))
    for raw, z, d, mask in cases:
        for mk, bg, last in ((mask, None, 1e10), (None, torch.tensor([10.0, 120.0, 250.0], device=dev), 1e10), (mask, None, 0.5)):
            rgb, acc, _, depth = ops.raw2outputs(raw, z, d, mk, bg, last)
            m = ops.raw2outputs_median(raw, z, d, mk, bg, last)
            assert set(m) == {"rgb", "acc", "depth", "depth_median"}
            assert torch.equal(m["rgb"], rgb) and torch.equal(m["acc"], acc) and torch.equal(m["depth"], depth)
            med = m["depth_median"]
            assert tuple(med.shape) == (z.shape[0],) and not med.requires_grad
            assert bool((med >= z[:, 0]).all()) and bool((med <= z[:, -1]).all())
    raw, z, d, mask = cases[0]
    assert not ops.raw2outputs_median(raw.clone().requires_grad_(True), z, d, mask)["rgb"].requires_grad
    with pytest.raises(_lib.HosLibraryError):
        ops.raw2outputs_median(torch.zeros(2, 257, 4, device=dev), torch.zeros(2, 257, device=dev), torch.ones(2, 3, device=dev))


# ------------------------------------------------------------------------------------------ module and frames
def _same_tensors(new, old, what):
    for k, v in old.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(new[k], v), (what, k)


def test_render_median_surface(dev, hos):
    B = 16
    _, gb = TM._gpu_batch("A", B, 31, dev)
    kw = dict(randomized=False, is_train=False, with_cycle=False)
    with torch.no_grad():
        base = hos.render(gb, **kw)
        maps = hos.render(gb, maps=True, **kw)
        out = hos.render(gb, maps=True, median=True, **kw)
        with pytest.raises(ValueError):
            hos.render(gb, median=True, **kw)                             # not without maps=True
        with pytest.raises(ValueError):
            hos.render(gb, randomized=False, is_train=True, with_cycle=False, maps=True, median=True)
    with pytest.raises(ValueError):
        hos.render(gb, maps=True, median=True, **kw)                      # grad enabled
    assert "depth_median" not in maps and "depth_median" not in base and set(out) == set(maps) | {"depth_median"}
    _same_tensors(out, maps, "render")
    med = out["depth_median"]
    assert tuple(med.shape) == (B,) and not med.requires_grad and bool(torch.isfinite(med).all())
    # inside [z_0, z_{S-1}] of the samples its ray composites
    z_b, z_h, fg = base["ray_history"][-1]["tdist"][..., :-1], base["z_vals_human"], out["idx_fg"].bool()
    assert 0 < int(fg.sum())
    lo = torch.where(fg, torch.minimum(z_b[:, 0], z_h.min(-1).values), z_b[:, 0])
    hi = torch.where(fg, torch.maximum(z_b[:, -1], z_h.max(-1).values), z_b[:, -1])
    assert bool((med >= lo).all()) and bool((med <= hi).all())


def test_render_bkg_only_median(dev, hos):
    _, gb = TM._gpu_batch("A", 16, 31, dev)
    bb = {"rays_o": gb["rays_o_bkg"], "rays_d": gb["rays_d_bkg"], "viewdirs": gb["viewdirs_bkg"], "radii": gb["radii"], "times": gb["time"]}
    with torch.no_grad():
        maps = hos.render_bkg_only(bb, randomized=False, is_train=False, maps=True)
        out = hos.render_bkg_only(bb, randomized=False, is_train=False, maps=True, median=True)
        _, hist = hos.model(bb, 1.0, False, False, hos.near_bkg, hos.far_bkg)
        with pytest.raises(ValueError):
            hos.render_bkg_only(bb, randomized=False, is_train=False, median=True)
    with pytest.raises(ValueError):
        hos.render_bkg_only(bb, randomized=False, is_train=False, maps=True, median=True)
    assert set(maps) == {"rgb", "alpha", "depth"} and set(out) == {"rgb", "alpha", "depth", "depth_median"}
    _same_tensors(out, maps, "render_bkg_only")
    last = {k: hist[-1][k].cpu() for k in ("tdist", "rgb", "density")}
    z = last["tdist"][..., :-1]
    judge("render_bkg_only", out["depth_median"], [(torch.ones(16, dtype=torch.bool), z, last["density"], torch.ones_like(z), bb["rays_d"].cpu(), None)],
          foreign_knots=False)


_RANK_WORKER = r"""
import os, sys
sys.path.insert(0, os.environ["HOS_ROOT"])
import torch, torch.distributed as dist
rank = int(os.environ["RANK"])
dist.init_process_group("gloo", rank=rank, world_size=int(os.environ["WORLD_SIZE"]))
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
from hosnerf_amd import eval as ev
from tests import test_gpu_eval as E
from tests.test_gpu_maps import build_frame_hos
hos = build_frame_hos(dev)
fr, _ = E.make_frame(dev, 20, 16)
maps = ev.render_frame(hos, fr, chunk_bkg=64, group=dist.group.WORLD, maps=True, median=True)
torch.cuda.synchronize()
if rank == 0:
    torch.save({k: v.cpu() for k, v in maps.items()}, os.environ["HOS_MAPS_OUT"])
dist.barrier()
dist.destroy_process_group()
print("MEDIAN_RANK_OK", rank)
"""


def test_render_frame_median(dev, tmp_path):
    from hosnerf_amd import eval as ev
    from tests.test_gpu_eval import make_frame
    hos_f = TM.build_frame_hos(dev)
    H, W = 20, 16
    fr, _ = make_frame(dev, H, W)
    maps = ev.render_frame(hos_f, fr, chunk_bkg=8192, maps=True)
    out = ev.render_frame(hos_f, fr, chunk_bkg=8192, maps=True, median=True)
    assert set(maps) == {"rgb", "alpha", "depth", "rgb_human", "alpha_human"} and set(out) == set(maps) | {"depth_median"}
    _same_tensors(out, maps, "render_frame")
    med = out["depth_median"]
    assert tuple(med.shape) == (H * W,) and bool(torch.isfinite(med).all()) and float(med.min()) > 0.0       # every pixel is in one list
    with pytest.raises(ValueError):
        ev.render_frame(hos_f, fr, median=True)
    # pixels of neither ray list: drop five rays of the background-only list
    miss_pix = torch.nonzero(fr["ray_mask_bkg"]).reshape(-1)
    assert miss_pix.numel() > 40
    fr2 = dict(fr)
    fr2["ray_mask_bkg"] = fr["ray_mask_bkg"].clone()
    fr2["ray_mask_bkg"][miss_pix[:5]] = False
    for k in ("rays_o_bkg_only", "rays_d_bkg_only", "viewdirs_bkg_only", "radii_bkg_only"):
        fr2[k] = fr[k][5:].contiguous()
    out2 = ev.render_frame(hos_f, fr2, chunk_bkg=8192, maps=True, median=True)
    assert float(out2["depth_median"][miss_pix[:5]].abs().sum()) == 0.0 and float(out2["depth"][miss_pix[:5]].abs().sum()) == 0.0
    assert torch.equal(out2["depth_median"][fr["ray_mask"]], med[fr["ray_mask"]])                           # the other list: the same launches
    # The frame's medians in the CDFs of the same rays rendered once more, whole lists in one launch each.  The median is a root of
    # the ray's CDF, not a sum: another chunking moves it by (what it moves the CDF by) / slope, so it is judged in CDF space.
    per_frame = {k: fr[k] for k in ev.FRAME_KEYS if k in fr}
    per_frame["is_train"] = False
    with ev.evaluating(hos_f):
        b = dict(per_frame)
        b.update({k: fr[k] for k in ("rays", "near", "far", "rays_o_bkg", "rays_d_bkg", "viewdirs_bkg", "radii")})
        o = hos_f.render(b, randomized=False, is_train=False, with_cycle=False)
        bb = {"rays_o": fr["rays_o_bkg_only"], "rays_d": fr["rays_d_bkg_only"], "viewdirs": fr["viewdirs_bkg_only"], "radii": fr["radii_bkg_only"],
              "times": fr["time"]}
        _, hist = hos_f.model(bb, 1.0, False, False, hos_f.near_bkg, hos_f.far_bkg)
    last = {k: o["ray_history"][-1][k].cpu() for k in ("tdist", "density")}
    fg_rows = merged_rows(last["tdist"], last["density"], o["human_rgbsigma"][..., 3].cpu(), o["pts_mask"].cpu(), fr["rays_d_bkg"].cpu(),
                          o["z_vals_human"].cpu())
    z_bg = hist[-1]["tdist"][..., :-1].cpu()
    bg_rows = [(torch.ones(z_bg.shape[0], dtype=torch.bool), z_bg, hist[-1]["density"].cpu(), torch.ones_like(z_bg), fr["rays_d_bkg_only"].cpu(), None)]

    def judge_frame(what, frame_median):
        judge(f"frame_{what}_fg", frame_median[fr["ray_mask"]], fg_rows, foreign_knots=True, rerun=True)
        judge(f"frame_{what}_bg", frame_median[fr["ray_mask_bkg"]], bg_rows, foreign_knots=True, rerun=True)

    judge_frame("one_rank", med)
    judge_frame("64_ray_chunks", ev.render_frame(hos_f, fr, chunk_bkg=64, maps=True, median=True)["depth_median"])
    # two ranks on the one GPU (gloo carries the gather; the rehearsal of tests/test_gpu_maps.py): one bounded child per rank; the maps
    # of before against the one-rank frame to the bounds of test_gpu_maps.py, the median as above
    env = dict(os.environ)
    env.update(HOS_ROOT=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29563", WORLD_SIZE="2",
               HOS_MAPS_OUT=str(tmp_path / "maps.pt"))
    procs = [subprocess.Popen(["timeout", "-k", "10", "600", sys.executable, "-c", _RANK_WORKER], env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT) for r in range(2)]
    outs = [p.communicate(timeout=700) for p in procs]
    for r, (p, (so, se)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"MEDIAN_RANK_OK {r}" in so, (r, so[-2000:], se[-4000:])
    two = {k: v.to(dev) for k, v in torch.load(env["HOS_MAPS_OUT"]).items()}
    assert set(two) == set(out)
    for k in maps:
        scale = maps[k].abs().clamp_min(1.0) if k == "depth" else torch.ones((), device=dev)
        assert float(((two[k] - maps[k]).abs() / scale).max()) <= (1.1e-5 if k == "depth" else 1e-6), k
    judge_frame("two_ranks", two["depth_median"])


def test_render_human_frame_median(dev):
    from hosnerf_amd import eval as ev, formats, tpose
    from tests.test_gpu_tpose import build_hos
    hos_t = build_hos(dev)
    joints = synth.tpose_joints()
    bbox = formats.skeleton_bbox(joints, float(hos_t.cfg.bbox_offset))
    turn = tpose.TposeTurn(joints, bbox, 32, dev, img_size=24, focal=1250.0 * 24 / 512)
    fr = tpose.tpose_frame(None, None, 6, 8, bgcolor=(255.0, 255.0, 255.0), turn=turn, iter_val=3e5, time=0.2)
    maps, u8 = ev.render_human_frame(hos_t, fr, maps=True, want_u8=True)
    out, u8m = ev.render_human_frame(hos_t, fr, maps=True, want_u8=True, median=True)
    assert set(maps) == {"rgb", "alpha", "depth"} and set(out) == {"rgb", "alpha", "depth", "depth_median"} and torch.equal(u8, u8m)
    _same_tensors(out, maps, "render_human_frame")
    with pytest.raises(ValueError):
        ev.render_human_frame(hos_t, fr, median=True)
    mask, n = fr["ray_mask"], fr["count"]
    med = out["depth_median"]
    assert 0 < n < 24 * 24 and tuple(med.shape) == (24 * 24,) and float(med[~mask].abs().sum()) == 0.0     # painted over 0
    with torch.no_grad(), ev.evaluating(hos_t):
        per = {k: fr[k] for k in ev.FRAME_KEYS if k in fr}
        net = hos_t.human(rays=fr["rays"], near=fr["near"], far=fr["far"], with_cycle=False, **per)
    net = {k: net[k].cpu() for k in ("human_density", "z_vals", "rays_d", "pts_mask")}
    judge("tpose_frame", med[mask], [(torch.ones(n, dtype=torch.bool), net["z_vals"], net["human_density"], net["pts_mask"], net["rays_d"], None)],
          foreign_knots=False)
    # the frame without rays still launches only the paint
    empty = tpose.TposeTurn(joints, {"min_xyz": np.array([50.0, 50.0, 50.0]), "max_xyz": np.array([51.0, 51.0, 51.0])}, 8, dev, img_size=16,
                            focal=1250.0 * 16 / 512)
    fr0 = tpose.tpose_frame(None, None, 0, 8, bgcolor=(0.0, 128.0, 255.0), turn=empty, time=0.2)
    assert fr0["count"] == 0
    m0 = ev.render_human_frame(None, fr0, maps=True, median=True)         # no network is touched
    assert set(m0) == {"rgb", "alpha", "depth", "depth_median"} and float(m0["depth_median"].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------ the launcher
def test_launcher_writes_the_median_next_to_the_frames(tmp_path):
    """`run.render_maps` alone writes no median file; with `run.render_median` every frame of run_eval / run_render / run_tpose gets
    <name>_depth_median.npy (float32 [H,W]) and .png next to it."""
    from PIL import Image
    from hosnerf_amd import tpose
    from hosnerf_amd.freeview import write_scene_pixels
    scene = str(tmp_path / "scene")
    H = W = 64
    write_scene_pixels(scene, synth.write_scene_dir(scene, 6, H, W, seed=9))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("patch:\n  N_patches: 2\n  size: 16\nfreeview:\n  frame_idx: 3\n")
    logs = str(tmp_path / "logs")
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "--ginc", os.path.join(ROOT, "configs", "hosnerf_backpack.gin"),
           "--ginb", "run.max_steps=1", "--ginb", f'run.datadir="{scene}"', "--ginb", 'run.human_path=""', "--ginb", 'run.bkgd_path=""',
           "--ginb", "run.run_eval=True", "--ginb", "run.run_render=True", "--ginb", "run.run_tpose=True", "--ginb", "run.render_maps=True",
           "--logbase", logs, "--scene_name", "synthetic", "--scene_dir", scene, "--cfg", str(cfg), "--eval_skip", "100", "--render_frames", "40",
           "--render_limit", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    logdir = [os.path.join(logs, d) for d in os.listdir(logs)][0]
    with open(os.path.join(scene, "transitions_times.json")) as f:
        times = tpose.tpose_times([v["time"] for v in json.load(f).values()])
    frames = [(os.path.join(logdir, "test_vis"), "frame_000000", (H, W)),
              (os.path.join(logdir, "freeview_vis_newtrans", "view_00003"), "image-00000", (H, W))]
    frames += [(os.path.join(logdir, "tpose_vis", "time_{:06}".format(t)), "image-00000", (512, 512)) for t in times]
    assert len(times) == 2
    for folder, name, _ in frames:
        assert any(f.startswith(name) for f in os.listdir(folder)), folder
        assert not [f for f in os.listdir(folder) if "depth_median" in f], folder                          # render_maps alone: none
    r2 = subprocess.run(cmd + ["--ginb", "run.run_train=False", "--ginb", "run.render_median=True"], capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r2.returncode == 0, (r2.stdout[-2000:], r2.stderr[-3000:])
    for folder, name, shape in frames:
        med = np.load(os.path.join(folder, name + "_depth_median.npy"))
        assert med.shape == shape and med.dtype == np.float32 and np.isfinite(med).all(), (folder, med.shape, med.dtype)
        assert np.asarray(Image.open(os.path.join(folder, name + "_depth_median.png"))).shape == shape
    depth = np.load(os.path.join(frames[0][0], "frame_000000_depth.npy"))
    assert depth.shape == (H, W)                                                                           # the other maps are still written
