"""Opacity, expected and median distance of a stage-1 ray from one launch (`hos_volrender_maps_fwd`) against the reference's functions
(tests/_bkgd_maps_expect.py, pinned to the reference by tests/golden/bkgd_maps.npz and tests/test_bkgd_maps_cpu.py) on identical
inputs, the same-launch guarantees, the module surface (`MipNeRF360.forward(maps=True)`), whole frames
(`eval.render_bkgd_frame(maps=True)`) and the stage-1 launcher's `run.render_maps`.

Bounds.  `acc` and `depth` (relative to sum w |t_mid|): |hip - fp64| <= 2 * max_rays |fp32 expectation - fp64| + 2^-23, the rule of
tests/test_gpu_maps.py.  The median is judged in CDF space, where it is well conditioned: with F the fp64 CDF of the ray (knots tdist,
values integrate_weights(w), linear in between; the mass of an interval is the difference of its knots, which is w_k except under the
forced last knot) evaluated at the kernel's distance,
    |F - 0.5| <= 2 * max_rays |F(fp32 expectation) - 0.5| + S * 2^-23 + 2 * ulp32(t) * slope,
S * 2^-23 being the worst rounding of an S-term sum of non-negative terms bounded by 1 and the last term one output ulp mapped into
CDF space; in a zero-width interval every value between its knots counts.  No ray is excluded."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _bkgd_maps_expect as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -23
MAPS = ("acc", "depth", "depth_median")
G = np.load(os.path.join(ROOT, "tests", "golden", "stage1_rays.npz"))
N, H, W = G["images_u8"].shape[:3]


def tie_case():
    """A CDF exactly 0.5 at a knot followed by a zero-weight bin, from weights exact in fp32: knots 0, 1/4, 1/2, 1/2, 1: the reference's
    mask `0.5 >= cw` reaches knot 3, so the median is t_3 (offset 0 in bin 3)."""
    S = 32
    w = torch.zeros(2, S)
    w[0, :4] = torch.tensor([0.25, 0.25, 0.0, 0.5])
    w[1, 20:25] = torch.tensor([0.125, 0.375, 0.0, 0.0, 0.5])                # ray 1: two zero-weight bins after the knot at 1/2
    g = torch.Generator().manual_seed(4)
    tdist = torch.sort(torch.rand(2, S + 1, generator=g) * 5 + 0.3, -1).values
    return torch.rand(2, S, 3, generator=g), w, tdist


def case_tensors(tag):
    if tag == "tie":
        return tie_case()
    c = X.load_case(tag)
    return c["rgb"], c["w32"], c["tdist"]


@pytest.fixture(scope="module")
def expectations():
    """tag -> (inputs on the CPU, fp32 expectation, fp64 expectation), computed once and left unchanged."""
    out = {}
    for tag in [c[0] for c in X.CASES] + ["tie"]:
        rgb, w, tdist = case_tensors(tag)
        out[tag] = ((rgb, w, tdist), X.expected_maps(rgb, w, tdist, X.BG, torch.float32), X.expected_maps(rgb, w, tdist, X.BG, torch.float64))
    return out


def median_in_cdf_space(t_hip, e32, e64, tdist):
    """(per-ray |F - 0.5| of the kernel, per-ray bound, worst |F - 0.5| of the fp32 expectation)."""
    S = tdist.shape[1] - 1
    t64, cw64 = tdist.double().numpy(), e64["cw"].numpy()
    t_hip = t_hip.cpu().numpy().astype(np.float32)
    F, slope = X.cdf_at(t_hip, t64, cw64)
    F32, _ = X.cdf_at(e32["depth_median"].numpy(), t64, cw64)
    ref = float(np.abs(F32 - 0.5).max())
    bound = 2.0 * ref + S * ULP + 2.0 * np.spacing(np.abs(t_hip)).astype(np.float64) * slope
    return np.abs(F - 0.5), bound, ref


@pytest.mark.parametrize("tag", [c[0] for c in X.CASES] + ["tie"])
def test_maps_kernel_vs_reference(tag, expectations):
    from hosnerf_amd import ops
    from tests._record import record
    (rgb, w, tdist), e32, e64 = expectations[tag]
    dev = torch.device("cuda")
    args = [t.to(dev) for t in (rgb, w, tdist)]
    got = ops.volrender_maps(*args, X.BG)
    assert set(got) == {"rgb", *MAPS} and all(tuple(got[k].shape) == (w.shape[0],) and not got[k].requires_grad for k in MAPS)
    assert torch.equal(got["rgb"], ops.volumetric_rendering(args[0], args[1], X.BG))                  # the same loop, the same wave_sum order
    dist = {}
    for k in ("acc", "depth"):
        scale = e64["depth_scale"].clamp_min(1e-30) if k == "depth" else torch.ones((), dtype=torch.float64)
        e = lambda x: float(((x.double().cpu() - e64[k]).abs() / scale).max())
        dist[k] = {"hip": e(got[k]), "fp32_expectation": e(e32[k])}
    err, bound, ref = median_in_cdf_space(got["depth_median"], e32, e64, tdist)
    worst = int(np.argmax(err - bound))
    dist["depth_median_cdf"] = {"hip": float(err.max()), "fp32_expectation": ref, "bound_at_worst_ray": float(bound[worst]),
                                "hip_at_worst_ray": float(err[worst])}
    dist["depth_median_t"] = {"hip": float(((got["depth_median"].double().cpu() - e64["depth_median"]).abs() / e64["depth_median"].abs()).max()),
                              "fp32_expectation": float(((e32["depth_median"].double() - e64["depth_median"]).abs() / e64["depth_median"].abs()).max())}
    record(f"bkgd_maps.kernel_vs_fp64_expectation[{tag}]", dist)
    print(f"bkgd maps parity [{tag}]:", json.dumps(dist))
    for k in ("acc", "depth"):
        assert dist[k]["hip"] <= 2.0 * dist[k]["fp32_expectation"] + ULP, (tag, k, dist[k])
    assert bool(np.all(err <= bound)), (tag, dist["depth_median_cdf"])
    if tag == "tie":                                                                                  # exact arithmetic: offset 0 in bins 3 / 24
        assert got["depth_median"].cpu().tolist() == [float(tdist[0, 3]), float(tdist[1, 24])]
        assert torch.equal(got["depth_median"].cpu(), e32["depth_median"])


def test_null_map_pointers_and_arguments(expectations):
    """Every subset of `want` gives the values of the full call and the same rgb; unknown names and S > 256 are refused."""
    from hosnerf_amd import _lib, ops
    dev = torch.device("cuda")
    for tag in ("s32", "s200"):
        args = [t.to(dev) for t in expectations[tag][0]]
        full = ops.volrender_maps(*args, X.BG)
        for n in range(len(MAPS) + 1):
            for want in itertools.combinations(MAPS, n):
                s = ops.volrender_maps(*args, X.BG, want=want)
                assert set(s) == {"rgb", *want}
                for k, v in s.items():
                    assert torch.equal(v, full[k]), (tag, want, k)
    with pytest.raises(ValueError):
        ops.volrender_maps(*args, X.BG, want=("weights",))
    big = [torch.zeros(2, 257, 3, device=dev), torch.zeros(2, 257, device=dev), torch.zeros(2, 258, device=dev)]
    with pytest.raises(_lib.HosLibraryError):
        ops.volrender_maps(*big, X.BG)
    req = [t.clone().requires_grad_(True) for t in args[:2]]                                           # inputs are detached
    assert not ops.volrender_maps(req[0], req[1], args[2], X.BG)["rgb"].requires_grad


# ------------------------------------------------------------------------------------------ module and frame
def fixture_scene():
    return {"extrinsics": G["extrinsics"], "intrinsics": G["intrinsics"], "times": G["times"], "render_poses": G["render_poses"],
            "render_times": G["render_times"], "i_split": (G["i_train"], G["i_train"][:2], G["i_test"], np.arange(N)),
            "bkgrays_sizes": np.sum(G["masks"] < 1, axis=(1, 2))}


@pytest.fixture(scope="module")
def bank():
    from hosnerf_amd.raybank import RayBank
    return RayBank(fixture_scene(), G["images_u8"], G["masks"], device="cuda", split="train")


def _model(tmp_path_factory, **kw):
    from hosnerf_amd import synth
    from hosnerf_amd.mipnerf360 import MipNeRF360
    d = str(tmp_path_factory.mktemp("base"))
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    m = MipNeRF360(d, opaque_background=True, **kw)
    m.load_state_dict(synth.background_state_dict(777, 2), strict=False)
    return m.to("cuda")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return _model(tmp_path_factory)


def chunked(model, bank, i, chunk):
    """Direct `model(..., maps=True)` calls over the frame's chunks: (renderings[-1] per key, tdist, weights), concatenated."""
    n = H * W
    rend, tdist, weights = [], [], []
    with torch.no_grad():
        for s in range(0, n, chunk):
            r, hist = model(bank.frame(i, s, min(chunk, n - s)), 0.5, False, False, 0.1, 1e6, maps=True)
            assert all(set(lvl) == {"rgb"} for lvl in r[:-1]) and set(r[-1]) == {"rgb", *MAPS}
            rend.append(r[-1])
            tdist.append(hist[-1]["tdist"])
            weights.append(hist[-1]["weights"])
    return {k: torch.cat([p[k] for p in rend], 0) for k in rend[0]}, torch.cat(tdist, 0), torch.cat(weights, 0)


def test_render_bkgd_frame_maps(bank, model):
    from hosnerf_amd import eval as ev
    from tests._record import record
    i, n = int(G["frame"]), H * W
    plain = ev.render_bkgd_frame(model, bank, i, 64, 0.5, 0.1, 1e6)
    a = ev.render_bkgd_frame(model, bank, i, 64, 0.5, 0.1, 1e6, maps=True)
    assert set(a) == {"rgb", "alpha", "depth", "depth_median"} and torch.equal(a["rgb"], plain)
    for k, v in a.items():
        assert tuple(v.shape) == ((n, 3) if k == "rgb" else (n,)) and bool(torch.isfinite(v).all()) and not v.requires_grad, k
    direct, td_a, w_a = chunked(model, bank, i, 64)
    for key, k in ev.BKGD_FRAME_MAPS.items():
        assert torch.equal(a[key], direct[k]), key
    assert float(a["alpha"].min()) >= 0.0 and float(a["alpha"].max()) <= 1.0 + 1e-5
    assert bool((a["depth_median"] >= td_a[:, 0]).all()) and bool((a["depth_median"] <= td_a[:, -1]).all())
    assert model.training                                                                               # left as it was
    # ---- another chunking: alpha and depth move by less than 1e-6 relative; the median is compared in CDF space (with
    # opaque_background and far = 1e6 a crossing in the last interval moves by hundreds in t for an ulp of CDF change, the fp32
    # reference's too): each run's distance in the OTHER run's fp64 CDF; in t only for crossings before the last interval
    b = ev.render_bkgd_frame(model, bank, i, 97, 0.5, 0.1, 1e6, maps=True)
    direct_b, td_b, w_b = chunked(model, bank, i, 97)
    assert torch.equal(b["depth_median"], direct_b["depth_median"])
    fig = {k: float(((a[k] - b[k]).abs() / a[k].abs().clamp_min(1e-30)).max()) for k in ("alpha", "depth")}
    fig["rgb"] = float((a["rgb"] - b["rgb"]).abs().max())
    cw_a, cw_b = X.integrate_weights(w_a.double().cpu()).numpy(), X.integrate_weights(w_b.double().cpu()).numpy()
    ta, tb = a["depth_median"].cpu().numpy(), b["depth_median"].cpu().numpy()
    F_a = X.cdf_at(ta, td_b.double().cpu().numpy(), cw_b, clamp=True)[0]
    F_b = X.cdf_at(tb, td_a.double().cpu().numpy(), cw_a, clamp=True)[0]
    fig["depth_median_cdf"] = float(np.abs(F_a - F_b).max())
    S = w_a.shape[1]
    bins = [X.expected_maps(torch.zeros(n, S, 3), w.cpu(), td.cpu(), 1.0, torch.float64)["bin"].numpy() for w, td in ((w_a, td_a), (w_b, td_b))]
    inner = (bins[0] < S - 1) & (bins[1] < S - 1)
    fig["rays_crossing_before_the_last_interval"] = int(inner.sum())
    fig["depth_median_t_inner"] = float((np.abs(ta.astype(np.float64) - tb)[inner] / np.abs(ta[inner])).max()) if inner.any() else 0.0
    record("bkgd_maps.frame_rechunk_64_97", fig)
    print("bkgd maps re-chunking 64 -> 97:", json.dumps(fig))
    assert fig["alpha"] < 1e-6 and fig["depth"] < 1e-6 and fig["rgb"] < 1e-6
    assert fig["depth_median_cdf"] <= 1e-6
    assert fig["depth_median_t_inner"] <= 1e-6
    p = ev.render_bkgd_frame(model, bank, ("pose", int(G["pose"])), 240, 0.5, 0.1, 1e6, maps=True)
    assert set(p) == set(a) and tuple(p["depth_median"].shape) == (n,) and bool(torch.isfinite(p["depth"]).all())


def test_forward_maps_surface(bank, model, tmp_path_factory, monkeypatch):
    from hosnerf_amd import ops
    batch = bank.frame(int(G["frame"]), 0, 37)
    with torch.no_grad():
        base, _ = model(batch, 0.5, False, False, 0.1, 1e6)
        out, hist = model(batch, 0.5, False, False, 0.1, 1e6, maps=True)
    assert all(set(lvl) == {"rgb"} for lvl in base) and set(out[-1]) == {"rgb", *MAPS}
    assert all(torch.equal(x["rgb"], y["rgb"]) for x, y in zip(base, out))
    one = ops.volrender_maps(hist[-1]["rgb"], hist[-1]["weights"], hist[-1]["tdist"], model.bg_intensity_range[0])
    assert all(torch.equal(one[k], out[-1][k]) for k in one)
    with pytest.raises(ValueError, match="evaluation output"):
        model(batch, 0.5, False, False, 0.1, 1e6, maps=True)                                            # grad enabled
    with torch.no_grad(), pytest.raises(ValueError, match="evaluation output"):
        model(batch, 0.5, False, True, 0.1, 1e6, maps=True)
    stage3 = _model(tmp_path_factory, render_levels=False)
    with torch.no_grad(), pytest.raises(ValueError, match="render_bkg_only"):
        stage3(batch, 1.0, False, False, 0.1, 1e6, maps=True)
    # the range guard's re-run (ops.guarded_forward: the flag fired -> the module is pinned to exact fp32 and run again) carries the
    # flag through; the guard's verdict is supplied here, no activation is driven out of range
    assert ops.RANGE_GUARD and model.gemm_mode is None
    monkeypatch.setattr(ops, "range_events", lambda device, reset=True: 1)
    try:
        with torch.no_grad(), pytest.warns(UserWarning, match="exact fp32"):
            rerun, _ = model(batch, 0.5, False, False, 0.1, 1e6, maps=True)
        assert model.gemm_mode == ops.GEMM_FP32
        with torch.no_grad():
            pinned, _ = model(batch, 0.5, False, False, 0.1, 1e6, maps=True)
    finally:
        model.gemm_mode = None
        monkeypatch.undo()
    assert set(rerun[-1]) == {"rgb", *MAPS} and all(torch.equal(rerun[-1][k], pinned[-1][k]) for k in pinned[-1])
    assert model.training


# ------------------------------------------------------------------------------------------ launcher
SH = SW = 24
N_FRAMES = 6
KINDS = ("depth.npy", "depth_median.npy", "depth.png", "depth_median.png", "alpha.png")


def _cmd(scene, logs, extra):
    return [sys.executable, os.path.join(ROOT, "run.py"), "--ginc", os.path.join(ROOT, "configs", "state_mipnerf360_backpack.gin"),
            "--ginb", "run.max_steps=3", "--ginb", "run.log_every_n_steps=1", "--ginb", f'run.datadir="{scene}"',
            "--ginb", "LitData.batch_size=512", "--ginb", "LitData.chunk=200", "--ginb", "run.run_eval=True", "--ginb", "run.run_render=True",
            "--logbase", logs, "--scene_name", "synthetic", "--scene_dir", scene, "--render_limit", "2"] + extra


def test_launcher_writes_stage1_maps(tmp_path):
    """`run.render_maps=True` on the stage-1 launcher: the five map files next to every image{NNN}.jpg of render_model/ and
    render_video/, the .npy files those of `render_bkgd_frame(maps=True)` from last.ckpt, results.json still PSNR only, and the jpgs
    byte for byte those of a run without the binding from the same checkpoint."""
    from PIL import Image
    import run as launcher
    from hosnerf_amd import eval as ev, select_option, synth
    from hosnerf_amd.freeview import write_scene_pixels
    scene, logs = str(tmp_path / "scene"), str(tmp_path / "logs")
    write_scene_pixels(scene, synth.write_scene_dir(scene, N_FRAMES, SH, SW, seed=9))
    r = subprocess.run(_cmd(scene, logs, ["--ginb", "run.render_maps=True"]), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    logdir = [os.path.join(logs, d) for d in os.listdir(logs)][0]
    frames = [("render_model", j) for j in range(N_FRAMES)] + [("render_video", k) for k in range(2)]
    for folder in ("render_model", "render_video"):
        want = sorted(f"image{k:03d}{tail}" for f, k in frames if f == folder for tail in (".jpg",) + tuple("_" + x for x in KINDS))
        assert sorted(os.listdir(os.path.join(logdir, folder))) == want
    assert set(json.load(open(os.path.join(logdir, "results.json")))) == {"PSNR"}
    dev = torch.device("cuda")
    lit = select_option.select_model("state_mipnerf360", scene, max_steps=3, grad_max_norm=0.001, near=0.1, far=1e6)
    select_option.load_checkpoint(lit, os.path.join(logdir, "last.ckpt"), strict=True)
    lit = lit.to(dev)
    bank = launcher.load_ray_bank(scene, dev, 0.1, 1e6)
    for folder, k in frames:
        m = ev.render_bkgd_frame(lit.model, bank, k if folder == "render_model" else ("pose", k), 200, 3 / 3, 0.1, 1e6, maps=True)
        for key in ("depth", "depth_median"):
            got = np.load(os.path.join(logdir, folder, f"image{k:03d}_{key}.npy"))
            want = m[key].view(SH, SW).cpu().numpy()
            assert got.dtype == np.float32 and got.shape == (SH, SW)
            print(folder, k, key, "max |file - recomputed|:", float(np.abs(got.astype(np.float64) - want).max()))
            assert np.array_equal(got, want), (folder, k, key)
        for key in ("depth.png", "depth_median.png", "alpha.png"):
            img = Image.open(os.path.join(logdir, folder, f"image{k:03d}_{key}"))
            assert img.size == (SW, SH) and img.mode == "L"
    logs2 = str(tmp_path / "logs2")
    r2 = subprocess.run(_cmd(scene, logs2, ["--ginb", "run.run_train=False", "--ckpt_path", os.path.join(logdir, "last.ckpt")]),
                        capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r2.returncode == 0, (r2.stdout[-3000:], r2.stderr[-4000:])
    logdir2 = [os.path.join(logs2, d) for d in os.listdir(logs2)][0]
    for folder, k in frames:
        assert sorted(os.listdir(os.path.join(logdir2, folder))) == sorted(f"image{j:03d}.jpg" for f, j in frames if f == folder)
        name = os.path.join(folder, f"image{k:03d}.jpg")
        assert open(os.path.join(logdir, name), "rb").read() == open(os.path.join(logdir2, name), "rb").read(), name
    assert json.load(open(os.path.join(logdir2, "results.json"))) == json.load(open(os.path.join(logdir, "results.json")))
