"""Stage-1 maps without a GPU: the restated expectation (tests/_bkgd_maps_expect.py) against the reference's own outputs
(tests/golden/bkgd_maps.npz, tests/golden/make_golden_bkgd_maps.py), the file writer `freeview.save_frame_maps`, the C ABI's
declaration of `hos_volrender_maps_fwd`, and the Python / launcher surface of `run.render_maps` for stage 1."""
import inspect
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import _bkgd_maps_expect as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ulps32(a, b):
    """Distance of two fp32 tensors in units of the larger one's spacing."""
    a, b = a.numpy().astype(np.float32), b.numpy().astype(np.float32)
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)))


@pytest.mark.parametrize("tag,B,S,opaque", X.CASES)
def test_expectation_is_the_reference(tag, B, S, opaque):
    """fp32: the median's interval bit-exact, values within 1 ulp; fp64: 1e-12.  This pins the oracle of the GPU tests."""
    c = X.load_case(tag)
    assert tuple(c["tdist"].shape) == (B, S + 1) and tuple(c["rgb"].shape) == (B, S, 3) and bool(c["opaque"]) is opaque
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        w = X.weights_from_density(c["density"], c["tdist"], c["dirs"], opaque, dt)
        e = X.expected_maps(c["rgb"], w, c["tdist"], X.BG, dt)
        assert torch.equal(e["bin"], c["bin" + name]), (tag, name)
        assert bool(((e["cw"][:, 1:] - e["cw"][:, :-1]) >= 0).all())                       # a sequential cumsum of non-negative terms
        pairs = ((w, c["w" + name]), (e["rgb"], c["rgb" + name]), (e["depth_median"], c["med" + name]), (e["acc"], c["w" + name].sum(-1)))
        if name == "32":
            worst = max(_ulps32(a, b) for a, b in pairs)
            print(f"{tag} fp32: worst distance {worst} ulp")
            assert worst <= 1.0, (tag, worst)
        else:
            worst = max(float(((a - b).abs() / b.abs().clamp_min(1.0)).max()) for a, b in pairs)
            print(f"{tag} fp64: worst distance {worst:.3e}")
            assert worst <= 1e-12, (tag, worst)
        k = e["bin"][:, None]
        lo, hi = torch.gather(e["cw"], 1, k)[:, 0], torch.gather(e["cw"], 1, k + 1)[:, 0]
        assert bool((lo <= 0.5).all()) and bool((hi > 0.5).all())                          # the interval the kernel's ballot defines


def test_hand_made_rays_are_what_they_claim():
    clear, opq = X.load_case("hand_clear"), X.load_case("hand_opaque")
    w = clear["w64"]
    assert float(w[0, 10]) == 1.0 and float(w[0].sum()) == 1.0                             # all weight in one bin
    assert abs(float(w[1].sum()) - 0.3) < 1e-6 and int(clear["bin64"][1]) == 31            # acc = 0.3: the forced last knot
    for c in (clear, opq):
        assert float(c["tdist"][2, 15]) == float(c["tdist"][2, 16]) and int(c["bin64"][2]) == 16 and float(c["w64"][2, 15]) == 0.0
    assert float(opq["w64"][0, 31]) == 1.0 and int(opq["bin64"][0]) == 31                  # all weight in the opaque last bin
    assert float(opq["tdist"][1, 31]) == float(opq["tdist"][1, 32]) and int(opq["bin64"][1]) == 31 and float(opq["w64"][1, 31]) > 0.6
    assert float(opq["med64"][1]) == float(opq["tdist"][1, 31])


def test_cdf_at():
    """The CDF-space measure of the GPU tests on a ray worked by hand: w = [1/4, 1/4, 0, 1/2] over t = [0, 1, 2, 2, 4]."""
    t = np.array([[0.0, 1.0, 2.0, 2.0, 4.0]])
    e = X.expected_maps(torch.zeros(1, 4, 3), torch.tensor([[0.25, 0.25, 0.0, 0.5]]), torch.from_numpy(t), 1.0, torch.float64)
    assert e["cw"].tolist() == [[0.0, 0.25, 0.5, 0.5, 1.0]] and int(e["bin"]) == 3 and float(e["depth_median"]) == 2.0
    assert float(e["acc"]) == 1.0 and float(e["depth"]) == 0.25 * 0.5 + 0.25 * 1.5 + 0.5 * 3.0
    cw = e["cw"].numpy()
    for q, F, s in ((0.5, 0.125, 0.25), (2.0, 0.5, 0.0), (3.0, 0.75, 0.25), (4.0, 1.0, 0.0), (0.0, 0.0, 0.0)):
        got = X.cdf_at(np.array([q]), t, cw)
        assert (float(got[0][0]), float(got[1][0])) == (F, s), (q, got)
    with pytest.raises(AssertionError):
        X.cdf_at(np.array([4.5]), t, cw)


def test_save_bkgd_maps(tmp_path):
    from PIL import Image
    from hosnerf_amd.freeview import depth_preview, save_frame_maps
    H, W = 5, 7
    rs = np.random.RandomState(3)
    maps = {"rgb": rs.uniform(size=(H * W, 3)).astype(np.float32), "alpha": rs.uniform(size=H * W).astype(np.float32),
            "depth": (rs.uniform(size=H * W) * 1e6).astype(np.float32), "depth_median": (rs.uniform(size=H * W) * 9).astype(np.float32)}
    for given in (maps, {k: torch.from_numpy(v) for k, v in maps.items()}):
        out = str(tmp_path / ("t" if isinstance(given["alpha"], torch.Tensor) else "n"))
        paths = save_frame_maps(out, "image003", given, H, W)
        assert set(paths) == {"depth.npy", "depth_median.npy", "depth.png", "depth_median.png", "alpha.png"}
        assert sorted(os.listdir(out)) == sorted(f"image003_{k}" for k in paths) and all(os.path.dirname(p) == out for p in paths.values())
        for k in ("depth", "depth_median"):
            back = np.load(paths[k + ".npy"])
            assert back.dtype == np.float32 and back.shape == (H, W) and np.array_equal(back, maps[k].reshape(H, W))
            png = Image.open(paths[k + ".png"])
            assert png.mode == "L" and png.size == (W, H) and np.array_equal(np.asarray(png), depth_preview(maps[k].reshape(H, W)))
        alpha = Image.open(paths["alpha.png"])
        assert alpha.mode == "L" and alpha.size == (W, H)
        assert np.array_equal(np.asarray(alpha), (maps["alpha"].reshape(H, W) * 255.0 + 0.5).astype(np.uint8))


def test_header_declares_the_entry_point():
    import re
    from hosnerf_amd import _lib
    header = open(_lib.HEADER).read()
    m = re.search(r"int hos_volrender_maps_fwd\(([^)]*)\);", header)
    assert m, "include/hosrender.h does not declare hos_volrender_maps_fwd"
    names = [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert names == ["rgbs", "weights", "tdist", "B", "S", "bg", "rgb", "acc", "depth", "depth_median", "stream"]
    restype, argtypes = _lib.parse_header(_lib.HEADER)["hos_volrender_maps_fwd"]
    P, I, F = _lib._P, _lib._I, _lib._F
    assert restype is I and len(argtypes) == 11 and argtypes == [P, P, P, I, I, F, P, P, P, P, P]
    assert _lib.abi_version(_lib.HEADER) == 101                                            # an added entry point leaves the revision alone
    lib = _lib.load()
    # argument validation precedes any launch: no inputs / no rgb buffer / more than 256 samples -> HOS_E_ARG
    import ctypes
    buf = (ctypes.c_float * 4)()
    a = ctypes.addressof(buf)
    assert lib.hos_volrender_maps_fwd(0, 0, 0, 4, 32, 1.0, 0, 0, 0, 0, 0) == -1
    assert lib.hos_volrender_maps_fwd(a, a, a, 4, 32, 1.0, 0, a, a, a, 0) == -1
    assert lib.hos_volrender_maps_fwd(a, a, a, 4, 257, 1.0, a, a, a, a, 0) == -1


def test_python_surface_without_gpu():
    import json
    from hosnerf_amd import eval as ev, ops
    from hosnerf_amd.mipnerf360 import MipNeRF360
    assert inspect.signature(ev.render_bkgd_frame).parameters["maps"].default is False
    assert inspect.signature(MipNeRF360.forward).parameters["maps"].default is False
    assert inspect.signature(ops.volrender_maps).parameters["want"].default == ("acc", "depth", "depth_median")
    with pytest.raises(ValueError):
        ops.volrender_maps(torch.zeros(2, 4, 3), torch.zeros(2, 4), torch.zeros(2, 5), 1.0, want=("weights",))
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    # refused before any kernel is reached: autograd on, a training call, a stage-3 background branch
    m = MipNeRF360(d, opaque_background=True)
    with pytest.raises(ValueError, match="evaluation output"):
        m({}, 0.5, False, False, 0.1, 1e6, maps=True)
    with torch.no_grad(), pytest.raises(ValueError, match="evaluation output"):
        m({}, 0.5, False, True, 0.1, 1e6, maps=True)
    with torch.no_grad(), pytest.raises(ValueError, match="render_bkg_only"):
        MipNeRF360(d, opaque_background=True, render_levels=False)({}, 0.5, False, False, 0.1, 1e6, maps=True)


def test_launcher_takes_render_maps_for_stage1():
    import run as launcher
    gin = os.path.join(ROOT, "configs", "state_mipnerf360_backpack.gin")
    plan = launcher.main(["--ginc", gin, "--scene_name", "Backpack", "--logbase", tempfile.mkdtemp(), "--cpu", "--ginb", "run.max_steps=3",
                          "--ginb", "run.render_maps=True"])
    assert plan["mode"] == "cpu-plumbing" and plan["model_name"] == "state_mipnerf360" and plan["gin"]["run.render_maps"] is True
    assert inspect.signature(launcher.evaluate_and_render_bkgd).parameters["render_maps"].default is False
