"""CPU side of the median depth of stage-3 and human-only frames: the definition on the hand cases (so that the GPU test's expectation
cannot be wrong in the kernel's direction), the two C entries in the header, the library and the ctypes mirror, the file pair
`freeview.save_frame_maps` writes, the launcher's `run.render_median` binding and the Python surface's refusals."""
import inspect
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle.human as oh
from tests import _median_expect as ME


@pytest.mark.parametrize("S", [150, 32, 256])
def test_definition_on_the_hand_cases(S):
    """The definition in fp64 gives the stated medians exactly, in fp32 the same numbers rounded once; the masks of the cases give
    the stated weights EXACTLY through the fp32 `_raw2outputs` (so the kernels see exact weights), and in fp64 up to its 1e-10 terms."""
    z = ME.hand_depths(S)
    d = torch.tensor([[0.0, 0.0, 1.0]])
    for name, (mask, w, want) in ME.hand_cases(S).items():
        got64, t, cw = ME.median_definition(w[None], z[None])
        assert float(got64[0]) == want, (name, float(got64[0]), want)
        assert t.shape == (1, S + 1) and float(t[0, -1]) == float(t[0, -2]) == float(z[-1])          # S + 1 knots, zero-width last interval
        assert float(cw[0, 0]) == 0.0 and float(cw[0, -1]) == 1.0
        got32, _, _ = ME.median_definition(w[None].float(), z[None].float())
        assert float(got32[0]) == ME.as_f32(want), (name, float(got32[0]), want)
        for dt, tol in ((torch.float32, 0.0), (torch.float64, (S + 1) * 1e-10)):          # fp64 keeps the 1e-10 of each factor
            sigma = torch.full((1, S), ME.SIGMA_OPAQUE, dtype=dt)
            _, acc, w_ref, _ = oh.raw2outputs(torch.zeros(1, S, 3, dtype=dt), sigma, z[None].to(dt), d.to(dt), mask[None].to(dt), None, last_dist=1.0)
            assert float((w_ref[0].double() - w).abs().max()) <= tol, (name, dt)
    cases = ME.hand_cases(S)
    assert cases["last"][2] == cases["nowhere"][2] == float(z[-1])
    assert cases["tie"][2] == float(z[2]) and cases["sample0"][2] == 1.0 + 1.0 / 128.0
    # the all-background ray of the merge entry: densities 0 / 1e30 give weights 0 / 1 exactly (mask = 1, last_dist = 1e10)
    for name, (den, want) in ME.merge_hand_cases(S).items():
        _, _, w32, _ = oh.raw2outputs(torch.zeros(1, S, 3), den[None].float(), z[None].float(), d, torch.ones(1, S))
        assert set(w32[0].tolist()) <= {0.0, 1.0}, name
        assert float(ME.median_definition(w32.double(), z[None])[0][0]) == want, name


def test_median_entries_are_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "hosrender.h")).read()
    flat = lambda s: [p.strip() for p in s.replace("\n", " ").split(",")]
    for new, old in (("hos_merge_composite_median_fwd", "hos_merge_composite_maps_fwd"), ("hos_raw2outputs_median_fwd", "hos_raw2outputs_fwd")):
        m = re.search(r"int %s\(([^;]*)\);" % new, header)
        assert m, f"include/hosrender.h does not declare {new}"
        params = flat(m.group(1))
        base = flat(re.search(r"int %s\(([^;]*)\);" % old, header).group(1))
        # the arguments of the entry it extends, then `float* depth_median`, then the stream
        assert params[:-2] == base[:-1] and params[-2] == "float* depth_median" and params[-1] == base[-1] == "hos_stream_t stream", new
        from hosnerf_amd import _lib
        assert len(_lib.PROTOTYPES[new]) == len(params) == len(_lib.PROTOTYPES[old]) + 1
    assert "M:73-94" in header and "helper.py:166-190" in header
    lib_path = os.path.join(ROOT, "hosnerf_amd", "lib", "libhosrender.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("hos_")}
    declared = set(re.findall(r"\b(hos_[a-z0-9_]+)\s*\(", header)) - {"hos_stream_t"}
    assert {"hos_merge_composite_median_fwd", "hos_raw2outputs_median_fwd"} <= exported and exported == declared, exported ^ declared
    lib = _lib.load()
    assert lib.hos_version() == _lib.abi_version(_lib.HEADER)            # entries were added, no signature changed: same revision
    # argument validation happens before any launch
    import ctypes
    buf = (ctypes.c_float * 4)()
    a = ctypes.addressof(buf)
    assert lib.hos_merge_composite_median_fwd(*([0] * 10), 4, 32, 128, 5e-3, *([0] * 10), 0) == -1
    assert lib.hos_merge_composite_median_fwd(*([a] * 10), 4, 32, 128, 5e-3, 0, *([0] * 9), 0) == -1          # no rgb buffer
    assert lib.hos_merge_composite_median_fwd(*([a] * 10), 4, 200, 128, 5e-3, a, *([0] * 9), 0) == -3         # Sb + Sh > 256
    assert lib.hos_raw2outputs_median_fwd(0, 4, 0, 4, 0, 0, 0, 0, 1e10, 4, 32, 0, 0, 0, 0, 0, 0) == -1
    assert lib.hos_raw2outputs_median_fwd(a, 4, a, 4, a, a, 0, 0, 1e10, 4, 32, 0, 0, 0, 0, a, 0) == -1         # no rgb buffer
    assert lib.hos_raw2outputs_median_fwd(a, 4, a, 4, a, a, 0, 0, 1e10, 4, 257, a, 0, 0, 0, a, 0) == -3        # S > 256


def test_save_median_files(tmp_path):
    from PIL import Image
    from hosnerf_amd.freeview import depth_preview, save_frame_maps
    H, W = 12, 16
    g = torch.Generator().manual_seed(6)
    med = torch.rand(H * W, generator=g) * 4 + 1
    med[:3] = 1e6                                                        # rays that never reach 0.5: the far sample
    paths = save_frame_maps(str(tmp_path / "out"), "image-00007", {"depth_median": med}, H, W)
    assert sorted(os.listdir(tmp_path / "out")) == ["image-00007_depth_median.npy", "image-00007_depth_median.png"]
    assert sorted(os.path.basename(p) for p in paths.values()) == sorted(os.listdir(tmp_path / "out"))
    back = np.load(paths["depth_median.npy"])
    assert back.dtype == np.float32 and back.shape == (H, W) and np.array_equal(back, med.view(H, W).numpy())
    prev = np.asarray(Image.open(paths["depth_median.png"]))
    assert prev.dtype == np.uint8 and prev.shape == (H, W) and np.array_equal(prev, depth_preview(med.view(H, W).numpy()))
    assert prev.max() == 255 and prev.min() == 0 and len(np.unique(prev)) > 10
    # a numpy array is taken as well (what a caller holds after .cpu().numpy())
    again = save_frame_maps(str(tmp_path / "out2"), "frame_000001", {"depth_median": med.numpy()}, H, W)
    assert np.array_equal(np.load(again["depth_median.npy"]), back)


def test_launcher_parses_render_median():
    import run as launcher
    from hosnerf_amd import gin_lite
    gin = os.path.join(ROOT, "configs", "hosnerf_backpack.gin")
    g = gin_lite.parse_config_files_and_bindings([gin], ["run.render_maps=True", "run.render_median=True"])
    assert g.kwargs("run")["render_median"] is True
    assert "render_median" not in gin_lite.parse_config_files_and_bindings([gin], None).kwargs("run")          # default: off
    base = ["--ginc", gin, "--scene_name", "Backpack", "--cpu", "--ginb", "run.max_steps=3"]
    plan = launcher.main(base + ["--logbase", tempfile.mkdtemp(), "--ginb", "run.render_maps=True", "--ginb", "run.render_median=True"])
    assert plan["gin"]["run.render_median"] is True and plan["model_name"] == "hosnerf"
    with pytest.raises(SystemExit) as e:
        launcher.main(base + ["--logbase", tempfile.mkdtemp(), "--ginb", "run.render_median=True"])
    assert "run.render_median" in str(e.value) and "run.render_maps" in str(e.value)
    with pytest.raises(SystemExit):
        launcher.main(base + ["--logbase", tempfile.mkdtemp(), "--ginb", "run.render_maps=False", "--ginb", "run.render_median=True"])
    # stage 1 accepts the binding (its maps contain the median already)
    s1 = os.path.join(ROOT, "configs", "state_mipnerf360_backpack.gin")
    plan1 = launcher.main(["--ginc", s1, "--scene_name", "Backpack", "--cpu", "--logbase", tempfile.mkdtemp(), "--ginb", "run.max_steps=3",
                           "--ginb", "run.render_maps=True", "--ginb", "run.render_median=True"])
    assert plan1["model_name"] == "state_mipnerf360"
    assert "run.render_median" in launcher.__doc__


def test_median_api_without_gpu():
    """`median=True` is one of the maps: refused without `maps=True`, and under the conditions that refuse `maps=True`, before any
    kernel is reached; every new argument defaults to off and the existing constants are the ones they were."""
    from hosnerf_amd import eval as ev, ops
    from hosnerf_amd.hosnerf import HOSNeRF
    from hosnerf_amd.human_nerf import default_cfg
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    hos = HOSNeRF(default_cfg(d))
    with torch.no_grad():
        with pytest.raises(ValueError):
            hos.render({}, is_train=False, median=True)                   # no maps=True
        with pytest.raises(ValueError):
            hos.render_bkg_only({}, median=True)
        with pytest.raises(ValueError):
            hos.render({}, is_train=True, maps=True, median=True)         # a training call
    with pytest.raises(ValueError):
        hos.render({}, is_train=False, maps=True, median=True)            # autograd on
    with pytest.raises(ValueError):
        hos.render_bkg_only({}, maps=True, median=True)
    with pytest.raises(ValueError):
        ev.render_frame(hos, {}, median=True)
    with pytest.raises(ValueError):
        ev.render_human_frame(hos, {}, median=True)
    with pytest.raises(ValueError):
        ops.merge_composite_maps(*([None] * 9), want=("depth_median", "median"))
    for fn in (hos.render, hos.render_bkg_only, ev.render_frame, ev.render_human_frame, ev.assemble_maps):
        assert inspect.signature(fn).parameters["median"].default is False, fn
    assert inspect.signature(ops.merge_composite_maps).parameters["want"].default == ops.MAP_KEYS
    assert ops.MAP_KEYS == ("acc", "depth", "rgb_human", "acc_human", "rgb_bkg", "acc_bkg") and "depth_median" not in ops.MAP_KEYS
    assert (ev.FG_MAP_WIDTH, ev.BG_MAP_WIDTH) == (9, 5) and "depth_median" not in ev.FG_MAP_COLS and "depth_median" not in ev.BG_MAP_COLS
    assert ev.FG_MEDIAN_COLS["depth_median"] == 9 and ev.BG_MEDIAN_COLS["depth_median"] == 5
    # one more column through pack_maps / assemble_maps, 0 on pixels of neither list
    H, W = 3, 4
    g = torch.Generator().manual_seed(2)
    ray_mask = torch.tensor([1, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0], dtype=torch.bool)
    miss = ~ray_mask
    miss[2] = False                                                       # pixel 2 belongs to neither list
    n_fg, n_bg = int(ray_mask.sum()), int(miss.sum())
    fg_out = {k: torch.rand((n_fg, 3) if k.startswith("rgb") else (n_fg,), generator=g) for k in ev.FG_MEDIAN_COLS}
    bg_out = {k: torch.rand((n_bg, 3) if k.startswith("rgb") else (n_bg,), generator=g) for k in ev.BG_MEDIAN_COLS}
    fg_p, bg_p = ev.pack_maps(fg_out, ev.FG_MEDIAN_COLS), ev.pack_maps(bg_out, ev.BG_MEDIAN_COLS)
    assert tuple(fg_p.shape) == (n_fg, 10) and tuple(bg_p.shape) == (n_bg, 6)
    maps = ev.assemble_maps(H, W, (0.0, 0.0, 0.0), ray_mask, miss, fg_p, bg_p, median=True)
    assert set(maps) == {"rgb", "alpha", "depth", "rgb_human", "alpha_human", "depth_median"}
    assert torch.equal(maps["depth_median"][ray_mask], fg_out["depth_median"]) and torch.equal(maps["depth_median"][miss], bg_out["depth_median"])
    assert float(maps["depth_median"][2]) == 0.0 and float(maps["depth"][2]) == 0.0
    plain = ev.assemble_maps(H, W, (0.0, 0.0, 0.0), ray_mask, miss, fg_p[:, :9], bg_p[:, :5])
    assert set(plain) == set(maps) - {"depth_median"} and all(torch.equal(plain[k], maps[k]) for k in plain)
