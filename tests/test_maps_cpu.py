"""CPU side of the depth / opacity / layer maps: the frame scatter (`eval.assemble_maps`), the files `freeview.save_frame_maps` writes, the
new C entry in the header, the library and the ctypes mirror, and the launcher's `run.render_maps` binding."""
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


def test_assemble_maps_scatters_both_ray_lists():
    from hosnerf_amd import eval as ev
    H, W = 5, 4
    g = torch.Generator().manual_seed(3)
    ray_mask = torch.rand(H * W, generator=g) > 0.5
    miss = ~ray_mask
    n_fg, n_bg = int(ray_mask.sum()), int(miss.sum())
    assert n_fg > 2 and n_bg > 2
    fg_out = {"rgb": torch.rand(n_fg, 3, generator=g), "alpha": torch.rand(n_fg, generator=g), "depth": torch.rand(n_fg, generator=g) * 1e5,
              "rgb_human": torch.rand(n_fg, 3, generator=g), "alpha_human": torch.rand(n_fg, generator=g),
              "rgb_bkg": torch.rand(n_fg, 3, generator=g), "idx_fg": torch.ones(n_fg, dtype=torch.int32)}       # extra keys are not packed
    bg_out = {"rgb": torch.rand(n_bg, 3, generator=g), "alpha": torch.rand(n_bg, generator=g), "depth": torch.rand(n_bg, generator=g) * 1e5}
    fg_packed, bg_packed = ev.pack_maps(fg_out, ev.FG_MAP_COLS), ev.pack_maps(bg_out, ev.BG_MAP_COLS)
    assert tuple(fg_packed.shape) == (n_fg, ev.FG_MAP_WIDTH) and tuple(bg_packed.shape) == (n_bg, ev.BG_MAP_WIDTH)
    maps = ev.assemble_maps(H, W, (10.0, 120.0, 250.0), ray_mask, miss, fg_packed, bg_packed)
    assert set(maps) == {"rgb", "alpha", "depth", "rgb_human", "alpha_human"}
    fg_pix, bg_pix = torch.nonzero(ray_mask).reshape(-1), torch.nonzero(miss).reshape(-1)
    for k in maps:
        assert tuple(maps[k].shape) == ((H * W, 3) if k.startswith("rgb") else (H * W,))
        assert torch.equal(maps[k][fg_pix], fg_out[k]), k                 # i-th ray of the list -> i-th set pixel of its mask, exact values
        if k in bg_out:
            assert torch.equal(maps[k][bg_pix], bg_out[k]), k
        else:
            assert float(maps[k][bg_pix].abs().sum()) == 0.0, k           # no human layer where the ray misses the box
    # a pixel of neither list keeps the frame's background colour and empty maps (M:1311-1313)
    hole = ray_mask.clone()
    hole[fg_pix[0]] = False
    m2 = ev.assemble_maps(H, W, (10.0, 120.0, 250.0), hole, miss, fg_packed[1:], bg_packed)
    assert torch.equal(m2["rgb"][fg_pix[0]], torch.tensor([10.0, 120.0, 250.0]) / 255.0)
    assert float(m2["alpha"][fg_pix[0]]) == 0.0 and float(m2["depth"][fg_pix[0]]) == 0.0
    # empty ray lists (a camera that sees only background, or only the box)
    m3 = ev.assemble_maps(H, W, (0.0, 0.0, 0.0), torch.zeros(H * W, dtype=torch.bool), torch.ones(H * W, dtype=torch.bool),
                          torch.zeros(0, ev.FG_MAP_WIDTH), torch.rand(H * W, ev.BG_MAP_WIDTH, generator=g))
    assert float(m3["alpha_human"].abs().sum()) == 0.0 and float(m3["alpha"].sum()) > 0.0


def test_save_maps_files(tmp_path):
    from PIL import Image
    from hosnerf_amd.freeview import depth_preview, save_frame_maps
    H, W = 12, 16
    g = torch.Generator().manual_seed(5)
    depth = torch.rand(H * W, generator=g) * 4 + 1
    depth[:2] = 1e6                                                       # 1 % of the pixels at the far plane
    ah = torch.rand(H * W, generator=g)
    ah[10:20] = 0.0
    straight = torch.rand(H * W, 3, generator=g)
    maps = {"rgb": torch.rand(H * W, 3, generator=g), "alpha": torch.rand(H * W, generator=g), "depth": depth,
            "rgb_human": straight * ah[:, None], "alpha_human": ah}
    paths = save_frame_maps(str(tmp_path / "out"), "image-00007", maps, H, W)
    assert sorted(os.path.basename(p) for p in paths.values()) == sorted(
        ["image-00007_depth.npy", "image-00007_depth.png", "image-00007_alpha.png", "image-00007_alpha_human.png", "image-00007_human.png"])
    back = np.load(paths["depth.npy"])
    assert back.dtype == np.float32 and back.shape == (H, W) and np.array_equal(back, depth.view(H, W).numpy())
    to8 = lambda x: (np.clip(x, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    prev = np.asarray(Image.open(paths["depth.png"]))
    d = depth.view(H, W).numpy().astype(np.float64)
    lo, hi = np.percentile(d, 2.0), np.percentile(d, 98.0)
    assert prev.dtype == np.uint8 and np.array_equal(prev, to8((d - lo) / (hi - lo))) and np.array_equal(prev, depth_preview(d))
    assert prev.max() == 255 and prev.min() == 0 and len(np.unique(prev)) > 10          # the far-plane pixels do not flatten the rest
    assert np.array_equal(np.asarray(Image.open(paths["alpha.png"])), to8(maps["alpha"].view(H, W).numpy()))
    assert np.array_equal(np.asarray(Image.open(paths["alpha_human.png"])), to8(ah.view(H, W).numpy()))
    rgba = np.asarray(Image.open(paths["human.png"]))
    assert rgba.shape == (H, W, 4) and np.array_equal(rgba[..., 3], to8(ah.view(H, W).numpy()))
    empty = (ah.view(H, W) == 0).numpy()
    assert empty.sum() == 10 and not rgba[empty].any()                     # nothing where the layer is empty
    got = rgba[..., :3][~empty].astype(np.int32)
    assert np.abs(got - to8(straight.view(H, W, 3).numpy())[~empty].astype(np.int32)).max() <= 1        # un-premultiplied colour
    # a constant depth map does not divide by zero
    assert np.array_equal(depth_preview(np.full((2, 2), 3.0)), np.zeros((2, 2), np.uint8))


def test_maps_entry_is_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "hosrender.h")).read()
    m = re.search(r"int hos_merge_composite_maps_fwd\(([^;]*)\);", header)
    assert m, "include/hosrender.h does not declare hos_merge_composite_maps_fwd"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    base = re.search(r"int hos_merge_composite_fwd\(([^;]*)\);", header).group(1).replace("\n", " ").split(",")
    assert params[:14] == [p.strip() for p in base[:14]]                  # all inputs of hos_merge_composite_fwd, same order
    assert [p.split()[-1] for p in params[14:]] == ["rgb", "idx_fg", "total_order", "acc", "depth", "rgb_human", "acc_human", "rgb_bkg",
                                                    "acc_bkg", "stream"]
    from hosnerf_amd import _lib
    assert len(_lib.PROTOTYPES["hos_merge_composite_maps_fwd"]) == len(params)              # the stream included
    lib_path = os.path.join(ROOT, "hosnerf_amd", "lib", "libhosrender.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("hos_")}
    declared = set(re.findall(r"\b(hos_[a-z0-9_]+)\s*\(", header)) - {"hos_stream_t"}
    assert "hos_merge_composite_maps_fwd" in exported and exported == declared, exported ^ declared
    lib = _lib.load()
    # argument validation happens before any launch: no rgb buffer / no inputs -> HOS_E_ARG, too many merged samples -> HOS_E_SHAPE
    assert lib.hos_merge_composite_maps_fwd(*([0] * 10), 4, 32, 128, 5e-3, *([0] * 9), 0) == -1
    import ctypes
    buf = (ctypes.c_float * 4)()
    a = ctypes.addressof(buf)
    assert lib.hos_merge_composite_maps_fwd(*([a] * 10), 4, 32, 128, 5e-3, 0, *([0] * 8), 0) == -1
    assert lib.hos_merge_composite_maps_fwd(*([a] * 10), 4, 200, 128, 5e-3, a, *([0] * 8), 0) == -3


def test_render_maps_api_without_gpu():
    """`maps=True` is refused before any kernel is reached when autograd is on or the call is a training one."""
    import json
    from hosnerf_amd.hosnerf import HOSNeRF
    from hosnerf_amd.human_nerf import default_cfg
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    hos = HOSNeRF(default_cfg(d))
    with pytest.raises(ValueError):
        hos.render({}, is_train=False, maps=True)
    with torch.no_grad(), pytest.raises(ValueError):
        hos.render({}, is_train=True, maps=True)
    with pytest.raises(ValueError):
        hos.render_bkg_only({}, maps=True)
    import inspect
    from hosnerf_amd import eval as ev
    assert inspect.signature(hos.render).parameters["maps"].default is False
    assert inspect.signature(hos.render_bkg_only).parameters["maps"].default is False
    assert inspect.signature(ev.render_frame).parameters["maps"].default is False


def test_launcher_parses_render_maps():
    import run as launcher
    from hosnerf_amd import gin_lite
    g = gin_lite.parse_config_files_and_bindings([os.path.join(ROOT, "configs", "hosnerf_backpack.gin")], ["run.render_maps=True"])
    assert g.kwargs("run")["render_maps"] is True
    g0 = gin_lite.parse_config_files_and_bindings([os.path.join(ROOT, "configs", "hosnerf_backpack.gin")], None)
    assert "render_maps" not in g0.kwargs("run")                          # default: off, outputs as before
    logs = tempfile.mkdtemp()
    plan = launcher.main(["--ginc", os.path.join(ROOT, "configs", "hosnerf_backpack.gin"), "--scene_name", "Backpack", "--logbase", logs,
                          "--cpu", "--ginb", "run.max_steps=3", "--ginb", "run.render_maps=True"])
    assert plan["gin"]["run.render_maps"] is True and plan["model_name"] == "hosnerf"
