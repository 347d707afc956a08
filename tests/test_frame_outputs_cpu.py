"""What the launcher's output entry points WRITE, without a GPU: `run.evaluate_and_render` (stage 3 and, through it, the T-pose turn
and stage 1), `run.extract_meshes` and `run.extract_frame_meshes` are called directly with the renderers, the checkpoint loader, the
T-pose cameras and the mesh extractors replaced by recording stubs that return known tensors; the assertions are about the files,
their contents, results.json / meshes.json, what the renderers were asked for, and the refusals' messages."""
import argparse
import io
import json
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import run as launcher
from hosnerf_amd import eval as ev, mesh, select_option, tpose

H, W = 3, 4
RAY_MASK = torch.tensor([1, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0], dtype=torch.bool)
MISS = ~RAY_MASK
MISS[2] = False                                                           # pixel 2 belongs to neither ray list
BGC = (10.0, 120.0, 250.0)
MAP_FILES = ("_depth.npy", "_depth.png", "_alpha.png", "_alpha_human.png", "_human.png")
MEDIAN_FILES = ("_depth_median.npy", "_depth_median.png")
MODES = [(False, False), (True, False), (True, True)]                     # (run.render_maps, run.render_median)


def known(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def stage3_frame(name, seed):
    n_fg, n_bg = int(RAY_MASK.sum()), int(MISS.sum())
    return {"frame_name": name, "seed": seed, "img_height": H, "img_width": W, "bgcolor": BGC, "ray_mask": RAY_MASK, "ray_mask_bkg": MISS,
            "rays_o_bkg": torch.zeros(n_fg, 3), "rays_o_bkg_only": torch.zeros(n_bg, 3), "target_rgbs": known(seed + 50, n_fg, 3),
            "target_rgbs_bkg": known(seed + 60, n_bg, 3)}


def stage3_maps(seed, median):
    m = {"rgb": known(seed, H * W, 3), "alpha": known(seed + 1, H * W), "depth": known(seed + 2, H * W) * 9, "rgb_human": known(seed + 3, H * W, 3),
         "alpha_human": known(seed + 4, H * W)}
    if median:
        m["depth_median"] = known(seed + 5, H * W) * 7
    return m


class Scene:
    canonical_joints, canonical_bbox = "joints", "bbox"

    def __init__(self, bad_pose=False):
        self.bad_pose = bad_pose

    def __len__(self):
        return 6

    def eval_frame(self, i, bgcolor):
        assert bgcolor == BGC
        return stage3_frame(f"frame_{i:06d}", 10 * i)

    def freeview_frame(self, fidx, k, total, bgcolor):
        assert (fidx, total, bgcolor) == (0, 5, BGC)
        return stage3_frame(f"view_{k}", 1000 + 10 * k)

    def frame_pose(self, i):
        return {"frame_name": f"frame_{i:06d}", "i": i, "bad": self.bad_pose}


def make_lit(max_steps=10):
    human = NS(transitions_times=[0.4])
    cfg = NS(chunk_bkg=8192, bgcolor=list(BGC), freeview=NS(frame_idx=0), mweight_volume=NS(volume_size=32))
    return NS(net=NS(human=human), human=human, cfg=cfg, model="model", max_steps=max_steps, near=0.1, far=1e6)


@pytest.fixture
def stubs(monkeypatch, tmp_path):
    """Recording stubs for everything that needs the GPU or a trained network, a checkpoint {"global_step": 3} and a log folder."""
    calls = {k: [] for k in ("load", "frame", "human", "bkgd", "turn", "tpose_frame", "extract", "extract_frame")}

    def render_frame(hos, fr, chunk_bkg=8192, randomized=False, group=None, cache_prologue=True, maps=False, median=False):
        calls["frame"].append({"name": fr["frame_name"], "chunk_bkg": chunk_bkg, "randomized": randomized, "maps": maps, "median": median})
        out = stage3_maps(fr["seed"], median)
        return out if maps else out["rgb"]

    def render_human_frame(hos, fr, maps=False, want_u8=False, median=False):
        calls["human"].append({"k": fr["k"], "time": fr["time"], "maps": maps, "want_u8": want_u8, "median": median})
        out = tpose_maps(fr["k"], fr["time"], median)
        return (out if maps else out["rgb"]), tpose_u8(fr["k"], fr["time"])

    def render_bkgd_frame(model, bank, frame_or_pose, chunk, train_frac, near, far, maps=False):
        calls["bkgd"].append({"what": frame_or_pose, "chunk": chunk, "train_frac": train_frac, "maps": maps})
        out = bkgd_maps(frame_or_pose)
        return out if maps else out["rgb"]

    def tpose_frame(a, b, k, total, bgcolor, turn, iter_val, time):
        calls["tpose_frame"].append({"k": k, "total": total, "iter_val": iter_val, "time": time})
        return {"img_height": H, "img_width": W, "k": k, "time": time}

    def extract(net, turn, time, resolution=256, level=0.5):
        calls["extract"].append({"time": time, "resolution": resolution, "level": level})
        return stub_mesh(int(time * 10))

    def extract_frame(net, pose, resolution=256, level=0.5, space="world", normals=False):
        calls["extract_frame"].append({"i": pose["i"], "resolution": resolution, "level": level, "space": space, "normals": normals})
        if pose["bad"]:
            raise ValueError("cameras.pkl has no smpl_to_scale_world")
        m = stub_mesh(pose["i"] + 1)
        m.update(frame_name=pose["frame_name"], time=pose["i"] / 8.0, space=space, to_world=np.eye(4) * (pose["i"] + 1),
                 normals=torch.ones_like(m["vertices"]) if normals else None)
        return m

    monkeypatch.setattr(ev, "render_frame", render_frame)
    monkeypatch.setattr(ev, "render_human_frame", render_human_frame)
    monkeypatch.setattr(ev, "render_bkgd_frame", render_bkgd_frame)
    monkeypatch.setattr(select_option, "load_checkpoint", lambda lit, ckpt, strict=False: calls["load"].append(strict))
    monkeypatch.setattr(tpose, "TposeTurn", lambda *a: calls["turn"].append(a) or "turn")
    monkeypatch.setattr(tpose, "tpose_frame", tpose_frame)
    monkeypatch.setattr(mesh, "extract", extract)
    monkeypatch.setattr(mesh, "extract_frame", extract_frame)
    ckpt = str(tmp_path / "last.ckpt")
    torch.save({"global_step": 3}, ckpt)
    return NS(calls=calls, ckpt=ckpt, logdir=str(tmp_path / "logs"), args=argparse.Namespace(eval_skip=3, render_frames=5, render_limit=2))


def listing(folder):
    return sorted(os.listdir(folder)) if os.path.isdir(folder) else []


# ------------------------------------------------------------------------------------------ stage 3
@pytest.mark.parametrize("render_maps,render_median", MODES)
def test_stage3_frames_files_and_results(stubs, render_maps, render_median):
    from PIL import Image
    kw = {"render_maps": render_maps, "render_median": render_median}
    got = launcher.evaluate_and_render(stubs.args, kw, make_lit(), "hosnerf", Scene(), stubs.ckpt, stubs.logdir, "cpu", 0, 1, True, True)
    kinds = (MAP_FILES if render_maps else ()) + (MEDIAN_FILES if render_median else ())
    frames = [("test_vis", "frame_000000", ".png", 0), ("test_vis", "frame_000003", ".png", 30),
              (os.path.join("freeview_vis_newtrans", "view_00000"), "image-00000", ".jpg", 1000),
              (os.path.join("freeview_vis_newtrans", "view_00000"), "image-00001", ".jpg", 1010)]
    for folder in {f[0] for f in frames}:                                 # each folder holds these files and nothing else
        want = sorted(stem + x for f, stem, ext, _ in frames if f == folder for x in (ext,) + kinds)
        assert listing(os.path.join(stubs.logdir, folder)) == want, folder
    psnrs = []
    for folder, stem, ext, seed in frames:
        maps = stage3_maps(seed, render_median)
        path = os.path.join(stubs.logdir, folder, stem)
        if ext == ".png":                                                 # lossless: the colour file is `to_8b_image` of the stub's colours
            assert np.array_equal(np.asarray(Image.open(path + ext)), ev.to_8b_image(maps["rgb"].view(H, W, 3)).numpy())
        for k in ("depth",) * render_maps + ("depth_median",) * render_median:
            back = np.load(f"{path}_{k}.npy")
            assert back.dtype == np.float32 and np.array_equal(back, maps[k].view(H, W).numpy()), (stem, k)
        if render_maps:
            assert np.array_equal(np.asarray(Image.open(path + "_alpha.png")), (maps["alpha"].view(H, W).numpy() * 255.0 + 0.5).astype(np.uint8))
        psnrs.append(ev.psnr_metric(maps["rgb"], ev.truth_frame(stage3_frame(stem, seed))))
    # the renderer was asked for exactly these maps, frame by frame in this order
    assert stubs.calls["frame"] == [{"name": n, "chunk_bkg": 8192, "randomized": False, "maps": render_maps, "median": render_median}
                                    for n in ("frame_000000", "frame_000003", "view_0", "view_1")]
    assert stubs.calls["load"] == [True] and stubs.calls["human"] == []
    want = {"test": {"psnr": float(sum(psnrs[:2]) / 2), "frames": {"frame_000000": psnrs[0], "frame_000003": psnrs[1]}},
            "freeview": {"frame_idx": 0, "frames": 2, "of": 5, "psnr_vs_training_frame": float(sum(psnrs[2:]) / 2)}}
    assert got == {"results": want}
    text = open(os.path.join(stubs.logdir, "results.json")).read()
    assert text == json.dumps(want, indent=1)
    assert sorted(os.listdir(stubs.logdir)) == ["freeview_vis_newtrans", "results.json", "test_vis"]


def test_stage3_other_ranks_write_nothing(stubs):
    got = launcher.evaluate_and_render(stubs.args, {"render_maps": True, "render_median": True}, make_lit(), "hosnerf", Scene(), stubs.ckpt,
                                       stubs.logdir, "cpu", 1, 1, True, True)
    assert not os.path.exists(stubs.logdir) or os.listdir(stubs.logdir) == []
    assert len(stubs.calls["frame"]) == 4 and got["results"]["freeview"]["frames"] == 2          # it renders its share and reports all the same


# ------------------------------------------------------------------------------------------ T-pose
ALPHAS = (0.998, 0.999, 0.5, 0.25, 1.0, 0.0)                              # 0.999 * 255 = 254.745, 0.5 * 255 = 127.5: truncating and rounding differ


def tpose_maps(k, time, median):
    seed = 100 * k + int(time * 10)
    alpha = known(seed + 1, H * W)
    alpha[:len(ALPHAS)] = torch.tensor(ALPHAS)
    m = {"rgb": known(seed, H * W, 3), "alpha": alpha, "depth": known(seed + 2, H * W) * 9}
    if median:
        m["depth_median"] = known(seed + 3, H * W) * 7
    return m


def tpose_u8(k, time):
    return (known(100 * k + int(time * 10) + 7, H * W, 3) * 255).to(torch.uint8)


@pytest.mark.parametrize("render_maps,render_median", MODES)
def test_tpose_turn_files(stubs, render_maps, render_median):
    from PIL import Image
    stubs.args.render_frames, stubs.args.render_limit = 4, 0
    kw = {"render_maps": render_maps, "render_median": render_median}
    got = launcher.evaluate_and_render(stubs.args, kw, make_lit(), "hosnerf", Scene(), stubs.ckpt, stubs.logdir, "cpu", 1, 2, False, False, True)
    times = tpose.tpose_times([0.4])
    assert len(times) == 2 and got == {"results": {"tpose": {"times": times, "frames": 4, "of": 4}}}
    assert listing(os.path.join(stubs.logdir, "tpose_vis")) == sorted("time_{:06}".format(t) for t in times)
    for t in times:
        folder = os.path.join(stubs.logdir, "tpose_vis", "time_{:06}".format(t))
        stems = ["image-{:05}".format(k) for k in (1, 3)]                 # rank 1 of 2: frames 1 and 3 only
        want = [s + x for s in stems for x in (".jpg",) + (("_alpha.png",) if render_maps else ()) + (MEDIAN_FILES if render_median else ())]
        assert listing(folder) == sorted(want)                            # never a _depth file, although the dict holds `depth`
        for k, stem in zip((1, 3), stems):
            maps = tpose_maps(k, t, render_median)
            buf = io.BytesIO()
            Image.fromarray(tpose_u8(k, t).view(H, W, 3).numpy()).save(buf, format="JPEG")
            assert open(os.path.join(folder, stem + ".jpg"), "rb").read() == buf.getvalue()          # the paint kernel's 8-bit frame as it is
            if render_maps:
                alpha8 = np.asarray(Image.open(os.path.join(folder, stem + "_alpha.png")))
                trunc = ev.to_8b_image(maps["alpha"].view(H, W)).numpy()
                assert np.array_equal(alpha8, trunc)
                assert not np.array_equal(trunc, (maps["alpha"].view(H, W).numpy() * 255.0 + 0.5).astype(np.uint8))          # truncation was kept
            if render_median:
                assert np.array_equal(np.load(os.path.join(folder, stem + "_depth_median.npy")), maps["depth_median"].view(H, W).numpy())
    assert stubs.calls["human"] == [{"k": k, "time": t, "maps": render_maps, "want_u8": True, "median": render_median} for t in times for k in (1, 3)]
    # the cameras of the whole turn, at the checkpoint's global_step
    assert stubs.calls["tpose_frame"] == [{"k": k, "total": 4, "iter_val": 3.0, "time": t} for t in times for k in (1, 3)]
    assert stubs.calls["turn"] == [("joints", "bbox", 32, "cpu")] and stubs.calls["frame"] == []


def test_tpose_step_of_a_bare_state_dict(stubs):
    torch.save({"some.weight": torch.zeros(1)}, stubs.ckpt)
    stubs.args.render_frames, stubs.args.render_limit = 4, 1
    launcher.evaluate_and_render(stubs.args, {}, make_lit(), "hosnerf", Scene(), stubs.ckpt, stubs.logdir, "cpu", 0, 1, False, False, True)
    assert [c["iter_val"] for c in stubs.calls["tpose_frame"]] == [1e7, 1e7] and [c["k"] for c in stubs.calls["tpose_frame"]] == [0, 0]
    assert all(c["maps"] is False and c["median"] is False for c in stubs.calls["human"])          # both bindings default to off


# ------------------------------------------------------------------------------------------ stage 1
def bkgd_maps(frame_or_pose):
    seed = 500 + (10 * frame_or_pose[1] if isinstance(frame_or_pose, tuple) else frame_or_pose)
    return {"rgb": known(seed, H * W, 3), "alpha": known(seed + 1, H * W), "depth": known(seed + 2, H * W) * 1e5, "depth_median": known(seed + 3, H * W) * 9}


class Bank:
    H, W, i_test, render_poses = H, W, np.array([0, 2, 4]), [None, None]

    def truth(self, i):
        return known(700 + i, H * W, 3)


@pytest.mark.parametrize("render_maps", [False, True])
def test_stage1_frames_files_and_results(stubs, render_maps):
    stubs.args.render_limit = 0
    got = launcher.evaluate_and_render(stubs.args, {"render_maps": render_maps}, make_lit(), "state_mipnerf360", Bank(), stubs.ckpt, stubs.logdir,
                                       "cpu", 0, 1, True, True, bkgd_chunk=4096)
    kinds = (".jpg",) + (("_depth.npy", "_depth.png", "_depth_median.npy", "_depth_median.png", "_alpha.png") if render_maps else ())
    assert listing(os.path.join(stubs.logdir, "render_model")) == sorted(f"image{j:03d}{x}" for j in range(3) for x in kinds)
    assert listing(os.path.join(stubs.logdir, "render_video")) == sorted(f"image{k:03d}{x}" for k in range(2) for x in kinds)
    if render_maps:
        for folder, j, what in (("render_model", 1, 2), ("render_video", 1, ("pose", 1))):
            for k in ("depth", "depth_median"):
                back = np.load(os.path.join(stubs.logdir, folder, f"image{j:03d}_{k}.npy"))
                assert np.array_equal(back, bkgd_maps(what)[k].view(H, W).numpy())
    whats = [0, 2, 4, ("pose", 0), ("pose", 1)]
    assert stubs.calls["bkgd"] == [{"what": w, "chunk": 4096, "train_frac": 0.3, "maps": render_maps} for w in whats]          # global_step 3 of 10
    want = ev.bkgd_results([ev.psnr_each(bkgd_maps(i)["rgb"], Bank().truth(i)) for i in (0, 2, 4)])
    assert got == {"results": want}
    assert open(os.path.join(stubs.logdir, "results.json")).read() == json.dumps(want, indent=4, sort_keys=True)


# ------------------------------------------------------------------------------------------ mesh sets
def stub_mesh(n):
    """A mesh of n + 2 vertices and n faces with measures that are exact in JSON."""
    v = torch.arange(3 * (n + 2), dtype=torch.float32).view(-1, 3)
    return {"vertices": v, "faces": torch.arange(3 * n, dtype=torch.int32).view(-1, 3) % (n + 2), "colors": (v * 7).to(torch.uint8), "state": n % 2,
            "volume": 0.5 * n, "area": 1.25 * n, "spacing": 0.03125, "dims": (n + 3, n + 4, n + 5), "normals": None}


# what the launcher wrote for these stub meshes before its two mesh entry points shared `write_mesh_set` (recorded from that code)
CANONICAL_ROWS = {
    "time_0.20000000298023224": {"time": 0.20000000298023224, "state": 0, "V": 4, "F": 2, "volume": 1.0, "area": 2.5, "level": 0.25,
                                 "spacing": 0.03125, "dims": [5, 6, 7]},
    "time_0.699999988079071": {"time": 0.699999988079071, "state": 0, "V": 8, "F": 6, "volume": 3.0, "area": 7.5, "level": 0.25,
                               "spacing": 0.03125, "dims": [9, 10, 11]}}
FRAME_ROWS = {
    "frame_000000": {"frame_name": "frame_000000", "time": 0.0, "state": 1, "V": 3, "F": 1, "volume": 0.5, "area": 1.25, "level": 0.25,
                     "spacing": 0.03125, "dims": [4, 5, 6], "space": "body",
                     "to_world": [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]},
    "frame_000003": {"frame_name": "frame_000003", "time": 0.375, "state": 0, "V": 6, "F": 4, "volume": 2.0, "area": 5.0, "level": 0.25,
                     "spacing": 0.03125, "dims": [7, 8, 9], "space": "body",
                     "to_world": [[4.0, 0.0, 0.0, 0.0], [0.0, 4.0, 0.0, 0.0], [0.0, 0.0, 4.0, 0.0], [0.0, 0.0, 0.0, 4.0]]}}


def test_canonical_mesh_set(stubs):
    from hosnerf_amd import formats
    kw = {"mesh_resolution": 16, "mesh_level": 0.25}
    got = launcher.extract_meshes(kw, make_lit(), Scene(), stubs.ckpt, stubs.logdir, "cpu", 0, 1)
    times = tpose.tpose_times([0.4])
    names = ["time_{:06}".format(t) for t in times]
    assert got == {"times": times, "resolution": 16, "level": 0.25}
    assert listing(os.path.join(stubs.logdir, "mesh")) == sorted([n + ".ply" for n in names] + ["meshes.json"])
    text = open(os.path.join(stubs.logdir, "mesh", "meshes.json")).read()
    assert names == list(CANONICAL_ROWS) and text == json.dumps(CANONICAL_ROWS, indent=1) and [list(r) for r in json.loads(text).values()] == [
        ["time", "state", "V", "F", "volume", "area", "level", "spacing", "dims"]] * 2
    v, f, c = formats.read_ply(os.path.join(stubs.logdir, "mesh", names[1] + ".ply"))
    m = stub_mesh(int(times[1] * 10))
    assert np.array_equal(v, m["vertices"].numpy()) and np.array_equal(f, m["faces"].numpy()) and np.array_equal(c, m["colors"].numpy())
    assert stubs.calls["extract"] == [{"time": t, "resolution": 16, "level": 0.25} for t in times] and stubs.calls["load"] == [True]
    assert not os.path.exists(os.path.join(stubs.logdir, "results.json"))


def test_frame_mesh_set(stubs):
    from hosnerf_amd import formats
    kw = {"mesh_resolution": 16, "mesh_level": 0.25, "mesh_space": "body"}
    got = launcher.extract_frame_meshes(stubs.args, kw, make_lit(), Scene(), stubs.ckpt, stubs.logdir, "cpu", 0, 1)
    names = ["frame_000000", "frame_000003"]                              # the frames `run.run_eval` chooses with --eval_skip 3
    assert got == {"frames": names, "resolution": 16, "level": 0.25, "space": "body"}
    assert listing(os.path.join(stubs.logdir, "mesh_frames")) == sorted([n + ".ply" for n in names] + ["meshes.json"])
    text = open(os.path.join(stubs.logdir, "mesh_frames", "meshes.json")).read()
    assert text == json.dumps(FRAME_ROWS, indent=1) and [list(r) for r in json.loads(text).values()] == [
        ["frame_name", "time", "state", "V", "F", "volume", "area", "level", "spacing", "dims", "space", "to_world"]] * 2
    v, f, c, n = formats.read_ply(os.path.join(stubs.logdir, "mesh_frames", "frame_000003.ply"), with_normals=True)
    assert v.shape == (6, 3) and f.shape == (4, 3) and np.array_equal(n, np.ones((6, 3), np.float32))          # run.mesh_normals defaults to True
    assert stubs.calls["extract_frame"] == [{"i": i, "resolution": 16, "level": 0.25, "space": "body", "normals": True} for i in (0, 3)]
    with pytest.raises(SystemExit) as e:
        launcher.extract_frame_meshes(stubs.args, kw, make_lit(), Scene(bad_pose=True), stubs.ckpt, stubs.logdir + "2", "cpu", 0, 1)
    assert str(e.value) == "run.run_mesh_frames: cameras.pkl has no smpl_to_scale_world"
    assert listing(os.path.join(stubs.logdir + "2", "mesh_frames")) == []                          # no half-written sequence


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_by_message(stubs):
    a, lit, missing = stubs.args, make_lit(), os.path.join(stubs.logdir, "none.ckpt")
    s3 = lambda scene, ckpt: launcher.evaluate_and_render(a, {}, lit, "hosnerf", scene, ckpt, stubs.logdir, "cpu", 0, 1, True, True)
    s1 = lambda bank, ckpt: launcher.evaluate_and_render(a, {}, lit, "state_mipnerf360", bank, ckpt, stubs.logdir, "cpu", 0, 1, True, True)
    cm = lambda scene, ckpt: launcher.extract_meshes({}, lit, scene, ckpt, stubs.logdir, "cpu", 0, 1)
    fm = lambda scene, ckpt: launcher.extract_frame_meshes(a, {}, lit, scene, ckpt, stubs.logdir, "cpu", 0, 1)
    tail = f": {missing} does not exist (train first, or pass --ckpt_path)"
    cases = [
        (lambda: s3(None, stubs.ckpt), "run.run_eval / run.run_render / run.run_tpose need --scene_dir (frames, cameras and SMPL fits to render)"),
        (lambda: s1(None, stubs.ckpt), "run.run_eval / run.run_render need --scene_dir (frames and cameras to render)"),
        (lambda: cm(None, stubs.ckpt), "run.run_mesh needs --scene_dir (canonical joints and box)"),
        (lambda: fm(None, stubs.ckpt), "run.run_mesh_frames needs --scene_dir (the frames' poses, boxes and cameras)"),
        (lambda: s3(Scene(), missing), "run.run_eval / run.run_render / run.run_tpose" + tail),
        (lambda: s1(Bank(), missing), "run.run_eval / run.run_render" + tail),
        (lambda: cm(Scene(), missing), "run.run_mesh" + tail),
        (lambda: fm(Scene(), missing), "run.run_mesh_frames" + tail),
        (lambda: launcher.evaluate_and_render(a, {}, lit, "state_humanobject", Scene(), stubs.ckpt, stubs.logdir, "cpu", 0, 1, True, False),
         "run.run_eval / run.run_render / run.run_tpose: full-frame rendering is the stage-1 (`state_mipnerf360`) and stage-3 (`hosnerf`) "
         "launchers'; stage 2 reports its training loss only"),
        (lambda: launcher.evaluate_and_render(a, {}, lit, "state_mipnerf360", Bank(), stubs.ckpt, stubs.logdir, "cpu", 0, 1, False, False, True),
         "run.run_tpose renders the human-object network (stage 3); stage 1 has run.run_eval / run.run_render"),
    ]
    for call, message in cases:
        with pytest.raises(SystemExit) as e:
            call()
        assert str(e.value) == message
    assert stubs.calls["load"] == [] and not os.path.exists(stubs.logdir)          # refused before anything is loaded or written
