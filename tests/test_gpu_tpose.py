"""The T-pose turntable on the device: the compacted frame rays (hos_frame_rays_compact) against the existing two entries bit for bit
and against the reference's arrays (tests/golden/tpose.npz), the paint kernel (hos_frame_paint) against the torch expressions it
replaces, a human-only frame (`eval.render_human_frame`) against the oracle, and the launcher's `run.run_tpose`."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle.human as oh
from hosnerf_amd import formats, synth, tpose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tpose.npz"))
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def camera(H, W):
    """The T-pose camera for an H x W image (principal point at the centre, the focal length of a 512-wide image scaled to W)."""
    K, E = tpose.tpose_camera(W, 6.0, 1250.0 * W / 512)
    K = K.astype(np.float64)
    K[1, 2] = H / 2.0
    return K, E.astype(np.float64)


def boxes(H, W):
    """Boxes hit by no ray, by every ray, by about half the rays, by ONE column of pixels (an input box of negative thickness: the
    kernel grows it by 0.01 on every side), and the fixture's rotated boxes."""
    dx = 6.0 / (1250.0 * W / 512)                       # pixel pitch on the plane z = 0, 6 in front of the camera
    xc = (W // 2 + 3 - W / 2.0) * dx
    out = {"none": [[50, 50, 50], [51, 51, 51]], "all": [[-5, -5, -1], [5, 5, 1]], "half": [[0.0, -5, -1], [5, 5, 1]],
           "column": [[xc + 0.01 - 0.3 * dx, -5, 0.0], [xc - 0.01 + 0.3 * dx, 5, 0.0]]}
    for i in G["idxs"]:
        out[f"fixture{int(i)}"] = [G[f"i{int(i)}_box_min"], G[f"i{int(i)}_box_max"]]
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}


def composed(H, W, K, E, box, dev):
    """The existing composition (`eval.frame_rays`, core/data/human_nerf/tpose.py:173-183): two launches + boolean indexing."""
    from hosnerf_amd import rays
    o, d = rays.get_rays_from_KRT(H, W, K, E[:3, :3], E[:3, 3], device=dev)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    near, far, m = rays.rays_intersect_3d_bbox(box, o, d)
    return {"ray_mask": m, "pix": torch.nonzero(m).reshape(-1).to(torch.int32), "rays_o": o[m], "rays_d": d[m], "near": near, "far": far}


# 37 x 29: a tail, five blocks; 64 x 64: whole blocks; 1024 x 512: 2048 block counts, two passes of the 1024-thread scan
@pytest.mark.parametrize("H,W", [(37, 29), (64, 64), (1024, 512)])
def test_compaction_equals_the_existing_kernels(dev, H, W):
    from hosnerf_amd import rays
    K, E = camera(H, W)
    seen = {}
    for name, box in boxes(H, W).items():
        want = composed(H, W, K, E, box, dev)
        got = rays.frame_rays_compact(H, W, K, E[:3, :3], E[:3, 3], box, device=dev)
        n = int(want["ray_mask"].sum())
        seen[name] = n
        assert got["count"] == n, (name, got["count"], n)
        assert torch.equal(got["slot"] >= 0, want["ray_mask"]), name
        for k in ("pix", "rays_o", "rays_d", "near", "far"):
            assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (name, k)          # bit for bit, no element excluded
        slot = got["slot"]
        assert slot.dtype == torch.int32 and slot.shape == (H * W,)
        assert torch.equal(slot[got["pix"].long()], torch.arange(n, dtype=torch.int32, device=dev))  # slot inverts pix ...
        assert int((slot == -1).sum()) == H * W - n and int(slot.min()) >= -1                       # ... and is -1 elsewhere
        if name == "column":
            assert int(want["ray_mask"].view(H, W).any(0).sum()) == 1 and n == H
    assert seen["none"] == 0 and seen["all"] == H * W and 0.4 * H * W < seen["half"] < 0.6 * H * W, seen
    assert any(0 < seen[k] < H * W for k in seen if k.startswith("fixture")), seen


def test_compaction_is_deterministic(dev):
    from hosnerf_amd import rays
    H, W = 1024, 512
    K, E = camera(H, W)
    box = boxes(H, W)["half"]
    a = rays.frame_rays_compact(H, W, K, E[:3, :3], E[:3, 3], box, device=dev)
    b = rays.frame_rays_compact(H, W, K, E[:3, :3], E[:3, 3], box, device=dev)
    assert a["count"] == b["count"] > 0
    for k in ("pix", "slot", "rays_o", "rays_d", "near", "far"):
        assert torch.equal(a[k], b[k]), k
    assert bool((a["pix"][1:] > a["pix"][:-1]).all())                     # pixel order, whatever the scheduling


def test_fixture_frames_vs_reference(dev):
    """The reference's own `Dataset.__getitem__` arrays, by the criterion of tests/test_gpu_rays.py::test_rays_aabb_vs_reference:
    validity flags exact, near / far to 5e-6."""
    from hosnerf_amd import rays
    S = int(G["img_size"])
    for i in (int(i) for i in G["idxs"]):
        p = f"i{i}_"
        got = rays.frame_rays_compact(S, S, G["K"], G["E"][:3, :3], G["E"][:3, 3], np.stack([G[p + "box_min"], G[p + "box_max"]]), device=dev)
        m = (got["slot"] >= 0).cpu().numpy()
        assert np.array_equal(m, G[p + "ray_mask"]), f"frame {i}: {int((m != G[p + 'ray_mask']).sum())} validity flags differ"
        assert np.abs(got["near"].cpu().numpy() - G[p + "near"][:, 0]).max() < 5e-6
        assert np.abs(got["far"].cpu().numpy() - G[p + "far"][:, 0]).max() < 5e-6
        assert np.abs(got["rays_o"].cpu().numpy() - G[p + "rays"][0]).max() < 2e-6          # tests/test_gpu_rays.py::test_camera_rays_vs_reference
        assert np.abs(got["rays_d"].cpu().numpy() - G[p + "rays"][1]).max() < 2e-6


@pytest.mark.parametrize("H,W", [(13, 11), (37, 29)])
def test_paint_equals_the_masked_assignment(dev, H, W):
    from hosnerf_amd import eval as ev, rays
    g = torch.Generator().manual_seed(H * W)
    bgcolor = (10.0, 120.0, 255.0)
    bg = torch.as_tensor(bgcolor, dtype=torch.float32, device=dev).reshape(3) / 255.0
    for fill in ("some", "none", "all"):
        mask = {"some": torch.rand(H * W, generator=g) > 0.4, "none": torch.zeros(H * W, dtype=torch.bool),
                "all": torch.ones(H * W, dtype=torch.bool)}[fill].to(dev)
        n = int(mask.sum())
        slot = torch.full((H * W,), -1, dtype=torch.int32, device=dev)
        slot[mask] = torch.arange(n, dtype=torch.int32, device=dev)
        rgb = (torch.randn(n, 3, generator=g) * 0.8 + 0.5)                # values below 0 and above 1
        exact = (torch.arange(256, dtype=torch.float32) / 255.0)          # values at k / 255 exactly
        m = min(rgb.numel() // 2, 256)
        rgb.view(-1)[:m] = exact[256 - m:]
        rgb = rgb.to(dev)
        if n:
            assert float(rgb.min()) < 0.0 and float(rgb.max()) > 1.0
        want = bg.expand(H * W, 3).clone()
        want[mask] = rgb
        want8 = ev.to_8b_image(want)
        f32, u8 = rays.paint_frame(slot, rgb if n else None, bgcolor, H, W)
        assert torch.equal(f32, want) and torch.equal(u8, want8), fill
        only8 = rays.paint_frame(slot, rgb, bgcolor, H, W, want_u8=True, want_f32=False)                 # each output NULL in turn
        only32 = rays.paint_frame(slot, rgb, bgcolor, H, W, want_u8=False)
        assert only8[0] is None and torch.equal(only8[1], want8) and only32[1] is None and torch.equal(only32[0], want), fill
    with pytest.raises(ValueError):
        rays.paint_frame(slot, rgb, bgcolor, H, W, want_u8=False, want_f32=False)


# ------------------------------------------------------------------------------------------ a human-only frame against the oracle
def build_hos(dev):
    from hosnerf_amd.hosnerf import HOSNeRF
    from hosnerf_amd.human_nerf import default_cfg
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    m = HOSNeRF(default_cfg(d))                                          # 128 samples, 32^3 volume: tests/test_gpu_human.py's network
    m.model.load_state_dict(synth.background_state_dict(777, 2), strict=False)
    m.human.load_state_dict(synth.human_state_dict(777, 2), strict=True)
    return m.to(dev)


@pytest.fixture(scope="module")
def human_frames(dev):
    """One 24 x 24 T-pose frame (camera 6 of 8: the box seen from the side covers part of the image) at the two times of
    `tpose_times([0.4])`, rendered once; the oracle's forward on the same rays and weights, computed once."""
    from hosnerf_amd import eval as ev
    hos = build_hos(dev)
    joints = synth.tpose_joints()
    bbox = formats.skeleton_bbox(joints, float(hos.cfg.bbox_offset))
    turn = tpose.TposeTurn(joints, bbox, 32, dev, img_size=24, focal=1250.0 * 24 / 512)
    hsd = synth.human_state_dict(777, 2)
    res = []
    for t in tpose.tpose_times(hos.human.transitions_times):
        fr = tpose.tpose_frame(None, None, 6, 8, bgcolor=(255.0, 255.0, 255.0), turn=turn, iter_val=3e5, time=t)
        maps, u8 = ev.render_human_frame(hos, fr, maps=True, want_u8=True)
        plain = ev.render_human_frame(hos, fr)
        with torch.no_grad(), ev.evaluating(hos):
            per = {k: fr[k] for k in ev.FRAME_KEYS if k in fr}
            net = hos.human(rays=fr["rays"], near=fr["near"], far=fr["far"], with_cycle=False, **per)
        cpu = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in fr.items()}
        with torch.no_grad():
            ref = oh.human_forward(hsd, cpu, transitions_times=[0.4], stage=3)
        res.append({"time": t, "frame": fr, "maps": maps, "u8": u8, "plain": plain, "net": net, "ref": ref})
    return res


def test_human_frame_vs_oracle(dev, human_frames):
    from hosnerf_amd import eval as ev
    from hosnerf_amd.mipnerf360 import select_state
    assert [select_state(r["time"], np.array([0.4], np.float32)) for r in human_frames] == [0, 1]          # both sides of the transition
    for r in human_frames:
        fr, maps, ref = r["frame"], r["maps"], r["ref"]
        H = W = 24
        n = fr["count"]
        assert 0 < n < H * W and set(maps) == {"rgb", "alpha", "depth"}
        assert torch.equal(maps["rgb"], r["plain"]) and torch.equal(r["u8"], ev.to_8b_image(maps["rgb"]))
        mask = fr["ray_mask"]
        # colour: the oracle's human forward + its _raw2outputs restatement; the bound of the composited colour of the human
        # forward (tests/test_gpu_stage2.py:73, the north-star RGB L-inf 1e-4 that smoke() holds the stage-2 network to)
        rgb_o, acc_o, _, depth_o = oh.raw2outputs(ref["human_rgb"], ref["human_density"], ref["z_vals"], ref["rays_d"], ref["pts_mask"], ref["bgcolor"])
        err = float((maps["rgb"][mask].cpu() - rgb_o).abs().max())
        print(f"tpose frame t={r['time']:.2f}: {n} rays, rgb L-inf vs oracle {err:.3e}")
        assert err < 1e-4
        white = torch.full((3,), 255.0, device=dev) / 255.0
        assert torch.equal(maps["rgb"][~mask], white.expand(H * W - n, 3))                                # the frame's background colour
        assert float(maps["alpha"][~mask].abs().sum()) == 0.0 and float(maps["depth"][~mask].abs().sum()) == 0.0
        # alpha / depth: the bound tests/test_gpu_maps.py holds the background-only maps of the same kernel to --
        # |hip - fp64| <= 2 |fp32 oracle - fp64| + one ulp on the kernel's own inputs, depth relative to sum w |z|
        net = {k: r["net"][k].cpu() for k in ("human_rgb", "human_density", "z_vals", "rays_d", "pts_mask")}
        out = {}
        for name, dt in (("fp32", torch.float32), ("fp64", torch.float64)):
            c = lambda t: t.to(dt)
            _, acc, w, depth = oh.raw2outputs(c(net["human_rgb"]), c(net["human_density"]), c(net["z_vals"]), c(net["rays_d"]), c(net["pts_mask"]))
            out[name] = {"alpha": acc, "depth": depth, "scale": torch.sum(w * c(net["z_vals"]).abs(), -1)}
        for k in ("alpha", "depth"):
            scale = out["fp64"]["scale"].clamp_min(1e-30) if k == "depth" else torch.ones((), dtype=torch.float64)
            e_hip = float(((maps[k][mask].double().cpu() - out["fp64"][k]).abs() / scale).max())
            e_ref = float(((out["fp32"][k].double() - out["fp64"][k]).abs() / scale).max())
            print(f"tpose frame t={r['time']:.2f}: {k} hip {e_hip:.3e} fp32 oracle {e_ref:.3e}")
            assert e_hip <= 2.0 * e_ref + ULP, (k, e_hip, e_ref)
        assert float(maps["alpha"].max()) > 0.0
    a, b = human_frames
    assert float((a["maps"]["rgb"] - b["maps"]["rgb"]).abs().max()) > 1e-3, "the state never reached the canonical MLP"


def test_frame_without_rays_launches_only_the_paint(dev):
    from hosnerf_amd import eval as ev
    joints = synth.tpose_joints()
    turn = tpose.TposeTurn(joints, {"min_xyz": np.array([50.0, 50.0, 50.0]), "max_xyz": np.array([51.0, 51.0, 51.0])}, 8, dev, img_size=16,
                           focal=1250.0 * 16 / 512)
    fr = tpose.tpose_frame(None, None, 0, 8, bgcolor=(0.0, 128.0, 255.0), turn=turn, time=0.2)
    assert fr["count"] == 0 and fr["rays"].shape == (2, 0, 3)
    out, u8 = ev.render_human_frame(None, fr, want_u8=True)             # no network is touched
    want = (torch.tensor([0.0, 128.0, 255.0], device=dev) / 255.0).expand(256, 3)
    assert torch.equal(out, want) and torch.equal(u8, ev.to_8b_image(want))
    maps = ev.render_human_frame(None, fr, maps=True)
    assert float(maps["alpha"].abs().sum()) == 0.0 and float(maps["depth"].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------ the launcher
def test_launcher_writes_one_turn_per_state(tmp_path):
    """`run.run_tpose = True` on a synthetic 2-state scene directory: 2 x 4 JPEGs of 512 x 512 under the reference's names; two ranks on
    one GPU (frames dealt round-robin, no collectives) write byte-identical files."""
    from PIL import Image
    from hosnerf_amd.freeview import write_scene_pixels
    scene = str(tmp_path / "scene")
    write_scene_pixels(scene, synth.write_scene_dir(scene, 6, 64, 64, seed=9))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("patch:\n  N_patches: 2\n  size: 16\n")
    logs = str(tmp_path / "logs")
    base = [os.path.join(ROOT, "run.py"), "--ginc", os.path.join(ROOT, "configs", "hosnerf_backpack.gin"), "--ginb", "run.max_steps=2",
            "--ginb", f'run.datadir="{scene}"', "--ginb", 'run.human_path=""', "--ginb", 'run.bkgd_path=""', "--ginb", "run.run_tpose=True",
            "--ginb", "run.render_maps=True", "--scene_name", "synthetic", "--scene_dir", scene, "--cfg", str(cfg), "--render_frames", "4"]
    r = subprocess.run([sys.executable] + base + ["--logbase", logs], capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    logdir = [os.path.join(logs, d) for d in os.listdir(logs)][0]
    with open(os.path.join(scene, "transitions_times.json")) as f:
        tt = [v["time"] for v in json.load(f).values()]
    times = tpose.tpose_times(tt)
    assert len(times) == 2
    files = {}
    for t in times:
        folder = os.path.join(logdir, "tpose_vis", "time_{:06}".format(t))
        assert sorted(os.listdir(folder)) == sorted(["image-{:05}.jpg".format(k) for k in range(4)] + ["image-{:05}_alpha.png".format(k) for k in range(4)])
        for k in range(4):
            path = os.path.join(folder, "image-{:05}.jpg".format(k))
            assert np.asarray(Image.open(path)).shape == (512, 512, 3)
            assert np.asarray(Image.open(os.path.join(folder, "image-{:05}_alpha.png".format(k)))).shape == (512, 512)
            files[(t, k)] = open(path, "rb").read()
    assert "results.json" in os.listdir(logdir) and json.load(open(os.path.join(logdir, "results.json")))["tpose"]["frames"] == 4
    # two ranks share the GPU (the rehearsal of tests/test_gpu_dist.py); same checkpoint, nothing trained again
    logs2 = str(tmp_path / "logs2")
    os.makedirs(os.path.join(logs2, os.path.basename(logdir)))
    import shutil
    shutil.copy(os.path.join(logdir, "last.ckpt"), os.path.join(logs2, os.path.basename(logdir), "last.ckpt"))
    env = dict(os.environ, HOS_ROOT=ROOT, HOS_BENCH_ONE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29571"] + \
        base + ["--logbase", logs2, "--ginb", "run.run_train=False"]
    r2 = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r2.returncode == 0, (r2.stdout[-3000:], r2.stderr[-4000:])
    for (t, k), data in files.items():
        path = os.path.join(logs2, os.path.basename(logdir), "tpose_vis", "time_{:06}".format(t), "image-{:05}.jpg".format(k))
        assert open(path, "rb").read() == data, (t, k)
