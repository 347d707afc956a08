"""The stage-1 ray bank on the device (hos_raybank.hip, hosnerf_amd/raybank.py) against the reference's own tables
(tests/golden/stage1_rays.npz = `batchified_get_rays` under `split_each` / `split_each_val`, tests/golden/make_golden_stage1_rays.py),
the sampler's properties, the whole-frame render loop and the stage-1 launcher from a scene directory.

Bounds: `times` / `target` exact (copied / one correctly rounded division); `rays_o`, `rays_d`, `viewdirs` within 2e-6 and `radii`
within 2e-7 + 1e-4 * max -- the bounds tests/test_gpu_rays.py uses for the same arithmetic (fp32 on the device against the reference's
float64 numpy rounded to float32)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "stage1_rays.npz"))
N, H, W = G["images_u8"].shape[:3]
KEYS = ("rays_o", "rays_d", "viewdirs", "radii", "times", "target")


def fixture_scene():
    return {"extrinsics": G["extrinsics"], "intrinsics": G["intrinsics"], "times": G["times"], "render_poses": G["render_poses"],
            "render_times": G["render_times"], "i_split": (G["i_train"], G["i_train"][:2], G["i_test"], np.arange(N)),
            "bkgrays_sizes": np.sum(G["masks"] < 1, axis=(1, 2))}


@pytest.fixture(scope="module")
def bank():
    from hosnerf_amd.raybank import RayBank
    return RayBank(fixture_scene(), G["images_u8"], G["masks"], device="cuda", split="train")


def check_table(got, prefix, rows=slice(None), target=True):
    g = {k: v.detach().cpu().numpy() for k, v in got.items()}
    want = {k: G[f"{prefix}_{k}"][rows] for k in KEYS if k != "target" or target}
    assert set(g) == set(want)
    assert g["radii"].shape == want["radii"].shape and g["radii"].ndim == 2 and g["times"].ndim == 1
    errs = {k: float(np.abs(g[k].astype(np.float64) - want[k]).max()) for k in want}
    print(prefix, {k: f"{v:.3e}" for k, v in errs.items()})
    assert np.array_equal(g["times"], want["times"])
    if target:
        assert np.array_equal(g["target"], want["target"])
    for k in ("rays_o", "rays_d", "viewdirs"):
        assert errs[k] < 2e-6, (k, errs[k])
    assert errs["radii"] < 2e-7 + 1e-4 * float(want["radii"].max())
    assert float(np.abs(np.linalg.norm(g["viewdirs"].astype(np.float64), axis=-1) - 1.0).max()) < 1e-6


def test_index_matches_the_reference_compaction(bank):
    keep = G["masks"] < 1
    assert np.array_equal(bank.counts_host, G["counts"]) and bank.counts_host[int(G["zero_image"])] == 0
    assert bank.counts_host[int(G["full_image"])] == H * W
    assert np.array_equal(bank.offsets_host, np.concatenate([[0], np.cumsum(G["counts"])]))
    want = np.concatenate([np.flatnonzero(keep[i].reshape(-1)) for i in range(N)])
    assert bank.pix.dtype == torch.int32 and np.array_equal(bank.pix.cpu().numpy()[:len(want)], want)


def test_index_across_workgroup_boundaries():
    """H = 3, W = 257: 771 pixels per image = four 256-pixel workgroups, the last one ragged; kept pixels on both sides of every
    boundary, an empty and a full image between irregular ones (the running offset passes over both)."""
    from hosnerf_amd.raybank import RayBank
    rs = np.random.RandomState(5)
    n, h, w = 4, 3, 257
    masks = (rs.rand(n, h, w) < 0.5).astype(np.float32)
    masks[1], masks[2] = 1.0, 0.0
    for i in (0, 3):
        flat = masks[i].reshape(-1)
        flat[[255, 256, 511, 512, 767, 768, 770]] = 0.0           # kept
        flat[[254, 257, 0]] = 1.0                                  # dropped
    keep = masks < 1
    scene = {"extrinsics": np.stack([np.eye(4)] * n), "intrinsics": np.stack([np.array([[300.0, 0, 128.5], [0, 300.0, 1.5], [0, 0, 1.0]])] * n),
             "times": np.linspace(0, 1, n).astype(np.float32), "render_poses": None, "render_times": None,
             "i_split": (np.arange(n), np.arange(2), np.arange(0), np.arange(n)), "bkgrays_sizes": keep.sum(axis=(1, 2))}
    b = RayBank(scene, np.zeros((n, h, w, 3), np.uint8), masks, device="cuda")
    assert b.counts_host.tolist() == [int(keep[i].sum()) for i in range(n)] and b.counts_host[1] == 0 and b.counts_host[2] == h * w
    want = np.concatenate([np.flatnonzero(keep[i].reshape(-1)) for i in range(n)])
    assert np.array_equal(b.pix.cpu().numpy()[:len(want)], want) and int(b.offsets_host[-1]) == len(want)


def test_gather_every_training_ray(bank):
    """Every entry of the reference's training table, addressed as (image id, rank in the image's list), in the table's order."""
    ids = np.concatenate([np.full(int(G["counts"][i]), i, np.int32) for i in G["i_train"]])
    ks = np.concatenate([np.arange(int(G["counts"][i]), dtype=np.int32) for i in G["i_train"]])
    assert len(ids) == len(G["train_rays_o"]) == int(G["counts"][G["i_train"]].sum())         # no entry is left out
    got = bank.gather(torch.from_numpy(ids).cuda(), torch.from_numpy(ks).cuda())
    check_table(got, "train")
    # the reference sampler's own batches: table rows idx_jump[image] + idx -> (image, rank) through the same cumulative counts
    jump = np.concatenate([[0], np.cumsum(G["counts"][G["i_train"]])])
    for row in G["sampler_idx"]:
        pos = np.searchsorted(jump, row, side="right") - 1
        assert len(set(pos.tolist())) == 1                                                      # single_image: one image per batch
        got = bank.gather(torch.from_numpy(G["i_train"][pos].astype(np.int32)).cuda(), torch.from_numpy((row - jump[pos]).astype(np.int32)).cuda())
        check_table(got, "train", rows=row)
    # a pair outside the bank reads nothing: NaN row, neighbours untouched
    bad = bank.gather(torch.tensor([0, int(G["zero_image"]), N, 0], dtype=torch.int32).cuda(),
                      torch.tensor([0, 0, 0, int(G["counts"][0])], dtype=torch.int32).cuda())
    assert bool(torch.isfinite(bad["rays_d"][0]).all()) and bool(torch.isnan(bad["rays_d"][1:]).all()) and bool(torch.isnan(bad["times"][1:]).all())


def test_frame_whole_chunked_and_without_target(bank):
    i = int(G["frame"])
    whole = bank.frame(i)
    check_table(whole, "frame")
    for chunk in (7, 64):                   # 7 puts chunk edges mid-row; neither divides 240
        parts = [bank.frame(i, s, min(chunk, H * W - s)) for s in range(0, H * W, chunk)]
        for k in KEYS:
            assert torch.equal(torch.cat([p[k] for p in parts], 0), whole[k]), (chunk, k)
    k = int(G["pose"])
    pose = bank.render_pose(k)              # NULL target
    assert "target" not in pose
    check_table(pose, "pose", rows=slice(k * H * W, (k + 1) * H * W), target=False)
    assert bank.frame(i, H * W, 0)["rays_o"].shape == (0, 3)                                   # an empty range launches nothing
    with pytest.raises(ValueError):
        bank.frame(i, H * W - 3, 4)


def test_sampler_properties(bank):
    dev = torch.device("cuda")

    def gen(seed):
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        return g

    def rows(b):         # (pixel-exact) identity of each sampled ray: its image through `times`, its pixel through the direction
        return torch.cat([b["times"][:, None], b["rays_d"], b["target"]], 1)

    train = [int(i) for i in G["i_train"]]
    seen = set()
    g = gen(3)
    for _ in range(24):
        b = bank.sample(64, g)
        assert all(b[k].shape[0] == 64 for k in KEYS) and b["radii"].shape == (64, 1)
        t = b["times"].unique()
        assert t.numel() == 1                                                                   # one image per step
        img = int(np.flatnonzero(G["times"] == float(t))[0])
        assert img in train and img != int(G["zero_image"]) and img not in [int(i) for i in G["i_test"]]
        seen.add(img)
    assert seen == set(train) - {int(G["zero_image"])}                                         # (3 images, 24 draws: 3 * (2/3)^24 < 2e-4)
    for seed in range(6):
        img, k = bank.draw(512, gen(seed))
        assert int(k.min()) >= 0 and int(k.max()) < int(G["counts"][int(img)]) and k.dtype == torch.int32
    # ranks 0 and 1 of 2 with equal seeds interleave to the world-1 draw
    full, r0, r1 = bank.sample(33, gen(9)), bank.sample(33, gen(9), 0, 2), bank.sample(33, gen(9), 1, 2)
    assert r0["times"].shape[0] == 17 and r1["times"].shape[0] == 16
    for k in KEYS:
        assert torch.equal(full[k][0::2], r0[k]) and torch.equal(full[k][1::2], r1[k]), k
    assert bank.sample(0, gen(1))["rays_o"].shape == (0, 3) and bank.sample(1, gen(1))["target"].shape == (1, 3)
    assert bank.sample(1, gen(1), 1, 2)["times"].shape == (0,)                                  # this rank's share of one ray: none


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from hosnerf_amd import synth
    from hosnerf_amd.mipnerf360 import MipNeRF360
    d = str(tmp_path_factory.mktemp("base"))
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    m = MipNeRF360(d, opaque_background=True)
    m.load_state_dict(synth.background_state_dict(777, 2), strict=False)
    return m.to("cuda")


def test_render_bkgd_frame_is_the_chunked_model_call(bank, model):
    from hosnerf_amd import eval as ev
    i, n = int(G["frame"]), H * W
    a = ev.render_bkgd_frame(model, bank, i, 64, 0.5, 0.1, 1e6)
    assert a.shape == (n, 3) and bool(torch.isfinite(a).all()) and float(a.std()) > 0
    with torch.no_grad():
        direct = torch.cat([model(bank.frame(i, s, min(64, n - s)), 0.5, False, False, 0.1, 1e6)[0][-1]["rgb"] for s in range(0, n, 64)], 0)
    assert torch.equal(a, direct)
    assert torch.equal(a, ev.render_bkgd_frame(model, bank, ("frame", i), 64, 0.5, 0.1, 1e6))
    b = ev.render_bkgd_frame(model, bank, i, 97, 0.5, 0.1, 1e6)
    print("re-chunking 64 -> 97:", float((a - b).abs().max()))
    assert float((a - b).abs().max()) < 1e-6                                                    # the bound of test_gpu_eval's re-chunking check
    p = ev.render_bkgd_frame(model, bank, ("pose", int(G["pose"])), 240, 0.5, 0.1, 1e6)
    assert p.shape == (n, 3) and bool(torch.isfinite(p).all())
    assert model.training                                                                        # left as it was


# ------------------------------------------------------------------------------------------ launcher
SH = SW = 24
N_FRAMES = 6


def _cmd(scene, logs, extra, ranks=1, port=29581):
    head = [sys.executable]
    if ranks > 1:
        head += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1", "--master-port", str(port)]
    return head + [os.path.join(ROOT, "run.py"), "--ginc", os.path.join(ROOT, "configs", "state_mipnerf360_backpack.gin"),
                   "--ginb", "run.max_steps=3", "--ginb", "run.log_every_n_steps=1", "--ginb", f'run.datadir="{scene}"',
                   "--ginb", "LitData.batch_size=512", "--ginb", "LitData.chunk=200", "--ginb", "run.run_eval=True", "--ginb", "run.run_render=True",
                   "--logbase", logs, "--scene_name", "synthetic", "--scene_dir", scene, "--render_limit", "2"] + extra


def _files(logdir):
    return sorted(os.path.join(d, f) for d in ("render_model", "render_video") for f in os.listdir(os.path.join(logdir, d))) + \
        sorted(f for f in os.listdir(logdir) if f == "results.json")


@pytest.fixture(scope="module")
def launched(tmp_path_factory):
    """One single-rank run of the stage-1 launcher on a scene directory: three steps, run_eval, run_render."""
    from hosnerf_amd import synth
    from hosnerf_amd.freeview import write_scene_pixels
    tmp = tmp_path_factory.mktemp("stage1")
    scene, logs = str(tmp / "scene"), str(tmp / "logs")
    write_scene_pixels(scene, synth.write_scene_dir(scene, N_FRAMES, SH, SW, seed=9))
    r = subprocess.run(_cmd(scene, logs, []), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    logdir = [os.path.join(logs, d) for d in os.listdir(logs)][0]
    return {"scene": scene, "logdir": logdir, "stdout": r.stdout, "tmp": tmp}


def test_launcher_trains_evaluates_and_renders_stage1(launched):
    from PIL import Image
    import run as launcher
    from hosnerf_amd import eval as ev, select_option
    out, logdir = launched["stdout"], launched["logdir"]
    steps = [l for l in out.splitlines() if l.startswith("[run] step")]
    assert len(steps) == 3 and all(np.isfinite(float(l.split(" loss ")[1].split()[0])) for l in steps) and "Test PSNR" in out
    want = [os.path.join("render_model", f"image{j:03d}.jpg") for j in range(N_FRAMES)] + \
           [os.path.join("render_video", f"image{k:03d}.jpg") for k in range(2)] + ["results.json"]
    assert _files(logdir) == want
    for f in want[:-1]:
        img = Image.open(os.path.join(logdir, f))
        assert img.size == (SW, SH) and img.mode == "RGB"
    res = json.load(open(os.path.join(logdir, "results.json")))
    assert set(res) == {"PSNR"} and set(res["PSNR"]) == {"mean", "test"} and res["PSNR"]["mean"] == res["PSNR"]["test"]
    # psnr_each (interface.py:42-50) recomputed here from the checkpoint, render_bkgd_frame and the scene's pixels
    dev = torch.device("cuda")
    lit = select_option.select_model("state_mipnerf360", launched["scene"], max_steps=3, grad_max_norm=0.001, near=0.1, far=1e6)
    select_option.load_checkpoint(lit, os.path.join(logdir, "last.ckpt"), strict=True)
    lit = lit.to(dev)
    ck = torch.load(os.path.join(logdir, "last.ckpt"), map_location="cpu", weights_only=False)
    assert ck["global_step"] == 3
    bank = launcher.load_ray_bank(launched["scene"], dev, 0.1, 1e6)
    assert [int(i) for i in bank.i_test] == list(range(N_FRAMES))
    px = np.stack([np.asarray(Image.open(os.path.join(launched["scene"], "images", f"frame_{i:06d}.png")).convert("RGB")) for i in range(N_FRAMES)])
    psnrs = []
    for i in range(N_FRAMES):
        pred = ev.render_bkgd_frame(lit.model, bank, i, 200, 3 / 3, 0.1, 1e6).double().cpu().clamp(0, 1)
        gt = torch.from_numpy(px[i].reshape(-1, 3).astype(np.float32) / np.float32(255.0)).double().clamp(0, 1)
        psnrs.append(-10.0 * float(torch.log(torch.mean((pred - gt) ** 2))) / np.log(10))
    print("PSNR", res["PSNR"]["test"], "recomputed", float(np.mean(psnrs)))
    assert 0.0 < res["PSNR"]["test"] < 60.0 and abs(res["PSNR"]["test"] - float(np.mean(psnrs))) < 1e-6


def test_launcher_two_ranks_on_one_gpu_stage1(launched):
    """The evaluation and the render path of the same checkpoint as TWO processes on the one GPU (HOS_BENCH_ONE_GPU=1: gloo transport,
    testing only, as tests/test_gpu_scene.py launches its two-rank cases): frames dealt round-robin, each rank writes its own files,
    one all-reduce of the PSNR vector -- the same file set and the same PSNRs."""
    logs = str(launched["tmp"] / "logs2")
    e = dict(os.environ)
    e.update(HOS_BENCH_ONE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    cmd = _cmd(launched["scene"], logs, ["--ginb", "run.run_train=False", "--ckpt_path", os.path.join(launched["logdir"], "last.ckpt")], ranks=2)
    r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    assert "world 2" in r.stdout and "[run] step" not in r.stdout and "Test PSNR" in r.stdout
    logdir = [os.path.join(logs, d) for d in os.listdir(logs)][0]
    assert _files(logdir) == _files(launched["logdir"])
    a = json.load(open(os.path.join(launched["logdir"], "results.json")))
    b = json.load(open(os.path.join(logdir, "results.json")))
    print("PSNR one rank", a["PSNR"], "two ranks", b["PSNR"])
    assert set(b) == {"PSNR"} and all(abs(a["PSNR"][k] - b["PSNR"][k]) < 1e-6 for k in ("mean", "test"))
