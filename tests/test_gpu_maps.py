"""Depth / opacity / layer maps of the stage-3 composite (`hos_merge_composite_maps_fwd`) against the reference's `_raw2outputs`
(M:73-99, restated in oracle/human.py::raw2outputs) on identical inputs, the same-launch guarantees of the maps variant, the module
surface (`HOSNeRF.render(maps=True)`, `render_bkg_only(maps=True)`), whole frames (`eval.render_frame(maps=True)`, one rank and the
two-ranks-on-one-GPU rehearsal) and the launcher's `run.render_maps`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle.background as ob
import oracle.human as oh
from hosnerf_amd import synth
from tests.test_gpu_stage3 import G, T, dev, hos, load  # noqa: F401  (fixtures + helpers of the stage-3 parity tests, read-only)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("A", 16, 31), ("tinyd", 8, 32), ("nofg", 8, 33)]
ULP = 2.0 ** -23                     # one fp32 ulp of a quantity of scale 1 (opacity, colour; depth after division by sum w|z|)
MAPS = ("acc", "depth", "rgb_human", "acc_human", "rgb_bkg", "acc_bkg")


def case_inputs(tag, B, seed):
    """The oracle's tensors of one case of test_stage3_step_vs_golden (tests/test_gpu_stage3.py:105-118), on the CPU."""
    st = load("stage3_step.npz")
    p = f"c_{tag}_"
    b = synth.human_batch(B, seed=seed, time=0.5, is_train=True, iter_val=3e5)
    if tag == "tinyd":
        b["rays_d_bkg"][0, 0] = 1e-7
        b["rays_d_bkg"][1, 1] = 5e-6
    if tag == "nofg":
        b["near"] += 50.0
        b["far"] += 50.0
    bsd, hsd = synth.background_state_dict(777, 2), synth.human_state_dict(777, 2)
    bb = {"rays_o": b["rays_o_bkg"], "rays_d": b["rays_d_bkg"], "viewdirs": b["viewdirs_bkg"], "radii": b["radii"], "times": b["time"]}
    with torch.no_grad():
        _, hist = ob.mipnerf360_forward(bsd, bb, 1.0, True, 0.1, 1e6, transitions_times=[0.4],
                                        jitters=[T(st[p + f"jitter{l}"]) for l in range(3)], render=False)
        human = oh.human_forward(hsd, b, transitions_times=[0.4])
    return b, hist[-1], human, st[p + "total_order"], st[p + "idx_fg"]


def kernel_args(b, last, human, dev):
    hrs = torch.cat([human["human_rgb"], human["human_density"][..., None]], -1)
    return [t.to(dev) for t in (last["tdist"], last["rgb"], last["density"], hrs, human["newsmpl_pts"], human["pts_mask"],
                                b["rays_o_bkg"], b["rays_d_bkg"], b["newsmpl_to_scale_world"])]


def expected_maps(b, last, human, dtype):
    """The reference's composite in `dtype`: total_order / z_h / idx_fg from oracle.human.stage3_composite, the merged
    [z | rgb,sigma | mask] rows rebuilt as oracle/human.py:339-344 does, oracle.human.raw2outputs for acc / depth / w, the layer sums
    as w summed under total_order >= Sb; background rays: the 32 background samples with an all-ones mask (oracle/human.py:349).
    Also returns sum_j w_j |z_j| (the scale the depth error is measured against)."""
    with torch.no_grad():
        _, idx_fg, total_order, _, z_h = oh.stage3_composite(last["tdist"], last["rgb"], last["density"], human, b["rays_o_bkg"],
                                                             b["rays_d_bkg"], b["newsmpl_to_scale_world"])
        c = lambda t: t.to(dtype)
        B, Sb = last["density"].shape
        z_b = last["tdist"][..., :-1]
        bkg = torch.cat([last["rgb"], last["density"][..., None]], -1)
        hum = torch.cat([human["human_rgb"], human["human_density"][..., None]], -1)
        mask, d = human["pts_mask"], b["rays_d_bkg"]
        fg, bg = idx_fg, ~idx_fg
        out = {k: torch.zeros((B, 3) if k.startswith("rgb") else (B,), dtype=dtype) for k in MAPS + ("rgb", "depth_scale")}

        def put(sel, rgb, acc, w, depth, z, col, is_h):
            out["rgb"][sel], out["acc"][sel], out["depth"][sel] = rgb, acc, depth
            out["depth_scale"][sel] = torch.sum(w * z.abs(), -1)
            for name, m in (("human", is_h), ("bkg", ~is_h)):
                wm = w * m.to(dtype)
                out["acc_" + name][sel] = torch.sum(wm, -1)
                out["rgb_" + name][sel] = torch.sum(wm[..., None] * col, -2)

        if int(fg.sum()) > 0:
            zz = torch.gather(torch.cat([z_b[fg], z_h[fg]], -1), 1, total_order)                       # = the sorted values of :339
            allv = torch.gather(torch.cat([bkg[fg], hum[fg]], 1), 1, total_order[..., None].expand(-1, -1, 4))
            m = torch.gather(torch.cat([torch.ones_like(z_b[fg]), mask[fg]], -1), 1, total_order)
            rgb, acc, w, depth = oh.raw2outputs(c(allv[..., :3]), c(allv[..., 3]), c(zz), c(d[fg]), c(m))
            put(fg, rgb, acc, w, depth, c(zz), c(allv[..., :3]), total_order >= Sb)
        if int(bg.sum()) > 0:
            rgb, acc, w, depth = oh.raw2outputs(c(bkg[bg][..., :3]), c(bkg[bg][..., 3]), c(z_b[bg]), c(d[bg]), torch.ones_like(c(z_b[bg])))
            put(bg, rgb, acc, w, depth, c(z_b[bg]), c(bkg[bg][..., :3]), torch.zeros_like(z_b[bg], dtype=torch.bool))
    return out, idx_fg, total_order


def distances(got, want32, want64):
    """Per map: worst-ray distance of the kernel and of the fp32 oracle from the fp64 expectation (depth: relative to sum w|z|)."""
    res = {}
    for k in MAPS + ("rgb",):
        scale = want64["depth_scale"].clamp_min(1e-30) if k == "depth" else torch.ones((), dtype=torch.float64)       # [B] for depth [B], else 1
        e = lambda x: float(((x.double().cpu() - want64[k]).abs() / scale).max())
        res[k] = {"hip": e(got[k]), "fp32_oracle": e(want32[k])}
    return res


@pytest.mark.parametrize("tag,B,seed", CASES)
def test_maps_kernel_vs_reference_composite(dev, tag, B, seed):
    """|hip - fp64| <= 2 * max|fp32 oracle - fp64| + one fp32 ulp, per map and case, no ray excluded; integer outputs bit-exact."""
    from hosnerf_amd import ops
    from tests._record import record
    b, last, human, want_order, want_fg = case_inputs(tag, B, seed)
    got = ops.merge_composite_maps(*kernel_args(b, last, human, dev))
    w32, idx_fg, total_order = expected_maps(b, last, human, torch.float32)
    w64, _, _ = expected_maps(b, last, human, torch.float64)
    fg = got["idx_fg"].cpu().numpy().astype(bool)
    assert np.array_equal(fg, want_fg) and np.array_equal(fg, idx_fg.numpy())
    order = got["total_order"].cpu().numpy().astype(np.int64)
    assert np.array_equal(order[fg], want_order) and np.array_equal(order[fg], total_order.numpy()) and np.all(order[~fg] == -1)
    dist = distances(got, w32, w64)
    record(f"maps.kernel_vs_fp64_expectation[{tag}]", dist)
    print(f"maps parity [{tag}]:", json.dumps(dist))
    for k in MAPS:
        assert dist[k]["hip"] <= 2.0 * dist[k]["fp32_oracle"] + ULP, (tag, k, dist[k])


def _random_batch(B, Sb, Sh, seed, dev):
    g = torch.Generator().manual_seed(seed)
    td = torch.sort(torch.rand(B, Sb + 1, generator=g) * 3 + 0.2, -1).values
    brgb, bden = torch.rand(B, Sb, 3, generator=g), torch.rand(B, Sb, generator=g) * 2
    hum = torch.rand(B, Sh, 4, generator=g)
    hum[..., 3] *= 3
    mask = torch.rand(B, Sh, generator=g) * (torch.rand(B, Sh, generator=g) > 0.5)
    mask[: B // 8] = 0.0                                  # background-only rays
    o = torch.randn(B, 3, generator=g) * 0.1
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * 0.7
    zt = torch.sort(torch.rand(B, Sh, generator=g) * 3 + 0.2, -1).values
    pts = o[:, None] + d[:, None] * zt[..., None]
    return [t.to(dev) for t in (td, brgb, bden, hum, pts, mask, o, d, torch.eye(4))]


def test_maps_share_the_launch_of_rgb(dev):
    """Exact guarantees of the maps variant: rgb / idx_fg / total_order bit-identical to hos_merge_composite_fwd; the two layers add up
    to the total; no human layer on background rays; NULL for any subset of the new pointers leaves the rest unchanged."""
    from hosnerf_amd import ops
    batches = [kernel_args(*case_inputs(*c)[:3], dev) for c in CASES] + [_random_batch(4096, 32, 128, 17, dev)]
    for args in batches:
        rgb, _, idx_fg, order, _ = ops.merge_composite(*args)
        m = ops.merge_composite_maps(*args)
        assert torch.equal(m["rgb"], rgb) and torch.equal(m["idx_fg"], idx_fg) and torch.equal(m["total_order"], order)
        # Each of the three sums (total, human, background) is `per - 1` additions inside a lane (per = ceil(St / 64) <= St / 64 + 1) and
        # the 6 levels of the wave_sum tree over the SAME rounded products w_j c_j, so each is within (St / 64 + 6) * 2^-24 * sum|terms| of
        # the exact sum; the exact sums agree, sum|terms| of the parts add up to the total's, and the test's own human + bkg addition
        # rounds once more: |human + bkg - total| <= (2 * (St / 64 + 6) + 1) * 2^-24 * sum|terms| <= k * 2^-23 * max(acc, |rgb|)
        # with k = St / 64 + 6 + 1/2 and sum|terms| <= acc (colours in [0, 1]).
        St = args[2].shape[1] + args[5].shape[1]
        k = St / 64 + 6 + 0.5
        acc = m["acc"]
        assert float((m["acc_human"] + m["acc_bkg"] - acc).abs().sub(k * ULP * acc).max()) <= 0.0
        scale = torch.maximum(acc[:, None], rgb.abs())
        assert float(((m["rgb_human"] + m["rgb_bkg"] - rgb).abs() - k * ULP * scale).max()) <= 0.0
        bgr = idx_fg == 0
        assert float(m["rgb_human"][bgr].abs().sum()) == 0.0 and float(m["acc_human"][bgr].abs().sum()) == 0.0
        assert torch.equal(m["acc_bkg"][bgr], acc[bgr])
        assert bool(torch.isfinite(m["depth"]).all()) and float(acc.min()) >= 0.0 and float(acc.max()) <= 1.0 + 1e-5
        for want in (("depth",), ("acc", "rgb_human"), ("acc_human", "rgb_bkg", "acc_bkg"), ()):
            s = ops.merge_composite_maps(*args, want=want)
            assert set(s) == {"rgb", "idx_fg", "total_order", *want}
            for key, v in s.items():
                assert torch.equal(v, m[key]), (want, key)
    assert 0 < int((idx_fg == 0).sum()) < 4096                     # the random batch has rays of both kinds
    with pytest.raises(ValueError):
        ops.merge_composite_maps(*batches[0], want=("weights",))


def _gpu_batch(tag, B, seed, dev):
    b = synth.human_batch(B, seed=seed, time=0.5, is_train=False, iter_val=3e5)
    return b, {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


def test_render_maps_surface(dev, hos):
    B = 16
    _, gb = _gpu_batch("A", B, 31, dev)
    with torch.no_grad():
        base = hos.render(gb, randomized=False, is_train=False, with_cycle=False)
        out = hos.render(gb, randomized=False, is_train=False, with_cycle=False, maps=True)
    for k, shape in (("alpha", (B,)), ("depth", (B,)), ("rgb_human", (B, 3)), ("alpha_human", (B,)), ("rgb_bkg", (B, 3)), ("alpha_bkg", (B,))):
        assert k not in base and tuple(out[k].shape) == shape and not out[k].requires_grad and bool(torch.isfinite(out[k]).all()), k
    assert torch.equal(out["rgb"], base["rgb"]) and torch.equal(out["idx_fg"], base["idx_fg"]) and torch.equal(out["total_order"], base["total_order"])
    assert int(out["idx_fg"].sum()) > 0 and float(out["alpha_human"].max()) > 0.0
    with pytest.raises(ValueError):
        hos.render(gb, randomized=False, is_train=False, with_cycle=False, maps=True)          # grad enabled
    with torch.no_grad(), pytest.raises(ValueError):
        hos.render(gb, randomized=False, is_train=True, with_cycle=False, maps=True)


def test_render_bkg_only_maps_vs_reference_composite(dev, hos):
    """`bkg_rgb, bkg_alpha, bkg_depth` (M:835): alpha / depth of the background-only path against oracle.human.raw2outputs on the
    level's own ray_history[-1], to the bound of test_maps_kernel_vs_reference_composite."""
    from tests._record import record
    _, gb = _gpu_batch("A", 16, 31, dev)
    bb = {"rays_o": gb["rays_o_bkg"], "rays_d": gb["rays_d_bkg"], "viewdirs": gb["viewdirs_bkg"], "radii": gb["radii"], "times": gb["time"]}
    with torch.no_grad():
        plain = hos.render_bkg_only(bb, randomized=False, is_train=False)
        out = hos.render_bkg_only(bb, randomized=False, is_train=False, maps=True)
        _, hist = hos.model(bb, 1.0, False, False, hos.near_bkg, hos.far_bkg)
    with pytest.raises(ValueError):
        hos.render_bkg_only(bb, randomized=False, is_train=False, maps=True)
    assert isinstance(plain, torch.Tensor) and set(out) == {"rgb", "alpha", "depth"} and torch.equal(out["rgb"], plain)
    assert tuple(out["alpha"].shape) == (16,) and tuple(out["depth"].shape) == (16,)
    last = {k: hist[-1][k].cpu() for k in ("tdist", "rgb", "density")}
    z, d = last["tdist"][..., :-1], bb["rays_d"].cpu()
    res = {}
    for name, dt in (("fp32", torch.float32), ("fp64", torch.float64)):
        c = lambda t: t.to(dt)
        _, acc, w, depth = oh.raw2outputs(c(last["rgb"]), c(last["density"]), c(z), c(d), torch.ones_like(c(z)))
        res[name] = {"alpha": acc, "depth": depth, "scale": torch.sum(w * c(z).abs(), -1)}
    dist = {}
    for k in ("alpha", "depth"):
        scale = res["fp64"]["scale"].clamp_min(1e-30) if k == "depth" else torch.ones((), dtype=torch.float64)
        dist[k] = {"hip": float(((out[k].double().cpu() - res["fp64"][k]).abs() / scale).max()),
                   "fp32_oracle": float(((res["fp32"][k].double() - res["fp64"][k]).abs() / scale).max())}
    record("maps.render_bkg_only_vs_fp64_expectation", dist)
    print("maps parity [bkg_only]:", json.dumps(dist))
    for k in dist:
        assert dist[k]["hip"] <= 2.0 * dist[k]["fp32_oracle"] + ULP, (k, dist[k])


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
maps = ev.render_frame(hos, fr, chunk_bkg=64, group=dist.group.WORLD, maps=True)
torch.cuda.synchronize()
if rank == 0:
    torch.save({k: v.cpu() for k, v in maps.items()}, os.environ["HOS_MAPS_OUT"])
dist.barrier()
dist.destroy_process_group()
print("MAPS_RANK_OK", rank)
"""


def build_frame_hos(dev):
    """The synthetic renderer of tests/test_gpu_eval.py's `hos` fixture (same weights), buildable outside pytest."""
    import tempfile
    from hosnerf_amd.hosnerf import HOSNeRF
    from hosnerf_amd.human_nerf import default_cfg
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    m = HOSNeRF(default_cfg(d))
    m.model.load_state_dict(synth.background_state_dict(777, 2), strict=False)
    m.human.load_state_dict(synth.human_state_dict(777, 2), strict=True)
    return m.to(dev)


def test_render_frame_maps(dev, tmp_path):
    from hosnerf_amd import eval as ev
    from tests.test_gpu_eval import make_frame
    hos_f = build_frame_hos(dev)
    H, W = 20, 16
    fr, _ = make_frame(dev, H, W)
    rendered = ev.render_frame(hos_f, fr, chunk_bkg=8192)
    maps = ev.render_frame(hos_f, fr, chunk_bkg=8192, maps=True)
    assert set(maps) == {"rgb", "alpha", "depth", "rgb_human", "alpha_human"}
    for k, v in maps.items():
        assert tuple(v.shape) == ((H * W, 3) if k.startswith("rgb") else (H * W,)), k
    assert torch.equal(maps["rgb"], rendered)
    assert float(maps["alpha"].min()) >= 0.0 and float(maps["alpha"].max()) <= 1.0 + 1e-5
    assert bool(torch.isfinite(maps["depth"]).all())
    miss = fr["ray_mask_bkg"]
    assert int(miss.sum()) > 40 and float(maps["alpha_human"][miss].abs().sum()) == 0.0 and float(maps["rgb_human"][miss].abs().sum()) == 0.0
    assert float(maps["alpha_human"].max()) > 0.0                         # the subject is in the frame
    assert bool((maps["alpha_human"] <= maps["alpha"] * (1 + 1e-6) + 1e-7).all())
    # Another chunking (ragged chunks, or a rank's share of the rays) changes the row count of the MLP GEMMs and with it last bits:
    # the project's bound for a re-chunked frame is 1e-6 on unit-scale outputs (tests/test_gpu_eval.py:118), taken over for the
    # unit-scale maps; the depth is a weighted mean of sample positions, which themselves carry ~1e-5 relative fp32 noise of the three
    # resampling levels (tests/test_gpu_stage3.py:97), so it gets 1e-5 + 1e-6 relative to max(1, |depth|).
    def assert_same_frame(other, what):
        for k in maps:
            o = other[k].to(maps[k].device)
            scale = maps[k].abs().clamp_min(1.0) if k == "depth" else torch.ones((), device=maps[k].device)
            err = float(((o - maps[k]).abs() / scale).max())
            print(f"maps frame [{what}] {k}: {err:.3e}")
            assert err <= (1.1e-5 if k == "depth" else 1e-6), (what, k, err)

    assert_same_frame(ev.render_frame(hos_f, fr, chunk_bkg=64, maps=True), "64-ray chunks")
    # two ranks on the one GPU (gloo carries the gather; the rehearsal pattern of tests/test_gpu_dist.py): one bounded child per rank
    env = dict(os.environ)
    env.update(HOS_ROOT=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29561", WORLD_SIZE="2",
               HOS_MAPS_OUT=str(tmp_path / "maps.pt"))
    procs = [subprocess.Popen(["timeout", "-k", "10", "600", sys.executable, "-c", _RANK_WORKER], env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT) for r in range(2)]
    outs = [p.communicate(timeout=700) for p in procs]
    for r, (p, (so, se)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"MAPS_RANK_OK {r}" in so, (r, so[-2000:], se[-4000:])
    assert_same_frame(torch.load(env["HOS_MAPS_OUT"]), "two ranks")


def test_launcher_writes_maps_next_to_the_frames(tmp_path):
    """`run.render_maps = True`: run.run_eval / run.run_render write depth (.npy + preview), opacity and human-layer files next to
    every frame they write; the colour images are the ones written without the binding."""
    from PIL import Image
    from hosnerf_amd.freeview import write_scene_pixels
    scene = str(tmp_path / "scene")
    H = W = 64
    write_scene_pixels(scene, synth.write_scene_dir(scene, 6, H, W, seed=9))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("patch:\n  N_patches: 2\n  size: 16\nfreeview:\n  frame_idx: 3\n")
    logs = str(tmp_path / "logs")
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "--ginc", os.path.join(ROOT, "configs", "hosnerf_backpack.gin"),
           "--ginb", "run.max_steps=1", "--ginb", f'run.datadir="{scene}"', "--ginb", 'run.human_path=""', "--ginb", 'run.bkgd_path=""',
           "--ginb", "run.run_eval=True", "--ginb", "run.run_render=True", "--ginb", "run.render_maps=True", "--logbase", logs,
           "--scene_name", "synthetic", "--scene_dir", scene, "--cfg", str(cfg), "--eval_skip", "100", "--render_frames", "40", "--render_limit", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    logdir = [os.path.join(logs, d) for d in os.listdir(logs)][0]
    for folder, name, colour in ((os.path.join(logdir, "test_vis"), "frame_000000", "frame_000000.png"),
                                 (os.path.join(logdir, "freeview_vis_newtrans", "view_00003"), "image-00000", "image-00000.jpg")):
        assert os.path.exists(os.path.join(folder, colour))
        depth = np.load(os.path.join(folder, name + "_depth.npy"))
        assert depth.shape == (H, W) and depth.dtype == np.float32 and np.isfinite(depth).all()
        assert np.asarray(Image.open(os.path.join(folder, name + "_depth.png"))).shape == (H, W)
        assert np.asarray(Image.open(os.path.join(folder, name + "_alpha.png"))).shape == (H, W)
        assert np.asarray(Image.open(os.path.join(folder, name + "_alpha_human.png"))).shape == (H, W)
        assert np.asarray(Image.open(os.path.join(folder, name + "_human.png"))).shape == (H, W, 4)
    first = np.asarray(Image.open(os.path.join(logdir, "test_vis", "frame_000000.png"))).copy()
    r2 = subprocess.run(cmd + ["--ginb", "run.run_train=False", "--ginb", "run.render_maps=False"],          # later bindings win
                        capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r2.returncode == 0, (r2.stdout[-2000:], r2.stderr[-3000:])
    assert np.array_equal(np.asarray(Image.open(os.path.join(logdir, "test_vis", "frame_000000.png"))), first)
