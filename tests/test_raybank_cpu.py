"""Host side of the stage-1 ray bank (no GPU): the three entries of hos_raybank.hip are declared, mirrored and exported, the 8-bit target
conversion equals the reference's load, the fixture is what its generator says, and the launcher's stage-1 pieces (plumbing run with
--scene_dir, results.json layout, frame dealing)."""
import json
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "stage1_rays.npz"))

ENTRIES = {
    "hos_raybank_index": ["keep", "N", "H", "W", "pix", "cap", "counts", "offsets", "ws", "stream"],
    "hos_raybank_gather": ["cams", "times", "images", "pix", "offsets", "counts", "img_id", "rank", "B", "N", "H", "W", "cap", "rays_o", "rays_d",
                           "viewdirs", "radii", "times_out", "target", "stream"],
    "hos_raybank_frame": ["cam16", "time", "H", "W", "start", "n", "image", "rays_o", "rays_d", "viewdirs", "radii", "times_out", "target", "stream"],
}


def test_entries_are_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "hosrender.h")).read()
    from hosnerf_amd import _lib
    for name, names in ENTRIES.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"include/hosrender.h does not declare {name}"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == names
        proto = _lib.PROTOTYPES[name]
        assert len(proto) == len(params)
        for p, t in zip(params, proto):
            kind = _lib._P if ("*" in p or p.startswith("hos_stream_t")) else {"int": _lib._I, "int64_t": _lib._L, "float": _lib._F}[p.split()[0]]
            assert t is kind, (name, p)
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "hosnerf_amd", "lib", "libhosrender.so")],
                        capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if " T " in l and l.split()[-1].startswith("hos_")}
    declared = set(re.findall(r"\b(hos_[a-z0-9_]+)\s*\(", header)) - {"hos_stream_t"}
    assert set(ENTRIES) <= exported and exported == declared, exported ^ declared
    assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)
    # argument validation happens before any launch, and an empty batch / pixel range launches nothing
    import ctypes
    lib = _lib.load()
    buf = (ctypes.c_float * 16)()
    a = ctypes.addressof(buf)
    assert lib.hos_raybank_index(0, 2, 4, 4, a, 8, a, a, a, 0) == -1                                   # no keep plane
    assert lib.hos_raybank_index(a, 0, 4, 4, a, 8, a, a, a, 0) == -1                                   # no image: nothing to launch over
    assert lib.hos_raybank_index(a, 1, 65536, 65536, a, 8, a, a, a, 0) == -3                           # pixel indices are int32
    assert lib.hos_raybank_gather(*([a] * 8), 0, 2, 4, 4, 8, *([a] * 6), 0) == 0                       # B = 0
    assert lib.hos_raybank_gather(*([a] * 8), -1, 2, 4, 4, 8, *([a] * 6), 0) == -1
    assert lib.hos_raybank_gather(0, *([a] * 7), 3, 2, 4, 4, 8, *([a] * 6), 0) == -1
    assert lib.hos_raybank_frame(a, 0.5, 4, 4, 16, 0, 0, *([a] * 5), 0, 0) == 0                        # n = 0 at the end of the frame
    assert lib.hos_raybank_frame(a, 0.5, 4, 4, 10, 7, 0, *([a] * 5), 0, 0) == -1                       # leaves the frame
    assert lib.hos_raybank_frame(a, 0.5, 4, 4, 0, 4, a, *([a] * 5), 0, 0) == -1                        # pixels without a target
    assert lib.hos_raybank_frame(0, 0.5, 4, 4, 0, 4, 0, *([a] * 5), 0, 0) == -1


def test_target_conversion_is_the_references_load():
    """The kernels report float32(u) / float32(255); the reference holds float32(u / 255.0) (double division, then rounded)."""
    from hosnerf_amd.raybank import to_uint8
    u = np.arange(256)
    assert np.array_equal(u.astype(np.float32) / np.float32(255.0), (u / 255.0).astype(np.float32))
    assert np.array_equal(to_uint8((u / 255.0).astype(np.float32)), u.astype(np.uint8))                 # decoded floats go back to their bytes
    assert to_uint8(u.astype(np.uint8)).dtype == np.uint8
    assert np.array_equal(G["train_target"][:50], (G["images_u8"][0].reshape(-1, 3)[np.flatnonzero((G["masks"][0] < 1).reshape(-1))][:50] / 255.0).astype(np.float32))


def test_fixture_is_what_the_generator_promises():
    masks, counts = G["masks"], G["counts"]
    n, h, w = masks.shape
    assert (n, h, w) == (5, 12, 20) and G["images_u8"].dtype == np.uint8
    assert np.array_equal(counts, (masks < 1).sum(axis=(1, 2)))
    assert len(G["train_rays_o"]) == int(counts[G["i_train"]].sum()) == len(G["train_times"]) == len(G["train_target"])
    assert counts[int(G["zero_image"])] == 0 and int(G["zero_image"]) in G["i_train"] and counts[int(G["full_image"])] == h * w
    assert int(G["frame"]) in G["i_test"] and len(G["frame_rays_o"]) == h * w and len(G["pose_rays_o"]) == len(G["render_poses"]) * h * w
    for i in (0, 2, 4):                                      # irregular masks with kept pixels in the last row and the last column
        keep = masks[i] < 1
        assert 0 < keep.sum() < h * w and keep[h - 1].any() and keep[:, w - 1].any() and keep[h - 1, w - 1]
    K = G["intrinsics"]
    assert (K[:, 0, 0] != K[:, 1, 1]).all() and (np.abs(K[:, 0, 2] - 0.5 * w) > 0.05).all() and (np.abs(K[:, 1, 2] - 0.5 * h) > 0.05).all()
    R = G["extrinsics"][:, :3, :3]
    assert (np.abs(R) < 0.999).all() and len({tuple(np.round(r.reshape(-1), 6)) for r in R}) == n          # distinct, not axis-aligned
    assert np.abs(np.linalg.norm(G["train_rays_d"], axis=-1) - 1).max() < 1e-6                             # rays_d is stored normalised
    assert np.array_equal(G["train_rays_d"], G["train_viewdirs"]) or np.abs(G["train_rays_d"] - G["train_viewdirs"]).max() < 2e-7
    jump = np.concatenate([[0], np.cumsum(counts[G["i_train"]])])
    assert G["sampler_idx"].min() >= 0 and G["sampler_idx"].max() < jump[-1]
    assert all(len(set((np.searchsorted(jump, row, side="right") - 1).tolist())) == 1 for row in G["sampler_idx"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "stage1_rays.npz")) < 400 * 1024


def test_camera_rows_layout():
    from hosnerf_amd.raybank import camera_rows
    rows = camera_rows(G["extrinsics"], G["intrinsics"])
    assert rows.shape == (5, 16) and rows.dtype == np.float32
    assert np.array_equal(rows[2, :12].reshape(3, 4), G["extrinsics"][2, :3, :4].astype(np.float32))
    K = G["intrinsics"][2]
    assert rows[2, 12:].tolist() == [np.float32(K[0, 0]), np.float32(K[1, 1]), np.float32(K[0, 2]), np.float32(K[1, 2])]
    assert camera_rows(G["render_poses"][1], G["intrinsics"][0]).shape == (1, 16)


def test_launcher_plumbing_run_with_scene_dir(tmp_path):
    import inspect
    import run as launcher
    from hosnerf_amd import synth
    scene = str(tmp_path / "scene")
    synth.write_scene_dir(scene, 3, 16, 16, seed=2)
    gin = os.path.join(ROOT, "configs", "state_mipnerf360_backpack.gin")
    plan = launcher.main(["--ginc", gin, "--scene_name", "Backpack", "--logbase", str(tmp_path / "logs"), "--cpu", "--scene_dir", scene,
                          "--ginb", "run.max_steps=3", "--ginb", "run.run_eval=True", "--ginb", "run.run_render=True"])
    assert plan["mode"] == "cpu-plumbing" and plan["model_name"] == "state_mipnerf360" and plan["checkpoint_roundtrip"] == {"missing": 0, "unexpected": 0}
    assert inspect.signature(launcher.evaluate_and_render).parameters["run_tpose"].default is False


def test_results_json_layout(tmp_path):
    from hosnerf_amd import eval as ev
    path = str(tmp_path / "results.json")
    d = ev.write_bkgd_results(path, [20.0, 22.0, 27.0])
    assert d == {"PSNR": {"mean": 23.0, "test": 23.0}}
    text = open(path).read()
    assert json.loads(text) == d and text == json.dumps(d, indent=4, sort_keys=True)          # write_stats, interface.py:121-132
    assert "SSIM" not in text and "LPIPS" not in text


def test_frames_are_dealt_round_robin():
    from hosnerf_amd.raybank import deal_frames
    for n in (0, 1, 2, 5, 6, 7):
        for world in (1, 2, 3):
            shares = [deal_frames(n, r, world) for r in range(world)]
            assert sorted(k for s in shares for k in s) == list(range(n))                     # every frame exactly once
            assert all(s == [k for k in range(n) if k % world == r] for r, s in enumerate(shares))
