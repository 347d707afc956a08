"""The mesh rasteriser on the MI355X (hos_raster.hip: `ops.mesh_project`, `ops.raster_faces`, `ops.raster_resolve`, `ops.frame_fit`;
`mesh.rasterize`, `mesh.fit`, `mesh.level_sweep`) against the numpy restatement tests/_raster_expect.py, and the loop it exists for:
a frame mesh seen through the frame's own camera, scored against the render of that frame.

Accuracy rule (tests/test_gpu_mesh.py): |hip - fp64 restatement| <= 2 * |fp32 restatement - fp64 restatement| + one fp32 ulp of the
largest value, in the maximum norm.  Coverage is integer arithmetic: masks, faces away from depth ties and counts are exact.

Frames: 48 x 40 and 67 x 3 (H x W) -- no multiple of a wave or a block, the second narrower than a block.  The sphere at resolution
12 (1344 triangles) through `sphere_camera`: measured on the CPU with the restatement, 0 of its 317 (48 x 40) and 0 of its 81
(67 x 3) covered pixels have their two nearest candidate depths within 1e-5 relative of each other (the bound is 1 %), and 2
triangles project to zero area and are dropped."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from hosnerf_amd import formats, synth
from tests import _raster_expect as RX
from tests._record import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = [(48, 40), (67, 3)]
FIT_KEYS = ("iou", "area_mesh", "area_ref", "depth_mae", "depth_bias", "depth_rmse", "depth_max")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


@pytest.fixture(scope="module")
def sphere():
    v, f, nrm, col = RX.sphere_mesh(12, np.float32)
    return {"vertices": v.astype(np.float32), "faces": f.astype(np.int32), "normals": nrm, "colors": col}


def hand_mesh(K, R, T):
    """The hand cases of tests/test_raster_cpu.py in one mesh, in the space of camera (K, R, T): a square of two triangles on pixel
    centres at depth 2, a triangle larger than the frame behind it at depth 5, and four triangles that must be dropped (behind the
    camera, beyond the guard band, zero area, an index outside the vertices)."""
    Kinv, Rt = np.linalg.inv(K), R.T

    def at(col, row, z):
        return Rt @ (Kinv @ np.array([col, row, 1.0]) * z - T)

    v = [at(1, 2, 2.0), at(3, 2, 2.0), at(3, 30, 2.0), at(1, 30, 2.0), at(-100, -100, 5.0), at(300, -100, 5.0), at(-100, 300, 5.0),
         at(0, 0, -1.0), at(40000, 3, 2.0), at(0.5, 4, 3.0), at(1.0, 6, 3.0), at(1.5, 8, 3.0)]
    f = [[0, 1, 2], [0, 2, 3], [4, 5, 6], [0, 1, 7], [0, 8, 2], [9, 10, 11], [0, 1, 12]]
    rs = np.random.RandomState(5)
    return {"vertices": np.asarray(v, dtype=np.float32), "faces": np.asarray(f, dtype=np.int32), "normals": None,
            "colors": rs.randint(0, 256, (len(v), 3)).astype(np.uint8)}


def to_dev(m, dev):
    return {k: (None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)) for k, x in m.items()}


def gpu_raster(md, K, R, T, H, W, dev, base=0):
    """project + raster + resolve of one device mesh through `ops` -> (xy, z, zbuf, dropped, outputs), all on the host."""
    from hosnerf_amd import ops
    xy, z = ops.mesh_project(md["vertices"], K, R, T)
    zbuf = torch.full((H * W,), -1, dtype=torch.int64, device=dev)
    dropped = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.raster_faces(xy, z, md["faces"], base, H, W, zbuf, dropped)
    out = new_outputs(H, W, dev)
    ops.raster_resolve(zbuf, xy, z, md["faces"], base, H, W, out, vertices=md["vertices"], colors=md["colors"], normals=md["normals"],
                       Kinv=np.linalg.inv(K), R=R)
    return xy.cpu().numpy(), z.cpu().numpy(), zbuf.cpu().numpy(), int(dropped.item()), {k: t.cpu().numpy() for k, t in out.items()}


def new_outputs(H, W, dev, poison=False):
    n = H * W
    f = (lambda *s: torch.full(s, -7.0, device=dev)) if poison else (lambda *s: torch.empty(*s, device=dev))
    return {"face": torch.full((n,), -7, dtype=torch.int32, device=dev), "depth": f(n), "mask": torch.full((n,), 9, dtype=torch.uint8, device=dev),
            "rgb": f(n, 3), "normal": f(n, 3), "shaded": f(n, 3)}


def assert_rule(got, r32, r64, tag):
    if r64.size == 0:
        return
    ulp = float(np.spacing(np.float32(np.abs(r64).max())))
    e_hip = float(np.abs(got.astype(np.float64) - r64).max())
    e_ref = float(np.abs(r32.astype(np.float64) - r64).max())
    print(f"{tag}: hip {e_hip:.3e}, fp32 restatement {e_ref:.3e}, ulp {ulp:.3e}")
    assert e_hip <= 2.0 * e_ref + ulp, (tag, e_hip, e_ref, ulp)


# ------------------------------------------------------------------------------------------ projection
@pytest.mark.parametrize("H,W", FRAMES)
def test_mesh_project_against_fp64(dev, sphere, H, W):
    from hosnerf_amd import ops
    K, R, T = RX.sphere_camera(H, W)
    hand = hand_mesh(K, R, T)
    v = np.concatenate([sphere["vertices"], hand["vertices"]], 0)
    xy, z = ops.mesh_project(torch.from_numpy(v).to(dev), K, R, T)
    xy, z = xy.cpu().numpy().astype(np.int64), z.cpu().numpy()
    xy64, z64, uv64 = RX.project(v, K, R, T, np.float64)
    xy32, z32, _ = RX.project(v, K, R, T, np.float32)
    assert_rule(z, z32, z64, f"project z {H}x{W}")
    usable = xy64[:, 0] != RX.SENTINEL
    assert np.array_equal(xy[:, 0] == RX.SENTINEL, ~usable) and (~usable).sum() == 2 and (xy[~usable, 1] == 0).all()
    diff = np.abs(xy[usable] - np.rint(256.0 * uv64[usable]))
    assert diff.max() <= 1, diff.max()              # the fp32 projection error is ~1e-4 pixel against a unit of 3.9e-3
    record(f"raster_project_xy_differ_share_{H}x{W}", float((diff != 0).mean()))
    print(f"project {H}x{W}: {float((diff != 0).mean()):.4%} of {diff.size} fixed-point coordinates differ from round(256 u_fp64)")


# ------------------------------------------------------------------------------------------ raster + resolve
def check_against_restatement(md_host, K, R, T, H, W, dev, tag, max_ambiguous):
    md = to_dev(md_host, dev)
    xy, z, zbuf, dropped, got = gpu_raster(md, K, R, T, H, W, dev)
    faces = md_host["faces"]
    c64 = RX.candidates(xy, z, faces, H, W, np.float64)
    c32 = RX.candidates(xy, z, faces, H, W, np.float32)
    assert dropped == c64["dropped"]
    w64, w32 = RX.zbuffer(c64, H * W), RX.zbuffer(c32, H * W)
    kw = dict(vertices=md_host["vertices"], faces=faces, colors=md_host["colors"], normals=md_host["normals"], Kinv=np.linalg.inv(K), R=R)
    r64, r32 = RX.resolve(c64, w64, H, W, np.float64, **kw), RX.resolve(c32, w32, H, W, np.float32, **kw)
    # coverage: integer arithmetic, exact
    assert np.array_equal(got["mask"], r64["mask"]) and np.array_equal(got["face"] >= 0, r64["mask"] != 0)
    assert np.array_equal(zbuf == -1, r64["mask"] == 0)
    covered = np.nonzero(r64["mask"])[0]
    # the class of pixels whose two nearest candidates are within 1e-5 relative in fp64
    order = np.lexsort((c64["face"], c64["depth"], c64["pix"]))
    p, d, fid = c64["pix"][order], c64["depth"][order], c64["face"][order]
    ambiguous = np.zeros(H * W, dtype=bool)
    for i in np.nonzero((p[1:] == p[:-1]))[0]:                       # consecutive candidates of one pixel, ascending depth
        lo = np.searchsorted(p, p[i])
        if (d[i + 1] - d[lo]) <= 1e-5 * d[lo]:
            ambiguous[p[i]] = True
    share = float(ambiguous[covered].mean()) if covered.size else 0.0
    print(f"{tag}: {covered.size} covered pixels, {int(ambiguous.sum())} with near-tied depths ({share:.3%}), dropped {dropped}")
    assert share <= max_ambiguous
    clear = (r64["mask"] != 0) & ~ambiguous
    assert np.array_equal(got["face"][clear], r64["face"][clear])
    for px in np.nonzero(ambiguous)[0]:                              # the winner must be one of the near-tied candidates
        sel = p == px
        near = fid[sel][d[sel] - d[sel].min() <= 1e-5 * d[sel].min()]
        assert got["face"][px] in near
    assert np.array_equal(got["face"][r64["mask"] == 0], np.full(int((r64["mask"] == 0).sum()), -1))
    agreed = (r64["mask"] != 0) & (got["face"] == r64["face"]) & (r32["face"] == r64["face"])
    assert agreed.sum() >= 0.99 * covered.size
    empty = r64["mask"] == 0
    for k in ("depth", "rgb", "normal", "shaded"):
        assert np.isfinite(got[k]).all(), k
        assert_rule(got[k][agreed], r32[k][agreed], r64[k][agreed], f"{tag} {k}")
        assert np.array_equal(got[k][empty], r32[k][empty]), k      # 0, the background colour
    length = np.linalg.norm(got["normal"][agreed].astype(np.float64), axis=1)
    assert ((np.abs(length - 1.0) < 1e-5) | (length == 0)).all()
    return got, r64


@pytest.mark.parametrize("H,W", FRAMES)
def test_sphere_raster_and_resolve(dev, sphere, H, W):
    K, R, T = RX.sphere_camera(H, W)
    got, r64 = check_against_restatement(sphere, K, R, T, H, W, dev, f"sphere {H}x{W}", 0.01)
    assert (r64["mask"] != 0).sum() > 50
    geo = dict(sphere, normals=None, colors=None)                    # absent colours: white; absent normals: the faces' own
    got, _ = check_against_restatement(geo, K, R, T, H, W, dev, f"sphere, no attributes {H}x{W}", 0.01)
    assert (got["rgb"] == 1.0).all()


@pytest.mark.parametrize("H,W", FRAMES)
def test_hand_cases(dev, H, W):
    K, R, T = RX.sphere_camera(H, W)
    got, r64 = check_against_restatement(hand_mesh(K, R, T), K, R, T, H, W, dev, f"hand cases {H}x{W}", 0.0)
    face = got["face"].reshape(H, W)
    assert (face >= 0).all() and (got["mask"] == 1).all()             # the triangle larger than the frame covers all H*W pixels
    square = np.zeros((H, W), dtype=bool)
    square[2:30, 1:3] = True                                          # [1,3) x [2,30): the square in front, one of its two triangles each
    assert (face[~square] == 2).all() and np.isin(face[square], (0, 1)).all()
    assert (got["depth"].reshape(H, W)[square] < 2.001).all() and (got["depth"].reshape(H, W)[~square] > 4.999).all()


def test_coincident_triangles_and_empty_meshes(dev):
    from hosnerf_amd import mesh, ops
    H, W = 48, 40
    K, R, T = RX.sphere_camera(H, W)
    hm = hand_mesh(K, R, T)
    v = torch.from_numpy(hm["vertices"]).to(dev)
    faces = torch.tensor([[4, 5, 6], [4, 5, 6], [4, 6, 5]], dtype=torch.int32, device=dev)
    for f in (faces, faces.flip(0).contiguous()):
        r = mesh.rasterize({"vertices": v, "faces": f}, K, np.concatenate([R, T[:, None]], 1), H, W, want=("face", "mask"))
        assert r["dropped"] == 0 and (r["face"] == 0).all() and (r["mask"] == 1).all()          # equal depths: the lowest id
    # V = 0 / F = 0: legal, nothing is launched, the frame is empty
    none = {"vertices": torch.zeros(0, 3, device=dev), "faces": torch.zeros(0, 3, dtype=torch.int32, device=dev)}
    for meshes in ([], none, [none, {"vertices": v, "faces": none["faces"]}]):
        r = mesh.rasterize(meshes, K, np.concatenate([R, T[:, None]], 1), H, W, bgcolor=(255.0, 0.0, 51.0))
        assert r["dropped"] == 0 and (r["face"] == -1).all() and (r["mask"] == 0).all() and (r["depth"] == 0).all() and (r["normal"] == 0).all()
        bg = torch.tensor([1.0, 0.0, 0.2], device=dev)
        assert torch.equal(r["rgb"], bg.expand(H * W, 3)) and torch.equal(r["shaded"], bg.expand(H * W, 3))
    xy, z = ops.mesh_project(none["vertices"], K, R, T)
    assert xy.shape == (0, 2) and z.shape == (0,)
    with pytest.raises(ValueError):
        mesh.rasterize(none, np.array([[50.0, 0, 20], [0, 50.0, 24], [0, 1e-3, 1]]), np.eye(4), H, W)


# ------------------------------------------------------------------------------------------ determinism and composition
def test_determinism_and_composition(dev, sphere):
    from hosnerf_amd import ops
    H, W = 48, 40
    K, R, T = RX.sphere_camera(H, W)
    A = to_dev(sphere, dev)
    shifted = dict(sphere, vertices=(sphere["vertices"] + np.float32([0.11, -0.07, 0.05])), colors=255 - sphere["colors"])
    B = to_dev(shifted, dev)                                           # a second sphere that cuts through the first
    FA, VA = A["faces"].shape[0], A["vertices"].shape[0]
    both = {"vertices": torch.cat([A["vertices"], B["vertices"]]), "faces": torch.cat([A["faces"], B["faces"] + VA]),
            "colors": torch.cat([A["colors"], B["colors"]]), "normals": torch.cat([A["normals"], B["normals"]])}
    Kinv = np.linalg.inv(K)

    def run(jobs, poison_between=False):
        zbuf = torch.full((H * W,), -1, dtype=torch.int64, device=dev)
        dropped = torch.zeros(1, dtype=torch.int32, device=dev)
        proj = []
        for m, base in jobs:
            xy, z = ops.mesh_project(m["vertices"], K, R, T)
            ops.raster_faces(xy, z, m["faces"], base, H, W, zbuf, dropped)
            proj.append((xy, z))
        out = new_outputs(H, W, dev, poison=True)
        stages = []
        for (m, base), (xy, z) in zip(jobs, proj):
            ops.raster_resolve(zbuf, xy, z, m["faces"], base, H, W, out, vertices=m["vertices"], colors=m["colors"], normals=m["normals"], Kinv=Kinv, R=R)
            stages.append({k: t.clone() for k, t in out.items()})
        return zbuf, int(dropped.item()), out, stages

    one = run([(both, 0)])
    again = run([(both, 0)])
    ab = run([(A, 0), (B, FA)])
    ba = run([(B, FA), (A, 0)])
    for other in (again, ab, ba):
        assert torch.equal(one[0], other[0]) and one[1] == other[1]
        for k in one[2]:
            assert torch.equal(one[2][k], other[2][k]), k
    ids = one[2]["face"]
    won_a, won_b = (ids >= 0) & (ids < FA), ids >= FA
    assert won_a.sum() > 20 and won_b.sum() > 20                        # both spheres are seen
    first = ab[3][0]                                                    # after resolving A alone: B's pixels still hold the poison
    assert (first["face"][won_b] == -7).all() and (first["depth"][won_b] == -7.0).all() and (first["mask"][won_b] == 9).all()
    for k in ("rgb", "normal", "shaded"):
        assert (first[k][won_b] == -7.0).all(), k
    assert torch.equal(first["face"][~won_b], ids[~won_b])
    first = ba[3][0]
    assert (first["face"][won_a] == -7).all() and torch.equal(first["face"][~won_a], ids[~won_a])


# ------------------------------------------------------------------------------------------ fit
def test_frame_fit_against_fp64(dev, sphere):
    from hosnerf_amd import mesh, ops
    H, W = 48, 40
    K, R, T = RX.sphere_camera(H, W)
    r = mesh.rasterize(to_dev(sphere, dev), K, np.concatenate([R, T[:, None]], 1), H, W, want=("depth", "mask"))
    mask, depth = r["mask"], r["depth"]
    rs = np.random.RandomState(3)
    alpha_b = torch.roll(mask.view(H, W), (3, -2), (0, 1)).float() * torch.from_numpy(rs.uniform(0.3, 1.0, (H, W)).astype(np.float32)).to(dev)
    depth_b = torch.roll(depth.view(H, W), (3, -2), (0, 1)) * 1.01 + 0.003
    alpha_b, depth_b = alpha_b.reshape(-1).contiguous(), depth_b.reshape(-1).contiguous()
    out = ops.frame_fit(mask, depth, alpha_b, depth_b, 0.5)
    assert torch.equal(out, ops.frame_fit(mask, depth, alpha_b, depth_b, 0.5))              # bit-equal
    counts, sums = RX.fit(mask.cpu().numpy(), depth.cpu().numpy(), alpha_b.cpu().numpy(), depth_b.cpu().numpy(), 0.5)
    host = out.cpu()
    assert host[:3].tolist() == counts and counts[2] > 50
    got = host[3:].view(torch.float64).tolist()
    for g, w in zip(got, sums):
        assert abs(g - w) <= 1e-6 * abs(w), (got, sums)
    fig = mesh.fit(r, alpha_b, depth_b, tau=0.5, spacing=0.25)
    want = RX.fit_figures(counts, sums)
    assert tuple(k for k in fig if not k.endswith("_vox")) == FIT_KEYS
    for k in FIT_KEYS:
        assert abs(fig[k] - want[k]) <= 1e-6 * abs(want[k]), k
    assert abs(fig["depth_mae_vox"] - want["depth_mae"] / 0.25) <= 1e-6 * want["depth_mae"] / 0.25
    sil = mesh.fit(r, alpha_b.view(H, W).cpu())                                            # the silhouette alone, a host mask
    assert sil == {k: fig[k] for k in ("iou", "area_mesh", "area_ref")}
    none = ops.frame_fit(mask, None, alpha_b, None, 0.5).cpu()
    assert none[:3].tolist() == counts and none[3:].tolist() == [0, 0, 0, 0]
    empty = ops.frame_fit(mask[:0], depth[:0], alpha_b[:0], depth_b[:0], 0.5).cpu()
    assert empty.tolist() == [0] * 7
    big = 300 * 1024 + 7                                                                    # more pixels than one pass of the blocks covers
    m2, a2 = (torch.arange(big, device=dev) % 3 == 0).to(torch.uint8), (torch.arange(big, device=dev) % 5).float() / 4.0
    d2 = torch.arange(big, device=dev).float() / big
    o2 = ops.frame_fit(m2, d2, a2, d2 * 0.5, 0.5).cpu()
    c2, s2 = RX.fit(m2.cpu().numpy(), d2.cpu().numpy(), a2.cpu().numpy(), (d2 * 0.5).cpu().numpy(), 0.5)
    assert o2[:3].tolist() == c2 and all(abs(g - w) <= 1e-6 * abs(w) for g, w in zip(o2[3:].view(torch.float64).tolist(), s2))


# ------------------------------------------------------------------------------------------ the loop this exists for
def basedir():
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    return d


@pytest.mark.parametrize("stage", [2, 3])
def test_frame_mesh_against_its_own_render(dev, tmp_path, stage):
    """Random weights: the field is noise, so the IoU and the depth figures are recorded, not bounded; what must hold for ANY field
    is asserted -- the mesh lies in the frame's box, so it is seen only through pixels whose ray hits the box, at a depth between
    the ray's entry and exit (grown by the voxel the mesh may stand out of the box by)."""
    from hosnerf_amd import eval as ev, mesh
    from hosnerf_amd.dataset import SceneItems
    from hosnerf_amd.human_nerf import Network, default_cfg
    scene = str(tmp_path / "scene")
    px = synth.write_scene_dir(scene, 6, 64, 64, seed=9)
    formats.load_scene(scene, (64, 64), masks=px["alphas"], near=0.1, far=1e6)
    ds = SceneItems(scene, px["images"], px["alphas"], px["flows"], n_patches=2, patch_size=8, device=dev, seed=5, stage=stage)
    net = Network(default_cfg(basedir()), stage=stage)
    net.load_state_dict(synth.human_state_dict(777, 2), strict=True)
    net = net.to(dev)
    idx = 3
    cam = ds.frame_camera(idx)
    assert cam["H"] == cam["W"] == 64 and cam["K"].dtype == np.float64 and cam["E"].shape == (4, 4) and set(cam) == {"K", "E", "E_colmap", "H", "W"}
    m = mesh.extract_frame(net, ds.frame_pose(idx), resolution=16, level=0.001, space="body", normals=True, keep_body=True)
    assert m["body"]["vertices"] is m["vertices"] and m["vertices"].shape[0] > 0
    r = mesh.rasterize(m, cam["K"], cam["E"], cam["H"], cam["W"])
    fr = ds.human_frame(idx, (255.0, 255.0, 255.0))
    assert net.stage == stage
    render = ev.render_human_frame(net, fr, maps=True, median=True)
    assert net.stage == stage and set(render) == {"rgb", "alpha", "depth", "depth_median"}
    covered = r["mask"] != 0
    slot = fr["slot"].long()
    h = m["spacing"]
    assert covered.sum() > 0
    outside = int((covered & (slot < 0)).sum())
    print(f"stage {stage}: {int(covered.sum())} covered pixels, {outside} outside the box's ray mask, V {m['vertices'].shape[0]} F {m['faces'].shape[0]}, "
          f"dropped {r['dropped']} (zero screen area)")
    assert outside == 0
    near, far = fr["near"].reshape(-1)[slot[covered]], fr["far"].reshape(-1)[slot[covered]]
    d = r["depth"][covered]
    assert (d >= near - h).all() and (d <= far + h).all(), (float((near - d).max()), float((d - far).max()), h)
    fig = mesh.fit(r, render["alpha"], render["depth_median"], spacing=h)
    sil = mesh.fit(r, ds.alphas[idx])
    assert all(np.isfinite(x) for x in fig.values()) and all(np.isfinite(x) for x in sil.values()) and set(sil) == {"iou", "area_mesh", "area_ref"}
    rows = mesh.level_sweep(m, (0.0005, 0.001, 0.01), cam, render)
    assert [row["level"] for row in rows] == [0.0005, 0.001, 0.01] and rows[1]["V"] == m["vertices"].shape[0]
    assert {k: rows[1][k] for k in fig} == fig                           # the same field at the same level: the same figures
    record(f"raster_untrained_fit_stage{stage}", {"render": fig, "mask": sil})
    print(f"stage {stage} (untrained, information only): fit vs render {fig}; vs subject mask {sil}")


# ------------------------------------------------------------------------------------------ the launcher
@pytest.mark.parametrize("gin,model", [("hosnerf_backpack.gin", "hosnerf"), ("state_humanobject_backpack.gin", "state_humanobject")])
def test_launcher_mesh_preview(tmp_path, gin, model):
    from hosnerf_amd.freeview import MESH_MAP_FILES, write_scene_pixels
    from PIL import Image
    scene = str(tmp_path / "scene")
    write_scene_pixels(scene, synth.write_scene_dir(scene, 6, 64, 64, seed=9))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("patch:\n  N_patches: 2\n  size: 16\n")

    def launch(logs, *extra, ckpt=None):
        cmd = [sys.executable, os.path.join(ROOT, "run.py"), "--ginc", os.path.join(ROOT, "configs", gin), "--ginb", "run.max_steps=2",
               "--ginb", f'run.datadir="{scene}"', "--ginb", "run.run_mesh_frames=True", "--ginb", "run.mesh_resolution=16", "--ginb", "run.mesh_level=0.001",
               "--scene_name", "synthetic", "--scene_dir", scene, "--cfg", str(cfg), "--logbase", logs, "--eval_skip", "3"]
        if model == "hosnerf":
            cmd += ["--ginb", 'run.human_path=""', "--ginb", 'run.bkgd_path=""']
        for b in extra:
            cmd += ["--ginb", b]
        if ckpt is not None:
            cmd += ["--ckpt_path", ckpt]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
        return os.path.join([os.path.join(logs, d) for d in os.listdir(logs)][0], "mesh_frames")

    # Two training runs do not end on the same weights bit for bit, so the run with the switch does not train: it meshes the
    # checkpoint the run without the switch left (`--ckpt_path`, `run.run_train=False`) into a log directory of its own.
    plain = launch(str(tmp_path / "plain"))
    ckpt = os.path.join(os.path.dirname(plain), "last.ckpt")
    assert os.path.exists(ckpt)
    prev = launch(str(tmp_path / "preview"), "run.run_train=False", "run.mesh_preview=True", "run.mesh_level_sweep=(0.001, 0.01)", ckpt=ckpt)
    assert prev != plain
    meta0, meta = json.load(open(os.path.join(plain, "meshes.json"))), json.load(open(os.path.join(prev, "meshes.json")))
    frames = sorted(meta0)
    assert len(frames) == 2 and sorted(meta) == frames
    assert sorted(os.listdir(plain)) == sorted(["meshes.json"] + [n + ".ply" for n in frames])                 # without the switch: nothing new
    assert sorted(os.listdir(prev)) == sorted(["meshes.json"] + [n + ".ply" for n in frames] + [n + k for n in frames for k in MESH_MAP_FILES])
    for name in frames:
        assert open(os.path.join(plain, name + ".ply"), "rb").read() == open(os.path.join(prev, name + ".ply"), "rb").read()
        row = dict(meta[name])
        fit, sweep = row.pop("fit"), row.pop("sweep")
        assert row == meta0[name] and "fit" not in meta0[name] and "sweep" not in meta0[name]
        assert set(fit) == {"render", "mask"} and set(fit["render"]) >= set(FIT_KEYS) and set(fit["mask"]) == {"iou", "area_mesh", "area_ref"}
        assert all(np.isfinite(x) for x in fit["render"].values()) and fit["render"]["area_mesh"] > 0
        assert [s["level"] for s in sweep] == [0.001, 0.01] and all(set(s) >= set(FIT_KEYS) for s in sweep)
        for k in MESH_MAP_FILES:
            p = os.path.join(prev, name + k)
            assert (np.load(p).shape == (64, 64)) if k.endswith(".npy") else (Image.open(p).size == (64, 64)), k
        print(f"{model} {name}: fit {fit}")
