"""The canonical mesh on the GPU: `ops.march_tets` against the numpy restatement of its rules (tests/_mesh_expect.py, whose own
properties tests/test_mesh_cpu.py checks), `ops.grid_points` / `ops.grid_alpha` against `human_sample_warp` and the oracle,
`mesh.extract` on stage-2 and stage-3 networks, and the launcher's `run.run_mesh`.

Vertex accuracy rule (the rule of tests/test_gpu_maps.py): |hip - fp64 restatement| <= 2 * |fp32 restatement - fp64 restatement| + one
fp32 ulp of the largest coordinate, in the maximum norm; faces, V and F are exact."""
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
from tests import _mesh_expect as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def hip_march(field, level, origin, h, dev, rgb=None):
    from hosnerf_amd import ops
    f = torch.from_numpy(np.ascontiguousarray(field, dtype=np.float32)).to(dev)
    c = None if rgb is None else torch.from_numpy(np.ascontiguousarray(rgb, dtype=np.float32)).to(dev)
    v, col, faces = ops.march_tets(f, level, origin, h, rgb=c)
    assert v.dtype == torch.float32 and faces.dtype == torch.int32 and v.shape[1:] == (3,) and faces.shape[1:] == (3,)
    assert (col is None) == (rgb is None) and (col is None or col.shape == v.shape)
    return v.cpu().numpy(), None if col is None else col.cpu().numpy(), faces.cpu().numpy()


def assert_equals_restatement(field, level, origin, h, got, rgb=None, tag=""):
    field = np.ascontiguousarray(field, dtype=np.float32)
    v64, c64, f = X.march(field, level, origin, h, rgb=rgb, dtype=np.float64)
    v32, c32, _ = X.march(field, level, origin, h, rgb=rgb, dtype=np.float32)
    gv, gc, gf = got
    assert gv.shape == v64.shape and gf.shape == f.shape, (tag, gv.shape, v64.shape, gf.shape, f.shape)
    assert np.array_equal(gf, f), tag
    if v64.shape[0] == 0:
        return 0, 0
    assert np.isfinite(gv).all(), tag
    pairs = [(gv, v32, v64, float(np.spacing(np.float32(np.abs(v64).max()))))]
    if rgb is not None:
        assert np.isfinite(gc).all(), tag
        pairs.append((gc, c32, c64, float(np.spacing(np.float32(np.abs(c64).max())))))
    for g, r32, r64, ulp in pairs:
        e_hip = float(np.abs(g.astype(np.float64) - r64).max())
        e_ref = float(np.abs(r32.astype(np.float64) - r64).max())
        assert e_hip <= 2.0 * e_ref + ulp, (tag, e_hip, e_ref, ulp)
    return v64.shape[0], f.shape[0]


def sink_rim(f, value):
    f[0] = f[-1] = value
    f[:, 0] = f[:, -1] = value
    f[:, :, 0] = f[:, :, -1] = value
    return f


def smooth_field(dims, seed):
    """A few blobs plus noise on a grid of dims (Nx,Ny,Nz), its outermost layer below the level 0."""
    Nx, Ny, Nz = dims
    rs = np.random.RandomState(seed)
    z, y, x = np.meshgrid(np.arange(Nz), np.arange(Ny), np.arange(Nx), indexing="ij")
    f = np.full((Nz, Ny, Nx), -0.3)
    for _ in range(6):
        c = rs.uniform(0.2, 0.8, 3) * (Nx, Ny, Nz)
        r = rs.uniform(0.1, 0.3) * min(dims)
        f = np.maximum(f, 1.0 - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / r)
    f = f + 0.2 * rs.randn(Nz, Ny, Nx)
    return sink_rim(f.astype(np.float32), -1.0)


# ------------------------------------------------------------------------------------------ march_tets
def test_one_cell_all_256_patterns(dev):
    """A 2x2x2 grid, every inside/outside pattern of its 8 corners, random magnitudes: V, F and the faces equal the restatement."""
    rs = np.random.RandomState(0)
    origin, h = (0.25, -0.5, 1.0), 0.375
    total = 0
    for pattern in range(256):
        bits = np.array([(pattern >> cb) & 1 for cb in range(8)], dtype=bool).reshape(2, 2, 2)        # [dz,dy,dx] = bit dx + 2dy + 4dz
        f = np.where(bits, 0.5 + rs.uniform(0.05, 1.0, (2, 2, 2)), 0.5 - rs.uniform(0.05, 1.0, (2, 2, 2))).astype(np.float32)
        got = hip_march(f, 0.5, origin, h, dev)
        V, F = assert_equals_restatement(f, 0.5, origin, h, got, tag=f"pattern {pattern}")
        assert (V == 0) == (pattern in (0, 255)) and (F == 0) == (V == 0)
        total += F
    assert total > 0


@pytest.mark.parametrize("seed", range(20))
def test_random_fields_7x5x4(dev, seed):
    """Distinct dimensions (a transposed index shows), the outer layer below the level: the restatement exactly, a closed oriented manifold."""
    rs = np.random.RandomState(100 + seed)
    f = sink_rim(rs.randn(4, 5, 7).astype(np.float32), -1.0)
    rgb = rs.uniform(0, 1, (4, 5, 7, 3)).astype(np.float32)
    origin, h = (-0.3, 0.1, 0.7), 0.05
    got = hip_march(f, 0.0, origin, h, dev, rgb=rgb)
    V, F = assert_equals_restatement(f, 0.0, origin, h, got, rgb=rgb, tag=f"seed {seed}")
    assert V > 0 and X.is_closed_oriented_manifold(got[2], V) and X.signed_volume(got[0], got[2]) > 0


@pytest.mark.parametrize("dims", [(67, 33, 19), (65, 65, 65), (16, 8, 8)])
def test_block_and_scan_boundaries(dev, dims):
    """Many blocks with a ragged last one; a cubic grid with more blocks than ONE pass of the scan workgroup covers (MT_SCAN); a
    vertex count that is an exact multiple of the block size (MT_BLOCK)."""
    from hosnerf_amd import ops
    N = dims[0] * dims[1] * dims[2]
    nblk = (N + ops.MT_BLOCK - 1) // ops.MT_BLOCK
    if dims == (65, 65, 65):
        assert nblk > ops.MT_SCAN
    if dims == (16, 8, 8):
        assert N % ops.MT_BLOCK == 0
    if dims == (67, 33, 19):
        assert N % ops.MT_BLOCK != 0 and nblk > 64
    f = smooth_field(dims, 5)
    origin, h = (0.0, -1.0, 0.5), 1.0 / 64
    got = hip_march(f, 0.0, origin, h, dev)
    V, F = assert_equals_restatement(f, 0.0, origin, h, got, tag=str(dims))
    assert V > (ops.MT_SCAN if dims == (65, 65, 65) else 0) and X.is_closed_oriented_manifold(got[2], V)


def test_edge_cases(dev):
    origin, h = (0.0, 0.0, 0.0), 0.1
    for value in (-1.0, 2.0):                                    # all below, all above: empty outputs
        v, c, f = hip_march(np.full((4, 5, 6), value, np.float32), 0.5, origin, h, dev, rgb=np.zeros((4, 5, 6, 3), np.float32))
        assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3)
    # NaN and +-inf entries: finite outputs, NaN counts as outside
    rs = np.random.RandomState(7)
    f = sink_rim(rs.randn(6, 6, 6).astype(np.float32), -1.0)
    f[2, 2, 2], f[2, 3, 2], f[3, 3, 3], f[1, 4, 2], f[4, 1, 1] = np.nan, np.inf, -np.inf, np.nan, 3e38
    f[4, 2, 1] = -3e38
    got = hip_march(f, 0.0, origin, h, dev)
    assert np.isfinite(got[0]).all() and len(got[0]) > 0
    want = X.march(f, 0.0, origin, h, dtype=np.float32)
    assert np.array_equal(got[2], want[2]) and got[0].shape == want[0].shape
    as_outside = np.where(np.isnan(f), -1.0, f).astype(np.float32)
    assert np.array_equal(got[2], X.march(as_outside, 0.0, origin, h)[2])
    assert X.is_closed_oriented_manifold(got[2], len(got[0]))
    assert np.allclose(got[0], want[0], rtol=0.0, atol=1e-6)                                # the fp32 restatement: t = 0.5 at the non-finite ends
    # an integer-valued field that hits the level exactly
    g = sink_rim(rs.randint(0, 3, (6, 7, 8)).astype(np.float32), 0.0)
    got = hip_march(g, 1.0, origin, h, dev)
    V, F = assert_equals_restatement(g, 1.0, origin, h, got, tag="level")
    assert V > 0 and np.isfinite(got[0]).all() and X.is_closed_oriented_manifold(got[2], V)


def test_determinism(dev):
    from hosnerf_amd import ops
    f = torch.from_numpy(smooth_field((40, 37, 29), 11)).to(dev)
    rgb = torch.rand(29, 37, 40, 3, device=dev)
    for colors in (None, rgb):
        a = ops.march_tets(f, 0.0, (0.0, 0.0, 0.0), 0.02, rgb=colors)
        b = ops.march_tets(f, 0.0, (0.0, 0.0, 0.0), 0.02, rgb=colors)
        assert a[0].shape[0] > 0 and torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
        assert (a[1] is None and b[1] is None) if colors is None else torch.equal(a[1], b[1])
    with_c, without = ops.march_tets(f, 0.0, (0.0, 0.0, 0.0), 0.02, rgb=rgb), ops.march_tets(f, 0.0, (0.0, 0.0, 0.0), 0.02)
    assert torch.equal(with_c[0], without[0]) and torch.equal(with_c[2], without[2])


# ------------------------------------------------------------------------------------------ the field
def basedir():
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    return d


@pytest.fixture(scope="module")
def nets(dev):
    """Stage-2 and stage-3 networks on the weights of tests/test_gpu_human.py, and the T-pose constants."""
    from hosnerf_amd.human_nerf import Network, default_cfg
    out = {}
    for stage in (2, 3):
        net = Network(default_cfg(basedir()), stage=stage)
        net.load_state_dict(synth.human_state_dict(777, 2), strict=True)
        out[stage] = net.to(dev)
    joints = synth.tpose_joints()
    bbox = formats.skeleton_bbox(joints, float(out[3].cfg.bbox_offset))
    return out, tpose.TposeTurn(joints, bbox, 32, dev)


def test_grid_points(dev):
    from hosnerf_amd import ops
    origin, h, dims = np.array([-0.7, 0.3, 1.1], np.float32), np.float32(0.013), (9, 7, 5)
    pts = ops.grid_points(origin, h, dims, 0, 9 * 7 * 5, device=dev).cpu().numpy().reshape(5, 7, 9, 3)
    for a, n in enumerate(dims):
        want = origin[a] + np.arange(n, dtype=np.float32) * h                # fp32, operation by operation
        got = np.moveaxis(pts[..., a], 2 - a, -1)
        assert np.array_equal(got, np.broadcast_to(want, got.shape))
    part = ops.grid_points(origin, h, dims, 100, 57, device=dev).cpu().numpy()
    assert np.array_equal(part, pts.reshape(-1, 3)[100:157]) and ops.grid_points(origin, h, dims, 315, 0, device=dev).shape == (0, 3)


def test_grid_alpha_mask_and_formula(dev, nets):
    from hosnerf_amd import mesh, ops
    from hosnerf_amd.eval import evaluating
    networks, turn = nets
    net, const = networks[3], turn.const
    bmin, bscale = const["cnl_bbox_min_xyz"], const["cnl_bbox_scale_xyz"]
    grid = mesh.grid_of_box(bmin.cpu().numpy(), const["cnl_bbox_max_xyz"].cpu().numpy(), 12)
    origin, h, dims = grid["origin"], grid["spacing"], grid["dims"]
    Nx, Ny, Nz = dims
    N = Nx * Ny * Nz
    K = net.cfg.total_bones
    with evaluating(net):
        vol = net._motion_weight_volume(const["motion_weights_priors"]).contiguous()
        pts = ops.grid_points(origin, h, dims, 0, N, device=dev)
        raw, _ = net._canonical_fwd(pts, 1, save=False)
    inner = np.zeros((Nz, Ny, Nx), dtype=bool)
    inner[1:-1, 1:-1, 1:-1] = True
    # mask: sigma = +inf makes alpha = mask * 1; bit-equal to the warp kernel's mask under identity transforms (rays of zero length)
    opaque = raw.clone()
    opaque[:, 3] = float("inf")
    alpha = torch.full((Nz, Ny, Nx), -7.0, device=dev)
    ops.grid_alpha(opaque, vol, bmin, bscale, origin, h, dims, 0, alpha, None, K=K)
    eye, zero = torch.eye(3, device=dev).expand(K, 3, 3).contiguous(), torch.zeros(K, 3, device=dev)
    zeros = torch.zeros(N, device=dev)
    _, wpts, _, wmask = ops.human_sample_warp(pts, torch.zeros_like(pts), zeros, zeros, 1, eye, zero, vol, bmin, bscale, K=K)
    assert torch.equal(wpts.reshape(N, 3), pts)
    a = alpha.cpu().numpy()
    assert np.array_equal(a[inner], wmask.cpu().numpy().reshape(Nz, Ny, Nx)[inner])
    assert float(wmask.max()) > 0.5 and (a[~inner] == 0.0).all() and not np.signbit(a[~inner]).any()      # the boundary layer is exactly 0
    # alpha against the oracle's canonical MLP and trilinear tap, 5e-5 (the bound of tests/test_gpu_human.py on raw)
    rgb = torch.full((Nz, Ny, Nx, 3), -7.0, device=dev)
    ops.grid_alpha(raw, vol, bmin, bscale, origin, h, dims, 0, alpha, rgb, K=K)
    assert torch.equal(rgb.reshape(N, 3), raw[:, :3])
    sd = synth.human_state_dict(777, 2)
    p = pts.cpu()
    with torch.no_grad():
        emb = torch.cat([oh.fourier_embed(p, 10), sd["human_stateembeds.1"].repeat(N, 1)], -1)
        raw_o = oh.canonical_mlp(sd, emb)
        vol_o = oh.motion_weight_volume(sd, const["motion_weights_priors"].cpu())
        mask_o = oh.trilinear_sample(vol_o[:K], (p - bmin.cpu()[None]) * bscale.cpu()[None] - 1.0).sum(-1)
        alpha_o = mask_o * (1.0 - torch.exp(-torch.relu(raw_o[:, 3]) * float(h)))
    err = float((alpha.cpu().reshape(-1) - alpha_o)[torch.from_numpy(inner.reshape(-1))].abs().max())
    print(f"grid_alpha vs oracle: {err:.3e}, max alpha {float(alpha.max()):.3f}")
    assert err < 5e-5 and float(alpha.max()) > 0.0
    assert (alpha.cpu().numpy()[~inner] == 0.0).all()
    # a vertex range writes its own part of the whole-grid arrays and nothing else
    part = torch.full((Nz, Ny, Nx), -7.0, device=dev)
    ops.grid_alpha(raw[300:500].contiguous(), vol, bmin, bscale, origin, h, dims, 300, part, None, K=K)
    flat = part.reshape(-1)
    assert torch.equal(flat[300:500], alpha.reshape(-1)[300:500]) and bool((flat[:300] == -7.0).all()) and bool((flat[500:] == -7.0).all())


def test_canonical_field_chunks(dev, nets):
    """Several chunks (the last one moved back to keep its rows) give the field of one chunk, up to the two kernel routes of the
    canonical MLP, each within 5e-5 of the oracle (tests/test_gpu_human.py)."""
    from hosnerf_amd import mesh
    networks, turn = nets
    one = mesh.canonical_field(networks[3], turn.const, 0.7, resolution=48)
    N = one["alpha"].numel()
    assert N > 2 * 16384 and N % 16384 != 0
    many = mesh.canonical_field(networks[3], turn.const, 0.7, resolution=48, chunk=16384)
    assert one["dims"] == many["dims"] and one["state"] == many["state"] == 1
    assert float((one["alpha"] - many["alpha"]).abs().max()) <= 1e-4 and float((one["rgb"] - many["rgb"]).abs().max()) <= 1e-4
    with pytest.raises(ValueError):
        mesh.canonical_field(networks[3], turn.const, 0.7, resolution=48, chunk=1000)


@pytest.mark.parametrize("stage", [2, 3])
def test_extract(dev, nets, stage, tmp_path):
    from hosnerf_amd import mesh
    networks, turn = nets
    net = networks[stage]
    fields = []
    for t, state in ((0.2, 0), (0.7, 1)):
        field = mesh.canonical_field(net, turn.const, t, resolution=24)
        a = field["alpha"]
        assert field["state"] == state and a.shape == tuple(reversed(field["dims"])) and bool(torch.isfinite(a).all())
        level = float(a[a > 0].median())                                   # unmeasured defaults: take a level that gives a surface
        m = mesh.extract(net, turn, t, resolution=24, level=level)
        assert m["state"] == state and m["dims"] == field["dims"] and m["spacing"] == float(field["spacing"])
        # the mesh equals the restatement run on the field it was extracted from
        got = (m["vertices"].cpu().numpy(), None, m["faces"].cpu().numpy())
        fa = m["alpha"].cpu().numpy()
        V, F = assert_equals_restatement(fa, level, m["origin"], m["spacing"], got, tag=f"stage {stage} t {t}")
        assert V > 0 and X.is_closed_oriented_manifold(got[2], V)
        assert abs(m["volume"] - X.signed_volume(got[0], got[2])) <= 1e-9 * max(1.0, m["area"]) and abs(m["area"] - X.area(got[0], got[2])) <= 1e-9 * m["area"]
        _, c64, _ = X.march(fa, level, m["origin"], m["spacing"], rgb=m["rgb"].cpu().numpy())
        col = m["colors"].cpu().numpy()
        assert col.dtype == np.uint8 and col.shape == (V, 3)
        assert np.abs(col.astype(np.int64) - np.floor(255.0 * np.clip(c64, 0, 1)).astype(np.int64)).max() <= 1
        path = str(tmp_path / f"s{stage}_{state}.ply")
        formats.write_ply(path, m["vertices"], m["faces"], m["colors"])
        v2, f2, c2 = formats.read_ply(path)
        assert np.array_equal(v2, got[0]) and np.array_equal(f2, got[2]) and np.array_equal(c2, col)
        fields.append(field["alpha"])
    assert float((fields[0] - fields[1]).abs().max()) > 1e-4, "the state never reached the canonical MLP"


# ------------------------------------------------------------------------------------------ the launcher
@pytest.mark.parametrize("gin,model", [("hosnerf_backpack.gin", "hosnerf"), ("state_humanobject_backpack.gin", "state_humanobject")])
def test_launcher_writes_one_mesh_per_state(tmp_path, gin, model):
    from hosnerf_amd.freeview import write_scene_pixels
    scene = str(tmp_path / "scene")
    write_scene_pixels(scene, synth.write_scene_dir(scene, 6, 64, 64, seed=9))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("patch:\n  N_patches: 2\n  size: 16\n")
    logs = str(tmp_path / "logs")
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "--ginc", os.path.join(ROOT, "configs", gin), "--ginb", "run.max_steps=2",
           "--ginb", f'run.datadir="{scene}"', "--ginb", "run.run_mesh=True", "--ginb", "run.mesh_resolution=16", "--ginb", "run.mesh_level=0.001",
           "--scene_name", "synthetic", "--scene_dir", scene, "--cfg", str(cfg), "--logbase", logs]      # an untrained field stays far below 0.5
    if model == "hosnerf":
        cmd += ["--ginb", 'run.human_path=""', "--ginb", 'run.bkgd_path=""']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    logdir = [os.path.join(logs, d) for d in os.listdir(logs)][0]
    assert os.path.basename(logdir).startswith(model)
    with open(os.path.join(scene, "transitions_times.json")) as f:
        times = tpose.tpose_times([v["time"] for v in json.load(f).values()])
    assert len(times) == 2
    assert sorted(os.listdir(os.path.join(logdir, "mesh"))) == sorted(["meshes.json"] + ["time_{:06}.ply".format(t) for t in times])
    meta = json.load(open(os.path.join(logdir, "mesh", "meshes.json")))
    assert sorted(meta) == sorted("time_{:06}".format(t) for t in times)
    for state, t in enumerate(times):
        row = meta["time_{:06}".format(t)]
        assert set(row) >= {"state", "V", "F", "volume", "area", "level", "spacing", "dims"}
        v, f, c = formats.read_ply(os.path.join(logdir, "mesh", "time_{:06}.ply".format(t)))
        assert row["state"] == state and row["V"] == v.shape[0] and row["F"] == f.shape[0] and c.shape == v.shape
        print(f"{model} t={t}: V {row['V']} F {row['F']} volume {row['volume']:.4f} area {row['area']:.4f}")
        assert row["level"] == 0.001 and max(row["dims"]) == 16 + 3 and X.is_closed_oriented_manifold(f, v.shape[0])
        assert row["V"] > 0 and row["volume"] > 0 and abs(row["volume"] - X.signed_volume(v, f)) < 1e-5 * max(1.0, row["area"])
    assert "results.json" not in os.listdir(logdir)
