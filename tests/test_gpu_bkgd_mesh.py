"""The background mesh on the GPU: the point-Gaussian encoder (`ops.encode_ipe_points` / `_planes`) against the float64 oracle chain
(tests/_bkgd_mesh_expect.py), `MipNeRF360MLP.query_points` / `mesh.bkgd_field` against `oracle.background.mlp_forward` in float64,
`ops.grid_alpha_density` against its restatement, `mesh.extract_bkgd` against the marching restatement of tests/_mesh_expect.py, and
the launcher's `run.run_mesh_bkgd`.

Tolerances.  Encoder: the project's own per-level bound of tests/test_gpu_bkgd.py::test_encode_ipe, 2e-6 + 2^level * 1.5e-6 (the
point path has fewer roundings ahead of the sine than the frustum path it was set for).  MLP outputs: no test of the suite compares
`MipNeRF360MLP.query` with the oracle sample by sample except test_gpu_bkgd.py::test_forward_vs_golden, whose bound on the NeRF MLP's
per-sample outputs is |hip - f64| <= 2 |oracle f32 - f64| + 2e-5 (both GEMM modes): used here unchanged, for the colours and for the
density (everything behind X is the same code).  Alpha and the mesh vertices follow the accuracy rule of tests/test_gpu_mesh.py:
|hip - f64 restatement| <= 2 |f32 restatement - f64 restatement| + one fp32 ulp of the largest value; faces, V and F are exact."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle.background as ob
from hosnerf_amd import formats, synth, tpose
from tests import _bkgd_mesh_expect as E
from tests import _mesh_expect as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
VARS = (0.0, float(np.float32((2.0 / 256) ** 2 / 12)), float(np.float32(1e-2)))
BOX = (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5)
RES, CHUNK = 24, 8192
STATE_TIMES = ((0.2, 0), (0.7, 1))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from hosnerf_amd import _lib
    _lib.load()
    return torch.device("cuda")


def maxerr(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def level_bounds(X_, want, scale=1.0):
    """max error per (half, level) block of the 504 IPE columns against `want`, with the project's per-level tolerance."""
    out = []
    for half in (0, 252):
        for lvl in range(12):
            sl = slice(half + lvl * 21, half + (lvl + 1) * 21)
            out.append((lvl, maxerr(X_[:, sl], want[:, sl]), 2e-6 + (2.0 ** lvl) * 1.5e-6 * scale))
    return out


# ------------------------------------------------------------------------------------------ 1. the encoder against float64
@pytest.mark.parametrize("var", VARS)
@pytest.mark.parametrize("P", [1, 63, 64, 65, 129])
def test_encode_ipe_points_vs_float64(dev, P, var):
    from hosnerf_amd import ops
    pts = E.point_mix(P, seed=P)
    basis = ob.generate_basis().contiguous()
    embed = torch.arange(64, dtype=torch.float32) * 0.5 - 7.0
    Xd = ops.encode_ipe_points(pts.to(dev), var, basis.to(dev), embed.to(dev), 576)
    assert Xd.shape == (P, 576) and bool(torch.isfinite(Xd).all())
    want = E.encode_points(pts, var, basis)
    for lvl, err, tol in level_bounds(Xd[:, :504], want):
        assert err < tol, (P, var, lvl, err, tol)
    assert torch.equal(Xd[:, 504:568].cpu(), embed.expand(P, 64))                        # the embedding columns are exact
    assert float(Xd[:, 568:].abs().max()) == 0                                           # the pad is zero
    if var == 0.0:                                                                       # a damping of exactly 1: level 0 of the origin's row is sin(0), sin(pi/2)
        assert float(Xd[0, :21].abs().max()) == 0 and float((Xd[0, 252:273] - 1.0).abs().max()) == 0
    # the planes form: the same fp32 values, split into fp16 / bf16 hi-lo pairs by the encoder itself
    p16, pb = ops.encode_ipe_points_planes(pts.to(dev), var, basis.to(dev), embed.to(dev), 576)
    q16, qb = ops.split_planes2(Xd, C=576, ld=576)
    assert torch.equal(p16.t, q16.t) and torch.equal(pb.t, qb.t)
    only16, none_b = ops.encode_ipe_points_planes(pts.to(dev), var, basis.to(dev), embed.to(dev), 576, want_bf16=False)
    none_16, onlyb = ops.encode_ipe_points_planes(pts.to(dev), var, basis.to(dev), embed.to(dev), 576, want_fp16=False)
    assert none_b is None and none_16 is None and torch.equal(only16.t, q16.t) and torch.equal(onlyb.t, qb.t)
    # a wider row: the pad grows, nothing else moves; a caller's buffer is written in place
    wide = torch.full((P, 608), -7.0, device=dev)
    assert ops.encode_ipe_points(pts.to(dev), var, basis.to(dev), embed.to(dev), 608, out=wide) is wide
    assert torch.equal(wide[:, :568], Xd[:, :568]) and float(wide[:, 568:].abs().max()) == 0


def test_encode_ipe_points_rejects_bad_input(dev):
    from hosnerf_amd import _lib, ops
    basis, embed = ob.generate_basis().contiguous().to(dev), torch.zeros(64, device=dev)
    for pts, var in ((torch.zeros(0, 3, device=dev), 0.1), (torch.zeros(4, 2, device=dev), 0.1), (torch.zeros(4, 3, device=dev), -1.0),
                     (torch.zeros(4, 3, device=dev), float("nan"))):
        with pytest.raises(_lib.HosLibraryError):
            ops.encode_ipe_points(pts, var, basis, embed)
        with pytest.raises(_lib.HosLibraryError):
            ops.encode_ipe_points_planes(pts, var, basis, embed)


# ------------------------------------------------------------------------------------------ 2. the range fallback
def test_encode_ipe_points_beyond_the_own_sine_range(dev):
    """The basis scaled by 40 (as test_encode_ipe_beyond_the_own_sine_range): workgroups whose lifted means leave the range of the
    encoder's own sine take the library's; finite, the tolerance scaled with the argument, levels 0-2 tight enough to tell a wrong
    quadrant, and two launches on the same input bit-equal."""
    from hosnerf_amd import ops
    P, var, scale = 129, VARS[1], 40.0
    pts = E.point_mix(P, seed=7)
    basis = (ob.generate_basis() * scale).contiguous()
    embed = torch.arange(64, dtype=torch.float32)
    a = ops.encode_ipe_points(pts.to(dev), var, basis.to(dev), embed.to(dev), 576)
    assert bool(torch.isfinite(a).all())
    want = E.encode_points(pts, var, basis)
    for lvl, err, tol in level_bounds(a[:, :504], want, scale):
        assert err < tol, (lvl, err, tol)
    assert maxerr(a[:, :63], want[:, :63]) < 4e-4
    assert torch.equal(a[:, 504:568].cpu(), embed.expand(P, 64))
    b = ops.encode_ipe_points(pts.to(dev), var, basis.to(dev), embed.to(dev), 576)
    assert torch.equal(a, b)
    p1, _ = ops.encode_ipe_points_planes(pts.to(dev), var, basis.to(dev), embed.to(dev), 576, want_bf16=False)
    p2, _ = ops.encode_ipe_points_planes(pts.to(dev), var, basis.to(dev), embed.to(dev), 576, want_bf16=False)
    assert torch.equal(p1.t, p2.t) and torch.equal(p1.t, ops.split_planes2(a, C=576, ld=576, wantb=False)[0].t)


# ------------------------------------------------------------------------------------------ 3. the frustum entries
def test_frustum_entries_are_stable(dev):
    """The frustum encoder shares everything after its first stage with the point encoder: the same inputs twice, bit-equal (its
    values are held by tests/test_gpu_bkgd.py::test_encode_ipe against the golden vectors)."""
    from hosnerf_amd import ops
    hv = np.load(os.path.join(G, "bkgd_helpers.npz"))
    tdist, o, d, radii, basis = (torch.from_numpy(np.ascontiguousarray(hv[k])).to(dev) for k in ("cast_tdist", "cast_o", "cast_d", "cast_radii", "basis"))
    embed = torch.arange(64, dtype=torch.float32, device=dev)
    a = ops.encode_ipe(tdist, o, d, radii, basis, embed, 576)
    b = ops.encode_ipe(tdist, o, d, radii, basis, embed, 576)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    pa, pb_ = ops.encode_ipe_planes(tdist, o, d, radii, basis, embed, 576)
    qa, qb = ops.encode_ipe_planes(tdist, o, d, radii, basis, embed, 576)
    assert torch.equal(pa.t, qa.t) and torch.equal(pb_.t, qb.t)


# ------------------------------------------------------------------------------------------ 4. the field
def _basedir():
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    return d


@pytest.fixture(scope="module")
def model(dev):
    from hosnerf_amd.mipnerf360 import MipNeRF360
    m = MipNeRF360(_basedir(), opaque_background=True)
    m.load_state_dict(synth.background_state_dict(777, 2), strict=False)
    return m.to(dev)


def oracle_mlp(dev, dtype):
    sd = {k: (v.to(dev).to(dtype) if v.is_floating_point() else v.to(dev)) for k, v in synth.background_state_dict(777, 2).items()}
    return ob.MLPWeights(sd, "mlps.2.")


def oracle_points(wts, pts, var, viewdirs, state, dtype):
    """`oracle.background.mlp_forward` at the Gaussians (pts, var I), one view direction per point: B = P rays of S = 1 sample."""
    P = pts.shape[0]
    covs = (float(var) * torch.eye(3, dtype=dtype, device=pts.device)).expand(P, 1, 3, 3)
    with torch.no_grad():
        out = ob.mlp_forward(wts, pts.to(dtype).view(P, 1, 3), covs, viewdirs.to(dtype), state)
    return out["density"].view(P), out["rgb"].view(P, 3)


@pytest.fixture(scope="module")
def fields(dev, model):
    """Both states' fields on the box, once; the float64 / float32 oracle densities at the same grid points (the oracle runs on the
    device: it is eager torch in either precision)."""
    from hosnerf_amd import mesh, ops
    out = {}
    w64, w32 = oracle_mlp(dev, torch.float64), oracle_mlp(dev, torch.float32)
    for t, state in STATE_TIMES:
        f = mesh.bkgd_field(model, BOX, t, resolution=RES, chunk=CHUNK)
        Nx, Ny, Nz = f["dims"]
        N = Nx * Ny * Nz
        pts = ops.grid_points(f["origin"], f["spacing"], f["dims"], 0, N, device=dev)
        view = torch.tensor([mesh.HEAD_ON_FALLBACK], device=dev).expand(N, 3)
        d64, _ = oracle_points(w64, pts, f["var"], view, state, torch.float64)
        d32, _ = oracle_points(w32, pts, f["var"], view, state, torch.float32)
        out[state] = {"field": f, "pts": pts, "d64": d64, "d32": d32, "time": t}
    return out


@pytest.mark.parametrize("state", [0, 1])
def test_bkgd_field(dev, fields, state):
    from hosnerf_amd import mesh
    f, d64, d32 = fields[state]["field"], fields[state]["d64"], fields[state]["d32"]
    Nx, Ny, Nz = f["dims"]
    N = Nx * Ny * Nz
    assert f["dims"] == (27, 27, 27) and N % CHUNK != 0 and N > 2 * CHUNK and f["state"] == state       # a ragged last chunk
    assert f["var"] == mesh.voxel_variance(f["spacing"]) and f["alpha"].shape == (Nz, Ny, Nx)
    r = fields[state]["pts"].norm(dim=1)
    assert bool((r <= 1).any()) and bool((r > 1).any())                                                 # both contraction branches
    dens = f["density"].reshape(-1)
    assert bool(torch.isfinite(dens).all()) and float(dens.min()) >= 0.0
    e_hip, e_ref = maxerr(dens, d64), maxerr(d32, d64)
    tol = 2.0 * e_ref + 2e-5
    print(f"state {state}: density vs f64 oracle {e_hip:.3e} (oracle f32 {e_ref:.3e}, bound {tol:.3e}), max density {float(d64.max()):.3f}")
    assert e_hip <= tol, (e_hip, e_ref, tol)
    # alpha: the restatement on the device's own density
    a = f["alpha"].cpu().numpy()
    dn = dens.cpu().numpy()
    a64, a32 = E.alpha_of_density(dn, f["spacing"], f["dims"]), E.alpha_of_density(dn, f["spacing"], f["dims"], np.float32)
    ea, er = float(np.abs(a.astype(np.float64) - a64).max()), float(np.abs(a32.astype(np.float64) - a64).max())
    ulp = float(np.spacing(np.float32(np.abs(a64).max())))
    print(f"state {state}: alpha vs f64 restatement {ea:.3e} (f32 restatement {er:.3e}, ulp {ulp:.3e}), max alpha {a.max():.4f}")
    assert ea <= 2.0 * er + ulp, (ea, er, ulp)
    rim = E.rim_mask(f["dims"])
    assert (a[rim] == 0.0).all() and not np.signbit(a[rim]).any() and (a[~rim] > 0).any()


def test_bkgd_field_states_and_chunks(dev, fields, model):
    from hosnerf_amd import mesh
    a0, a1 = fields[0]["field"]["alpha"], fields[1]["field"]["alpha"]
    assert float((a0 - a1).abs().max()) > 1e-4, "the state never reached the NeRF MLP"
    # one chunk for the whole grid: the same field up to the GEMM's tile routes, inside the density bound
    one = mesh.bkgd_field(model, BOX, fields[1]["time"], resolution=RES, chunk=1 << 18)
    assert one["dims"] == fields[1]["field"]["dims"] and float((one["density"] - fields[1]["field"]["density"]).abs().max()) <= 2e-5
    with pytest.raises(ValueError):
        mesh.bkgd_field(model, BOX, 0.7, resolution=RES, chunk=0)


def test_query_points_refuses_autograd(dev, model):
    pts = torch.zeros(4, 3, device=dev)
    with pytest.raises(RuntimeError):
        model.mlps[-1].query_points(pts, 0.01, pts, 0.5)
    with torch.no_grad():
        with pytest.raises(ValueError):
            model.mlps[-1].query_points(pts, 0.01, pts[:2], 0.5)
        prop = model.mlps[0].query_points(pts, 0.01, pts, 0.5)                                          # a proposal MLP: density only
        assert prop["density"].shape == (4,) and prop["rgb"].shape == (4, 3) and float(prop["rgb"].abs().max()) == 0


# ------------------------------------------------------------------------------------------ 5. the mesh
@pytest.mark.parametrize("state", [0, 1])
def test_extract_bkgd(dev, fields, model, state, tmp_path):
    from hosnerf_amd import eval as ev, mesh
    from tests.test_gpu_mesh import assert_equals_restatement
    f, t = fields[state]["field"], fields[state]["time"]
    inner = f["alpha"][1:-1, 1:-1, 1:-1]
    level = float(inner.median())                                       # random weights never reach 0.5: a level that gives a surface
    m = mesh.extract_bkgd(model, BOX, t, resolution=RES, level=level, chunk=CHUNK)
    assert set(m) >= {"vertices", "faces", "colors", "normals", "origin", "spacing", "dims", "state", "volume", "area", "level", "alpha"}
    assert m["state"] == state and m["dims"] == f["dims"] and m["spacing"] == float(f["spacing"]) and m["level"] == level
    assert torch.equal(m["alpha"], f["alpha"]) and m["box"] == list(BOX)
    got = (m["vertices"].cpu().numpy(), None, m["faces"].cpu().numpy())
    V, F = assert_equals_restatement(m["alpha"].cpu().numpy(), level, m["origin"], m["spacing"], got, tag=f"state {state}")
    assert V > 0 and F > 0 and X.is_closed_oriented_manifold(got[2], V)
    assert abs(m["volume"] - X.signed_volume(got[0], got[2])) <= 1e-9 * max(1.0, m["area"]) and abs(m["area"] - X.area(got[0], got[2])) <= 1e-9 * m["area"]
    # normals: unit or exactly zero
    n = m["normals"]
    length = n.double().norm(dim=1)
    zero = (n == 0).all(dim=1)
    assert n.shape == (V, 3) and bool(((length - 1.0).abs() < 1e-5)[~zero].all()) and not bool(zero.all())
    # colours: the NeRF MLP at the device's vertices seen head-on, against the oracle in float64
    view = mesh.head_on_viewdirs(n)
    assert torch.equal(view[~zero], -n[~zero]) and bool((view[zero] == torch.tensor(mesh.HEAD_ON_FALLBACK, device=dev)).all())
    _, c64 = oracle_points(oracle_mlp(dev, torch.float64), m["vertices"], m["var"], view, state, torch.float64)
    _, c32 = oracle_points(oracle_mlp(dev, torch.float32), m["vertices"], m["var"], view, state, torch.float32)
    e_hip, e_ref = maxerr(m["vertex_rgb"], c64), maxerr(c32, c64)
    print(f"state {state}: V {V} F {F} level {level:.5f}; vertex rgb vs f64 oracle {e_hip:.3e} (oracle f32 {e_ref:.3e})")
    assert e_hip <= 2.0 * e_ref + 2e-5, (e_hip, e_ref)
    assert m["colors"].dtype == torch.uint8 and torch.equal(m["colors"], ev.to_8b_image(m["vertex_rgb"]))
    # normals=False only drops them
    bare = mesh.extract_bkgd(model, BOX, t, resolution=RES, level=level, normals=False, chunk=CHUNK)
    assert bare["normals"] is None and torch.equal(bare["vertices"], m["vertices"]) and torch.equal(bare["faces"], m["faces"])
    assert torch.equal(bare["colors"], m["colors"])
    path = str(tmp_path / f"bkgd_{state}.ply")
    formats.write_ply(path, m["vertices"], m["faces"], m["colors"], m["normals"])
    v2, f2, c2, n2 = formats.read_ply(path, with_normals=True)
    assert np.array_equal(v2, got[0]) and np.array_equal(f2, got[2]) and np.array_equal(c2, m["colors"].cpu().numpy()) and np.array_equal(n2, n.cpu().numpy())


def test_extract_bkgd_empty_mesh(dev, model):
    from hosnerf_amd import mesh
    m = mesh.extract_bkgd(model, BOX, 0.7, resolution=8, level=2.0)                                     # alpha < 1 everywhere: nothing to cut
    assert m["vertices"].shape == (0, 3) and m["faces"].shape == (0, 3) and m["colors"].shape == (0, 3) and m["normals"].shape == (0, 3)
    assert m["volume"] == 0.0 and m["area"] == 0.0


# ------------------------------------------------------------------------------------------ 6. the launcher
@pytest.mark.parametrize("gin,model_name", [("state_mipnerf360_backpack.gin", "state_mipnerf360"), ("hosnerf_backpack.gin", "hosnerf")])
def test_launcher_writes_one_background_mesh_per_state(tmp_path, gin, model_name):
    from hosnerf_amd.freeview import write_scene_pixels
    scene = str(tmp_path / "scene")
    logs = str(tmp_path / "logs")
    box = (-1.25, -1.0, -1.0, 1.25, 1.0, 1.0)
    common = ["--ginb", "run.max_steps=2", "--ginb", f'run.datadir="{scene}"', "--ginb", "run.run_mesh_bkgd=True", "--ginb", "run.mesh_resolution=16",
              "--ginb", "run.mesh_level=0.001", "--ginb", f"run.mesh_bkgd_box={box}", "--scene_name", "synthetic", "--scene_dir", scene, "--logbase", logs]
    if model_name == "hosnerf":
        write_scene_pixels(scene, synth.write_scene_dir(scene, 6, 64, 64, seed=9))
        cfg = tmp_path / "cfg.yaml"
        cfg.write_text("patch:\n  N_patches: 2\n  size: 16\n")
        extra = ["--cfg", str(cfg), "--ginb", 'run.human_path=""', "--ginb", 'run.bkgd_path=""']
    else:
        write_scene_pixels(scene, synth.write_scene_dir(scene, 6, 24, 24, seed=9))
        extra = ["--ginb", "LitData.batch_size=512"]
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "--ginc", os.path.join(ROOT, "configs", gin)] + common + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    logdir = [os.path.join(logs, d) for d in os.listdir(logs)][0]
    assert os.path.basename(logdir).startswith(model_name)
    with open(os.path.join(scene, "transitions_times.json")) as f:
        times = tpose.tpose_times([v["time"] for v in json.load(f).values()])
    assert len(times) == 2
    folder = os.path.join(logdir, "mesh_bkgd")
    assert sorted(os.listdir(folder)) == sorted(["meshes.json"] + ["time_{:06}.ply".format(t) for t in times])
    meta = json.load(open(os.path.join(folder, "meshes.json")))
    assert sorted(meta) == sorted("time_{:06}".format(t) for t in times)
    for state, t in enumerate(times):
        row = meta["time_{:06}".format(t)]
        assert set(row) >= {"time", "state", "V", "F", "volume", "area", "level", "spacing", "dims", "box"}
        v, f, c, n = formats.read_ply(os.path.join(folder, "time_{:06}.ply".format(t)), with_normals=True)
        assert row["state"] == state and row["V"] == v.shape[0] and row["F"] == f.shape[0] and c.shape == v.shape and n.shape == v.shape
        assert row["box"] == list(box) and row["level"] == 0.001 and max(row["dims"]) == 16 + 3 and row["dims"] == [19, 16, 16]
        print(f"{model_name} t={t}: V {row['V']} F {row['F']} volume {row['volume']:.4f} area {row['area']:.4f}")
        # an untrained density is small but positive: at this level the surface is the box's cap, closed, inside the grid (the box grown
        # by a voxel, and on an axis whose extent is no multiple of the spacing by less than one more)
        assert row["V"] > 0 and row["F"] > 0 and X.is_closed_oriented_manifold(f, v.shape[0])
        assert (v >= np.array(box[:3]) - row["spacing"] - 1e-6).all() and (v <= np.array(box[3:]) + 2 * row["spacing"] + 1e-6).all()
        assert abs(row["volume"] - X.signed_volume(v, f)) < 1e-5 * max(1.0, row["area"])
    assert "results.json" not in os.listdir(logdir)
    assert not os.path.exists(os.path.join(logdir, "mesh")) and not os.path.exists(os.path.join(logdir, "mesh_frames"))
