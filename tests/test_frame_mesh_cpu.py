"""CPU side of the frame mesh: the numpy restatements the GPU tests judge the kernels by (tests/_frame_mesh_expect.py) against the
oracle's backward LBS and on analytic fields, the PLY pair with normals, `SceneItems.frame_pose`, the world transform, the argument
checks of the three new C entries (no launch) and of `mesh.frame_field` / `mesh.extract_frame`, and the launcher's refusals."""
import ctypes
import os
import pickle
import tempfile

import numpy as np
import pytest
import torch

import oracle.human as oh
from hosnerf_amd import synth
from tests import _frame_mesh_expect as FX
from tests import _mesh_expect as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the backward-LBS restatement
def test_backward_lbs_restatement_agrees_with_the_oracle():
    """On a posed `synth.human_batch`, at the vertices of the frame's own grid: float64 and float32 restatement against
    `oracle.human.backward_lbs` within the bounds tests/test_gpu_human.py sets for the kernel (mask 2e-6, x_skel 5e-5)."""
    from hosnerf_amd.mesh import grid_of_box
    hb = synth.human_batch(8, seed=3)
    sd = synth.human_state_dict(777, 2)
    with torch.no_grad():
        R_b, T_b, _, _ = oh.motion_basis(hb["dst_Rs"], hb["dst_Ts"], hb["cnl_gtfms"])
        vol = oh.motion_weight_volume(sd, hb["motion_weights_priors"])
    assert float((R_b - torch.eye(3)).abs().max()) > 0.05, "the pose must not be the T-pose"
    g = grid_of_box(hb["dst_bbox_min_xyz"].numpy(), hb["dst_bbox_max_xyz"].numpy(), 12)
    ax = [g["origin"][a] + np.arange(g["dims"][a], dtype=np.float32) * g["spacing"] for a in range(3)]
    Z, Y, Xc = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    pts = np.stack([Xc, Y, Z], -1).reshape(-1, 3).astype(np.float32)
    with torch.no_grad():
        x_o, m_o = oh.backward_lbs(torch.from_numpy(pts), R_b, T_b, vol, hb["cnl_bbox_min_xyz"], hb["cnl_bbox_scale_xyz"])
    x_o, m_o = x_o.double().numpy(), m_o.double().numpy()[:, 0]
    assert m_o.max() > 0.5 and (m_o == 0).any()                    # points inside the body and points the volume does not reach
    for dtype in (np.float64, np.float32):
        x, m = FX.backward_lbs(pts, R_b.numpy(), T_b.numpy(), vol.numpy(), hb["cnl_bbox_min_xyz"].numpy(), hb["cnl_bbox_scale_xyz"].numpy(), dtype)
        assert x.dtype == dtype and m.dtype == dtype
        em, ex = float(np.abs(m - m_o).max()), float(np.abs(x - x_o).max())
        print(f"backward LBS restatement {np.dtype(dtype).name} vs oracle: mask {em:.3e}, x_skel {ex:.3e}")
        assert em < 2e-6 and ex < 5e-5


# ------------------------------------------------------------------------------------------ the normals restatement
SPHERE_C, SPHERE_R = np.array([0.47, 0.52, 0.49]), 0.37           # as tests/test_mesh_cpu.py: centre off the lattice of both grids


def _sphere(n):
    o, h, dims, P = X.unit_box_grid(n)
    return o, h, SPHERE_R - np.linalg.norm(P - SPHERE_C, axis=-1)                      # |grad| = 1 wherever the surface is


def test_normals_restatement_on_the_sphere():
    worst = []
    for n in (16, 32):
        o, h, f = _sphere(n)
        v, _, faces = X.march(f, 0.0, o, h, dtype=np.float32)
        nrm = FX.vertex_normals(f, o, h, v)
        length = np.linalg.norm(nrm, axis=1)
        assert nrm.shape == v.shape and (np.abs(length - 1.0) < 1e-12).all()          # |grad| ~ 1: no vertex has g == 0, none is excluded
        radial = (v - SPHERE_C) / np.linalg.norm(v - SPHERE_C, axis=1, keepdims=True)
        cos = np.einsum("ij,ij->i", nrm, radial)
        assert (cos > 0).all()                                                         # outward
        worst.append(float(np.degrees(np.arccos(np.clip(cos, -1, 1))).max()))
        # the float32 restatement: the same normals to fp32 rounding of a well-conditioned quotient
        n32 = FX.vertex_normals(f, o, h, v, dtype=np.float32)
        assert n32.dtype == np.float32 and np.abs(n32 - nrm).max() < 1e-4
        # the normals agree with the faces' orientation: area-weighted face normals point the same way
        fn = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]).astype(np.float64)
        assert (np.einsum("ij,ij->i", fn, nrm[faces[:, 0]]) > 0).all()
    print("largest angle between normal and radius, degrees, resolution 16 / 32:", worst)
    assert worst[1] < worst[0]


def test_normals_restatement_zero_gradient_and_outside():
    """Where the field is 0 all around (outside the mask alpha IS 0) g == 0: exact zeros.  A vertex whose taps are all outside the
    grid, or at a NaN position: zeros too."""
    f = np.zeros((5, 6, 7), dtype=np.float32)
    f[4, 5, 6] = 1.0                                                                   # the far corner: no tap of the vertices below
    v = np.array([[0.3, 0.3, 0.3], [0.31, 0.22, 0.27], [50.0, 0.3, 0.3], [np.nan, 0.3, 0.3]], dtype=np.float32)
    for dtype in (np.float64, np.float32):
        n = FX.vertex_normals(f, (0.0, 0.0, 0.0), 0.1, v, dtype=dtype)
        assert (n == 0).all() and not np.isnan(n).any()
        assert np.abs(FX.vertex_normals(f, (0.0, 0.0, 0.0), 0.1, np.array([[0.55, 0.45, 0.35]], np.float32), dtype=dtype)).max() > 0.1
    # the interpolant reproduces a linear field exactly enough that the normal is the (negative, normalised) gradient
    z, y, x = np.meshgrid(np.arange(5), np.arange(6), np.arange(7), indexing="ij")
    lin = (0.5 * x - 0.25 * y + 1.0 * z).astype(np.float32)
    n = FX.vertex_normals(lin, (0.0, 0.0, 0.0), 1.0, np.array([[2.5, 2.25, 1.75]], dtype=np.float32))
    assert np.allclose(n[0], -np.array([0.5, -0.25, 1.0]) / np.linalg.norm([0.5, -0.25, 1.0]), atol=1e-12)
    # taps outside the grid are zero: at the grid's face the one-sided difference tilts the normal, it does not fail
    edge = FX.vertex_normals(lin + 1.0, (0.0, 0.0, 0.0), 1.0, np.array([[0.0, 2.0, 2.0]], dtype=np.float32))
    assert np.isfinite(edge).all() and abs(np.linalg.norm(edge) - 1.0) < 1e-12


# ------------------------------------------------------------------------------------------ PLY
def test_ply_with_normals_bytes_and_round_trip(tmp_path):
    from hosnerf_amd import formats
    v = np.array([[0.0, 1.0, 2.0], [-1.5, 0.25, 8.0]], dtype=np.float32)
    f = np.array([[0, 1, 0]], dtype=np.int32)
    c = np.array([[1, 2, 3], [250, 251, 252]], dtype=np.uint8)
    n = np.array([[0.0, 0.0, 1.0], [0.6, -0.8, 0.0]], dtype=np.float32)
    path = str(tmp_path / "n.ply")
    formats.write_ply(path, v, f, c, n)
    head = (b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
            b"property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
            b"element face 1\nproperty list uchar int vertex_indices\nend_header\n")
    body = v[0].tobytes() + n[0].tobytes() + c[0].tobytes() + v[1].tobytes() + n[1].tobytes() + c[1].tobytes() + b"\x03" + f[0].tobytes()
    assert open(path, "rb").read() == head + body and len(body) == 2 * 27 + 13
    v2, f2, c2, n2 = formats.read_ply(path, with_normals=True)
    assert v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes() and c2.tobytes() == c.tobytes()
    assert n2.dtype == np.float32 and n2.tobytes() == n.tobytes()
    three = formats.read_ply(path)                                                    # the default still returns three values
    assert len(three) == 3 and three[0].tobytes() == v.tobytes() and three[2].tobytes() == c.tobytes()
    # normals without colours
    formats.write_ply(path, v, f, None, n)
    v3, f3, c3, n3 = formats.read_ply(path, with_normals=True)
    colour_lines = len(b"property uchar red\nproperty uchar green\nproperty uchar blue\n")
    assert c3 is None and n3.tobytes() == n.tobytes() and v3.tobytes() == v.tobytes()
    assert len(open(path, "rb").read()) == len(head) - colour_lines + 2 * 24 + 13
    with pytest.raises(ValueError):
        formats.write_ply(path, v, f, c, n[:1])
    # torch tensors are taken as arrays are
    formats.write_ply(path, torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c), torch.from_numpy(n))
    assert open(path, "rb").read() == head + body


def test_ply_without_normals_is_byte_equal_to_the_earlier_writer(tmp_path):
    from hosnerf_amd import formats
    v = np.array([[0.0, 1.0, 2.0], [-1.5, 0.25, 8.0]], dtype=np.float32)
    f = np.array([[0, 1, 0]], dtype=np.int32)
    c = np.array([[1, 2, 3], [250, 251, 252]], dtype=np.uint8)
    head = (b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
            b"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n")
    plain = head.replace(b"property uchar red\nproperty uchar green\nproperty uchar blue\n", b"")
    face = b"\x03" + f[0].tobytes()
    path = str(tmp_path / "c.ply")
    formats.write_ply(path, v, f, c)
    assert open(path, "rb").read() == head + v[0].tobytes() + c[0].tobytes() + v[1].tobytes() + c[1].tobytes() + face
    formats.write_ply(path, v, f, normals=None)
    assert open(path, "rb").read() == plain + v.tobytes() + face
    assert formats.ply_header(2, 1, True) == head and formats.ply_header(2, 1, False) == plain
    v2, f2, c2, n2 = formats.read_ply(path, with_normals=True)
    assert n2 is None and c2 is None and v2.tobytes() == v.tobytes() and len(formats.read_ply(path)) == 3


# ------------------------------------------------------------------------------------------ SceneItems.frame_pose
POSE_KEYS = {"dst_Rs", "dst_Ts", "dst_posevec", "cnl_gtfms", "canonical_joints", "motion_weights_priors", "cnl_bbox_min_xyz", "cnl_bbox_max_xyz",
             "cnl_bbox_scale_xyz", "time", "iter_val", "is_train", "newsmpl_to_scale_world", "dst_bbox", "frame_name"}


@pytest.fixture(scope="module")
def scene_dir():
    from hosnerf_amd import formats
    d = os.path.join(tempfile.mkdtemp(prefix="hos_frame_pose_"), "scene")
    px = synth.write_scene_dir(d, 6, 32, 32, seed=9)
    formats.load_scene(d, (32, 32), masks=px["alphas"], near=0.1, far=1e6)          # leaves cameras_scaleworld.pkl behind
    return d, px


@pytest.mark.parametrize("stage", [2, 3])
def test_frame_pose(scene_dir, stage):
    from hosnerf_amd.dataset import SceneItems, smpl_frame_camera
    from hosnerf_amd.eval import FRAME_KEYS
    d, px = scene_dir
    ds = SceneItems(d, px["images"], px["alphas"], px["flows"], n_patches=2, patch_size=8, device="cpu", seed=5, stage=stage)
    for idx in (0, 4):
        p = ds.frame_pose(idx)
        name = ds.frames[idx]
        assert set(p) == POSE_KEYS and POSE_KEYS - {"dst_bbox", "frame_name"} <= set(FRAME_KEYS)
        assert not any(k in p for k in ("rays", "near", "far", "ray_mask", "rays_o_bkg"))
        assert p["frame_name"] == name and p["time"] == float(ds.times[idx]) and p["is_train"] is False
        assert float(torch.as_tensor(p["iter_val"]).reshape(-1)[0]) == 1e7
        Rs, Ts, posevec = ds._pose(name)
        assert np.array_equal(p["dst_Rs"].numpy(), Rs) and np.array_equal(p["dst_Ts"].numpy(), Ts) and np.array_equal(p["dst_posevec"].numpy(), posevec)
        assert p["motion_weights_priors"] is ds._prior and np.array_equal(p["cnl_bbox_min_xyz"].numpy(), ds._cnl["cnl_bbox_min_xyz"])
        box = ds.mesh_infos[name]["bbox"]                                           # the frame's, not the canonical one
        assert np.array_equal(p["dst_bbox"]["min_xyz"], box["min_xyz"].astype(np.float32)) and np.array_equal(p["dst_bbox"]["max_xyz"], box["max_xyz"].astype(np.float32))
        assert not np.array_equal(p["dst_bbox"]["min_xyz"], ds._cnl["cnl_bbox_min_xyz"])
        # the expression of eval_frame (tests/test_gpu_frame_mesh.py compares with eval_frame itself, which needs the device)
        cam, m = ds.cameras[name], ds.mesh_infos[name]
        _, newsmpl_to_smpl = smpl_frame_camera(cam["smpl_to_camera"], m["Rh"], m["Th"])
        want = (np.asarray(cam["smpl_to_scale_world"], dtype=np.float64) @ newsmpl_to_smpl).astype(np.float32)
        assert p["newsmpl_to_scale_world"].dtype == torch.float32 and np.array_equal(p["newsmpl_to_scale_world"].numpy(), want)


def test_frame_pose_without_a_world_and_the_refusal(scene_dir, tmp_path):
    """Cameras without `smpl_to_scale_world`: the pose has no `newsmpl_to_scale_world`, and space="world" says so."""
    import shutil
    from hosnerf_amd import mesh
    from hosnerf_amd.dataset import SceneItems
    d, px = scene_dir
    bare = str(tmp_path / "scene")
    shutil.copytree(d, bare)
    with open(os.path.join(bare, "cameras_scaleworld.pkl"), "rb") as f:
        cams = pickle.load(f)
    for c in cams.values():
        c.pop("smpl_to_scale_world")
    with open(os.path.join(bare, "cameras_scaleworld.pkl"), "wb") as f:
        pickle.dump(cams, f)
    ds = SceneItems(bare, px["images"], px["alphas"], px["flows"], device="cpu", seed=5, stage=2)
    p = ds.frame_pose(1)
    assert set(p) == POSE_KEYS - {"newsmpl_to_scale_world"}
    with pytest.raises(ValueError) as e:
        mesh.extract_frame(None, p, resolution=8, space="world")
    assert "smpl_to_scale_world" in str(e.value)


# ------------------------------------------------------------------------------------------ the world transform
def _similarity(scale, mirror):
    r = np.array([0.1, -0.4, 0.05])
    th = np.linalg.norm(r)
    k = np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]]) / th
    Rw = np.eye(3) + np.sin(th) * k + (1.0 - np.cos(th)) * (k @ k)                     # Rodrigues, float64: orthogonal to rounding
    A = np.eye(4)
    A[:3, :3] = scale * Rw @ (np.diag([1.0, -1.0, 1.0]) if mirror else np.eye(3))
    A[:3, 3] = (0.05, -0.02, 0.1)
    return A


@pytest.mark.parametrize("mirror", [False, True])
def test_world_transform(mirror):
    from hosnerf_amd import mesh
    o, h, f = _sphere(16)
    v, _, faces = X.march(f, 0.0, o, h, dtype=np.float32)
    nrm = FX.vertex_normals(f, o, h, v).astype(np.float32)
    nrm[3] = 0.0                                                                   # a zero normal stays zero
    A = _similarity(0.2, mirror)
    det = np.linalg.det(A[:3, :3])
    assert (det < 0) == mirror and abs(abs(det) - 0.2 ** 3) < 1e-12
    v64, f64, n64 = FX.to_space(v, faces, nrm, A)
    gv, gf, gn = mesh.to_space(torch.from_numpy(v), torch.from_numpy(faces), torch.from_numpy(nrm), A)
    assert gv.dtype == torch.float32 and gf.dtype == torch.int32 and gn.dtype == torch.float32
    assert np.array_equal(gf.numpy(), f64) and np.array_equal(gf.numpy(), faces[:, [0, 2, 1]] if mirror else faces)
    assert (np.abs(gv.numpy().astype(np.float64) - v64) <= np.spacing(np.abs(v64).astype(np.float32))).all()          # one rounding
    assert np.abs(gn.numpy() - n64).max() < 1e-6 and (gn.numpy()[3] == 0).all()
    # a similarity: volume scales by |det|, area by |det|^(2/3); the signed volume stays positive, the normals outward
    vol0, area0 = X.signed_volume(v, faces), X.area(v, faces)
    vol1, area1 = X.signed_volume(v64, f64), X.area(v64, f64)
    assert vol0 > 0 and abs(vol1 - abs(det) * vol0) < 1e-12 and abs(area1 - abs(det) ** (2.0 / 3.0) * area0) < 1e-12
    mv, ma = mesh.mesh_measures(gv, gf)
    assert mv > 0 and abs(mv - vol1) < 1e-5 * vol1 and abs(ma - area1) < 1e-5 * area1
    centre = A[:3, :3] @ SPHERE_C + A[:3, 3]
    keep = np.arange(len(v)) != 3
    assert (np.einsum("ij,ij->i", n64[keep], (v64 - centre)[keep]) > 0).all()
    assert (np.einsum("ij,ij->i", gn.numpy()[keep].astype(np.float64), (v64 - centre)[keep]) > 0).all()
    fn = np.cross(v64[f64[:, 1]] - v64[f64[:, 0]], v64[f64[:, 2]] - v64[f64[:, 0]])
    assert (np.einsum("ij,ij->i", fn, (v64[f64[:, 0]] - centre)) > 0).all()        # the faces too


# ------------------------------------------------------------------------------------------ the layers past the box
def test_layers_in_box_and_clip():
    """`grid_of_box` rounds a shorter extent up to whole voxels: the layer that then lies past the box is found per axis, and
    `clip_to_box` zeroes it (and the rim) and nothing else."""
    from hosnerf_amd import mesh
    bmin, bmax = np.array([-0.5, -1.0, 0.25], np.float32), np.array([0.5, 1.0, 0.55], np.float32)       # extents 1, 2, 0.3; h = 0.125
    g = mesh.grid_of_box(bmin, bmax, 16)
    assert g["dims"] == (8 + 3, 16 + 3, 3 + 3)
    k = mesh.layers_in_box(g["origin"], g["spacing"], g["dims"], bmax)
    assert k == (10, 18, 4)                                # x and y: only the rim; z: 0.3 = 2.4 voxels, the layer at 0.625 is past 0.55
    for a in range(3):
        c = g["origin"][a] + np.arange(g["dims"][a], dtype=np.float32) * g["spacing"]
        assert (c[:k[a]] <= bmax[a] + 1e-4 * g["spacing"]).all() and (c[k[a]:] > bmax[a]).all() and k[a] < g["dims"][a]
    # the longest axis of a box whose extent is no fp32 multiple of the spacing keeps its last layer (the tolerance of grid_of_box)
    g3 = mesh.grid_of_box([0.1, 0.1, 0.1], [0.1 + 1.7, 0.4, 0.4], 256)
    assert mesh.layers_in_box(g3["origin"], g3["spacing"], g3["dims"], [0.1 + 1.7, 0.4, 0.4])[0] == g3["dims"][0] - 1
    Nx, Ny, Nz = g["dims"]
    a = torch.full((Nz, Ny, Nx), 0.5)
    out = mesh.clip_to_box(a, g["origin"], g["spacing"], g["dims"], bmax)
    assert out is a and bool((a[:4, :18, :10] == 0.5).all()) and float(a.sum()) == 0.5 * 4 * 18 * 10
    assert not bool(torch.signbit(a).any())


# ------------------------------------------------------------------------------------------ argument checks
def test_python_argument_checks():
    from hosnerf_amd import _lib, mesh, ops
    with pytest.raises(ValueError):
        mesh.frame_field(None, {}, resolution=16, chunk=16383)                      # before anything is read
    with pytest.raises(ValueError) as e:
        mesh.extract_frame(None, {}, space="camera")
    assert "camera" in str(e.value)
    with pytest.raises(ValueError):
        mesh.extract_frame(None, {}, space="world")                                 # no newsmpl_to_scale_world
    with pytest.raises(_lib.HosLibraryError):
        ops.mesh_vertex_normals(torch.zeros(4, 4, 4), (0.0, 0.0, 0.0), 0.1, torch.zeros(3, 3))          # no CPU path
    with pytest.raises(_lib.HosLibraryError):
        ops.grid_warp(torch.zeros(26, 3, 3), torch.zeros(26, 3), torch.zeros(27, 4, 4, 4), torch.zeros(3), torch.ones(3), (0.0, 0.0, 0.0), 0.1,
                      (4, 4, 4), 0, 64)
    for text in ("backward warp", "lbs_forward", "unmeasured", "frame_prologue"):
        assert text in mesh.__doc__.lower(), text


def test_entry_points_validate_without_gpu():
    """-1 (HOS_E_ARG) / -3 (HOS_E_SHAPE) of the three new entries on null, zero and oversized arguments, before any launch."""
    from hosnerf_amd import _lib
    lib = _lib.load()
    for name in ("hos_grid_warp", "hos_grid_alpha_masked", "hos_mesh_vertex_normals"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert lib.hos_version() == _lib.abi_version(_lib.HEADER)
    buf = (ctypes.c_float * 16)()
    a = ctypes.addressof(buf)
    grid = (0.0, 0.0, 0.0, 0.1, 4, 4, 4)
    warp = lambda R=a, T=a, vol=a, V=32, K=26, bmin=a, bscale=a, g=grid, first=0, count=4, x=a, m=a: \
        lib.hos_grid_warp(R, T, vol, V, K, bmin, bscale, *g, first, count, x, m, 0)
    masked = lambda raw=a, mask=a, g=grid, first=0, count=4, alpha=a, rgb=0: lib.hos_grid_alpha_masked(raw, mask, *g, first, count, alpha, rgb, 0)
    normals = lambda field=a, g=grid, v=a, V=4, n=a: lib.hos_mesh_vertex_normals(field, *g, v, V, n, 0)
    # null pointers
    for k in ("R", "T", "vol", "bmin", "bscale", "x", "m"):
        assert warp(**{k: 0}) == -1, k
    for k in ("raw", "mask", "alpha"):
        assert masked(**{k: 0}) == -1, k
    for k in ("field", "v", "n"):
        assert normals(**{k: 0}) == -1, k
    assert normals(V=-1) == -1
    # a dimension below 2, a grid whose edge ids leave int32
    big = (0.0, 0.0, 0.0, 0.1, 51130557, 3, 2)
    for g in ((0.0, 0.0, 0.0, 0.1, 1, 4, 4), (0.0, 0.0, 0.0, 0.1, 4, 1, 4), (0.0, 0.0, 0.0, 0.1, 4, 4, 0), big,
              (0.0, 0.0, 0.0, 0.1, 2 ** 30, 2 ** 30, 2 ** 30)):
        assert warp(g=g) == -3 and masked(g=g) == -3 and normals(g=g) == -3, g
    # bones and volume size
    assert warp(K=33) == -3 and warp(K=0) == -3 and warp(V=0) == -3 and warp(K=32, count=0) == 0
    # vertex ranges outside the grid; more mesh vertices than the grid can carry
    for first, count in ((60, 5), (-1, 5), (0, 65), (65, 0), (0, -1)):
        assert warp(first=first, count=count) == -1 and masked(first=first, count=count) == -1, (first, count)
    assert normals(V=7 * 64 + 1) == -3
    # nothing to do: no launch, and the outputs may then be NULL for the normals
    assert warp(first=64, count=0) == 0 and masked(first=0, count=0) == 0 and normals(V=0) == 0 and normals(V=0, v=0, n=0) == 0


def test_launcher_bindings_and_refusals():
    import run as launcher
    for name, model in (("hosnerf_backpack.gin", "hosnerf"), ("state_humanobject_backpack.gin", "state_humanobject")):
        plan = launcher.main(["--ginc", os.path.join(ROOT, "configs", name), "--scene_name", "Backpack", "--cpu", "--logbase", tempfile.mkdtemp(),
                              "--ginb", "run.max_steps=3", "--ginb", "run.run_mesh_frames=True", "--ginb", 'run.mesh_space="body"',
                              "--ginb", "run.mesh_normals=False"])
        assert plan["model_name"] == model and plan["gin"]["run.run_mesh_frames"] is True and plan["gin"]["run.mesh_space"] == "body"
        assert plan["gin"]["run.mesh_normals"] is False
    s1 = os.path.join(ROOT, "configs", "state_mipnerf360_backpack.gin")
    with pytest.raises(SystemExit) as e:                                            # stage 1 has no human-object network
        launcher.main(["--ginc", s1, "--scene_name", "Backpack", "--cpu", "--logbase", tempfile.mkdtemp(), "--ginb", "run.max_steps=3",
                       "--ginb", "run.run_mesh_frames=True"])
    assert "run.run_mesh_frames" in str(e.value) and "stage 1" in str(e.value)
    with pytest.raises(SystemExit) as e:
        launcher.main(["--ginc", os.path.join(ROOT, "configs", "hosnerf_backpack.gin"), "--scene_name", "Backpack", "--cpu", "--logbase",
                       tempfile.mkdtemp(), "--ginb", "run.max_steps=3", "--ginb", "run.run_mesh_frames=True", "--ginb", 'run.mesh_space="camera"'])
    assert "run.mesh_space" in str(e.value)
    with pytest.raises(SystemExit) as e:                                            # no scene directory
        launcher.extract_frame_meshes(None, {}, None, None, "/nonexistent/last.ckpt", tempfile.mkdtemp(), "cpu", 0, 1)
    assert "--scene_dir" in str(e.value)
    with pytest.raises(SystemExit) as e:                                            # a scene, no checkpoint
        launcher.extract_frame_meshes(None, {}, None, object(), os.path.join(tempfile.mkdtemp(), "last.ckpt"), tempfile.mkdtemp(), "cpu", 0, 1)
    assert "does not exist" in str(e.value) and "run.run_mesh_frames" in str(e.value)
    assert launcher.eval_frame_indices(6, 0) == [0, 1, 2, 3, 4, 5] and launcher.eval_frame_indices(20, 0) == [0, 3, 5, 8, 11, 14, 16, 19]
    assert launcher.eval_frame_indices(6, 4) == [0, 4] and launcher.eval_frame_indices(1, 0) == [0]
    assert "run.run_mesh_frames" in launcher.__doc__
