"""CPU side of the canonical mesh: the PLY pair, the grid of a box, the argument checks of the five C entries (no launch), the
properties of the numpy restatement of marching tetrahedra the GPU tests compare the kernels with (so that their expectation is a
closed oriented manifold of the right volume before any kernel is judged by it), and the launcher's `run.run_mesh` binding."""
import ctypes
import os
import tempfile

import numpy as np
import pytest

from tests import _mesh_expect as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ PLY
@pytest.mark.parametrize("with_colors", [False, True])
def test_ply_round_trip(tmp_path, with_colors):
    from hosnerf_amd import formats
    rs = np.random.RandomState(3)
    v = rs.randn(11, 3).astype(np.float32)
    f = rs.randint(0, 11, size=(7, 3)).astype(np.int32)
    c = rs.randint(0, 256, size=(11, 3)).astype(np.uint8) if with_colors else None
    path = str(tmp_path / "m.ply")
    formats.write_ply(path, v, f, c)
    data = open(path, "rb").read()
    head = formats.ply_header(11, 7, with_colors)
    assert data.startswith(head) and head.endswith(b"end_header\n") and b"format binary_little_endian 1.0\n" in head
    assert (b"property uchar red\nproperty uchar green\nproperty uchar blue\n" in head) == with_colors
    assert b"property float x\nproperty float y\nproperty float z\n" in head and b"property list uchar int vertex_indices\n" in head
    assert len(data) == len(head) + 11 * (15 if with_colors else 12) + 7 * 13
    v2, f2, c2 = formats.read_ply(path)
    assert v2.dtype == np.float32 and f2.dtype == np.int32 and v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()
    assert (c2 is None) if not with_colors else (c2.dtype == np.uint8 and c2.tobytes() == c.tobytes())
    # the first vertex and the first face, byte for byte
    body = data[len(head):]
    assert body[:12] == v[0].tobytes() and (not with_colors or body[12:15] == c[0].tobytes())
    fo = 11 * (15 if with_colors else 12)
    assert body[fo:fo + 1] == b"\x03" and body[fo + 1:fo + 13] == f[0].tobytes()


def test_ply_empty_mesh_and_refusals(tmp_path):
    from hosnerf_amd import formats
    for k, colors in enumerate((None, np.zeros((0, 3), np.uint8))):
        path = str(tmp_path / f"e{k}.ply")
        formats.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), colors)
        assert open(path, "rb").read() == formats.ply_header(0, 0, colors is not None)
        v, f, c = formats.read_ply(path)
        assert v.shape == (0, 3) and f.shape == (0, 3) and ((c is None) if colors is None else c.shape == (0, 3))
    with pytest.raises(ValueError):
        formats.write_ply(str(tmp_path / "bad.ply"), np.zeros((2, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((1, 3), np.uint8))
    (tmp_path / "ascii.ply").write_bytes(b"ply\nformat ascii 1.0\nend_header\n")
    with pytest.raises(ValueError):
        formats.read_ply(str(tmp_path / "ascii.ply"))
    (tmp_path / "short.ply").write_bytes(formats.ply_header(2, 0, False) + b"\0" * 23)
    with pytest.raises(ValueError):
        formats.read_ply(str(tmp_path / "short.ply"))


# ------------------------------------------------------------------------------------------ the grid
def test_grid_of_box():
    from hosnerf_amd.mesh import grid_of_box
    bmin, bmax = np.array([-0.5, -1.0, 0.25], np.float32), np.array([0.5, 1.0, 0.5], np.float32)       # extents 1, 2, 0.25
    g = grid_of_box(bmin, bmax, 16)
    h = np.float32(2.0 / 16)
    assert g["spacing"].dtype == np.float32 and g["spacing"] == h and g["origin"].dtype == np.float32
    # per axis ceil(extent / h) + 1 vertices over the box, plus one layer outside on each side
    assert g["dims"] == (8 + 1 + 2, 16 + 1 + 2, 2 + 1 + 2)
    assert np.array_equal(g["origin"], bmin - h)
    for a in range(3):
        last = g["origin"][a] + np.float32(g["dims"][a] - 1) * h
        assert g["origin"][a] < bmin[a] and g["origin"][a] + h >= bmin[a] - 1e-6             # layer 0 outside, layer 1 on the box
        assert last > bmax[a] and last - h >= bmax[a] - 1e-4 * h                             # the last but one covers the box
    # an extent that is no multiple of h is rounded up
    g2 = grid_of_box([0, 0, 0], [1.0, 0.3, 0.26], 4)
    assert g2["dims"] == (4 + 3, 2 + 3, 2 + 3) and g2["spacing"] == np.float32(0.25)
    # a longest extent whose quotient by the fp32 spacing is not exactly the resolution still gives `resolution` cells
    g3 = grid_of_box([0.1, 0.1, 0.1], [0.1 + 1.7, 0.4, 0.4], 256)
    assert g3["dims"][0] == 256 + 3
    for bad in (1, 0, -3):
        with pytest.raises(ValueError):
            grid_of_box(bmin, bmax, bad)
    with pytest.raises(ValueError):
        grid_of_box(bmin, bmin, 8)


# ------------------------------------------------------------------------------------------ the C entries, before any launch
def test_entry_points_validate_without_gpu():
    from hosnerf_amd import _lib
    lib = _lib.load()                                          # loads without a GPU
    for name in ("hos_grid_points", "hos_grid_alpha", "hos_march_tets_blocks", "hos_march_tets_count", "hos_march_tets_write"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    buf = (ctypes.c_float * 16)()
    a = ctypes.addressof(buf)
    # null pointers: HOS_E_ARG
    assert lib.hos_grid_points(0.0, 0.0, 0.0, 0.1, 4, 4, 4, 0, 64, 0, 0) == -1
    assert lib.hos_grid_alpha(0, 0, 32, 26, 0, 0, 0.0, 0.0, 0.0, 0.1, 4, 4, 4, 0, 64, 0, 0, 0) == -1
    assert lib.hos_grid_alpha(a, a, 32, 26, a, a, 0.0, 0.0, 0.0, 0.1, 4, 4, 4, 0, 64, 0, 0, 0) == -1            # alpha NULL
    assert lib.hos_march_tets_count(0, 4, 4, 4, 0.5, 0, 0, 0, 0) == -1
    assert lib.hos_march_tets_count(a, 4, 4, 4, 0.5, a, a, 0, 0) == -1                                            # counts NULL
    assert lib.hos_march_tets_write(0, 0, 4, 4, 4, 0.5, 0.0, 0.0, 0.0, 0.1, 0, 0, 5, 5, 0, 0, 0, 0) == -1
    assert lib.hos_march_tets_write(a, 0, 4, 4, 4, 0.5, 0.0, 0.0, 0.0, 0.1, a, a, 5, 5, 0, 0, a, 0) == -1         # vertices NULL
    assert lib.hos_march_tets_write(a, a, 4, 4, 4, 0.5, 0.0, 0.0, 0.0, 0.1, a, a, 5, 5, a, 0, a, 0) == -1         # rgb without colors
    # a dimension of 1: HOS_E_SHAPE (with valid pointers: the shape is what is refused)
    for dims in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4)):
        assert lib.hos_grid_points(0.0, 0.0, 0.0, 0.1, *dims, 0, 4, a, 0) == -3
        assert lib.hos_grid_alpha(a, a, 32, 26, a, a, 0.0, 0.0, 0.0, 0.1, *dims, 0, 4, a, 0, 0) == -3
        assert lib.hos_march_tets_blocks(*dims) == -3
        assert lib.hos_march_tets_count(a, *dims, 0.5, a, a, a, 0) == -3
        assert lib.hos_march_tets_write(a, 0, *dims, 0.5, 0.0, 0.0, 0.0, 0.1, a, a, 5, 5, a, 0, a, 0) == -3
    # 7 N >= 2^31 - 256: HOS_E_SHAPE.  N = 306783342 = 2 * 3 * 51130557 is the first such N
    limit = (2 ** 31 - 256 + 6) // 7
    assert 7 * limit >= 2 ** 31 - 256 > 7 * (limit - 1) and limit == 2 * 3 * 51130557
    big, ok = (51130557, 3, 2), (51130557, 2, 2)
    assert lib.hos_march_tets_blocks(*big) == -3 and lib.hos_march_tets_blocks(*ok) == (51130557 * 4 + 255) // 256
    assert lib.hos_march_tets_blocks(2 ** 30, 2 ** 30, 2 ** 30) == -3                      # no overflow on the way to the check
    assert lib.hos_grid_points(0.0, 0.0, 0.0, 0.1, *big, 0, 4, a, 0) == -3
    assert lib.hos_grid_alpha(a, a, 32, 26, a, a, 0.0, 0.0, 0.0, 0.1, *big, 0, 4, a, 0, 0) == -3
    assert lib.hos_march_tets_count(a, *big, 0.5, a, a, a, 0) == -3
    assert lib.hos_march_tets_write(a, 0, *big, 0.5, 0.0, 0.0, 0.0, 0.1, a, a, 5, 5, a, 0, a, 0) == -3
    # a vertex range outside the grid, more bones than the kernel holds: refused; an empty range and an empty mesh: nothing to do
    assert lib.hos_grid_points(0.0, 0.0, 0.0, 0.1, 4, 4, 4, 60, 5, a, 0) == -1 and lib.hos_grid_points(0.0, 0.0, 0.0, 0.1, 4, 4, 4, -1, 5, a, 0) == -1
    assert lib.hos_grid_alpha(a, a, 32, 33, a, a, 0.0, 0.0, 0.0, 0.1, 4, 4, 4, 0, 4, a, 0, 0) == -3
    assert lib.hos_grid_points(0.0, 0.0, 0.0, 0.1, 4, 4, 4, 64, 0, a, 0) == 0
    assert lib.hos_grid_alpha(a, a, 32, 26, a, a, 0.0, 0.0, 0.0, 0.1, 4, 4, 4, 0, 0, a, 0, 0) == 0
    assert lib.hos_march_tets_write(a, 0, 4, 4, 4, 0.5, 0.0, 0.0, 0.0, 0.1, a, a, 0, 0, 0, 0, 0, 0) == 0


def test_python_surface_without_gpu():
    import torch
    from hosnerf_amd import _lib, mesh, ops
    assert ops.MT_BLOCK == 256 and ops.MT_SCAN == 1024
    with pytest.raises(_lib.HosLibraryError):
        ops.march_tets(torch.zeros(4, 4, 4), 0.5, (0.0, 0.0, 0.0), 0.1)                   # no CPU path
    with pytest.raises(_lib.HosLibraryError):
        ops.grid_points((0.0, 0.0, 0.0), 0.1, (4, 4, 4), 0, 64, device="cpu")
    for text in ("non-rigid", "unmeasured", "1e-2"):
        assert text in (mesh.__doc__ + mesh.extract.__doc__).replace("not been measured", "unmeasured")


# ------------------------------------------------------------------------------------------ the restatement
SPHERE_C, SPHERE_R = np.array([0.47, 0.52, 0.49]), 0.37           # centre off the lattice of both grids


def _sphere(n):
    o, h, dims, P = X.unit_box_grid(n)
    return o, h, SPHERE_R - np.linalg.norm(P - SPHERE_C, axis=-1)


def test_tables_are_consistent():
    assert X.PERMS == [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
    assert X.TET_CORNERS == [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]
    for t, (cb, odd) in enumerate(zip(X.TET_CORNERS, X.TET_ODD)):
        p = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in cb], dtype=np.float64)
        assert np.linalg.det(p[1:] - p[0]) == (-1.0 if odd else 1.0)                       # handedness = parity of the permutation
        for lo, up in X.TET_EDGES:
            assert cb[up] & cb[lo] == cb[lo] and 1 <= cb[up] - cb[lo] <= 7                # every edge runs from v to v + d
    for m, tris in enumerate(X.TRI):
        assert len(tris) == (0 if m in (0, 15) else 2 if bin(m).count("1") == 2 else 1)
        for tri in tris:                                                                   # only edges with exactly one end inside
            assert all(((m >> X.TET_EDGES[e][0]) & 1) != ((m >> X.TET_EDGES[e][1]) & 1) for e in tri)
        assert sorted(tuple(sorted(t)) for t in X.TRI[15 - m]) == sorted(tuple(sorted(t)) for t in tris)


def test_restatement_sphere_is_a_closed_oriented_manifold_of_the_right_volume():
    errs = []
    for n in (16, 32):
        o, h, f = _sphere(n)
        v, _, faces = X.march(f, 0.0, o, h)
        V, F = v.shape[0], faces.shape[0]
        assert V > 0 and faces.dtype == np.int32 and faces.min() == 0 and faces.max() == V - 1
        assert X.is_closed_oriented_manifold(faces, V)                 # every directed edge once, its reverse once
        assert X.euler_characteristic(faces, V) == 2
        vol = X.signed_volume(v, faces)
        assert vol > 0                                                 # normals point from inside to outside
        errs.append(abs(vol - 4.0 / 3.0 * np.pi * SPHERE_R ** 3))
        assert np.abs(np.linalg.norm(v - SPHERE_C, axis=1) - SPHERE_R).max() < float(h) ** 2       # linear interpolation of a distance
        # the same rules in fp32 give the same faces and positions within fp32 rounding of a unit box
        v32, _, f32 = X.march(f, 0.0, o, h, dtype=np.float32)
        assert v32.dtype == np.float32 and np.array_equal(f32, faces) and np.abs(v32 - v).max() < 4 * 2.0 ** -23
    assert errs[0] / errs[1] >= 3.0, errs                              # theory: 4 for linear interpolation; measured 3.98
    print("sphere volume errors", errs, errs[0] / errs[1])


def test_restatement_topology_of_two_spheres_and_a_torus():
    o, h, dims, P = X.unit_box_grid(32)
    two = np.maximum(0.2 - np.linalg.norm(P - [0.27, 0.3, 0.31], axis=-1), 0.2 - np.linalg.norm(P - [0.73, 0.7, 0.69], axis=-1))
    v, _, faces = X.march(two, 0.0, o, h)
    assert X.is_closed_oriented_manifold(faces, len(v)) and X.euler_characteristic(faces, len(v)) == 4
    q = P - [0.5, 0.51, 0.49]
    torus = 0.12 - np.sqrt((np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - 0.3) ** 2 + q[..., 2] ** 2)
    v, _, faces = X.march(torus, 0.0, o, h)
    assert X.is_closed_oriented_manifold(faces, len(v)) and X.euler_characteristic(faces, len(v)) == 0
    assert abs(X.signed_volume(v, faces) - 2 * np.pi ** 2 * 0.3 * 0.12 ** 2) < 2e-3


def test_restatement_edge_rules():
    """NaN and a value equal to the level are outside; a non-finite end puts the vertex at t = 0.5; order and colours."""
    f = np.full((3, 3, 3), -1.0, dtype=np.float32)
    f[1, 1, 1] = 1.0
    rgb = np.zeros((3, 3, 3, 3), dtype=np.float32)
    rgb[1, 1, 1] = (1.0, 0.5, 0.25)
    v, c, faces = X.march(f, 0.0, (0.0, 0.0, 0.0), 1.0, rgb=rgb)
    assert len(v) == 14 and X.is_closed_oriented_manifold(faces, 14) and X.euler_characteristic(faces, 14) == 2    # 7 edges each way
    assert np.allclose(c, 0.5 * np.array([1.0, 0.5, 0.25])) and abs(np.abs(v - 1.0).max() - 0.5) < 1e-12
    # owners ascend (vertices 0, 1, 3, 4, 9, 10, 12 own the edges INTO the centre, d = 7 .. 1), then the centre's families 0 .. 6
    want = [(.5, .5, .5), (1, .5, .5), (.5, 1, .5), (1, 1, .5), (.5, .5, 1), (1, .5, 1), (.5, 1, 1),
            (1.5, 1, 1), (1, 1.5, 1), (1.5, 1.5, 1), (1, 1, 1.5), (1.5, 1, 1.5), (1, 1.5, 1.5), (1.5, 1.5, 1.5)]
    assert np.array_equal(v, np.array(want))
    for centre in (np.inf, 3e38):
        g = f.copy()
        g[1, 1, 1] = centre
        g[1, 1, 2] = np.nan if centre == np.inf else -3e38
        v, _, faces = X.march(g, 0.0, (0.0, 0.0, 0.0), 1.0)
        assert np.isfinite(v).all() and X.is_closed_oriented_manifold(faces, len(v)) and len(v) == 14
    level = X.march(np.where(f > 0, 2.0, 0.0), 0.0, (0.0, 0.0, 0.0), 1.0)                # the outside sits exactly on the level
    assert len(level[0]) == 14 and np.isfinite(level[0]).all()
    assert len(X.march(np.zeros((3, 3, 3)), 0.0, (0, 0, 0), 1.0)[2]) == 0 and len(X.march(np.ones((3, 3, 3)), 0.0, (0, 0, 0), 1.0)[0]) == 0


# ------------------------------------------------------------------------------------------ launcher
def test_launcher_run_mesh_binding():
    import run as launcher
    for name, model in (("hosnerf_backpack.gin", "hosnerf"), ("state_humanobject_backpack.gin", "state_humanobject")):
        plan = launcher.main(["--ginc", os.path.join(ROOT, "configs", name), "--scene_name", "Backpack", "--cpu", "--logbase", tempfile.mkdtemp(),
                              "--ginb", "run.max_steps=3", "--ginb", "run.run_mesh=True", "--ginb", "run.mesh_resolution=16"])
        assert plan["mode"] == "cpu-plumbing" and plan["model_name"] == model and plan["gin"]["run.run_mesh"] is True
        assert plan["gin"]["run.mesh_resolution"] == 16
    s1 = os.path.join(ROOT, "configs", "state_mipnerf360_backpack.gin")
    with pytest.raises(SystemExit) as e:
        launcher.main(["--ginc", s1, "--scene_name", "Backpack", "--cpu", "--logbase", tempfile.mkdtemp(), "--ginb", "run.max_steps=3",
                       "--ginb", "run.run_mesh=True"])
    assert "run.run_mesh" in str(e.value)
    plan1 = launcher.main(["--ginc", s1, "--scene_name", "Backpack", "--cpu", "--logbase", tempfile.mkdtemp(), "--ginb", "run.max_steps=3"])
    assert plan1["model_name"] == "state_mipnerf360"                                      # without the binding: as before
    assert "run.run_mesh" in launcher.__doc__
