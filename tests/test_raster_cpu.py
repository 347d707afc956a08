"""The mesh rasteriser's rules without a GPU: the numpy restatement (tests/_raster_expect.py) on hand cases with exact arithmetic and
on the analytic sphere, `fit` on hand-made maps, the files `freeview.save_mesh_maps` writes and the launcher's argument checks.
tests/test_gpu_raster.py holds the kernels to the same restatement."""
import os
import tempfile

import numpy as np
import pytest

from tests import _raster_expect as RX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a camera whose projections of the hand cases are dyadic: focal 64, centre (8, 8), looking down +z from the origin
K0 = np.array([[64.0, 0.0, 8.0], [0.0, 64.0, 8.0], [0.0, 0.0, 1.0]])
R0, T0 = np.eye(3), np.zeros(3)
H0 = W0 = 16


def at(col, row, z=2.0):
    """The point that projects to pixel (col, row) at depth z (exact: every quantity is a dyadic rational)."""
    return [(col - 8.0) * z / 64.0, (row - 8.0) * z / 64.0, z]


def square(x0, y0, x1, y1, z=2.0):
    return np.array([at(x0, y0, z), at(x1, y0, z), at(x1, y1, z), at(x0, y1, z)], dtype=np.float32)


def counts(vertices, faces, H=H0, W=W0):
    xy, z, _ = RX.project(vertices, K0, R0, T0, np.float32)
    per_face, dropped = RX.coverage(xy, faces, H, W)
    total = np.zeros(H * W, dtype=np.int64)
    for p in per_face:
        np.add.at(total, p, 1)
    return total.reshape(H, W), dropped, per_face


def test_projection_of_the_hand_points_is_exact():
    v = np.array([at(3, 5), at(12.5, 0.25, 4.0), at(-2, 20, 0.5)], dtype=np.float32)
    for dtype in (np.float32, np.float64):
        xy, z, uv = RX.project(v, K0, R0, T0, dtype)
        assert xy.tolist() == [[3 * 256, 5 * 256], [3200, 64], [-512, 5120]]
        assert z.tolist() == [2.0, 4.0, 0.5]


@pytest.mark.parametrize("split", [[[0, 1, 2], [0, 2, 3]], [[0, 1, 3], [1, 2, 3]]])
def test_square_on_pixel_centres_covers_the_half_open_box_once(split):
    v = square(3, 4, 11, 9)
    want = np.zeros((H0, W0), dtype=np.int64)
    want[4:9, 3:11] = 1                                          # [x0,x1) x [y0,y1): the top and left edges in, the bottom and right out
    seen = []
    for faces in (split, [f[::-1] for f in split], [f[1:] + f[:1] for f in split], [split[1], split[0]]):
        total, dropped, _ = counts(v, np.array(faces))
        assert dropped == 0 and np.array_equal(total, want), faces
        seen.append(total)
    assert all(np.array_equal(seen[0], s) for s in seen)         # whatever the vertex order and the orientation


def test_a_fan_about_a_pixel_centre_covers_it_once():
    """Six triangles about a vertex ON a pixel centre, the spokes through other centres: every centre of the hexagon's interior once."""
    ring = [(10, 8), (9, 11), (6, 11), (4, 8), (6, 5), (9, 5)]
    v = np.array([at(7, 8)] + [at(c, r) for c, r in ring], dtype=np.float32)
    faces = np.array([[0, 1 + k, 1 + (k + 1) % 6] for k in range(6)])
    total, dropped, _ = counts(v, faces)
    assert dropped == 0 and total.max() == 1 and total[8, 7] == 1 and total[8, 5:10].tolist() == [1] * 5


def test_coincident_triangles_go_to_the_lower_face_id():
    v = square(2, 2, 12, 12)
    faces = np.array([[0, 1, 2], [0, 1, 2], [0, 2, 1]])
    for dtype in (np.float32, np.float64):
        xy, z, _ = RX.project(v, K0, R0, T0, dtype)
        c = RX.candidates(xy, z, faces, H0, W0, dtype, face_base=7)
        win = RX.zbuffer(c, H0 * W0)
        assert win.size > 0 and (c["face"][win] == 7).all() and np.unique(c["pix"][win]).size == win.size
        assert np.abs(c["depth"][win] - 2.0).max() < 1e-6        # a plane at z = 2 (b_i = e_i / area is rounded, so not exactly 2)
        for p in np.unique(c["pix"]):                             # the three faces tie in every bit: the id alone decides
            assert np.unique(c["depth"][c["pix"] == p]).size == 1 and (c["pix"] == p).sum() == 3
        back = RX.candidates(xy, z, faces[::-1].copy(), H0, W0, dtype, face_base=7)
        assert (back["face"][RX.zbuffer(back, H0 * W0)] == 7).all()


def test_unusable_triangles_are_dropped_and_counted():
    v = np.array([at(2, 2), at(10, 2), at(2, 10),                # 0-2: visible
                  [0.0, 0.0, -1.0], [0.0, 0.0, 0.0],              # 3, 4: behind the camera, in its plane
                  at(20000, 3), at(4, 4), at(6, 6), at(8, 8)],     # 5: beyond the guard band; 6-8: collinear
                 dtype=np.float32)
    xy, z, _ = RX.project(v, K0, R0, T0, np.float32)
    assert [int(x) for x in xy[[3, 4, 5], 0]] == [RX.SENTINEL] * 3 and (xy[[0, 1, 2, 6, 7, 8], 0] != RX.SENTINEL).all()
    faces = np.array([[0, 1, 2], [0, 1, 3], [4, 1, 2], [0, 5, 2], [6, 7, 8], [0, 0, 1], [0, 1, 99], [0, -1, 2]])
    per_face, dropped = RX.coverage(xy, faces, H0, W0)
    assert dropped == 7 and per_face[0].size > 0 and all(p.size == 0 for p in per_face[1:])
    assert RX.candidates(xy, z, faces, H0, W0, np.float32)["dropped"] == 7


def test_a_triangle_larger_than_the_frame_covers_every_pixel():
    v = np.array([at(-4000, -4000), at(9000, -4000), at(-4000, 9000)], dtype=np.float32)
    for H, W in ((16, 16), (5, 9)):
        total, dropped, _ = counts(v, np.array([[0, 1, 2]]), H, W)
        assert dropped == 0 and total.shape == (H, W) and (total == 1).all()


# ------------------------------------------------------------------------------------------ the analytic sphere
# Measured here (numpy 2.x, x86-64; fp64 restatement, 96 x 96 frame, `sphere_camera`): resolution 16 -> IoU 0.990588, depth MAE
# 3.0368e-3 on the pixels with |n . d| >= 0.5; resolution 32 -> IoU 0.996078, MAE 7.5064e-4.  The bounds are twice these (1 - IoU
# for the silhouette): the factor covers nothing but platform differences in numpy.
SPHERE_MEASURED = {16: (1.0 - 0.990588, 3.0368e-3), 32: (1.0 - 0.996078, 7.5064e-4)}


@pytest.fixture(scope="module")
def sphere_figures():
    H = W = 96
    K, R, T = RX.sphere_camera(H, W)
    hit, depth, facing = RX.sphere_truth(K, R, T, H, W)
    out = {}
    for n in (16, 32):
        v, f, nrm, _ = RX.sphere_mesh(n, np.float64)
        r = RX.rasterize(v, f, K, R, T, H, W, np.float64, normals=nrm)
        m = r["mask"] != 0
        sel = m & hit & (facing >= 0.5)              # grazing pixels have unbounded z error by geometry
        out[n] = {"iou": (m & hit).sum() / (m | hit).sum(), "mae": float(np.abs(r["depth"][sel] - depth[sel]).mean()), "mask": m.reshape(H, W),
                  "dropped": r["dropped"], "sel": int(sel.sum())}
        print(f"sphere at resolution {n}: IoU {out[n]['iou']:.6f}, depth MAE {out[n]['mae']:.4e} over {out[n]['sel']} pixels, dropped {r['dropped']}")
    return out


def test_sphere_silhouette_and_depth_improve_with_resolution(sphere_figures):
    a, b = sphere_figures[16], sphere_figures[32]
    assert b["iou"] > a["iou"] and b["mae"] < a["mae"]
    for n, fig in sphere_figures.items():
        miss, mae = SPHERE_MEASURED[n]
        assert fig["sel"] > 500 and 1.0 - fig["iou"] <= 2.0 * miss and fig["mae"] <= 2.0 * mae, (n, fig["iou"], fig["mae"])


def test_sphere_mask_rows_are_contiguous(sphere_figures):
    """A closed convex surface has no cracks: every covered row of the mask is one run."""
    for n, fig in sphere_figures.items():
        m = fig["mask"]
        rows = np.nonzero(m.any(1))[0]
        assert rows.size > 20 and np.array_equal(rows, np.arange(rows[0], rows[-1] + 1))
        for r in rows:
            cols = np.nonzero(m[r])[0]
            assert cols.size == cols[-1] - cols[0] + 1, (n, r)


def test_sphere_attributes_are_interpolated():
    """rgb / normal / shaded of the restatement on the sphere: the interpolated normal is the analytic one to the mesh's accuracy,
    the head-light shade follows it, and fp32 agrees with fp64 to rounding."""
    H, W = 48, 40
    K, R, T = RX.sphere_camera(H, W)
    v, f, nrm, col = RX.sphere_mesh(12, np.float32)
    r64 = RX.rasterize(v, f, K, R, T, H, W, np.float64, colors=col, normals=nrm)
    r32 = RX.rasterize(v, f, K, R, T, H, W, np.float32, colors=col, normals=nrm)
    m = r64["mask"] != 0
    assert np.array_equal(r32["mask"], r64["mask"]) and m.sum() > 200
    length = np.linalg.norm(r64["normal"][m], axis=1)
    assert np.abs(length - 1.0).max() < 1e-12 and (r64["normal"][~m] == 0).all() and (r64["rgb"][~m] == 1.0).all()
    hit, depth, facing = RX.sphere_truth(K, R, T, H, W)
    both = m & hit & (facing >= 0.5)                             # away from the rim, where a voxel of position error turns the normal
    shade = r64["shaded"][both] / r64["rgb"][both]
    assert both.sum() > 100 and np.abs(shade - (0.3 + 0.7 * facing[both, None])).max() < 0.05
    # the same fixed-point corners and depths in both precisions (a unit of xy moves a grazing depth by more than rounding does)
    xy, z, _ = RX.project(v, K, R, T, np.float32)
    both = {}
    for dtype in (np.float32, np.float64):
        c = RX.candidates(xy, z, f, H, W, dtype)
        both[dtype] = RX.resolve(c, RX.zbuffer(c, H * W), H, W, dtype, colors=col, normals=nrm, Kinv=np.linalg.inv(K), R=R)
    a32, a64 = both[np.float32], both[np.float64]
    agree = a32["face"] == a64["face"]
    assert np.array_equal(a32["mask"], a64["mask"]) and agree[a64["mask"] != 0].mean() > 0.99
    for k in ("depth", "rgb", "normal", "shaded"):
        assert np.abs(a32[k][agree].astype(np.float64) - a64[k][agree]).max() < 2e-6, k
    g = RX.rasterize(v, f, K, R, T, H, W, np.float64)                                       # no colours, no normals: white, geometric normals
    assert (g["rgb"] == 1.0).all() and (np.einsum("ij,ij->i", g["normal"][m], r64["normal"][m]) > 0.9).all()


# ------------------------------------------------------------------------------------------ fit
def test_fit_on_hand_made_maps():
    mask = np.array([1, 1, 1, 0, 0, 1, 0, 0], dtype=np.uint8)
    alpha = np.array([0.9, 0.6, 0.5, 0.7, 0.2, 1.0, 0.0, 0.51], dtype=np.float32)           # 0.5 is not > 0.5
    da = np.array([2.0, 3.0, 9.0, 9.0, 9.0, 1.5, 9.0, 9.0], dtype=np.float32)
    db = np.array([2.5, 2.0, 0.0, 1.0, 1.0, 1.5, 1.0, 1.0], dtype=np.float32)
    counts, sums = RX.fit(mask, da, alpha, db, 0.5)
    assert counts == [4, 5, 3] and sums == [1.5, 0.5, 1.25, 1.0]
    fig = RX.fit_figures(counts, sums)
    assert fig["iou"] == 3 / 6 and fig["area_mesh"] == 4.0 and fig["area_ref"] == 5.0
    assert fig["depth_mae"] == 0.5 and fig["depth_bias"] == 0.5 / 3 and fig["depth_rmse"] == np.sqrt(1.25 / 3) and fig["depth_max"] == 1.0
    counts, sums = RX.fit(mask, None, alpha, None, 0.5)                                      # the silhouette alone
    assert counts == [4, 5, 3] and sums == [0.0] * 4
    counts, sums = RX.fit(mask, da, 1.0 - mask.astype(np.float32), db, 0.5)                  # an empty intersection
    assert counts == [4, 4, 0] and sums == [0.0] * 4 and RX.fit_figures(counts, sums)["iou"] == 0.0
    counts, sums = RX.fit(np.zeros(0, np.uint8), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32))   # an empty frame
    assert counts == [0, 0, 0] and sums == [0.0] * 4
    fig = RX.fit_figures(counts, sums)
    assert fig["iou"] == 1.0 and all(np.isfinite(x) for x in fig.values())


def test_mesh_fit_keys():
    from hosnerf_amd import mesh
    assert mesh.FIT_KEYS == tuple(RX.fit_figures([0, 0, 0], [0.0] * 4))
    assert mesh.RASTER_MAPS == ("depth", "mask", "face", "rgb", "normal", "shaded")
    with pytest.raises(ValueError):                                                         # the last row of K must be (0,0,1)
        mesh.rasterize([], np.array([[64.0, 0, 8], [0, 64.0, 8], [0, 0.001, 1]]), np.eye(4), 16, 16)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """HOS_E_ARG (-1) / HOS_E_SHAPE (-3) on null pointers and impossible sizes, HOS_OK for V = 0 / F = 0: none of these reaches a
    launch, so the library answers without a GPU."""
    import ctypes
    from hosnerf_amd import _lib
    lib = _lib.load()
    for name in ("hos_mesh_project", "hos_raster_faces", "hos_raster_resolve", "hos_frame_fit", "hos_frame_fit_blocks"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert lib.hos_frame_fit_blocks() == 1024
    cam = (ctypes.c_float * 9)(*([1.0] * 9))
    p = ctypes.addressof(cam)                          # a non-null pointer: never dereferenced by a call that is refused
    assert lib.hos_mesh_project(0, 0, p, p, p, 1e-6, 0, 0, 0) == 0
    assert lib.hos_mesh_project(0, 5, p, p, p, 1e-6, p, p, 0) == -1 and lib.hos_mesh_project(p, 5, p, p, p, 1e-6, 0, p, 0) == -1
    assert lib.hos_mesh_project(p, 5, 0, p, p, 1e-6, p, p, 0) == -1 and lib.hos_mesh_project(p, -1, p, p, p, 1e-6, p, p, 0) == -1
    assert lib.hos_mesh_project(p, 5, p, p, p, -1.0, p, p, 0) == -1 and lib.hos_mesh_project(p, 5, p, p, p, float("nan"), p, p, 0) == -1
    assert lib.hos_mesh_project(p, 2 ** 31, p, p, p, 1e-6, p, p, 0) == -3
    assert lib.hos_raster_faces(p, p, 5, p, 0, 0, 4, 4, p, p, 0) == 0 and lib.hos_raster_faces(0, 0, 0, 0, 0, 0, 4, 4, p, p, 0) == 0
    assert lib.hos_raster_faces(p, p, 5, p, 3, 0, 4, 4, 0, p, 0) == -1 and lib.hos_raster_faces(p, p, 5, p, 3, 0, 4, 4, p, 0, 0) == -1
    assert lib.hos_raster_faces(p, p, 5, 0, 3, 0, 4, 4, p, p, 0) == -1 and lib.hos_raster_faces(0, p, 5, p, 3, 0, 4, 4, p, p, 0) == -1
    assert lib.hos_raster_faces(p, p, 5, p, 3, -1, 4, 4, p, p, 0) == -1 and lib.hos_raster_faces(p, p, 5, p, -3, 0, 4, 4, p, p, 0) == -1
    assert lib.hos_raster_faces(p, p, 5, p, 3, 0, 0, 4, p, p, 0) == -3 and lib.hos_raster_faces(p, p, 5, p, 3, 0, 65536, 65536, p, p, 0) == -3
    assert lib.hos_raster_faces(p, p, 5, p, 5000, 2 ** 31 - 1000, 4, 4, p, p, 0) == -3           # ids past int32
    res = lambda **kw: lib.hos_raster_resolve(*[kw.get(k, d) for k, d in (
        ("zbuf", p), ("xy", p), ("z", p), ("V", 5), ("faces", p), ("F", 3), ("base", 0), ("vertices", p), ("colors", 0), ("normals", 0), ("Kinv", p),
        ("R", p), ("bg", p), ("H", 4), ("W", 4), ("face", p), ("depth", p), ("mask", p), ("rgb", p), ("normal", p), ("shaded", p), ("stream", 0))])
    assert res(F=0) == 0 and res(V=0) == 0
    assert res(zbuf=0) == -1 and res(bg=0) == -1 and res(faces=0) == -1 and res(xy=0) == -1 and res(base=-1) == -1
    assert res(face=0, depth=0, mask=0, rgb=0, normal=0, shaded=0) == -1                         # nothing asked for
    assert res(vertices=0) == -1 and res(Kinv=0) == -1                                           # geometric normals need positions, shading the camera
    assert res(H=0) == -3 and res(F=5000, base=2 ** 31 - 1000) == -3
    assert lib.hos_frame_fit(p, p, p, p, 0.5, -1, p, p, p, 0) == -1 and lib.hos_frame_fit(p, p, p, p, 0.5, 8, 0, p, p, 0) == -1
    assert lib.hos_frame_fit(p, p, p, p, 0.5, 8, p, 0, p, 0) == -1 and lib.hos_frame_fit(0, p, p, p, 0.5, 8, p, p, p, 0) == -1
    assert lib.hos_frame_fit(p, p, p, 0, 0.5, 8, p, p, p, 0) == -1 and lib.hos_frame_fit(p, p, p, p, float("nan"), 8, p, p, p, 0) == -1


# ------------------------------------------------------------------------------------------ files
def test_save_mesh_maps_writes_five_files():
    from PIL import Image
    from hosnerf_amd.freeview import MESH_MAP_FILES, save_mesh_maps
    H, W = 12, 10
    K, R, T = RX.sphere_camera(H, W)
    v, f, nrm, col = RX.sphere_mesh(8, np.float32)
    r = RX.rasterize(v, f, K, R, T, H, W, np.float32, colors=col, normals=nrm)
    d = tempfile.mkdtemp()
    paths = save_mesh_maps(d, "frame_000003", r, H, W)
    assert sorted(os.listdir(d)) == sorted("frame_000003" + k for k in MESH_MAP_FILES)
    assert MESH_MAP_FILES == ("_mesh.png", "_mesh_normal.png", "_mesh_mask.png", "_mesh_depth.npy", "_mesh_depth.png")
    assert sorted(paths) == sorted(MESH_MAP_FILES)
    m = r["mask"].reshape(H, W) != 0
    assert m.any() and not m.all()
    for kind, mode in (("_mesh.png", "RGB"), ("_mesh_normal.png", "RGB"), ("_mesh_mask.png", "L"), ("_mesh_depth.png", "L")):
        img = Image.open(paths[kind])
        assert img.size == (W, H) and img.mode == mode, kind
    assert np.array_equal(np.asarray(Image.open(paths["_mesh_mask.png"])) == 255, m)
    depth = np.load(paths["_mesh_depth.npy"])
    assert depth.dtype == np.float32 and depth.shape == (H, W) and (depth[~m] == 0).all() and (depth[m] > 0).all()
    assert (np.asarray(Image.open(paths["_mesh_depth.png"]))[~m] == 0).all()
    assert (np.asarray(Image.open(paths["_mesh_normal.png"]))[~m] == 128).all() and (np.asarray(Image.open(paths["_mesh.png"]))[~m] == 255).all()
    empty = {"shaded": np.ones((H * W, 3), np.float32), "normal": np.zeros((H * W, 3), np.float32), "mask": np.zeros(H * W, np.uint8),
             "depth": np.zeros(H * W, np.float32)}
    save_mesh_maps(d, "empty", empty, H, W)                                                  # a frame the mesh misses: still five files
    assert (np.asarray(Image.open(os.path.join(d, "empty_mesh_depth.png"))) == 0).all()


# ------------------------------------------------------------------------------------------ the launcher's arguments
def launch(*bindings, gin="hosnerf_backpack.gin"):
    import run as launcher
    argv = ["--ginc", os.path.join(ROOT, "configs", gin), "--scene_name", "Backpack", "--cpu", "--logbase", tempfile.mkdtemp(), "--ginb", "run.max_steps=3"]
    for b in bindings:
        argv += ["--ginb", b]
    return launcher.main(argv)


def test_launcher_bindings_and_refusals():
    import run as launcher
    for gin in ("hosnerf_backpack.gin", "state_humanobject_backpack.gin"):
        plan = launch("run.run_mesh_frames=True", "run.mesh_preview=True", "run.mesh_level_sweep=(0.1, 0.3, 0.5)", gin=gin)
        assert plan["gin"]["run.mesh_preview"] is True and tuple(plan["gin"]["run.mesh_level_sweep"]) == (0.1, 0.3, 0.5)
    with pytest.raises(SystemExit) as e:                                                    # the preview is of the frame meshes
        launch("run.mesh_preview=True")
    assert "run.mesh_preview" in str(e.value) and "run.run_mesh_frames" in str(e.value)
    for bad in ("0.5", "(0.1, 1e999)", '("a",)', "(True,)"):
        with pytest.raises(SystemExit) as e:
            launch("run.run_mesh_frames=True", "run.mesh_preview=True", f"run.mesh_level_sweep={bad}")
        assert "run.mesh_level_sweep" in str(e.value), bad
    with pytest.raises(SystemExit) as e:                                                    # a sweep needs the preview's render
        launch("run.run_mesh_frames=True", "run.mesh_level_sweep=(0.1, 0.3)")
    assert "run.mesh_level_sweep" in str(e.value) and "run.mesh_preview" in str(e.value)
    assert launcher.mesh_level_sweep({}) == () and launcher.mesh_level_sweep({"mesh_preview": True, "mesh_level_sweep": (0.25, 1)}) == (0.25, 1.0)
    plan = launch("run.run_mesh_frames=True")                                               # without the switch: as before
    assert "run.mesh_preview" not in plan["gin"]
    assert "run.mesh_preview" in launcher.__doc__
