"""Mesh components without a GPU: the numpy restatement tests/_components_expect.py on meshes whose components are known (it must be
right before the kernels are judged by it), the host simulation of the kernels' rounds against union-find, the argument checks of
`mesh.components` / `mesh.drop_floaters` / the `ops` wrappers / the C entry points, and the `run.mesh_min_component` binding."""
import ctypes
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _components_expect as cx
import _mesh_expect as mx


def component_mesh(v, f, comp, c):
    """Component c on its own: (vertices, faces renumbered)."""
    keep = np.zeros(comp["count"], dtype=np.uint8)
    keep[c] = 1
    return cx.compact(keep, comp["component"], comp["face_component"], v, f)[:2]


# ------------------------------------------------------------------------------------------ the restatement on known meshes
@pytest.mark.parametrize("name", list(cx.MARCHED))
def test_marched_meshes_have_the_known_components(name):
    _, _, V, F, C = cx.MARCHED[name]
    v, f = cx.marched(name)
    comp = cx.components(v, f)
    assert (v.shape[0], f.shape[0], comp["count"], comp["invalid_faces"]) == (V, F, C, 0)
    assert int(comp["n_vertices"].sum()) == V and int(comp["n_faces"].sum()) == F
    for c in range(C):                                     # every component is a closed oriented surface of its own
        cv, cf = component_mesh(v, f, comp, c)
        assert (cv.shape[0], cf.shape[0]) == (comp["n_vertices"][c], comp["n_faces"][c])
        assert mx.is_closed_oriented_manifold(cf, cv.shape[0])
        assert abs(mx.signed_volume(cv, cf) - comp["volume"][c]) <= 1e-12 and abs(mx.area(cv, cf) - comp["area"][c]) <= 1e-12
    assert abs(comp["volume"].sum() - mx.signed_volume(v, f)) <= 1e-12 and abs(comp["area"].sum() - mx.area(v, f)) <= 1e-12
    # label = the smallest vertex id of the component; dense ids ascend with it
    for c in range(C):
        members = np.flatnonzero(comp["component"] == c)
        assert (comp["label"][members] == members.min()).all()
    roots = np.unique(comp["label"])
    assert np.array_equal(comp["component"], np.searchsorted(roots, comp["label"]))


def test_two_spheres_torus_and_shell():
    v, f = cx.marched("two_spheres")
    assert (cx.components(v, f)["volume"] > 0).all()
    v, f = cx.marched("torus")
    assert mx.euler_characteristic(f, v.shape[0]) == 0
    v, f = cx.marched("shell")
    vol = cx.components(v, f)["volume"]
    assert abs(vol[0] - 0.3042) < 5e-5 and abs(vol[1] + 0.0306) < 5e-5                 # the outer wall and the wall of the hollow


def test_subject_and_floaters():
    v, f = cx.marched("floaters")
    comp = cx.components(v, f)
    assert tuple(comp["n_faces"]) == cx.FLOATER_FACES
    ratio = comp["area"] / comp["area"].max()
    assert np.abs(ratio - np.array(cx.FLOATER_AREA_RATIO)).max() < 5e-5
    for c in range(6):
        cv, cf = component_mesh(v, f, comp, c)
        assert mx.euler_characteristic(cf, cv.shape[0]) == 2
    for (r, n), kept in cx.KEEP_SETS:
        keep = cx.keep_rule(comp["n_faces"], comp["area"], r, n)
        assert int(keep.sum()) == kept
        # a threshold is at least 15 % away from every ratio it decides on (1.0 meets the largest component's own ratio, exactly 1)
        assert (np.abs(ratio[ratio < 1.0] / max(r, 1e-300) - 1.0) >= 0.15).all()
        kv, kf, _, _ = cx.compact(keep, comp["component"], comp["face_component"], v, f)
        assert mx.is_closed_oriented_manifold(kf, kv.shape[0])
        assert abs(mx.signed_volume(kv, kf) - comp["volume"][keep != 0].sum()) <= 1e-12
        assert kv.shape[0] == comp["n_vertices"][keep != 0].sum() and kf.shape[0] == comp["n_faces"][keep != 0].sum()
    # with the float64 vertices of the marching restatement: the figure of the issue
    o, h, _, P = mx.unit_box_grid(16)
    v64, _, f64 = mx.march(cx.field_floaters(P), 0.0, o, h)
    c64 = cx.components(v64, f64)
    assert abs(c64["volume"].sum() - 0.11596006696511493) < 1e-15 * 8 and abs(mx.signed_volume(v64, f64) - 0.11596006696511492) < 1e-15 * 8


def test_permuting_ids_or_shuffling_faces_keeps_the_partition():
    for name in cx.MARCHED:
        v, f = cx.marched(name)
        base = cx.components(v, f)
        pv, pf = cx.permuted(v, f, seed=1)
        p = np.random.default_rng(1).permutation(v.shape[0])
        perm = cx.components(pv, pf)
        assert perm["count"] == base["count"]
        assert np.array_equal(np.sort(perm["n_faces"]), np.sort(base["n_faces"]))
        a, b = base["component"], perm["component"][p]      # the same partition under other names
        assert len(set(zip(a.tolist(), b.tolist()))) == base["count"]
        shuf = cx.components(v, cx.shuffled_faces(f, seed=1))
        assert np.array_equal(shuf["label"], base["label"]) and np.array_equal(shuf["n_faces"], base["n_faces"])
        assert np.abs(shuf["volume"] - base["volume"]).max() <= 1e-14


def test_hand_cases():
    hc = cx.hand_cases()
    want = {   # name: (label, component, count, invalid, face_component, n_vertices, n_faces)
        "no_faces": ([0, 1, 2, 3, 4], [0, 1, 2, 3, 4], 5, 0, [], [1] * 5, [0] * 5),
        "no_vertices": ([], [], 0, 0, [], [], []),
        "unreferenced_vertex": ([0, 0, 0, 3, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0], 2, 0, [0, 0, 0], [6, 1], [3, 0]),
        "repeated_corner": ([0, 1, 0, 0, 1, 5], [0, 1, 0, 0, 1, 2], 3, 0, [1, 0, 2], [3, 2, 1], [1, 1, 1]),
        "duplicated_face": ([0, 0, 0, 3, 3, 3], [0, 0, 0, 1, 1, 1], 2, 0, [1, 1, 0, 1], [3, 3], [1, 3]),
        "out_of_range": ([0, 0, 0, 3, 4, 4, 4, 4], [0, 0, 0, 1, 2, 2, 2, 2], 3, 2, [0, -1, 2, -1, 2], [3, 1, 4], [1, 0, 2]),
    }
    assert set(hc) == set(want)
    for name, (v, f) in hc.items():
        c = cx.components(v, f)
        got = (c["label"].tolist(), c["component"].tolist(), c["count"], c["invalid_faces"], c["face_component"].tolist(),
               c["n_vertices"].tolist(), c["n_faces"].tolist())
        assert got == want[name], name
    v, f = hc["out_of_range"]
    c = cx.components(v, f)
    kv, kf, _, _ = cx.compact(np.array([1, 1, 1], dtype=np.uint8), c["component"], c["face_component"], v, f)
    assert kv.shape[0] == 8 and kf.tolist() == [[0, 1, 2], [4, 5, 6], [7, 6, 5]]          # an invalid face is never kept
    kv, kf, _, _ = cx.compact(np.array([0, 1, 1], dtype=np.uint8), c["component"], c["face_component"], v, f)
    assert np.array_equal(kv, v[3:]) and kf.tolist() == [[1, 2, 3], [4, 3, 2]]


STRIPS = [(4099, "order"), (4099, "reversed"), (4099, "permuted"), (1, "order"), (63, "order")]


def test_the_kernels_rounds_reach_union_find_under_the_stalest_reads():
    """hook + 2 jumps with every read taken from the state at the start of its launch: the labels are union-find's, within V + 2 rounds."""
    cases = [(n, cx.marched(n)) for n in cx.MARCHED]
    cases += [(n + "/permuted", cx.permuted(*cx.marched(n))) for n in cx.MARCHED]
    cases += [(n + "/shuffled", (cx.marched(n)[0], cx.shuffled_faces(cx.marched(n)[1]))) for n in cx.MARCHED]
    cases += [(f"strip{n}/{num}", cx.strip(n, num)) for n, num in STRIPS] + list(cx.hand_cases().items())
    rounds = {}
    for name, (v, f) in cases:
        want, _ = cx.labels(f, v.shape[0])
        got, rounds[name] = cx.simulate_rounds(f, v.shape[0])
        assert np.array_equal(got, want), name
        assert rounds[name] <= v.shape[0] + 2
    print(rounds)


# ------------------------------------------------------------------------------------------ argument checks
def test_mesh_level_argument_checks():
    from hosnerf_amd import mesh
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    for bad_v, bad_f in ((v.double(), f), (torch.zeros(4, 2), f), (v, f.long()), (v, torch.zeros(2, 4, dtype=torch.int32)), (v.numpy(), f)):
        with pytest.raises(ValueError):
            mesh.components(bad_v, bad_f)
    m = {"vertices": v, "faces": f, "colors": None, "normals": None}
    assert mesh.drop_floaters(m) is m and mesh.drop_floaters(m, 0.0, 0) is m          # both thresholds 0: the same object, no launch
    for kw in ({"min_area_ratio": -0.1}, {"min_area_ratio": 1.5}, {"min_area_ratio": float("nan")}, {"min_faces": -1}, {"min_faces": 2.5}):
        with pytest.raises(ValueError):
            mesh.drop_floaters(m, **kw)
    with pytest.raises(ValueError):
        mesh.drop_floaters({**m, "faces": f.long()}, min_area_ratio=0.5)
    for fn in (mesh.extract, mesh.extract_frame, mesh.extract_bkgd):                   # refused before any field is evaluated
        with pytest.raises(ValueError):
            fn(None, None, 0.5, min_area_ratio=2.0)
    comp = {"area": torch.tensor([1.0, 0.04, 0.5], dtype=torch.float64), "n_faces": torch.tensor([100, 40, 8])}
    assert mesh.keep_flags(comp, 0.05, 0).tolist() == [1, 0, 1] and mesh.keep_flags(comp, 0.0, 10).tolist() == [1, 1, 0]
    assert mesh.keep_flags(comp, 1.0, 0).tolist() == [1, 0, 0] and mesh.keep_flags(comp).dtype == torch.uint8
    for text in ("mesh components", "floaters", "smallest vertex id", "negative volume", "min_area_ratio", "before the colour query"):
        assert text in mesh.__doc__.lower().replace("\n", " "), text


def test_ops_argument_checks():
    from hosnerf_amd import _lib, ops
    E = _lib.HosLibraryError
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    comp, fc, keep = torch.zeros(4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.ones(1, dtype=torch.uint8)
    for bad in (f.long(), torch.zeros(2, 2, dtype=torch.int32), torch.zeros(6, dtype=torch.int32), None):
        with pytest.raises(E):
            ops.mesh_label(bad, 4)
    for V in (-1, 2 ** 31 - 256):
        with pytest.raises(E):
            ops.mesh_label(f, V)
    with pytest.raises(E):                                 # a device op: host tensors are refused, there is no CPU path
        ops.mesh_label(f, 4)
    # empty inputs: empty tensors without a launch (this runs where there is no GPU)
    label, component, count, rounds, invalid = ops.mesh_label(torch.zeros(0, 3, dtype=torch.int32), 0)
    assert (label.shape, component.shape, label.dtype, count, rounds, invalid) == ((0,), (0,), torch.int32, 0, 0, 0)
    assert ops.mesh_label(f, 0)[4] == 2                   # without a vertex every face is out of range
    for args in ((torch.zeros(4, 2), f, comp, 1), (v, f.long(), comp, 1), (v, f, comp.long(), 1), (v, f, comp[:3], 1), (v, f, comp, 5), (v, f, comp, -1)):
        with pytest.raises(E):
            ops.mesh_component_measures(*args)
    fc0, nv, nf, area, vol = ops.mesh_component_measures(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 0)
    assert (fc0.shape, nv.dtype, nf.shape, area.dtype, vol.shape) == ((0,), torch.int64, (0,), torch.float64, (0,))
    good = dict(keep=keep, component=comp, face_component=fc, vertices=v, faces=f)
    for k, bad in (("keep", keep.bool()), ("keep", torch.ones(5, dtype=torch.uint8)), ("component", comp.long()), ("component", comp[:2]),
                   ("face_component", fc[:1]), ("vertices", torch.zeros(4, 2)), ("faces", f.long()), ("colors", torch.zeros(4, 3)),
                   ("colors", torch.zeros(3, 3, dtype=torch.uint8)), ("normals", torch.zeros(4, 3, dtype=torch.float64))):
        with pytest.raises(E):
            ops.mesh_compact(**{**good, k: bad})
    z = torch.zeros(0, dtype=torch.int32)
    ov, of, oc, on = ops.mesh_compact(torch.zeros(0, dtype=torch.uint8), z, z, torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32),
                                      colors=torch.zeros(0, 3, dtype=torch.uint8))
    assert (ov.shape, of.shape, of.dtype, oc.shape, oc.dtype, on) == ((0, 3), (0, 3), torch.int32, (0, 3), torch.uint8, None)


def test_entry_points_validate_without_gpu():
    """HOS_E_ARG (-1) / HOS_E_SHAPE (-3) on null, negative and oversized arguments, 0 on V = 0 -- all before any launch."""
    from hosnerf_amd import _lib
    lib = _lib.load()
    counts = {"hos_mesh_blocks": 1, "hos_mesh_label_begin": 4, "hos_mesh_label_round": 7, "hos_mesh_component_ids": 6,
              "hos_mesh_component_terms": 11, "hos_mesh_component_sums": 9, "hos_mesh_compact_count": 10, "hos_mesh_compact_write": 19}
    for name, n in counts.items():
        assert name in _lib.PROTOTYPES and hasattr(lib, name) and len(_lib.PROTOTYPES[name]) == n, name
    assert lib.hos_version() == 101                        # an added entry point leaves the ABI revision alone
    buf = (ctypes.c_int64 * 16)()
    a, big = ctypes.addressof(buf), 2 ** 31 - 256
    assert lib.hos_mesh_blocks(0) == 0 and lib.hos_mesh_blocks(1) == 1 and lib.hos_mesh_blocks(256) == 1 and lib.hos_mesh_blocks(4101) == 17
    assert lib.hos_mesh_blocks(-1) == -1 and lib.hos_mesh_blocks(big) == -3 and lib.hos_mesh_blocks(big - 1) == (big - 1 + 255) // 256

    def sweep(fn, names, base, pointers, negative, oversized, shape=()):
        call = lambda **kw: fn(*[{**base, **kw}[n] for n in names], 0)
        for k in pointers:
            assert call(**{k: 0}) == -1, (fn.__name__, k)
        for k in negative:
            assert call(**{k: -1}) == -1, (fn.__name__, k)
        for k in oversized:
            assert call(**{k: big}) == -3, (fn.__name__, k)
        for kw in shape:
            assert call(**kw) == -3, (fn.__name__, kw)
        return call

    begin = sweep(lib.hos_mesh_label_begin, ("V", "label", "words"), dict(V=5, label=a, words=a), ("label", "words"), ("V",), ("V",))
    assert begin(V=0) == 0 and begin(V=0, label=0, words=0) == 0
    rnd = sweep(lib.hos_mesh_label_round, ("faces", "F", "V", "round", "label", "words"), dict(faces=a, F=3, V=5, round=0, label=a, words=a),
                ("faces", "label", "words"), ("F", "V", "round"), ("F", "V"))
    assert rnd(V=0) == 0 and rnd(F=0) == 0                 # nothing to launch
    ids = sweep(lib.hos_mesh_component_ids, ("label", "V", "component", "ws", "words"), dict(label=a, V=5, component=a, ws=a, words=a),
                ("label", "component", "ws", "words"), ("V",), ("V",))
    assert ids(V=0) == 0
    terms = sweep(lib.hos_mesh_component_terms, ("vertices", "faces", "component", "V", "F", "C", "fc", "terms", "nv", "nf"),
                  dict(vertices=a, faces=a, component=a, V=5, F=3, C=2, fc=a, terms=a, nv=a, nf=a),
                  ("vertices", "faces", "component", "fc", "terms", "nv", "nf"), ("V", "F", "C"), ("V", "F"), shape=(dict(C=6),))
    assert terms(V=0, C=0) == 0 and terms(C=0) == 0
    sums = sweep(lib.hos_mesh_component_sums, ("terms", "order", "start", "nf", "F", "C", "area", "volume"),
                 dict(terms=a, order=a, start=a, nf=a, F=3, C=2, area=a, volume=a), ("terms", "order", "start", "nf", "area", "volume"),
                 ("F", "C"), ("F",))
    assert sums(C=0) == 0
    cnt = sweep(lib.hos_mesh_compact_count, ("keep", "C", "component", "V", "faces", "fc", "F", "ws", "counts"),
                dict(keep=a, C=2, component=a, V=5, faces=a, fc=a, F=3, ws=a, counts=a), ("keep", "component", "faces", "fc", "ws", "counts"),
                ("C", "V", "F"), ("V", "F"), shape=(dict(C=6),))
    assert cnt(V=0, C=0) == 0 and cnt(C=0) == -1
    names = ("keep", "C", "component", "V", "faces", "fc", "F", "ws", "new_id", "vertices", "colors", "normals", "Vout", "Fout", "ov", "oc", "on", "of")
    base = dict(keep=a, C=2, component=a, V=5, faces=a, fc=a, F=3, ws=a, new_id=a, vertices=a, colors=a, normals=a, Vout=4, Fout=2, ov=a, oc=a,
                on=a, of=a)
    wr = sweep(lib.hos_mesh_compact_write, names, base, ("keep", "component", "faces", "fc", "ws", "new_id", "vertices", "ov", "of", "colors", "oc",
                                                          "normals", "on"), ("C", "V", "F", "Vout", "Fout"), (), shape=(dict(C=6),))
    assert wr(Vout=6) == -1 and wr(Fout=4) == -1           # more rows out than in
    assert wr(V=big, Vout=0) == -3 and wr(F=big) == -3
    assert wr(V=0, Vout=0, C=0) == 0 and wr(Vout=0, Fout=0) == 0


# ------------------------------------------------------------------------------------------ the launcher's binding
def test_mesh_min_component_parsing_and_refusal():
    import run as launcher
    assert launcher.mesh_min_component({}) == 0.0 and launcher.floater_kwargs({}) == {} and launcher.floater_kwargs({"mesh_min_component": 0}) == {}
    assert launcher.mesh_min_component({"mesh_min_component": 1}) == 1.0
    assert launcher.floater_kwargs({"mesh_min_component": 0.05}) == {"min_area_ratio": 0.05}
    for bad in (-0.01, 1.01, float("nan"), "0.1", True, None, (0.1,)):
        with pytest.raises(SystemExit) as e:
            launcher.mesh_min_component({"mesh_min_component": bad})
        assert str(e.value).startswith(f"run.mesh_min_component = {bad!r}: a number in [0, 1]")
    gin = os.path.join(ROOT, "configs", "hosnerf_backpack.gin")
    plan = launcher.main(["--ginc", gin, "--scene_name", "Backpack", "--cpu", "--logbase", tempfile.mkdtemp(), "--ginb", "run.max_steps=3",
                          "--ginb", "run.run_mesh=True", "--ginb", "run.mesh_min_component=0.05"])
    assert plan["gin"]["run.mesh_min_component"] == 0.05
    with pytest.raises(SystemExit) as e:                   # refused before anything is trained
        launcher.main(["--ginc", gin, "--scene_name", "Backpack", "--cpu", "--logbase", tempfile.mkdtemp(), "--ginb", "run.max_steps=3",
                       "--ginb", "run.mesh_min_component=1.5"])
    assert "run.mesh_min_component" in str(e.value)
    assert "run.mesh_min_component" in launcher.__doc__ and "unfiltered" in launcher.mesh_level_sweep.__doc__.lower()
