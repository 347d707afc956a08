"""Mesh components on the GPU (hos_components.hip): `ops.mesh_label` / `mesh_component_measures` / `mesh_compact` and
`mesh.components` / `drop_floaters` against the numpy restatement tests/_components_expect.py (whose own properties
tests/test_components_cpu.py checks), the extractors' thresholds, and the launcher's `run.mesh_min_component`.

Labels, dense ids, counts and the compacted mesh are exact (`torch.equal`).  The float64 sums per component: the per-face terms are
the same doubles on both sides, only the order of summation differs, so |hip - restatement| <= F * 2^-52 * sum |terms| per component
(F additions, each rounding a partial sum no larger than sum |terms| by at most 2^-53 relative, on either side); two runs are bit-equal."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _components_expect as cx
import _mesh_expect as mx
from hosnerf_amd import formats, synth, tpose

ROUNDS = {}                                  # case -> rounds the labelling took on the GPU, written to profiles/components_parity.json


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


@pytest.fixture(scope="module", autouse=True)
def record_rounds():
    yield
    if ROUNDS:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "components_parity.json"), "w") as f:
            json.dump({"what": "rounds of hook + 2 jumps `ops.mesh_label` took on the GPU per case of tests/test_gpu_components.py (the last "
                               "round changes nothing), next to the host simulation with the stalest reads and the cap V + 2",
                       "cases": ROUNDS}, f, indent=1)


def cases():
    out = [(n, cx.marched(n)) for n in cx.MARCHED]
    out += [(n + "/permuted", cx.permuted(*cx.marched(n), seed=1)) for n in cx.MARCHED]
    out += [(n + "/shuffled", (cx.marched(n)[0], cx.shuffled_faces(cx.marched(n)[1], seed=1))) for n in cx.MARCHED]
    out += [(f"strip{n}/{num}", cx.strip(n, num)) for n, num in ((4099, "order"), (4099, "reversed"), (4099, "permuted"), (1, "order"), (63, "order"))]
    return out + list(cx.hand_cases().items())


CASES = cases()
_expect = {}


def expect(name):
    """The restatement of a case, computed once and shared."""
    if name not in _expect:
        v, f = dict(CASES)[name]
        _expect[name] = cx.components(v, f)
    return _expect[name]


def on_device(dev, v, f):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32)).to(dev)


def term_bound(want, which):
    """F * 2^-52 * sum |terms| per component (module docstring)."""
    terms = np.abs(want["terms"][which])
    fc = want["face_component"]
    C = want["count"]
    s = np.zeros(C)
    np.add.at(s, fc[fc >= 0], terms[fc >= 0])
    return np.maximum(want["n_faces"], 1) * 2.0 ** -52 * s


# ------------------------------------------------------------------------------------------ 1, 2: labels, ids, counts, sums
@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_components_equal_the_restatement(dev, name):
    from hosnerf_amd import mesh
    v, f = dict(CASES)[name]
    want = expect(name)
    dv, df = on_device(dev, v, f)
    got = mesh.components(dv, df)
    V = v.shape[0]
    ROUNDS[name] = {"V": V, "F": int(f.shape[0]), "components": want["count"], "rounds": got["rounds"],
                    "rounds_simulated_stalest_reads": cx.simulate_rounds(f, V)[1], "cap": V + 2}
    print(name, ROUNDS[name])
    assert got["rounds"] <= V + 2
    assert got["count"] == want["count"] and got["invalid_faces"] == want["invalid_faces"]
    for k, dtype in (("label", torch.int32), ("component", torch.int32), ("face_component", torch.int32), ("n_vertices", torch.int64),
                     ("n_faces", torch.int64)):
        assert got[k].dtype == dtype and torch.equal(got[k].cpu(), torch.from_numpy(want[k])), (name, k)
    for which, k in enumerate(("area", "volume")):
        assert got[k].dtype == torch.float64 and got[k].shape == (want["count"],)
        err = np.abs(got[k].cpu().numpy() - want[k])
        bound = term_bound(want, which)
        print(f"  {k}: max |hip - restatement| {err.max() if err.size else 0.0:.3e}, bound {bound.max() if bound.size else 0.0:.3e}")
        assert (err <= bound).all(), (name, k, err, bound)
    again = mesh.components(dv, df)                        # two runs are bit-equal
    for k in ("label", "component", "face_component", "n_vertices", "n_faces", "area", "volume"):
        assert torch.equal(again[k], got[k]), (name, k)


# ------------------------------------------------------------------------------------------ 3: compaction
@pytest.mark.parametrize("name", ["floaters", "floaters/permuted", "shell", "out_of_range", "unreferenced_vertex", "no_faces"])
def test_compact_equals_the_restatement(dev, name):
    from hosnerf_amd import ops
    v, f = dict(CASES)[name]
    want = expect(name)
    C, V = want["count"], v.shape[0]
    rng = np.random.default_rng(3)
    colors = rng.integers(0, 256, (V, 3), dtype=np.uint8)
    normals = rng.standard_normal((V, 3)).astype(np.float32)
    keeps = [cx.keep_rule(want["n_faces"], want["area"], r, n) for (r, n), _ in cx.KEEP_SETS]
    keeps += [np.ones(C, dtype=np.uint8), np.zeros(C, dtype=np.uint8), (np.arange(C) % 2).astype(np.uint8)]
    if name == "floaters":
        assert [int(k.sum()) for k in keeps[:3]] == [kept for _, kept in cx.KEEP_SETS]
    dv, df = on_device(dev, v, f)
    dc, dn = torch.from_numpy(colors).to(dev), torch.from_numpy(normals).to(dev)
    comp, fc = torch.from_numpy(want["component"]).to(dev), torch.from_numpy(want["face_component"]).to(dev)
    for keep in keeps:
        wv, wf, wc, wn = cx.compact(keep, want["component"], want["face_component"], v, f, colors, normals)
        gv, gf, gc, gn = ops.mesh_compact(torch.from_numpy(keep).to(dev), comp, fc, dv, df, dc, dn)
        assert gv.dtype == torch.float32 and gf.dtype == torch.int32 and gc.dtype == torch.uint8 and gn.dtype == torch.float32
        for g, w in ((gv, wv), (gf, wf), (gc, wc), (gn, wn)):
            assert g.shape == w.shape and torch.equal(g.cpu(), torch.from_numpy(np.ascontiguousarray(w))), (name, keep)
        bare = ops.mesh_compact(torch.from_numpy(keep).to(dev), comp, fc, dv, df)              # colours and normals may be absent
        assert bare[2] is None and bare[3] is None and torch.equal(bare[0], gv) and torch.equal(bare[1], gf)
        only_n = ops.mesh_compact(torch.from_numpy(keep).to(dev), comp, fc, dv, df, None, dn)
        assert only_n[2] is None and torch.equal(only_n[3], gn)


# ------------------------------------------------------------------------------------------ 4: drop_floaters
def test_drop_floaters_on_the_subject_and_floaters(dev):
    from hosnerf_amd import mesh
    v, f = cx.marched("floaters")
    want = expect("floaters")
    dv, df = on_device(dev, v, f)
    colors = (dv * 255.0).clamp(0, 255).to(torch.uint8)
    body = {"vertices": dv * 2.0, "faces": df, "colors": colors, "normals": None}
    field = torch.zeros(2, 2, 2, device=dev)
    m = {"vertices": dv, "faces": df, "colors": colors, "normals": dv.clone(), "volume": 1.0, "area": 2.0, "state": 1, "alpha": field,
         "rgb": field, "body": body}
    assert mesh.drop_floaters(m) is m and mesh.drop_floaters(m, 0.0, 0) is m
    for (r, n), kept in cx.KEEP_SETS:
        out = mesh.drop_floaters(m, min_area_ratio=r, min_faces=n)
        keep = cx.keep_rule(want["n_faces"], want["area"], r, n)
        wv, wf, _, _ = cx.compact(keep, want["component"], want["face_component"], v, f)
        assert out is not m and m["vertices"] is dv and "components" not in m
        assert torch.equal(out["vertices"].cpu(), torch.from_numpy(wv)) and torch.equal(out["faces"].cpu(), torch.from_numpy(wf))
        assert torch.equal(out["normals"], out["vertices"]) and torch.equal(out["colors"], (out["vertices"] * 255.0).clamp(0, 255).to(torch.uint8))
        assert torch.equal(out["body"]["vertices"], out["vertices"] * 2.0) and torch.equal(out["body"]["faces"], out["faces"])
        assert out["alpha"] is field and out["rgb"] is field and out["state"] == 1              # the field passes through untouched
        gone = keep == 0
        c = out["components"]
        assert (c["count"], c["kept"], c["V_dropped"], c["F_dropped"]) == (6, kept, int(want["n_vertices"][gone].sum()), int(want["n_faces"][gone].sum()))
        assert c["invalid_faces"] == 0 and c["negative_volume"] == 0 and 1 <= c["rounds"] <= v.shape[0] + 2
        assert abs(c["area_dropped"] - want["area"][gone].sum()) <= 1e-12 and abs(c["volume_dropped"] - want["volume"][gone].sum()) <= 1e-12
        gf = out["faces"].cpu().numpy()
        assert mx.is_closed_oriented_manifold(gf, out["vertices"].shape[0])
        assert abs(out["volume"] - want["volume"][keep != 0].sum()) <= 1e-12 and abs(out["area"] - want["area"][keep != 0].sum()) <= 1e-12
    hollow = mesh.drop_floaters({"vertices": on_device(dev, *cx.marched("shell"))[0], "faces": on_device(dev, *cx.marched("shell"))[1],
                                 "colors": None, "normals": None}, min_faces=1)
    assert hollow["components"]["negative_volume"] == 1 and hollow["components"]["kept"] == 2      # the hollow's wall: a component like any other


def basedir():
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    return d


def gap_ratio(area):
    """A `min_area_ratio` in the middle of the widest gap (in the logarithm) between the components' area ratios: no rounding flips it."""
    r = np.sort(np.asarray(area) / np.max(area))
    r = r[r > 0]
    i = int(np.argmax(np.log(r[1:]) - np.log(r[:-1])))
    return float(np.sqrt(r[i] * r[i + 1]))


def test_drop_floaters_on_an_extracted_mesh(dev):
    """`mesh.extract` of the synthetic stage-2 network at resolution 16, at a level picked on the CPU (restatement) for its several components."""
    from hosnerf_amd import mesh
    from hosnerf_amd.human_nerf import Network, default_cfg
    net = Network(default_cfg(basedir()), stage=2)
    net.load_state_dict(synth.human_state_dict(777, 2), strict=True)
    net = net.to(dev)
    joints = synth.tpose_joints()
    turn = tpose.TposeTurn(joints, formats.skeleton_bbox(joints, float(net.cfg.bbox_offset)), 32, dev)
    field = mesh.canonical_field(net, turn.const, 0.7, resolution=16)
    a = field["alpha"].cpu().numpy()
    best = None
    for q in (0.3, 0.5, 0.7, 0.8, 0.9, 0.95, 0.98, 0.99, 0.995, 0.998, 0.999):
        level = float(np.quantile(a[a > 0], q))
        v, _, f = mx.march(a, level, field["origin"], field["spacing"])
        c = cx.components(v.astype(np.float32), f)
        if best is None or c["count"] > best[1]["count"]:
            best = (level, c, f)
    level, want, faces = best
    print(f"level {level:.6g}: {want['count']} components, faces per component {want['n_faces'].tolist()}")
    assert want["count"] >= 1
    plain = mesh.extract(net, turn, 0.7, resolution=16, level=level)
    assert "components" not in plain and np.array_equal(plain["faces"].cpu().numpy(), faces)
    comp = mesh.components(plain["vertices"], plain["faces"])
    assert comp["count"] == want["count"] and torch.equal(comp["component"].cpu(), torch.from_numpy(want["component"]))
    assert mesh.drop_floaters(plain) is plain
    r = gap_ratio(want["area"]) if want["count"] > 1 else 0.5
    out = mesh.extract(net, turn, 0.7, resolution=16, level=level, normals=True, min_area_ratio=r)
    keep = cx.keep_rule(want["n_faces"], want["area"], r, 0)
    c = out["components"]
    assert (c["count"], c["kept"]) == (want["count"], int(keep.sum())) and c["kept"] >= 1
    kv = torch.from_numpy(keep.astype(bool)[want["component"]]).to(dev)
    assert torch.equal(out["vertices"], plain["vertices"][kv]) and torch.equal(out["colors"], plain["colors"][kv])
    assert out["normals"].shape == out["vertices"].shape and torch.equal(out["alpha"], plain["alpha"])
    gf = out["faces"].cpu().numpy()
    assert gf.shape[0] == int(want["n_faces"][keep != 0].sum()) and mx.is_closed_oriented_manifold(gf, out["vertices"].shape[0])


# ------------------------------------------------------------------------------------------ 5: the background mesh filters first
def test_extract_bkgd_filters_before_normals_and_colours(dev):
    from hosnerf_amd import mesh
    from hosnerf_amd.mipnerf360 import MipNeRF360
    model = MipNeRF360(basedir(), opaque_background=True)
    model.load_state_dict(synth.background_state_dict(777, 2), strict=False)
    model = model.to(dev)
    box = (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5)
    f = mesh.bkgd_field(model, box, 0.7, resolution=12)
    level = float(f["alpha"][1:-1, 1:-1, 1:-1].median())                # random weights never reach 0.5: a level that gives a surface
    whole = mesh.extract_bkgd(model, box, 0.7, resolution=12, level=level)
    comp = mesh.components(whole["vertices"], whole["faces"])
    print(f"level {level:.6g}: V {whole['vertices'].shape[0]}, {comp['count']} components, faces {comp['n_faces'].tolist()}")
    assert comp["count"] >= 2, "the field gives one component at this level: nothing to filter"
    r = gap_ratio(comp["area"].cpu().numpy())
    kept = mesh.extract_bkgd(model, box, 0.7, resolution=12, level=level, min_area_ratio=r)
    keep = mesh.keep_flags(comp, r)
    kv = keep.bool()[comp["component"].long()]
    c = kept["components"]
    assert 1 <= c["kept"] < c["count"] == comp["count"] and c["V_dropped"] == int((~kv).sum()) > 0
    assert torch.equal(kept["vertices"], whole["vertices"][kv])
    assert torch.equal(kept["normals"], whole["normals"][kv])
    assert torch.equal(kept["vertex_rgb"], whole["vertex_rgb"][kv]) and torch.equal(kept["colors"], whole["colors"][kv])
    assert mx.is_closed_oriented_manifold(kept["faces"].cpu().numpy(), kept["vertices"].shape[0])
    assert torch.equal(kept["alpha"], whole["alpha"]) and kept["box"] == whole["box"]
    # the same through drop_floaters of the whole mesh, vertex_rgb included
    after = mesh.drop_floaters(whole, min_area_ratio=r)
    for k in ("vertices", "faces", "colors", "normals", "vertex_rgb"):
        assert torch.equal(after[k], kept[k]), k


# ------------------------------------------------------------------------------------------ 6: the launcher
@pytest.mark.parametrize("gin,model", [("hosnerf_backpack.gin", "hosnerf"), ("state_humanobject_backpack.gin", "state_humanobject")])
def test_launcher_with_the_switch_on(tmp_path, gin, model):
    from hosnerf_amd.freeview import write_scene_pixels
    scene = str(tmp_path / "scene")
    write_scene_pixels(scene, synth.write_scene_dir(scene, 6, 64, 64, seed=9))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("patch:\n  N_patches: 2\n  size: 16\n")
    logs = str(tmp_path / "logs")
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "--ginc", os.path.join(ROOT, "configs", gin), "--ginb", "run.max_steps=2",
           "--ginb", f'run.datadir="{scene}"', "--ginb", "run.run_mesh=True", "--ginb", "run.run_mesh_frames=True", "--ginb", "run.run_mesh_track=True",
           "--ginb", "run.mesh_resolution=16", "--ginb", "run.mesh_level=0.001", "--ginb", "run.mesh_min_component=0.05", "--ginb", 'run.mesh_space="body"',
           "--scene_name", "synthetic", "--scene_dir", scene, "--cfg", str(cfg), "--logbase", logs, "--eval_skip", "3"]
    sets = ["mesh", "mesh_frames", "mesh_track"]
    if model == "hosnerf":
        cmd += ["--ginb", 'run.human_path=""', "--ginb", 'run.bkgd_path=""', "--ginb", "run.run_mesh_bkgd=True"]
        sets.append("mesh_bkgd")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    logdir = [os.path.join(logs, d) for d in os.listdir(logs)][0]
    for name in sets:
        folder = os.path.join(logdir, name)
        meta = json.load(open(os.path.join(folder, "meshes.json")))
        assert len(meta) == 2
        for stem, row in meta.items():
            v, f = formats.read_ply(os.path.join(folder, stem + ".ply"))[:2]
            c = row["components"]
            print(f"{model} {name}/{stem}: V {row['V']} F {row['F']} components {c}")
            assert row["V"] == v.shape[0] and row["F"] == f.shape[0]
            assert c["count"] >= c["kept"] >= 1 and c["rounds"] >= 1 and c["invalid_faces"] == 0
            if name == "mesh_track":
                tv = formats.read_ply(os.path.join(folder, row["template"]))[0]
                assert row["V"] == tv.shape[0]                                     # the frames have the filtered template's V
            else:
                assert mx.is_closed_oriented_manifold(f, v.shape[0])
                assert c["V_dropped"] >= 0 and abs(row["volume"] - mx.signed_volume(v, f)) < 1e-5 * max(1.0, row["area"])
