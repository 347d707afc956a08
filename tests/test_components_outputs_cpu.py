"""What the launcher's four mesh outputs write with `run.mesh_min_component`, without a GPU (the approach of
tests/test_frame_outputs_cpu.py, whose stub meshes and scene these tests share): the extractors, the tracker and the checkpoint
loader are recording stubs.  At 0 the extractors are called exactly as before the binding existed and every file is byte-identical;
above 0 they are handed `min_area_ratio`, the rows gain `components`, and the templates are filtered once, before any frame."""
import argparse
import json
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import run as launcher
import test_frame_outputs_cpu as fo
from hosnerf_amd import formats, mesh, select_option, tpose

COMPONENTS = {"count": 5, "kept": 2, "V_dropped": 1, "F_dropped": 1, "area_dropped": 0.25, "volume_dropped": 0.125, "rounds": 3,
              "invalid_faces": 0, "negative_volume": 0}


def filtered(m, ratio):
    """What a stub extractor returns for `min_area_ratio = ratio`: the stub mesh less its last vertex and face, plus `components`."""
    V, F = m["vertices"].shape[0] - 1, m["faces"].shape[0] - 1
    out = dict(m, vertices=m["vertices"][:V], colors=m["colors"][:V], faces=m["faces"][:F] % V, components=dict(COMPONENTS, ratio=ratio))
    if m.get("normals") is not None:
        out["normals"] = m["normals"][:V]
    return out


class Scene(fo.Scene):
    def frame_pose(self, i):
        return {"frame_name": f"frame_{i:06d}", "i": i, "bad": False, "time": i / 8.0}


@pytest.fixture
def env(monkeypatch, tmp_path):
    monkeypatch.setattr(select_option, "load_checkpoint", lambda lit, ckpt, strict=False: None)
    monkeypatch.setattr(tpose, "TposeTurn", lambda *a: "turn")
    ckpt = str(tmp_path / "last.ckpt")
    torch.save({"global_step": 3}, ckpt)
    return NS(ckpt=ckpt, tmp=tmp_path, args=argparse.Namespace(eval_skip=3, render_frames=5, render_limit=2), calls=[])


def old_extractors(monkeypatch, env):
    """The extractors with the signatures they had before `min_area_ratio` existed: handing them the keyword is a TypeError."""
    def extract(net, turn, time, resolution=256, level=0.5, normals=False):
        env.calls.append(("extract", time))
        return dict(fo.stub_mesh(int(time * 10)), normals=None)

    def extract_frame(net, pose, resolution=256, level=0.5, space="world", normals=False):
        env.calls.append(("extract_frame", pose["i"]))
        m = fo.stub_mesh(pose["i"] + 1)
        m.update(frame_name=pose["frame_name"], time=pose["i"] / 8.0, space=space, to_world=np.eye(4) * (pose["i"] + 1), normals=torch.ones_like(m["vertices"]) if normals else None)
        return m

    def extract_bkgd(model, box, time, resolution=256, level=0.5):
        env.calls.append(("extract_bkgd", time))
        return dict(fo.stub_mesh(int(time * 10) + 2), box=list(box), normals=None)

    for name, fn in (("extract", extract), ("extract_frame", extract_frame), ("extract_bkgd", extract_bkgd)):
        monkeypatch.setattr(mesh, name, fn)


def new_extractors(monkeypatch, env):
    def extract(net, turn, time, resolution=256, level=0.5, normals=False, min_area_ratio=0.0):
        env.calls.append(("extract", time, min_area_ratio))
        return filtered(dict(fo.stub_mesh(int(time * 10) + 2), normals=None), min_area_ratio)

    def extract_frame(net, pose, resolution=256, level=0.5, space="world", normals=False, min_area_ratio=0.0):
        env.calls.append(("extract_frame", pose["i"], min_area_ratio))
        m = fo.stub_mesh(pose["i"] + 2)
        m.update(frame_name=pose["frame_name"], time=pose["i"] / 8.0, space=space, to_world=np.eye(4), normals=torch.ones_like(m["vertices"]) if normals else None)
        return filtered(m, min_area_ratio)

    def extract_bkgd(model, box, time, resolution=256, level=0.5, min_area_ratio=0.0):
        env.calls.append(("extract_bkgd", time, min_area_ratio))
        return filtered(dict(fo.stub_mesh(int(time * 10) + 2), box=list(box), normals=None), min_area_ratio)

    def track(net, template, pose, space="world", normals=False):
        env.calls.append(("track", pose["i"], int(template["vertices"].shape[0])))
        V = template["vertices"].shape[0]
        return {"vertices": template["vertices"] + 1.0, "faces": template["faces"], "colors": template["colors"], "normals": None,
                "residual": torch.zeros(V), "converged": torch.ones(V, dtype=torch.bool), "mask": torch.ones(V), "mask_canonical": torch.ones(V),
                "state": int(template["state"]), "frame_name": pose["frame_name"], "time": pose["time"], "volume": 1.0, "area": 2.0,
                "spacing": template["spacing"], "dims": template["dims"], "to_world": np.eye(4)}

    for name, fn in (("extract", extract), ("extract_frame", extract_frame), ("extract_bkgd", extract_bkgd), ("track", track)):
        monkeypatch.setattr(mesh, name, fn)


def make_lit():
    lit = fo.make_lit()
    lit.net.model = NS(mlps=[NS(transitions_times=[0.4])])
    return lit


def write_all(env, kw, logdir, with_track=False):
    lit = make_lit()
    kw = {"mesh_resolution": 16, "mesh_level": 0.25, "mesh_space": "body", **kw}
    launcher.extract_meshes(kw, lit, Scene(), env.ckpt, logdir, "cpu", 0, 1)
    launcher.extract_frame_meshes(env.args, kw, lit, Scene(), env.ckpt, logdir, "cpu", 0, 1)
    launcher.extract_bkgd_meshes(kw, lit, "hosnerf", Scene(), env.ckpt, logdir, "cpu", 0, 1)
    if with_track:
        launcher.track_meshes(env.args, kw, lit, Scene(), env.ckpt, logdir, "cpu", 0, 1)


def tree(logdir):
    out = {}
    for folder, _, files in os.walk(logdir):
        for name in files:
            path = os.path.join(folder, name)
            out[os.path.relpath(path, logdir)] = open(path, "rb").read()
    return out


def test_files_are_byte_identical_with_the_switch_at_zero(monkeypatch, env):
    old_extractors(monkeypatch, env)                       # a `min_area_ratio` keyword would be a TypeError here
    a, b, c = (str(env.tmp / n) for n in ("absent", "zero", "zero_int"))
    write_all(env, {}, a)
    write_all(env, {"mesh_min_component": 0.0}, b)
    write_all(env, {"mesh_min_component": 0}, c)
    ta, tb, tc = tree(a), tree(b), tree(c)
    assert sorted(ta) == sorted(tb) == sorted(tc) and len(ta) == 2 + 1 + 2 + 1 + 2 + 1
    assert ta == tb == tc
    # and they are the bytes tests/test_frame_outputs_cpu.py pins for these stub meshes
    assert ta[os.path.join("mesh", "meshes.json")].decode() == json.dumps(fo.CANONICAL_ROWS, indent=1)
    assert ta[os.path.join("mesh_frames", "meshes.json")].decode() == json.dumps(fo.FRAME_ROWS, indent=1)
    assert all("components" not in row for name, data in ta.items() if name.endswith(".json") for row in json.loads(data).values())


def test_rows_gain_components_with_the_switch_on(monkeypatch, env):
    new_extractors(monkeypatch, env)
    logdir = str(env.tmp / "on")
    write_all(env, {"mesh_min_component": 0.05}, logdir, with_track=True)
    want = dict(COMPONENTS, ratio=0.05)
    for folder, keys in (("mesh", ["time", "state", "V", "F", "volume", "area", "level", "spacing", "dims", "components"]),
                         ("mesh_frames", ["frame_name", "time", "state", "V", "F", "volume", "area", "level", "spacing", "dims", "space", "to_world",
                                          "components"]),
                         ("mesh_bkgd", ["time", "state", "V", "F", "volume", "area", "level", "spacing", "dims", "box", "components"])):
        rows = json.load(open(os.path.join(logdir, folder, "meshes.json")))
        assert len(rows) == 2
        for stem, row in rows.items():
            assert list(row) == keys and row["components"] == want
            v, f, _ = formats.read_ply(os.path.join(logdir, folder, stem + ".ply"))[:3]
            assert (row["V"], row["F"]) == (v.shape[0], f.shape[0])               # the row describes the written, filtered mesh
    # every extractor was handed the ratio
    assert all(c[-1] == 0.05 for c in env.calls if c[0].startswith("extract")) and {c[0] for c in env.calls} == {
        "extract", "extract_frame", "extract_bkgd", "track"}
    # the tracked set: one filtered template per state, extracted once, before the first frame that uses it; its .ply is the filtered one
    tracked = env.calls[[c[0] for c in env.calls].index("track") - 1:]
    assert [c[0] for c in tracked].count("extract") == 2 and tracked[0][0] == "extract"
    rows = json.load(open(os.path.join(logdir, "mesh_track", "meshes.json")))
    assert list(rows) == ["frame_000000", "frame_000003"]
    for stem, row in rows.items():
        assert row["components"] == want and list(row)[-1] == "components"
        tv = formats.read_ply(os.path.join(logdir, "mesh_track", row["template"]))[0]
        fv = formats.read_ply(os.path.join(logdir, "mesh_track", stem + ".ply"))[0]
        assert row["V"] == tv.shape[0] == fv.shape[0]                             # the frames have the filtered template's V
    # both chosen frames are of state 0: they were tracked with the filtered state-0 template; state 1's is written all the same
    assert {c[2] for c in env.calls if c[0] == "track"} == {formats.read_ply(os.path.join(logdir, "mesh_track", "template_state_0.ply"))[0].shape[0]}
    assert os.path.exists(os.path.join(logdir, "mesh_track", "template_state_1.ply"))


def test_a_bad_ratio_stops_every_output_before_it_loads_anything(env):
    lit = make_lit()
    kw = {"mesh_min_component": 1.5}
    for call in (lambda: launcher.extract_meshes(kw, lit, Scene(), env.ckpt, str(env.tmp / "x"), "cpu", 0, 1),
                 lambda: launcher.extract_frame_meshes(env.args, kw, lit, Scene(), env.ckpt, str(env.tmp / "x"), "cpu", 0, 1),
                 lambda: launcher.track_meshes(env.args, kw, lit, Scene(), env.ckpt, str(env.tmp / "x"), "cpu", 0, 1),
                 lambda: launcher.extract_bkgd_meshes(kw, lit, "hosnerf", Scene(), env.ckpt, str(env.tmp / "x"), "cpu", 0, 1)):
        with pytest.raises(SystemExit) as e:
            call()
        assert str(e.value).startswith("run.mesh_min_component = 1.5: a number in [0, 1]")
    assert not os.path.exists(str(env.tmp / "x" / "mesh" / "meshes.json"))
