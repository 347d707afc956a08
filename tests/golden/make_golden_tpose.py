"""Golden vectors for the T-pose turntable: outputs of the REFERENCE's own `core/data/human_nerf/tpose.py` (`Dataset.setup_camera`,
`Dataset.__getitem__`, imported here, in the build container only) for `synth.tpose_joints()`, a turn of 8 frames (idx 0, 1, 3, 6) and a
48 x 48 image with focal = 1250 * 48 / 512 and cfg.bbox_offset = 0.1, so that the box covers part of the image.
cv2 is not installed in this image; the reference calls exactly one cv2 function on this path, `cv2.Rodrigues`, in both directions
(vector -> matrix, T:160-161, and matrix -> vector, T:163) -- the generator provides a numpy stand-in for it (the closed forms cv2
documents; the inverse is the generic one, singular at angle pi, which is why idx 4 is not a case), nothing of the reference is altered:
`RENDER_SIZE` / `CAM_PARAMS` are class attributes and are set as such.
  python tests/golden/make_golden_tpose.py   ->  tests/golden/tpose.npz"""
import importlib.util
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden import refload

IMG, TOTAL, IDXS, VOLUME = 48, 8, (0, 1, 3, 6), 8
BBOX_OFFSET = 0.1          # cfg.bbox_offset: with the default 0.6 the box of this skeleton fills the 48 x 48 image in three of the four frames
KEYFILTER = ["rays", "motion_bases", "motion_weights_priors", "cnl_bbox", "dst_posevec_75"]


def _rodrigues(src):
    a = np.asarray(src, dtype=np.float64)
    if a.size == 9:                                     # matrix -> vector [3,1]
        R = a.reshape(3, 3)
        th = np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))
        if th < 1e-12:
            return np.zeros((3, 1)), None
        r = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (2.0 * np.sin(th))
        return (r * th).reshape(3, 1), None
    v = a.reshape(3)
    th = np.linalg.norm(v)
    if th < 1e-12:
        return np.eye(3), None
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx, None


def main():
    from hosnerf_amd import synth
    d = tempfile.mkdtemp(prefix="hos_tpose_")
    with open(os.path.join(d, "canonical_joints.pkl"), "wb") as f:
        pickle.dump({"joints": synth.tpose_joints()[:24].astype(np.float32)}, f)
    cfg = types.SimpleNamespace(bbox_offset=BBOX_OFFSET, render_frames=TOTAL, mweight_volume=types.SimpleNamespace(volume_size=VOLUME))
    with refload.stage(3):
        sys.modules["cv2"].Rodrigues = _rodrigues
        spec = importlib.util.spec_from_file_location("ref_tpose", os.path.join(refload.STAGE[3], "core", "data", "human_nerf", "tpose.py"))
        T = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(T)
        T.Dataset.RENDER_SIZE = IMG
        T.Dataset.CAM_PARAMS = {"radius": 6.0, "focal": 1250.0 * IMG / 512}
        ds = T.Dataset(cfg, d, keyfilter=KEYFILTER, bgcolor=[255.0, 255.0, 255.0])
        out = {"img_size": IMG, "total_frames": TOTAL, "idxs": np.array(IDXS), "volume_size": VOLUME, "bbox_offset": BBOX_OFFSET, "radius": 6.0,
               "focal": 1250.0 * IMG / 512, "K": ds.camera["K"], "E": ds.camera["E"], "joints24": synth.tpose_joints()[:24].astype(np.float32),
               "canonical_joints": ds.canonical_joints, "cnl_min": ds.canonical_bbox["min_xyz"], "cnl_max": ds.canonical_bbox["max_xyz"]}
        K512, E512 = T.Dataset.setup_camera(img_size=512, radius=6.0, focal=1250.0)
        out["K512"], out["E512"] = K512, E512
        assert len(ds) == TOTAL
        partial = 0
        for idx in IDXS:
            r = ds[idx]
            p = f"i{idx}_"
            angle = 2 * np.pi / TOTAL * idx
            add = _rodrigues(np.array([0, -angle, 0], dtype="float32"))[0]
            box = T.Dataset.rotate_bbox(ds.canonical_bbox.copy(), add)
            out[p + "add_rmtx"], out[p + "box_min"], out[p + "box_max"] = add, box["min_xyz"], box["max_xyz"]
            for k in ("ray_mask", "rays", "near", "far", "bgcolor", "dst_Rs", "dst_Ts", "cnl_gtfms", "cnl_bbox_min_xyz", "cnl_bbox_max_xyz",
                      "cnl_bbox_scale_xyz", "dst_posevec"):
                out[p + k] = np.asarray(r[k])
            # the root rotation vector the item was built from (T:160-163), through the same calls
            out[p + "root"] = _rodrigues(add @ _rodrigues(np.zeros(3, "float32"))[0])[0][:, 0].astype("float32")
            assert r["img_width"] == IMG and r["img_height"] == IMG and r["is_train"] is False
            n = int(r["ray_mask"].sum())
            partial += int(0 < n < IMG * IMG)
            print(f"idx {idx}: {n} of {IMG * IMG} rays hit the box")
        assert partial == len(IDXS), "the box must cover part of the image"
        out["motion_weights_priors"] = np.asarray(ds[0]["motion_weights_priors"])
    path = os.path.join(HERE, "tpose.npz")
    np.savez_compressed(path, **out)
    print("tpose.npz", os.path.getsize(path) / 1024, "KB")


if __name__ == "__main__":
    main()
