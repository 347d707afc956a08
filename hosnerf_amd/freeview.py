"""Free-viewpoint cameras and evaluation frames of a scene directory (BASELINE configs[4]).

The reference renders its free-viewpoint sequence from ONE training frame: `FreeviewDataset` (3rd_Complete_HOSNeRF/core/data/
human_nerf/freeview.py:39-337) takes the cameras / SMPL fit of frame `cfg.freeview.frame_idx` and, for k = 0 .. render_frames-1,
turns the camera about the subject with `rotate_camera_by_frame_idx` (core/utils/camera_util.py:106-131 -> `_update_extrinsics`,
:14-70): a rotation by 2 pi k / period about an axis tilted 15 degrees out of the vertical, centred on the subject's translation
Th.  `LitMipNeRF360.free_view` (src/model/mipnerf360/model.py:1293-1494) renders those frames; `test_metrics` (:884-1085) renders
the held-out frames with their own cameras and reports PSNR.

Here: `orbit_camera` is that camera (pinned against the reference's function by tests/golden/freeview.npz), `freeview_frame` /
`eval_frame` build the frame dicts `eval.render_frame` consumes with every per-pixel quantity produced on the device
(`eval.frame_rays`), and `load_scene_pixels` decodes `images/*.png` / `masks/*.png` / `images_flow/*_bwd.npz` of a scene
directory (PIL; the reference uses cv2 / PIL, core/utils/image_util.py)."""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

TILT_DEG = 15.0          # the orbit's axis: (0, cos 15, sin 15) in SMPL space (camera_util.py:45)


def rodrigues(rvec: np.ndarray) -> np.ndarray:
    """Rotation matrix of an axis-angle vector (what cv2.Rodrigues(rvec)[0] returns), float64."""
    r = np.asarray(rvec, dtype=np.float64).reshape(3)
    theta = float(np.sqrt(r @ r))
    if theta < 1e-12:
        return np.eye(3)
    k = r / theta
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + math.sin(theta) * Kx + (1.0 - math.cos(theta)) * (Kx @ Kx)


def orbit_camera(extrinsics: np.ndarray, frame_idx: int, period: int, trans: Optional[np.ndarray] = None,
                 inv_angle: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """`rotate_camera_by_frame_idx` (camera_util.py:106-131): camera k of a `period`-frame turn about the subject.

    Returns (E_k [4,4], T_smpl [4,4]): E_k = E @ T_smpl, where T_smpl is the inverse of the rigid motion "rotate by the angle about
    the tilted axis through `trans`" -- moving the scene by T_smpl^-1 in front of the fixed camera is the same picture as moving
    the camera.  The angle changes sign when the camera's up vector points down in SMPL space (camera_util.py:40-42) and with
    `inv_angle` (the 'zju_mocap' source type; 'wild' = False, freeview.py:34-37).  The rotation is rounded to float32 like the
    reference's (`.astype('float32')`, camera_util.py:46)."""
    E = np.asarray(extrinsics, dtype=np.float64)
    angle = 2.0 * math.pi * (frame_idx / period)
    if inv_angle:
        angle = -angle
    cam_to_smpl = np.linalg.inv(E)
    if cam_to_smpl[:3, :3].T[1, 1] < 0.0:
        angle = -angle
    axis = np.array([0.0, math.cos(math.radians(TILT_DEG)), math.sin(math.radians(TILT_DEG))])
    G = rodrigues(axis * angle).astype(np.float32).astype(np.float64)
    T = np.eye(4)
    T[:3, :3] = G
    if trans is not None:
        t = np.asarray(trans, dtype=np.float64).reshape(3)
        # x -> G (x - t) + t
        T[:3, 3] = t - G @ t
    T_smpl = np.linalg.inv(T)
    return E @ T_smpl, T_smpl


def load_scene_pixels(scene_dir: str, frames: Optional[Sequence[str]] = None) -> Dict:
    """Decode what the reference's datasets read per frame (core/data/human_nerf/train.py:300-345, freeview.py:173-197):
    `images/<frame>.png` -> [N,H,W,3] in 0..1, `masks/<frame>.png` -> [N,H,W] in 0..1 (all ones if the folder is missing),
    `images_flow/<frame>_bwd.npz` {flow [H,W,2], mask [H,W]} -> [N,H,W,3] (zeros where a file is missing), and the frame names
    (sorted file stems, `list_files` order)."""
    from PIL import Image
    img_dir = os.path.join(scene_dir, "images")
    if frames is None:
        frames = sorted(os.path.splitext(f)[0] for f in os.listdir(img_dir) if f.lower().endswith(".png"))
    images, alphas, flows = [], [], []
    any_flow = False
    for name in frames:
        img = np.asarray(Image.open(os.path.join(img_dir, name + ".png")).convert("RGB"), dtype=np.float32) / 255.0
        images.append(img)
        mp = os.path.join(scene_dir, "masks", name + ".png")
        if os.path.exists(mp):
            m = np.asarray(Image.open(mp), dtype=np.float32)
            alphas.append((m[..., 0] if m.ndim == 3 else m) / 255.0)
        else:
            alphas.append(np.ones(img.shape[:2], np.float32))
        fp = os.path.join(scene_dir, "images_flow", name + "_bwd.npz")
        if os.path.exists(fp):
            d = np.load(fp)
            flows.append(np.concatenate([d["flow"].astype(np.float32), d["mask"].astype(np.float32)[..., None]], -1))
            any_flow = True
        else:
            flows.append(np.zeros(img.shape[:2] + (3,), np.float32))
    return {"frames": list(frames), "images": np.stack(images, 0), "alphas": np.stack(alphas, 0),
            "flows": np.stack(flows, 0) if any_flow else None}


def write_scene_pixels(scene_dir: str, px: Dict):
    """The inverse of `load_scene_pixels` for synthetic scenes (tests, the launcher's synthetic mode): 8-bit PNGs + flow archives."""
    from PIL import Image
    for sub in ("images", "masks", "images_flow"):
        os.makedirs(os.path.join(scene_dir, sub), exist_ok=True)
    for i, name in enumerate(px["frames"]):
        Image.fromarray((np.clip(px["images"][i], 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)).save(os.path.join(scene_dir, "images", name + ".png"))
        Image.fromarray((np.clip(px["alphas"][i], 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)).save(os.path.join(scene_dir, "masks", name + ".png"))
        if px.get("flows") is not None:
            np.savez(os.path.join(scene_dir, "images_flow", name + "_bwd.npz"), flow=px["flows"][i][..., :2], mask=px["flows"][i][..., 2])


def depth_preview(depth: np.ndarray) -> np.ndarray:
    """8-bit preview of a depth map, normalised by the frame's own 2nd..98th percentile (near = dark).  The expected depth of
    the background reaches the far plane (1e6), so a min/max normalisation would show nothing of the subject."""
    d = np.asarray(depth, dtype=np.float64)
    lo, hi = np.percentile(d, 2.0), np.percentile(d, 98.0)
    return (np.clip((d - lo) / max(hi - lo, 1e-12), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def save_frame_maps(out_dir: str, name: str, maps: Dict, H: int, W: int) -> Dict[str, str]:
    """Write the maps of one frame next to its colour image, one group of files per key present in `maps` (tensors or arrays, [H*W]
    or [H*W,3]; other keys, `rgb` for one, are ignored); returns {kind: path}:
      depth         <name>_depth.npy         float32 [H,W], the un-normalised expected depth (stage 3: `depth_map`, M:94; stage 1: sum w t_mid,
                                             helper.py:166-190), and <name>_depth.png, its 8-bit preview (`depth_preview`)
      depth_median  <name>_depth_median.npy  float32 [H,W], the depth at which the ray's cumulative weight crosses 0.5, in the units of
                                             <name>_depth.npy (the last sample's depth where alpha <= 0.5), and <name>_depth_median.png
      alpha         <name>_alpha.png         opacity (`acc_map`, M:93; stage 1: sum w, helper.py:233), 8-bit greyscale
      alpha_human together with rgb_human
                    <name>_alpha_human.png   opacity of the human-object layer, 8-bit greyscale
                    <name>_human.png         that layer as RGBA: colour un-premultiplied where alpha_human > 0, alpha = alpha_human
    What a caller passes is what is written: `eval.render_frame(maps=True)` / `eval.render_bkgd_frame(maps=True)` dicts as they
    come, or a sub-dict (the T-pose turn passes `depth_median` alone)."""
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    to8 = lambda x: (np.clip(x, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    host = lambda k, *c: np.asarray(maps[k].detach().float().cpu() if isinstance(maps[k], torch.Tensor) else maps[k], dtype=np.float32).reshape(H, W, *c)
    paths = {}

    def path(kind):
        paths[kind] = os.path.join(out_dir, f"{name}_{kind}")
        return paths[kind]

    for k in ("depth", "depth_median"):
        if k in maps:
            np.save(path(k + ".npy"), host(k))
            Image.fromarray(depth_preview(host(k))).save(path(k + ".png"))
    if "alpha" in maps:
        Image.fromarray(to8(host("alpha"))).save(path("alpha.png"))
    if "alpha_human" in maps and "rgb_human" in maps:
        ah, colour = host("alpha_human"), host("rgb_human", 3)
        Image.fromarray(to8(ah)).save(path("alpha_human.png"))
        straight = np.where(ah[..., None] > 0.0, colour / np.where(ah > 0.0, ah, 1.0)[..., None], 0.0)
        Image.fromarray(np.concatenate([to8(straight), to8(ah)[..., None]], -1), mode="RGBA").save(path("human.png"))
    return paths


MESH_MAP_FILES = ("_mesh.png", "_mesh_normal.png", "_mesh_mask.png", "_mesh_depth.npy", "_mesh_depth.png")


def save_mesh_maps(out_dir: str, name: str, raster: Dict, H: int, W: int) -> Dict[str, str]:
    """Write the maps of one rasterised mesh (`mesh.rasterize` with `shaded`, `normal`, `mask` and `depth`; tensors or arrays, [H*W]
    or [H*W,3]) next to its .ply; returns {kind: path}:
      <name>_mesh.png          the shaded preview (vertex colours under a two-sided head-light, over the background colour), 8-bit RGB
      <name>_mesh_normal.png   0.5 + 0.5 n of the interpolated normals, 8-bit RGB (grey where empty)
      <name>_mesh_mask.png     the silhouette, 8-bit greyscale 0 / 255
      <name>_mesh_depth.npy    float32 [H,W], camera-space z = the ray parameter of the frame's human rays, 0 where empty
      <name>_mesh_depth.png    `depth_preview` of the covered pixels (near = dark), 0 where empty"""
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    to8 = lambda x: (np.clip(x, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    host = lambda k, *c: np.asarray(raster[k].detach().float().cpu() if isinstance(raster[k], torch.Tensor) else raster[k], dtype=np.float32).reshape(H, W, *c)
    paths = {kind: os.path.join(out_dir, name + kind) for kind in MESH_MAP_FILES}
    Image.fromarray(to8(host("shaded", 3))).save(paths["_mesh.png"])
    Image.fromarray(to8(0.5 + 0.5 * host("normal", 3))).save(paths["_mesh_normal.png"])
    covered = host("mask") != 0
    Image.fromarray(covered.astype(np.uint8) * 255).save(paths["_mesh_mask.png"])
    depth = host("depth")
    np.save(paths["_mesh_depth.npy"], depth)
    preview = np.zeros((H, W), dtype=np.uint8)
    if covered.any():
        preview[covered] = depth_preview(depth[covered])
    Image.fromarray(preview).save(paths["_mesh_depth.png"])
    return paths
