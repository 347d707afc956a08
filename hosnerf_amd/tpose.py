"""The T-pose turntable of the canonical human-object (`test_tpose`, 3rd_Complete_HOSNeRF/src/model/mipnerf360/model.py:591-658 = `M:`).

The reference renders the canonical subject in T-pose, with no background, turned once about the vertical in `cfg.render_frames`
steps -- one such turn for every object state, at the times halfway between the scene's transitions (M:643-658).  Its frames come
from `core/data/human_nerf/tpose.py` (`T:` below): a fixed camera on the z axis (T:74-93), a zero pose whose ROOT rotation turns
by -2 pi k / total about y (T:155-163), the canonical box turned with it (T:120-141, T:166), full-image rays cut by that box
(T:173-185) and the per-subject constants (T:197-227).

Here the host part of that file is restated function by function; the per-pixel part is one entry of hos_rays.hip
(`rays.frame_rays_compact`), and `eval.render_human_frame` renders what `tpose_frame` returns."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import formats
from . import rays as rays_mod
from .freeview import rodrigues

RENDER_SIZE = 512                                        # T:29
CAM_PARAMS = {"radius": 6.0, "focal": 1250.0}            # T:30-32


def get_camrot(campos: np.ndarray, lookat: Optional[np.ndarray] = None, inv_camera: bool = False) -> np.ndarray:
    """core/utils/camera_util.py:74-104: rows (right, up, forward) of a camera at `campos` looking at `lookat`, float32."""
    if lookat is None:
        lookat = np.array([0.0, 0.0, 0.0], dtype=np.float32)
    up = np.array([0.0, 1.0, 0.0], dtype=np.float32)
    if inv_camera:
        up[1] *= -1.0
    forward = lookat - campos
    forward = forward / np.linalg.norm(forward)
    right = np.cross(up, forward)
    right = right / np.linalg.norm(right)
    up = np.cross(forward, right)
    up = up / np.linalg.norm(up)
    return np.array([right, up, forward], dtype=np.float32)


def tpose_camera(img_size: int = RENDER_SIZE, radius: float = CAM_PARAMS["radius"], focal: float = CAM_PARAMS["focal"]) -> Tuple[np.ndarray, np.ndarray]:
    """`Dataset.setup_camera` (T:74-93) -> (K [3,3], E [4,4]), float32: the camera sits at (0, -0.25, radius), looks at
    (0, -0.25, 0) with its up vector pointing down (`inv_camera=True`), principal point at the image centre."""
    x, y, z = 0.0, -0.25, radius
    campos = np.array([x, y, z], dtype="float32")
    camrot = get_camrot(campos, lookat=np.array([0, y, 0.0]), inv_camera=True)
    E = np.eye(4, dtype="float32")
    E[:3, :3] = camrot
    E[:3, 3] = -camrot.dot(campos)
    K = np.eye(3, dtype="float32")
    K[0, 0] = focal
    K[1, 1] = focal
    K[:2, 2] = img_size / 2.0
    return K, E


def rotate_bbox(bbox: Dict[str, np.ndarray], rmtx: np.ndarray) -> Dict[str, np.ndarray]:
    """`Dataset.rotate_bbox` (T:120-141): the axis-aligned box of the eight corners after `corners.dot(rmtx)` -- the reference
    multiplies from the RIGHT (row vectors), i.e. it turns the corners by rmtx^T; kept."""
    min_x, min_y, min_z = bbox["min_xyz"]
    max_x, max_y, max_z = bbox["max_xyz"]
    pts = np.array([[min_x, min_y, min_z], [min_x, min_y, max_z], [min_x, max_y, min_z], [min_x, max_y, max_z],
                    [max_x, min_y, min_z], [max_x, min_y, max_z], [max_x, max_y, min_z], [max_x, max_y, max_z]])
    rotated = pts.dot(rmtx)
    return {"min_xyz": np.min(rotated, axis=0), "max_xyz": np.max(rotated, axis=0)}


def rotvec_of(R: np.ndarray) -> np.ndarray:
    """Axis-angle vector of a rotation matrix (what `cv2.Rodrigues(R)[0][:, 0]` returns, T:163), float64, angle in [0, pi].
    Away from angle pi: axis = (R - R^T)^vee / (2 sin), angle = acos((tr - 1) / 2).  At pi the antisymmetric part vanishes and
    the axis is read off the diagonal, R = 2 a a^T - I, with the signs of the off-diagonal terms -- the branch cv2 takes there,
    so that the half turn of frame total/2 is well defined."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    r = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = math.sqrt(float(r @ r) * 0.25)
    c = min(max((R[0, 0] + R[1, 1] + R[2, 2] - 1.0) * 0.5, -1.0), 1.0)
    theta = math.acos(c)
    if s < 1e-5:
        if c > 0.0:
            return np.zeros(3)
        a = np.sqrt(np.maximum((np.diag(R) + 1.0) * 0.5, 0.0))
        if R[0, 1] < 0.0:
            a[1] = -a[1]
        if R[0, 2] < 0.0:
            a[2] = -a[2]
        if abs(a[0]) < abs(a[1]) and abs(a[0]) < abs(a[2]) and (R[1, 2] > 0.0) != (a[1] * a[2] > 0.0):
            a[2] = -a[2]
        return a * (theta / np.linalg.norm(a))
    return r * (theta / (2.0 * s))


def tpose_pose(idx: int, total_frames: int) -> Tuple[np.ndarray, np.ndarray]:
    """T:155-163: the 78-vector of frame `idx` of a `total_frames` turn -- all zero but the root, which carries the rotation by
    -angle about y (angle = 2 pi idx / total, rounded to float32 like the reference's rvec), written back as an axis-angle
    vector -- and that rotation's matrix `add_rmtx` (the one the box is turned by, T:166)."""
    poses = np.zeros(78, dtype="float32")
    angle = 2 * np.pi / total_frames * idx
    add_rmtx = rodrigues(np.array([0, -angle, 0], dtype="float32"))
    root_rmtx = rodrigues(poses[:3])
    poses[:3] = rotvec_of(add_rmtx @ root_rmtx)
    return poses, add_rmtx


class TposeTurn:
    """What does not change over a turn (T:48-57, T:201, T:208-218): the canonical joints and box, `cnl_gtfms`, the motion-weight
    priors (3.5 MB, kept on the device) and the camera -- computed once, shared by every frame of every state."""

    def __init__(self, canonical_joints: np.ndarray, canonical_bbox: Dict[str, np.ndarray], volume_size: int = 32, device="cuda",
                 img_size: int = RENDER_SIZE, radius: float = CAM_PARAMS["radius"], focal: float = CAM_PARAMS["focal"]):
        self.device = torch.device(device)
        self.joints = np.asarray(canonical_joints, dtype=np.float32)
        self.bbox = {"min_xyz": np.asarray(canonical_bbox["min_xyz"]), "max_xyz": np.asarray(canonical_bbox["max_xyz"])}
        self.img_size = int(img_size)
        self.K, self.E = tpose_camera(img_size, radius, focal)
        bmin, bmax = self.bbox["min_xyz"].astype("float32"), self.bbox["max_xyz"].astype("float32")
        scale = 2.0 / (bmax - bmin)
        assert np.all(scale >= 0)                                                                    # T:219
        host = {"cnl_gtfms": formats.get_canonical_global_tfms(self.joints), "cnl_bbox_min_xyz": bmin, "cnl_bbox_max_xyz": bmax,
                "cnl_bbox_scale_xyz": scale,
                "motion_weights_priors": formats.approx_gaussian_bone_volumes(self.joints, bmin, bmax, grid_size=volume_size).astype("float32")}
        self.const = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(self.device) for k, v in host.items()}


def tpose_frame(canonical_joints, canonical_bbox, idx: int, total_frames: int, volume_size: int = 32, bgcolor=(255.0, 255.0, 255.0),
                device="cuda", turn: Optional[TposeTurn] = None, iter_val: float = 1e7, time: Optional[float] = None) -> Dict:
    """`Dataset.__getitem__(idx)` (T:146-229) with the per-pixel part on the device: the batch of the reference -- `img_width`,
    `img_height`, `ray_mask`, `rays` [2,n,3], `near`, `far` [n,1], `bgcolor`, `dst_Rs`, `dst_Ts`, `cnl_gtfms`,
    `motion_weights_priors`, `cnl_bbox_*`, `dst_posevec`, `is_train=False` -- plus `pix` / `slot` / `count` of
    `rays.frame_rays_compact` for the paint and `iter_val` / `time` when given (M:614-615).  Pass a `TposeTurn` to share the
    per-turn constants between frames; without one they are built here."""
    if turn is None:
        turn = TposeTurn(canonical_joints, canonical_bbox, volume_size, device)
    dev = turn.device
    H = W = turn.img_size
    poses, add_rmtx = tpose_pose(idx, total_frames)
    dst_bbox = rotate_bbox(turn.bbox, add_rmtx)                                                     # T:166
    E = turn.E
    r = rays_mod.frame_rays_compact(H, W, turn.K, E[:3, :3], E[:3, 3], dst_bbox, device=dev)       # T:173-183
    dst_Rs, dst_Ts = formats.body_pose_to_body_RTs(poses, turn.joints)                              # T:198-200
    host = {"dst_Rs": dst_Rs, "dst_Ts": dst_Ts, "dst_posevec": poses[3:] + 1e-2,                   # T:224
            "bgcolor": np.asarray(bgcolor, dtype="float32")}
    frame = {"img_width": W, "img_height": H, "ray_mask": r["slot"] >= 0, "rays": torch.stack([r["rays_o"], r["rays_d"]], 0),
             "near": r["near"][:, None], "far": r["far"][:, None], "pix": r["pix"], "slot": r["slot"], "count": r["count"],
             "dst_bbox": dst_bbox, "is_train": False, "iter_val": torch.full((1,), float(iter_val))}
    frame.update({k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for k, v in host.items()})
    frame.update(turn.const)
    if time is not None:
        frame["time"] = float(time)
    return frame


def tpose_times(transitions_times: Optional[Sequence[float]]) -> List[float]:
    """M:648-658: one time per object state -- halfway between 0, the transitions and 1 (float32 like the reference's
    `transitions_times`); `[0.5]` for a scene without transitions."""
    if transitions_times is None or len(transitions_times) == 0:
        return [0.5]
    tt = [np.float32(t) for t in np.asarray(transitions_times, dtype=np.float32).reshape(-1)]
    times = [(0.0 + tt[0]) / 2]
    times += [(tt[i - 1] + tt[i]) / 2 for i in range(1, len(tt))]
    times.append((tt[-1] + 1.0) / 2)
    return [float(t) for t in times]


def tpose_paths(time: float, idx: int) -> Tuple[str, str]:
    """M:631-635: (folder under <logdir>/tpose_vis, file name) of frame `idx` of the turn rendered at `time`."""
    return "time_{:06}".format(time), "image-{:05}.jpg".format(idx)
