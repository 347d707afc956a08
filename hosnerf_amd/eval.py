"""Full-frame rendering loops of stage 3 (SURVEY 8(f).1 + 8(f).3).

The reference renders a frame in four near-identical methods of `LitMipNeRF360` -- `progress` (M:680-880), `test_metrics`
(M:884-1085), `allimgs_metrics` (M:1089-1289) and `free_view` (M:1293-1494), M = 3rd_Complete_HOSNeRF/src/model/mipnerf360/model.py:
    for each `chunk_bkg` = 8192 rays that hit the human bounding box:  background model + human network + z-merge composite
    for each `chunk_bkg` rays that miss it:                            background model + 32-sample `_raw2outputs`
    rendered[ray_mask] = rgb; rendered[ray_mask_bkg] = bkg_rgbs; PSNR against the ground-truth pixels.
The per-frame inputs come from a dataset `__getitem__` that builds full-image rays in numpy
(3rd_Complete_HOSNeRF/core/data/human_nerf/freeview.py:199-337).

Here the same loop is one function, `render_frame`, with three differences in HOW (not WHAT) it computes:
  * rays, radii and the box test are produced on the device by `frame_rays` (hos_rays.hip) under the dataset's batch keys;
  * the ray-independent prologue of the human network (pose refinement, motion bases, the 253 MB motion-weight volume
    decoder) runs once per frame instead of once per chunk (`Network.frame_prologue`);
  * with a process group the two ray lists are split into contiguous per-rank ranges and the colours are all-gathered
    (`train.shard_frame` / `train.gather_frame`, the role of `alter_gather_cat`, S1/src/model/interface.py:30-39).
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict, Optional

import numpy as np
import torch

from . import rays as rays_mod
from .train import gather_frame, shard_frame

# per-frame (ray independent) keys of the human network's batch (M:1337-1352)
FRAME_KEYS = ("bgcolor", "dst_Rs", "dst_Ts", "cnl_gtfms", "canonical_joints", "motion_weights_priors", "cnl_bbox_min_xyz",
              "cnl_bbox_max_xyz", "cnl_bbox_scale_xyz", "dst_posevec", "iter_val", "time", "is_train", "newsmpl_to_scale_world")


@contextlib.contextmanager
def evaluating(hos):
    """`test_begin` / `test_end` (M:670-678): eval mode, no depth jitter in the human branch, no autograd."""
    was_training = hos.training
    perturb = hos.cfg.perturb
    hos.eval()
    hos.cfg.perturb = 0.0
    try:
        with torch.no_grad():
            yield hos
    finally:
        hos.cfg.perturb = perturb
        hos.train(was_training)


def frame_rays(H: int, W: int, K, E, dst_bbox, E_colmap, device="cuda") -> Dict[str, torch.Tensor]:
    """The ray part of `FreeviewDataset.__getitem__` (freeview.py:239-283) on the device.  `E` is the SMPL-space camera
    (after `apply_global_tfm_to_camera`), `E_colmap` the background-world camera; both [4,4] or [3,4] host arrays."""
    E = np.asarray(E, dtype=np.float64)
    Ec = np.asarray(E_colmap, dtype=np.float64)
    o, d = rays_mod.get_rays_from_KRT(H, W, K, E[:3, :3], E[:3, 3], device=device)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    near, far, ray_mask = rays_mod.rays_intersect_3d_bbox(dst_bbox, o, d)
    ob, db, vb, rad = rays_mod.get_rays_from_KRT_bkg(H, W, K, Ec[:3, :3], Ec[:3, 3], device=device)
    ob, db, vb, rad = ob.reshape(-1, 3), db.reshape(-1, 3), vb.reshape(-1, 3), rad.reshape(-1, 1)
    miss = ~ray_mask
    return {
        "img_width": W, "img_height": H, "ray_mask": ray_mask, "ray_mask_bkg": miss,
        "rays": torch.stack([o[ray_mask], d[ray_mask]], 0), "near": near[:, None], "far": far[:, None],
        "rays_o_bkg": ob[ray_mask], "rays_d_bkg": db[ray_mask], "viewdirs_bkg": vb[ray_mask], "radii": rad[ray_mask],
        "rays_o_bkg_only": ob[miss], "rays_d_bkg_only": db[miss], "viewdirs_bkg_only": vb[miss], "radii_bkg_only": rad[miss],
    }


def _local(tensors: Dict[str, torch.Tensor], n: int, group) -> Dict[str, torch.Tensor]:
    """This rank's contiguous share of `n` rays (padded by repeating the last ray, like S1/src/data/interface.py:152-166)."""
    if group is None or n == 0:
        return tensors
    import torch.distributed as dist
    idx, _ = shard_frame(n, dist.get_rank(group), dist.get_world_size(group))
    idx = idx.to(next(iter(tensors.values())).device)
    return {k: v.index_select(1 if k == "rays" else 0, idx) for k, v in tensors.items()}


# column layout of a ray list's packed maps (one [n, C] tensor per list, so that a frame still costs one gather per list)
FG_MAP_COLS = {"rgb": slice(0, 3), "alpha": 3, "depth": 4, "rgb_human": slice(5, 8), "alpha_human": 8}      # [n_fg, 9]
BG_MAP_COLS = {"rgb": slice(0, 3), "alpha": 3, "depth": 4}                                                  # [n_bg, 5]
FG_MAP_WIDTH, BG_MAP_WIDTH = 9, 5
# with `median=True` one more column at the end of each list (`depth_median`); the layouts above are the ones without it
FG_MEDIAN_COLS = dict(FG_MAP_COLS, depth_median=FG_MAP_WIDTH)                                               # [n_fg, 10]
BG_MEDIAN_COLS = dict(BG_MAP_COLS, depth_median=BG_MAP_WIDTH)                                               # [n_bg, 6]


def pack_maps(out: Dict[str, torch.Tensor], cols: Dict) -> torch.Tensor:
    """The maps of one rendered chunk (`HOSNeRF.render(maps=True)` / `render_bkg_only(maps=True)`) as one [n, C] tensor."""
    return torch.cat([out[k] if out[k].dim() == 2 else out[k][:, None] for k in cols], 1)


def assemble_maps(H: int, W: int, bgcolor, ray_mask: torch.Tensor, ray_mask_bkg: torch.Tensor, fg_packed: torch.Tensor,
                  bg_packed: torch.Tensor, median: bool = False) -> Dict[str, torch.Tensor]:
    """Scatter the two ray lists' packed maps into whole-frame buffers the way `rendered` is assembled (M:1456-1459):
    `rgb` [H*W,3] starts from bgcolor / 255 (M:1311-1313), `alpha` / `depth` [H*W] and the human layer `rgb_human` [H*W,3] /
    `alpha_human` [H*W] from zero; rays through the human box (`ray_mask`) take all five from `fg_packed` [n_fg,9], rays that
    miss it (`ray_mask_bkg`) take rgb / alpha / depth from `bg_packed` [n_bg,5] and have no human layer.  `median`: both lists
    carry one more column (`FG_MEDIAN_COLS` / `BG_MEDIAN_COLS`) and the frame gets `depth_median` [H*W], from zero like `depth`."""
    return _assemble(H, W, bgcolor, ray_mask, ray_mask_bkg, fg_packed, bg_packed,
                     FG_MEDIAN_COLS if median else FG_MAP_COLS, BG_MEDIAN_COLS if median else BG_MAP_COLS)


RGB_COLS = {"rgb": slice(0, 3)}          # the layout of a frame rendered without maps: the colours alone, [n, 3]


def _assemble(H: int, W: int, bgcolor, ray_mask, ray_mask_bkg, fg_packed, bg_packed, fg_cols: Dict, bg_cols: Dict) -> Dict[str, torch.Tensor]:
    """`assemble_maps` for any column layout: one whole-frame buffer per key of `fg_cols` (`bg_cols` is a subset of it)."""
    dev = fg_packed.device
    bg = torch.as_tensor(bgcolor, dtype=torch.float32, device=dev).reshape(3) / 255.0
    maps = {k: bg.expand(H * W, 3).clone() if k == "rgb" else torch.zeros((H * W, 3) if isinstance(c, slice) else (H * W,), device=dev)
            for k, c in fg_cols.items()}
    for k, c in fg_cols.items():
        maps[k][ray_mask] = fg_packed[:, c]
    for k, c in bg_cols.items():
        maps[k][ray_mask_bkg] = bg_packed[:, c]
    return maps


def render_frame(hos, frame: Dict, chunk_bkg: int = 8192, randomized: bool = False, group=None,
                 cache_prologue: bool = True, maps: bool = False, median: bool = False):
    """One frame of `free_view` / `test_metrics` / `progress` (M:1320-1458).  `frame` carries the keys of the reference's
    evaluation batch (freeview.py:284-335).  Returns `rendered` [H*W, 3] on the device (every rank holds the whole frame
    when `group` is given).  `randomized` is False in free_view/test_metrics and True in progress (M:720-723).

    `maps=True` returns a dict of whole-frame device buffers instead: `rgb` [H*W,3] (the same `rendered`), `alpha` [H*W],
    `depth` [H*W] (`alpha_onlyfg, depth_onlyfg` / `bkg_alpha, bkg_depth` of the reference's frame loops, M:809-835) and the
    human-object layer `rgb_human` [H*W,3] (premultiplied) / `alpha_human` [H*W]; see `assemble_maps`.  `median=True` (with
    `maps=True` only) adds `depth_median` [H*W], the median depth of each ray's composite (`HOSNeRF.render(median=True)`), 0 on
    pixels of neither ray list: one more column of the packed lists, so still one gather per list."""
    if median and not maps:
        raise ValueError("render_frame(median=True) is one of the maps: pass maps=True as well")
    if maps:
        fg_cols, bg_cols = (FG_MEDIAN_COLS, BG_MEDIAN_COLS) if median else (FG_MAP_COLS, BG_MAP_COLS)
        want = {"maps": True, "median": median}
        packed = pack_maps
    else:                                          # the differentiable composite's entry, as `bench.py` times it: no `maps` argument
        fg_cols = bg_cols = RGB_COLS
        want = {}
        packed = lambda out, cols: out["rgb"] if isinstance(out, dict) else out
    H, W = int(frame["img_height"]), int(frame["img_width"])
    dev = frame["rays_o_bkg"].device
    per_frame = {k: frame[k] for k in FRAME_KEYS if k in frame}
    per_frame["is_train"] = False

    def ray_list(tensors, n, render, cols):
        """This rank's share of one ray list through `render`, `chunk_bkg` rays at a time -> [rays of the share, columns of `cols`]."""
        tensors = _local(tensors, n, group)
        parts = []
        for i in range(0, tensors["radii"].shape[0], chunk_bkg):
            sl = slice(i, i + chunk_bkg)
            parts.append(packed(render({k: (v[:, sl] if k == "rays" else v[sl]).contiguous() for k, v in tensors.items()}), cols))
        return torch.cat(parts, 0) if parts else torch.zeros(0, sum(3 if isinstance(c, slice) else 1 for c in cols.values()), device=dev)

    with evaluating(hos):
        # ---- rays through the human box: both branches + merge (M:1322-1432)
        n_fg = frame["rays_o_bkg"].shape[0]
        pro = hos.human.frame_prologue(**per_frame) if (cache_prologue and n_fg > 0) else None
        fg = ray_list({k: frame[k] for k in ("rays", "near", "far", "rays_o_bkg", "rays_d_bkg", "viewdirs_bkg", "radii")}, n_fg,
                      lambda b: hos.render({**per_frame, **b}, randomized=randomized, is_train=False, prologue=pro, with_cycle=False, **want), fg_cols)
        # ---- rays that miss it: background only (M:1434-1452)
        n_bg = frame["rays_o_bkg_only"].shape[0]
        bg = ray_list({"rays_o": frame["rays_o_bkg_only"], "rays_d": frame["rays_d_bkg_only"], "viewdirs": frame["viewdirs_bkg_only"],
                       "radii": frame["radii_bkg_only"]}, n_bg,
                      lambda b: hos.render_bkg_only({**b, "times": frame["time"]}, randomized=randomized, is_train=False, **want), bg_cols)
        if group is not None:
            fg = gather_frame(fg, n_fg, group) if n_fg else fg
            bg = gather_frame(bg, n_bg, group) if n_bg else bg
    frame_maps = _assemble(H, W, frame.get("bgcolor", (0.0, 0.0, 0.0)), frame["ray_mask"], frame["ray_mask_bkg"], fg, bg, fg_cols, bg_cols)
    return frame_maps if maps else frame_maps["rgb"]                              # M:1311-1313, :1456-1459


@contextlib.contextmanager
def per_sample_outputs(net):
    """A stage-2 `Network` composites its own samples and returns the maps, not the per-sample radiance (`human_rgbsigma`, `z_vals`,
    `pts_mask`, `rays_d`) that `render_human_frame` composites itself -- with the same `ops.raw2outputs` arguments, so the colours
    are the same.  Under `no_grad` its `stage` selects nothing but that return layout, so for the duration of the block it answers
    as stage 3 does.  A stage-3 network is left as it is."""
    stage = net.stage
    net.stage = 3
    try:
        yield net
    finally:
        net.stage = stage


def render_human_frame(hos, frame: Dict, maps: bool = False, want_u8: bool = False, median: bool = False):
    """One frame of `test_tpose` (M:614-629): the human-object network alone over every ray of the frame's box, `_raw2outputs`
    over the frame's background colour, no scene.  `frame` is a `tpose.tpose_frame` batch (the reference's T-pose batch plus the
    `slot` / `count` of `rays.frame_rays_compact`, `time` and `iter_val`).  Under `evaluating(hos)`:
      1. one `frame_prologue`;
      2. the human network over all `count` rays with `with_cycle=False` (it chunks by `cfg.chunk` itself);
      3. `ops.raw2outputs(human_rgbsigma, z_vals, rays_d, pts_mask, bgcolor)` (M:621-623);
      4. `rays.paint_frame` (M:610-612, :627, :629).
    Returns the float frame [H*W,3]; `maps=True` returns a dict `rgb` / `alpha` [H*W] / `depth` [H*W] (`alpha_`, `depth_` of the same
    `_raw2outputs` call, painted over 0).  `want_u8=True` adds the paint kernel's 8-bit frame: a (frame-or-dict, uint8 [H*W,3])
    pair.  `median=True` (with `maps=True` only) adds `depth_median` [H*W], the median depth of the human samples' composite
    (`ops.raw2outputs_median`, the same launch), painted over 0.  A frame whose camera misses the box (`count == 0`) launches nothing
    but the paint."""
    from . import ops
    if median and not maps:
        raise ValueError("render_human_frame(median=True) is one of the maps: pass maps=True as well")
    H, W = int(frame["img_height"]), int(frame["img_width"])
    slot, n = frame["slot"], int(frame["count"])
    dev = slot.device
    bgcolor = frame["bgcolor"]
    rgb = acc = depth = med = None
    human = getattr(hos, "human", hos)                   # a `HOSNeRF`, or the human-object network itself (stage 2's `lit.human`)
    if n > 0:
        per_frame = {k: frame[k] for k in FRAME_KEYS if k in frame}
        per_frame["is_train"] = False
        with evaluating(hos), per_sample_outputs(human):
            pro = human.frame_prologue(**per_frame)
            out = human(rays=frame["rays"], near=frame["near"], far=frame["far"], prologue=pro, with_cycle=False, **per_frame)
            bg = torch.as_tensor(bgcolor, dtype=torch.float32, device=dev)
            if median:
                m = ops.raw2outputs_median(out["human_rgbsigma"], out["z_vals"], out["rays_d"], out["pts_mask"], bg)
                rgb, acc, depth, med = m["rgb"], m["acc"], m["depth"], m["depth_median"]
            else:
                rgb, acc, _, depth = ops.raw2outputs(out["human_rgbsigma"], out["z_vals"], out["rays_d"], out["pts_mask"], bg)
    rendered, u8 = rays_mod.paint_frame(slot, rgb, bgcolor, H, W, want_u8=want_u8)
    if maps:
        zero = torch.zeros(3, device=dev)
        layers = {"alpha": acc, "depth": depth, **({"depth_median": med} if median else {})}
        rendered = {"rgb": rendered}
        for k, x in layers.items():
            rendered[k] = rays_mod.paint_frame(slot, None if x is None else x[:, None].expand(-1, 3), zero, H, W, want_u8=False)[0][:, 0].contiguous()
    return (rendered, u8) if want_u8 else rendered


BKGD_FRAME_MAPS = {"rgb": "rgb", "alpha": "acc", "depth": "depth", "depth_median": "depth_median"}     # frame key -> rendering key


def render_bkgd_frame(model, bank, frame_or_pose, chunk: int, train_frac: float, near: float, far: float, maps: bool = False):
    """One whole frame of the stage-1 background model, the loop of `trainer.test` / `trainer.predict` over `render_rays`
    (1st_State-Conditional_Scene/src/model/mipnerf360/model.py:516-534): for each `chunk` (= `LitData.chunk`) rays of the frame,
    `model(batch, train_frac, False, False, near, far)` and the last level's colour.  `model` is the `MipNeRF360`, `bank` a
    `raybank.RayBank`; `frame_or_pose` is a scene image index i (`bank.frame`: its own camera, time and pixels) or `("pose", k)`
    (`bank.render_pose`: camera k of the render path).  Returns [H*W,3] on the device.

    `randomized=False` reaches the resampling kernel (no jitter: bin centres, `sample_intervals`), the only place the reference's
    forward uses it with its shipped configuration (density / bottleneck noise are 0 and refused otherwise by `MipNeRF360MLP`);
    `is_train=False` only selects how the reference evaluates the contraction's Jacobian (helper.py:40-52, the same numbers), so
    the model needs nothing further for this mode.  No autograd, and the module's training flag is left as it was.

    `maps=True` returns a dict of whole-frame device buffers instead: `rgb` [H*W,3] (the same colours), `alpha` [H*W] (the last
    level's `acc`, under stage 3's key name), `depth` [H*W] (sum w t_mid, not divided by alpha) and `depth_median` [H*W] (the
    distance at which the weight CDF crosses 0.5), all from `model(..., maps=True)`: the same chunk loop, one `cat` per key."""
    if isinstance(frame_or_pose, tuple):
        kind, idx = frame_or_pose
        if kind not in ("frame", "pose"):
            raise ValueError(f"frame_or_pose: {frame_or_pose!r}")
    else:
        kind, idx = "frame", frame_or_pose
    rays = bank.frame if kind == "frame" else bank.render_pose
    n = bank.H * bank.W
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be positive")
    parts = []
    with torch.no_grad():
        for start in range(0, n, chunk):
            batch = rays(int(idx), start, min(chunk, n - start))
            rend, _ = model(batch, train_frac, False, False, near, far, maps=maps)
            parts.append(rend[-1])
    if maps:
        return {key: torch.cat([p[k] for p in parts], 0) for key, k in BKGD_FRAME_MAPS.items()}
    return torch.cat([p["rgb"] for p in parts], 0)


def psnr_each(img_pred: torch.Tensor, img_gt: torch.Tensor) -> float:
    """`psnr_each` of the stage-1 launcher (1st_State-Conditional_Scene/src/model/interface.py:42-50) for one image: both clipped to
    0..1, then -10 log10(mean squared error)."""
    mse = torch.mean((img_pred.double().clamp(0.0, 1.0) - img_gt.double().clamp(0.0, 1.0)) ** 2).item()
    return -10.0 * math.log(mse) / math.log(10.0)


def bkgd_results(psnrs) -> Dict[str, Dict[str, float]]:
    """What `write_stats` (interface.py:121-132) leaves in results.json for `eval_test_only` (:77-89), PSNR only: SSIM and LPIPS
    are not computed for stage 1 and are not mentioned."""
    mean = float(np.mean(np.asarray(psnrs, dtype=np.float64)))
    return {"PSNR": {"mean": mean, "test": mean}}


def write_bkgd_results(path: str, psnrs) -> Dict[str, Dict[str, float]]:
    import json
    d = bkgd_results(psnrs)
    with open(path, "w") as fp:
        json.dump(d, fp, indent=4, sort_keys=True)          # interface.py:131-132
    return d


def psnr_metric(img_pred: torch.Tensor, img_gt: torch.Tensor) -> float:
    """M:101-112: -10 log10(mean squared error) over the whole frame, images in [0, 1]."""
    mse = torch.mean((img_pred.double() - img_gt.double()) ** 2).item()
    return -10.0 * math.log(mse) / math.log(10.0)


def truth_frame(frame: Dict) -> torch.Tensor:
    """`truth` of M:1314-1316, :1457-1460 from `target_rgbs` / `target_rgbs_bkg`."""
    H, W = int(frame["img_height"]), int(frame["img_width"])
    dev = frame["rays_o_bkg"].device
    bg = torch.as_tensor(frame.get("bgcolor", (0.0, 0.0, 0.0)), dtype=torch.float32, device=dev).reshape(3) / 255.0
    truth = bg.expand(H * W, 3).clone()
    truth[frame["ray_mask"]] = frame["target_rgbs"].to(dev).float()
    truth[frame["ray_mask_bkg"]] = frame["target_rgbs_bkg"].to(dev).float()
    return truth


def to_8b_image(image: torch.Tensor) -> torch.Tensor:
    """core/utils/image_util.py:28-29."""
    return (255.0 * image.clamp(0.0, 1.0)).to(torch.uint8)
