"""The canonical human-object of one object state as a triangle mesh (this build's addition; the reference has no counterpart, as
it has none for `depth_median`).

The field, for a canonical point x and the object state s that `select_state` picks for a time exactly as a frame does:

    alpha(x) = mask(x) * (1 - exp(-sigma_s(x) * h))

`sigma_s` is column 3 of `Network._canonical_fwd(x, s)`, `mask` the sum over the bone channels of the motion-weight volume at x --
what `human_sample_warp` writes as `mask` when every bone transform is the identity -- and `h` the grid spacing: the per-sample
alpha of `_raw2outputs` (M:73-94, masked alphas) for a sample as long as a voxel.  At the default level 0.5 a ray that crosses one
voxel loses half its transmittance.  The canonical MLP takes no view direction, so its colour is a per-point albedo, interpolated
to the mesh vertices.

This is the canonical field BEFORE the non-rigid offset: the T-pose turntable (`tpose`, `eval.render_human_frame`) warps every
sample by the non-rigid MLP at `dst_posevec = 1e-2`, the mesh does not.

Both defaults, level 0.5 and resolution 256, are parameters and have not been measured on a real scene.

The isosurface is marching tetrahedra on the Kuhn split of every cell (hos_mesh.hip): no ambiguous case, so wherever the
outermost vertex layer is outside -- `hos_grid_alpha` writes 0 there -- the surface is a closed, oriented 2-manifold."""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch

from . import ops
from .eval import evaluating
from .mipnerf360 import select_state

THIN_ROWS = 16384            # from this many rows on the canonical MLP runs on the thin kernels (ops.thin_dgrad_rows)


def grid_of_box(bmin, bmax, resolution: int) -> Dict:
    """The grid over the box [bmin, bmax]: cubic voxels of h = longest extent / resolution, per axis ceil(extent / h) + 1 vertices
    over the box plus one layer outside it on each side -> {"origin" float32 [3] (= bmin - h), "spacing" float32,
    "dims" (Nx, Ny, Nz)}.  Vertex i of an axis sits at origin + float32(i) * spacing."""
    resolution = int(resolution)
    if resolution < 2:
        raise ValueError(f"grid_of_box: resolution {resolution} < 2")
    lo, hi = np.asarray(bmin, dtype=np.float32).reshape(3), np.asarray(bmax, dtype=np.float32).reshape(3)
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    if not (np.all(np.isfinite(ext)) and np.all(ext > 0)):
        raise ValueError(f"grid_of_box: empty or non-finite box {lo} .. {hi}")
    h = np.float32(ext.max() / resolution)
    # cells per axis: ceil(extent / h), where a quotient within 1e-4 of an integer is that integer (h is rounded to fp32, so the
    # longest axis gives resolution +- 1e-7 * resolution)
    cells = [max(1, int(math.ceil(e / float(h) - 1e-4))) for e in ext]
    return {"origin": lo - h, "spacing": h, "dims": tuple(c + 3 for c in cells)}


def canonical_field(net, const: Dict[str, torch.Tensor], time: float, resolution: int = 256, chunk: int = 1 << 18) -> Dict:
    """alpha [Nz,Ny,Nx] and rgb [Nz,Ny,Nx,3] of `net` (a `human_nerf.Network`, stage 2 or 3) on `grid_of_box` of the canonical box,
    for the object state of `time`; `const` is `TposeTurn.const`.  Under `evaluating`, `no_grad` and `ops.guarded_forward`; the
    motion-weight volume is built once, the canonical MLP runs over chunks of `chunk` >= 16384 vertices (the last chunk is moved
    back to end at the last vertex, so every launch has a full chunk's rows and stays on the thin kernels)."""
    chunk = int(chunk)
    if chunk < THIN_ROWS:
        raise ValueError(f"canonical_field: chunk {chunk} < {THIN_ROWS} rows (the thin kernels' lower bound)")
    bmin, bscale = const["cnl_bbox_min_xyz"].contiguous(), const["cnl_bbox_scale_xyz"].contiguous()
    dev = bmin.device
    grid = grid_of_box(bmin.cpu().numpy(), const["cnl_bbox_max_xyz"].cpu().numpy(), resolution)
    origin, h, dims = grid["origin"], grid["spacing"], grid["dims"]
    Nx, Ny, Nz = dims
    N = Nx * Ny * Nz
    state = select_state(float(time), net.transitions_times)
    K = int(net.cfg.total_bones)
    alpha = torch.empty(Nz, Ny, Nx, device=dev)
    rgb = torch.empty(Nz, Ny, Nx, 3, device=dev)

    def run():
        vol = net._motion_weight_volume(const["motion_weights_priors"]).contiguous()       # [K+1,V,V,V], once per call
        rows = min(chunk, N)
        for c0 in range(0, N, rows):
            first = min(c0, N - rows)
            pts = ops.grid_points(origin, h, dims, first, rows, device=dev)
            raw, _ = net._canonical_fwd(pts, state, save=False)
            ops.grid_alpha(raw, vol, bmin, bscale, origin, h, dims, first, alpha, rgb, K=K)

    with evaluating(net):
        ops.guarded_forward(net, dev, run)
    return {"alpha": alpha, "rgb": rgb, "origin": origin, "spacing": h, "dims": dims, "state": state}


def mesh_measures(vertices: torch.Tensor, faces: torch.Tensor):
    """(signed volume 1/6 sum v0 . (v1 x v2), area) of a triangle mesh, accumulated in float64 on the device."""
    if faces.shape[0] == 0:
        return 0.0, 0.0
    v = vertices.double()[faces.long()]                    # [F,3,3]
    a, b, c = v[:, 0], v[:, 1], v[:, 2]
    volume = (a * torch.linalg.cross(b, c)).sum() / 6.0
    area = torch.linalg.cross(b - a, c - a).norm(dim=1).sum() / 2.0
    return float(volume), float(area)


def extract(net, turn, time: float, resolution: int = 256, level: float = 0.5, chunk: int = 1 << 18) -> Dict:
    """The mesh of the canonical human-object at `time`'s object state: `canonical_field` on `turn` (a `tpose.TposeTurn`: canonical
    box, joints and priors), then `ops.march_tets` at `level`.  Returns `vertices` f32 [V,3], `faces` int32 [F,3] and `colors` uint8
    [V,3] (the 8-bit truncation of `to_8b_image`) on the device, `origin`, `spacing`, `dims`, `state`, the signed `volume` and
    the `area` as floats, and the field it was extracted from (`alpha` [Nz,Ny,Nx], `rgb` [Nz,Ny,Nx,3]).  `level` and `resolution` are unmeasured defaults (module docstring)."""
    field = canonical_field(net, turn.const, time, resolution, chunk)
    vertices, colors, faces = ops.march_tets(field["alpha"], level, field["origin"], field["spacing"], rgb=field["rgb"])
    volume, area = mesh_measures(vertices, faces)
    return {"vertices": vertices, "faces": faces, "colors": (255.0 * colors.clamp(0.0, 1.0)).to(torch.uint8), "origin": field["origin"],
            "spacing": float(field["spacing"]), "dims": field["dims"], "state": int(field["state"]), "volume": volume, "area": area,
            "level": float(level), "alpha": field["alpha"], "rgb": field["rgb"]}
