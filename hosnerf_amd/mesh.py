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
outermost vertex layer is outside -- `hos_grid_alpha` writes 0 there -- the surface is a closed, oriented 2-manifold.

The frame mesh (`frame_field`, `extract_frame`): the same subject as it stands in ONE frame -- posed, with that frame's
pose-dependent deformation, in the body frame of the frame's rays or in the coordinates of the scene.  Take a frame with pose
(`dst_Rs`, `dst_Ts`, `dst_posevec`), time t and box `mesh_infos[name]["bbox"]`: the body frame of the item's `rays`, the space
`frame_rays` tests against.  With pro = `net.frame_prologue(...)` at `is_train=False` and `iter_val=1e7` (as the evaluation frames
of `dataset.SceneItems`), for a body-frame point p of `grid_of_box(bbox.min, bbox.max, resolution)` (spacing h):

    (x_skel, mask) = backward LBS of p         # N:304-355, the K-loop of human_sample_warp_kernel on pro["R_b"], pro["T_b"], pro["vol"]
    cnl            = net._nonrigid_fwd(net._nr, x_skel, pro["cond"], pro["band_w"], save=False)[0]
    raw            = net._canonical_fwd(cnl, pro["state"], save=False)[0]
    alpha(p)       = 0 on the outermost vertex layer, else mask * (1 - exp(-raw[3] * h));   colour raw[:3]

and alpha(p) = 0 as well on a vertex layer past the box (`grid_of_box` rounds an extent up to whole voxels, so a shorter axis can
have one; `clip_to_box`): the renderer's rays are cut to the box, and every mesh vertex then lies within the box grown by h.  This is
the masked alpha of `_raw2outputs` (M:73-94) for a sample of length h at p: what `render_human_frame` and the stage-3 merge
composite for that frame.  The field is taken THROUGH THE BACKWARD WARP, the one the renderer samples; canonical vertices pushed
forward by `lbs_forward` would follow the approximate inverse the cycle loss trains and would not sit where the rendered pixels are.
The canonical mesh is the special case of identity transforms and no non-rigid offset.  Level 0.5 and resolution 256 are the same
parameters, as unmeasured on a real scene as they are for the canonical mesh.  Each frame is marched on its own: there is no vertex
correspondence between frames -- the tracked mesh below is the counterpart that has it.

The tracked mesh (`track`): ONE topology per object state, posed per frame.  The template is the canonical mesh of the state
(`extract`); for a frame of that state every template vertex c is carried to the body-frame point p with

    G(p) = nonrigid(x_skel(p)) = c              # x_skel: the frame's backward LBS, the map the renderer samples through

i.e. the renderer's backward map is INVERTED per vertex, not replaced by `lbs_forward` (which only supplies the first guess).  The
rigid part x_skel(p) = c - delta is solved by Newton's method on the trilinear motion-weight volume with the analytic Jacobian
(`ops.warp_invert`, hos_track.hip), the non-rigid offset delta = G(p) - x_skel(p) by a plain fixed point around it (`outer` rounds).
That fixed point converges where the offset is a contraction (small against a voxel of the volume, as the reference initialises it);
an offset field that folds space (det(I + d offset / dx) <= 0) has no inverse, and nothing converges on it.  Whether a trained
scene stays in the convergent regime is unmeasured: `residual` and `converged` are returned per vertex so that it can be seen.
What the tracked surface is: on the template alpha_c(c) = mask_c(c) (1 - exp(-sigma h)) = level; at the tracked point the frame's
field is mask(p) (1 - exp(-sigma h)) = level * mask(p) / mask_c(c).  So a tracked vertex lies on the frame's own isosurface exactly
where the posed and the canonical mask agree; `mask` and `mask_canonical` are both returned so that their ratio can be seen.
Tracking is per object state: the states have different canonical fields, hence different templates and no correspondence across
a transition.  Tracked normals (`normals=True`) are the normalised J^T n_c, J = d x_skel / dp at p and n_c the template's normal: the
pull-back of the canonical field's gradient through the rigid warp -- this NEGLECTS the Jacobian of the non-rigid offset and the
gradient of the mask ratio above.

Normals (`normals=True`, both meshes): per vertex the normalised negative central difference, step h, of the field's trilinear
interpolant (`ops.mesh_vertex_normals`), so they follow the field the surface was cut from and need no face adjacency.

The background mesh (`bkgd_field`, `extract_bkgd`): the scene those meshes stand in -- the state-conditional mip-NeRF-360 model of
stage 1, which is also stage 3's background branch -- per object state, in the background rays' own space: the scaled world that
`extract_frame(space="world")` writes, so the two load aligned.  For a point x of `grid_of_box(box)` (spacing h) and the state s of
`time`:

    sigma_s(x) = density of the NeRF MLP (`model.mlps[-1]`, not a proposal MLP) at the Gaussian (x, h^2/12 I)
    alpha(x)   = 0 on the outermost vertex layer, else 1 - exp(-sigma_s(x) * h)

h^2/12 is the per-axis variance of a uniform voxel of side h: the voxel plays the role the conical frustum plays for a ray sample
(`MipNeRF360MLP.query_points`, hos_encode_ipe_points: contraction, var J J^T, integrated positional encoding).  alpha is the alpha of
`compute_alpha_weights` (H:235-261) for a sample as long as a voxel: the definition of the human-object meshes without a mask.  The
box may reach beyond the unit ball, the contraction takes any point; the default launcher box is the cube [-1,1]^3 about the region
the contraction leaves linear.  The zero rim closes the surface, so WHERE THE BOX CUTS SOLID MATTER (the ground, a wall) THE MESH IS
CAPPED by faces on the box's walls: they are the box, not the scene.  The NeRF MLP's colour depends on the view direction: the
vertex colours come from a second query at the mesh vertices, each seen head-on (view direction = -normal; (0,0,-1) where the normal
is the zero vector).  Level 0.5 and resolution 256 are the same parameters, as unmeasured on a real scene as for the other two meshes.

Mesh components (`components`, `drop_floaters`; hos_components.hip): on a NeRF density field marching tetrahedra gives the subject or
the scene PLUS FLOATERS, small closed blobs of stray density, and every measure above counts them as if they were the object.  Two
vertices are connected when a face names both; `components` labels every vertex with the smallest vertex id of its connected
component (a definition that fixes the result whatever the GPU's scheduling), numbers the components densely by ascending root, and
measures each: vertices, faces, area, signed volume -- a NEGATIVE volume is the inner wall of a hollow, reported by its sign and
otherwise a component like any other.  `drop_floaters` keeps component c iff n_faces[c] >= min_faces and area[c] >= min_area_ratio *
max(area) and compacts the mesh to the kept ones in their original order.  The extractors take the same two thresholds
(`min_area_ratio`, `min_faces`; both 0 = nothing is labelled, the mesh is what it always was) and filter BEFORE the per-vertex work:
`extract_frame` before the normals and `to_space`, `extract_bkgd` before the colour query, so the NeRF MLP never runs on a dropped
vertex.  Normals and colours are functions of the vertex alone, so the kept vertices get the values they would have had.  A faces
row with a corner outside [0, V) is ignored and counted (`invalid_faces`).  Out of scope: filling cavities, merging components,
correspondence of components across frames; `track` tracks whatever template it is given."""
from __future__ import annotations

import contextlib
import math
from typing import Dict

import numpy as np
import torch

from . import ops
from .eval import FRAME_KEYS, evaluating
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


def _mesh_tensors(what: str, vertices, faces):
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise ValueError(f"{what}: vertices must be a float32 tensor [V,3], got {getattr(vertices, 'dtype', type(vertices))} "
                         f"{tuple(getattr(vertices, 'shape', ()))}")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{what}: faces must be an int32 tensor [F,3], got {getattr(faces, 'dtype', type(faces))} "
                         f"{tuple(getattr(faces, 'shape', ()))}")
    if faces.device != vertices.device:
        raise ValueError(f"{what}: vertices are on {vertices.device}, faces on {faces.device}")
    return vertices.contiguous(), faces.contiguous()


def components(vertices: torch.Tensor, faces: torch.Tensor) -> Dict:
    """The connected components of a triangle mesh on the device (`vertices` f32 [V,3], `faces` int32 [F,3]: a marched mesh, a tracked
    one, one read back with `formats.read_ply`): `label` int32 [V] (the smallest vertex id of the vertex's component), `component`
    int32 [V] (dense ids by ascending root), `face_component` int32 [F] (-1 for a face with a corner outside [0,V), which every
    kernel ignores), `count`, per component `n_vertices` / `n_faces` int64 [C] and `area` / `volume` float64 [C] (the terms of
    `mesh_measures`; bit-equal from run to run), `rounds` (hook + jump rounds the labelling took, the last one changing nothing)
    and `invalid_faces`.  `ops.mesh_label` then `ops.mesh_component_measures`; a vertex no face names is a component of its own."""
    vertices, faces = _mesh_tensors("components", vertices, faces)
    label, component, count, rounds, invalid = ops.mesh_label(faces, vertices.shape[0])
    face_component, n_vertices, n_faces, area, volume = ops.mesh_component_measures(vertices, faces, component, count)
    return {"label": label, "component": component, "face_component": face_component, "count": count, "n_vertices": n_vertices,
            "n_faces": n_faces, "area": area, "volume": volume, "rounds": rounds, "invalid_faces": invalid}


def _thresholds(what: str, min_area_ratio, min_faces):
    r, n = float(min_area_ratio), int(min_faces)
    if not (0.0 <= r <= 1.0) or n < 0 or n != min_faces:
        raise ValueError(f"{what}: min_area_ratio {min_area_ratio!r} must lie in [0, 1] and min_faces {min_faces!r} be an integer >= 0")
    return r, n


def keep_flags(comp: Dict, min_area_ratio: float = 0.0, min_faces: int = 0) -> torch.Tensor:
    """uint8 [C]: component c of `comp` (`components`) is kept iff n_faces[c] >= min_faces and area[c] >= min_area_ratio * max(area)."""
    r, n = _thresholds("keep_flags", min_area_ratio, min_faces)
    area = comp["area"]
    if area.numel() == 0:
        return torch.zeros(0, dtype=torch.uint8, device=area.device)
    return ((comp["n_faces"] >= n) & (area >= r * area.max())).to(torch.uint8)


def drop_floaters(m: Dict, min_area_ratio: float = 0.0, min_faces: int = 0) -> Dict:
    """The mesh dict `m` (as `extract` / `extract_frame` / `extract_bkgd` return it) without its floaters: component c is kept iff
    n_faces[c] >= min_faces and area[c] >= min_area_ratio * max(area).  With both thresholds 0 this is `m` itself, nothing is launched.
    Otherwise a copy whose `vertices`, `faces`, `colors` and `normals` are compacted to the kept components (`ops.mesh_compact`:
    original order, faces renumbered), `volume` / `area` recomputed by `mesh_measures`, and `components` added: `count`, `kept`,
    `V_dropped`, `F_dropped`, `area_dropped`, `volume_dropped`, `rounds`, `invalid_faces`, `negative_volume` (how many components
    have a negative volume: inner walls of hollows, kept or dropped by the same rule as any other).  A `body` mesh (`extract_frame(
    keep_body=True)`: the same topology) gets the same keep flags, the labelling runs once; `vertex_rgb` (`extract_bkgd`) is gathered
    like the normals.  Every other entry -- the field `alpha` /
    `rgb`, the grid, `state` -- passes through untouched."""
    r, n = _thresholds("drop_floaters", min_area_ratio, min_faces)
    if r == 0.0 and n == 0:
        return m
    vertices, faces = _mesh_tensors("drop_floaters", m["vertices"], m["faces"])
    comp = components(vertices, faces)
    keep = keep_flags(comp, r, n)
    pick = lambda d: ops.mesh_compact(keep, comp["component"], comp["face_component"], d["vertices"].contiguous(), d["faces"].contiguous(),
                                      d.get("colors"), d.get("normals"))
    out = dict(m)
    out["vertices"], out["faces"], out["colors"], out["normals"] = pick(m)
    out["volume"], out["area"] = mesh_measures(out["vertices"], out["faces"])
    if m.get("vertex_rgb") is not None:                     # `extract_bkgd`'s colours before truncation: per vertex, like the normals
        out["vertex_rgb"] = ops.mesh_compact(keep, comp["component"], comp["face_component"], vertices, faces, None, m["vertex_rgb"].contiguous())[3]
    if m.get("body") is not None:
        body = dict(m["body"])
        body["vertices"], body["faces"], body["colors"], body["normals"] = pick(m["body"])
        out["body"] = body
    gone = keep == 0
    out["components"] = {"count": int(comp["count"]), "kept": int(keep.sum()), "V_dropped": int(vertices.shape[0] - out["vertices"].shape[0]),
                         "F_dropped": int(faces.shape[0] - out["faces"].shape[0]), "area_dropped": float(comp["area"][gone].sum()),
                         "volume_dropped": float(comp["volume"][gone].sum()), "rounds": int(comp["rounds"]),
                         "invalid_faces": int(comp["invalid_faces"]), "negative_volume": int((comp["volume"] < 0).sum())}
    return out


def extract(net, turn, time: float, resolution: int = 256, level: float = 0.5, chunk: int = 1 << 18, normals: bool = False,
            min_area_ratio: float = 0.0, min_faces: int = 0) -> Dict:
    """The mesh of the canonical human-object at `time`'s object state: `canonical_field` on `turn` (a `tpose.TposeTurn`: canonical
    box, joints and priors), then `ops.march_tets` at `level`.  Returns `vertices` f32 [V,3], `faces` int32 [F,3] and `colors` uint8
    [V,3] (the 8-bit truncation of `to_8b_image`) on the device, `origin`, `spacing`, `dims`, `state`, the signed `volume` and
    the `area` as floats, and the field it was extracted from (`alpha` [Nz,Ny,Nx], `rgb` [Nz,Ny,Nx,3]).  `level` and `resolution` are unmeasured defaults (module docstring).
    `normals=True` adds `normals` f32 [V,3] (`ops.mesh_vertex_normals`; `None` otherwise); nothing else changes.
    `min_area_ratio` / `min_faces` above 0: `drop_floaters` of the result (adds `components`); at 0 the path is exactly the above."""
    _thresholds("extract", min_area_ratio, min_faces)
    field = canonical_field(net, turn.const, time, resolution, chunk)
    vertices, colors, faces = ops.march_tets(field["alpha"], level, field["origin"], field["spacing"], rgb=field["rgb"])
    volume, area = mesh_measures(vertices, faces)
    out = {"vertices": vertices, "faces": faces, "colors": (255.0 * colors.clamp(0.0, 1.0)).to(torch.uint8), "origin": field["origin"],
           "spacing": float(field["spacing"]), "dims": field["dims"], "state": int(field["state"]), "volume": volume, "area": area,
           "level": float(level), "alpha": field["alpha"], "rgb": field["rgb"],
           "normals": ops.mesh_vertex_normals(field["alpha"], field["origin"], field["spacing"], vertices) if normals else None}
    return drop_floaters(out, min_area_ratio, min_faces)


# ------------------------------------------------------------------------------------------ the frame mesh
SPACES = ("world", "body")


def layers_in_box(origin, spacing, dims, bmax):
    """Per axis the index of the first vertex layer BEYOND the box: `grid_of_box` rounds an extent that is no multiple of the spacing
    up, so on such an axis the last layer before the rim lies past `bmax` (by less than one spacing; a layer within 1e-4 spacings of
    `bmax` counts as on it, the tolerance of `grid_of_box`).  Positions are `grid_coord`'s: origin + float32(i) * spacing in fp32."""
    h = np.float32(spacing)
    o, hi = np.asarray(origin, dtype=np.float32).reshape(3), np.asarray(bmax, dtype=np.float32).reshape(3)
    out = []
    for a in range(3):
        c = (o[a] + np.arange(int(dims[a]), dtype=np.float32) * h).astype(np.float64)
        out.append(int(np.searchsorted(c, float(hi[a]) + 1e-4 * float(h), side="right")))
    return tuple(out)


def clip_to_box(alpha: torch.Tensor, origin, spacing, dims, bmax) -> torch.Tensor:
    """alpha [Nz,Ny,Nx] := +0 on every vertex layer beyond the box (`layers_in_box`), in place.  The renderer's rays are cut to the
    frame's box (`rays_intersect_3d_bbox`), so whatever the network says past it is never composited; and every mesh vertex then lies
    within the box grown by one spacing."""
    kx, ky, kz = layers_in_box(origin, spacing, dims, bmax)
    alpha[:, :, kx:] = 0.0
    alpha[:, ky:] = 0.0
    alpha[kz:] = 0.0
    return alpha


def frame_field(net, pose: Dict, resolution: int = 256, chunk: int = 1 << 18) -> Dict:
    """alpha [Nz,Ny,Nx] and rgb [Nz,Ny,Nx,3] of `net` (stage 2 or 3) on `grid_of_box` of the FRAME's box `pose["dst_bbox"]`
    (`min_xyz` / `max_xyz`, body frame), through the backward warp of the frame (module docstring).  `pose` is
    `dataset.SceneItems.frame_pose(idx)`: the per-frame keys of `eval.FRAME_KEYS` plus `dst_bbox`; `is_train` is False here whatever
    it holds, `iter_val` 1e7 unless given.  Under `evaluating`, `no_grad` and `ops.guarded_forward`; one `frame_prologue` per call,
    then per chunk of `chunk` >= 16384 vertices (the last one moved back, as `canonical_field`) `ops.grid_warp`, the non-rigid chain,
    the canonical MLP and `ops.grid_alpha_masked`; at the end `clip_to_box`: alpha is 0 on the layers past the box, as on the rim."""
    chunk = int(chunk)
    if chunk < THIN_ROWS:
        raise ValueError(f"frame_field: chunk {chunk} < {THIN_ROWS} rows (the thin kernels' lower bound)")
    bmin, bscale = pose["cnl_bbox_min_xyz"].contiguous(), pose["cnl_bbox_scale_xyz"].contiguous()
    dev = bmin.device
    box = pose["dst_bbox"]
    grid = grid_of_box(np.asarray(box["min_xyz"], dtype=np.float32), np.asarray(box["max_xyz"], dtype=np.float32), resolution)
    origin, h, dims = grid["origin"], grid["spacing"], grid["dims"]
    Nx, Ny, Nz = dims
    N = Nx * Ny * Nz
    per_frame = {k: pose[k] for k in FRAME_KEYS if k in pose}
    per_frame["is_train"] = False
    per_frame.setdefault("iter_val", 1e7)
    K = int(net.cfg.total_bones)
    alpha = torch.empty(Nz, Ny, Nx, device=dev)
    rgb = torch.empty(Nz, Ny, Nx, 3, device=dev)
    found = {}

    def run():
        pro = net.frame_prologue(**per_frame)                                                # once per call
        found["state"] = pro["state"]
        rows = min(chunk, N)
        for c0 in range(0, N, rows):
            first = min(c0, N - rows)
            x_skel, mask = ops.grid_warp(pro["R_b"], pro["T_b"], pro["vol"], bmin, bscale, origin, h, dims, first, rows, K=K)
            cnl, _ = net._nonrigid_fwd(net._nr, x_skel, pro["cond"], pro["band_w"], save=False)
            raw, _ = net._canonical_fwd(cnl, pro["state"], save=False)
            ops.grid_alpha_masked(raw, mask, origin, h, dims, first, alpha, rgb)
        clip_to_box(alpha, origin, h, dims, box["max_xyz"])

    with evaluating(net):
        ops.guarded_forward(net, dev, run)
    return {"alpha": alpha, "rgb": rgb, "origin": origin, "spacing": h, "dims": dims, "state": found["state"]}


def to_space(vertices: torch.Tensor, faces: torch.Tensor, normals, A) -> tuple:
    """A mesh under the affine map `A` [4,4]: v' = A[:3,:3] v + A[:3,3], evaluated in float64 and rounded once; normals turned by the
    linear part and renormalised (a zero normal stays zero) -- exact for a similarity, mirrored or not; where det A[:3,:3] < 0 two
    indices of every face are swapped, so that the orientation stays outward.  -> (vertices, faces, normals)."""
    A = torch.as_tensor(np.asarray(A, dtype=np.float64), device=vertices.device)
    L, t = A[:3, :3], A[:3, 3]
    v = (vertices.double() @ L.T + t).float()
    if normals is not None:
        n = normals.double() @ L.T
        length = n.norm(dim=1, keepdim=True)
        normals = torch.where(length > 0, n / length.clamp_min(1e-300), torch.zeros_like(n)).float()
    if float(torch.linalg.det(L)) < 0:
        faces = faces[:, [0, 2, 1]].contiguous()
    return v, faces, normals


def extract_frame(net, pose: Dict, resolution: int = 256, level: float = 0.5, space: str = "world", normals: bool = False,
                  chunk: int = 1 << 18, keep_body: bool = False, min_area_ratio: float = 0.0, min_faces: int = 0) -> Dict:
    """The mesh of the human-object as it stands in the frame of `pose` (`dataset.SceneItems.frame_pose`): `frame_field`, then
    `ops.march_tets` at `level`.  Returns what `extract` returns (`origin`, `spacing`, `dims` and the field `alpha` / `rgb` are the
    body-frame grid's) plus `space`, `to_world` (float32 [4,4] host array: `pose["newsmpl_to_scale_world"]`, the body frame -> the
    scene's scaled world; the identity for `space="body"`), `normals` (f32 [V,3] or None), `frame_name` and `time`.
    `space="world"` writes the vertices (and turns the normals) by `to_space`; `volume` and `area` are those of the returned
    vertices.  `level` and `resolution` are unmeasured defaults (module docstring).  `keep_body=True` adds `body`: the mesh BEFORE
    `to_space` (`vertices`, `faces`, `colors`, `normals` in the body frame, the space of the frame's rays: what `rasterize` takes
    with `SceneItems.frame_camera`), the very tensors for `space="body"`; nothing else changes.
    `min_area_ratio` / `min_faces` above 0: the marched mesh goes through `drop_floaters` BEFORE the normals and `to_space` (so `body`
    is the filtered mesh too) and `components` is added; at 0 the path is exactly the above."""
    if space not in SPACES:
        raise ValueError(f"extract_frame: space {space!r} is not one of {SPACES}")
    filtering = _thresholds("extract_frame", min_area_ratio, min_faces) != (0.0, 0)
    to_world = np.eye(4, dtype=np.float32)
    if space == "world":
        if pose.get("newsmpl_to_scale_world") is None:
            raise ValueError("extract_frame: space=\"world\" needs pose[\"newsmpl_to_scale_world\"], which this scene's cameras do not "
                             "give (no `smpl_to_scale_world`); use space=\"body\"")
        A = pose["newsmpl_to_scale_world"]
        to_world = np.ascontiguousarray(A.detach().cpu().numpy() if hasattr(A, "detach") else A, dtype=np.float32).reshape(4, 4)
    field = frame_field(net, pose, resolution, chunk)
    vertices, colors, faces = ops.march_tets(field["alpha"], level, field["origin"], field["spacing"], rgb=field["rgb"])
    colors8 = (255.0 * colors.clamp(0.0, 1.0)).to(torch.uint8)
    kept = None
    if filtering:
        kept = drop_floaters({"vertices": vertices, "faces": faces, "colors": colors8, "normals": None}, min_area_ratio, min_faces)
        vertices, faces, colors8 = kept["vertices"], kept["faces"], kept["colors"]
    vn = ops.mesh_vertex_normals(field["alpha"], field["origin"], field["spacing"], vertices) if normals else None
    body = {"vertices": vertices, "faces": faces, "colors": colors8, "normals": vn} if keep_body else None
    if space == "world":
        vertices, faces, vn = to_space(vertices, faces, vn, to_world)
    volume, area = mesh_measures(vertices, faces)
    time = pose.get("time")
    out = {"vertices": vertices, "faces": faces, "colors": colors8, "origin": field["origin"],
           "spacing": float(field["spacing"]), "dims": field["dims"], "state": int(field["state"]), "volume": volume, "area": area,
           "level": float(level), "alpha": field["alpha"], "rgb": field["rgb"], "normals": vn, "space": space, "to_world": to_world,
           "frame_name": pose.get("frame_name"), "time": None if time is None else float(time)}
    if keep_body:
        out["body"] = body
    if kept is not None:
        out["components"] = kept["components"]
    return out


# ------------------------------------------------------------------------------------------ the tracked mesh
def _padded_rows(x: torch.Tensor, rows: int) -> torch.Tensor:
    """`x` [n,...] repeated from its first row on up to `rows` rows (n >= 1), so that a short template still runs the MLP on the
    thin kernels; the copies are computed and dropped."""
    n = x.shape[0]
    if n >= rows:
        return x.contiguous()
    return x[torch.arange(rows, device=x.device) % n].contiguous()


def track(net, template: Dict, pose: Dict, outer: int = 6, iters: int = 4, tol=None, space: str = "world", normals: bool = False,
          chunk: int = 1 << 18) -> Dict:
    """The canonical mesh `template` (what `extract` returned for the object state of `pose`'s time) posed into the frame of `pose`
    (`dataset.SceneItems.frame_pose`) VERTEX BY VERTEX: for every template vertex c the body-frame point p with G(p) = c, G the
    renderer's backward map of the frame (module docstring, "The tracked mesh").  `outer` rounds of the fixed point, each one
    `ops.warp_invert` of at most `iters` Newton steps (tolerance `tol` / 4, steps of at most one voxel of the motion-weight volume)
    and one non-rigid chain; `tol` defaults to 1e-3 * template["spacing"].  Under `evaluating`, `no_grad` and `ops.guarded_forward`;
    one `frame_prologue` per call (`is_train` False, `iter_val` 1e7 unless given, as `frame_field`); per chunk of `chunk` >= 16384
    vertices (the last one moved back; a shorter template is padded with copies of its own rows).

    Returns `vertices` f32 [V,3] in `space` ("world" through `to_space`, as `extract_frame`; `to_world` likewise), `faces` and
    `colors`: the TEMPLATE's own tensors (faces flipped by `to_space` where it mirrors), `residual` f32 [V] = |G(p) - c|_2,
    `converged` bool [V] (the last inner solve converged, residual <= tol, never lost), `mask` f32 [V] (the posed mask at p),
    `mask_canonical` f32 [V] (the template's own mask at c), `cnl` f32 [V,3] (the device's G(p)), `normals` (f32 [V,3] with
    `normals=True`, which needs the template's; else None), `state`, `frame_name`, `time`, `volume`, `area` (of the returned
    vertices), `tol`, `space`, `to_world` and the template's `level`, `spacing`, `dims`.  A vertex that is lost in some round (no
    motion weight, a singular Jacobian, a non-finite residual) keeps its last finite p and is not converged."""
    if space not in SPACES:
        raise ValueError(f"track: space {space!r} is not one of {SPACES}")
    if pose.get("time") is None:
        raise ValueError("track: pose has no `time` (the object state of the frame is selected by it)")
    state = select_state(float(pose["time"]), net.transitions_times)
    if int(template["state"]) != int(state):
        raise ValueError(f"track: the template is of object state {int(template['state'])}, the frame at time {float(pose['time'])} of state "
                         f"{int(state)}: the states have different canonical fields, a template tracks within its own state only")
    if normals and template.get("normals") is None:
        raise ValueError("track: normals=True needs a template with normals (`extract(..., normals=True)`)")
    outer, iters, chunk = int(outer), int(iters), int(chunk)
    if outer < 1 or iters < 0:
        raise ValueError(f"track: outer {outer} < 1 or iters {iters} < 0")
    if chunk < THIN_ROWS:
        raise ValueError(f"track: chunk {chunk} < {THIN_ROWS} rows (the thin kernels' lower bound)")
    tol = 1e-3 * float(template["spacing"]) if tol is None else float(tol)
    if not tol > 0:
        raise ValueError(f"track: tol {tol} must be positive")
    to_world = np.eye(4, dtype=np.float32)
    if space == "world":
        if pose.get("newsmpl_to_scale_world") is None:
            raise ValueError("track: space=\"world\" needs pose[\"newsmpl_to_scale_world\"], which this scene's cameras do not "
                             "give (no `smpl_to_scale_world`); use space=\"body\"")
        A = pose["newsmpl_to_scale_world"]
        to_world = np.ascontiguousarray(A.detach().cpu().numpy() if hasattr(A, "detach") else A, dtype=np.float32).reshape(4, 4)
    c_all = template["vertices"]
    dev = c_all.device
    V = int(c_all.shape[0])
    bmin, bscale = pose["cnl_bbox_min_xyz"].contiguous(), pose["cnl_bbox_scale_xyz"].contiguous()
    per_frame = {k: pose[k] for k in FRAME_KEYS if k in pose}
    per_frame["is_train"] = False
    per_frame.setdefault("iter_val", 1e7)
    K = int(net.cfg.total_bones)
    out = {"p": torch.zeros(V, 3, device=dev), "cnl": torch.full((V, 3), float("nan"), device=dev), "mask": torch.zeros(V, device=dev),
           "mask_canonical": torch.zeros(V, device=dev), "residual": torch.full((V,), float("inf"), device=dev),
           "converged": torch.zeros(V, dtype=torch.bool, device=dev), "jac": torch.zeros(V, 3, 3, device=dev) if normals else None}

    def run():
        pro = net.frame_prologue(**per_frame)                                                # once per call
        vol = pro["vol"]
        max_step = 2.0 / float(bscale.min()) / (int(vol.shape[-1]) - 1)                      # one voxel: longest box extent / (V - 1)
        eye, zero = torch.eye(3, device=dev).expand(K, 3, 3).contiguous(), torch.zeros(K, 3, device=dev)
        padded = _padded_rows(c_all, THIN_ROWS)
        n = padded.shape[0]
        rows = min(chunk, n)
        for c0 in range(0, n, rows):
            first = min(c0, n - rows)
            c = padded[first:first + rows].contiguous()
            p = ops.lbs_forward(c, pro["R_f"], pro["T_f"], pro["vol_cl"], bmin, bscale, K)
            delta = torch.zeros_like(c)
            alive = torch.ones(rows, dtype=torch.bool, device=dev)
            status = torch.full((rows,), ops.TRACK_LOST, dtype=torch.int32, device=dev)
            cnl, mask, res = torch.full_like(c, float("nan")), torch.zeros(rows, device=dev), torch.full((rows,), float("inf"), device=dev)
            for _ in range(outer):
                p_o, x_o, m_o, _, st_o = ops.warp_invert(c - delta, p, pro["R_b"], pro["T_b"], vol, bmin, bscale, K=K, iters=iters,
                                                         tol=tol / 4.0, max_step=max_step)
                cnl_o, _ = net._nonrigid_fwd(net._nr, x_o, pro["cond"], pro["band_w"], save=False)
                ok = alive & torch.isfinite(p_o).all(dim=1)                                  # a frozen row, or a step that blew up: keep
                ok3 = ok[:, None]
                p, cnl, delta = torch.where(ok3, p_o, p), torch.where(ok3, cnl_o, cnl), torch.where(ok3, cnl_o - x_o, delta)
                mask, res = torch.where(ok, m_o, mask), torch.where(ok, (cnl_o - c).norm(dim=1), res)
                status = torch.where(ok, st_o, status)
                alive = ok & (st_o != ops.TRACK_LOST)
            live = slice(0, max(0, min(rows, V - first)))                                    # the rows that are template vertices
            dst = slice(first, first + live.stop)
            out["p"][dst], out["cnl"][dst], out["mask"][dst], out["residual"][dst] = p[live], cnl[live], mask[live], res[live]
            out["converged"][dst] = (alive & (status == ops.TRACK_CONVERGED) & (res <= tol))[live]
            out["mask_canonical"][dst] = ops.warp_invert(c, c, eye, zero, vol, bmin, bscale, K=K, iters=0, tol=tol, max_step=max_step)[2][live]
            if normals:
                out["jac"][dst] = ops.warp_invert(c, p.contiguous(), pro["R_b"], pro["T_b"], vol, bmin, bscale, K=K, iters=0, tol=tol,
                                                  max_step=max_step, want_jac=True)[5][live]

    if V > 0:
        with evaluating(net):
            ops.guarded_forward(net, dev, run)
    vn = None
    if normals:
        n = torch.einsum("vab,va->vb", out["jac"].double(), template["normals"].double())    # J^T n_c: the gradient pulled back
        length = n.norm(dim=1, keepdim=True)
        vn = torch.where(torch.isfinite(length) & (length > 0), n / length.clamp_min(1e-300), torch.zeros_like(n)).float()
    vertices, faces = out["p"], template["faces"]
    if space == "world":
        vertices, faces, vn = to_space(vertices, faces, vn, to_world)
    volume, area = mesh_measures(vertices, faces)
    time = float(pose["time"])
    return {"vertices": vertices, "faces": faces, "colors": template["colors"], "normals": vn, "residual": out["residual"],
            "converged": out["converged"], "mask": out["mask"], "mask_canonical": out["mask_canonical"], "cnl": out["cnl"],
            "state": int(state), "frame_name": pose.get("frame_name"), "time": time, "volume": volume, "area": area, "tol": tol,
            "space": space, "to_world": to_world, "level": template.get("level"), "spacing": float(template["spacing"]),
            "dims": template["dims"]}


# ------------------------------------------------------------------------------------------ the background mesh
HEAD_ON_FALLBACK = (0.0, 0.0, -1.0)          # the view direction of a vertex whose normal is the zero vector


@contextlib.contextmanager
def _evaluating_bkgd(model):
    """`evaluating` for a `MipNeRF360` (it has no `cfg.perturb` to silence): eval mode, no autograd."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            yield model
    finally:
        model.train(was_training)


def _box_corners(box):
    b = np.asarray(box, dtype=np.float64).reshape(-1)
    if b.shape != (6,):
        raise ValueError(f"box must be (xmin, ymin, zmin, xmax, ymax, zmax), got {box!r}")
    return b[:3], b[3:]


def voxel_variance(spacing) -> float:
    """h^2 / 12 in fp32: the per-axis variance of a uniform voxel of side h, the `var` of every background-mesh query."""
    h = np.float32(spacing)
    return float(np.float32(h * h) / np.float32(12.0))


def bkgd_field(model, box, time: float, resolution: int = 256, chunk: int = 1 << 18) -> Dict:
    """alpha [Nz,Ny,Nx] of the background `model` (a `MipNeRF360`: stage 1's, or `HOSNeRF.model`) on `grid_of_box` of `box` =
    (xmin, ymin, zmin, xmax, ymax, zmax), for the object state of `time` (module docstring).  Under eval mode, `no_grad` and
    `ops.guarded_forward`; per chunk of `chunk` vertices (the last one shorter) `ops.grid_points`, the NeRF MLP's `query_points` with
    var = h^2/12 and `ops.grid_alpha_density`.  The view head runs on a constant direction and its colours are dropped (a few
    percent of the trunk's work).  Also returns `density` [Nz,Ny,Nx], what alpha was computed from."""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"bkgd_field: chunk {chunk} < 1")
    bmin, bmax = _box_corners(box)
    grid = grid_of_box(bmin, bmax, resolution)
    origin, h, dims = grid["origin"], grid["spacing"], grid["dims"]
    Nx, Ny, Nz = dims
    N = Nx * Ny * Nz
    mlp = model.mlps[-1]
    dev = model.flat_param.device
    state = select_state(float(time), mlp.transitions_times)
    var = voxel_variance(h)
    alpha = torch.empty(Nz, Ny, Nx, device=dev)
    density = torch.empty(Nz, Ny, Nx, device=dev)
    flat = density.view(-1)
    view = torch.tensor([HEAD_ON_FALLBACK], device=dev)

    def run():
        for first in range(0, N, chunk):
            rows = min(chunk, N - first)
            pts = ops.grid_points(origin, h, dims, first, rows, device=dev)
            d = mlp.query_points(pts, var, view.expand(rows, 3).contiguous(), float(time))["density"]
            flat[first:first + rows] = d
            ops.grid_alpha_density(d, h, dims, first, alpha)

    with _evaluating_bkgd(model):
        ops.guarded_forward(model, dev, run)
    return {"alpha": alpha, "density": density, "origin": origin, "spacing": h, "dims": dims, "state": state, "var": var,
            "box": [float(x) for x in bmin] + [float(x) for x in bmax]}


def head_on_viewdirs(normals: torch.Tensor) -> torch.Tensor:
    """-normal per vertex, `HEAD_ON_FALLBACK` where the normal is the exact zero vector."""
    zero = (normals == 0).all(dim=1, keepdim=True)
    return torch.where(zero, torch.tensor(HEAD_ON_FALLBACK, device=normals.device).expand_as(normals), -normals).contiguous()


def extract_bkgd(model, box, time: float, resolution: int = 256, level: float = 0.5, normals: bool = True, chunk: int = 1 << 18,
                 min_area_ratio: float = 0.0, min_faces: int = 0) -> Dict:
    """The mesh of the background at `time`'s object state inside `box`: `bkgd_field`, `ops.march_tets` at `level`,
    `ops.mesh_vertex_normals`, then the colours from a second `query_points` at the vertices (same var, view direction
    `head_on_viewdirs`).  Returns what `extract` returns -- `vertices` f32 [V,3] in the background rays' space (the scaled world),
    `faces` int32 [F,3], `colors` uint8 [V,3] (the truncation of `to_8b_image`), `normals` f32 [V,3] (None with `normals=False`: they
    are computed regardless, the colours need them), `origin`, `spacing`, `dims`, `state`, `volume`, `area`, `level`, `alpha` -- plus
    `vertex_rgb` f32 [V,3] (the colours before truncation), `density`, `var` and `box`.  `level` and `resolution` are unmeasured
    defaults; the surface is capped where the box cuts solid matter (module docstring).
    `min_area_ratio` / `min_faces` above 0: the marched mesh goes through `drop_floaters` BEFORE the normals and the colour query, so
    the NeRF MLP does not run on a dropped vertex, and `components` is added; at 0 the path is exactly the above."""
    filtering = _thresholds("extract_bkgd", min_area_ratio, min_faces) != (0.0, 0)
    field = bkgd_field(model, box, time, resolution, chunk)
    vertices, _, faces = ops.march_tets(field["alpha"], level, field["origin"], field["spacing"])
    kept = None
    if filtering:
        kept = drop_floaters({"vertices": vertices, "faces": faces, "colors": None, "normals": None}, min_area_ratio, min_faces)
        vertices, faces = kept["vertices"], kept["faces"]
    vn = ops.mesh_vertex_normals(field["alpha"], field["origin"], field["spacing"], vertices)
    V = vertices.shape[0]
    dev = vertices.device
    rgb = torch.empty(V, 3, device=dev)
    mlp = model.mlps[-1]
    view = head_on_viewdirs(vn)

    def run():
        for first in range(0, V, int(chunk)):
            sl = slice(first, min(first + int(chunk), V))
            rgb[sl] = mlp.query_points(vertices[sl].contiguous(), field["var"], view[sl].contiguous(), float(time))["rgb"]

    if V > 0:
        with _evaluating_bkgd(model):
            ops.guarded_forward(model, dev, run)
    volume, area = mesh_measures(vertices, faces)
    out = {"vertices": vertices, "faces": faces, "colors": (255.0 * rgb.clamp(0.0, 1.0)).to(torch.uint8), "origin": field["origin"],
           "spacing": float(field["spacing"]), "dims": field["dims"], "state": int(field["state"]), "volume": volume, "area": area,
           "level": float(level), "alpha": field["alpha"], "normals": vn if normals else None, "vertex_rgb": rgb,
           "density": field["density"], "var": field["var"], "box": field["box"]}
    if kept is not None:
        out["components"] = kept["components"]
    return out


# ------------------------------------------------------------------------------------------ the meshes seen again: raster and fit
RASTER_MAPS = ("depth", "mask", "face", "rgb", "normal", "shaded")
FIT_KEYS = ("iou", "area_mesh", "area_ref", "depth_mae", "depth_bias", "depth_rmse", "depth_max")


def _pinhole(K):
    K = np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float64)
    if K.shape != (3, 3) or not np.array_equal(K[2], [0.0, 0.0, 1.0]):
        raise ValueError(f"rasterize: K must be [3,3] with last row (0,0,1) -- only then is the depth of a pixel the ray parameter t; got {K!r}")
    return K


def rasterize(meshes, K, E, H: int, W: int, bgcolor=(255.0, 255.0, 255.0), want=RASTER_MAPS, z_near: float = 1e-6) -> Dict:
    """One mesh (a dict as `extract` / `extract_frame` / `extract_bkgd` return them: `vertices` f32 [V,3], `faces` int32 [F,3],
    optionally `colors` uint8 [V,3] and `normals` f32 [V,3]) or a list of them, seen by the camera `K` [3,3] (last row (0,0,1), else
    `ValueError`), `E` [4,4] or [3,4] (X_cam = E[:3,:3] x + E[:3,3]) in an `H` x `W` frame: the convention of the ray kernels
    (`rays.frame_rays_compact`, hos_rays.hip), pixel centres at integer coordinates, depth = camera-space z = the ray parameter t of
    that camera's human rays.  For a frame mesh in body space (`extract_frame(space="body")`, or `keep_body`) the camera is
    `SceneItems.frame_camera(idx)`; any mesh and camera give pictures.

    All faces go into one z-buffer at consecutive `face_base` values (`ops.mesh_project`, `ops.raster_faces`, `ops.raster_resolve`).
    Returns the whole-frame device tensors named in `want` -- `depth` f32 [H*W] (0 where empty), `mask` uint8 [H*W], `face` int32
    [H*W] (-1 where empty), `rgb` [H*W,3] (vertex colours, white without; `bgcolor` / 255 where empty), `normal` [H*W,3] (vertex normals,
    the faces' own without; 0 where empty), `shaded` [H*W,3] (`rgb` under a two-sided head-light) -- plus `dropped` (int: triangles
    with a corner behind the camera or past the guard band, or of zero screen area), `face_base` (one int per mesh), `H`, `W`.
    The read-back of `dropped` is the only host synchronisation."""
    meshes = [meshes] if isinstance(meshes, dict) else list(meshes)
    want = tuple(want)
    if not want or set(want) - set(RASTER_MAPS):
        raise ValueError(f"rasterize: want {want!r} must name some of {RASTER_MAPS}")
    K = _pinhole(K)
    E = np.asarray(E.detach().cpu() if isinstance(E, torch.Tensor) else E, dtype=np.float64)
    R, T = E[:3, :3], E[:3, 3]
    H, W = int(H), int(W)
    n = H * W
    dev = meshes[0]["vertices"].device if meshes else torch.device("cuda")
    zbuf = torch.full((n,), -1, dtype=torch.int64, device=dev)
    dropped = torch.zeros(1, dtype=torch.int32, device=dev)
    projected, bases, base = [], [], 0
    for m in meshes:
        xy, z = ops.mesh_project(m["vertices"].contiguous(), K, R, T, z_near)
        faces = m["faces"].contiguous()
        ops.raster_faces(xy, z, faces, base, H, W, zbuf, dropped)
        projected.append((xy, z, faces))
        bases.append(base)
        base += int(faces.shape[0])
    # the background exactly as `ops.raster_resolve` hands it to the kernel: divided on the host, rounded to fp32 once
    bg = torch.from_numpy((np.asarray(bgcolor, dtype=np.float64).reshape(3) / 255.0).astype(np.float32)).to(dev)
    empty = {"depth": lambda: torch.zeros(n, device=dev), "mask": lambda: torch.zeros(n, dtype=torch.uint8, device=dev),
             "face": lambda: torch.full((n,), -1, dtype=torch.int32, device=dev), "rgb": lambda: bg.expand(n, 3).contiguous(),
             "normal": lambda: torch.zeros(n, 3, device=dev), "shaded": lambda: bg.expand(n, 3).contiguous()}
    out = {k: empty[k]() for k in want}                      # what a frame without a single face shows; resolve overwrites the rest
    Kinv = np.linalg.inv(K)
    for m, (xy, z, faces), b in zip(meshes, projected, bases):
        if faces.shape[0] == 0 or xy.shape[0] == 0:
            continue
        ops.raster_resolve(zbuf, xy, z, faces, b, H, W, out, vertices=m["vertices"].contiguous(), colors=m.get("colors"),
                           normals=m.get("normals"), Kinv=Kinv, R=R, bgcolor=bgcolor)
    out.update(dropped=int(dropped.item()), face_base=bases, H=H, W=W)
    return out


def fit(raster: Dict, alpha, depth=None, tau: float = 0.5, spacing=None) -> Dict:
    """How well a rasterised mesh (`rasterize` with `mask` and, for the depth figures, `depth`) agrees with a render of the same
    frame from the same camera: `alpha` [H*W] or [H,W] (the render's opacity, or the scene's subject mask `SceneItems.alphas[idx]`)
    thresholded at `tau`, `depth` the render's depth in the units of the ray parameter (`depth_median` of
    `eval.render_human_frame`), or None for the silhouette figures alone.  Returns floats: `iou` (1 when both silhouettes are
    empty), `area_mesh`, `area_ref` (pixels), and over the pixels both cover `depth_mae`, `depth_bias` (mesh - reference),
    `depth_rmse`, `depth_max` (0 without a common pixel; absent with `depth=None`); with `spacing` (the mesh's voxel) also
    `depth_*_vox`, the same in voxels.  One launch pair (`ops.frame_fit`), one read-back.  Defined for the human-object's
    body-space camera: the background rays' t is not camera z."""
    mask = raster["mask"].reshape(-1)
    dev = mask.device
    as_f32 = lambda x: torch.as_tensor(x).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    alpha = as_f32(alpha)
    if depth is not None:
        out = ops.frame_fit(mask, raster["depth"].reshape(-1).contiguous(), alpha, as_f32(depth), tau)
    else:
        out = ops.frame_fit(mask, None, alpha, None, tau)
    host = out.cpu()
    a, b, ab = (int(c) for c in host[:3].tolist())
    union = a + b - ab
    res = {"iou": 1.0 if union == 0 else ab / union, "area_mesh": float(a), "area_ref": float(b)}
    if depth is not None:
        s_abs, s, s_sq, mx = (float(x) for x in host[3:].view(torch.float64).tolist())
        k = max(ab, 1)
        res.update(depth_mae=s_abs / k, depth_bias=s / k, depth_rmse=math.sqrt(s_sq / k), depth_max=mx)
        if spacing is not None:
            res.update({key + "_vox": res[key] / float(spacing) for key in ("depth_mae", "depth_bias", "depth_rmse", "depth_max")})
    return res


def level_sweep(field: Dict, levels, camera: Dict, ref_maps: Dict, tau: float = 0.5):
    """The instrument for `run.mesh_level`: the already computed `field` (`frame_field`: `alpha`, `rgb`, `origin`, `spacing`) marched
    again at each of `levels`, rasterised from `camera` (`SceneItems.frame_camera`: `K`, `E`, `H`, `W`) and scored by `fit` against
    `ref_maps` (`alpha` and `depth_median`, else `depth`: `eval.render_human_frame(maps=True, median=True)` from the same
    camera).  One row per level: `level`, `V`, `F`, `dropped` and the figures of `fit`, voxel units included.  No network runs."""
    ref_depth = ref_maps.get("depth_median", ref_maps.get("depth"))
    rows = []
    for level in levels:
        vertices, _, faces = ops.march_tets(field["alpha"], float(level), field["origin"], field["spacing"])
        r = rasterize({"vertices": vertices, "faces": faces}, camera["K"], camera["E"], camera["H"], camera["W"], want=("depth", "mask"))
        rows.append({"level": float(level), "V": int(vertices.shape[0]), "F": int(faces.shape[0]), "dropped": r["dropped"],
                     **fit(r, ref_maps["alpha"], ref_depth, tau=tau, spacing=field["spacing"])})
    return rows
