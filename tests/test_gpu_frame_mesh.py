"""The frame mesh on the GPU: `ops.grid_warp` against `ops.human_sample_warp` (bit for bit) and the oracle, `mesh.frame_field`
against the oracle's chain, `mesh.extract_frame` on stage-2 and stage-3 networks in both spaces, `ops.mesh_vertex_normals` against
its numpy restatement (tests/_frame_mesh_expect.py, whose own properties tests/test_frame_mesh_cpu.py checks), and the launcher's
`run.run_mesh_frames`.

Accuracy rule of the normals (the rule tests/test_gpu_mesh.py applies to vertices): |hip - fp64 restatement| <= 2 * |fp32 restatement -
fp64 restatement| + one fp32 ulp of the largest component (1.0), in the maximum norm over ALL vertices; faces, V and F are exact.

Measured on one MI355X: the kernel's normals are bit-equal to the fp32 restatement on every field here; the field's distance to the
oracle is in the docstring of test_frame_field_against_the_oracle."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle.human as oh
from hosnerf_amd import formats, synth, tpose
from tests import _frame_mesh_expect as FX
from tests import _mesh_expect as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def basedir():
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    return d


@pytest.fixture(scope="module")
def nets(dev):
    """Stage-2 and stage-3 networks on the weights of tests/test_gpu_human.py, and the T-pose constants."""
    from hosnerf_amd.human_nerf import Network, default_cfg
    out = {}
    for stage in (2, 3):
        net = Network(default_cfg(basedir()), stage=stage)
        net.load_state_dict(synth.human_state_dict(777, 2), strict=True)
        out[stage] = net.to(dev)
    joints = synth.tpose_joints()
    bbox = formats.skeleton_bbox(joints, float(out[3].cfg.bbox_offset))
    return out, tpose.TposeTurn(joints, bbox, 32, dev)


def host_pose(time):
    """A posed frame without rays, on the host: the per-frame keys of `synth.human_batch` as `SceneItems.frame_pose` lays them out."""
    hb = synth.human_batch(8, seed=3, time=time, is_train=False, iter_val=1e7)
    keys = ("dst_Rs", "dst_Ts", "dst_posevec", "cnl_gtfms", "canonical_joints", "motion_weights_priors", "cnl_bbox_min_xyz", "cnl_bbox_max_xyz",
            "cnl_bbox_scale_xyz", "newsmpl_to_scale_world", "iter_val")
    p = {k: hb[k] for k in keys}
    p.update(time=float(time), is_train=False, frame_name=f"frame_{int(round(time * 100)):03d}",
             dst_bbox={"min_xyz": hb["dst_bbox_min_xyz"].numpy(), "max_xyz": hb["dst_bbox_max_xyz"].numpy()})
    return p


def on_device(p, dev):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in p.items()}


@pytest.fixture(scope="module")
def poses(dev):
    """time -> (host pose, device pose), either side of the transition at 0.4."""
    return {t: (host_pose(t), on_device(host_pose(t), dev)) for t in (0.2, 0.7)}


@pytest.fixture(scope="module")
def prologue(dev, nets, poses):
    from hosnerf_amd.eval import FRAME_KEYS, evaluating
    net = nets[0][3]
    pose = poses[0.7][1]
    with evaluating(net):
        pro = net.frame_prologue(**{k: pose[k] for k in FRAME_KEYS if k in pose})
    assert float((pro["R_b"] - torch.eye(3, device=dev)).abs().max()) > 0.05, "the pose must not be the T-pose"
    return pro


def frame_grid(pose, resolution):
    from hosnerf_amd import mesh
    g = mesh.grid_of_box(pose["dst_bbox"]["min_xyz"], pose["dst_bbox"]["max_xyz"], resolution)
    return g["origin"], g["spacing"], g["dims"]


def inner_mask(dims):
    Nx, Ny, Nz = dims
    inner = np.zeros((Nz, Ny, Nx), dtype=bool)
    inner[1:-1, 1:-1, 1:-1] = True
    return inner


# ------------------------------------------------------------------------------------------ grid_warp
def test_grid_warp_is_the_renderers_warp(dev, nets, poses, prologue):
    from hosnerf_amd import ops
    from hosnerf_amd._lib import call, ptr
    net, pose, pro = nets[0][3], poses[0.7][1], prologue
    K = net.cfg.total_bones
    bmin, bscale = pose["cnl_bbox_min_xyz"], pose["cnl_bbox_scale_xyz"]
    origin, h, dims = frame_grid(pose, 12)
    N = dims[0] * dims[1] * dims[2]
    assert N > 2 * ops.MT_BLOCK and N % ops.MT_BLOCK != 0                       # several blocks, a ragged last one
    pts = ops.grid_points(origin, h, dims, 0, N, device=dev)
    x_skel, mask = ops.grid_warp(pro["R_b"], pro["T_b"], pro["vol"], bmin, bscale, origin, h, dims, 0, N, K=K)
    assert x_skel.shape == (N, 3) and mask.shape == (N,)
    # the renderer's kernel on the same points, as rays of zero length: bit for bit
    zeros = torch.zeros(N, device=dev)
    _, wpts, wx, wmask = ops.human_sample_warp(pts, torch.zeros_like(pts), zeros, zeros, 1, pro["R_b"], pro["T_b"], pro["vol"], bmin, bscale, K=K)
    assert torch.equal(wpts.reshape(N, 3), pts)
    assert torch.equal(x_skel, wx) and torch.equal(mask, wmask)
    assert float(mask.max()) > 0.5 and bool((mask == 0).any()) and bool(torch.isfinite(x_skel).all())
    # the oracle on the same transforms and volume: the bounds of tests/test_gpu_human.py for the warp kernel
    with torch.no_grad():
        x_o, m_o = oh.backward_lbs(pts.cpu(), pro["R_b"].cpu(), pro["T_b"].cpu(), pro["vol"].cpu(), bmin.cpu(), bscale.cpu())
    em, ex = float((mask.cpu() - m_o[:, 0]).abs().max()), float((x_skel.cpu() - x_o).abs().max())
    print(f"grid_warp vs oracle: mask {em:.3e}, x_skel {ex:.3e}")
    assert em < 2e-6 and ex < 5e-5
    # a vertex range writes its own rows and nothing else (the C entry on the middle of two larger buffers)
    first, count = 301, 517
    xb, mb = torch.full((count + 20, 3), -7.0, device=dev), torch.full((count + 20,), -7.0, device=dev)
    call("hos_grid_warp", ptr(pro["R_b"]), ptr(pro["T_b"]), ptr(pro["vol"]), pro["vol"].shape[-1], K, ptr(bmin), ptr(bscale),
         *ops._grid_args(origin, h, dims), first, count, ptr(xb[10:10 + count]), ptr(mb[10:10 + count]))
    assert torch.equal(xb[10:10 + count], x_skel[first:first + count]) and torch.equal(mb[10:10 + count], mask[first:first + count])
    assert bool((xb[:10] == -7.0).all()) and bool((xb[10 + count:] == -7.0).all()) and bool((mb[:10] == -7.0).all()) and bool((mb[10 + count:] == -7.0).all())
    px, pm = ops.grid_warp(pro["R_b"], pro["T_b"], pro["vol"], bmin, bscale, origin, h, dims, first, count, K=K)
    assert torch.equal(px, x_skel[first:first + count]) and torch.equal(pm, mask[first:first + count])
    ex_, em_ = ops.grid_warp(pro["R_b"], pro["T_b"], pro["vol"], bmin, bscale, origin, h, dims, N, 0, K=K)          # nothing to launch
    assert ex_.shape == (0, 3) and em_.shape == (0,)


def test_grid_warp_identity_is_the_canonical_mask(dev, nets, prologue):
    """Under identity bone transforms the warp's mask is `hos_grid_alpha`'s (sigma = +inf makes alpha = mask), bit for bit, and
    `grid_alpha_masked` fed that mask writes what `grid_alpha` writes."""
    from hosnerf_amd import mesh, ops
    networks, turn = nets
    net, const, vol = networks[3], turn.const, prologue["vol"]
    K = net.cfg.total_bones
    bmin, bscale = const["cnl_bbox_min_xyz"], const["cnl_bbox_scale_xyz"]
    grid = mesh.grid_of_box(bmin.cpu().numpy(), const["cnl_bbox_max_xyz"].cpu().numpy(), 12)
    origin, h, dims = grid["origin"], grid["spacing"], grid["dims"]
    Nx, Ny, Nz = dims
    N = Nx * Ny * Nz
    eye, zero = torch.eye(3, device=dev).expand(K, 3, 3).contiguous(), torch.zeros(K, 3, device=dev)
    x_skel, mask = ops.grid_warp(eye, zero, vol, bmin, bscale, origin, h, dims, 0, N, K=K)
    raw = torch.rand(N, 4, device=dev)
    opaque = raw.clone()
    opaque[:, 3] = float("inf")
    a_vol = torch.full((Nz, Ny, Nx), -7.0, device=dev)
    ops.grid_alpha(opaque, vol, bmin, bscale, origin, h, dims, 0, a_vol, None, K=K)
    inner = torch.from_numpy(inner_mask(dims)).to(dev)
    assert torch.equal(a_vol[inner], mask.view(Nz, Ny, Nx)[inner]) and float(mask.max()) > 0.5
    # the two instantiations of the alpha kernel: the same alpha and colours from the same mask, the same rim
    for sigma in (opaque, raw):
        a1, c1 = torch.full((Nz, Ny, Nx), -7.0, device=dev), torch.full((Nz, Ny, Nx, 3), -7.0, device=dev)
        a2, c2 = torch.full((Nz, Ny, Nx), -7.0, device=dev), torch.full((Nz, Ny, Nx, 3), -7.0, device=dev)
        ops.grid_alpha(sigma, vol, bmin, bscale, origin, h, dims, 0, a1, c1, K=K)
        ops.grid_alpha_masked(sigma, mask, origin, h, dims, 0, a2, c2)
        assert torch.equal(a1, a2) and torch.equal(c1, c2) and torch.equal(c2.view(N, 3), sigma[:, :3])
        rim = a2[~inner]
        assert bool((rim == 0).all()) and not bool(torch.signbit(rim).any())
    # the formula, fp32 operation by operation up to expf: 1 ulp of alpha <= 1
    want = mask.double() * (1.0 - torch.exp(-raw[:, 3].double() * float(h)))
    assert float((a2.view(-1).double() - want)[inner.view(-1)].abs().max()) < 3e-7
    # a vertex range writes its own part of the whole-grid arrays and nothing else; no colours asked, none written
    part = torch.full((Nz, Ny, Nx), -7.0, device=dev)
    ops.grid_alpha_masked(raw[300:500].contiguous(), mask[300:500].contiguous(), origin, h, dims, 300, part, None)
    flat = part.view(-1)
    assert torch.equal(flat[300:500], a2.view(-1)[300:500]) and bool((flat[:300] == -7.0).all()) and bool((flat[500:] == -7.0).all())


# ------------------------------------------------------------------------------------------ the field
def oracle_alpha(pose_host, pts, h):
    """The oracle's chain at the points: backward_lbs, hannw_embed + nonrigid_mlp, fourier_embed + state embedding + canonical_mlp
    (`oracle.human.human_forward` on rays of zero length with one sample each) -> (alpha [P], rgb [P,3], state mask)."""
    P = pts.shape[0]
    batch = dict(pose_host)
    batch.update(rays=torch.stack([pts, torch.zeros_like(pts)], 0), near=torch.zeros(P, 1), far=torch.zeros(P, 1), bgcolor=torch.zeros(3))
    with torch.no_grad():
        out = oh.human_forward(synth.human_state_dict(777, 2), batch, cfg={"N_samples": 1}, transitions_times=[0.4], stage=3)
    assert torch.equal(out["newsmpl_pts"].reshape(P, 3), pts)
    m, sigma = out["pts_mask"].reshape(P), out["human_density"].reshape(P)
    return m * (1.0 - torch.exp(-sigma * float(h))), out["human_rgb"].reshape(P, 3), m


def test_frame_field_against_the_oracle(dev, nets, poses):
    """`frame_field` at resolution 12 against the oracle chain on the inner vertices.  Bound: 1e-5 + 2e-4 * h -- the full-forward
    bounds of tests/test_gpu_human.py (pts_mask 1e-5, density * mask 2e-4) through |d alpha / d mask| <= 1 and
    |d alpha / d sigma| <= mask * h.  The outermost layer, and a layer past the box, are exactly +0 (in the oracle's field too: the
    renderer's rays end at the box).  Measured on one MI355X: alpha 1.8e-6 against the bound 6.1e-5 (h = 0.255), colour 1.7e-5."""
    from hosnerf_amd import mesh, ops
    net = nets[0][3]
    fields = {}
    for t, state in ((0.7, 1), (0.2, 0)):
        host, pose = poses[t]
        field = mesh.frame_field(net, pose, resolution=12)
        origin, h, dims = frame_grid(pose, 12)
        Nx, Ny, Nz = dims
        N = Nx * Ny * Nz
        assert field["dims"] == dims and field["spacing"] == h and field["state"] == state and field["alpha"].shape == (Nz, Ny, Nx)
        assert field["rgb"].shape == (Nz, Ny, Nx, 3) and bool(torch.isfinite(field["alpha"]).all())
        fields[t] = field
        if t != 0.7:
            continue
        inner = inner_mask(dims)
        a = field["alpha"].cpu().numpy()
        assert (a[~inner] == 0.0).all() and not np.signbit(a[~inner]).any()
        pts = ops.grid_points(origin, h, dims, 0, N, device=dev).cpu()
        alpha_o, rgb_o, mask_o = oracle_alpha(host, pts, h)
        # a layer past the box (an extent rounded up to whole voxels) is 0 like the rim: the renderer's rays end at the box
        kx, ky, kz = mesh.layers_in_box(origin, h, dims, pose["dst_bbox"]["max_xyz"])
        assert min(Nx - kx, Ny - ky, Nz - kz) == 1 and max(Nx - kx, Ny - ky, Nz - kz) == 2        # the longest axis has none, another has one
        past = np.zeros((Nz, Ny, Nx), dtype=bool)
        past[:, :, kx:], past[:, ky:], past[kz:] = True, True, True
        assert (pts.numpy().reshape(Nz, Ny, Nx, 3)[~past] <= pose["dst_bbox"]["max_xyz"] + 1e-4 * h).all()
        assert (pts.numpy().reshape(Nz, Ny, Nx, 3)[past & inner] > pose["dst_bbox"]["max_xyz"] + 1e-4 * h).any(-1).all()
        assert (a[past] == 0.0).all() and not np.signbit(a[past]).any()
        alpha_o = torch.where(torch.from_numpy(past.reshape(-1)), torch.zeros(()), alpha_o)
        sel = torch.from_numpy(inner.reshape(-1))
        err = float((field["alpha"].cpu().reshape(-1) - alpha_o)[sel].abs().max())
        on = sel & (mask_o > 0.01)
        err_rgb = float((field["rgb"].cpu().reshape(-1, 3) - rgb_o)[on].abs().max())
        bound = 1e-5 + 2e-4 * float(h)
        print(f"frame_field vs oracle at resolution 12: alpha {err:.3e} (bound {bound:.3e}), rgb where mask > 0.01 {err_rgb:.3e}, "
              f"max alpha {float(field['alpha'].max()):.4f}, max mask {float(mask_o.max()):.3f}")
        assert float(field["alpha"].max()) > 0.0 and float(mask_o.max()) > 0.5
        assert err <= bound
    # two times on either side of the transition: other states, other fields
    assert float((fields[0.2]["alpha"] - fields[0.7]["alpha"]).abs().max()) > 1e-4, "the state never reached the canonical MLP"


def test_frame_field_chunks(dev, nets, poses):
    """Several chunks (the last one moved back to keep its rows) give the field of one chunk to 1e-4, the bound
    tests/test_gpu_mesh.py sets for the canonical field."""
    from hosnerf_amd import mesh
    net, pose = nets[0][3], poses[0.7][1]
    one = mesh.frame_field(net, pose, resolution=48)
    N = one["alpha"].numel()
    assert N > 2 * 16384 and N % 16384 != 0
    many = mesh.frame_field(net, pose, resolution=48, chunk=16384)
    assert one["dims"] == many["dims"] and one["state"] == many["state"] == 1
    assert float((one["alpha"] - many["alpha"]).abs().max()) <= 1e-4 and float((one["rgb"] - many["rgb"]).abs().max()) <= 1e-4
    with pytest.raises(ValueError):
        mesh.frame_field(net, pose, resolution=48, chunk=1000)


# ------------------------------------------------------------------------------------------ the mesh
def assert_equals_restatement(field, level, origin, h, got, tag=""):
    """The logic of tests/test_gpu_mesh.py: faces, V, F exact; vertices by the 2x-fp32 + one ulp rule."""
    field = np.ascontiguousarray(field, dtype=np.float32)
    v64, _, f = X.march(field, level, origin, h, dtype=np.float64)
    v32, _, _ = X.march(field, level, origin, h, dtype=np.float32)
    gv, gf = got
    assert gv.shape == v64.shape and gf.shape == f.shape, (tag, gv.shape, v64.shape, gf.shape, f.shape)
    assert np.array_equal(gf, f), tag
    assert v64.shape[0] > 0 and np.isfinite(gv).all(), tag
    e_hip = float(np.abs(gv.astype(np.float64) - v64).max())
    e_ref = float(np.abs(v32.astype(np.float64) - v64).max())
    assert e_hip <= 2.0 * e_ref + float(np.spacing(np.float32(np.abs(v64).max()))), (tag, e_hip, e_ref)
    return v64.shape[0], f.shape[0]


def assert_normals(field, origin, h, vertices, normals, tag=""):
    """The kernel's normals against the fp64 restatement by the 2x-fp32 + one ulp rule, over every vertex; exact zeros where g == 0."""
    n64 = FX.vertex_normals(field, origin, h, vertices, dtype=np.float64)
    n32 = FX.vertex_normals(field, origin, h, vertices, dtype=np.float32)
    assert normals.shape == n64.shape and normals.dtype == np.float32 and np.isfinite(normals).all(), tag
    e_hip = float(np.abs(normals.astype(np.float64) - n64).max())
    e_ref = float(np.abs(n32.astype(np.float64) - n64).max())
    same = float((normals == n32).mean())
    print(f"normals {tag}: {normals.shape[0]} vertices, hip vs fp64 {e_hip:.3e}, fp32 restatement vs fp64 {e_ref:.3e}, bit-equal to fp32 {same:.4f}")
    assert e_hip <= 2.0 * e_ref + float(np.spacing(np.float32(1.0))), (tag, e_hip, e_ref)
    zero = (n64 == 0).all(1)
    assert (normals[zero] == 0).all(), tag
    length = np.linalg.norm(normals[~zero].astype(np.float64), axis=1)
    assert (np.abs(length - 1.0) < 1e-6).all(), tag
    return int(zero.sum())


@pytest.mark.parametrize("stage", [2, 3])
def test_extract_frame(dev, nets, poses, stage, tmp_path):
    from hosnerf_amd import mesh
    net, pose = nets[0][stage], poses[0.7][1]
    a = mesh.frame_field(net, pose, resolution=24)["alpha"]
    level = float(a[a > 0].median())                                   # unmeasured defaults: take a level that gives a surface
    body = mesh.extract_frame(net, pose, resolution=24, level=level, space="body", normals=True)
    assert body["state"] == 1 and body["space"] == "body" and body["frame_name"] == "frame_070" and body["time"] == 0.7 and body["level"] == level
    assert body["to_world"].dtype == np.float32 and np.array_equal(body["to_world"], np.eye(4, dtype=np.float32))
    assert torch.equal(body["alpha"], a)
    bv, bf = body["vertices"].cpu().numpy(), body["faces"].cpu().numpy()
    fa = body["alpha"].cpu().numpy()
    V, F = assert_equals_restatement(fa, level, body["origin"], body["spacing"], (bv, bf), tag=f"stage {stage}")
    assert X.is_closed_oriented_manifold(bf, V) and body["volume"] > 0
    assert abs(body["volume"] - X.signed_volume(bv, bf)) <= 1e-9 * abs(body["volume"]) and abs(body["area"] - X.area(bv, bf)) <= 1e-9 * body["area"]
    col = body["colors"].cpu().numpy()
    _, c64, _ = X.march(fa, level, body["origin"], body["spacing"], rgb=body["rgb"].cpu().numpy())
    assert col.dtype == np.uint8 and col.shape == (V, 3) and np.abs(col.astype(np.int64) - np.floor(255.0 * np.clip(c64, 0, 1)).astype(np.int64)).max() <= 1
    assert_normals(fa, body["origin"], body["spacing"], bv, body["normals"].cpu().numpy(), tag=f"network field, stage {stage}")
    lo, hi = pose["dst_bbox"]["min_xyz"] - body["spacing"] - 1e-6, pose["dst_bbox"]["max_xyz"] + body["spacing"] + 1e-6     # the box grown by one h
    assert (bv >= lo).all() and (bv <= hi).all()
    # the scene's coordinates
    world = mesh.extract_frame(net, pose, resolution=24, level=level, space="world", normals=True)
    A = pose["newsmpl_to_scale_world"].cpu().numpy()
    assert world["space"] == "world" and world["to_world"].dtype == np.float32 and world["to_world"].shape == (4, 4) and np.array_equal(world["to_world"], A)
    wv, wf = world["vertices"].cpu().numpy(), world["faces"].cpu().numpy()
    v64, f64, n64 = FX.to_space(bv, bf, body["normals"].cpu().numpy(), A.astype(np.float64))
    assert wv.dtype == np.float32 and (np.abs(wv.astype(np.float64) - v64) <= np.spacing(np.abs(v64).astype(np.float32))).all()       # 1 fp32 ulp
    det = float(np.linalg.det(A[:3, :3].astype(np.float64)))
    assert det > 0 and np.array_equal(wf, bf) and np.array_equal(wf, f64)
    assert abs(world["volume"] - det * body["volume"]) <= 1e-5 * det * body["volume"]
    assert abs(world["volume"] - X.signed_volume(wv, wf)) <= 1e-9 * world["volume"] and abs(world["area"] - X.area(wv, wf)) <= 1e-9 * world["area"]
    assert np.abs(world["normals"].cpu().numpy() - n64).max() < 1e-6 and torch.equal(world["colors"], body["colors"])
    # without normals: the same mesh, no normals
    plain = mesh.extract_frame(net, pose, resolution=24, level=level)
    assert plain["normals"] is None and plain["space"] == "world" and torch.equal(plain["vertices"], world["vertices"]) and torch.equal(plain["faces"], world["faces"])
    # PLY round trip with normals
    path = str(tmp_path / f"s{stage}.ply")
    formats.write_ply(path, world["vertices"], world["faces"], world["colors"], world["normals"])
    v2, f2, c2, n2 = formats.read_ply(path, with_normals=True)
    assert np.array_equal(v2, wv) and np.array_equal(f2, wf) and np.array_equal(c2, col) and np.array_equal(n2, world["normals"].cpu().numpy())
    with pytest.raises(ValueError):
        mesh.extract_frame(net, pose, resolution=24, level=level, space="camera")
    with pytest.raises(ValueError):
        mesh.extract_frame(net, {k: v for k, v in pose.items() if k != "newsmpl_to_scale_world"}, resolution=24, level=level)


def test_extract_frame_is_deterministic(dev, nets, poses):
    from hosnerf_amd import mesh
    net, pose = nets[0][3], poses[0.2][1]
    a = mesh.frame_field(net, pose, resolution=24)["alpha"]
    level = float(a[a > 0].median())
    one = mesh.extract_frame(net, pose, resolution=24, level=level, normals=True)
    two = mesh.extract_frame(net, pose, resolution=24, level=level, normals=True)
    assert one["state"] == 0 and one["vertices"].shape[0] > 0
    for k in ("vertices", "faces", "colors", "normals", "alpha"):
        assert torch.equal(one[k], two[k]), k


# ------------------------------------------------------------------------------------------ the normals kernel
def analytic_fields():
    o, h, dims, P = X.unit_box_grid(32)
    sphere = 0.37 - np.linalg.norm(P - [0.47, 0.52, 0.49], axis=-1)
    q = P - [0.5, 0.51, 0.49]
    torus = 0.12 - np.sqrt((np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - 0.3) ** 2 + q[..., 2] ** 2)
    return o, h, {"sphere": sphere.astype(np.float32), "torus": torus.astype(np.float32)}


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_vertex_normals_on_analytic_fields(dev, name):
    from hosnerf_amd import ops
    o, h, fields = analytic_fields()
    f = torch.from_numpy(fields[name]).to(dev)
    v, _, faces = ops.march_tets(f, 0.0, o, h)
    assert v.shape[0] > 2 * ops.MT_BLOCK                                          # several blocks
    n = ops.mesh_vertex_normals(f, o, h, v)
    ragged = ops.MT_BLOCK + 1                                                      # a last block with one live thread
    assert torch.equal(ops.mesh_vertex_normals(f, o, h, v[:ragged].contiguous()), n[:ragged])
    assert assert_normals(fields[name], o, h, v.cpu().numpy(), n.cpu().numpy(), tag=name) == 0          # |grad| ~ 1: no zero normal
    # outward: along the faces' orientation
    vn, fn = v.cpu().numpy().astype(np.float64), faces.cpu().numpy()
    face_normal = np.cross(vn[fn[:, 1]] - vn[fn[:, 0]], vn[fn[:, 2]] - vn[fn[:, 0]])
    assert (np.einsum("ij,ij->i", face_normal, n.cpu().numpy().astype(np.float64)[fn[:, 0]]) > 0).all()
    assert torch.equal(n, ops.mesh_vertex_normals(f, o, h, v))
    assert ops.mesh_vertex_normals(f, o, h, v[:0]).shape == (0, 3)


def test_vertex_normals_zero_gradient_and_grid_faces(dev):
    """Points whose taps are all 0 (outside the mask alpha IS 0), outside the grid or not finite: exact zeros.  Points next to the
    grid's faces and ordinary ones, on a grid of three distinct dimensions: the restatement."""
    from hosnerf_amd import ops
    rs = np.random.RandomState(4)
    f = np.zeros((9, 11, 13), dtype=np.float32)
    f[4:, 5:, 6:] = rs.uniform(0.1, 1.0, (5, 6, 7)).astype(np.float32)
    o, h = np.array([-0.2, 0.1, 0.3], np.float32), np.float32(0.05)
    flat = np.array([[-0.1, 0.2, 0.4], [-0.07, 0.23, 0.41], [40.0, 0.2, 0.4], [np.nan, 0.2, 0.4], [-0.1, np.inf, 0.4]], dtype=np.float32)
    hi = o + np.float32(h) * (np.array([13, 11, 9], np.float32) - 1)
    inside = (o + rs.uniform(0.0, 1.0, (400, 3)) * (hi - o)).astype(np.float32)
    faces_of_grid = np.array([[hi[0], hi[1], hi[2]], [hi[0] + 0.5 * h, hi[1], hi[2] - h], [hi[0] - 0.5 * h, hi[1] + 0.9 * h, hi[2]], [o[0], hi[1], hi[2]]], np.float32)
    v = np.concatenate([flat, inside, faces_of_grid], 0)
    n = ops.mesh_vertex_normals(torch.from_numpy(f).to(dev), o, h, torch.from_numpy(v).to(dev)).cpu().numpy()
    assert (n[:5] == 0).all()
    zeros = assert_normals(f, o, h, v, n, tag="zero region, grid faces")
    assert 5 <= zeros < len(v) - 100


def test_canonical_mesh_with_and_without_normals(dev, nets):
    """`mesh.extract(normals=False)` is what it was: `canonical_field`, `march_tets` and the 8-bit colours, bit for bit; `normals=True`
    adds the normals and changes nothing else."""
    from hosnerf_amd import mesh, ops
    networks, turn = nets
    net = networks[3]
    field = mesh.canonical_field(net, turn.const, 0.7, resolution=24)
    a = field["alpha"]
    level = float(a[a > 0].median())
    v, c, f = ops.march_tets(a, level, field["origin"], field["spacing"], rgb=field["rgb"])
    plain = mesh.extract(net, turn, 0.7, resolution=24, level=level)
    assert plain["normals"] is None and torch.equal(plain["vertices"], v) and torch.equal(plain["faces"], f)
    assert torch.equal(plain["colors"], (255.0 * c.clamp(0.0, 1.0)).to(torch.uint8)) and torch.equal(plain["alpha"], a)
    withn = mesh.extract(net, turn, 0.7, resolution=24, level=level, normals=True)
    for k in ("vertices", "faces", "colors", "alpha", "rgb"):
        assert torch.equal(plain[k], withn[k]), k
    assert plain["volume"] == withn["volume"] and plain["area"] == withn["area"]
    assert_normals(a.cpu().numpy(), field["origin"], field["spacing"], v.cpu().numpy(), withn["normals"].cpu().numpy(), tag="canonical network field")


# ------------------------------------------------------------------------------------------ SceneItems.frame_pose on the device
def test_frame_pose_matches_eval_frame(dev, tmp_path):
    from hosnerf_amd.dataset import SceneItems
    scene = str(tmp_path / "scene")
    px = synth.write_scene_dir(scene, 6, 32, 32, seed=9)
    formats.load_scene(scene, (32, 32), masks=px["alphas"], near=0.1, far=1e6)
    ds = SceneItems(scene, px["images"], px["alphas"], px["flows"], n_patches=2, patch_size=8, device=dev, seed=5)
    for idx in (0, 3):
        p, ev = ds.frame_pose(idx), ds.eval_frame(idx)
        for k in ("newsmpl_to_scale_world", "dst_Rs", "dst_Ts", "dst_posevec", "cnl_gtfms", "cnl_bbox_min_xyz", "cnl_bbox_scale_xyz"):
            assert p[k].device.type == "cuda" and torch.equal(p[k], ev[k]), k
        assert p["time"] == ev["time"] and p["frame_name"] == ev["frame_name"] and p["is_train"] is False and torch.equal(p["iter_val"], ev["iter_val"])
        assert p["motion_weights_priors"] is ev["motion_weights_priors"]


# ------------------------------------------------------------------------------------------ the launcher
@pytest.mark.parametrize("gin,model,space", [("hosnerf_backpack.gin", "hosnerf", "world"), ("state_humanobject_backpack.gin", "state_humanobject", "body")])
def test_launcher_writes_one_mesh_per_frame(tmp_path, gin, model, space):
    from hosnerf_amd.freeview import write_scene_pixels
    from hosnerf_amd.human_nerf import default_cfg
    scene = str(tmp_path / "scene")
    write_scene_pixels(scene, synth.write_scene_dir(scene, 6, 64, 64, seed=9))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("patch:\n  N_patches: 2\n  size: 16\n")
    logs = str(tmp_path / "logs")
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "--ginc", os.path.join(ROOT, "configs", gin), "--ginb", "run.max_steps=2",
           "--ginb", f'run.datadir="{scene}"', "--ginb", "run.run_mesh_frames=True", "--ginb", "run.mesh_resolution=16", "--ginb", "run.mesh_level=0.001",
           "--scene_name", "synthetic", "--scene_dir", scene, "--cfg", str(cfg), "--logbase", logs, "--eval_skip", "3"]      # an untrained field stays far below 0.5
    if space != "world":
        cmd += ["--ginb", f'run.mesh_space="{space}"']
    if model == "hosnerf":
        cmd += ["--ginb", 'run.human_path=""', "--ginb", 'run.bkgd_path=""']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    logdir = [os.path.join(logs, d) for d in os.listdir(logs)][0]
    assert os.path.basename(logdir).startswith(model)
    infos = formats.load_mesh_infos(os.path.join(scene, "mesh_infos.pkl"), float(default_cfg(scene).bbox_offset))
    meta = json.load(open(os.path.join(logdir, "mesh_frames", "meshes.json")))
    frames = sorted(meta)
    assert len(frames) == 2 and all(name in infos for name in frames)
    assert sorted(os.listdir(os.path.join(logdir, "mesh_frames"))) == sorted(["meshes.json"] + [name + ".ply" for name in frames])
    times = np.linspace(0.0, 1.0, 6)
    chosen = {name: int(round(meta[name]["time"] * 5)) for name in frames}
    assert sorted(chosen.values()) == [0, 3]                                         # what run.run_eval chooses with --eval_skip 3 of 6 frames
    for name, i in chosen.items():
        row = meta[name]
        assert row["frame_name"] == name
        assert set(row) >= {"time", "state", "V", "F", "volume", "area", "level", "spacing", "dims", "space", "to_world"}
        v, f, c, n = formats.read_ply(os.path.join(logdir, "mesh_frames", name + ".ply"), with_normals=True)
        assert row["V"] == v.shape[0] and row["F"] == f.shape[0] and c.shape == v.shape and n.shape == v.shape          # run.mesh_normals defaults to True
        print(f"{model} {name} ({space}): V {row['V']} F {row['F']} volume {row['volume']:.5f} area {row['area']:.5f}")
        assert abs(row["time"] - times[i]) < 1e-6 and row["state"] == int(times[i] > 0.4) and row["space"] == space
        assert row["level"] == 0.001 and max(row["dims"]) == 16 + 3 and X.is_closed_oriented_manifold(f, v.shape[0])
        assert row["V"] > 0 and row["volume"] > 0 and abs(row["volume"] - X.signed_volume(v, f)) < 1e-5 * max(row["volume"], row["area"])
        length = np.linalg.norm(n.astype(np.float64), axis=1)
        assert (((np.abs(length - 1.0) < 1e-5) | (length == 0))).all() and (length > 0).mean() > 0.9
        A = np.array(row["to_world"])
        assert A.shape == (4, 4)
        if space == "body":
            box, h = infos[name]["bbox"], row["spacing"]
            assert np.array_equal(A, np.eye(4))
            assert (v >= box["min_xyz"] - h - 1e-6).all() and (v <= box["max_xyz"] + h + 1e-6).all()       # inside the frame's box grown by one h
        else:
            assert abs(np.linalg.det(A[:3, :3])) > 0 and not np.array_equal(A, np.eye(4))
    assert "results.json" not in os.listdir(logdir)
