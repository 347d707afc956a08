"""The tracked mesh on the GPU: `ops.warp_invert` (hos_track.hip) against its restatement tests/_track_expect.py (whose own
properties tests/test_track_cpu.py checks) as a point warp, in its Jacobian and on known roots; `mesh.track` against the oracle's
float64 outer loop; and the launcher's `run.run_mesh_track`.

The weights are those of tests/test_gpu_frame_mesh.py with the output layer of the non-rigid MLP scaled by 0.1: as drawn, that
layer gives offsets of 0.6 voxel whose Jacobian folds space (det(I + d offset/dx) down to -0.36), a map without an inverse; at 0.1 it
is still 100 times the reference's initialisation.  The template is cut at level 0.05, not at the median of the positive alpha the
other mesh tests use: that median is 4e-6 on these weights and its surface lies where the canonical mask is 1e-5, so that no
vertex carries enough motion weight to be judged (mask_canonical >= 0.05); at 0.05 nine in ten do.

The measured figures are recorded as `track.<test>` (tests/_record.py; the committed copy is profiles/track_parity.json)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hosnerf_amd import formats, synth, tpose
from tests import _frame_mesh_expect as FX
from tests import _record
from tests import _track_expect as X
from tests.test_gpu_frame_mesh import basedir, frame_grid, on_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NR_LAST = ("non_rigid_mlp.block_mlps.12.weight", "non_rigid_mlp.block_mlps.12.bias")
LEVEL = 0.05


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def state_dict(scale):
    sd = synth.human_state_dict(777, 2)
    for k in NR_LAST:
        sd[k] = sd[k] * scale
    return sd


@pytest.fixture(scope="module")
def nets(dev):
    """scale of the non-rigid output layer -> stage-3 network, and the T-pose constants."""
    from hosnerf_amd.human_nerf import Network, default_cfg
    out = {}
    for scale in (0.1, 0.0):
        net = Network(default_cfg(basedir()), stage=3)
        net.load_state_dict(state_dict(scale), strict=True)
        out[scale] = net.to(dev)
    joints = synth.tpose_joints()
    bbox = formats.skeleton_bbox(joints, float(out[0.1].cfg.bbox_offset))
    return out, tpose.TposeTurn(joints, bbox, 32, dev)


def host_pose(time, seed=3):
    """A posed frame without rays, on the host (the layout of `SceneItems.frame_pose`)."""
    hb = synth.human_batch(8, seed=seed, time=time, is_train=False, iter_val=1e7)
    keys = ("dst_Rs", "dst_Ts", "dst_posevec", "cnl_gtfms", "canonical_joints", "motion_weights_priors", "cnl_bbox_min_xyz", "cnl_bbox_max_xyz",
            "cnl_bbox_scale_xyz", "newsmpl_to_scale_world", "iter_val")
    p = {k: hb[k] for k in keys}
    p.update(time=float(time), is_train=False, frame_name=f"frame_{int(round(time * 100)):03d}",
             dst_bbox={"min_xyz": hb["dst_bbox_min_xyz"].numpy(), "max_xyz": hb["dst_bbox_max_xyz"].numpy()})
    return p


@pytest.fixture(scope="module")
def frame(dev, nets):
    """The pose at 0.7 on the host and the device, the device's prologue, and its transforms and volume as numpy arrays."""
    from hosnerf_amd.eval import FRAME_KEYS, evaluating
    net = nets[0][0.1]
    host = host_pose(0.7)
    pose = on_device(host, dev)
    with evaluating(net):
        pro = net.frame_prologue(**{k: pose[k] for k in FRAME_KEYS if k in pose})
    K = int(net.cfg.total_bones)
    assert float((pro["R_b"] - torch.eye(3, device=dev)).abs().max()) > 0.05, "the pose must not be the T-pose"
    arrays = tuple(t.cpu().numpy() for t in (pro["R_b"], pro["T_b"], pro["vol"], pose["cnl_bbox_min_xyz"], pose["cnl_bbox_scale_xyz"]))
    voxel = float(2.0 / arrays[4].min() / (arrays[2].shape[-1] - 1))
    return {"host": host, "pose": pose, "pro": pro, "np": arrays, "K": K, "voxel": voxel}


def invert(frame, target, guess, **kw):
    from hosnerf_amd import ops
    pro, pose = frame["pro"], frame["pose"]
    return ops.warp_invert(target, guess, pro["R_b"], pro["T_b"], pro["vol"], pose["cnl_bbox_min_xyz"], pose["cnl_bbox_scale_xyz"], K=frame["K"], **kw)


@pytest.fixture(scope="module")
def roots(dev, frame):
    """700 body-frame points p* with mask64 > 0.2 (found with the kernel's own mask: the body fills under 1 % of the box), their
    float64 images, Jacobians and guesses within half a voxel."""
    P = 700
    lo, hi = (torch.from_numpy(frame["host"]["dst_bbox"][k]).to(dev) for k in ("min_xyz", "max_xyz"))
    g = torch.Generator().manual_seed(11)
    cand = (lo + torch.rand(200000, 3, generator=g).to(dev) * (hi - lo)).contiguous()
    mask = invert(frame, cand, cand, iters=0, tol=1e-5, max_step=frame["voxel"])[2]
    star = cand[mask > 0.25][:P].cpu().numpy()
    assert star.shape[0] == P
    x64, W64, J64 = X.backward_lbs_jac(star, *frame["np"], np.float64)
    assert (W64 > 0.2).all()
    guess = (star + np.random.RandomState(12).uniform(-0.5, 0.5, (P, 3)) * frame["voxel"]).astype(np.float32)
    return {"star": star, "x64": x64, "J64": J64, "guess": guess}


# ------------------------------------------------------------------------------------------ the kernel
def test_point_warp(dev, frame):
    """iters = 0 on the vertices of the frame's resolution-12 grid (several blocks, a ragged last one): x_skel / mask within the
    bounds tests/test_gpu_frame_mesh.py holds `grid_warp` to (5e-5 / 2e-6) of the float64 restatement, p == guess bit for bit, and
    the status of the float32 restatement wherever its residual is not within 1 % of tol.  Measured on one MI355X: see
    profiles/track_parity.json (`track.point_warp`)."""
    from hosnerf_amd import ops
    origin, h, dims = frame_grid(frame["pose"], 12)
    N = dims[0] * dims[1] * dims[2]
    assert N > 2 * ops.MT_BLOCK and N % ops.MT_BLOCK != 0
    pts = ops.grid_points(origin, h, dims, 0, N, device=dev)
    pn = pts.cpu().numpy()
    x64, W64, J64 = X.backward_lbs_jac(pn, *frame["np"], np.float64)
    assert (np.abs(W64 - 1e-4) > 1e-6).all()                                       # no row sits on the weight threshold itself
    tol = 1e-3
    rs = np.random.RandomState(2)
    d = rs.normal(size=(N, 3))
    target = (x64 + d / np.linalg.norm(d, axis=1, keepdims=True) * rs.uniform(0.0, 2.0 * tol, (N, 1))).astype(np.float32)
    target[::97] = np.nan                                                          # a target that is not finite: lost
    p, x, m, res, st, jac = invert(frame, torch.from_numpy(target).to(dev), pts, iters=0, tol=tol, max_step=frame["voxel"], want_jac=True)
    assert x.shape == (N, 3) and m.shape == (N,) and res.shape == (N,) and st.shape == (N,) and st.dtype == torch.int32 and jac.shape == (N, 3, 3)
    assert torch.equal(p, pts)
    ex, em = float(np.abs(x.cpu().numpy() - x64).max()), float(np.abs(m.cpu().numpy() - W64).max())
    _, _, _, rn32, st32, _ = X.warp_invert(target, pn, *frame["np"], 0, tol, frame["voxel"], np.float32)
    clear = ~(np.abs(rn32 - np.float32(tol)) <= 0.01 * tol)
    got = st.cpu().numpy()
    counts = np.bincount(got, minlength=3).tolist()
    print(f"point warp on {N} rows: x_skel {ex:.3e}, mask {em:.3e} vs float64; status counts {counts}, {int((~clear).sum())} rows within 1 % of tol")
    _record.record("track.point_warp", {"rows": N, "x_skel_vs_fp64": ex, "mask_vs_fp64": em, "status_counts": counts})
    assert ex < 5e-5 and em < 2e-6
    assert min(counts) > 10 and len(counts) == 3                                   # converged, out of steps and lost all occur
    assert np.array_equal(got[clear], st32[clear])
    fin = np.isfinite(rn32)
    assert np.abs(res.cpu().numpy()[fin] - rn32[fin]).max() < 1e-6 and not np.isfinite(res.cpu().numpy()[~fin]).any()
    e, _, _, _, s0 = invert(frame, pts[:0], pts[:0], iters=0, tol=tol, max_step=0.1)          # nothing to launch
    assert e.shape == (0, 3) and s0.shape == (0,) and s0.dtype == torch.int32


def smooth_case(dev):
    """K = 3 bones on a V = 8 volume of smooth positive weights, a box that is no cube, 1000 points reaching past the box."""
    rs = np.random.RandomState(7)
    K, V = 3, 8
    z, y, x = np.meshgrid(*(np.linspace(-1, 1, V),) * 3, indexing="ij")
    vol = np.stack([0.3 + 0.2 * np.sin(a[0] * x + a[1] * y + a[2] * z + ph) for a, ph in zip(rs.uniform(-2, 2, (K, 3)), rs.uniform(0, 6, K))], 0)
    from hosnerf_amd.freeview import rodrigues
    R = np.stack([rodrigues(r.astype(np.float32)) for r in rs.uniform(-0.5, 0.5, (K, 3))], 0)
    T = rs.uniform(-0.1, 0.1, (K, 3))
    bmin, ext = np.array([-1.0, -1.2, -0.9]), np.array([2.0, 2.4, 1.8])
    pts = bmin + rs.uniform(-0.05, 1.05, (1000, 3)) * ext
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    return K, f(pts), f(R), f(T), f(vol), f(bmin), f(2.0 / ext)


def test_jacobian(dev, frame, roots):
    """`jac` against the float64 restatement on K = 26, V = 32 (the synthetic prologue: points on the body and grid vertices) and on
    K = 3, V = 8.  Bound: 8 x the largest difference between the restatement's own float32 and float64 runs on the same inputs (a
    different summation order, FMA contraction).  Measured on one MI355X: see profiles/track_parity.json (`track.jacobian`)."""
    from hosnerf_amd import ops
    origin, h, dims = frame_grid(frame["pose"], 12)
    grid = ops.grid_points(origin, h, dims, 0, dims[0] * dims[1] * dims[2], device=dev)
    body = torch.cat([torch.from_numpy(roots["star"]).to(dev), grid], 0).contiguous()
    pro, pose = frame["pro"], frame["pose"]
    K3, pts3, R3, T3, vol3, bmin3, bscale3 = smooth_case(dev)
    record = {}
    for tag, K, pts, R, T, vol, bmin, bscale in (("K26_V32", frame["K"], body, pro["R_b"], pro["T_b"], pro["vol"], pose["cnl_bbox_min_xyz"], pose["cnl_bbox_scale_xyz"]),
                                                 ("K3_V8", K3, pts3, R3, T3, vol3, bmin3, bscale3)):
        out = ops.warp_invert(pts, pts, R, T, vol, bmin, bscale, K=K, iters=0, tol=1e-5, max_step=0.1, want_jac=True)
        a = [t.cpu().numpy() for t in (pts, R, T, vol, bmin, bscale)]
        x64, W64, J64 = X.backward_lbs_jac(*a, np.float64)
        x32, W32, J32 = X.backward_lbs_jac(*a, np.float32)
        e_ref = float(np.abs(J32.astype(np.float64) - J64).max())
        e_hip = float(np.abs(out[5].cpu().numpy().astype(np.float64) - J64).max())
        same = float((out[5].cpu().numpy() == J32).mean())
        print(f"jacobian {tag}: {pts.shape[0]} rows ({int((W64 > 1e-4).sum())} with weight), hip vs fp64 {e_hip:.3e}, fp32 restatement vs fp64 {e_ref:.3e} "
              f"(bound {8 * e_ref:.3e}), bit-equal to fp32 {same:.4f}, |J| max {np.abs(J64).max():.3f}")
        record[tag] = {"rows": int(pts.shape[0]), "e_hip": e_hip, "e_ref": e_ref, "bound": 8 * e_ref, "bit_equal_to_fp32": same}
        assert (W64 > 0.2).sum() > 100 and e_ref > 0 and np.isfinite(J64).all()
        assert e_hip <= 8 * e_ref
        assert float(np.abs(out[1].cpu().numpy() - x64).max()) < 5e-5 and float(np.abs(out[2].cpu().numpy() - W64).max()) < 2e-6
    _record.record("track.jacobian", record)


def test_known_roots(dev, frame, roots):
    """P = 700 roots p* (mask64 > 0.2), targets x64(p*), guesses within half a voxel, 8 steps, tol 1e-5.  With E the largest
    |x_kernel - x64| at the returned points: status 0 on >= 99 % of the rows; on every such row |x64(p) - target| <= tol + E and
    |p - p*| <= 2 (tol + E) / sigma_min(J64(p*)) (rows with sigma_min < 0.1 left out, at most 5 %).  The C entry on the middle of
    larger buffers writes its rows alone; two calls are bit-equal.  Measured on one MI355X: see profiles/track_parity.json
    (`track.known_roots`)."""
    from hosnerf_amd._lib import call, ptr
    pro, pose = frame["pro"], frame["pose"]
    P, tol, iters = roots["star"].shape[0], 1e-5, 8
    target = torch.from_numpy(roots["x64"].astype(np.float32)).to(dev)
    guess = torch.from_numpy(roots["guess"]).to(dev)
    one = invert(frame, target, guess, iters=iters, tol=tol, max_step=frame["voxel"], want_jac=True)
    two = invert(frame, target, guess, iters=iters, tol=tol, max_step=frame["voxel"], want_jac=True)
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    p, x, m, res, st, jac = (t.cpu().numpy() for t in one)
    x64, W64, J64p = X.backward_lbs_jac(p, *frame["np"], np.float64)
    E = float(np.linalg.norm(x - x64, axis=1).max())
    ok = st == X.CONVERGED
    smin = np.linalg.svd(roots["J64"], compute_uv=False)[:, -1]
    resid64 = np.linalg.norm(x64 - target.cpu().numpy().astype(np.float64), axis=1)
    dist = np.linalg.norm(p.astype(np.float64) - roots["star"], axis=1)
    judged = ok & (smin >= 0.1)
    print(f"known roots: status counts {np.bincount(st, minlength=3).tolist()} of {P}, E {E:.3e}, |x64(p) - target| max {resid64[ok].max():.3e} "
          f"(bound {tol + E:.3e}), sigma_min min {smin.min():.3f}, |p - p*| sigma_min / (tol + E) max {float((dist * smin)[judged].max() / (tol + E)):.3f} (bound 2)")
    _record.record("track.known_roots", {"rows": P, "converged": float(ok.mean()), "E": E, "residual64_max": float(resid64[ok].max()),
                                         "sigma_min_min": float(smin.min()), "dist_factor_max": float((dist * smin)[judged].max() / (tol + E))})
    assert ok.mean() >= 0.99
    assert (resid64[ok] <= tol + E).all()
    assert (smin < 0.1).mean() <= 0.05 and (dist[judged] <= 2 * (tol + E) / smin[judged]).all()
    assert (res[ok] <= tol).all() and float(np.abs(m - W64).max()) < 2e-6
    # the C entry on the middle of larger buffers filled with -7: its own rows, and nothing else
    first, count = 37, 517
    f = lambda *shape, dtype=torch.float32: torch.full(shape, -7, dtype=dtype, device=dev)
    pb, xb, mb, rb, sb, jb = f(count + 20, 3), f(count + 20, 3), f(count + 20), f(count + 20), f(count + 20, dtype=torch.int32), f(count + 20, 9)
    mid = slice(10, 10 + count)
    call("hos_warp_invert", ptr(target[first:first + count]), ptr(guess[first:first + count]), ptr(pro["R_b"]), ptr(pro["T_b"]), ptr(pro["vol"]),
         pro["vol"].shape[-1], frame["K"], ptr(pose["cnl_bbox_min_xyz"]), ptr(pose["cnl_bbox_scale_xyz"]), iters, tol, frame["voxel"], count,
         ptr(pb[mid]), ptr(xb[mid]), ptr(mb[mid]), ptr(rb[mid]), ptr(sb[mid], torch.int32), ptr(jb[mid]))
    for buf, whole in zip((pb, xb, mb, rb, sb, jb), one):
        assert torch.equal(buf[mid], whole[first:first + count].reshape(buf[mid].shape))
        assert bool((buf[:10] == -7).all()) and bool((buf[10 + count:] == -7).all())


# ------------------------------------------------------------------------------------------ mesh.track
@pytest.fixture(scope="module")
def template(dev, nets):
    from hosnerf_amd import mesh
    networks, turn = nets
    return mesh.extract(networks[0.1], turn, 0.7, resolution=24, level=LEVEL, normals=True)


def test_track_against_the_oracle(dev, nets, frame, template):
    """`mesh.track` of the resolution-24 template into the pose at 0.7, judged on the vertices with mask_canonical >= 0.05 (at least
    half of the template): >= 98 % converged where the float64 loop of tests/_track_expect.py on the oracle converges on >= 99 %;
    on converged vertices |G64(p) - c| <= tol + E_G with E_G = max |cnl_device - G64(p)|; `mask` within 2e-6 of the float64 mask at
    p; normals unit or zero and within 1e-3 of the float64 J^T n_c.  Measured on one MI355X: see profiles/track_parity.json
    (`track.mesh_track`)."""
    from hosnerf_amd import mesh
    net, pose, host = nets[0][0.1], frame["pose"], frame["host"]
    tpl = template
    V = tpl["vertices"].shape[0]
    assert tpl["state"] == 1 and V > 100 and tpl["normals"] is not None
    body = mesh.track(net, tpl, pose, space="body", normals=True)
    tol = 1e-3 * tpl["spacing"]
    assert body["tol"] == tol and body["state"] == 1 and body["frame_name"] == "frame_070" and body["time"] == 0.7 and body["space"] == "body"
    assert body["level"] == LEVEL and body["spacing"] == tpl["spacing"] and body["dims"] == tpl["dims"]
    assert body["faces"] is tpl["faces"] and body["colors"] is tpl["colors"]
    assert np.array_equal(body["to_world"], np.eye(4, dtype=np.float32))
    for k, shape, dtype in (("vertices", (V, 3), torch.float32), ("residual", (V,), torch.float32), ("converged", (V,), torch.bool),
                            ("mask", (V,), torch.float32), ("mask_canonical", (V,), torch.float32), ("cnl", (V, 3), torch.float32),
                            ("normals", (V, 3), torch.float32)):
        assert tuple(body[k].shape) == shape and body[k].dtype == dtype, k
    c = tpl["vertices"].cpu().numpy()
    p = body["vertices"].cpu().numpy()
    assert np.isfinite(p).all()
    mc = body["mask_canonical"].cpu().numpy()
    eye, zero = np.broadcast_to(np.eye(3, dtype=np.float32), (frame["K"], 3, 3)), np.zeros((frame["K"], 3), np.float32)
    assert np.abs(mc - FX.backward_lbs(c, eye, zero, *frame["np"][2:], np.float64)[1]).max() < 2e-6
    judged = mc >= 0.05
    assert judged.mean() >= 0.5, judged.mean()
    conv = body["converged"].cpu().numpy()
    # the input condition: the float64 loop on the oracle converges on these vertices
    pro64 = X.oracle_prologue(state_dict(0.1), host, np.float64)
    _, _, _, res64, conv64 = X.track(pro64, c[judged], 6, 4, tol)
    assert conv64.mean() >= 0.99, conv64.mean()
    ok = conv & judged
    G64, _, _ = X.G(pro64, p[ok].astype(np.float64))
    E_G = float(np.linalg.norm(body["cnl"].cpu().numpy()[ok] - G64, axis=1).max())
    back = np.linalg.norm(G64 - c[ok], axis=1)
    m64 = FX.backward_lbs(p, *frame["np"], np.float64)[1]
    em = float(np.abs(body["mask"].cpu().numpy() - m64).max())
    ratio = body["mask"].cpu().numpy()[judged] / mc[judged]
    print(f"mesh.track: V {V}, judged {judged.mean():.3f}, converged {conv[judged].mean():.4f} of them (float64 oracle {conv64.mean():.4f}), {conv.mean():.4f} of all; "
          f"residual median {np.median(body['residual'].cpu().numpy()[judged]):.3e} (tol {tol:.3e}), E_G {E_G:.3e}, |G64(p) - c| max {back.max():.3e}, "
          f"mask vs fp64 {em:.3e}, mask / mask_canonical median {np.median(ratio):.3f}")
    assert conv[judged].mean() >= 0.98
    assert (body["residual"].cpu().numpy()[conv] <= tol).all()
    assert (back <= tol + E_G).all()
    assert em < 2e-6
    # normals: unit or zero, and the float64 J^T n_c
    n = body["normals"].cpu().numpy().astype(np.float64)
    length = np.linalg.norm(n, axis=1)
    assert ((np.abs(length - 1.0) < 1e-5) | (length == 0)).all() and (length > 0).mean() > 0.9
    J64 = X.backward_lbs_jac(p, *frame["np"], np.float64)[2]
    want = np.einsum("vab,va->vb", J64, tpl["normals"].cpu().numpy().astype(np.float64))
    wl = np.linalg.norm(want, axis=1, keepdims=True)
    sure = judged & (wl[:, 0] > 0.1)                                               # a vanishing pull-back has no direction to compare
    en = float(np.abs(n - want / np.where(wl > 0, wl, 1.0))[sure].max())
    assert sure.mean() > 0.5 and en < 1e-3, en
    _record.record("track.mesh_track", {"V": int(V), "judged": float(judged.mean()), "converged_of_judged": float(conv[judged].mean()),
                                        "converged_fp64_oracle": float(conv64.mean()), "converged_of_all": float(conv.mean()), "tol": tol,
                                        "E_G": E_G, "back_max": float(back.max()), "mask_vs_fp64": em, "normals_vs_fp64": en,
                                        "mask_ratio_median": float(np.median(ratio))})
    # the scene's coordinates: `to_space` of the body-frame result
    world = mesh.track(net, tpl, pose, space="world", normals=True)
    A = pose["newsmpl_to_scale_world"].cpu().numpy()
    v64, f64, n64 = FX.to_space(p, tpl["faces"].cpu().numpy(), body["normals"].cpu().numpy(), A.astype(np.float64))
    assert np.array_equal(world["to_world"], A) and world["space"] == "world"
    assert (np.abs(world["vertices"].cpu().numpy().astype(np.float64) - v64) <= np.spacing(np.abs(v64).astype(np.float32))).all()
    assert np.array_equal(world["faces"].cpu().numpy(), f64) and np.abs(world["normals"].cpu().numpy() - n64).max() < 1e-6
    assert torch.equal(world["residual"], body["residual"]) and torch.equal(world["colors"], tpl["colors"])
    # another pose of the same state: the same topology, other vertices; the other state's template is refused
    other = mesh.track(net, tpl, on_device(host_pose(0.8, seed=4), dev), space="body")
    assert other["vertices"].shape == (V, 3) and other["faces"] is tpl["faces"] and other["normals"] is None
    assert float((other["vertices"] - body["vertices"]).abs().max()) > 1e-2
    with pytest.raises(ValueError):
        mesh.track(net, tpl, on_device(host_pose(0.2), dev), space="body")
    with pytest.raises(ValueError):
        mesh.track(net, {**tpl, "normals": None}, pose, space="body", normals=True)
    again = mesh.track(net, tpl, pose, space="body", normals=True)
    for k in ("vertices", "residual", "converged", "mask", "cnl", "normals"):
        assert torch.equal(again[k], body[k]), k


def test_track_at_the_identity(dev, nets, template):
    """Identity bone transforms (the T-pose, below the pose refiner's kick-in) and the non-rigid output layer zeroed: G is the
    identity wherever there is motion weight, and the tracked vertices are the template's."""
    from hosnerf_amd import mesh
    networks, turn = nets
    net, tpl = networks[0.0], template
    Rs, Ts = formats.body_pose_to_body_RTs(np.zeros(78, dtype=np.float32), turn.joints)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    pose = {"dst_Rs": f(Rs), "dst_Ts": f(Ts), "dst_posevec": torch.zeros(75, device=dev), "time": 0.7, "is_train": False,
            "iter_val": torch.zeros(1), "frame_name": "tpose", **turn.const}
    out = mesh.track(net, tpl, pose, space="body")
    assert float(out["mask_canonical"].min()) > 1e-3                               # every template vertex carries weight at this level
    assert float((out["vertices"] - tpl["vertices"]).abs().max()) <= 1e-6 and bool(out["converged"].all())
    # the T-pose's transforms are the identity up to the rounding of the kinematic chain, so a bone's q is c to about 1e-6; a trilinear
    # interpolant of weights in [0,1] changes by at most 1 / voxel = 9 per unit length: 1e-6 * 9 -> 1e-5
    assert float((out["mask"] - out["mask_canonical"]).abs().max()) <= 1e-5


# ------------------------------------------------------------------------------------------ the launcher
@pytest.mark.parametrize("gin,model,space", [("hosnerf_backpack.gin", "hosnerf", "world"), ("state_humanobject_backpack.gin", "state_humanobject", "body")])
def test_launcher_writes_one_topology_per_state(tmp_path, gin, model, space):
    from hosnerf_amd.freeview import write_scene_pixels
    scene = str(tmp_path / "scene")
    write_scene_pixels(scene, synth.write_scene_dir(scene, 6, 64, 64, seed=9))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("patch:\n  N_patches: 2\n  size: 16\n")
    logs = str(tmp_path / "logs")
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "--ginc", os.path.join(ROOT, "configs", gin), "--ginb", "run.max_steps=2",
           "--ginb", f'run.datadir="{scene}"', "--ginb", "run.run_mesh_track=True", "--ginb", "run.mesh_resolution=16", "--ginb", "run.mesh_level=0.001",
           "--scene_name", "synthetic", "--scene_dir", scene, "--cfg", str(cfg), "--logbase", logs, "--eval_skip", "3"]
    if space != "world":
        cmd += ["--ginb", f'run.mesh_space="{space}"']
    if model == "hosnerf":
        cmd += ["--ginb", 'run.human_path=""', "--ginb", 'run.bkgd_path=""']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    logdir = [os.path.join(logs, d) for d in os.listdir(logs)][0]
    folder = os.path.join(logdir, "mesh_track")
    meta = json.load(open(os.path.join(folder, "meshes.json")))
    frames = sorted(meta)
    assert len(frames) == 2
    assert sorted(os.listdir(folder)) == sorted(["meshes.json", "template_state_0.ply", "template_state_1.ply"] + [n + ".ply" for n in frames]
                                                + [n + "_residual.npy" for n in frames])
    templates = {s: formats.read_ply(os.path.join(folder, f"template_state_{s}.ply"), with_normals=True) for s in (0, 1)}
    assert sorted(meta[n]["state"] for n in frames) == [0, 1]                       # frames 0 and 3 of 6: either side of the transition
    for name in frames:
        row = meta[name]
        assert set(row) == {"frame_name", "time", "state", "template", "V", "F", "converged", "residual", "mask_ratio", "volume", "area", "level",
                            "spacing", "dims", "space", "to_world"}
        assert set(row["residual"]) == {"median", "p99", "max"} and set(row["mask_ratio"]) == {"median", "min", "max"}
        assert row["frame_name"] == name and row["template"] == f"template_state_{row['state']}.ply" and row["space"] == space
        assert row["level"] == 0.001 and max(row["dims"]) == 16 + 3 and 0.0 <= row["converged"] <= 1.0
        tv, tf, tc, tn = templates[row["state"]]
        v, f, c, n = formats.read_ply(os.path.join(folder, name + ".ply"), with_normals=True)
        assert row["V"] == v.shape[0] == tv.shape[0] > 0 and row["F"] == f.shape[0] and n.shape == v.shape          # run.mesh_normals defaults to True
        assert np.array_equal(c, tc) and np.isfinite(v).all()
        A = np.array(row["to_world"])
        mirrored = space == "world" and np.linalg.det(A[:3, :3]) < 0
        assert np.array_equal(f, tf[:, [0, 2, 1]] if mirrored else tf)             # one topology per state
        res = np.load(os.path.join(folder, name + "_residual.npy"))
        assert res.dtype == np.float32 and res.shape == (row["V"],)
        print(f"{model} {name} ({space}): state {row['state']} V {row['V']} F {row['F']} converged {row['converged']:.3f} residual {row['residual']} "
              f"mask_ratio {row['mask_ratio']}")
    assert "results.json" not in os.listdir(logdir)
    if model == "hosnerf":
        s1 = subprocess.run([sys.executable, os.path.join(ROOT, "run.py"), "--ginc", os.path.join(ROOT, "configs", "state_mipnerf360_backpack.gin"),
                             "--ginb", "run.max_steps=2", "--ginb", "run.run_mesh_track=True", "--scene_name", "synthetic", "--cpu",
                             "--logbase", str(tmp_path / "logs1")], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert s1.returncode != 0 and "run.run_mesh_track" in s1.stderr and "stage 1" in s1.stderr
