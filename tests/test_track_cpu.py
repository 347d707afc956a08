"""The tracked mesh without a GPU: the restatement tests/_track_expect.py against torch autograd of the oracle's backward LBS and on
known roots (it must be right before the kernel is judged by it), its status codes, the argument checks of `mesh.track` /
`ops.warp_invert` / `hos_warp_invert`, and the launcher's `run.run_mesh_track` binding."""
import ctypes
import os
import tempfile
import types

import numpy as np
import pytest
import torch

import oracle.human as oh
from hosnerf_amd import synth
from tests import _frame_mesh_expect as FX
from tests import _track_expect as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOTS_SEED = 11                # known roots: the seed of the points and the guesses (every row converges; see the test)


def host_pose(time=0.7):
    hb = synth.human_batch(8, seed=3, time=time, is_train=False, iter_val=1e7)
    p = {k: hb[k] for k in ("dst_Rs", "dst_Ts", "dst_posevec", "cnl_gtfms", "motion_weights_priors", "cnl_bbox_min_xyz", "cnl_bbox_max_xyz",
                            "cnl_bbox_scale_xyz", "iter_val")}
    p.update(time=float(time), box=(hb["dst_bbox_min_xyz"].numpy(), hb["dst_bbox_max_xyz"].numpy()))
    return p


def build_prologue():
    """The float64 prologue of the synthetic pose at 0.7 (rotations well away from the identity), as numpy float64 arrays too."""
    pro = X.oracle_prologue(synth.human_state_dict(777, 2), host_pose(), np.float64)
    K = pro["K"]
    assert float((pro["R_b"] - torch.eye(3, dtype=torch.float64)).abs().max()) > 0.05
    # the kernel's inputs are fp32 numbers: round the transforms and the volume once, so that every float64 run below sees those
    f32 = lambda t: t.float().double()
    pro.update(R_b=f32(pro["R_b"]), T_b=f32(pro["T_b"]), vol=f32(pro["vol"]))
    pro["np"] = tuple(pro[k].numpy() for k in ("R_b", "T_b", "vol", "bmin", "bscale"))
    pro["np"] = (pro["np"][0][:K], pro["np"][1][:K]) + pro["np"][2:]
    pro["voxel"] = float(2.0 / pro["bscale"].min() / (pro["vol"].shape[-1] - 1))
    return pro


@pytest.fixture(scope="module")
def pro():
    return build_prologue()


def body_points(n, seed, box):
    rs = np.random.RandomState(seed)
    lo, hi = box
    return (lo + rs.uniform(0.0, 1.0, (n, 3)) * (hi - lo)).astype(np.float32)


def weighted_points(pro, n, seed, lo):
    """n points of the frame's box (fp32 values) whose float64 mask exceeds `lo`: the body fills under 1 % of the box."""
    R, T, vol, bmin, bscale = pro["np"]
    cand = body_points(160 * n, seed, host_pose()["box"])
    _, W, _ = X.backward_lbs_jac(cand, R, T, vol, bmin, bscale, np.float64)
    out = cand[W > lo][:n]
    assert out.shape[0] == n, (out.shape[0], n)
    return out


def test_jacobian_is_autograd_of_the_oracle(pro):
    """J of the restatement in float64 == torch autograd of `oracle.human.backward_lbs` on 200 random points of the frame's box
    (most of them off the body), 200 on the body and 100 body points moved so that their heaviest bone maps them to within 1e-3
    voxel of a cell face (not onto it: on a face the derivative is one-sided)."""
    R, T, vol, bmin, bscale = pro["np"]
    V = vol.shape[-1]
    rs = np.random.RandomState(5)
    rand = body_points(200, 5, host_pose()["box"])
    body = weighted_points(pro, 300, 6, 0.05)
    src = body[200:].astype(np.float64)
    q = np.einsum("kab,pb->pka", R, src) + T[None]                                    # [100,K,3]
    w = np.stack([FX.trilinear_zero(vol[i], *((q[:, i] - bmin) * bscale - 1.0).T) for i in range(R.shape[0])], 1)
    k = w.argmax(1)
    qk = q[np.arange(100), k]
    idx = ((qk - bmin) * bscale) / 2.0 * (V - 1)
    axis = rs.randint(0, 3, 100)
    off = rs.uniform(2e-4, 1e-3, 100) * rs.choice([-1.0, 1.0], 100)
    idx[np.arange(100), axis] = np.round(idx[np.arange(100), axis]) + off
    q_new = bmin + (idx / (V - 1) * 2.0) / bscale
    near = (src + np.einsum("pab,pb->pa", np.linalg.inv(R[k]), q_new - qk)).astype(np.float32)
    pts = np.concatenate([rand, body[:200], near], 0)
    x, W, J = X.backward_lbs_jac(pts, R, T, vol, bmin, bscale, np.float64)
    t = torch.from_numpy(pts).double().requires_grad_(True)
    xo, wo = oh.backward_lbs(t, pro["R_b"], pro["T_b"], pro["vol"], pro["bmin"], pro["bscale"])
    Jo = torch.stack([torch.autograd.grad(xo[:, a].sum(), t, retain_graph=True)[0] for a in range(3)], 1).numpy()
    assert np.allclose(x, xo.detach().numpy(), rtol=1e-9, atol=1e-9) and np.allclose(W, wo.detach().numpy()[:, 0], rtol=1e-9, atol=1e-12)
    assert (W[200:400] > 0.05).all() and (W[400:] > 1e-4).mean() > 0.9 and (W < 1e-4).sum() > 50                                     # on the body, near faces, and off it
    qn = np.einsum("pab,pb->pa", R[k], pts[400:].astype(np.float64)) + T[k]
    frac = (((qn - bmin) * bscale) / 2.0 * (V - 1))[np.arange(100), axis]
    assert (np.abs(frac - np.round(frac)) < 2e-3).all() and (np.abs(frac - np.round(frac)) > 1e-5).all()
    assert np.allclose(J, Jo, rtol=1e-9, atol=1e-9), float(np.abs(J - Jo).max())
    # the value is the frame mesh's restatement, bit for bit, in both dtypes
    for dt in (np.float32, np.float64):
        xf, wf = FX.backward_lbs(pts, R, T, vol, bmin, bscale, dt)
        xj, wj, _ = X.backward_lbs_jac(pts, R, T, vol, bmin, bscale, dt)
        assert np.array_equal(xf, xj) and np.array_equal(wf, wj)


def known_roots(pro, n, seed):
    """p* [n,3] (fp32 values) with mask64 > 0.2, their targets x64(p*) and guesses p* + U(-1/2, 1/2) voxel."""
    R, T, vol, bmin, bscale = pro["np"]
    star = weighted_points(pro, n, seed, 0.2)
    x64, _, J64 = X.backward_lbs_jac(star, R, T, vol, bmin, bscale, np.float64)
    guess = (star + np.random.RandomState(seed + 1).uniform(-0.5, 0.5, (n, 3)) * pro["voxel"]).astype(np.float32)
    return star, x64, guess, J64


def test_known_roots_are_recovered(pro):
    """p* with mask > 0.2, target x64(p*), guess within half a voxel, 8 steps of at most one voxel: every row converges to 1e-9 and
    lands on p* (the map is one-to-one there: sigma_min(J) is bounded away from 0)."""
    R, T, vol, bmin, bscale = pro["np"]
    star, x64, guess, J64 = known_roots(pro, 300, ROOTS_SEED)
    p, x, W, rn, status, J = X.warp_invert(x64, guess, R, T, vol, bmin, bscale, 8, 1e-9, pro["voxel"], np.float64, exact=True)
    smin = np.linalg.svd(J64, compute_uv=False)[:, -1]
    print(f"known roots: status counts {np.bincount(status, minlength=3)}, residual max {rn.max():.3e}, sigma_min(J) min {smin.min():.3f}, "
          f"|p - p*| max {np.abs(p - star).max():.3e}")
    assert (status == X.CONVERGED).all() and rn.max() <= 1e-9
    assert np.abs(p - star).max() <= 2 * 1e-9 / smin.min() + 1e-12
    # what is returned is evaluated at the returned p
    xe, We, Je = X.backward_lbs_jac(p, R, T, vol, bmin, bscale, np.float64, exact=True)
    assert np.array_equal(xe, x) and np.array_equal(We, W) and np.array_equal(Je, J)
    assert np.array_equal(rn, X._norm3(x64 - x))


def test_status_codes(pro):
    R, T, vol, bmin, bscale = pro["np"]
    star, x64, guess, _ = known_roots(pro, 8, ROOTS_SEED)
    vox = pro["voxel"]
    for dt in (np.float32, np.float64):
        # a NaN target, a guess outside the volume: lost at once, p stays the guess
        bad = x64.copy()
        bad[0, 1] = np.nan
        far = guess.copy()
        far[1] = [50.0, -60.0, 70.0]
        p, x, W, rn, st, _ = X.warp_invert(bad, far, R, T, vol, bmin, bscale, 8, 1e-5, vox, dt)
        assert st[0] == X.LOST and st[1] == X.LOST and W[1] == 0 and (st[2:] == X.CONVERGED).all()
        assert np.array_equal(p[:2], far[:2].astype(dt)) and not np.isfinite(rn[0])
        # iters = 0: a point warp; out of steps unless the guess is the root already
        p, x, W, rn, st, J = X.warp_invert(x64, guess, R, T, vol, bmin, bscale, 0, 1e-5, vox, dt)
        xe, We, Je = X.backward_lbs_jac(guess, R, T, vol, bmin, bscale, dt)
        assert (st == X.LIMIT).all() and np.array_equal(p, guess.astype(dt)) and np.array_equal(x, xe) and np.array_equal(W, We) and np.array_equal(J, Je)
        p, _, _, _, st, _ = X.warp_invert(x64, star, R, T, vol, bmin, bscale, 0, 1e-5, vox, dt)
        assert (st == X.CONVERGED).all() and np.array_equal(p, star.astype(dt))
        # the identity pose: x(p) = p wherever there is weight, so p == c and the row converges at it = 0
        eye, zero = np.broadcast_to(np.eye(3), R.shape).copy(), np.zeros_like(T)
        c = x64.astype(np.float32)
        p, x, W, rn, st, _ = X.warp_invert(c, c, eye, zero, vol, bmin, bscale, 4, 1e-5, vox, dt)
        on = W > 1e-4
        assert on.sum() >= 4 and (st[on] == X.CONVERGED).all() and (st[~on] == X.LOST).all() and np.array_equal(p, c.astype(dt))
    # a singular Jacobian: a volume that is constant in space and bones that do not turn give J = sum w_i R_i / W with R_i = 0
    flat = np.ones((2, 4, 4, 4), np.float32)
    p, x, W, rn, st, _ = X.warp_invert(np.ones((1, 3)), np.zeros((1, 3)), np.zeros((2, 3, 3)), np.zeros((2, 3)), flat, -np.ones(3), np.ones(3), 3, 1e-5, 0.1)
    assert st[0] == X.LOST and W[0] == 2.0 and np.array_equal(p, np.zeros((1, 3)))


# ------------------------------------------------------------------------------------------ argument checks
def test_track_argument_errors():
    from hosnerf_amd import _lib, mesh, ops
    net = types.SimpleNamespace(transitions_times=np.array([0.4], np.float32))
    tpl = {"vertices": torch.zeros(4, 3), "faces": torch.zeros(2, 3, dtype=torch.int32), "colors": torch.zeros(4, 3, dtype=torch.uint8),
           "state": 1, "spacing": 0.1, "dims": (4, 4, 4), "level": 0.5, "normals": None}
    pose = {"time": 0.7}
    with pytest.raises(ValueError) as e:
        mesh.track(net, tpl, pose, space="camera")
    assert "camera" in str(e.value)
    with pytest.raises(ValueError) as e:
        mesh.track(net, dict(tpl, state=0), pose, space="body")                      # the template of the other object state
    assert "state" in str(e.value)
    with pytest.raises(ValueError) as e:
        mesh.track(net, tpl, {"time": 0.2}, space="body")
    assert "state" in str(e.value)
    with pytest.raises(ValueError) as e:
        mesh.track(net, tpl, pose, space="body", normals=True)                       # a template without normals
    assert "normals" in str(e.value)
    with pytest.raises(ValueError) as e:
        mesh.track(net, tpl, pose, space="world")                                    # no newsmpl_to_scale_world
    assert "newsmpl_to_scale_world" in str(e.value)
    for kw in ({"chunk": 16383}, {"outer": 0}, {"iters": -1}, {"tol": 0.0}):
        with pytest.raises(ValueError):
            mesh.track(net, tpl, pose, space="body", **kw)
    with pytest.raises(ValueError):
        mesh.track(net, tpl, {}, space="body")                                       # no time: no object state
    z = torch.zeros
    with pytest.raises(_lib.HosLibraryError):                                        # shapes that do not fit (and no CPU path)
        ops.warp_invert(z(5, 3), z(4, 3), z(26, 3, 3), z(26, 3), z(27, 4, 4, 4), z(3), torch.ones(3))
    with pytest.raises(_lib.HosLibraryError):
        ops.warp_invert(z(4, 3), z(4, 3), z(26, 3, 3), z(26, 3), z(25, 4, 4, 4), z(3), torch.ones(3))
    for text in ("tracked mesh", "mask_canonical", "neglects", "per object state", "counterpart"):
        assert text in mesh.__doc__.lower().replace("\n", " "), text


def test_entry_point_validates_without_gpu():
    """-1 (HOS_E_ARG) / -3 (HOS_E_SHAPE) of hos_warp_invert on null, empty and oversized arguments, before any launch."""
    from hosnerf_amd import _lib
    lib = _lib.load()
    assert "hos_warp_invert" in _lib.PROTOTYPES and hasattr(lib, "hos_warp_invert") and len(_lib.PROTOTYPES["hos_warp_invert"]) == 20
    buf = (ctypes.c_float * 16)()
    a = ctypes.addressof(buf)
    names = ("target", "guess", "R", "T", "vol", "V", "K", "bmin", "bscale", "iters", "tol", "max_step", "P", "p", "x", "mask", "res", "status", "jac")
    base = dict(zip(names, (a, a, a, a, a, 32, 26, a, a, 4, 1e-5, 0.1, 1, a, a, a, a, a, 0)))
    inv = lambda **kw: lib.hos_warp_invert(*[{**base, **kw}[n] for n in names], 0)
    for k in ("target", "guess", "R", "T", "vol", "bmin", "bscale", "p", "x", "mask", "res", "status"):
        assert inv(**{k: 0}) == -1, k
    assert inv(P=0) == -1 and inv(P=-3) == -1 and inv(iters=-1) == -1
    for k in ("tol", "max_step"):
        assert inv(**{k: 0.0}) == -1 and inv(**{k: -1.0}) == -1 and inv(**{k: float("nan")}) == -1, k
    assert inv(K=0) == -3 and inv(K=33) == -3 and inv(V=1) == -3 and inv(P=256 * (2 ** 31 - 1) + 1) == -3


def test_launcher_binding_and_refusals():
    import run as launcher
    for name, model in (("hosnerf_backpack.gin", "hosnerf"), ("state_humanobject_backpack.gin", "state_humanobject")):
        plan = launcher.main(["--ginc", os.path.join(ROOT, "configs", name), "--scene_name", "Backpack", "--cpu", "--logbase", tempfile.mkdtemp(),
                              "--ginb", "run.max_steps=3", "--ginb", "run.run_mesh_track=True", "--ginb", 'run.mesh_space="body"'])
        assert plan["model_name"] == model and plan["gin"]["run.run_mesh_track"] is True and plan["gin"]["run.mesh_space"] == "body"
    s1 = os.path.join(ROOT, "configs", "state_mipnerf360_backpack.gin")
    with pytest.raises(SystemExit) as e:                                            # stage 1 has no human-object network
        launcher.main(["--ginc", s1, "--scene_name", "Backpack", "--cpu", "--logbase", tempfile.mkdtemp(), "--ginb", "run.max_steps=3",
                       "--ginb", "run.run_mesh_track=True"])
    assert "run.run_mesh_track" in str(e.value) and "stage 1" in str(e.value)
    with pytest.raises(SystemExit) as e:
        launcher.main(["--ginc", os.path.join(ROOT, "configs", "hosnerf_backpack.gin"), "--scene_name", "Backpack", "--cpu", "--logbase",
                       tempfile.mkdtemp(), "--ginb", "run.max_steps=3", "--ginb", "run.run_mesh_track=True", "--ginb", 'run.mesh_space="camera"'])
    assert "run.mesh_space" in str(e.value)
    with pytest.raises(SystemExit) as e:                                            # no scene directory
        launcher.track_meshes(None, {}, None, None, "/nonexistent/last.ckpt", tempfile.mkdtemp(), "cpu", 0, 1)
    assert "--scene_dir" in str(e.value) and "run.run_mesh_track" in str(e.value)
    assert "run.run_mesh_track" in launcher.__doc__
