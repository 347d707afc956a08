"""The tracked mesh restated: what `ops.warp_invert` (hos_track.hip) and `mesh.track` must produce, operation by operation in the
dtype asked for (float32: the kernel's own arithmetic; float64: the yardstick).  Built on tests/_frame_mesh_expect.py (the taps and
the backward LBS).  Used by test_track_cpu.py (the restatement against autograd of the oracle and on known roots) and
test_gpu_track.py (the kernel and `mesh.track` against it).

Rules (include/hosrender.h, "The tracked mesh"):
  x(p), W(p)   the backward LBS of `_frame_mesh_expect.backward_lbs`
  J = dx/dp    (sum_i (q_i (x) g_i + w_i R_i) - x (x) sum_i g_i) / W,  g_i = R_i^T grad_q w_i;  grad_q w_i the gradient of the trilinear
               interpolant inside the cell of floor, per axis times bbox_scale * (V - 1) / 2; M / 1e-4 where W <= 1e-4 (the clamp)
  row          p = guess; evaluate; r = target - x; LOST (2) on a non-finite r or W <= 1e-4; CONVERGED (0) on |r| <= tol; LIMIT (1) at
               it == iters; LOST on !(|det J| > 1e-12); else p += J^-1 r (adjugate / det) cut to max_step, and again
  track        guess = forward LBS of c; `outer` rounds of warp_invert on c - delta and delta = G(p) - x_skel(p)"""
import numpy as np
import torch

import oracle.human as oh
from tests import _frame_mesh_expect as FX

CONVERGED, LIMIT, LOST = 0, 1, 2


def _as(a, dtype, exact=False):
    """The kernel's inputs are fp32 numbers: round through fp32, then widen.  `exact`: take a float64 quantity of the oracle as it is."""
    return np.asarray(a, dtype=dtype) if exact else np.asarray(a, dtype=np.float32).astype(dtype)


def trilinear_zero_grad(vol, gx, gy, gz, dtype=np.float64, exact=False):
    """One channel vol [V,V,V] (z,y,x) at normalised coordinates [P] -> (value, d/dix, d/diy, d/diz) [P] each, the derivatives per
    voxel index; `trilinear_zero_grad` of hos_trilinear_grad.h.  The value is `_frame_mesh_expect.trilinear_zero`'s."""
    V = vol.shape[-1]
    flat = _as(vol, dtype, exact).reshape(-1)
    s = dtype(V - 1)
    cx, cy, cz = ((gx + dtype(1)) / dtype(2)) * s, ((gy + dtype(1)) / dtype(2)) * s, ((gz + dtype(1)) / dtype(2)) * s
    with np.errstate(invalid="ignore"):
        fx, wx0, wx1 = FX._taps(cx, dtype)
        fy, wy0, wy1 = FX._taps(cy, dtype)
        fz, wz0, wz1 = FX._taps(cz, dtype)
        sane = (fx >= -1) & (fx <= V) & (fy >= -1) & (fy <= V) & (fz >= -1) & (fz <= V)
    x0, y0, z0 = (np.where(sane, f, -2).astype(np.int64) for f in (fx, fy, fz))
    out, ax, ay, az = (np.zeros(cx.shape, dtype=dtype) for _ in range(4))
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                x, y, z = x0 + dx, y0 + dy, z0 + dz
                ok = sane & (x >= 0) & (x < V) & (y >= 0) & (y < V) & (z >= 0) & (z < V)
                wx, wy, wz = (wx1 if dx else wx0), (wy1 if dy else wy0), (wz1 if dz else wz0)
                v = flat[(np.clip(z, 0, V - 1) * V + np.clip(y, 0, V - 1)) * V + np.clip(x, 0, V - 1)]
                with np.errstate(invalid="ignore"):
                    out = np.where(ok, out + v * ((wx * wy) * wz), out)
                    tx, ty, tz = v * (wy * wz), v * (wx * wz), v * (wx * wy)
                    ax = np.where(ok, ax + tx if dx else ax - tx, ax)
                    ay = np.where(ok, ay + ty if dy else ay - ty, ay)
                    az = np.where(ok, az + tz if dz else az - tz, az)
    return out, ax, ay, az


def backward_lbs_jac(pts, R, T, vol, bbox_min, bbox_scale, dtype=np.float64, exact=False):
    """pts [P,3], R [K,3,3], T [K,3], vol [>=K,V,V,V], bbox_min / bbox_scale [3] -> (x [P,3], W [P], J [P,3,3] = dx/dp, [out][in])."""
    c = lambda a: _as(a, dtype, exact)
    p, R, T, bmin, bscale = c(pts), c(R), c(T), c(bbox_min), c(bbox_scale)
    K, V, P = R.shape[0], vol.shape[-1], p.shape[0]
    scale = bscale * dtype(V - 1) / dtype(2)
    wsum = np.zeros(P, dtype=dtype)
    acc = np.zeros((P, 3), dtype=dtype)
    G = np.zeros((P, 3), dtype=dtype)
    M = np.zeros((P, 3, 3), dtype=dtype)
    with np.errstate(all="ignore"):
        for i in range(K):
            q = np.stack([((R[i, a, 0] * p[:, 0] + R[i, a, 1] * p[:, 1]) + R[i, a, 2] * p[:, 2]) + T[i, a] for a in range(3)], 1)
            g = (q - bmin[None]) * bscale[None] - dtype(1)
            w, dx, dy, dz = trilinear_zero_grad(vol[i], g[:, 0], g[:, 1], g[:, 2], dtype, exact)
            dx, dy, dz = dx * scale[0], dy * scale[1], dz * scale[2]
            h = np.stack([(R[i, 0, b] * dx + R[i, 1, b] * dy) + R[i, 2, b] * dz for b in range(3)], 1)
            wsum = wsum + w
            acc = acc + w[:, None] * q
            G = G + h
            M = M + (q[:, :, None] * h[:, None, :] + w[:, None, None] * R[i][None])
        den = np.maximum(wsum, dtype(1e-4))
        x = acc / den[:, None]
        M = np.where((wsum > dtype(1e-4))[:, None, None], M - x[:, :, None] * G[:, None, :], M)
        J = M / den[:, None, None]
    return x, wsum, J


def _norm3(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def warp_invert(target, guess, R, T, vol, bbox_min, bbox_scale, iters, tol, max_step, dtype=np.float64, exact=False):
    """The row algorithm of hos_warp_invert -> (p [P,3], x [P,3], W [P], residual [P], status int32 [P], J [P,3,3]), everything at
    the returned p."""
    t = _as(target, dtype, exact)
    p = _as(guess, dtype, exact).copy()
    R, T, vol, bbox_min, bbox_scale = (_as(a, dtype, exact) for a in (R, T, vol, bbox_min, bbox_scale))          # from here on nothing is rounded again
    tol, max_step = dtype(np.float32(tol)), dtype(np.float32(max_step))
    P = p.shape[0]
    x, W, J = np.zeros((P, 3), dtype), np.zeros(P, dtype), np.zeros((P, 3, 3), dtype)
    rn, status = np.zeros(P, dtype), np.full(P, -1, np.int32)
    active = np.ones(P, dtype=bool)
    for it in range(int(iters) + 1):
        idx = np.nonzero(active)[0]
        if idx.size == 0:
            break
        xe, We, Je = backward_lbs_jac(p[idx], R, T, vol, bbox_min, bbox_scale, dtype, exact=True)
        with np.errstate(all="ignore"):
            r = t[idx] - xe
            rne = _norm3(r)
            x[idx], W[idx], J[idx], rn[idx] = xe, We, Je, rne
            lost = ~np.isfinite(r).all(1) | ~(We > dtype(1e-4))
            conv = ~lost & (rne <= tol)
            limit = ~lost & ~conv & (it == int(iters))
            j = lambda a, b: Je[:, a, b]
            c00, c01, c02 = j(1, 1) * j(2, 2) - j(1, 2) * j(2, 1), j(1, 0) * j(2, 2) - j(1, 2) * j(2, 0), j(1, 0) * j(2, 1) - j(1, 1) * j(2, 0)
            det = (j(0, 0) * c00 - j(0, 1) * c01) + j(0, 2) * c02
            singular = ~lost & ~conv & ~limit & ~(np.abs(det) > dtype(1e-12))
            lost = lost | singular
            go = ~lost & ~conv & ~limit
            rx, ry, rz = r[:, 0], r[:, 1], r[:, 2]
            d = np.stack([((c00 * rx + (j(0, 2) * j(2, 1) - j(0, 1) * j(2, 2)) * ry) + (j(0, 1) * j(1, 2) - j(0, 2) * j(1, 1)) * rz) / det,
                          (((j(1, 2) * j(2, 0) - j(1, 0) * j(2, 2)) * rx + (j(0, 0) * j(2, 2) - j(0, 2) * j(2, 0)) * ry)
                           + (j(0, 2) * j(1, 0) - j(0, 0) * j(1, 2)) * rz) / det,
                          ((c02 * rx + (j(0, 1) * j(2, 0) - j(0, 0) * j(2, 1)) * ry) + (j(0, 0) * j(1, 1) - j(0, 1) * j(1, 0)) * rz) / det], 1)
            dn = _norm3(d)
            d = np.where((dn > max_step)[:, None], d * (max_step / dn)[:, None], d)
        status[idx[lost]], status[idx[conv]], status[idx[limit]] = LOST, CONVERGED, LIMIT
        p[idx[go]] = p[idx[go]] + d[go]
        active[idx[~go]] = False
    assert (status >= 0).all()
    return p, x, W, rn, status, J


# ------------------------------------------------------------------------------------------ the outer loop, on the oracle
def oracle_prologue(sd, pose, dtype=np.float64, cfg=None):
    """The per-frame part of `oracle.human.human_forward` for a pose dict (host tensors; `SceneItems.frame_pose`'s keys) at
    is_train = False, in torch float32 or float64 -> R_b, T_b, R_f, T_f, vol, band_w, cond, bmin, bscale and `sd` in that dtype."""
    c = dict(oh.DEFAULT_CFG)
    c.update(cfg or {})
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    sd = {k: v.to(tdt) for k, v in sd.items()}
    f = lambda k: pose[k].detach().cpu().to(tdt)
    iter_val = float(torch.as_tensor(pose.get("iter_val", 1e7)).reshape(-1)[0])
    Rs, Ts, pv = f("dst_Rs"), f("dst_Ts"), f("dst_posevec").reshape(-1)
    with torch.no_grad():
        if iter_val >= c["pose_kick_in_iter"]:
            dR, dT = oh.pose_refiner(sd, pv[None], total_bones=c["total_bones"])
            Rs, Ts = torch.cat([Rs[0:1], torch.matmul(Rs[1:], dR[0])], 0), torch.cat([Ts[0:1], Ts[1:] + dT[0]], 0)
        R_b, T_b, R_f, T_f = oh.motion_basis(Rs, Ts, f("cnl_gtfms"))
        vol = oh.motion_weight_volume(sd, f("motion_weights_priors"))
        band_w = oh.hannw_weights(iter_val, c["nonrigid_kick_in_iter"], c["nonrigid_full_band_iter"], c["nonrigid_multires"]).to(tdt)
    cond = (torch.zeros_like(pv) * pv if iter_val < c["nonrigid_kick_in_iter"] else pv)[None]
    return {"R_b": R_b, "T_b": T_b, "R_f": R_f, "T_f": T_f, "vol": vol, "band_w": band_w, "cond": cond, "bmin": f("cnl_bbox_min_xyz"),
            "bscale": f("cnl_bbox_scale_xyz"), "sd": sd, "K": c["total_bones"]}


def nonrigid(pro, x):
    """G's second half: the non-rigid MLP of the oracle at x_skel [P,3] (numpy) -> [P,3] numpy, in the prologue's dtype."""
    xt = torch.as_tensor(np.asarray(x), dtype=pro["vol"].dtype)
    with torch.no_grad():
        return oh.nonrigid_mlp(pro["sd"], "non_rigid_mlp.", oh.hannw_embed(xt, pro["band_w"]), xt, pro["cond"]).numpy()


def G(pro, p):
    """The frame's backward map at body-frame points p [P,3], in the prologue's dtype with nothing rounded to fp32 on the way ->
    (cnl [P,3], x_skel [P,3], mask [P])."""
    K, dtype = pro["K"], (np.float64 if pro["vol"].dtype == torch.float64 else np.float32)
    n = lambda t: t.numpy()
    x, W, _ = backward_lbs_jac(p, n(pro["R_b"])[:K], n(pro["T_b"])[:K], n(pro["vol"]), n(pro["bmin"]), n(pro["bscale"]), dtype, exact=True)
    return nonrigid(pro, x), x, W


def track(pro, c, outer, iters, tol, dtype=np.float64):
    """`mesh.track`'s loop for the canonical points c [P,3] on an `oracle_prologue` of the same dtype -> (p, cnl, mask, residual,
    converged): guess = the oracle's forward LBS of c; per round `warp_invert` (tolerance tol / 4, steps of one voxel) on c - delta,
    then delta = G(p) - x_skel(p).  A row lost in some round, or stepped to a non-finite p, keeps what it had and is not converged."""
    K = pro["K"]
    n = lambda t: t.numpy()
    R, T, vol, bmin, bscale = n(pro["R_b"])[:K], n(pro["T_b"])[:K], n(pro["vol"]), n(pro["bmin"]), n(pro["bscale"])
    c = np.asarray(c, dtype=np.float32).astype(dtype)
    ct = torch.as_tensor(c)
    with torch.no_grad():
        p = n(oh.forward_lbs(ct, pro["R_f"], pro["T_f"], pro["vol"], pro["bmin"], pro["bscale"])).astype(dtype)
    max_step = dtype(2.0) / bscale.min() / dtype(vol.shape[-1] - 1)
    P = c.shape[0]
    delta, alive, status = np.zeros_like(c), np.ones(P, bool), np.full(P, LOST, np.int32)
    cnl, mask, res = np.full_like(c, np.nan), np.zeros(P, dtype), np.full(P, np.inf, dtype)
    for _ in range(int(outer)):
        p_o, x_o, m_o, _, st_o, _ = warp_invert(c - delta, p, R, T, vol, bmin, bscale, iters, tol / 4.0, max_step, dtype, exact=True)
        cnl_o = nonrigid(pro, x_o).astype(dtype)
        ok = alive & np.isfinite(p_o).all(1)
        with np.errstate(all="ignore"):
            p, cnl, delta = np.where(ok[:, None], p_o, p), np.where(ok[:, None], cnl_o, cnl), np.where(ok[:, None], cnl_o - x_o, delta)
            mask, res = np.where(ok, m_o, mask), np.where(ok, np.linalg.norm(cnl_o - c, axis=1), res)
        status = np.where(ok, st_o, status)
        alive = ok & (st_o != LOST)
    return p, cnl, mask, res, alive & (status == CONVERGED) & (res <= tol)
