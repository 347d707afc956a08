"""The frame mesh restated in numpy: what `ops.grid_warp` and `ops.mesh_vertex_normals` (hos_mesh.hip) and `mesh.to_space` must
produce, operation by operation in the dtype asked for (float32: the kernels' own arithmetic; float64: the yardstick).  Used by
test_frame_mesh_cpu.py (the restatements against the oracle and on analytic fields) and test_gpu_frame_mesh.py (the kernels against
them).

Rules (include/hosrender.h, "The frame mesh"):
  backward LBS   q_i = (R_i p) + T_i;  w_i = zero-padded trilinear tap of vol channel i at (q_i - bbox_min) * bbox_scale - 1 (the tap
                 order and weights of F.grid_sample, align_corners=True);  mask = sum_i w_i;  x_skel = sum_i w_i q_i / max(mask, 1e-4)
  normals        g_a = T(v + h e_a) - T(v - h e_a);  n = -s / |s| with s = g / max_a |g_a|, zero where g is 0 or not finite;  T the
                 trilinear interpolant of the whole-grid field [Nz,Ny,Nx] at the grid-index coordinates (p - origin) / h, taps
                 outside the grid zero."""
import numpy as np


def _taps(c, dtype):
    """floor, lower and upper weight of the coordinates c (one axis), as the kernels form them: w1 = c - f, w0 = (f + 1) - c."""
    f = np.floor(c)
    return f, (f + dtype(1)) - c, c - f


def trilinear_zero(vol, gx, gy, gz, dtype=np.float64):
    """One channel vol [V,V,V] (z,y,x) at normalised coordinates [P] -> [P]; `trilinear_zero` of hos_trilinear.h."""
    V = vol.shape[-1]
    v = np.asarray(vol, dtype=np.float32).astype(dtype).reshape(-1)
    s = dtype(V - 1)
    ix, iy, iz = ((gx + dtype(1)) / dtype(2)) * s, ((gy + dtype(1)) / dtype(2)) * s, ((gz + dtype(1)) / dtype(2)) * s
    return _gather8(v, (V, V, V), ix, iy, iz, dtype)


def _gather8(flat, dims, cx, cy, cz, dtype):
    """sum over the 8 taps of flat[(z*Ny + y)*Nx + x] * (wx * wy * wz), dz outermost, dx innermost; taps outside dims contribute 0."""
    Nx, Ny, Nz = dims
    with np.errstate(invalid="ignore"):
        fx, wx0, wx1 = _taps(cx, dtype)
        fy, wy0, wy1 = _taps(cy, dtype)
        fz, wz0, wz1 = _taps(cz, dtype)
        sane = (fx >= -1) & (fx <= Nx) & (fy >= -1) & (fy <= Ny) & (fz >= -1) & (fz <= Nz)          # NaN / huge: every tap out of range
    x0, y0, z0 = (np.where(sane, f, -2).astype(np.int64) for f in (fx, fy, fz))
    out = np.zeros(cx.shape, dtype=dtype)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                x, y, z = x0 + dx, y0 + dy, z0 + dz
                ok = sane & (x >= 0) & (x < Nx) & (y >= 0) & (y < Ny) & (z >= 0) & (z < Nz)
                w = ((wx1 if dx else wx0) * (wy1 if dy else wy0)) * (wz1 if dz else wz0)
                lin = (np.clip(z, 0, Nz - 1) * Ny + np.clip(y, 0, Ny - 1)) * Nx + np.clip(x, 0, Nx - 1)
                with np.errstate(invalid="ignore"):
                    out = np.where(ok, out + flat[lin] * w, out)
    return out


def backward_lbs(pts, R, T, vol, bbox_min, bbox_scale, dtype=np.float64):
    """pts [P,3], R [K,3,3], T [K,3], vol [>=K,V,V,V], bbox_min / bbox_scale [3] -> (x_skel [P,3], mask [P])."""
    c = lambda a: np.asarray(a, dtype=np.float32).astype(dtype)
    p, R, T, bmin, bscale = c(pts), c(R), c(T), c(bbox_min), c(bbox_scale)
    K = R.shape[0]
    wsum = np.zeros(p.shape[0], dtype=dtype)
    acc = np.zeros((p.shape[0], 3), dtype=dtype)
    for i in range(K):
        q = np.stack([((R[i, a, 0] * p[:, 0] + R[i, a, 1] * p[:, 1]) + R[i, a, 2] * p[:, 2]) + T[i, a] for a in range(3)], 1)
        g = (q - bmin[None]) * bscale[None] - dtype(1)
        w = trilinear_zero(vol[i], g[:, 0], g[:, 1], g[:, 2], dtype)
        wsum = wsum + w
        acc = acc + w[:, None] * q
    den = np.maximum(wsum, dtype(1e-4))
    return acc / den[:, None], wsum


def trilinear_grid(field, origin, spacing, x, y, z, dtype=np.float64):
    """T(p) of the normals: field [Nz,Ny,Nx] at the positions (x, y, z) [P] -> [P]."""
    f = np.asarray(field, dtype=np.float32)
    Nz, Ny, Nx = f.shape
    o = np.asarray(origin, dtype=np.float32).astype(dtype)
    h = dtype(np.float32(spacing))
    return _gather8(f.astype(dtype).reshape(-1), (Nx, Ny, Nz), (x - o[0]) / h, (y - o[1]) / h, (z - o[2]) / h, dtype)


def vertex_normals(field, origin, spacing, vertices, dtype=np.float64):
    """normals [V,3] of the mesh vertices [V,3] (float32 values, as the march wrote them)."""
    v = np.asarray(vertices, dtype=np.float32).astype(dtype)
    h = dtype(np.float32(spacing))
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    T = lambda a, b, c: trilinear_grid(field, origin, spacing, a, b, c, dtype)
    gx = T(x + h, y, z) - T(x - h, y, z)
    gy = T(x, y + h, z) - T(x, y - h, z)
    gz = T(x, y, z + h) - T(x, y, z - h)
    with np.errstate(all="ignore"):
        m = np.maximum(np.maximum(np.abs(gx), np.abs(gy)), np.abs(gz))
        ok = (m > 0) & np.isfinite(gx) & np.isfinite(gy) & np.isfinite(gz)
        sx, sy, sz = gx / m, gy / m, gz / m                      # scaled first: the squares of a tiny gradient would underflow
        length = np.sqrt((sx * sx + sy * sy) + sz * sz)
        n = np.stack([(-sx) / length, (-sy) / length, (-sz) / length], 1)
    return np.where(ok[:, None], n, dtype(0)).astype(dtype)


def to_space(vertices, faces, normals, A):
    """`mesh.to_space` in float64: v' = L v + t; normals L n renormalised (zero stays zero); det L < 0 swaps two indices per face."""
    A = np.asarray(A, dtype=np.float64)
    L, t = A[:3, :3], A[:3, 3]
    v = np.asarray(vertices, dtype=np.float64) @ L.T + t
    f = np.asarray(faces)
    if np.linalg.det(L) < 0:
        f = f[:, [0, 2, 1]]
    n = None
    if normals is not None:
        n = np.asarray(normals, dtype=np.float64) @ L.T
        length = np.linalg.norm(n, axis=1, keepdims=True)
        n = np.where(length > 0, n / np.where(length > 0, length, 1.0), 0.0)
    return v, f, n
