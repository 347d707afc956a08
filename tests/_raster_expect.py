"""The mesh rasteriser (hos_raster.hip, include/hosrender.h "Mesh rasteriser") restated in numpy: what `ops.mesh_project`,
`ops.raster_faces`, `ops.raster_resolve` and `ops.frame_fit` must produce.  Used by test_raster_cpu.py (the restatement's own
properties, no GPU) and test_gpu_raster.py (the kernels against it).

Every function takes a `dtype`: float32 evaluates operation by operation as the kernels do (same association, no fused multiply-add),
float64 is the yardstick.  Coverage is integer arithmetic and never depends on it.

Camera: X_cam = R x + T, u = (K X_cam).x / X_cam.z, v = (K X_cam).y / X_cam.z, pixel (col,row) sampled at (u,v) = (col,row), depth =
X_cam.z; screen positions in 1/256-pixel fixed point."""
import numpy as np

from tests._mesh_expect import march, unit_box_grid          # noqa: F401  (the analytic sphere and the marcher: re-exported)

SENTINEL = -2 ** 31            # xy[:,0] of a vertex no triangle may use
GUARD = 16384.0                # |u|, |v| <= 2^14 pixels


def project(vertices, K, R, T, dtype, z_near=1e-6):
    """(xy int64 [V,2], z dtype [V], uv dtype [V,2]).  K, R, T are rounded to fp32 first, as the kernel receives them."""
    v = np.asarray(vertices, dtype=np.float32).astype(dtype).reshape(-1, 3)
    K = np.asarray(K, dtype=np.float64).astype(np.float32).astype(dtype).reshape(3, 3)
    R = np.asarray(R, dtype=np.float64).astype(np.float32).astype(dtype).reshape(3, 3)
    T = np.asarray(T, dtype=np.float64).astype(np.float32).astype(dtype).reshape(3)
    x, y, w = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        q = [((R[a, 0] * x + R[a, 1] * y) + R[a, 2] * w) + T[a] for a in range(3)]
        px = (K[0, 0] * q[0] + K[0, 1] * q[1]) + K[0, 2] * q[2]
        py = (K[1, 0] * q[0] + K[1, 1] * q[1]) + K[1, 2] * q[2]
        u, vv = px / q[2], py / q[2]
        ok = (q[2] > dtype(np.float32(z_near))) & np.isfinite(q[2]) & (np.abs(u) <= GUARD) & (np.abs(vv) <= GUARD)
        xi = np.where(ok, np.rint(dtype(256.0) * np.where(ok, u, 0)), SENTINEL).astype(np.int64)
        yi = np.where(ok, np.rint(dtype(256.0) * np.where(ok, vv, 0)), 0).astype(np.int64)
    return np.stack([xi, yi], 1), q[2].astype(dtype), np.stack([u, vv], 1)


def _setup(xy, faces, f, V):
    """The triangle after sign normalisation, or None where it is dropped: (ids [3], x [3], y [3], area2 > 0, bias [3]) in Python ints."""
    ids = [int(i) for i in faces[f]]
    if any(i < 0 or i >= V for i in ids):
        return None
    x = [int(xy[i, 0]) for i in ids]
    y = [int(xy[i, 1]) for i in ids]
    if SENTINEL in x:
        return None
    a2 = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    if a2 == 0:
        return None
    if a2 < 0:
        ids, x, y, a2 = [ids[0], ids[2], ids[1]], [x[0], x[2], x[1]], [y[0], y[2], y[1]], -a2
    bias = []
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        dx, dy = x[b] - x[a], y[b] - y[a]
        bias.append(0 if (dy < 0 or (dy == 0 and dx > 0)) else -1)           # a left edge, or a top edge
    return ids, x, y, a2, bias


def _cover(tri, H, W):
    """(rows, cols, e [3, n] int64) of the pixel centres the set-up triangle covers: its box clamped to the frame, top-left rule."""
    ids, x, y, a2, bias = tri
    c0, c1 = max(-((-min(x)) // 256), 0), min(max(x) // 256, W - 1)
    r0, r1 = max(-((-min(y)) // 256), 0), min(max(y) // 256, H - 1)
    if c1 < c0 or r1 < r0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, np.zeros((3, 0), dtype=np.int64)
    rows, cols = np.meshgrid(np.arange(r0, r1 + 1, dtype=np.int64), np.arange(c0, c1 + 1, dtype=np.int64), indexing="ij")
    rows, cols = rows.reshape(-1), cols.reshape(-1)
    px, py = cols * 256, rows * 256
    e = []
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        e.append((x[b] - x[a]) * (py - y[a]) - (y[b] - y[a]) * (px - x[a]))
    e = np.stack(e, 0)
    inside = (e[0] + bias[0] >= 0) & (e[1] + bias[1] >= 0) & (e[2] + bias[2] >= 0)
    return rows[inside], cols[inside], e[:, inside]


def coverage(xy_int, faces, H, W):
    """(per face one int64 array of the covered pixel indices row * W + col, empty for a dropped face; the number of dropped
    faces).  Integer arithmetic, top-left rule, either orientation."""
    xy = np.asarray(xy_int, dtype=np.int64)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    out, dropped = [], 0
    for f in range(faces.shape[0]):
        tri = _setup(xy, faces, f, xy.shape[0])
        if tri is None:
            dropped += 1
            out.append(np.zeros(0, dtype=np.int64))
            continue
        rows, cols, _ = _cover(tri, H, W)
        out.append(rows * W + cols)
    return out, dropped


def candidates(xy_int, z, faces, H, W, dtype, face_base=0):
    """Every (pixel, face) pair the coverage test accepts: dict of arrays `pix`, `face` (id = face_base + f), `depth` (dtype),
    `w` [n,3] (b_i / z_i in dtype), `ids` [n,3] (the vertex ids in the normalised order); and `dropped`."""
    xy = np.asarray(xy_int, dtype=np.int64)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    zz = np.asarray(z, dtype=np.float32).astype(dtype)
    pix, fid, depth, ws, vid, dropped = [], [], [], [], [], 0
    for f in range(faces.shape[0]):
        tri = _setup(xy, faces, f, xy.shape[0])
        if tri is None:
            dropped += 1
            continue
        rows, cols, e = _cover(tri, H, W)
        if rows.size == 0:
            continue
        ids, _, _, a2, _ = tri
        iz = [dtype(1.0) / zz[i] for i in ids]
        area = dtype(np.int64(a2))
        w = np.stack([(e[k].astype(dtype) / area) * iz[k] for k in range(3)], 1)
        with np.errstate(divide="ignore"):
            d = dtype(1.0) / ((w[:, 0] + w[:, 1]) + w[:, 2])
        pix.append(rows * W + cols)
        fid.append(np.full(rows.size, face_base + f, dtype=np.int64))
        depth.append(d.astype(dtype))
        ws.append(w.astype(dtype))
        vid.append(np.tile(np.asarray(ids, dtype=np.int64), (rows.size, 1)))
    cat = lambda parts, shape, dt: np.concatenate(parts, 0) if parts else np.zeros(shape, dtype=dt)
    return {"pix": cat(pix, (0,), np.int64), "face": cat(fid, (0,), np.int64), "depth": cat(depth, (0,), dtype), "w": cat(ws, (0, 3), dtype),
            "ids": cat(vid, (0, 3), np.int64), "dropped": dropped}


def zbuffer(cands, n_pixels):
    """The key minimum: per pixel the candidate of least depth, at equal depth of least face id -> the indices into `cands` of the
    winners, one per covered pixel, ordered by pixel."""
    order = np.lexsort((cands["face"], cands["depth"], cands["pix"]))
    p = cands["pix"][order]
    first = np.ones(p.shape[0], dtype=bool)
    first[1:] = p[1:] != p[:-1]
    return order[first]


def merge(*cands):
    """The candidates of several meshes in one buffer."""
    keys = ("pix", "face", "depth", "w", "ids")
    out = {k: np.concatenate([c[k] for c in cands], 0) for k in keys}
    out["dropped"] = sum(c["dropped"] for c in cands)
    return out


def resolve(cands, winners, H, W, dtype, vertices=None, faces=None, face_base=0, colors=None, normals=None, Kinv=None, R=None,
            bgcolor=(255.0, 255.0, 255.0)):
    """The maps of one mesh from the winners of its candidates: `face` int32 (-1 empty), `depth`, `mask` uint8, `rgb`, `normal`,
    `shaded` (dtype; [H*W] / [H*W,3])."""
    n = H * W
    bg = (np.asarray(bgcolor, dtype=np.float64) / 255.0).astype(np.float32).astype(dtype)
    face = np.full(n, -1, dtype=np.int32)
    depth = np.zeros(n, dtype=dtype)
    mask = np.zeros(n, dtype=np.uint8)
    rgb = np.tile(bg, (n, 1))
    normal = np.zeros((n, 3), dtype=dtype)
    shaded = np.tile(bg, (n, 1))
    p = cands["pix"][winners]
    d = cands["depth"][winners].astype(dtype)
    w = cands["w"][winners].astype(dtype)
    ids = cands["ids"][winners]
    face[p] = cands["face"][winners]
    depth[p] = d
    mask[p] = 1
    interp = lambda a: ((w[:, 0:1] * a[ids[:, 0]] + w[:, 1:2] * a[ids[:, 1]]) + w[:, 2:3] * a[ids[:, 2]]) * d[:, None]
    colour = np.ones((p.shape[0], 3), dtype=dtype)
    if colors is not None:
        colour = interp(np.asarray(colors, dtype=np.uint8).astype(dtype)) / dtype(255.0)
    rgb[p] = colour
    if normals is not None:
        nrm = interp(np.asarray(normals, dtype=np.float32).astype(dtype))
    else:
        v = np.asarray(vertices, dtype=np.float32).astype(dtype)
        fc = np.asarray(faces, dtype=np.int64).reshape(-1, 3)[cands["face"][winners] - face_base]
        a, b = v[fc[:, 1]] - v[fc[:, 0]], v[fc[:, 2]] - v[fc[:, 0]]
        nrm = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    with np.errstate(all="ignore"):
        m = np.abs(nrm).max(1)
        ok = (m > 0) & np.isfinite(m)
        s = nrm / np.where(ok, m, 1)[:, None]
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        nrm = np.where(ok[:, None], s / np.where(ok, length, 1)[:, None], 0).astype(dtype)
    normal[p] = nrm
    if Kinv is not None and R is not None:
        Ki = np.asarray(Kinv, dtype=np.float64).astype(np.float32).astype(dtype).reshape(3, 3)
        Rm = np.asarray(R, dtype=np.float64).astype(np.float32).astype(dtype).reshape(3, 3)
        col, row = (p % W).astype(dtype), (p // W).astype(dtype)
        pc = [(col * Ki[a, 0] + row * Ki[a, 1]) + Ki[a, 2] for a in range(3)]
        dr = [(pc[0] * Rm[0, b] + pc[1] * Rm[1, b]) + pc[2] * Rm[2, b] for b in range(3)]
        dl = np.sqrt((dr[0] * dr[0] + dr[1] * dr[1]) + dr[2] * dr[2])
        nd = ((nrm[:, 0] * dr[0] + nrm[:, 1] * dr[1]) + nrm[:, 2] * dr[2]) / dl
        shade = dtype(np.float32(0.3)) + dtype(np.float32(0.7)) * np.abs(nd)
        shaded[p] = colour * shade[:, None]
    return {"face": face, "depth": depth, "mask": mask, "rgb": rgb.astype(dtype), "normal": normal, "shaded": shaded.astype(dtype)}


def rasterize(vertices, faces, K, R, T, H, W, dtype, colors=None, normals=None, bgcolor=(255.0, 255.0, 255.0)):
    """project -> candidates -> zbuffer -> resolve of one mesh; also returns `dropped`, `xy`, `z`."""
    xy, z, _ = project(vertices, K, R, T, dtype)
    c = candidates(xy, z, faces, H, W, dtype)
    out = resolve(c, zbuffer(c, H * W), H, W, dtype, vertices=vertices, faces=faces, colors=colors, normals=normals,
                  Kinv=np.linalg.inv(np.asarray(K, dtype=np.float64)), R=R, bgcolor=bgcolor)
    out.update(dropped=c["dropped"], xy=xy, z=z)
    return out


def fit(mask_a, depth_a, alpha_b, depth_b, tau=0.5):
    """(counts int [3] = |A|, |B|, |A and B|; sums float64 [4] = sum |dz|, sum dz, sum dz^2, max |dz| over A and B), dz = depth_a -
    depth_b in float64 of the fp32 inputs; the sums are zero without depths."""
    a = np.asarray(mask_a).reshape(-1) != 0
    b = np.asarray(alpha_b, dtype=np.float32).reshape(-1) > np.float32(tau)
    both = a & b
    counts = [int(a.sum()), int(b.sum()), int(both.sum())]
    sums = [0.0, 0.0, 0.0, 0.0]
    if depth_a is not None and depth_b is not None and counts[2] > 0:
        dz = np.asarray(depth_a, dtype=np.float32).astype(np.float64).reshape(-1)[both] - np.asarray(depth_b, dtype=np.float32).astype(np.float64).reshape(-1)[both]
        sums = [float(np.abs(dz).sum()), float(dz.sum()), float((dz * dz).sum()), float(np.abs(dz).max())]
    return counts, sums


def fit_figures(counts, sums):
    """`mesh.fit`'s figures from the counts and sums."""
    a, b, ab = counts
    union = a + b - ab
    k = max(ab, 1)
    return {"iou": 1.0 if union == 0 else ab / union, "area_mesh": float(a), "area_ref": float(b), "depth_mae": sums[0] / k,
            "depth_bias": sums[1] / k, "depth_rmse": float(np.sqrt(sums[2] / k)), "depth_max": sums[3]}


# ------------------------------------------------------------------------------------------ the analytic sphere
SPHERE_C, SPHERE_R = (0.5, 0.5, 0.5), 0.3


def sphere_mesh(n, dtype=np.float32):
    """The sphere |x - c| = r inside the unit box, marched at resolution n from the field f = r - |x - c| at level 0 (`march`):
    (vertices dtype [V,3], faces int32 [F,3], normals float32 [V,3] analytic, colors uint8 [V,3] a smooth pattern)."""
    o, h, dims, pts = unit_box_grid(n)
    f = SPHERE_R - np.sqrt(((pts - np.asarray(SPHERE_C)) ** 2).sum(-1))
    v, _, faces = march(f.astype(np.float32), 0.0, o, h, dtype=dtype)
    nrm = v.astype(np.float64) - np.asarray(SPHERE_C)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    colors = np.clip(127.5 + 127.5 * nrm, 0, 255).astype(np.uint8)
    return v, faces, nrm.astype(np.float32), colors


def sphere_camera(H, W, distance=1.6, focal_scale=1.1):
    """A perspective camera looking at the sphere from an oblique direction: (K [3,3], R [3,3], T [3]) float64, X_cam = R x + T."""
    c = np.asarray(SPHERE_C)
    eye = c + distance * np.array([0.35, -0.25, -0.9]) / np.linalg.norm([0.35, -0.25, -0.9])
    fwd = (c - eye) / np.linalg.norm(c - eye)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd], 0)
    T = -R @ eye
    f = focal_scale * max(H, W)
    K = np.array([[f, 0.0, (W - 1) / 2.0 + 0.25], [0.0, f, (H - 1) / 2.0 - 0.125], [0.0, 0.0, 1.0]])
    return K, R, T


def sphere_truth(K, R, T, H, W):
    """Analytic maps of the sphere through the camera: (hit bool [H*W], depth float64 [H*W] = camera z of the first intersection,
    facing float64 [H*W] = |n . d| of the unit ray direction with the sphere's normal there)."""
    Kinv = np.linalg.inv(K)
    rows, cols = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pc = np.stack([cols.reshape(-1), rows.reshape(-1), np.ones(H * W)], 1) @ Kinv.T          # camera-space direction, z = 1
    d = pc @ R                                                                              # R^T pc, per row
    o = -R.T @ T
    oc = o - np.asarray(SPHERE_C)
    a, b, c = (d * d).sum(1), 2.0 * (d @ oc), oc @ oc - SPHERE_R ** 2
    disc = b * b - 4 * a * c
    hit = disc > 0
    t = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0))) / (2 * a), 0.0)                # d has camera z = 1: t IS the depth
    x = o + t[:, None] * d
    nrm = (x - np.asarray(SPHERE_C)) / SPHERE_R
    facing = np.abs((nrm * d).sum(1)) / np.sqrt(a)
    return hit, t, np.where(hit, facing, 0.0)
