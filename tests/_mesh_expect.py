"""Marching tetrahedra on the Kuhn split, restated in vectorised numpy: what `ops.march_tets` (hos_mesh.hip) must produce, with the
same tables written out.  Used by test_mesh_cpu.py (the restatement's own properties) and test_gpu_mesh.py (the kernels against it).

Rules (include/hosrender.h, "Canonical mesh"): field [Nz,Ny,Nx], vertex (ix,iy,iz) at origin + float32(i) * h, inside iff f > level
(NaN and == level outside).  Cell c0 is cut into the tetrahedra {c0, c0+e_a, c0+e_a+e_b, c7}, one per permutation (a,b,c) of the
axes in lexicographic order; every tetrahedron edge runs from a lower corner v to v + d, d in 1..7 a corner bit mask (dx + 2dy +
4dz), owned by v, family d - 1.  Mesh vertices ascend by (owner, family); faces by (cell, tetrahedron, triangle)."""
import itertools

import numpy as np

PERMS = list(itertools.permutations(range(3)))                     # xyz, xzy, yxz, yzx, zxy, zyx
TET_CORNERS = [(0, 1 << a, (1 << a) | (1 << b), 7) for a, b, c in PERMS]      # corner bits of the tetrahedron's vertices 0..3
TET_EDGES = [(0, 1), (1, 2), (2, 3), (0, 2), (1, 3), (0, 3)]      # tetrahedron edges 0..5 as (lower, upper) tetrahedron vertex
TET_ODD = [0, 1, 1, 0, 0, 1]                                      # parity of the permutation: an odd tetrahedron is left-handed
# Triangles per inside mask (bit i = tetrahedron vertex i inside), as tetrahedron edges, for a RIGHT-handed tetrahedron; an odd one
# swaps the last two.  One corner i inside (or outside): the edges from i to the other three in ascending order, turned so that the
# normal points away from the inside.  Two inside (i < j; k < l outside): the quad (ik, il, jl, jk), cut along ik-jl.
TRI = [[], [(0, 3, 5)], [(0, 4, 1)], [(3, 5, 4), (3, 4, 1)], [(3, 1, 2)], [(0, 2, 5), (0, 1, 2)], [(0, 4, 2), (0, 2, 3)], [(5, 4, 2)],
       [(5, 2, 4)], [(0, 3, 2), (0, 2, 4)], [(0, 2, 1), (0, 5, 2)], [(3, 2, 1)], [(3, 1, 4), (3, 4, 5)], [(0, 1, 4)], [(0, 5, 3)], []]


def _off(d):
    return d & 1, (d >> 1) & 1, (d >> 2) & 1


def march(field, level, origin, spacing, rgb=None, dtype=np.float64):
    """(vertices [V,3] dtype, colors [V,3] dtype or None, faces int32 [F,3]).  The inside test and the ordering never depend on
    `dtype`; t and the positions are evaluated in it (float32: operation by operation as the kernel; float64: the yardstick)."""
    f32 = np.asarray(field, dtype=np.float32)
    Nz, Ny, Nx = f32.shape
    N = Nx * Ny * Nz
    level32 = np.float32(level)
    with np.errstate(invalid="ignore"):
        inside = f32 > level32
    f = f32.astype(dtype)
    lin = np.arange(N, dtype=np.int64).reshape(Nz, Ny, Nx)
    keys, ts, ds = [], [], []
    for d in range(1, 8):
        dx, dy, dz = _off(d)
        a = (slice(0, Nz - dz), slice(0, Ny - dy), slice(0, Nx - dx))
        b = (slice(dz, Nz), slice(dy, Ny), slice(dx, Nx))
        cross = inside[a] != inside[b]
        fv, fw = f[a][cross], f[b][cross]
        with np.errstate(all="ignore"):
            t = (dtype(level32) - fv) / (fw - fv)
        t = np.where(np.isfinite(fv) & np.isfinite(fw), t, dtype(0.5))
        with np.errstate(invalid="ignore"):
            t = np.where((t >= 0) & (t <= 1), t, dtype(0.5))
        keys.append(lin[a][cross] * 7 + (d - 1))
        ts.append(t)
        ds.append(np.full(t.shape, d, dtype=np.int64))
    keys, ts, ds = np.concatenate(keys), np.concatenate(ts), np.concatenate(ds)
    order = np.argsort(keys, kind="stable")
    keys, ts, ds = keys[order], ts[order].astype(dtype), ds[order]
    V = keys.shape[0]
    edge_id = np.full(7 * N, -1, dtype=np.int64)
    edge_id[keys] = np.arange(V)
    owner = keys // 7
    idx = np.stack([owner % Nx, (owner // Nx) % Ny, owner // (Nx * Ny)], 1)
    h = dtype(np.float32(spacing))
    o = np.asarray(origin, dtype=np.float32).astype(dtype)
    dvec = np.stack([ds & 1, (ds >> 1) & 1, (ds >> 2) & 1], 1).astype(dtype)
    verts = (o[None, :] + idx.astype(np.float32).astype(dtype) * h) + ts[:, None] * (dvec * h)
    colors = None
    if rgb is not None:
        c = np.asarray(rgb, dtype=np.float32).reshape(N, 3).astype(dtype)
        step = (ds & 1) + ((ds >> 1) & 1) * Nx + ((ds >> 2) & 1) * Nx * Ny
        cv, cw = c[owner], c[owner + step]
        colors = cv + ts[:, None] * (cw - cv)
    # faces
    cell = lin[:Nz - 1, :Ny - 1, :Nx - 1].reshape(-1)
    corner_lin = {cb: cell + (cb & 1) + ((cb >> 1) & 1) * Nx + ((cb >> 2) & 1) * Nx * Ny for cb in range(8)}
    ins_flat = inside.reshape(-1)
    chunks = []
    for tet in range(6):
        cb = TET_CORNERS[tet]
        mask = sum(ins_flat[corner_lin[cb[i]]].astype(np.int64) << i for i in range(4))
        eids = []
        for lo, up in TET_EDGES:
            d = cb[up] - cb[lo]                                      # the corner bits of `up` contain those of `lo`
            eids.append(edge_id[corner_lin[cb[lo]] * 7 + (d - 1)])
        eids = np.stack(eids, 1)
        for m in range(1, 15):
            sel = np.nonzero(mask == m)[0]
            if sel.size == 0:
                continue
            for k, tri in enumerate(TRI[m]):
                tri = (tri[0], tri[2], tri[1]) if TET_ODD[tet] else tri
                fc = eids[sel][:, list(tri)]
                chunks.append(np.concatenate([cell[sel, None], np.full((sel.size, 1), tet), np.full((sel.size, 1), k), fc], 1))
    if chunks:
        allf = np.concatenate(chunks, 0)
        allf = allf[np.lexsort((allf[:, 2], allf[:, 1], allf[:, 0]))]
        faces = allf[:, 3:].astype(np.int32)
    else:
        faces = np.zeros((0, 3), dtype=np.int32)
    assert faces.size == 0 or faces.min() >= 0
    return verts, colors, faces


def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)


def is_closed_oriented_manifold(faces, n_vertices):
    """Every directed edge occurs exactly once and its reverse exactly once; every vertex is used."""
    e = directed_edges(faces)
    if e.shape[0] == 0:
        return n_vertices == 0
    key = e[:, 0] * (n_vertices + 1) + e[:, 1]
    rev = e[:, 1] * (n_vertices + 1) + e[:, 0]
    uk, cnt = np.unique(key, return_counts=True)
    return bool((cnt == 1).all() and np.array_equal(uk, np.unique(rev)) and np.unique(e).size == n_vertices)


def euler_characteristic(faces, n_vertices):
    e = directed_edges(faces)
    und = np.unique(np.sort(e, 1), axis=0).shape[0]
    return int(n_vertices - und + np.asarray(faces).shape[0])


def signed_volume(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    if f.shape[0] == 0:
        return 0.0
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def area(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    if f.shape[0] == 0:
        return 0.0
    return float(np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum() / 2.0)


def unit_box_grid(n):
    """The unit box with h = 1/n and one vertex layer outside: (origin [3] float32, h float32, dims (Nx,Ny,Nz), points [Nz,Ny,Nx,3] float64)."""
    h = np.float32(1.0 / n)
    N = n + 3
    o = np.full(3, -h, dtype=np.float32)
    ax = o[0].astype(np.float64) + np.arange(N, dtype=np.float32).astype(np.float64) * np.float64(h)
    Z, Y, X = np.meshgrid(ax, ax, ax, indexing="ij")
    return o, h, (N, N, N), np.stack([X, Y, Z], -1)
