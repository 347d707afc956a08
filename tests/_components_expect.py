"""The mesh components restated in numpy (no scipy): union-find labels, dense ids by ascending root, per-component counts and
float64 sums, the keep rule and the compaction -- what hos_components.hip, `ops.mesh_label` / `mesh_component_measures` /
`mesh_compact` and `mesh.components` / `drop_floaters` are judged by.  Also the fields and hand meshes the tests share, and a
synchronous simulation of the kernels' round (every read taken from the state at the start of the launch: the worst case for stale
loads), which must reach the union-find labels."""
import numpy as np

import _mesh_expect as mx


# ------------------------------------------------------------------------------------------ the restatement
def valid_faces(faces, V):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(axis=1)


def labels(faces, V):
    """(label int32 [V], invalid): label[v] = the smallest vertex id of v's connected component, by union-find over the valid faces."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = valid_faces(f, V)
    parent = list(range(V))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for a, b, c in f[ok].tolist():
        for u, w in ((a, b), (b, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)         # the smaller id stays the root
    return np.array([find(v) for v in range(V)], dtype=np.int32).reshape(V), int((~ok).sum())


def dense(label):
    """(component int32 [V], C): the rank of label[v] among the roots (label[r] == r) in ascending order."""
    label = np.asarray(label, dtype=np.int64)
    roots = np.flatnonzero(label == np.arange(label.shape[0]))
    return np.searchsorted(roots, label).astype(np.int32), int(roots.shape[0])


def face_terms(vertices, faces, ok):
    """(area, volume) terms float64 [F] of the vertices promoted to double (fp32 ones as a mesh on the device holds them; float64
    ones stay as they are), in the kernel's order of operations; 0 where not ok."""
    v = np.asarray(vertices).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F = f.shape[0]
    area, volume = np.zeros(F), np.zeros(F)
    if ok.any():
        a, b, c = (v[f[ok, k]] for k in range(3))
        u, w = b - a, c - a
        nx, ny, nz = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        area[ok] = np.sqrt((nx * nx + ny * ny) + nz * nz) / 2.0
        m0, m1, m2 = b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1], b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2], b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]
        volume[ok] = ((a[:, 0] * m0 + a[:, 1] * m1) + a[:, 2] * m2) / 6.0
    return area, volume


def measures(vertices, faces, component, C):
    """face_component int32 [F] (-1: invalid), n_vertices / n_faces int64 [C], area / volume float64 [C] (summed in face order), and
    the per-face terms (for the tests' error bound)."""
    V = np.asarray(component).shape[0]
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = valid_faces(f, V)
    fc = np.full(f.shape[0], -1, dtype=np.int32)
    fc[ok] = np.asarray(component)[f[ok, 0]]
    ta, tv = face_terms(vertices, f, ok)
    n_vertices = np.bincount(np.asarray(component, dtype=np.int64), minlength=C).astype(np.int64)
    n_faces = np.bincount(fc[ok].astype(np.int64), minlength=C).astype(np.int64)
    area, volume = np.zeros(C), np.zeros(C)
    np.add.at(area, fc[ok], ta[ok])
    np.add.at(volume, fc[ok], tv[ok])
    return {"face_component": fc, "n_vertices": n_vertices, "n_faces": n_faces, "area": area, "volume": volume, "terms": (ta, tv)}


def components(vertices, faces):
    V = np.asarray(vertices).reshape(-1, 3).shape[0]
    label, invalid = labels(faces, V)
    component, C = dense(label)
    return {"label": label, "component": component, "count": C, "invalid_faces": invalid, **measures(vertices, faces, component, C)}


def keep_rule(n_faces, area, min_area_ratio=0.0, min_faces=0):
    """uint8 [C]: component c is kept iff n_faces[c] >= min_faces and area[c] >= min_area_ratio * max(area)."""
    area = np.asarray(area, dtype=np.float64)
    if area.shape[0] == 0:
        return np.zeros(0, dtype=np.uint8)
    return ((np.asarray(n_faces) >= min_faces) & (area >= min_area_ratio * area.max())).astype(np.uint8)


def compact(keep, component, face_component, vertices, faces, colors=None, normals=None):
    """The sub-mesh of the kept components in the original relative order -> (vertices, faces int32, colors, normals)."""
    keep = np.asarray(keep).astype(bool)
    component, fc = np.asarray(component, dtype=np.int64), np.asarray(face_component, dtype=np.int64)
    kv = keep[component] if component.shape[0] else np.zeros(0, dtype=bool)
    new_id = np.cumsum(kv) - kv                           # the exclusive scan of keep[component[v]]
    kf = np.zeros(fc.shape[0], dtype=bool)
    kf[fc >= 0] = keep[fc[fc >= 0]]
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)[kf]
    pick = lambda a: None if a is None else np.asarray(a)[kv]
    return pick(vertices), new_id[f].astype(np.int32).reshape(-1, 3), pick(colors), pick(normals)


def simulate_rounds(faces, V, jumps=2, cap=None):
    """The kernels' rounds on the host, every launch reading the state at its start: hook (per face m = min of the three labels; each
    corner x with label l > m: label[x] and label[l] lowered to m), then the jump (label[v] := label[label[v]], `jumps` times, the
    carried value following the read chain).  -> (label, rounds), rounds counting the last one, which changes nothing."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[valid_faces(f, V)]
    label = np.arange(V, dtype=np.int64)
    cap = V + 2 if cap is None else cap
    rounds = 0
    while True:
        assert rounds < cap, "no fixed point within V + 2 rounds"
        before = label.copy()
        if f.shape[0]:
            l = before[f]                                  # [F,3]
            m = np.repeat(l.min(axis=1), 3)
            x, lx = f.reshape(-1), l.reshape(-1)
            low = lx > m
            np.minimum.at(label, x[low], m[low])
            np.minimum.at(label, lx[low], m[low])
        start = label.copy()
        l = start.copy()
        for _ in range(jumps):
            l = np.minimum(l, start[l])
        label = np.minimum(label, l)
        rounds += 1
        if np.array_equal(label, before):
            return label.astype(np.int32), rounds


# ------------------------------------------------------------------------------------------ the meshes the tests share
def _ball(P, centre, radius):
    return radius - np.linalg.norm(P - np.asarray(centre, dtype=np.float64), axis=-1)


def field_two_spheres(P):
    return np.maximum(_ball(P, (.27, .5, .5), 0.22), _ball(P, (.77, .5, .5), 0.16))


def field_torus(P):
    d = P - 0.5
    return 0.12 - np.sqrt((np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2) - 0.3) ** 2 + d[..., 2] ** 2)


def field_shell(P):
    r = np.linalg.norm(P - 0.5, axis=-1)
    return np.minimum(0.42 - r, r - 0.2)


FLOATER_BALLS = (((.5, .5, .5), 0.30), ((.12, .12, .12), 0.08), ((.88, .12, .15), 0.07), ((.13, .87, .85), 0.09), ((.86, .88, .88), 0.06),
                 ((.5, .5, .93), 0.05))


def field_floaters(P):
    return np.max([_ball(P, c, r) for c, r in FLOATER_BALLS], axis=0)


# name: (field, n, V, F, components) -- the figures of the issue, checked by tests/test_components_cpu.py
MARCHED = {"two_spheres": (field_two_spheres, 12, 568, 1128, 2), "torus": (field_torus, 12, 928, 1856, 1),
           "shell": (field_shell, 12, 1744, 3480, 2), "floaters": (field_floaters, 16, 1572, 3120, 6)}
FLOATER_FACES = (144, 116, 2520, 228, 88, 24)                         # by ascending root
FLOATER_AREA_RATIO = (0.0595, 0.0418, 1.0, 0.0791, 0.0273, 0.0182)
# (min_area_ratio, min_faces) -> components kept; every threshold at least 15 % away from any ratio
KEEP_SETS = (((0.05, 0), 3), ((1.0, 0), 1), ((0.0, 100), 4))

_marched = {}


def marched(name):
    """(vertices float32 [V,3], faces int32 [F,3], grid) of MARCHED[name], marched once by the marching-tetrahedra restatement at
    level 0; the vertices are rounded to fp32 as a mesh on the device holds them."""
    if name not in _marched:
        field, n = MARCHED[name][:2]
        o, h, dims, P = mx.unit_box_grid(n)
        v, _, f = mx.march(field(P), 0.0, o, h)
        _marched[name] = (np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32), (o, h, dims))
    return _marched[name][:2]


def permuted(vertices, faces, seed=1):
    """The same mesh with the vertex ids permuted: vertex v becomes p[v]."""
    V = vertices.shape[0]
    p = np.random.default_rng(seed).permutation(V)
    out = np.empty_like(vertices)
    out[p] = vertices
    f = np.asarray(faces, dtype=np.int64)
    ok = valid_faces(f, V)
    g = f.copy()
    g[ok] = p[f[ok]]
    return out, g.astype(np.int32)


def shuffled_faces(faces, seed=1):
    return np.ascontiguousarray(np.asarray(faces)[np.random.default_rng(seed).permutation(np.asarray(faces).shape[0])])


def strip(n, numbering="order", seed=1):
    """A strip of n triangles (i, i+1, i+2) over n + 2 vertices on a zig-zag line, the vertex ids in order, reversed or permuted."""
    V = n + 2
    i = np.arange(V)
    v = np.stack([0.5 * i, (i % 2).astype(np.float64), 0.01 * i], -1).astype(np.float32)
    f = np.stack([i[:-2], i[1:-1], i[2:]], -1).astype(np.int32)
    if numbering == "reversed":
        return v[::-1].copy(), (V - 1 - f).astype(np.int32)
    if numbering == "permuted":
        return permuted(v, f, seed)
    assert numbering == "order"
    return v, f


def hand_cases():
    """name -> (vertices float32 [V,3], faces int32 [F,3]): the small cases written out by hand."""
    rng = np.random.default_rng(5)
    pts = lambda n: rng.random((n, 3)).astype(np.float32)
    f = lambda *rows: np.array(rows, dtype=np.int32).reshape(-1, 3)
    return {
        "no_faces": (pts(5), f()),
        "no_vertices": (pts(0), f()),
        "unreferenced_vertex": (pts(7), f((0, 1, 2), (2, 4, 5), (6, 5, 4))),            # vertex 3 stands alone
        "repeated_corner": (pts(6), f((1, 1, 4), (0, 2, 3), (5, 5, 5))),                # (a,a,b) connects a and b
        "duplicated_face": (pts(6), f((3, 4, 5), (3, 4, 5), (0, 1, 2), (5, 4, 3))),
        "out_of_range": (pts(8), f((0, 1, 2), (2, 3, 8), (4, 5, 6), (6, -1, 7), (7, 6, 5))),      # a corner >= V, a corner < 0
    }
