"""What looking at a frame mesh again costs, measured on one MI355X (a record, not a benchmark of the project: bench.py is; there is
no pass threshold).  The mesh is the synthetic posed frame mesh of scripts/frame_mesh_cost.py -- the stage-3 `Network` on the
synthetic weights of the tests, a posed `synth.human_batch` frame, resolution 256, level = the median of the positive alphas (the
untrained field does not reach 0.5) -- seen in a 512 x 512 frame by a camera on the box's -z side that fits the box into the frame.

Device events around each of `ops.mesh_project`, `ops.raster_faces`, `ops.raster_resolve` (all six maps) and `ops.frame_fit` (the
mesh's maps against a copy shifted by a few pixels), median of --repeats after one warm-up; `mesh.rasterize` as a whole (its buffer
fills and the read-back of `dropped` included) next to them.  Also recorded: V, F, the covered pixels, the dropped triangles, and the
per-triangle pixel boxes the raster kernel loops over (clamped to the frame): the largest, the mean and the 99th percentile.  The
expectation to confirm or refute: the whole preview is small next to the 72 ms of `mesh.frame_field` at this resolution
(profiles/frame_mesh_cost.json).

Everything lands in --out (default profiles/raster_cost.json)."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_cost.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()

    import numpy as np
    import torch
    from hosnerf_amd import mesh, ops, synth
    from hosnerf_amd.eval import FRAME_KEYS
    from hosnerf_amd.human_nerf import Network, default_cfg
    dev = torch.device("cuda")
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    net = Network(default_cfg(d), stage=3)
    net.load_state_dict(synth.human_state_dict(777, 2), strict=True)
    net = net.to(dev)
    hb = synth.human_batch(8, seed=3, time=0.7, is_train=False, iter_val=1e7)
    pose = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in hb.items() if k in FRAME_KEYS}
    bmin, bmax = hb["dst_bbox_min_xyz"].numpy().astype(np.float64), hb["dst_bbox_max_xyz"].numpy().astype(np.float64)
    pose.update(time=0.7, is_train=False, frame_name="frame_070", dst_bbox={"min_xyz": bmin.astype(np.float32), "max_xyz": bmax.astype(np.float32)})

    field = mesh.frame_field(net, pose, resolution=args.resolution)
    a = field["alpha"]
    level = float(a[a > 0].median())
    vertices, colors, faces = ops.march_tets(a, level, field["origin"], field["spacing"], rgb=field["rgb"])
    normals = ops.mesh_vertex_normals(a, field["origin"], field["spacing"], vertices)
    m = {"vertices": vertices, "faces": faces, "colors": (255.0 * colors.clamp(0.0, 1.0)).to(torch.uint8), "normals": normals}
    V, F = int(vertices.shape[0]), int(faces.shape[0])

    H = W = args.size
    centre, extent = (bmin + bmax) / 2.0, float((bmax - bmin).max())
    dist = 2.5 * extent
    focal = 0.9 * W * (dist - extent / 2.0) / extent                    # the box's near face fills nine tenths of the frame
    K = np.array([[focal, 0.0, (W - 1) / 2.0], [0.0, focal, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    R, T = np.eye(3), np.array([0.0, 0.0, dist]) - centre
    E = np.concatenate([R, T[:, None]], 1)
    Kinv = np.linalg.inv(K)
    n = H * W
    names = ("project", "raster_faces", "resolve", "frame_fit", "rasterize_whole")
    times = {k: [] for k in names}

    def timed(key, fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        t1.synchronize()
        times[key].append(t0.elapsed_time(t1))
        return out

    out = {"face": torch.empty(n, dtype=torch.int32, device=dev), "depth": torch.empty(n, device=dev), "mask": torch.empty(n, dtype=torch.uint8, device=dev),
           "rgb": torch.empty(n, 3, device=dev), "normal": torch.empty(n, 3, device=dev), "shaded": torch.empty(n, 3, device=dev)}
    for rep in range(args.repeats + 1):
        zbuf = torch.full((n,), -1, dtype=torch.int64, device=dev)
        dropped = torch.zeros(1, dtype=torch.int32, device=dev)
        xy, z = timed("project", lambda: ops.mesh_project(vertices, K, R, T))
        timed("raster_faces", lambda: ops.raster_faces(xy, z, faces, 0, H, W, zbuf, dropped))
        timed("resolve", lambda: ops.raster_resolve(zbuf, xy, z, faces, 0, H, W, out, vertices=vertices, colors=m["colors"], normals=normals, Kinv=Kinv, R=R))
        alpha_b = torch.roll(out["mask"].view(H, W), (3, -2), (0, 1)).float().reshape(-1).contiguous()
        depth_b = torch.roll(out["depth"].view(H, W), (3, -2), (0, 1)).reshape(-1).contiguous()
        fit = timed("frame_fit", lambda: ops.frame_fit(out["mask"], out["depth"], alpha_b, depth_b, 0.5))
        whole = timed("rasterize_whole", lambda: mesh.rasterize(m, K, E, H, W))
    same = all(bool(torch.equal(whole[k], out[k])) for k in out)
    # the pixel boxes the raster kernel loops over: per usable triangle, clamped to the frame
    tri = xy.long()[faces.long()]                                        # [F,3,2]
    usable = (tri[:, :, 0] != -2 ** 31).all(1)
    lo, hi = tri.min(1).values, tri.max(1).values
    c0, c1 = ((lo[:, 0] + 255) >> 8).clamp_min(0), (hi[:, 0] >> 8).clamp_max(W - 1)
    r0, r1 = ((lo[:, 1] + 255) >> 8).clamp_min(0), (hi[:, 1] >> 8).clamp_max(H - 1)
    box = ((c1 - c0 + 1).clamp_min(0) * (r1 - r0 + 1).clamp_min(0))[usable].double()
    med = {k: statistics.median(v[1:]) for k, v in times.items()}        # the first round is the warm-up
    host = fit.cpu()
    res = {"workload": f"synthetic posed frame mesh (stage-3 Network on synthetic weights, posed synth.human_batch frame), resolution {args.resolution}, "
                       f"level {level:.6g} (median of the positive alphas), {H} x {W} frame, focal {focal:.1f}, 1 GPU, device events",
           "repeats": args.repeats, "V": V, "F": F, "covered_pixels": int(out["mask"].sum()), "dropped": int(dropped.item()),
           "triangle_pixel_box": {"max": float(box.max()) if F else 0.0, "mean": float(box.mean()) if F else 0.0,
                                  "p99": float(torch.quantile(box[:: max(1, box.numel() // 1000000)], 0.99)) if F else 0.0,
                                  "share_of_empty_boxes": float((box == 0).double().mean()) if F else 0.0},
           "median_ms": med, "min_ms": {k: min(v[1:]) for k, v in times.items()}, "max_ms": {k: max(v[1:]) for k, v in times.items()},
           "kernels_sum_ms": med["project"] + med["raster_faces"] + med["resolve"] + med["frame_fit"],
           "rasterize_whole_equals_the_separate_calls": same, "fit_counts": host[:3].tolist(),
           "frame_field_ms_for_scale": 72.0,
           "note": "rasterize_whole = mesh.rasterize of the same mesh: the three kernels plus the fill of the z-buffer and the read-back of `dropped`; "
                   "frame_field_ms_for_scale is mesh.frame_field at resolution 256 from profiles/frame_mesh_cost.json, not measured here"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
