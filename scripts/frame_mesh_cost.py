"""What the frame mesh costs at resolution 256, measured on one MI355X (a record, not a benchmark of the project: bench.py is; there
is no pass threshold).  The network is the stage-3 `Network` on the synthetic weights of the tests, the frame a posed
`synth.human_batch` item (its pose, its `dst_bbox`); the untrained field does not reach 0.5 at this spacing, so the level is the
median of the positive alphas (recorded).

Device events around each phase of `mesh.extract_frame(normals=True)`, --repeats times after one warm-up of every shape: the frame
prologue, warp (`ops.grid_warp` over the chunks), the non-rigid chain (`Network._nonrigid_fwd`), the canonical MLP
(`Network._canonical_fwd`), alpha (`ops.grid_alpha_masked` + `mesh.clip_to_box`), the march (`ops.march_tets`, its read-back included) and the normals
(`ops.mesh_vertex_normals`).  The yardstick, in the same process: `mesh.canonical_field` as a whole on a grid of the SAME vertex count
(the canonical constants with the frame's box put in the place of the canonical one, which changes where the points lie and nothing
about the work), next to `mesh.frame_field` as a whole.  The expectation was "canonical field + one non-rigid chain + a warp of
the size of `human_sample_warp` at that row count"; the JSON says what was found.

Everything lands in --out (default profiles/frame_mesh_cost.json)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_mesh_cost.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=1 << 18)
    args = ap.parse_args()

    import torch
    from hosnerf_amd import formats, mesh, ops, synth, tpose
    from hosnerf_amd.eval import FRAME_KEYS, evaluating
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
    pose.update(time=0.7, is_train=False, frame_name="frame_070",
                dst_bbox={"min_xyz": hb["dst_bbox_min_xyz"].numpy(), "max_xyz": hb["dst_bbox_max_xyz"].numpy()})
    joints = synth.tpose_joints()
    turn = tpose.TposeTurn(joints, formats.skeleton_bbox(joints, float(net.cfg.bbox_offset)), 32, dev)
    same_count = dict(turn.const)                                 # the yardstick's grid: the frame's box in the canonical field's place
    same_count["cnl_bbox_min_xyz"], same_count["cnl_bbox_max_xyz"] = hb["dst_bbox_min_xyz"].to(dev), hb["dst_bbox_max_xyz"].to(dev)

    field = mesh.frame_field(net, pose, resolution=args.resolution, chunk=args.chunk)
    a = field["alpha"]
    level = float(a[a > 0].median())
    origin, h, dims = field["origin"], field["spacing"], field["dims"]
    Nx, Ny, Nz = dims
    N = Nx * Ny * Nz
    rows = min(args.chunk, N)
    firsts = [min(c0, N - rows) for c0 in range(0, N, rows)]
    bmin, bscale = pose["cnl_bbox_min_xyz"].contiguous(), pose["cnl_bbox_scale_xyz"].contiguous()
    K = int(net.cfg.total_bones)
    per_frame = {k: pose[k] for k in FRAME_KEYS if k in pose}
    alpha, rgb = torch.empty_like(field["alpha"]), torch.empty_like(field["rgb"])
    names = ("prologue", "warp", "nonrigid_chain", "canonical_mlp", "alpha", "march", "normals", "frame_field_whole", "canonical_field_whole")
    times = {k: [] for k in names}

    def timed(key, fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        t1.synchronize()
        times[key].append(t0.elapsed_time(t1))
        return out

    with evaluating(net):
        for rep in range(args.repeats + 1):
            pro = timed("prologue", lambda: net.frame_prologue(**per_frame))
            warped = timed("warp", lambda: [ops.grid_warp(pro["R_b"], pro["T_b"], pro["vol"], bmin, bscale, origin, h, dims, f0, rows, K=K) for f0 in firsts])
            cnls = timed("nonrigid_chain", lambda: [net._nonrigid_fwd(net._nr, x, pro["cond"], pro["band_w"], save=False)[0] for x, _ in warped])
            raws = timed("canonical_mlp", lambda: [net._canonical_fwd(c, pro["state"], save=False)[0] for c in cnls])
            timed("alpha", lambda: ([ops.grid_alpha_masked(r, m, origin, h, dims, f0, alpha, rgb) for r, (_, m), f0 in zip(raws, warped, firsts)],
                                    mesh.clip_to_box(alpha, origin, h, dims, pose["dst_bbox"]["max_xyz"])))
            del warped, cnls, raws
            vertices, colors, faces = timed("march", lambda: ops.march_tets(alpha, level, origin, h, rgb=rgb))
            normals = timed("normals", lambda: ops.mesh_vertex_normals(alpha, origin, h, vertices))
    for rep in range(args.repeats + 1):
        whole = timed("frame_field_whole", lambda: mesh.frame_field(net, pose, resolution=args.resolution, chunk=args.chunk))
        yard = timed("canonical_field_whole", lambda: mesh.canonical_field(net, same_count, 0.7, resolution=args.resolution, chunk=args.chunk))
    assert yard["dims"] == dims, (yard["dims"], dims)
    same = bool(torch.equal(alpha, field["alpha"])) and bool(torch.equal(whole["alpha"], field["alpha"]))
    med = {k: statistics.median(v[1:]) for k, v in times.items()}                      # the first round is the warm-up
    volume, area = mesh.mesh_measures(vertices, faces)
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    res = {"workload": f"mesh.extract_frame phases, stage-3 Network on synthetic weights, posed synth.human_batch frame, resolution {args.resolution}, "
                       f"dims {list(dims)} = {N} vertices, {len(firsts)} chunks of {rows} rows, level {level:.6g} (median of the positive alphas), "
                       f"1 GPU, device events",
           "repeats": args.repeats, "alpha_bit_identical_to_frame_field": same, "V": V, "F": F, "volume": volume, "area": area,
           "unit_normals": float((normals.norm(dim=1) > 0.5).float().mean()) if V else 0.0, "median_ms": med,
           "min_ms": {k: min(v[1:]) for k, v in times.items()}, "max_ms": {k: max(v[1:]) for k, v in times.items()},
           "frame_field_ms_over_canonical_field_ms": med["frame_field_whole"] / med["canonical_field_whole"],
           "frame_field_minus_canonical_field_ms": med["frame_field_whole"] - med["canonical_field_whole"],
           "warp_plus_nonrigid_chain_ms": med["warp"] + med["nonrigid_chain"],
           "note": "canonical_field_whole: mesh.canonical_field on a grid of the same vertex count (the frame's box in the canonical constants), "
                   "volume decoder included; frame_field_whole includes the frame prologue (pose refiner, motion bases, volume decoder)"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
