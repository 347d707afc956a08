"""What the tracked mesh costs for a resolution-256 template, measured on one MI355X (a record, not a benchmark of the project:
bench.py is; there is no pass threshold).  The network is the stage-3 `Network` on the synthetic weights of the tests and the
benchmark, the non-rigid output layer AS IT IS DRAWN (offsets of 0.6 voxel that fold space: the fixed point is not expected to
converge on them, and the converged share says so); the frame a posed `synth.human_batch` item.  The untrained field does not reach
0.5 at this spacing, so the template's level is the median of the positive alphas (recorded), as in scripts/frame_mesh_cost.py.

Device events, the median of --repeats after one warm-up: one `ops.warp_invert` call on one chunk of `mesh.track` (2^18 template
vertices) from the `lbs_forward` guess (the first round's solve), the same call on as many points that all carry motion weight, one non-rigid chain, `mesh.track` as a whole
(prologue, guess, `outer` rounds, the canonical mask) and, in the same process and on the same frame, `mesh.extract_frame` for the
ratio.

Everything lands in --out (default profiles/track_mesh_cost.json)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_mesh_cost.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--outer", type=int, default=6)
    ap.add_argument("--iters", type=int, default=4)
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

    a = mesh.canonical_field(net, turn.const, 0.7, resolution=args.resolution)["alpha"]
    level = float(a[a > 0].median())
    del a
    tpl = mesh.extract(net, turn, 0.7, resolution=args.resolution, level=level)
    V = int(tpl["vertices"].shape[0])
    fa = mesh.frame_field(net, pose, resolution=args.resolution)["alpha"]
    frame_level = float(fa[fa > 0].median())
    del fa
    bmin, bscale = pose["cnl_bbox_min_xyz"].contiguous(), pose["cnl_bbox_scale_xyz"].contiguous()
    K = int(net.cfg.total_bones)
    tol = 1e-3 * tpl["spacing"]
    names = ("warp_invert_call", "warp_invert_call_on_body", "nonrigid_chain_call", "track_whole", "extract_frame_whole")
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
        pro = net.frame_prologue(**{k: pose[k] for k in FRAME_KEYS if k in pose})
        max_step = 2.0 / float(bscale.min()) / (int(pro["vol"].shape[-1]) - 1)
        rows = min(V, 1 << 18)                                                          # one chunk of `mesh.track`
        c = tpl["vertices"][:rows].contiguous()
        guess = ops.lbs_forward(c, pro["R_f"], pro["T_f"], pro["vol_cl"], bmin, bscale, K)
        for rep in range(args.repeats + 1):
            solved = timed("warp_invert_call", lambda: ops.warp_invert(c, guess, pro["R_b"], pro["T_b"], pro["vol"], bmin, bscale, K=K,
                                                                       iters=args.iters, tol=tol / 4.0, max_step=max_step))
            timed("nonrigid_chain_call", lambda: net._nonrigid_fwd(net._nr, solved[1], pro["cond"], pro["band_w"], save=False)[0])
        status = torch.bincount(solved[4].long(), minlength=3).tolist()
        del solved, guess
        # the same call where every row works: points of the frame's box with mask > 0.2 (under 1 % of it), their own images as targets,
        # guesses within half a voxel -- the known-roots case of tests/test_gpu_track.py at the size of a chunk
        lo, hi = (torch.from_numpy(pose["dst_bbox"][k]).to(dev) for k in ("min_xyz", "max_xyz"))
        gen, found = torch.Generator().manual_seed(11), []
        while sum(f.shape[0] for f in found) < rows:
            cand = (lo + torch.rand(1 << 22, 3, generator=gen).to(dev) * (hi - lo)).contiguous()
            m = ops.warp_invert(cand, cand, pro["R_b"], pro["T_b"], pro["vol"], bmin, bscale, K=K, iters=0, tol=tol, max_step=max_step)[2]
            found.append(cand[m > 0.2])
        star = torch.cat(found, 0)[:rows].contiguous()
        image = ops.warp_invert(star, star, pro["R_b"], pro["T_b"], pro["vol"], bmin, bscale, K=K, iters=0, tol=tol, max_step=max_step)[1]
        near = (star + (torch.rand(rows, 3, generator=gen).to(dev) - 0.5) * max_step).contiguous()
        for rep in range(args.repeats + 1):
            on_body = timed("warp_invert_call_on_body", lambda: ops.warp_invert(image, near, pro["R_b"], pro["T_b"], pro["vol"], bmin, bscale, K=K,
                                                                               iters=args.iters, tol=tol / 4.0, max_step=max_step))
        body_status = torch.bincount(on_body[4].long(), minlength=3).tolist()
        del found, star, image, near, on_body
    for rep in range(args.repeats + 1):
        tracked = timed("track_whole", lambda: mesh.track(net, tpl, pose, outer=args.outer, iters=args.iters, space="body"))
        frame = timed("extract_frame_whole", lambda: mesh.extract_frame(net, pose, resolution=args.resolution, level=frame_level, space="body"))
    med = {k: statistics.median(v[1:]) for k, v in times.items()}                      # the first round is the warm-up
    on = tracked["mask_canonical"] >= 0.05
    res = {"workload": f"mesh.track of a resolution-{args.resolution} template ({V} vertices, level {level:.6g} = median of the positive alphas) into a posed "
                       f"synth.human_batch frame, stage-3 Network on synthetic weights with the non-rigid output layer as drawn, outer {args.outer}, "
                       f"iters {args.iters}, tol {tol:.4g}; 1 GPU, device events",
           "repeats": args.repeats, "V": V, "rows_per_call": rows, "F": int(tpl["faces"].shape[0]), "median_ms": med,
           "min_ms": {k: min(v[1:]) for k, v in times.items()}, "max_ms": {k: max(v[1:]) for k, v in times.items()},
           "first_solve_status_counts": status, "on_body_status_counts": body_status, "converged_share": float(tracked["converged"].double().mean()),
           "share_with_mask_canonical_ge_0.05": float(on.double().mean()),
           "converged_share_where_mask_canonical_ge_0.05": float(tracked["converged"][on].double().mean()) if bool(on.any()) else None,
           "residual_median": float(tracked["residual"].median()),
           "frame_mesh": {"V": int(frame["vertices"].shape[0]), "level": frame_level, "grid_vertices": int(frame["alpha"].numel())},
           "track_ms_over_extract_frame_ms": med["track_whole"] / med["extract_frame_whole"],
           "note": "warp_invert_call / nonrigid_chain_call: one launch over rows_per_call template vertices, the solve from the lbs_forward guess (a row that is lost "
                   "stops at its first evaluation: see first_solve_status_counts); warp_invert_call_on_body: the same launch on rows_per_call points with mask > 0.2, "
                   "targets their own images, guesses within half a voxel -- every row iterates; track_whole includes the frame prologue "
                   "(pose refiner, motion bases, volume decoder), as extract_frame_whole does"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
