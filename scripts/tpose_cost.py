"""What a T-pose frame costs, measured on one MI355X (not a benchmark of the project: bench.py is).

  frame     `tpose.tpose_frame` + `eval.render_human_frame` of one 512 x 512 T-pose frame (synthetic weights, camera --idx of a 100-frame
            turn), host clock around a frame that ends in a device synchronise.
  setup     the ray set-up plus the image assembly ALONE, through the new launches (`rays.frame_rays_compact` + `rays.paint_frame`)
            and through the existing composition `eval.frame_rays` uses for a box (`get_rays_from_KRT` + `rays_intersect_3d_bbox` + the
            boolean indexing of four tensors, then `bg.expand().clone()`, one masked assignment and `to_8b_image`), ALTERNATING in one
            process after a warm-up of each, on the same camera, box and colours.

Median, min, max and inter-quartile range over --repeats; everything lands in --out (default profiles/tpose_cost.json)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms):
    ms = sorted(ms)
    q = statistics.quantiles(ms, n=4)
    return {"n": len(ms), "median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "iqr_ms": q[2] - q[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tpose_cost.json"))
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--idx", type=int, default=13)
    args = ap.parse_args()
    import numpy as np
    import torch
    from hosnerf_amd import eval as ev, formats, rays, synth, tpose
    from hosnerf_amd.hosnerf import HOSNeRF
    from hosnerf_amd.human_nerf import default_cfg
    dev = torch.device("cuda")
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    hos = HOSNeRF(default_cfg(d))
    hos.model.load_state_dict(synth.background_state_dict(777, 2), strict=False)
    hos.human.load_state_dict(synth.human_state_dict(777, 2), strict=True)
    hos = hos.to(dev)
    joints = synth.tpose_joints()
    turn = tpose.TposeTurn(joints, formats.skeleton_bbox(joints, float(hos.cfg.bbox_offset)), 32, dev)
    H = W = turn.img_size
    bgc = (255.0, 255.0, 255.0)

    def frame():
        fr = tpose.tpose_frame(None, None, args.idx, 100, bgcolor=bgc, turn=turn, iter_val=3e5, time=0.2)
        return fr, ev.render_human_frame(hos, fr, want_u8=True)

    fr, _ = frame()                                             # warm-up
    torch.cuda.synchronize()
    t_frame = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        frame()
        torch.cuda.synchronize()
        t_frame.append(1e3 * (time.perf_counter() - t0))

    _, add = tpose.tpose_pose(args.idx, 100)
    box = tpose.rotate_bbox(turn.bbox, add)
    K, E = turn.K, turn.E
    rgb = torch.rand(fr["count"], 3, device=dev)
    bg = torch.as_tensor(bgc, dtype=torch.float32, device=dev) / 255.0

    def new_path():
        r = rays.frame_rays_compact(H, W, K, E[:3, :3], E[:3, 3], box, device=dev)
        return rays.paint_frame(r["slot"], rgb, bgc, H, W)

    def old_path():
        o, dd = rays.get_rays_from_KRT(H, W, K, E[:3, :3], E[:3, 3], device=dev)
        o, dd = o.reshape(-1, 3), dd.reshape(-1, 3)
        near, far, m = rays.rays_intersect_3d_bbox(box, o, dd)
        batch = torch.stack([o[m], dd[m]], 0), near[:, None], far[:, None]
        out = bg.expand(H * W, 3).clone()
        out[m] = rgb
        return batch, out, ev.to_8b_image(out)

    for fn in (new_path, old_path):
        fn()
    torch.cuda.synchronize()
    t = {"new": [], "old": []}
    for _ in range(args.repeats):
        for name, fn in (("new", new_path), ("old", old_path)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append(1e3 * (time.perf_counter() - t0))
    a, b = new_path(), old_path()
    res = {"workload": f"T-pose frame {W}x{H}, camera {args.idx} of 100, {fr['count']} of {H * W} rays hit the box, synthetic weights, eager, 1 GPU",
           "frame": summary(t_frame),
           "setup_plus_assembly": {"new_launches": summary(t["new"]), "existing_composition": summary(t["old"]),
                                   "new_over_existing_median": statistics.median(t["new"]) / statistics.median(t["old"]),
                                   "same_frame": bool(torch.equal(a[0], b[1]) and torch.equal(a[1], b[2]))},
           "note": "host clock around calls that end in a device synchronise; the two set-up paths alternate call by call"}
    res["setup_plus_assembly"]["share_of_frame_new"] = res["setup_plus_assembly"]["new_launches"]["median_ms"] / res["frame"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
