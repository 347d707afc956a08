"""What the depth / opacity / layer maps cost, measured on one MI355X (not a benchmark of the project: bench.py is).

  frames   `eval.render_frame` of the synthetic 1920x1080 frame (the frame of scripts/bench_infer.py, 65536-ray chunks, eager like the
           launcher's frame loop) with and without `maps`, ALTERNATING the two in one process after a warm-up frame of each; host
           clock around a frame that ends in a device synchronise; median, min, max, inter-quartile range over --repeats frames.
           With --parent-root DIR (a checkout of the parent commit with its library built) the same loop without maps runs there too,
           in a process of its own, between two halves of this tree's run, so that drift of the shared host shows.
  kernel   the merge kernel alone at 8192 rays (32 + 128 samples), rgb-only and maps instantiation alternating, meant to be run
           under a kernel trace of its own:
               rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/maps_cost.py kernel
           `python scripts/maps_cost.py stats <dir>` then reads the trace's kernel statistics into the JSON.

Everything lands in --out (default profiles/maps_cost.json), one section per sub-command."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(ms):
    ms = sorted(ms)
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [ms[0], statistics.median(ms), ms[-1]]
    return {"n": len(ms), "median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "iqr_ms": q[2] - q[0]}


def merge_out(path, section, value):
    d = json.load(open(path)) if os.path.exists(path) else {}
    d[section] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def build_scene(root, H, W):
    sys.path.insert(0, root)
    import torch
    from hosnerf_amd import eval as ev, synth
    from hosnerf_amd.hosnerf import HOSNeRF
    from hosnerf_amd.human_nerf import default_cfg
    dev = torch.device("cuda")
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    cfg = default_cfg(d)
    cfg.chunk = min(max(65536, int(cfg.chunk)), 32768)
    hos = HOSNeRF(cfg)
    hos.model.load_state_dict(synth.background_state_dict(777, 2), strict=False)
    hos.human.load_state_dict(synth.human_state_dict(777, 2), strict=True)
    hos = hos.to(dev)
    hb = synth.human_batch(8, seed=2, time=0.5, is_train=False, iter_val=3e5)
    K, E, Ec = synth.eval_camera(H, W, hb)
    bbox = {"min_xyz": hb["dst_bbox_min_xyz"].numpy(), "max_xyz": hb["dst_bbox_max_xyz"].numpy()}
    fr = ev.frame_rays(H, W, K, E, bbox, Ec, device=dev)
    fr.update({k: (hb[k].to(dev) if isinstance(hb[k], torch.Tensor) else hb[k]) for k in ev.FRAME_KEYS})
    return torch, ev, hos, fr


def worker(args):
    """Times frames of the tree at --root; variants alternate frame by frame.  Prints one JSON line."""
    torch, ev, hos, fr = build_scene(args.root, args.height, args.width)
    variants = [v for v in args.variants.split(",") if v]
    kw = {"off": {}, "on": {"maps": True}}
    times = {v: [] for v in variants}
    for v in variants:                                          # warm-up: every shape of the timed window
        ev.render_frame(hos, fr, chunk_bkg=65536, **kw[v])
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for v in variants:
            t0 = time.perf_counter()
            out = ev.render_frame(hos, fr, chunk_bkg=65536, **kw[v])
            torch.cuda.synchronize()
            times[v].append(1e3 * (time.perf_counter() - t0))
    print("MAPS_COST " + json.dumps({"times_ms": times, "rays": args.height * args.width, "foreground_fraction": float(fr["ray_mask"].float().mean()),
                                     "finite": bool(torch.isfinite(out["rgb"] if isinstance(out, dict) else out).all())}))


def run_worker(root, variants, repeats, args):
    cmd = [sys.executable, os.path.abspath(__file__), "worker", "--root", root, "--variants", variants, "--repeats", str(repeats),
           "--height", str(args.height), "--width", str(args.width)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout, cwd=root)
    if r.returncode != 0:
        raise SystemExit(f"worker in {root} failed ({r.returncode}): {r.stderr[-3000:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("MAPS_COST ")][-1][len("MAPS_COST "):])


def frames(args):
    half = max(1, args.repeats // 2)
    runs = [run_worker(ROOT, "off,on", half, args)]
    parent = run_worker(os.path.abspath(args.parent_root), "off", 2 * half, args) if args.parent_root else None
    runs.append(run_worker(ROOT, "off,on", half, args))
    off = runs[0]["times_ms"]["off"] + runs[1]["times_ms"]["off"]
    on = runs[0]["times_ms"]["on"] + runs[1]["times_ms"]["on"]
    res = {"workload": f"eval.render_frame, synthetic {args.width}x{args.height} frame, 65536-ray chunks, eager, forward only, 1 GPU",
           "rays": runs[0]["rays"], "foreground_fraction": runs[0]["foreground_fraction"], "finite": all(r["finite"] for r in runs),
           "maps_off": summary(off), "maps_on": summary(on),
           "maps_off_first_half_vs_second_half_median_ms": [statistics.median(r["times_ms"]["off"]) for r in runs],
           "maps_on_overhead_of_median": statistics.median(on) / statistics.median(off) - 1.0}
    if parent is not None:
        res["parent_commit_maps_off"] = summary(parent["times_ms"]["off"])
        res["maps_off_vs_parent_median"] = statistics.median(off) / statistics.median(parent["times_ms"]["off"]) - 1.0
    else:
        res["parent_commit_maps_off"] = "not measured (no --parent-root)"
    merge_out(args.out, "frames", res)
    print(json.dumps(res))


def kernel(args):
    sys.path.insert(0, ROOT)
    import torch
    from hosnerf_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(17)
    B, Sb, Sh = args.rays, 32, 128
    td = torch.sort(torch.rand(B, Sb + 1, generator=g) * 3 + 0.2, -1).values
    hum = torch.rand(B, Sh, 4, generator=g)
    mask = torch.rand(B, Sh, generator=g) * (torch.rand(B, Sh, generator=g) > 0.5)
    mask[: B // 8] = 0.0
    o = torch.randn(B, 3, generator=g) * 0.1
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * 0.7
    zt = torch.sort(torch.rand(B, Sh, generator=g) * 3 + 0.2, -1).values
    a = [t.to(dev) for t in (td, torch.rand(B, Sb, 3, generator=g), torch.rand(B, Sb, generator=g) * 2, hum,
                             o[:, None] + d[:, None] * zt[..., None], mask, o, d, torch.eye(4))]
    with torch.no_grad():
        for i in range(args.warmup + args.repeats):
            ops.merge_composite(*a)
            ops.merge_composite_maps(*a)
    torch.cuda.synchronize()
    print(f"merge kernels launched: {args.warmup + args.repeats} x (rgb-only, maps) at {B} rays")


def stats(args):
    rows = {}
    for path in glob.glob(os.path.join(args.trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "merge_composite_kernel" in r["Name"]:
                rows["maps" if "MergeMapsArgs" in r["Name"] else "rgb_only"] = {
                    "kernel": r["Name"], "calls": int(r["Calls"]), "mean_ns": float(r["AverageNs"]), "min_ns": float(r["MinNs"]),
                    "max_ns": float(r["MaxNs"]), "stddev_ns": float(r["StdDev"])}
    if set(rows) != {"maps", "rgb_only"}:
        raise SystemExit(f"no merge kernel statistics under {args.trace_dir}: {sorted(rows)}")
    rows["rays"] = args.rays
    rows["note"] = "rocprofv3 --kernel-trace --stats, warm-up launches included in the statistics; alternating launches"
    rows["maps_over_rgb_only_mean"] = rows["maps"]["mean_ns"] / rows["rgb_only"]["mean_ns"] - 1.0
    merge_out(args.out, "merge_kernel", rows)
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("frames", "kernel", "stats", "worker"))
    ap.add_argument("trace_dir", nargs="?", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maps_cost.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--variants", default="off,on")
    args = ap.parse_args()
    {"frames": frames, "kernel": kernel, "stats": stats, "worker": worker}[args.what](args)


if __name__ == "__main__":
    main()
