"""What the stage-1 maps (opacity, expected and median distance) cost, measured on one MI355X (not a benchmark of the project: bench.py is).

  frames   `eval.render_bkgd_frame` of one synthetic 1920x1080 stage-1 frame at `LitData.chunk` of configs/state_mipnerf360_backpack.gin
           (eager, like the launcher's frame loop) with and without `maps`, ALTERNATING the two in one process after a warm-up frame of
           each; host clock around a frame that ends in a device synchronise; median, quartiles, min, max over --repeats rounds.
  frames --chunk 32768 --section frames_chunk_32768: the same frame in 64 chunks instead of 507 (what scales with the number of chunks).
  host     host time to enqueue one call of `ops.volumetric_rendering` / `ops.volrender_maps`, no synchronise inside the window.
  kernel   the rendering kernel alone at --rays rays of 32 samples, rgb-only and maps instantiation alternating, meant to be run
           under a kernel trace of its own:
               rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/bkgd_maps_cost.py kernel
           `python scripts/bkgd_maps_cost.py stats <dir>` then reads the trace's kernel statistics into the JSON.

Everything lands in --out (default profiles/bkgd_maps_cost.json), one section per sub-command."""
import argparse
import csv
import glob
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
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [ms[0], statistics.median(ms), ms[-1]]
    return {"n": len(ms), "median_ms": statistics.median(ms), "q1_ms": q[0], "q3_ms": q[2], "min_ms": ms[0], "max_ms": ms[-1]}


def merge_out(path, section, value):
    d = json.load(open(path)) if os.path.exists(path) else {}
    d[section] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)


def frames(args):
    import numpy as np
    import torch
    from hosnerf_amd import eval as ev, gin_lite, synth
    from hosnerf_amd.mipnerf360 import MipNeRF360
    from hosnerf_amd.raybank import RayBank
    gin = gin_lite.parse_config_files_and_bindings([os.path.join(ROOT, "configs", "state_mipnerf360_backpack.gin")], None)
    chunk = int(args.chunk or gin.get_param("LitData.chunk", 1024 * 32))
    H, W = args.height, args.width
    dev = torch.device("cuda")
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    model = MipNeRF360(d, opaque_background=True)
    model.load_state_dict(synth.background_state_dict(777, 2), strict=False)
    model = model.to(dev)
    f = 1.2 * W
    scene = {"extrinsics": np.eye(4)[None], "intrinsics": np.array([[[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]]]), "times": np.array([0.5], np.float32),
             "render_poses": None, "render_times": None, "i_split": (np.arange(1), np.arange(1), np.arange(1), np.arange(1)),
             "bkgrays_sizes": np.array([H * W])}
    bank = RayBank(scene, np.zeros((1, H, W, 3), np.uint8), np.zeros((1, H, W), np.float32), device=dev, split="all")
    kw = {v: {"off": {}, "on": {"maps": True}}[v] for v in args.variants.split(",")}
    times, host_ms = {v: [] for v in kw}, {v: [] for v in kw}
    for v in kw:                                                  # warm-up: every shape of the timed window
        ev.render_bkgd_frame(model, bank, 0, chunk, 0.5, 0.1, 1e6, **kw[v])
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for v in kw:
            t0 = time.perf_counter()
            out = ev.render_bkgd_frame(model, bank, 0, chunk, 0.5, 0.1, 1e6, **kw[v])
            host_ms[v].append(1e3 * (time.perf_counter() - t0))       # the loop has ENQUEUED the frame: the host's share
            torch.cuda.synchronize()
            times[v].append(1e3 * (time.perf_counter() - t0))
    if set(kw) != {"off", "on"}:                                  # one variant alone: a run under a kernel trace of its own
        print(json.dumps({v: summary(t) for v, t in times.items()}))
        return
    off, on = summary(times["off"]), summary(times["on"])
    res = {"workload": f"eval.render_bkgd_frame, synthetic {W}x{H} stage-1 frame, {chunk}-ray chunks (LitData.chunk), eager, forward only, 1 GPU",
           "rays": H * W, "chunks": -(-H * W // chunk), "finite": bool(all(torch.isfinite(v).all() for v in out.values())),
           "maps_off": off, "maps_on": on, "times_ms": times,
           "host_enqueue_of_the_frame_ms": {v: summary(t) for v, t in host_ms.items()},
           "maps_on_overhead_of_median": on["median_ms"] / off["median_ms"] - 1.0,
           "maps_on_median_inside_maps_off_quartiles": bool(off["q1_ms"] <= on["median_ms"] <= off["q3_ms"])}
    merge_out(args.out, args.section, res)
    print(json.dumps({k: v for k, v in res.items() if k != "times_ms"}))


def kernel(args):
    import torch
    from hosnerf_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(17)
    B, S = args.rays, 32
    td = torch.sort(torch.rand(B, S + 1, generator=g) * 3 + 0.2, -1).values.to(dev)
    w = torch.softmax(torch.randn(B, S, generator=g), -1).to(dev)
    rgb = torch.rand(B, S, 3, generator=g).to(dev)
    with torch.no_grad():
        for _ in range(args.warmup + args.repeats):
            ops.volumetric_rendering(rgb, w, 1.0)
            ops.volrender_maps(rgb, w, td, 1.0)
    torch.cuda.synchronize()
    print(f"rendering kernels launched: {args.warmup + args.repeats} x (rgb-only, maps) at {B} rays of {S} samples")


def host(args):
    """Host time to ENQUEUE one call of either op (no synchronise inside the window): what a chunk adds where the frame loop waits on
    the host rather than on the device."""
    import torch
    from hosnerf_amd import ops
    dev = torch.device("cuda")
    B, S = args.rays, 32
    td = torch.sort(torch.rand(B, S + 1) * 3 + 0.2, -1).values.to(dev)
    w = torch.softmax(torch.randn(B, S), -1).to(dev)
    rgb = torch.rand(B, S, 3).to(dev)
    calls = {"rgb_only": lambda: ops.volumetric_rendering(rgb, w, 1.0), "maps": lambda: ops.volrender_maps(rgb, w, td, 1.0)}
    res = {}
    with torch.no_grad():
        for name, fn in calls.items():
            per_call = []
            for _ in range(args.repeats):
                fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(200):
                    fn()
                per_call.append(1e6 * (time.perf_counter() - t0) / 200)
                torch.cuda.synchronize()
            res[name + "_enqueue_us"] = {"median": statistics.median(per_call), "min": min(per_call), "max": max(per_call)}
    res["rays"] = B
    merge_out(args.out, "host_enqueue", res)
    print(json.dumps(res))


def stats(args):
    rows = {}
    for path in glob.glob(os.path.join(args.trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "volrender_fwd_kernel" in r["Name"]:
                rows["rgb_only" if "VolNoMaps" in r["Name"] else "maps"] = {
                    "kernel": r["Name"], "calls": int(r["Calls"]), "mean_ns": float(r["AverageNs"]), "min_ns": float(r["MinNs"]),
                    "max_ns": float(r["MaxNs"]), "stddev_ns": float(r["StdDev"])}
    if set(rows) != {"maps", "rgb_only"}:
        raise SystemExit(f"no rendering kernel statistics under {args.trace_dir}: {sorted(rows)}")
    rows["rays"] = args.rays
    rows["note"] = "rocprofv3 --kernel-trace --stats, warm-up launches included in the statistics; alternating launches"
    rows["maps_over_rgb_only_mean"] = rows["maps"]["mean_ns"] / rows["rgb_only"]["mean_ns"] - 1.0
    merge_out(args.out, "volrender_kernel", rows)
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("frames", "kernel", "stats", "host"))
    ap.add_argument("trace_dir", nargs="?", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bkgd_maps_cost.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=0, help="rays per chunk (default: LitData.chunk of the shipped configuration)")
    ap.add_argument("--variants", default="off,on", help="frames: off,on (alternating) or one of them alone (nothing is written)")
    ap.add_argument("--section", default="frames", help="frames: the JSON section to write (a second chunk size next to the first)")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    args = ap.parse_args()
    {"frames": frames, "kernel": kernel, "stats": stats, "host": host}[args.what](args)


if __name__ == "__main__":
    main()
