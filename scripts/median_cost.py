"""What the median depth of stage-3 frames costs, measured on one MI355X (not a benchmark of the project: bench.py is).  The baseline is
the maps path of this same build, whose kernels are the parent commit's instruction for instruction.

  frames   `eval.render_frame(maps=True)` of the synthetic 1920x1080 frame of scripts/maps_cost.py (65536-ray chunks, eager like the
           launcher's frame loop) with and without `median=True`, ALTERNATING the two in one process after a warm-up frame of each; host
           clock around a frame that ends in a device synchronise; median, min, max, quartiles over --repeats frames, in two worker
           processes (first half, second half) so that drift of the shared host shows.
  kernel   the merge kernel alone at 8192 rays (32 + 128 samples), maps and median instantiation alternating, meant to be run under a
           kernel trace of its own:
               rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/median_cost.py kernel
           `python scripts/median_cost.py stats <dir>` then reads the trace's kernel statistics into the JSON.

Everything lands in --out (default profiles/median_cost.json), one section per sub-command."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from maps_cost import build_scene, merge_out  # noqa: E402  (the frame and the JSON sections of the maps measurement)


def summary(ms):
    ms = sorted(ms)
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [ms[0], statistics.median(ms), ms[-1]]
    return {"n": len(ms), "median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "q1_ms": q[0], "q3_ms": q[2], "iqr_ms": q[2] - q[0]}


def worker(args):
    """Times frames; the variants alternate frame by frame.  Prints one JSON line."""
    torch, ev, hos, fr = build_scene(ROOT, args.height, args.width)
    kw = {"maps": {"maps": True}, "median": {"maps": True, "median": True}}
    times = {v: [] for v in kw}
    for v in kw:                                                # warm-up: every shape of the timed window
        ev.render_frame(hos, fr, chunk_bkg=65536, **kw[v])
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for v in kw:
            t0 = time.perf_counter()
            out = ev.render_frame(hos, fr, chunk_bkg=65536, **kw[v])
            torch.cuda.synchronize()
            times[v].append(1e3 * (time.perf_counter() - t0))
    med, alpha = out["depth_median"], out["alpha"]
    print("MEDIAN_COST " + json.dumps({"times_ms": times, "rays": args.height * args.width, "foreground_fraction": float(fr["ray_mask"].float().mean()),
                                       "finite": bool(torch.isfinite(med).all()), "fraction_alpha_above_half": float((alpha > 0.5).float().mean())}))


def run_worker(repeats, args):
    cmd = [sys.executable, os.path.abspath(__file__), "worker", "--repeats", str(repeats), "--height", str(args.height), "--width", str(args.width)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"worker failed ({r.returncode}): {r.stderr[-3000:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("MEDIAN_COST ")][-1][len("MEDIAN_COST "):])


def frames(args):
    half = max(1, args.repeats // 2)
    runs = [run_worker(half, args), run_worker(half, args)]
    off = runs[0]["times_ms"]["maps"] + runs[1]["times_ms"]["maps"]
    on = runs[0]["times_ms"]["median"] + runs[1]["times_ms"]["median"]
    s_off, s_on = summary(off), summary(on)
    res = {"workload": f"eval.render_frame(maps=True), synthetic {args.width}x{args.height} frame, 65536-ray chunks, eager, forward only, 1 GPU",
           "rays": runs[0]["rays"], "foreground_fraction": runs[0]["foreground_fraction"], "finite": all(r["finite"] for r in runs),
           "fraction_alpha_above_half": runs[0]["fraction_alpha_above_half"],
           "maps": s_off, "maps_median": s_on,
           "maps_first_half_vs_second_half_median_ms": [statistics.median(r["times_ms"]["maps"]) for r in runs],
           "median_overhead_of_median": s_on["median_ms"] / s_off["median_ms"] - 1.0,
           "median_frame_inside_quartiles_of_maps_frame": bool(s_off["q1_ms"] <= s_on["median_ms"] <= s_off["q3_ms"])}
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
    want = ops.MAP_KEYS + (ops.MEDIAN_KEY,)
    with torch.no_grad():
        for i in range(args.warmup + args.repeats):
            ops.merge_composite_maps(*a)
            ops.merge_composite_maps(*a, want=want)
    torch.cuda.synchronize()
    print(f"merge kernels launched: {args.warmup + args.repeats} x (maps, median) at {B} rays")


def stats(args):
    rows = {}
    for path in glob.glob(os.path.join(args.trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "merge_composite_kernel" in r["Name"]:
                key = "median" if "MergeMedianArgs" in r["Name"] else "maps" if "MergeMapsArgs" in r["Name"] else "rgb_only"
                rows[key] = {"kernel": r["Name"], "calls": int(r["Calls"]), "mean_ns": float(r["AverageNs"]), "min_ns": float(r["MinNs"]),
                             "max_ns": float(r["MaxNs"]), "stddev_ns": float(r["StdDev"])}
    if not {"maps", "median"} <= set(rows):
        raise SystemExit(f"no merge kernel statistics under {args.trace_dir}: {sorted(rows)}")
    rows["rays"] = args.rays
    rows["note"] = "rocprofv3 --kernel-trace --stats, warm-up launches included in the statistics; alternating launches"
    rows["median_over_maps_mean"] = rows["median"]["mean_ns"] / rows["maps"]["mean_ns"] - 1.0
    merge_out(args.out, "merge_kernel", rows)
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("frames", "kernel", "stats", "worker"))
    ap.add_argument("trace_dir", nargs="?", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "median_cost.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--step-timeout", type=int, default=900)
    args = ap.parse_args()
    {"frames": frames, "kernel": kernel, "stats": stats, "worker": worker}[args.what](args)


if __name__ == "__main__":
    main()
