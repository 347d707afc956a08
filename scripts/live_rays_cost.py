"""What running the human branch on the foreground rays only (ops.LIVE_RAYS; M:1547-1551) is worth, measured on one MI355X in ONE
process (not a benchmark of the project: bench.py is).

The workload is bench.py's primary line: the stage-3 step at 4096 rays, seeds as bench.py, both optimisers, captured as a hipGraph.
Two graphs are captured from the same modules -- ops.LIVE_RAYS off (the parent commit's path) and on -- and replayed in ALTERNATING
rounds of --steps replays each, a device synchronise at both ends of a round, host clock around it.  Both graphs run the optimiser
step, so the two series advance the same parameters; the live-ray share is read once per graph after its first replay.

The same is repeated on an item without a background ray (`aim_sigma=0`: every ray goes through a joint), where the on path pays
its extra launches and saves nothing.

Everything lands in --out (default profiles/live_rays_cost.json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms):
    s = sorted(ms)
    q = statistics.quantiles(s, n=4) if len(s) >= 4 else [s[0], statistics.median(s), s[-1]]
    return {"rounds_ms_per_step": ms, "median_ms": statistics.median(s), "q1_ms": q[0], "q3_ms": q[2], "min_ms": s[0], "max_ms": s[-1]}


def capture(torch, wl, warm):
    """bench.run_workload's capture of a whole single-GPU step (fwd + bwd + clip + both Adams)."""
    for o in wl.opts():
        o.set_step_hyper(wl.lr(warm))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            wl.fwd_bwd(warm)
            wl.finish(warm, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = wl.fwd_bwd(warm)
        wl.finish(warm, True)
    return graph, loss, wl.cycle_count, wl.last_out.get("live_ray_rows"), wl.last_out["idx_fg"]


def measure(torch, bench, ops, dev, rays, aim_sigma, args):
    from hosnerf_amd import synth
    from hosnerf_amd.train import batch_to_device, prepare_patch_targets, stage3_losses

    class Wl(bench.Stage3):
        def fwd_bwd(self, i):                      # bench.Stage3.fwd_bwd, keeping the forward's dict
            self.ob.zero_grad()
            self.oh.zero_grad()
            self.hos.human.split_decoder_backward = True
            out = self.hos.render(self.batch, randomized=True, is_train=True, static_cycle=True)
            self.cycle_count = out.get("cycle_count")
            self.last_out = out
            loss, _ = stage3_losses(out, self.batch)
            loss.backward()
            return loss.detach()

    wl = Wl(dev, 0, 1, rays)
    if aim_sigma is not None:
        n_patches = max(1, (rays + 1023) // 1024)
        item = synth.add_patch_supervision(synth.human_batch(rays, seed=777, time=0.5, is_train=True, iter_val=3e5, aim_sigma=aim_sigma),
                                           n_patches, 32, 777)
        wl.batch = batch_to_device(prepare_patch_targets(item), dev)
    graphs = {}
    for name, flag in (("off", False), ("on", True)):
        ops.LIVE_RAYS = flag
        for i in range(args.warmup):
            wl.eager_step(i)
        torch.cuda.synchronize()
        graphs[name] = capture(torch, wl, args.warmup)
    ops.LIVE_RAYS = True
    info = {}
    for name, (graph, loss, cyc, rows, fg) in graphs.items():
        for o in wl.opts():
            o.set_step_hyper(wl.lr(args.warmup))
        graph.replay()
        torch.cuda.synchronize()
        info[name] = {"f_cyc": float(cyc.reshape(-1)[0]) / (rays * 128), "foreground_share": float(fg.float().mean()),
                      "live_ray_rows_over_capacity": None if rows is None else float(rows.reshape(-1)[0]) / (rays * 128),
                      "loss": float(loss)}
    times = {"off": [], "on": []}
    for _ in range(args.rounds):
        for name in ("off", "on"):
            graph = graphs[name][0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                for o in wl.opts():
                    o.set_step_hyper(wl.lr(args.warmup + i))
                graph.replay()
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    off, on = summary(times["off"]), summary(times["on"])
    res = {"rays": rays, "aim_sigma": 0.25 if aim_sigma is None else aim_sigma, "steps_per_round": args.steps, "rounds": args.rounds,
           "off": {**off, **info["off"]}, "on": {**on, **info["on"]},
           "on_over_off_median": on["median_ms"] / off["median_ms"],
           "every_on_round_faster_than_every_off_round": max(times["on"]) < min(times["off"]),
           "on_median_inside_off_interquartile_range": off["q1_ms"] <= on["median_ms"] <= off["q3_ms"]}
    del graphs
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_rays_cost.json"))
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import bench
    from hosnerf_amd import ops
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"workload": "bench.py Stage3 (4096 rays, seed 777, two streams, one hipGraph per ops.LIVE_RAYS value), alternating rounds in one process",
           "bench_item": measure(torch, bench, ops, dev, args.rays, None, args)}
    print("LIVE_RAYS_COST bench_item " + json.dumps(res["bench_item"]), flush=True)
    torch.cuda.empty_cache()
    res["all_foreground_item"] = measure(torch, bench, ops, dev, args.rays, 0.0, args)
    print("LIVE_RAYS_COST all_foreground_item " + json.dumps(res["all_foreground_item"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
