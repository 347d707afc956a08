"""What drawing a stage-1 batch from the device ray bank costs next to the step it feeds, measured on one MI355X (not a benchmark of
the project: bench.py is).

  sample   `RayBank.sample(4096, generator)` on a synthetic scene of --frames frames of --size x --size pixels (disc masks): two device
           random draws, the rank slice and hos_raybank_gather; host clock around a call that ends in a device synchronise.
  step     the stage-1 training step (`train.train_step_stage1`: forward, losses, backward, clipped fused Adam) on a synthetic batch
           of 4096 rays (`synth.stage1_batch`), same process, same clock.

The two alternate call by call after a warm-up of each.  Median, min, max and inter-quartile range over --repeats, and the ratio of the
medians; everything lands in --out (default profiles/raybank_cost.json)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raybank_cost.json"))
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    args = ap.parse_args()
    import torch
    from hosnerf_amd import formats, synth
    from hosnerf_amd.mipnerf360 import MipNeRF360
    from hosnerf_amd.raybank import RayBank
    from hosnerf_amd.train import FusedAdam, train_step_stage1
    dev = torch.device("cuda")
    d = tempfile.mkdtemp(prefix="hos_raybank_scene_")
    px = synth.write_scene_dir(d, args.frames, args.size, args.size, seed=7)
    scene = formats.load_scene(d, (args.size, args.size), masks=px["alphas"], near=0.1, far=1e6)
    t0 = time.perf_counter()
    bank = RayBank(scene, px["images"], px["alphas"], device=dev, split="train")
    torch.cuda.synchronize()
    t_build = 1e3 * (time.perf_counter() - t0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    model = MipNeRF360(d, opaque_background=True)
    model.load_state_dict(synth.background_state_dict(777, 2), strict=False)
    model = model.to(dev)
    opt = FusedAdam(model, lr=1e-5, max_grad_norm=0.001)
    batch = {k: v.to(dev) for k, v in synth.stage1_batch(args.rays, seed=5).items()}

    def sample():
        return bank.sample(args.rays, gen)

    def step():
        return train_step_stage1(model, opt, batch, 0.5, 0.1, 1e6)

    for fn in (sample, step, sample, step):          # warm-up of every shape the timed window uses
        fn()
    torch.cuda.synchronize()
    t = {"sample": [], "step": []}
    for _ in range(args.repeats):
        for name, fn in (("sample", sample), ("step", step)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append(1e3 * (time.perf_counter() - t0))
    res = {"workload": f"{args.rays} rays; bank of {args.frames} frames {args.size}x{args.size}, {int(bank.offsets_host[-1])} unmasked rays, "
                       f"{len(bank.choice_host)} training images; synthetic weights, eager, 1 GPU",
           "bank_build_ms_once": t_build,
           "sample": summary(t["sample"]), "train_step": summary(t["step"]),
           "sample_over_step_median": statistics.median(t["sample"]) / statistics.median(t["step"]),
           "note": "host clock around calls that end in a device synchronise; the two alternate call by call; the bank build includes "
                   "the uploads, the index pass and its first-launch code load"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
