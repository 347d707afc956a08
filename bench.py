#!/usr/bin/env python
"""bench.py -- train rays/s of the HOSNeRF training steps on MI355X (BASELINE.json metric: "train rays/sec at 1/2/4/8 MI355X").

PRIMARY line (the `value` / `ms_per_step` / `roofline` of the one JSON line):
  BASELINE configs[3] -- stage-3 full HOSNeRF (background mip-NeRF-360 + human-object branch + z-merged composite + MSE /
  flow / cycle losses + two flat Adam updates), **4096 rays per step GLOBAL, STRONG scaling**: 4096 / N rays per GPU, every
  rank's gradients all-reduced over RCCL: 38 MB background + 4 MB human + the 3.5 MB volume gradient -- the 253 MB gradient of
  the human network's volume decoder (replicated forward, no ray enters it) is reduced at the decoder's OUTPUT instead.  This is the series the north-star's
  ">= 6x at 8 GPUs" refers to.  At N = 1 all 4096 rays run on one GPU.
SECONDARY objects in the same line (`stages`):
  stage2  BASELINE configs[2] -- the reference's stage-2 step (human-object network with its in-network composite, 0.2 MSE on
          unpacked patches + 0.01 flow + 0.01 cycle, Adam; 2048 rays = 2 patches of 32x32), N = 1 only, next to the SAME op
          graph as plain PyTorch-ROCm ops on the same GPU (`torch_rocm`: the denominator of the north-star's ">= 10x").
  stage1  BASELINE configs[1] -- stage-1 background mip-NeRF-360, 1024 rays per GPU (weak scaling), one all-reduce per step.
  infer_1080p  BASELINE configs[4] -- one whole synthetic 1920x1080 free-viewpoint frame (forward only, ray set-up included),
          rays sharded over the N ranks with one RGB all-gather per ray list; rays/s, algorithmic TFLOP/s and the dominant
          forward kernel's roofline fraction.
One "step" = forward + losses + backward + gradient all-reduce (N > 1) + gradient-norm clip (the Trainer's gradient_clip_val =
run.grad_max_norm = 0.001 of every Backpack.gin; ONE norm over both modules in stage 3) + Adam; nothing skipped, inputs resident in
HBM.  Steps are captured once in a hipGraph (forward + backward [+ optimiser at N = 1]) and replayed; per-step scalars that
change (learning rate, Adam bias corrections) live in device memory.

A PLAIN run measures the PRIMARY line only: set-up, warm-up, the timed steps, the JSON line.  `--full` adds everything else this
file measures or checks -- the secondary stages, the PyTorch-ROCm and CPU baseline legs, the exact-fp32 companions, the 1080p
frame, the per-kernel / roofline post-pass and the replayed PSNR record.  `--dump-outputs DIR` writes what the last timed step of
the primary workload computed (loss, rendered colours, updated parameters) as DIR/<name>.npy; all inputs and draws are seeded, so
two builds of the library can be compared output for output.

    python bench.py --gpus 1 --steps 20 --warmup 5 [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
        bench.py --gpus N --steps K --warmup W [--full]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
SPLIT_MFMA_PEAK_TFLOPS = 2500.0 / 3   # 3 bf16/fp16 MFMAs (dense peak ~2.5 PFLOP/s) per algorithmic product
# SURVEY 8(d) algorithmic FLOP per ray (2 FLOP per MAC; forward + weight gradients + the data gradients that are needed):
# (fixed part, part proportional to f_cyc = the fraction of the human sample points selected into the cycle set -- MEASURED on
# the workload after warm-up, `cycle_count / (rays * 128)`, not assumed to be 1)
FLOP_PER_RAY = {"stage1": (1841e6, 0.0), "stage2": (558e6, 77.7e6), "stage3": (2261e6, 77.7e6)}
# SURVEY 8(d) config 5, forward only: background-only ray / ray through the subject's box (+ 160.2 M for the human branch core)
FWD_FLOP_BG, FWD_FLOP_FG = 651.0e6, 811.3e6
GLOBAL_RAYS_S3 = 4096
GRAD_MAX_NORM = 0.001       # run.grad_max_norm of the reference's three Backpack.gin files -> Trainer(gradient_clip_val=..., "norm")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--primary", choices=["stage3", "stage2", "stage1"], default="stage3")
    ap.add_argument("--rays", type=int, default=0, help="override the primary workload's GLOBAL ray count (stage 3 / 2) or per-GPU count (stage 1)")
    ap.add_argument("--full", action="store_true", help="also run everything beyond the primary line: secondary stages, baseline legs, exact-fp32 "
                    "companions, the 1080p frame, the per-kernel / roofline post-pass, the replayed PSNR record (the --only-primary / --no-* "
                    "switches below trim a --full run; a plain run has none of it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the primary workload's last timed "
                    "step computed as DIR/<name>.npy (float32; at most 64 MB in all, large arrays as a fixed seeded sample)")
    ap.add_argument("--only-primary", action="store_true", help="skip the secondary stages and the baseline legs")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-torch-baseline", action="store_true")
    ap.add_argument("--no-kernel-events", action="store_true")
    ap.add_argument("--no-fp32-exact", action="store_true", help="skip the exact-fp32 companion legs (stages.*_fp32_exact)")
    ap.add_argument("--no-infer", action="store_true", help="skip the config-5 leg (one 1080p inference frame, ~10 s)")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel eagerly instead of replaying a captured hipGraph")
    ap.add_argument("--h2d", action="store_true", help="PCIe-inclusive variant (never the headline `value`): every timed step first "
                    "re-uploads the item's tensors from pinned host memory into the step's device batch")
    ap.add_argument("--gemm", choices=["planes", "split", "fp32"], default="planes",
                    help="split = fp16/bf16 hi-lo split MFMA (3 products, fp32 accumulate); fp32 = exact fp32 MFMA")
    args = ap.parse_args()
    if not args.full:       # a plain run does what the headline figure needs and nothing else
        args.only_primary = args.no_kernel_events = True
    return args


def basedir():
    d = tempfile.mkdtemp(prefix="hos_bench_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    return d


# ------------------------------------------------------------------------------------------------ workloads
class Workload:
    """One stage's training step on this rank: eager step, captured step, per-step host work."""

    name = ""
    scaling = "weak"
    static_vol_grad = None
    cycle_count = None          # device scalar of the last forward (human stages): rows selected into the cycle set

    def f_cyc(self):
        """Measured fraction of the human sample points in the cycle set (one 4-byte read, outside the timed region)."""
        if self.cycle_count is None:
            return 0.0
        return float(self.cycle_count.reshape(-1)[0]) / (self.rays_local * 128)

    def freeze_static(self):
        """After the first half of a step has been captured: remember the tensors the eager collectives act on."""

    def fwd_bwd(self, i):
        raise NotImplementedError

    def opts(self):
        raise NotImplementedError

    def lr(self, i):
        raise NotImplementedError

    def reduce(self):
        """Eager collectives between the two captured halves of a step (N > 1): flat-gradient all-reduces."""
        from hosnerf_amd.train import allreduce_flat_grad
        for o in self.opts():
            allreduce_flat_grad(o.module, o.group)

    def finish(self, i, dynamic):
        """Second half: ONE gradient norm over the (already reduced) flat gradients of every module of the step -- the Trainer's
        `gradient_clip_val = run.grad_max_norm = 0.001`, norm clipping, bound by all three Backpack.gin files -- then the Adams."""
        from hosnerf_amd.train import step_all
        step_all(self.opts(), None if dynamic else self.lr(i), dynamic=dynamic, reduced=True)

    # N > 1, captured: the second half in two graphs so that the volume decoder's backward (0.7 ms, needs only the 3.5 MB
    # volume gradient) runs UNDER the exchange of the other gradients (38 MB + 4.3 MB on the communicator's stream)
    overlap = False

    def reduce_begin(self):
        """Enqueue every collective; wait for the one the decoder's backward needs.  Returns the handles still in flight."""
        self.reduce()
        return []

    def finish_decoder(self):
        """Captured between reduce_begin and the waits (workloads with a volume decoder)."""

    def finish_optim(self, i, dynamic):
        Workload.finish(self, i, dynamic)

    def eager_step(self, i):
        loss = self.fwd_bwd(i)
        self.reduce()
        self.finish(i, False)
        return loss

    def outputs(self):
        """What a caller of the step holds after it, next to the loss: the rendered colours of its forward and the updated flat
        parameter buffers (in a captured step these tensors are static: after a replay they hold that step's values)."""
        raise NotImplementedError


class Stage1(Workload):
    name, scaling = "stage1", "weak"
    describe = ("BASELINE configs[1]: stage-1 background mip-NeRF-360, 1024 rays/batch per GPU, 64/64/32 samples, "
                "PropMLP 4x256 x2 + NeRFMLP 8x1024, 2 states")

    def __init__(self, dev, rank, world, rays):
        from hosnerf_amd import synth
        from hosnerf_amd.mipnerf360 import MipNeRF360
        from hosnerf_amd.train import FusedAdam
        self.rays_local, self.rays_global = rays, rays * world
        self.model = MipNeRF360(basedir(), opaque_background=True)
        self.model.load_state_dict(synth.background_state_dict(777, 2), strict=False)   # identical replicas on every rank
        self.model = self.model.to(dev)
        self.opt = FusedAdam(self.model, lr=2e-3, max_grad_norm=GRAD_MAX_NORM)
        self.batch = {k: v.to(dev) for k, v in synth.stage1_batch(rays, seed=777 + rank).items()}
        self.batch["times"] = 0.5      # python float: no host sync inside the step (the reference syncs on `time` every call)
        self.max_steps = 500000
        self.frac = torch.zeros(1, device=dev)       # train_frac lives on the device: the captured step anneals like the eager one

    def opts(self):
        return [self.opt]

    def lr(self, i):
        from hosnerf_amd.train import stage1_lr
        return stage1_lr(i, self.max_steps)

    def host_prepare(self, i):
        self.frac.fill_(i / self.max_steps)

    def fwd_bwd(self, i):
        from hosnerf_amd.train import stage1_loss
        self.opt.zero_grad()
        rend, hist = self.model(self.batch, self.frac, True, True, 0.1, 1e6)
        self.last_rgb = rend[-1]["rgb"].detach()
        loss, _ = stage1_loss(rend[-1]["rgb"], self.batch["target"], hist)
        loss.backward()
        return loss.detach()

    def outputs(self):
        return {"rgb": self.last_rgb, "params_background": self.model.flat_param}


def _human_item(rays, rank, stage):
    from hosnerf_amd import synth
    from hosnerf_amd.train import prepare_patch_targets
    n_patches = max(1, (rays + 1023) // 1024)
    b = synth.add_patch_supervision(synth.human_batch(rays, seed=777 + rank, time=0.5, is_train=True, iter_val=3e5), n_patches, 32, 777 + rank)
    return b, prepare_patch_targets(b)


_HOSCOMM = {}


def hoscomm(rank, world):
    """HOS_HOSCOMM=1 (opt-in; no N > 1 RCCL run has been possible on the build hardware): the step's collectives go through
    libhoscomm.so (include/hoscomm.h) on the capture stream, so a rank's WHOLE data-parallel step -- forward, backward, gradient
    exchange, decoder backward, clip + Adam -- is ONE hipGraph replay instead of two or three graphs with eager torch.distributed
    collectives in between.  Returns the communicator (created once per process) or None."""
    if os.environ.get("HOS_HOSCOMM", "0") != "1":
        return None
    if "c" not in _HOSCOMM:
        from hosnerf_amd import comm, train
        _HOSCOMM["c"] = comm.HosComm(rank, world)
        train.use_hoscomm(_HOSCOMM["c"])
    return _HOSCOMM["c"]


def _maybe_shard_decoder(net, rank, world):
    """HOS_SHARD_DECODER=1 (opt-in, N > 1): the volume decoder's first three transposed convolutions sharded over the ranks by input
    channel (`Network.shard_decoder`; their collectives through libhoscomm when HOS_HOSCOMM=1, else torch.distributed -- then the
    step cannot be captured and runs eagerly).  Must run before the optimiser is built."""
    if world > 1 and os.environ.get("HOS_SHARD_DECODER", "0") == "1":
        from hosnerf_amd.train import ShardComm
        net.shard_decoder(ShardComm(rank, world, hos=hoscomm(rank, world)))
    elif world == 1 and model_shard() > 1:
        net.shard_decoder(_ModelComm(model_shard()))


def model_shard() -> int:
    """HOS_MODEL_SHARD=N on ONE GPU: a TIMING MODEL of rank 0's share of an N-rank step with the sharded volume decoder -- this
    process computes 1/N of the decoder's first three layers and updates 1/N of their parameters, and the two collectives of the
    sharded decoder are replaced by identities (so the rendered values are NOT the model's: the line is labelled and never the
    headline).  What it shows: the per-rank work of the strong-scaling point without the communication."""
    return int(os.environ.get("HOS_MODEL_SHARD", "0") or 0)


class _ModelComm:
    """rank 0 of `world`, no peers: all_reduce_sum = identity, all_gather = this rank's piece repeated (timing model only)."""

    def __init__(self, world):
        self.rank, self.world, self.group, self.hos = 0, int(world), None, None

    def all_reduce_sum(self, t):
        return t

    def all_gather(self, send):
        return send.contiguous().unsqueeze(0).expand(self.world, *send.shape).contiguous()


def _reduce_human(net, opt, static_g=None):
    """The human network's exchange: the volume gradient (3.5 MB) + every parameter outside the volume decoder (4.3 MB).
    `static_g`: the volume-gradient tensor of a captured step (its address is fixed by the graph's memory pool)."""
    import torch.distributed as dist
    from hosnerf_amd import train
    g = static_g if static_g is not None else net.pending_volume_grad()
    if g is not None and train._HOS_COMM is not None:
        train._HOS_COMM.all_reduce(g, average=False)
    elif g is not None and dist.is_available() and dist.is_initialized() and dist.get_world_size(opt.group) > 1:
        dist.all_reduce(g, group=opt.group)
    train.allreduce_flat_grad(net, opt.group, net.reduce_ranges())


def _reduce_human_begin(net, opt, static_g=None):
    """Async form of `_reduce_human`: the volume gradient first (the decoder's backward waits for it alone), then the other spans."""
    import torch.distributed as dist
    from hosnerf_amd.train import allreduce_flat_grad_async
    g = static_g if static_g is not None else net.pending_volume_grad()
    hv = None
    if g is not None and dist.is_available() and dist.is_initialized() and dist.get_world_size(opt.group) > 1:
        hv = dist.all_reduce(g, group=opt.group, async_op=True)
    rest = allreduce_flat_grad_async(net, opt.group, net.reduce_ranges())
    return hv, rest


class Stage2(Workload):
    name, scaling = "stage2", "strong"
    describe = ("BASELINE configs[2]: stage-2 human-object network (pose refiner + motion bases + volume decoder, backward LBS, "
                "non-rigid 6x128 + canonical 8x256 MLPs, flow + cycle sets, in-network composite), 128 samples/ray, 2 states")

    def __init__(self, dev, rank, world, rays_global):
        from hosnerf_amd import synth
        from hosnerf_amd.human_nerf import Network, default_cfg
        from hosnerf_amd.train import FusedAdam, batch_to_device, human_lr_ranges
        self.rays_global, self.rays_local = rays_global, rays_global // world
        cfg = default_cfg(basedir())
        cfg.perturb = 1.0
        cfg.chunk = max(cfg.chunk, self.rays_local)
        self.net = Network(cfg, stage=2)
        self.net.load_state_dict(synth.human_state_dict(777, 2), strict=True)
        self.net = self.net.to(dev)
        _maybe_shard_decoder(self.net, rank, world)
        self.host_item, prepared = _human_item(self.rays_local, rank, 2)
        self.batch = batch_to_device(prepared, dev)      # control scalars (time, iter_val) stay on the host
        self.opt = FusedAdam(self.net, lr=6.667e-4, lr_ranges=human_lr_ranges(self.net, 6.667e-4, 6.667e-5), max_grad_norm=GRAD_MAX_NORM)

    def opts(self):
        return [self.opt]

    def lr(self, i):
        from hosnerf_amd.train import human_lr_decay
        return 6.667e-4 * human_lr_decay(300000 + i)

    def host_prepare(self, i):
        pass

    def fwd_bwd(self, i):
        from hosnerf_amd.train import stage2_losses
        self.opt.zero_grad()
        self.net.split_decoder_backward = True          # the 253 MB decoder gradient is reduced at the decoder's 3.5 MB output
        out = self.net(static_cycle=True, **self.batch)
        self.cycle_count = out.get("cycle_count")
        self.last_rgb = out["rgb"].detach()
        loss, _ = stage2_losses(out, self.batch)
        loss.backward()
        return loss.detach()

    def outputs(self):
        return {"rgb": self.last_rgb, "params_human": self.net.flat_param}

    def reduce(self):
        _reduce_human(self.net, self.opt, self.static_vol_grad)

    def freeze_static(self):
        self.static_vol_grad = self.net.pending_volume_grad()

    def finish(self, i, dynamic):
        self.net.finish_decoder_backward()
        Workload.finish(self, i, dynamic)

    overlap = True

    def reduce_begin(self):
        hv, rest = _reduce_human_begin(self.net, self.opt, self.static_vol_grad)
        if hv is not None:
            hv.wait()
        return rest

    def finish_decoder(self):
        self.net.finish_decoder_backward()


class Stage3(Workload):
    name, scaling = "stage3", "strong"
    describe = ("BASELINE configs[3]: stage-3 full HOSNeRF (mip-NeRF-360 background 64/64/32 samples + human-object branch 128 "
                "samples + 160-sample z-merged composite), 4096 rays/batch GLOBAL, DDP over ray shards")

    def __init__(self, dev, rank, world, rays_global):
        from hosnerf_amd import synth
        from hosnerf_amd.hosnerf import HOSNeRF
        from hosnerf_amd.human_nerf import default_cfg
        from hosnerf_amd.train import FusedAdam, GradClip, batch_to_device, human_lr_ranges
        self.rays_global, self.rays_local = rays_global, rays_global // world
        cfg = default_cfg(basedir())
        cfg.perturb = 1.0
        cfg.chunk = max(cfg.chunk, self.rays_local)
        self.hos = HOSNeRF(cfg)
        self.hos.model.load_state_dict(synth.background_state_dict(777, 2), strict=False)
        self.hos.human.load_state_dict(synth.human_state_dict(777, 2), strict=True)
        self.hos = self.hos.to(dev)
        _maybe_shard_decoder(self.hos.human, rank, world)
        self.host_item, prepared = _human_item(self.rays_local, rank, 3)
        self.batch = batch_to_device(prepared, dev)
        clip = GradClip(GRAD_MAX_NORM)      # ONE norm over both modules: the reference has a single Adam over both (optimizer.py:19-60)
        self.ob = FusedAdam(self.hos.model, lr=6.667e-5, clip=clip)
        self.oh = FusedAdam(self.hos.human, lr=6.667e-5, lr_ranges=human_lr_ranges(self.hos.human), clip=clip)

    def opts(self):
        return [self.ob, self.oh]

    def lr(self, i):
        from hosnerf_amd.train import human_lr_decay
        return 6.667e-5 * human_lr_decay(300000 + i)

    def host_prepare(self, i):
        pass

    def fwd_bwd(self, i):
        from hosnerf_amd.train import stage3_losses
        self.ob.zero_grad()
        self.oh.zero_grad()
        self.hos.human.split_decoder_backward = True
        out = self.hos.render(self.batch, randomized=True, is_train=True, static_cycle=True)
        self.cycle_count = out.get("cycle_count")
        self.last_rgb = out["rgb"].detach()
        loss, _ = stage3_losses(out, self.batch)
        loss.backward()
        return loss.detach()

    def outputs(self):
        return {"rgb": self.last_rgb, "params_background": self.hos.model.flat_param, "params_human": self.hos.human.flat_param}

    def reduce(self):
        from hosnerf_amd.train import allreduce_flat_grad
        allreduce_flat_grad(self.hos.model, self.ob.group)
        _reduce_human(self.hos.human, self.oh, self.static_vol_grad)

    def freeze_static(self):
        self.static_vol_grad = self.hos.human.pending_volume_grad()

    def finish(self, i, dynamic):
        self.hos.human.finish_decoder_backward()
        Workload.finish(self, i, dynamic)

    overlap = True

    def reduce_begin(self):
        from hosnerf_amd.train import allreduce_flat_grad_async
        hv, rest = _reduce_human_begin(self.hos.human, self.oh, self.static_vol_grad)     # volume gradient first: it gates the decoder
        rest += allreduce_flat_grad_async(self.hos.model, self.ob.group)
        if hv is not None:
            hv.wait()
        return rest

    def finish_decoder(self):
        self.hos.human.finish_decoder_backward()


class Stage3LPIPS(Stage3):
    """The stage-3 step WITH the reference's LPIPS term (weight 1.0; `hosnerf_amd.lpips`): what the term costs per step.  The VGG-16
    filters are He-normal random (torchvision's ImageNet weights are a download) and so are the calibration weights: a timing leg."""
    name = "stage3_with_lpips"
    describe = ("stage-3 step at 4096 rays + 1.0 x LPIPS(net='vgg') on the four unpacked 32x32 patches (forward of prediction and target "
                "through VGG-16 relu1_2..relu5_3, input gradient of the prediction; random filters: timing only)")

    def __init__(self, dev, rank, world, rays_global):
        from hosnerf_amd.lpips import LPIPS, VGG16_CFG, CHNS, patch_ray_index
        Stage3.__init__(self, dev, rank, world, rays_global)
        g = torch.Generator().manual_seed(4321)
        sd, cin, idx = {}, 3, 0
        for v in VGG16_CFG:
            if v == "M":
                idx += 1
                continue
            sd[f"{idx}.weight"] = torch.randn(v, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
            sd[f"{idx}.bias"] = torch.zeros(v)
            cin, idx = v, idx + 2
        self.lpips = LPIPS().load_vgg16_features(sd, dev).load_lin(torch.rand(sum(CHNS), generator=g) * 0.1, dev)
        self.batch["patch_ray_idx"] = patch_ray_index(self.batch["patch_masks"].to(dev))

    def fwd_bwd(self, i):
        from hosnerf_amd.train import stage3_losses
        self.ob.zero_grad()
        self.oh.zero_grad()
        self.hos.human.split_decoder_backward = True
        out = self.hos.render(self.batch, randomized=True, is_train=True, static_cycle=True)
        self.cycle_count = out.get("cycle_count")
        self.last_rgb = out["rgb"].detach()
        loss, _ = stage3_losses(out, self.batch, lpips=self.lpips)
        loss.backward()
        return loss.detach()


class Stage3Fresh(Stage3):
    """The stage-3 step with a NEW training item every step: a synthetic scene directory in the reference's
    on-disk formats (`synth.write_scene_dir`) -> `dataset.SceneItems` builds each item on the device (two camera ray sets,
    radii, the subject's box test, the random patch gather: hos_rays.hip + torch index ops; 26-joint pose algebra on the host)
    -> the item's tensors are copied into the static batch of the captured step.  Everything `items[i]` does is inside the
    timed region; the headline leg replays ONE resident batch instead."""
    name = "stage3_fresh_items"
    describe = ("stage-3 step at 4096 rays with the training item REBUILT every step from a scene directory (device-side rays / "
                "box test / patch gather of dataset.SceneItems + copy into the captured step's batch), 192x192 synthetic frames")

    def __init__(self, dev, rank, world, rays_global):
        import shutil
        import tempfile
        from hosnerf_amd import formats, synth
        from hosnerf_amd.dataset import SceneItems
        Stage3.__init__(self, dev, rank, world, rays_global)
        self.scene = tempfile.mkdtemp(prefix="hos_bench_scene_")
        try:
            H = W = 192
            px = synth.write_scene_dir(self.scene, 16, H, W, seed=777)
            formats.load_scene(self.scene, (H, W), masks=px["alphas"], near=0.1, far=1e6)
            n_patches = max(1, self.rays_local // 1024)
            self.ds = SceneItems(self.scene, px["images"], px["alphas"], px["flows"], n_patches=n_patches, patch_size=32, device=dev,
                                 seed=777 + rank, bgcolor=[0.0, 0.0, 0.0])
        finally:
            shutil.rmtree(self.scene, ignore_errors=True)
        # frames 8..15 lie behind the transition time 0.4 of the synthetic base directory: one state, flow supervision on
        self.frames = list(range(8, 16))
        first = self.ds[self.frames[0]]
        drop = {"frame_name", "img_width", "img_height", "ray_mask", "ray_mask_bkg", "patch_div_indices", "rays_o_bkg_only",
                "rays_d_bkg_only", "viewdirs_bkg_only", "radii_bkg_only"}
        self.batch = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in first.items() if k not in drop}
        self.batch["iter_val"] = 3e5
        self.item_bytes = sum(v.numel() * v.element_size() for v in self.batch.values() if isinstance(v, torch.Tensor))

    def host_prepare(self, i):
        # the item is built on a side stream: SceneItems reads two candidate counts back per item, and on the step's stream that
        # read would wait for the previous step's whole replay
        if not hasattr(self, "side"):
            self.side = torch.cuda.Stream()
        with torch.cuda.stream(self.side):
            item = self.ds[self.frames[i % len(self.frames)]]
        torch.cuda.current_stream().wait_stream(self.side)
        for k, dst in self.batch.items():
            if isinstance(dst, torch.Tensor) and dst is not item.get(k):
                dst.copy_(item[k], non_blocking=True)
                item[k].record_stream(torch.cuda.current_stream())


# ------------------------------------------------------------------------------------------------ timing
DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(dirname, tensors):
    """--dump-outputs: every tensor as <dirname>/<name>.npy, float32.  All files together stay under DUMP_BUDGET_BYTES: an
    array over its equal share of the budget is written as a fixed sample of its elements (indices drawn once from a seeded
    generator, ascending, the same for every run and every build; they are stored next to it as <name>.index.npy, float64).
    Inputs and draws repeat exactly; the outputs of two runs of ONE build still differ in their last bits, because the steps' slab
    reductions add with floating-point atomics and 25 optimiser steps carry that on: measured at 20 + 5 steps of stage 3, loss
    within 1e-6, parameters within 1e-5, colours within 2e-4 on the median ray (a ray whose sample crosses a proposal bin: up to 4e-2)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    cap = DUMP_BUDGET_BYTES // (16 * len(tensors))        # elements per array: 4 B per value + 8 B per index, and headroom
    for name, t in tensors.items():
        t = t.detach()
        if t.numel() > cap:
            idx = torch.randint(t.numel(), (cap,), generator=torch.Generator().manual_seed(777)).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
            np.save(os.path.join(dirname, name + ".index.npy"), idx.to(torch.float64).numpy())
        np.save(os.path.join(dirname, name + ".npy"), t.to(torch.float32).cpu().numpy())


def run_workload(wl, args, dev, rank, world, dist, want_events, dump_dir=None):
    """Warm up, capture, time exactly args.steps steps between barriers; returns (seconds [max over ranks], info dict).  `dump_dir`:
    after the timed steps, the outputs of the last one are written there (`dump_outputs`)."""
    from hosnerf_amd import ops

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for i in range(args.warmup):
        wl.host_prepare(i)
        wl.eager_step(i)
    barrier()
    f_cyc = wl.f_cyc() if args.warmup > 0 else None          # read once, after warm-up, before anything is captured or timed
    graph, graph2, graph3, static_loss, launch, overlap = None, None, None, None, "eager", False
    # torch.distributed's collectives stay outside the captured region (two or three graphs with the eager collectives in between);
    # through libhoscomm (HOS_HOSCOMM=1) they are stream work like any kernel and the whole step is one graph
    in_graph_comm = world > 1 and hoscomm(rank, world) is not None
    full_graph = world == 1 or in_graph_comm
    second_half = None
    # a decoder sharded over torch.distributed has its per-layer collectives INSIDE the forward: nothing to capture (HOS_HOSCOMM=1 moves
    # them onto the stream and the whole step into one graph)
    shard_eager = world > 1 and os.environ.get("HOS_SHARD_DECODER", "0") == "1" and not in_graph_comm
    if shard_eager:
        launch = "eager (volume decoder sharded over torch.distributed: its collectives sit inside the forward; HOS_HOSCOMM=1 captures them)"
    if not args.no_graph and not shard_eager:
        # N > 1: first the overlapped second half (async collectives), then the sequential one, then eager launches
        want_overlap = (not full_graph) and wl.overlap and os.environ.get("HOS_BENCH_OVERLAP", "1") == "1"
        for try_overlap in ([True, False] if want_overlap else [False]):
            try:
                for o in wl.opts():
                    o.set_step_hyper(wl.lr(args.warmup))
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):
                        wl.fwd_bwd(args.warmup)
                        wl.reduce()
                        wl.finish(args.warmup, True)
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                # thread_local: the RCCL watchdog thread of a multi-rank run may touch the runtime while this thread captures
                mode = "thread_local" if world > 1 else "global"
                with torch.cuda.graph(graph, capture_error_mode=mode):
                    static_loss = wl.fwd_bwd(args.warmup)
                    if full_graph:
                        if in_graph_comm:
                            wl.reduce()                    # RCCL on the capture stream (libhoscomm)
                        wl.finish(args.warmup, True)
                overlap = try_overlap
                if not full_graph:
                    wl.freeze_static()
                    if overlap:
                        for h in wl.reduce_begin():
                            h.wait()
                        torch.cuda.synchronize()           # nothing of the exchange is in flight while the next graphs are captured
                        graph2 = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(graph2, pool=graph.pool(), capture_error_mode=mode):
                            wl.finish_decoder()
                        graph3 = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(graph3, pool=graph.pool(), capture_error_mode=mode):
                            wl.finish_optim(args.warmup, True)
                    else:
                        wl.reduce()
                        torch.cuda.synchronize()
                        graph2 = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(graph2, pool=graph.pool(), capture_error_mode=mode):
                            wl.finish(args.warmup, True)

                def second_half():
                    if overlap:
                        pending = wl.reduce_begin()         # all collectives enqueued; the volume gradient has arrived
                        graph2.replay()                     # decoder backward under the remaining exchange
                        for h in pending:
                            h.wait()
                        graph3.replay()                     # Adam on the reduced gradients
                    else:
                        wl.reduce()
                        graph2.replay()

                for _ in range(2):
                    for o in wl.opts():
                        o.set_step_hyper(wl.lr(args.warmup))
                    graph.replay()
                    if not full_graph:
                        second_half()
                torch.cuda.synchronize()
                launch = ("hipGraph replay (collectives inside the graph: libhoscomm / RCCL)" if in_graph_comm else "hipGraph replay" if full_graph else
                          "hipGraph replay (fwd+bwd) + async all-reduces + hipGraph replay (decoder bwd, under the exchange) + hipGraph replay (Adam)" if overlap else
                          "hipGraph replay (fwd+bwd) + eager all-reduce + hipGraph replay (decoder bwd + Adam)")
                break
            except Exception as e:      # fall back (sequential second half, then eager launches), and say so on stderr / in the JSON
                print(f"[bench] {wl.name}: graph capture failed ({type(e).__name__}: {e}) with overlap={try_overlap}; "
                      + ("retrying without the overlapped exchange" if try_overlap else "running eagerly"), file=sys.stderr)
                graph, launch = None, "eager"
                torch.cuda.synchronize()
                ops.clear_last_error()          # the invalidated capture's sticky error must not be reported by the next (eager) launch
    h2d, h2d_bytes = None, 0
    if getattr(args, "h2d", False):
        # the item as a data loader hands it over: pinned host tensors, copied into the (static) device batch every step
        h2d = [(v, v.detach().cpu().pin_memory()) for v in wl.batch.values() if isinstance(v, torch.Tensor) and v.is_cuda]
        h2d_bytes = sum(h.numel() * h.element_size() for _, h in h2d)
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step = args.warmup + i
        wl.host_prepare(step)
        if h2d is not None:
            for dst, src in h2d:
                dst.copy_(src, non_blocking=True)
        if graph is not None:
            for o in wl.opts():
                o.set_step_hyper(wl.lr(step))
            graph.replay()
            if not full_graph:
                second_half()
            loss = static_loss
        else:
            loss = wl.eager_step(step)
    barrier()
    dt = time.perf_counter() - t0
    tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax)
    info = {"launch": launch, "final_loss": float(loss.detach()), "f_cyc": wl.f_cyc() if f_cyc is None else f_cyc}
    if dump_dir and rank == 0:
        dump_outputs(dump_dir, {"loss": loss.detach(), **wl.outputs()})
    if getattr(getattr(wl, "hos", None), "two_streams", False):
        info["launch"] += "; background branch and human branch on two streams inside the graph"
    if h2d is not None:
        info["h2d_bytes_per_step"] = h2d_bytes
    table = None
    if want_events and rank == 0:
        # per-kernel HIP-event timing cannot be recorded inside a captured graph: time the same steps eagerly right after
        # the timed region (same kernels, same shapes; rocprofv3 --stats of this command agrees)
        # ... in the ONE-stream order: a (start, stop) event pair around a launch measures that kernel only if nothing of the
        # other branch shares the GPU with it (the timed step runs the two branches on two streams)
        hos = getattr(wl, "hos", None)
        two = getattr(hos, "two_streams", False)
        if hos is not None:
            hos.two_streams = False
        prof = ops.KernelEvents()
        ops.set_kernel_events(prof)
        for i in range(min(args.steps, 3)):
            wl.fwd_bwd(args.warmup + args.steps + i)       # rank-local: no collective outside the timed region
        torch.cuda.synchronize()
        ops.set_kernel_events(None)
        if hos is not None:
            hos.two_streams = two
        table = prof.summary()
    return dt, info, table


def source_hash(*rel):
    h = hashlib.sha256()
    for r in rel:
        with open(os.path.join(ROOT, r), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def roofline_of(table, gemm):
    """The dominant GEMM launch of the step against the MFMA peak of the arithmetic it uses.  `traffic` (HBM bytes per launch, PMC)
    comes from the committed rocprofv3 --pmc pass of the same kernel and shape (scripts/pmc_gemmp.sh) and is reported only
    if that pass was made on the kernel sources this library was built from; null otherwise."""
    if not table:
        return None
    dom = max(table, key=lambda r: r["total_ms"])
    traffic = None
    # the newest committed PMC pass whose kernel sources are the ones this library was built from
    for tname in ("r06_pmc_gemmp_traffic.json", "r05_pmc_gemmp_traffic.json", "r04_pmc_gemmp_traffic.json", "r03_pmc_gemmp_traffic.json"):
        tpath = os.path.join(ROOT, "profiles", tname)
        if not os.path.exists(tpath) or traffic is not None:
            continue
        with open(tpath) as f:
            tj = json.load(f)
        if tj.get("source_hash") == source_hash("hosnerf_amd/csrc/hos_gemmp.hip", "hosnerf_amd/csrc/hos_gemm_common.h", "Makefile"):
            traffic = tj.get("kernels", {}).get(dom["kernel"], {}).get("hbm_bytes_per_launch")
    peak = FP32_MFMA_PEAK_TFLOPS if gemm == "fp32" else SPLIT_MFMA_PEAK_TFLOPS
    return {"bound": "mfma", "achieved": dom["tflops"], "peak": peak, "unit": "TFLOP/s", "frac": dom["tflops"] / peak,
            "traffic": traffic, "kernel": dom["kernel"], "launches": dom["launches"], "avg_us": dom["avg_us"],
            "flop_per_launch": dom["flop_per_launch"]}


# ------------------------------------------------------------------------------------------------ config 5: 1080p inference
def infer_1080p(dev, rank, world, dist, want_events, height=1080, width=1920, chunk=65536):
    """BASELINE configs[4] / SURVEY 8(d).5: one whole synthetic 1920x1080 free-viewpoint frame through `eval.render_frame` -- the
    reference's `free_view` loop (3rd_.../src/model/mipnerf360/model.py:1293-1494): rays through the subject's box take both
    branches + the 160-sample z-merged composite, the others the background model + 32-sample composite; the frame's ray set-up
    (two camera ray sets, radii, box test: `eval.frame_rays`) is inside the timed region.  N > 1: every rank renders a
    contiguous share of both ray lists, one RGB all-gather per list (strong scaling).  One warm-up frame, one timed frame
    (barrier + synchronize on both sides, max over ranks); then, on rank 0, one more frame under per-launch HIP events for the
    dominant forward kernel's roofline fraction."""
    from hosnerf_amd import eval as ev, ops, synth
    from hosnerf_amd.hosnerf import HOSNeRF
    from hosnerf_amd.human_nerf import default_cfg
    cfg = default_cfg(basedir())
    cfg.chunk = min(max(chunk, int(cfg.chunk)), 32768)      # human inner chunk: 32768 rays x 128 samples = 4.3 GB per activation
    hos = HOSNeRF(cfg)
    hos.model.load_state_dict(synth.background_state_dict(777, 2), strict=False)
    hos.human.load_state_dict(synth.human_state_dict(777, 2), strict=True)
    hos = hos.to(dev)
    hb = synth.human_batch(8, seed=2, time=0.5, is_train=False, iter_val=3e5)
    K, E, Ec = synth.eval_camera(height, width, hb)
    bbox = {"min_xyz": hb["dst_bbox_min_xyz"].numpy(), "max_xyz": hb["dst_bbox_max_xyz"].numpy()}
    per_frame = {k: (hb[k].to(dev) if isinstance(hb[k], torch.Tensor) else hb[k]) for k in ev.FRAME_KEYS}
    group = dist.group.WORLD if world > 1 else None

    def one_frame():
        fr = ev.frame_rays(height, width, K, E, bbox, Ec, device=dev)
        fr.update(per_frame)
        return fr, ev.render_frame(hos, fr, chunk_bkg=chunk, group=group)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    one_frame()
    barrier()
    t0 = time.perf_counter()
    fr, img = one_frame()
    barrier()
    dt = time.perf_counter() - t0
    tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax)
    n_rays = height * width
    n_fg = int(fr["ray_mask"].sum())
    flops = (n_rays - n_fg) * FWD_FLOP_BG + n_fg * FWD_FLOP_FG
    res = {"workload": f"BASELINE configs[4]: stage-3 free-viewpoint inference, one synthetic {width}x{height} frame "
                       f"({n_rays} rays, {n_fg / n_rays:.3f} of them through the subject's box), {chunk}-ray chunks, forward only",
           "value": n_rays / dt, "unit": "rays/s", "frames_per_s": 1.0 / dt, "ms_per_frame": 1e3 * dt, "scaling": "strong",
           "n_gpus": world, "rays_per_gpu": (n_rays + world - 1) // world, "foreground_fraction": n_fg / n_rays,
           "algorithmic_tflops": flops / dt / 1e12, "frac_of_split_mfma_peak": flops / dt / 1e12 / (SPLIT_MFMA_PEAK_TFLOPS * world),
           "finite": bool(torch.isfinite(img).all())}
    if want_events and rank == 0 and world == 1:
        prof = ops.KernelEvents()
        ops.set_kernel_events(prof)
        one_frame()
        torch.cuda.synchronize()
        ops.set_kernel_events(None)
        table = prof.summary()
        if table:
            dom = max(table, key=lambda r: r["total_ms"])
            res["roofline"] = {"bound": "mfma", "achieved": dom["tflops"], "peak": SPLIT_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": dom["tflops"] / SPLIT_MFMA_PEAK_TFLOPS, "traffic": None, "kernel": dom["kernel"],
                               "launches": dom["launches"], "avg_us": dom["avg_us"], "flop_per_launch": dom["flop_per_launch"],
                               "measured": "HIP events per launch over one extra (untimed) frame"}
            res["kernels"] = table[:6]
    del hos
    torch.cuda.empty_cache()
    return res


# ------------------------------------------------------------------------------------------------ baseline legs
def _time_steps(step, warm, budget_s, max_n, sync=None):
    for _ in range(warm):
        step()
    if sync:
        sync()
    t0 = time.perf_counter()
    n = 0
    while True:
        step()
        n += 1
        if sync:
            sync()
        if time.perf_counter() - t0 > budget_s or n >= max_n:
            break
    return (time.perf_counter() - t0) / n, n


def _median_step(step, warm, n):
    """`warm` untimed steps, then the MEDIAN of `n` individually timed steps (seconds)."""
    for _ in range(warm):
        step()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        step()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2], ts


def cpu_baseline(stage: str, device=None, rays: int = 0):
    """THE BASELINE LEG -- the only place this file touches oracle/: the oracle (torch fp32 restatement of the reference's op
    graph, autograd backward, torch Adam) timed as the reference would run,
      * device=None: on the host cores, on a bounded sample of the workload (the `cpu_baseline` object), and
      * device=cuda: the same op graph as plain PyTorch-ROCm ops on this GPU (fp32 rocBLAS / MIOpen kernels) -- what the
        reference does on this hardware, the denominator of the north-star's ">= 10x the reference PyTorch path".
    Never the product path: nothing measured as `value` runs through here."""
    import oracle.steps as osteps
    from hosnerf_amd import synth
    on_gpu = device is not None
    dev = device if on_gpu else "cpu"
    if not on_gpu:
        # torch's CPU GEMMs stop scaling (and oversubscribe badly) far below the hardware threads of the GPU host: try a few
        # thread counts on a 64-ray item, keep the fastest, and report exactly that next to the CPU model and the thread count
        # the host offers
        host_threads = os.cpu_count() or 1
        rays = 256 if stage == "stage1" else 512
    if stage == "stage1":
        step = osteps.stage1_step(synth.background_state_dict(777, 2), synth.stage1_batch(rays, seed=777), device=dev)
    else:
        b = synth.add_patch_supervision(synth.human_batch(rays, seed=777, time=0.5, is_train=True, iter_val=3e5), max(1, rays // 1024), 32, 777)
        if stage == "stage2":
            step = osteps.stage2_step(synth.human_state_dict(777, 2), b, device=dev)
        else:
            step = osteps.stage3_step(synth.background_state_dict(777, 2), synth.human_state_dict(777, 2), b, device=dev)
    if not on_gpu:
        sweep, cores = {}, 1
        tb = synth.add_patch_supervision(synth.human_batch(64, seed=778, time=0.5, is_train=True, iter_val=3e5), 1, 32, 778)
        # Thread sweep 8 ... 64 in every run; 128 and ALL hardware threads only with HOS_CPU_SWEEP_ALL=1: at 256 threads torch's
        # intra-op pool oversubscribes so badly (0.3 rays/s against 110 at 16, measured in round 4) that the one 64-ray step of the
        # sweep takes minutes, which the default run (a few minutes in total) cannot afford.
        counts = (8, 16, 32, 64) + ((128, host_threads) if os.environ.get("HOS_CPU_SWEEP_ALL") else ())
        for th in sorted({min(host_threads, c) for c in counts}):
            torch.set_num_threads(th)
            if stage == "stage1":
                st = osteps.stage1_step(synth.background_state_dict(777, 2), synth.stage1_batch(64, seed=778), device="cpu")
            elif stage == "stage2":
                st = osteps.stage2_step(synth.human_state_dict(777, 2), tb, device="cpu")
            else:
                st = osteps.stage3_step(synth.background_state_dict(777, 2), synth.human_state_dict(777, 2), tb, device="cpu")
            dts, _ = _time_steps(st, 1, 1.5, 2)
            sweep[str(th)] = round(64 / dts, 1)
            del st
        cores = int(max(sweep, key=lambda k: sweep[k]))
        env = os.environ.get("HOS_CPU_THREADS")
        if env:
            cores = min(host_threads, int(env))
        torch.set_num_threads(cores)
    if on_gpu:
        dt, n = _time_steps(step, 1, 4.0, 5, sync=torch.cuda.synchronize)
        del step
        torch.cuda.empty_cache()
        return {"value": rays / dt, "unit": "rays/s", "rays": rays, "steps": n,
                "what": "the reference's op graph (oracle restatement) as PyTorch-ROCm ops on the same GPU: fp32 rocBLAS, autograd, torch Adam"}
    dt, ts = _median_step(step, 1, 5)
    n = len(ts)
    full = {"stage1": 1024, "stage2": 2048, "stage3": GLOBAL_RAYS_S3}[stage]
    return {"value": rays / dt, "unit": "rays/s", "cores": cores, "kind": "port", "workload": stage,
            "cpu_model": cpu_model(), "host_threads": host_threads, "thread_sweep_rays_per_s": sweep,
            "step_seconds": [round(t, 3) for t in ts],
            "sample": f"1 warm-up + MEDIAN of {n} timed steps of {rays} rays (same model/losses/optimizer, torch CPU fp32, {cores} threads = the fastest of "
                      f"the thread counts tried on a 64-ray item, rays/s per count: {sweep}; all {host_threads} hardware threads: 0.3 rays/s, "
                      f"measured in round 4, re-measured with HOS_CPU_SWEEP_ALL=1).  The full {full}-ray item was not run: at "
                      f"this rate one step of it takes about {dt * full / rays:.0f} s (per-ray cost constant; its per-step work -- volume "
                      f"decoder, Adam over all parameters -- is already inside every timed sample step)"}


def cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or "unknown"


# ------------------------------------------------------------------------------------------------ main
def main():
    args = parse()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback); use tests -m 'not gpu' on CPU")
    # HOS_BENCH_ONE_GPU=1 (testing only): all ranks share cuda:0 and exchange through gloo, so the multi-rank code
    # path (graph replay + eager all-reduce, max-over-ranks timing) can be exercised on a 1-GPU box
    one_gpu = os.environ.get("HOS_BENCH_ONE_GPU") == "1"
    if one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if one_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    # every draw of the steps (sample jitter, t_rand) comes from torch's default generators, which start each process from a seed of
    # their own: seeded here, so that a run repeats its inputs exactly
    torch.manual_seed(777 + rank)

    from hosnerf_amd import ops
    ops.set_gemm_mode({"planes": ops.GEMM_PLANES, "split": ops.GEMM_BF16X3, "fp32": ops.GEMM_FP32}[args.gemm])

    def make(name, rays_global=None):
        if name == "stage1":
            return Stage1(dev, rank, world, args.rays if (args.rays and args.primary == "stage1") else 1024)
        g = rays_global or (args.rays if (args.rays and args.primary == name) else (GLOBAL_RAYS_S3 if name == "stage3" else 2048))
        if g % world:
            raise SystemExit(f"{g} global rays do not divide over {world} ranks")
        if name == "stage3_with_lpips":
            return Stage3LPIPS(dev, rank, world, args.rays if (args.rays and args.primary == "stage3") else GLOBAL_RAYS_S3)
        if name == "stage3_fresh_items":
            return Stage3Fresh(dev, rank, world, args.rays if (args.rays and args.primary == "stage3") else GLOBAL_RAYS_S3)
        return (Stage3 if name == "stage3" else Stage2)(dev, rank, world, g)

    def measure(name, events, rays_global=None, describe=None, run_args=None, dump_dir=None):
        wl = make(name, rays_global)
        if describe is not None:
            wl.describe = describe
        dt, info, table = run_workload(wl, run_args or args, dev, rank, world, dist, events, dump_dir)
        steps = (run_args or args).steps
        rays_total = wl.rays_global * steps
        fkey = "stage3" if name in ("stage3_fresh_items", "stage3_with_lpips") else name
        flop_ray = FLOP_PER_RAY[fkey][0] + FLOP_PER_RAY[fkey][1] * info["f_cyc"]
        res = {"value": rays_total / dt, "unit": "rays/s", "ms_per_step": 1e3 * dt / steps, "scaling": wl.scaling,
               "rays_per_gpu": wl.rays_local, "global_rays": wl.rays_global, "workload": wl.describe,
               "grad_max_norm": GRAD_MAX_NORM, "flop_per_ray": flop_ray,
               "algorithmic_tflops": rays_total * flop_ray / dt / 1e12, **info}
        del wl
        torch.cuda.empty_cache()
        return res, table

    def guarded(label, fn, limit_s=240.0):
        """A secondary leg can never cost the primary line: exceptions become {"error": ...}; a leg that HANGS (a collective some rank
        never reaches) is cut by a watchdog on every rank -- rank 0 prints the line it has (primary + the legs finished so far, this leg
        marked "timed out") and the process exits 0, so the driver still gets its one JSON line."""
        import threading

        def fire():
            if rank == 0:
                stages[label] = {"error": f"timed out after {limit_s:.0f} s (watchdog; the legs after it were not run)"}
                emit()
            sys.stdout.flush()
            os._exit(0)

        t = threading.Timer(limit_s, fire)
        t.daemon = True
        t.start()
        # ... and a leg that KILLS the process (abort() inside RCCL, a fault in a captured collective, the launcher's SIGTERM after
        # another rank died) leaves the same line as its last words (libhoscomm's signal handlers; multi-rank legs only)
        armed = False
        if world > 1:
            try:
                from hosnerf_amd import comm as _comm
                snap = dict(out)
                snap["stages"] = dict(stages, **{label: {"error": "the process was killed by a signal inside this leg (the legs after it were not run)"}})
                armed = _comm.crash_line_set((json.dumps(snap) + "\n") if rank == 0 else "")
            except Exception:
                armed = False
        try:
            return fn()
        except Exception as e:
            torch.cuda.synchronize()
            try:
                ops.clear_last_error()
            except Exception:
                pass
            return {"error": f"{type(e).__name__}: {e}"}
        finally:
            t.cancel()
            if armed:
                _comm.crash_line_clear()

    events = not args.no_kernel_events
    stages, out, emitted = {}, {}, []

    def emit():
        """THE one JSON line (rank 0), printed once: at the end of main, or by a leg's watchdog."""
        if rank != 0 or emitted:
            return
        emitted.append(True)
        if stages:
            out["stages"] = stages
        print(json.dumps(out), flush=True)

    # ---- who is here: proof that the gradient communicator saw N ranks on N devices -- an all-reduce of ones
    # over the group the flat gradients are exchanged on, and every rank's device name
    comm_info = {"backend": "none (single process)", "rccl_ranks_seen": 1, "devices": [torch.cuda.get_device_name(dev)]}
    if world > 1:
        ones = torch.ones(1, device=dev)
        dist.all_reduce(ones)
        names = [None] * world
        dist.all_gather_object(names, f"rank {rank}: cuda:{local_rank} {torch.cuda.get_device_name(dev)}")
        comm_info = {"backend": dist.get_backend() + (" (gloo stands in for RCCL: HOS_BENCH_ONE_GPU=1, all ranks on one device, testing only)"
                                                       if one_gpu else " (= RCCL on ROCm)"),
                     "rccl_ranks_seen": int(ones.item()), "devices": names}

    prim, table = measure(args.primary, events, dump_dir=args.dump_outputs)
    if rank == 0:
        out.update({
            "metric": f"train rays/sec ({args.primary}: forward + losses + backward + gradient all-reduce + Adam"
                      + ("; LPIPS term OFF in this line -- stages.stage3_with_lpips carries it" if args.primary == "stage3" else "") + ")",
            "value": prim["value"], "unit": "rays/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": prim["ms_per_step"], "higher_is_better": True, "scaling": prim["scaling"], "vs_baseline": None,
            "dtype": "f32" if args.gemm == "fp32" else "f32 (fp16/bf16 hi-lo split MFMA x3, fp32 accumulate)",
            "gemm": args.gemm, "launch": prim["launch"],
            "data": "synthetic rays / poses (seeded), random-init weights of the reference architecture",
            "config": {"workload": prim["workload"], "rays_per_gpu": prim["rays_per_gpu"], "global_rays": prim["global_rays"],
                       "parallelism": f"dp{world} (ray shards; flat-gradient all-reduce per module per step)"},
            "comm": comm_info,
            "final_loss": prim["final_loss"], "algorithmic_tflops": prim["algorithmic_tflops"],
            "flop_per_ray": prim["flop_per_ray"], "f_cyc": prim["f_cyc"],
            "step": f"forward + losses + backward + all-reduce + ONE gradient-norm clip (max_norm {GRAD_MAX_NORM}, the Trainer's "
                    "gradient_clip_val of the reference's Backpack.gin) + Adam",
            "parity_note": ("parity with the reference (tests/, oracle pinned by fixtures generated from the imported reference): RGB within 1e-4 "
                            "L-inf on rays whose DISCRETE decisions agree with the oracle's (identical inverse-CDF sample bins; identical "
                            "z-merge order), sample / merge indices bit-exact on identical inputs; rays where an fp32 last-bit difference "
                            "moves a sample across an empty proposal bin or swaps two coinciding samples are counted and bounded by the "
                            "reference's own fp32-CPU vs fp32-ROCm disagreement (tests/test_gpu_selfnoise.py), on random-init AND on "
                            "trained weights (tests/test_gpu_convergence.py)" + ("" if args.gemm == "fp32" else
                            "; arithmetic of this line: 3-product 16-bit split MFMA with fp32 accumulation (SURVEY 7.1's admissible mode), "
                            "the exact-fp32 MFMA companions are stages.stage3_fp32_exact / stage2_fp32_exact")),
        })
        # BASELINE's metric also names "PSNR vs. reference": the held-out PSNR of the HIP path and of the reference's op graph trained side
        # by side (tests/test_gpu_convergence.py) -- REPLAYED from the committed record of that test, not measured by this run
        if args.full:
            try:
                with open(os.path.join(ROOT, "profiles", "r06_parity_counts.json")) as f:
                    pc = json.load(f)
                eq = {k.split(".")[1]: {"psnr_db_hip": pc[k]["psnr_hip"], "psnr_db_reference_graph": pc[k]["psnr_oracle"], "steps": pc[k]["steps"]}
                      for k in ("convergence.stage1", "convergence.stage2", "convergence.stage3") if k in pc}
                wf = pc.get("trained.stage3.whole_frame_eval[held-out frame, jointly trained weights]")
                if wf:
                    eq["stage3_whole_frame_eval_same_weights"] = {"psnr_db_hip": wf["psnr_hip"], "psnr_db_reference_graph": wf["psnr_oracle"], "rgb_linf": wf["rgb_linf"]}
                if eq:
                    out["psnr_vs_reference"] = dict(eq, source="profiles/r06_parity_counts.json (tests/test_gpu_convergence.py on a synthetic scene directory; "
                                                                 "replayed, not measured in this run; the Backpack sequence does not exist offline)")
            except Exception:
                pass
        if model_shard() > 1:
            out["metric"] += f" -- ONE-GPU TIMING MODEL of rank 0 of {model_shard()} with the sharded volume decoder, collectives replaced by identities"
            out["model_shard"] = model_shard()
        if "h2d_bytes_per_step" in prim:       # --h2d: the PCIe-inclusive variant, labelled so that it is never read as the headline
            out["metric"] += " + per-step host-to-device upload of the item"
            out["h2d_bytes_per_step"] = prim["h2d_bytes_per_step"]
        roof = roofline_of(table, args.gemm)
        if roof is not None:
            src = ("HIP events around each GEMM launch in an EAGER, ONE-STREAM post-pass of 3 forward+backward passes right after the "
                   "timed region (same kernels and shapes as the replayed graph, which cannot host per-launch events and runs the "
                   "two branches concurrently on two streams); the rocprofv3 --kernel-trace --stats summary of the replayed graph "
                   "is under profiles/")
            roof["measured"] = "eager post-pass"
            if args.gemm == "planes":
                roof["note"] = ("peak = 2.5 PF dense 16-bit MFMA / 3 products at the 2.4 GHz nominal clock; the same binary on zero-filled operands "
                                "reaches 0.62-0.66 of it, and by counter the launch takes the same ~1.2 M cycles per XCD at 1.5-1.8 GHz on random data "
                                "against 2.1-2.3 GHz on zeros (profiles/r05_pmc_gemmp_clock.json, DESIGN 3.1): the kernel is held by the "
                                "power-limited clock, not by its schedule")
            out["roofline"] = roof
            out["kernels"] = table[:16]
            out["kernels_source"] = src

    def leg(label, fn, limit_s=240.0):
        r = guarded(label, fn, limit_s)
        stages[label] = r[0] if isinstance(r, tuple) else r
        return stages[label]

    if not args.only_primary:
        for name in ("stage2", "stage1"):
            if name == args.primary or (name == "stage2" and world > 1):
                continue
            leg(name, lambda name=name: measure(name, False))
        if args.primary == "stage3" and world == 1:
            r = leg("stage3_fresh_items", lambda: measure("stage3_fresh_items", False))
            if "value" in r:
                r["vs_resident_batch"] = r["value"] / prim["value"]
            r = leg("stage3_with_lpips", lambda: measure("stage3_with_lpips", False))
            if "value" in r:
                r["vs_without_lpips"] = r["value"] / prim["value"]
        if args.primary == "stage3" and world > 1:
            # ---- WEAK scaling: the reference's DDP semantic -- every rank its own full batch (3rd_Complete_HOSNeRF/run.py:173-190,
            # configs/default.yaml N_patches per rank); 4096 rays PER GPU, value = the rays all ranks processed / time
            r = leg("stage3_weak", lambda: measure("stage3", False, rays_global=GLOBAL_RAYS_S3 * world,
                                                   describe=Stage3.describe.replace("4096 rays/batch GLOBAL", f"{GLOBAL_RAYS_S3} rays/batch PER GPU (weak scaling)")))
            if "value" in r:
                r["scaling"] = "weak"
    if not args.only_primary and not args.no_infer and args.gemm == "planes":
        leg("infer_1080p", lambda: infer_1080p(dev, rank, world, dist, events))
    if not args.only_primary and args.primary == "stage3" and world > 1:      # LAST: the one leg that has never met N real devices
        # ---- the sharded volume decoder with the collectives inside ONE hipGraph per rank (libhoscomm / RCCL on the capture
        # stream) -- the best strong-scaling form, opt-in until it has met N real devices
        prev = {k: os.environ.get(k) for k in ("HOS_SHARD_DECODER", "HOS_HOSCOMM")}
        os.environ["HOS_SHARD_DECODER"] = "1"
        if not one_gpu:                       # (RCCL refuses two ranks on one device: the one-GPU rehearsal shards over gloo, eagerly)
            os.environ["HOS_HOSCOMM"] = "1"
        try:
            r = leg("stage3_sharded_onegraph", lambda: measure("stage3", False, describe=Stage3.describe + "; volume decoder SHARDED over the ranks"
                                                               + ("" if one_gpu else ", collectives inside one hipGraph per rank (libhoscomm)")))
            if "value" in r:
                r["vs_default_path"] = r["value"] / prim["value"]
        finally:
            from hosnerf_amd import train as _train
            _train.use_hoscomm(None)
            c = _HOSCOMM.pop("c", None)
            if c is not None:
                try:
                    c.close()
                except Exception:
                    pass
            for k, v in prev.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    if world == 1 and not args.only_primary and rank == 0:
        torch_rocm = {}
        if not args.no_torch_baseline:
            for name, rays in (("stage2", 2048), (args.primary, prim["global_rays"])):
                tb = cpu_baseline(name, device=dev, rays=rays)
                torch_rocm[name] = tb
                tgt = stages.get(name, prim if name == args.primary else None)
                if tgt is not None and "value" in tgt:
                    tgt["torch_rocm"] = tb
                    tgt["speedup_vs_torch_rocm"] = tgt["value"] / tb["value"]
                if name == args.primary:
                    out["torch_rocm"] = tb
                    out["speedup_vs_torch_rocm"] = prim["value"] / tb["value"]
        if args.gemm != "fp32" and not args.no_fp32_exact:
            # ---- the IEEE-fp32 companions of the two headline stages: the same steps with every GEMM on the exact
            # fp32 MFMA (v_mfma_f32_32x32x2_f32, hos_gemm.hip), each against its own peak (157.3 TF) and against the same torch-ROCm
            # denominator (the reference's fp32 rocBLAS path)
            import argparse as _ap
            fa = _ap.Namespace(**{**vars(args), "steps": max(3, min(args.steps, 10)), "warmup": max(1, min(args.warmup, 3))})
            for name in (args.primary, "stage2"):
                if name == "stage1" or f"{name}_fp32_exact" in stages:
                    continue
                ops.set_gemm_mode(ops.GEMM_FP32)
                try:
                    r = guarded(f"{name}_fp32_exact", lambda name=name: measure(name, events and name == args.primary, run_args=fa))
                finally:
                    ops.set_gemm_mode({"planes": ops.GEMM_PLANES, "split": ops.GEMM_BF16X3}[args.gemm])
                if isinstance(r, tuple):
                    r, tab = r
                    r["dtype"] = "f32 (exact fp32 MFMA, fp32 accumulate)"
                    r["frac_of_fp32_mfma_peak"] = r["algorithmic_tflops"] / FP32_MFMA_PEAK_TFLOPS
                    roof32 = roofline_of(tab, "fp32")
                    if roof32 is not None:
                        roof32["measured"] = "eager post-pass"
                        r["roofline"] = roof32
                    if name in torch_rocm:
                        r["speedup_vs_torch_rocm"] = r["value"] / torch_rocm[name]["value"]
                    tgt = prim if name == args.primary else stages.get(name)
                    if tgt is not None and "value" in tgt:
                        r["vs_split_mfma_line"] = r["value"] / tgt["value"]
                stages[f"{name}_fp32_exact"] = r
        if not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.primary)
    emit()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
