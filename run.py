#!/usr/bin/env python
"""Launcher with the reference's command line (`run.py` of each stage directory: 1st_State-Conditional_Scene/run.py:141-156,
3rd_Complete_HOSNeRF/run.py:75-292): `--ginc` / `--ginb` (gin files and bindings), `--scene_name`, `--seed`, `--logbase`,
`--resume_training`, `--ckpt_path`, `--cfg`; `run.model_name` selects the stage (`state_mipnerf360 | state_humanobject |
hosnerf`), `run.max_steps`, `run.grad_max_norm`, `run.bkgd_path` / `run.human_path` (stage-3 warm start, run.py:206-212),
`run.run_train`, `run.run_eval` (S3/run.py:224-231 -> `trainer.test`: the held-out frames rendered by their own cameras, PSNR,
`test_metrics`, M:884-1085) and `run.run_render` (S3/run.py:233-239 -> `trainer.predict`: the free-viewpoint turn about the subject
of `freeview.frame_idx`, `free_view`, M:1293-1494, cameras of core/utils/camera_util.py:106-131), both from `last.ckpt` (stage 3), and `run.run_tpose` (this build's
binding for the last output of the reference's `test_step`, `test_tpose`, M:591-658: the canonical human-object in T-pose, no background, one
`--render_frames` turn per object state).  Stage 1 (`state_mipnerf360`) with `--scene_dir`: training batches from the scene's unmasked pixels
(`raybank.RayBank.sample`, the reference's `SingleImageDDPSampler`), `run.run_eval` -> the test split's whole frames under
<logdir>/render_model + results.json (PSNR), `run.run_render` -> the interpolated camera path under <logdir>/render_video.
`run.render_maps` writes depth / opacity (stage 3: and human-layer) files next to every frame of run_eval / run_render / run_tpose;
`run.render_median` (needs `run.render_maps`) adds <name>_depth_median.npy / .png to the stage-3 frames -- the depth at which the
composited ray's cumulative weight crosses 0.5, the usable depth where the expected depth runs to the far plane -- and changes nothing
for stage 1, whose maps contain the median already.
`run.run_mesh` (stages 2 and 3, with `--scene_dir`; this build's addition) writes the canonical human-object of every object state as
a triangle mesh, <logdir>/mesh/time_<t>.ply + meshes.json (`hosnerf_amd/mesh.py`; `run.mesh_resolution` 256, `run.mesh_level` 0.5).
`run.run_mesh_frames` (same stages, same two parameters; this build's addition) writes the POSED human-object of each frame that
`run.run_eval` would choose (`--eval_skip`), through the renderer's backward warp and in the scene's coordinates,
<logdir>/mesh_frames/<frame_name>.ply + meshes.json (`mesh.extract_frame`; `run.mesh_space` "world" | "body", `run.mesh_normals` True).
`run.mesh_preview` (needs `run.run_mesh_frames`; off by default) looks at each of those meshes again through the frame's own camera:
<frame_name>_mesh.png (shaded), _mesh_normal.png, _mesh_mask.png, _mesh_depth.npy / .png next to the .ply (`mesh.rasterize`,
hos_raster.hip), and in meshes.json the frame's `fit` against the human-object rendered from that camera (silhouette IoU, depth error
against `depth_median`) and against the scene's subject mask; `run.mesh_level_sweep = (l0, l1, ...)` adds the same fit per level.
`run.run_mesh_track` (stages 2 and 3, with `--scene_dir`; this build's addition) writes the TRACKED human-object: per object state
the canonical mesh as a template, and for each frame `run.run_eval` would choose that template posed vertex by vertex through the
inverted backward warp -- one topology per state -- <logdir>/mesh_track/template_state_<s>.ply, <frame_name>.ply,
<frame_name>_residual.npy + meshes.json (`mesh.track`; the same `run.mesh_resolution` / `run.mesh_level` / `run.mesh_space` /
`run.mesh_normals`).
`run.run_mesh_bkgd` (stages 1 and 3, with `--scene_dir`; this build's addition) writes the BACKGROUND scene of every object state as
a triangle mesh in the same scaled-world coordinates, <logdir>/mesh_bkgd/time_<t>.ply + meshes.json (`mesh.extract_bkgd`;
`run.mesh_bkgd_box` (-1,-1,-1, 1,1,1), the same `run.mesh_resolution` / `run.mesh_level`).
`run.mesh_min_component = r` (0 <= r <= 1, default 0.0 = off; this build's addition) drops the floaters of every mesh the four mesh
outputs write: the connected components whose area is below r times the largest component's (`mesh.drop_floaters`,
hos_components.hip) -- the canonical and background meshes, each frame mesh (its preview and fit included) and the templates of
`run.run_mesh_track`, filtered once per state before any frame is tracked.  The rows of meshes.json then describe the written mesh
and gain `components` (count, kept, what was dropped).  At 0 every file is byte-identical to a run without the binding.
The reference's .gin files parse unchanged (hosnerf_amd/gin_lite.py).

What is NOT here: Lightning's Trainer (a plain loop drives `training_step` / `optimizer_step` / checkpoints the way the Trainer
does; DDP = one process per GPU under torch.distributed.run, ray shards + one flat-gradient all-reduce per module), the
datasets and image IO (out of scope -- training items are synthetic unless `--items` points at a torch-saved
list of dataset items with the reference's keys), LPIPS / SSIM.

    python run.py --ginc configs/hosnerf_backpack.gin --scene_name Backpack --logbase logs --ginb "run.max_steps=200"
    python run.py --ginc ... --cpu        # BASELINE configs[0] "CPU plumbing": everything except the kernels, no GPU needed
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def str2bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--ginc", action="append", help="gin config file")
    p.add_argument("--ginb", action="append", help="gin bindings")
    p.add_argument("--resume_training", type=str2bool, nargs="?", const=True, default=False)
    p.add_argument("--ckpt_path", type=str, default=None, help="path to checkpoints")
    p.add_argument("--scene_name", type=str, default=None, help="scene name to render")
    p.add_argument("--seed", type=int, default=220901, help="seed to use")
    p.add_argument("--logbase", type=str, default=None, help="folder to save results")
    p.add_argument("--cfg", default=None, type=str, help="yaml of the human-object network (configs/human_nerf/...), optional")
    # additions of this build
    p.add_argument("--cpu", action="store_true", help="plumbing only (BASELINE configs[0]): no kernel is launched, no GPU needed")
    p.add_argument("--items", type=str, default=None, help="torch-saved list of dataset items (reference keys); default: synthetic")
    p.add_argument("--lpips_vgg16", type=str, default=None, help="torchvision's vgg16 checkpoint (vgg16-397923af.pth): with --lpips_lin "
                   "enables the reference's LPIPS term (weight 1.0, configs/default.yaml:97-101) in stages 2 / 3")
    p.add_argument("--lpips_lin", type=str, default=None, help="the reference's third_parties/lpips/weights/v0.1/vgg.pth")
    p.add_argument("--rays", type=int, default=0, help="rays per step and GPU for synthetic items (default: the stage's reference batch)")
    p.add_argument("--scene_dir", type=str, default=None, help="scene directory in the reference's on-disk formats (cameras.pkl / "
                   "poses_bounds.npy, mesh_infos.pkl, canonical_joints.pkl, images/, masks/, images_flow/): training items, evaluation "
                   "frames and free-viewpoint frames are built from it on the device (stages 2 / 3); stage 1 trains on its unmasked "
                   "pixels (a device-resident ray bank), evaluates its test split and renders its camera path")
    p.add_argument("--eval_skip", type=int, default=0, help="run_eval: render every eval_skip-th frame of the scene (default: 8 frames spread over the sequence)")
    p.add_argument("--render_frames", type=int, default=100, help="run_render / run_tpose: cameras per turn (cfg.render_frames)")
    p.add_argument("--render_limit", type=int, default=0, help="run_render / run_tpose: stop after this many cameras of a turn (0 = all)")
    return p.parse_args(argv)


def make_cfg(args, basedir):
    """S3/run.py:33-62: defaults + configs/default.yaml + --cfg merged; here the hot-path fields of those yaml files are the
    defaults of `default_cfg`, and an optional --cfg yaml overrides them."""
    from hosnerf_amd.human_nerf import Cfg, default_cfg
    cfg = default_cfg(basedir)
    if args.cfg:
        import yaml

        def merge(dst, src):
            for k, v in src.items():
                if isinstance(v, dict):
                    node = dst.get(k)
                    if not isinstance(node, dict):
                        node = Cfg()
                        dst[k] = node
                    merge(node, v)
                else:
                    dst[k] = v
        with open(args.cfg) as f:
            merge(cfg, yaml.safe_load(f) or {})
    return cfg


def synthetic_item(model_name: str, rays: int, seed: int, step: int):
    from hosnerf_amd import synth
    from hosnerf_amd.train import prepare_patch_targets
    if model_name == "state_mipnerf360":
        return synth.stage1_batch(rays, seed=seed + step)
    b = synth.human_batch(rays, seed=seed + step, time=((step * 37) % 100) / 99.0, is_train=True, iter_val=float(step))
    return prepare_patch_targets(synth.add_patch_supervision(b, max(1, rays // 1024), 32, seed + step))


def crop_rays_64(seed: int = 777):
    """BASELINE configs[0] / SURVEY 8(d).1: the 64x64 crop = 4096 rays of a pin-hole camera (f = 64 * 1.2) at z = +1 looking
    at the origin, radii from the neighbouring-ray distance * 2 / sqrt(12) (S1/src/data/ray_utils.py:94-108)."""
    H = W = 64
    f = 64 * 1.2
    j, i = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    d = torch.stack([(i + 0.5 - W / 2) / f, -(j + 0.5 - H / 2) / f, -torch.ones_like(i)], -1).reshape(-1, 3)
    o = torch.tensor([0.0, 0.0, 1.0]).expand_as(d).contiguous()
    dn = d.view(H, W, 3)
    dx = torch.sqrt(((dn[:-1] - dn[1:]) ** 2).sum(-1))
    dx = torch.cat([dx, dx[-2:-1]], 0).reshape(-1, 1)
    vd = d / d.norm(dim=-1, keepdim=True)
    g = torch.Generator().manual_seed(seed)
    return {"rays_o": o, "rays_d": d, "viewdirs": vd, "radii": dx * 2 / (12 ** 0.5), "times": torch.full((H * W,), 0.5),
            "target": torch.rand(H * W, 3, generator=g)}


def run(args, gin):
    from hosnerf_amd import select_option
    from hosnerf_amd.train import batch_to_device, prepare_patch_targets
    kw = gin.kwargs("run")
    model_name = kw.get("model_name")
    if model_name is None:
        raise SystemExit("run.model_name is not bound (pass a --ginc file or --ginb 'run.model_name=\"hosnerf\"')")
    if bool(kw.get("render_median", False)) and not bool(kw.get("render_maps", False)):
        raise SystemExit("run.render_median = True requires run.render_maps = True (the median depth is one of the maps)")
    if bool(kw.get("run_mesh", False)) and model_name == "state_mipnerf360":
        raise SystemExit("run.run_mesh extracts the canonical human-object (stage 2 `state_humanobject`, stage 3 `hosnerf`); stage 1 has no human-object network")
    if bool(kw.get("run_mesh_frames", False)) and model_name == "state_mipnerf360":
        raise SystemExit("run.run_mesh_frames extracts the posed human-object of each frame (stage 2 `state_humanobject`, stage 3 `hosnerf`); stage 1 has no human-object network")
    if bool(kw.get("run_mesh_track", False)) and model_name == "state_mipnerf360":
        raise SystemExit("run.run_mesh_track poses the canonical human-object into each frame (stage 2 `state_humanobject`, stage 3 `hosnerf`); stage 1 has no human-object network")
    if (bool(kw.get("run_mesh_frames", False)) or bool(kw.get("run_mesh_track", False))) and str(kw.get("mesh_space", "world")) not in ("world", "body"):
        raise SystemExit(f"run.mesh_space = {kw.get('mesh_space')!r}: \"world\" (the scene's coordinates) or \"body\" (the frame's body frame)")
    if bool(kw.get("mesh_preview", False)) and not bool(kw.get("run_mesh_frames", False)):
        raise SystemExit("run.mesh_preview = True requires run.run_mesh_frames = True (the preview and the fit are of the frame meshes)")
    mesh_level_sweep(kw)                              # a malformed sweep stops the run before anything is trained
    if bool(kw.get("run_mesh_bkgd", False)):
        if model_name == "state_humanobject":
            raise SystemExit("run.run_mesh_bkgd extracts the background scene (stage 1 `state_mipnerf360`, stage 3 `hosnerf`); stage 2 has no background model")
        mesh_bkgd_box(kw)                             # an empty or non-finite box stops the run before anything is trained
    mesh_min_component(kw)                            # so does a ratio outside [0, 1]
    dataset_name = kw.get("dataset_name", "synthetic")
    scene = args.scene_name or "scene"
    exp_name = f"{model_name}_{dataset_name}_{scene}_{str(args.seed).zfill(3)}"          # S3/run.py:108-110
    if kw.get("postfix"):
        exp_name += "_" + kw["postfix"]
    logdir = os.path.join(args.logbase or "logs", exp_name)
    os.makedirs(logdir, exist_ok=True)
    basedir = kw.get("datadir") if (kw.get("datadir") and os.path.isdir(str(kw.get("datadir")))) else logdir
    if not os.path.exists(os.path.join(basedir, "transitions_times.json")):
        with open(os.path.join(logdir, "transitions_times.json"), "w") as f:       # one transition -> two states, like Backpack
            json.dump({"f0": {"time": 0.4}}, f)
        basedir = logdir
    torch.manual_seed(args.seed)                                                         # seed_everything (run.py:155)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # `run.grad_max_norm` -> Trainer(gradient_clip_val=..., algorithm "norm") in all three launchers (S1/run.py:155,
    # 2nd_.../run.py:185-186, 3rd_.../run.py:188-189); every Backpack.gin binds 0.001
    model_kw = {"grad_max_norm": float(kw.get("grad_max_norm", 0.0))}
    if str(kw.get("grad_clip_algorithm", "norm")) != "norm":
        raise SystemExit("run.grad_clip_algorithm: only 'norm' (the reference's default and the one its configs use) is implemented")
    if model_name == "state_mipnerf360":
        model_kw.update(max_steps=int(kw.get("max_steps", 500000)))
        for k in ("lr_init", "lr_final", "lr_delay_steps", "lr_delay_mult"):
            if gin.get_param(f"LitMipNeRF360.{k}") is not None:
                model_kw[k] = gin.get_param(f"LitMipNeRF360.{k}")
        for side, name in (("near", "LitDataNeRF360V2.near"), ("far", "LitDataNeRF360V2.far")):
            if gin.get_param(name) is not None:
                model_kw[side] = float(gin.get_param(name))
    else:
        model_kw["cfg"] = make_cfg(args, basedir)
    lit = select_option.select_model(model_name, basedir, **model_kw)
    n_params = sum(p.numel() for p in lit.parameters())
    if model_name == "hosnerf":                                                          # warm start, S3/run.py:206-212
        for key in ("human_path", "bkgd_path"):
            path = kw.get(key)
            if path and os.path.exists(str(path)):
                missing, unexpected = select_option.load_checkpoint(lit, path, strict=False)
                print(f"[run] {key}: loaded {path} ({len(missing)} missing, {len(unexpected)} unexpected keys)")
            elif path and args.items:
                # the reference fails in pl_load when a bound warm-start file is missing; training a real scene's stage 3
                # from random initialisation is never what was asked for
                raise SystemExit(f"run.{key} = {path!r} does not exist")
            elif path:
                print(f"[run] WARNING: run.{key} = {path!r} does not exist -- stage 3 starts from RANDOM initialisation "
                      f"(tolerated for synthetic items only)", file=sys.stderr)
    opt = lit.configure_optimizers()
    ckpt = args.ckpt_path or os.path.join(logdir, "last.ckpt")
    step0 = 0
    if args.resume_training and os.path.exists(ckpt):
        select_option.load_checkpoint(lit, ckpt, strict=True)
        step0 = select_option.load_optimizer_states(ckpt, opt)
        print(f"[run] resumed from {ckpt} at step {step0}")
    max_steps = int(kw.get("max_steps", 0))
    default_rays = {"state_mipnerf360": int(gin.get_param("LitData.batch_size", 4096)) // max(world, 1), "state_humanobject": 2048, "hosnerf": 2048}
    rays = args.rays or default_rays[model_name]
    print(f"[run] {exp_name}: {model_name}, {n_params / 1e6:.2f} M parameters, {rays} rays/step/GPU, world {world}, max_steps {max_steps}, logdir {logdir}")

    if args.cpu:
        # BASELINE configs[0] "CPU PyTorch single process (plumbing, no GPU)": flags, gin, module construction under the
        # reference's names, optimiser + schedule, a 64x64-crop ray batch, checkpoint round trip.  The renderer itself has no
        # CPU implementation (by design: hosnerf_amd never falls back); its CPU restatement is the test oracle (tests/).
        crop = crop_rays_64(args.seed)
        lit._step = step0
        lit.apply_lr(opt, step0)
        select_option.save_checkpoint(lit, ckpt, global_step=step0, optimizer=opt)
        missing, unexpected = select_option.load_checkpoint(lit, ckpt, strict=True)
        plan = {"mode": "cpu-plumbing", "exp_name": exp_name, "model_name": model_name, "parameters": n_params, "state_dict_keys": len(lit.state_dict()),
                "crop_rays": int(crop["rays_o"].shape[0]), "samples_per_ray": "64/64/32 background, 128 human", "lr": [g["lr"] for g in opt.param_groups],
                "checkpoint": ckpt, "checkpoint_roundtrip": {"missing": len(missing), "unexpected": len(unexpected)}, "max_steps": max_steps,
                "gin": {k: v for k, v in sorted(gin.items())}}
        print(json.dumps(plan))
        return plan

    if not torch.cuda.is_available():
        raise SystemExit("run.py needs an MI355X for training / rendering (there is no CPU renderer); use --cpu for the plumbing check")
    # HOS_BENCH_ONE_GPU=1 (testing only, as in bench.py): all ranks share cuda:0 and exchange through gloo, so that the multi-rank
    # launcher path -- shards of rays / frames, gradient exchange, sharded decoder, checkpoint of rank 0 -- runs on a one-GPU box
    one_gpu = os.environ.get("HOS_BENCH_ONE_GPU") == "1"
    local = 0 if one_gpu else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if one_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
    lit = lit.to(dev)
    if world > 1 and bool(kw.get("shard_decoder", False)) and hasattr(lit, "human"):
        # `run.shard_decoder = True` (this build's addition; the reference replicates the module under DDP): the volume decoder's
        # first three layers sharded over the ranks (Network.shard_decoder); the optimiser is rebuilt on the remaining active spans
        from hosnerf_amd.train import ShardComm
        lit.human.shard_decoder(ShardComm(rank, world))
        opt = lit.configure_optimizers()
        if args.resume_training and os.path.exists(ckpt):
            select_option.load_optimizer_states(ckpt, opt)
        print(f"[run] volume decoder sharded over {world} ranks: this rank owns {sum(n for _, n in lit.human.decoder_shard_spans()) / 1e6:.2f} M of its parameters")
    if args.lpips_vgg16 or args.lpips_lin:
        if not (args.lpips_vgg16 and args.lpips_lin) or not hasattr(lit, "human"):
            raise SystemExit("--lpips_vgg16 and --lpips_lin go together and apply to the stages that own the human-object network")
        from hosnerf_amd.lpips import LPIPS
        lit.lpips = LPIPS.from_files(args.lpips_vgg16, args.lpips_lin, dev)          # M:582-584
        print(f"[run] LPIPS term enabled (weight 1.0): {args.lpips_vgg16}, {args.lpips_lin}")
    items = torch.load(args.items, weights_only=False) if args.items else None
    if items and model_name == "hosnerf":
        # The stage-3 reference unpacks the rendered rays with a PLAIN reshape (`_unpack_imgs`, S3 model.py:41-50: patches are never
        # cut by the box in stage 3, core/data/human_nerf/train.py:322-330), for the MSE and for the LPIPS term alike: an item whose
        # `patch_masks` has holes is a stage-2 item and would be rendered against the wrong pixels -- refuse it here, once, on the host
        for n, it in enumerate(items):
            if "patch_masks" in it and not bool(torch.as_tensor(it["patch_masks"]).all()):
                raise SystemExit(f"--items[{n}]: patch_masks has holes; stage 3 takes whole patches (the reference's stage-3 _unpack_imgs is a reshape)")
    scene = bank = None
    if args.scene_dir and model_name == "state_mipnerf360":
        # stage 1: the scene's unmasked pixels as a device-resident ray bank (hosnerf_amd/raybank.py) -- the role of LitData.split_each +
        # SingleImageDDPSampler (S1/src/data/interface.py:105-205, sampler.py:52-101) without the host ray table
        bank = load_ray_bank(args.scene_dir, dev, lit.near, lit.far)
        bank_gen = torch.Generator(device=dev)
        bank_gen.manual_seed(args.seed)                  # the SAME seed on every rank: a step's draw is shared, each rank keeps [rank::world]
        print(f"[run] scene {args.scene_dir}: {bank.N} frames of {bank.W}x{bank.H}, {int(bank.offsets_host[-1])} unmasked rays, "
              f"{len(bank.choice_host)} of {len(bank.split)} training images with rays, {len(bank.i_test)} test frames")
    elif args.scene_dir:
        from hosnerf_amd import formats
        from hosnerf_amd.dataset import SceneItems
        from hosnerf_amd.freeview import load_scene_pixels
        px = load_scene_pixels(args.scene_dir)
        if not os.path.exists(os.path.join(args.scene_dir, "cameras_scaleworld.pkl")):     # what the stage-1 loader leaves behind
            formats.load_scene(args.scene_dir, px["images"].shape[1:3], masks=px["alphas"], near=0.1, far=1e6)
        scene = SceneItems(args.scene_dir, px["images"], px["alphas"], px["flows"], frames=px["frames"], device=dev, seed=args.seed + rank,
                           stage=2 if model_name == "state_humanobject" else 3,
                           n_patches=int(model_kw["cfg"].patch.N_patches), patch_size=int(model_kw["cfg"].patch.size),
                           sample_subject_ratio=float(model_kw["cfg"].patch.sample_subject_ratio), bbox_offset=float(model_kw["cfg"].bbox_offset),
                           resize_img_scale=float(model_kw["cfg"].resize_img_scale))
        print(f"[run] scene {args.scene_dir}: {len(scene)} frames of {px['images'].shape[2]}x{px['images'].shape[1]}")
    run_train = bool(kw.get("run_train", True))
    log_every = int(kw.get("log_every_n_steps", 100))
    t0 = time.perf_counter()
    lit._step = step0
    # `last.ckpt` every `run.save_every_n_steps` steps (default 5000; the reference's ModelCheckpoint writes per validation
    # epoch), written to a temporary name and renamed so that a crash during the write never leaves a truncated file
    save_every = int(kw.get("save_every_n_steps", 5000)) if bool(kw.get("save_last", True)) else 0

    def save_last(global_step):
        tmp = ckpt + ".tmp"
        select_option.save_checkpoint(lit, tmp, global_step=global_step, optimizer=opt)
        os.replace(tmp, ckpt)

    if run_train:
        for step in range(step0, max_steps):
            if bank is not None:
                item = bank.sample(rays * world, bank_gen, rank, world)        # LitData.batch_size rays of ONE image; this rank's [rank::world]
            elif scene is not None:
                item = scene[int(torch.randint(len(scene), (1,)))] if len(scene) > 1 else scene[0]      # shuffled frames (DataLoader(shuffle=True))
            else:
                item = items[step % len(items)] if items else synthetic_item(model_name, rays, args.seed + 1000 * rank, step)
            if items and model_name != "state_mipnerf360" and "mse_count" not in item:
                item = prepare_patch_targets(item)          # items straight from the reference's dataset: derive the patch-MSE constants
            batch = batch_to_device(item, dev) if model_name != "state_mipnerf360" else {k: v.to(dev) for k, v in item.items()}
            opt.zero_grad()
            loss = lit.training_step(batch, step)
            lit.backward(loss)           # human stages: volume decoder reduced at its 3.5 MB output gradient (train.backward_human)
            lit.optimizer_step(0, step, opt)
            if save_every > 0 and (step + 1) % save_every == 0 and step + 1 < max_steps:
                if getattr(getattr(lit, "human", None), "decoder_shard", None) is not None:
                    lit.human.gather_decoder_shards(opt)        # collective: every rank's flat buffer is complete before rank 0 writes it
                if rank == 0:
                    save_last(step + 1)
            if (step + 1) % log_every == 0 and rank == 0:
                dt = time.perf_counter() - t0
                print(f"[run] step {step + 1}/{max_steps} loss {float(loss):.5f} lr {opt.param_groups[0]['lr']:.3e} "
                      f"{(step + 1 - step0) * rays * world / dt:.0f} rays/s")
        if getattr(getattr(lit, "human", None), "decoder_shard", None) is not None:
            lit.human.gather_decoder_shards(opt)
        if rank == 0 and bool(kw.get("save_last", True)):
            save_last(max_steps)
            print(f"[run] wrote {ckpt}")
        if world > 1:
            import torch.distributed as dist
            dist.barrier()              # the other ranks' evaluation reads the checkpoint rank 0 has just written
    result = {"exp_name": exp_name, "checkpoint": ckpt}
    run_eval, run_render, run_tpose = bool(kw.get("run_eval", False)), bool(kw.get("run_render", False)), bool(kw.get("run_tpose", False))
    if run_eval or run_render or run_tpose:
        result.update(evaluate_and_render(args, kw, lit, model_name, scene if bank is None else bank, ckpt, logdir, dev, rank, world, run_eval,
                                          run_render, run_tpose, bkgd_chunk=int(gin.get_param("LitData.chunk", 1024 * 32))))
    if bool(kw.get("run_mesh", False)):
        result["mesh"] = extract_meshes(kw, lit, scene, ckpt, logdir, dev, rank, world)
    if bool(kw.get("run_mesh_frames", False)):
        result["mesh_frames"] = extract_frame_meshes(args, kw, lit, scene, ckpt, logdir, dev, rank, world)
    if bool(kw.get("run_mesh_track", False)):
        result["mesh_track"] = track_meshes(args, kw, lit, scene, ckpt, logdir, dev, rank, world)
    if bool(kw.get("run_mesh_bkgd", False)):
        result["mesh_bkgd"] = extract_bkgd_meshes(kw, lit, model_name, scene if bank is None else bank, ckpt, logdir, dev, rank, world)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return result


def load_ray_bank(scene_dir: str, dev, near: float, far: float):
    """Decode a scene directory and build the stage-1 `RayBank`: `formats.load_scene` (normalised cameras, splits, render path,
    `bkgrays_sizes`; writes cameras_scaleworld.pkl for the later stages like the reference's loader) over `freeview.load_scene_pixels`."""
    from hosnerf_amd import formats
    from hosnerf_amd.freeview import load_scene_pixels
    from hosnerf_amd.raybank import RayBank
    px = load_scene_pixels(scene_dir)
    scene = formats.load_scene(scene_dir, px["images"].shape[1:3], masks=px["alphas"], near=near, far=far)
    split = "train"
    if len(scene["i_split"][0]) == 0:
        # fewer than 16 frames: `load_scene` holds every frame out as a test frame (the reference needs >= 16 frames); such a scene
        # trains on the frames it has
        print(f"[run] {scene_dir}: every frame is a test frame (fewer than 16 frames); training draws from all of them")
        split = "all"
    return RayBank(scene, px["images"], px["alphas"], device=dev, split=split)


def load_last(lit, source, ckpt, names: str, hint: str):
    """What every output entry point starts with: refuse a run without `source` (the scene or ray bank of `--scene_dir`) or without
    the checkpoint, under the bindings' `names`, then load the checkpoint into `lit` (strict).  Returns the checkpoint's
    `global_step`, None for a bare state_dict, from that one read of the file."""
    from hosnerf_amd import select_option
    if source is None:
        raise SystemExit(f"{names} need{'' if '/' in names else 's'} --scene_dir ({hint})")
    if not os.path.exists(ckpt):
        raise SystemExit(f"{names}: {ckpt} does not exist (train first, or pass --ckpt_path)")
    ck = torch.load(ckpt, map_location="cpu", weights_only=False)
    select_option.load_checkpoint(lit, ck, strict=True)
    return ck.get("global_step") if isinstance(ck, dict) else None


def turn_counts(args, total):
    """(cameras to render, cameras of the whole turn): `--render_limit` stops a turn early, 0 = all of it."""
    total = int(total)
    return (min(total, args.render_limit) if args.render_limit > 0 else total), total


def write_frame(folder: str, file_name: str, rendered, H: int, W: int, maps=None, u8: bool = False):
    """The files of one frame: its colour image <folder>/<file_name> -- `to_8b_image` of the float frame `rendered` [H*W,3]
    (model.py:1471-1486), or with `u8` the paint kernel's 8-bit frame as it is -- and `freeview.save_frame_maps` of `maps` (a dict
    or None) under the file's stem."""
    from PIL import Image
    from hosnerf_amd.eval import to_8b_image
    from hosnerf_amd.freeview import save_frame_maps
    os.makedirs(folder, exist_ok=True)
    Image.fromarray((rendered if u8 else to_8b_image(rendered)).view(H, W, 3).cpu().numpy()).save(os.path.join(folder, file_name))
    if maps:
        save_frame_maps(folder, os.path.splitext(file_name)[0], maps, H, W)


def evaluate_and_render_bkgd(args, lit, bank, ckpt, logdir, dev, rank, world, run_eval: bool, run_render: bool, chunk: int,
                             render_maps: bool = False):
    """`trainer.test` / `trainer.predict` of the stage-1 launcher (S1/run.py, S1/src/model/mipnerf360/model.py:516-534, :582-609,
    S1/src/model/interface.py:137-150) from `last.ckpt`: the whole frames of the test split `i_test` through `eval.render_bkgd_frame`
    -> <logdir>/render_model/image{NNN}.jpg + <logdir>/results.json (PSNR as `psnr_each`; SSIM / LPIPS are not computed), and the
    cameras of the interpolated path `render_poses` / `render_times` -> <logdir>/render_video/image{NNN}.jpg (`--render_limit` stops
    early; no mp4).  `train_frac` is the checkpoint's global_step / run.max_steps.  With several ranks the FRAMES are dealt
    round-robin (as `render_tpose`), each rank writes its own files, and one all-reduce of the per-frame PSNR vector precedes rank
    0's results.json.  `render_maps` (`run.render_maps`): every frame is rendered with `maps=True` and `freeview.save_frame_maps`
    writes image{NNN}_depth / _depth_median (.npy + preview) and image{NNN}_alpha.png next to its jpg; PSNR and results.json are
    those of the colours, which are the same."""
    from hosnerf_amd import eval as ev
    from hosnerf_amd.raybank import deal_frames
    step = load_last(lit, bank, ckpt, "run.run_eval / run.run_render", "frames and cameras to render")
    train_frac = int(lit.max_steps if step is None else step) / max(int(lit.max_steps), 1)

    def render(frame_or_pose):
        out = ev.render_bkgd_frame(lit.model, bank, frame_or_pose, chunk, train_frac, lit.near, lit.far, maps=render_maps)
        return (out["rgb"], out) if render_maps else (out, None)

    def write(folder, k, rendered, frame_maps):
        write_frame(os.path.join(logdir, folder), f"image{str(k).zfill(3)}.jpg", rendered, bank.H, bank.W, frame_maps)

    out = {}
    if run_eval:
        frames = [int(i) for i in bank.i_test]
        psnrs = torch.zeros(len(frames), dtype=torch.float64)
        for j in deal_frames(len(frames), rank, world):
            rendered, frame_maps = render(frames[j])
            psnrs[j] = ev.psnr_each(rendered, bank.truth(frames[j]))
            write("render_model", j, rendered, frame_maps)
        if world > 1:
            import torch.distributed as dist
            if dist.get_backend() == "nccl":
                psnrs = psnrs.to(dev)
            dist.all_reduce(psnrs)                       # every frame was rendered by exactly one rank: the sum is the vector
            psnrs = psnrs.cpu()
        if rank == 0:
            out.update(ev.write_bkgd_results(os.path.join(logdir, "results.json"), psnrs.numpy()))
            print(f"[run] Test PSNR is {out['PSNR']['test']:.4f} over {len(frames)} frames")
    if run_render:
        count, total = turn_counts(args, len(bank.render_poses))
        for k in deal_frames(count, rank, world):
            write("render_video", k, *render(("pose", k)))
        if rank == 0:
            print(f"[run] Render path: {count} of {total} cameras written to {os.path.join(logdir, 'render_video')}")
    return {"results": out}


def evaluate_and_render(args, kw, lit, model_name, scene, ckpt, logdir, dev, rank, world, run_eval: bool, run_render: bool,
                        run_tpose: bool = False, bkgd_chunk: int = 1024 * 32):
    """`trainer.test` / `trainer.predict` of the stage-3 launcher (S3/run.py:224-239) from `last.ckpt`: `test_metrics` over held-out
    frames (PSNR against the frame's pixels, images under <logdir>/test_vis) and `free_view` over the orbit cameras of
    `freeview.frame_idx` (images under <logdir>/freeview_vis_newtrans/view_<idx>), every frame through `eval.render_frame`; with
    several ranks each frame's rays are split over the group.  `run_tpose` (`test_tpose`, M:591-658, the last output of the reference's
    `test_step`): the canonical human-object in T-pose without background, one turn of `--render_frames` cameras per object state,
    through `eval.render_human_frame`, images under <logdir>/tpose_vis/time_<t>; with several ranks the FRAMES are dealt round-robin
    (no collectives).  Writes <logdir>/results.json."""
    from hosnerf_amd import eval as ev
    render_maps = bool(kw.get("render_maps", False))          # run.render_maps: depth / opacity / human-layer files next to each frame
    render_median = bool(kw.get("render_median", False))      # run.render_median: + <name>_depth_median.npy / .png (stage 1: in its maps already)
    if model_name == "state_mipnerf360":
        if run_tpose:
            raise SystemExit("run.run_tpose renders the human-object network (stage 3); stage 1 has run.run_eval / run.run_render")
        return evaluate_and_render_bkgd(args, lit, scene, ckpt, logdir, dev, rank, world, run_eval, run_render, bkgd_chunk, render_maps)
    if model_name != "hosnerf":
        raise SystemExit("run.run_eval / run.run_render / run.run_tpose: full-frame rendering is the stage-1 (`state_mipnerf360`) and stage-3 (`hosnerf`) launchers'; stage 2 reports its training loss only")
    step = load_last(lit, scene, ckpt, "run.run_eval / run.run_render / run.run_tpose", "frames, cameras and SMPL fits to render")
    hos = lit.net                                   # the composite renderer that owns `model` and `human`
    group = None
    if world > 1:
        import torch.distributed as dist
        group = dist.group.WORLD
    chunk = int(lit.cfg.chunk_bkg)
    bgc = tuple(float(c) for c in lit.cfg.bgcolor)

    def frame(fr, folder, file_name):
        """Render one stage-3 frame (its rays split over the group), rank 0 writes it; returns its PSNR against the frame's pixels."""
        rendered = ev.render_frame(hos, fr, chunk_bkg=chunk, randomized=False, group=group, maps=render_maps, median=render_median)
        frame_maps, rendered = (rendered, rendered["rgb"]) if render_maps else (None, rendered)
        psnr = ev.psnr_metric(rendered, ev.truth_frame(fr))
        if rank == 0:
            write_frame(os.path.join(logdir, folder), file_name, rendered, int(fr["img_height"]), int(fr["img_width"]), frame_maps)
        return psnr

    out = {}
    if run_eval:
        psnrs = {}
        for i in eval_frame_indices(len(scene), args.eval_skip):
            fr = scene.eval_frame(i, bgcolor=bgc)
            psnrs[fr["frame_name"]] = frame(fr, "test_vis", fr["frame_name"] + ".png")
        out["test"] = {"psnr": float(sum(psnrs.values()) / len(psnrs)), "frames": psnrs}
        if rank == 0:
            print(f"[run] Test PSNR is {out['test']['psnr']:.4f} over {len(psnrs)} frames")
    if run_render:
        fidx = min(int(lit.cfg.freeview.frame_idx), len(scene) - 1)
        count, total = turn_counts(args, args.render_frames)
        # the reference reports the PSNR against the training frame too (M:1462)
        psnrs = [frame(scene.freeview_frame(fidx, k, total, bgcolor=bgc), os.path.join("freeview_vis_newtrans", f"view_{fidx:05d}"), f"image-{k:05d}.jpg")
                 for k in range(count)]
        out["freeview"] = {"frame_idx": fidx, "frames": count, "of": total, "psnr_vs_training_frame": float(sum(psnrs) / len(psnrs))}
        if rank == 0:
            print(f"[run] Freeview: {count} of {total} cameras about frame {fidx} written to {os.path.join(logdir, 'freeview_vis_newtrans')}")
    if run_tpose:
        out["tpose"] = render_tpose(args, lit, hos, scene, ckpt, logdir, dev, rank, world, bgc, render_maps, render_median, global_step=step)
    if rank == 0:
        with open(os.path.join(logdir, "results.json"), "w") as f:
            json.dump(out, f, indent=1)
    return {"results": out}


def render_tpose(args, lit, hos, scene, ckpt, logdir, dev, rank, world, bgc, render_maps: bool, render_median: bool = False, global_step=None):
    """`test_tpose` for every time of `tpose.tpose_times` (M:643-658): `--render_frames` cameras per turn (`--render_limit` stops a
    turn early), rank r renders the frames k % world == r and writes its own files -- <logdir>/tpose_vis/time_{:06}/image-{:05}.jpg
    (M:631-635) from the paint kernel's 8-bit buffer and, with `run.render_maps`, <name>_alpha.png; with `run.render_median` also
    <name>_depth_median.npy / .png (`freeview.save_frame_maps`).  `global_step` is the loaded checkpoint's (`load_last`), None for
    a bare state_dict."""
    from PIL import Image
    from hosnerf_amd import eval as ev, tpose
    count, total = turn_counts(args, args.render_frames)
    step = 1e7 if global_step is None else float(global_step)          # M:615; a bare state_dict: as the other frames
    turn = tpose.TposeTurn(scene.canonical_joints, scene.canonical_bbox, int(lit.cfg.mweight_volume.volume_size), dev)
    times = tpose.tpose_times(hos.human.transitions_times)
    for t in times:
        for k in range(rank, count, world):
            folder, name = tpose.tpose_paths(t, k)
            fr = tpose.tpose_frame(None, None, k, total, bgcolor=bgc, turn=turn, iter_val=step, time=t)
            rendered, u8 = ev.render_human_frame(hos, fr, maps=render_maps, want_u8=True, median=render_median)
            H, W = int(fr["img_height"]), int(fr["img_width"])
            write_frame(os.path.join(logdir, "tpose_vis", folder), name, u8, H, W, {"depth_median": rendered["depth_median"]} if render_median else None, u8=True)
            if render_maps:
                # truncated (`to_8b_image`, the reference's conversion), not rounded like every other _alpha.png: changing it would change bytes
                alpha8 = ev.to_8b_image(rendered["alpha"].view(H, W)).cpu().numpy()
                Image.fromarray(alpha8).save(os.path.join(logdir, "tpose_vis", folder, os.path.splitext(name)[0] + "_alpha.png"))
    if rank == 0:
        print(f"[run] T-pose: {count} of {total} cameras for each of {len(times)} states written to {os.path.join(logdir, 'tpose_vis')}")
    return {"times": times, "frames": count, "of": total}


def write_mesh_set(folder: str, n: int, rank: int, world: int, job, key):
    """One set of meshes under `folder`: the `n` jobs are dealt round-robin over the ranks, `job(j)` -> (file stem, mesh, the row's own
    fields) and this rank writes <stem>.ply; every row gets the mesh's measures, the rows are gathered, and rank 0 writes
    meshes.json as {key(row): row}.  Returns the rows, whole on every rank."""
    from hosnerf_amd import formats
    from hosnerf_amd.raybank import deal_frames
    os.makedirs(folder, exist_ok=True)
    rows = [None] * n
    for j in deal_frames(n, rank, world):
        stem, m, row = job(j)
        formats.write_ply(os.path.join(folder, stem + ".ply"), m["vertices"], m["faces"], m["colors"], m.get("normals"))
        rows[j] = row
    if world > 1:
        import torch.distributed as dist
        gathered = [None] * world
        dist.all_gather_object(gathered, rows)
        rows = [next(g[j] for g in gathered if g[j] is not None) for j in range(n)]
    if rank == 0:
        with open(os.path.join(folder, "meshes.json"), "w") as f:
            json.dump({key(r): r for r in rows}, f, indent=1)
    return rows


def mesh_measures(m, level: float):
    """The fields every row of meshes.json has, in its order."""
    return {"state": m["state"], "V": int(m["vertices"].shape[0]), "F": int(m["faces"].shape[0]), "volume": m["volume"], "area": m["area"],
            "level": level, "spacing": m["spacing"], "dims": list(m["dims"])}


def extract_meshes(kw, lit, scene, ckpt, logdir, dev, rank, world):
    """`run.run_mesh` (this build's addition; stage 2 and stage 3): the canonical human-object of every object state as a triangle
    mesh, from `last.ckpt`, at the times of `tpose.tpose_times` -- `mesh.extract` at `run.mesh_resolution` (256) and `run.mesh_level`
    (0.5) -> <logdir>/mesh/time_{:06}.ply (binary PLY, per-vertex albedo) and <logdir>/mesh/meshes.json (per time: state, V, F,
    volume, area, level, spacing, dims).  With several ranks the states are dealt round-robin, each rank writes its own .ply and
    rank 0 the JSON.  `results.json` is not touched.  `run.mesh_min_component` > 0: the floaters are dropped (`mesh_min_component`)."""
    from hosnerf_amd import mesh, tpose
    load_last(lit, scene, ckpt, "run.run_mesh", "canonical joints and box")
    resolution, level = int(kw.get("mesh_resolution", 256)), float(kw.get("mesh_level", 0.5))
    floaters = floater_kwargs(kw)
    net = lit.human
    turn = tpose.TposeTurn(scene.canonical_joints, scene.canonical_bbox, int(lit.cfg.mweight_volume.volume_size), dev)
    times = tpose.tpose_times(net.transitions_times)

    def job(j):
        m = mesh.extract(net, turn, times[j], resolution=resolution, level=level, **floaters)
        return "time_{:06}".format(times[j]), m, {"time": times[j], **mesh_measures(m, level), **components_row(m, floaters)}

    write_mesh_set(os.path.join(logdir, "mesh"), len(times), rank, world, job, lambda r: "time_{:06}".format(r["time"]))
    if rank == 0:
        print(f"[run] mesh: {len(times)} object states at resolution {resolution}, level {level} written to {os.path.join(logdir, 'mesh')}")
    return {"times": times, "resolution": resolution, "level": level}


def eval_frame_indices(n: int, eval_skip: int):
    """The frames `run.run_eval` renders: every `--eval_skip`-th, else eight spread over the sequence."""
    return list(range(0, n, eval_skip)) if eval_skip > 0 else sorted({int(round(i * (n - 1) / 7.0)) for i in range(8)} if n > 1 else {0})


def extract_frame_meshes(args, kw, lit, scene, ckpt, logdir, dev, rank, world):
    """`run.run_mesh_frames` (this build's addition; stage 2 and stage 3): the human-object as it stands in each chosen frame --
    posed, with the frame's non-rigid offset, through the renderer's backward warp (`mesh.extract_frame`) -- from `last.ckpt`, for the
    frames `run.run_eval` chooses (`--eval_skip`, else eight over the sequence), at `run.mesh_resolution` (256) and `run.mesh_level`
    (0.5), in `run.mesh_space` ("world": the scene's scaled world, or "body"), with per-vertex normals unless `run.mesh_normals =
    False` -> <logdir>/mesh_frames/<frame_name>.ply and <logdir>/mesh_frames/meshes.json (per frame: time, state, V, F, volume, area,
    level, spacing, dims, space, to_world).  With several ranks the frames are dealt round-robin, each rank writes its own .ply and
    rank 0 the JSON.  `results.json` is not touched.

    `run.mesh_preview = True` (opt-in; without it the files and the JSON are exactly the above): every frame's BODY-space mesh --
    the one extraction, before `mesh.to_space` -- is rasterised from the frame's own camera (`scene.frame_camera`, `mesh.rasterize`)
    -> <frame_name>_mesh.png / _mesh_normal.png / _mesh_mask.png / _mesh_depth.npy / _mesh_depth.png next to the .ply
    (`freeview.save_mesh_maps`); the human-object alone is rendered from the same camera (`eval.render_human_frame` of
    `scene.human_frame`, maps and median depth), and the frame's row gets `fit`: `render` (`mesh.fit` against the render's alpha /
    depth_median) and `mask` (against the scene's subject mask, silhouette only).  `run.mesh_level_sweep = (l0, l1, ...)` adds
    `sweep`: `mesh.level_sweep` of the same field against the render, one row per level.  `run.mesh_min_component` > 0: the
    floaters are dropped (`mesh_min_component`) before the normals and `mesh.to_space`; the preview and the fit are of the
    filtered body mesh, the sweep's re-marches stay unfiltered."""
    from hosnerf_amd import mesh
    load_last(lit, scene, ckpt, "run.run_mesh_frames", "the frames' poses, boxes and cameras")
    floaters = floater_kwargs(kw)
    resolution, level = int(kw.get("mesh_resolution", 256)), float(kw.get("mesh_level", 0.5))
    space, normals = str(kw.get("mesh_space", "world")), bool(kw.get("mesh_normals", True))
    preview, sweep = bool(kw.get("mesh_preview", False)), mesh_level_sweep(kw)
    net = lit.human
    idxs = eval_frame_indices(len(scene), args.eval_skip)
    folder = os.path.join(logdir, "mesh_frames")

    def job(j):
        try:
            m = mesh.extract_frame(net, scene.frame_pose(idxs[j]), resolution=resolution, level=level, space=space, normals=normals,
                                   **({"keep_body": True} if preview else {}), **floaters)      # without the switches: the call as it always was
        except ValueError as e:                      # cameras without smpl_to_scale_world: say so and stop, no half-written sequence
            raise SystemExit(f"run.run_mesh_frames: {e}")
        row = {"frame_name": m["frame_name"], "time": m["time"], **mesh_measures(m, level), "space": space,
               "to_world": [[float(x) for x in r] for r in m["to_world"]], **components_row(m, floaters)}
        if preview:
            row.update(preview_frame_mesh(lit, scene, idxs[j], m, folder, sweep))
        return m["frame_name"], m, row

    rows = write_mesh_set(folder, len(idxs), rank, world, job, lambda r: r["frame_name"])
    if rank == 0:
        print(f"[run] frame meshes: {len(idxs)} frames at resolution {resolution}, level {level}, space {space} written to {os.path.join(logdir, 'mesh_frames')}")
    return {"frames": [r["frame_name"] for r in rows], "resolution": resolution, "level": level, "space": space}


def _spread(x):
    """{median, p99, max} of a device vector as floats (empty: zeros)."""
    x = x.double()
    if x.numel() == 0:
        return {"median": 0.0, "p99": 0.0, "max": 0.0}
    return {"median": float(x.median()), "p99": float(torch.quantile(x, 0.99)), "max": float(x.max())}


def track_meshes(args, kw, lit, scene, ckpt, logdir, dev, rank, world):
    """`run.run_mesh_track` (this build's addition; stage 2 and stage 3): the human-object as ONE mesh per object state that moves
    -- the canonical mesh of the state (`mesh.extract` at the state's time of `tpose.tpose_times`, `run.mesh_resolution` (256),
    `run.mesh_level` (0.5), with normals unless `run.mesh_normals = False`) posed into every frame `run.run_eval` chooses
    (`--eval_skip`, else eight over the sequence) by `mesh.track`, in `run.mesh_space` -> <logdir>/mesh_track/template_state_<s>.ply
    per state, <frame_name>.ply (the template's faces and colours, the frame's vertices) and <frame_name>_residual.npy (float32 [V],
    |G(p) - c| per vertex) per frame, and meshes.json (per frame: frame_name, time, state, template, V, F, converged (share),
    residual {median, p99, max}, mask_ratio {median, min, max} of mask / mask_canonical over the vertices whose canonical mask exceeds 1e-4,
    volume, area, level, spacing, dims, space, to_world).  The templates are extracted once per state on every rank that needs them;
    the frames are dealt round-robin, each rank writes its own files and rank 0 the JSON (and the templates).  `results.json` is not
    touched.  `run.mesh_min_component` > 0: every template loses its floaters (`mesh_min_component`) once, when it is extracted and
    before any frame is tracked; template_state_<s>.ply is the filtered template and every row gains its `components`."""
    import numpy as np
    from hosnerf_amd import formats, mesh, tpose
    load_last(lit, scene, ckpt, "run.run_mesh_track", "the frames' poses and the canonical joints and box")
    resolution, level = int(kw.get("mesh_resolution", 256)), float(kw.get("mesh_level", 0.5))
    space, normals = str(kw.get("mesh_space", "world")), bool(kw.get("mesh_normals", True))
    floaters = floater_kwargs(kw)
    net = lit.human
    turn = tpose.TposeTurn(scene.canonical_joints, scene.canonical_bbox, int(lit.cfg.mweight_volume.volume_size), dev)
    state_time = {mesh.select_state(float(t), net.transitions_times): float(t) for t in tpose.tpose_times(net.transitions_times)}
    idxs = eval_frame_indices(len(scene), args.eval_skip)
    folder = os.path.join(logdir, "mesh_track")
    os.makedirs(folder, exist_ok=True)
    templates = {}

    def template_of(state):
        if state not in templates:
            templates[state] = mesh.extract(net, turn, state_time[state], resolution=resolution, level=level, normals=normals, **floaters)
        return templates[state]

    def job(j):
        pose = scene.frame_pose(idxs[j])
        tpl = template_of(mesh.select_state(float(pose["time"]), net.transitions_times))
        try:
            m = mesh.track(net, tpl, pose, space=space, normals=normals)
        except ValueError as e:                      # cameras without smpl_to_scale_world: say so and stop
            raise SystemExit(f"run.run_mesh_track: {e}")
        np.save(os.path.join(folder, m["frame_name"] + "_residual.npy"), m["residual"].cpu().numpy().astype(np.float32))
        on = m["mask_canonical"] > 1e-4                 # the solver's own weight threshold: below it a vertex is lost by definition
        ratio = (m["mask"][on] / m["mask_canonical"][on]).double()
        row = {"frame_name": m["frame_name"], "time": m["time"], "state": m["state"], "template": f"template_state_{m['state']}.ply",
               "V": int(m["vertices"].shape[0]), "F": int(m["faces"].shape[0]),
               "converged": float(m["converged"].double().mean()) if m["converged"].numel() else 0.0, "residual": _spread(m["residual"]),
               "mask_ratio": {"median": float(ratio.median()), "min": float(ratio.min()), "max": float(ratio.max())} if ratio.numel()
               else {"median": 0.0, "min": 0.0, "max": 0.0},
               "volume": m["volume"], "area": m["area"], "level": level, "spacing": m["spacing"], "dims": list(m["dims"]), "space": space,
               "to_world": [[float(x) for x in r] for r in m["to_world"]], **components_row(tpl, floaters)}
        return m["frame_name"], m, row

    rows = write_mesh_set(folder, len(idxs), rank, world, job, lambda r: r["frame_name"])
    if rank == 0:                                    # every object state, extracted here if this rank met none of its frames
        for s in sorted(state_time):
            t = template_of(s)
            formats.write_ply(os.path.join(folder, f"template_state_{s}.ply"), t["vertices"], t["faces"], t["colors"], t.get("normals"))
        print(f"[run] tracked meshes: {len(idxs)} frames of {len({r['state'] for r in rows})} object states at resolution {resolution}, "
              f"level {level}, space {space} written to {folder}")
    return {"frames": [r["frame_name"] for r in rows], "states": sorted({r["state"] for r in rows}), "resolution": resolution, "level": level,
            "space": space}


def mesh_level_sweep(kw):
    """`run.mesh_level_sweep` = (l0, l1, ...): the levels `run.mesh_preview` re-marches each frame's field at, a tuple of finite
    floats; absent or empty = no sweep -> tuple.  The sweep scores UNFILTERED re-marches: `run.mesh_min_component` does not apply to
    them (a level is judged by everything it extracts, floaters included)."""
    levels = kw.get("mesh_level_sweep", ())
    ok = isinstance(levels, (tuple, list)) and all(isinstance(x, (int, float)) and not isinstance(x, bool) and math.isfinite(x) for x in levels)
    if not ok:
        raise SystemExit(f"run.mesh_level_sweep = {levels!r}: a tuple of finite floats, e.g. (0.1, 0.3, 0.5)")
    if len(levels) > 0 and not bool(kw.get("mesh_preview", False)):
        raise SystemExit("run.mesh_level_sweep requires run.mesh_preview = True (the sweep is scored against the preview's render)")
    return tuple(float(x) for x in levels)


def preview_frame_mesh(lit, scene, idx: int, m, folder: str, sweep=()):
    """`run.mesh_preview` for one frame: the body-space mesh `m["body"]` (`mesh.extract_frame(keep_body=True)`) rasterised from the
    frame's own camera and written by `freeview.save_mesh_maps` under `folder`, the human-object alone rendered from that camera,
    and the two compared -> {"fit": {"render": ..., "mask": ...}} and, with `sweep` levels, "sweep": the rows of `mesh.level_sweep`."""
    from hosnerf_amd import eval as ev, mesh
    from hosnerf_amd.freeview import save_mesh_maps
    cam = scene.frame_camera(idx)
    bgc = tuple(float(c) for c in lit.cfg.bgcolor)
    raster = mesh.rasterize(m["body"], cam["K"], cam["E"], cam["H"], cam["W"], bgcolor=bgc)
    save_mesh_maps(folder, m["frame_name"], raster, cam["H"], cam["W"])
    hos = lit.net if getattr(lit, "net", None) is not None else lit.human     # stage 3: the renderer that owns `human`; stage 2: the network itself
    render = ev.render_human_frame(hos, scene.human_frame(idx, bgc), maps=True, median=True)
    out = {"fit": {"render": mesh.fit(raster, render["alpha"], render["depth_median"], spacing=m["spacing"]),
                   "mask": mesh.fit(raster, scene.alphas[idx])}}
    if sweep:
        out["sweep"] = mesh.level_sweep({"alpha": m["alpha"], "origin": m["origin"], "spacing": m["spacing"]}, sweep, cam, render)
    return out


def mesh_min_component(kw):
    """`run.mesh_min_component` = r: every written mesh keeps the connected components whose area is at least r times the largest
    component's (`mesh.drop_floaters(min_area_ratio=r)`).  A number in [0, 1], default 0.0 = no filtering, or the run stops."""
    r = kw.get("mesh_min_component", 0.0)
    if isinstance(r, bool) or not isinstance(r, (int, float)) or not 0.0 <= float(r) <= 1.0:
        raise SystemExit(f"run.mesh_min_component = {r!r}: a number in [0, 1], the smallest component kept as a share of the largest one's area (0 = keep all)")
    return float(r)


def floater_kwargs(kw):
    """What the extractors are handed for `run.mesh_min_component`: nothing at 0 -- the call as it always was."""
    r = mesh_min_component(kw)
    return {"min_area_ratio": r} if r > 0.0 else {}


def components_row(m, floaters):
    """The `components` entry a row of meshes.json gains with `run.mesh_min_component` > 0; nothing without."""
    return {"components": m["components"]} if floaters else {}


def mesh_bkgd_box(kw):
    """`run.mesh_bkgd_box` = (xmin, ymin, zmin, xmax, ymax, zmax), default the cube (-1,-1,-1, 1,1,1) about the region the scene
    contraction leaves linear; a larger box is legal (the contraction takes any point).  Six finite numbers with min < max on every
    axis, or the run stops."""
    box = kw.get("mesh_bkgd_box", (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0))
    try:
        b = [float(x) for x in box]
    except (TypeError, ValueError):
        b = []
    if len(b) != 6 or not all(x == x and abs(x) != float("inf") for x in b) or not all(b[a] < b[a + 3] for a in range(3)):
        raise SystemExit(f"run.mesh_bkgd_box = {box!r}: (xmin, ymin, zmin, xmax, ymax, zmax), finite, with min < max on every axis")
    return b


def extract_bkgd_meshes(kw, lit, model_name, source, ckpt, logdir, dev, rank, world):
    """`run.run_mesh_bkgd` (this build's addition; stage 1 and stage 3): the background scene of every object state as a triangle
    mesh, from `last.ckpt`, at the times of `tpose.tpose_times` -- `mesh.extract_bkgd` inside `run.mesh_bkgd_box` at
    `run.mesh_resolution` (256) and `run.mesh_level` (0.5) -> <logdir>/mesh_bkgd/time_{:06}.ply (binary PLY: position, nx ny nz,
    colour seen head-on) and <logdir>/mesh_bkgd/meshes.json (per time: the fields of mesh/meshes.json plus box).  The vertices are
    in the background rays' own space, the scene's scaled world: the space the stage-3 z-merge maps the human samples into by
    `newsmpl_to_scale_world` (hosnerf.py, `ops.merge_composite`) and therefore the one `run.mesh_space = "world"` writes the frame
    meshes in -- mesh_frames/*.ply and mesh_bkgd/*.ply load aligned.  With several ranks the states are dealt round-robin, each rank
    writes its own .ply and rank 0 the JSON.  `results.json` is not touched.  `run.mesh_min_component` > 0: the floaters are dropped
    (`mesh_min_component`) before the colour query, which then runs on the kept vertices only."""
    from hosnerf_amd import mesh, tpose
    load_last(lit, source, ckpt, "run.run_mesh_bkgd", "the scene whose checkpoint is meshed")
    floaters = floater_kwargs(kw)
    resolution, level = int(kw.get("mesh_resolution", 256)), float(kw.get("mesh_level", 0.5))
    box = mesh_bkgd_box(kw)
    model = lit.model if model_name == "state_mipnerf360" else lit.net.model
    times = tpose.tpose_times(model.mlps[-1].transitions_times)

    def job(j):
        m = mesh.extract_bkgd(model, box, times[j], resolution=resolution, level=level, **floaters)
        return "time_{:06}".format(times[j]), m, {"time": times[j], **mesh_measures(m, level), "box": m["box"], **components_row(m, floaters)}

    write_mesh_set(os.path.join(logdir, "mesh_bkgd"), len(times), rank, world, job, lambda r: "time_{:06}".format(r["time"]))
    if rank == 0:
        print(f"[run] background mesh: {len(times)} object states at resolution {resolution}, level {level}, box {box} written to {os.path.join(logdir, 'mesh_bkgd')}")
    return {"times": times, "resolution": resolution, "level": level, "box": box}


def main(argv=None):
    from hosnerf_amd import gin_lite
    args = parse_args(argv)
    gin = gin_lite.parse_config_files_and_bindings(args.ginc, args.ginb)
    return run(args, gin)


if __name__ == "__main__":
    main()
