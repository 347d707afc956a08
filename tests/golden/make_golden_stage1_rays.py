"""Golden vectors for the stage-1 ray bank (hosnerf_amd/raybank.py, hos_raybank.hip): the tables the REFERENCE's own stage-1 data
code builds -- `batchified_get_rays` (src/data/ray_utils.py) under `LitData.split_each` (training split, masked) and
`LitData.split_each_val` (one whole test frame, the render-path cameras), plus batches of `SingleImageDDPSampler` -- imported here
from where the reference lies (build container only) and run on a seeded scene of 5 cameras of 12 x 20 pixels.
  python tests/golden/make_golden_stage1_rays.py   ->  tests/golden/stage1_rays.npz"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refload  # noqa: E402

N, H, W = 5, 12, 20
I_TRAIN, I_TEST = np.array([0, 1, 3, 4]), np.array([2])
ZERO_IMAGE, FULL_IMAGE, FRAME, POSE = 1, 3, 2, 1


def rotation(rs):
    ax = rs.randn(3)
    ax /= np.linalg.norm(ax)
    ang = rs.uniform(0.3, 1.2)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def scene(rs):
    extr = np.stack([np.eye(4) for _ in range(N)])
    intr = np.zeros((N, 3, 3))
    for i in range(N):
        extr[i, :3, :3] = rotation(rs)
        extr[i, :3, 3] = rs.uniform(-1.0, 1.0, 3)
        intr[i] = [[23.0 + i, 0.0, 0.5 * W + 1.3 - 0.4 * i], [0.0, 19.5 - 0.7 * i, 0.5 * H - 0.8 + 0.3 * i], [0.0, 0.0, 1.0]]
    poses = np.stack([np.eye(4) for _ in range(3)])
    for k in range(3):
        poses[k, :3, :3] = rotation(rs)
        poses[k, :3, 3] = rs.uniform(-1.0, 1.0, 3)
    images_u8 = rs.randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)
    masks = (rs.rand(N, H, W) < 0.45).astype(np.float32)                   # 1 = human pixel (dropped), < 1 = background ray (kept)
    soft = rs.rand(N, H, W) < 0.1
    masks[soft] = rs.uniform(0.05, 0.95, size=int(soft.sum())).astype(np.float32)   # anti-aliased mask edges are kept (mask < 1)
    masks[ZERO_IMAGE] = 1.0
    masks[FULL_IMAGE] = 0.0
    for i in (0, 2, 4):
        masks[i, H - 1, 3], masks[i, H - 1, W - 1], masks[i, 5, W - 1], masks[i, 0, 0] = 0.0, 0.0, 0.0, 1.0
    return extr, intr, poses, images_u8, masks


def main():
    rs = np.random.RandomState(20240521)
    extr, intr, poses, images_u8, masks = scene(rs)
    times = np.linspace(0.0, 1.0, N).astype(np.float32)
    render_times = np.linspace(0.0, 1.0, len(poses)).astype(np.float32)
    with refload.stage(1):
        di = importlib.import_module("src.data.interface")
        sm = importlib.import_module("src.data.sampler")
        lit = di.LitData("unused", batch_size=16, load_radii=True, batch_sampler="single_image")
        lit.extrinsics, lit.intrinsics = extr, intr
        lit.image_sizes = np.array([[H, W] for _ in range(N)])
        lit.images = (images_u8 / 255.0).astype(np.float32)                  # the loader's `imageio.imread(f) / 255.0` as float32
        lit.masks, lit.times, lit.render_times = masks, times, render_times
        lit.ndc_coeffs, lit.num_devices = (-1.0, -1.0), 1
        lit.normals = lit.multlosses = None
        lit.bkgrays_sizes = np.sum(masks < 1, axis=(1, 2))
        train, _ = lit.split_each(lit.images, lit.masks, None, None, I_TRAIN, dummy=False)
        frame, _ = lit.split_each_val(lit.images, None, None, np.array([FRAME]), dummy=False)
        pose, _ = lit.split_each_val(None, None, poses[..., :4], np.arange(len(poses)), dummy=False)      # every camera of the path, in order
        sampler = sm.SingleImageDDPSampler(batch_size=16, num_replicas=1, rank=0, N_img=len(I_TRAIN),
                                           N_pixels=lit.bkgrays_sizes[I_TRAIN], epoch_size=6, tpu=False, precrop=False, precrop_steps=0)
        # the reference's np.random.choice over an empty range raises when a step picks the zero-count image: take the first seed
        # whose epoch never picks it
        seed = 11
        while True:
            np.random.seed(seed)
            try:
                sampler_idx = np.stack(list(iter(sampler)))
                break
            except ValueError:
                seed += 1

    def table(prefix, rs_):
        out = {f"{prefix}_rays_o": rs_.rays_o, f"{prefix}_rays_d": rs_.rays_d, f"{prefix}_viewdirs": rs_.viewdirs,
               f"{prefix}_radii": rs_.radii, f"{prefix}_times": rs_.times}
        if rs_.images is not None:
            out[f"{prefix}_target"] = rs_.images.astype(np.float32)
        return {k: np.asarray(v, np.float32) for k, v in out.items()}

    out = {"extrinsics": extr, "intrinsics": intr, "render_poses": poses, "times": times, "render_times": render_times,
           "images_u8": images_u8, "masks": masks, "i_train": I_TRAIN, "i_test": I_TEST, "counts": lit.bkgrays_sizes.astype(np.int64),
           "zero_image": ZERO_IMAGE, "full_image": FULL_IMAGE, "frame": FRAME, "pose": POSE, "sampler_idx": sampler_idx.astype(np.int64),
           "sampler_seed": seed}
    out.update(table("train", train))
    out.update(table("frame", frame))
    out.update(table("pose", pose))
    path = os.path.join(HERE, "stage1_rays.npz")
    np.savez_compressed(path, **out)
    print("stage1_rays.npz:", len(train), "training rays, counts", lit.bkgrays_sizes.tolist(), "frame", len(frame), "pose", len(pose),
          "sampler", sampler_idx.shape, "seed", seed, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
