"""Stage-1 training / evaluation rays of a scene directory, resident on the device (hos_raybank.hip).

The reference's stage-1 data module (1st_State-Conditional_Scene/src/data/interface.py:105-205 `split_each` over
src/data/ray_utils.py:34-139 `batchified_get_rays`) builds a HOST table of every unmasked ray of the training split -- rays_o,
rays_d, viewdirs, radii, times: 44 bytes per ray, about 27 GB for 300 frames of 1080p -- and `SingleImageDDPSampler`
(src/data/sampler.py:52-101, the sampler the Backpack gin binds) indexes it from DataLoader workers every step.  `RayBank` keeps
what the table is computed FROM: the 8-bit images, a camera table, the frame times and, per image, the list of kept pixels
(`mask < 1`) in pixel order, built once by `hos_raybank_index`.  A batch is drawn as (image, rank in the image's list) on the device
and its rays are rebuilt from the pixels by `hos_raybank_gather`; whole frames (`split_each_val`: the test split, the render path)
come from `hos_raybank_frame` chunk by chunk.  Pinned against the reference's own tables by tests/golden/stage1_rays.npz."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from ._lib import call, ptr

INDEX_BLOCK = 256          # pixels per workgroup of hos_raybank_index (RB_BLOCK in hos_raybank.hip): sizes its scratch
BATCH_KEYS = ("rays_o", "rays_d", "viewdirs", "radii", "times", "target")


def camera_rows(extrinsics, intrinsics) -> np.ndarray:
    """[M,16] fp32 rows of the camera table: camera-to-world 3x4 row-major, then fx, fy, cx, cy."""
    e = np.asarray(extrinsics, dtype=np.float64)
    k = np.asarray(intrinsics, dtype=np.float64)
    if e.ndim == 2:
        e, k = e[None], k[None]
    rows = np.concatenate([e[:, :3, :4].reshape(len(e), 12), k[:, 0, 0:1], k[:, 1, 1:2], k[:, 0, 2:3], k[:, 1, 2:3]], axis=1)
    return np.ascontiguousarray(rows, dtype=np.float32)


def to_uint8(images) -> np.ndarray:
    """Decoded pixels as the 8-bit values they were read from: uint8 stays, floats in 0..1 (`u / 255`, what
    `freeview.load_scene_pixels` and the reference's loader hold) are rounded back.  The kernels return `float32(u) / 255`."""
    a = np.asarray(images)
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(np.rint(a.astype(np.float64) * 255.0).clip(0, 255).astype(np.uint8))


def deal_frames(n: int, rank: int, world: int):
    """Whole frames dealt round-robin over the ranks (as `run.render_tpose` deals its cameras): rank r takes k % world == r."""
    return list(range(rank, n, world))


class RayBank:
    """Device-resident stage-1 rays of one scene.

    `scene` is `formats.load_scene` output (needs `bkgrays_sizes`, i.e. `load_scene(..., masks=...)`), `images` [N,H,W,3] uint8 or
    floats in 0..1, `masks` [N,H,W] floats in 0..1 (a pixel is a training ray where `mask < 1`, interface.py:145-146).  `split`
    names the images `sample` draws from: "train" (`i_split[0]`), "test" (`i_split[2]`), "all", or an explicit index array.
    Holds `images` uint8 [N,H,W,3], `cams` [N,16], `times` [N], `pix` int32 [sum counts], `counts` int32 [N] and `offsets` int64
    [N+1] on the device, `counts_host` / `offsets_host` as numpy.  The uint8 `keep` plane is uploaded for the index pass only."""

    def __init__(self, scene: Dict, images, masks, device="cuda", split="train"):
        self.device = dev = torch.device(device)
        img8 = to_uint8(images)
        N, H, W = img8.shape[:3]
        if img8.shape != (N, H, W, 3) or N < 1:
            raise ValueError(f"images must be [N,H,W,3], got {img8.shape}")
        keep = np.asarray(masks, dtype=np.float32) < 1                       # `masks_idx = _masks_idx < 1`
        if keep.shape != (N, H, W):
            raise ValueError(f"masks must be [{N},{H},{W}], got {keep.shape}")
        self.N, self.H, self.W = N, H, W
        self.scene = scene
        self.intrinsics = np.asarray(scene["intrinsics"], dtype=np.float64)
        self.extrinsics = np.asarray(scene["extrinsics"], dtype=np.float64)
        self.times_host = np.asarray(scene["times"], dtype=np.float32)
        self.render_poses = np.asarray(scene["render_poses"], dtype=np.float64) if scene.get("render_poses") is not None else None
        self.render_times = np.asarray(scene["render_times"], dtype=np.float32) if scene.get("render_times") is not None else None
        self.cams_host = camera_rows(self.extrinsics, self.intrinsics)
        if len(self.cams_host) != N or len(self.times_host) != N:
            raise ValueError("the scene's cameras / times and the images differ in number")
        i_train, _, i_test, i_all = scene["i_split"]
        self.i_train, self.i_test = np.asarray(i_train, dtype=np.int64), np.asarray(i_test, dtype=np.int64)
        if isinstance(split, str):
            split = {"train": i_train, "test": i_test, "all": i_all}[split]
        self.split = np.asarray(split, dtype=np.int64)

        self.images = torch.from_numpy(img8).to(dev)
        self.cams = torch.from_numpy(self.cams_host).to(dev)
        self.times = torch.from_numpy(self.times_host).to(dev)
        total = int(keep.sum())
        keep_dev = torch.from_numpy(keep.astype(np.uint8)).to(dev)
        self.pix = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        self.cap = total
        self.counts = torch.empty(N, dtype=torch.int32, device=dev)
        self.offsets = torch.empty(N + 1, dtype=torch.int64, device=dev)
        ws = torch.empty(N * ((H * W + INDEX_BLOCK - 1) // INDEX_BLOCK), dtype=torch.int32, device=dev)
        call("hos_raybank_index", keep_dev.data_ptr(), N, H, W, ptr(self.pix, torch.int32), total, ptr(self.counts, torch.int32),
             ptr(self.offsets, torch.int64), ptr(ws, torch.int32))
        self.counts_host = self.counts.cpu().numpy()                          # (synchronises: keep_dev / ws outlive the launches)
        self.offsets_host = self.offsets.cpu().numpy()
        del keep_dev, ws
        want = np.asarray(scene["bkgrays_sizes"]).astype(np.int64)
        if not np.array_equal(self.counts_host.astype(np.int64), want):
            raise AssertionError(f"hos_raybank_index counts {self.counts_host.tolist()} != bkgrays_sizes {want.tolist()}")
        assert int(self.offsets_host[-1]) == total
        # images `sample` may choose: the split's images that own at least one ray
        self.choice_host = self.split[self.counts_host[self.split] > 0]
        self.choice = torch.from_numpy(self.choice_host.astype(np.int32)).to(dev)

    # ------------------------------------------------------------------------------------------ batches
    def _empty(self, n: int, target: bool) -> Dict[str, torch.Tensor]:
        dev = self.device
        out = {"rays_o": torch.empty(n, 3, device=dev), "rays_d": torch.empty(n, 3, device=dev), "viewdirs": torch.empty(n, 3, device=dev),
               "radii": torch.empty(n, 1, device=dev), "times": torch.empty(n, device=dev)}
        if target:
            out["target"] = torch.empty(n, 3, device=dev)
        return out

    def gather(self, img_id: torch.Tensor, rank_in_image: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The rays (image `img_id[r]`, entry `rank_in_image[r]` of its list), both int32 [B] on the device: the stage-1 batch dict."""
        B = int(img_id.shape[0])
        out = self._empty(B, True)
        if B > 0:
            call("hos_raybank_gather", ptr(self.cams), ptr(self.times), self.images.data_ptr(), ptr(self.pix, torch.int32),
                 ptr(self.offsets, torch.int64), ptr(self.counts, torch.int32), ptr(img_id, torch.int32), ptr(rank_in_image, torch.int32),
                 B, self.N, self.H, self.W, self.cap, ptr(out["rays_o"]), ptr(out["rays_d"]), ptr(out["viewdirs"]), ptr(out["radii"]),
                 ptr(out["times"]), ptr(out["target"]))
        return out

    def draw(self, batch_size: int, generator: torch.Generator):
        """One step's draw of `SingleImageDDPSampler.__iter__` (sampler.py:73-95), on the device and without a read-back: one image
        of the split, uniformly, and `batch_size` ranks in its list with replacement.  Returns (image id int32 [1], ranks int32
        [batch_size]); every rank of a data-parallel group that seeds `generator` alike gets the same draw."""
        if len(self.choice_host) == 0:
            raise ValueError("RayBank.sample: no image of the split has a kept pixel")
        dev = self.device
        j = torch.randint(1 << 62, (1,), generator=generator, device=dev) % len(self.choice_host)
        img = self.choice[j]                                                                   # [1] int32
        cnt = self.counts[img.long()].long()                                                   # [1], > 0
        # a 62-bit draw modulo the count: the bias is below count / 2^62
        k = (torch.randint(1 << 62, (int(batch_size),), generator=generator, device=dev) % cnt).to(torch.int32)
        return img, k

    def sample(self, batch_size: int, generator: torch.Generator, rank: int = 0, world: int = 1) -> Dict[str, torch.Tensor]:
        """One training batch as `SingleImageDDPSampler` forms it (sampler.py:73-96): ONE image of the split chosen uniformly,
        `batch_size` entries of its ray list drawn with replacement, and this rank's share `[rank::world]` of that one draw -- so all
        ranks must seed `generator` alike.  The draws come from a device `torch.Generator`; numpy's random stream is not matched.

        One deliberate difference: images without a kept pixel are left out of the image choice (the reference would raise in
        `np.random.choice` over an empty range when it picks one).

        Returns the stage-1 batch dict with the reference's keys: `rays_o`, `rays_d`, `viewdirs` [B,3], `radii` [B,1], `times` [B],
        `target` [B,3] (B = len(range(rank, batch_size, world)))."""
        img, k = self.draw(batch_size, generator)
        k = k[rank::world].contiguous()
        return self.gather(img.expand(k.shape[0]).contiguous(), k)

    # ------------------------------------------------------------------------------------------ whole frames
    def _frame(self, cam16: np.ndarray, time: float, start: int, n: int, image: Optional[torch.Tensor]) -> Dict[str, torch.Tensor]:
        HW = self.H * self.W
        if n is None:
            n = HW - start
        if start < 0 or n < 0 or start + n > HW:
            raise ValueError(f"pixels [{start}, {start + n}) leave the {self.H} x {self.W} frame")
        out = self._empty(n, image is not None)
        if n > 0:
            cam16 = np.ascontiguousarray(cam16, dtype=np.float32)
            call("hos_raybank_frame", cam16.ctypes.data_as(ctypes.c_void_p).value, float(time), self.H, self.W, int(start), int(n),
                 0 if image is None else image.data_ptr(), ptr(out["rays_o"]), ptr(out["rays_d"]), ptr(out["viewdirs"]), ptr(out["radii"]),
                 ptr(out["times"]), ptr(out.get("target")))
        return out

    def frame(self, i: int, start: int = 0, n: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Pixels [start, start + n) of scene image i with its own camera and time, unmasked (`split_each_val`, interface.py:207-296):
        the batch dict with `target`.  n = None: to the end of the frame."""
        return self._frame(self.cams_host[i], float(self.times_host[i]), start, n, self.images[i])

    def render_pose(self, k: int, start: int = 0, n: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Pixels [start, start + n) of camera k of the render path (`render_poses[k]`, `render_times[k]`, the intrinsics of image 0:
        interface.py:227-234): the batch dict without `target`."""
        cam = camera_rows(self.render_poses[k], self.intrinsics[0])[0]
        return self._frame(cam, float(self.render_times[k]), start, n, None)

    def truth(self, i: int) -> torch.Tensor:
        """[H*W,3] pixels of image i as the kernels report them (`float32(u) / 255`)."""
        return self.images[i].reshape(-1, 3).float() / 255.0
