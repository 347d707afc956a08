"""The expectation for the stage-1 maps (`hos_volrender_maps_fwd`), restated from the reference's own functions and pinned to them by
tests/golden/bkgd_maps.npz (tests/test_bkgd_maps_cpu.py): opacity `acc = sum w` (stage 1's helper.py:233), expected distance
`depth = sum w (t_s + t_{s+1}) / 2` and the median distance `sorted_interp(0.5, integrate_weights(w), tdist)` (helper.py:166-190),
plus the piecewise-linear CDF in fp64 in which the GPU tests judge the median (tests/test_gpu_bkgd_maps.py)."""
import os

import numpy as np
import torch

import oracle.background as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "bkgd_maps.npz")
MODEL_CASES = (("s32", 7, 32, True), ("s64", 7, 64, True), ("s200", 5, 200, False))        # tag, B, S, opaque_background
HAND_CASES = (("hand_opaque", 3, 32, True), ("hand_clear", 3, 32, False))
CASES = MODEL_CASES + HAND_CASES
BG = 1.0                                                                                    # bg_intensity_range of the shipped configuration


def integrate_weights(w):
    """helper.py:166-173: [0, clip(cumsum(w[:-1]), max=1), 1]."""
    cw = torch.cumsum(w[..., :-1], dim=-1).clip(max=1.0)
    z = torch.zeros_like(w[..., :1])
    return torch.cat([z, cw, torch.ones_like(z)], dim=-1)


def weights_from_density(density, tdist, dirs, opaque, dtype):
    return ob.compute_alpha_weights(density.to(dtype), tdist.to(dtype), dirs.to(dtype), bool(opaque))[0]


def expected_maps(rgbs, weights, tdist, bg, dtype):
    """What one ray batch renders to in `dtype`, from the tensors the kernel receives: `rgb` [B,3], `acc`, `depth`, `depth_median` [B],
    `bin` [B] (the median's interval: the last knot whose CDF is <= 0.5), `cw` [B,S+1] and `depth_scale` = sum w |t_mid|."""
    col, w, t = rgbs.to(dtype), weights.to(dtype), tdist.to(dtype)
    t_mid = (t[..., 1:] + t[..., :-1]) / 2
    cw = integrate_weights(w)
    half = torch.full(w.shape[:-1] + (1,), 0.5, dtype=dtype)
    median, k = ob.sorted_interp_indexed(half, cw, t)
    return {"rgb": ob.volumetric_rendering(col, w, bg), "acc": w.sum(dim=-1), "depth": (w * t_mid).sum(dim=-1),
            "depth_scale": (w * t_mid.abs()).sum(dim=-1), "depth_median": median[..., 0], "bin": k[..., 0], "cw": cw}


def cdf_at(t, tdist, cw, clamp=False):
    """The fp64 CDF (knots `tdist`, values `cw`, linear in between) at the distances `t` [B]: (F [B], slope [B]).  A distance that
    coincides with knots a..b-1 takes the value of [cw_a, cw_{b-1}] closest to 0.5 (every value of a zero-width interval counts)
    and slope 0; `t` outside [t_0, t_S] raises, or with `clamp` (knots of another run of the same ray) is moved to the nearer end."""
    t, tdist, cw = (np.asarray(x, dtype=np.float64) for x in (t, tdist, cw))
    if clamp:
        t = np.clip(t, tdist[:, 0], tdist[:, -1])
    F, slope = np.zeros_like(t), np.zeros_like(t)
    for r in range(t.shape[0]):
        a, b = int(np.sum(tdist[r] < t[r])), int(np.sum(tdist[r] <= t[r]))
        if b > a:
            F[r] = min(max(0.5, cw[r, a]), cw[r, b - 1])
        else:
            if a == 0 or a == tdist.shape[1]:
                raise AssertionError(f"ray {r}: t = {t[r]!r} outside [{tdist[r, 0]!r}, {tdist[r, -1]!r}]")
            j = a - 1
            slope[r] = (cw[r, j + 1] - cw[r, j]) / (tdist[r, j + 1] - tdist[r, j])
            F[r] = cw[r, j] + (t[r] - tdist[r, j]) * slope[r]
    return F, slope


def load_case(tag):
    """The fixture's tensors of one case: inputs `tdist`, `rgb`, `density`, `dirs`, `opaque` and the reference's outputs
    `w32/w64`, `rgb32/rgb64`, `med32/med64`, `bin32/bin64`."""
    g = np.load(FIXTURE)
    p = tag + "_"
    return {k[len(p):]: (torch.from_numpy(g[k]) if g[k].ndim else g[k].item()) for k in g.files if k.startswith(p)}
