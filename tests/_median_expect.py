"""The expectation for the median depth of stage-3 and human-only rays (`hos_merge_composite_median_fwd`, `hos_raw2outputs_median_fwd`).
The reference has no median for these composites; the definition is stage 1's, from the two functions tests/golden/bkgd_maps.npz pins to
the reference (`integrate_weights` of tests/_bkgd_maps_expect.py, `oracle.background.sorted_interp_indexed`), on the weights of
`_raw2outputs` (M:73-92) with the unbounded last interval collapsed to zero width:
    knots t = [z_0 .. z_{S-1}, z_{S-1}],  cw = [0, clip(cumsum(w[:-1]), max=1), 1],  depth_median = sorted_interp(0.5, cw, t).
Also the hand cases both kernels are held to exactly: masks (raw2outputs) / densities (merge, an all-background ray) whose weights are
exact in fp32, and the medians they must give."""
import numpy as np
import torch

import oracle.background as ob
from tests._bkgd_maps_expect import integrate_weights

SIGMA_OPAQUE = 1e30          # exp(-sigma * dist) == 0 in fp32 and fp64 for every dist used here: alpha == mask exactly


def median_definition(w, z):
    """(depth_median [B], knots t [B,S+1], cw [B,S+1]) in the dtype of `w`; `z` [B,S] sorted."""
    t = torch.cat([z, z[..., -1:]], -1).to(w.dtype)
    cw = integrate_weights(w)
    half = torch.full(w.shape[:-1] + (1,), 0.5, dtype=w.dtype)
    return ob.sorted_interp_indexed(half, cw, t)[0][..., 0], t, cw


def hand_depths(S):
    """z_j = 1 + j / 64: exact in fp32, as are all their differences and midpoints."""
    return 1.0 + torch.arange(S, dtype=torch.float64) / 64.0


def hand_cases(S):
    """name -> (mask [S] for `_raw2outputs` with sigma = SIGMA_OPAQUE, |d| = 1 and last_dist = 1, the weights [S] those masks give --
    exact in fp32: w_j = m_j prod_{i<j} (1 - m_i), every factor a multiple of 1/4, and 1 - m + 1e-10 rounds to 1 - m unless m = 1, after
    which every mask is 0 -- and the median the definition gives, as a Python float).  With S = 150 a lane holds three samples: sample
    2 is the last one of lane 0, sample 3 the first one of lane 1."""
    z = hand_depths(S).tolist()
    third = 1.0 / 3.0                                   # (0.5 - 0.25) / (1 - 0.25)
    spec = {
        "sample0":     ({0: 1.0},            {0: 1.0},               z[0] + 0.5 * (z[1] - z[0])),
        # cw = [0, .5, .5, 1, ..]: the reference's mask `0.5 >= cw` reaches knot 2, offset 0 in the interval of sample 2 (stage 1's `tie`)
        "tie":         ({0: 0.5, 2: 1.0},    {0: 0.5, 2: 0.5},       z[2]),
        "lane1_first": ({0: 0.25, 3: 1.0},   {0: 0.25, 3: 0.75},     z[3] + third * (z[4] - z[3])),
        "lane0_last":  ({0: 0.25, 2: 1.0},   {0: 0.25, 2: 0.75},     z[2] + third * (z[3] - z[2])),
        "last":        ({0: 0.25, S - 1: 1.0}, {0: 0.25, S - 1: 0.75}, z[S - 1]),
        "nowhere":     ({0: 0.25},           {0: 0.25},              z[S - 1]),                 # opacity 0.25: the last sample's depth
    }
    out = {}
    for name, (m, w, t) in spec.items():
        mask, wt = torch.zeros(S, dtype=torch.float64), torch.zeros(S, dtype=torch.float64)
        for j, v in m.items():
            mask[j] = v
        for j, v in w.items():
            wt[j] = v
        out[name] = (mask, wt, t)
    return out


def merge_hand_cases(Sb):
    """name -> (density [Sb] of an all-background ray with tdist = hand_depths(Sb + 1), |d| = 1, and the median).  A background
    sample's alpha is 1 - exp(-density * dist) with no mask, so the only weights exact in fp32 are 0 and 1: the crossing in sample 0,
    in the last sample of lane 0 / the first of lane 1 (Sb = 150), in the last sample, and nowhere (opacity 0); a knot at exactly 0.5
    and an opacity of 0.25 cannot be produced exactly through this entry and are covered by `hand_cases` through the same device function."""
    z = hand_depths(Sb).tolist()
    spec = {"sample0": (0, z[0] + 0.5 * (z[1] - z[0])), "lane1_first": (3, z[3] + 0.5 * (z[4] - z[3])),
            "lane0_last": (2, z[2] + 0.5 * (z[3] - z[2])), "last": (Sb - 1, z[Sb - 1]), "nowhere": (None, z[Sb - 1])}
    out = {}
    for name, (j, t) in spec.items():
        den = torch.zeros(Sb, dtype=torch.float64)
        if j is not None:
            den[j] = SIGMA_OPAQUE
        out[name] = (den, t)
    return out


def as_f32(x):
    return float(np.float32(x))
