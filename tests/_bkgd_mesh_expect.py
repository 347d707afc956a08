"""Restatements for the background mesh (tests/test_bkgd_mesh_cpu.py checks their own properties; tests/test_gpu_bkgd_mesh.py holds
the kernels against them): the point-Gaussian encoding through the oracle's `encode_samples`, and the alpha-of-density rule with
its zero rim.  float64 is the reference value, float32 the same expressions in the device's number format."""
import numpy as np
import torch

import oracle.background as ob


def point_mix(P: int, seed: int = 0) -> torch.Tensor:
    """float32 [P,3], fixed seed, cycling through: the origin, inside the unit ball, exactly on |x| = 1 (an axis point: its fp32
    square sum is exactly 1), |x| up to 50 (a random direction times a radius in (1, 50])."""
    g = torch.Generator().manual_seed(1000 + seed)
    out = torch.zeros(P, 3)
    for p in range(P):
        kind = p % 4
        v = torch.randn(3, generator=g)
        v = v / v.norm()
        u = float(torch.rand(1, generator=g))
        if kind == 1:
            out[p] = v * (0.05 + 0.9 * u)
        elif kind == 2:
            out[p, int(3 * u) % 3] = 1.0 if u < 0.5 else -1.0
        elif kind == 3:
            out[p] = v * (1.0 + 49.0 * u)
    return out


def isotropic_covs(P: int, var: float, dtype=torch.float64) -> torch.Tensor:
    """[1,P,3,3]: var * I per point."""
    return (float(var) * torch.eye(3, dtype=dtype)).expand(1, P, 3, 3).contiguous()


def encode_points(pts, var: float, basis, dtype=torch.float64) -> torch.Tensor:
    """[P,504]: `oracle.background.encode_samples(means, var * I, basis)` -- contraction with J cov J^T, lift, IPE -- in `dtype`."""
    pts = torch.as_tensor(pts).to(dtype).reshape(1, -1, 3)
    return ob.encode_samples(pts, isotropic_covs(pts.shape[1], var, dtype), torch.as_tensor(basis).to(dtype))[0]


def jacobian(pts, dtype=torch.float64) -> torch.Tensor:
    """[P,3,3]: the closed-form Jacobian of the contraction (`oracle.background.contract`'s), the identity on |x|^2 <= 1."""
    x = torch.as_tensor(pts).to(dtype).reshape(-1, 3)
    r2 = (x * x).sum(-1, keepdim=True).clip(min=1e-32)
    r = torch.sqrt(r2)
    eye = torch.eye(3, dtype=dtype)
    J = ((2 * r - 1) / r2)[..., None] * eye + ((2 / (r2 * r) - 2 / r2) / r)[..., None] * (x[:, :, None] * x[:, None, :])
    return torch.where((r2 <= 1)[..., None], eye.expand_as(J), J)


def rim_mask(dims) -> np.ndarray:
    """bool [Nz,Ny,Nx]: the outermost vertex layer of a grid of dims (Nx,Ny,Nz)."""
    Nx, Ny, Nz = (int(d) for d in dims)
    rim = np.ones((Nz, Ny, Nx), dtype=bool)
    rim[1:-1, 1:-1, 1:-1] = False
    return rim


def alpha_of_density(density, h, dims, dtype=np.float64) -> np.ndarray:
    """[Nz,Ny,Nx]: 1 - exp(-density * h), every operation in `dtype`, exactly 0 on the rim."""
    Nx, Ny, Nz = (int(d) for d in dims)
    d = np.asarray(density, dtype=np.float32).astype(dtype).reshape(Nz, Ny, Nx)
    hh = dtype(np.float32(h))
    a = (dtype(1.0) - np.exp(-d * hh)).astype(dtype)
    a[rim_mask(dims)] = 0.0
    return a
