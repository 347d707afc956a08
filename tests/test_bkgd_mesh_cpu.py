"""The background mesh without a GPU: the restatements of tests/_bkgd_mesh_expect.py against the oracle step by step, the isotropic
form var * J J^T the point encoder uses, the zero rim of the alpha rule, the argument checks of the new entry points, and the
launcher's refusals."""
import ctypes
import os
import tempfile

import numpy as np
import pytest
import torch

import oracle.background as ob
from tests import _bkgd_mesh_expect as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARS = (0.0, float(np.float32((2.0 / 256) ** 2 / 12)), float(np.float32(1e-2)))


def test_point_mix_has_every_kind():
    pts = E.point_mix(129).double()
    r = pts.norm(dim=1)
    assert bool((r == 0).any()) and bool(((r > 0) & (r < 1)).any()) and bool((r == 1).any()) and float(r.max()) > 10 and float(r.max()) <= 50
    assert torch.equal(E.point_mix(129), E.point_mix(129))


@pytest.mark.parametrize("var", VARS)
def test_restatement_is_the_oracle_chain(var):
    """`encode_points` equals contract -> lift_and_diagonalize -> integrated_pos_enc on covs = var * I, step by step."""
    pts = E.point_mix(65).double()
    basis = ob.generate_basis().double()
    covs = E.isotropic_covs(65, var)
    z, c = ob.contract(pts[None], covs)
    lm, lv = ob.lift_and_diagonalize(z, c, basis)
    want = ob.integrated_pos_enc(lm, lv, 0, 12)[0]
    got = E.encode_points(pts, var, basis)
    assert got.shape == (65, 504) and torch.equal(got, want)
    inside = pts.norm(dim=1) <= 1
    assert torch.equal(z[0][inside], pts[inside]) and torch.equal(c[0][inside], covs[0][inside])      # identity branch, the origin included
    if var == 0.0:
        sm = (lm[0][:, None, :] * (2.0 ** torch.arange(12, dtype=torch.float64))[:, None]).reshape(65, -1)
        assert torch.equal(got[:, :252], torch.sin(sm))                                                # a damping of exactly 1


@pytest.mark.parametrize("var", VARS)
def test_isotropic_form(var):
    """var * (J J^T) equals J (var I) J^T to float64 rounding, and the oracle's contracted covariance."""
    pts = E.point_mix(129).double()
    J = E.jacobian(pts)
    a = var * (J @ J.transpose(-1, -2))
    b = J @ (var * torch.eye(3, dtype=torch.float64)) @ J.transpose(-1, -2)
    scale = max(var, 1e-300) * float((J @ J.transpose(-1, -2)).abs().max())
    assert float((a - b).abs().max()) <= 8 * np.finfo(np.float64).eps * scale
    _, c = ob.contract(pts[None], E.isotropic_covs(129, var))
    assert float((a - c[0]).abs().max()) <= 8 * np.finfo(np.float64).eps * scale
    if var == 0.0:
        assert float(a.abs().max()) == 0.0


def test_alpha_rule_and_rim():
    dims = (7, 5, 4)
    rs = np.random.RandomState(3)
    density = rs.uniform(0.0, 40.0, 7 * 5 * 4).astype(np.float32)
    density[17] = np.inf
    h = np.float32(0.0625)
    rim = E.rim_mask(dims)
    assert rim.shape == (4, 5, 7) and int((~rim).sum()) == 5 * 3 * 2
    for dtype in (np.float64, np.float32):
        a = E.alpha_of_density(density, h, dims, dtype)
        assert a.dtype == dtype and a.shape == (4, 5, 7)
        assert (a[rim] == 0.0).all() and not np.signbit(a[rim]).any()                                  # exact +0 on the rim
        inner = a[~rim]
        assert (inner >= 0).all() and (inner <= 1).all() and inner.max() > 0.5
    a64 = E.alpha_of_density(density, h, dims)
    d = density.astype(np.float64).reshape(4, 5, 7)
    assert np.array_equal(a64[~rim], (1.0 - np.exp(-d * float(h)))[~rim])
    assert np.abs(E.alpha_of_density(density, h, dims, np.float32).astype(np.float64) - a64).max() < 2e-7


def test_new_entry_points_reject_bad_arguments():
    from hosnerf_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    a = ctypes.addressof(buf)
    assert lib.hos_encode_ipe_points(0, 4, 0.1, a, a, a, 576, 0) == -1 and lib.hos_encode_ipe_points(a, 4, 0.1, a, a, 0, 576, 0) == -1
    assert lib.hos_encode_ipe_points(a, 0, 0.1, a, a, a, 576, 0) == -1 and lib.hos_encode_ipe_points(a, 4, -1.0, a, a, a, 576, 0) == -1
    assert lib.hos_encode_ipe_points(a, 4, float("nan"), a, a, a, 576, 0) == -1
    assert lib.hos_encode_ipe_points(a, 4, 0.1, a, a, a, 567, 0) == -3 and lib.hos_encode_ipe_points(a, 2 ** 38, 0.1, a, a, a, 576, 0) == -3
    assert lib.hos_encode_ipe_points_planes(a, 4, 0.1, a, a, 0, 0, 576, 0) == -1 and lib.hos_encode_ipe_points_planes(0, 4, 0.1, a, a, a, a, 576, 0) == -1
    assert lib.hos_encode_ipe_points_planes(a, 4, 0.1, a, a, a, 0, 580, 0) == -3 and lib.hos_encode_ipe_points_planes(a, 4, 0.1, a, a, a, 0, 544, 0) == -3
    assert lib.hos_grid_alpha_density(0, 0.1, 4, 4, 4, 0, 4, a, 0) == -1 and lib.hos_grid_alpha_density(a, 0.1, 4, 4, 4, 0, 4, 0, 0) == -1
    assert lib.hos_grid_alpha_density(a, 0.1, 1, 4, 4, 0, 4, a, 0) == -3
    assert lib.hos_grid_alpha_density(a, 0.1, 4, 4, 4, 60, 5, a, 0) == -1 and lib.hos_grid_alpha_density(a, 0.1, 4, 4, 4, -1, 5, a, 0) == -1
    assert lib.hos_grid_alpha_density(a, 0.1, 4, 4, 4, 64, 0, a, 0) == 0                               # an empty range launches nothing


def test_launcher_bindings_and_refusals():
    import run as launcher
    for name, model in (("hosnerf_backpack.gin", "hosnerf"), ("state_mipnerf360_backpack.gin", "state_mipnerf360")):
        plan = launcher.main(["--ginc", os.path.join(ROOT, "configs", name), "--scene_name", "Backpack", "--cpu", "--logbase", tempfile.mkdtemp(),
                              "--ginb", "run.max_steps=3", "--ginb", "run.run_mesh_bkgd=True", "--ginb", "run.mesh_bkgd_box=(-2, -2, -1, 2, 2, 1.5)"])
        assert plan["model_name"] == model and plan["gin"]["run.run_mesh_bkgd"] is True
        assert tuple(plan["gin"]["run.mesh_bkgd_box"]) == (-2, -2, -1, 2, 2, 1.5)
    s2 = os.path.join(ROOT, "configs", "state_humanobject_backpack.gin")
    with pytest.raises(SystemExit) as e:                                            # stage 2 has no background
        launcher.main(["--ginc", s2, "--scene_name", "Backpack", "--cpu", "--logbase", tempfile.mkdtemp(), "--ginb", "run.max_steps=3",
                       "--ginb", "run.run_mesh_bkgd=True"])
    assert "run.run_mesh_bkgd" in str(e.value) and "stage 2" in str(e.value)
    s1 = os.path.join(ROOT, "configs", "state_mipnerf360_backpack.gin")
    for box in ("(-1, -1, -1, 1, -1, 1)", "(1, 1, 1, -1, -1, -1)", "(-1, -1, -1, 1, 1)", "(-1, -1, -1, 1, 1, 1e999)"):
        with pytest.raises(SystemExit) as e:                                        # an empty, short or non-finite box
            launcher.main(["--ginc", s1, "--scene_name", "Backpack", "--cpu", "--logbase", tempfile.mkdtemp(), "--ginb", "run.max_steps=3",
                           "--ginb", "run.run_mesh_bkgd=True", "--ginb", f"run.mesh_bkgd_box={box}"])
        assert "run.mesh_bkgd_box" in str(e.value), box
    assert launcher.mesh_bkgd_box({}) == [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
    with pytest.raises(SystemExit) as e:                                            # no scene directory
        launcher.extract_bkgd_meshes({}, None, "state_mipnerf360", None, "/nonexistent/last.ckpt", tempfile.mkdtemp(), "cpu", 0, 1)
    assert "--scene_dir" in str(e.value)
    with pytest.raises(SystemExit) as e:                                            # a scene, no checkpoint
        launcher.extract_bkgd_meshes({}, None, "state_mipnerf360", object(), "/nonexistent/last.ckpt", tempfile.mkdtemp(), "cpu", 0, 1)
    assert "last.ckpt" in str(e.value)


def test_bkgd_field_rejects_a_bad_box():
    from hosnerf_amd import mesh
    for box in ((0, 0, 0, 0, 1, 1), (0, 0, 0, 1, 1), (0, 0, 0, 1, 1, float("nan"))):
        with pytest.raises(ValueError):
            mesh.bkgd_field(None, box, 0.5, resolution=8)
    assert mesh.voxel_variance(0.125) == float(np.float32(0.125 * 0.125) / np.float32(12))
