"""Stage-3 training on the foreground rays only (ops.LIVE_RAYS; M:1547-1551): ray selection against the z-merge's own decision,
the gather / scatter pair, the device-side row bound of every kernel of the canonical-MLP path, and the whole step against the
all-rays path (eager, without a live ray, and as a captured graph whose live count changes between replays)."""
import json
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hosnerf_amd import synth

S = 128
THR = 5e-3
CAP = 32768           # 256 rays x 128 samples: the smallest capacity at which the thin fast kernels and 256-block slabs are taken
BOUNDS = [0, 128, 16384 + 128, 32768]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


@pytest.fixture(scope="module")
def hos(dev):
    from hosnerf_amd.hosnerf import HOSNeRF
    from hosnerf_amd.human_nerf import default_cfg
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    cfg = default_cfg(d)
    cfg.perturb = 1.0
    m = HOSNeRF(cfg)
    m.model.load_state_dict(synth.background_state_dict(777, 2), strict=False)
    m.human.load_state_dict(synth.human_state_dict(777, 2), strict=True)
    return m.to(dev)


# ---------------------------------------------------------------------------------------------- 1. selection
def _merge_flags(mask, dev):
    """idx_fg of ops.merge_composite on `mask` [B, S] (every other input arbitrary but valid)."""
    from hosnerf_amd import ops
    B = mask.shape[0]
    g = torch.Generator().manual_seed(11)
    Sb = 32
    td = torch.sort(torch.rand(B, Sb + 1, generator=g) * 3 + 0.2, -1).values
    brgb, bden = torch.rand(B, Sb, 3, generator=g), torch.rand(B, Sb, generator=g) * 2
    hum = torch.rand(B, S, 4, generator=g)
    o = torch.randn(B, 3, generator=g) * 0.1
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * 0.7
    zt = torch.sort(torch.rand(B, S, generator=g) * 3 + 0.2, -1).values
    pts = o[:, None] + d[:, None] * zt[..., None]
    with torch.no_grad():
        out = ops.merge_composite(td.to(dev), brgb.to(dev), bden.to(dev), hum.to(dev), pts.to(dev), mask, o.to(dev), d.to(dev),
                                  torch.eye(4).to(dev))
    return out[2]


def _hand_made_mask():
    thr = np.float32(THR)
    below, above = np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(1))
    m = np.zeros((64, S), np.float32)
    m[1] = 1.0                                          # all ones
    m[2, 5], m[3, 5], m[4, 5] = below, thr, above        # one value: the sum IS the value
    m[5, 100], m[6, 100], m[7, 100] = below, thr, above  # ... on a lane-strided second pass (s >= 64)
    # 128 equal values: every partial sum of the lane-strided order and of the xor tree is a power-of-two multiple, hence exact
    m[8], m[9], m[10] = below / 128, thr / 128, above / 128
    m[11, 64:] = 3.0                                     # large values on s >= 64 only
    m[12, :64] = 3.0
    m[13, 127] = 1e-2
    m[14] = 1e-6                                         # 128e-6 < thr
    m[15] = 1e-4                                         # 1.28e-2 > thr
    rs = np.random.RandomState(3)
    m[16:40] = rs.uniform(0, 2 * THR / S, size=(24, S))  # sums scattered around the threshold
    m[40:56] = rs.uniform(0, 1, size=(16, S)) * (rs.uniform(size=(16, S)) > 0.9)
    return m                                             # rays 0, 56..63: sum 0


@pytest.mark.parametrize("case", ["mixed", "all_dead", "all_live"])
def test_selection_equals_merge_decision(dev, case):
    from hosnerf_amd import ops
    m = _hand_made_mask()
    if case == "all_dead":
        m = np.minimum(m, np.float32(1e-6))
    if case == "all_live":
        m = m + np.float32(1e-3)
    mask = torch.from_numpy(m).to(dev)
    live = ops.select_live_rays(mask, THR)
    fg = _merge_flags(mask, dev)
    assert torch.equal(live.flag, fg)
    n = int(live.flag.sum())
    if case == "mixed":
        want = np.zeros(64, np.int32)
        want[[1, 4, 7, 10, 11, 12, 13, 15]] = 1
        assert np.array_equal(live.flag.cpu().numpy()[:16], want[:16]), live.flag.cpu().numpy()[:16]
        assert 8 < n < 56
    if case == "all_dead":
        assert n == 0
    if case == "all_live":
        assert n == 64
    ids = live.ray_ids.cpu().numpy()
    assert np.array_equal(ids[:n], np.nonzero(live.flag.cpu().numpy())[0])          # ascending = stable
    assert np.all(ids[n:] == -1)
    assert int(live.rows) == S * n


# ---------------------------------------------------------------------------------------------- 2. gather / scatter
@pytest.mark.parametrize("C", [1, 3, 4])
def test_gather_scatter_round_trip_and_autograd(dev, C):
    from hosnerf_amd import ops
    mask = torch.from_numpy(_hand_made_mask()).to(dev)
    live = ops.select_live_rays(mask, THR)
    B = 64
    n = int(live.flag.sum())
    g = torch.Generator(device=dev).manual_seed(C)
    src = torch.randn(B * S, C, device=dev, generator=g)
    packed = ops.gather_rays(src, live)
    fgrows = live.flag.bool().repeat_interleave(S)
    assert torch.equal(packed[:n * S], src[fgrows])                                 # live rays, in order
    assert torch.equal(packed[n * S:], torch.zeros_like(packed[n * S:]))            # the tail
    back = ops.scatter_rays(packed, live)
    assert torch.equal(back[fgrows], src[fgrows])                                   # round trip restores live rays exactly
    assert torch.equal(back[~fgrows], torch.zeros_like(back[~fgrows]))              # dead rays
    # a tail full of NaN (uninitialised rows behind the bound) must not leak into the scatter
    dirty = packed.clone()
    dirty[n * S:] = float("nan")
    assert torch.equal(ops.scatter_rays(dirty, live), back)
    # autograd: each is the other's backward
    go = torch.randn(B * S, C, device=dev, generator=g)
    a = src.clone().requires_grad_(True)
    ops.gather_rays(a, live).backward(go)
    assert torch.equal(a.grad, ops.scatter_rays(go, live))
    b = packed.clone().requires_grad_(True)
    ops.scatter_rays(b, live).backward(go)
    assert torch.equal(b.grad, ops.gather_rays(go, live))


# ---------------------------------------------------------------------------------------------- 3. row bound of each kernel
def _rows(r, dev):
    return torch.tensor([r], dtype=torch.int32, device=dev)


def _nan_tail(t, r):
    t = t.clone()
    t[r:] = float("nan")
    return t


@pytest.fixture(scope="module")
def operands(dev):
    """One set of operands for every bound (left unchanged): layer input X [CAP, 320] >= 0, weights, cotangents."""
    from hosnerf_amd import ops
    ops.set_gemm_mode(ops.GEMM_PLANES)
    g = torch.Generator(device=dev).manual_seed(41)
    X = torch.relu(torch.randn(CAP, 320, device=dev, generator=g))
    W = torch.randn(256, 320, device=dev, generator=g) / 16
    b = torch.randn(256, device=dev, generator=g) * 0.1
    dY = torch.randn(CAP, 256, device=dev, generator=g) * 1e-3
    # the N = 4 head: weight rows and cotangent columns >= 4 are zero by contract
    Wh = torch.zeros(32, 256, device=dev)
    Wh[:4] = torch.randn(4, 256, device=dev, generator=g) / 16
    dz8 = torch.zeros(CAP, 32, device=dev)
    dz8[:, :4] = torch.randn(CAP, 4, device=dev, generator=g) * 1e-3
    x3 = torch.randn(CAP, 3, device=dev, generator=g)
    y4 = torch.rand(CAP, 4, device=dev, generator=g)
    y4[:, 3] = torch.relu(y4[:, 3] - 0.3)
    g4 = torch.randn(CAP, 4, device=dev, generator=g)
    return {"X": X, "W": W, "b": b, "dY": dY, "Wh": Wh, "dz8": dz8, "x3": x3, "y4": y4, "g4": g4}


def _fwd(op, K, r, dev, bounded):
    """Y, bits of the ReLU layer [.., K] -> 256 over the first r rows: `bounded` = capacity CAP + device bound, else host M = r."""
    from hosnerf_amd import ops
    M = CAP if bounded else r
    X = (_nan_tail(op["X"], r) if bounded else op["X"][:r])[:, :K].contiguous()
    Y = torch.full((M, 256), float("nan"), device=dev)
    bits = torch.full((ops.thin_relu_bits(M, dev).numel(),), -21846, dtype=torch.int16, device=dev)
    ops.linear_fwd(X, K, op["W"][:, :K].contiguous(), op["b"], 256, Y, ops.EPI_RELU, relu_bits=bits, rows_dev=_rows(r, dev) if bounded else None)
    return Y, bits


@pytest.mark.parametrize("r", BOUNDS)
@pytest.mark.parametrize("K", [64, 256, 320])
def test_row_bound_thin_fwd(dev, operands, r, K):
    op = operands
    Y, bits = _fwd(op, K, r, dev, True)
    assert bool(torch.isnan(Y[r:]).all()), "rows behind the bound were written"
    assert bool((bits[r // 32 * 512:] == -21846).all()), "ReLU bits behind the bound were written"
    assert bool(torch.isfinite(Y[:r]).all())
    if r >= 16384:
        Yr, bitsr = _fwd(op, K, r, dev, False)
        assert torch.equal(Y[:r], Yr) and torch.equal(bits[:r // 32 * 512], bitsr)
    elif r > 0:
        want = torch.relu(op["X"][:r, :K].double() @ op["W"][:, :K].double().t() + op["b"].double())
        err = float((Y[:r].double() - want).abs().max())
        print(f"thin_fwd K={K} r={r}: err {err:.3e}")
        assert err < 2e-6 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("r", BOUNDS)
@pytest.mark.parametrize("with_bits", [True, False])
def test_row_bound_thin_dgrad(dev, operands, r, with_bits):
    from hosnerf_amd import ops
    op = operands
    W = op["W"][:, :256].contiguous()
    Y, bits = _fwd(op, 256, r, dev, True)                      # the layer whose ReLU mask the backward reads (N == K == 256)

    def run(bounded):
        M = CAP if bounded else r
        dY = _nan_tail(op["dY"], r) if bounded else op["dY"][:r].contiguous()
        dX = torch.full((M, 256), float("nan"), device=dev)
        ops.linear_dgrad(dY, W, 256, 256, dX, mask_bits=(bits if bounded else bits[:r // 32 * 512].contiguous()) if with_bits else None,
                         rows_dev=_rows(r, dev) if bounded else None)
        return dX

    dX = run(True)
    assert bool(torch.isnan(dX[r:]).all())
    assert bool(torch.isfinite(dX[:r]).all())
    if r >= 16384:
        assert torch.equal(dX[:r], run(False))
    elif r > 0:
        want = op["dY"][:r].double() @ W.double()
        if with_bits:
            want = want * (Y[:r] > 0)
        err = float((dX[:r].double() - want).abs().max())
        print(f"thin_dgrad bits={with_bits} r={r}: err {err:.3e}")
        assert err < 2e-5 * float(want.abs().max())


@pytest.mark.parametrize("r", BOUNDS)
def test_row_bound_head_dgrad(dev, operands, r):
    """The N = 4 head's input gradient (K = 32 reduction columns): the generic thin kernel, masked by the fp32 activations."""
    from hosnerf_amd import ops
    op = operands
    act = op["X"][:, :256].contiguous()

    def run(bounded):
        M = CAP if bounded else r
        dz = _nan_tail(op["dz8"], r) if bounded else op["dz8"][:r].contiguous()
        a = _nan_tail(act, r) if bounded else act[:r].contiguous()
        dX = torch.full((M, 256), float("nan"), device=dev)
        ops.linear_dgrad(dz, op["Wh"], 32, 256, dX, mask_src=a, rows_dev=_rows(r, dev) if bounded else None)
        return dX

    dX = run(True)
    assert bool(torch.isnan(dX[r:]).all())
    assert bool(torch.isfinite(dX[:r]).all())
    if r >= 16384:
        assert torch.equal(dX[:r], run(False))
    elif r > 0:
        want = (op["dz8"][:r].double() @ op["Wh"].double()) * (act[:r] > 0)
        err = float((dX[:r].double() - want).abs().max())
        print(f"head dgrad r={r}: err {err:.3e}")
        assert err < 2e-5 * float(want.abs().max())


@pytest.mark.parametrize("r", BOUNDS)
@pytest.mark.parametrize("K", [256, 64, 320])
def test_row_bound_wgrad_tr(dev, operands, r, K):
    """wgrad_tr_fast<8>, <2> and the 320-column form (256 + 64): slabs of all 256 workgroups are summed, whatever the bound."""
    from hosnerf_amd import ops
    op = operands
    X = _nan_tail(op["X"], r)[:, :K].contiguous()
    dY = _nan_tail(op["dY"], r)
    dW = torch.zeros(256, K, device=dev)
    db = torch.zeros(256, device=dev)
    ev = ops.KernelEvents()
    ops.set_kernel_events(ev)
    try:
        ops.linear_wgrad(dY, X, dW, db, 256, K, rows_dev=_rows(r, dev))
    finally:
        ops.set_kernel_events(None)
    assert all(k.startswith("wgrad_tr") for k in ev.records), list(ev.records)
    assert bool(torch.isfinite(dW).all()) and bool(torch.isfinite(db).all())
    if r == 0:
        assert not bool(dW.any()) and not bool(db.any()), "no live row: exactly zero"
        return
    want = op["dY"][:r].double().t() @ op["X"][:r, :K].double()
    wb = op["dY"][:r].double().sum(0)
    err, errb = float((dW.double() - want).abs().max()), float((db.double() - wb).abs().max())
    print(f"wgrad_tr K={K} r={r}: dW err {err:.3e} of {float(want.abs().max()):.3e}, db err {errb:.3e} of {float(wb.abs().max()):.3e}")
    assert err < 3e-5 * float(want.abs().max())
    assert errb < 3e-5 * float(wb.abs().max()) + 1e-8


@pytest.mark.parametrize("r", BOUNDS)
def test_row_bound_head_wgrad(dev, operands, r):
    from hosnerf_amd import ops
    op = operands
    act = _nan_tail(op["X"][:, :256].contiguous(), r)
    dz = _nan_tail(op["dz8"], r)
    dW = torch.zeros(32, 256, device=dev)
    db = torch.zeros(32, device=dev)
    ops.linear_wgrad(dz, act, dW, db, 4, 256, rows_dev=_rows(r, dev))
    assert bool(torch.isfinite(dW).all()) and bool(torch.isfinite(db).all())
    if r == 0:
        assert not bool(dW.any()) and not bool(db.any())
        return
    want = op["dz8"][:r, :4].double().t() @ op["X"][:r, :256].double()
    wb = op["dz8"][:r, :4].double().sum(0)
    err, errb = float((dW[:4].double() - want).abs().max()), float((db[:4].double() - wb).abs().max())
    print(f"head wgrad r={r}: dW err {err:.3e} of {float(want.abs().max()):.3e}, db err {errb:.3e}")
    assert err < 3e-5 * float(want.abs().max())
    assert errb < 3e-5 * float(wb.abs().max()) + 1e-8


@pytest.mark.parametrize("r", BOUNDS)
def test_row_bound_embed_fourier_and_rgbsigma_grad(dev, operands, r):
    from hosnerf_amd import ops
    op = operands

    def embed(bounded):
        M = CAP if bounded else r
        x = _nan_tail(op["x3"], r) if bounded else op["x3"][:r].contiguous()
        E = torch.full((M, 64), float("nan"), device=dev)
        CAT = torch.full((M, 320), float("nan"), device=dev)
        ops.embed_fourier(x, 10, ops.zero1(dev), E, CAT, rows_dev=_rows(r, dev) if bounded else None)
        return E, CAT

    def head(bounded):
        M = CAP if bounded else r
        g4 = _nan_tail(op["g4"], r) if bounded else op["g4"][:r].contiguous()
        y4 = _nan_tail(op["y4"], r) if bounded else op["y4"][:r].contiguous()
        dz = torch.full((M, 32), float("nan"), device=dev)
        ops.rgbsigma_grad(g4, y4, dz, rows_dev=_rows(r, dev) if bounded else None)
        return dz

    E, CAT = embed(True)
    dz = head(True)
    assert bool(torch.isnan(E[r:]).all()) and bool(torch.isnan(CAT[r:]).all()) and bool(torch.isnan(dz[r:]).all())
    assert bool(torch.isnan(CAT[:, 64:]).all())                # the h part of the concat row is not the embedder's
    assert bool(torch.isfinite(E[:r]).all()) and bool(torch.isfinite(CAT[:r, :64]).all()) and bool(torch.isfinite(dz[:r]).all())
    if r > 0:                                                  # the same kernel at every row count: bit-identical
        Er, CATr = embed(False)
        assert torch.equal(E[:r], Er) and torch.equal(CAT[:r, :64], CATr[:, :64])
        assert torch.equal(dz[:r], head(False))


# ---------------------------------------------------------------------------------------------- 4.-6. the step
GRAD_BOUND = 2e-5        # of max|ref|: the bound test_two_stream_step_equals_one_stream_step uses for order-dependent fp32 partial sums


def _item(seed, dev):
    from hosnerf_amd.train import batch_to_device, prepare_patch_targets
    b = synth.add_patch_supervision(synth.human_batch(256, seed=seed, time=0.5, is_train=True, iter_val=3e5), 1, 16, 9)
    return batch_to_device(prepare_patch_targets(b), dev)


@pytest.fixture(scope="module")
def draws(dev):
    g = torch.Generator().manual_seed(2)
    return torch.rand(256, 128, generator=g).to(dev), [torch.rand(256, generator=g).to(dev) for _ in range(3)]


def _step(hos, gb, draws, live, two_streams=None):
    """One forward + backward; returns the outputs the issue names and copies of both flat gradients."""
    from hosnerf_amd import ops
    from hosnerf_amd.train import stage3_losses
    keep = ops.LIVE_RAYS, hos.two_streams
    ops.LIVE_RAYS = live
    if two_streams is not None:
        hos.two_streams = two_streams
    try:
        hos.zero_grad()
        out = hos.render(gb, randomized=True, is_train=True, static_cycle=True, jitters=draws[1], t_rand=draws[0])
        loss, parts = stage3_losses(out, gb)
        loss.backward()
        res = {"rgb": out["rgb"].detach().clone(), "idx_fg": out["idx_fg"].clone(), "total_order": out["total_order"].clone(),
               "cycle_count": out["cycle_count"].clone(), "loss": loss.detach().clone(),
               **{"loss_" + k: v.detach().clone() for k, v in parts.items()},
               "g_bkg": hos.model.flat_grad.clone(), "g_human": hos.human.flat_grad.clone(),
               "live_ray_rows": out["live_ray_rows"].clone() if "live_ray_rows" in out else None}
    finally:
        ops.LIVE_RAYS, hos.two_streams = keep
        hos.zero_grad()
    return res


EXACT = ("rgb", "idx_fg", "total_order", "cycle_count", "loss", "loss_mse", "loss_flow", "loss_cycle")


def _assert_step_equal(got, ref, what):
    for k in EXACT:
        assert torch.equal(got[k], ref[k]), (what, k, got[k], ref[k])
    for k in ("g_bkg", "g_human"):
        diff, scale = float((got[k] - ref[k]).abs().max()), float(ref[k].abs().max())
        print(f"{what}: {k} max|diff| {diff:.3e}, max|ref| {scale:.3e}, ratio {diff / max(scale, 1e-300):.3e}")
        assert diff <= GRAD_BOUND * scale, (what, k, f"max|diff| {diff:.3e} > {GRAD_BOUND} * max|ref| {scale:.3e}")


@pytest.fixture(scope="module")
def step_ref(dev, hos, draws):
    """The all-rays step on the item of test_two_stream_step_equals_one_stream_step: computed once, shared, left unchanged."""
    gb = _item(9, dev)
    return gb, _step(hos, gb, draws, live=False, two_streams=False)


@pytest.mark.parametrize("two_streams", [False, True])
def test_step_equals_all_rays_step(dev, hos, draws, step_ref, two_streams):
    gb, ref = step_ref
    bg_share = 1.0 - float(ref["idx_fg"].float().mean())
    assert 0.1 <= bg_share <= 0.9, bg_share
    assert float(ref["g_human"].abs().max()) > 0 and float(ref["g_bkg"].abs().max()) > 0 and ref["live_ray_rows"] is None
    got = _step(hos, gb, draws, live=True, two_streams=two_streams)
    assert int(got["live_ray_rows"]) == S * int(ref["idx_fg"].sum())
    _assert_step_equal(got, ref, f"live rays, two_streams={two_streams}, background share {bg_share:.3f}")


def _mlp_grads(net):
    return [t for L in list(net._nr) + list(net._nrf) + list(net._cnl) for t in net._w(L, grad=True) if t is not None]


def test_step_without_a_live_ray(dev, hos, draws):
    """All rays aimed away from the subject (the `nofg` item of test_stage3_step_vs_golden): rows_live == 0."""
    gb = dict(_item(9, dev))
    gb["near"] = gb["near"] + 50.0
    gb["far"] = gb["far"] + 50.0
    ref = _step(hos, gb, draws, live=False)
    from hosnerf_amd import ops
    keep = ops.LIVE_RAYS
    ops.LIVE_RAYS = True
    try:
        hos.zero_grad()
        out = hos.render(gb, randomized=True, is_train=True, static_cycle=True, jitters=draws[1], t_rand=draws[0])
        from hosnerf_amd.train import stage3_losses
        loss, _ = stage3_losses(out, gb)
        loss.backward()
        assert int(out["live_ray_rows"]) == 0 and int(out["idx_fg"].sum()) == 0 and int(out["cycle_count"]) == 0
        # (`deform_pts_final` is not in the list: rows behind `cycle_count` are unwritten storage on both paths)
        for k in ("rgb", "human_rgbsigma", "deform_pts_prev_final", "observe_pts", "human_weights_sorted"):
            assert bool(torch.isfinite(out[k]).all()), k
        assert torch.equal(out["rgb"], ref["rgb"])
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(hos.human.flat_grad).all()) and bool(torch.isfinite(hos.model.flat_grad).all())
        for t in _mlp_grads(hos.human):
            assert not bool(t.any()), "MLP gradient of the human module is not exactly zero without a live ray"
        assert float(hos.model.flat_grad.abs().max()) > 0
    finally:
        ops.LIVE_RAYS = keep
        hos.zero_grad()


def test_captured_step_follows_the_live_count(dev, hos, draws):
    """One captured step, replayed on two items with different live counts: the count is device data, not part of the capture."""
    from hosnerf_amd import ops
    from hosnerf_amd.train import stage3_losses
    gb = _item(9, dev)
    second = _item(10, dev)
    first = {k: v.clone() for k, v in gb.items() if isinstance(v, torch.Tensor)}
    keep = ops.LIVE_RAYS
    ops.LIVE_RAYS = True
    static = {}

    def fwd_bwd():
        hos.zero_grad()
        out = hos.render(gb, randomized=True, is_train=True, static_cycle=True, jitters=draws[1], t_rand=draws[0])
        loss, parts = stage3_losses(out, gb)
        loss.backward()
        static.update(rgb=out["rgb"], idx_fg=out["idx_fg"], total_order=out["total_order"], cycle_count=out["cycle_count"], loss=loss,
                      live_ray_rows=out["live_ray_rows"], **{"loss_" + k: v for k, v in parts.items()})

    def snapshot():
        return {**{k: v.detach().clone() for k, v in static.items()}, "g_bkg": hos.model.flat_grad.clone(), "g_human": hos.human.flat_grad.clone()}

    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                fwd_bwd()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fwd_bwd()
        graph.replay()
        rep1 = snapshot()
        # the second item, written into the captured step's input tensors in place
        n_over = 0
        for k, v in gb.items():
            if isinstance(v, torch.Tensor) and v.shape == second[k].shape and v.dtype == second[k].dtype:
                v.copy_(second[k])
                n_over += 1
        assert n_over >= 8
        graph.replay()
        rep2 = snapshot()
        torch.cuda.synchronize()
        assert int(rep1["live_ray_rows"]) != int(rep2["live_ray_rows"]), "the two items must differ in their live count"
        assert int(rep2["live_ray_rows"]) == S * int(rep2["idx_fg"].sum())
    finally:
        ops.LIVE_RAYS = keep
    # eager steps on the same (overwritten) inputs, then on the first item again
    want2 = _step(hos, gb, draws, live=True)
    _assert_step_equal(rep2, want2, "replay on the second item vs eager")
    for k, v in first.items():
        gb[k].copy_(v)
    want1 = _step(hos, gb, draws, live=True)
    _assert_step_equal(rep1, want1, "replay on the first item vs eager")
