"""The float64 references, inputs and the rank emulator of tests/_decoder_expect.py, checked on the CPU before
tests/test_gpu_decoder.py holds the volume-decoder kernels against them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _decoder_expect as X


def test_live_taps_are_the_layer_at_one_voxel_and_dead_taps_get_no_gradient():
    g = X.gen(1)
    Cin, Cout = 12, 5
    full = X.full_nonzero_ints(g, Cin, Cout, 4, 4, 4).double()
    assert bool((full != 0).all())
    x = X.ints(g, 1, Cin).double()
    b = X.ints(g, Cout).double()
    go = X.ints(g, 8, Cout).double()
    y, gx, gw, gb, _ = X.deconv(x, full, b, 1, False, go=go)
    wc = X.compact(full)
    assert wc.shape == (Cin, 8 * Cout)
    assert torch.equal((x @ wc).view(8, Cout) + b, y)                       # the product, viewed [8, Cout], IS the channel-last output
    live = torch.zeros(64, dtype=torch.bool)
    live[X.LIVE_TAPS] = True
    gw = gw.reshape(Cin, Cout, 64)
    assert bool((gw[:, :, ~live] == 0).all()) and bool((gw[:, :, live] != 0).any())
    assert torch.equal(X.compact(gw), x.t() @ go.reshape(1, 8 * Cout))      # the live-tap slice of the weight gradient
    assert torch.equal(gx, go.reshape(1, 8 * Cout) @ wc.t())
    assert torch.equal(gb, go.sum(0))
    from hosnerf_amd.human_nerf import Network
    assert list(Network._LIVE_TAPS) == X.LIVE_TAPS


def test_exact_inputs_equal_float64_in_float32():
    """fp32 conv_transpose3d on integer inputs == float64 (the premise of every bit-equality assertion), LeakyReLU included."""
    g = X.gen(2)
    D, Cin, Cout = 2, 512, 6
    x, w, b = X.ints(g, D ** 3, Cin), X.ints(g, Cin, Cout, 4, 4, 4), X.ints(g, Cout)
    y64 = X.deconv(x.double(), w.double(), b.double(), D, True)
    go = X.ints_for(g, y64)
    r64 = X.deconv(x.double(), w.double(), b.double(), D, True, go=go.double(), round32=True)
    r32 = X.deconv(x, w, b, D, True, go=go)
    assert bool((y64 < 0).any()) and bool((go.abs() > 4).any())
    for a, t in zip(r32[:4], r64[:4]):
        assert torch.equal(a, X.f32(t))
    # the slope on a multiple of 5 is an integer again
    j = torch.arange(-4, 5).float()
    assert torch.equal(X.f32((5 * j).double() * X.SLOPE), j) and torch.equal((5 * j) * np.float32(0.2), j)


def test_exact_budget_below_2_24_at_every_listed_shape():
    lim = 2 ** 24
    for K, N, _ in X.GEMV_SHAPES:
        assert X.exact_budget(K) + 4 < lim
    for M, K, N, _ in X.OUTER_SHAPES:
        assert X.exact_budget(M) + 4 < lim
    for N, K in X.ROWDOT_SHAPES:
        assert X.exact_budget(K) + 4 < lim and X.exact_budget(N) + 4 < lim          # forward / gx
    for D, Cin, Cout, _ in X.DECONV_SHAPES:
        assert 8 * X.exact_budget(Cin) + 4 < lim                                     # forward: 8 taps of Cin products
        assert X.exact_budget(Cout * 64) < lim                                       # input gradient
        assert 2 * X.exact_budget(D ** 3) + 4 < lim and 2 * 4 * 8 * D ** 3 + 4 < lim  # two backward passes onto G0: weight, bias
    for Cin, Cout in X.FIRST_SHAPES:
        assert X.exact_budget(Cin) + 4 < lim and X.exact_budget(8 * Cout) < lim
    for Cin, Cout, _ in X.SHARD_FIRST_SHAPES:
        assert X.exact_budget(Cin) + 4 < lim and X.exact_budget(8 * Cout) < lim
    for D, Cin, Cout, _ in X.SHARD_SHAPES:
        assert 8 * X.exact_budget(Cin) + 4 < lim and X.exact_budget(Cout * 64) < lim and X.exact_budget(D ** 3) + 4 < lim


def test_outer_accum_shapes_land_on_the_route_named_for_them():
    """gx * ceil(K / 32) < 256 -> 8 weight rows per thread, else 32 (hos_outer_accum): recomputed here, so a retuned threshold
    fails this test and the shapes get revisited.  Both routes must see a partial last k-block."""
    seen = {8: False, 32: False}
    for M, K, N, route in X.OUTER_SHAPES:
        gx = (N // 4 + 255) // 256
        assert (8 if gx * ((K + 31) // 32) < 256 else 32) == route == X.outer_accum_route(K, N), (M, K, N)
        seen[route] |= K % route != 0
    assert seen == {8: True, 32: True}
    # what ops.deconv3d passes at M = 8: K = Cin, N = Cout * 64
    assert X.outer_accum_route(64, 8 * 64) == 8 and X.outer_accum_route(512, 512 * 64) == 32
    assert X.outer_accum_route(1024, 8 * 512) == 8                       # the compact first layer


@pytest.mark.parametrize("C,V", X.SOFTMAX_SHAPES)
def test_softmax_inputs_keep_a_finite_logit_per_voxel(C, V):
    z, prior, cot = X.softmax_inputs(C, V)
    logit = z.double().t() + torch.log(prior.double())
    assert bool(torch.isfinite(logit).any(0).all()) and bool((prior[0] > 0).all())
    if C > 1:
        assert bool((prior[1:, ::5] == 0).all()) and bool(torch.isinf(logit).any())
    with np.errstate(over="ignore"):
        assert not bool(torch.isfinite(torch.exp(z.float())).all())      # without the max subtraction these overflow
    vol, gz = X.softmax(z.double(), prior.double(), cot.double())
    assert bool(torch.isfinite(vol).all()) and bool(torch.isfinite(gz).all())
    assert float((vol.sum(0) - 1).abs().max()) < 1e-12
    assert bool((vol[prior == 0] == 0).all()) and bool((gz.t()[prior == 0] == 0).all())
    # the closed form the backward kernel states
    want = vol * (cot.double() - (vol * cot.double()).sum(0))
    assert float((gz.t() - want).abs().max()) < 1e-12


def test_pair_and_channel_last_references():
    g = X.gen(3)
    C, Kb, V3 = 5, 3, 7
    vol = torch.randn(C, V3, generator=g)
    cl = X.channel_last(vol, Kb)
    assert cl.shape == (V3, 32) and torch.equal(cl[:, :Kb], vol[:Kb].t()) and bool((cl[:, Kb:] == 0).all())
    gv, gc = torch.randn(C, V3, generator=g), torch.randn(V3, 32, generator=g)
    volr = vol.clone().requires_grad_(True)
    (volr * gv).sum().backward(retain_graph=False)
    v2 = vol.clone().requires_grad_(True)
    ((v2 * gv).sum() + (X.channel_last(v2, Kb) * gc).sum()).backward()
    assert torch.allclose(X.pair_bwd(gv, gc, C, Kb), v2.grad, atol=1e-6)
    assert torch.equal(X.pair_bwd(gv, None, C, Kb), gv)
    assert torch.equal(X.pair_bwd(None, gc, C, Kb)[:Kb], gc[:, :Kb].t()) and bool((X.pair_bwd(None, gc, C, Kb)[Kb:] == 0).all())


def test_head_reference_is_linear_plus_leaky_relu():
    g = X.gen(4)
    N, K = 33, 300
    W, x, b, go = (torch.randn(N, K, generator=g).double(), torch.randn(K, generator=g).double(), torch.randn(N, generator=g).double(),
                   torch.randn(N, generator=g).double())
    Wr, xr, br = (t.clone().requires_grad_(True) for t in (W, x, b))
    y = F.leaky_relu(F.linear(xr[None], Wr, br), 0.2)[0]
    y.backward(go)
    # float32(0.2) = 0.2 (1 + 7.5e-9)
    assert float((X.head(x, W, b) - y.detach()).abs().max()) < 1e-8 * float(y.detach().abs().max())
    gW, gb, gx = X.head_bwd(go, y.detach(), x, W)
    for a, t in ((gW, Wr.grad), (gb, br.grad), (gx, xr.grad)):
        assert float((a - t).abs().max()) < 1e-6 * max(1.0, float(t.abs().max()))


@pytest.mark.parametrize("first", [False, True], ids=["general", "first"])
@pytest.mark.parametrize("world", [2, 4, 8])
def test_rank_emulator_sharded_model_equals_the_unsharded_layer(world, first):
    """A pure-torch sharded layer driven through the emulator == the unsharded layer on every rank: output, bias gradient, the
    gathered input gradient in channel order, and ROW OWNERSHIP of the weight gradient (other rows == G0)."""
    g = X.gen(10 * world + first)
    D, Cin, Cout, leaky = (1, 32, 3, True) if first else (2, 32, 3, True)
    x = X.ints(g, D ** 3, Cin).double()
    full = X.full_nonzero_ints(g, Cin, Cout, 4, 4, 4).double()
    if first:                                       # dead taps do not exist in the compact weight
        live = torch.zeros(64, dtype=torch.bool)
        live[X.LIVE_TAPS] = True
        full = (full.reshape(Cin, Cout, 64) * live).reshape(Cin, Cout, 4, 4, 4)
    b = X.ints(g, Cout).double()
    y_ref = X.deconv(x, full, b, D, leaky)
    go = X.ints_for(g, y_ref).double()
    y_ref, gx_ref, gw_ref, gb_ref, _ = X.deconv(x, full, b, D, leaky, go=go, round32=True)
    w2 = X.compact(full) if first else full.reshape(Cin, Cout * 64)
    gw_ref2 = X.compact(gw_ref) if first else gw_ref.reshape(Cin, Cout * 64)
    gw0, gb0 = X.ints(g, *w2.shape).double() + 0.5, X.ints(g, Cout).double() + 0.5
    emu = X.RankEmulator(world)
    res = emu.run(lambda comm: X.sharded_layer_model(comm, x, w2, b, D, leaky, go, gw0, gb0, first=first))
    assert emu.passes == 3 and [c["kind"] for c in emu.log] == ["sum", "gather"]
    cs = Cin // world
    assert bool((y_ref < 0).any())
    for r, (y, dx, gw, gb) in enumerate(res):
        assert torch.equal(y, y_ref) and torch.equal(dx, gx_ref) and torch.equal(gb, gb0 + gb_ref)
        own = torch.zeros(Cin, dtype=torch.bool)
        own[r * cs:(r + 1) * cs] = True
        assert torch.equal(gw[own], (gw0 + gw_ref2)[own]) and torch.equal(gw[~own], gw0[~own])


def test_rank_emulator_sums_in_rank_order_and_stacks():
    emu = X.RankEmulator(4)

    def fn(comm):
        t = torch.tensor([float(10 ** comm.rank)])
        comm.all_reduce_sum(t)
        return t, comm.all_gather(t * (comm.rank + 1))

    res = emu.run(fn)
    for r, (s, st) in enumerate(res):
        assert float(s) == 1111.0 and torch.equal(st.view(-1), torch.tensor([1111.0, 2222.0, 3333.0, 4444.0]))
