"""The motion-weight volume decoder, entry point by entry point (hos_deconv.hip and its autograd nodes in ops.py), against float64.

Exact inputs (integers in -4..4, tests/_decoder_expect.py): the kernel must be torch.equal to the float64 result cast to float32.
Random inputs: e_hip <= 8 e_ref + 4 * 2^-24 with e_ref the same operation in fp32 torch on the CPU; the measured worst factor of
every such test is recorded as `decoder.<test>` (tests/_record.py; the committed copy is profiles/decoder_parity.json).
Whatever a kernel is documented to write is NaN beforehand, whatever it accumulates into holds a known G0, and rows / columns it must
leave alone are compared bit for bit afterwards."""
import json
import math
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _decoder_expect as X
from tests._record import record

E_ARG, E_ALIGN, E_SHAPE = -1, -2, -3
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def call(name, *args):
    from hosnerf_amd import _lib
    _lib.call(name, *args)


def P(t, off=0):
    """device pointer of element `off` of a float32 tensor (None -> NULL); views with a row stride go through here"""
    return 0 if t is None else t.data_ptr() + 4 * off


def nans(dev, *shape):
    return torch.full(shape, NAN, device=dev)


def padded(dev, t, ld):
    """t [R, C] as the first C columns of a NaN-filled [R, ld] device buffer"""
    buf = nans(dev, t.shape[0], ld)
    buf[:, :t.shape[1]] = t.to(dev)
    return buf


def rejects(code, name, *args):
    from hosnerf_amd._lib import HosLibraryError
    with pytest.raises(HosLibraryError, match=f"code {code}:"):
        call(name, *args)


def same(a, t64):
    """bit-equal to the float64 value cast to float32"""
    return torch.equal(a.detach().cpu(), X.f32(t64))


class Parity:
    """Collects (quantity, e_hip, e_ref) of one random-input test; `finish` records the worst factor, then asserts every bound."""

    def __init__(self, err=X.err):
        self.rows, self.err = [], err

    def add(self, what, a, a32, t64, other=None):
        """a: the kernel's value, a32: fp32 torch's, t64: float64's.  other: a second kernel's value of the same quantity -- then
        e_hip is the distance between the two kernels (scaled like the error of either), e_ref still fp32 torch's from float64."""
        e_ref = self.err(a32, t64)
        e_hip = self.err(a, t64) if other is None else float((a.detach().double() - other.detach().double()).abs().max()) / max(1.0, float(t64.abs().max()))
        self.rows.append((X.factor(e_hip, e_ref), what, e_hip, e_ref))
        print(f"{what}: e_hip {e_hip:.3e} e_ref {e_ref:.3e} factor {self.rows[-1][0]:.2f}")

    def finish(self, key):
        f, what, e_hip, e_ref = max(self.rows)
        record("decoder." + key, {"worst_factor": f, "quantity": what, "e_hip": e_hip, "e_ref": e_ref, "quantities": len(self.rows)})
        for _, what, e_hip, e_ref in self.rows:
            assert e_hip <= X.bound(e_ref), (what, e_hip, e_ref)


# ====================================================================================================== 1. raw entry points
def _gemv(dev, x, W, bias, bias_mod, leaky, ldw=None, xoff=0):
    from hosnerf_amd import _lib
    K, N = W.shape
    ldw = ldw or N
    Wb = padded(dev, W, ldw)
    xb = nans(dev, xoff + K)
    xb[xoff:] = x.to(dev)
    nws = int(_lib.load().hos_gemv_ws_floats(K, N))
    assert nws == (K + 15) // 16 * N
    ws, y = nans(dev, nws), nans(dev, N + 8)
    bd = None if bias is None else bias.to(dev)
    call("hos_gemv_rowvec", P(xb, xoff), P(Wb), ldw, K, N, P(bd), bias_mod, 0.2, int(leaky), P(ws), P(y))
    assert bool(torch.isnan(y[N:]).all())
    return y[:N]


def _gemv_ref(x, W, bias, bias_mod, leaky):
    y = x @ W
    if bias is not None:
        y = y + bias[torch.arange(W.shape[1]) % bias_mod]
    return X.lrelu(y) if leaky else y


@pytest.mark.parametrize("K,N,bias_mod,ldw,xoff", [s + (None, 0) for s in X.GEMV_SHAPES[:3]] + [X.GEMV_SHAPES[3] + (320, 3)])
def test_gemv_rowvec_exact(dev, K, N, bias_mod, ldw, xoff):
    g = X.gen(K + N)
    x, W, b = X.ints(g, K), X.ints(g, K, N), X.ints(g, bias_mod)
    for bias in (b, None):
        for leaky in (0, 1):
            y = _gemv(dev, x, W, bias, bias_mod, leaky, ldw, xoff)
            want = _gemv_ref(x.double(), W.double(), None if bias is None else bias.double(), bias_mod, leaky)
            assert same(y, want), (bias is None, leaky)
            if leaky:
                assert bool((want < 0).any()) or N <= 8


def test_gemv_rowvec_random(dev):
    K, N, bias_mod = X.GEMV_SHAPES[2]
    g = X.gen(7)
    x, W, b = torch.randn(K, generator=g), torch.randn(K, N, generator=g) / math.sqrt(K), 0.1 * torch.randn(bias_mod, generator=g)
    par = Parity()
    for leaky in (0, 1):
        par.add(f"y[leaky={leaky}]", _gemv(dev, x, W, b, bias_mod, leaky), _gemv_ref(x, W, b, bias_mod, leaky),
                _gemv_ref(x.double(), W.double(), b.double(), bias_mod, leaky))
    par.finish("gemv_rowvec_random")          # measured worst e_hip / max(e_ref, 2^-24): 0.29; bound 8 e_ref + 4 * 2^-24


def test_gemv_rowvec_rejections(dev):
    t = torch.zeros(4096, device=dev)
    rejects(E_ALIGN, "hos_gemv_rowvec", P(t), P(t), 8, 16, 6, P(t), 1, 0.2, 0, P(t), P(t))
    rejects(E_ALIGN, "hos_gemv_rowvec", P(t), P(t), 1030, 2, 8, P(t), 1, 0.2, 0, P(t), P(t))
    rejects(E_ARG, "hos_gemv_rowvec", P(t), P(t), 8, 0, 8, P(t), 1, 0.2, 0, P(t), P(t))


def _outer(dev, x, dy, G0, ldx=None, lddy=None):
    """gW [K, ldw] (= G0's shape) += x^T dy through the library; x / dy sit in NaN-padded rows when ldx / lddy exceed K / N"""
    M, K = x.shape
    N = dy.shape[1]
    xb, dyb = padded(dev, x, ldx or K), padded(dev, dy, lddy or N)
    gW = G0.to(dev).clone()
    call("hos_outer_accum", P(xb), xb.stride(0), P(dyb), dyb.stride(0), P(gW), gW.stride(0), M, K, N)
    return gW


@pytest.mark.parametrize("M,K,N,route", X.OUTER_SHAPES)
def test_outer_accum_exact(dev, M, K, N, route):
    assert X.outer_accum_route(K, N) == route
    g = X.gen(M + K + N)
    x, dy, G0 = X.ints(g, M, K), X.ints(g, M, N), X.ints(g, K, N)
    gW = _outer(dev, x, dy, G0)
    assert same(gW, G0.double() + x.double().t() @ dy.double())


@pytest.mark.parametrize("M,K,N", [(8, 44, 1028), (3, 500, 16384)])
def test_outer_accum_leading_dimensions(dev, M, K, N):
    """ldx > K, lddy > N, ldw > N on both routes: the pad columns of gW hold G0 and come back bit-identical; the pads of x / dy are NaN."""
    assert X.outer_accum_route(K, N) == (8 if K == 44 else 32)
    g = X.gen(M + K)
    x, dy, G0 = X.ints(g, M, K), X.ints(g, M, N), X.ints(g, K, N + 12)
    gW = _outer(dev, x, dy, G0, ldx=K + 5, lddy=N + 8).cpu()
    assert same(gW[:, :N], G0[:, :N].double() + x.double().t() @ dy.double())
    assert torch.equal(gW[:, N:], G0[:, N:])


def test_outer_accum_random(dev):
    M, K, N, _ = X.OUTER_SHAPES[4]
    g = X.gen(11)
    x, dy, G0 = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g), X.ints(g, K, N)
    par = Parity()
    par.add("gW", _outer(dev, x, dy, G0), G0 + x.t() @ dy, G0.double() + x.double().t() @ dy.double())
    par.finish("outer_accum_random")          # measured worst e_hip / max(e_ref, 2^-24): 0.98; bound 8 e_ref + 4 * 2^-24


def test_outer_accum_rejections(dev):
    t = torch.zeros(65 * 8, device=dev)
    rejects(E_SHAPE, "hos_outer_accum", P(t), 8, P(t), 8, P(t), 8, 65, 8, 8)
    rejects(E_ALIGN, "hos_outer_accum", P(t), 8, P(t), 8, P(t), 8, 2, 8, 6)


def _rowdot_fwd(dev, x, W, b, ldw=None):
    N, K = W.shape
    Wb = padded(dev, W, ldw or K)
    y = nans(dev, N + 4)
    xd, bd = x.to(dev), (None if b is None else b.to(dev))          # named: a temporary's block could be handed to the next one
    call("hos_rowdot_lrelu_fwd", P(xd), P(Wb), Wb.stride(0), P(bd), N, K, 0.2, P(y))
    assert bool(torch.isnan(y[N:]).all())
    return y[:N]


@pytest.mark.parametrize("N,K", X.ROWDOT_SHAPES)
def test_rowdot_lrelu_fwd_exact(dev, N, K):
    g = X.gen(N + K)
    x, W, b = X.ints(g, K), X.ints(g, N, K), X.ints(g, N)
    for bias, ldw in ((b, None), (None, None), (b, K + 8)):          # with bias, NULL bias, ldw > K (NaN pad columns)
        want = X.head(x.double(), W.double(), None if bias is None else bias.double())
        assert same(_rowdot_fwd(dev, x, W, bias, ldw), want), (bias is None, ldw)


def _rowdot_bwd(dev, g_, y, x, W, G0W, G0b, G0x, ldw=None, want_gb=True, want_gx=True):
    N, K = W.shape
    Wb = padded(dev, W, ldw or K)
    gW = G0W.to(dev).clone()                     # [N, ldgw]
    gb = G0b.to(dev).clone() if want_gb else None
    gx = G0x.to(dev).clone() if want_gx else None
    gd, yd, xd = g_.to(dev), y.to(dev), x.to(dev)
    call("hos_rowdot_lrelu_bwd", P(gd), P(yd), P(xd), P(Wb), Wb.stride(0), N, K, 0.2, P(gW), gW.stride(0), P(gb), P(gx))
    return gW, gb, gx


@pytest.mark.parametrize("N,K", X.ROWDOT_SHAPES)
def test_rowdot_lrelu_bwd_exact(dev, N, K):
    """gW += d x^T, gb += d, gx += W^T d with d = g (y > 0 ? 1 : 0.2): outputs pre-filled with G0, y exactly 0 takes the slope."""
    g = X.gen(3 * N + K)
    x, W, y = X.ints(g, K), X.ints(g, N, K), X.ints(g, N)
    y[::3] = 0.0
    go = X.ints_for(g, y)
    assert bool((go[::3].abs() % 5 == 0).all())
    G0W, G0b, G0x = X.ints(g, N, K + 4), X.ints(g, N), X.ints(g, K)
    rW, rb, rx = X.head_bwd(go.double(), y.double(), x.double(), W.double(), round32=True)
    for ldw, ldgw, want_gb, want_gx in ((None, K, True, True), (None, K, False, True), (None, K, True, False), (K + 8, K + 4, True, True)):
        G = G0W[:, :ldgw].contiguous()
        gW, gb, gx = _rowdot_bwd(dev, go, y, x, W, G, G0b, G0x, ldw, want_gb, want_gx)
        assert same(gW[:, :K], G[:, :K].double() + rW) and torch.equal(gW[:, K:].cpu(), G[:, K:])
        assert gb is None or same(gb, G0b.double() + rb)
        assert gx is None or same(gx, G0x.double() + rx)


def test_rowdot_lrelu_random(dev):
    N, K = X.ROWDOT_SHAPES[3]
    g = X.gen(13)
    x, W, b = torch.randn(K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), 0.1 * torch.randn(N, generator=g)
    par = Parity()
    par.add("y", _rowdot_fwd(dev, x, W, b), X.head(x, W, b), X.head(x.double(), W.double(), b.double()))
    y = torch.randn(N, generator=g)
    y[::7] = 0.0
    go = torch.randn(N, generator=g)
    G0W, G0b, G0x = X.ints(g, N, K), X.ints(g, N), X.ints(g, K)
    got = _rowdot_bwd(dev, go, y, x, W, G0W, G0b, G0x)
    r32 = X.head_bwd(go, y, x, W)
    r64 = X.head_bwd(go.double(), y.double(), x.double(), W.double())
    for name, a, G, a32, t in zip(("gW", "gb", "gx"), got, (G0W, G0b, G0x), r32, r64):
        par.add(name, a, G + a32, G.double() + t)
    par.finish("rowdot_lrelu_random")          # measured worst e_hip / max(e_ref, 2^-24): 0.90; bound 8 e_ref + 4 * 2^-24


def _softmax_raw(dev, z, prior, cot):
    V3, C = z.shape
    vol, gz = nans(dev, C * V3 + 8), nans(dev, C * V3 + 8)
    zd, pd, cd = z.to(dev), prior.to(dev), cot.to(dev)
    call("hos_volume_softmax_fwd", P(zd), P(pd), C, V3, P(vol))
    call("hos_volume_softmax_bwd", P(cd), P(vol), C, V3, P(gz))
    assert bool(torch.isnan(vol[C * V3:]).all()) and bool(torch.isnan(gz[C * V3:]).all())
    return vol[:C * V3].view(C, V3), gz[:C * V3].view(V3, C)


def test_volume_softmax_fwd_bwd(dev):
    """softmax_c(z + log prior) and its backward at V^3 that are no multiple of 256 (but 512): logits that need the max
    subtraction, zero priors (channel excluded EXACTLY, forward and backward), absolute errors (vol in [0, 1], |gz| <~ 1)."""
    par = Parity(err=X.err_abs)
    for C, V in X.SOFTMAX_SHAPES:
        z, prior, cot = X.softmax_inputs(C, V)
        vol, gz = _softmax_raw(dev, z, prior, cot)
        v64, g64 = X.softmax(z.double(), prior.double(), cot.double())
        v32, g32 = X.softmax(z, prior, cot)
        assert bool(torch.isfinite(vol).all()) and bool(torch.isfinite(gz).all())
        zero = (prior == 0)
        assert bool((vol.cpu()[zero] == 0).all()) and bool((gz.cpu().t()[zero] == 0).all())
        par.add(f"vol[{C},{V}]", vol, v32, v64)
        par.add(f"gz[{C},{V}]", gz, g32, g64)
    par.finish("volume_softmax_fwd_bwd")          # measured worst e_hip / max(e_ref, 2^-24): 1.16; bound 8 e_ref + 4 * 2^-24
    t = torch.ones(33 * 8, device=dev)
    rejects(E_SHAPE, "hos_volume_softmax_fwd", P(t), P(t), 33, 8, P(t))
    rejects(E_SHAPE, "hos_volume_softmax_bwd", P(t), P(t), 33, 8, P(t))


@pytest.mark.parametrize("C,Kb,V", X.PAIR_SHAPES)
def test_volume_channel_last_and_pair_bwd(dev, C, Kb, V):
    g = X.gen(C + Kb + V)
    V3 = V ** 3
    vol = torch.randn(C, V3, generator=g)
    cl = nans(dev, V3 * 32 + 8)
    vold = vol.to(dev)
    call("hos_volume_channel_last", P(vold), Kb, V3, P(cl))
    assert torch.equal(cl[:V3 * 32].view(V3, 32).cpu(), X.channel_last(vol, Kb)) and bool(torch.isnan(cl[V3 * 32:]).all())
    g_vol, g_cl = torch.randn(C, V3, generator=g), torch.randn(V3, 32, generator=g)
    g_cl[:, Kb:] = NAN                           # the pad channels carry no gradient: they must not leak
    for gv, gc in ((g_vol, g_cl), (g_vol, None), (None, g_cl)):
        out = nans(dev, C * V3 + 8)
        gvd, gcd = (None if gv is None else gv.to(dev)), (None if gc is None else gc.to(dev))
        call("hos_volume_pair_bwd", P(gvd), P(gcd), C, Kb, V3, P(out))
        want = X.pair_bwd(gv, None if gc is None else torch.nan_to_num(gc, nan=0.0), C, Kb)      # one add per element: fp32 torch, bit for bit
        assert torch.equal(out[:C * V3].view(C, V3).cpu(), want), (gv is None, gc is None)
        assert bool(torch.isnan(out[C * V3:]).all())
    t = torch.zeros(32 * V3, device=dev)
    rejects(E_ARG, "hos_volume_pair_bwd", 0, 0, C, Kb, V3, P(t))
    rejects(E_SHAPE, "hos_volume_pair_bwd", P(t), P(t), C, C + 1, V3, P(t))


@pytest.mark.parametrize("M,N", X.BIAS_SHAPES)
def test_bias_lrelu_exact(dev, M, N):
    g = X.gen(M + N)
    y0, b = X.ints(g, M, N), X.ints(g, N)
    for bias in (b, None):
        for leaky in (0, 1):
            buf = nans(dev, M * N + 8)
            buf[:M * N] = y0.reshape(-1).to(dev)
            bd = None if bias is None else bias.to(dev)
            call("hos_bias_lrelu", P(buf), P(bd), M, N, 0.2, leaky)
            want = y0.double() + (0 if bias is None else bias.double())
            assert same(buf[:M * N].view(M, N), X.lrelu(want) if leaky else want) and bool(torch.isnan(buf[M * N:]).all())


@pytest.mark.parametrize("world,M,cs", X.INTERLEAVE_SHAPES)
def test_shard_interleave(dev, world, M, cs):
    parts = X.ints(X.gen(world + M + cs), world, M, cs) + torch.arange(world).view(-1, 1, 1) * 16.0      # the rank shows in the value
    out = nans(dev, world * M * cs + 8)
    pd = parts.to(dev)
    call("hos_shard_interleave", P(pd), world, M, cs, P(out))
    assert torch.equal(out[:world * M * cs].view(M, world * cs).cpu(), parts.permute(1, 0, 2).reshape(M, world * cs))
    assert bool(torch.isnan(out[world * M * cs:]).all())


# ====================================================================================================== 2. autograd nodes
def _layer_inputs(g, D, Cin, Cout, exact, nonzero_w=False):
    M = D ** 3
    if exact:
        w = (X.full_nonzero_ints if nonzero_w else X.ints)(g, Cin, Cout, 4, 4, 4)
        return X.ints(g, M, Cin), w, X.ints(g, Cout)
    w = torch.randn(Cin, Cout, 4, 4, 4, generator=g) / math.sqrt(Cin * 8)           # scaled as test_deconv3d_matches_torch
    return torch.randn(M, Cin, generator=g), w, 0.1 * torch.randn(Cout, generator=g)


def _cotangent(g, y64, exact, leaky):
    """From the float64 output only.  Exact: multiples of 5 where the slope applies.  Random: 0 where a LeakyReLU input lies within
    1e-4 of its kink, so that a sign decided by the last bit (in either fp32 implementation) cannot reach a gradient."""
    if exact:
        return X.ints_for(g, y64) if leaky else X.ints(g, *y64.shape)
    go = torch.randn(y64.shape, generator=g)
    if leaky:
        go[y64.abs() < 1e-4] = 0.0
    return go


def _leaf(t, dev, grad=None):
    p = t.to(dev).requires_grad_(True)
    if grad is not None:
        p.grad = grad.to(dev).clone()
    return p


def _deconv_accumulate(dev, D, Cin, Cout, leaky, exact, par=None):
    """weight.grad = G0w, bias.grad = G0b, two backward passes over two fresh forwards -> G0 + 2 * reference, in place."""
    from hosnerf_amd import ops
    g = X.gen(100 * D + Cin + Cout + exact)
    x, w, b = _layer_inputs(g, D, Cin, Cout, exact)
    G0w, G0b = X.ints(g, *w.shape), X.ints(g, Cout)
    y64 = X.deconv(x.double(), w.double(), b.double(), D, leaky)
    go = _cotangent(g, y64, exact, leaky)
    _, gx64, gw64, gb64, _ = X.deconv(x.double(), w.double(), b.double(), D, leaky, go=go.double(), round32=exact)
    xg, wg, bg = _leaf(x, dev), _leaf(w, dev, G0w), _leaf(b, dev, G0b)
    slots = wg.grad.data_ptr(), bg.grad.data_ptr()
    god = go.to(dev)
    ys, gxs = [], []
    for _ in range(2):
        xg.grad = None
        y = ops.deconv3d(xg, wg, bg, D, leaky)
        y.backward(god)
        ys.append(y.detach())
        gxs.append(xg.grad)
    assert (wg.grad.data_ptr(), bg.grad.data_ptr()) == slots          # accumulated in place; the node returned None for both
    if exact:
        for y, gx in zip(ys, gxs):
            assert same(y, y64) and same(gx, gx64)
        assert same(wg.grad, G0w.double() + 2 * gw64) and same(bg.grad, G0b.double() + 2 * gb64)
    else:
        y32, gx32, gw32, gb32, _ = X.deconv(x, w, b, D, leaky, go=go)
        tag = f"[{D},{Cin},{Cout}]"
        par.add("y" + tag, ys[1], y32, y64)
        par.add("gx" + tag, gxs[1], gx32, gx64)
        par.add("gw" + tag, wg.grad, G0w + gw32 + gw32, G0w.double() + 2 * gw64)
        par.add("gb" + tag, bg.grad, G0b + gb32 + gb32, G0b.double() + 2 * gb64)


@pytest.mark.parametrize("D,Cin,Cout,leaky", X.DECONV_SHAPES)
def test_deconv3d_accumulates_in_place_exact(dev, D, Cin, Cout, leaky):
    """The branch a training step takes (`in_place` / `db_in_place`): outer_accum<8> at M = 8, <32>, linear_wgrad accumulating,
    and the grid-stride loops of im2col (D = 8) and col2im (D = 16) past their 8192-block caps."""
    if D == 8:
        assert D ** 3 * Cout * 64 > 8192 * 256
    if D == 16:
        assert 8 * D ** 3 * Cout > 8192 * 256
    _deconv_accumulate(dev, D, Cin, Cout, leaky, exact=True)


def test_deconv3d_accumulates_in_place_random(dev):
    par = Parity()
    for D, Cin, Cout, leaky in (X.DECONV_SHAPES[1], X.DECONV_SHAPES[2]):
        _deconv_accumulate(dev, D, Cin, Cout, leaky, exact=False, par=par)
    par.finish("deconv3d_accumulates_in_place_random")          # measured worst e_hip / max(e_ref, 2^-24): 1.04-1.61 over three runs (a bias gradient: fp32 atomics); bound 8 e_ref + 4 * 2^-24


def test_deconv3d_weight_in_place_bias_through_autograd(dev):
    """weight.grad set, bias.grad None: the weight gradient accumulates in place, the bias gradient comes back through autograd once."""
    from hosnerf_amd import ops
    D, Cin, Cout, leaky = X.DECONV_SHAPES[2]
    g = X.gen(42)
    x, w, b = _layer_inputs(g, D, Cin, Cout, True)
    G0w = X.ints(g, *w.shape)
    y64 = X.deconv(x.double(), w.double(), b.double(), D, leaky)
    go = _cotangent(g, y64, True, leaky)
    _, gx64, gw64, gb64, _ = X.deconv(x.double(), w.double(), b.double(), D, leaky, go=go.double(), round32=True)
    xg, wg, bg = _leaf(x, dev), _leaf(w, dev, G0w), _leaf(b, dev)
    ops.deconv3d(xg, wg, bg, D, leaky).backward(go.to(dev))
    assert same(wg.grad, G0w.double() + gw64) and same(bg.grad, gb64) and same(xg.grad, gx64)


def _first_case(dev, Cin, Cout, leaky, exact, par=None, bias_grad=True):
    """The split-K input gradient reduces over 8 * Cout in tiles of 32, so it exists for Cout % 4 == 0 only (any other Cout is
    answered with HOS_E_SHAPE): Cout = 129 runs without an input gradient -- output, weight and bias gradient -- and 132 with it."""
    from hosnerf_amd import ops
    from hosnerf_amd.human_nerf import Network
    assert list(Network._LIVE_TAPS) == X.LIVE_TAPS
    x_grad = (8 * Cout) % 32 == 0
    g = X.gen(Cin + Cout + 2 * leaky + exact)
    x, full, b = _layer_inputs(g, 1, Cin, Cout, exact, nonzero_w=True)
    assert not exact or bool((full != 0).all())   # every tap alive: a dead one that leaks into the layer shows
    wc = full.view(Cin, Cout, 64)[:, :, Network._LIVE_TAPS].permute(0, 2, 1).reshape(Cin, 8 * Cout).contiguous()
    G0, G0b = X.ints(g, Cin, 8 * Cout), X.ints(g, Cout)
    y64 = X.deconv(x.double(), full.double(), b.double(), 1, leaky)
    go = _cotangent(g, y64, exact, leaky)
    _, gx64, gw64, gb64, _ = X.deconv(x.double(), full.double(), b.double(), 1, leaky, go=go.double(), round32=exact)
    gwc64 = X.compact(gw64)                      # the live-tap slice of the float64 weight gradient
    xg, bg = (_leaf(x, dev) if x_grad else x.to(dev)), _leaf(b, dev, G0b if bias_grad else None)
    wcd, gwc = wc.to(dev), G0.to(dev).clone()
    y = ops.deconv3d_first(xg, wcd, gwc, bg, leaky)
    assert y.shape == (8, Cout)
    y.backward(go.to(dev))
    gb_want = (G0b.double() if bias_grad else 0) + gb64
    # the same layer through the general node on the full weight
    x2, w2, b2 = _leaf(x, dev), _leaf(full, dev), _leaf(b, dev)
    y2 = ops.deconv3d(x2, w2, b2, 1, leaky)
    if exact:
        assert same(y, y64) and torch.equal(y.detach(), y2.detach())
        assert same(gwc, G0.double() + gwc64) and same(bg.grad, gb_want) and (not x_grad or same(xg.grad, gx64))
    else:
        y32, gx32, gw32, gb32, _ = X.deconv(x, full, b, 1, leaky, go=go)
        tag = f"[{Cin},{Cout},leaky={int(leaky)}]"
        par.add("y" + tag, y, y32, y64)
        par.add("y vs ops.deconv3d" + tag, y, y32, y64, other=y2)                   # two HIP routes to one value: as close as the bound on y
        par.add("gwc" + tag, gwc, G0 + X.compact(gw32), G0.double() + gwc64)
        if x_grad:
            par.add("gx" + tag, xg.grad, gx32, gx64)
        par.add("gb" + tag, bg.grad, (G0b if bias_grad else 0) + gb32, gb_want)


@pytest.mark.parametrize("leaky", [True, False])
@pytest.mark.parametrize("Cin,Cout", X.FIRST_SHAPES)
def test_deconv3d_first_exact(dev, Cin, Cout, leaky):
    _first_case(dev, Cin, Cout, leaky, exact=True)


def test_deconv3d_first_bias_through_autograd(dev):
    _first_case(dev, 64, 129, True, exact=True, bias_grad=False)


def test_deconv3d_first_random(dev):
    par = Parity()
    for Cin, Cout in X.FIRST_SHAPES:
        for leaky in (True, False):
            _first_case(dev, Cin, Cout, leaky, exact=False, par=par)
    par.finish("deconv3d_first_random")          # measured worst e_hip / max(e_ref, 2^-24): 1.53-2.11 over three runs (a bias gradient: fp32 atomics); bound 8 e_ref + 4 * 2^-24


def _head_leaves(dev, x, W, b, G0=None, flat=False):
    ps = []
    for t, G in zip((x, W, b), G0 or (None, None, None)):
        p = _leaf(t, dev, G)
        if flat:
            p._hos_flat_grad = True
        ps.append(p)
    return ps


@pytest.mark.parametrize("N,K", [(1024, 256), (33, 300)])
def test_decoder_head(dev, N, K):
    from hosnerf_amd import ops
    g = X.gen(N * K)
    x, W, b = X.ints(g, K), X.ints(g, N, K), X.ints(g, N)
    y64 = X.head(x.double(), W.double(), b.double())
    go = X.ints_for(g, y64)
    rW, rb, rx = X.head_bwd(go.double(), y64, x.double(), W.double(), round32=True)
    G0 = (X.ints(g, K), X.ints(g, N, K), X.ints(g, N))
    god = go.to(dev)[None]
    # (a) plain leaves: (gx, gW, gb) come back, and again the same from a second call: nothing was counted twice
    e, w, bb = _head_leaves(dev, x, W, b)
    y = ops.decoder_head(e, w, bb)
    assert y.shape == (1, N) and same(y[0], y64)
    for _ in range(2):
        gx, gW, gb = torch.autograd.grad(y, (e, w, bb), god, retain_graph=True)
        assert same(gx, rx) and same(gW, rW) and same(gb, rb)
    assert e.grad is None and w.grad is None and bb.grad is None
    # (b) parameters whose .grad the flat store owns: accumulated in place, None returned
    e, w, bb = _head_leaves(dev, x, W, b, G0, flat=True)
    slots = [p.grad.data_ptr() for p in (e, w, bb)]
    ops.decoder_head(e, w, bb).backward(god)
    assert [p.grad.data_ptr() for p in (e, w, bb)] == slots
    assert same(e.grad, G0[0].double() + rx) and same(w.grad, G0[1].double() + rW) and same(bb.grad, G0[2].double() + rb)
    # (c) the same with the in-place route switched off: returned to autograd, which adds them to .grad ONCE
    e, w, bb = _head_leaves(dev, x, W, b, G0, flat=True)
    prev = ops.DECODER_HEAD_INPLACE
    ops.DECODER_HEAD_INPLACE = False
    try:
        ops.decoder_head(e, w, bb).backward(god)
    finally:
        ops.DECODER_HEAD_INPLACE = prev
    assert same(e.grad, G0[0].double() + rx) and same(w.grad, G0[1].double() + rW) and same(bb.grad, G0[2].double() + rb)


class _Drop(torch.autograd.Function):
    """identity whose backward hands an undefined gradient on: a consumer that turned out not to need the volume"""

    @staticmethod
    def forward(ctx, v):
        return v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        return None


def test_volume_softmax_and_pair_composed(dev):
    """ops.volume_softmax + ops.volume_pair as Network's prologue composes them, with the consumers only vol, only vol_cl, both
    and neither, against float64 autograd of softmax -> (vol, channel-last copy of its first K channels)."""
    from hosnerf_amd import ops
    C, K = 27, 26
    par = Parity(err=X.err_abs)
    for V in (7, 8):
        z, prior, cot = X.softmax_inputs(C, V, seed=5)
        g = X.gen(V)
        gc = torch.randn(V ** 3, 32, generator=g)

        def reference(dtype, use_vol, use_cl):
            zr = z.detach().clone().to(dtype).requires_grad_(True)
            vol = torch.softmax(zr.t() + torch.log(prior.to(dtype)), 0)
            cl = X.channel_last(vol, K)
            loss = (vol * cot.to(dtype)).sum() * use_vol + (cl * gc.to(dtype)).sum() * use_cl
            loss.backward()
            return vol.detach(), cl.detach(), zr.grad

        for use_vol, use_cl in ((1, 0), (0, 1), (1, 1)):
            zd = _leaf(z, dev)
            vol, vol_cl = ops.volume_pair(ops.volume_softmax(zd, prior.view(C, V, V, V).to(dev)), K)
            assert vol.shape == (C, V, V, V) and vol_cl.shape == (V, V, V, 32)
            outs = [(vol, cot.view(C, V, V, V))] * use_vol + [(vol_cl, gc.view(V, V, V, 32))] * use_cl
            torch.autograd.backward([o for o, _ in outs], [c.to(dev) for _, c in outs])
            v64, cl64, gz64 = reference(torch.float64, use_vol, use_cl)
            v32, cl32, gz32 = reference(torch.float32, use_vol, use_cl)
            assert torch.equal(vol_cl.detach().view(-1, 32)[:, :K], vol.detach().view(C, -1)[:K].t()) and bool((vol_cl[..., K:] == 0).all())
            tag = f"[V={V},vol={use_vol},cl={use_cl}]"
            par.add("vol" + tag, vol.view(C, -1), v32, v64)
            par.add("gz" + tag, zd.grad, gz32, gz64)
        # neither consumer.  (1) Nothing downstream asks for a gradient: the nodes do not run, z.grad stays None.
        zd, other = _leaf(z, dev), torch.ones(3, device=dev, requires_grad=True)
        vol, vol_cl = ops.volume_pair(ops.volume_softmax(zd, prior.view(C, V, V, V).to(dev)), K)
        (other.sum() + 0.0 * float(vol_cl.detach()[0, 0, 0, 0])).backward()
        assert zd.grad is None
        # (2) Both consumers are in the graph but pass no gradient back: volume_pair's backward gets (None, None), launches nothing
        # and raises nothing (hos_volume_pair_bwd would answer HOS_E_ARG); autograd then feeds the softmax a zero cotangent.
        (_Drop.apply(vol).sum() + _Drop.apply(vol_cl).sum()).backward()
        assert zd.grad is None or not bool(zd.grad.any())
    par.finish("volume_softmax_and_pair_composed")          # measured worst e_hip / max(e_ref, 2^-24): 1.02; bound 8 e_ref + 4 * 2^-24


# ====================================================================================================== 3. sharded layers
def _shard_case(dev, D, Cin, Cout, world, first, exact, par=None):
    """Every rank of `world`, one after another on this device (X.RankEmulator): output == the float64 UNSHARDED layer, rows
    [c0, c1) of the weight-gradient buffer == G0 + reference and every other row bit-identical to G0, the full bias gradient on
    every rank, dx assembled through the gather (+ hos_shard_interleave) in channel order."""
    from hosnerf_amd import ops
    leaky = True
    cs = Cin // world
    assert cs % 32 == 0 and cs * world == Cin
    g = X.gen(1000 * world + Cin + Cout + D + exact)
    x, full, b = _layer_inputs(g, D, Cin, Cout, exact, nonzero_w=True)
    y64 = X.deconv(x.double(), full.double(), b.double(), D, leaky)
    go = _cotangent(g, y64, exact, leaky)
    _, gx64, gw64, gb64, _ = X.deconv(x.double(), full.double(), b.double(), D, leaky, go=go.double(), round32=exact)
    w2 = X.compact(full) if first else full.reshape(Cin, Cout * 64)
    gw64 = X.compact(gw64) if first else gw64.reshape(Cin, Cout * 64)
    G0, G0b = X.ints(g, *w2.shape), X.ints(g, Cout)
    xd, wd, bd, god, G0d, G0bd = (t.to(dev) for t in (x, w2, b, go, G0, G0b))

    def rank(comm):
        xg = xd.clone().requires_grad_(True)
        bg = bd.clone().requires_grad_(True)
        bg.grad = G0bd.clone()
        if first:
            gw = G0d.clone()
            y = ops.deconv3d_first_sharded(xg, wd, gw, bg, leaky, comm)
        else:
            wg = wd.view(Cin, Cout, 4, 4, 4).detach().requires_grad_(True)
            wg.grad = G0d.clone().view(Cin, Cout, 4, 4, 4)
            y = ops.deconv3d_sharded(xg, wg, bg, D, leaky, comm)
        y.backward(god)
        return y.detach(), xg.grad, (gw if first else wg.grad.view(Cin, Cout * 64)), bg.grad

    emu = X.RankEmulator(world)
    res = emu.run(rank)
    assert [c["kind"] for c in emu.log] == ["sum", "gather"] and emu.passes == 3
    if not exact:
        y32, gx32, gw32, gb32, _ = X.deconv(x, full, b, D, leaky, go=go)
        gw32 = X.compact(gw32) if first else gw32.reshape(Cin, Cout * 64)
    want_gw = X.f32(G0.double() + gw64)
    for r, (y, dx, gw, gb) in enumerate(res):
        gw = gw.cpu()
        own = torch.zeros(Cin, dtype=torch.bool)
        own[r * cs:(r + 1) * cs] = True
        assert torch.equal(gw[~own], G0[~own]), f"rank {r} touched rows it does not own"
        if exact:
            assert same(y, y64) and same(dx, gx64) and same(gb, G0b.double() + gb64), r
            assert torch.equal(gw[own], want_gw[own]), r
        else:
            tag = f"[{'first,' if first else ''}{D},{Cin},{Cout},world={world},rank={r}]"
            par.add("y" + tag, y, y32, y64)
            par.add("dx" + tag, dx, gx32, gx64)
            par.add("gb" + tag, gb, G0b + gb32, G0b.double() + gb64)
            par.add("gw rows" + tag, gw[own], (G0 + gw32)[own], (G0.double() + gw64)[own])


@pytest.mark.parametrize("Cin,Cout,world", X.SHARD_FIRST_SHAPES)
def test_deconv3d_first_sharded_exact(dev, Cin, Cout, world):
    _shard_case(dev, 1, Cin, Cout, world, first=True, exact=True)


@pytest.mark.parametrize("D,Cin,Cout,world", X.SHARD_SHAPES)
def test_deconv3d_sharded_exact(dev, D, Cin, Cout, world):
    _shard_case(dev, D, Cin, Cout, world, first=False, exact=True)


def test_sharded_layers_random(dev):
    par = Parity()
    _shard_case(dev, 1, *X.SHARD_FIRST_SHAPES[0], first=True, exact=False, par=par)
    _shard_case(dev, 1, *X.SHARD_FIRST_SHAPES[1], first=True, exact=False, par=par)
    _shard_case(dev, *X.SHARD_SHAPES[0], first=False, exact=False, par=par)
    _shard_case(dev, *X.SHARD_SHAPES[1], first=False, exact=False, par=par)
    par.finish("sharded_layers_random")          # measured worst e_hip / max(e_ref, 2^-24): 2.32 (weight-gradient rows at world = 8); bound 8 e_ref + 4 * 2^-24


def test_sharded_layers_need_flat_gradients(dev):
    """A missing or non-contiguous .grad raises HosLibraryError before the backward launches anything: bias.grad (which the first
    launch of the backward would add to) still holds G0."""
    from hosnerf_amd import ops
    from hosnerf_amd._lib import HosLibraryError
    g = X.gen(9)
    D, Cin, Cout = 2, 64, 8
    x, w, b = _layer_inputs(g, D, Cin, Cout, True)
    go = X.ints(g, 8 * D ** 3, Cout).to(dev)
    G0b = X.ints(g, Cout)
    for wgrad in (None, torch.zeros(Cin, Cout, 4, 4, 8, device=dev)[..., ::2]):
        kept = []

        def rank(comm):
            xg, wg, bg = _leaf(x, dev), _leaf(w, dev), _leaf(b, dev, G0b)
            wg.grad = wgrad
            kept.append(bg)
            ops.deconv3d_sharded(xg, wg, bg, D, True, comm).backward(go)

        with pytest.raises(HosLibraryError, match="flat gradient buffer"):
            X.RankEmulator(2).run(rank)
        assert torch.equal(kept[0].grad.cpu(), G0b)
    x1, full, _ = _layer_inputs(g, 1, Cin, Cout, True)
    wc = X.compact(full).to(dev)

    def rank1(comm):
        xg, bg = _leaf(x1, dev), _leaf(b, dev)
        ops.deconv3d_first_sharded(xg, wc, torch.zeros_like(wc), bg, True, comm).backward(go[:8])

    with pytest.raises(HosLibraryError, match="flat gradient buffer"):
        X.RankEmulator(2).run(rank1)


# ====================================================================================================== 4. the whole decoder
@pytest.fixture(scope="module")
def net(dev):
    from hosnerf_amd import synth
    from hosnerf_amd.human_nerf import Network, default_cfg
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    cfg = default_cfg(d)
    cfg.perturb = 0.0
    n = Network(cfg)
    n.load_state_dict(synth.human_state_dict(777, 2), strict=True)
    return n.to(dev)


def test_whole_decoder_vs_float64(dev, net):
    """Network._motion_weight_volume on the FULL [27, 32, 32, 32] volume (odd voxels included) and the gradient of each of its 13
    tensors for one random cotangent, against oracle.human.motion_weight_volume in float64; e_ref = the fp32 oracle's own error."""
    import oracle.human as oh
    from hosnerf_amd import synth
    sd = synth.human_state_dict(777, 2)
    keys = [k for k in sd if k.startswith("mweight_vol_decoder.")]
    assert len(keys) == 13
    priors = synth.human_batch(8, seed=3)["motion_weights_priors"]
    cot = torch.randn(priors.shape, generator=X.gen(31))
    assert tuple(priors.shape) == (27, 32, 32, 32)

    def oracle(dtype):
        p = {k: sd[k].to(dtype).requires_grad_(True) for k in keys}
        vol = oh.motion_weight_volume(p, priors.to(dtype))
        vol.backward(cot.to(dtype))
        return vol.detach(), {k: p[k].grad for k in keys}

    v64, g64 = oracle(torch.float64)
    v32, g32 = oracle(torch.float32)
    live = torch.zeros(64, dtype=torch.bool)
    live[X.LIVE_TAPS] = True
    k0 = "mweight_vol_decoder.decoder.block_conv.0.weight"
    assert bool((g64[k0].reshape(*g64[k0].shape[:2], 64)[:, :, ~live] == 0).all())
    try:
        net.zero_grad()
        vol = net._motion_weight_volume(priors.to(dev))
        vol.backward(cot.to(dev))
        net.scatter_compact_grads()
        params = dict(net.named_parameters())
        fwd = Parity(err=X.err_abs)
        fwd.add("vol", vol, v32, v64)
        par = Parity(err=X.err_l2)
        for k in keys:
            par.add(k, params[k].grad, g32[k], g64[k])
        dead = params[k0].grad.reshape(*g64[k0].shape[:2], 64)[:, :, ~live.to(dev)]
        dead_ok = not bool(dead.any())
    finally:
        net.zero_grad()
        net.load_state_dict(sd, strict=True)
    fwd.finish("whole_decoder_vs_float64.forward")          # measured worst e_hip / max(e_ref, 2^-24): 0.76; bound 8 e_ref + 4 * 2^-24
    par.finish("whole_decoder_vs_float64")          # measured worst e_hip / max(e_ref, 2^-24): 0.81-0.86 (a bias gradient); bound 8 e_ref + 4 * 2^-24
    assert dead_ok, "the dead taps of the first layer's weight gradient are exactly 0"
