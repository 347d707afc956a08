"""Float64 statements of what the volume-decoder kernels (hos_deconv.hip, the autograd nodes around them in ops.py) compute, the
two kinds of test input, and a rank emulator for the sharded layers.  Torch on the CPU only; tests/test_decoder_expect_cpu.py
checks these helpers before tests/test_gpu_decoder.py holds a kernel against them.

Exact inputs: every operand an integer in -4..4, so every product and every partial sum of at most 2^24 / 16 terms is a float32
and the order of a sum cannot matter: kernel == float64 result cast to float32, bit for bit.  LeakyReLU keeps that property where
ONE correctly rounded product by float32(0.2) ends the chain (a forward output); a backward pass goes on summing after the slope,
so there the cotangent is a multiple of 5 wherever the slope applies: float32(5 j * float32(0.2)) == j for |j| <= 4, again integers.

Random inputs: e = max|a - t| / max(1, max|t|) against the float64 value t, for the kernel (e_hip) and for the same operation in
fp32 torch on the CPU (e_ref); the bound is 8 e_ref + 4 * 2^-24 (`bound`)."""
import numpy as np
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
SLOPE = float(np.float32(0.2))                  # the float32 the kernels multiply by, as a float64
# taps of a 4^3 kernel that reach the 2^3 output of ONE input voxel (o = 2 i - 1 + k, i = 0: k = o + 1), output-voxel major
LIVE_TAPS = [(od + 1) * 16 + (oh + 1) * 4 + (ow + 1) for od in range(2) for oh in range(2) for ow in range(2)]

# ---- the shapes of the GPU tests (the CPU test checks the exactness budget and the kernel routes on these lists)
GEMV_SHAPES = [(16, 8, 1), (40, 1032, 129), (1024, 4096, 512), (64, 256, 32)]                 # (K, N, bias_mod)
OUTER_SHAPES = [(1, 1024, 4096, 8), (8, 40, 512, 8), (8, 44, 1028, 8), (8, 500, 16384, 32), (64, 500, 16384, 32)]   # (M, K, N, route)
ROWDOT_SHAPES = [(1, 4), (5, 260), (33, 300), (1024, 256)]                                    # (N, K)
SOFTMAX_SHAPES = [(1, 3), (25, 7), (27, 8), (32, 5)]                                          # (C, V)
PAIR_SHAPES = [(27, 26, 7), (32, 32, 4), (5, 1, 3)]                                           # (C, Kb, V)
BIAS_SHAPES = [(8, 27), (1, 1), (4100, 257)]                                                  # (M, N)
INTERLEAVE_SHAPES = [(2, 1, 32), (8, 8, 64), (4, 4096, 96)]                                   # (world, M, cs)
DECONV_SHAPES = [(2, 64, 8, True), (2, 512, 512, True), (4, 64, 96, True), (8, 32, 72, False), (16, 32, 72, False)]   # (D, Cin, Cout, leaky)
FIRST_SHAPES = [(32, 4), (64, 129), (64, 132), (1024, 512)]                                   # (Cin, Cout); 129: no input gradient
SHARD_FIRST_SHAPES = [(64, 4, 2), (256, 8, 8), (1024, 512, 8)]                                # (Cin, Cout, world)
SHARD_SHAPES = [(2, 128, 8, 4), (4, 256, 8, 8), (2, 512, 512, 8)]                             # (D, Cin, Cout, world)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, *shape):
    """float32 integers in -4..4"""
    return torch.randint(-4, 5, shape, generator=g).float()


def ints_for(g, y):
    """An exact cotangent for an output `y` that went through LeakyReLU: integers where the gradient passes, multiples of 5 where
    the slope applies (y <= 0: `!(y > 0)` in the kernels, as F.leaky_relu's backward)."""
    j = ints(g, *y.shape)
    return torch.where(y > 0, j, 5.0 * j)


def lrelu(t):
    return torch.where(t > 0, t, t * (SLOPE if t.dtype == torch.float64 else 0.2))


def dlrelu(g, y, round32=False):
    """g * (y > 0 ? 1 : slope) in g's precision; round32: the product rounded to float32 as the kernels' is (exact inputs: the
    float64 reference must take that ONE rounding, after it everything is an integer again)"""
    d = g * (SLOPE if g.dtype == torch.float64 else 0.2)
    if round32:
        d = d.float().to(g.dtype)
    return torch.where(y > 0, g, d)


def f32(t):
    return t.to(torch.float32)


def err(a, t):
    """max|a - t| / max(1, max|t|), t the float64 value"""
    a = a.detach().double().cpu()
    return float((a - t).abs().max()) / max(1.0, float(t.abs().max()))


def err_abs(a, t):
    return float((a.detach().double().cpu() - t).abs().max())


def err_l2(a, t):
    a = a.detach().double().cpu().reshape(-1)
    t = t.reshape(-1)
    return float((a - t).norm() / t.norm())


def bound(e_ref):
    return 8.0 * e_ref + 4.0 * U24


def factor(e_hip, e_ref):
    return e_hip / max(e_ref, U24)


def exact_budget(terms, operand=4, weight=4):
    """Largest partial sum of `terms` products: must stay below 2^24 for float32 to hold every one exactly."""
    return terms * operand * weight


def outer_accum_route(K, N):
    """The template route hos_outer_accum takes: 256 threads x 4 columns per workgroup, OA_KR = 32 weight rows per thread unless
    that grid is under 256 workgroups (one per CU), then 8 (the constants of the comment above `outer_accum_kernel`)."""
    gx = (N // 4 + 255) // 256
    return 8 if gx * ((K + 31) // 32) < 256 else 32


# ---------------------------------------------------------------------------------------------- ConvTranspose3d(4, 2, 1)
def deconv(x, w, b, D, leaky, go=None, cot=None, round32=False):
    """The layer in the precision of its arguments.  x [D^3, Cin] channel-last, w [Cin, Cout, 4, 4, 4], b [Cout] or None ->
    y [(2D)^3, Cout]; with a cotangent `go` (or `cot(y)` making one) also (gx [D^3, Cin], gw, gb, go).  round32: see dlrelu."""
    Cin, Cout = w.shape[0], w.shape[1]
    need = go is not None or cot is not None
    xr = x.t().reshape(1, Cin, D, D, D).detach().requires_grad_(need)
    wr = w.detach().requires_grad_(need)
    br = None if b is None else b.detach().requires_grad_(need)
    pre = F.conv_transpose3d(xr, wr, br, stride=2, padding=1)[0].reshape(Cout, -1).t()
    ycl = lrelu(pre.detach()) if leaky else pre.detach()
    if not need:
        return ycl
    if go is None:
        go = cot(ycl)
    gp = go.to(ycl.dtype)
    pre.backward(dlrelu(gp, ycl, round32) if leaky else gp)
    return ycl, xr.grad[0].reshape(Cin, -1).t().contiguous(), wr.grad, (None if br is None else br.grad), go


def compact(full):
    """[Cin, Cout, 4, 4, 4] -> the live taps, tap-major: [Cin, 8 * Cout]"""
    Cin, Cout = full.shape[0], full.shape[1]
    return full.reshape(Cin, Cout, 64)[:, :, LIVE_TAPS].permute(0, 2, 1).reshape(Cin, 8 * Cout).contiguous()


def full_nonzero_ints(g, *shape):
    """integers in -4..4 without 0: every tap of the full weight is alive, so a dead tap that leaks shows"""
    w = ints(g, *shape)
    return torch.where(w == 0, torch.ones_like(w), w)


# ---------------------------------------------------------------------------------------------- head and tail
def head(x, W, b):
    y = W @ x
    if b is not None:
        y = y + b
    return lrelu(y)


def head_bwd(g, y, x, W, round32=False):
    """(gW, gb, gx) of y = lrelu(W x + b) given y"""
    d = dlrelu(g, y, round32)
    return d[:, None] * x[None, :], d, W.t() @ d


def softmax_inputs(C, V, seed=0):
    """(z [V^3, C], prior [C, V^3], g [C, V^3]): logits that overflow without the max subtraction, priors with exact zeros (a
    channel excluded exactly) and a denormal-range one; channel 0 stays positive, so every voxel keeps a finite logit."""
    g = gen(1000 * C + V + seed)
    V3 = V ** 3
    z = 8.0 * torch.randn(V3, C, generator=g)
    z[0] += 90.0
    z[1] -= 90.0
    z[2, 0] = 95.0
    prior = torch.rand(C, V3, generator=g) * 0.9 + 0.05
    prior[1:, ::5] = 0.0
    prior[C // 2, 3] = 1e-30
    cot = torch.randn(C, V3, generator=g)
    return z, prior, cot


def softmax(z, prior, cot=None):
    """vol [C, V3] = softmax_c(z^T + log prior) in the arguments' precision; with `cot` also gz [V3, C]"""
    zr = z.detach().requires_grad_(cot is not None)
    vol = F.softmax(zr.t() + torch.log(prior), 0)
    if cot is None:
        return vol.detach()
    vol.backward(cot.to(vol.dtype))
    return vol.detach(), zr.grad


def channel_last(vol, Kb):
    """vol [C, V3] -> [V3, 32]: the first Kb channels, zero padded"""
    return F.pad(vol[:Kb].t(), (0, 32 - Kb)).contiguous()


def pair_bwd(g_vol, g_cl, C, Kb):
    """[C, V3]: g_vol (or 0) + the first Kb channels of g_cl [V3, 32] (or 0)"""
    V3 = (g_vol.shape[1] if g_vol is not None else g_cl.shape[0])
    out = torch.zeros(C, V3, dtype=(g_vol if g_vol is not None else g_cl).dtype) if g_vol is None else g_vol.clone()
    if g_cl is not None:
        out[:Kb] += g_cl[:, :Kb].t()
    return out


# ---------------------------------------------------------------------------------------------- ranks, one after another
class _Unresolved(Exception):
    pass


class RankComm:
    """What ops.deconv3d_sharded / deconv3d_first_sharded need of a train.ShardComm: rank, world, all_reduce_sum (in place) and
    all_gather ([world, ...])."""

    def __init__(self, emu, rank):
        self.emu, self.rank, self.world = emu, rank, emu.world
        self.n = 0

    def _collective(self, kind, t):
        i, self.n = self.n, self.n + 1
        log = self.emu.log
        if i == len(log):
            log.append({"kind": kind, "parts": {}})
        assert log[i]["kind"] == kind, "the ranks must issue the same collectives in the same order"
        if i < self.emu.resolved:
            return log[i]["parts"]
        if i == self.emu.resolved:                 # everything before it is resolved: this rank's contribution is the real one
            log[i]["parts"][self.rank] = t.detach().clone()
        return None

    def all_reduce_sum(self, t):
        parts = self._collective("sum", t)
        if parts is not None:
            s = parts[0].clone()
            for r in range(1, self.world):         # added in rank order
                s = s + parts[r]
            t.copy_(s)
        return t

    def all_gather(self, send):
        parts = self._collective("gather", send.contiguous())
        if parts is None:
            return torch.stack([send.contiguous()] * self.world)
        return torch.stack([parts[r] for r in range(self.world)])


class RankEmulator:
    """Runs `fn(comm)` for the ranks 0..world-1 one after another in this process: no torch.distributed, no second device.  The
    first pass records every rank's contribution to the first collective; each further pass replays the collectives resolved so
    far (the sum in rank order / the [world, ...] stack) and records the next one, whose inputs are now what real ranks would
    have sent.  A layer with one all-reduce (forward) and one all-gather (backward) takes three passes; `fn` must start from
    the same state in every pass (fresh gradient buffers).  Returns the last pass's results, one per rank."""

    def __init__(self, world):
        self.world = world
        self.log, self.resolved, self.passes = [], 0, 0

    def run(self, fn):
        while True:
            out = [fn(RankComm(self, r)) for r in range(self.world)]
            self.passes += 1
            if self.resolved >= len(self.log):
                return out
            assert len(self.log[self.resolved]["parts"]) == self.world
            self.resolved += 1


def sharded_layer_model(comm, x, w2, b, D, leaky, go, gw0, gb0, first=False, round32=True):
    """The sharded layer in plain torch, as ops._Deconv3dSharded / _Deconv3dFirstSharded state it: rank r multiplies its input
    channels [c0, c1), the partial pre-activations are summed over the ranks, bias + LeakyReLU follow; backward: bias gradient and
    mask on the full output gradient, this rank's ROWS of the weight gradient, its columns of the input gradient, gathered.
    w2 = the weight as [Cin, Cout * 64] (first: the compact [Cin, 8 * Cout]).  Returns (y, dx, gw, gb) with gw = gw0 + its rows."""
    Cin = w2.shape[0]
    cs = Cin // comm.world
    c0 = comm.rank * cs
    M = D ** 3
    Cout = w2.shape[1] // (8 if first else 64)

    def expand(rows):                               # [cs, cols] -> a [cs, Cout, 4, 4, 4] weight
        if not first:
            return rows.reshape(-1, Cout, 4, 4, 4)
        fullw = torch.zeros(rows.shape[0], Cout, 64, dtype=rows.dtype)
        fullw[:, :, LIVE_TAPS] = rows.reshape(-1, 8, Cout).permute(0, 2, 1)
        return fullw.reshape(-1, Cout, 4, 4, 4)

    xs = x[:, c0:c0 + cs].detach().requires_grad_(True)
    ws = w2[c0:c0 + cs].detach().requires_grad_(True)
    pre = F.conv_transpose3d(xs.t().reshape(1, cs, D, D, D), expand(ws), None, stride=2, padding=1)[0].reshape(Cout, -1).t()
    tot = comm.all_reduce_sum(pre.detach().clone()) + b
    y = lrelu(tot) if leaky else tot
    dpre = dlrelu(go, y, round32) if leaky else go
    pre.backward(dpre)
    parts = comm.all_gather(xs.grad)                # [world, M, cs]
    dx = parts.permute(1, 0, 2).reshape(M, Cin)
    gw = gw0.clone()
    gw[c0:c0 + cs] += ws.grad
    return y, dx, gw, gb0 + dpre.sum(0)
