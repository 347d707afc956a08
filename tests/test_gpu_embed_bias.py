"""The background MLPs with the state embedding as a bias instead of 64 columns of every row.

The reference concatenates the state embedding to every sample's encoding (M:295-296); here the encoder writes 512-column rows
[IPE 504 | 0 x 8] (`embed = None`), `ops.embed_bias_fold` forms b' = b + W[:, embedding columns] @ embed once per MLP call, and
`ops.state_embed_grad_w` adds the rank-1 weight gradient of those columns next to the bias / embedding gradients.

1. encoder: the 512-column form against the 576-column one, bit for bit, every output format, both first stages;
2. the bias fold against float64;
3. the MLPs' layers that read X, and every gradient the fold touches, against a float64 restatement of the reference layout
   (the embedding as columns) from the same parameters, in the three GEMM modes.
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hosnerf_amd import synth

G = os.path.join(os.path.dirname(__file__), "golden")
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from hosnerf_amd import _lib
    _lib.load()
    return torch.device("cuda")


def _golden_rays(dev):
    hv = np.load(os.path.join(G, "bkgd_helpers.npz"))
    return tuple(torch.from_numpy(np.ascontiguousarray(hv[k])).to(dev) for k in ("cast_tdist", "cast_o", "cast_d", "cast_radii", "basis"))


def _ragged_rays(dev, B=300, S=33, seed=31):
    """300 rays x 33 samples = 9900 rows: 154 encoder workgroups of 64 rows and a last one of 44.  301 x 32 = 9632 rows: a multiple
    of 32 (what the planes weight-gradient GEMM takes) but not of 64 or 256 -- the last encoder workgroup has 32 rows, the last
    256-row GEMM tile 160."""
    b = synth.stage1_batch(B, seed=seed)
    g = torch.Generator().manual_seed(seed)
    tdist = torch.cumsum(torch.rand(B, S + 1, generator=g) * 0.2 + 0.01, -1) + 0.1
    hv = np.load(os.path.join(G, "bkgd_helpers.npz"))
    return (tdist.to(dev), b["rays_o"].to(dev).contiguous(), b["rays_d"].to(dev).contiguous(), b["radii"].to(dev).contiguous(),
            torch.from_numpy(np.ascontiguousarray(hv["basis"])).to(dev))


# ------------------------------------------------------------------------------------------ 1. encoder
@pytest.mark.parametrize("rays", ["golden", "ragged"])
@pytest.mark.parametrize("stage", ["frustum", "points"])
def test_encoder_512_column_form(dev, rays, stage):
    from hosnerf_amd import ops
    tdist, o, d, radii, basis = _golden_rays(dev) if rays == "golden" else _ragged_rays(dev)
    P = tdist.shape[0] * (tdist.shape[1] - 1)
    embed = (torch.arange(64, dtype=torch.float32, device=dev) - 31.5) * 0.37          # mixed sign, none zero
    if stage == "frustum":
        rows = lambda e, ld: ops.encode_ipe(tdist, o, d, radii, basis, e, ld)
        planes = lambda e, ld: ops.encode_ipe_planes(tdist, o, d, radii, basis, e, ld)
    else:
        g = torch.Generator().manual_seed(7)
        pts = ((torch.rand(P, 3, generator=g) - 0.5) * 6.0).to(dev)                        # inside and outside the unit ball
        rows = lambda e, ld: ops.encode_ipe_points(pts, 0.01, basis, e, ld)
        planes = lambda e, ld: ops.encode_ipe_points_planes(pts, 0.01, basis, e, ld)
    old, new = rows(embed, 576), rows(None, 512)
    assert new.shape == (P, 512) and torch.equal(new[:, :504], old[:, :504])
    assert bool((new[:, 504:] == 0).all())
    # the old form, called the old way, keeps its layout
    assert torch.equal(old[:, 504:568], embed.expand(P, 64)) and bool((old[:, 568:] == 0).all())
    assert torch.isfinite(old[:, :504]).all() and float(old[:, :504].abs().max()) > 0.5
    o16, ob_ = planes(embed, 576)
    n16, nb = planes(None, 512)
    for po, pn in ((o16, n16), (ob_, nb)):
        assert pn.ld == 512 and pn.rows == P
        assert torch.equal(pn.hi[:, :504], po.hi[:, :504]) and torch.equal(pn.lo[:, :504], po.lo[:, :504])
        assert bool((pn.hi[:, 504:] == 0).all()) and bool((pn.lo[:, 504:] == 0).all())
    q16, qb = ops.split_planes2(old, C=576, ld=576)                                        # old planes = the split of the old rows
    assert torch.equal(o16.t, q16.t) and torch.equal(ob_.t, qb.t)
    r16, rb = ops.split_planes2(new, C=512, ld=512)
    assert torch.equal(n16.t, r16.t) and torch.equal(nb.t, rb.t)
    # a NULL embedding at the old width: zeros where the embedding stood
    wide = rows(None, 576)
    assert torch.equal(wide[:, :504], old[:, :504]) and bool((wide[:, 504:] == 0).all())


def test_encoder_row_widths_are_checked(dev):
    from hosnerf_amd import _lib, ops
    tdist, o, d, radii, basis = _golden_rays(dev)
    embed = torch.ones(64, device=dev)
    with pytest.raises(_lib.HosLibraryError):
        ops.encode_ipe(tdist, o, d, radii, basis, embed, 512)          # the embedding does not fit 512 columns
    with pytest.raises(_lib.HosLibraryError):
        ops.encode_ipe_planes(tdist, o, d, radii, basis, None, 480)
    with pytest.raises(_lib.HosLibraryError):
        ops.encode_ipe(tdist, o, d, radii, basis, None, 500)


# ------------------------------------------------------------------------------------------ 2. bias fold
def _fold_inputs(N, skip, n_states, seed):
    g = torch.Generator().manual_seed(seed)
    ldw = (N if skip else 0) + 576
    c0 = (N if skip else 0) + 504
    W = torch.randn(N, ldw, generator=g) / 24.0
    b = torch.randn(N, generator=g) * 0.05
    embeds = torch.randn(n_states, 64, generator=g)                       # mixed sign
    return W, b, embeds, c0


def fold_reference(W, b, e, c0):
    """(float64 value, float32 value summed one term after the other, sum |w e|) of b + W[:, c0:c0+len(e)] @ e."""
    E = e.numel()
    w64, e64 = W[:, c0:c0 + E].double(), e.double()
    ref64 = b.double() + (w64 * e64).sum(1)
    acc = b.clone()
    for k in range(E):
        acc = acc + W[:, c0 + k] * e[k]                                    # fp32, sequential: the worst order
    return ref64, acc, (w64 * e64).abs().sum(1)


@pytest.mark.parametrize("N", [256, 1024])
@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("n_states", [1, 3])
def test_bias_fold_vs_float64(dev, N, skip, n_states):
    """Bound: |b' - fp32(float64 value)| <= k 2^-24 sum |w e| per output, k = twice what the sequential float32 reference itself
    needs on the same inputs (both factors are written to the suite's parity record; profiles/embed_bias_fold_k.json is a copy
    of those entries)."""
    from hosnerf_amd import ops
    from tests._record import record
    W, b, embeds, c0 = _fold_inputs(N, skip, n_states, 100 + N + 7 * skip + n_states)
    e = embeds[n_states - 1]
    ref64, ref32, S = fold_reference(W, b, e, c0)
    target = ref64.float().double()
    k = 2.0 * float(((ref32.double() - target).abs() / (EPS * S)).max())
    Wd, bd, ed = W.to(dev), b.to(dev), embeds.to(dev)[n_states - 1]
    out = ops.embed_bias_fold([Wd], [c0], [bd], ed, N)[0]
    again = ops.embed_bias_fold([Wd], [c0], [bd], ed, N)[0]
    assert torch.equal(out, again)
    ratio = float(((out.double().cpu() - target).abs() / (EPS * S)).max())
    print(f"embed_bias_fold N={N} c0={c0} states={n_states}: k_ref x2 = {k:.3f}, kernel {ratio:.3f}")
    record(f"embed_bias.fold_k[N={N},c0={c0},states={n_states}]", {"float32_sequential_reference_factor": k / 2.0, "bound_k": k, "kernel_factor": ratio})
    assert ratio <= k, (ratio, k)
    # two layers in one launch give the same bits as one each; a NULL bias is a zero bias
    W2, b2, _, c2 = _fold_inputs(N, not skip, 1, 5)
    both = ops.embed_bias_fold([Wd, W2.to(dev)], [c0, c2], [bd, None], ed, N)
    assert torch.equal(both[0], out)
    assert torch.equal(both[1], ops.embed_bias_fold([W2.to(dev)], [c2], [torch.zeros(N, device=dev)], ed, N)[0])


@pytest.mark.parametrize("E", [1, 40])
def test_bias_fold_short_embedding_and_many_layers(dev, E):
    """An embedding shorter than a wave (lanes E.. hold no product), same bound as above; and more layers than one launch takes
    (six: two launches) give the bits of one launch each."""
    from hosnerf_amd import ops
    N = 256
    W, b, embeds, c0 = _fold_inputs(N, True, 1, 900 + E)
    e = embeds[0, :E].contiguous()
    ref64, ref32, S = fold_reference(W, b, e, c0)
    target = ref64.float().double()
    k = 2.0 * max(float(((ref32.double() - target).abs() / (EPS * S)).max()), 0.5)     # never below one rounding of the result
    Wd, bd, ed = W.to(dev), b.to(dev), e.to(dev)
    out = ops.embed_bias_fold([Wd], [c0], [bd], ed, N)[0]
    ratio = float(((out.double().cpu() - target).abs() / (EPS * S)).max())
    print(f"embed_bias_fold E={E}: k_ref x2 = {k:.3f}, kernel {ratio:.3f}")
    assert ratio <= k, (ratio, k)
    c0s = [c0, c0 - 8, c0 + 8 - E // 8, 0, c0, 504]
    six = ops.embed_bias_fold([Wd] * 6, c0s, [bd, None, bd, bd, None, bd], ed, N)
    for o, c, bb in zip(six, c0s, [bd, None, bd, bd, None, bd]):
        assert torch.equal(o, ops.embed_bias_fold([Wd], [c], [bb], ed, N)[0])


# ------------------------------------------------------------------------------------------ 3. the MLPs
MODES = {"fp32": "GEMM_FP32", "split": "GEMM_BF16X3", "planes": "GEMM_PLANES"}


@pytest.fixture(params=list(MODES))
def mode(request, dev):
    from hosnerf_amd import ops
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(getattr(ops, MODES[request.param]))
    yield request.param
    ops.set_gemm_mode(prev)


def _make_mlp(kind, dev, d):
    from hosnerf_amd.mipnerf360 import NeRFMLP, PropMLP
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.3}, "f1": {"time": 0.6}}, f)              # three states; time 0.5 selects state 1
    torch.manual_seed(1234)
    return (NeRFMLP if kind == "nerf" else PropMLP)(d).to(dev)


@pytest.fixture(scope="module")
def mlps(dev, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("embed_bias"))
    return {k: _make_mlp(k, dev, d) for k in ("nerf", "prop")}


def _rays(dev, shape):
    if shape == "8x32":
        b = synth.stage1_batch(8, seed=3)
        g = torch.Generator().manual_seed(3)
        tdist = torch.cumsum(torch.rand(8, 33, generator=g) * 0.3 + 0.01, -1) + 0.1
        return tdist.to(dev), b["rays_o"].to(dev).contiguous(), b["rays_d"].to(dev).contiguous(), b["radii"].to(dev).contiguous(), b["viewdirs"].to(dev).contiguous()
    B, S = (int(v) for v in shape.split("x"))
    tdist, o, d, radii, _ = _ragged_rays(dev, B, S)
    return tdist, o, d, radii, synth.stage1_batch(B, seed=31)["viewdirs"].to(dev).contiguous()


def _reference(sd, ipe, viewdirs, S, state, W, dtype, cot, masks, mask_v):
    """The reference-layout computation (oracle.background.mlp_forward after its encoder: the embedding as 64 columns of every row)
    from the IPE features `ipe` [P,504], in `dtype`; returns (layer outputs, density, rgb | None, gradients by state_dict name).
    Every ReLU is applied as the 0/1 mask the device's forward took (`masks` per trunk layer, `mask_v` of the view layer): a
    pre-activation within rounding of 0 that falls on the other side in another arithmetic changes a whole row of the gradients
    (tests/test_gpu_bkgd.py::test_gradients_vs_oracle says the same of its 128 samples), which is no error of the kernels under
    test; the forward checks above hold the layers this file is about against float64 without any such help."""
    import torch.nn.functional as F
    import oracle.background as ob
    p = {k: v.detach().cpu().to(dtype).requires_grad_(v.dtype.is_floating_point and "basis" not in k) for k, v in sd.items()}
    w = ob.MLPWeights(p)
    x = torch.cat([ipe.to(dtype), w.embeds[state].expand(ipe.shape[0], 64)], -1)
    inputs, outs = x, []
    for idx, (Wt, b) in enumerate(w.pts):
        x = F.linear(x, Wt, b) * masks[idx].to(dtype)
        outs.append(x)
        if idx % 4 == 0 and idx > 0:
            x = torch.cat([x, inputs], -1)
    density = F.softplus(F.linear(x, *w.density)[..., 0] - 1.0)
    rgb = None
    loss = (density * cot[0].to(dtype)).sum()
    if w.has_rgb:
        bott = F.linear(x, *w.bottleneck)
        de = ob.pos_enc(viewdirs.cpu().to(dtype), 0, 4, True).repeat_interleave(S, 0)
        h = F.linear(torch.cat([bott, de], -1), *w.views) * mask_v.to(dtype)
        rgb = torch.sigmoid(F.linear(h, *w.rgb)) * (1 + 2 * 0.001) - 0.001
        loss = loss + (rgb * cot[1].to(dtype)).sum()
    loss.backward()
    return outs, density.detach(), None if rgb is None else rgb.detach(), {k: v.grad for k, v in p.items() if v.requires_grad and v.grad is not None}


# what the existing GEMM unit tests allow one layer at unit scale (tests/test_gpu_bkgd.py): test_linear_fwd 2e-5 (fp32) and 10 x
# that (split), test_planes_gemm_matches_fp64 2e-5 (fp16 planes) and 2e-4 (bf16 planes)
def _layer_tol(mode, bf16):
    return {"fp32": 2e-5, "split": 2e-4, "planes": 2e-4 if bf16 else 2e-5}[mode]


@pytest.mark.parametrize("kind", ["nerf", "prop"])
@pytest.mark.parametrize("shape", ["8x32", "300x33", "301x32"])
def test_mlp_forward_and_gradients(dev, mlps, mode, kind, shape):
    """Forward: the two layers that read X (layer 0, the skip consumer), each against float64 from the operands that layer read
    on the device, with the embedding as columns -- bound: the existing GEMM unit tests' for that mode, times max(1, max |ref|).
    Gradients from accumulators pre-filled with G0 != 0, against float64 autograd of the whole reference-layout MLP (ReLUs as the
    device's masks, see `_reference`) -- bound: the model-level one of tests/test_gpu_bkgd.py::test_gradients_vs_oracle,
    e_hip <= 2 e_ref + 2e-4 max |t| with e_ref the error of the same graph in float32; and the algebra the fold relies on, to
    rounding: dW[:, embedding columns] - G0 = db (x) embed.

    `dW[:, 504:512]`: these are the first 8 embedding weights, whose gradient is db (x) embed[:8] like the other 56; what must hold
    is that the weight-gradient GEMM over the 512-column rows adds exactly 0 there (test_wgrad_over_512_columns_adds_exact_zero)
    and that the padding columns 568:576 keep G0 bit for bit (here).

    Density and colour of the whole MLP against the same float64 graph, same form of bound.

    Planes mode at 300 x 33 = 9900 rows: hos_linearp_wgrad takes row counts that are multiples of 32 only (HOS_E_SHAPE otherwise,
    before and after this change), so there only the forward is checked; 301 x 32 = 9632 rows is the ragged shape whose gradients
    all three modes are held to (partial last encoder workgroup, partial last GEMM tile, several split-K slabs)."""
    from hosnerf_amd import ops
    from hosnerf_amd.mipnerf360 import X_LD, select_state
    mlp = mlps[kind]
    W, state = mlp.netwidth, 1
    assert select_state(0.5, mlp.transitions_times) == state and len(mlp.bkgd_stateembeds) == 3
    tdist, o, d, radii, viewdirs = _rays(dev, shape)
    B, S = tdist.shape[0], tdist.shape[1] - 1
    P = B * S
    planes = mode == "planes"
    bf16 = planes and mlp._bf16_fwd()
    if planes:
        X = ops.encode_ipe_planes(tdist, o, d, radii, mlp.pos_basis_t, None, X_LD, want_bf16=True, want_fp16=not bf16)
    else:
        X = ops.encode_ipe(tdist, o, d, radii, mlp.pos_basis_t, None, X_LD)
    ipe32 = ops.encode_ipe(tdist, o, d, radii, mlp.pos_basis_t, None, X_LD)[:, :504].cpu()
    with torch.no_grad():
        density, rgb, saved = mlp._forward_impl(X, viewdirs, B, S, save=True, state=state)
    sd = mlp.state_dict()
    skip = sorted(mlp._skip_consumers)[0] if mlp._skip_consumers else None
    if planes:
        sv = saved[0]
        x_read = (sv.Xb if bf16 else sv.X16).float()[:, :504].double().cpu()
        acts = [y.float()[:, :W].double().cpu() for y in sv.y16]
    else:
        x_read = saved[0][:, :504].double().cpu()
        acts = [a.double().cpu() for a in saved[1]]
    e64 = sd[f"bkgd_stateembeds.{state}"].double().cpu()
    xin = torch.cat([x_read, e64.expand(P, 64)], -1)
    tol = _layer_tol(mode, bf16)
    checks = [(0, xin)] + ([(skip, torch.cat([acts[skip - 1], xin], -1))] if skip is not None and skip < len(acts) else [])
    for i, inp in checks:
        ref = torch.relu(inp @ sd[f"pts_linear.{i}.weight"].double().cpu().T + sd[f"pts_linear.{i}.bias"].double().cpu())
        err = float((acts[i] - ref).abs().max())
        print(f"{kind} {shape} {mode}: layer {i} err {err:.3e} (max |ref| {float(ref.max()):.3f}, bound {tol * max(1.0, float(ref.max())):.1e})")
        assert err <= tol * max(1.0, float(ref.max())), (i, err)

    # gradients
    g = torch.Generator().manual_seed(P)
    cot = (torch.randn(P, generator=g) / P, torch.randn(P, 3, generator=g) / P)
    n = mlp.store.grad.numel()
    G0 = (((torch.arange(n) % 5) - 2).float() * 2.0 ** -10).to(dev)
    emb = mlp._embeds.view(G0)
    emb[0].zero_(); emb[2].zero_()                  # the states that take no part: their rows must stay identically zero
    mlp.store.grad.copy_(G0)
    g_rgb = None if rgb is None else cot[1].to(dev)
    backward = not (planes and P % 32)               # the planes weight-gradient GEMM refuses such a row count (docstring)
    if backward:
        mlp._backward_impl(saved, density, rgb, cot[0].to(dev), g_rgb, state)
    got = {k: (p.grad.double() - mlp_view(mlp, G0, k).double()).cpu() for k, p in mlp.named_parameters()}
    raw = {k: p.grad.clone() for k, p in mlp.named_parameters()}
    gemb_all = mlp._embeds.view(mlp.store.grad).clone()
    g0pad = {i: mlp._layers[i].W.view(G0) for i, _ in checks}
    gpad = {i: mlp._layers[i].W.view(mlp.store.grad).clone() for i, _ in checks}
    mlp.zero_grad()
    masks = [a > 0 for a in acts]
    mask_v = None if rgb is None else (saved[3] > 0).cpu()
    r64, r32 = (_reference(sd, ipe32, viewdirs, S, state, W, dt, cot, masks, mask_v) for dt in (torch.float64, torch.float32))
    g64, g32 = r64[3], r32[3]
    for what, a, t, r in (("density", density, r64[1], r32[1]), ("rgb", rgb, r64[2], r32[2])):
        if a is None:
            continue
        a, r = a.double().cpu().reshape(t.shape), r.double()
        e_hip, e_ref, scale = float((a - t).abs().max()), float((r - t).abs().max()), float(t.abs().max())
        print(f"{kind} {shape} {mode}: {what} e_hip {e_hip:.3e} e_ref {e_ref:.3e} max|t| {scale:.3e}")
        assert scale > 0 and e_hip <= 2.0 * e_ref + 2e-4 * scale, (what, e_hip, e_ref, scale)
    if not backward:
        return

    def bounded(name, sl=None):
        a, t, r = got[name], g64[name], g32[name].double()
        if sl is not None:
            a, t, r = a[:, sl], t[:, sl], r[:, sl]
        e_hip, e_ref, scale = float((a - t).abs().max()), float((r - t).abs().max()), float(t.abs().max())
        print(f"{kind} {shape} {mode}: {name}{'' if sl is None else [sl.start, sl.stop]} e_hip {e_hip:.3e} e_ref {e_ref:.3e} max|t| {scale:.3e}")
        assert scale > 0 and e_hip <= 2.0 * e_ref + 2e-4 * scale, (name, e_hip, e_ref, scale)

    embed32 = sd[f"bkgd_stateembeds.{state}"].double().cpu()
    for i, _ in checks:
        c0 = 504 if i == 0 else W + 504
        wn, bn = f"pts_linear.{i}.weight", f"pts_linear.{i}.bias"
        bounded(wn, slice(c0, c0 + 64))                 # the rank-1 term
        bounded(wn, slice(c0 - 504, c0))                # the IPE columns, from the 512-column weight-gradient GEMM
        bounded(bn)
        # dW[:, embedding columns] - G0 = db (x) embed to rounding: db is recovered from gb - G0 within 2^-24 |gb|, the product and
        # the accumulation round once each
        db = got[bn]
        lhs = got[wn][:, c0:c0 + 64]
        slack = EPS * (raw[bn].double().abs().cpu()[:, None] * embed32.abs()[None] + (db[:, None] * embed32[None]).abs()
                       + raw[wn][:, c0:c0 + 64].double().abs().cpu())
        assert bool(((lhs - db[:, None] * embed32[None]).abs() <= 2.0 * slack).all()), i
        # the zero padding of the weight rectangle keeps its accumulator bit for bit
        assert torch.equal(gpad[i][:, c0 + 64:c0 + 72], g0pad[i][:, c0 + 64:c0 + 72])
    bounded_embed = got[f"bkgd_stateembeds.{state}"]
    t, r = g64[f"bkgd_stateembeds.{state}"], g32[f"bkgd_stateembeds.{state}"].double()
    e_hip, e_ref, scale = float((bounded_embed - t).abs().max()), float((r - t).abs().max()), float(t.abs().max())
    print(f"{kind} {shape} {mode}: g_embed e_hip {e_hip:.3e} e_ref {e_ref:.3e} max|t| {scale:.3e}")
    assert scale > 0 and e_hip <= 2.0 * e_ref + 2e-4 * scale
    assert bool((gemb_all[0] == 0).all()) and bool((gemb_all[2] == 0).all())


def mlp_view(mlp, flat, name):
    """The window of the flat buffer `flat` that parameter `name` of `mlp` is bound to."""
    p = dict(mlp.named_parameters())[name]
    off = (p.data_ptr() - mlp.store.param.data_ptr()) // 4
    return torch.as_strided(flat, p.shape, p.stride(), off)


@pytest.mark.parametrize("M", [256, 9920])
def test_wgrad_over_512_columns_adds_exact_zero(dev, mode, M):
    """A weight-gradient GEMM over the 512-column rows into a [N, 576] rectangle: columns 504:512 meet X's zero padding and get
    exactly +0 (bit-identical accumulators), columns 512:576 are not touched."""
    from hosnerf_amd import ops
    g = torch.Generator().manual_seed(M)
    N = 256
    X = torch.zeros(M, 512)
    X[:, :504] = torch.randn(M, 504, generator=g)
    dY = torch.randn(M, N, generator=g)
    G0 = torch.randn(N, 576, generator=g).to(dev)
    dW, db = G0.clone(), torch.zeros(N, device=dev)
    if mode == "planes":
        _, Xb = ops.split_planes2(X.to(dev), want16=False)
        _, dZ = ops.split_planes2(dY.to(dev), want16=False)
        ops.linearp_wgrad(dZ, Xb, dW, db, M, N, 512)
    else:
        ops.linear_wgrad(dY.to(dev), X.to(dev), dW, db, N, 512)
    assert torch.equal(dW[:, 504:], G0[:, 504:])
    ref = dY.double().T @ X[:, :504].double()
    assert float(((dW[:, :504] - G0[:, :504]).double().cpu() - ref).abs().max()) < 2e-4 * float(ref.abs().max()) + 1e-5
