"""What the background mesh costs at resolution 256, measured on one MI355X (a record, not a benchmark of the project: bench.py is;
there is no pass threshold).  The model is the benchmark's background `MipNeRF360` (`synth.background_state_dict(777, 2)`), the box
the launcher's default cube (-1,-1,-1, 1,1,1); the untrained field does not reach 0.5 at this spacing, so the level is the median of
the interior alphas (recorded).

Device events around each phase of `mesh.extract_bkgd`, --repeats times after one warm-up round of every shape, min and median
reported: the point encoder (`ops.encode_ipe_points_planes` over the chunks, the one plane format the NeRF MLP consumes), the MLP
(`MipNeRF360MLP._forward_impl` on those rows), the alpha kernel (`ops.grid_alpha_density`), and march + normals + vertex colours
(`ops.march_tets` with its read-back, `ops.mesh_vertex_normals`, the second `query_points` at the vertices); next to them
`mesh.bkgd_field` and `mesh.extract_bkgd` as a whole.  Grid generation (`ops.grid_points`) is inside the wholes only.

The encoder pair, same process, 262 144 rows, one plane format (bf16), --encoder_repeats launches each after a warm-up: the point
encoder next to the frustum encoder (4096 rays x 64 samples of `synth.stage1_batch`) -- the figure hos_encode.hip quotes.

Everything lands in --out (default profiles/bkgd_mesh_cost.json)."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bkgd_mesh_cost.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--encoder_repeats", type=int, default=50)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=1 << 18)
    args = ap.parse_args()

    import torch
    from hosnerf_amd import mesh, ops, synth
    from hosnerf_amd.mipnerf360 import X_LD, MipNeRF360
    dev = torch.device("cuda")
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    model = MipNeRF360(d, opaque_background=True)
    model.load_state_dict(synth.background_state_dict(777, 2), strict=False)
    model = model.to(dev)
    mlp = model.mlps[-1]
    box, time = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0), 0.7

    def timed(store, key, fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        t1.synchronize()
        store.setdefault(key, []).append(t0.elapsed_time(t1))
        return out

    field = mesh.bkgd_field(model, box, time, resolution=args.resolution, chunk=args.chunk)
    level = float(field["alpha"][1:-1, 1:-1, 1:-1].median())
    origin, h, dims, var = field["origin"], field["spacing"], field["dims"], field["var"]
    Nx, Ny, Nz = dims
    N = Nx * Ny * Nz
    firsts = list(range(0, N, args.chunk))
    embed = None            # the MLP's row form: no embedding columns, the state embedding enters as a bias
    planes = mlp._use_planes()
    one_fmt = mlp._bf16_fwd()
    alpha = torch.empty_like(field["alpha"])
    view = torch.tensor([mesh.HEAD_ON_FALLBACK], device=dev)
    times = {}

    def encode(pts):
        if planes:
            return ops.encode_ipe_points_planes(pts, var, mlp.pos_basis_t, embed, X_LD, want_bf16=one_fmt, want_fp16=not one_fmt)
        return ops.encode_ipe_points(pts, var, mlp.pos_basis_t, embed, X_LD)

    with mesh._evaluating_bkgd(model), ops.gemm_mode(ops.get_gemm_mode() if model.gemm_mode is None else model.gemm_mode):
        for rep in range(args.repeats + 1):
            enc = mlp_ms = alpha_ms = 0.0
            for first in firsts:                                   # chunk by chunk, as bkgd_field: the rows of one chunk are all that is alive
                rows = min(args.chunk, N - first)
                pts = ops.grid_points(origin, h, dims, first, rows, device=dev)
                vd = view.expand(rows, 3).contiguous()
                part = {}
                X = timed(part, "e", lambda: encode(pts))
                dens = timed(part, "m", lambda: mlp._forward_impl(X, vd, rows, 1, save=False, state=field["state"])[0])
                timed(part, "a", lambda: ops.grid_alpha_density(dens, h, dims, first, alpha))
                enc, mlp_ms, alpha_ms = enc + part["e"][0], mlp_ms + part["m"][0], alpha_ms + part["a"][0]
                del X, dens
            times.setdefault("encoder", []).append(enc)
            times.setdefault("mlp", []).append(mlp_ms)
            times.setdefault("alpha_kernel", []).append(alpha_ms)

            def surface():
                vertices, _, faces = ops.march_tets(alpha, level, origin, h)
                vn = ops.mesh_vertex_normals(alpha, origin, h, vertices)
                vdirs = mesh.head_on_viewdirs(vn)
                rgb = torch.empty(vertices.shape[0], 3, device=dev)
                for v0 in range(0, vertices.shape[0], args.chunk):
                    sl = slice(v0, min(v0 + args.chunk, vertices.shape[0]))
                    rgb[sl] = mlp.query_points(vertices[sl].contiguous(), var, vdirs[sl].contiguous(), time)["rgb"]
                return vertices, faces

            vertices, faces = timed(times, "march_normals_vertex_colours", surface)
    same = bool(torch.equal(alpha, field["alpha"]))
    for rep in range(args.repeats + 1):
        timed(times, "bkgd_field_whole", lambda: mesh.bkgd_field(model, box, time, resolution=args.resolution, chunk=args.chunk))
        whole = timed(times, "extract_bkgd_whole", lambda: mesh.extract_bkgd(model, box, time, resolution=args.resolution, level=level, chunk=args.chunk))
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    assert V == int(whole["vertices"].shape[0]) and F == int(whole["faces"].shape[0])

    # the encoder pair at 262 144 rows, one plane format (bf16)
    R = 262144
    enc_times = {}
    pts = ops.grid_points(origin, h, dims, N // 2 - R // 2, R, device=dev)
    b = {k: v.to(dev) for k, v in synth.stage1_batch(4096, seed=777).items()}
    _, tdist = ops.resample(torch.tensor([[0.0, 1.0]], device=dev).repeat(4096, 1), torch.ones(4096, 1, device=dev), 64, 0.5025, 1.0, False, 0.1, 1e6)
    for rep in range(args.encoder_repeats + 1):
        timed(enc_times, "point", lambda: ops.encode_ipe_points_planes(pts, var, mlp.pos_basis_t, embed, X_LD, want_bf16=True, want_fp16=False))
        timed(enc_times, "frustum", lambda: ops.encode_ipe_planes(tdist, b["rays_o"], b["rays_d"], b["radii"], mlp.pos_basis_t, embed, X_LD,
                                                                  want_bf16=True, want_fp16=False))
    stat = lambda v: {"min": min(v[1:]), "median": statistics.median(v[1:])}                 # the first round is the warm-up
    res = {"workload": f"mesh.extract_bkgd phases, benchmark background weights (synth.background_state_dict(777, 2)), box {list(box)}, time {time} "
                       f"(state {field['state']}), resolution {args.resolution}, dims {list(dims)} = {N} vertices, {len(firsts)} chunks of {args.chunk} rows, "
                       f"level {level:.6g} (median of the interior alphas), gemm mode {ops.get_gemm_mode()}, 1 GPU, device events",
           "repeats": args.repeats, "alpha_bit_identical_to_bkgd_field": same, "V": V, "F": F, "volume": whole["volume"], "area": whole["area"],
           "ms": {k: stat(v) for k, v in times.items()},
           "encoder_us_per_262144_rows_bf16_planes": {k: {s: 1e3 * x for s, x in stat(v).items()} for k, v in enc_times.items()},
           "encoder_repeats": args.encoder_repeats,
           "note": "encoder / mlp / alpha_kernel: sums over the chunks of one field; the wholes include ops.grid_points, the density copy and the "
                   "range guard's read-back; the frustum encoder's rows are 4096 rays x 64 level-0 samples of synth.stage1_batch"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
