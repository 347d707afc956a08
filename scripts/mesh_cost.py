"""What the canonical mesh costs at resolution 256, measured on one MI355X (a record, not a benchmark of the project: bench.py is; there
is no pass threshold).  The network is the stage-3 `Network` on the synthetic weights of the tests, the box the synthetic T-pose
skeleton's; its untrained field does not reach 0.5 at this spacing, so the level is the median of the positive alphas (recorded).

  phases   device events around each phase of `mesh.extract`, --repeats times after one warm-up of every shape: points + MLP
           (`ops.grid_points` + `Network._canonical_fwd` over the chunks), alpha (`ops.grid_alpha` over the chunks), count + scan
           (`hos_march_tets_count`: two launches), the (V, F) read-back, write (`hos_march_tets_write`), and the volume decoder.
  kernel   the march alone, --repeats times, meant to be run under a kernel trace of its own:
               rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/mesh_cost.py kernel
           `python scripts/mesh_cost.py stats <dir>` then reads the three march launches' statistics and sets the bytes each must
           move (formulas in the JSON) against its time.

Everything lands in --out (default profiles/mesh_cost.json), one section per sub-command."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def merge_out(path, section, value):
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[section] = value
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(data, f, indent=1)


def build(resolution):
    import torch
    from hosnerf_amd import formats, mesh, synth, tpose
    from hosnerf_amd.human_nerf import Network, default_cfg
    dev = torch.device("cuda")
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    net = Network(default_cfg(d), stage=3)
    net.load_state_dict(synth.human_state_dict(777, 2), strict=True)
    net = net.to(dev)
    joints = synth.tpose_joints()
    turn = tpose.TposeTurn(joints, formats.skeleton_bbox(joints, float(net.cfg.bbox_offset)), 32, dev)
    field = mesh.canonical_field(net, turn.const, 0.7, resolution=resolution)
    a = field["alpha"]
    level = float(a[a > 0].median())
    return torch, net, turn, field, level


def march_bytes(N, nblk, V, F, colors):
    """Bytes each march launch must move: count reads the field and writes the 7-entry edge table and two block counts; the scan reads
    and writes the block counts; write reads the field, per mesh vertex its table entry (and two colours), per triangle three table
    entries and three block offsets, and writes the outputs."""
    return {"count": 4 * N + 28 * N + 8 * nblk, "scan": 16 * nblk,
            "write": 4 * N + V * (4 + 12 + (24 + 12 if colors else 0)) + F * (3 * 8 + 12)}


def phases(args):
    torch, net, turn, field, level = build(args.resolution)
    from hosnerf_amd import mesh, ops
    from hosnerf_amd._lib import call, ptr
    from hosnerf_amd.eval import evaluating
    dev = field["alpha"].device
    const = turn.const
    origin, h, dims = field["origin"], field["spacing"], field["dims"]
    Nx, Ny, Nz = dims
    N = Nx * Ny * Nz
    rows = min(args.chunk, N)
    firsts = [min(c0, N - rows) for c0 in range(0, N, rows)]
    bmin, bscale = const["cnl_bbox_min_xyz"].contiguous(), const["cnl_bbox_scale_xyz"].contiguous()
    K = int(net.cfg.total_bones)
    alpha, rgb = torch.empty_like(field["alpha"]), torch.empty_like(field["rgb"])
    nblk = (N + ops.MT_BLOCK - 1) // ops.MT_BLOCK
    edge_slot = torch.empty(7 * N, dtype=torch.int32, device=dev)
    ws = torch.empty(2 * nblk, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    ga = ops._grid_args(origin, h, dims)
    times = {k: [] for k in ("volume_decoder", "points_mlp", "alpha", "count_scan", "readback", "write")}

    def timed(key, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        times[key].append(a.elapsed_time(b))
        return out

    V = F = 0
    with evaluating(net):
        for rep in range(args.repeats + 1):
            vol = timed("volume_decoder", lambda: net._motion_weight_volume(const["motion_weights_priors"]).contiguous())
            raws = timed("points_mlp", lambda: [net._canonical_fwd(ops.grid_points(origin, h, dims, f0, rows, device=dev), 1, save=False)[0] for f0 in firsts])
            timed("alpha", lambda: [ops.grid_alpha(r, vol, bmin, bscale, origin, h, dims, f0, alpha, rgb, K=K) for r, f0 in zip(raws, firsts)])
            del raws
            timed("count_scan", lambda: call("hos_march_tets_count", ptr(alpha), Nx, Ny, Nz, level, ptr(edge_slot, torch.int32), ptr(ws, torch.int32),
                                             ptr(counts, torch.int32)))
            V, F = timed("readback", lambda: [int(c) for c in counts.tolist()])
            vertices, colors, faces = torch.empty(V, 3, device=dev), torch.empty(V, 3, device=dev), torch.empty(F, 3, dtype=torch.int32, device=dev)
            timed("write", lambda: call("hos_march_tets_write", ptr(alpha), ptr(rgb), Nx, Ny, Nz, level, *ga[:4], ptr(edge_slot, torch.int32),
                                        ptr(ws, torch.int32), V, F, ptr(vertices), ptr(colors), ptr(faces, torch.int32)))
    same = bool(torch.equal(alpha, field["alpha"]))
    med = {k: statistics.median(v[1:]) for k, v in times.items()}                      # the first round is the warm-up
    march = med["count_scan"] + med["write"]
    volume, area = mesh.mesh_measures(vertices, faces)
    res = {"workload": f"mesh.extract phases, stage-3 Network on synthetic weights, resolution {args.resolution}, dims {list(dims)} = {N} vertices, "
                       f"{len(firsts)} chunks of {rows} rows, level {level:.6g} (median of the positive alphas), 1 GPU, device events",
           "repeats": args.repeats, "alpha_bit_identical_to_canonical_field": same, "V": V, "F": F, "volume": volume, "area": area, "median_ms": med,
           "min_ms": {k: min(v[1:]) for k, v in times.items()}, "max_ms": {k: max(v[1:]) for k, v in times.items()},
           "march_ms_over_points_mlp_ms": march / med["points_mlp"],
           "march_costs_more_than_the_mlp_phase": bool(march > med["points_mlp"]),
           "device_bytes_resolution": {"field": 4 * N, "rgb": 12 * N, "edge_table": 28 * N, "block_counts": 8 * nblk, "mesh": 24 * V + 12 * F + 3 * V}}
    merge_out(args.out, "phases", res)
    print(json.dumps(res))


def kernel(args):
    torch, net, turn, field, level = build(args.resolution)
    from hosnerf_amd import ops
    for _ in range(args.repeats + 1):
        v, c, f = ops.march_tets(field["alpha"], level, field["origin"], field["spacing"], rgb=field["rgb"])
    torch.cuda.synchronize()
    Nx, Ny, Nz = field["dims"]
    print("MESH_KERNEL " + json.dumps({"N": Nx * Ny * Nz, "V": v.shape[0], "F": f.shape[0], "level": level, "launches": args.repeats + 1}))


def stats(args):
    meta = json.loads(args.meta)
    N, V, F = meta["N"], meta["V"], meta["F"]
    need = march_bytes(N, (N + 255) // 256, V, F, True)
    rows = {}
    for path in glob.glob(os.path.join(args.trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            for key in ("count", "scan", "write"):
                if f"march_{key}_kernel" in r["Name"]:
                    ns = float(r["AverageNs"])
                    rows[key] = {"kernel": r["Name"], "calls": int(r["Calls"]), "mean_ns": ns, "min_ns": float(r["MinNs"]), "max_ns": float(r["MaxNs"]),
                                 "bytes_needed": need[key], "achieved_bytes_per_s": need[key] / (ns * 1e-9)}
    if set(rows) != {"count", "scan", "write"}:
        raise SystemExit(f"no march kernel statistics under {args.trace_dir}: {sorted(rows)}")
    rows.update(meta)
    rows["note"] = "rocprofv3 --kernel-trace --stats, the first (warm-up) launch included; bytes_needed: march_bytes() of scripts/mesh_cost.py"
    merge_out(args.out, "march_kernels", rows)
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("phases", "kernel", "stats"))
    ap.add_argument("trace_dir", nargs="?", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_cost.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=1 << 18)
    ap.add_argument("--meta", default=None, help="stats: the JSON the `kernel` run printed after MESH_KERNEL")
    args = ap.parse_args()
    {"phases": phases, "kernel": kernel, "stats": stats}[args.what](args)


if __name__ == "__main__":
    main()
