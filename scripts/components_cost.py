"""What labelling, measuring and dropping a mesh's components costs, measured on one MI355X (a record, not a benchmark of the
project: bench.py is; there is no pass threshold).  Three cases, each on the synthetic weights of the tests:

  canonical   the resolution-256 canonical template of the stage-3 `Network` (`mesh.extract` at the median of the positive alphas)
  frame       the posed frame mesh of the same network (`mesh.extract_frame`, body space) at the median level of the untrained
              field: millions of vertices of noise, the hard case for rounds
  bkgd        `mesh.extract_bkgd` of the benchmark's background weights in the launcher's default box, with and without
              `min_area_ratio`: how many vertices the colour query is spared and the time that saves (on an untrained field this
              may be nothing; it is reported as it is)

Device events, the median (and the minimum) of --repeats runs after one warm-up round of every shape, one process.  Per mesh: the
rounds the labelling took; each ENTRY POINT of hos_components.hip on its own (a round is its hook and jump launches, the ids four
launches, the compaction's two halves two each: include/hosrender.h), the labelling rounds replayed without the read-backs;
torch's stable sort of the face ids; `mesh.components` and `mesh.drop_floaters` as a whole, read-backs included -- next to
`ops.march_tets` of the same field and to the evaluation of that field (`mesh.canonical_field` / `mesh.frame_field`), so that a
reader sees whether the clean-up matters beside the field.

Everything lands in --out (default profiles/components_cost.json)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_cost.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--bkgd_resolution", type=int, default=256)
    ap.add_argument("--ratio", type=float, default=0.05)
    ap.add_argument("--cases", default="canonical,frame,bkgd")
    args = ap.parse_args()

    import torch
    from hosnerf_amd import _lib, formats, mesh, ops, synth, tpose
    from hosnerf_amd._lib import call, ptr
    from hosnerf_amd.eval import FRAME_KEYS
    from hosnerf_amd.human_nerf import Network, default_cfg
    dev = torch.device("cuda")
    d = tempfile.mkdtemp(prefix="hos_basedir_")
    with open(os.path.join(d, "transitions_times.json"), "w") as f:
        json.dump({"f0": {"time": 0.4}}, f)
    I32, I64, F64, U8 = torch.int32, torch.int64, torch.float64, torch.uint8

    def timed(store, key, fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        t1.synchronize()
        store.setdefault(key, []).append(t0.elapsed_time(t1))
        return out

    stat = lambda v: {"median": statistics.median(v[1:]), "min": min(v[1:])}                    # the first round is the warm-up

    def measure(vertices, faces, field, field_fn, level, rgb):
        """One mesh: the entry points one by one, then the wholes."""
        V, F = int(vertices.shape[0]), int(faces.shape[0])
        first = mesh.components(vertices, faces)
        rounds, C = int(first["rounds"]), int(first["count"])
        nbv, nbf = _lib.load().hos_mesh_blocks(V), _lib.load().hos_mesh_blocks(F)
        keep = mesh.keep_flags(first, args.ratio)
        t, seen = {}, [rounds]
        for rep in range(args.repeats + 1):
            label, component, words = torch.empty(V, dtype=I32, device=dev), torch.empty(V, dtype=I32, device=dev), torch.empty(4, dtype=I32, device=dev)
            timed(t, "label_begin", lambda: call("hos_mesh_label_begin", V, ptr(label, I32), ptr(words, I32)))
            per_round = {}
            for k in range(rounds):                        # the rounds the host loop ran, replayed without its read-backs
                timed(per_round, k, lambda: call("hos_mesh_label_round", ptr(faces, I32), F, V, k, ptr(label, I32), ptr(words, I32)))
            t.setdefault("label_rounds_sum", []).append(sum(v[0] for v in per_round.values()))
            t.setdefault("label_round_first", []).append(per_round[0][0])
            t.setdefault("label_round_last", []).append(per_round[rounds - 1][0])
            k = rounds                                     # stale loads differ from run to run: finish, untimed, if this replay needs more rounds
            while words.tolist()[1 + ((k - 1) & 1)]:
                call("hos_mesh_label_round", ptr(faces, I32), F, V, k, ptr(label, I32), ptr(words, I32))
                k += 1
            seen.append(k)
            ws = torch.empty(nbv, dtype=I32, device=dev)
            timed(t, "component_ids", lambda: call("hos_mesh_component_ids", ptr(label, I32), V, ptr(component, I32), ptr(ws, I32), ptr(words, I32)))
            assert torch.equal(label, first["label"]) and torch.equal(component, first["component"])
            fc, terms = torch.empty(F, dtype=I32, device=dev), torch.empty(F, 2, dtype=F64, device=dev)
            nv, nf = torch.zeros(C, dtype=I64, device=dev), torch.zeros(C, dtype=I64, device=dev)
            area, volume = torch.zeros(C, dtype=F64, device=dev), torch.zeros(C, dtype=F64, device=dev)
            timed(t, "component_terms", lambda: call("hos_mesh_component_terms", ptr(vertices), ptr(faces, I32), ptr(component, I32), V, F, C,
                                                     ptr(fc, I32), ptr(terms, F64), ptr(nv, I64), ptr(nf, I64)))
            order = timed(t, "torch_stable_sort", lambda: torch.sort(fc, stable=True).indices.contiguous())
            start = ((F - nf.sum()) + torch.cumsum(nf, 0) - nf).contiguous()
            timed(t, "component_sums", lambda: call("hos_mesh_component_sums", ptr(terms, F64), ptr(order, I64), ptr(start, I64), ptr(nf, I64), F, C,
                                                    ptr(area, F64), ptr(volume, F64)))
            assert torch.equal(area, first["area"]) and torch.equal(volume, first["volume"])            # bit-equal from run to run
            ws2, counts = torch.empty(nbv + nbf, dtype=I32, device=dev), torch.empty(2, dtype=I32, device=dev)
            timed(t, "compact_count", lambda: call("hos_mesh_compact_count", ptr(keep, U8), C, ptr(component, I32), V, ptr(faces, I32), ptr(fc, I32), F,
                                                   ptr(ws2, I32), ptr(counts, I32)))
            Vo, Fo = (int(c) for c in counts.tolist())
            new_id, ov, of = torch.empty(V, dtype=I32, device=dev), torch.empty(Vo, 3, device=dev), torch.empty(Fo, 3, dtype=I32, device=dev)
            timed(t, "compact_write", lambda: call("hos_mesh_compact_write", ptr(keep, U8), C, ptr(component, I32), V, ptr(faces, I32), ptr(fc, I32), F,
                                                   ptr(ws2, I32), ptr(new_id, I32), ptr(vertices), 0, 0, Vo, Fo, ptr(ov), 0, 0, ptr(of, I32)))
            del label, component, fc, terms, order, new_id, ov, of
            m = {"vertices": vertices, "faces": faces, "colors": None, "normals": None}
            seen.append(int(timed(t, "mesh_components_whole", lambda: mesh.components(vertices, faces))["rounds"]))
            dropped = timed(t, "mesh_drop_floaters_whole", lambda: mesh.drop_floaters(m, min_area_ratio=args.ratio))
            timed(t, "march_tets", lambda: ops.march_tets(field["alpha"], level, field["origin"], field["spacing"], rgb=rgb))
            timed(t, "field_evaluation", field_fn)
        nfaces = first["n_faces"]
        return {"V": V, "F": F, "components": C, "rounds": rounds, "rounds_seen_over_all_runs": sorted(set(seen)), "invalid_faces": int(first["invalid_faces"]), "level": level,
                "largest_component_faces": int(nfaces.max()) if C else 0, "components_of_at_most_8_faces": int((nfaces <= 8).sum()),
                "negative_volume_components": int((first["volume"] < 0).sum()), "min_area_ratio": args.ratio,
                "kept": dropped["components"]["kept"], "V_dropped": dropped["components"]["V_dropped"], "F_dropped": dropped["components"]["F_dropped"],
                "ms": {k: stat(v) for k, v in t.items()},
                "components_over_field_evaluation": stat(t["mesh_components_whole"])["median"] / stat(t["field_evaluation"])["median"],
                "drop_floaters_over_field_evaluation": stat(t["mesh_drop_floaters_whole"])["median"] / stat(t["field_evaluation"])["median"],
                "drop_floaters_over_march_tets": stat(t["mesh_drop_floaters_whole"])["median"] / stat(t["march_tets"])["median"]}

    res = {"what": "hos_components.hip per entry point and mesh.components / mesh.drop_floaters as wholes next to ops.march_tets and the field "
                   "evaluation of the same mesh; device events, median and min of the repeats after one warm-up round, 1 GPU, one process",
           "repeats": args.repeats, "cases": {}}
    cases = args.cases.split(",")
    if "canonical" in cases or "frame" in cases:
        net = Network(default_cfg(d), stage=3)
        net.load_state_dict(synth.human_state_dict(777, 2), strict=True)
        net = net.to(dev)
        joints = synth.tpose_joints()
        turn = tpose.TposeTurn(joints, formats.skeleton_bbox(joints, float(net.cfg.bbox_offset)), 32, dev)
    if "canonical" in cases:
        field = mesh.canonical_field(net, turn.const, 0.7, resolution=args.resolution)
        level = float(field["alpha"][field["alpha"] > 0].median())
        v, _, f = ops.march_tets(field["alpha"], level, field["origin"], field["spacing"], rgb=field["rgb"])
        res["cases"]["canonical"] = {"workload": f"mesh.extract of the stage-3 Network on synthetic weights, time 0.7, resolution {args.resolution}, dims "
                                                 f"{list(field['dims'])}, level the median of the positive alphas",
                                     **measure(v, f, field, lambda: mesh.canonical_field(net, turn.const, 0.7, resolution=args.resolution), level, field["rgb"])}
        print(json.dumps(res["cases"]["canonical"]), flush=True)
        del field, v, f
    if "frame" in cases:
        hb = synth.human_batch(8, seed=3, time=0.7, is_train=False, iter_val=1e7)
        pose = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in hb.items() if k in FRAME_KEYS}
        pose.update(time=0.7, is_train=False, frame_name="frame_070",
                    dst_bbox={"min_xyz": hb["dst_bbox_min_xyz"].numpy(), "max_xyz": hb["dst_bbox_max_xyz"].numpy()})
        field = mesh.frame_field(net, pose, resolution=args.resolution)
        level = float(field["alpha"][field["alpha"] > 0].median())
        v, _, f = ops.march_tets(field["alpha"], level, field["origin"], field["spacing"], rgb=field["rgb"])
        res["cases"]["frame"] = {"workload": f"mesh.extract_frame of the same network, posed synth.human_batch frame, resolution {args.resolution}, dims "
                                             f"{list(field['dims'])}, level the median of the positive alphas of the untrained field (noise)",
                                 **measure(v, f, field, lambda: mesh.frame_field(net, pose, resolution=args.resolution), level, field["rgb"])}
        print(json.dumps(res["cases"]["frame"]), flush=True)
        del field, v, f
    if "bkgd" in cases:
        from hosnerf_amd.mipnerf360 import MipNeRF360
        model = MipNeRF360(d, opaque_background=True)
        model.load_state_dict(synth.background_state_dict(777, 2), strict=False)
        model = model.to(dev)
        box, time = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0), 0.7
        field = mesh.bkgd_field(model, box, time, resolution=args.bkgd_resolution)
        level = float(field["alpha"][1:-1, 1:-1, 1:-1].median())
        del field
        t = {}
        for rep in range(min(args.repeats, 5) + 1):
            whole = timed(t, "extract_bkgd", lambda: mesh.extract_bkgd(model, box, time, resolution=args.bkgd_resolution, level=level))
            V, F = int(whole["vertices"].shape[0]), int(whole["faces"].shape[0])
            del whole
            kept = timed(t, "extract_bkgd_filtered", lambda: mesh.extract_bkgd(model, box, time, resolution=args.bkgd_resolution, level=level,
                                                                              min_area_ratio=args.ratio))
            c, Vk = kept["components"], int(kept["vertices"].shape[0])
            del kept
        s = {k: stat(v) for k, v in t.items()}
        res["cases"]["bkgd"] = {"workload": f"mesh.extract_bkgd, benchmark background weights (synth.background_state_dict(777, 2)), box {list(box)}, time "
                                            f"{time}, resolution {args.bkgd_resolution}, level {level:.6g} (median of the interior alphas), without and with "
                                            f"min_area_ratio {args.ratio}",
                                "V": V, "F": F, "V_kept": Vk, "vertices_spared_the_colour_query": V - Vk, "components": c, "ms": s,
                                "ms_saved_by_the_filter": s["extract_bkgd"]["median"] - s["extract_bkgd_filtered"]["median"]}
        print(json.dumps(res["cases"]["bkgd"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
