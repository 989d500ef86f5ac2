#!/usr/bin/env python3
"""The where pass alone, timed with HIP events on the config-5 batch (10k sampled tiles) planned with
properties.  Decode, assemble, bounding boxes, measures and property materialization once, 3 warm-up launches,
then `reps` rounds on the same buffers -- alternating, in the same run -- of: the where pass (WRITE mode) for
three predicates (one INT64 clause; `class in (3 literals)`; four mixed clauses), the geometric predicate pass
with a window over a quarter of each tile, and a device-to-device copy of as many bytes as the batch has mask
bytes (the floor of any pass that writes every mask).  Medians, and the algorithmic bytes of each predicate: per
bound clause and feature one validity bit and the value's bytes (BOOLEAN a bit, INT64 8, FLOAT and STRING 4;
none for a null test), plus one mask byte written (and one read in AND mode, not timed here).
usage: where_run.py [reps] [--json PATH]   (COVT_LIB_VARIANT picks the library)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from wkb_run import HBM_PEAK, clocks  # noqa: E402

PREDICATES = {
    "int64_clause": (("rank", "<=", 3),),
    "class_in_3": (("class", "in", ["motorway", "trunk", "primary"]),),
    "four_mixed": (("class", "in", ["motorway", "trunk", "primary"]), ("rank", "<=", 3, True), ("name:de", "is null"),
                   ("max-text-width", "==", 100.0, True)),
}


def algorithmic_bytes(covt, plan, where, bind):
    """(bytes read, bytes written, bound (clause, column) pairs) of one WRITE-mode pass over the plan."""
    value_bits = {covt.PROP_BOOLEAN: 1, covt.PROP_INT64: 64, covt.PROP_FLOAT: 32, covt.PROP_STRING: 32}
    by_desc = np.zeros(max(plan.num_property_columns, 1), np.int64)
    by_desc[plan.props["desc_index"]] = np.arange(plan.num_property_columns)
    live = (plan.select["flags"] == 0) & (plan.select["n_features"] > 0)
    bits = bound = 0
    for c in np.nonzero(live)[0]:
        n = int(plan.select["n_features"][c])
        row = bind[int(plan.select["desc_index"][c])]
        for k in range(where.n_clauses):
            if row[k] < 0:
                continue
            bound += 1
            null_test = where.clauses[k].op >= covt.WHERE_IS_NULL
            t = int(plan.props["type"][by_desc[row[k]]])
            bits += n * (1 + (0 if null_test else value_bits.get(t, 0)))
    return bits // 8, int(plan.select["n_features"][live].sum()), bound


def measure(covt, torch, tiles, reps, label):
    plan = covt.Plan.from_tiles(tiles, flags=covt.PLAN_PROPERTIES)
    b = covt.DeviceBatch(plan, "cuda")
    s = torch.cuda.current_stream()
    quarter = covt.SelectPred(window=(0.0, 0.0, 2048.0, 2048.0))
    for step in (b.decode, b.assemble, b.bbox, b.measures, b.materialize_properties):
        step(s)
    torch.cuda.synchronize()
    n_features = int(plan.select["n_features"][plan.select["n_features"] > 0].sum())
    d_a = torch.zeros(max(n_features, 16), dtype=torch.uint8, device=b.device)
    d_b = torch.empty_like(d_a)
    wheres = {name: covt.Where(*clauses) for name, clauses in PREDICATES.items()}
    binds = {name: plan.where_bind(w) for name, w in wheres.items()}
    dev = {}
    for name, w in wheres.items():  # every blob and bind table uploaded once, kept for the run
        dev[name] = (torch.from_numpy(np.frombuffer(w.tobytes(), np.uint8).copy()).to(b.device),
                     torch.from_numpy(binds[name].reshape(-1).copy()).to(b.device))
    b._buffers("select")
    d_status = torch.zeros(max(plan.num_geometry_columns, 1), dtype=torch.int32, device=b.device)

    def run_where(name):
        d_where, d_bind = dev[name]
        st = covt.lib().covt_select_where_device(b.d_pdesc.data_ptr(), b.d_props.data_ptr(), b.d_pres.data_ptr(),
                                                 plan.num_property_columns, b.d_sdesc.data_ptr(),
                                                 plan.num_geometry_columns, d_where.data_ptr(), d_bind.data_ptr(),
                                                 covt.WHERE_WRITE, b.d_select.data_ptr(), d_status.data_ptr(),
                                                 s.cuda_stream)
        assert st == 0, st

    cases = [(name, (lambda name=name: run_where(name))) for name in PREDICATES]
    cases += [("geometric_predicate", lambda: b.select_predicate(quarter, s)), ("mask_copy", lambda: d_b.copy_(d_a))]
    kept = {}
    for name, fn in cases:  # warm-up, and what each predicate keeps
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        if name in PREDICATES:
            buf = b.d_select.cpu().numpy()
            k = 0
            for c in range(plan.num_geometry_columns):
                o, n = int(plan.select["off"][c]), int(plan.select["n_features"][c])
                if n > 0 and not int(plan.select["flags"][c]):
                    k += int(np.count_nonzero(buf[o:o + n]))
            kept[name] = k
    times = {name: [] for name, _ in cases}
    ev = []
    for _ in range(reps):  # alternating, so every pass sees the same clocks and neighbours
        row = []
        for name, fn in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            row.append((name, e0, e1))
        ev.append(row)
    torch.cuda.synchronize()
    for row in ev:
        for name, e0, e1 in row:
            times[name].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in times.items()}
    rec = {"workload": label, "tiles": len(tiles), "columns": int(plan.num_geometry_columns),
           "property_columns": int(plan.num_property_columns), "features": n_features, "reps": reps,
           "geometric_predicate_ms_median": round(med["geometric_predicate"], 4),
           "mask_copy_ms_median": round(med["mask_copy"], 4), "mask_copy_bytes": int(d_a.numel()), "predicates": {}}
    for name in PREDICATES:
        read, written, bound = algorithmic_bytes(covt, plan, wheres[name], binds[name])
        ms = med[name]
        rec["predicates"][name] = {
            "clauses": int(wheres[name].n_clauses), "bound_clause_columns": bound, "ms_median": round(ms, 4),
            "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4), "kept": kept[name],
            "read_bytes": read, "written_bytes": written,
            "over_geometric_predicate": round(ms / med["geometric_predicate"], 3),
            "over_mask_copy": round(ms / med["mask_copy"], 3),
            "tb_per_s": round((read + written) / (ms * 1e-3) / 1e12, 4),
            "share_of_hbm_peak": round((read + written) / (ms * 1e-3) / HBM_PEAK, 4)}
        print("%s, %s: %.4f ms (min %.4f) | geometric predicate %.4f ms | mask copy %.4f ms | kept %d of %d | "
              "%.2f MB read + %.2f MB written" % (label, name, ms, min(times[name]), med["geometric_predicate"],
                                                 med["mask_copy"], kept[name], n_features, read / 1e6, written / 1e6))
    return rec


def main():
    import torch

    args = [a for a in sys.argv[1:]]
    path = None
    if "--json" in args:
        i = args.index("--json")
        path = args[i + 1]
        del args[i:i + 2]
    reps = int(args[0]) if args else 30
    if not torch.cuda.is_available():
        raise SystemExit("where_run.py needs a GPU")
    covt = bench.load_covt()
    lib = bench.tile_library()
    out = {"library": os.environ.get("COVT_LIB_VARIANT", "libcovt.so"), "build": covt.library_build_id(),
           "device": torch.cuda.get_device_name(0), "clocks": clocks(), "runs": []}
    out["runs"].append(measure(covt, torch, [t for _, t in bench.sample_batch(lib, 10000, bench.SEED)], reps,
                               "config 5: 10k-tile batch"))
    print(json.dumps(out))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
