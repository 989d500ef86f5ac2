#!/usr/bin/env python3
"""The query pass alone, timed with HIP events on the config-5 batch (10k sampled tiles).  Decode, assemble,
bounding boxes and measures once, 3 warm-up launches, then `reps` rounds on the same buffers -- alternating, in
the same run -- of: the query pass (WRITE mode, INTERSECTS) in three shapes (a window over a quarter of each
tile; a point with radius 8 at the tile's centre; a window covering the tile), the measures pass (the same
skeleton over the same coordinates: the yardstick) and the geometric predicate pass with the quarter window.
Medians, what each shape keeps, and the algorithmic bytes of the pass: 8 per coordinate and 4 per ring offset
read and one ring byte written by the rings kernel; per feature two geometry offsets' worth (4), one type byte
and its ring bytes read and one mask byte written by the features kernel (part offsets: 4 per part).
usage: query_run.py [reps] [--json PATH]   (COVT_LIB_VARIANT picks the library)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from wkb_run import HBM_PEAK, clocks  # noqa: E402

SHAPES = {"quarter_tile": (0, 0, 2048, 2048), "point_r8": (2040, 2040, 2056, 2056), "whole_tile": (0, 0, 4096, 4096)}


def algorithmic_bytes(gres, plan):
    """(bytes read, bytes written) of one WRITE-mode pass over the live columns."""
    live = gres["status"] == 0
    coords, rings, parts = (int(gres[k][live].sum()) for k in ("num_coords", "num_rings", "num_parts"))
    feats = int(plan.select["n_features"][live].sum())
    return 8 * coords + 4 * rings + rings + 4 * parts + 5 * feats, rings + feats


def measure(covt, torch, tiles, reps, label):
    plan = covt.Plan.from_tiles(tiles)
    b = covt.DeviceBatch(plan, "cuda")
    s = torch.cuda.current_stream()
    quarter = covt.SelectPred(window=(0.0, 0.0, 2048.0, 2048.0))
    for step in (b.decode, b.assemble, b.bbox, b.measures):
        step(s)
    torch.cuda.synchronize()
    _, gres = b.assembly_results()
    queries = {name: covt.SelectQuery(w) for name, w in SHAPES.items()}
    cases = [(name, (lambda q=q: b.select_query(q, covt.WHERE_WRITE, s))) for name, q in queries.items()]
    cases += [("measures", lambda: b.measures(s)), ("geometric_predicate", lambda: b.select_predicate(quarter, s))]
    n_features = int(plan.select["n_features"][plan.select["n_features"] > 0].sum())
    kept = {}
    for name, fn in cases:  # warm-up, and what each shape keeps
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        if name in SHAPES:
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
    read, written = algorithmic_bytes(gres, plan)
    rec = {"workload": label, "tiles": len(tiles), "columns": int(plan.num_geometry_columns), "features": n_features,
           "coords": int(gres["num_coords"][gres["status"] == 0].sum()),
           "rings": int(gres["num_rings"][gres["status"] == 0].sum()), "reps": reps,
           "measures_ms_median": round(med["measures"], 4), "measures_ms_min": round(min(times["measures"]), 4),
           "geometric_predicate_ms_median": round(med["geometric_predicate"], 4),
           "read_bytes": read, "written_bytes": written, "shapes": {}}
    for name in SHAPES:
        ms = med[name]
        rec["shapes"][name] = {
            "window": list(SHAPES[name]), "ms_median": round(ms, 4), "ms_min": round(min(times[name]), 4),
            "ms_max": round(max(times[name]), 4), "kept": kept[name],
            "over_measures": round(ms / med["measures"], 3),
            "over_geometric_predicate": round(ms / med["geometric_predicate"], 3),
            "tb_per_s": round((read + written) / (ms * 1e-3) / 1e12, 4),
            "share_of_hbm_peak": round((read + written) / (ms * 1e-3) / HBM_PEAK, 4)}
        print("%s, %s: %.4f ms (min %.4f) | measures %.4f ms | geometric predicate %.4f ms | kept %d of %d | "
              "%.2f MB read + %.2f MB written" % (label, name, ms, min(times[name]), med["measures"],
                                                 med["geometric_predicate"], kept[name], n_features, read / 1e6,
                                                 written / 1e6))
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
        raise SystemExit("query_run.py needs a GPU")
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
