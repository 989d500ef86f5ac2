#!/usr/bin/env python3
"""The measures pass alone, timed with HIP events: the config-5 batch (10k sampled tiles) and BASELINE config
1's single tile.  Decode and assemble once, 3 warm-up launches, then `reps` rounds of assembly, bounding-box
and measures launches on the same buffers -- alternating, in the same run; medians, the algorithmic bytes of
the measures pass (read: the three offset levels, a type byte per feature and 8 B per coordinate, and the
ring scratch back; written: 20 B per feature, 16 B per ring of scratch, 8 B per column), TB/s, the share of
the 8 TB/s HBM peak and the ratio to the bounding-box pass, which streams the same coordinates once.
usage: measures_run.py [reps] [--json PATH]   (COVT_LIB_VARIANT picks the library)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from wkb_run import HBM_PEAK, clocks  # noqa: E402


def measure(covt, torch, tiles, reps, label):
    plan = covt.Plan.from_tiles(tiles)
    b = covt.DeviceBatch(plan, "cuda")
    s = torch.cuda.current_stream()
    b.decode(s)
    for _ in range(3):  # warm-up: code objects, the assembly scratch, the buffers
        b.assemble(s)
        b.bbox(s)
        b.measures(s)
    torch.cuda.synchronize()
    _, mres = b.measures_results()
    _, gres = b.assembly_results()
    ok = mres["status"] == 0
    n = plan.measures["n_features"][ok].astype(np.int64)
    rings = gres["num_rings"][ok].astype(np.int64)
    read = int((4 * (n + 1 + gres["num_parts"][ok] + 1 + rings + 1) + n
                + 8 * gres["num_coords"][ok].astype(np.int64) + 16 * rings).sum())
    written = int((20 * n + 16 * rings).sum() + 8 * int(ok.sum()))
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
    for e0, e1, e2, e3 in ev:  # alternating, so all three see the same clocks and neighbours
        e0.record(s)
        b.assemble(s)
        e1.record(s)
        b.bbox(s)
        e2.record(s)
        b.measures(s)
        e3.record(s)
    torch.cuda.synchronize()
    t_asm = [e[0].elapsed_time(e[1]) for e in ev]
    t_box = [e[1].elapsed_time(e[2]) for e in ev]
    t_ms = [e[2].elapsed_time(e[3]) for e in ev]
    ms, bms, ams = float(np.median(t_ms)), float(np.median(t_box)), float(np.median(t_asm))
    rec = {"workload": label, "tiles": len(tiles), "columns": int(plan.num_geometry_columns),
           "columns_ok": int(ok.sum()), "features": int(n.sum()), "rings": int(rings.sum()),
           "coords": int(gres["num_coords"][ok].sum()), "reps": reps, "measures_ms_median": round(ms, 4),
           "measures_ms_min": round(min(t_ms), 4), "measures_ms_max": round(max(t_ms), 4),
           "bbox_ms_median": round(bms, 4), "asm_ms_median": round(ams, 4), "measures_over_bbox": round(ms / bms, 3),
           "measures_over_asm": round(ms / ams, 3), "read_bytes": read, "written_bytes": written,
           "tb_per_s": round((read + written) / (ms * 1e-3) / 1e12, 4),
           "share_of_hbm_peak": round((read + written) / (ms * 1e-3) / HBM_PEAK, 4)}
    print("%s: measures %.4f ms (min %.4f) | bbox %.4f ms | assembly %.4f ms | %.1f MB read + %.1f MB written = %.3f TB/s, "
          "%.1f %% of 8 TB/s" % (label, ms, min(t_ms), bms, ams, read / 1e6, written / 1e6, rec["tb_per_s"],
                                 100 * rec["share_of_hbm_peak"]))
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
        raise SystemExit("measures_run.py needs a GPU")
    covt = bench.load_covt()
    lib = bench.tile_library()
    out = {"library": os.environ.get("COVT_LIB_VARIANT", "libcovt.so"), "build": covt.library_build_id(),
           "device": torch.cuda.get_device_name(0), "clocks": clocks(), "runs": []}
    out["runs"].append(measure(covt, torch, [t for _, t in bench.sample_batch(lib, 10000, bench.SEED)], reps,
                               "config 5: 10k-tile batch"))
    out["runs"].append(measure(covt, torch, [bench.config1_tile(lib)], reps, "config 1: one z5 tile"))
    print(json.dumps(out))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
