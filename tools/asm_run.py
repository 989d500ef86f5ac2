#!/usr/bin/env python3
"""Geometry assembly alone, timed with HIP events (a profiling / A-B target): the config-5 batch (10k
sampled tiles: one wave per column) and BASELINE config 1's single tile (the split passes).  Decode once,
3 warm-up launches, then `reps` assembly launches; medians, and one JSON line.
usage: asm_run.py [reps] [--json PATH]   (COVT_LIB_VARIANT picks the library)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from wkb_run import clocks  # noqa: E402


def measure(covt, torch, tiles, reps, label):
    plan = covt.Plan.from_tiles(tiles)
    b = covt.DeviceBatch(plan, "cuda")
    s = torch.cuda.current_stream()
    b.decode(s)
    for _ in range(3):  # warm-up: code objects, the assembly scratch, the buffers
        b.assemble(s)
    torch.cuda.synchronize()
    _, gres = b.assembly_results()
    ok = gres["status"] == 0
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record(s)
        b.assemble(s)
        e1.record(s)
    torch.cuda.synchronize()
    t = [a.elapsed_time(c) for a, c in ev]
    rec = {"workload": label, "tiles": len(tiles), "columns": int(plan.num_geometry_columns),
           "columns_ok": int(ok.sum()), "coords": int(gres["num_coords"][ok].astype(np.int64).sum()), "reps": reps,
           "asm_ms_median": round(float(np.median(t)), 4), "asm_ms_min": round(min(t), 4),
           "asm_ms_max": round(max(t), 4)}
    print("%s: assembly %.4f ms (min %.4f, max %.4f) over %d columns" % (label, rec["asm_ms_median"], rec["asm_ms_min"],
                                                                        rec["asm_ms_max"], rec["columns"]))
    return rec


def main():
    import torch

    args = [a for a in sys.argv[1:]]
    path = None
    if "--json" in args:
        i = args.index("--json")
        path = args[i + 1]
        del args[i:i + 2]
    reps = int(args[0]) if args else 20
    if not torch.cuda.is_available():
        raise SystemExit("asm_run.py needs a GPU")
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
