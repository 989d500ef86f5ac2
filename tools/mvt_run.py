#!/usr/bin/env python3
"""The MVT encoding pass alone, timed with HIP events, beside the WKB pass on the same column in the same run: the
config-5 batch (10k sampled tiles).  Decode and assemble once, warm up, then `reps` rounds of WKB, mvt (orientation
off) and mvt (orientation on) launches on the same buffers, interleaved; medians and the output bytes per
coordinate of both.  (The WKB pass is the one this pass is held against; its kernels are the same from one build to
the next unless covt_wkb.hip changes, so both are timed in one run, with the same clocks and neighbours.)
usage: mvt_run.py [reps] [--json PATH]   (COVT_LIB_VARIANT picks the library)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def measure(covt, torch, tiles, reps, label):
    plan = covt.Plan.from_tiles(tiles)
    b = covt.DeviceBatch(plan, "cuda")
    s = torch.cuda.current_stream()
    plain, orient = covt.MvtOptions(), covt.MvtOptions(orient=True)
    b.decode(s)
    for _ in range(3):  # warm-up: code objects, the assembly scratch, the buffers
        b.assemble(s)
        b.wkb(s)
        b.mvt(plain, s)
        b.mvt(orient, s)
    torch.cuda.synchronize()
    _, wres = b.wkb_results()
    _, mres = b.mvt_results()
    _, gres = b.assembly_results()
    ok = mres["status"] == 0
    coords = int(gres["num_coords"][ok].astype(np.int64).sum())
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
    for e in ev:  # alternating, so all three see the same clocks and neighbours
        e[0].record(s)
        b.wkb(s)
        e[1].record(s)
        b.mvt(plain, s)
        e[2].record(s)
        b.mvt(orient, s)
        e[3].record(s)
    torch.cuda.synchronize()
    t = [[e[k].elapsed_time(e[k + 1]) for e in ev] for k in range(3)]
    med = [float(np.median(x)) for x in t]
    rec = {"workload": label, "tiles": len(tiles), "columns": int(plan.num_geometry_columns), "columns_ok": int(ok.sum()),
           "features": int(plan.mvt["n_features"][ok].sum()), "rings": int(gres["num_rings"][ok].astype(np.int64).sum()),
           "coords": coords, "reps": reps, "wkb_bytes": int(wres["n_bytes"][wres["status"] == 0].sum()),
           "mvt_bytes": int(mres["n_bytes"][ok].sum()), "mvt_empty_features": int(mres["n_empty"][ok].sum()),
           "wkb_bytes_per_coord": round(int(wres["n_bytes"][wres["status"] == 0].sum()) / max(coords, 1), 3),
           "mvt_bytes_per_coord": round(int(mres["n_bytes"][ok].sum()) / max(coords, 1), 3)}
    for name, x, m in zip(("wkb", "mvt", "mvt_orient"), t, med):
        rec[name + "_ms_median"], rec[name + "_ms_min"], rec[name + "_ms_max"] = round(m, 4), round(min(x), 4), round(max(x), 4)
    rec["mvt_over_wkb"] = round(med[1] / med[0], 3)
    print("%s: wkb %.4f ms | mvt %.4f ms | mvt oriented %.4f ms | %.2f / %.2f output bytes a coordinate (wkb / mvt)"
          % (label, med[0], med[1], med[2], rec["wkb_bytes_per_coord"], rec["mvt_bytes_per_coord"]))
    return rec


def main():
    import torch

    args = list(sys.argv[1:])
    path = None
    if "--json" in args:
        i = args.index("--json")
        path = args[i + 1]
        del args[i:i + 2]
    reps = int(args[0]) if args else 20
    if not torch.cuda.is_available():
        raise SystemExit("mvt_run.py needs a GPU")
    covt = bench.load_covt()
    lib = bench.tile_library()
    out = {"library": os.environ.get("COVT_LIB_VARIANT", "libcovt.so"), "build": covt.library_build_id(),
           "device": torch.cuda.get_device_name(0), "runs": []}
    out["runs"].append(measure(covt, torch, [t for _, t in bench.sample_batch(lib, 10000, bench.SEED)], reps,
                               "config 5: 10k-tile batch"))
    print(json.dumps(out))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
