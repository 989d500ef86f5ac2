#!/usr/bin/env python3
"""The WKB serialization pass alone, timed with HIP events: the config-5 batch (10k sampled tiles) and
BASELINE config 1's single tile.  Decode and assemble once, warm up, then `reps` WKB launches and -- in the
same run, interleaved -- `reps` assembly launches on the same buffers; medians, the algorithmic bytes of
the WKB pass (read: assembled offsets + types + 8 B per coordinate; written: WKB bytes + offsets), TB/s,
the share of the 8 TB/s HBM peak and the ratio to the assembly time.
usage: wkb_run.py [reps] [--json PATH]   (COVT_LIB_VARIANT picks the library)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s (MI355X)


def clocks():
    """Current shader / memory clocks as the driver reports them (noted with the numbers; nothing is set)."""
    out = {}
    for name in ("pp_dpm_sclk", "pp_dpm_mclk"):
        try:
            with open("/sys/class/drm/card0/device/" + name) as f:
                cur = [ln.strip() for ln in f if ln.strip().endswith("*")]
            out[name] = cur[0] if cur else "unknown"
        except OSError:
            out[name] = "unknown"
    return out


def measure(covt, torch, tiles, reps, label):
    plan = covt.Plan.from_tiles(tiles)
    b = covt.DeviceBatch(plan, "cuda")
    s = torch.cuda.current_stream()
    b.decode(s)
    for _ in range(3):  # warm-up: code objects, the assembly scratch, the buffers
        b.assemble(s)
        b.wkb(s)
    torch.cuda.synchronize()
    buf, wres = b.wkb_results()
    _, gres = b.assembly_results()
    ok = wres["status"] == 0
    w = plan.wkb
    read = int((4 * (w["n_features"][ok].astype(np.int64) + 1 + gres["num_parts"][ok] + 1 + gres["num_rings"][ok] + 1)
                + w["n_features"][ok] + 8 * gres["num_coords"][ok].astype(np.int64)).sum())
    written = int((wres["n_bytes"][ok] + 4 * (w["n_features"][ok].astype(np.int64) + 1)).sum())
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e0, e1, e2 in ev:  # alternating, so both see the same clocks and neighbours
        e0.record(s)
        b.assemble(s)
        e1.record(s)
        b.wkb(s)
        e2.record(s)
    torch.cuda.synchronize()
    t_asm = [a.elapsed_time(c) for a, c, _ in ev]
    t_wkb = [c.elapsed_time(d) for _, c, d in ev]
    ms, ams = float(np.median(t_wkb)), float(np.median(t_asm))
    rec = {"workload": label, "tiles": len(tiles), "columns": int(plan.num_geometry_columns),
           "columns_ok": int(ok.sum()), "features": int(w["n_features"][ok].sum()),
           "coords": int(gres["num_coords"][ok].sum()), "wkb_bytes": int(wres["n_bytes"][ok].sum()),
           "reps": reps, "wkb_ms_median": round(ms, 4), "wkb_ms_min": round(min(t_wkb), 4),
           "wkb_ms_max": round(max(t_wkb), 4), "asm_ms_median": round(ams, 4), "asm_ms_min": round(min(t_asm), 4),
           "wkb_over_asm": round(ms / ams, 3), "read_bytes": read, "written_bytes": written,
           "tb_per_s": round((read + written) / (ms * 1e-3) / 1e12, 4),
           "share_of_hbm_peak": round((read + written) / (ms * 1e-3) / HBM_PEAK, 4)}
    print("%s: wkb %.4f ms (min %.4f) | assembly %.4f ms | ratio %.2f | %.1f MB read + %.1f MB written = %.3f TB/s, "
          "%.1f %% of 8 TB/s" % (label, ms, min(t_wkb), ams, ms / ams, read / 1e6, written / 1e6, rec["tb_per_s"],
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
        raise SystemExit("wkb_run.py needs a GPU")
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
