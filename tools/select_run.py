#!/usr/bin/env python3
"""The select passes alone, timed with HIP events: the config-5 batch (10k sampled tiles) and BASELINE config
1's single tile.  Decode, assemble, WKB, bounding boxes and measures once, 3 warm-up launches, then `reps`
rounds on the same buffers -- alternating, in the same run -- of: the WKB write pass, a device-to-device copy
of the WKB buffer (the ceiling for keep-all), predicate + select at keep-all, at keep-alternate (a
caller-written mask, so the predicate is not in that figure) and with a window over a quarter of each tile.
Medians, and the algorithmic bytes of each selection: read the mask, the WKB offsets, 12 B per kept value for the
copy's windows and the kept bytes; written sel, offsets and the kept bytes (the predicate's own reads, 8 B of xmin per feature or 32 B with a window, are
listed beside them).  The yardsticks are the copy and the WKB pass of the same run.
usage: select_run.py [reps] [--json PATH]   (COVT_LIB_VARIANT picks the library)"""
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
    keep_all = covt.SelectPred(keep_empty=True)
    quarter = covt.SelectPred(window=(0.0, 0.0, 2048.0, 2048.0))
    for step in (b.decode, b.assemble, b.wkb, b.bbox, b.measures):
        step(s)
    torch.cuda.synchronize()
    nc = plan.num_geometry_columns
    # (the results only: the buffers stay on the device)
    wres = b.d_wres.cpu().numpy().view(covt.WKB_RESULT_DTYPE)[:nc][plan.wkb["desc_index"]]
    ok = wres["status"] == 0
    n = plan.select["n_features"][ok].astype(np.int64)
    wkb_bytes = int(wres["n_bytes"][ok].sum())
    d_copy = torch.empty_like(b.d_wkb)
    # the alternate mask of every column, uploaded once: feature f of a column is kept when f is odd
    alt = np.zeros(max(plan.select_bytes, 16), np.uint8)
    for c in range(plan.num_geometry_columns):
        o, k = int(plan.select["off"][c]), int(plan.select["n_features"][c])
        alt[o:o + k] = np.arange(k) & 1
    d_alt = torch.from_numpy(alt).to(b.device)

    def put_alt():  # the masks only: one strided copy would do, a full-buffer copy outside the timed span does too
        b.d_select.copy_(d_alt)

    def run_wkb():
        b.wkb(s)

    def run_copy():
        d_copy.copy_(b.d_wkb)

    def run_all():
        b.select_predicate(keep_all, s)
        b.select(s)

    def run_quarter():
        b.select_predicate(quarter, s)
        b.select(s)

    def run_alt():
        b.select(s)

    cases = [("wkb", run_wkb, None), ("copy", run_copy, None), ("keep_all", run_all, None),
             ("keep_alternate", run_alt, put_alt), ("window_quarter", run_quarter, None)]
    kept = {}
    for name, fn, prep in cases:  # warm-up, and what each selection keeps
        for _ in range(3):
            if prep:
                prep()
            fn()
        torch.cuda.synchronize()
        if name not in ("wkb", "copy"):
            sres = b.d_sres.cpu().numpy().view(covt.SELECT_RESULT_DTYPE)[:nc]
            good = sres["status"] == 0
            kept[name] = (int(sres["n_selected"][good].sum()), int(sres["n_bytes"][good].sum()))
    times = {name: [] for name, _, _ in cases}
    ev = []
    for _ in range(reps):  # alternating, so every pass sees the same clocks and neighbours
        row = []
        for name, fn, prep in cases:
            if prep:
                prep()
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
           "columns_ok": int(ok.sum()), "features": int(n.sum()), "wkb_bytes": wkb_bytes, "reps": reps,
           "wkb_ms_median": round(med["wkb"], 4), "copy_ms_median": round(med["copy"], 4),
           "wkb_buffer_bytes": int(b.d_wkb.numel()),  # (what the copy moves: offsets, values and the slices' slack)
           "copy_tb_per_s": round(2 * int(b.d_wkb.numel()) / (med["copy"] * 1e-3) / 1e12, 4), "selections": {}}
    for name in ("keep_all", "keep_alternate", "window_quarter"):
        n_sel, n_bytes = kept[name]
        # the scan reads the mask and the WKB offsets; the copy sel, offsets and wkb_offsets[sel] (12 B per kept
        # value, staged once per window) and the kept bytes
        read = int(n.sum()) + 4 * int((n + 1).sum()) + 12 * n_sel + n_bytes
        written = 4 * n_sel + 4 * (n_sel + int(ok.sum())) + n_bytes + 16 * int(ok.sum())
        pred_read = 0 if name == "keep_alternate" else (32 if name == "window_quarter" else 8) * int(n.sum())
        ms = med[name]
        rec["selections"][name] = {
            "ms_median": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
            "n_selected": n_sel, "kept_bytes": n_bytes, "read_bytes": read, "written_bytes": written,
            "predicate_read_bytes": pred_read, "predicate_written_bytes": 0 if name == "keep_alternate" else int(n.sum()),
            "over_copy": round(ms / med["copy"], 3), "over_wkb": round(ms / med["wkb"], 3),
            "tb_per_s": round((read + written) / (ms * 1e-3) / 1e12, 4),
            "share_of_hbm_peak": round((read + written) / (ms * 1e-3) / HBM_PEAK, 4)}
        print("%s, %s: %.4f ms (min %.4f) | copy %.4f ms | wkb %.4f ms | kept %d of %d features, %.1f of %.1f MB | "
              "%.1f MB read + %.1f MB written" % (label, name, ms, min(times[name]), med["copy"], med["wkb"], n_sel,
                                                 int(n.sum()), n_bytes / 1e6, wkb_bytes / 1e6, read / 1e6, written / 1e6))
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
        raise SystemExit("select_run.py needs a GPU")
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
