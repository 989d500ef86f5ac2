#!/usr/bin/env python3
"""The plain and the georeferenced WKB and bounding-box passes, timed with HIP events in one process on the
benchmark's batch (10k sampled tiles, built as bench.py builds it; tile addresses from the fixture names).

Decode and assemble once, warm every variant up, then `reps` rounds; each round launches every variant once,
in an order rotated from round to round, so all of them see the same clocks and neighbours:

  WKB:  plain | Web Mercator | CRS84 | (the yardstick library's plain pass)
  bbox: plain | Web Mercator | CRS84 | (the yardstick library's plain pass)

The yardstick is another build of libcovt (--yardstick PATH, e.g. the parent commit's library), loaded next
to this one and launched on the same device buffers: its plain passes are what "did the plain entry points get
slower" is measured against, not this build's identity instantiation.  The spread reported with every median
is the run-to-run spread of this session: the medians of the rounds' first and second half, and p10 / p90.

usage: geo_prof.py [reps] [--tiles N] [--yardstick PATH] [--json PATH]
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def zxy_of_key(key):
    z, x, y = (int(v) for v in key.split("/")[-1].replace("-", "_").split("_"))
    return z, x, y


def stats(t):
    t = np.asarray(t, dtype=np.float64)
    h = t.size // 2
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4),
            "p10_ms": round(float(np.percentile(t, 10)), 4), "p90_ms": round(float(np.percentile(t, 90)), 4),
            "first_half_median_ms": round(float(np.median(t[:h])), 4),
            "second_half_median_ms": round(float(np.median(t[h:])), 4)}


def main():
    import torch

    args = list(sys.argv[1:])

    def opt(name, default=None):
        if name in args:
            i = args.index(name)
            v = args[i + 1]
            del args[i:i + 2]
            return v
        return default

    path, yard_path, n_tiles = opt("--json"), opt("--yardstick"), int(opt("--tiles", "10000"))
    reps = int(args[0]) if args else 30
    if not torch.cuda.is_available():
        raise SystemExit("geo_prof.py needs a GPU")
    covt = bench.load_covt()
    L = covt.lib()
    picks = bench.sample_batch(bench.tile_library(), n_tiles, bench.SEED)
    zxy = [zxy_of_key(k) for k, _ in picks]
    plan = covt.Plan.from_tiles([t for _, t in picks])
    b = covt.DeviceBatch(plan, "cuda")
    s = torch.cuda.current_stream()
    b.decode(s)
    b.assemble(s)
    merc, lonlat = plan.geo_transforms(covt.CRS_WEB_MERCATOR, zxy), plan.geo_transforms(covt.CRS_CRS84, zxy)
    b.wkb(s)
    b.bbox(s)  # (the buffers exist)
    up = lambda t: torch.from_numpy(t.view(np.uint8).reshape(-1).copy()).to(b.device)  # noqa: E731
    d_merc, d_lonlat = up(merc[0]), up(lonlat[0])
    n, hs = plan.num_geometry_columns, s.cuda_stream
    wargs = (b.d_out.data_ptr(), b.d_gdesc.data_ptr(), b.d_asm.data_ptr(), b.d_gres.data_ptr(), b.d_wdesc.data_ptr(), n,
             b.d_wkb.data_ptr(), b.d_wres.data_ptr())
    bargs = (b.d_gdesc.data_ptr(), b.d_asm.data_ptr(), b.d_gres.data_ptr(), b.d_bdesc.data_ptr(), n,
             b.d_bbox.data_ptr(), b.d_bres.data_ptr())
    variants = {
        "wkb_plain": lambda: L.covt_geometry_wkb_device(*wargs, hs),
        "wkb_web_mercator": lambda: L.covt_geometry_wkb_projected_device(*wargs, d_merc.data_ptr(), merc[1], hs),
        "wkb_crs84": lambda: L.covt_geometry_wkb_projected_device(*wargs, d_lonlat.data_ptr(), lonlat[1], hs),
        "bbox_plain": lambda: L.covt_geometry_bbox_device(*bargs, hs),
        "bbox_web_mercator": lambda: L.covt_geometry_bbox_projected_device(*bargs, d_merc.data_ptr(), merc[1], hs),
        "bbox_crs84": lambda: L.covt_geometry_bbox_projected_device(*bargs, d_lonlat.data_ptr(), lonlat[1], hs),
    }
    if yard_path:
        Y = C.CDLL(os.path.abspath(yard_path))
        for name, proto in (("covt_geometry_wkb_device", "covt_geometry_wkb_device"),
                            ("covt_geometry_bbox_device", "covt_geometry_bbox_device")):
            fn = getattr(Y, name)
            fn.restype, fn.argtypes = covt._SIGNATURES[proto]
        variants["wkb_plain_yardstick"] = lambda: Y.covt_geometry_wkb_device(*wargs, hs)
        variants["bbox_plain_yardstick"] = lambda: Y.covt_geometry_bbox_device(*bargs, hs)
    names = list(variants)
    for _ in range(3):  # warm-up: code objects of every variant
        for k in names:
            assert variants[k]() == 0, k
    torch.cuda.synchronize()
    times = {k: [] for k in names}
    ev = []
    for r in range(reps):
        order = names[r % len(names):] + names[:r % len(names)]
        for k in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            assert variants[k]() == 0, k
            e1.record(s)
            ev.append((k, e0, e1))
    torch.cuda.synchronize()
    for k, e0, e1 in ev:
        times[k].append(e0.elapsed_time(e1))
    _, gres = b.assembly_results()
    _, wres = b.wkb_results()
    ok = wres["status"] == 0
    out = {"library": os.environ.get("COVT_LIB_VARIANT", "libcovt.so"), "build": covt.library_build_id(),
           "yardstick": yard_path, "device": torch.cuda.get_device_name(0), "tiles": len(picks), "columns": int(n),
           "coords": int(gres["num_coords"][ok].sum()), "wkb_bytes": int(wres["n_bytes"][ok].sum()), "reps": reps,
           "kinds": {"web_mercator": merc[1], "crs84": lonlat[1]}, "runs": {k: stats(times[k]) for k in names}}
    for k in names:
        st = out["runs"][k]
        print("%-22s median %.4f ms  min %.4f  p10 %.4f  p90 %.4f  halves %.4f / %.4f"
              % (k, st["median_ms"], st["min_ms"], st["p10_ms"], st["p90_ms"], st["first_half_median_ms"],
                 st["second_half_median_ms"]))
    print(json.dumps(out))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
