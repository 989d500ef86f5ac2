"""The real (non-dry-run) N-rank bench path on the one-GPU test box: `bench.py --gpus 2 --share-device`
spawns two ranks before anything touches the GPU, both decode their shard of one batch on cuda:0 (gloo
barriers, max-over-ranks timing; then each its own whole batch for the weak figure), and rank 0 prints one line with both ranks' kernel times and the CPU baseline
(north_star: every 1/2/4/8 figure next to the CPU decoder in the same run)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_steps_outputs(gpu_available, covt, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: a plain run (no legs, no CPU baseline) whose
    float64 dump equals an independent decode of the same seeded batch -- every stream's status and consumed
    bytes, and the sampled streams' arrays value for value.  300 tiles decode to more values than the dump
    holds, so the seeded sample is a real subset."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--tiles", "300", "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=110,
                       env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0 and not line["full"]
    assert line["cpu_baseline"] is None and "configs" not in line and "strong_shards" not in line
    names = sorted(f for f in os.listdir(tmp_path))
    assert names == ["consumed.npy", "status.npy", "value_offsets.npy", "value_streams.npy", "values.npy"]
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in names) <= 64 * 1000 * 1000
    d = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in names}
    assert all(a.dtype == np.float64 for a in d.values())

    picks = bench.sample_batch(bench.tile_library(), 300, bench.SEED)
    plan = covt.Plan.from_tiles([t for _, t in picks])
    batch = covt.DeviceBatch(plan, "cuda:0")
    batch.decode()
    out, res = batch.results()
    assert np.array_equal(d["status"], res[:, 0]) and np.array_equal(d["consumed"], res[:, 1])
    pick, voff = d["value_streams"].astype(np.int64), d["value_offsets"].astype(np.int64)
    total = int(plan.streams["out_elems"].sum())
    assert 0 < pick.size < plan.num_streams and voff[-1] == d["values"].size <= bench.DUMP_MAX_VALUES < total
    assert d["values"].size > bench.DUMP_MAX_VALUES // 2  # the sample fills its budget
    assert (np.diff(pick) > 0).all() and len({int(plan.streams["elem_bytes"][i]) for i in pick}) > 1
    for j, i in enumerate(pick):
        assert np.array_equal(d["values"][voff[j]:voff[j + 1]], plan.stream_array(out, int(i)).astype(np.float64)), i


def test_two_ranks_share_device(gpu_available):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-device",
                        "--tiles", "500", "--steps", "3", "--warmup", "1", "--no-props", "--no-assemble",
                        "--no-configs", "--e2e-reps", "0", "--abi-host-reps", "0", "--device-plan-reps", "0",
                        "--cpu-iters", "2", "--full"], capture_output=True, text=True, timeout=110, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["shared_device"] and "dry_run" not in line
    pr = line["per_rank"]
    # strong scaling (the default, BASELINE config 5): the ranks share ONE 500-tile batch by LPT shards
    assert [r["rank"] for r in pr] == [0, 1] and len({r["seed"] for r in pr}) == 1
    assert all(r["kernel_ms"] > 0 for r in pr) and sum(r["tiles"] for r in pr) == 500
    assert line["scaling"] == "strong" and line["config"]["tiles_total"] == 500
    assert line["value"] > 0 and line["roofline"]["frac"] > 0
    w = line["weak"]  # the weak figure beside it: each rank its own 500-tile batch
    assert w["tiles_per_gpu"] == 500 and w["tiles_total"] == 1000 and len(set(w["seeds"])) == 2 and w["value"] > 0
    cb = line["cpu_baseline"]
    assert cb is not None and cb["value"] > 0 and cb["cores"] >= 1
