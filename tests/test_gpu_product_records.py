"""The per-column products of a device plan (covt_device_plan_geometry; cov-tiles_amd/csrc/covt_products.h) against
the host plan's: records, descriptors and totals byte for byte, for every listed product, and unchanged by a
second geometry() call.  Only the plan kernels run; no pass does."""
import os

import numpy as np
import pytest

from conftest import ROOT, tile_paths
from oracle import gend as W

pytestmark = pytest.mark.gpu

KINDS = ("wkb", "bbox", "measures", "select", "simplify", "mvt")
BATCHES = ("id_only", "one_tile", "twelve_tiles")


def _tiles(covt, batch):
    if batch == "id_only":  # one layer with an id column and no geometry column: no column at all, one arena row
        ids = np.arange(40, dtype=np.uint64) * 3
        return [W.tile([W.layer("ids", 4096, len(ids), [W.id_column(ids)])])], covt.FORMAT_GEND
    if batch == "one_tile":
        return [open(os.path.join(ROOT, "tests", "golden", "tiles", "omt", "5_16_20.covt"), "rb").read()], covt.FORMAT_GENC
    paths = tile_paths()
    return [open(p, "rb").read() for p in paths[::len(paths) // 12][:12]], covt.FORMAT_GENC


@pytest.fixture(scope="module")
def built(covt, gpu_available):
    """batch -> (host plan, device plan with its geometry part built), made once for the six products."""
    import torch

    out = {}
    for batch in BATCHES:
        tiles, fmt = _tiles(covt, batch)
        hp = covt.Plan.from_tiles(tiles, fmt)
        dp = covt.DevicePlan(torch.from_numpy(hp.blob).cuda(), hp.offsets.astype(np.int64), hp.sizes.astype(np.int64),
                             fmt, options=hp.options)
        dp.geometry()
        out[batch] = (hp, dp)
    yield out
    for hp, dp in out.values():
        dp.close()
        hp.close()


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_device_records_are_the_host_plans(covt, built, kind, batch):
    hp, dp = built[batch]
    q = covt._PRODUCTS[kind]
    assert np.array_equal(dp.host_copy()[2], hp.tile_status)
    n = hp.num_geometry_columns
    assert dp.num_geometry_columns == n
    if batch == "id_only":
        assert n == 0
    elif batch == "one_tile":
        assert n > 1 and int(hp.tile_status[0]) == 0
    else:
        assert hp.n_tiles == 12 and n > 24
    copy = getattr(dp, kind + "_copy")
    info, descs = copy()
    nbytes = getattr(dp, q.nbytes)
    assert info.tobytes() == getattr(hp, q.records).tobytes()
    assert descs.tobytes() == getattr(hp, q.descs).tobytes()
    assert nbytes == getattr(hp, q.nbytes) and (nbytes > 0) == (n > 0)
    # built once: a second call changes nothing
    assert dp.geometry() == n
    info2, descs2 = copy()
    assert info2.tobytes() == info.tobytes() and descs2.tobytes() == descs.tobytes() and getattr(dp, q.nbytes) == nbytes
