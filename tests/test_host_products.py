"""The four whole-plan host entry points (covt_plan_assemble_host, covt_plan_wkb_host, covt_plan_bbox_host,
covt_plan_properties_host) share one pipeline in covt_host.cpp.  What that pipeline must keep for each of
them: the argument checks that return before any device call (CPU), and on the GPU results that repeat
call after call, equal the DeviceBatch path's and leave nothing allocated behind.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

# (Plan method, C entry point, Plan attribute with the product's byte count, ... with its column count)
PRODUCTS = {
    "assemble": ("assemble_host", "covt_plan_assemble_host", "assembly_bytes", "num_geometry_columns"),
    "wkb": ("wkb_host", "covt_plan_wkb_host", "wkb_bytes", "num_geometry_columns"),
    "bbox": ("bbox_host", "covt_plan_bbox_host", "bbox_bytes", "num_geometry_columns"),
    "properties": ("properties_host", "covt_plan_properties_host", "property_bytes", "num_property_columns"),
}
GEOM_FIELDS = ("geometry_offsets", "part_offsets", "ring_offsets", "coords")


def _tile():
    return open(os.path.join(ROOT, "tests", "golden", "tiles", "omt", "5_16_20.covt"), "rb").read()


@pytest.fixture(scope="module")
def plan(covt):
    """The fixture tile planned once, with its property columns."""
    return covt.Plan.from_tiles([_tile()], flags=covt.PLAN_PROPERTIES)


@pytest.mark.parametrize("product", list(PRODUCTS))
def test_host_entry_points_check_their_arguments(covt, plan, product):
    _, entry, nbytes, ncols = PRODUCTS[product]
    fn = getattr(covt.lib(), entry)
    nbytes, ncols = getattr(plan, nbytes), getattr(plan, ncols)
    assert nbytes > 0 and ncols > 0
    tiles = plan.blob.ctypes.data_as(C.POINTER(C.c_uint8))
    n = int(plan.offsets[0] + plan.sizes[0])
    assert n <= plan.blob.size
    out = np.zeros(nbytes, dtype=np.uint8)
    res = np.full(ncols * 64, 0x5A, dtype=np.uint8)  # (larger than any result record)
    assert fn(None, tiles, n, out.ctypes.data, res.ctypes.data) == covt.ERR_INVALID_ARG  # no plan
    assert fn(plan._h, tiles, n - 1, out.ctypes.data, res.ctypes.data) == covt.ERR_INVALID_ARG  # a tile past the buffer
    assert fn(plan._h, tiles, n, None, res.ctypes.data) == covt.ERR_INVALID_ARG  # no output buffer
    assert fn(plan._h, tiles, n, out.ctypes.data, None) == covt.ERR_INVALID_ARG  # no result array
    assert (res == 0x5A).all() and not out.any()  # nothing written on failure


def _same_product(plan, product, a, b):
    """Two (buffer, results) of one product agree on the results and on every byte the product defines;
    returns the number of columns compared."""
    (abuf, ares), (bbuf, bres) = a, b
    assert ares.tobytes() == bres.tobytes(), product
    n_ok = 0
    for c in range(len(ares)):
        if int(ares["status"][c]):
            continue
        n_ok += 1
        if product == "assemble":  # (the padding between a column's arrays is uninitialised)
            x, y = plan.geometry_arrays(abuf, ares, c), plan.geometry_arrays(bbuf, bres, c)
            cols = [(getattr(x, f), getattr(y, f)) for f in GEOM_FIELDS]
        elif product == "wkb":
            x, y = plan.wkb_column(abuf, ares, c), plan.wkb_column(bbuf, bres, c)
            cols = [(x.offsets, y.offsets), (x.data, y.data)]
        elif product == "bbox":
            x, y = plan.bbox_column(abuf, ares, c), plan.bbox_column(bbuf, bres, c)
            cols = [(getattr(x, f), getattr(y, f)) for f in ("xmin", "ymin", "xmax", "ymax")]
        else:
            x, y = plan.property_column(abuf, ares, c), plan.property_column(bbuf, bres, c)
            cols = [(x.validity, y.validity), (x.values, y.values)]
            if x.dict_offsets is not None:
                cols += [(x.dict_offsets, y.dict_offsets), (x.dict_bytes, y.dict_bytes)]
        for u, v in cols:
            assert u.tobytes() == v.tobytes(), (product, c)
    return n_ok


@pytest.mark.gpu
def test_host_products_repeat_and_match_device_batch(covt, plan, gpu_available):
    import torch

    def one_round():
        got = {k: getattr(plan, PRODUCTS[k][0])() for k in PRODUCTS}  # A B C D
        torch.cuda.synchronize()
        return got, covt.scratch_blocks(), torch.cuda.memory_allocated()

    first, blocks1, mem1 = one_round()
    second, blocks2, mem2 = one_round()
    for k in PRODUCTS:
        assert len(first[k][0]) == getattr(plan, PRODUCTS[k][2]) and len(first[k][1]) == getattr(plan, PRODUCTS[k][3])
        assert _same_product(plan, k, first[k], second[k]) > 0, k
    assert (blocks2, mem2) == (blocks1, mem1)  # the second round left nothing more behind than the first
    b = covt.DeviceBatch(plan, "cuda:0")
    b.decode()
    b.assemble()
    b.wkb()
    b.bbox()
    b.materialize_properties()
    torch.cuda.synchronize()
    batch = {"assemble": b.assembly_results(), "wkb": b.wkb_results(), "bbox": b.bbox_results(),
             "properties": b.property_results()}
    for k in PRODUCTS:
        assert _same_product(plan, k, second[k], batch[k]) > 0, k


@pytest.mark.gpu
def test_properties_host_of_a_plan_without_property_columns(covt, gpu_available):
    plan = covt.Plan.from_tiles([_tile()])
    assert plan.num_property_columns == 0 and plan.property_bytes == 0 and plan.num_streams > 0
    buf, pres = plan.properties_host()  # (raises on a status other than OK)
    assert buf.dtype == np.uint8 and buf.size == 0
    assert pres.dtype == covt.PROP_RESULT_DTYPE and pres.size == 0
