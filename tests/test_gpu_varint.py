"""The varint engine (covt_decode.hip win_load / win_value / varint_take / sink_values / sink_u64) against the plain
reference of tests/covt_varint.py, on the corpus that module builds around the kernel's own step sizes: the eleven
varint ops one wave per stream, and the VariableByte tail of both FastPFOR kernels.  tests/test_varint_ref.py
proves on the CPU that the reference is the oracle's and that the corpus reaches what it aims at.

Every descriptor of a family goes into one launch; output slots are 128-byte aligned as a plan lays them out,
in shuffled order in a buffer pre-filled with 0x5A with a guard before and after.  Every row is checked: the
status and consumed bytes exactly (consumed is 0 for a failed stream, include/covt.h), the values of OK rows byte
for byte, and no byte outside the descriptors' own slots may change, failed streams included."""
import ctypes as C

import numpy as np
import pytest

import covt_varint as CV
from test_gpu_split import DESC
from test_varint_ref import corpus

pytestmark = pytest.mark.gpu

GUARD = 256  # bytes of 0x5A before the first and after the last output slot
_CACHE = {}


def _layout(c, idx, order):
    """Descriptors of rows `idx` in launch order ("corpus", or "largest" first as a plan orders a family) and their
    output slots in an order of their own.  -> (DESC array, row per descriptor, slot offsets, slot sizes, bytes)."""
    key = (tuple(idx[:3]), len(idx), order)
    if key in _CACHE:
        return _CACHE[key]
    idx = np.asarray(idx)
    rows = c.rows
    if order == "largest":
        cost = np.array([max(rows[i]["avail"], 0) + max(rows[i]["n"], 0) * c.ref.elem[rows[i]["op"]] // 4 for i in idx])
        idx = idx[np.argsort(-cost, kind="stable")]
    size = np.array([max(CV.align(max(rows[i]["n"], 0) * c.ref.elem[rows[i]["op"]], 128), 128) for i in idx],
                    dtype=np.int64)
    pos = np.random.default_rng(len(idx)).permutation(idx.size)
    off = np.zeros(idx.size, dtype=np.int64)
    off[pos] = GUARD + np.concatenate(([0], np.cumsum(size[pos])[:-1]))
    d = np.zeros(idx.size, dtype=DESC)
    for k, i in enumerate(idx):
        r = rows[i]
        d[k] = (r["in_off"], off[k], r["avail"], r["n"], r["op"], r["nb"], 0, r["bl"])
    _CACHE[key] = (d, idx, off, size, GUARD + int(size.sum()) + GUARD)
    return _CACHE[key]


def _device_input(covt, c):
    import torch

    if "d_in" not in _CACHE:
        dev = torch.device("cuda")
        d_in = torch.full((len(c.blob) + covt.INPUT_PADDING + 16,), CV.FILL, dtype=torch.uint8, device=dev)
        d_in[:len(c.blob)] = torch.frombuffer(bytearray(c.blob), dtype=torch.uint8).to(dev)
        assert d_in.data_ptr() % 256 == 0  # the corpus places streams by address residue
        _CACHE["d_in"] = d_in
    return _CACHE["d_in"]


def _buffers(d, total, dev):
    import torch

    d_desc = torch.from_numpy(d.view(np.uint8).copy()).to(dev)
    d_out = torch.full((total,), 0x5A, dtype=torch.uint8, device=dev)
    d_res = torch.full((d.size * 2,), 0x33, dtype=torch.int32, device=dev)
    assert d_out.data_ptr() % 128 == 0
    return d_desc, d_out, d_res


def _enqueue(covt, d_in, d_desc, n, family, d_out, d_res, stream, launch):
    """launch None: covt_decode_streams_device, the ungrouped entry."""
    if launch is None:
        st = covt.lib().covt_decode_streams_device(d_in.data_ptr(), d_desc.data_ptr(), n, d_out.data_ptr(),
                                                   d_res.data_ptr(), stream)
    else:
        counts = np.zeros(covt.NUM_FAMILIES, dtype=np.int64)
        counts[family] = n
        st = covt.lib().covt_decode_streams_device_grouped_mode(
            d_in.data_ptr(), d_desc.data_ptr(), counts.ctypes.data_as(C.POINTER(C.c_int64)), d_out.data_ptr(),
            d_res.data_ptr(), stream, launch)
    assert st == 0


def _run(covt, c, idx, family, launch, order="corpus"):
    """One launch of rows idx -> (layout, output bytes, result rows); kept, so tests that compare launches share."""
    import torch

    key = ("run", family, launch, order)
    if key not in _CACHE:
        d_in = _device_input(covt, c)
        lay = _layout(c, idx, order)
        d, _, _, _, total = lay
        d_desc, d_out, d_res = _buffers(d, total, d_in.device)
        _enqueue(covt, d_in, d_desc, d.size, family, d_out, d_res, torch.cuda.current_stream().cuda_stream, launch)
        torch.cuda.synchronize()
        _CACHE[key] = (lay, d_out.cpu().numpy(), d_res.cpu().numpy().reshape(-1, 2))
    return _CACHE[key]


def _check(c, exp, lay, out, res, what):
    """Every descriptor against the reference; -> (descriptors checked, streams whose values were compared)."""
    _, order, off, size, total = lay
    assert out.size == total and res.shape[0] == order.size
    bad = []
    n_checked = n_values = 0
    free = np.ones(out.size, dtype=bool)
    for k, i in enumerate(order):
        r, (st, vals, cons) = c.rows[i], exp[i]
        free[off[k]:off[k] + size[k]] = False
        tag = (what, r["group"], r["note"], int(i), r["op"], r["n"], r["avail"], r["in_off"] & 15)
        if int(res[k, 0]) != st:
            bad.append(("status", tag, int(res[k, 0]), st))
        elif int(res[k, 1]) != cons:
            bad.append(("consumed", tag, int(res[k, 1]), cons))
        elif st == 0:
            got = out[off[k]:off[k] + vals.nbytes]
            if got.tobytes() != vals.tobytes():
                first = int(np.nonzero(got != np.frombuffer(vals.tobytes(), np.uint8))[0][0])
                bad.append(("values", tag, "first differing output byte %d" % first))
            n_values += 1
        n_checked += 1
    kinds = sorted({(b[0], b[1][1], b[1][4]) + tuple(b[2:]) for b in bad if b[0] != "values"} |
                   {(b[0], b[1][1], b[1][4]) for b in bad if b[0] == "values"})
    assert not bad, (len(bad), kinds[:40], bad[:8])
    stray = np.nonzero(free & (out != 0x5A))[0]
    assert stray.size == 0, (what, "bytes outside every slot were written", stray[:8].tolist())
    return n_checked, n_values


def _same_rows(c, exp, a, b):
    """Two launches of the same rows in whatever orders: identical (status, consumed) rows and value bytes."""
    (la, out_a, res_a), (lb, out_b, res_b) = a, b
    at = {int(i): k for k, i in enumerate(la[1])}
    assert len(at) == lb[1].size
    for kb, i in enumerate(lb[1]):
        ka = at[int(i)]
        assert np.array_equal(res_a[ka], res_b[kb]), (int(i), res_a[ka], res_b[kb])
        if exp[i][0] == 0:
            nb = exp[i][1].nbytes
            assert np.array_equal(out_a[la[2][ka]:la[2][ka] + nb], out_b[lb[2][kb]:lb[2][kb] + nb]), int(i)


VARINT_LAUNCHES = {"fused": 1, "forked": 2, "ungrouped": None}      # COVT_LAUNCH_FUSED / _FORKED
FPF_LAUNCHES = {"stream": 2 | 4, "classic": 2 | 8, "fused": 1}      # FORKED | FPF_STREAM / FPF_CLASSIC


@pytest.mark.parametrize("launch", list(VARINT_LAUNCHES))
def test_varint_corpus(covt, oracle, gpu_available, launch):
    c, exp = corpus(covt, oracle)
    assert (covt.LAUNCH_FUSED, covt.LAUNCH_FORKED) == (1, 2)
    idx = c.varint_rows()
    lay, out, res = _run(covt, c, idx, covt.FAMILY_VARINT, VARINT_LAUNCHES[launch])
    n_ok = sum(1 for i in idx if exp[i][0] == 0)
    assert _check(c, exp, lay, out, res, launch) == (len(idx), n_ok)  # no descriptor is left unchecked


@pytest.mark.parametrize("launch", list(FPF_LAUNCHES))
def test_fastpfor_corpus(covt, oracle, gpu_available, launch):
    c, exp = corpus(covt, oracle)
    assert (covt.LAUNCH_FPF_STREAM, covt.LAUNCH_FPF_CLASSIC) == (4, 8)
    idx = c.fpf_rows()
    lay, out, res = _run(covt, c, idx, covt.FAMILY_FASTPFOR, FPF_LAUNCHES[launch])
    n_ok = sum(1 for i in idx if exp[i][0] == 0)
    assert _check(c, exp, lay, out, res, launch) == (len(idx), n_ok)


def test_fastpfor_kernels_agree(covt, oracle, gpu_available):
    """The streamed and the per-block FastPFOR kernel: the same rows and the same value bytes."""
    c, exp = corpus(covt, oracle)
    runs = [_run(covt, c, c.fpf_rows(), covt.FAMILY_FASTPFOR, FPF_LAUNCHES[k]) for k in ("stream", "classic")]
    assert np.array_equal(runs[0][2], runs[1][2])
    _same_rows(c, exp, runs[0], runs[1])


@pytest.mark.parametrize("family", ["varint", "fastpfor"])
def test_launch_order(covt, oracle, gpu_available, family):
    """Descriptors largest first, as a plan orders a family, and in corpus order: identical rows."""
    c, exp = corpus(covt, oracle)
    idx, fam, launch = ((c.varint_rows(), covt.FAMILY_VARINT, 2) if family == "varint" else
                        (c.fpf_rows(), covt.FAMILY_FASTPFOR, 2 | 4))
    a = _run(covt, c, idx, fam, launch)
    b = _run(covt, c, idx, fam, launch, order="largest")
    assert not np.array_equal(a[0][1], b[0][1])
    n_ok = sum(1 for i in idx if exp[i][0] == 0)
    assert _check(c, exp, b[0], b[1], b[2], family + " largest first") == (len(idx), n_ok)
    _same_rows(c, exp, a, b)


def test_graph_replay(covt, oracle, gpu_available):
    """The forked varint launch captured in a HIP graph and replayed twice into poisoned buffers: the eager bytes."""
    import torch

    c, exp = corpus(covt, oracle)
    idx = c.varint_rows()
    lay, out, res = _run(covt, c, idx, covt.FAMILY_VARINT, covt.LAUNCH_FORKED)
    d, _, _, _, total = lay
    d_in = _device_input(covt, c)
    dev = d_in.device
    d_desc, d_out, d_res = _buffers(d, total, dev)

    def launch(stream):
        _enqueue(covt, d_in, d_desc, d.size, covt.FAMILY_VARINT, d_out, d_res, stream.cuda_stream, covt.LAUNCH_FORKED)

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):  # the fork streams and events exist before the capture
        launch(side)
    torch.cuda.current_stream(dev).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(torch.cuda.current_stream(dev))
    for _ in range(2):
        d_out.fill_(0x5A)
        d_res.fill_(0x33)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_res.cpu().numpy().reshape(-1, 2), res)
        assert np.array_equal(d_out.cpu().numpy(), out)
