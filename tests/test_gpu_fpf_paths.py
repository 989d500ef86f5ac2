"""The directed FastPFOR corpus (tests/covt_fpf.py; its frames are asserted on the CPU by tests/test_fpf_ref.py)
through every route that runs a FastPFOR decoder: the family kernel's two variants (COVT_LAUNCH_FPF_STREAM:
run_fastpfor_stream, COVT_LAUNCH_FPF_CLASSIC: run_fastpfor), the fused kernel, and split chunks of 256 and 512
values with and without the plan's start states.  Every row (case x address residue 0/4/8/12 x op x value
count) must equal the oracle (DecodingUtils.java:316-444) in values, status and consumed bytes, and leave the
128 guard bytes after its 128-byte-aligned output slot untouched.

The malformed set (every whole-word truncation of `small3` and single-field edits of it) runs through the two
family routes and the fused route: the three must agree, and their statuses are pinned by
tests/golden/fpf_status.json (recorded with the library of the commit before the decoders were rebuilt from
shared pieces; COVT_FPF_RECORD=path writes such a file instead of comparing).  A failed row's values are
compared over the blocks every route has stored by then: run_fastpfor_stream stores every block before the
failing one, run_fastpfor walks block j + 1's header before it stores block j, so one block fewer."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import covt_fpf as F
from conftest import GOLDEN
from test_gpu_split import DESC
from test_split_plan import _states_hook

pytestmark = pytest.mark.gpu

GUARD = 128


@pytest.fixture(scope="module")
def rows(covt, oracle):
    return F.rows(covt, oracle)


def _layout(rws):
    """Input blob (row r at an address of residue r["residue"] modulo 16; the device buffer is 256-byte
    aligned) and output offsets: 128-byte-aligned slots, each followed by a guard."""
    blob, ins, outs, out_off = bytearray(), [], [], 0
    for r in rws:
        while len(blob) % 16 != r["residue"]:
            blob.append(0xA5)
        ins.append(len(blob))
        blob += r["enc"]
        outs.append(out_off)
        out_off += (4 * r["ne"] + 127) // 128 * 128 + GUARD
    return bytes(blob), ins, outs, out_off


def _launch(covt, blob, d, family, out_bytes, launch):
    import torch

    counts = np.zeros(covt.NUM_FAMILIES, dtype=np.int64)
    counts[family] = d.size
    dev = torch.device("cuda")
    d_in = torch.zeros(len(blob) + covt.INPUT_PADDING + 16, dtype=torch.uint8, device=dev)
    assert d_in.data_ptr() % 16 == 0
    d_in[:len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    d_desc = torch.from_numpy(d.view(np.uint8)).to(dev)
    d_out = torch.full((out_bytes + 16,), 0x5A, dtype=torch.uint8, device=dev)
    d_res = torch.full((d.size * 2,), 0x33, dtype=torch.int32, device=dev)
    st = covt.lib().covt_decode_streams_device_grouped_mode(
        d_in.data_ptr(), d_desc.data_ptr(), counts.ctypes.data_as(C.POINTER(C.c_int64)), d_out.data_ptr(),
        d_res.data_ptr(), torch.cuda.current_stream().cuda_stream, launch)
    assert st == 0
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_res.cpu().numpy().reshape(-1, 2)


def _family_route(covt, rws, launch):
    """Whole streams, one wave each -> (output bytes, output offsets, (status, consumed) per row)."""
    blob, ins, outs, out_bytes = _layout(rws)
    order = sorted(range(len(rws)), key=lambda k: -len(rws[k]["enc"]))  # largest first, as the plan orders a family
    d = np.array([(ins[k], outs[k], len(rws[k]["enc"]), rws[k]["nv"], rws[k]["op"], rws[k]["nb"], 0, len(rws[k]["enc"]))
                  for k in order], dtype=DESC)
    out, res = _launch(covt, blob, d, covt.FAMILY_FASTPFOR, out_bytes, launch)
    back = np.empty(len(rws), dtype=np.int64)
    back[order] = np.arange(len(rws))
    return out, outs, res[back]


def _split_route(covt, rws, chunk, with_states):
    """Every row as value chunks (a group of SPLIT_SLOTS descriptors each: the head, the range pad, the state
    pads), all rows in one launch; a stream's result is its first group's."""
    blob, ins, outs, out_bytes = _layout(rws)
    groups, first = [], []
    for k, r in enumerate(rws):
        n, bl = r["nv"], len(r["enc"])
        nch = (n + chunk - 1) // chunk
        states = _states_hook(covt, r["enc"], n, chunk) if with_states else None
        d = np.zeros(nch * covt.SPLIT_SLOTS, dtype=DESC)
        for c in range(nch):
            g = c * covt.SPLIT_SLOTS
            d[g] = (ins[k], outs[k], c, n, r["op"], r["nb"], covt.DESC_SPLIT | covt.DESC_SPLIT_FPF, bl)
            d[g + 1:g + covt.SPLIT_SLOTS]["flags"] = covt.DESC_SPLIT_PAD | covt.DESC_SPLIT_FPF
            d[g + 1]["in_off"], d[g + 1]["out_off"] = c * chunk, min((c + 1) * chunk, n)
            if states is not None:  # seven int32 slots per pad, every field but op / num_bits / flags
                raw = d.view(np.uint8).reshape(-1, 32)
                for i in range(42):
                    o = (0, 4, 8, 12, 16, 20, 28)[i % 7]
                    raw[g + 2 + i // 7, o:o + 4] = np.frombuffer(np.int32(states[c, i]).tobytes(), dtype=np.uint8)
        first.append(sum(x.size for x in groups))
        groups.append(d)
    out, res = _launch(covt, blob, np.concatenate(groups), covt.FAMILY_SPLIT_FPF, out_bytes, 0)
    return out, outs, res[first]


def _check(covt, rws, out, outs, res, route):
    n_ok = 0
    for k, r in enumerate(rws):
        o_st, o_arr, o_pos = r["oracle"]
        key = (route, r["name"], r["residue"], r["op"], r["nv"])
        assert int(res[k, 0]) == o_st, key + (int(res[k, 0]), o_st)
        slot = (4 * r["ne"] + 127) // 128 * 128
        assert (out[outs[k] + slot:outs[k] + slot + GUARD] == 0x5A).all(), key  # nothing past the slot
        if o_st != 0:
            assert int(res[k, 1]) == 0, key  # a failed stream consumed nothing (include/covt.h)
            continue
        assert int(res[k, 1]) == len(r["enc"]) == o_pos, key
        got = out[outs[k]:outs[k] + 4 * r["ne"]].view(np.int32)
        assert np.array_equal(got, np.asarray(o_arr, dtype=np.int32)), key
        n_ok += 1
    return n_ok


def test_rows_cover_the_table(covt, rows):
    assert 300 <= len(rows) <= 400
    assert {r["residue"] for r in rows} == set(F.RESIDUES)
    assert sum(r["oracle"][0] == covt.ERR_COUNT_MISMATCH for r in rows) >= 4 * 6  # odd x,y counts
    assert all(r["oracle"][0] in (0, covt.ERR_COUNT_MISMATCH) for r in rows)


@pytest.mark.parametrize("route", ["stream", "classic", "fused"])
def test_whole_streams(covt, gpu_available, rows, route):
    launch = {"stream": covt.LAUNCH_FORKED | covt.LAUNCH_FPF_STREAM, "classic": covt.LAUNCH_FORKED | covt.LAUNCH_FPF_CLASSIC,
              "fused": covt.LAUNCH_FUSED}[route]
    out, outs, res = _family_route(covt, rows, launch)
    assert _check(covt, rows, out, outs, res, route) > 250


@pytest.mark.parametrize("with_states", [False, True], ids=["walked", "host_states"])
@pytest.mark.parametrize("chunk", [256, 512])
def test_split_chunks(covt, gpu_available, rows, chunk, with_states):
    def fill_past_tail_chunk(r):
        # Left out: a zero fill that crosses a chunk edge after the VariableByte tail's first value (here: 255
        # tail values and 10 more asked for).  The chunk holding value n - 1 then stores the whole tail from
        # the chunk before it, which adds its carry to that range in place (run_fastpfor_chunk's one-pass ops):
        # the order of the two is not defined, before as after this corpus was written.  A plan asks for more
        # values than a stream codes only for a damaged tile.  Morton chunks decode twice and are kept.
        L = F.words(r["enc"])[0] // F.BLOCK * F.BLOCK
        return r["op"] != covt.OP_FPF_DELTA_MORTON and (L // chunk + 1) * chunk < r["nv"]

    rws = [r for r in rows if not (r["op"] == covt.OP_FPF_ZZ_DELTA_XY and r["nv"] & 1)]  # (never split: the plan's rule)
    n_all = len(rws)
    rws = [r for r in rws if not fill_past_tail_chunk(r)]
    assert n_all - len(rws) == 8  # small3+255 and b32+255 with 10 more values, int32 op, four residues
    out, outs, res = _split_route(covt, rws, chunk, with_states)
    assert _check(covt, rws, out, outs, res, "split%d" % chunk) > 250


def test_malformed_statuses(covt, oracle, gpu_available):
    bad = F.malformed(oracle)
    ops = ((covt.OP_FPF_ZZ_DELTA_I32, 0), (covt.OP_FPF_ZZ_DELTA_XY, 0), (covt.OP_FPF_DELTA_MORTON, 14))
    rws = [dict(name=name, enc=enc, residue=0, op=op, nb=nb, nv=n, ne=2 * n if nb else n, good=good)
           for name, enc, n, good in bad for op, nb in ops]
    got = [_family_route(covt, rws, launch) for launch in
           (covt.LAUNCH_FORKED | covt.LAUNCH_FPF_STREAM, covt.LAUNCH_FORKED | covt.LAUNCH_FPF_CLASSIC, covt.LAUNCH_FUSED)]
    (o1, outs, r1) = got[0]
    for o2, _, r2 in got[1:]:
        assert np.array_equal(r1, r2)
        for k, r in enumerate(rws):
            # a decoded row: all of it; a failed one: the blocks every route has stored by then
            ne = r["ne"] if r1[k, 0] == 0 else max(r["good"] - 1, 0) * F.BLOCK * (2 if r["nb"] else 1)
            a = outs[k]
            assert np.array_equal(o1[a:a + 4 * ne], o2[a:a + 4 * ne]), (r["name"], r["op"])
    status = {"%s/%d" % (r["name"], r["op"]): [int(r1[k, 0]), int(r1[k, 1])] for k, r in enumerate(rws)}
    assert sum(v[0] != 0 for v in status.values()) > 300 and sum(v[0] == 0 for v in status.values()) >= 3
    record = os.environ.get("COVT_FPF_RECORD")
    if record:
        with open(record, "w") as f:
            json.dump({"columns": ["status", "consumed"], "rows": status}, f, indent=0, sort_keys=True)
            f.write("\n")
        return
    with open(os.path.join(GOLDEN, "fpf_status.json")) as f:
        pinned = json.load(f)["rows"]
    assert status == pinned
