"""GPU: witness rows checked against a circom .r1cs system where they lie, in HBM (include/pzkwit.h
pzk_r1cs_check_batch, csrc/r1cs.hpp k_r1cs_check / k_r1cs_check_long). Every expectation comes from the Python
evaluator of tests/r1cs_ref.py, never from the library: the case list of tests/test_r1cs_file.py (constraint counts
around the wave and the chunk, a chunk cut by its term budget, every LC shape and coefficient, long constraints of 33 to
1,000 terms, elements at and above p), the reported index and count, caller streams, and rows a RegisterIdentityLight
instance has just written."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import r1cs_ref as R  # noqa: E402
from pzkwit import light, native  # noqa: E402
from pzkwit.r1cs import R1cs  # noqa: E402

pytestmark = pytest.mark.gpu

R1CS_WT = 8  # csrc/r1cs.hpp: witnesses per tile of k_r1cs_check
DEV = "cuda:0"
P = R.P
_loaded = {}


def system(name):
    """the case's R1cs object, loaded (and uploaded) once"""
    if name not in _loaded:
        n, cons, _ = R.case(name)
        _loaded[name] = R1cs(R.write_r1cs(n, cons))
    return _loaded[name]


def check_rows(r, rows, with_counts=True, stream=None):
    """rows: (batch, stride) uint8 with the padding 0xFF -> [(first_failed, n_failed)] from the device; the result
    buffers are pre-filled with 7 (the call presets them itself)"""
    import torch
    b = rows.shape[0]
    d = torch.from_numpy(rows).to(DEV)
    first = torch.full((b,), 7, dtype=torch.int32, device=DEV)
    cnt = torch.full((b,), 7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    r.check_device(d.data_ptr(), b, rows.shape[1], first.data_ptr(), cnt.data_ptr() if with_counts else None,
                   stream=stream, sync=True)
    return list(zip(first.cpu().tolist(), cnt.cpu().tolist()))


@pytest.mark.parametrize("batch", R.BATCHES)
@pytest.mark.parametrize("name", sorted(R.CASE_BUILDERS))
def test_case_list(name, batch):
    """every case at batches 1, 3 and R1CS_WT + 1 (the smallest batch with a partial second tile): the satisfying row
    first, then rows that violate one, a few or almost all constraints; stride 32 * n_wires + 48"""
    assert R.BATCHES == [1, 3, R1CS_WT + 1] and R.R1CS_WT == R1CS_WT
    n, cons, _ = R.case(name)
    ws = R.batch_of(name, batch)
    want = [R.evaluate(cons, w) for w in ws]
    rows = R.rows_of(ws, n)
    assert rows.shape[1] == 32 * n + 48
    assert check_rows(system(name), rows) == want


@pytest.mark.parametrize("name", ["m257", "budget", "directed", "long", "only_long"])
def test_satisfying_batch(name):
    n, cons, w = R.case(name)
    assert check_rows(system(name), R.rows_of([w] * (R1CS_WT + 1), n)) == [(-1, 0)] * (R1CS_WT + 1)


def broken(cons, ks):
    """the system with C + 1 in constraints ks: exactly those fail on a witness that satisfied it (w0 = 1)"""
    out = list(cons)
    for k in ks:
        a, b, c = out[k]
        out[k] = (a, b, c + [(0, 1)])
    return out


def long_indices(cons):
    return [k for k, con in enumerate(cons) if max(len({i for i, _ in lc}) for lc in con) > R.R1CS_LONG_T]


@pytest.mark.parametrize("name,ks", [("m257", [0]), ("m257", [63]), ("m257", [64]), ("m257", [256]), ("long", [-1]),
                                     ("long", "long"), ("only_long", "long"), ("m257", [200, 5, 64]),
                                     ("long", "long3")])
def test_reported_index_and_count(name, ks):
    """one violated constraint at index 0, 63, 64, the last, and a long one: that index, count 1; three violated
    constraints in one row (short ones; a short and two long ones): the lowest index, count 3"""
    n, cons, w = R.case(name)
    if ks == "long":
        ks = [long_indices(cons)[len(long_indices(cons)) // 2]]
    elif ks == "long3":
        li = long_indices(cons)
        ks = [li[-1], li[3], li[3] + 1]
        assert li[3] + 1 not in li
    ks = [k % len(cons) for k in ks]
    bad = broken(cons, ks)
    want = R.evaluate(bad, w)
    assert want == (min(ks), len(ks))
    r = R1cs(R.write_r1cs(n, bad))
    rows = R.rows_of([w] * 3, n)
    assert check_rows(r, rows) == [want] * 3
    assert [f for f, _ in check_rows(r, rows, with_counts=False)] == [want[0]] * 3  # n_failed = NULL


def test_one_bad_row_in_a_batch():
    """one row of R1CS_WT + 1 (in the first tile, then alone in the second) with an element replaced that a long
    constraint reads: every other row, of both tiles, stays at -1"""
    n, cons, w = R.case("long")
    rng = np.random.default_rng(5)
    for bad_row in (2, R1CS_WT):
        ws = [list(w) for _ in range(R1CS_WT + 1)]
        wire = cons[long_indices(cons)[0]][0][7][0]  # a wire of the first long constraint's A
        ws[bad_row][wire] = (ws[bad_row][wire] + int(rng.integers(1, 1 << 62))) % P
        want = [R.evaluate(cons, x) for x in ws]
        assert want[bad_row][0] >= 0 and all(v == (-1, 0) for i, v in enumerate(want) if i != bad_row)
        assert check_rows(system("long"), R.rows_of(ws, n)) == want


def test_elements_at_and_above_p():
    """p, p + 1 and 2^256 - 1 at wires read through +1, -1 and general coefficients count as their residues"""
    n, cons, raw = R.residue_case()
    r = R1cs(R.write_r1cs(n, cons))
    other = list(raw)
    other[12] = (1 << 256) - 2  # one less than the satisfying 2^256 - 1
    other[15] = P + 1
    ws = [raw, other, [v % P for v in raw]]
    want = [R.evaluate(cons, w) for w in ws]
    assert want[0] == want[2] == (-1, 0) and want[1][1] > 0
    assert check_rows(r, R.rows_of(ws, n)) == want


def test_host_buffers():
    """R1cs.check (pzk_r1cs_check_batch_host: rows copied to the device and checked there)"""
    n, cons, _ = R.case("long")
    ws = R.batch_of("long", R1CS_WT + 1)
    first, cnt = system("long").check(R.rows_of(ws, n, pad=0).reshape(len(ws), n, 32))
    assert list(zip(first.tolist(), cnt.tolist())) == [R.evaluate(cons, w) for w in ws]


def test_caller_stream_and_back_to_back_checks():
    """the rows are written on a torch stream immediately before the check on the same stream, with no synchronise in
    between (the buffer held other rows until then); a second check of other rows follows back to back into its own
    result buffers"""
    import torch
    n, cons, w = R.case("m257")
    r = system("m257")
    b = R1CS_WT + 1
    ws1, ws2 = R.batch_of("m257", b), [w] * b
    src1 = torch.from_numpy(R.rows_of(ws1, n)).to(DEV)
    src2 = torch.from_numpy(R.rows_of(ws2, n)).to(DEV)
    d1 = torch.from_numpy(R.rows_of(ws2, n)).to(DEV)  # stale rows: all satisfying
    d2 = torch.from_numpy(R.rows_of(ws1, n)).to(DEV)  # stale rows: mostly failing
    res = [torch.full((b,), 7, dtype=torch.int32, device=DEV) for _ in range(4)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        d1.copy_(src1, non_blocking=True)
        d2.copy_(src2, non_blocking=True)
        r.check_device(d1.data_ptr(), b, d1.shape[1], res[0].data_ptr(), res[1].data_ptr(), stream=s.cuda_stream, sync=False)
        r.check_device(d2.data_ptr(), b, d2.shape[1], res[2].data_ptr(), res[3].data_ptr(), stream=s.cuda_stream, sync=False)
    s.synchronize()
    got = [t.cpu().tolist() for t in res]
    assert list(zip(got[0], got[1])) == [R.evaluate(cons, x) for x in ws1]
    assert list(zip(got[2], got[3])) == [(-1, 0)] * b


def test_arguments():
    import torch
    n, cons, w = R.case("m1")
    r = system("m1")
    d = torch.from_numpy(R.rows_of([w], n)).to(DEV)
    first = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    r.check_device(d.data_ptr(), 0, 0, first.data_ptr())  # batch 0: a no-op
    assert first.cpu().tolist() == [7]
    for stride in (32 * n - 16, 32 * n + 8):
        with pytest.raises(native.PzkError, match="stride"):
            r.check_device(d.data_ptr(), 1, stride, first.data_ptr())
    with pytest.raises(native.PzkError, match="aligned"):
        r.check_device(d.data_ptr() + 8, 1, 32 * n, first.data_ptr())
    with pytest.raises(native.PzkError, match="device"):
        r.check_device(d.data_ptr(), 1, 32 * n + 48, first.data_ptr(), device=torch.cuda.device_count())


def test_light_rows_checked_in_place():
    """RegisterIdentityLight(256, 3), batch 3, written by pzk_witness_batch and checked where it lies against the facts
    DESIGN.md §13 states about the layout (tests/r1cs_ref.py light_system; the offsets hold on the reference row
    tests/test_gpu_light.py pins): all rows pass; after one byte of b2n.sum[100] of row 1 is changed on the device,
    row 1 reports the first constraint that reads it (and the next one, which reads it too), rows 0 and 2 pass"""
    import torch
    inst = native.Instance(native.PZK_CIRCUIT_LIGHT, 0, dict(dg_hash=256, doc=3))
    W = inst.witness_size
    cons = R.light_system(W)
    info = R.info_of(cons)
    assert info["n_long"] == 1 and info["max_terms"] == 249
    r = R1cs(R.write_r1cs(W, cons))
    assert {k: r.info[k] for k in info} == info
    rows = light.batch_rows(3)
    d_in = torch.from_numpy(rows).to(DEV)
    stride = 32 * W + 48
    out = torch.full((3, stride), 0xFF, dtype=torch.uint8, device=DEV)
    st = torch.full((3,), 7, dtype=torch.int32, device=DEV)
    first = torch.full((3,), 7, dtype=torch.int32, device=DEV)
    cnt = torch.full((3,), 7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    inst.witness_batch_device(d_in.data_ptr(), 3, out.data_ptr(), stride, st.data_ptr(), sync=True)
    inst.sync()
    assert st.cpu().tolist() == [0, 0, 0]
    r.check_device(out.data_ptr(), 3, stride, first.data_ptr(), cnt.data_ptr())
    assert (first.cpu().tolist(), cnt.cpu().tolist()) == ([-1, -1, -1], [0, 0, 0])
    assert (out[:, 32 * W:] == 0xFF).all().item()
    out[1, 32 * (W - 248 + 100) + 3] ^= 0x10
    torch.cuda.synchronize()
    r.check_device(out.data_ptr(), 3, stride, first.data_ptr(), cnt.data_ptr())
    assert (first.cpu().tolist(), cnt.cpu().tolist()) == ([-1, R.LIGHT_SUM100, -1], [0, 2, 0])
    # the evaluator on the downloaded row agrees
    w1 = [int.from_bytes(bytes(e), "little") for e in out[1, : 32 * W].cpu().numpy().reshape(W, 32)]
    assert R.evaluate(cons, w1) == (R.LIGHT_SUM100, 2)
    inst.close()
