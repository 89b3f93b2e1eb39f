"""GPU: Groth16's quotient evaluations for witness rows in HBM (include/pzkwit.h pzk_r1cs_quotient_batch,
csrc/kernels_quotient.hip, csrc/ntt.hpp). Every expectation comes from the Python definition of tests/quotient_ref.py,
byte for byte: the r1cs_ref case list at batches 1, 3 and T + 1 with padded strides, public wires, M a power of two and
one above it, elements at and above p, the host twin, a caller stream behind a RegisterIdentityLight instance, the
check after the quotient on one object, and scratch reuse over calls of different batches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quotient_ref as Q  # noqa: E402
import r1cs_ref as R  # noqa: E402
import test_quotient_host as H  # noqa: E402  (the shared case list and its reference results)
from pzkwit import light, native  # noqa: E402
from pzkwit.r1cs import R1cs  # noqa: E402

pytestmark = pytest.mark.gpu

T = 8  # pzk_quotient_info.tile
DEV = "cuda:0"
P = R.P
_loaded = {}
_want = {}


def system(name):
    if name not in _loaded:
        _loaded[name] = R1cs(H.cases()[name][0])
    return _loaded[name]


def want_h(name, w):
    """h of one witness of a case as bytes, computed once"""
    _, _, cons, n_pub, _ = H.cases()[name]
    key = (name, hash(tuple(w)))
    if key not in _want:
        _want[key] = Q.h_bytes(Q.quotient(cons, w, n_pub))
    return _want[key]


def device_h(r, rows, stream=None, pad=48):
    """rows: (batch, stride) uint8 -> (batch, 32 N + pad) uint8 from the device; h pre-filled with 0xFF"""
    import torch
    b = rows.shape[0]
    n = r.quotient_info()["n"]
    d = torch.from_numpy(rows).to(DEV)
    h = torch.full((b, 32 * n + pad), 0xFF, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    r.quotient_device(d.data_ptr(), b, rows.shape[1], h.data_ptr(), h.shape[1], stream=stream, sync=True)
    return h.cpu().numpy()


def assert_rows(name, r, ws, got):
    n = r.quotient_info()["n"]
    assert (got[:, 32 * n:] == 0xFF).all(), "padding written"
    for i, w in enumerate(ws):
        assert got[i, :32 * n].tobytes() == want_h(name, w), (name, i)


@pytest.mark.parametrize("batch", [1, 3, T + 1])
@pytest.mark.parametrize("name", H.CASES)
def test_case_list(name, batch):
    """the satisfying row first, then perturbed and unrelated rows (h is defined for all of them); witness stride
    32 n_wires + 48, h stride 32 N + 48, both paddings 0xFF; T + 1 is the smallest batch with a partial second tile"""
    _, n, cons, _, _ = H.cases()[name]
    r = system(name)
    assert r.quotient_info()["tile"] == T
    ws = R.batch_of(name, batch)
    if batch > 3:  # the reference of a row costs as much as the device call: rows 3 .. repeat rows 0 .. 2
        ws = [ws[i % 3] for i in range(batch)]
    rows = R.rows_of(ws, n)
    assert rows.shape[1] == 32 * n + 48
    got = device_h(r, rows)
    assert got.shape[1] == 32 * r.quotient_info()["n"] + 48
    assert_rows(name, r, ws, got)
    # the host twin gives the same bytes
    host = r.quotient_host(R.rows_of(ws[:3], n, pad=0).reshape(len(ws[:3]), n, 32))
    for i in range(len(ws[:3])):
        assert host[i].tobytes() == got[i, :host[i].size].tobytes()


@pytest.mark.parametrize("name", ["residue"] + ["pub_%d_%d_%d" % c for c in H.PUB_CASES])
def test_public_wires_powers_of_two_and_residues(name):
    """nPub in {0, 1, 5}, M a power of two and one above it; elements p, p + 1, 2^256 - 1 count as their residues"""
    _, n, cons, n_pub, ws = H.cases()[name]
    r = system(name)
    got = device_h(r, R.rows_of(ws, n))
    assert_rows(name, r, ws, got)
    host = r.quotient_host(R.rows_of(ws, n, pad=0).reshape(len(ws), n, 32))
    assert [host[i].tobytes() for i in range(len(ws))] == [got[i, :host[i].size].tobytes() for i in range(len(ws))]


def test_host_buffers():
    """R1cs.quotient (pzk_r1cs_quotient_batch_host: rows copied to the device, h copied back)"""
    _, n, cons, _, ws = H.cases()["long"]
    r = system("long")
    h = r.quotient(R.rows_of(ws, n, pad=0).reshape(len(ws), n, 32))
    assert [h[i].tobytes() for i in range(len(ws))] == [want_h("long", w) for w in ws]


def test_back_to_back_calls_reuse_the_scratch():
    """two calls on one object with different batches, back to back on one stream, into their own h rows"""
    import torch
    _, n, cons, _, _ = H.cases()["m257"]
    r = system("m257")
    big_n = r.quotient_info()["n"]
    ws = R.batch_of("m257", 3)
    ws1, ws2 = [ws[i % 3] for i in range(T + 1)], [ws[2], ws[0]]
    d1 = torch.from_numpy(R.rows_of(ws1, n)).to(DEV)
    d2 = torch.from_numpy(R.rows_of(ws2, n)).to(DEV)
    h1 = torch.full((len(ws1), 32 * big_n), 0xFF, dtype=torch.uint8, device=DEV)
    h2 = torch.full((len(ws2), 32 * big_n + 16), 0xFF, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        r.quotient_device(d1.data_ptr(), len(ws1), d1.shape[1], h1.data_ptr(), h1.shape[1], stream=s.cuda_stream, sync=False)
        r.quotient_device(d2.data_ptr(), len(ws2), d2.shape[1], h2.data_ptr(), h2.shape[1], stream=s.cuda_stream, sync=False)
    s.synchronize()
    assert_rows("m257", r, ws1, np.concatenate([h1.cpu().numpy(), np.full((len(ws1), 1), 0xFF, np.uint8)], axis=1))
    assert_rows("m257", r, ws2, h2.cpu().numpy())


def test_arguments():
    import torch
    _, n, cons, _, ws = H.cases()["budget"]
    r = system("budget")
    big_n = r.quotient_info()["n"]
    d = torch.from_numpy(R.rows_of(ws[:1], n)).to(DEV)
    h = torch.full((32 * big_n + 64,), 7, dtype=torch.uint8, device=DEV)
    r.quotient_device(d.data_ptr(), 0, 0, h.data_ptr(), 0)  # batch 0: a no-op
    assert (h == 7).all().item()
    with pytest.raises(native.PzkError, match="witness stride"):
        r.quotient_device(d.data_ptr(), 1, 32 * n - 16, h.data_ptr(), 32 * big_n)
    for h_stride in (32 * big_n - 16, 32 * big_n + 8):
        with pytest.raises(native.PzkError, match="h stride"):
            r.quotient_device(d.data_ptr(), 1, 32 * n, h.data_ptr(), h_stride)
    with pytest.raises(native.PzkError, match="aligned"):
        r.quotient_device(d.data_ptr(), 1, 32 * n, h.data_ptr() + 8, 32 * big_n)
    with pytest.raises(native.PzkError, match="device"):
        r.quotient_device(d.data_ptr(), 1, 32 * n + 48, h.data_ptr(), 32 * big_n, device=torch.cuda.device_count())
    assert (h == 7).all().item()


def test_light_rows_on_the_writer_s_stream_then_the_check():
    """RegisterIdentityLight(256, 3), 2 rows written by pzk_witness_batch on a caller stream, then the quotient of
    r1cs_ref.light_system on the same stream with no synchronise in between; afterwards the same object still passes
    check_device (the two paths share the device program)"""
    import torch
    inst = native.Instance(native.PZK_CIRCUIT_LIGHT, 0, dict(dg_hash=256, doc=3))
    W = inst.witness_size
    cons = R.light_system(W)
    r = R1cs(R.write_r1cs(W, cons))
    qi = r.quotient_info()
    assert (qi["n_rows"], qi["log2_n"]) == (len(cons) + 1, 10)
    big_n = qi["n"]
    d_in = torch.from_numpy(light.batch_rows(2)).to(DEV)
    stride = 32 * W + 48
    out = torch.full((2, stride), 0xFF, dtype=torch.uint8, device=DEV)
    st = torch.full((2,), 7, dtype=torch.int32, device=DEV)
    h = torch.full((2, 32 * big_n + 48), 0xFF, dtype=torch.uint8, device=DEV)
    first = torch.full((2,), 7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        inst.witness_batch_device(d_in.data_ptr(), 2, out.data_ptr(), stride, st.data_ptr(), stream=s.cuda_stream, sync=False)
        r.quotient_device(out.data_ptr(), 2, stride, h.data_ptr(), h.shape[1], stream=s.cuda_stream, sync=False)
        r.check_device(out.data_ptr(), 2, stride, first.data_ptr(), stream=s.cuda_stream, sync=False)
    s.synchronize()
    assert st.cpu().tolist() == [0, 0] and first.cpu().tolist() == [-1, -1]
    rows, got = out.cpu().numpy(), h.cpu().numpy()
    assert (got[:, 32 * big_n:] == 0xFF).all()
    for i in range(2):
        w = [int.from_bytes(rows[i, 32 * j:32 * j + 32].tobytes(), "little") for j in range(W)]
        assert R.evaluate(cons, w) == (-1, 0)
        assert got[i, :32 * big_n].tobytes() == Q.h_bytes(Q.quotient(cons, w, 0))
    inst.close()
