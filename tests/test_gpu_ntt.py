"""GPU: the transforms of csrc/ntt.hpp through the test-only probe library (csrc/probe/probe_ntt.hip), bit for bit
against Python integers (tests/quotient_ref.py): forward and inverse at every k = 1 .. r + 2 on the default plan,
explicit splits that reach every pass count and partial-pass shape, and one large size (k = 20) checked by a round trip
on the device and by Horner evaluation at four points."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quotient_ref as Q  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(REPO, "passport-zk-circuits_amd", "lib", "libpzkprobe.so")
P = Q.P
DEV = "cuda:0"
_ref = {}


@pytest.fixture(scope="module")
def probe():
    L = ctypes.CDLL(PROBE)
    IP = ctypes.POINTER(ctypes.c_int)
    L.pzk_probe_ntt.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, IP, ctypes.c_int,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.pzk_probe_ntt_plan.argtypes = [ctypes.c_int, IP, IP]
    return L


def plan_of(probe, k):
    q, r = (ctypes.c_int * 24)(), ctypes.c_int()
    n = probe.pzk_probe_ntt_plan(k, q, ctypes.byref(r))
    return list(q)[:n], r.value


def to_words(vecs):
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for v in vecs for x in v), dtype=np.uint32).copy()


def from_words(a, batch, n):
    b = a.tobytes()
    return [[int.from_bytes(b[32 * (r * n + i):32 * (r * n + i + 1)], "little") for i in range(n)] for r in range(batch)]


def run(probe, inverse, shift, k, vecs, split=None):
    a = to_words(vecs)
    out = np.zeros_like(a)
    sp = (ctypes.c_int * len(split))(*split) if split else None
    rc = probe.pzk_probe_ntt(int(inverse), int(shift), k, len(vecs), sp, len(split) if split else 0, a.ctypes.data,
                             out.ctypes.data, 0)
    assert rc == 0, rc
    return from_words(out, len(vecs), 1 << k)


def vectors(k):
    """dense random canonical inputs (three of them: batch 3), all-zero, all p - 1, and a single 1 at 0, 1, N / 2, N - 1"""
    n = 1 << k
    rng = random.Random(0x177 + k)
    dense = [[rng.randrange(P) for _ in range(n)] for _ in range(3)]
    special = [[0] * n, [P - 1] * n]
    for i in sorted({0, 1, n // 2, n - 1}):
        v = [0] * n
        v[i] = 1
        special.append(v)
    return dense, special


def want(kind, k, v):
    """reference results, computed once per (transform, k, vector)"""
    key = (kind, k, hash(tuple(v)))
    if key not in _ref:
        _ref[key] = (Q.forward_bitrev_in(v, k) if kind == "fwd" else Q.inverse_bitrev_out(v, k, kind == "inv_shift"))
    return _ref[key]


def check(probe, k, vecs, split=None):
    for kind in ("fwd", "inv_shift", "inv"):
        got = run(probe, kind != "fwd", kind == "inv_shift", k, vecs, split)
        for g, v in zip(got, vecs):
            assert g == want(kind, k, v), (kind, k, split)


def test_default_plan_and_r(probe):
    _, r = plan_of(probe, 1)
    assert 8 <= r <= 12 and (32 << r) * 2 <= 160 * 1024  # at least two workgroups of 2^r points per CU
    for k in range(1, 25):
        q, _ = plan_of(probe, k)
        assert sum(q) == k and all(1 <= x <= r for x in q) and len(q) == -(-k // r)
    assert len(plan_of(probe, 22)[0]) <= 3
    assert probe.pzk_probe_ntt_plan(0, None, None) == 0 and probe.pzk_probe_ntt_plan(25, None, None) == 0


@pytest.mark.parametrize("k", range(1, 13))
def test_every_size_on_the_default_plan(probe, k):
    """k = 1 .. r + 2: one pass up to r, two passes above; batches 3 (the dense vectors) and 1 (each special vector)"""
    _, r = plan_of(probe, 1)
    assert r + 2 == 12
    dense, special = vectors(k)
    check(probe, k, dense)
    for v in special:
        check(probe, k, [v])
    check(probe, k, dense[:1])


@pytest.mark.parametrize("split", [[3, 3, 3], [4, 5], [1, 8], [8, 1], [2, 3, 4]])
def test_explicit_splits_k9(probe, split):
    dense, special = vectors(9)
    check(probe, 9, dense, split)
    check(probe, 9, special[:1] + special[2:4], split)


@pytest.mark.parametrize("order", ["r1", "1r"])
def test_explicit_splits_r_plus_one(probe, order):
    _, r = plan_of(probe, 1)
    split = [r, 1] if order == "r1" else [1, r]
    dense, special = vectors(r + 1)
    check(probe, r + 1, dense, split)
    check(probe, r + 1, special[-2:], split)


def test_bad_splits_are_refused(probe):
    _, r = plan_of(probe, 1)
    a = to_words([[1] * 2048])
    for split in ([4, 4], [5, 5], [0, 9], [9, 0], [-1, r], [r + 1]):
        sp = (ctypes.c_int * len(split))(*split)
        assert probe.pzk_probe_ntt(0, 0, 9, 1, sp, len(split), a.ctypes.data, a.ctypes.data, 0) == 1


def test_large_size_round_trip_and_horner(probe):
    """k = 20, default plan (two passes of 10), batch 1: inverse(forward(x)) = x, compared on the device; the forward
    output at 4 indices against Horner evaluation of the 2^20 coefficients"""
    import torch
    k, n = 20, 1 << 20
    rng = np.random.default_rng(20)
    words = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    words[:, 7] &= 0x1FFFFFFF  # below 2^253 < p: canonical
    x = torch.from_numpy(words.view(np.int32)).to(DEV)
    y = torch.empty_like(x)
    z = torch.empty_like(x)
    torch.cuda.synchronize()
    assert probe.pzk_probe_ntt(0, 0, k, 1, None, 0, x.data_ptr(), y.data_ptr(), 1) == 0
    assert probe.pzk_probe_ntt(1, 0, k, 1, None, 0, y.data_ptr(), z.data_ptr(), 1) == 0
    assert torch.equal(x, z)
    assert not torch.equal(x, y)
    # x holds coefficient i at index bitrev(i)
    idx = np.arange(n, dtype=np.uint32)
    rev = np.zeros(n, dtype=np.uint32)
    for b in range(k):
        rev |= ((idx >> b) & 1) << (k - 1 - b)
    raw = words[rev].tobytes()  # coefficient order
    coef = [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(n)]
    w = Q.root_of_unity(k)
    picks = [0, n - 1, n // 2 + 1, random.Random(7).randrange(n)]
    got = y[picks].cpu().numpy().view(np.uint32)
    for j, row in zip(picks, got):
        pt, acc = pow(w, j, P), 0
        for c in reversed(coef):
            acc = (acc * pt + c) % P
        assert int.from_bytes(row.tobytes(), "little") == acc, j
