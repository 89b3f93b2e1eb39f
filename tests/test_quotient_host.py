"""CPU: the quotient's host twin (include/pzkwit.h pzk_r1cs_quotient_host / _quotient_info, csrc/r1cs.cpp) against the
Python definition (tests/quotient_ref.py), byte for byte: the r1cs_ref case list, elements at and above p, systems with
0, 1 and 5 public wires, M a power of two and one above it; the rejects; the device entry points without a device; and
the same cases through a host AddressSanitizer + UndefinedBehaviorSanitizer build of the twin (tools/fuzz/quotient_san.cpp,
a stand-alone program run directly, its buffers heap blocks of exactly the documented sizes)."""
import ctypes
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quotient_ref as Q  # noqa: E402
import r1cs_ref as R  # noqa: E402
from pzkwit import native  # noqa: E402
from pzkwit.r1cs import R1cs  # noqa: E402

P = R.P
PZK_E_ARG, PZK_E_NODEVICE = -1, -6
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "tools", "fuzz", "build", "quotient_san")
CASES = ["m257", "budget", "directed", "long", "only_long"]
# (constraints, public outputs, public inputs): nPub in {0, 1, 5}; M = nC + nPub + 1 a power of two and one above it
PUB_CASES = [(20, 0, 0), (20, 1, 0), (20, 2, 3), (63, 0, 0), (64, 0, 0), (62, 1, 0), (63, 0, 1), (122, 4, 1), (123, 0, 5)]
_cache = {}


def cases():
    """name -> (.r1cs bytes, n_wires, constraints, n_pub, witness rows as integers); built once, shared with the GPU test"""
    if not _cache:
        for name in CASES:
            n, cons, _ = R.case(name)
            _cache[name] = (R.write_r1cs(n, cons), n, cons, 0, R.batch_of(name, 3))
        n, cons, raw = R.residue_case()
        other = list(raw)
        other[12] = (1 << 256) - 2
        _cache["residue"] = (R.write_r1cs(n, cons), n, cons, 0, [raw, other, [v % P for v in raw]])
        for n_con, n_out, n_in in PUB_CASES:
            n, cons, w = Q.pub_case(n_con, n_out, n_in, seed=100 * n_con + 10 * n_out + n_in)
            name = "pub_%d_%d_%d" % (n_con, n_out, n_in)
            rows = [w, R.perturbed(__import__("random").Random(n_con), w, 2)]
            _cache[name] = (R.write_r1cs(n, cons, n_pub_out=n_out, n_pub_in=n_in), n, cons, n_out + n_in, rows)
    return _cache


def want_bytes(name):
    _, _, cons, n_pub, ws = cases()[name]
    key = ("want", name)
    if key not in _cache:
        _cache[key] = [Q.h_bytes(Q.quotient(cons, w, n_pub)) for w in ws]
    return _cache[key]


ALL = CASES + ["residue"] + ["pub_%d_%d_%d" % c for c in PUB_CASES]


@pytest.mark.parametrize("name", ALL)
def test_host_twin_equals_the_definition(name):
    data, n, cons, n_pub, ws = cases()[name]
    r = R1cs(data)
    m, k, big_n = Q.domain(len(cons), n_pub)
    qi = r.quotient_info()
    assert (qi["log2_n"], qi["n"], qi["n_rows"], qi["tile"]) == (k, big_n, m, 8)
    assert qi["scratch_bytes"] >= 2 * 8 * 32 * big_n
    rows = R.rows_of(ws, n, pad=0).reshape(len(ws), n, 32)
    h = r.quotient_host(rows)
    assert h.shape == (len(ws), big_n, 32)
    for i, want in enumerate(want_bytes(name)):
        assert h[i].tobytes() == want, (name, i)


def test_power_of_two_rows():
    got = {c: Q.domain(c[0], c[1] + c[2])[::2] for c in PUB_CASES}
    assert got[(63, 0, 0)] == (64, 64) and got[(64, 0, 0)] == (65, 128) and got[(62, 1, 0)] == (64, 64)
    assert got[(63, 0, 1)] == (65, 128) and got[(122, 4, 1)] == (128, 128) and got[(123, 0, 5)] == (129, 256)


def test_strided_rows_and_untouched_padding():
    """witness stride 32 n_wires + 48 and h stride 32 N + 48: the padding of h comes back as it was"""
    data, n, cons, n_pub, ws = cases()["m257"]
    r = R1cs(data)
    big_n = r.quotient_info()["n"]
    rows = R.rows_of(ws, n)
    h = np.full((len(ws), 32 * big_n + 48), 0xFF, dtype=np.uint8)
    native._check(native.lib().pzk_r1cs_quotient_host(r._h, rows.ctypes.data, len(ws), rows.shape[1], h.ctypes.data, h.shape[1]))
    assert (h[:, 32 * big_n:] == 0xFF).all()
    assert [h[i, :32 * big_n].tobytes() for i in range(len(ws))] == want_bytes("m257")


def test_rejects():
    L = native.lib()
    data, n, cons, _, ws = cases()["budget"]
    r = R1cs(data)
    big_n = r.quotient_info()["n"]
    rows = R.rows_of(ws[:1], n, pad=0)
    h = np.zeros(32 * big_n + 64, dtype=np.uint8)
    call = lambda stride, h_stride: L.pzk_r1cs_quotient_host(r._h, rows.ctypes.data, 1, stride, h.ctypes.data, h_stride)  # noqa: E731
    assert call(32 * n, 32 * big_n) == 0
    assert call(32 * n, 32 * big_n - 16) == PZK_E_ARG and b"h stride" in L.pzk_last_error()  # h_stride < 32 N
    assert call(32 * n, 32 * big_n + 8) == PZK_E_ARG and b"h stride" in L.pzk_last_error()   # misaligned
    assert call(32 * n - 16, 32 * big_n) == PZK_E_ARG and b"witness stride" in L.pzk_last_error()
    assert call(32 * n + 8, 32 * big_n) == PZK_E_ARG
    assert L.pzk_r1cs_quotient_host(r._h, None, 0, 0, None, 0) == 0  # batch 0
    assert L.pzk_r1cs_quotient_host(r._h, None, 1, 32 * n, h.ctypes.data, 32 * big_n) == PZK_E_ARG
    assert L.pzk_r1cs_quotient_info(r._h, None) == PZK_E_ARG


def test_domain_limits():
    """k = 0 (an empty system without public wires: M = 1, N = 1) and k > 24 are rejected with a reason by every entry
    point, before anything is allocated; k = 1 and k = 24 are the limits"""
    L = native.lib()
    info = native.PzkQuotientInfo()
    buf = np.zeros(96, dtype=np.uint8)
    ex = native.PzkExec(device=-1, flags=1, stream=None)
    empty = R1cs(R.write_r1cs(3, []))
    assert L.pzk_r1cs_quotient_info(empty._h, ctypes.byref(info)) == PZK_E_ARG and b"1 <= k <= 24" in L.pzk_last_error()
    assert L.pzk_r1cs_quotient_host(empty._h, buf.ctypes.data, 1, 96, buf.ctypes.data, 32) == PZK_E_ARG
    assert b"1 <= k <= 24" in L.pzk_last_error()
    for fn in (L.pzk_r1cs_quotient_batch, L.pzk_r1cs_quotient_batch_host):
        assert fn(empty._h, buf.ctypes.data & ~15, 1, 96, buf.ctypes.data & ~15, 32, ctypes.byref(ex)) == PZK_E_ARG
        assert b"1 <= k <= 24" in L.pzk_last_error()
    # M = 2: the constant wire's row and one public wire's, no constraint
    r = R1cs(R.write_r1cs(3, [], n_pub_out=1))
    assert r.quotient_info()["log2_n"] == 1 and r.quotient_info()["n"] == 2 and r.quotient_info()["n_rows"] == 2
    w = [1, 5, 7]
    rows = R.rows_of([w], 3, pad=0).reshape(1, 3, 32)
    assert r.quotient_host(rows).tobytes() == Q.h_bytes(Q.quotient([], w, 1))
    # public wires alone push M past 2^24 (the loader takes the header's counts as they are)
    ok = R1cs(R.write_r1cs(3, [], n_pub_in=(1 << 24) - 1))
    assert ok.quotient_info()["log2_n"] == 24 and ok.quotient_info()["n_rows"] == 1 << 24
    # ... but its rows cannot be read: wires 0 .. nPub must exist
    assert L.pzk_r1cs_quotient_host(ok._h, buf.ctypes.data, 1, 96, buf.ctypes.data, 32 << 24) == PZK_E_ARG
    assert b"public wires" in L.pzk_last_error()
    big = R1cs(R.write_r1cs(3, [], n_pub_in=1 << 24))
    assert L.pzk_r1cs_quotient_info(big._h, ctypes.byref(info)) == PZK_E_ARG
    assert b"1 <= k <= 24" in L.pzk_last_error()
    assert L.pzk_r1cs_quotient_host(big._h, buf.ctypes.data, 1, 96, buf.ctypes.data, 1 << 40) == PZK_E_ARG
    assert b"1 <= k <= 24" in L.pzk_last_error()
    for fn in (L.pzk_r1cs_quotient_batch, L.pzk_r1cs_quotient_batch_host):
        assert fn(big._h, buf.ctypes.data & ~15, 1, 96, buf.ctypes.data & ~15, 1 << 40, ctypes.byref(ex)) == PZK_E_ARG
        assert b"1 <= k <= 24" in L.pzk_last_error()


def test_quotient_needs_a_device():
    """the device entry points are not served by the host twin: without a device they fail with PZK_E_NODEVICE"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("device present")
    data, n, _, _, _ = cases()["budget"]
    r = R1cs(data)
    big_n = r.quotient_info()["n"]
    rows = np.zeros((1, n * 32 + 16), dtype=np.uint8)
    h = np.zeros(32 * big_n + 16, dtype=np.uint8)
    ex = native.PzkExec(device=-1, flags=1, stream=None)
    L = native.lib()
    # (the pointers are never dereferenced: the call fails before any launch)
    assert L.pzk_r1cs_quotient_batch(r._h, (rows.ctypes.data + 15) & ~15, 1, 32 * n, (h.ctypes.data + 15) & ~15, 32 * big_n,
                                     ctypes.byref(ex)) == PZK_E_NODEVICE
    assert b"no HIP device" in L.pzk_last_error()
    assert L.pzk_r1cs_quotient_batch_host(r._h, rows.ctypes.data, 1, 32 * n, h.ctypes.data, 32 * big_n,
                                          ctypes.byref(ex)) == PZK_E_NODEVICE
    with pytest.raises(native.PzkError, match="no HIP device"):
        r.quotient(rows[:, :32 * n].reshape(1, n, 32))
    assert L.pzk_r1cs_quotient_batch(r._h, None, 0, 0, None, 0, None) == 0  # batch 0: a no-op on any host


# ---- the sanitizer leg
@pytest.fixture(scope="module")
def san_bin():
    if not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None:
        pytest.skip("no hipcc for the host sanitizer build")
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tools", "fuzz"), "build/quotient_san"])
    return BIN


def test_host_twin_under_sanitizers(san_bin):
    names = ALL
    rec = []
    for name in names:
        data, n, _, _, ws = cases()[name]
        rows = R.rows_of(ws, n)  # stride 32 n + 48
        rec.append(struct.pack("<I", len(data)) + data + struct.pack("<II", rows.shape[0], rows.shape[1]) + rows.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="allocator_may_return_null=1:detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([san_bin], input=b"".join(rec), capture_output=True, timeout=600, env=env)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err and "BAD" not in err, err[-3000:]
    out, at = p.stdout, 0
    for name in names:
        _, _, cons, n_pub, ws = cases()[name]
        _, k, big_n = Q.domain(len(cons), n_pub)
        assert struct.unpack_from("<iI", out, at) == (0, k), name
        at += 8
        for want in want_bytes(name):
            assert out[at:at + 32 * big_n] == want, name
            at += 32 * big_n
    assert at == len(out)
