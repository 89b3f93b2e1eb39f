"""The device arithmetic primitives on directed operands (tests/arith_cases.py), called directly through the test-only
probe library libpzkprobe.so (csrc/probe/) and compared bit for bit with plain Python integers: the one-lane Fr
functions, the quad-spread products and their carry settles, the 128/64 division steps, the Knuth D long divisions and
the curves' Montgomery fields. The end-to-end witness tests cannot steer these operands; tests/test_arith_cases.py
shows on the CPU which rare branches the cases reach."""
import ctypes
import os

import numpy as np
import pytest

import arith_cases as A

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(REPO, "passport-zk-circuits_amd", "lib", "libpzkprobe.so")
U32P = ctypes.POINTER(ctypes.c_uint32)
U64P = ctypes.POINTER(ctypes.c_uint64)
I32P = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def probe():
    # a missing library fails the tests (make -C passport-zk-circuits_amd/csrc builds it); it never skips them
    assert os.path.exists(PROBE), "%s is missing: build it with make -C passport-zk-circuits_amd/csrc" % PROBE
    L = ctypes.CDLL(PROBE)
    L.pzk_probe_fr.argtypes = [ctypes.c_int, U32P, U32P, U32P, ctypes.c_int]
    L.pzk_probe_fr_batch_inv.argtypes = [U32P, U32P, ctypes.c_int, ctypes.c_int]
    L.pzk_probe_fq.argtypes = [ctypes.c_int, U32P, U32P, U32P, U32P, U32P, ctypes.c_int]
    L.pzk_probe_div64.argtypes = [ctypes.c_int, U64P, U64P, U64P, U64P, U64P, ctypes.c_int]
    L.pzk_probe_kd_div.argtypes = [U64P, I32P, ctypes.c_int, U64P, I32P, ctypes.c_int, U64P, U64P, ctypes.c_int]
    L.pzk_probe_ec_field.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, U32P, U32P, U32P, ctypes.c_int]
    L.pzk_probe_ec_divmod.argtypes = [ctypes.c_int, ctypes.c_int, U64P, I32P, U64P, U64P, ctypes.c_int]
    return L


def pack(values, nwords, bits):
    """integers -> (len, nwords) little-endian words"""
    dt = np.uint32 if bits == 32 else np.uint64
    nbytes = nwords * bits // 8
    buf = b"".join(int(v).to_bytes(nbytes, "little") for v in values)
    return np.frombuffer(buf, dtype=dt).reshape(len(values), nwords).copy()


def unpack(arr):
    rows = np.ascontiguousarray(arr)
    n = rows.shape[-1] * rows.itemsize
    return [int.from_bytes(rows[i].tobytes(), "little") for i in range(rows.shape[0])] if n else []


def p32(a):
    return a.ctypes.data_as(U32P)


def p64(a):
    return a.ctypes.data_as(U64P)


def pint(a):
    return a.ctypes.data_as(I32P)


def first_mismatch(name, got, want, describe):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            n = sum(1 for x, y in zip(got, want) if x != y)
            return "%s: %d of %d cases differ; first case %d: %s\n  got  %#x\n  want %#x" % (
                name, n, len(want), i, describe(i), g, w)
    return ""


# ------------------------------------------------------------------------------------------------- fr
@pytest.mark.parametrize("op", A.FR_OPS)
def test_fr(probe, op):
    cases = A.fr_cases(op)
    assert len(cases) <= A.MAX_CASES
    a = pack([c[0] for c in cases], 8, 32)
    b = pack([c[1] for c in cases], 8, 32)
    out = np.zeros_like(a)
    rc = probe.pzk_probe_fr(A.FR_OPS.index(op), p32(a), p32(b) if op in A.FR_BINARY else None, p32(out), len(cases))
    assert rc == 0, "HIP error %d" % rc
    want = [A.fr_expected(op, x, y) for x, y in cases]
    rep = first_mismatch("fr_" + op, unpack(out), want, lambda i: "a=%#x b=%#x" % cases[i])
    assert not rep, rep


def test_fr_batch_inv(probe):
    cases = A.fr_batch_inv_cases()
    for m in range(1, 9):
        sub = [x for mm, x in cases if mm == m]
        x = pack([v for row in sub for v in row], 8, 32)
        out = np.zeros_like(x)
        rc = probe.pzk_probe_fr_batch_inv(p32(x), p32(out), len(sub), m)
        assert rc == 0, "HIP error %d" % rc
        flat = [v for row in sub for v in row]
        want = [A.fr_expected("inv", v) for v in flat]
        rep = first_mismatch("fr_batch_inv m=%d" % m, unpack(out), want,
                             lambda i: "row %s element %d" % ([hex(v) for v in sub[i // m]], i % m))
        assert not rep, rep


# ------------------------------------------------------------------------------------------------- fq
@pytest.mark.parametrize("op", A.FQ_OPS)
def test_fq(probe, op):
    cases = A.fq_cases(op)
    n = len(cases)
    assert n <= A.MAX_CASES
    a = pack([c.a for c in cases], 8, 32)
    b = pack([v for c in cases for v in c.b], 8, 32)
    k = pack([c.k for c in cases], 8, 32)
    out, canon = np.zeros_like(a), np.zeros_like(a)
    rc = probe.pzk_probe_fq(A.FQ_OPS.index(op), p32(a), p32(b), p32(k), p32(out), p32(canon), n)
    assert rc == 0, "HIP error %d" % rc
    exp = A.fq_expected(op, cases)
    got, gotc = unpack(out), unpack(canon)

    def describe(i):
        c = cases[i]
        s = "quad %d of its wave, a=%#x b=%s k=%#x" % (i % 16, c.a, [hex(v) for v in c.b], c.k)
        if op in A.FQ_NR:
            s += " row a=%s" % [hex(r.a) for r in cases[i & ~3:(i & ~3) + 4]]
        return s

    want = [w for _, w in exp]
    if exp[0][0] == "exact":
        rep = first_mismatch("fq_" + op, got, want, describe)
        assert not rep, rep
        return
    # non-canonical results: below the documented bound, congruent to the plain-integer product, equal to it after the
    # device's own canonicalisation (fq_canon twice, as the chain does), and equal, bit for bit, to the plain-integer
    # value of the Montgomery reduction without a final subtraction (arith_cases.mont_exact)
    for i, g in enumerate(got):
        bound = A.fq_result_bound(op, cases, i)
        assert g < bound, "fq_%s case %d: result %#x not below %#x; %s" % (op, i, g, bound, describe(i))
    rep = first_mismatch("fq_%s (mod p)" % op, [g % A.P for g in got], want, describe)
    assert not rep, rep
    rep = first_mismatch("fq_%s -> fq_canon" % op, gotc, want, describe)
    assert not rep, rep
    rep = first_mismatch("fq_%s (exact)" % op, got, [A.fq_exact(op, cases, i) for i in range(n)], describe)
    assert not rep, rep


# ------------------------------------------------------------------------------------------------- divisions
@pytest.mark.parametrize("op", ["divlu", "div_preinv"])
def test_div64(probe, op):
    cases = A.div64_cases()
    n = len(cases)
    u1, u0, v = (np.array([c[i] for c in cases], dtype=np.uint64) for i in range(3))
    q, r = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    rc = probe.pzk_probe_div64(["divlu", "div_preinv"].index(op), p64(u1), p64(u0), p64(v), p64(q), p64(r), n)
    assert rc == 0, "HIP error %d" % rc
    want = [divmod((c[0] << 64) | c[1], c[2]) for c in cases]
    got = [(int(q[i]) << 64) | int(r[i]) for i in range(n)]
    rep = first_mismatch(op + " (q : r)", got, [(a << 64) | b for a, b in want],
                         lambda i: "u1=%#x u0=%#x v=%#x" % cases[i])
    assert not rep, rep


def test_kd_div(probe):
    cases = A.kd_cases()
    n, sa, sb = len(cases), A.KD_STRIDE_A, A.KD_STRIDE_B
    assert n <= A.MAX_CASES
    a = pack([c[0] for c in cases], sa, 64)
    b = pack([c[2] for c in cases], sb, 64)
    na = np.array([c[1] for c in cases], dtype=np.intc)
    nb = np.array([c[3] for c in cases], dtype=np.intc)
    q, r = np.zeros_like(a), np.zeros_like(b)
    rc = probe.pzk_probe_kd_div(p64(a), pint(na), sa, p64(b), pint(nb), sb, p64(q), p64(r), n)
    assert rc == 0, "HIP error %d" % rc
    want = [divmod(c[0], c[2]) for c in cases]
    desc = lambda i: "na=%d nb=%d a=%#x b=%#x" % (cases[i][1], cases[i][3], cases[i][0], cases[i][2])
    rep = first_mismatch("kd_div quotient", unpack(q), [w[0] for w in want], desc)
    assert not rep, rep
    rep = first_mismatch("kd_div remainder", unpack(r), [w[1] for w in want], desc)
    assert not rep, rep


CURVE_IDS = [c["name"] for c in A.EC_CURVES]


@pytest.mark.parametrize("mod_n", [0, 1], ids=["p", "n"])
@pytest.mark.parametrize("cv", range(4), ids=CURVE_IDS)
def test_mp_divmod(probe, cv, mod_n):
    c = A.EC_CURVES[cv]
    assert probe.pzk_probe_ec_pwords(cv) == c["pwords"] and probe.pzk_probe_ec_nw(cv) == c["nw"]
    v = c["n"] if mod_n else c["p"]
    cases = A.ec_divmod_cases(cv, mod_n)
    n = len(cases)
    a = pack([x[0] for x in cases], 32, 64)
    na = np.array([x[1] for x in cases], dtype=np.intc)
    q = np.zeros_like(a)
    r = np.zeros((n, c["pwords"]), dtype=np.uint64)
    rc = probe.pzk_probe_ec_divmod(cv, mod_n, p64(a), pint(na), p64(q), p64(r), n)
    assert rc == 0, "HIP error %d" % rc
    want = [divmod(x[0], v) for x in cases]
    desc = lambda i: "na=%d a=%#x divisor=%#x" % (cases[i][1], cases[i][0], v)
    rep = first_mismatch("mp_divmod quotient", unpack(q), [w[0] for w in want], desc)
    assert not rep, rep
    rep = first_mismatch("mp_divmod remainder", unpack(r), [w[1] for w in want], desc)
    assert not rep, rep


# ------------------------------------------------------------------------------------------------- EC fields
@pytest.mark.parametrize("op", A.EC_OPS)
@pytest.mark.parametrize("mod_n", [0, 1], ids=["ModP", "ModN"])
@pytest.mark.parametrize("cv", range(4), ids=CURVE_IDS)
def test_ec_field(probe, cv, mod_n, op):
    c = A.EC_CURVES[cv]
    m, nw = (c["n"] if mod_n else c["p"]), c["nw"]
    cases = A.ec_field_cases(cv, mod_n, op)
    n = len(cases)
    a = pack([x[0] for x in cases], nw, 32)
    b = pack([x[1] for x in cases], nw, 32)
    out = np.zeros_like(a)
    rc = probe.pzk_probe_ec_field(cv, mod_n, A.EC_OPS.index(op), p32(a), p32(b), p32(out), n)
    assert rc == 0, "HIP error %d" % rc
    want = [A.ec_field_expected(m, nw, op, x, y) for x, y in cases]
    rep = first_mismatch("m_%s %s %s" % (op, c["name"], "ModN" if mod_n else "ModP"), unpack(out), want,
                         lambda i: "a=%#x b=%#x" % cases[i])
    assert not rep, rep
