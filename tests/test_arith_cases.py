"""CPU checks of tests/arith_cases.py: the lane-level models agree with plain integers on every committed case, the
cases stay inside the callees' contracts, and every branch event a model can reach is reached by at least MIN_HITS
cases of the committed seed (the counts are printed; run with -s, or read them in the assertion message). The GPU
counterpart, tests/test_gpu_arith.py, runs the same cases through the device functions."""
import collections

import pytest

import arith_cases as A

MIN_HITS = 8


def _report(name, counts, wanted):
    line = "%s: %s" % (name, ", ".join("%s=%d" % (e, counts.get(e, 0)) for e in wanted))
    print(line)
    return line


def _assert_covered(name, counts, wanted, unreachable=()):
    line = _report(name, counts, wanted)
    for e in wanted:
        if e in unreachable:
            assert counts.get(e, 0) == 0, "%s: '%s' is listed as unreachable but was reached\n%s" % (name, e, line)
        else:
            assert counts.get(e, 0) >= MIN_HITS, "%s: event '%s' reached by fewer than %d cases\n%s" % (
                name, e, MIN_HITS, line)
    extra = set(counts) - set(wanted)
    assert not extra, "%s: the model reached events listed as unreachable: %s" % (name, sorted(extra))


def test_constants():
    from pzkwit import field
    assert A.P == field.P
    assert A.from_digits(A.PD) == A.P and A.R1 == (1 << 256) % A.P


@pytest.mark.parametrize("op", A.FR_OPS)
def test_fr_cases_inside_contract(op):
    cases = A.fr_cases(op)
    assert 0 < len(cases) <= A.MAX_CASES
    lim = (1 << 128) if op == "from_i128" else A.FR_LIMIT[op]
    for a, b in cases:
        assert 0 <= a < lim and 0 <= b < lim
        assert 0 <= A.fr_expected(op, a, b) < A.P
    assert cases == A.fr_cases(op), "the case list must be reproducible"


def test_fr_batch_inv_cases():
    cases = A.fr_batch_inv_cases()
    assert all(1 <= m <= 8 and len(x) == m and all(0 <= v < A.P for v in x) for m, x in cases)
    assert any(all(v == 0 for v in x) for _, x in cases) and any(x[0] == 0 and any(x[1:]) for _, x in cases)


@pytest.mark.parametrize("op", A.FQ_OPS)
def test_fq_models_and_coverage(op):
    cases = A.fq_cases(op)
    assert 0 < len(cases) <= A.MAX_CASES
    if op in A.FQ_NR:
        assert len(cases) % 4 == 0
    exp = A.fq_expected(op, cases)
    counts = collections.Counter()
    for i, c in enumerate(cases):
        # contracts
        if op in ("mul", "mul64"):
            assert c.a < 2 * A.P and c.b[0] < 2 * A.P
        elif op == "mulq":
            assert (c.a <= A.LIM22 and c.b[0] <= A.LIM22) or (c.a < A.R and c.b[0] == A.R2)
        elif op in A.FQ_NR:
            assert c.a <= A.LIM22 and c.b[0] <= A.LIM22 and c.b[1] < A.P and c.b[2] < A.P and c.k < A.P
        elif op == "canon":
            assert c.a < 2 * A.P
        elif op == "add_raw":
            assert c.a + c.b[0] < A.R
        else:
            assert c.a < A.R
        value, ev = A.fq_model(op, cases, i)
        kind, want = exp[i]
        if kind == "mod":
            # the plain-integer value of the non-canonical result itself, its residue and its documented bound
            assert value == A.fq_exact(op, cases, i), (op, i, hex(c.a), hex(c.b[0]), hex(value))
            assert value % A.P == want and value < A.fq_result_bound(op, cases, i), (op, i, hex(c.a), hex(value))
        else:
            assert value == want, (op, i, hex(c.a), hex(value), hex(want))
        counts.update(ev)
    # gen0 / prop1 / gen3 / prop3 / pend1 of the carry settles: unreachable, see arith_cases.py
    _assert_covered("fq_" + op, counts, A.fq_events(op))


@pytest.mark.parametrize("op", A.FQ_OPS)
def test_fq_neighbour_layout(op):
    """The committed list ends with 17 whole waves in which, for every quad position i of a wave (i = 3, 7, 11 cross a
    row boundary, i = 15 the wave boundary), quad i holds a case that by the model raises a carry or borrow inside the
    quad, and quad i + 1 a case that a stray carry or borrow from outside would change in every digit."""
    cases = A.fq_cases(op)
    start = len(cases) - A.FQ_LAYOUT
    assert start > 0 and start % 16 == 0
    for i in range(16):
        at = start + 16 * i + i
        assert at % 16 == i and (at + 1) % 16 == (i + 1) % 16
        ev = A.fq_model(op, cases, at)[1]
        nxt = cases[at + 1]
        if op in ("canon", "geq_p"):
            # the borrow leaves the top lane (a < p); the neighbour's lowest digit is p's, so it would pass a borrow on
            assert ev & {"gen3", "prop3"}, (op, i, sorted(ev))
            assert A.digits(nxt.a)[0] == A.PD[0] and nxt.a >= A.P, (op, i, hex(nxt.a))
            continue
        if op == "add_raw":
            assert "gen0" in ev and {"prop1", "prop2"} <= ev, (op, i, sorted(ev))
            result = nxt.a + nxt.b[0]
        else:
            assert ev & {"gen1", "gen2", "prop2"}, (op, i, sorted(ev))
            result = A.fq_exact(op, cases, at + 1)
            assert result == A.fq_model(op, cases, at + 1)[0]
        assert A.digits(result)[:3] == [A.M64] * 3, (op, i, hex(result))


def test_div64_models_and_coverage():
    cases = A.div64_cases()
    assert 0 < len(cases) <= A.MAX_CASES
    cl, cp = collections.Counter(), collections.Counter()
    for u1, u0, v in cases:
        q, r = divmod((u1 << 64) | u0, v)
        ql, rl, ev = A.model_divlu(u1, u0, v)
        assert (ql, rl) == (q, r), (hex(u1), hex(u0), hex(v))
        cl.update(ev)
        qp, rp, ev = A.model_div_preinv(u1, u0, v)
        assert (qp, rp) == (q, r), (hex(u1), hex(u0), hex(v))
        cp.update(ev)
    _assert_covered("divlu", cl, A.DIVLU_EVENTS)
    _assert_covered("div_preinv", cp, A.PREINV_EVENTS)


def _knuth_counts(cases, divisor_of):
    counts = collections.Counter()
    for c in cases:
        a, na, b, nb = divisor_of(c)
        q, r, ev = A.model_knuth_d(a, na, b, nb)
        assert (q, r) == divmod(a, b), (hex(a), na, hex(b), nb)
        counts.update(ev)
    return counts


def test_kd_div_models_and_coverage():
    cases = A.kd_cases()
    assert 0 < len(cases) <= A.MAX_CASES
    assert {nb for _, _, _, nb in cases} == set(A.KD_NB)
    for a, na, b, nb in cases:
        assert 2 <= nb <= A.KD_STRIDE_B and nb <= na < A.KD_STRIDE_A and a < (1 << (64 * na)) and b >> (64 * (nb - 1))
    _assert_covered("kd_div", _knuth_counts(cases, lambda c: c), A.KD_EVENTS)


@pytest.mark.parametrize("mod_n", [0, 1], ids=["p", "n"])
@pytest.mark.parametrize("cv", range(4), ids=[c["name"] for c in A.EC_CURVES])
def test_mp_divmod_models_and_coverage(cv, mod_n):
    c = A.EC_CURVES[cv]
    v = c["n"] if mod_n else c["p"]
    cases = A.ec_divmod_cases(cv, mod_n)
    assert 0 < len(cases) <= A.MAX_CASES
    assert all(c["pwords"] <= na <= 31 and a < (1 << (64 * na)) for a, na in cases)
    counts = _knuth_counts(cases, lambda x: (x[0], x[1], v, c["pwords"]))
    # what this divisor's top words rule out (reasons in arith_cases.knuth_reachable); e.g. secp256r1's p has a zero
    # second word, so its refinement loop never fires and add-back alone fixes every over-estimate
    unreachable = set(A.KD_EVENTS) - A.knuth_reachable(v, c["pwords"])
    if not mod_n and cv == 0:
        assert unreachable == {"qmax_ovf", "ref1", "ref2", "ref_ovf"}
    _assert_covered("mp_divmod %s %s" % (c["name"], "n" if mod_n else "p"), counts, A.KD_EVENTS, unreachable)


@pytest.mark.parametrize("cv", range(4), ids=[c["name"] for c in A.EC_CURVES])
def test_ec_field_cases_inside_contract(cv):
    c = A.EC_CURVES[cv]
    for mod_n in (0, 1):
        m = c["n"] if mod_n else c["p"]
        for op in A.EC_OPS:
            cases = A.ec_field_cases(cv, mod_n, op)
            assert 0 < len(cases) <= A.MAX_CASES
            assert all(0 <= a < m and 0 <= b < m for a, b in cases)


@pytest.mark.parametrize("limbs", [32, 31])
def test_barrett_model_coverage(limbs):
    found = A.barrett_search(limbs)
    counts = {"corr%d" % k: len(v) for k, v in found.items()}
    for k, rows in found.items():
        for n, sig in rows:
            assert A.model_barrett(n, sig, sig) == k
            assert 1 <= n >> (64 * (limbs - 1)) <= 5 and sig < A.B64 ** limbs
    _assert_covered("barrett %d limbs" % limbs, counts, ["corr0", "corr1", "corr2"])


def test_rsa_knuth_addback_row_found():
    row = A.rsa_knuth_addback_row()
    assert row is not None
    n, sig = row
    assert sig >= n and A.model_barrett(n, sig, sig) is None
