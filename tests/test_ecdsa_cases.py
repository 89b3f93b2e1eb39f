"""CPU checks of tests/ecdsa_cases.py: the committed rows of every curve reach every branch label of the point chains
(a condition on the case list), and the reference is pinned on them before the device is compared with it
(tests/test_gpu_ecdsa_cases.py): a row built to verify is accepted by the oracle (code 0) and by the constraint
checker, with r equal to independent curve arithmetic; a failing row carries exactly its check site's code and breaks
at least one constraint. F4 (u1 G = +-u2 Q) only has to fail: the oracle's code there is the first site in its own
evaluation order."""
import pytest

from pzkwit import inputs as I

import ecdsa_cases as E
from test_r1cs import _ok, expected_uncovered

pyr1cs = pytest.importorskip("pyr1cs")


@pytest.mark.parametrize("sig", E.SIGS)
def test_cases_reach_every_chain_feature(sig):
    seen = {}
    for c in E.cases(sig):
        for f in E.chain_features(sig, c.u1, c.u2):
            assert f in E.FEATURES, f
            seen.setdefault(f, []).append(c.name)
    print("\n".join("%-28s %s" % (f, ", ".join(seen.get(f, []))) for f in E.FEATURES))
    missing = [f for f in E.FEATURES if f not in seen]
    assert not missing, "sig %d: no case reaches %s" % (sig, missing)
    # the forwarded results k_ec_final has to resolve: a table entry, the key, the dummy
    byname = {c.name: c for c in E.cases(sig)}
    assert "gm_result_forwarded" in E.chain_features(sig, *_u(next(c for n, c in byname.items() if n.startswith("V6"))))
    assert "sm_result_is_Q" in E.chain_features(sig, *_u(byname["V1_u2_1"]))
    assert "sm_result_dummy" in E.chain_features(sig, *_u(byname["F2_r_0"]))


def _u(c):
    return c.u1, c.u2


def test_case_lists():
    """P-256 carries every row; the recorded scalars are those of the packed signature"""
    names = [c.name for c in E.cases(20)]
    assert len(names) == len(set(names)) == 21
    for sig in E.SIGS:
        cs = E.cases(sig)
        assert 9 <= len(cs) <= 24
        for c in cs:
            assert (c.u1, c.u2) == E.scalars(sig, E.digest_int(c.pp, sig), *c.pp["sig"]), c.name
        pps, labels = E.batch(sig)
        assert len(pps) == 2 * len(cs) + 1 and labels[0] in (0, 1) and labels[-1] in (0, 1)
        assert [x for x in labels if isinstance(x, E.Case)] == cs and all(isinstance(x, E.Case) for x in labels[1::2])


def _oracle_row(oracle, sig, pp):
    params = I.instance_params(sig)
    return oracle.register_witness(oracle.register_params(**params), I.pack_register_inputs(pp, params))


@pytest.mark.parametrize("sig", E.SIGS)
def test_plain_rows_verify(oracle, sig):
    for pp in E.plain_passports(sig):
        rc, _ = _oracle_row(oracle, sig, pp)
        assert rc == 0


@pytest.mark.parametrize("sig,name", [(s, c.name) for s in E.SIGS for c in E.cases(s) if c.valid])
def test_valid_row_is_accepted(oracle, sig, name):
    c = next(c for c in E.cases(sig) if c.name == name)
    curve = I.EC_CURVES[sig]
    r, s = c.pp["sig"]
    assert curve.add(curve.mul(c.u1), curve.mul(c.u2, c.pp["n"]))[0] % curve.n == r
    rc, w = _oracle_row(oracle, sig, c.pp)
    assert rc == 0, (name, rc)
    _ok(pyr1cs.check_register(w, **I.instance_params(sig)), expected_uncovered(sig))


@pytest.mark.parametrize("sig,name", [(s, c.name) for s in E.SIGS for c in E.cases(s) if not c.valid])
def test_failing_row_carries_its_code(oracle, sig, name):
    c = next(c for c in E.cases(sig) if c.name == name)
    rc, w = _oracle_row(oracle, sig, c.pp)
    print("sig %d %s: oracle code %d" % (sig, name, rc))
    if c.code is None:
        assert rc != 0
    else:
        assert rc == c.code, (name, rc, c.code)
    rc2, rep = pyr1cs.check_register(w, **I.instance_params(sig))
    assert rc2 != 0 and rep["n_failed"] > 0, rep
