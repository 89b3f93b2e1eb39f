"""CPU checks of tests/query_cases.py: the committed rows of both document types reach every decision label of the
device's comparison, date and SMT shortcuts (a condition on the case list), and the reference is pinned on them
before the device is compared with it (tests/test_gpu_query_cases.py): every row carries its stated code on the
oracle; a code-0 row satisfies and covers every constraint of the independent checker and its public outputs equal
independent math; a failing row is named by the checker at its template; and every row differs from its unedited
make_query query only in the inputs its case names, plus the root."""
import os
import re

import pytest

from pzkwit import query as Q

import query_cases as C

pyr1cs = pytest.importorskip("pyr1cs")

TD = [False, True]
IDS = ["td3", "td1"]
# the constraint a failing row violates (template, reference line), as the checker names it
FAIL_CONSTRAINT = {C.ST_QUERY: ("ForceEqualIfEnabled", 42), C.ST_DATE: ("DateDecoder", 22), C.ST_NUM2BITS: ("Num2Bits", 26)}


def test_lane_segment_constant_is_the_header_s():
    """NL, the levels per lane of k_smt_prep, decides which masks sit on a segment edge"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(Q.__file__))), "csrc")
    text = open(os.path.join(csrc, "layout.hpp")).read()
    levels = int(re.search(r"constexpr int SMT_LEVELS = (\d+);", text).group(1))
    lanes = int(re.search(r"constexpr int SMT_PREP_LANES = (\d+);", text).group(1))
    assert (levels, lanes) == (C.SMT_LEVELS, C.SMT_PREP_LANES) and C.NL == levels // lanes == 10
    assert "NL = SMT_LEVELS / SMT_PREP_LANES" in open(os.path.join(csrc, "regcore.hpp")).read()


@pytest.mark.parametrize("td1", TD, ids=IDS)
def test_cases_reach_every_feature(td1):
    seen = {}
    for c in C.cases(td1):
        fs = C.features(c.inp, c.info)
        assert (c.group == "domain") == (not fs), c.name
        for f in fs:
            assert f in C.FEATURES, f
            seen.setdefault(f, []).append(c.name)
    print("\n".join("%-24s %s" % (f, ", ".join(seen.get(f, []))) for f in C.FEATURES))
    missing = [f for f in C.FEATURES if f not in seen]
    assert not missing, "no case reaches %s" % missing
    # what make_query's own draws reach: none of the edges but a few date orders
    plain = set().union(*(C.features(inp, info) for inp, info in C.plain_queries(td1)))
    assert not any(f.startswith(("smt_interior", "smt_zero", "cmp0_carry", "cmp2_carry")) or "_false_" in f or
                   "_100" in f for f in plain), sorted(plain)


@pytest.mark.parametrize("td1", TD, ids=IDS)
def test_case_lists(td1):
    cs = C.cases(td1)
    assert len(cs) <= 120 and [c.name for c in cs] == [c.name for c in C.cases(not td1)]
    assert {c.group for c in cs} == set(C.GROUPS) and all(c.info["td1"] == td1 for c in cs)
    by = {c.name: c for c in cs}
    for z in (0, C.NL - 1, C.NL, 2 * C.NL - 1, 31, 32, 63, 64, 77):  # exactly one empty sibling inside the path
        sib = by["smt_zero_%d" % z].inp["idStateSiblings"]
        assert [i for i in range(C.insertion_level(sib)) if sib[i] == 0] == [z]
    assert [i for i, s in enumerate(by["smt_only_78"].inp["idStateSiblings"]) if s] == [78]
    assert [i for i, s in enumerate(by["smt_zero_1_to_77"].inp["idStateSiblings"]) if s] == [0, 78]
    assert [i for i, s in enumerate(by["smt_alternating_from_0"].inp["idStateSiblings"]) if s] == list(range(1, 78, 2))
    assert [i for i, s in enumerate(by["smt_alternating_from_1"].inp["idStateSiblings"]) if s] == list(range(0, 79, 2))
    for want in (0, 1):
        c = by["smt_keybit_%d" % want]
        assert (c.info["key"] >> C.insertion_level(c.inp["idStateSiblings"])) & 1 == want
    for b in range(18):  # a selector bit alone, every condition true
        c = by["select_bit_%d" % b]
        assert c.inp["selector"] == 1 << b and all(C.conditions(c.inp, c.info))
    for groups in (C.GROUPS, C.GROUPS[:-1]):  # the whole batch, and the one that can be packed
        inps, labels = C.batch(td1, groups)
        n = len(inps)
        assert n % 8 and n % 32, n  # the shared inversions' groups (8, 32 witnesses) end partly live
        assert labels[0] in (0, 1) and labels[-1] in (0, 1) and all(isinstance(x, C.Case) for x in labels[1::2])
        assert [x for x in labels if isinstance(x, C.Case)] == [c for c in cs if c.group in groups]


@pytest.mark.parametrize("td1", TD, ids=IDS)
def test_date_helper_rebuilds_what_make_query_built(td1):
    """writing a DG1 date's own bytes back changes nothing: bits, commitment, field and root as make_query made them"""
    inp, info = C.plain_queries(td1)[0]
    for which in ("birth", "exp"):
        inp2, info2 = dict(inp), dict(info)
        date = info["fields"][C.DATE_FIELD[which]].to_bytes(6, "big")
        C.set_dg1_date(inp2, info2, which, date)
        assert inp2 == inp and info2 == info


@pytest.mark.parametrize("td1", TD, ids=IDS)
def test_plain_rows_pass(oracle, td1):
    for inp, info in C.plain_queries(td1):
        rc, _ = oracle.query_witness(Q.pack(inp), td1=td1)
        assert rc == 0


@pytest.mark.parametrize("group", C.GROUPS)
@pytest.mark.parametrize("td1", TD, ids=IDS)
def test_rows_carry_their_code(oracle, td1, group):
    nout = 10 if td1 else 9
    problems = []
    for c in (c for c in C.cases(td1) if c.group == group):
        rc, w = oracle.query_witness(Q.pack(c.inp), td1=td1)
        crc, rep = pyr1cs.check_query(w, td1=td1)
        print("%-34s oracle %2d, checker %d failed, %d uncovered %s:%d" % (
            c.name, rc, rep["n_failed"], rep["n_uncovered"], rep["first_template"], rep["first_line"]))
        if rc != c.code:
            problems.append("%s: oracle code %d, stated %d" % (c.name, rc, c.code))
        elif rc == 0:
            if crc != 0 or rep["n_failed"] or rep["n_uncovered"] or rep["size_walked"] != w.shape[0]:
                problems.append("%s: the checker rejects an accepted row: %s" % (c.name, rep))
            if [oracle.from_elem(w[1 + i]) for i in range(nout)] != Q.public_outputs(c.inp, c.info):
                problems.append("%s: public outputs differ from independent math" % c.name)
        else:
            tmpl, line = FAIL_CONSTRAINT[rc]
            if not (crc == 1 and rep["n_failed"] >= 1 and rep["first_template"].startswith(tmpl) and
                    rep["first_line"] == line):
                problems.append("%s: the checker does not name %s:%d: %s" % (c.name, tmpl, line, rep))
            if rc == C.ST_QUERY and rep["n_failed"] != 1:
                problems.append("%s: %d failed constraints, expected one" % (c.name, rep["n_failed"]))
        if group != "domain" and c.code in (0, C.ST_QUERY):  # the status k_qry_prep restates from the conditions
            failing = any(not v and (c.inp["selector"] >> (8 + k)) & 1 for k, v in enumerate(C.conditions(c.inp, c.info)))
            if failing != (c.code == C.ST_QUERY):
                problems.append("%s: the restated conditions disagree with the stated code" % c.name)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("td1", TD, ids=IDS)
def test_rows_differ_only_in_their_stated_edits(td1):
    for c in C.cases(td1):
        inp, info = C.unedited(c, td1)
        changed = {k for k in inp if inp[k] != c.inp[k]}
        extra = changed - c.edits - {"idStateRoot"}
        assert not extra, (c.name, sorted(extra))
        assert bool(changed) == bool(c.edits), c.name
        root_follows = bool(changed & {"timestamp", "identityCounter", "idStateSiblings", "dg1"})
        assert ("idStateRoot" in changed) == root_follows, c.name
        assert info["key"] == c.info["key"] and info["nullifier"] == c.info["nullifier"]
