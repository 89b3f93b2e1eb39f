"""GPU: QueryIdentity's comparisons, dates and SMT proofs on steered rows (tests/query_cases.py; the rows are pinned on
the oracle and the constraint checker by tests/test_query_cases.py).

Per document type one instance and one witness_batch_host call over plain, crafted, plain, crafted, ..., plain. The
batch length is no multiple of 8 or 32, so the shared inversions of k_qry_prep (8 witnesses) and k_smt_prep (32)
straddle crafted and plain rows and end in a partly live group. Every row is compared with the oracle:

  oracle code 0, 19, 20     the same status and the witness identical, element for element (a failing
                            ForceEqualIfEnabled or DateDecoder leaves every signal defined)
  domain (an input = 2^64)  the status DESIGN.md §5 defines: 64 (PZK_ST_INPUT_RANGE), or the smaller code of a check that
                            fails on the low 64 bits as well (the date decoder's 20); the witness is unspecified;
                            the plain rows on both sides exact

and the TD3 batch again through the O2-shaped query map (against the gather of the O0 rows) and, without the domain
rows (a limb >= 2^64 has no packed form), through the packed entry point."""
import numpy as np
import pytest

from pzkwit import native, query as Q, symmap

import query_cases as C

pytestmark = pytest.mark.gpu


def _int(e):
    return int.from_bytes(e.tobytes(), "little")


class Run:
    """one document type's call: the rows, the device's witnesses and statuses, and the oracle's witnesses of the two
    plain rows (a crafted row's reference is computed where it is compared, and dropped)"""

    def __init__(self, oracle, td1):
        self.td1, self.oracle = td1, oracle
        inps, self.labels = C.batch(td1)
        packed = {}  # the two plain rows are packed once
        self.rows = np.stack([packed.setdefault(id(inp), Q.pack(inp)) for inp in inps])
        self.rows.setflags(write=False)
        assert self.rows.shape[0] % 8 and self.rows.shape[0] % 32
        self.inst = native.Instance(native.PZK_CIRCUIT_QUERY, 80, {"doc": 1} if td1 else None)
        self.wit, self.st = self.inst.witness_batch_host(self.rows)
        print("td1 %d statuses %s" % (td1, self.st.tolist()))
        self._plain = {}

    def reference(self, b):
        lab = self.labels[b]
        if isinstance(lab, C.Case):
            return self.oracle.query_witness(self.rows[b], td1=self.td1)
        if lab not in self._plain:
            rc, w = self.oracle.query_witness(self.rows[b], td1=self.td1)
            w.setflags(write=False)
            self._plain[lab] = (rc, w)
        return self._plain[lab]


@pytest.fixture(scope="module")
def runs(oracle):
    """td1 -> its Run, one call per document type; one type's witnesses are held at a time (1 GB), so the tests below
    are ordered by type"""
    held = {}

    def get(td1):
        if td1 not in held:
            for r in held.values():
                r.inst.close()
            held.clear()
            held[td1] = Run(oracle, td1)
        return held[td1]

    yield get
    for r in held.values():
        r.inst.close()
    held.clear()


def test_steered_rows_through_an_o2_shaped_map(runs):
    """the emitters' kept-element paths on the same rows: mapped rows == the O0 device rows of the same call at the
    map's indices, and the same statuses"""
    run = runs(False)
    txt = symmap.sym_text_wit(symmap.load_shape("query", 2))
    inv = symmap.parse_sym(txt)
    mp = native.Instance(native.PZK_CIRCUIT_QUERY, 80, sym=txt)
    try:
        assert mp.witness_size == inv.shape[0]
        wm, sm = mp.witness_batch_host(run.rows)
    finally:
        mp.close()
    assert sm.tolist() == run.st.tolist()
    for b in range(run.rows.shape[0]):
        bad = np.nonzero((wm[b] != run.wit[b][inv]).any(axis=1))[0]
        assert bad.size == 0, "row %d (%s): %d mapped elements differ (first k=%d, O0 %d)" % (
            b, run.labels[b], bad.size, bad[0], inv[bad[0]])


def test_steered_rows_packed(runs):
    """pzk_witness_batch_host_packed over the packed rows == the unpacked call, in every witness byte and status"""
    run = runs(False)
    keep = [b for b, lab in enumerate(run.labels) if not (isinstance(lab, C.Case) and lab.group == "domain")]
    assert len(keep) % 8 and len(keep) % 32
    packed, pst = native.pack_inputs(run.rows[keep], None, native.PZK_CIRCUIT_QUERY, 80)
    assert (pst == 0).all(), [str(run.labels[keep[i]]) for i in np.nonzero(pst)[0]]
    got, got_st = run.inst.witness_batch_host_packed(packed)
    assert got_st.tolist() == run.st[keep].tolist()
    for i, b in enumerate(keep):
        bad = np.nonzero((got[i] != run.wit[b]).any(axis=1))[0]
        assert bad.size == 0, "row %d (%s): %d elements differ from the unpacked call (first %d)" % (
            b, run.labels[b], bad.size, bad[0])


CASES = [(td1, g) for td1 in (False, True) for g in C.GROUPS]


@pytest.mark.parametrize("td1,group", CASES, ids=["%s-%s" % ("td1" if t else "td3", g) for t, g in CASES])
def test_steered_rows_match_oracle(runs, td1, group):
    """the group's crafted rows and the plain row before each; the last group also takes the batch's last row"""
    run = runs(td1)
    mine = [b for b, lab in enumerate(run.labels) if isinstance(lab, C.Case) and lab.group == group]
    rows = sorted({b - 1 for b in mine} | set(mine) | ({len(run.labels) - 1} if group == C.GROUPS[-1] else set()))
    problems = []
    for b in rows:
        lab = run.labels[b]
        rc, ref = run.reference(b)
        st = int(run.st[b])
        if isinstance(lab, C.Case):
            name, want, exact = lab.name, lab.device, lab.group != "domain"
            assert rc == lab.code, (name, rc)  # as test_query_cases.py pinned it
        else:
            name, want, exact = "plain", 0, True
            assert rc == 0
        bad = np.nonzero((ref != run.wit[b]).any(axis=1))[0] if exact else np.zeros(0, dtype=int)
        print("row %d %s: status %d (oracle %d), %d elements differ" % (b, name, st, rc, bad.size))
        if st != want:
            problems.append("row %d %s: status %d, expected %d" % (b, name, st, want))
        if bad.size:
            problems.append("row %d %s: %d elements differ, first %d: oracle %d, device %d" % (
                b, name, bad.size, bad[0], _int(ref[bad[0]]), _int(run.wit[b][bad[0]])))
    assert not problems, "\n".join(problems)
