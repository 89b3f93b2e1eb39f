"""GPU: the ECDSA point chains on steered scalars (tests/ecdsa_cases.py; the rows are pinned on the oracle and the
constraint checker by tests/test_ecdsa_cases.py).

Per curve one instance and one witness_batch_host call over plain, crafted, plain, crafted, ..., plain, so that the
64-lane groups of k_ec_inv straddle rows with zero differences and rows without. Every row is compared with the
oracle element for element:

  rows that verify          status 0, the witness identical
  oracle code 15 or 16      the same status; a code-16 row (only the last === fails, everything before it is
                            defined) also identical element for element
  F4 (u1 G = +-u2 Q)        a non-zero status, and the plain rows next to it exact

and the P-256 batch once more through the register_sig20 O2-shaped map, against the gather of the O0 rows."""
import numpy as np
import pytest

from pzkwit import inputs as I, native, symmap

import ecdsa_cases as E
import test_gpu_ecdsa  # noqa: F401  (the ECDSA region names of mismatch_report)
from test_gpu_register import mismatch_report, region_table

pytestmark = pytest.mark.gpu


class Run:
    """one curve's call: the rows, the device's witnesses and statuses, and a cache of oracle witnesses of the two
    plain rows (a crafted row's reference is computed where it is compared, and dropped)"""

    def __init__(self, oracle, sig):
        self.sig, self.params = sig, I.instance_params(sig)
        pps, self.labels = E.batch(sig)
        self.rows = np.stack([I.pack_register_inputs(pp, self.params) for pp in pps])
        self.rows.setflags(write=False)
        inst = native.Instance(native.PZK_CIRCUIT_REGISTER, 0, self.params)
        self.wit, self.st = inst.witness_batch_host(self.rows)
        print("sig %d statuses %s" % (sig, self.st.tolist()))
        self.regions = region_table(self.params)
        self.oracle, self.prm = oracle, oracle.register_params(**self.params)
        self._plain = {}

    def reference(self, b):
        lab = self.labels[b]
        if isinstance(lab, E.Case):
            return self.oracle.register_witness(self.prm, self.rows[b])
        if lab not in self._plain:
            rc, w = self.oracle.register_witness(self.prm, self.rows[b])
            w.setflags(write=False)
            self._plain[lab] = (rc, w)
        return self._plain[lab]


@pytest.fixture(scope="module")
def runs(oracle):
    """sig -> its Run, one call per curve; one curve's witnesses are held at a time (4 to 8 GB), so the tests below
    are ordered by curve"""
    held = {}

    def get(sig):
        if sig not in held:
            held.clear()
            held[sig] = Run(oracle, sig)
        return held[sig]

    yield get
    held.clear()


def test_steered_rows_through_an_o2_shaped_map(runs):
    """the emitters' kept-element paths on the same rows: mapped rows == the O0 device rows of the same call at the
    map's indices, merged signals through their class's first signal, and the same statuses"""
    run = runs(20)
    txt = symmap.sym_text_wit(symmap.load_shape("register_sig20", 2))
    inv = symmap.parse_sym(txt)
    mp = native.Instance(native.PZK_CIRCUIT_REGISTER, 0, run.params, sym=txt)
    assert mp.witness_size == inv.shape[0]
    wm, sm = mp.witness_batch_host(run.rows)
    assert sm.tolist() == run.st.tolist()
    for b in range(run.rows.shape[0]):
        bad = np.nonzero((wm[b] != run.wit[b][inv]).any(axis=1))[0]
        assert bad.size == 0, "row %d (%s): %d mapped elements differ (first k=%d, O0 %d)" % (
            b, run.labels[b], bad.size, bad[0], inv[bad[0]])


GROUPS = [(sig, g) for sig in E.SIGS for g in E.groups(sig)]


@pytest.mark.parametrize("sig,group", GROUPS, ids=["sig%d-%s" % sg for sg in GROUPS])
def test_steered_rows_match_oracle(runs, sig, group):
    """the group's crafted rows and the plain row before each; the last group also takes the batch's last row"""
    run = runs(sig)
    mine = [b for b, lab in enumerate(run.labels) if isinstance(lab, E.Case) and lab.group == group]
    rows = sorted({b - 1 for b in mine} | set(mine) | ({len(run.labels) - 1} if group == E.groups(run.sig)[-1] else set()))
    problems = []
    for b in rows:
        lab = run.labels[b]
        rc, ref = run.reference(b)
        st = int(run.st[b])
        if not isinstance(lab, E.Case):
            name, want, exact = "plain", 0, True
        else:
            name, want, exact = lab.name, lab.code, lab.code in (0, E.ST_ECDSA_R)
            assert (rc == want) if want is not None else rc != 0, (name, rc)  # as test_ecdsa_cases.py pinned it
        rep = mismatch_report(ref, run.wit[b], run.regions) if exact else ""
        print("row %d %s: status %d (oracle %d)%s" % (b, name, st, rc, ", " + rep.splitlines()[0] if rep else ""))
        if want is None:
            if st == 0:
                problems.append("row %d %s: status 0, the oracle rejects it with %d" % (b, name, rc))
        elif st != want:
            problems.append("row %d %s: status %d, expected %d" % (b, name, st, want))
        if rep:
            problems.append("row %d %s: %s" % (b, name, rep))
    assert not problems, "\n".join(problems)
