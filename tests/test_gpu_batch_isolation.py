"""GPU: rows of one batch do not reach each other through the inversions that a workgroup's witnesses share.

k_smt_prep, k_bjj_core (the scratch core, the default), k_rsa_inv and k_qry_prep multiply the non-zero values of
several witnesses into one total and invert it once per workgroup. Rows and expected codes come from
tests/test_batch_isolation.py, which proves them on the oracle. Here:

a, b  batch sizes that leave those workgroups partly live, every row (query) / the rows at the workgroup edges
      (register) element for element against the oracle;
c, d  one row of the batch carries an input element >= p (or past its bit width): that row is flagged as DESIGN.md §5
      promises, and EVERY other row of the batch is bit-exact against the oracle with the oracle's status;
e     the same through an O2-shaped mapped instance.

Nothing is asserted about the witness of a poisoned row: the oracle is undefined there."""
import numpy as np
import pytest

from pzkwit import inputs as I, native, symmap
from test_batch_isolation import (POISON, POISONED_ROW, QUERY_CASES, QUERY_ELEMS, REGISTER_CALL, ST_INPUT_RANGE, poison,
                                  query_base, register_base, register_poisoned)
from test_gpu_register import mismatch_report, region_table

pytestmark = pytest.mark.gpu

# Witnesses that share one inversion (one workgroup), by kernel:
#   k_qry_prep  QP_WAVES = 8                                        (query.hpp)
#   k_bjj_core  64 * BJJ_WG_WAVES / BJJ_SEGS = 64 * 4 / 16 = 16     (regcore.hpp; BJJ_SEGS 16 is launch_bjj_core's default)
#   k_smt_prep  64 * SMT_PREP_WAVES / SMT_PREP_LANES = 64 * 4 / 8 = 32  (regcore.hpp, layout.hpp)
#   k_rsa_inv   RI_WAVES = 8                                        (regcore.hpp; register only)
# A change of one of these constants moves the edges below.
QRY_WG, BJJ_WG, SMT_WG, RSA_WG = 8, 16, 32, 8
QUERY_SIZES = sorted({1} | {wg + d for wg in (QRY_WG, BJJ_WG, SMT_WG) for d in (-1, 0, 1)})
assert QUERY_SIZES == [1, 7, 8, 9, 15, 16, 17, 31, 32, 33]
# the last row of a full k_rsa_inv / k_bjj_core workgroup and the lone row of the next one
REGISTER_EDGES = sorted({0} | {wg + d for wg in (RSA_WG, BJJ_WG) for d in (-1, 0)})
assert REGISTER_EDGES == [0, 7, 8, 15, 16]


@pytest.fixture(scope="module")
def qref(oracle):
    """the 33 query base rows and their oracle witnesses, computed once and never written to"""
    rows, _, codes = query_base()
    wits = np.empty((rows.shape[0], oracle.query_sizes()[1], 32), dtype=np.uint8)
    for i in range(rows.shape[0]):
        rc, _ = oracle.query_witness(rows[i], out=wits[i])
        assert rc == codes[i], (i, rc)
    rows.setflags(write=False)
    wits.setflags(write=False)
    return rows, wits, np.array(codes, dtype=np.int32)


@pytest.fixture(scope="module")
def qinst():
    return native.Instance(native.PZK_CIRCUIT_QUERY, 80)


@pytest.fixture(scope="module")
def rref(oracle):
    """the 17 register base rows and a cache of their oracle witnesses (72 MB each: only the rows compared)"""
    base = register_base()
    base.setflags(write=False)
    prm = oracle.register_params(**I.CANONICAL)
    cache = {}

    def ref(i):
        if i not in cache:
            rc, w = oracle.register_witness(prm, base[i])
            assert rc == 0, (i, rc)
            w.setflags(write=False)
            cache[i] = w
        return cache[i]

    return base, ref


def _query_rows_equal(wit, st, wits, codes, rows, inv=None, skip=()):
    for b in rows:
        if b in skip:
            continue
        want = wits[b] if inv is None else wits[b][inv]
        bad = np.nonzero((want != wit[b]).any(axis=1))[0]
        print("row %d: status %d (oracle %d), %d elements differ" % (b, st[b], codes[b], bad.size))
        assert bad.size == 0, "row %d: %d elements differ, first %s" % (b, bad.size, bad[:6])
        assert st[b] == codes[b], (b, st[b], codes[b])


@pytest.mark.parametrize("n", QUERY_SIZES)
def test_query_partly_live_workgroups(qref, qinst, n):
    rows, wits, codes = qref
    wit, st = qinst.witness_batch_host(np.ascontiguousarray(rows[:n]))
    assert wit.shape[0] == n
    _query_rows_equal(wit, st, wits, codes, range(n))


def test_register_partly_live_workgroups(rref):
    base, ref = rref
    inst = native.Instance(native.PZK_CIRCUIT_REGISTER, 0, I.CANONICAL)
    wit, st = inst.witness_batch_host(np.ascontiguousarray(base))
    regions = region_table(I.CANONICAL)
    assert (st == 0).all(), st
    for b in REGISTER_EDGES:
        rep = mismatch_report(ref(b), wit[b], regions)
        assert not rep, "row %d: %s" % (b, rep)


def _poisoned_batch(rows, elem, value):
    batch = np.array(rows[:32])
    batch[POISONED_ROW] = poison(rows[POISONED_ROW], elem, value)
    return batch


@pytest.mark.parametrize("case", QUERY_CASES, ids=[c[0] for c in QUERY_CASES])
def test_query_poisoned_row_is_flagged_and_neighbours_are_exact(qref, qinst, case):
    name, elem, value, code = case
    rows, wits, codes = qref
    wit, st = qinst.witness_batch_host(_poisoned_batch(rows, elem, value))
    print("%s: status of the poisoned row %d, expected %d" % (name, st[POISONED_ROW], code))
    _query_rows_equal(wit, st, wits, codes, range(32), skip=(POISONED_ROW,))
    assert st[POISONED_ROW] != 0
    assert st[POISONED_ROW] == code, (name, st[POISONED_ROW], code)


def test_register_poisoned_rows_are_flagged_and_neighbours_are_exact(rref):
    base, ref = rref
    rows, where = register_poisoned(base)
    inst = native.Instance(native.PZK_CIRCUIT_REGISTER, 0, I.CANONICAL)
    wit, st = inst.witness_batch_host(rows)
    print("statuses", st.tolist())
    regions = region_table(I.CANONICAL)
    for b in range(REGISTER_CALL):
        if b in where:
            continue
        rep = mismatch_report(ref(b), wit[b], regions)
        assert not rep, "row %d: %s" % (b, rep)
        assert st[b] == 0, (b, st[b])
    for b in where:
        assert st[b] == ST_INPUT_RANGE, (b, st[b])


def test_query_poisoned_row_through_an_o2_shaped_map(qref):
    """c's sibling = p case (the zero sibling of the poisoned row: no other check fails, code 64) on an O2-shaped
    mapped instance: its emitters read the same cores, so the neighbours are compared at the kept indices"""
    rows, wits, codes = qref
    txt = symmap.sym_text_wit(symmap.load_shape("query", 2))
    inv = symmap.parse_sym(txt)
    inst = native.Instance(native.PZK_CIRCUIT_QUERY, 80, sym=txt)
    assert inst.witness_size == inv.shape[0]
    wit, st = inst.witness_batch_host(_poisoned_batch(rows, QUERY_ELEMS["sibling_above"], POISON["p"]))
    _query_rows_equal(wit, st, wits, codes, range(32), inv=inv, skip=(POISONED_ROW,))
    assert st[POISONED_ROW] == ST_INPUT_RANGE, st[POISONED_ROW]
