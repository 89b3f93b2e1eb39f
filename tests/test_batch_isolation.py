"""CPU: the rows of tests/test_gpu_batch_isolation.py, pinned on the oracle.

Four core kernels share one field inversion among the witnesses of a workgroup (k_smt_prep 32, k_bjj_core 16 at the
default BJJ_SEGS, k_rsa_inv 8, k_qry_prep 8), so the rows of one batch are not independent on the device: a value in
one row can reach its neighbours' witnesses through the shared total. This file builds

* 33 QueryIdentity(80) base rows whose zero patterns differ between the witnesses of one workgroup: proof depths
  cycle 0, 1, 40, 79, random (depth 0: every sibling zero, the witness total is exactly 1), and the citizenship sits
  at list index 0, 63, 64, 239 (k_qry_prep's zero difference in lane 0, lane 63, the second j, the last live j) and,
  in one row, nowhere in the list;
* 17 canonical register base rows (depth (7 i) % 80, the proof's root);
* poisoned copies: exactly one input element replaced by raw little-endian bytes of p, p + 1, 2p or 2^256 - 1 (not
  reduced), or by a value past the element's bit width (selector = 2^18, citizenshipMask = 2^240).

A base row's reference is the oracle. A poisoned row's is the contract of DESIGN.md §5: the lane is flagged with
PZK_ST_INPUT_RANGE (64), or with a smaller check code when the row ALSO fails that check. Which smaller code that is
follows from the circuit, which sees its inputs mod p (circom reduces them): it is the oracle's code for the row with
the poisoned element reduced. The expected codes are written out per case below with the check they come from, and
proved against the oracle here. (The oracle copies input bytes verbatim, so it is never run on a poisoned row.)

The base row without a listed citizenship is the one row that is not a passing query: CitizenshipCheck rejects it
(citizenshipCheck.circom:274, code 22) on the oracle and on the device alike. Its witness is still defined element
for element, so it is compared like every other row, with status 22 in place of 0."""
import numpy as np
import pytest

from pzkwit import field, inputs as I, query as Q
from pzkwit.field import SplitMix64

P = field.P
ST_NUM2BITS, ST_SMT_LAST, ST_CIT_LIST, ST_ISV_ROOT, ST_INPUT_RANGE = 1, 13, 22, 23, 64  # include/pzkwit.h PZK_ST_*

# the out-of-field values, all below 2^256 (p ~ 2^253.6)
POISON = {
    "p": 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001,
    "p+1": 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000002,
    "2p": 0x60C89CE5C263405370A08B6D0302B0BA5067D090F372E12287C3EB27E0000002,
    "2^256-1": 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF,
}
assert POISON == {"p": P, "p+1": P + 1, "2p": 2 * P, "2^256-1": (1 << 256) - 1}

# ---------------------------------------------------------------------------------------------- query base rows
N_QUERY = 33
QUERY_SEED = 0xB150
DEPTHS = [0, 1, 40, 79, None]
# base row -> list index of its citizenship (None: a code that is not in the list)
CIT_AT = {2: 0, 5: 63, 6: None, 9: 64, 12: 239, 18: 63, 20: 0, 27: 239, 32: 64}
UNLISTED = b"XXX"
POISONED_ROW = 13  # of base[:32]; in the second k_qry_prep workgroup and the first of k_bjj_core


def query_base():
    """-> (rows (33, 842, 32) uint8, infos, expected oracle codes)"""
    C = Q.countries()
    rng = SplitMix64(QUERY_SEED)
    rows, infos, codes = [], [], []
    for i in range(N_QUERY):
        kw = {}
        if i in CIT_AT:
            kw["cit_code"] = UNLISTED if CIT_AT[i] is None else C[CIT_AT[i]].to_bytes(3, "big")
        inp, info = Q.make_query(rng, depth=DEPTHS[i % 5], **kw)
        cit = info["fields"][Q_F_CIT]
        if cit in C:  # make_query clears the blacklist bit of the index it drew, not of a given code
            inp["citizenshipMask"] &= ~(1 << (239 - C.index(cit)))
        rows.append(Q.pack(inp))
        infos.append(info)
        codes.append(0 if cit in C else ST_CIT_LIST)
    return np.stack(rows), infos, codes


Q_F_CIT = 5  # DG1DataExtractor field holding the citizenship (query_layout.hpp q_f_cit, TD3)


def poison(row, elem, value):
    """a copy of `row` with input element `elem` replaced by the raw little-endian bytes of `value` (not reduced)"""
    assert 0 <= value < 1 << 256
    out = row.copy()
    out[elem] = np.frombuffer(int(value).to_bytes(32, "little"), dtype=np.uint8)
    return out


def elem_int(row, elem):
    return int.from_bytes(row[elem].tobytes(), "little")


SIB_BELOW, SIB_ABOVE = 5, 79  # idStateSiblings[k] of the poisoned row (depth 79): a non-zero sibling, the zero one
QUERY_ELEMS = {
    "sibling_below": Q.OFF["idStateSiblings"] + SIB_BELOW,
    "sibling_above": Q.OFF["idStateSiblings"] + SIB_ABOVE,
    "idStateRoot": Q.OFF["idStateRoot"],
    "skIdentity": Q.OFF["skIdentity"],
    "pkPassportHash": Q.OFF["pkPassportHash"],
    "eventID": Q.OFF["eventID"],
    "eventData": Q.OFF["eventData"],
}
# decomposed inputs with a value past their width (both below p): element, value, bits
QUERY_WIDTH = {"selector": (Q.OFF["selector"], 1 << 18, 18), "citizenshipMask": (Q.OFF["citizenshipMask"], 1 << 240, 240)}

# The code each case reports: 64 unless the row, read mod p as the circuit reads it, also fails a smaller check.
#   23  IdentityStateVerifier's smtVerifier.isVerified === 1 (identityStateVerifier.circom:46; k_smt_chain4's
#       ST_ISV_ROOT): the value mod p differs from the one the proof was built over, so the SMT root differs. This
#       holds for a sibling below the insertion level, for idStateRoot itself, and for skIdentity / pkPassportHash,
#       which enter the tree position Poseidon2(pkPassportHash, Poseidon2(sk * Base8)).
#   13  SMTLevIns: (1 - isZero(siblings[79])) === 0 (SMTVerifier.circom:54; k_smt_prep's ST_SMT_LAST): p + 1 and
#       2^256 - 1 are non-zero mod p in the last sibling. p and 2p are 0 mod p there: the proof is unchanged, and
#       only the range flag is left.
#   64  eventID (the nullifier's third input) and eventData (squared, nothing else) enter no check.
#    1  Num2Bits(18)(selector) and Num2Bits(240)(citizenshipMask): out bits recompose to `in` (bitify.circom:26;
#       k_emit_bits' ST_NUM2BITS). These two values are below p, so the range flag is not owed; they are here because
#       they are past the width the layout reads.
QUERY_CODES = {
    "sibling_below": {"p": 23, "p+1": 23, "2p": 23, "2^256-1": 23},
    "sibling_above": {"p": 64, "p+1": 13, "2p": 64, "2^256-1": 13},
    "idStateRoot": {"p": 23, "p+1": 23, "2p": 23, "2^256-1": 23},
    "skIdentity": {"p": 23, "p+1": 23, "2p": 23, "2^256-1": 23},
    "pkPassportHash": {"p": 23, "p+1": 23, "2p": 23, "2^256-1": 23},
    "eventID": {"p": 64, "p+1": 64, "2p": 64, "2^256-1": 64},
    "eventData": {"p": 64, "p+1": 64, "2p": 64, "2^256-1": 64},
}
WIDTH_CODE = ST_NUM2BITS

# (case id, element offset, value, expected status) of every query poison
QUERY_CASES = [("%s=%s" % (name, vn), off, POISON[vn], QUERY_CODES[name][vn])
               for name, off in QUERY_ELEMS.items() for vn in POISON]
QUERY_CASES += [("%s=2^%d" % (name, bits), off, val, WIDTH_CODE) for name, (off, val, bits) in QUERY_WIDTH.items()]

# ---------------------------------------------------------------------------------------------- register rows
N_REGISTER = 17
REGISTER_SEED = 0xB151


def register_gen():
    return I.PassportGen(seed=REGISTER_SEED, n_keys=2, workers=1)


def register_base(gen=None):
    g = gen or register_gen()
    return np.stack([I.pack_register_inputs(g.passport_at(i, smt_depth=(7 * i) % 80, smt_root=True))
                     for i in range(N_REGISTER)])


def register_offsets(n_in):
    """input element offsets (pzkwit.inputs.pack_register_inputs): slaveMerkleRoot first, the 80 branches and
    skIdentity last"""
    return {"slaveMerkleRoot": 0, "slaveMerkleInclusionBranches": n_in - 81, "skIdentity": n_in - 1}


# row of the 9-row call -> (element name, index in it, value); every one reports 64: the register circuit leaves
# smtVerifier.isVerified unenforced (passportVerificationBuilder.circom:240), sibling 3 of a depth-14 proof is not the
# last one, and skIdentity = p + 5 is the valid key 5 mod p
REGISTER_POISON = {2: ("slaveMerkleInclusionBranches", 3, P), 5: ("skIdentity", 0, P + 5),
                   7: ("slaveMerkleRoot", 0, (1 << 256) - 1)}
REGISTER_CALL = 9


def register_poisoned(base):
    """-> (rows of the 9-row call, {row: input element that was replaced})"""
    rows = base[:REGISTER_CALL].copy()
    off = register_offsets(base.shape[1])
    where = {}
    for r, (name, k, val) in REGISTER_POISON.items():
        where[r] = off[name] + k
        rows[r] = poison(base[r], where[r], val)
    return rows, where


def reduced(row, elem):
    """the row as the circuit reads it: element `elem` mod p"""
    return poison(row, elem, elem_int(row, elem) % P)


def contract_code(rc_reduced, value):
    """the smallest failing code; an element >= p fails PZK_ST_INPUT_RANGE"""
    codes = [c for c in (rc_reduced, ST_INPUT_RANGE if value >= P else 0) if c]
    return min(codes) if codes else 0


# ---------------------------------------------------------------------------------------------- the proofs
@pytest.fixture(scope="module")
def qbase():
    return query_base()


def test_query_base_rows_pass_and_cover_the_patterns(oracle, qbase):
    rows, infos, codes = qbase
    C = Q.countries()
    assert rows.shape == (N_QUERY, Q.N_INPUTS, 32)
    for i in range(N_QUERY):
        rc, _ = oracle.query_witness(rows[i])
        assert rc == codes[i], (i, rc)
    assert [i for i, c in enumerate(codes) if c] == [6] and codes[6] == ST_CIT_LIST
    # depths: the cycle is really there, and the zero-sibling mask of the input row agrees with it
    sib = Q.OFF["idStateSiblings"]
    for i, info in enumerate(infos):
        d = info["depth"]
        if DEPTHS[i % 5] is not None:
            assert d == DEPTHS[i % 5], (i, d)
        nz = rows[i, sib:sib + 80].any(axis=1)
        assert nz[:d].all() and not nz[d:].any(), i
    first32 = [info["depth"] for info in infos[:32]]
    assert {0, 1, 40, 79} <= set(first32) and len(set(first32) - {0, 1, 40, 79}) >= 2
    # the four witnesses of a k_smt_prep wave (8 lanes each) do not share one zero pattern
    for w0 in range(0, 32, 8):
        assert len(set(first32[w0:w0 + 8])) >= 4, w0
    # citizenship: list index 0, 63, 64, 239 and an unlisted code, read back from the DG1 fields
    where = {}
    for i, info in enumerate(infos):
        cit = info["fields"][Q_F_CIT]
        where[i] = C.index(cit) if cit in C else None
    for i, idx in CIT_AT.items():
        assert where[i] == idx, (i, where[i], idx)
    assert {0, 63, 64, 239, None} <= set(where[i] for i in range(32))
    assert where[6] is None and infos[6]["fields"][Q_F_CIT] == int.from_bytes(UNLISTED, "big")
    # the poisoned row is an ordinary passing one of depth 79
    assert codes[POISONED_ROW] == 0 and where[POISONED_ROW] is not None
    assert 0 < SIB_BELOW < infos[POISONED_ROW]["depth"] <= SIB_ABOVE < 80


def test_register_base_rows_pass(oracle):
    g = register_gen()
    base = register_base(g)
    prm = oracle.register_params(**I.CANONICAL)
    off = register_offsets(base.shape[1])
    br = off["slaveMerkleInclusionBranches"]
    for i in range(N_REGISTER):
        rc, _ = oracle.register_witness(prm, base[i])
        assert rc == 0, (i, rc)
        d = (7 * i) % 80
        nz = base[i, br:br + 80].any(axis=1)
        assert nz[:d].all() and not nz[d:].any(), i
        pp = g.passport_at(i, smt_depth=d, smt_root=True)
        assert elem_int(base[i], off["slaveMerkleRoot"]) == pp["root"] and elem_int(base[i], off["skIdentity"]) == pp["sk"]


def test_base_rows_satisfy_the_constraints(oracle, qbase):
    import pyr1cs
    from test_r1cs import _ok, expected_uncovered
    rows = qbase[0]
    for i in (0, POISONED_ROW):
        rc, w = oracle.query_witness(rows[i])
        crc, rep = pyr1cs.check_query(w)
        assert rc == 0 and crc == 0 and rep["n_failed"] == 0 and rep["n_uncovered"] == 0, (i, rep)
    base = register_base()
    prm = oracle.register_params(**I.CANONICAL)
    for i in (2, 16):
        rc, w = oracle.register_witness(prm, base[i])
        assert rc == 0
        _ok(pyr1cs.check_register(w, **I.CANONICAL), expected_uncovered(1))


def _one_element_differs(base_row, row, elem):
    diff = np.nonzero((base_row != row).any(axis=1))[0]
    assert diff.tolist() == [elem], diff


@pytest.mark.parametrize("case", QUERY_CASES, ids=[c[0] for c in QUERY_CASES])
def test_query_poison_is_one_element_with_the_stated_code(oracle, qbase, case):
    name, elem, value, code = case
    base_row = qbase[0][POISONED_ROW]
    row = poison(base_row, elem, value)
    _one_element_differs(base_row, row, elem)
    assert elem_int(row, elem) == value
    width = [bits for _, (off, _, bits) in QUERY_WIDTH.items() if off == elem]
    if width:
        assert (1 << width[0]) <= value < P
    else:
        assert value >= P
    rc, _ = oracle.query_witness(reduced(row, elem))
    assert contract_code(rc, value) == code, (name, rc)


def test_register_poison_is_one_element_each_and_flags_range_only(oracle):
    base = register_base()
    rows, where = register_poisoned(base)
    prm = oracle.register_params(**I.CANONICAL)
    assert rows.shape[0] == REGISTER_CALL and sorted(where) == [2, 5, 7]
    for r in range(REGISTER_CALL):
        if r not in where:
            assert (rows[r] == base[r]).all()
            continue
        _one_element_differs(base[r], rows[r], where[r])
        value = elem_int(rows[r], where[r])
        assert value == REGISTER_POISON[r][2] >= P
        rc, _ = oracle.register_witness(prm, reduced(rows[r], where[r]))
        assert contract_code(rc, value) == ST_INPUT_RANGE, (r, rc)
    assert 0 < REGISTER_POISON[2][1] < (7 * 2) % 80  # the poisoned branch is below row 2's depth
