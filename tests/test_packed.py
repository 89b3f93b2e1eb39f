"""CPU: packed input rows (include/pzkwit.h). The layout queries against the format rules restated in
Python (tests/packed_ref.py), the packed bytes against numpy (independent of the library's own unpack), the host
pack -> unpack round trip on generated rows of every family, the rows that must not pack, and the passport
preprocessor's packed rows against pack_inputs of its full rows."""
import json
import os

import numpy as np
import pytest

import packed_ref as PR
from pzkwit import inputs as I, light, native, passport as PP, query as Q
from pzkwit.field import SplitMix64

IDS = [i[0] for i in PR.INSTANCES]


@pytest.mark.parametrize("name", IDS)
def test_layout_matches_format_rules(name):
    """row size and every group's (kind, byte offset, byte length) = the rules; the groups tile [0, n_inputs) in
    order; every group and the row at a multiple of 16 bytes"""
    _, circuit, size, params, groups = PR.BY_ID[name]
    row_bytes, lay = native.packed_layout(params, circuit, size)
    want_bytes, want, _ = PR.layout(groups)
    assert (row_bytes, lay) == (want_bytes, want)
    info = native.layout_info(params, circuit, size)
    assert info.n_input_groups == len(groups) and info.n_inputs == sum(n for _, n in groups)
    assert row_bytes % 16 == 0 and all(off % 16 == 0 for _, off, _ in lay)
    p = native._params(params, circuit, size)
    assert native.lib().pzk_packed_group(p, len(groups), None, None, None) == -1  # PZK_E_ARG past the last group


def test_row_sizes_of_the_lines():
    """the three sizes DESIGN.md §14 quotes: config 3, QueryIdentity(80) TD3, RegisterIdentityLight"""
    assert native.packed_layout(I.CANONICAL)[0] == 3840
    assert native.packed_layout({}, native.PZK_CIRCUIT_QUERY, 80)[0] == 3232
    assert native.packed_layout(dict(dg_hash=256, doc=3), native.PZK_CIRCUIT_LIGHT)[0] == 160
    assert native.layout_inputs(I.CANONICAL) * 32 == 184896


def _generated_rows(name):
    """in-domain rows from the project's input generators, else (the standalone circuits) random domain rows"""
    _, circuit, size, params, groups = PR.BY_ID[name]
    if circuit == native.PZK_CIRCUIT_REGISTER:
        assert params == I.CANONICAL
        g = I.PassportGen(seed=0x9A, n_keys=1, workers=1)
        return np.stack([I.pack_register_inputs(g.passport_at(i, smt_depth=3 * i)) for i in range(3)])
    if circuit == native.PZK_CIRCUIT_QUERY:
        return Q.batch_rows(3, seed=0x9B, td1=bool(params.get("doc") == 1))
    if circuit == native.PZK_CIRCUIT_LIGHT:
        return light.batch_rows(3, seed=0x9C, dg_hash=params["dg_hash"], doc=params["doc"])
    return PR.edge_rows(groups, 3, 0x9D)


GEN_IDS = ["register_canonical", "query_td3", "query_td1", "light_256_3", "light_512_1", "poseidon_2", "sha256_1"]


@pytest.mark.parametrize("name", GEN_IDS)
def test_format_pin_and_round_trip(name):
    """packed bytes: BIT groups = np.packbits(bits, bitorder="big"), LIMB groups = <u8, FIELD groups verbatim, pad
    bytes zero (PR.pack writes nothing else); unpack_inputs_host(pack_inputs(rows)) == rows byte for byte"""
    _, circuit, size, params, groups = PR.BY_ID[name]
    rows = _generated_rows(name)
    packed, st = native.pack_inputs(rows, params, circuit, size)
    assert (st == 0).all(), st
    np.testing.assert_array_equal(packed, PR.pack(groups, rows))
    np.testing.assert_array_equal(native.unpack_inputs_host(packed, params, circuit, size), rows)


@pytest.mark.parametrize("name", ["register_canonical", "register_sig2", "register_sig20", "register_sig24", "query_td3"])
def test_round_trip_over_the_domain(name):
    """every value a packed row can hold survives: limbs 0 and 2^64 - 1, field elements 0, p - 1, p, 2^256 - 1
    (a scalar >= p stays representable); threads = 1 and 4 agree"""
    _, circuit, size, params, groups = PR.BY_ID[name]
    rows = PR.edge_rows(groups, 5, 0xE0)
    packed, st = native.pack_inputs(rows, params, circuit, size, threads=1)
    packed4, st4 = native.pack_inputs(rows, params, circuit, size, threads=4)
    assert (st == 0).all() and (st4 == 0).all()
    np.testing.assert_array_equal(packed, packed4)
    np.testing.assert_array_equal(packed, PR.pack(groups, rows))
    np.testing.assert_array_equal(native.unpack_inputs_host(packed, params, circuit, size), rows)


def test_rows_that_must_not_pack():
    """a 2 in dg1, a limb of 2^64, a bit element with a high byte set: status 1 and a zero packed row; the rows
    between them pack normally"""
    groups = PR.register_groups(I.CANONICAL)
    _, lay, el = PR.layout(groups)
    rows = PR.edge_rows(groups, 7, 0xE1)
    good = rows.copy()
    rows[1, el[2] + 17, 0] = 2           # dg1[17] = 2
    rows[3, el[5] + 4, :9] = [0] * 8 + [1]  # signature[4] = 2^64
    rows[5, el[1] + 300, 31] = 1         # encapsulatedContent[300] = 2^248 (+ its bit)
    packed, st = native.pack_inputs(rows, I.CANONICAL)
    assert st.tolist() == [0, 1, 0, 1, 0, 1, 0]
    assert not packed[[1, 3, 5]].any()
    np.testing.assert_array_equal(packed[[0, 2, 4, 6]], PR.pack(groups, good[[0, 2, 4, 6]]))
    # Light: the same for its dg1
    lrows = PR.edge_rows(PR.LIGHT_GROUPS, 3, 0xE2)
    lrows[1, 1023, 0] = 2
    lp, lst = native.pack_inputs(lrows, dict(dg_hash=256, doc=3), native.PZK_CIRCUIT_LIGHT)
    assert lst.tolist() == [0, 1, 0] and not lp[1].any() and lp[0].any() and lp[2].any()


def test_bad_arguments():
    p = native._params(I.CANONICAL)
    L = native.lib()
    assert L.pzk_packed_layout(None, None) == -1
    assert L.pzk_pack_inputs(p, None, 1, None, None, 1) == -1
    assert L.pzk_unpack_inputs_host(p, None, 1, None) == -1
    assert L.pzk_pack_inputs(p, None, 0, None, None, 1) == 0  # an empty batch needs no buffers
    bad = native._params(dict(I.CANONICAL, sig=22))
    assert L.pzk_packed_layout(bad, None) == -2  # PZK_E_PARAMS


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sod_vectors.json")


def test_passport_packed_rows():
    """passport.packed_rows == pack_inputs(passport.input_rows(...)) byte for byte on the SOD fixtures, with the
    same per-passport statuses, for the canonical instance and for every instance a fixture needs"""
    cases = json.load(open(GOLDEN))["cases"]
    srcs = [{f: c[f] for f in ("dg1", "dg15", "sod")} for c in cases]
    rng = SplitMix64(0x1D)
    ident = np.stack([PP.identity_elements(rng.fr(), rng.fr(), [rng.fr() for _ in range(80)]) for _ in srcs])
    seen, ok_rows = [], 0
    for c, s in zip(cases, srcs):
        params = PP.parse(s)["params"]
        if params in seen:
            continue
        seen.append(params)
        try:
            native.layout_witness_size(params)
        except native.PzkError:
            continue
        rows, st = PP.input_rows(params, srcs, ident, threads=2)
        prow, pst = PP.packed_rows(params, srcs, ident, threads=2)
        np.testing.assert_array_equal(st, pst)
        want, wst = native.pack_inputs(rows, params)
        assert (wst == 0).all()
        np.testing.assert_array_equal(prow, want)
        assert not prow[st != 0].any()
        ok_rows += int((st == 0).sum())
        # identity = None: zeros
        prow0, _ = PP.packed_rows(params, srcs, None, threads=1)
        rows0, _ = PP.input_rows(params, srcs, None, threads=1)
        np.testing.assert_array_equal(prow0, native.pack_inputs(rows0, params)[0])
    assert len(seen) >= 3 and ok_rows >= 3
