"""CPU: the RegisterIdentityBuilder edge instances and flow-failing rows of tests/register_cases.py, pinned before the
device sees them (tests/test_gpu_register_cases.py):

  - each flow instance's rows reach every label of FEATURES, the AA_SIGNATURE_ALGO = 0 instance those of FEATURES_V0;
  - on every row the oracle returns 0, or 7 exactly where the row was tampered with, and its PassportVerificationFlow
    region (kind 11 of the library's region table) equals flow_ref() element for element;
  - the library's layout and the oracle agree on every instance's input count and witness size;
  - for every bound build_register checks, the parameter set just inside is accepted by the library and by the
    oracle and the set just outside is rejected by both; the sanitised stand-alone oracle (oracle/san_main.c) takes a
    row of each accepted set and refuses each rejected one before it reads anything."""
import os
import struct
import subprocess

import numpy as np
import pytest

from pzkwit import inputs as I

import register_cases as C
from test_capi import layout_sizes, region_table
from test_sanitize import DATA, KEYS, _record, san_main  # noqa: F401  (san_main: the fixture that builds it)

# san_main's rc / check / failed / uncovered_nonzero of a row whose flow fails and nothing else: the one constraint that
# does not hold is the builder's `flowResult === 1` (passportVerificationBuilder.circom:155)
SANFAIL = ("7", "1", "1", "0")

RK_FLOW = 11
NAMES = list(C.PARAMS)
FLOW_NAMES = [n for n in NAMES if C.PARAMS[n][1]]


def _ints(w):
    return [int.from_bytes(w[i].tobytes(), "little") for i in range(w.shape[0])]


def test_instances_are_the_issues():
    """the list itself: what each named case must have (a wrong shift here would quietly test something else)"""
    p = {n: C.PARAMS[n][0] for n in NAMES}
    assert all(p["odd"][k] % 8 for k in ("dg1_shift", "dg15_shift", "ec_shift", "aa_shift"))
    assert p["dg1_first"]["dg1_shift"] == 0 and p["dg15_first"]["dg15_shift"] == 24 and p["ec_first"]["ec_shift"] == 0
    assert p["aa_first"]["aa_shift"] == 0 and p["d15_1"]["aa_shift"] == 0
    last = p["last"]
    assert last["dg15_shift"] + 256 == C.usable(4, 512) and last["ec_shift"] + 256 == C.usable(2, 512)
    assert last["aa_shift"] + 1024 == C.usable(3, 512) and last["dg1_shift"] == 8
    assert p["ec16"]["ec_blocks"] == 16 and p["ec16"]["dg1_shift"] + 256 == C.usable(16, 512)
    assert p["ec16"]["dg15_shift"] > 4096 and p["ec16"]["dg15_shift"] % 2
    assert (p["ec1"]["ec_blocks"], p["ec1"]["aa"], p["ec1"]["dg15_blocks"]) == (1, 0, 0)
    assert (p["d15_1"]["dg15_blocks"], p["d15_1"]["aa"]) == (1, 23)
    assert p["d15_16"]["dg15_blocks"] == 16 and p["d15_16"]["aa_shift"] + 1024 == C.usable(16, 512)
    for n, aa in (("aa2", 2), ("aa19", 19), ("aa21", 21), ("aa25", 25), ("aa22", 22), ("flow_aa23", 23)):
        assert p[n]["aa"] == aa and p[n]["aa_shift"] % 2
    assert p["aa20_end"]["aa"] == 20 and p["aa20_end"]["aa_shift"] + 512 == 3 * 512
    s13 = p["sig13_dg384_aa22"]
    assert s13["dg15_shift"] + 384 == C.usable(2, 1024) and s13["ec_shift"] + 384 == C.usable(1, 1024)
    assert s13["aa_shift"] + 640 == C.usable(2, 1024) and s13["dg1_shift"] % 2
    assert [p[n]["aa"] for n in FLOW_NAMES] == [1, 7, 23]
    for n in NAMES:
        assert all(len(b) <= C.MAX_BATCH for b in C.batches(n)[1])


@pytest.mark.parametrize("name", FLOW_NAMES)
def test_flow_rows_reach_every_feature(name):
    params, rows = C.instance_rows(name)
    reached = set()
    for r in rows:
        f = C.features(params, r)
        assert ("passing" in f) == (r.code == 0), (str(r), f)
        reached |= f
    want = set(C.FEATURES)
    if params["aa"] < 2:
        want -= {"diff_+V", "diff_-V"}  # V = 1: the scaled differences are the plain +-1
    assert want <= reached, sorted(want - reached)
    if name == C.PREFIX_INSTANCE:
        d15 = params["dg15_shift"] - C.PREFIX_SHIFT
        assert {("ec", d15 + i) for i in range(8)} <= {t for r in rows for t in r.tamper}
    assert {"diff_+V", "diff_-V"} <= reached or params["aa"] < 2


def test_aa0_rows_pass_on_any_dg15_content():
    params, rows = C.instance_rows(C.V0_INSTANCE)
    assert params["aa"] == 0
    for r in rows:
        assert {"passing"} | set(C.FEATURES_V0) <= C.features(params, r), str(r)


@pytest.mark.parametrize("name", NAMES)
def test_rows_on_the_oracle(oracle, name):
    params, rows = C.instance_rows(name)
    rc, nin, nw = layout_sizes(params)
    prm = oracle.register_params(**params)
    assert rc == 0 and (nin, nw) == oracle.register_sizes(prm)
    flow = [(o, ln) for o, ln, k in region_table(params) if k == RK_FLOW]
    assert len(flow) == 1
    off, ln = flow[0]
    assert len(rows) >= 2 and rows[0].code == 0 and rows[1].code == 0 and any(rows[1].pp["siblings"])
    w = np.zeros((nw, 32), dtype=np.uint8)
    for r in rows:
        assert r.packed.shape[0] == nin
        code, _ = oracle.register_witness(prm, r.packed, out=w)
        assert code == r.code, (str(r), code)
        ref = C.flow_ref(params, r)
        assert len(ref) == ln
        got = _ints(w[off:off + ln])
        bad = [i for i in range(ln) if got[i] != ref[i]]
        assert not bad, "%s: %d flow elements differ, first local %d: oracle %d, flow_ref %d" % (
            r, len(bad), bad[0], got[bad[0]], ref[bad[0]])
        NC = 3 * params["dg_hash"] + 8
        chain0 = ln - 7 * NC
        assert ref[0] == ref[chain0 + NC - 1] == int(r.code == 0)


# ------------------------------------------------------------------------------------------------ acceptance bounds
def _accepts(oracle, params):
    rc, _, _ = layout_sizes(params)
    assert rc in (0, -2), rc
    nw = oracle.register_sizes(oracle.register_params(**params))[1]
    return rc == 0, nw != 0


@pytest.mark.parametrize("bound", list(C.BOUNDS))
def test_bounds_agree(oracle, bound):
    inside, outside = C.BOUNDS[bound]
    assert _accepts(oracle, inside) == (True, True), bound
    assert _accepts(oracle, outside) == (False, False), bound
    # a rejected set evaluates nothing: orc_register_witness returns -1 without touching its buffers
    assert oracle.lib().orc_register_witness(oracle.register_params(**outside), None, None) == -1


def _fits(params):
    """the windows of the set lie before the SHA padding of their messages, so build_row() can build it as it is"""
    g = C.geometry(params)
    ec_use, sa_use = C.usable(params["ec_blocks"], g["HB"]), C.usable(1024 // g["HB"], g["HB"])
    d1s, d15s, DG = params["dg1_shift"], params["dg15_shift"], g["DG"]
    ok = d1s + DG <= ec_use and params["ec_shift"] + DG <= sa_use
    if params["aa"]:
        ok = ok and d15s + DG <= ec_use and (d1s + DG <= d15s - C.PREFIX_SHIFT or d15s + DG <= d1s)
    return ok


def _edge_row(params):
    """-> (row, fits). A bound set sits on the end of a signal array, so its window may cover the SHA padding, where
    no message can put a hash: such a row is built at shifts that fit and read at the set's own, where its flow fails
    and nothing else does. A set that fits is built as it is, and passes."""
    key = C.signer(params["sig"])
    if _fits(params):
        return C.build_row(params, key, 77), True
    g = C.geometry(params)
    fit = dict(params, dg1_shift=0, ec_shift=0, aa_shift=0,
               dg15_shift=g["DG"] + C.PREFIX_SHIFT if params["aa"] else params["dg15_shift"])
    assert _fits(fit)
    row = C.build_row(fit, key, 77)
    assert I.pack_register_inputs(row.pp, params).shape == row.packed.shape
    return row, False


def test_bounds_on_the_sanitised_oracle(oracle, san_main, tmp_path):
    """oracle/san_main.c (AddressSanitizer + UndefinedBehaviorSanitizer, stand-alone) on one inside and one outside set
    per bound. A row of every inside set evaluates with no report: code 0 and every constraint satisfied where the set's
    windows fit before the padding, else code 7 and exactly one constraint failing (SANFAIL). Every
    outside set comes with a row of the oracle's own input count for it, so only the witness size 0 that params_ok
    gives can refuse it (exit 2, no report); were it accepted, the oracle would run on it under the sanitisers."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")
    seen, recs, exact = set(), [], []
    for bound, (inside, _) in C.BOUNDS.items():
        key = tuple(inside[k] for k in KEYS)
        if key in seen or bound.startswith(("sums", "negative")):
            continue  # (the overflow pairs' inside sets are interior sets, not bound sets)
        seen.add(key)
        row, fits = _edge_row(inside)
        recs.append(_record(0, list(key), row.packed))
        exact.append(fits)
    cases = tmp_path / "inside.bin"
    cases.write_bytes(b"".join(recs))
    r = subprocess.run([san_main, DATA, str(cases)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(recs), r.stdout
    assert any(exact) and not all(exact)
    for ln, fits in zip(lines, exact):
        f = ln.split()
        assert (f[5], f[7], f[9], f[11]) == (("0", "0", "0", "0") if fits else SANFAIL), ln
    for bound, (_, outside) in C.BOUNDS.items():
        nin = oracle.register_sizes(oracle.register_params(**outside))[0]
        assert 0 < nin < 1 << 20, (bound, nin)
        one = tmp_path / "outside.bin"
        one.write_bytes(struct.pack("<i10ii", 0, *[outside[k] for k in KEYS], nin) + bytes(32 * nin))
        r = subprocess.run([san_main, DATA, str(one)], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 2 and "size mismatch (%d inputs expected)" % nin in r.stderr, (bound, r.returncode,
                                                                                             r.stderr[-2000:])
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (bound, r.stderr[-3000:])
