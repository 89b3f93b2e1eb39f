"""CPU: circom's binary .r1cs format through the C ABI (include/pzkwit.h pzk_r1cs_load / _get_info / _eval_host,
csrc/r1cs.cpp). Hand-written files give their header fields and merged term counts back; every malformed file of the
header's list is rejected with PZK_E_ARG and a reason, sizes of 2^40 and 2^63 in a 100-byte file included; the host
twin of the kernels agrees with the Python evaluator (tests/r1cs_ref.py) on the case list the GPU test uses; and the
device entry points refuse to run without a device."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import r1cs_ref as R  # noqa: E402
from pzkwit import native  # noqa: E402
from pzkwit.r1cs import R1cs  # noqa: E402

P = R.P
PZK_E_ARG, PZK_E_NODEVICE = -1, -6
SMALL = [([(1, 1)], [(2, 1)], [(3, 1)]), ([(0, 5), (1, P - 1)], [(0, 1)], [(2, 2), (3, 1 << 64)])]


def load_rc(data):
    h = ctypes.c_void_p()
    buf = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    rc = native.lib().pzk_r1cs_load(buf, len(data), ctypes.byref(h))
    msg = native.lib().pzk_last_error().decode()
    if rc == 0:
        native.lib().pzk_r1cs_destroy(h)
    else:
        assert not h.value
    return rc, msg


def test_info_fields():
    r = R1cs(R.write_r1cs(7, SMALL, n_pub_out=1, n_pub_in=2, n_prv_in=3, n_labels=1234567890123))
    assert r.info == dict(n_wires=7, n_pub_out=1, n_pub_in=2, n_prv_in=3, n_labels=1234567890123, n_constraints=2,
                          n_long=0, n_terms=8, n_coeffs=5, max_terms=2)  # coefficients 1, p - 1, 5, 2, 2^64
    r.close()
    r.close()


@pytest.mark.parametrize("kw", [dict(header_last=True), dict(labels=True), dict(extra=[(4, b"\x01\x02\x03"), (77, b"")]),
                                dict(header_last=True, labels=True, extra=[(5, b"x" * 40)])])
def test_section_order_and_skipped_sections(kw):
    """a header after the constraints, a wire -> label section, custom-gate and unknown sections skipped by size"""
    r = R1cs(R.write_r1cs(7, SMALL, **kw))
    assert (r.info["n_wires"], r.info["n_constraints"], r.info["n_terms"]) == (7, 2, 8)


def test_no_constraints():
    r = R1cs(R.write_r1cs(3, []))
    assert r.info["n_constraints"] == 0 and r.info["n_terms"] == 0 and r.info["n_coeffs"] == 2
    first, n = r.eval_host(np.zeros((2, 3, 32), dtype=np.uint8))
    assert list(first) == [-1, -1] and list(n) == [0, 0]


def test_terms_after_merging():
    """a wire listed three times merges into one term or none, an explicit 0 is no term, and an LC of 40 listed terms
    over 20 wires is short (20 <= 32) while 33 distinct wires are long"""
    cons = [([(1, 3), (1, 5), (1, P - 8)], [(2, 0)], [(3, 1), (3, 1), (4, 7), (3, P - 1)]),
            ([(i % 20, 1) for i in range(40)], [], []),
            ([], [], [(i, 2) for i in range(33)])]
    r = R1cs(R.write_r1cs(64, cons))
    want = R.info_of(cons)
    assert want == dict(n_terms=2 + 20 + 33, max_terms=33, n_long=1, n_coeffs=4)
    assert {k: r.info[k] for k in want} == want


def test_path_and_bytes(tmp_path):
    data = R.write_r1cs(7, SMALL)
    p = tmp_path / "c.r1cs"
    p.write_bytes(data)
    assert R1cs(p).info == R1cs(data).info == R1cs(bytearray(data)).info


def _hdr(**kw):
    return R.header_payload(7, kw.pop("m", len(SMALL)), **kw)


CON = R.constraints_payload(SMALL)
REJECTS = {
    "empty": b"",
    "short": b"r1cs\x01\x00\x00",
    "magic": R.assemble([(1, _hdr()), (2, CON)], magic=b"r1cz"),
    "version 0": R.assemble([(1, _hdr()), (2, CON)], version=0),
    "version 2": R.assemble([(1, _hdr()), (2, CON)], version=2),
    "field size 31": R.assemble([(1, R.header_payload(7, 2, field_size=31, prime=P >> 8)), (2, CON)]),
    "field size 64": R.assemble([(1, R.header_payload(7, 2, field_size=64)), (2, CON)]),
    "prime p + 2": R.assemble([(1, _hdr(prime=P + 2)), (2, CON)]),
    "prime bn254 q": R.assemble([(1, _hdr(prime=0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47)), (2, CON)]),
    "no header": R.assemble([(2, CON)]),
    "no constraints": R.assemble([(1, _hdr())]),
    "no sections": R.assemble([]),
    "two headers": R.assemble([(1, _hdr()), (2, CON), (1, _hdr())]),
    "two constraint sections": R.assemble([(1, _hdr()), (2, CON), (2, CON)]),
    "section count past the buffer": R.assemble([(1, _hdr()), (2, CON)], n_sections=3),
    "section count 2^32 - 1": R.assemble([(1, _hdr()), (2, CON)], n_sections=0xFFFFFFFF),
    "section size past the buffer": R.assemble([(1, _hdr())]) + struct.pack("<IQ", 2, len(CON) + 1) + CON,
    "truncated": R.assemble([(1, _hdr()), (2, CON)])[:-1],
    "section size 2^40": (R.assemble([(1, _hdr())], n_sections=2) + struct.pack("<IQ", 2, 1 << 40)).ljust(100, b"\0"),
    "section size 2^63": (R.assemble([(1, _hdr())], n_sections=2) + struct.pack("<IQ", 2, 1 << 63)).ljust(100, b"\0"),
    "section size 2^64 - 1": (R.assemble([(1, _hdr())], n_sections=2) + struct.pack("<IQ", 9, (1 << 64) - 1)).ljust(100, b"\0"),
    "header too short": R.assemble([(1, _hdr()[:-4]), (2, CON)]),
    "header too long": R.assemble([(1, _hdr() + b"\0" * 4), (2, CON)]),
    "header of 3 bytes": R.assemble([(1, b"\x20\0\0"), (2, CON)]),
    "constraint count past the section": R.assemble([(1, _hdr(m=3)), (2, CON)]),
    "constraint count 2^31 - 1 in a small section": R.assemble([(1, _hdr(m=(1 << 31) - 1)), (2, CON)]),
    "constraint count 2^31": R.assemble([(1, _hdr(m=1 << 31)), (2, CON)]),
    "constraint count 2^32 - 1": R.assemble([(1, _hdr(m=0xFFFFFFFF)), (2, CON)]),
    "term count past the section": R.assemble([(1, _hdr(m=1)), (2, struct.pack("<I", 2) + R.lc_bytes([(1, 1)])[4:] + R.lc_bytes([]) * 2)]),
    "term count 2^32 - 1": R.assemble([(1, _hdr(m=1)), (2, struct.pack("<I", 0xFFFFFFFF) + b"\0" * 80)]),
    "trailing bytes in the constraints": R.assemble([(1, _hdr()), (2, CON + b"\0")]),
    "fewer constraints than the section holds": R.assemble([(1, _hdr(m=1)), (2, CON)]),
    "wire = nWires": R.assemble([(1, _hdr(m=1)), (2, R.constraints_payload([([(7, 1)], [], [])]))]),
    "wire 2^32 - 1": R.assemble([(1, _hdr(m=1)), (2, R.constraints_payload([([], [], [(0xFFFFFFFF, 1)])]))]),
    "coefficient p": R.assemble([(1, _hdr(m=1)), (2, R.constraints_payload([([(1, P)], [], [])]))]),
    "coefficient 2^256 - 1": R.assemble([(1, _hdr(m=1)), (2, R.constraints_payload([([], [(1, (1 << 256) - 1)], [])]))]),
    "no wires": R.assemble([(1, R.header_payload(0, 0)), (2, b"")]),
    "label section too short": R.assemble([(1, _hdr()), (2, CON), (3, b"\0" * 48)]),
    "label section too long": R.assemble([(3, b"\0" * 64), (1, _hdr()), (2, CON)]),
}


@pytest.mark.parametrize("name", sorted(REJECTS))
def test_rejects(name):
    rc, msg = load_rc(REJECTS[name])
    assert rc == PZK_E_ARG and msg.startswith("r1cs: ") and len(msg) > 12, (rc, msg)


def test_huge_sizes_in_a_100_byte_file():
    for name in ("section size 2^40", "section size 2^63", "section size 2^64 - 1"):
        assert len(REJECTS[name]) == 100
        rc, msg = load_rc(REJECTS[name])
        assert rc == PZK_E_ARG and "runs past the buffer" in msg, msg


def test_null_arguments():
    L = native.lib()
    h = ctypes.c_void_p()
    assert L.pzk_r1cs_load(None, 10, ctypes.byref(h)) == PZK_E_ARG
    buf = (ctypes.c_uint8 * 4)()
    assert L.pzk_r1cs_load(buf, 4, None) == PZK_E_ARG
    assert L.pzk_r1cs_get_info(None, None) == PZK_E_ARG
    L.pzk_r1cs_destroy(None)
    r = R1cs(R.write_r1cs(7, SMALL))
    first = np.zeros(1, dtype=np.int32)
    rows = np.zeros((1, 7 * 32), dtype=np.uint8)
    assert L.pzk_r1cs_eval_host(r._h, rows.ctypes.data, 1, 7 * 32 - 16, first.ctypes.data, None) == PZK_E_ARG  # stride
    assert L.pzk_r1cs_eval_host(r._h, rows.ctypes.data, 1, 7 * 32 + 8, first.ctypes.data, None) == PZK_E_ARG
    assert L.pzk_r1cs_eval_host(r._h, None, 1, 7 * 32, first.ctypes.data, None) == PZK_E_ARG
    assert L.pzk_r1cs_eval_host(r._h, None, 0, 0, None, None) == 0  # batch 0: a no-op
    assert L.pzk_r1cs_eval_host(r._h, rows.ctypes.data, 1, 7 * 32, first.ctypes.data, None) == 0  # n_failed may be NULL


def eval_rows(r, rows):
    b = rows.shape[0]
    first, n = np.full(b, 7, dtype=np.int32), np.full(b, 7, dtype=np.uint32)
    assert native.lib().pzk_r1cs_eval_host(r._h, rows.ctypes.data, b, rows.shape[1], first.ctypes.data, n.ctypes.data) == 0
    return [(int(a), int(c)) for a, c in zip(first, n)]


@pytest.mark.parametrize("name", sorted(R.CASE_BUILDERS))
def test_host_twin_matches_the_evaluator(name):
    """pzk_r1cs_eval_host against Python integers on the GPU test's case list: rows with 48 bytes of 0xFF padding, the
    satisfying row first, then rows that violate one, a few or almost all constraints"""
    n, cons, w = R.case(name)
    r = R1cs(R.write_r1cs(n, cons))
    want = R.info_of(cons)
    assert {k: r.info[k] for k in want} == want
    for batch in R.BATCHES:
        ws = R.batch_of(name, batch)
        want_rows = [R.evaluate(cons, x) for x in ws]
        assert want_rows[0] == (-1, 0) and (batch == 1 or any(f >= 0 for f, _ in want_rows))
        assert eval_rows(r, R.rows_of(ws, n)) == want_rows


def test_host_twin_reads_residues():
    n, cons, raw = R.residue_case()
    r = R1cs(R.write_r1cs(n, cons))
    assert eval_rows(r, R.rows_of([raw], n)) == [(-1, 0)]
    # and a raw element that differs from the satisfying residue is seen
    bad = list(raw)
    bad[12] = (1 << 256) - 2
    assert eval_rows(r, R.rows_of([raw, bad], n)) == [(-1, 0), R.evaluate(cons, bad)] and R.evaluate(cons, bad)[1] > 0


def test_check_needs_a_device():
    """the device entry points are not served by the host twin: without a device they fail with PZK_E_NODEVICE"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("device present")
    r = R1cs(R.write_r1cs(7, SMALL))
    rows = np.zeros((1, 7 * 32), dtype=np.uint8)
    first = np.zeros(1, dtype=np.int32)
    ex = native.PzkExec(device=-1, flags=1, stream=None)
    L = native.lib()
    # (the pointer is never dereferenced: the call fails before any launch)
    assert L.pzk_r1cs_check_batch(r._h, rows.ctypes.data & ~15, 1, 7 * 32, first.ctypes.data, None, ctypes.byref(ex)) == PZK_E_NODEVICE
    assert b"no HIP device" in L.pzk_last_error()
    assert L.pzk_r1cs_check_batch_host(r._h, rows.ctypes.data, 1, 7 * 32, first.ctypes.data, None, ctypes.byref(ex)) == PZK_E_NODEVICE
    with pytest.raises(native.PzkError, match="no HIP device"):
        r.check(rows.reshape(1, 7, 32))
    assert L.pzk_r1cs_check_batch(r._h, None, 0, 0, None, None, None) == 0  # batch 0: a no-op on any host
