"""CPU: the .r1cs loader and the kernels' host twin (pzk_r1cs_load / _get_info / _eval_host, csrc/r1cs.cpp) as a host
AddressSanitizer + UndefinedBehaviorSanitizer build (tools/fuzz/r1cs_fuzz.cpp), run the way tests/test_pack_fuzz.py
runs pack_fuzz: about 1,000 mutations of three valid files — byte flips, truncations at every field boundary, huge
counts and sizes in every count and size field, swapped, dropped and doubled sections — in heap blocks of exactly the
file's size. Every record must come back "ok ..." or "err <code>" with no sanitizer report."""
import os
import random
import shutil
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import r1cs_ref as R  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "tools", "fuzz", "build", "r1cs_fuzz")
HUGE = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 1 << 40, 1 << 63, (1 << 64) - 1]


@pytest.fixture(scope="module")
def fuzz_bin():
    if not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None:
        pytest.skip("no hipcc for the host sanitizer build")
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tools", "fuzz"), "build/r1cs_fuzz"])
    return BIN


def run(fuzz_bin, files, timeout=600):
    env = dict(os.environ, ASAN_OPTIONS="allocator_may_return_null=1:detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    data = b"".join(struct.pack("<I", len(f)) + f for f in files)
    p = subprocess.run([fuzz_bin], input=data, capture_output=True, timeout=timeout, env=env)
    err = p.stderr.decode(errors="replace")
    out = p.stdout.decode().splitlines()
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (out[-3:], err[-3000:])
    assert len(out) == len(files), (len(out), len(files), err[-2000:])
    return out


def valid_files():
    """three valid files with their sections [(type, payload)]: a small one with every section kind, the directed
    case (every LC shape), and long constraints"""
    small = [([(1, 1)], [(2, 1)], [(3, 1)]), ([(0, 5), (1, R.P - 1), (1, 3)], [(0, 1)], [(2, 2), (3, 1 << 64)]), ([], [], [])]
    out = []
    for n, cons, extra in ((7, small, [(4, b"\x01\x02\x03")]), R.case("directed")[:2] + ([],), R.case("only_long")[:2] + ([],)):
        secs = [(1, R.header_payload(n, len(cons))), (2, R.constraints_payload(cons))] + extra
        secs.append((3, b"".join(struct.pack("<Q", i) for i in range(n))))
        out.append((n, cons, secs))
    return out


def field_boundaries(secs):
    """offsets of every field boundary of the assembled file, as far as the first 40 terms of the constraints"""
    at, pos = [0, 4, 8, 12], 12
    for kind, payload in secs:
        at += [pos + 4, pos + 12]
        body = pos + 12
        if kind == 1:
            at += [body + o for o in (4, 36, 40, 44, 48, 52, 60, 64)]
        elif kind == 2:
            o, terms = 0, 0
            while o < len(payload) and terms < 40:
                nt = struct.unpack_from("<I", payload, o)[0]
                o += 4
                at.append(body + o)
                for _ in range(nt):
                    at += [body + o + 4, body + o + 36]
                    o += 36
                    terms += 1
        pos = body + len(payload)
        at.append(pos)
    return sorted(set(at))


def mutations(rng, n, cons, secs):
    base = R.assemble(secs)
    out = []
    bounds = field_boundaries(secs)
    for b in bounds:                                   # truncations at every field boundary, and one byte around it
        out += [base[:b], base[:max(b - 1, 0)], base[:b + 1]]
    for _ in range(120):                               # byte flips, biased to the structured head of the file
        f = bytearray(base)
        for _ in range(rng.randint(1, 3)):
            i = rng.randrange(min(len(f), 400)) if rng.random() < 0.7 else rng.randrange(len(f))
            f[i] ^= 1 << rng.randrange(8)
        out.append(bytes(f))
    # huge counts and sizes: the section count, every section's size, the header's counts, term counts
    for v in HUGE:
        out.append(base[:8] + struct.pack("<I", v & 0xFFFFFFFF) + base[12:])
        pos = 12
        for kind, payload in secs:
            out.append(base[:pos + 4] + struct.pack("<Q", v) + base[pos + 12:])
            if kind == 1:
                for o, fmt in ((0, "<I"), (36, "<I"), (40, "<I"), (52, "<Q"), (60, "<I")):
                    w = struct.pack(fmt, v & (0xFFFFFFFF if fmt == "<I" else (1 << 64) - 1))
                    out.append(base[:pos + 12 + o] + w + base[pos + 12 + o + len(w):])
            if kind == 2:
                for o in (0, 4 + 36 * len(cons[0][0])):  # the first two term counts
                    out.append(base[:pos + 12 + o] + struct.pack("<I", v & 0xFFFFFFFF) + base[pos + 16 + o:])
                out.append(base[:pos + 16] + struct.pack("<I", v & 0xFFFFFFFF) + base[pos + 20:])  # the first wire id
            pos += 12 + len(payload)
    # sections swapped, dropped, doubled
    for _ in range(12):
        s = list(secs)
        rng.shuffle(s)
        out.append(R.assemble(s))
    for i in range(len(secs)):
        out.append(R.assemble(secs[:i] + secs[i + 1:]))
        out.append(R.assemble(secs + [secs[i]]))
        out.append(R.assemble(secs[:i] + [(secs[i][0], secs[i][1] + b"\0")] + secs[i + 1:]))
    return out


def test_r1cs_fuzz(fuzz_bin):
    rng = random.Random(0xF5)
    files, valid = [], 0
    for n, cons, secs in valid_files():
        muts = mutations(rng, n, cons, secs)
        for k in range(10):  # valid files mixed in: the same sections in every order
            s = list(secs)
            rng.shuffle(s)
            muts.insert(rng.randrange(len(muts)), R.assemble(s))
            valid += 1
        files += muts
    assert 900 <= len(files) <= 3000, len(files)
    out = run(fuzz_bin, files)
    assert all(o.startswith("ok ") or o.startswith("err -") for o in out), [o for o in out if o[:2] not in ("ok", "er")][:5]
    n_ok, n_err = sum(o.startswith("ok") for o in out), sum(o.startswith("err") for o in out)
    assert n_ok >= max(20, valid) and n_err >= 20, (n_ok, n_err)


def test_valid_files_report_their_sizes(fuzz_bin):
    """the driver's "ok" line carries what the file says: wires, constraints, merged terms, and -1 for the zero row"""
    vf = valid_files()
    out = run(fuzz_bin, [R.assemble(secs) for _, _, secs in vf])
    for o, (n, cons, _) in zip(out, vf):
        assert o == "ok %d %d %d -1" % (n, len(cons), R.info_of(cons)["n_terms"]), o
