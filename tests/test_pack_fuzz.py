"""CPU: the packed input rows' host code (pzk_packed_layout / pzk_packed_group / pzk_pack_inputs /
pzk_unpack_inputs_host, csrc/host_api.cpp) as a host AddressSanitizer + UndefinedBehaviorSanitizer build
(tools/fuzz/pack_fuzz.cpp), run the way tests/test_host_fuzz.py runs sym_fuzz: pack -> unpack round trips, rows pushed
out of the packed domain, random packed rows and perturbed parameters over every family, in heap buffers of exactly
the documented sizes. Every record must come back "ok" or "err <code>" with no sanitizer report."""
import os
import random
import shutil
import struct
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "tools", "fuzz", "build", "pack_fuzz")
sys.path.insert(0, os.path.join(REPO, "passport-zk-circuits_amd"))

from pzkwit import inputs as I, native  # noqa: E402

from test_host_fuzz import FIELDS, pack_params  # noqa: E402

FAMILIES = [(native.PZK_CIRCUIT_REGISTER, 0, I.instance_params(s)) for s in (1, 2, 3, 13, 20, 24, 25)] + [
    (native.PZK_CIRCUIT_REGISTER, 0, dict(I.instance_params(13), dg_hash=256, aa=0, dg15_blocks=0)),  # empty dg15
    (native.PZK_CIRCUIT_QUERY, 80, {}), (native.PZK_CIRCUIT_QUERY, 80, {"doc": 1}),
    (native.PZK_CIRCUIT_LIGHT, 0, dict(dg_hash=256, doc=3)), (native.PZK_CIRCUIT_LIGHT, 0, dict(dg_hash=512, doc=1)),
    (native.PZK_CIRCUIT_POSEIDON, 2, {}), (native.PZK_CIRCUIT_POSEIDON, 5, {}), (native.PZK_CIRCUIT_SHA256, 1, {}),
    (native.PZK_CIRCUIT_SHA1, 2, {}), (native.PZK_CIRCUIT_SHA384, 1, {})]


def rec(pp, n, seed, mode):
    return pp + struct.pack("<IIB", n, seed, mode)


@pytest.fixture(scope="module")
def fuzz_bin():
    if not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None:
        pytest.skip("no hipcc for the host sanitizer build")
    subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tools", "fuzz"), "build/pack_fuzz"])
    return BIN


def run(fuzz_bin, records, timeout=600):
    env = dict(os.environ, ASAN_OPTIONS="allocator_may_return_null=1:detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([fuzz_bin], input=b"".join(records), capture_output=True, timeout=timeout, env=env)
    err = p.stderr.decode(errors="replace")
    out = p.stdout.decode().splitlines()
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (out[-3:], err[-3000:])
    assert len(out) == len(records), (len(out), len(records), err[-2000:])
    return out


def test_pack_round_trips_every_family(fuzz_bin):
    """every family, modes 0-2, batches 0, 1 and 5: round trips hold, every third row of mode 1 is refused"""
    recs, want_refused = [], []
    for k, (circuit, size, prm) in enumerate(FAMILIES):
        pp, _ = pack_params(circuit, size, prm)
        for mode in (0, 1, 2):
            for n in (0, 1, 5):
                recs.append(rec(pp, n, 0x1000 * k + 16 * mode + n, mode))
                narrow = circuit != native.PZK_CIRCUIT_POSEIDON  # PoseidonHash(n) has FIELD inputs only
                want_refused.append(len(range(1, n, 3)) if mode == 1 and narrow else 0)
    out = run(fuzz_bin, recs)
    for o, w in zip(out, want_refused):
        assert o.startswith("ok ") and int(o.split()[2]) == w, (o, w)
    sizes = {int(o.split()[1]) for o in out}
    assert {3840, 3232, 160} <= sizes  # config 3, QueryIdentity TD3, Light


def test_pack_param_fuzz(fuzz_bin):
    """the template parameters perturbed around every family (tests/test_host_fuzz.py test_layout_param_fuzz): each
    instance packs and unpacks, or is rejected with PZK_E_PARAMS"""
    rng = random.Random(0xFA3)
    vals = [-(1 << 31), -1, 0, 1, 2, 3, 5, 7, 16, 20, 21, 24, 25, 64, 100, 160, 224, 256, 384, 512, 1000, 4096, 1 << 16,
            (1 << 31) - 1]
    recs = []
    for circuit, size, prm in FAMILIES:
        _, f = pack_params(circuit, size, prm)
        for _ in range(12):
            g = dict(f)
            for _ in range(rng.randint(1, 2)):
                k = rng.choice(FIELDS[1:])
                g[k] = rng.choice(vals) if rng.random() < 0.7 else g[k] + rng.randint(-64, 64)
                g[k] = max(-(1 << 31), min((1 << 31) - 1, g[k]))
            recs.append(rec(struct.pack("<12i", *[g[k] for k in FIELDS]), 2, rng.randrange(1 << 32), rng.randrange(3)))
    out = run(fuzz_bin, recs, timeout=900)
    assert all(o.startswith("ok ") or o.startswith("err -") for o in out), [o for o in out if o[:2] not in ("ok", "er")]
    assert sum(o.startswith("ok") for o in out) >= 20 and sum(o.startswith("err") for o in out) >= 20
