"""GPU: the SHA-256 emitter's store loop (k_emit_sha stage 2, kernels.hip). A wave takes groups of 64 consecutive
elements of a work item's run, evaluates each element once (one per lane) and writes a group with two wave stores
whose lanes fetch the values across the wave (store_pair, mapsink.hpp). What can go wrong is the geometry: runs shorter
than a group, runs that end inside a group's first or second store, runs longer than one full iteration of the
workgroup with a ragged end, and lanes past the run taking part in the exchange. PZK_CHUNK_1 (E_SHA = 1) sets the work
items' length, so the chunk sizes below put the run ends where those paths split; every row is compared element for
element with the CPU oracle (O0) or with the O0 instance's rows on the device (mapped: kept counts per work item are
arbitrary). PZK_CHUNK_<e> is read when an instance is created, PZK_SHA_U once per process (hence the child runs)."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# work-item lengths: below one group (33, 63), exactly one (64), one element / 33 elements into the next (65, 97),
# one workgroup iteration at PZK_SHA_U = 16 (2,048 elements) less one and plus one, the default (4,096: one full
# iteration at the default PZK_SHA_U = 32, two at 16; a block's last default chunk, 150,762 - 36 * 4,096 = 3,306
# elements, ends 42 into a group), one full iteration at 32 plus one element, and two plus a ragged end
CHUNKS = [33, 63, 64, 65, 97, 2047, 2049, None, 4097, 8300]
BATCH = 3


@contextlib.contextmanager
def chunk_env(chunk, emitters=(1,)):
    names = ["PZK_CHUNK_%d" % e for e in emitters]
    old = {n: os.environ.get(n) for n in names}
    try:
        for n in names:
            if chunk is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = str(chunk)
        yield
    finally:
        for n, v in old.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v


_sha_ref = {}


def sha_case(oracle, blocks):
    """(input rows, oracle witnesses) of Sha256HashChunks(blocks), batch 3: computed once, never modified."""
    if blocks not in _sha_ref:
        from pzkwit import inputs
        _, rows = inputs.sha256_config2_batch(BATCH, seed=0x5E + blocks, blocks=blocks)
        refs = []
        for b in range(BATCH):
            rc, ref = oracle.sha256_witness(rows[b], blocks)
            assert rc == 0
            ref.setflags(write=False)
            refs.append(ref)
        _sha_ref[blocks] = (rows, refs)
    return _sha_ref[blocks]


def check_sha(oracle, blocks, chunk):
    from pzkwit import native
    rows, refs = sha_case(oracle, blocks)
    with chunk_env(chunk):
        inst = native.Instance(native.PZK_CIRCUIT_SHA256, blocks)
    wit, st = inst.witness_batch_host(rows)
    assert (st == 0).all(), st
    for b in range(BATCH):
        assert wit[b].shape == refs[b].shape
        bad = np.nonzero((refs[b] != wit[b]).any(axis=1))[0]
        assert bad.size == 0, "blocks %d chunk %s row %d: %d elements differ, first %s" % (
            blocks, chunk, b, bad.size, bad[:8].tolist())


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("blocks", [1, 2])
def test_sha256_rows_equal_oracle_at_chunk(oracle, blocks, chunk):
    check_sha(oracle, blocks, chunk)


# ---- mapped (k_emit_sha<16, MAP_DIRECT>: the kept elements' descriptors, stored consecutively) against O0
_o0 = {}


def o0_rows():
    """(input rows on the device, the O0 instance's witness rows on the device) of the canonical register
    instance, batch 2, at the default chunk: the reference of every mapped case."""
    if not _o0:
        import torch
        from pzkwit import inputs as I, native
        g = I.PassportGen(seed=0x7A, n_keys=1, workers=1)
        rows = np.stack([I.pack_register_inputs(g.passport_at(i, smt_depth=3 * i)) for i in range(2)])
        inst = native.Instance(native.PZK_CIRCUIT_REGISTER, 0, I.CANONICAL)
        W = inst.witness_size
        d_in = torch.from_numpy(rows).cuda()
        out = torch.empty((2, W, 32), dtype=torch.uint8, device="cuda:0")
        st = torch.full((2,), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()  # the library's streams do not wait for torch's stream
        inst.witness_batch_device(d_in.data_ptr(), 2, out.data_ptr(), 32 * W, st.data_ptr(), sync=True)
        assert bool((st == 0).all())
        _o0["v"] = (d_in, out, int(rows.shape[1]))
    return _o0["v"]


@pytest.mark.parametrize("chunk", [None, 97])
@pytest.mark.parametrize("fraction,salt", [(2, 0x5A), (2, 0x33), (3, 0x5A), (3, 0x33), (7, 0x5A), (7, 0x33)])
def test_mapped_rows_equal_o0_rows_on_device(fraction, salt, chunk):
    import torch
    from pzkwit import inputs as I, native, symmap
    d_in, out0, n_in = o0_rows()
    keep = symmap.synthetic_keep(out0.shape[1], 1 + 4 + n_in, fraction=fraction, salt=salt)
    txt = symmap.sym_text(keep)
    inv = np.concatenate([[0], np.flatnonzero(keep[1:]) + 1])  # parse_sym(txt) of a map without merged signals
    with chunk_env(chunk, emitters=(1, 9)):  # E_SHA and E_SHAD
        mp = native.Instance(native.PZK_CIRCUIT_REGISTER, 0, I.CANONICAL, sym=txt)
    Wm = mp.witness_size
    assert Wm == inv.shape[0]
    outm = torch.empty((2, Wm, 32), dtype=torch.uint8, device="cuda:0")
    st = torch.full((2,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    mp.witness_batch_device(d_in.data_ptr(), 2, outm.data_ptr(), 32 * Wm, st.data_ptr(), sync=True)
    assert bool((st == 0).all())
    d_inv = torch.from_numpy(inv).cuda()
    bad = torch.nonzero((out0[:, d_inv] != outm).any(dim=2))
    assert bad.shape[0] == 0, "fraction %d salt %#x chunk %s: %d mapped elements differ, first (row, k) %s" % (
        fraction, salt, chunk, bad.shape[0], bad[:4].tolist())


# ---- PZK_SHA_U = 8 / 16 / 32 (stores in flight per wave and iteration): the switch is read once per process
def _child(u):
    """Runs in a fresh process: chunk 65 and the default, Sha256HashChunks(1) and (2)."""
    import conftest  # noqa: F401  (the suite's import paths)
    import pyoracle
    pyoracle.lib()
    assert os.environ["PZK_SHA_U"] == str(u)
    for blocks in (1, 2):
        for chunk in (65, None):
            check_sha(pyoracle, blocks, chunk)
    print("sha_u %d ok" % u)


@pytest.mark.parametrize("u", [8, 16, 32])
def test_sha_u_variants_in_child_process(u):
    env = dict(os.environ, PZK_SHA_U=str(u))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), str(u)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sha_u %d ok" % u in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child(int(sys.argv[1]))
