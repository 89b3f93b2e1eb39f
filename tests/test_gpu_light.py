"""GPU: RegisterIdentityLight(DG_HASH_TYPE, DOCUMENT_TYPE) (PZK_CIRCUIT_LIGHT,
identityManagement/registerIdentityLight.circom:15-92) element for element against the witness tests/light_ref.py
assembles from oracle output and independent math: every hash algorithm, unpadded inputs, batch shapes around the
kernels' workgroup sizes, the scalar edges, out-of-domain lanes, calls left in flight, a .sym-mapped instance and
streamed delivery."""
import struct

import numpy as np
import pytest

import light_ref as R
from pzkwit import field, inputs as I, light, native, symmap

pytestmark = pytest.mark.gpu

P = field.P
ST_INPUT_RANGE = 64


def instance(dg, doc, sym=None):
    return native.Instance(native.PZK_CIRCUIT_LIGHT, 0, dict(dg_hash=dg, doc=doc), sym=sym)


def dg1_of(gen, i, doc):
    """a synthetic DG1 from the passport stream: 93 bytes (TD3), or 95 bytes with the TD1 header (three 30-character
    MRZ lines: the passport's 88 MRZ characters and the first two again)"""
    pp = gen.passport_at(i)
    if doc == 3:
        return pp["dg1"], pp["sk"]
    return bytes.fromhex("615d5f1f5a") + pp["dg1"][5:] + pp["dg1"][5:7], pp["sk"]


@pytest.fixture(scope="module")
def gen():
    return I.PassportGen(seed=0x11, n_keys=1, workers=1)


def rows_of(gen, idx, dg, doc, rng=None):
    """Light rows of passports idx: properly padded DG1s; random keys from rng (else the passports' own)"""
    out = []
    for i in idx:
        dg1, sk = dg1_of(gen, i, doc)
        out.append(light.pack(dg1, rng.fr() if rng else sk, dg))
    return np.stack(out)


def check_rows(oracle, dg, doc, rows, wit, st, which=None):
    regions = R.region_table(dg, doc)
    reports = []
    for b in (range(rows.shape[0]) if which is None else which):
        ref, _ = R.expected_row(oracle, dg, doc, rows[b])
        rep = R.mismatch_report(ref, wit[b], regions)
        if rep:
            reports.append("row %d: %s" % (b, rep))
        assert st[b] == 0, (b, st)
    assert not reports, "\n".join(reports)


@pytest.mark.parametrize("dg,doc", [(160, 3), (224, 3), (256, 3), (384, 3), (512, 3), (256, 1)])
def test_light_parity(oracle, gen, dg, doc):
    """every algorithm: 3 padded DG1s with random keys; every element, status 0, the outputs = light.public_outputs"""
    inst = instance(dg, doc)
    assert inst.input_groups == light.GROUPS
    assert (inst.n_inputs, inst.n_outputs, inst.n_public_inputs) == (1025, 3, 0)
    assert inst.witness_size == R.witness_size(oracle, dg, doc)
    rng = field.SplitMix64(0xA0 + dg)
    rows = rows_of(gen, range(3), dg, doc, rng)
    wit, st = inst.witness_batch_host(rows)
    check_rows(oracle, dg, doc, rows, wit, st)
    for b in range(3):
        dg1, _ = dg1_of(gen, b, doc)
        want = light.public_outputs(dg1, R.to_int(rows[b, 1024]), dg, doc)
        assert tuple(R.to_int(wit[b, 1 + k]) for k in range(3)) == want, b


@pytest.mark.parametrize("dg", [256, 384])
def test_light_unpadded_input(oracle, dg):
    """dg1 = 1024 random bits, not a padded message: the circuit hashes what it is given"""
    rng = field.SplitMix64(0xB0 + dg)
    row = np.zeros((1, 1025, 32), dtype=np.uint8)
    row[0, :1024, 0] = [(rng.next() >> 17) & 1 for _ in range(1024)]
    row[0, 1024] = R.el(rng.fr())
    wit, st = instance(dg, 3).witness_batch_host(row)
    check_rows(oracle, dg, 3, row, wit, st)


@pytest.mark.parametrize("batch", [1, 37, 65])
def test_light_batch_shapes(oracle, gen, batch):
    """batches of 1, 37 (one past a 32-witness group plus a partial 8-wide group of the shared kernels) and 65:
    k_light_prep's workgroup covers 64 witnesses (LIGHT_PREP_THREADS, light.hpp), so 65 is the smallest batch that
    crosses its boundary by an odd remainder. Seven distinct inputs repeat along the batch (7 and 64 are coprime, so
    every lane position meets every input); every row is compared."""
    uniq = rows_of(gen, range(7), 256, 3, field.SplitMix64(0xC0))
    rows = uniq[np.arange(batch) % 7]
    wit, st = instance(256, 3).witness_batch_host(rows)
    check_rows(oracle, 256, 3, rows, wit, st)


def test_light_scalar_edges(oracle):
    """sk in {0, 1, 2, 2^248, 2^251 + x, 2^253 + x, p - 2, p - 1} (tests/test_scalar_edges.py): the same passports and
    scalars through an oracle register witness; the Light lane's BabyJubJub block, pkIdentityHash and status equal the
    oracle's tail and its check-site code"""
    from test_scalar_edges import EDGE_SK, edge_rows
    g = I.PassportGen(seed=0x5C, n_keys=1, workers=1)
    reg_rows = edge_rows(g)
    rows = np.stack([light.pack(g.passport_at(k)["dg1"], sk, 256) for k, sk in enumerate(EDGE_SK)])
    wit, st = instance(256, 3).witness_batch_host(rows)
    prm = oracle.register_params(**I.CANONICAL)
    T = R.tail_size(oracle, 3)
    bjj_off = R.pos_size(oracle, 5) + 4 * R.sz_bits2num(186) + R.pos_size(oracle, 1)  # inside the tail
    tail0 = R.positions(oracle, 256, 3)["tail"][0]
    for b, sk in enumerate(EDGE_SK):
        rc, ref = oracle.register_witness(prm, reg_rows[b])
        tail = ref[-T:]
        assert st[b] == rc, (hex(sk), st[b], rc)
        got = wit[b, tail0 + bjj_off: tail0 + bjj_off + R.SZ_BJJ]
        bad = np.nonzero((got != tail[bjj_off: bjj_off + R.SZ_BJJ]).any(axis=1))[0]
        assert bad.size == 0, "sk %s: %d BabyJubJub elements differ, first %s" % (hex(sk), bad.size, bad[:6])
        assert (wit[b, 3] == tail[bjj_off + R.SZ_BJJ]).all(), hex(sk)  # pkIdentityHash = pkIdentityHasher.out
        assert (wit[b, tail0: tail0 + T] == tail).all(), hex(sk)       # (and the whole tail)


def test_light_out_of_domain_lanes(oracle, gen):
    """row 1: a dg1 element equal to 2; row 3: skIdentity = p. Both report PZK_ST_INPUT_RANGE; rows 0, 2 and 4 are
    bit-exact with status 0"""
    rows = rows_of(gen, range(10, 15), 256, 3, field.SplitMix64(0xD0))
    rows[1, 10, 0] = 2
    rows[3, 1024] = R.el(P)
    wit, st = instance(256, 3).witness_batch_host(rows)
    assert st[1] == ST_INPUT_RANGE and st[3] == ST_INPUT_RANGE, st
    check_rows(oracle, 256, 3, rows, wit, st, which=(0, 2, 4))


def test_light_calls_in_flight(oracle, gen):
    """four back-to-back pzk_witness_batch calls with a NULL stream (more than the three scratch sets), distinct
    inputs, batch 5, then pzk_instance_sync (tests/test_gpu_pipeline.py): every call's rows are correct"""
    import torch
    inst = instance(256, 3)
    pool = rows_of(gen, range(20, 26), 256, 3, field.SplitMix64(0xE0))
    dev = torch.device("cuda:0")
    W, calls = inst.witness_size, []
    for k in range(4):
        rows = pool[(np.arange(5) + k) % 6]  # every call: another window of the six inputs
        calls.append((rows, torch.from_numpy(rows).to(dev), torch.empty((5, W, 32), dtype=torch.uint8, device=dev),
                      torch.full((5,), -1, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()  # the library's streams do not wait for torch's stream (the buffers' fills)
    for rows, d_in, out, st in calls:
        inst.witness_batch_device(d_in.data_ptr(), 5, out.data_ptr(), 32 * W, st.data_ptr())
    inst.sync()
    for rows, d_in, out, st in calls:
        check_rows(oracle, 256, 3, rows, out.cpu().numpy(), st.cpu().numpy())
    del calls
    torch.cuda.empty_cache()


def _keep_map(oracle):
    W = R.witness_size(oracle, 256, 3)
    keep = symmap.synthetic_keep(W, 1 + 3 + 1025)
    txt = symmap.sym_text(keep)
    return txt, symmap.parse_sym(txt)


def test_light_mapped(oracle, gen):
    """pzk_instance_create_mapped with the synthetic keep map of tests/test_light.py: element k = the expected O0
    element whose witness index is k; the .wtns header reports the mapped size"""
    txt, inv = _keep_map(oracle)
    inst = instance(256, 3, sym=txt)
    assert inst.witness_size == len(inv) < R.witness_size(oracle, 256, 3)
    rows = rows_of(gen, range(30, 33), 256, 3, field.SplitMix64(0xF0))
    wit, st = inst.witness_batch_host(rows)
    assert (st == 0).all(), st
    for b in range(3):
        ref, _ = R.expected_row(oracle, 256, 3, rows[b])
        bad = np.nonzero((ref[inv] != wit[b]).any(axis=1))[0]
        assert bad.size == 0, "row %d: %d mapped elements differ, first %s (O0 %s)" % (b, bad.size, bad[:6], inv[bad[:6]])
    assert struct.unpack_from("<I", inst.wtns_header(), 60)[0] == len(inv)


def test_light_stream_and_wtns(oracle, gen):
    """pzk_witness_stream with chunk = 2 over 5 rows delivers the rows of witness_batch_host; the .wtns header
    carries witness_size"""
    inst = instance(256, 3)
    rows = rows_of(gen, range(40, 45), 256, 3, field.SplitMix64(0xF8))
    want, want_st = inst.witness_batch_host(rows)
    check_rows(oracle, 256, 3, rows, want, want_st, which=(0, 4))
    got = np.zeros_like(want)
    got_st = np.full(5, -1, dtype=np.int32)
    order = []

    def sink(first, w, st):
        order.append((first, w.shape[0]))
        got[first: first + w.shape[0]] = w
        got_st[first: first + w.shape[0]] = st

    inst.witness_stream(rows, sink, chunk=2)
    assert order == [(0, 2), (2, 2), (4, 1)]
    assert (got_st == want_st).all() and (got == want).all()
    hdr = inst.wtns_header()
    assert hdr[:4] == b"wtns" and struct.unpack_from("<I", hdr, 60)[0] == inst.witness_size
    assert struct.unpack_from("<Q", hdr, 68)[0] == 32 * inst.witness_size
