"""GPU: packed input rows (include/pzkwit.h). k_unpack_inputs alone against the host unpack and the
original rows, then the packed entry points against the unpacked ones (the oracle-tested path: parity by
transitivity) — whole batches, a lane outside the field, calls left in flight over the scratch sets, the chunked
path of a non-monotone map, and a caller stream."""
import numpy as np
import pytest
import torch

import light_ref as R
import packed_ref as PR
from pzkwit import field, inputs as I, light, native, query as Q, symmap

pytestmark = pytest.mark.gpu

UNPACK_WT = 8  # csrc/unpack.hpp: witnesses per tile of k_unpack_inputs
ST_INPUT_RANGE = 64
LIGHT = dict(dg_hash=256, doc=3)
DEV = "cuda:0"

_instances = {}


def instance(name):
    """one instance per family for the whole module"""
    if name not in _instances:
        _, circuit, size, params, _ = PR.BY_ID[name]
        _instances[name] = native.Instance(circuit, size, params or None)
    return _instances[name]


@pytest.fixture(scope="module", autouse=True)
def _close_instances():
    yield
    for inst in _instances.values():
        inst.close()
    _instances.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def line_rows():
    """distinct in-domain rows of the three lines, generated once: 7 register, 8 query, 8 Light"""
    g = I.PassportGen(seed=0x7A, n_keys=1, workers=1)
    return {"register_canonical": np.stack([I.pack_register_inputs(g.passport_at(i, smt_depth=5 * i)) for i in range(7)]),
            "query_td3": Q.batch_rows(8, seed=0x7B),
            "light_256_3": light.batch_rows(8, seed=0x7C)}


def tiled(rows, batch, shift=0):
    return rows[(np.arange(batch) + shift) % rows.shape[0]]


@pytest.mark.parametrize("batch", [1, 3, UNPACK_WT + 1])
@pytest.mark.parametrize("name", ["register_canonical", "register_no_dg15", "query_td3", "query_td1", "light_256_3",
                                  "poseidon_2", "sha256_1"])
def test_unpack_kernel(name, batch):
    """pzk_unpack_inputs alone, batches 1, 3 and 9: a workgroup of k_unpack_inputs takes UNPACK_WT = 8 witnesses per
    tile (unpack.hpp), so 9 is the smallest batch that crosses a tile by an odd remainder. Rows over the whole packed
    domain (random bits; limbs with 0 and 2^64 - 1; field elements with 0, p - 1, p, 2^256 - 1) into a destination
    pre-filled with 0xFF: the device rows equal unpack_inputs_host and the original rows byte for byte — the zero
    high bytes, group boundaries inside a wave (slaveMerkleRoot then bits at element 1; the query's 16 scalars then
    93 bytes of bits), an empty group, and the partial last wave of a row."""
    _, circuit, size, params, groups = PR.BY_ID[name]
    inst = instance(name)
    rows = PR.edge_rows(groups, batch, 0x51 + batch)
    packed, st = native.pack_inputs(rows, params, circuit, size)
    assert (st == 0).all() and packed.shape[1] == inst.packed_row_bytes
    host = native.unpack_inputs_host(packed, params, circuit, size)
    np.testing.assert_array_equal(host, rows)
    d_packed = torch.from_numpy(packed).to(DEV)
    d_rows = torch.full((batch, inst.n_inputs, 32), 0xFF, dtype=torch.uint8, device=DEV)
    guard = torch.full((4096,), 0xFF, dtype=torch.uint8, device=DEV)  # (allocated right behind: stays 0xFF)
    torch.cuda.synchronize()  # the library's streams do not wait for torch's
    inst.unpack_inputs_device(d_packed.data_ptr(), batch, d_rows.data_ptr(), sync=True)
    got = d_rows.cpu().numpy()
    bad = np.argwhere(got != rows)
    assert bad.size == 0, "%d bytes differ, first (row, element, byte) %s" % (bad.shape[0], bad[:5].tolist())
    assert bool((guard == 0xFF).all())


def test_unpack_domain_covered():
    """the rows of test_unpack_kernel hold every edge value the issue names"""
    groups = PR.register_groups(I.CANONICAL)
    rows = PR.edge_rows(groups, 3, 0x51 + 3)
    _, _, el = PR.layout(groups)
    limbs = rows[:, el[5]:el[7], :8].reshape(-1, 8)
    assert (limbs == 0).all(axis=1).any() and (limbs == 255).all(axis=1).any()
    fe = {rows[b, e].tobytes() for b in range(3) for e in [0] + list(range(el[7], el[7] + 81))}
    for v in (0, field.P - 1, field.P, (1 << 256) - 1):
        assert v.to_bytes(32, "little") in fe, hex(v)


def test_unpack_rejects_bad_arguments():
    inst = instance("poseidon_2")
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    with pytest.raises(native.PzkError):
        inst.unpack_inputs_device(buf.data_ptr() + 8, 1, buf.data_ptr() + 1024)  # packed rows not 16-byte aligned
    with pytest.raises(native.PzkError):
        inst.unpack_inputs_device(buf.data_ptr(), 1, buf.data_ptr() + 1032)
    with pytest.raises(native.PzkError):
        inst.unpack_inputs_device(0, 1, buf.data_ptr())
    with pytest.raises(native.PzkError):
        inst.witness_batch_packed_device(buf.data_ptr() + 4, 1, buf.data_ptr() + 1024, 32 * inst.witness_size)


@pytest.mark.parametrize("batch", [3, 37])
@pytest.mark.parametrize("name", ["register_canonical", "query_td3", "light_256_3"])
def test_packed_equals_unpacked(oracle, line_rows, name, batch):
    """witness_batch_host_packed(pack(rows)) == witness_batch_host(rows) in every witness byte and every status;
    for Light also tests/light_ref.py's element check on one row"""
    _, circuit, size, params, _ = PR.BY_ID[name]
    inst = instance(name)
    rows = tiled(line_rows[name], batch)
    packed, pst = native.pack_inputs(rows, params, circuit, size)
    assert (pst == 0).all()
    want, want_st = inst.witness_batch_host(rows)
    got, got_st = inst.witness_batch_host_packed(packed)
    np.testing.assert_array_equal(got_st, want_st)
    assert (want_st == 0).all(), want_st
    for b in range(batch):  # row by row: a 37 x 72 MB comparison in one expression doubles the peak memory
        assert np.array_equal(got[b], want[b]), "row %d: first element %d" % (
            b, np.nonzero((got[b] != want[b]).any(axis=1))[0][0])
    if name == "light_256_3":
        ref, _ = R.expected_row(oracle, 256, 3, rows[batch - 1])
        assert not R.mismatch_report(ref, got[batch - 1], R.region_table(256, 3))


def test_packed_range_semantics(line_rows):
    """a 32-row Light batch whose row 13 has skIdentity = p: the packed row keeps the 32 bytes, the lane reports
    PZK_ST_INPUT_RANGE through the packed path, and the other 31 rows equal the unpacked result"""
    inst = instance("light_256_3")
    rows = tiled(line_rows["light_256_3"], 32).copy()
    rows[13, 1024] = R.el(field.P)
    packed, pst = native.pack_inputs(rows, LIGHT, native.PZK_CIRCUIT_LIGHT)
    assert (pst == 0).all()  # a scalar >= p is representable
    want, want_st = inst.witness_batch_host(rows)
    got, got_st = inst.witness_batch_host_packed(packed)
    assert got_st[13] == ST_INPUT_RANGE and want_st[13] == ST_INPUT_RANGE
    others = np.arange(32) != 13
    assert (got_st[others] == 0).all()
    assert np.array_equal(got[others], want[others])


@pytest.mark.parametrize("name", ["query_td3", "light_256_3"])
def test_packed_calls_in_flight(line_rows, name):
    """2 x pipeline_depth + 1 packed device calls on a NULL stream, back to back, each with its own inputs and its own
    output buffers, one sync at the end: every call equals the unpacked result of its rows. Every scratch set's
    expanded rows are written three (or two) times while earlier calls may still read them."""
    _, circuit, size, params, _ = PR.BY_ID[name]
    inst = instance(name)
    W, B = inst.witness_size, 5
    n_calls = 2 * inst.pipeline_depth + 1
    want = {}
    calls = []
    for k in range(n_calls):
        rows = tiled(line_rows[name], B, shift=k)
        key = k % line_rows[name].shape[0]
        if key not in want:
            want[key] = inst.witness_batch_host(rows)
        packed, pst = native.pack_inputs(rows, params, circuit, size)
        assert (pst == 0).all()
        calls.append((key, torch.from_numpy(packed).to(DEV), torch.full((B, W, 32), 0xFF, dtype=torch.uint8, device=DEV),
                      torch.full((B,), -1, dtype=torch.int32, device=DEV)))
    torch.cuda.synchronize()
    for _, d_in, out, st in calls:
        inst.witness_batch_packed_device(d_in.data_ptr(), B, out.data_ptr(), 32 * W, st.data_ptr())
    inst.sync()
    for k, (key, _, out, st) in enumerate(calls):
        w, s = want[key]
        assert np.array_equal(st.cpu().numpy(), s), k
        assert np.array_equal(out.cpu().numpy(), w), k
    del calls
    torch.cuda.empty_cache()


def test_packed_mapped_chunking():
    """Sha256HashChunks(1) under a non-monotone .sym map (two kept signals with swapped witness indices), batch 1025:
    batch_mapped runs two chunks (1024 + 1), the second one's packed pointer advanced by row_bytes per witness.
    Packed equals unpacked on all 1025 rows."""
    n_o0 = int(native.layout_info({}, native.PZK_CIRCUIT_SHA256, 1).witness_size)
    lines = symmap.sym_text(symmap.synthetic_keep(n_o0, 1 + 256 + 512, fraction=3)).splitlines()
    kept = [i for i, ln in enumerate(lines) if int(ln.split(",")[1]) > 800]
    a, b = kept[10], kept[2000]
    la, lb = lines[a].split(","), lines[b].split(",")
    la[1], lb[1] = lb[1], la[1]
    lines[a], lines[b] = ",".join(la), ",".join(lb)
    txt = "\n".join(lines) + "\n"
    assert (np.diff(symmap.parse_sym(txt)[1:]) < 0).any()
    inst = native.Instance(native.PZK_CIRCUIT_SHA256, 1, sym=txt)
    try:
        rows = PR.edge_rows([(PR.BIT, 512)], 1025, 0x61)
        packed, pst = native.pack_inputs(rows, None, native.PZK_CIRCUIT_SHA256, 1)
        assert (pst == 0).all()
        want, want_st = inst.witness_batch_host(rows)
        got, got_st = inst.witness_batch_host_packed(packed)
        assert (want_st == 0).all() and np.array_equal(got_st, want_st)
        assert np.array_equal(got, want)
        assert not np.array_equal(want[1024], want[0])  # (the last row is its own)
    finally:
        inst.close()


def test_packed_caller_stream(line_rows):
    """one packed device call with exec.stream set and PZK_EXEC_SYNC, the inputs uploaded on that stream"""
    inst = instance("light_256_3")
    W, B = inst.witness_size, 6
    rows = tiled(line_rows["light_256_3"], B, shift=2)
    packed, _ = native.pack_inputs(rows, LIGHT, native.PZK_CIRCUIT_LIGHT)
    want, want_st = inst.witness_batch_host(rows)
    s = torch.cuda.Stream(device=DEV)
    h_packed = torch.from_numpy(packed).pin_memory()
    with torch.cuda.stream(s):
        d_in = h_packed.to(DEV, non_blocking=True)
        out = torch.full((B, W, 32), 0xFF, dtype=torch.uint8, device=DEV)
        st = torch.full((B,), -1, dtype=torch.int32, device=DEV)
        inst.witness_batch_packed_device(d_in.data_ptr(), B, out.data_ptr(), 32 * W, st.data_ptr(), stream=s.cuda_stream,
                                         sync=True)
    assert np.array_equal(st.cpu().numpy(), want_st)
    assert np.array_equal(out.cpu().numpy(), want)
