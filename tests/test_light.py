"""CPU: the RegisterIdentityLight(DG_HASH_TYPE, DOCUMENT_TYPE) family (PZK_CIRCUIT_LIGHT,
identityManagement/registerIdentityLight.circom:15-92) through the host-only half of the C-ABI: layout sizes against
the witness the tests assemble from oracle output (tests/light_ref.py), the region table, the input groups, parameter
rejections, input marshalling and the .sym check. tests/test_gpu_light.py runs the same instances on the device."""
import ctypes

import numpy as np
import pytest

import light_ref as R
from pzkwit import field, inputs as I, light, native, symmap, witness_calculator as WC


def layout(dg, doc):
    p = R.light_params(dg, doc)
    info, n = native.PzkInfo(), ctypes.c_uint32()
    rc = native.lib().pzk_layout_query(ctypes.byref(p), ctypes.byref(info), ctypes.byref(n))
    return rc, info, n.value


def input_groups(dg, doc):
    """the instance's named inputs without a device: the host layout reports their number and the row length;
    pzk_instance_input needs an instance, so tests/test_gpu_light.py checks light.GROUPS against it"""
    rc, info, _ = layout(dg, doc)
    assert rc == 0 and info.n_input_groups == len(light.GROUPS)
    assert sum(ln for _, _, ln in light.GROUPS) == info.n_inputs
    return light.GROUPS


@pytest.mark.parametrize("dg,doc", R.PAIRS)
def test_light_layout(oracle, dg, doc):
    rc, info, n_regions = layout(dg, doc)
    assert rc == 0, native.lib().pzk_last_error()
    assert (info.n_inputs, info.n_outputs, info.n_public_inputs, info.n_input_groups) == (1025, 3, 0, 2)
    # witness_size = the length of the witness assembled from oracle blocks and the template signal counts
    assert info.witness_size == R.witness_size(oracle, dg, doc)
    bits = I.padded_bits(bytes(range(93 if doc == 3 else 95)), light.block_bits(dg))
    if dg in (256, 384):  # (one full assembly per block size: the others differ in the SHA block only)
        w, _ = R.expected(oracle, dg, doc, bits, 5)
        assert w.shape[0] == info.witness_size
    # the regions tile the witness (test_capi.py::test_regions_tile_the_witness)
    pos = 0
    for off, ln, _ in sorted(R.region_table(dg, doc)):
        assert off == pos and ln > 0
        pos += ln
    assert pos == info.witness_size and n_regions == len(R.region_table(dg, doc))
    # native.layout_inputs / layout_info report the input row and its two groups
    prm = dict(dg_hash=dg, doc=doc)
    assert native.layout_inputs(prm, native.PZK_CIRCUIT_LIGHT) == 1025
    assert native.layout_witness_size(prm, native.PZK_CIRCUIT_LIGHT) == info.witness_size
    assert native.layout_info(prm, native.PZK_CIRCUIT_LIGHT).n_input_groups == 2


def test_light_ignores_other_params():
    """every pzk_params field but dg_hash_type / document_type is ignored"""
    p = R.light_params(256, 3)
    q = native.PzkParams(circuit=native.PZK_CIRCUIT_LIGHT, dg_hash_type=256, document_type=3, size_arg=9,
                         signature_type=99, ec_block_number=-1, ec_shift=7, dg1_shift=-5, aa_signature_algo=77,
                         dg15_shift=1, dg15_block_number=99, aa_shift=-3)
    a, b = native.PzkInfo(), native.PzkInfo()
    assert native.lib().pzk_layout_query(ctypes.byref(p), ctypes.byref(a), None) == 0
    assert native.lib().pzk_layout_query(ctypes.byref(q), ctypes.byref(b), None) == 0
    assert a.witness_size == b.witness_size


@pytest.mark.parametrize("dg,doc,name", [(0, 3, "dg_hash_type"), (255, 3, "dg_hash_type"), (320, 3, "dg_hash_type"),
                                         (1024, 3, "dg_hash_type"), (256, 0, "document_type"),
                                         (256, 2, "document_type")])
def test_light_rejections(dg, doc, name):
    rc, _, _ = layout(dg, doc)
    assert rc == -2  # PZK_E_PARAMS
    assert name.encode() in native.lib().pzk_last_error(), native.lib().pzk_last_error()
    n = ctypes.c_uint64()
    p = R.light_params(dg, doc)
    assert native.lib().pzk_sym_check(ctypes.byref(p), b"1,1,0,s\n", 8, ctypes.byref(n)) == -2
    assert native.lib().pzk_layout_region(ctypes.byref(p), 0, None, None, None) == -2


@pytest.mark.parametrize("dg", [256, 512])
def test_light_json_marshals_like_pack(dg):
    """a reference-style input JSON through the host-only marshalling path = light.pack's row"""
    dg1 = bytes.fromhex("615b5f1f58") + bytes(65 + i % 26 for i in range(88))
    sk = field.SplitMix64(dg).fr()
    row = light.pack(dg1, sk, dg)
    js = {"dg1": [str(int(b)) for b in light.dg1_bits(dg1, dg)], "skIdentity": hex(sk)}
    got = WC.marshal_inputs(input_groups(dg, 3), 1025, js)
    assert got.shape == row.shape and (got == row).all()
    with pytest.raises(WC.WitnessError, match="Not enough values for input signal dg1"):
        WC.marshal_inputs(input_groups(dg, 3), 1025, {"dg1": js["dg1"][:-1], "skIdentity": "1"})
    with pytest.raises(WC.WitnessError, match="Signal slaveMerkleRoot not found"):
        WC.marshal_inputs(input_groups(dg, 3), 1025, dict(js, slaveMerkleRoot="0"))


def test_light_public_outputs_formulas():
    """light.public_outputs against direct restatements: hashlib's digest mod 2^248, the dg1 commitment of
    tests/refmath.py (TD3), Poseidon2 of refmath's BabyJubJub multiplication"""
    import hashlib
    from refmath import bjj_mul, dg1_commitment
    dg1 = bytes.fromhex("615b5f1f58") + bytes(48 + i % 10 for i in range(88))
    sk = field.SplitMix64(7).fr()
    for dg, hf in ((160, hashlib.sha1), (224, hashlib.sha224), (256, hashlib.sha256), (384, hashlib.sha384),
                   (512, hashlib.sha512)):
        c, h, k = light.public_outputs(dg1, sk, dg, 3)
        assert h == int.from_bytes(hf(dg1).digest(), "big") % (1 << 248)
        assert c == dg1_commitment(dg1, sk)  # the 744 message bits do not depend on the block size
        assert k == field.poseidon(list(bjj_mul(sk)))


def test_light_sym_check(oracle):
    """pzk_sym_check accepts a .sym over the Light O0 numbering and reports the kept count + 1"""
    W = R.witness_size(oracle, 256, 3)
    keep = symmap.synthetic_keep(W, 1 + 3 + 1025)
    sym = symmap.sym_text(keep)
    n = native.sym_check(dict(dg_hash=256, doc=3), sym, native.PZK_CIRCUIT_LIGHT)
    assert n == int(keep[1:].sum()) + 1
    with pytest.raises(native.PzkError, match="outside"):
        native.sym_check(dict(dg_hash=256, doc=3), "%d,1,0,s\n" % W, native.PZK_CIRCUIT_LIGHT)
