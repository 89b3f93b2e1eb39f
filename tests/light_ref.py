"""The expected RegisterIdentityLight(DG, doc) witness, assembled element for element from oracle output and
independent math — never from the library under test (tests/test_light.py, tests/test_gpu_light.py).

Every component of the circuit (identityManagement/registerIdentityLight.circom:15-92) also occurs, with identical
inputs, in witnesses the CPU oracle already produces:

* the tail dg1Hasher .. pkIdentityHasher is the last T elements of a RegisterIdentityBuilder witness with the same
  DOCUMENT_TYPE, the same skIdentity and a dg1 that agrees on its first 4 CH bits (identity.circom:89-120 ends the
  register circuit with the same components in the same creation order);
* dg1ShaHasher = ShaHashChunks(B, DG) (hasher/hash.circom:32-68) is the wrapper's out[DG] | in[1024] followed by the
  standalone hasher's witness without its leading 1 (224: the first hasher block of a register witness with
  DG_HASH_TYPE 224, which has no standalone oracle entry);
* the main block and b2n = Bits2Num(248) are computed here.

Block positions follow the --O0 rule: witness[0] = 1, then each component is its own signals (outputs,
inputs, intermediates in declaration order) followed by its subcomponents in creation order.
"""
import functools

import numpy as np

from pzkwit import field, inputs as I, light

P = field.P
DGS = (160, 224, 256, 384, 512)
PAIRS = [(dg, doc) for dg in DGS for doc in (1, 3)]

# signal counts read off the templates
SZ_N2B254 = (254 + 1 + 254) + 254 + (1 + 254 + 127 + 1) + (135 + 1 + 135)
#   Num2Bits(254) (bitify/bitify.circom:10-36: out[254] | in | sum[254]) + AliasCheck (aliascheck.circom:7-14: in[254])
#   + CompConstant (compconstant.circom:7-55: out | in[254] | parts[127], sout) + its Num2Bits(135)
SZ_BJJ = (2 + 1 + 2) + SZ_N2B254 + (2 + 2 + 2 + 3 + 3 + 10 + 4 * 6) + 253 * (14 + 46)
#   BabyjubjubBase8Multiplication (babyjubjub/curve.circom:143-171): out[2] | scalar | GetBabyjubjubBase8 out[2];
#   Num2Bits(254) + AliasCheck; adders[0] = BabyjubjubAddition (out[2] | in1[2], in2[2] | 2 IsZero of 3 | adder of 10 |
#   4 Switchers of 6) = 46 signals; then 253 x (doubler: out[2] | in[2] | its adder of 10 = 14, adder 46)


def sz_bits2num(n):
    return 1 + n + n  # bitify/bitify.circom:38-57: out | in[n] | sum[n]


def chunk(doc):
    return 190 if doc == 1 else 186


def blocks(dg):
    return (1, 1024) if dg > 256 else (2, 512)


def _orc(oracle):
    return oracle.lib()


def pos_size(oracle, n):
    """signals of a PoseidonHash(n) block (the standalone witness without its leading 1)"""
    return int(_orc(oracle).orc_poseidon_witness_size(n)) - 1


def tail_size(oracle, doc):
    """T: dg1Hasher, dg1Chunking[0..3], skIndentityHasher, pkIdentityCalc, pkIdentityHasher"""
    return pos_size(oracle, 5) + 4 * sz_bits2num(chunk(doc)) + pos_size(oracle, 1) + SZ_BJJ + pos_size(oracle, 2)


def sha_inner_size(oracle, dg):
    L = _orc(oracle)
    if dg == 160:
        return int(L.orc_sha1_witness_size(2)) - 1
    if dg > 256:
        return int(L.orc_sha512_witness_size(1, dg)) - 1
    return int(L.orc_sha256_witness_size(2)) - 1 - (256 - dg)  # Sha224HashChunks: out[224], else as Sha256HashChunks


def witness_size(oracle, dg, doc):
    main = 1 + 3 + 1025 + dg
    return main + tail_size(oracle, doc) + (dg + 1024 + sha_inner_size(oracle, dg)) + sz_bits2num(248)


def positions(oracle, dg, doc):
    """name -> (offset, length) of the blocks, in creation order"""
    out, o = {}, 0
    for name, ln in (("main", 1 + 3 + 1025 + dg), ("tail", tail_size(oracle, doc)),
                     ("sha", dg + 1024 + sha_inner_size(oracle, dg)), ("b2n", sz_bits2num(248))):
        out[name] = (o, ln)
        o += ln
    return out


def el(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)


def els(vals):
    out = np.zeros((len(vals), 32), dtype=np.uint8)
    for i, v in enumerate(vals):
        out[i] = el(v)
    return out


def to_int(e):
    return int.from_bytes(bytes(e), "little")


def _register_row(gen_params, bits, sk):
    """a RegisterIdentityBuilder input row (any valid passport of the instance) with dg1 and skIdentity replaced"""
    g = _gen(tuple(sorted(gen_params.items())))
    row = I.pack_register_inputs(g.passport_at(0), gen_params).copy()
    hb = I.hash_block(I.sig_hash_type(gen_params["sig"]))
    in_dg1 = 1 + gen_params["ec_blocks"] * hb
    row[in_dg1:in_dg1 + 1024] = 0
    row[in_dg1:in_dg1 + 1024, 0] = bits
    row[-1] = el(sk % P)
    return row, in_dg1


@functools.lru_cache(maxsize=None)
def _gen(items):
    if items != tuple(sorted(I.CANONICAL.items())):  # one RSA-2048 signer key for every register instance used here
        return I.PassportGen(seed=0x71, params=dict(items), keys=_gen(tuple(sorted(I.CANONICAL.items()))).keys)
    return I.PassportGen(seed=0x71, n_keys=1, params=dict(items), workers=1)


_tails = {}


def register_tail(oracle, doc, bits, sk):
    """last T elements of the canonical register witness with this DOCUMENT_TYPE, dg1 and sk (the oracle completes the
    witness although the replaced dg1 fails the flow check, which is not part of the tail)"""
    key = (doc, bytes(bits[:4 * chunk(doc)]), sk)
    if key not in _tails:
        params = dict(I.CANONICAL, doc=doc)
        row, _ = _register_row(params, bits, sk)
        _, w = oracle.register_witness(oracle.register_params(**params), row)
        _tails[key] = w[-tail_size(oracle, doc):].copy()
    return _tails[key]


def sha_block(oracle, dg, bits):
    """ShaHashChunks(B, DG) block over the 1024 bits: out[DG] | in[1024] | the inner hasher's block; -> (block, out bits)"""
    in_el = np.zeros((1024, 32), dtype=np.uint8)
    in_el[:, 0] = bits
    if dg == 224:
        params = dict(I.CANONICAL, dg_hash=224)
        row, in_dg1 = _register_row(params, bits, 1)
        rc, w = oracle.register_witness(oracle.register_params(**params), row)
        n_in = row.shape[0]
        # main: 1 | outputs(4) | inputs; PassportVerificationBuilder own: passportHash | its inputs (all but skIdentity)
        # | dg1Hash[224], dg15Hash[224], ecHash[256], saHash[256], pubkeyHash, tempModulus[5]; then dg1PassportHasher
        off = 1 + 4 + n_in + 1 + (n_in - 1) + 224 + 224 + 256 + 256 + 1 + 5
        blk = w[off:off + 224 + 1024 + sha_inner_size(oracle, 224)].copy()
        assert (blk[224:224 + 1024] == in_el).all(), "register(224) block position"
        return blk, blk[:224, 0].copy()
    if dg == 160:
        rc, w = oracle.sha1_witness(in_el, 2)
    elif dg == 256:
        rc, w = oracle.sha256_witness(in_el, 2)
    else:
        rc, w = oracle.sha512_witness(in_el, 1, dg)
    assert rc == 0
    inner = w[1:]
    return np.concatenate([inner[:dg], in_el, inner]), inner[:dg, 0].copy()


def bits2num_block(in_bits):
    """Bits2Num(n): out | in[n] | sum[n], sum[k] = in[0] + .. + in[k] 2^k (the order every Bits2Num block of the oracle
    witness shows)"""
    n = len(in_bits)
    acc, sums = 0, []
    for k in range(n):
        acc += int(in_bits[k]) << k
        sums.append(acc)
    return els([acc] + [int(b) for b in in_bits] + sums)


def expected(oracle, dg, doc, bits, sk):
    """-> (expected witness (W, 32) uint8, (dg1Commitment, dg1Hash, pkIdentityHash))."""
    bits = np.asarray(bits, dtype=np.uint8)
    assert bits.shape == (1024,) and bits.max() <= 1
    key = (dg, doc, bits.tobytes(), sk)
    if key not in _expected:
        _expected[key] = _assemble(oracle, dg, doc, bits, sk)
    return _expected[key]


_expected = {}  # shared among the tests: treat the arrays as read-only


def _assemble(oracle, dg, doc, bits, sk):
    ch = chunk(doc)
    tail = register_tail(oracle, doc, bits, sk)
    sha, hbits = sha_block(oracle, dg, bits)
    n = min(248, dg)
    b2n_in = [int(hbits[dg - 1 - i]) for i in range(n)] + [0] * (248 - n)
    b2n = bits2num_block(b2n_in)
    chunks = [sum(int(bits[i * ch + j]) << j for j in range(ch)) for i in range(4)]
    commit = field.poseidon(chunks + [field.poseidon([sk % P])])
    from refmath import bjj_mul
    pkh = field.poseidon(list(bjj_mul(sk % P)))
    dg1_hash = to_int(b2n[0])
    main = np.zeros((1 + 3 + 1025 + dg, 32), dtype=np.uint8)
    main[0] = el(1)
    main[1], main[2], main[3] = el(commit), el(dg1_hash), el(pkh)
    main[4:4 + 1024, 0] = bits
    main[4 + 1024] = el(sk % P)
    main[4 + 1025:, 0] = hbits
    w = np.concatenate([main, tail, sha, b2n])
    assert w.shape[0] == witness_size(oracle, dg, doc)
    return w, (commit, dg1_hash, pkh)


def expected_row(oracle, dg, doc, row):
    """the same from a Light input row (1025, 32)"""
    return expected(oracle, dg, doc, row[:1024, 0].copy(), to_int(row[1024]))


KIND_NAMES = {0: "ONE", 1: "INCOPY", 2: "SHA_OWN", 3: "SHA_BLOCK", 4: "POSEIDON", 6: "VALUE", 7: "BITS2NUM", 8: "NUM2BITS",
              9: "DIGEST", 21: "BJJ_OWN", 22: "BJJ_STEPS", 45: "SHA1_OWN", 46: "SHA1_BLOCK", 47: "SHA5_OWN", 48: "SHA5_BLOCK"}


def light_params(dg, doc):
    from pzkwit import native
    return native.PzkParams(circuit=native.PZK_CIRCUIT_LIGHT, dg_hash_type=dg, document_type=doc)


def region_table(dg, doc):
    """the library's region table, used only to word mismatch reports"""
    import ctypes
    from pzkwit import native
    L = native.lib()
    p = light_params(dg, doc)
    info, n = native.PzkInfo(), ctypes.c_uint32()
    rc = L.pzk_layout_query(ctypes.byref(p), ctypes.byref(info), ctypes.byref(n))
    assert rc == 0, L.pzk_last_error()
    out = []
    for i in range(n.value):
        off, ln, kd = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        L.pzk_layout_region(ctypes.byref(p), i, ctypes.byref(off), ctypes.byref(ln), ctypes.byref(kd))
        out.append((off.value, ln.value, kd.value))
    return out


def mismatch_report(ref, got, regions, limit=12):
    """test_gpu_register.mismatch_report with this family's region names"""
    bad = np.nonzero((ref != got).any(axis=1))[0]
    if bad.size == 0:
        return ""
    lines = ["%d mismatching elements" % bad.size]
    seen = {}
    for idx in bad[:4096]:
        for ri, (off, ln, kd) in enumerate(regions):
            if off <= idx < off + ln:
                seen.setdefault(ri, []).append(int(idx - off))
                break
    for ri, locs in list(seen.items())[:limit]:
        off, ln, kd = regions[ri]
        e = off + locs[0]
        lines.append("region %d %s off=%d len=%d: %d bad, first local %s ref=%s got=%s" % (
            ri, KIND_NAMES.get(kd, kd), off, ln, len(locs), locs[:6], to_int(ref[e]), to_int(got[e])))
    return "\n".join(lines)
