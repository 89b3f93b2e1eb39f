"""RegisterIdentityBuilder instances at the edges of build_register's accepted parameter ranges, and rows that fail the
PassportVerificationFlow block one comparison at a time. Plain Python: no GPU, no oracle.

The device reads its inputs at parameter-dependent offsets (csrc/regemit.hpp k_emit_flow: the encapsulated content at
DG1_SHIFT, DG15_SHIFT and DG15_SHIFT - 24, the signed attributes at EC_SHIFT; csrc/regcore.hpp k_prep: DG15 at
AA_SHIFT over 200 / 224 / 248 / 192-bit windows), and pzkwit.inputs.PassportGen only writes hashes at byte offsets
of the canonical kind. build_row() writes them at bit offsets, so a shift may be odd, zero, or put its window's last
bit on the last bit a SHA-padded message can carry:

    usable(blocks, block) = blocks * block - (block // 8 + 8) bits    (0x80 and the 64 / 128-bit length follow)

Messages stay byte strings with ordinary SHA padding, so hashlib is the hash reference. A window that crosses
usable() is a mistake in the case, never a reason to skip it: build_row() asserts it. The one exception the issue
names is the AA key window of `aa20_end`, which ends at DG15_BLOCK_NUMBER x block exactly: the circuit does not
parse DG15, so the key bits may be the padding's.

flow_ref() restates the whole PassportVerificationFlow block over Python integers from passportVerificationFlow.circom
and comparators.circom (IsEqual: out | in[2] | IsZero out, in, inv with in = in[1] - in[0], inv = 1 / in or 0);
features() names what a row reaches. tests/test_register_cases.py pins the oracle on every row and requires the
committed rows to reach all of FEATURES; tests/test_gpu_register_cases.py compares the device.

No case was dropped: every parameter set below is one the reference circuit compiles (each index it reads lies
inside its signal array). One set the library used to accept is not: SIGNATURE_TYPE 24 has HASH_TYPE 224 but
EC_HASH_TYPE 256, so with DG_HASH_TYPE 256 the flow reads signedAttributes[EC_SHIFT + i] for i < 256, and
EC_SHIFT + 224 <= 1024 does not keep that inside the 1024 attributes; BOUNDS holds it as `ec_shift_dg`."""
import numpy as np

from pzkwit import inputs as I
from pzkwit.field import P, SplitMix64

PREFIX = (0, 0, 0, 0, 1, 1, 1, 1)  # passportVerificationFlow.circom:68, 0x0F MSB first
PREFIX_SHIFT = 24


# ------------------------------------------------------------------------------------------------ geometry
def geometry(params):
    """the sizes the templates derive from the parameters (passportVerificationBuilder.circom:16-68, identity.circom)"""
    ht, dg = I.sig_hash_type(params["sig"]), params["dg_hash"]
    hb, aa = I.hash_block(ht), params["aa"]
    aa_f = 320 if aa == 22 else 192 if aa == 23 else 256
    return dict(DG=dg, HT=ht, EH=I.ec_hash_type(params["sig"]), HB=hb, DB=I.hash_block(dg), ecLen=params["ec_blocks"] * hb,
                d15Len=params["dg15_blocks"] * hb, V=aa, dg15shift=params["dg15_shift"] if aa else dg,
                aa_span=0 if not aa else 2 * aa_f if aa >= 20 else 1024)


def usable(blocks, block):
    """message bits of a SHA-padded input of exactly `blocks` blocks; the last usable bit is usable() - 1"""
    return blocks * block - (block // 8 + 8)


def msg_len(blocks, block):
    """the longest byte string that pads to `blocks` blocks"""
    return usable(blocks, block) // 8


def get_bits(data):
    return np.unpackbits(np.frombuffer(bytes(data), dtype=np.uint8))


def put_bits(data, at, bits):
    a = get_bits(data)
    assert 0 <= at and at + len(bits) <= a.size, (at, len(bits), a.size)
    a[at:at + len(bits)] = bits
    return np.packbits(a).tobytes()


def flip_bit(data, at):
    a = bytearray(data)
    assert 0 <= at < 8 * len(a), (at, len(a))
    a[at // 8] ^= 0x80 >> (at % 8)
    return bytes(a)


# ------------------------------------------------------------------------------------------------ signer keys
_KEYS = {}
KEY_SEED = 0x52C


def signer(sig):
    """one signer key per SIGNATURE_TYPE, shared by every instance: a PassportGen around it (for its pk_hash)"""
    if sig not in _KEYS:
        bits = {20: "p256", 21: "bp256", 24: "p224", 25: "bp384"}.get(sig, 4096 if sig == 2 else 3072 if sig in (4, 14)
                                                                      else 2048)
        e = 3 if sig == 10 else 37187 if sig == 4 else 65537
        key = I._keygen((KEY_SEED, sig, bits) if e == 65537 else (KEY_SEED, sig, bits, e))
        _KEYS[sig] = I.PassportGen(seed=KEY_SEED, params=I.instance_params(sig), keys=[key])
    return _KEYS[sig]


# ------------------------------------------------------------------------------------------------ rows
class Row:
    """pp: the passport dict pack_register_inputs takes; packed: its row; code: the status the circuit gives it (0, or
    7 = the flow); tamper: the (stage, bit) list it was built with; name: for messages"""

    def __init__(self, pp, packed, tamper, name):
        self.pp, self.packed, self.tamper, self.name = pp, packed, tamper, name
        self.code = 7 if tamper else 0

    def __str__(self):
        return self.name


def random_dg15(rng, params):
    """a DG15 of the longest length that pads to DG15_BLOCK_NUMBER blocks (b"" without a DG15)"""
    return rng.bytes(msg_len(params["dg15_blocks"], I.hash_block(params["dg_hash"]))) if params["dg15_blocks"] else b""


def build_row(params, key, seed, dg15=None, tamper=None, smt_depth=0, name=None):
    """key: signer(sig). dg15: bytes, None = the generator's RSA-1024 blob (3 x 512-bit blocks) or, where that does
    not pad to DG15_BLOCK_NUMBER blocks, random_dg15(). tamper: (stage, bit) or a list of them; stage "ec" / "sa" flips
    that bit of the encapsulated content / signed attributes after the hashes are written into it and before it is
    hashed itself, "dg15" flips an input bit of DG15 after its hash went into the content: the comparisons of the
    flipped bits fail and nothing else does (the signature is made over the final attributes)."""
    g = geometry(params)
    sg, DG, hb, db = params["sig"], g["DG"], g["HB"], g["DB"]
    tamper = [] if tamper is None else [tamper] if isinstance(tamper[0], str) else list(tamper)
    assert all(st in ("ec", "sa", "dg15") for st, _ in tamper)
    rng = SplitMix64((seed << 20) ^ 0x524F57)
    dg1 = I._mrz_dg1(rng)
    blob = I._dg15_rsa1024(rng)
    if dg15 is None:
        fits = params["dg15_blocks"] and len(I.sha_pad(blob, db)) * 8 == params["dg15_blocks"] * db
        dg15 = blob if fits else random_dg15(rng, params)
    assert len(I.sha_pad(dg15, db)) * 8 == params["dg15_blocks"] * db if params["dg15_blocks"] else not dg15
    dgh, sah, ech = I.HASHES[DG], I.HASHES[g["HT"]], I.HASHES[g["EH"]]
    # encapsulated content: random, then the DG hashes and the prefix at their bit offsets
    ec_use = usable(params["ec_blocks"], hb)
    ec = rng.bytes(ec_use // 8)
    d1s, d15s = params["dg1_shift"], params["dg15_shift"]
    assert d1s + DG <= ec_use, "dg1 window past the last usable bit"
    ec = put_bits(ec, d1s, get_bits(dgh(dg1).digest()))
    if params["aa"]:  # DG15_VERIFICATION = 0 compares nothing: the content stays random there
        assert d15s + DG <= ec_use and d15s >= PREFIX_SHIFT, "dg15 window outside the usable bits"
        assert d1s + DG <= d15s - PREFIX_SHIFT or d15s + DG <= d1s, "dg1 and dg15 windows overlap"
        ec = put_bits(ec, d15s, get_bits(dgh(dg15).digest()))
        ec = put_bits(ec, d15s - PREFIX_SHIFT, np.array(PREFIX, dtype=np.uint8))
        assert g["aa_span"] + params["aa_shift"] <= g["d15Len"]
    for st, bit in tamper:
        if st == "ec":
            ec = flip_bit(ec, bit)
        elif st == "dg15":
            dg15 = flip_bit(dg15, bit)
    # signed attributes: random, then as much of the content's hash as fits before the padding (the flow compares DG
    # bits of it; a real SOD carries all of it)
    sa_use = usable(1024 // hb, hb)
    sa = rng.bytes(sa_use // 8)
    ecs = params["ec_shift"]
    assert ecs + DG <= sa_use, "ec hash window past the last usable bit"
    sa = put_bits(sa, ecs, get_bits(ech(ec).digest())[:min(g["EH"], sa_use - ecs)])
    for st, bit in tamper:
        if st == "sa":
            sa = flip_bit(sa, bit)
    k = key.keys[0]
    if isinstance(k, I.EcKey):
        sig = k.sign(sa, rng)
    elif 10 <= sg <= 14:
        sig = I.pss_sign(k, sa, rng.bytes(I.pss_salt_len(sg)), sah)
    elif sg in (3, 4):
        sig = I.pkcs1v15_sha1_sign(k, sa)
    else:
        sig = I.pkcs1v15_sha256_sign(k, sa)
    pkh = key.pk_hash(k)
    sk_hex, root_hex, _ = I.fake_iden_data(ec, pkh)
    siblings = [0] * 80
    root = int(root_hex, 16)
    if smt_depth:  # the circuit does not enforce the root (passportVerificationBuilder.circom:240)
        for j in range(smt_depth):
            siblings[j] = 1 + rng.below(P - 1)
        root = rng.fr()
    pp = dict(dg1=dg1, dg15=dg15, ec=ec, sa=sa, sig=sig, n=k.n, sk=int(sk_hex, 16), root=root, siblings=siblings,
              pk_hash=pkh)
    packed = I.pack_register_inputs(pp, params)
    packed.setflags(write=False)
    return Row(pp, packed, tamper, name or ("tamper %s" % tamper if tamper else "pass seed %d depth %d" % (seed, smt_depth)))


# ------------------------------------------------------------------------------------------------ the flow, restated
def _digest_bits(h, msg):
    return [int(b) for b in get_bits(h(msg).digest())]


def flow_inputs(params, pp):
    """(dg1Hash, dg15Hash, encapsulatedContent, encapsulatedContentHash, signedAttributes) as lists of 0 / 1"""
    g = geometry(params)
    dgh = I.HASHES[g["DG"]]
    h15 = _digest_bits(dgh, pp["dg15"]) if params["aa"] else [0] * g["DG"]  # passportVerificationBuilder.circom:115-128
    ec = [int(b) for b in I.padded_bits(pp["ec"], g["HB"])]
    sa = [int(b) for b in I.padded_bits(pp["sa"], g["HB"])]
    assert len(ec) == g["ecLen"] and len(sa) == 1024
    return _digest_bits(dgh, pp["dg1"]), h15, ec, _digest_bits(I.HASHES[g["EH"]], pp["ec"]), sa


def flow_pairs(params, pp):
    """in[0], in[1] of the 3 H + 8 IsEqual components in creation order (passportVerificationFlow.circom:27-79)"""
    g = geometry(params)
    H, V, d15 = g["DG"], g["V"], g["dg15shift"]
    h1, h15, ec, ech, sa = flow_inputs(params, pp)
    pairs = [(h1[i], ec[params["dg1_shift"] + i]) for i in range(H)]
    pairs += [(h15[i] * V % P, ec[d15 + i] * V % P) for i in range(H)]
    pairs += [(ech[i], sa[params["ec_shift"] + i]) for i in range(H)]
    pairs += [(PREFIX[i] * V % P, ec[d15 - PREFIX_SHIFT + i] * V % P) for i in range(8)]
    return pairs


def flow_ref(params, row):
    """every signal of PassportVerificationFlow as a Python integer, in witness order: flowResult | dg1Hash[H],
    dg15Hash[H], encapsulatedContent, encapsulatedContentHash[EH], signedAttributes[1024] | verifyAllChecksPassed
    [3 H + 8] | IsEqual x (3 H + 8), each out | in[0], in[1] | IsZero out, in, inv"""
    pp = row.pp if isinstance(row, Row) else row
    h1, h15, ec, ech, sa = flow_inputs(params, pp)
    pairs = flow_pairs(params, pp)
    chain, blocks, c = [], [], 1
    for a, b in pairs:
        d = (b - a) % P                      # comparators.circom IsEqual: isz.in <== in[1] - in[0]
        inv = pow(d, P - 2, P) if d else 0   # IsZero: inv <-- in != 0 ? 1 / in : 0
        out = (1 - d * inv) % P              # out <== -in * inv + 1
        assert out == int(a == b)
        c = c * out % P                      # verifyAllChecksPassed[k] = [k - 1] * out (:82-105)
        chain.append(c)
        blocks += [out, a, b, out, d, inv]
    return [chain[-1]] + h1 + h15 + ec + ech + sa + chain + blocks


FEATURES = ("passing", "first_0", "first_H-1", "first_H", "first_2H-1", "first_2H", "first_3H-1", "first_3H",
            "first_3H+7", "diff_+1", "diff_-1", "diff_+V", "diff_-V", "fail_then_equal", "two_groups", "dg15_half")
FEATURES_V0 = ("v0_dg15_differs", "v0_prefix_differs")


def features(params, row):
    """labels of what a row reaches in the flow: a subset of FEATURES + FEATURES_V0"""
    pp = row.pp if isinstance(row, Row) else row
    g = geometry(params)
    H, V = g["DG"], g["V"]
    pairs = flow_pairs(params, pp)
    bad = [k for k, (a, b) in enumerate(pairs) if a != b]
    f = set()
    if V == 0:  # the scaled inputs are all 0; name what the unscaled ones hide
        _, _, ec, _, _ = flow_inputs(params, pp)
        d15 = g["dg15shift"]
        if any(ec[d15:d15 + H]):
            f.add("v0_dg15_differs")  # dg15Hash is zeros
        if tuple(ec[d15 - PREFIX_SHIFT:d15 - PREFIX_SHIFT + 8]) != PREFIX:
            f.add("v0_prefix_differs")
    if not bad:
        f.add("passing")
        return f
    names = {0: "0", H - 1: "H-1", H: "H", 2 * H - 1: "2H-1", 2 * H: "2H", 3 * H - 1: "3H-1", 3 * H: "3H", 3 * H + 7: "3H+7"}
    if bad[0] in names:
        f.add("first_" + names[bad[0]])
    for k in bad:
        a, b = pairs[k]
        d = b - a  # both < p / 2: an integer difference
        scaled = H <= k < 2 * H or k >= 3 * H
        if scaled and V >= 2:
            assert abs(d) == V
            f.add("diff_+V" if d > 0 else "diff_-V")
        elif not scaled:
            assert abs(d) == 1
            f.add("diff_+1" if d > 0 else "diff_-1")
    if any(k not in bad for k in range(bad[0] + 1, len(pairs))):
        f.add("fail_then_equal")
    if len({min(k // H, 3) for k in bad}) >= 2:
        f.add("two_groups")
    n15 = sum(1 for k in bad if H <= k < 2 * H)
    if H // 4 <= n15 <= 3 * H // 4 and {pairs[k][1] > pairs[k][0] for k in bad if H <= k < 2 * H} == {True, False}:
        f.add("dg15_half")  # a different DG15: about half the hash bits differ, with both signs
    return f


# ------------------------------------------------------------------------------------------------ instances
C = I.CANONICAL
ODD = dict(C, dg1_shift=251, dg15_shift=1499, ec_shift=603, aa_shift=259)
U4, U3, USA = usable(4, 512), usable(3, 512), usable(2, 512)  # 1976, 1464, 952
S13 = I.instance_params(13)  # 1024-bit blocks: 2 content blocks, 2 DG15 blocks, one attributes block
W2, WSA = usable(2, 1024), usable(1, 1024)  # 1912, 888

# name -> (params, is a flow instance). Shifts and sizes on SIG 1 / DG 256 / TD3 unless the name says otherwise.
PARAMS = {
    "flow_aa1": (dict(C), True),
    "flow_aa7": (dict(C, aa=7), True),
    # aa 23: 192-bit field and hash size, one odd aa_shift
    "flow_aa23": (dict(C, aa=23, aa_shift=267), True),
    "odd": (ODD, False),
    "dg1_first": (dict(C, dg1_shift=0), False),
    "dg15_first": (dict(C, dg15_shift=24, dg1_shift=600), False),
    "last": (dict(C, dg1_shift=8, dg15_shift=U4 - 256, ec_shift=USA - 256, aa_shift=U3 - 1024), False),
    "ec_first": (dict(C, ec_shift=0), False),
    "aa_first": (dict(C, aa_shift=0), False),
    "ec16": (dict(C, ec_blocks=16, dg1_shift=usable(16, 512) - 256, dg15_shift=4099), False),
    "ec1": (dict(C, ec_blocks=1, aa=0, dg15_blocks=0, dg1_shift=179), False),
    "d15_1": (dict(C, dg15_blocks=1, aa=23, aa_shift=0), False),
    "d15_16": (dict(C, dg15_blocks=16, aa_shift=usable(16, 512) - 1024), False),
    "aa2": (dict(C, aa=2, aa_shift=257), False),
    "aa19": (dict(C, aa=19, aa_shift=261), False),
    "aa21": (dict(C, aa=21, aa_shift=263), False),
    "aa25": (dict(C, aa=25, aa_shift=301), False),
    "aa22": (dict(C, aa=22, aa_shift=265), False),
    "aa20_end": (dict(C, aa=20, aa_shift=3 * 512 - 512), False),
    "sig3_dg160": (I.instance_params(3), False),
    "sig1_dg224_td1": (dict(ODD, dg_hash=224, doc=1), False),
    "sig1_dg160_td1": (dict(ODD, dg_hash=160, doc=1), False),
    "sig13_dg384_aa22": (dict(S13, aa=22, dg1_shift=251, dg15_shift=W2 - 384, ec_shift=WSA - 384, aa_shift=W2 - 640), False),
    "sig13_dg160_aa0": (dict(S13, dg_hash=160, aa=0, dg15_blocks=0), False),
    "sig24_dg224": (I.instance_params(24), False),
    "sig25_dg384_td1": (dict(I.instance_params(25), doc=1), False),
    "sig21_aa23": (dict(C, sig=21, aa=23), False),
}
V0_INSTANCE = "ec1"       # AA_SIGNATURE_ALGO 0: its rows' DG15 window and prefix byte are random content
PREFIX_INSTANCE = "flow_aa7"  # a row for each of the eight prefix bits
PACKED_INSTANCES = ("odd", "flow_aa23")
MAX_BATCH = 16


def _dg15_for(name, params, rng):
    if name == "d15_1":
        return rng.bytes(48)  # x | y of a 192-bit key, nothing else
    if name in ("last", "aa20_end", "sig13_dg384_aa22"):
        return random_dg15(rng, params)  # the longest message: the key window's last usable bit is a message bit
    return None


def _pick(bits, want, lo, hi):
    """the first index in [lo, hi) whose bit is `want`"""
    for i in range(lo, hi):
        if bits[i] == want:
            return i
    raise AssertionError("no %d bit in [%d, %d)" % (want, lo, hi))


def flow_tampers(name, params, base):
    """the tamper lists of a flow instance's failing rows. base: the untampered row of the same seed (its hashes
    choose, per group, an interior index where the hash bit is 0 and one where it is 1: the content bit is its
    complement after the flip, so in = in[1] - in[0] takes both signs)"""
    g = geometry(params)
    H, d1s, d15s, ecs = g["DG"], params["dg1_shift"], params["dg15_shift"], params["ec_shift"]
    h1, h15, _, ech, _ = flow_inputs(params, base.pp)
    t = [("first_0", ("ec", d1s)), ("first_H-1", ("ec", d1s + H - 1)), ("first_H", ("ec", d15s)),
         ("first_2H-1", ("ec", d15s + H - 1)), ("first_2H", ("sa", ecs)), ("first_3H-1", ("sa", ecs + H - 1)),
         ("first_3H", ("ec", d15s - PREFIX_SHIFT)), ("first_3H+7", ("ec", d15s - PREFIX_SHIFT + 7))]
    for grp, bits, st, at in (("dg1", h1, "ec", d1s), ("dg15", h15, "ec", d15s), ("ec", ech, "sa", ecs)):
        for want in (0, 1):
            i = _pick(bits, want, 30 + 33 * want, H - 1)  # crosses a 32-bit word of the digest between the two
            t.append(("%s hash bit %d = %d" % (grp, i, want), (st, at + i)))
    t.append(("another dg15", ("dg15", 8 * 40 + 3)))
    t.append(("dg1 and ec hash", [("ec", d1s + 5), ("sa", ecs + 9)]))
    if name == PREFIX_INSTANCE:
        t += [("prefix bit %d" % i, ("ec", d15s - PREFIX_SHIFT + i)) for i in range(1, 7)]
    return t


_BUILT = {}


def instance_rows(name):
    """-> (params, [Row]). Two passing rows (the second with smt_depth > 0); a flow instance then its failing rows."""
    if name not in _BUILT:
        params, flow = PARAMS[name]
        key = signer(params["sig"])
        seed = 1 + sorted(PARAMS).index(name) * 100
        d15 = _dg15_for(name, params, SplitMix64(seed))
        rows = [build_row(params, key, seed, dg15=d15), build_row(params, key, seed + 1, dg15=d15, smt_depth=5)]
        if flow:
            for label, tamper in flow_tampers(name, params, rows[0]):
                rows.append(build_row(params, key, seed, dg15=d15, tamper=tamper, name=label))
        _BUILT[name] = (params, rows)
    return _BUILT[name]


def batches(name):
    """the instance's rows as the device calls take them: one batch of the two passing rows, or for a flow instance
    passing, failing, passing, ..., passing in batches of at most MAX_BATCH rows (every failing lane between two clean
    ones; the passing rows alternate). -> (params, [[Row]])"""
    params, rows = instance_rows(name)
    good, bad = rows[:2], rows[2:]
    if not bad:
        return params, [good]
    out, per = [], (MAX_BATCH - 1) // 2
    for s in range(0, len(bad), per):
        b = [good[0]]
        for j, r in enumerate(bad[s:s + per]):
            b += [r, good[(j + 1) % 2]]
        out.append(b)
    return params, out


# ------------------------------------------------------------------------------------------------ acceptance bounds
def _b(base, **kw):
    return dict(base, **kw)


# name -> (the parameter set just inside, the set just outside) of every bound build_register checks
# (csrc/builder_register.cpp; oracle/witness_oracle.c params_ok has the same). ecLen 2048, d15Len 1536 on CANONICAL.
BOUNDS = {
    "dg1_shift + DG <= ecLen": (_b(C, dg1_shift=2048 - 256), _b(C, dg1_shift=2048 - 255)),
    "0 <= dg1_shift": (_b(C, dg1_shift=0), _b(C, dg1_shift=-1)),
    "24 <= dg15_shift": (_b(C, dg15_shift=24, dg1_shift=600), _b(C, dg15_shift=23, dg1_shift=600)),
    "dg15_shift + DG <= ecLen": (_b(C, dg15_shift=2048 - 256), _b(C, dg15_shift=2048 - 255)),
    "0 <= ec_shift": (_b(C, ec_shift=0), _b(C, ec_shift=-1)),
    "ec_shift + HT <= 1024": (_b(C, ec_shift=1024 - 256), _b(C, ec_shift=1024 - 255)),
    "ec_shift + HT <= 1024 (160)": (_b(I.instance_params(3), ec_shift=1024 - 160), _b(I.instance_params(3), ec_shift=1024 - 159)),
    "ec_shift_dg": (_b(C, sig=24, dg_hash=256, ec_shift=1024 - 256), _b(C, sig=24, dg_hash=256, ec_shift=1024 - 255)),
    "0 <= aa_shift": (_b(C, aa_shift=0), _b(C, aa_shift=-1)),
    "aa_shift + 1024 <= d15Len": (_b(C, aa_shift=1536 - 1024), _b(C, aa_shift=1536 - 1023)),
    "aa_shift + 2 x 256 <= d15Len": (_b(C, aa=20, aa_shift=1536 - 512), _b(C, aa=20, aa_shift=1536 - 511)),
    "aa_shift + 2 x 320 <= d15Len": (_b(C, aa=22, aa_shift=1536 - 640), _b(C, aa=22, aa_shift=1536 - 639)),
    "aa_shift + 2 x 192 <= d15Len": (_b(C, aa=23, aa_shift=1536 - 384), _b(C, aa=23, aa_shift=1536 - 383)),
    "aa != 0 needs a dg15": (_b(C, aa=0, dg15_blocks=0), _b(C, aa=1, dg15_blocks=0, aa_shift=0)),
    "ec_blocks >= 1": (_b(C, ec_blocks=1, aa=0, dg15_blocks=0, dg1_shift=0), _b(C, ec_blocks=0, aa=0, dg15_blocks=0, dg1_shift=0)),
    "ec_blocks <= 16": (_b(C, ec_blocks=16), _b(C, ec_blocks=17)),
    "dg15_blocks >= 0": (_b(C, aa=0, dg15_blocks=0), _b(C, aa=0, dg15_blocks=-1)),
    "dg15_blocks <= 16": (_b(C, dg15_blocks=16), _b(C, dg15_blocks=17)),
    "aa <= 25": (_b(C, aa=25), _b(C, aa=26)),
    "aa >= 0": (_b(C, aa=0), _b(C, aa=-1)),
    "doc 1 | 3": (_b(C, doc=1), _b(C, doc=2)),
    "sums in 64 bits: dg1_shift": (_b(C, dg1_shift=1), _b(C, dg1_shift=2 ** 31 - 1)),
    "sums in 64 bits: dg15_shift": (_b(C, dg15_shift=1496), _b(C, dg15_shift=2 ** 31 - 1)),
    "sums in 64 bits: ec_shift": (_b(C, ec_shift=1), _b(C, ec_shift=2 ** 31 - 1)),
    "sums in 64 bits: aa_shift": (_b(C, aa_shift=1), _b(C, aa_shift=2 ** 31 - 1)),
    "negative: dg15_shift": (_b(C, dg15_shift=1496), _b(C, dg15_shift=-(2 ** 31))),
    "negative: aa_shift": (_b(C, aa_shift=256), _b(C, aa_shift=-(2 ** 31))),
}
