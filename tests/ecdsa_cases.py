"""ECDSA rows whose scalars u1 = h/s and u2 = r/s (mod n) are steered, for the four ECDSA instances
(SIGNATURE_TYPE 20, 21, 24, 25). Plain Python: no GPU, no oracle.

The device's point chains (k_ec_chain, ec_core.hpp) branch on the bytes of u1 and the nibbles of u2; a random
signature reaches almost none of those branches. The digest h of the signed attributes does not depend on the signer
key, so a signature that verifies can be built around a chosen scalar by choosing the key last:

  steer u2:  r = x(kG) mod n,  s = r / u2,  u1 = h / s,  d = (k - u1) / u2,  Q = dG
  steer u1:  s = h / u1,  u2 = r / s,  d and Q as above
  steer s:   u2 = r / s,  u1 = h / s,  d and Q as above

(u1 G + u2 Q = (u1 + u2 d) G = kG.) chain_features restates the chains' handle decisions, without any point
arithmetic, and names the branches a pair (u1, u2) takes; tests/test_ecdsa_cases.py requires the committed rows of
every curve to reach all of them and pins the oracle on them, tests/test_gpu_ecdsa_cases.py compares the device."""
import hashlib

from pzkwit import field, inputs as I

SIGS = (20, 21, 24, 25)
SEED = 0xEC5A  # PassportGen seed of the base passports
ST_ECDSA_INV, ST_ECDSA_R = 15, 16  # s has no inverse mod n (bigInt.circom:364-368); x1 mod n === r (ecdsa.circom:81-83)

FEATURES = ("gm_first_dummy", "gm_dummy_even", "gm_dummy_odd", "gm_dummy_pair", "gm_right_dummy_after_real",
            "gm_byte_255", "gm_top_part_nonzero", "gm_result_forwarded",
            "sm_lead_zero", "sm_zero_after_zero_lead", "sm_zero_nibble", "sm_zero_run", "sm_nibble_1", "sm_nibble_15",
            "sm_result_is_Q", "sm_result_dummy", "sm_result_is_doubling")

# point handles, as ec_core.hpp names them: >= 0 an op's output, H_D the dummy, H_Q the key, <= -1000 a table entry
H_D, H_Q, OP_SD = -1, -2, 0


def geometry(sig):
    """(fb, parts, wins): bits of a scalar, bytes of u1 (generator multiplication), nibbles of u2 (window 4)"""
    n, cs = I.EC_CHUNKS[sig]
    fb = n * cs
    return fb, fb // 8, fb // 4


def hash_fn(sig):
    return I.HASHES[I.sig_hash_type(sig)]


def digest_int(pp, sig):
    """h of EcKey.sign: the digest of the signed attributes as an integer, not reduced"""
    return int.from_bytes(hash_fn(sig)(pp["sa"]).digest(), "big")


def scalars(sig, h, r, s):
    """(u1, u2) as BigModInv / the two BigMultModP give them: inputs reduced mod n, the inverse of 0 is 0"""
    n = I.EC_CURVES[sig].n
    sinv = pow(s % n, -1, n) if s % n else 0
    return h % n * sinv % n, r % n * sinv % n


def gm_handles(sig, u1):
    """the generator multiplication's handles: (additionPoints, resultingPoints, steps as (left, right))"""
    parts = geometry(sig)[1]

    def ap(i):
        b = (u1 >> (8 * i)) & 255
        return -(1000 + 256 * i + b) if b else (H_D if i % 2 == 0 else OP_SD)

    aps = [ap(i) for i in range(parts)]
    left, rps, steps = aps[0], [], []
    for i in range(parts - 1):
        right = aps[i + 1]
        ld, rd = left in (H_D, OP_SD), right in (H_D, OP_SD)
        steps.append((left, right))
        left = right if ld else left if rd else 1 + i
        rps.append(left)
    return aps, rps, steps


def sm_handles(sig, u2):
    """the window-4 multiplication of the key: per window w >= 1 (nibble, izr, iza), and the result's handle;
    op handles are ("pre", n), ("dbl", w), ("add", w)"""
    fb, _, wins = geometry(sig)
    nib = [(u2 >> (fb - 4 - 4 * w)) & 15 for w in range(wins)]

    def pre(n):
        return H_D if n == 0 else H_Q if n == 1 else ("pre", n)

    rp, wnd = pre(nib[0]), []
    for w in range(1, wins):
        ap = pre(nib[w])
        izr, iza = rp == H_D, ap == H_D
        wnd.append((nib[w], izr, iza))
        rp = ap if izr else ("dbl", w) if iza else ("add", w)
    return wnd, rp


def chain_features(sig, u1, u2):
    """labels of the handle decisions k_ec_chain and k_ec_final take on (u1, u2); a subset of FEATURES"""
    parts = geometry(sig)[1]
    f = set()
    byte = [(u1 >> (8 * i)) & 255 for i in range(parts)]
    _, rps, steps = gm_handles(sig, u1)
    if byte[0] == 0:
        f.add("gm_first_dummy")
    if any(b == 0 for b in byte[0::2]):
        f.add("gm_dummy_even")
    if any(b == 0 for b in byte[1::2]):
        f.add("gm_dummy_odd")
    if any(byte[i] == 0 and byte[i + 1] == 0 for i in range(parts - 1)):
        f.add("gm_dummy_pair")
    if any(right in (H_D, OP_SD) and left not in (H_D, OP_SD) for left, right in steps):
        f.add("gm_right_dummy_after_real")
    if 255 in byte:
        f.add("gm_byte_255")
    if byte[parts - 1]:
        f.add("gm_top_part_nonzero")
    if rps[-1] < 0:
        f.add("gm_result_forwarded")
    wnd, h2 = sm_handles(sig, u2)
    for k, (n, izr, iza) in enumerate(wnd):
        if izr:
            f.add("sm_lead_zero")
        if izr and iza:
            f.add("sm_zero_after_zero_lead")
        if iza and not izr:
            f.add("sm_zero_nibble")
            if k and wnd[k - 1][2] and not wnd[k - 1][1]:
                f.add("sm_zero_run")
        if n == 1:
            f.add("sm_nibble_1")
        if n == 15:
            f.add("sm_nibble_15")
    if h2 == H_Q:
        f.add("sm_result_is_Q")
    if h2 == H_D:
        f.add("sm_result_dummy")
    if isinstance(h2, tuple) and h2[0] == "dbl":
        f.add("sm_result_is_doubling")
    return f


def _with_key(pp, sig, q, rs):
    fb = geometry(sig)[0]
    out = dict(pp)
    out["n"], out["sig"] = q, rs
    out["pk_hash"] = I.ecdsa_pk_hash(q, fb)
    out["root"] = field.poseidon([out["pk_hash"], out["pk_hash"], 1])  # depth 0
    return out


def craft(pp, curve, hash_fn, k, u1=None, u2=None, s=None):
    """A signature over pp's signed attributes that verifies, with nonce k and exactly one of u1, u2, s chosen; the
    signer key follows. -> (patched passport dict, (u1, u2))"""
    assert (u1 is not None) + (u2 is not None) + (s is not None) == 1
    n = curve.n
    h = int.from_bytes(hash_fn(pp["sa"]).digest(), "big")
    assert h % n, "the digest is 0 mod n"
    r = curve.mul(k)[0] % n
    assert r
    if u2 is not None:
        s = r * pow(u2, -1, n) % n
        u1 = h * pow(s, -1, n) % n
    elif u1 is not None:
        s = h * pow(u1, -1, n) % n
        u2 = r * pow(s, -1, n) % n
    else:
        u2 = r * pow(s, -1, n) % n
        u1 = h * pow(s, -1, n) % n
    assert 0 < s < n and 0 < u1 < n and 0 < u2 < n
    d = (k - u1) * pow(u2, -1, n) % n
    assert d
    q = curve.mul(d)
    sinv = pow(s, -1, n)
    assert h * sinv % n == u1 and r * sinv % n == u2
    assert curve.add(curve.mul(u1), curve.mul(u2, q))[0] % n == r  # verifies
    sig = {c.name: t for t, c in I.EC_CURVES.items()}[curve.name]
    return _with_key(pp, sig, q, (r, s)), (u1, u2)


def both_chosen(pp, curve, hash_fn, u1, u2, q=None):
    """A row with both scalars chosen: s = h / u1, r = u2 s. It does not verify (x(u1 G + u2 Q) mod n == r would be
    a coincidence), with any key q (default: the passport's own). -> (patched passport dict, (u1, u2))"""
    n = curve.n
    h = int.from_bytes(hash_fn(pp["sa"]).digest(), "big")
    s = h * pow(u1, -1, n) % n
    r = u2 * s % n
    assert 0 < s < n and 0 < r < n
    sig = {c.name: t for t, c in I.EC_CURVES.items()}[curve.name]
    out = _with_key(pp, sig, pp["n"] if q is None else q, (r, s))
    sinv = pow(s, -1, n)
    assert h * sinv % n == u1 and r * sinv % n == u2
    return out, (u1, u2)


class Case:
    """name; group (the GPU tests compare one group at a time); pp; (u1, u2); code: the oracle's check-site code, 0
    for a row that verifies, None where only 'non-zero' is specified (F4)"""

    def __init__(self, name, group, pp, u, code):
        self.name, self.group, self.pp, self.u1, self.u2, self.code = name, group, pp, u[0], u[1], code

    @property
    def valid(self):
        return self.code == 0

    def __repr__(self):
        return "Case(%s)" % self.name


def nonce(sig, name):
    """a fixed nonce per (curve, case)"""
    n = I.EC_CURVES[sig].n
    return 1 + int.from_bytes(hashlib.sha512(("ecdsa_cases %d %s" % (sig, name)).encode()).digest(), "big") % (n - 1)


def u2_sparse(sig):
    """V4: nibbles 0 0 0 1 0 f from the top, ...f00f... and ...101... in the middle, last nibble 0"""
    fb = geometry(sig)[0]
    return (0x10f << (fb - 24)) | (0xf00f << (fb // 2)) | (0x101 << 40) | 0x7a30


def u1_holes(sig):
    """V7: byte 0 zero, the even/odd pair 4, 5 zero, byte 7 = 0xff, byte 9 zero after a real byte, a non-zero top
    byte (below the top byte of every curve's n)"""
    parts = geometry(sig)[1]
    byte = [((0x5b + 7 * i) & 0xff) or 1 for i in range(parts)]
    byte[0] = byte[4] = byte[5] = byte[9] = 0
    byte[7] = 0xff
    byte[parts - 1] = 0x3c
    return sum(b << (8 * i) for i, b in enumerate(byte))


S_SMALL = 0xb3c1_5a7e_9d20_46f1_88e3_0c55  # V9: 96 bits, so s + n < 2^fb on every curve (P-224: 2^224 - n ~ 2^112)


def generator(sig):
    return I.PassportGen(seed=SEED + sig, n_keys=1, params=I.instance_params(sig), workers=1)


_CASES = {}


def cases(sig):
    """The committed rows of one curve (built once per process). P-256 gets every row; the other curves get V1, V4,
    one V6, V7, V9, F2, F3, F4, and brainpoolP256r1 also F5 from a signature that verifies (on P-256 no reachable
    nonce gives r < 2^256 - n ~ 2^224, so its F5 row chooses r)."""
    if sig in _CASES:
        return _CASES[sig]
    curve, hf, g = I.EC_CURVES[sig], hash_fn(sig), generator(sig)
    n = curve.n
    fb, parts, _ = geometry(sig)
    full = sig == 20
    out, idx = [], [0]

    def base():
        idx[0] += 1
        return g.passport_at(idx[0] - 1)

    def valid(name, group, **kw):
        pp, u = craft(base(), curve, hf, nonce(sig, name), **kw)
        out.append(Case(name, group, pp, u, 0))
        return pp

    def failing(name, group, pp, code):
        h = digest_int(pp, sig)
        out.append(Case(name, group, pp, scalars(sig, h, *pp["sig"]), code))

    valid("V1_u2_1", "u2", u2=1)
    if full:
        valid("V2_u2_2", "u2", u2=2)
        valid("V3_u2_0x10", "u2", u2=0x10)
    valid("V4_u2_sparse", "u2", u2=u2_sparse(sig))
    if full:
        valid("V5_u2_n_minus_1", "u2", u2=n - 1)
        valid("V6_u1_byte_0", "u1", u1=0x37)
    mid = (parts // 2) | 1
    valid("V6_u1_byte_%d" % mid, "u1", u1=0x37 << (8 * mid))
    if full:
        valid("V6_u1_byte_top", "u1", u1=0x37 << (fb - 8))
    valid("V7_u1_holes", "u1", u1=u1_holes(sig))
    if full:
        valid("V8_u1_bytes_0_top", "u1", u1=0x37 | (0x21 << (fb - 8)))
    pp = valid("V9_s_small", "rs", s=S_SMALL)
    assert S_SMALL + n < 1 << fb
    out.append(Case("V9_s_plus_n", "rs", dict(pp, sig=(pp["sig"][0], S_SMALL + n)), (out[-1].u1, out[-1].u2), 0))

    if full:
        pp = base()
        failing("F1_r_eq_s", "rs", dict(pp, sig=(pp["sig"][0], pp["sig"][0])), ST_ECDSA_R)
    pp = base()
    failing("F2_r_0", "rs", dict(pp, sig=(0, pp["sig"][1])), ST_ECDSA_R)
    if full:
        pp = base()
        failing("F2_r_n", "rs", dict(pp, sig=(n, pp["sig"][1])), ST_ECDSA_R)
    pp = base()
    failing("F3_s_0", "fail", dict(pp, sig=(pp["sig"][0], 0)), ST_ECDSA_INV)
    if full:
        pp = base()
        failing("F3_s_n", "fail", dict(pp, sig=(pp["sig"][0], n)), ST_ECDSA_INV)
    # F4: u1 G = +-u2 Q with the stream's own key Q = dG: the final addition degenerates
    d = g.keys[0].d
    u2 = nonce(sig, "F4_u2")
    for name, u1 in (("F4_u1G_eq_u2Q", u2 * d % n),) + ((("F4_u1G_eq_minus_u2Q", -u2 * d % n),) if full else ()):
        pp, u = both_chosen(base(), curve, hf, u1, u2)
        assert curve.mul(u1)[0] == curve.mul(u2, pp["n"])[0]
        out.append(Case(name, "fail", pp, u, None))
    if full:  # F5 with r chosen small (see the docstring), F6
        pp = base()
        failing("F5_r_plus_n", "fail", dict(pp, sig=((pp["sig"][0] >> 40) + n, pp["sig"][1])), ST_ECDSA_R)
        pp, u = both_chosen(base(), curve, hf, u1_holes(sig), u2_sparse(sig))
        out.append(Case("F6_both_steered", "fail", pp, u, ST_ECDSA_R))
    if sig == 21:  # F5 from a signature that verifies: the first nonce of the sequence with r + n < 2^fb
        pp = base()
        for t in range(64):
            k = nonce(sig, "F5_%d" % t)
            if curve.mul(k)[0] % n + n < 1 << fb:
                break
        pp, _ = craft(pp, curve, hf, k, s=nonce(sig, "F5_s"))
        failing("F5_r_plus_n", "fail", dict(pp, sig=(pp["sig"][0] + n, pp["sig"][1])), ST_ECDSA_R)
    for c in out:
        if not full:  # few rows: two groups
            c.group = "valid" if c.valid else "failing"
        assert all(0 <= v < 1 << fb for v in c.pp["sig"]), c.name  # every value fits the chunks
    _CASES[sig] = out
    return out


def groups(sig):
    """group names in case order"""
    seen = []
    for c in cases(sig):
        if c.group not in seen:
            seen.append(c.group)
    return seen


def plain_passports(sig):
    """two plain stream rows (random nonce, the stream's key), far from the crafted rows' passports"""
    g = generator(sig)
    return [g.passport_at(1000), g.passport_at(1001)]


def batch(sig):
    """One call's rows: plain, crafted, plain, crafted, ..., plain, the plain rows alternating between the two
    plain passports. -> (passports, labels): labels[b] is the Case of a crafted row, 0 / 1 for a plain one."""
    plain = plain_passports(sig)
    pps, labels = [], []
    for i, c in enumerate(cases(sig)):
        pps += [plain[i % 2], c.pp]
        labels += [i % 2, c]
    pps.append(plain[len(cases(sig)) % 2])
    labels.append(len(cases(sig)) % 2)
    return pps, labels
