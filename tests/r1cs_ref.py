"""circom's binary .r1cs format and the check A.w * B.w = C.w restated in Python integers, independent of the library
(include/pzkwit.h pzk_r1cs_*): a writer, an evaluator, a generator of satisfied systems, and the case
list shared by tests/test_r1cs_file.py (CPU, the host twin) and tests/test_gpu_r1cs_check.py (the kernels).

A constraint is (A, B, C), each a list of (wire, coefficient) terms; a system is a list of constraints; a witness is a
list of integers (any value below 2^256: the evaluator reads it as its residue, as circom_tester's field operations
would)."""
import random
import struct
import zlib

import numpy as np

P = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001  # BN254's r
R1CS_WT = 8        # csrc/r1cs.hpp: witnesses per tile of k_r1cs_check
R1CS_LONG_T = 32   # csrc/r1cs.hpp: an LC with more terms puts its constraint on the wave-per-constraint path
R1CS_CHUNK_TERMS = 2560  # csrc/r1cs.hpp: a chunk of short constraints ends at 256 constraints or this many terms


def section(kind, payload):
    return struct.pack("<IQ", kind, len(payload)) + payload


def header_payload(n_wires, m, n_pub_out=0, n_pub_in=0, n_prv_in=0, n_labels=None, prime=P, field_size=32):
    return (struct.pack("<I", field_size) + prime.to_bytes(field_size, "little") +
            struct.pack("<IIIIQI", n_wires, n_pub_out, n_pub_in, n_prv_in, n_wires if n_labels is None else n_labels, m))


def lc_bytes(lc):
    return struct.pack("<I", len(lc)) + b"".join(struct.pack("<I", w) + c.to_bytes(32, "little") for w, c in lc)


def constraints_payload(constraints):
    return b"".join(lc_bytes(lc) for con in constraints for lc in con)


def assemble(sections, version=1, magic=b"r1cs", n_sections=None):
    """sections: [(type, payload bytes)] in file order"""
    return (magic + struct.pack("<II", version, len(sections) if n_sections is None else n_sections) +
            b"".join(section(k, p) for k, p in sections))


def write_r1cs(n_wires, constraints, labels=False, header_last=False, extra=(), **hdr):
    """The file circom / snarkjs write: header (1), constraints (2), optionally wire -> label (3). header_last: the
    header after the constraints (legal); extra: further (type, payload) sections put between the two."""
    secs = [(1, header_payload(n_wires, len(constraints), **hdr)), (2, constraints_payload(constraints))]
    if header_last:
        secs.reverse()
    secs[1:1] = list(extra)
    if labels:
        secs.append((3, b"".join(struct.pack("<Q", i) for i in range(n_wires))))
    return assemble(secs)


def lc_value(lc, w):
    return sum(c * (w[i] % P) for i, c in lc) % P


def evaluate(constraints, w):
    """-> (lowest violated constraint index or -1, number of violated constraints)"""
    bad = [k for k, (a, b, c) in enumerate(constraints) if (lc_value(a, w) * lc_value(b, w) - lc_value(c, w)) % P]
    return (bad[0] if bad else -1), len(bad)


def info_of(constraints):
    """n_terms, max_terms, n_long, n_coeffs as the parser must report them: duplicate wires merged, zero sums dropped,
    the coefficient table holding 1, p - 1 and every other distinct coefficient in use"""
    n_terms = max_terms = n_long = 0
    coeffs = {1, P - 1}
    for con in constraints:
        longest = 0
        for lc in con:
            merged = {}
            for i, c in lc:
                merged[i] = (merged.get(i, 0) + c) % P
            kept = [c for c in merged.values() if c]
            coeffs.update(kept)
            n_terms += len(kept)
            longest = max(longest, len(kept))
        max_terms = max(max_terms, longest)
        n_long += longest > R1CS_LONG_T
    return dict(n_terms=n_terms, max_terms=max_terms, n_long=n_long, n_coeffs=len(coeffs))


def close_c(w, a, b, c):
    """c plus one term that makes (a, b, c) hold on w: the coefficient of a wire with a non-zero value is solved for
    (the highest such wire of the system, so that the last wire is read), else C = v * w0 is not possible either
    (w0 = 1 always is), so wire 0 it is."""
    need = (lc_value(a, w) * lc_value(b, w) - lc_value(c, w)) % P
    for i in range(len(w) - 1, -1, -1):
        if w[i] % P:
            return c + [(i, need * pow(w[i] % P, P - 2, P) % P)]
    raise AssertionError("w[0] = 1")


SPECIAL_COEFFS = [1, P - 1, 2, 1 << 64, 1 << 253, P - 2]
SPECIAL_VALUES = [0, 1, P - 1]


def random_witness(rng, n_wires):
    w = [rng.choice(SPECIAL_VALUES) if rng.random() < 0.3 else rng.randrange(P) for _ in range(n_wires)]
    w[0] = 1
    return w


def random_lc(rng, n_wires, n, window=None):
    lo, hi = (0, n_wires) if window is None else (max(0, window[0]), min(n_wires, window[1]))
    wires = rng.sample(range(lo, hi), min(n, hi - lo))
    return [(i, rng.choice(SPECIAL_COEFFS) if rng.random() < 0.7 else rng.randrange(1, P)) for i in wires]


def satisfying_system(rng, n_wires, shapes, w=None):
    """shapes: (terms of A, of B, of C) per constraint, C >= 1 -> (constraints, witness): a random witness with
    w[0] = 1, random sparse A, B and all but one term of C, and the last C coefficient solved for on a wire with a
    non-zero value, falling back to C = v * w0."""
    w = random_witness(rng, n_wires) if w is None else w
    cons = []
    for na, nb, nc in shapes:
        a, b, c = random_lc(rng, n_wires, na), random_lc(rng, n_wires, nb), random_lc(rng, n_wires, nc - 1)
        need = (lc_value(a, w) * lc_value(b, w) - lc_value(c, w)) % P
        free = [i for i in rng.sample(range(n_wires), min(n_wires, 8)) if w[i] % P and i not in dict(c)]
        if free:
            c.append((free[0], need * pow(w[free[0]] % P, P - 2, P) % P))
        else:
            c.append((0, need))  # w0 = 1; a wire 0 already in C is then listed twice, and the coefficients add
        rng.shuffle(c)
        cons.append((a, b, c))
    assert evaluate(cons, w) == (-1, 0)
    return cons, w


def rows_of(witnesses, n_wires, pad=48):
    """witness integer lists -> (batch, 32 * n_wires + pad) uint8 rows, the padding 0xFF (it must not be read)"""
    out = np.full((len(witnesses), 32 * n_wires + pad), 0xFF, dtype=np.uint8)
    for r, w in enumerate(witnesses):
        assert len(w) == n_wires
        out[r, : 32 * n_wires] = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in w), dtype=np.uint8)
    return out


def perturbed(rng, w, k=1, among=None):
    """w with k elements other than w[0] replaced (among: the wires to choose from)"""
    v = list(w)
    for i in rng.sample(sorted(among) if among else range(1, len(w)), k):
        v[i] = (v[i] + 1 + rng.randrange(P - 1)) % P
    return v


# ---- the case list: name -> (n_wires, constraints, satisfying witness)
def _counts(m):
    rng = random.Random(0xC0 + m)
    return (300,) + satisfying_system(rng, 300, [(rng.randrange(4), rng.randrange(4), rng.randrange(1, 4)) for _ in range(m)])


def _budget():
    # 120 constraints of 3 x 20 terms: 42 fit the chunk's term budget, so chunks are cut at 42, not at 256
    rng = random.Random(0xB0)
    assert 256 * 60 > R1CS_CHUNK_TERMS
    return (500,) + satisfying_system(rng, 500, [(20, 20, 20)] * 120)


def _directed():
    """every LC shape and coefficient the issue lists, on a witness holding 0, 1, p - 1 and random values"""
    rng = random.Random(0xD1)
    n = 2048
    w = random_witness(rng, n)
    w[1], w[2], w[3], w[4], w[n - 1] = 0, 1, P - 1, rng.randrange(2, P), rng.randrange(2, P)
    rc = rng.randrange(2, P)
    cons = []

    def add(a, b, c, solve=True):
        cons.append((a, b, close_c(w, a, b, c) if solve else c))

    add([], [(5, 1)], [], solve=False)                    # empty A: 0 * B = 0 with an empty C
    add([(5, 1)], [], [], solve=False)                    # empty B, empty C
    add([], [], [], solve=False)                          # all empty
    add([(1, 7)], [(6, 3)], [], solve=False)              # A = 7 * w1 = 0, empty C
    add([(0, 1)], [(0, 1)], [(0, 1)], solve=False)        # wire 0 only: w0 * w0 = w0
    add([(0, P - 1)], [(0, 2)], [(0, P - 2)], solve=False)
    add([(n - 1, 1)], [(n - 1, P - 1)], [(n - 2, 5)])     # the last wire, through +1 and -1
    add([(n - 1, rc)], [(0, 1)], [(n - 1, rc)], solve=False)
    add([(7, 3), (7, 5), (7, P - 8)], [(8, 1)], [], solve=False)             # a wire three times, sum 0: no term
    add([(7, 3), (9, 1), (7, 5), (7, 11)], [(8, 1)], [(10, 2)])              # three times, sum 19
    add([(7, 1), (7, P - 1), (7, 1)], [(8, 1), (8, 1), (8, 1)], [(9, 1), (9, 1)])  # +-1 merging to 1, 3 and 2
    add([(11, 0), (12, 1)], [(13, 0)], [(14, 0)], solve=False)               # explicit zero coefficients: B = 0
    add([(11, 0), (12, 4)], [(13, 1), (2, 0)], [(14, 0), (15, 1)])
    for c in SPECIAL_COEFFS + [rc]:                       # each coefficient against each special value and a random one
        for i in (1, 2, 3, 4):
            add([(i, c)], [(0, 1)], [(i, c)], solve=False)
            add([(i, c), (20, 1)], [(21, c), (i, P - 1)], [(22, c)])
    add([(30, 2), (29, 1), (31, P - 1), (28, 1 << 64)], [(33, 1), (32, 1)], [(40, 1 << 253), (35, P - 2)])  # any order
    assert evaluate(cons, w) == (-1, 0)
    return n, cons, w


LONG_SIZES = [33, 64, 65, 249, 1000]


def _long(only_long=False):
    """long constraints of 33, 64, 65, 249 and 1,000 terms in A, in C, and in both, between short ones"""
    rng = random.Random(0x10 + only_long)
    n = 2048
    shapes = []
    for t in LONG_SIZES:
        for sh in ((t, 2, 3), (1, 2, t), (t, 1, t)):
            shapes.append(sh)
            if not only_long:
                shapes += [(rng.randrange(1, 4), rng.randrange(1, 4), rng.randrange(1, 4))] * rng.randrange(1, 3)
    if only_long:
        shapes = shapes[:2] + [(40, 40, 40)] + shapes[2:]
    return (n,) + satisfying_system(rng, n, shapes)


CASE_BUILDERS = {
    "m1": lambda: _counts(1), "m63": lambda: _counts(63), "m64": lambda: _counts(64), "m65": lambda: _counts(65),
    "m256": lambda: _counts(256), "m257": lambda: _counts(257), "budget": _budget, "directed": _directed,
    "long": _long, "only_long": lambda: _long(True),
}
BATCHES = [1, 3, R1CS_WT + 1]
_cases = {}


def case(name):
    """(n_wires, constraints, satisfying witness), built once"""
    if name not in _cases:
        _cases[name] = CASE_BUILDERS[name]()
    return _cases[name]


def batch_of(name, batch):
    """the case's witnesses for a batch: row 0 satisfies; the others alternate between the satisfying row with one or
    three elements replaced and an unrelated random row (which violates almost every constraint)"""
    n, cons, w = case(name)
    rng = random.Random(zlib.crc32(("%s/%d" % (name, batch)).encode()))
    read = {i for con in cons for lc in con for i, _ in lc} - {0}  # a replaced element is one the system reads
    rows = [w]
    for r in range(1, batch):
        rows.append(perturbed(rng, w, 1 if r % 3 == 1 else 3, read) if r % 3 else random_witness(rng, n))
    return rows


def residue_case():
    """Elements >= p (p, p + 1, 2^256 - 1) at wires read through +1, through -1 and through a general coefficient: the
    row must be judged as its residues are. The system holds on the residues, so any element read raw breaks it."""
    rng = random.Random(0xE5)
    n = 64
    w = random_witness(rng, n)
    big = {10: P, 11: P + 1, 12: (1 << 256) - 1, 13: P + 5, 14: (1 << 256) - 1, 15: P}
    g = rng.randrange(2, P)
    cons = []
    for i in (10, 11, 12):
        w[i] = big[i] % P
    for i in (13, 14, 15):
        w[i] = big[i] % P
    for i in (10, 11, 12, 13, 14, 15):
        for c in (1, P - 1, g, 2):
            a, b = [(i, c), (20, 1)], [(i, c), (21, P - 1)]
            cons.append((a, b, close_c(w[:22] + [0] * (n - 22), a, b, [(i, c)])))
    assert evaluate(cons, w) == (-1, 0)
    raw = list(w)
    for i, v in big.items():
        raw[i] = v
    assert evaluate(cons, raw) == (-1, 0)  # the evaluator reads residues
    return n, cons, raw


# ---- RegisterIdentityLight(256, 3): what DESIGN.md §13 states about the layout, as constraints over a whole row
LIGHT_HASH_BITS = 1029  # main: 1 | three outputs | dg1[1024], skIdentity | dg1HashBits[256]
LIGHT_SUM100 = 498 + 99  # the first constraint that reads b2n.sum[100]


def light_system(witness_size):
    """b2n = Bits2Num(248) is the last 2 * 248 + 1 elements: out | in[248] | sum[248]. In file order: w0 * w0 = w0 (0);
    in[k] (in[k] - 1) = 0 (1 .. 248); in[i] = dg1HashBits[255 - i] (249 .. 496); sum[0] = in[0] (497);
    sum[k] - sum[k - 1] = 2^k in[k] (498 .. 744: coefficients up to 2^247); out = sum over 2^k in[k], one 249-term LC
    on the long path (745); w[2] = dg1Hash = b2n.out and out = sum[247] (746, 747)."""
    out = witness_size - 497
    inp, acc = out + 1, out + 249
    one = [(0, 1)]
    cons = [(one, one, one)]
    cons += [([(inp + k, 1)], [(inp + k, 1), (0, P - 1)], []) for k in range(248)]
    cons += [([(inp + i, 1), (LIGHT_HASH_BITS + 255 - i, P - 1)], one, []) for i in range(248)]
    cons.append(([(acc, 1), (inp, P - 1)], one, []))
    cons += [([(acc + k, 1), (acc + k - 1, P - 1)], one, [(inp + k, 1 << k)]) for k in range(1, 248)]
    cons.append(([(inp + k, 1 << k) for k in range(248)] + [(out, P - 1)], one, []))
    cons.append(([(2, 1)], one, [(out, 1)]))
    cons.append(([(out, 1)], one, [(acc + 247, 1)]))
    assert acc + 100 in dict(cons[LIGHT_SUM100][0]) and all(acc + 100 not in dict(lc) for con in cons[:LIGHT_SUM100] for lc in con)
    return cons


# ---- a circom-sized local system, for tools/r1cs_rate.py
RATE_POOL = [1, P - 1, 2, P - 2, 1 << 64, 0x2A5C1B3D4E6F708192A3B4C5D6E7F8091A2B3C4D5E6F70819 % P]
RATE_POOL_P = [0.5, 0.35, 0.06, 0.03, 0.03, 0.03]  # circom's systems are mostly +-1


def local_system(m, seed=0x5EED, window=64, long_every=512, long_terms=254, general=None):
    """-> (.r1cs bytes, witness bytes, facts): m wires and m constraints in the shape of a circuit: wires 0 .. window
    are free (w0 = 1), constraint k < m - window defines wire k + window as A * B - C', with 1 - 3 terms per LC drawn
    from wires within +-window of k (all defined by then) and C = C' + 1 * w[k + window] (a C' of two terms starts with
    a constant, c * w0); the last `window`
    constraints close on wire 0 (C = v * w0). One constraint in long_every is long: A = long_terms preceding wires.
    Runs of long_every - 1 constraints share their term counts, so that numpy writes each run at once. Coefficients
    come from RATE_POOL with RATE_POOL_P (15 % other than +-1), or with `general` as the share of the four others."""
    rng = np.random.default_rng(seed)
    pool_p = RATE_POOL_P if general is None else [0.6 * (1 - general), 0.4 * (1 - general)] + [general / 4] * 4
    pool_b = np.frombuffer(b"".join(c.to_bytes(32, "little") for c in RATE_POOL), dtype=np.uint8).reshape(-1, 32)
    w = [0] * m
    w[0] = 1
    prng = random.Random(seed)
    for i in range(1, min(window, m)):
        w[i] = prng.randrange(P)
    parts, n_terms, n_long = [], 0, 0
    one_lc = lc_bytes([(0, 1)])
    k = 0
    while k < m:
        defines = k + window < m
        if k % long_every == long_every - 1 and k + window >= long_terms and defines:
            lo = k + window - long_terms
            ids = rng.choice(len(RATE_POOL), size=long_terms, p=pool_p)
            a = [(lo + i, RATE_POOL[c]) for i, c in enumerate(ids)]
            w[k + window] = lc_value(a, w)
            parts.append(lc_bytes(a) + one_lc + lc_bytes([(k + window, 1)]))
            n_terms += long_terms + 2
            n_long += 1
            k += 1
            continue
        end = min(m, (k // long_every) * long_every + long_every - 1)
        if defines:
            end = min(end, m - window)
        end = max(end, k + 1)
        n = end - k
        na, nb, nc = (int(x) for x in rng.integers(1, 4, size=3))
        ks = np.arange(k, end)
        cols = na + nb + nc
        wires = ks[:, None] + rng.integers(-window, window, size=(n, cols))
        wires = np.clip(wires, 0, np.minimum(ks + window, m)[:, None] - 1)
        ids = rng.choice(len(RATE_POOL), size=(n, cols), p=pool_p)
        if defines:
            wires[:, cols - 1] = ks + window  # C's last term: + the wire this constraint defines
        else:
            wires[:, cols - 1] = 0            # C = ... + v * w0, v solved below
        ids[:, cols - 1] = 0
        if nc >= 2:
            wires[:, na + nb] = 0  # a constant in C: keeps zeros (A = 0 or B = 0) from spreading down the chain
        term = np.dtype([("wire", "<u4"), ("coeff", "u1", (32,))])
        rec = np.dtype([("na", "<u4"), ("a", term, (na,)), ("nb", "<u4"), ("b", term, (nb,)), ("nc", "<u4"), ("c", term, (nc,))])
        out = np.zeros(n, dtype=rec)
        out["na"], out["nb"], out["nc"] = na, nb, nc
        for name, c0, cnt in (("a", 0, na), ("b", na, nb), ("c", na + nb, nc)):
            out[name]["wire"] = wires[:, c0:c0 + cnt]
            out[name]["coeff"] = pool_b[ids[:, c0:c0 + cnt]]
        wl, il = wires.tolist(), ids.tolist()
        for r in range(n):
            wr, ir = wl[r], il[r]
            va = sum(RATE_POOL[ir[j]] * w[wr[j]] for j in range(na)) % P
            vb = sum(RATE_POOL[ir[j]] * w[wr[j]] for j in range(na, na + nb)) % P
            vc = sum(RATE_POOL[ir[j]] * w[wr[j]] for j in range(na + nb, cols - 1)) % P
            v = (va * vb - vc) % P
            if defines:
                w[k + r + window] = v
            else:
                out["c"]["coeff"][r, nc - 1] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)
        parts.append(out.tobytes())
        n_terms += n * cols
        k = end
    body = b"".join(parts)
    data = assemble([(1, header_payload(m, m)), (2, body)])
    wit = b"".join(v.to_bytes(32, "little") for v in w)
    return data, wit, dict(n_terms_listed=n_terms, n_long=n_long)
