"""Directed operands for the device arithmetic primitives, and small models of their branch structure.

Everything here is plain Python on integers, seeded, and needs no GPU. The EXPECTED value of every case is a plain
integer expression (a * b * R^-1 % p, divmod, pow(a, -1, m); for the non-canonical products also mont_exact, the
Montgomery reduction without a final subtraction); it never comes from a model. The lane-level models
(fq settles, borrow lookahead, Knuth D, divlu, div_preinv, the Barrett estimate) exist only to SELECT cases and to
show on the CPU (tests/test_arith_cases.py) that the selected cases reach the rare branches that random operands
reach with probability 2^-32 .. 2^-96. tests/test_gpu_arith.py runs the same cases through libpzkprobe.so.

Contracts, quoted from the comments above the functions (an operand outside the contract is not a test case):
  fr_reduce_once   "r = a - p if a >= p (a < 2p)"
  fr_add / fr_sub  canonical operands (sum < 2p through fr_reduce_once; fr_sub adds p once)
  fr_mul / fr_sqr  "Montgomery product a*b*2^-256 mod p" with the "no final carry" shortcut: operands < 2p
                   (fr_to_mont_in's comment: "fine for a < 2p"); second operand of fr_mul(R2, a) any 256-bit value
  fr_mul_fast      "fr_mul_fast: < (2.2p * 2.2p + R p) / R < 2p before its final subtraction" (smt_chain4.hpp):
                   operands <= floor(2.2 p)
  fr_from_mont_fast "fr_from_mont_fast: < p + 1" for inputs below 2.2p (same comment)
  fr_geq_p, fr_to_mont_in  "for ANY 256-bit a"
  fr_inv*          Montgomery in/out, "inverse of 0 is 0"; canonical operand
  fq_mul, fq_mul64 "a, b < 2p: result < 2p, normalised"
  fq_mulq / fq_dot "Result < (K + sum_r |a_r| |b_r| + R p) / R; the caller keeps it below 2^256", "K (< p)";
                   operands up to 2.2p ("With canonical constants every state stays below 2.2p (products of inputs
                   < 2.2p are < 2.0p + the K term ...)", smt_chain4.hpp): the first operands and b_0 are states
                   (<= 2.2p), b_1 and b_2 the chain's canonical constants (< p); fq_mulq(raw, R^2) with raw any
                   256-bit value is the chain's to_mont
  fq_canon         "a - p if a >= p (a < 2p)"
  fq_geq_p         "a >= p for any 256-bit a"
  fq_add_raw       "a + b (no reduction; callers keep the sum < 2^256)"
  divlu            "requires u1 < v and v normalised"
  div_preinv       "requires u1 < v", v normalised, vinv = floor((2^128 - 1) / v) - 2^64
  kd_div           "a: na words, b: nb >= 2 words with b[nb-1] != 0"
  mp_divmod<NB>    "b = NB words with b[NB-1] != 0 (this curve's p or n)"; na <= 31 (its u[32])
  m_mul_inl & co   operands < m (m_reduce: "t < 2m, t given with a carry word")
"""
import functools
import random

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
R = 1 << 256
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617  # BN254 Fr (fr.hpp P_)
PINV = 0xefffffff  # -p^-1 mod 2^32 (fr.hpp)
R1 = R % P
R2 = R * R % P
RINV = pow(R, -1, P)
LIM22 = 22 * P // 10  # floor(2.2 p)
SEED = 20240607
MAX_CASES = 4096  # per probe launch

assert (P * PINV + 1) & M32 == 0


def words32(v, n=8):
    return [(v >> (32 * i)) & M32 for i in range(n)]


def words64(v, n):
    return [(v >> (64 * i)) & M64 for i in range(n)]


def digits(v):
    return [(v >> (64 * i)) & M64 for i in range(4)]


def from_digits(d):
    return sum(x << (64 * i) for i, x in enumerate(d))


PD = digits(P)

# ----------------------------------------------------------------------------------------------- field values


def edge_values(limit):
    """0, 1, 2, p-2, p-1, R mod p, R^2 mod p, 2^k and 2^k - 1 at every word boundary, single all-ones words (32 and
    64 bit), the contract's own ends, all below `limit` (exclusive)."""
    v = [0, 1, 2, P - 2, P - 1, P, P + 1, 2 * P - 1, 2 * P, LIM22 - 1, LIM22, R1, R2, R - 1, R - 2]
    for k in range(32, 257, 32):
        v += [1 << k, (1 << k) - 1, (1 << k) + 1]
    for i in range(8):
        v.append(M32 << (32 * i))
    for i in range(4):
        v.append(M64 << (64 * i))
        v.append(R - 1 - (M64 << (64 * i)))
    out = []
    for x in v:
        if 0 <= x < limit and x not in out:
            out.append(x)
    return out


def rand_values(rng, n, limit):
    return [rng.randrange(limit) for _ in range(n)]


DIGIT_SET = [0, 1, M64 - 1, M64, 1 << 32, M32, M64 - M32, 1 << 63]


def target_values(rng, n, limit):
    """Values below `limit` whose 64-bit digits come from {0, 1, 2^64-2, 2^64-1, 2^32, ...} or are random: results
    with such digits are what the carry settles' generate / propagate branches need."""
    out = []
    top_max = limit >> 192
    while len(out) < n:
        d = [rng.choice(DIGIT_SET) if rng.random() < 0.8 else rng.getrandbits(64) for _ in range(3)]
        t = rng.choice([0, 1, top_max, top_max - 1, rng.randrange(top_max + 1)])
        v = from_digits(d + [t])
        if v < limit:
            out.append(v)
    return out


# ----------------------------------------------------------------------------------------------- fr (one lane)

FR_OPS = ["add", "sub", "reduce_once", "geq_p", "mul", "sqr", "mul_fast", "from_mont", "from_mont_fast", "to_mont",
          "to_mont_in", "inv", "inv_fast", "inv_sw", "inv_sw_fast", "from_i128"]
FR_BINARY = {"add", "sub", "mul", "mul_fast"}
# exclusive operand limits per the contracts above
FR_LIMIT = {"add": P, "sub": P, "reduce_once": 2 * P, "geq_p": R, "mul": 2 * P, "sqr": 2 * P, "mul_fast": LIM22 + 1,
            "from_mont": 2 * P, "from_mont_fast": LIM22 + 1, "to_mont": 2 * P, "to_mont_in": R, "inv": P,
            "inv_fast": P, "inv_sw": P, "inv_sw_fast": P}


def fr_expected(op, a, b=0):
    if op == "add": return (a + b) % P
    if op == "sub": return (a - b) % P
    if op == "reduce_once": return a - P if a >= P else a
    if op == "geq_p": return 1 if a >= P else 0
    if op in ("mul", "mul_fast"): return a * b * RINV % P
    if op == "sqr": return a * a * RINV % P
    if op in ("from_mont", "from_mont_fast"): return a * RINV % P
    if op in ("to_mont", "to_mont_in"): return a * R % P
    if op.startswith("inv"): return 0 if a % P == 0 else pow(a * RINV % P, -1, P) * R % P  # Montgomery in and out
    if op == "from_i128":
        x = a & ((1 << 128) - 1)
        return (x - (1 << 128)) % P if x >> 127 else x
    raise KeyError(op)


def fr_cases(op, seed=SEED):
    """[(a, b)] for one fr function."""
    rng = random.Random("%d fr %s" % (seed, op))
    if op == "from_i128":
        e = [0, 1, M64, 1 << 64, (1 << 127) - 1, 1 << 127, (1 << 127) + 1, (1 << 128) - 1, (1 << 128) - M64 - 1,
             (1 << 128) - (1 << 64), M64 << 64]
        return [(x, 0) for x in e + [rng.getrandbits(128) for _ in range(500)]]
    lim = FR_LIMIT[op]
    edges = edge_values(lim)
    n_rand = 40 if op.startswith("inv") else 600
    singles = edges + rand_values(rng, n_rand, lim) + target_values(rng, 60 if op.startswith("inv") else 400, lim)
    if op not in FR_BINARY:
        if op in ("from_mont", "from_mont_fast", "to_mont", "to_mont_in", "sqr"):
            # pre-images: results with chosen digits
            for v in target_values(rng, 300, P):
                if op in ("from_mont", "from_mont_fast"):
                    singles.append(v * R % P)
                elif op in ("to_mont", "to_mont_in"):
                    singles.append(v * RINV % P)
        return [(a, 0) for a in singles]
    cases = [(a, b) for a in edges for b in edges]
    if len(cases) > 1500:
        cases = rng.sample(cases, 1500)
    cases += [(a, rng.choice(singles)) for a in singles]
    if op in ("mul", "mul_fast"):
        for v in target_values(rng, 800, P):  # b = v R / a: the product is v
            a = rng.randrange(1, P)
            b = v * R * pow(a, -1, P) % P
            if rng.random() < 0.3 and a + P < lim: a += P
            if rng.random() < 0.3 and b + P < lim: b += P
            cases.append((a, b))
    if op in ("add", "sub"):
        for v in target_values(rng, 400, P):  # sums / differences with chosen digits, and the ends around p
            a = rng.randrange(P)
            cases.append((a, (v - a) % P) if op == "add" else (a, (a - v) % P))
        cases += [(a, P - a) for a in rand_values(rng, 20, P) if a] + [(a, P - 1 - a) for a in rand_values(rng, 20, P)]
    return cases[:MAX_CASES]


def fr_batch_inv_cases(seed=SEED):
    """[(m, [x_0 .. x_{m-1}])], Montgomery form, zeros at chosen positions."""
    rng = random.Random("%d fr batch_inv" % seed)
    out = []
    for m in range(1, 9):
        for zmask in sorted({0, 1, 1 << (m - 1), (1 << m) - 1, 0x55 & ((1 << m) - 1), 0xaa & ((1 << m) - 1),
                             rng.getrandbits(m), rng.getrandbits(m)}):
            for _ in range(3):
                out.append((m, [0 if (zmask >> i) & 1 else rng.choice([1, R1, P - 1, rng.randrange(1, P)])
                                for i in range(m)]))
    return out


# ----------------------------------------------------------------------------------------------- fq models
# Events. Carry settles (fq_settle, fq_settle_eo, fq_add_raw): gen<q> = lane q carries out of its digit, prop<q> =
# lane q's digit is all ones AND a carry comes in (the lookahead passes it on), ripple = a carry comes into a lane
# whose low word is all ones (the final add carries into the high word). Borrow lookahead (fq_canon, fq_geq_p): the
# same names for borrows; prop<q> = the digit equals p's digit and a borrow comes in.
#
# Unreachable, by the models and by the ranges:
#   gen0 / prop1 in fq_settle and fq_settle_eo: quad lane 0 receives lane 3's pending word, which is 0 for every value
#       below 2^256, so lane 0 never generates and no carry ever enters lane 1 for lane 1 to pass on.
#   gen3 / prop3 in every settle: the result is below 2^256 (callers' ranges), so the top lane never carries out; its
#       ballot bits are masked (NOT_TOP) and nothing reads them.
#   pend1 in fq_settle_eo (a pending word y1 != 0): the column tops et, ot stay below 8 (a column adds at most
#       2 (NR + 1) products below 2^64 per iteration), so y0 + carries never reach 2^32.
SETTLE_EVENTS = ["gen1", "gen2", "prop2", "ripple"]
ADD_EVENTS = ["gen0", "gen1", "gen2", "prop1", "prop2", "ripple"]
# fq_canon / fq_geq_p: a borrow out of lane 3 (gen3 / prop3) is the "a < p" answer itself and is reachable
BORROW_EVENTS = ["gen0", "gen1", "gen2", "gen3", "prop1", "prop2", "prop3", "ripple"]


def _lookahead(g, pr):
    """carry into each lane of a quad: quad_carry_in with NOT_TOP (nothing enters lane 0)"""
    c = [0, 0, 0, 0]
    for q in range(3):
        c[q + 1] = 1 if (g[q] or (pr[q] and c[q])) else 0
    return c


def _settle(z, g, ev):
    """z: per lane (z0, z1) after the pending word went in, g: carry out of that; the ballot step of the settles"""
    pr = [(z0 & z1) == M32 for z0, z1 in z]
    c = _lookahead(g, pr)
    assert not g[3], "value >= 2^256"
    for q in range(4):
        if g[q]: ev.add("gen%d" % q)
        if pr[q] and c[q]: ev.add("prop%d" % q)
        if c[q] and z[q][0] == M32: ev.add("ripple")
    out = []
    for q in range(4):
        s = z[q][0] + c[q]
        out.append((s & M32) | (((z[q][1] + (s >> 32)) & M32) << 32))
    return from_digits(out)


def _fq_settle(x, ev):
    """fq_settle over the quad: x[q] = (x0, x1, x2)"""
    z, g = [], []
    for q in range(4):
        cin = x[(q - 1) & 3][2]
        s = x[q][0] + cin
        z0 = s & M32
        s = x[q][1] + (s >> 32)
        z.append((z0, s & M32))
        g.append(s >> 32)
    return _settle(z, g, ev)


def model_fq_mul(a, b):
    """lane-level model of fq_mul: (value, events)"""
    aw, bd = words32(a), digits(b)
    x = [[0, 0, 0] for _ in range(4)]
    for j in range(8):
        aj = aw[j]
        X = [aj * (bd[q] & M32) + x[q][0] for q in range(4)]
        m = ((X[0] & M32) * PINV) & M32
        Z, nxt = [], []
        for q in range(4):
            Y = aj * (bd[q] >> 32) + (X[q] >> 32) + x[q][1]
            assert Y <= M64
            z = m * (PD[q] & M32) + (X[q] & M32)
            W = m * (PD[q] >> 32) + (z >> 32) + (Y & M32)
            Z.append(z & M32)
            nxt.append((W, Y))
        assert Z[0] == 0
        for q in range(4):
            W, Y = nxt[q]
            S = x[q][2] + (Y >> 32) + (W >> 32) + Z[(q + 1) & 3]
            x[q] = [W & M32, S & M32, S >> 32]
    ev = set()
    return _fq_settle(x, ev), ev


def model_fq_mul64(a, b):
    """lane-level model of fq_mul64 (the 96-bit accumulator of fr_mac as one integer per lane)"""
    aw, bd = words32(a), digits(b)
    T = [0, 0, 0, 0]
    for J in range(4):
        a0, a1 = aw[2 * J], aw[2 * J + 1]
        blo = [d & M32 for d in bd]
        bhi = [d >> 32 for d in bd]
        plo = [d & M32 for d in PD]
        phi = [d >> 32 for d in PD]
        T = [T[q] + a0 * blo[q] for q in range(4)]
        m0 = ((T[0] & M32) * PINV) & M32
        T = [T[q] + m0 * plo[q] for q in range(4)]
        w0 = [t & M32 for t in T]
        T = [(T[q] >> 32) + a0 * bhi[q] + a1 * blo[q] + m0 * phi[q] for q in range(4)]
        m1 = ((T[0] & M32) * PINV) & M32
        T = [T[q] + m1 * plo[q] for q in range(4)]
        w1 = [t & M32 for t in T]
        assert w0[0] == 0 and w1[0] == 0
        T = [(T[q] >> 32) + a1 * bhi[q] + m1 * phi[q] for q in range(4)]
        T = [T[q] + (w0[(q + 1) & 3] | (w1[(q + 1) & 3] << 32)) for q in range(4)]
        assert all(t < (1 << 96) for t in T)
    ev = set()
    return _fq_settle([[t & M32, (t >> 32) & M32, t >> 64] for t in T], ev), ev


def model_fq_dot(rows, k):
    """lane-level model of fq_dot<NR>: rows = [(a_r, b_r)], K = k; fq_mulq(a, b) is model_fq_dot([(a, b)], 0)"""
    kd = digits(k)
    E = [d & M32 for d in kd]
    O = [d >> 32 for d in kd]
    aw = [words32(a) for a, _ in rows]
    bd = [digits(b) for _, b in rows]
    for j in range(8):
        for r in range(len(rows)):
            for q in range(4):
                E[q] += aw[r][j] * (bd[r][q] & M32)
                O[q] += aw[r][j] * (bd[r][q] >> 32)
        m = ((E[0] & M32) * PINV) & M32
        for q in range(4):
            E[q] += m * (PD[q] & M32)
            O[q] += m * (PD[q] >> 32)
        assert E[0] & M32 == 0 and all(e < (1 << 96) for e in E + O)
        nx = [E[(q + 1) & 3] & M32 for q in range(4)]
        E = [O[q] + (E[q] >> 32) for q in range(4)]
        O = nx
    ev = set()
    x0, x1, y0, y1 = [], [], [], []
    for q in range(4):
        e, et, o = E[q] & M64, E[q] >> 64, O[q]
        assert E[q] < (1 << 96)
        x0.append(e & M32)
        s = (e >> 32) + (o & M32)
        x1.append(s & M32)
        s = et + (o >> 32) + (s >> 32)
        y0.append(s & M32)
        y1.append(s >> 32)
        if y1[q]: ev.add("pend1")
    z, g = [], []
    for q in range(4):
        s = x0[q] + y0[(q - 1) & 3]
        z0 = s & M32
        s = x1[q] + y1[(q - 1) & 3] + (s >> 32)
        z.append((z0, s & M32))
        g.append(s >> 32)
    return _settle(z, g, ev), ev


def model_fq_borrow(a):
    """fq_canon / fq_geq_p: (canonical value for a < 2p else None, a >= p, events)"""
    ad = digits(a)
    d0, d1, g = [], [], []
    for q in range(4):
        d = (ad[q] & M32) - (PD[q] & M32)
        d0.append(d & M32)
        d = (ad[q] >> 32) - (PD[q] >> 32) - (1 if d < 0 else 0)
        d1.append(d & M32)
        g.append(1 if d < 0 else 0)
    pr = [(d0[q] | d1[q]) == 0 for q in range(4)]
    c = _lookahead(g, pr)
    ev = set()
    for q in range(4):
        if g[q]: ev.add("gen%d" % q)
        if pr[q] and c[q]: ev.add("prop%d" % q)
        if c[q] and d0[q] == 0: ev.add("ripple")
    lt = bool(g[3] or (pr[3] and c[3]))
    out = []
    for q in range(4):
        d = d0[q] - c[q]
        e0 = d & M32
        e1 = (d1[q] - (1 if d < 0 else 0)) & M32
        out.append(e0 | (e1 << 32))
    return (a if lt else from_digits(out)), (not lt), ev


def model_fq_add_raw(a, b):
    ad, bd = digits(a), digits(b)
    z, g = [], []
    for q in range(4):
        s = (ad[q] & M32) + (bd[q] & M32)
        s0 = s & M32
        s = (ad[q] >> 32) + (bd[q] >> 32) + (s >> 32)
        z.append((s0, s & M32))
        g.append(s >> 32)
    ev = set()
    return _settle(z, g, ev), ev


# ----------------------------------------------------------------------------------------------- fq cases
FQ_OPS = ["mul", "mul64", "mulq", "dot1", "dot2", "dot3", "canon", "geq_p", "add_raw"]
FQ_NR = {"dot1": 1, "dot2": 2, "dot3": 3}


class FqCase:
    """One quad's operands: a, b[3], k. For the dots the first operands are the `a` of quads 0..2 of the case's
    16-lane row (four consecutive cases, the first at a multiple of 4)."""
    __slots__ = ("a", "b", "k")

    def __init__(self, a, b=(0, 0, 0), k=0):
        self.a, self.b, self.k = a, tuple(b), k


FQ_LAYOUT = 17 * 16  # the neighbour layout: the last 17 waves of every fq case list
PNEG = (-pow(P, -1, R)) % R  # -p^-1 mod 2^256


def mont_exact(t):
    """The Montgomery reduction of t without a final subtraction, as one plain-integer expression: the word-serial
    products add m_j p 2^(32 j) with m_j chosen to clear word j, and sum_j m_j 2^(32 j) = -t p^-1 mod R is the only
    multiple of p below R p that makes the sum divisible by R. fq_mul, fq_mul64, fq_mulq and fq_dot return exactly
    this for t = K + sum_r a_r b_r (not only a value congruent to it)."""
    return (t + (t * PNEG % R) * P) // R


def fq_total(op, cases, i):
    """t = K + sum_r a_r b_r of case i of a product"""
    c = cases[i]
    if op in FQ_NR:
        row = cases[i & ~3:(i & ~3) + 4]
        return c.k + sum(row[r].a * c.b[r] for r in range(FQ_NR[op]))
    return c.a * c.b[0]


def _pad16(cases, room):
    """cut to `room` and to whole waves, so that the layout appended after it starts at quad 0 of a wave"""
    return cases[:min(len(cases), room) & ~15]


def _carry_targets(rng, n, lim):
    """results whose middle digits are zero or all ones under a random low and top digit: what a carry that a lane
    generates and the next lane passes on (prop2) leaves behind"""
    out = []
    while len(out) < n:
        lo = rng.choice([0, 1, M64, M64 - 1, rng.getrandbits(64), rng.getrandbits(32)])
        mid = rng.choice([[0, 0], [M64, M64], [rng.getrandbits(64), 0], [rng.getrandbits(64), M64], [0, M64]])
        v = from_digits([lo] + mid + [rng.randrange((lim >> 192) + 1)])
        if v < lim:
            out.append(v)
    return out


def _settle_model(op):
    return {"mul": model_fq_mul, "mul64": model_fq_mul64}.get(op, lambda a, b: model_fq_dot([(a, b)], 0))


def _preimage(rng, v, lim):
    a = rng.randrange(1, P)
    b = v * R * pow(a, -1, P) % P
    if rng.random() < 0.3 and a + P < lim: a += P
    if rng.random() < 0.3 and b + P < lim: b += P
    return a, b


def _mul_case(rng, v, lim):
    """operands with a * b * R^-1 = v (mod p): the pre-image b = v R / a, sometimes plus p where the contract allows"""
    a, b = _preimage(rng, v, lim)
    return FqCase(a, (b, 0, 0))


def _ones_target(rng, top):
    """three all-ones low digits under a random top digit: a stray carry in would ripple through every lane"""
    return from_digits([M64, M64, M64, rng.randrange(top)])


def _mul_ones_case(rng, lim):
    """operands whose exact result (not only its residue) has three all-ones low digits; fixed try count"""
    for _ in range(400):
        w = _ones_target(rng, (2 * P) >> 192)
        a, b = _preimage(rng, w % P, lim)
        if mont_exact(a * b) == w:
            return FqCase(a, (b, 0, 0))
    raise AssertionError("no all-ones result found")


def _mul_layout(rng, op, cases, lim):
    """17 waves of 16 quads: in quad i of wave i a case whose settle generates or propagates a carry inside the quad
    (selected by the model from `cases`), in quad i + 1 a case whose result has all-ones low digits, for every quad
    position i (i = 3, 7, 11 cross a row boundary, i = 15 the wave boundary). A carry must never cross a quad."""
    model, busy = _settle_model(op), []
    for c in cases:
        if model(c.a, c.b[0])[1] & {"gen1", "gen2", "prop2"}:
            busy.append(c)
            if len(busy) == 16: break
    assert len(busy) == 16
    lay = [rng.choice(cases) for _ in range(FQ_LAYOUT)]
    for i in range(16):
        lay[16 * i + i] = busy[i]
        lay[16 * i + i + 1] = _mul_ones_case(rng, lim)
    return lay


def _dot_bk(rng, nr, arow, edges, v):
    """(b[3], k) with K + sum_r a_r b_r = v R (mod p) for the row's first operands `arow`"""
    b = [0, rng.choice(edges + [rng.randrange(P)] * 40) % P, rng.choice(edges + [rng.randrange(P)] * 40) % P]
    k = rng.choice([0, 1, P - 1, R1, rng.randrange(P), rng.randrange(P)])
    rest = k + sum(arow[r] * b[r] for r in range(1, nr))
    b[0] = (v * R - rest) * pow(arow[0], -1, P) % P
    if rng.random() < 0.3 and b[0] + P <= LIM22: b[0] += P
    return b, k


def _dot_ones_bk(rng, nr, arow, edges):
    for _ in range(400):
        w = _ones_target(rng, (11 * P // 4) >> 192)
        b, k = _dot_bk(rng, nr, arow, edges, w % P)
        if mont_exact(k + sum(arow[r] * b[r] for r in range(nr))) == w:
            return b, k
    raise AssertionError("no all-ones result found")


def _dot_arow(rng, edges):
    arow = [rng.choice(edges) if rng.random() < 0.15 else rng.randrange(1, LIM22 + 1) for _ in range(4)]
    while arow[0] % P == 0:
        arow[0] = rng.randrange(1, LIM22 + 1)
    return arow


def _dot_layout(rng, nr, cases, edges, tg):
    """_mul_layout for the dots. A case's first operands belong to its 16-lane row, so the busy case moves to quad
    i % 4 of a row with its own row's first operands, and the row's other cases are built against them."""
    busy = []
    for i, c in enumerate(cases):
        row = [r.a for r in cases[i & ~3:(i & ~3) + 4]]
        if model_fq_dot([(row[r], c.b[r]) for r in range(nr)], c.k)[1] & {"gen1", "gen2", "prop2"}:
            busy.append((row, c.b, c.k))
            if len(busy) == 16: break
    assert len(busy) == 16
    rows = []
    for _ in range(FQ_LAYOUT // 4):
        arow = _dot_arow(rng, edges)
        rows.append((arow, [_dot_bk(rng, nr, arow, edges, rng.choice(tg)) for _ in range(4)]))
    for i in range(16):
        at, col = 4 * i + i // 4, i % 4
        arow, b, k = busy[i]
        bks = [_dot_bk(rng, nr, arow, edges, rng.choice(tg)) for _ in range(4)]
        bks[col] = (list(b), k)
        if col < 3:
            bks[col + 1] = _dot_ones_bk(rng, nr, arow, edges)
        else:
            rows[at + 1][1][0] = _dot_ones_bk(rng, nr, rows[at + 1][0], edges)
        rows[at] = (arow, bks)
    return [FqCase(arow[c], bks[c][0], bks[c][1]) for arow, bks in rows for c in range(4)]


def fq_cases(op, seed=SEED):
    """[FqCase] for one fq function, at most MAX_CASES, whole waves, the last FQ_LAYOUT of them the neighbour layout"""
    return list(_fq_cases(op, seed))


@functools.lru_cache(maxsize=None)
def _fq_cases(op, seed):
    rng = random.Random("%d fq %s" % (seed, op))
    room = MAX_CASES - FQ_LAYOUT
    if op in ("mul", "mul64"):
        # "a, b < 2p: result < 2p, normalised"
        lim = 2 * P
        edges = edge_values(lim)
        tg = target_values(rng, 2400, P) + _carry_targets(rng, 400, P)
        cases = [_mul_case(rng, v, lim) for v in tg]
        cases += [FqCase(rng.randrange(lim), (rng.randrange(lim), 0, 0)) for _ in range(300)]
        cases += [FqCase(a, (b, 0, 0)) for a in edges for b in rng.sample(edges, 6)]
        cases = _pad16(cases, room)
        return tuple(cases + _mul_layout(rng, op, cases, lim))
    if op == "mulq":
        # products of values up to 2.2p ("products of inputs < 2.2p are < 2.0p", smt_chain4.hpp), and the chain's
        # to_mont: fq_mulq(raw, R^2) with raw any 256-bit value (raw R^2 < R p, so that result is below 2p too)
        lim = LIM22 + 1
        edges = edge_values(lim)
        tg = target_values(rng, 1800, P) + _carry_targets(rng, 400, P)
        cases = [_mul_case(rng, v, lim) for v in tg]
        cases += [FqCase(a, (R2, 0, 0)) for a in edge_values(R) + rand_values(rng, 200, R)]
        cases += [FqCase(v * RINV % P + rng.choice([0, 0, P, 2 * P, 3 * P, 4 * P]), (R2, 0, 0))
                  for v in target_values(rng, 500, P)]
        cases += [FqCase(a, (b, 0, 0)) for a in edges for b in rng.sample(edges, 4)]
        cases = _pad16(cases, room)
        return tuple(cases + _mul_layout(rng, op, cases, lim))
    if op in FQ_NR:
        # The contract tested is the chain's (smt_chain4.hpp): "With canonical constants every state stays below 2.2p
        # (products of inputs < 2.2p are < 2.0p + the K term ...)". The first operands a_r are states (<= 2.2p); b_0
        # is a state or a product of states (<= 2.2p: "x^3 (x) (S0 x^2)"); b_1 and b_2 are always canonical constants
        # (Mat, S1, S2, 1), so they stay below p here; "K (< p)". Then K + sum < (4.84 + 2.2 + 2.2) p^2 + p < 2 p R,
        # the result is below 3p, and two fq_canon (the chain's "two conditional subtractions") make it canonical.
        nr = FQ_NR[op]
        edges = edge_values(LIM22 + 1)
        tg = target_values(rng, 2400, P) + _carry_targets(rng, 400, P)
        rng.shuffle(tg)
        cases = []
        for r0 in range(0, min(len(tg), room) & ~15, 4):
            arow = _dot_arow(rng, edges)
            for c in range(4):
                b, k = _dot_bk(rng, nr, arow, edges, tg[r0 + c])
                cases.append(FqCase(arow[c], b, k))
        return tuple(cases + _dot_layout(rng, nr, cases, edges, tg))
    if op in ("canon", "geq_p"):
        # fq_canon: "a - p if a >= p (a < 2p)"; fq_geq_p: "a >= p for any 256-bit a"
        lim = 2 * P if op == "canon" else R
        vals = edge_values(lim)
        # every digit: p's digit, p's digit -+ 1, the same low word with the high word -+ 1, 0, all ones, random
        def alts(q):
            d = PD[q]
            return [d, (d - 1) & M64, (d + 1) & M64, (d - (1 << 32)) & M64, (d + (1 << 32)) & M64, 0, M64,
                    rng.getrandbits(64)]
        for d0 in alts(0):
            for d1 in alts(1):
                for d2 in alts(2):
                    for d3 in alts(3):
                        vals.append(from_digits([d0, d1, d2, d3]))
        vals = [v for v in vals if v < lim]
        if len(vals) > room - 600:
            vals = vals[:60] + rng.sample(vals[60:], room - 660)
        vals += rand_values(rng, 300, lim)
        vals = _pad16(vals, room)
        # neighbours: a value below p (a borrow leaves the top lane) next to p itself and p + 2^64, p + 2^128 (the lowest
        # digit is p's, so an incoming borrow would be passed on)
        lay = [rng.choice(vals) for _ in range(FQ_LAYOUT)]
        for i in range(16):
            lay[16 * i + i] = [P - 1, from_digits([0, 0, 0, PD[3]]), 0, from_digits(PD[:3] + [PD[3] - 1])][i % 4]
            lay[16 * i + i + 1] = [P, from_digits([PD[0], PD[1] + 1, PD[2], PD[3]]),
                                   from_digits([PD[0], PD[1], PD[2] + 1, PD[3]]), P][i % 4]
        return tuple(FqCase(v) for v in vals + lay)
    if op == "add_raw":
        # "a + b (no reduction; callers keep the sum < 2^256)"
        # per digit a pair (x, y): sum all ones (propagate), sum 2^64 (generate, digit 0), all ones twice, ...
        def pairs():
            x = rng.getrandbits(64)
            return [(x, M64 - x), (x, (M64 - x + 1) & M64), (M64, M64), (M64, 1), (0, 0), (M32, 1),
                    (rng.getrandbits(64), rng.getrandbits(64)), (M64 - M32, M32)]
        cases = []
        for p0 in pairs():
            for p1 in pairs():
                for p2 in pairs():
                    for p3 in pairs():
                        a = from_digits([p0[0], p1[0], p2[0], p3[0]])
                        b = from_digits([p0[1], p1[1], p2[1], p3[1]])
                        if a + b < R:
                            cases.append(FqCase(a, (b, 0, 0)))
        cases = rng.sample(cases, min(len(cases), 3000))
        e = edge_values(R)
        cases += [FqCase(a, (b, 0, 0)) for a in e for b in rng.sample(e, 8) if a + b < R][:600]
        cases = _pad16(cases, room)
        # neighbours: a carry generated in lane 0 that runs through all-ones digits up into the top lane (the sum stays
        # below 2^256, so the top lane itself never carries out) next to a sum with all-ones low digits
        lay = [rng.choice(cases) for _ in range(FQ_LAYOUT)]
        for i in range(16):
            t = rng.getrandbits(62)
            lay[16 * i + i] = FqCase(from_digits([M64, M64, M64, t]), (from_digits([1 + rng.getrandbits(32), 0, 0, t]), 0, 0))
            y = rng.getrandbits(190)
            lay[16 * i + i + 1] = FqCase(y, ((1 << 192) - 1 - y, 0, 0))
        return tuple(cases + lay)
    raise KeyError(op)


def fq_expected(op, cases):
    """[(kind, value)] per case from plain integers: kind 'mod' = the result is only fixed modulo p (value is the
    canonical residue), 'exact' = bit-exact"""
    out = []
    for i, c in enumerate(cases):
        if op in ("mul", "mul64", "mulq"):
            out.append(("mod", c.a * c.b[0] * RINV % P))
        elif op in FQ_NR:
            row = cases[i & ~3:(i & ~3) + 4]
            out.append(("mod", (c.k + sum(row[r].a * c.b[r] for r in range(FQ_NR[op]))) * RINV % P))
        elif op == "canon":
            out.append(("exact", c.a - P if c.a >= P else c.a))
        elif op == "geq_p":
            out.append(("exact", 1 if c.a >= P else 0))
        elif op == "add_raw":
            out.append(("exact", c.a + c.b[0]))
    return out


def fq_exact(op, cases, i):
    """the exact (non-canonical) result of product case i from plain integers"""
    return mont_exact(fq_total(op, cases, i))


def fq_result_bound(op, cases, i):
    """exclusive bound of the non-canonical result of case i: 2p for fq_mul / fq_mul64 ("a, b < 2p: result < 2p") and
    for fq_mulq ("products of inputs < 2.2p are < 2.0p"; raw R^2 < R p for the chain's to_mont), and for fq_dot its
    comment's "Result < (K + sum_r |a_r| |b_r| + R p) / R" on the case's own operands"""
    if op in FQ_NR:
        return -(-(fq_total(op, cases, i) + R * P) // R)
    return 2 * P


def fq_model(op, cases, i):
    """(value, events) of case i by the lane-level model"""
    c = cases[i]
    if op == "mul": return model_fq_mul(c.a, c.b[0])
    if op == "mul64": return model_fq_mul64(c.a, c.b[0])
    if op == "mulq": return model_fq_dot([(c.a, c.b[0])], 0)
    if op in FQ_NR:
        row = cases[i & ~3:(i & ~3) + 4]
        return model_fq_dot([(row[r].a, c.b[r]) for r in range(FQ_NR[op])], c.k)
    if op == "canon":
        v, _, ev = model_fq_borrow(c.a)
        return v, ev
    if op == "geq_p":
        _, ge, ev = model_fq_borrow(c.a)
        return (1 if ge else 0), ev
    if op == "add_raw": return model_fq_add_raw(c.a, c.b[0])
    raise KeyError(op)


def fq_events(op):
    return BORROW_EVENTS if op in ("canon", "geq_p") else ADD_EVENTS if op == "add_raw" else SETTLE_EVENTS


# ----------------------------------------------------------------------------------------------- 128 / 64 steps
# divlu (Hacker's Delight): per half (q1, q0) the correction loop runs 0, 1 or 2 times; it leaves early when rhat
# reaches 2^32 ("brk"); "big" = the first estimate is 2^32 or more.
DIVLU_EVENTS = ["q1_dec1", "q1_dec2", "q1_brk", "q1_big", "q0_dec1", "q0_dec2", "q0_brk", "q0_big"]
# div_preinv (Moller & Granlund Alg. 4): the two adjustments
PREINV_EVENTS = ["dec", "inc"]


def model_divlu(u1, u0, v):
    b = 1 << 32
    vn1, vn0 = v >> 32, v & M32
    un1, un0 = u0 >> 32, u0 & M32
    ev = set()

    def half(num, low, tag):
        q = num // vn1
        rhat = num - q * vn1
        n = 0
        if q >= b: ev.add(tag + "_big")
        while q >= b or q * vn0 > b * rhat + low:
            q -= 1
            rhat += vn1
            n += 1
            if rhat >= b:
                ev.add(tag + "_brk")
                break
        assert n <= 2
        if n: ev.add("%s_dec%d" % (tag, n))
        return q

    q1 = half(u1, un1, "q1")
    un21 = (u1 * b + un1 - q1 * v) & M64
    q0 = half(un21, un0, "q0")
    rem = (un21 * b + un0 - q0 * v) & M64
    return (q1 * b + q0) & M64, rem, ev


def model_div_preinv(u1, u0, v):
    vinv = ((1 << 128) - 1) // v - (1 << 64)
    assert 0 <= vinv <= M64
    q = vinv * u1 + u0
    q0 = q & M64
    q1 = ((vinv * u1 >> 64) + u1 + 1 + (1 if (vinv * u1 & M64) + u0 > M64 else 0)) & M64
    r = (u0 - q1 * v) & M64
    ev = set()
    if r > q0:
        q1 = (q1 - 1) & M64
        r = (r + v) & M64
        ev.add("dec")
    if r >= v:
        q1 = (q1 + 1) & M64
        r -= v
        ev.add("inc")
    return q1, r, ev


def div64_cases(seed=SEED):
    """[(u1, u0, v)]: v normalised, u1 < v"""
    rng = random.Random("%d div64" % seed)
    vs = [1 << 63, M64, (1 << 63) + 1, M64 - 1, M64 - M32, (1 << 63) | M32, (1 << 63) + (1 << 32), M64 - M32 + 1,
          (M32 << 32) | 1, (1 << 63) + (1 << 31), 0x8000000100000000, 0xfffffffe00000001, 0x80000000fffffffe]
    vs += [rng.getrandbits(63) | (1 << 63) for _ in range(30)]
    vs += [(rng.getrandbits(31) | (1 << 31)) << 32 | rng.choice([0, 1, M32, M32 - 1]) for _ in range(20)]
    words = [0, 1, 2, M32, 1 << 32, (1 << 32) + 1, 1 << 63, M64 - 1, M64, M64 - M32, (1 << 63) - 1]
    cases = []
    for v in vs:
        u1s = {0, 1, v - 1, v - 2, v >> 1, v >> 32, (v >> 32) << 32, ((v >> 32) << 32) - 1, M32, 1 << 32,
               rng.randrange(v), rng.randrange(v)}
        for u1 in u1s:
            if not 0 <= u1 < v:
                continue
            for u0 in rng.sample(words, 4) + [rng.getrandbits(64)]:
                cases.append((u1, u0, v))
        for _ in range(24):  # q v + r with directed q and r
            q = rng.choice(words + [rng.getrandbits(64)] * 3)
            r = rng.choice([0, 1, v - 1, v - 2, v - 1 - rng.getrandbits(20), rng.randrange(v)]) % v
            u = q * v + r
            cases.append((u >> 64, u & M64, v))
    assert all(u1 < v and v >> 63 for u1, _, v in cases)
    return cases[:MAX_CASES]


# ----------------------------------------------------------------------------------------------- Knuth D
# Events per division (64-bit words): qmax = the "qhat = ~0" branch without the overflow exit, qmax_ovf = with it (rhat
# overflows 2^64, the refinement is skipped), ref1 / ref2 = the refinement loop decrements once / twice, ref_ovf = it
# leaves because rhat overflowed, addback = the multiply-subtract went negative.
#
# Unreachable for some divisors (knuth_reachable below gives the reasons): ref1 / ref2 / ref_ovf for secp256r1's p,
# whose normalised words are ff..ff00000001, 0, 00000000ffffffff, ff..ff: qhat * 0 never exceeds rhat : u, so every
# over-estimate is fixed by add-back alone; qmax_ovf / ref_ovf for the brainpool moduli (vsec < 2^64 - vtop); ref2 for
# every curve modulus but secp256r1's n (it needs vsec > vtop).
KD_EVENTS = ["qmax", "qmax_ovf", "ref1", "ref2", "ref_ovf", "addback"]


def model_knuth_d(a, na, b, nb):
    """Knuth D on 64-bit words as kd_div / mp_divmod / the one-lane division run it: (q, r, events)"""
    assert nb >= 2 and (b >> (64 * (nb - 1))) and a < (1 << (64 * na)) and b < (1 << (64 * nb)) and na >= nb
    s = 64 - (b >> (64 * (nb - 1))).bit_length()
    V, U = b << s, a << s
    vtop, vsec = (V >> (64 * (nb - 1))) & M64, (V >> (64 * (nb - 2))) & M64
    ev = set()
    qv = 0
    W = (1 << (64 * (nb + 1))) - 1
    for j in range(na - nb, -1, -1):
        ut, um, ul = (U >> (64 * (j + nb))) & M64, (U >> (64 * (j + nb - 1))) & M64, (U >> (64 * (j + nb - 2))) & M64
        ovf = False
        if ut >= vtop:
            qhat = M64
            rhat = um + vtop
            ovf = rhat > M64
            rhat &= M64
            ev.add("qmax_ovf" if ovf else "qmax")
        else:
            qhat, rhat = divmod((ut << 64) | um, vtop)
        n = 0
        while not ovf:
            if qhat * vsec > ((rhat << 64) | ul):
                qhat -= 1
                n += 1
                rhat += vtop
                ovf = rhat > M64
                rhat &= M64
                if ovf: ev.add("ref_ovf")
            else:
                break
        assert n <= 2
        if n: ev.add("ref%d" % n)
        win = (U >> (64 * j)) & W
        t = win - qhat * V
        if t < 0:
            ev.add("addback")
            qhat -= 1
            t += V
        assert 0 <= t < V
        U = (U & ~(W << (64 * j))) | (t << (64 * j))
        qv |= qhat << (64 * j)
    return qv, U >> s, ev


Q_WORDS = [0, 1, 2, 1 << 32, (1 << 32) - 1, 1 << 63, (1 << 63) - 1, M64 - 1, M64]


def knuth_reachable(v, nb):
    """The events a divisor's Knuth D can reach at all, from its normalised top words vtop, vsec (b = 2^64):
      qmax      always: a remainder with top word vtop and a small second word is below the divisor.
      qmax_ovf  needs um + vtop >= b with (vtop, um, ..) a remainder below the divisor, so um <= vsec: vsec >= b - vtop.
      ref1      needs qhat * vsec > rhat b + u: never with vsec = 0 (secp256r1's p: every over-estimate is then fixed
                by add-back alone).
      ref_ovf   a decrement followed by rhat + vtop >= b: the decrement at rhat >= b - vtop needs
                qhat * vsec > rhat b, so vsec > b - vtop.
      ref2      a second decrement needs (qhat - 1) * vsec > (rhat + vtop) b with qhat < b: vsec > vtop + 2.
      addback   always."""
    s = 64 - (v >> (64 * (nb - 1))).bit_length()
    vtop, vsec = ((v << s) >> (64 * (nb - 1))) & M64, ((v << s) >> (64 * (nb - 2))) & M64
    ev = {"qmax", "addback"}
    if vsec >= B64 - vtop: ev.add("qmax_ovf")
    if vsec > 0: ev.add("ref1")
    if vsec > B64 - vtop: ev.add("ref_ovf")
    if vsec > vtop + 2: ev.add("ref2")
    return ev


def _windowed_dividend(rng, v, nb, na):
    """A dividend (na > nb words) whose division meets a chosen window at one step: the remainder carried into that
    step has the top words (ut, um) = qhat vtop + rhat for a directed (qhat, rhat), or ut = vtop (the qhat = ~0
    branch), and the third word sits at the refinement test's threshold."""
    s = 64 - (v >> (64 * (nb - 1))).bit_length()
    V = v << s
    vtop, vsec = (V >> (64 * (nb - 1))) & M64, (V >> (64 * (nb - 2))) & M64
    if rng.random() < 0.35:
        ut = vtop
        um = rng.choice([0, 1, vsec, max(vsec - 1, 0), (B64 - vtop) & M64, (B64 - vtop - 1) & M64, rng.randrange(vsec + 1)])
        qhat, rhat = M64, (um + vtop) & M64
    else:
        qhat = rng.choice([M64, M64 - 1, M64 - 2, M64 - rng.getrandbits(20), (vtop + rng.getrandbits(8)) & M64,
                           rng.getrandbits(64) | (1 << 63), rng.getrandbits(64)])
        rhat = rng.choice([0, 1, 2, B64 - vtop - 1, B64 - vtop, B64 - vtop + 1, vtop - 1, rng.getrandbits(31),
                           rng.randrange(vtop)]) % vtop
        ut, um = divmod(qhat * vtop + rhat, B64)
    thr = qhat * vsec - (rhat << 64)
    ul = min(max(thr + rng.choice([-1, 0, 1, -2, 2]), 0), M64) if rng.random() < 0.6 else rng.choice([0, M64, rng.getrandbits(64)])
    t = rng.randrange(1, na - nb + 1)
    low = sum((rng.choice(Q_WORDS) if rng.random() < 0.5 else rng.getrandbits(64)) << (64 * i) for i in range(t))
    rem = (ut << (64 * (nb - 1))) | (um << (64 * (nb - 2)))
    if nb >= 3:
        rem |= (ul << (64 * (nb - 3))) | (rng.getrandbits(64 * (nb - 3)) if nb > 3 else 0)
    else:
        low = (low & ~(M64 << (64 * (t - 1)))) | (ul << (64 * (t - 1)))
    if rem >= V:
        rem = V - 1 - rng.getrandbits(16)
    nqh = na - nb - t
    qh = rng.getrandbits(64 * nqh) if nqh else 0
    low &= ~((1 << s) - 1)
    while True:
        a = (((qh * V + rem) << (64 * t)) | low) >> s
        if a < (1 << (64 * na)):
            return a
        qh >>= 1


def directed_dividends(rng, v, nb, na, n):
    """n dividends below 2^(64 na): q v + r with q words from Q_WORDS or random and r from {0, 1, v-2, v-1, v-1-small,
    random}, and (na > nb) dividends that steer one step's window (_windowed_dividend)"""
    out = []
    lim = 1 << (64 * na)
    nq = na - nb + 1
    while len(out) < n:
        if na > nb and rng.random() < 0.5:
            out.append(_windowed_dividend(rng, v, nb, na))
            continue
        style = rng.random()
        if style < 0.5:
            q = sum(rng.choice(Q_WORDS) << (64 * i) for i in range(nq))
        elif style < 0.8:
            q = sum((rng.choice(Q_WORDS) if rng.random() < 0.5 else rng.getrandbits(64)) << (64 * i) for i in range(nq))
        else:
            q = rng.getrandbits(64 * nq)
        r = rng.choice([0, 1, v - 2, v - 1, v - 1 - rng.getrandbits(rng.choice([8, 40, 64, 70])), rng.randrange(v),
                        v >> 1, (v >> 64) << 64]) % v
        a = q * v + r
        if a >= lim:
            a = (lim - 1 - r) // v * v + r if rng.random() < 0.5 else a % lim
        out.append(a)
    return out


KD_NB = [2, 3, 31, 32, 48, 64]
KD_STRIDE_A, KD_STRIDE_B = 130, 64


def kd_divisors(rng, nb):
    """top limbs {1, 2^63, 2^64 - 1, random}; second limbs that make the refinement likely (large against the top) or
    impossible (0)"""
    out = []
    for top in (1, 1 << 63, M64, rng.getrandbits(64) | 1, rng.randrange(1, 6)):
        for sec in (0, M64, rng.getrandbits(64), 1 << 63):
            low = rng.getrandbits(64 * (nb - 2)) if nb > 2 else 0
            if rng.random() < 0.3 and nb > 2: low = (1 << (64 * (nb - 2))) - 1
            out.append((top << (64 * (nb - 1))) | (sec << (64 * (nb - 2))) | low)
    return out


def kd_cases(seed=SEED):
    """[(a, na, b, nb)] for kd_div: nb in KD_NB, na in {nb, nb+1, 2nb, 2nb+1, 2K = 128 (and 64)}"""
    rng = random.Random("%d kd" % seed)
    cases = []
    for nb in KD_NB:
        nas = sorted({nb, nb + 1, 2 * nb, 2 * nb + 1, 128} | ({64} if nb <= 32 else set()))
        per = 3 if nb >= 31 else 8
        for b in kd_divisors(rng, nb):
            for na in nas:
                if na < nb or na > KD_STRIDE_A - 1:
                    continue
                for a in directed_dividends(rng, b, nb, na, per if na <= 2 * nb + 1 else 1):
                    cases.append((a, na, b, nb))
    return cases[:MAX_CASES]


# curve constants (SEC 2, RFC 5639), as ec_common.hpp EC_CURVE_K holds them; NW 32-bit field words, PWORDS 64-bit
# division words, and the dividend lengths div_signed ((MCN CS + 63) / 64 for MCN = 3N, 3N + 1, 2N + 1: PointOnCurve,
# PointOnTangent, PointOnLine) and divmod_n ((2 N CS + 63) / 64 + 1) pass to mp_divmod, plus na = PWORDS
EC_CURVES = [
    dict(name="secp256r1", nw=8, pwords=4, nl=4, cs=64,
         p=0xffffffff00000001000000000000000000000000ffffffffffffffffffffffff,
         n=0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551),
    dict(name="brainpoolP256r1", nw=8, pwords=4, nl=4, cs=64,
         p=0xa9fb57dba1eea9bc3e660a909d838d726e3bf623d52620282013481d1f6e5377,
         n=0xa9fb57dba1eea9bc3e660a909d838d718c397aa3b561a6f7901e0e82974856a7),
    dict(name="secp224r1", nw=7, pwords=4, nl=7, cs=32,
         p=0xffffffffffffffffffffffffffffffff000000000000000000000001,
         n=0xffffffffffffffffffffffffffff16a2e0b8f03e13dd29455c5c2a3d),
    dict(name="brainpoolP384r1", nw=12, pwords=6, nl=6, cs=64,
         p=0x8cb91e82a3386d280f5d6f7e50e641df152f7109ed5456b412b1da197fb71123acd3a729901d1a71874700133107ec53,
         n=0x8cb91e82a3386d280f5d6f7e50e641df152f7109ed5456b31f166e6cac0425a7cf3ab6af6b7fc3103b883202e9046565),
]


def ec_divmod_nas(cv, mod_n):
    c = EC_CURVES[cv]
    N, cs, pw = c["nl"], c["cs"], c["pwords"]
    if mod_n:
        nas = {(2 * N * cs + 63) // 64 + 1}
    else:
        nas = {max(pw, (m * cs + 63) // 64) for m in (3 * N, 3 * N + 1, 2 * N + 1)}
    nas.add(pw)
    assert max(nas) <= 31
    return sorted(nas)


def ec_divmod_cases(cv, mod_n, seed=SEED):
    """[(a, na)] for mp_divmod<PWORDS> by the curve's p (mod_n = 0) or n (1)"""
    rng = random.Random("%d ecdiv %d %d" % (seed, cv, mod_n))
    c = EC_CURVES[cv]
    v = c["n"] if mod_n else c["p"]
    cases = []
    for na in ec_divmod_nas(cv, mod_n):
        cases += [(a, na) for a in directed_dividends(rng, v, c["pwords"], na, 700)]
        cases += [(a, na) for a in (0, 1, v - 1, v, v + 1, (1 << (64 * na)) - 1, 1 << (64 * na - 1))
                  if a < (1 << (64 * na))]
    return cases[:MAX_CASES]


# ----------------------------------------------------------------------------------------------- EC fields
EC_OPS = ["mul", "add", "sub", "to", "from", "inv"]


def ec_field_expected(m, nw, op, a, b=0):
    Rm = 1 << (32 * nw)
    ri = pow(Rm, -1, m)
    if op == "mul": return a * b * ri % m
    if op == "add": return (a + b) % m
    if op == "sub": return (a - b) % m
    if op == "to": return a * Rm % m
    if op == "from": return a * ri % m
    if op == "inv": return 0 if a == 0 else pow(a * ri % m, -1, m) * Rm % m
    raise KeyError(op)


def ec_field_cases(cv, mod_n, op, seed=SEED):
    """[(a, b)], operands below the modulus"""
    rng = random.Random("%d ecf %d %d %s" % (seed, cv, mod_n, op))
    c = EC_CURVES[cv]
    m, nw = (c["n"] if mod_n else c["p"]), c["nw"]
    Rm = 1 << (32 * nw)
    e = [0, 1, 2, m - 1, m - 2, Rm % m, Rm * Rm % m, (m - 1) // 2, (m + 1) // 2, Rm - m if Rm - m < m else 1]
    for k in range(32, 32 * nw, 32):
        e += [1 << k, (1 << k) - 1]
    for i in range(nw):
        e.append(M32 << (32 * i))
    e = sorted({x % m for x in e})
    if op == "inv":
        return [(a, 0) for a in e[:12] + [rng.randrange(m) for _ in range(52)]]
    singles = e + [rng.randrange(m) for _ in range(400)]
    # results with all-ones / zero words: the top-carry word of m_mul_inl / m_reduce, sums that wrap 2^(32 NW)
    tg = []
    for _ in range(600):
        v = sum((rng.choice([0, 1, M32, M32 - 1]) if rng.random() < 0.8 else rng.getrandbits(32)) << (32 * i)
                for i in range(nw))
        tg.append(v % m)
    if op in ("to", "from"):
        pre = [(v * pow(Rm, -1, m) % m) if op == "to" else (v * Rm % m) for v in tg]
        return [(a, 0) for a in singles + pre]
    cases = [(a, b) for a in e for b in rng.sample(e, 8)] + [(a, rng.choice(singles)) for a in singles]
    for v in tg:
        a = rng.randrange(1, m)
        if op == "mul": cases.append((a, v * Rm * pow(a, -1, m) % m))
        elif op == "add": cases.append((a, (v - a) % m))
        else: cases.append((a, (a - v) % m))
    cases += [(m - 1, m - 1), (m - 1, 1), (0, m - 1), (m - 1, 0)]
    return cases[:MAX_CASES]


# ----------------------------------------------------------------------------------------------- Barrett estimate
B64 = 1 << 64


def model_barrett(n, x, y):
    """k_rsa_core2's estimate for u = x y < b^(2 nb): q3 = floor(floor(u / b^(nb-1)) mu / b^(nb+1)), mu =
    floor(b^(2 nb) / n); returns corr = floor(u / n) - q3 (0, 1 or 2), or None outside the Barrett domain"""
    nb = (n.bit_length() + 63) // 64
    u = x * y
    if nb < 2 or u >= B64 ** (2 * nb):
        return None
    mu = B64 ** (2 * nb) // n
    q3 = ((u >> (64 * (nb - 1))) * mu) >> (64 * (nb + 1))
    corr = u // n - q3
    assert 0 <= corr <= 2
    return corr


BARRETT_TRIES = 60000


def barrett_search(limbs, seed=SEED, tries=BARRETT_TRIES):
    """Seeded search with a fixed try count: {corr: [(modulus, signature)]} for squarings (multiplication 0:
    x = y = signature) at `limbs` significant limbs, top limb of the modulus 1..5, signature near b^limbs."""
    rng = random.Random("%d barrett %d" % (seed, limbs))
    found = {0: [], 1: [], 2: []}
    mods = []
    for _ in range(24):
        n = (rng.randrange(1, 6) << (64 * (limbs - 1))) | rng.getrandbits(64 * (limbs - 1)) | 1
        mods.append((n, B64 ** (2 * limbs) // n))
    top = B64 ** limbs
    for t in range(tries):
        n, mu = mods[t % len(mods)]
        sig = top - 1 - rng.getrandbits(rng.choice([64, 512, 64 * limbs - 8]))
        u = sig * sig
        q3 = ((u >> (64 * (limbs - 1))) * mu) >> (64 * (limbs + 1))
        corr = u // n - q3
        assert 0 <= corr <= 2
        if len(found[corr]) < 16:
            found[corr].append((n, sig))
            if all(len(v) == 16 for v in found.values()):
                break
    return found


def rsa_knuth_addback_row(seed=SEED, K=32):
    """(modulus, signature) with signature >= modulus (multiplication 0 outside the Barrett domain: 31 significant
    limbs, full-width signature) whose Knuth D division of signature^2 reaches add-back; fixed try count."""
    # Add-back needs the three-word estimate to be exact while the divisor's lower words still push the product over:
    # modulus (2^63, 0, ff..ff, ..) and a signature c b^(K-1) + low with c = d 2^32, so that the window of the first
    # nonzero quotient word is (d^2, 0, small) = 2 d^2 * (2^63, 0) exactly and 2 d^2 * (the all-ones words) goes over.
    rng = random.Random("%d rsa addback" % seed)
    nb = K - 1
    n = (1 << (64 * nb - 1)) | ((1 << (64 * (nb - 2))) - 1)
    for _ in range(64):
        d = rng.getrandbits(31) | (1 << 30)
        sig = ((d << 32) << (64 * (K - 1))) | rng.getrandbits(64 * (K - 3) - 2)  # the cross term stays below word 62
        _, _, ev = model_knuth_d(sig * sig, 2 * K, n, nb)
        if "addback" in ev:
            return n, sig
    return None
