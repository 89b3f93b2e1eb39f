"""Groth16's quotient evaluations h restated in Python integers, independent of the library (include/pzkwit.h
pzk_r1cs_quotient_*). For a system with nC constraints and nPub = n_pub_out + n_pub_in public wires:

    M = nC + nPub + 1, N = 2^k the smallest power of two >= M (1 <= k <= 24)
    a_i = A_i.w, b_i = B_i.w (i < nC);  a_{nC + s} = w_s, b_{nC + s} = 0 (s = 0 .. nPub);  0 from M on;  c_i = a_i b_i
    v' = NTT_N(g^i * iNTT_N(v)_i) for v in {a, b, c}, g = w_2N: the evaluations on the coset g * <w_N>
    h_j = a'_j b'_j - c'_j

Systems are read through tests/r1cs_ref.py (constraint lists, witnesses as integers of any 256-bit value)."""
import r1cs_ref as R

P = R.P
ROOT_2_28 = pow(5, (P - 1) >> 28, P)  # 5 is the smallest quadratic non-residue of Fr
MAX_K = 24


def root_of_unity(s):
    """w_{2^s}, s <= 28"""
    assert 0 <= s <= 28
    return pow(ROOT_2_28, 1 << (28 - s), P)


def domain(n_constraints, n_pub):
    """-> (M, k, N); the library takes 1 <= k <= 24 (M = 1 gives k = 0: rejected)"""
    m = n_constraints + n_pub + 1
    k = (m - 1).bit_length()
    return m, k, 1 << k


def bitrev(i, k):
    return int(format(i, "0%db" % k)[::-1], 2) if k else 0


def ntt(v, w):
    """[sum_i v_i w^(i j)]_j for len(v) a power of two and w a primitive len(v)-th root; recursive radix 2"""
    n = len(v)
    if n == 1:
        return list(v)
    w2 = w * w % P
    ev, od = ntt(v[0::2], w2), ntt(v[1::2], w2)
    out, t = [0] * n, 1
    for j in range(n // 2):
        x = t * od[j] % P
        out[j], out[j + n // 2] = (ev[j] + x) % P, (ev[j] - x) % P
        t = t * w % P
    return out


def intt(v, w):
    """coefficients from evaluations, the factor 1 / N included"""
    n_inv = pow(len(v), P - 2, P)
    return [x * n_inv % P for x in ntt(v, pow(w, P - 2, P))]


def dft_direct(v, w):
    """the same as ntt(v, w) by the O(N^2) definition (small N)"""
    n = len(v)
    pw = [pow(w, e, P) for e in range(n)]
    return [sum(v[i] * pw[i * j % n] for i in range(n)) % P for j in range(n)]


def rows(constraints, w, n_pub):
    """-> (a, b, c), each N integers"""
    m, k, n = domain(len(constraints), n_pub)
    assert k <= MAX_K
    a = [R.lc_value(A, w) for A, _, _ in constraints] + [w[s] % P for s in range(n_pub + 1)]
    b = [R.lc_value(B, w) for _, B, _ in constraints] + [0] * (n_pub + 1)
    a += [0] * (n - m)
    b += [0] * (n - m)
    return a, b, [x * y % P for x, y in zip(a, b)]


def coset(v, k, transform=ntt):
    """evaluations on <w_N> -> evaluations on g * <w_N>"""
    w, g = root_of_unity(k), root_of_unity(k + 1)
    coef = intt(v, w) if transform is ntt else [x * pow(len(v), P - 2, P) % P for x in transform(v, pow(w, P - 2, P))]
    t, shifted = 1, []
    for x in coef:
        shifted.append(x * t % P)
        t = t * g % P
    return transform(shifted, w)


def quotient(constraints, w, n_pub, transform=ntt):
    """-> h, N integers"""
    _, k, _ = domain(len(constraints), n_pub)
    a, b, c = (coset(v, k, transform) for v in rows(constraints, w, n_pub))
    return [(x * y - z) % P for x, y, z in zip(a, b, c)]


def h_bytes(h):
    return b"".join(x.to_bytes(32, "little") for x in h)


# ---- the transforms as the device passes leave them (tests/test_gpu_ntt.py)
def forward_bitrev_in(v, k):
    """v holds coefficient i at index bitrev(i) -> the evaluations at w_N^j, natural order"""
    return ntt([v[bitrev(i, k)] for i in range(1 << k)], root_of_unity(k))


def inverse_bitrev_out(v, k, shift):
    """natural-order evaluations -> coefficient i (times g^i when shift) at index bitrev(i)"""
    coef = intt(v, root_of_unity(k))
    g = root_of_unity(k + 1) if shift else 1
    out, t = [0] * (1 << k), 1
    for i, x in enumerate(coef):
        out[bitrev(i, k)] = x * t % P
        t = t * g % P
    return out


# ---- systems with public wires, for the nPub and power-of-two cases
def pub_case(n_constraints, n_pub_out, n_pub_in, seed):
    """(n_wires, constraints, satisfying witness) of short random constraints; the header's public counts are the
    caller's to write (R.write_r1cs(..., n_pub_out=, n_pub_in=))"""
    import random
    rng = random.Random(seed)
    n_wires = max(16, n_pub_out + n_pub_in + 4)
    shapes = [(rng.randrange(4), rng.randrange(4), rng.randrange(1, 4)) for _ in range(n_constraints)]
    return (n_wires,) + R.satisfying_system(rng, n_wires, shapes)
