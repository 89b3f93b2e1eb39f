"""CPU: the Python definition of the quotient evaluations (tests/quotient_ref.py) against itself: the recursive
transform against the O(N^2) definition, h against -2 H on the coset with H from exact polynomial division, the root
constants, and the domain size around powers of two."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quotient_ref as Q  # noqa: E402
import r1cs_ref as R  # noqa: E402

P = Q.P


def small_systems():
    """(name, constraints, witness, n_pub) with N <= 256"""
    out = []
    for name in ("m1", "m63", "m64", "m65"):
        _, cons, w = R.case(name)
        out.append((name, cons, w, 0))
    for n_con, n_out, n_in in ((5, 0, 0), (3, 1, 0), (10, 2, 3), (122, 0, 5), (123, 1, 4)):
        _, cons, w = Q.pub_case(n_con, n_out, n_in, seed=n_con)
        out.append(("pub%d_%d_%d" % (n_con, n_out, n_in), cons, w, n_out + n_in))
    return out


def test_root_constants():
    assert Q.ROOT_2_28 == 0x2A3C09F0A58A7E8500E0A7EB8EF62ABC402D111E41112ED49BD61B6E725B19F0
    assert pow(Q.ROOT_2_28, 1 << 27, P) == P - 1
    assert (P - 1) % (1 << 28) == 0 and (P - 1) % (1 << 29) != 0
    # 5 is the smallest quadratic non-residue
    assert [x for x in range(2, 6) if pow(x, (P - 1) // 2, P) == P - 1] == [5]
    for s in (1, 2, 10, 22, 24, 25):
        w = Q.root_of_unity(s)
        assert pow(w, 1 << s, P) == 1 and pow(w, 1 << (s - 1), P) == P - 1
    assert Q.root_of_unity(23) ** 2 % P == Q.root_of_unity(22)


@pytest.mark.parametrize("m,k", [(1, 0), (2, 1), (3, 2), (4, 2), (5, 3), (255, 8), (256, 8), (257, 9), (1 << 22, 22),
                                 ((1 << 22) + 1, 23), (1 << 24, 24)])
def test_domain_size(m, k):
    """M exactly a power of two, one below and one above (M = nC + nPub + 1 >= 1; M = 1 is k = 0, which the library rejects)"""
    for n_pub in (0, 1, 5):
        if m - n_pub - 1 >= 0:
            assert Q.domain(m - n_pub - 1, n_pub) == (m, k, 1 << k)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
def test_recursive_transform_is_the_definition(k):
    rng = random.Random(k)
    v = [rng.randrange(P) for _ in range(1 << k)]
    w = Q.root_of_unity(k)
    assert Q.ntt(v, w) == Q.dft_direct(v, w)
    assert Q.intt(Q.ntt(v, w), w) == v
    assert Q.forward_bitrev_in([v[Q.bitrev(i, k)] for i in range(1 << k)], k) == Q.dft_direct(v, w)
    for shift in (False, True):
        g = Q.root_of_unity(k + 1) if shift else 1
        got = Q.inverse_bitrev_out(Q.dft_direct(v, w), k, shift)
        assert [got[Q.bitrev(i, k)] for i in range(1 << k)] == [x * pow(g, i, P) % P for i, x in enumerate(v)]


def poly_mul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % P
    return out


@pytest.mark.parametrize("name,cons,w,n_pub", small_systems(), ids=[s[0] for s in small_systems()])
def test_h_is_minus_two_h_on_the_coset(name, cons, w, n_pub):
    """A B - C vanishes on the domain, so it is H (X^N - 1) exactly; on the coset X^N - 1 = g^N - 1 = -2"""
    m, k, n = Q.domain(len(cons), n_pub)
    assert n <= 256
    assert R.evaluate(cons, w) == (-1, 0)
    wn, g = Q.root_of_unity(k), Q.root_of_unity(k + 1)
    a, b, c = (Q.intt(v, wn) for v in Q.rows(cons, w, n_pub))
    t = poly_mul(a, b)
    t = [(x - (c[i] if i < n else 0)) % P for i, x in enumerate(t)] + [0]
    # division by X^N - 1: t = H X^N - H, H of degree < N - 1
    hi, lo = t[n:2 * n], t[:n]
    assert [(x + y) % P for x, y in zip(hi, lo)] == [0] * n  # the remainder is zero
    assert pow(g, n, P) == P - 1
    want = [(-2 * sum(hc * pow(g * pow(wn, j, P) % P, i, P) for i, hc in enumerate(hi))) % P for j in range(n)]
    h = Q.quotient(cons, w, n_pub)
    assert h == want
    assert Q.quotient(cons, w, n_pub, transform=Q.dft_direct) == h


def test_h_is_defined_on_a_violating_row():
    _, cons, w = R.case("m63")
    bad = R.perturbed(random.Random(3), w, 3)
    assert R.evaluate(cons, bad)[0] >= 0
    h = Q.quotient(cons, bad, 0)
    assert len(h) == 64 and h != Q.quotient(cons, w, 0)
