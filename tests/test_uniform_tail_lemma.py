"""The lemma the uniform-tail mode of the head-row path rests on (csrc/daco_scan_sparse.hip SpRowUT): for float32
t >= 0 and e >= c >= 0, t * e == 0 implies t * c == 0 -- rounding to nearest is monotone, so t * c <= t * e.  A step whose head
has no live mass may therefore draw from tau * c instead of tau * eta: every open head candidate has a zero term either way.
Exercised over denormal and boundary values, where an underflowing product is the only way t * e == 0 with t, e > 0."""
import itertools

import numpy as np

F = np.float32
TINY = np.finfo(F).tiny                 # smallest normal
DEN = F(1.401298464e-45)                # smallest denormal
BOUNDARY = np.array([0.0, DEN, 2 * DEN, 3 * DEN, TINY / 2, np.nextafter(F(TINY), F(0)), TINY, np.nextafter(F(TINY), F(1)),
                     1e-30, 1e-23, np.sqrt(DEN), np.sqrt(TINY), 1e-10, 2.0 ** -75, 2.0 ** -74, 2.0 ** -64, 1e-5, 0.05, 0.5,
                     np.nextafter(F(1), F(0)), 1.0, np.nextafter(F(1), F(2)), 3.0, 1e10, 1e30, np.finfo(F).max], dtype=F)


def test_boundary_values_exhaustively():
    assert BOUNDARY.dtype == F
    hit = 0
    for t, e, c in itertools.product(BOUNDARY, repeat=3):
        if c > e:
            continue
        with np.errstate(under="ignore", over="ignore"):
            pe, pc = F(t) * F(e), F(t) * F(c)
        assert pe.dtype == F and pc <= pe                     # monotone rounding
        if pe == 0:
            assert pc == 0 and not np.signbit(pc), (t, e, c)
            hit += t > 0 and e > 0                             # (an underflow, not a zero factor)
    assert hit > 100                                           # the interesting case occurs


def test_random_denormal_neighbourhood():
    rng = np.random.default_rng(5)
    # exponents around the underflow edge of the product: 2^-149 = 2^a * 2^b for a + b = -149
    a = rng.integers(-149, 1, 200000)
    t = (np.ldexp(1.0 + rng.random(a.size), a)).astype(F)
    e = (np.ldexp(1.0 + rng.random(a.size), -150 - a + rng.integers(-3, 4, a.size))).astype(F)
    c = (e.astype(np.float64) * rng.random(a.size)).astype(F)
    c = np.minimum(c, e)
    with np.errstate(under="ignore"):
        pe, pc = t * e, t * c
    zero = pe == 0
    assert zero.sum() > 1000 and (~zero).sum() > 1000          # both sides of the edge
    assert (pc[zero] == 0).all() and (pc <= pe).all()


def test_the_lemma_needs_c_not_above_e():
    """the set-up's check `head >= c` is not decoration: with c > e the product with c can be positive where t * e is zero"""
    t, e, c = F(2.0 ** -75), F(2.0 ** -75), F(1.0)
    with np.errstate(under="ignore"):
        assert t * e == 0 and t * c > 0
