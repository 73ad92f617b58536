"""The committed tie pairs (tests/relarg_ties.py) re-verified with rational arithmetic, and RelArg
(csrc/device_common.hpp) emulated in rationals on them: with the tie-break on the FMA residuals it
returns the larger quotient in either order; without it (``>`` on the rounded products alone) it keeps
whichever pair came first, which is the smaller quotient in one of the two orders. So the GPU tests
that plant these pairs (tests/test_gpu_sweep_bits.py) fail for a kernel that drops the tie-break.
The emulation also gives the magnitude down to which the tie-break is exact, per type.
"""
from fractions import Fraction

import pytest

from bits import round_fraction
from relarg_ties import FORMATS, LOW, SAFE, pairs, relarg

def exact_bound(p, emin):
    """The least exponent e such that the residual of a product in [2^e, 2^(e+1)) is representable: the
    product of two p-bit numbers is a multiple of 2^(e - 2p + 2) there (e the product's exponent, at
    the least the sum of the factors' exponents), and the subnormal spacing is 2^(emin - p + 1)."""
    return emin + p - 1


@pytest.mark.parametrize("name", ["F64", "F32"])
def test_tie_pairs_are_ties(name):
    p, emin = FORMATS[name]
    rows = pairs(name)
    assert len(rows) >= 64
    for d1, f1, d2, f2 in rows:
        rn = lambda x: round_fraction(x, p, emin)  # noqa: E731
        for v in (d1, f1, d2, f2, f1 + d1, f2 + d2):
            assert v > 0 and rn(v) == v  # representable, u = f + d included
        assert rn(d1 * f2) == rn(d2 * f1)
        assert d1 * f2 != d2 * f1 and rn(d1 / f1) != rn(d2 / f2)
        assert Fraction(1, 8) < d1 / f1 < Fraction(1, 2)


@pytest.mark.parametrize("name", ["F64", "F32"])
def test_relarg_needs_its_tie_break_on_them(name):
    p, emin = FORMATS[name]
    wrong = 0
    for d1, f1, d2, f2 in pairs(name):
        want = max(d1 / f1, d2 / f2)
        for seq in ([(d1, f1), (d2, f2)], [(d2, f2), (d1, f1)]):
            n, d = relarg([(Fraction(0), Fraction(1))] + seq, p, emin)
            assert n / d == want
            n, d = relarg(seq, p, emin, tie_break=False)
            wrong += n / d != want
    assert wrong == len(pairs(name))  # without the tie-break: wrong in exactly one order of every pair


def _wrong(name, k):
    """Orders (of 128) in which RelArg keeps the smaller quotient with the pairs scaled by 2^k."""
    p, emin = FORMATS[name]
    s, wrong = Fraction(2) ** k, 0
    for d1, f1, d2, f2 in pairs(name):
        a, b = (d1 * s, f1 * s), (d2 * s, f2 * s)
        for seq in ([a, b], [b, a]):
            n, d = relarg([(Fraction(0), s)] + seq, p, emin)
            wrong += n / d != max(d1 / f1, d2 / f2)
    return wrong


@pytest.mark.parametrize("name", ["F64", "F32"])
def test_relarg_exact_down_to_the_bound(name):
    """Scaled by a power of two the pairs stay ties. RelArg is exact while every product it forms has an
    exponent of at least ``emin + p - 1`` (fp64 2^-970 = 1e-292, fp32 2^-103 = 1e-31): the residual of a
    product in [2^e, 2^(e+1)) is a multiple of 2^(e - 2p + 2), representable once that is a multiple of
    the subnormal spacing 2^(emin - p + 1). With d >= 2^-5 and f >= 2^-3 unscaled, the scale SAFE = 2^-481
    (fp64; |d|, |f| ~ 1e-146) / 2^-47 (fp32; ~ 1e-15) keeps every product there.

    Below that bound the residuals are rounded, and the comparison of two rounded residuals can tie or
    turn. Measured here on the 128 orders: no wrong answer as long as the products stay normal numbers
    (fp64 down to 2^-507), apart from 1 of 128 in fp32 at 2^-59; with subnormal products most are wrong
    (LOW: fp64 2^-513 62 of 128, fp32 2^-65 62 of 128; all 128 a few binades further down). RelArg's
    comment promises exactness "as long as the products are normal numbers": true of every fp64 pair
    here, not quite of fp32, and guaranteed only from emin + p - 1 on. tests/test_gpu_sweep_bits.py asserts
    equality with the oracle at SAFE and pins the device's answers at LOW to this emulation."""
    p, emin = FORMATS[name]
    assert SAFE[name] == -((-(exact_bound(p, emin) + 8)) // 2)
    assert _wrong(name, SAFE[name]) == 0
    assert _wrong(name, {"F64": -507, "F32": -57}[name]) == 0
    assert _wrong(name, LOW[name]) == 62
    if name == "F32":
        assert _wrong(name, -59) == 1
