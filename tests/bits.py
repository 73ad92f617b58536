"""Bit-level comparisons for the kernel tests, and the range on which the kernels' constant division
(``div_const``, csrc/stencil_math.hpp) is promised to equal true division.

A plain helper module (``from bits import ...``): no fixtures, no pytest hooks.
"""
import math
from fractions import Fraction

import torch

_INT = {torch.float32: torch.int32, torch.float64: torch.int64}
# precision p (bits of the significand, the hidden one included), emin, emax
_FORMAT = {torch.float32: (24, -126, 127), torch.float64: (53, -1022, 1023)}
_I64_MAX = 2 ** 63 - 1


def round_fraction(x: Fraction, p: int, emin: int) -> Fraction:
    """x rounded to the nearest binary number of p significant bits (ties to even; below ``2^emin`` the
    fixed subnormal spacing ``2^(emin - p + 1)``), by integer arithmetic alone. No overflow handling."""
    if x == 0:
        return Fraction(0)
    s, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    q = max(e, emin) - (p - 1)  # the exponent of one unit in the last place
    scaled = a / Fraction(2) ** q
    n, r = divmod(scaled.numerator, scaled.denominator)
    if 2 * r > scaled.denominator or (2 * r == scaled.denominator and n & 1):
        n += 1
    return s * n * Fraction(2) ** q


def _int_view(t: torch.Tensor) -> torch.Tensor:
    if t.dtype not in _INT:
        raise TypeError(f"float32 or float64 expected, not {t.dtype}")
    return t.detach().cpu().contiguous().view(_INT[t.dtype])


def assert_same_bits(got: torch.Tensor, exp: torch.Tensor, what: str = "") -> None:
    """``got`` and ``exp`` hold the same values bit for bit: equal NaN masks (a NaN's payload and sign
    are not compared) and equal integer views everywhere else, so ``-0.0 != +0.0``."""
    assert got.dtype == exp.dtype and tuple(got.shape) == tuple(exp.shape), \
        f"{what}: {got.dtype} {tuple(got.shape)} against {exp.dtype} {tuple(exp.shape)}"
    g, e = got.detach().cpu(), exp.detach().cpu()
    gn, en = torch.isnan(g), torch.isnan(e)
    bad = (gn != en) | (~gn & ~en & (_int_view(g) != _int_view(e)))
    n = int(bad.sum())
    if n:
        idx = torch.nonzero(bad)[:8]
        rows = "; ".join(f"{tuple(i.tolist())}: got {g[tuple(i)].item()!r} ({float(g[tuple(i)]).hex()}), "
                         f"expected {e[tuple(i)].item()!r} ({float(e[tuple(i)]).hex()})" for i in idx)
        raise AssertionError(f"{what + ': ' if what else ''}{n} of {bad.numel()} values differ in their bits "
                             f"({int((gn != en).sum())} in being NaN); first: {rows}")


def _ordered(t: torch.Tensor) -> torch.Tensor:
    """int64 that counts the representable values monotonically: ... -min subnormal -> -1, both zeros -> 0,
    min subnormal -> 1 ... inf."""
    iv = _int_view(t).to(torch.int64)
    if t.dtype == torch.float32:
        mag = iv & 0x7FFFFFFF
    else:
        mag = iv & _I64_MAX
    return torch.where(iv < 0, -mag, mag)


def ulp_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Number of representable values between ``a`` and ``b`` (int64, elementwise): the difference of
    the sign-magnitude integer views, so it counts straight through zero (``-0.0`` and ``+0.0`` are 0
    apart, the two smallest subnormals of opposite sign 2) and through the subnormal range, where a
    step is the fixed spacing. Saturates at 2^63 - 1 (fp64 values of opposite sign far apart). A NaN on
    either side is an error: compare the NaN masks first."""
    if a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"{a.dtype} {tuple(a.shape)} against {b.dtype} {tuple(b.shape)}")
    if bool(torch.isnan(a).any()) or bool(torch.isnan(b).any()):
        raise ValueError("ulp_distance of a NaN")
    x, y = _ordered(a), _ordered(b)
    hi, lo = torch.maximum(x, y), torch.minimum(x, y)
    # hi - lo overflows only for hi > 0 > lo with hi > MAX + lo
    over = (lo < 0) & (hi > _I64_MAX + lo)
    return torch.where(over, torch.full_like(hi, _I64_MAX), hi - torch.where(over, torch.zeros_like(lo), lo))


def spacing(x: torch.Tensor) -> torch.Tensor:
    """The distance from ``|x|`` to the next larger representable value (one unit in the last place of
    x's binade; the fixed subnormal spacing below the smallest normal). x finite."""
    p, emin, _ = _FORMAT[x.dtype]
    e = torch.frexp(x.abs().double())[1] - 1  # |x| in [2^e, 2^(e+1)); frexp(0) has exponent 0
    e = torch.where(x == 0, torch.full_like(e, emin), torch.clamp(e, min=emin))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), (e - (p - 1)).to(torch.int32)).to(x.dtype)


def division_range(dtype, h2: float) -> tuple[float, float]:
    """The interval ``[lo, hi]`` of ``|t|`` on which ``div_const(t, b, y)``, ``b = RN(h2)`` and
    ``y = RN(1 / b)`` in ``dtype``, is promised to be ``RN(t / b)``; ``t = 0`` belongs to it too
    (``+0`` for either zero).

    div_const forms ``q = RN(t y)``, ``r = fma(-q, b, t)`` and ``q' = fma(r, y, q)``. Markstein's theorem
    makes ``q' = RN(t / b)`` provided the residual is exact, ``r = t - q b``, and nothing overflows.

    lo: for ``t`` in the binade ``[2^e, 2^(e+1))`` the exponents of ``q`` and ``b`` add up to ``e - 1`` at
    the least, so ``t - q b`` is a multiple of ``ulp(q) ulp(b) >= 2^(e - 1 - 2 (p - 1)) = 2^(e - 2p + 1)``.
    It is representable (it has at most p bits, that is the theorem) once that step is a multiple of
    the subnormal spacing ``2^(emin - p + 1)``: ``e >= emin + p``. One binade is kept in hand:
    ``lo = 2^(emin + p + 1)`` (fp32 2^-101 = 3.9e-31, fp64 2^-968 = 4.0e-292). This end assumes ``h2`` of
    moderate size (``2^-p < b < 2^p``: the quotient of an in-range numerator is a normal number).

    hi: the first product must stay finite. With ``E = ceil(log2 y)``, ``y <= 2^E``, every
    ``|t| <= 2^(emax - E)`` has ``|t y| <= 2^emax``, a finite number, so ``q`` is finite; then
    ``|q b| ~ |t|`` and ``r``, ``r y`` are small, and ``t / b = t y (1 + eps)`` stays below the largest
    finite value. ``hi = min(2^(emax - E), largest finite)``: for ``h2 = 0.011`` 2^120 (fp32) and 2^1016
    (fp64); for ``h2 >= 2`` the whole finite range. Above it ``t y`` overflows to inf and ``q'`` is
    NaN (``inf - inf``), as it is for ``t = +-inf``."""
    p, emin, emax = _FORMAT[dtype]
    b = torch.tensor(h2, dtype=dtype)
    if not (math.isfinite(b.item()) and b.item() > 0):
        raise ValueError(f"h2 must be positive and finite in {dtype}, not {h2!r}")
    y = (torch.ones((), dtype=dtype) / b).item()
    f, k = math.frexp(y)  # y = f 2^k, 0.5 <= f < 1
    E = k - 1 if f == 0.5 else k
    biggest = torch.finfo(dtype).max
    hi = biggest if emax - E > emax else min(math.ldexp(1.0, emax - E), biggest)
    return math.ldexp(1.0, emin + p + 1), hi


def numerators(u1, box, h2, order: int = 2, mirror=None, buoyancy=None, correlate=None):
    """The three per-axis numerators ``(t_x, t_y, t_z)`` of the oracle's Laplacian of ``u1`` on ``box``
    (what is divided by hx2, hy2, hz2), and the mask of the box nodes at which every numerator is
    zero or inside ``division_range`` of its axis.

    They come from the oracle itself: ``reference._lap_box`` with two of the three ``h^2`` infinite and
    the third 1, so ``((0 + t_x / 1) + t_y / inf) + t_z / inf = t_x`` for finite numerators (up to the sign
    of a zero, which the range does not look at); a non-finite numerator gives NaN on every axis and a
    False in the mask. ``correlate = v``: the numerators of ``reference.face_correlation(u1, v, box)``
    instead."""
    from wave3d.ops import reference

    inf = math.inf
    ts = []
    for axis in range(3):
        hs = [inf, inf, inf]
        hs[axis] = 1.0
        if correlate is not None:
            ts.append(reference.face_correlation(u1, correlate, box, *hs))
        else:
            ts.append(reference._lap_box(u1, tuple(int(v) for v in box), *hs, order, mirror, buoyancy))
    ok = torch.ones(ts[0].shape, dtype=torch.bool)
    for t, h in zip(ts, h2):
        lo, hi = division_range(u1.dtype, h)
        a = t.abs()
        ok &= (a == 0) | ((a >= lo) & (a <= hi))
    return tuple(ts), ok
