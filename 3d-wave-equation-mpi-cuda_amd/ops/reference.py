"""Plain-PyTorch reference implementations (the oracle for the HIP kernels).

Every operation is a separate, individually rounded elementwise op in the reference's
order, so in fp64 on the CPU the results are bitwise those of mpi_new (no contraction).
"""
from __future__ import annotations

import math

import torch


def laplace7(u: torch.Tensor, hx2, hy2, hz2) -> torch.Tensor:
    """7-point Laplacian on all interior nodes u[1:-1,1:-1,1:-1] (mpi_new.cpp:104-111)."""
    c = u[1:-1, 1:-1, 1:-1]
    two_c = 2 * c
    ans = torch.zeros_like(c)
    ans = ans + (u[:-2, 1:-1, 1:-1] - two_c + u[2:, 1:-1, 1:-1]) / hx2
    ans = ans + (u[1:-1, :-2, 1:-1] - two_c + u[1:-1, 2:, 1:-1]) / hy2
    ans = ans + (u[1:-1, 1:-1, :-2] - two_c + u[1:-1, 1:-1, 2:]) / hz2
    return ans


def step(u1, u2, box, *, first: bool, hx2, hy2, hz2, coef) -> torch.Tensor:
    """Layer update on ``box`` (local inclusive indices); returns the updated box values."""
    i0, i1, j0, j1, k0, k1 = box
    lap = laplace7(u1, hx2, hy2, hz2)[i0 - 1:i1, j0 - 1:j1, k0 - 1:k1]
    c = u1[i0:i1 + 1, j0:j1 + 1, k0:k1 + 1]
    if first:
        return c + coef * lap
    return (2 * c - u2[i0:i1 + 1, j0:j1 + 1, k0:k1 + 1]) + coef * lap


def analytic(tx, ty, tz, ct) -> torch.Tensor:
    """f = ((sx*sy)*sz)*ct on the tensor product of the 1-D tables."""
    return ((tx[:, None, None] * ty[None, :, None]) * tz[None, None, :]) * ct


def max_errors(u: torch.Tensor, f: torch.Tensor, init: float = -100.0) -> tuple[float, float]:
    """max |u-f| and max |u-f|/|f| with the reference's NaN-ignoring `if (e > m)` rule."""
    d = (u - f).abs()
    r = d / f.abs()
    neg = torch.tensor(-math.inf, dtype=u.dtype, device=u.device)
    a = torch.where(torch.isnan(d), neg, d).max().item() if d.numel() else -math.inf
    b = torch.where(torch.isnan(r), neg, r).max().item() if r.numel() else -math.inf
    return max(a, init), max(b, init)


def tables(N: int, K: int, L=("pi", "pi", "pi"), T: float = 1.0, pi: str = "ref",
           phase: float = 0.0, dtype=torch.float64):
    """1-D analytic tables, evaluated with the reference's expressions (mpi_new.cpp:151)."""
    PI = 3.1415926535 if pi == "ref" else math.pi
    Lx, Ly, Lz = (PI if v == "pi" else float(v) for v in L)
    a_t = 0.5 * math.sqrt(4 / (Lx * Lx) + 1 / (Ly * Ly) + 1 / (Lz * Lz))
    tau = T / K
    hx, hy, hz = Lx / N, Ly / N, Lz / N
    if phase == 0.0:
        sx = [math.sin(2 * PI * (hx * g) / Lx) for g in range(N + 1)]
    else:
        sx = [math.sin(2 * PI * (hx * g) / Lx + phase) for g in range(N + 1)]
    sy = [math.sin(PI * (hy * g) / Ly) for g in range(N + 1)]
    sz = [math.sin(PI * (hz * g) / Lz) for g in range(N + 1)]
    ct = [math.cos(a_t * (tau * n) + 2 * PI) for n in range(K + 1)]
    a2 = 1 / (4 * PI * PI)
    consts = dict(a2=a2, a_t=a_t, tau=tau, hx=hx, hy=hy, hz=hz, hx2=hx * hx, hy2=hy * hy,
                  hz2=hz * hz, coef=a2 * tau * tau, coef_first=a2 * tau * tau * 0.5)
    t = lambda v: torch.tensor(v, dtype=dtype)  # noqa: E731
    return t(sx), t(sy), t(sz), ct, consts


def solve(N: int, K: int, L=("pi", "pi", "pi"), T: float = 1.0, pi: str = "ref",
          phase: float = 0.0, dtype=torch.float64, device="cpu", scheme: str = "leapfrog", math: str = "exact"):
    """Whole single-domain solve in PyTorch; returns (max_abs[0..K], max_rel[0..K], u_K).
    math "fma": the FMA form (``solve_fma``; CPU only), bit for bit the ``cpu`` backend's ``math="fma"``.

    Storage: x has ghost planes (local = global + 1), y/z none (faces are Dirichlet).
    scheme "delta": increment form, d^n = d^{n-1} + coef*lap u^{n-1}, u^n = u^{n-1} + d^n.
    """
    if math == "fma":
        if str(device) != "cpu":
            raise ValueError("the FMA-form oracle runs on the CPU")
        return solve_fma(N, K, L, T, pi, phase, dtype, scheme)
    if math != "exact":
        raise ValueError(f"math must be 'exact' or 'fma', not {math!r}")
    sx, sy, sz, ct, c = tables(N, K, L, T, pi, phase, dtype)
    sx, sy, sz = sx.to(device), sy.to(device), sz.to(device)
    g = [torch.zeros(N + 3, N + 1, N + 1, dtype=dtype, device=device) for _ in range(3)]

    def wrap(u):
        u[0] = u[N]       # ghost x=-1  <- global N-1
        u[N + 2] = u[2]   # ghost x=N+1 <- global 1

    f0 = analytic(sx, sy, sz, ct[0])
    g[0][1:N + 2] = f0
    wrap(g[0])
    ma, mr = max_errors(f0, f0)
    abs_e, rel_e = [ma], [mr]
    d = None
    for n in range(1, K + 1):
        u1, u2, u = g[(n + 2) % 3], g[(n + 1) % 3], g[n % 3]
        u.zero_()
        # stencil points: all x (incl. the periodic planes), y/z global 1..N-1
        box = (1, N + 1, 1, N - 1, 1, N - 1)
        coef = c["coef_first"] if n == 1 else c["coef"]
        if scheme == "delta":
            lap = laplace7(u1, c["hx2"], c["hy2"], c["hz2"])[0:N + 1, 0:N - 1, 0:N - 1]
            d = coef * lap if n == 1 else d + coef * lap
            vals = u1[1:N + 2, 1:N, 1:N] + d
        else:
            vals = step(u1, u2, box, first=n == 1, hx2=c["hx2"], hy2=c["hy2"], hz2=c["hz2"],
                        coef=coef)
        u[1:N + 2, 1:N, 1:N] = vals
        wrap(u)
        f = analytic(sx[1:N], sy[1:N], sz[1:N], ct[n])
        ma, mr = max_errors(u[2:N + 1, 1:N, 1:N], f)
        abs_e.append(ma)
        rel_e.append(mr)
    return abs_e, rel_e, g[K % 3]


def stencil_field(u1, u2, *, first: bool, hx2, hy2, hz2, coef) -> torch.Tensor:
    """One layer on every node with a full 7-point neighbourhood: values for u1[1:-1, 1:-1, 1:-1]
    (u2 unused when ``first``). The temporal-blocking oracle chains this per layer."""
    lap = laplace7(u1, hx2, hy2, hz2)
    c = u1[1:-1, 1:-1, 1:-1]
    if first:
        return c + coef * lap
    return (2 * c - u2[1:-1, 1:-1, 1:-1]) + coef * lap


def chained_delta(A, Dm1, *, first: bool, mask, hx2, hy2, hz2, coefs):
    """Two-layer increment-form oracle (the first two layers of a k_tb3 / k_tbn delta sweep): d^m = d^{m-1} + c0*lap A (c0*lap A when
    ``first``), C = A + d^m, d^{m+1} = d^m + c1*lap C, D = C + d^{m+1}; C and d are 0 where
    ``mask`` is False. Returns (C, D, d^{m+1}) on the full grid."""
    zero = torch.zeros((), dtype=A.dtype)
    inner = (slice(1, -1),) * 3

    def lap_of(u):
        v = torch.zeros_like(u)
        v[inner] = laplace7(u, hx2, hy2, hz2)
        return v
    m = mask.clone()
    m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = (False,) * 6
    la = lap_of(A)
    dm = coefs[0] * la if first else Dm1 + coefs[0] * la
    dm = torch.where(m, dm, zero)
    Cf = torch.where(m, A + dm, zero)
    dn = dm + coefs[1] * lap_of(Cf)
    return Cf, Cf + dn, dn


def chained_delta_layers(A, Dm1, nlayers: int, *, first: bool, mask, hx2, hy2, hz2, coefs):
    """Increment-form deep-sweep oracle (k_tbn DELTA): d_l = d_{l-1} + c_l lap U_{l-1} (layer 0 of
    the first sweep: c_0 lap A alone), U_l = U_{l-1} + d_l with U_{-1} = A, d_{-1} = Dm1; U and d are
    0 where ``mask`` is False and on the outermost ring. Returns ([U_0 .. U_{n-1}], d_{n-1})."""
    zero = torch.zeros((), dtype=A.dtype)
    inner = (slice(1, -1),) * 3
    m = mask.clone()
    m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = (False,) * 6
    out, u, d = [], A, Dm1
    for q in range(nlayers):
        la = torch.zeros_like(u)
        la[inner] = laplace7(u, hx2, hy2, hz2)
        d = coefs[q] * la if (first and q == 0) else d + coefs[q] * la
        d = torch.where(m, d, zero)
        u = torch.where(m, u + d, zero)
        out.append(u)
    return out, d


def chained_layers(A, B, nlayers: int, *, first: bool, mask, hx2, hy2, hz2, coefs):
    """Layers m, m+1, ... of a temporal-blocking sweep on full grids: C from (A, B), D from
    (C, A), E from (D, C); each layer is 0 where ``mask`` is False (Dirichlet faces) and on the
    outermost node ring of the grid (no stencil there)."""
    out, prev2, prev1 = [], B, A
    zero = torch.zeros((), dtype=A.dtype)
    for q in range(nlayers):
        v = torch.zeros_like(A)
        val = stencil_field(prev1, prev2, first=first and q == 0, hx2=hx2, hy2=hy2, hz2=hz2,
                            coef=coefs[q])
        v[1:-1, 1:-1, 1:-1] = torch.where(mask[1:-1, 1:-1, 1:-1], val, zero)
        out.append(v)
        prev2, prev1 = prev1, v
    return out


# ---- the --math fma form (csrc/stencil_math.hpp, FMA section), bit for bit ------------------------
#
# The FMA form is a fixed sequence of individually rounded operations, some of them fused
# multiply-adds. PyTorch has no elementwise fma, so ``fma`` below builds the correctly rounded result
# from error-free transformations; everything else is written out from stencil_math.hpp's comments
# (second_diff, coef_lap_fma, fm_kc, leap_fm, leap_fm_masked) and from the launchers' coefficient
# rule. Nothing here calls the native module. ``variant`` swaps in a subtly different arithmetic, for
# the sensitivity tests alone: "unfused" (every fma as a rounded product and a rounded add), "swap"
# (the fp32 composition on fp64 data and the reverse), "fold2c" (the chain with 2c folded into kc
# that stencil_math.hpp records as rejected).

FMA_VARIANTS = (None, "unfused", "swap", "fold2c")


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _odd_sum(a, b):
    """a + b rounded to odd (float64): the rounded sum, moved one step towards the exact sum where
    the sum is inexact and its last bit is even."""
    s, e = _two_sum(a, b)
    iv = s.contiguous().view(torch.int64)
    step = torch.where((e > 0) == (s > 0), torch.ones_like(iv), -torch.ones_like(iv))
    fix = (e != 0) & ((iv & 1) == 0)
    return torch.where(fix, iv + step, iv).view(torch.float64)


def _split(a):
    t = a * 134217729.0  # 2^27 + 1 (Veltkamp)
    hi = t - (t - a)
    return hi, a - hi


def fma(a, b, c) -> torch.Tensor:
    """``RN(a b + c)`` with one rounding, elementwise, for float64 or float32 tensors (broadcast like
    ``a * b + c``; Python scalars are taken in the tensors' type).

    float64: TwoProduct (Veltkamp split) gives ``a b = ph + pl`` exactly, TwoSum ``c + ph = sh + sl``
    exactly, and ``RN(sh + RO(sl + pl))`` with RO the sum rounded to odd is the correctly rounded result
    (Boldo and Melquiond). float32: the product is exact in float64 (48 bits), ``RO(ab + c)`` in float64
    keeps 53 >= 2 * 24 + 2 bits, and its cast to float32 is the correctly rounded result.

    Range: correctly rounded as long as the product neither overflows nor loses bits to underflow
    and, in float64, the split does not overflow: float64 ``|a|, |b| < 2^996`` and either ``a b = 0`` or
    ``2^-968 <= |a b| < 2^1023``; float32 whenever ``a b`` and ``c`` are normal float64 numbers or zero (every
    float32 input) and the result does not overflow. Where an operand or the plain ``a * b + c`` is not
    finite, and where a factor is zero (the product is then exact), the result is ``a * b + c``: infinities,
    NaNs and the signs of zeros as the hardware instruction gives them."""
    ts = [t for t in (a, b, c) if isinstance(t, torch.Tensor)]
    if not ts or any(t.dtype != ts[0].dtype for t in ts) or ts[0].dtype not in (torch.float32, torch.float64):
        raise TypeError("fma: float32 or float64 tensors of one type")
    dt = ts[0].dtype
    a, b, c = (t if isinstance(t, torch.Tensor) else torch.tensor(t, dtype=dt, device=ts[0].device) for t in (a, b, c))
    a, b, c = torch.broadcast_tensors(a, b, c)
    plain = a * b + c
    if dt == torch.float32:
        soft = _odd_sum(a.double() * b.double(), c.double()).to(torch.float32)
    else:
        ph = a * b
        ah, al = _split(a)
        bh, bl = _split(b)
        pl = ((ah * bh - ph) + ah * bl + al * bh) + al * bl
        sh, sl = _two_sum(c, ph)
        soft = sh + _odd_sum(sl, pl)
    ok = torch.isfinite(a) & torch.isfinite(b) & torch.isfinite(c) & torch.isfinite(plain) & (a != 0) & (b != 0)
    return torch.where(ok, soft, plain)


def _fma_v(a, b, c, variant):
    return a * b + c if variant == "unfused" else fma(a, b, c)


def fma_coefs(coef, hx2, hy2, hz2, dtype) -> tuple:
    """(cx, cy, cz, kc) as the launchers form them: ``c_d = T(coef / h_d^2)``, the quotient in double and
    then cast, and ``kc = fm_kc(cx, cy, cz) = -2 ((cx + cy) + cz)`` from the cast values, in T."""
    cx, cy, cz = (torch.tensor(float(coef) / float(h), dtype=torch.float64).to(dtype) for h in (hx2, hy2, hz2))
    return cx, cy, cz, -2 * ((cx + cy) + cz)


def _nbrs(u):
    i = slice(1, -1)
    return (u[i, i, i], u[:-2, i, i], u[2:, i, i], u[i, :-2, i], u[i, 2:, i], u[i, i, :-2], u[i, i, 2:])


def _second_diff(m, c, p, f32: bool):
    """second_diff: fp64 ``fma(-2, c, m + p)`` (2c is exact, so one rounded sum and one rounded
    difference); fp32 ``(m - c) + (p - c)``."""
    return (m - c) + (p - c) if f32 else (m + p) - 2 * c


def coef_lap_fma_field(u, fc, variant=None) -> torch.Tensor:
    """coef_lap_fma on ``u[1:-1, 1:-1, 1:-1]``: ``fma(cx, sx, fma(cy, sy, cz sz))`` with the second
    differences of the grid's type. ``fc`` = ``fma_coefs``."""
    c, xm, xp, ym, yp, zm, zp = _nbrs(u)
    f32 = (u.dtype == torch.float32) != (variant == "swap")
    sx, sy, sz = _second_diff(xm, c, xp, f32), _second_diff(ym, c, yp, f32), _second_diff(zm, c, zp, f32)
    return _fma_v(fc[0], sx, _fma_v(fc[1], sy, fc[2] * sz, variant), variant)


def taylor_fma_field(u1, fc, variant=None) -> torch.Tensor:
    """The Taylor start in FMA form: ``c + coef_lap_fma`` (fc from ``coef_first``)."""
    return u1[1:-1, 1:-1, 1:-1] + coef_lap_fma_field(u1, fc, variant)


def leap_fma_field(u1, u2, fc, m=None, variant=None) -> torch.Tensor:
    """leap_fm on ``u1[1:-1, 1:-1, 1:-1]``. fp64: ``t = cz (zm + zp)``, ``t = fma(cy, ym + yp, t)``,
    ``t = fma(cx, xm + xp, t)``, ``t = fma(kc, c, t)``, result ``(2c - u2) + t``; fp32: ``(2c - u2) +
    coef_lap_fma``. ``2c - u2`` is ``fma(2, c, -u2)``: 2c is exact, so the difference carries the one
    rounding. ``m`` (a 0/1 grid like the result): leap_fm_masked, ``fma(t, m, 2c - u2)``."""
    c, xm, xp, ym, yp, zm, zp = _nbrs(u1)
    cx, cy, cz, kc = fc
    base = 2 * c - u2[1:-1, 1:-1, 1:-1]
    chain = (u1.dtype == torch.float64) != (variant == "swap")
    if variant == "fold2c":  # the rejected single chain: kc' = kc + 2, no separate 2c - u2
        t = cz * (zm + zp)
        t = fma(cy, ym + yp, t)
        t = fma(cx, xm + xp, t)
        t = fma(kc + 2, c, t)
        return t - u2[1:-1, 1:-1, 1:-1] if m is None else fma(t, m, -u2[1:-1, 1:-1, 1:-1])
    if chain:
        t = cz * (zm + zp)
        t = _fma_v(cy, ym + yp, t, variant)
        t = _fma_v(cx, xm + xp, t, variant)
        t = _fma_v(kc, c, t, variant)
    else:
        t = coef_lap_fma_field(u1, (cx, cy, cz), variant)
    return base + t if m is None else _fma_v(t, m, base, variant)


def _cmask(mask, dtype):
    """The kernels' 0/1 factor of the computed-domain mask on the interior nodes."""
    m = mask.clone()
    m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = (False,) * 6
    return m[1:-1, 1:-1, 1:-1].to(dtype)


def chained_layers_fma(A, B, nlayers: int, *, first: bool, mask, hx2, hy2, hz2, coefs, variant=None):
    """``chained_layers`` in FMA form, as k_tbn / k_tb3 ``fma=True`` compute it. ``coefs[0]`` is the Taylor
    start's coefficient when ``first``; every other layer uses ``coefs[1]`` (the sweeps keep one triple for
    the non-first layers). The mask is a product, as in the kernels (``upd`` in hip_tbn.hip): layers 0 and
    1 multiply the result by m, later layers carry m inside the last fma (leap_fm_masked), so a
    non-finite value on a masked node gives NaN there, not 0. h^2 and coefs are taken as doubles."""
    dt = A.dtype
    m = _cmask(mask, dt)
    f0 = fma_coefs(coefs[0], hx2, hy2, hz2, dt)
    f1 = fma_coefs(coefs[1], hx2, hy2, hz2, dt)
    out, prev2, prev1 = [], B, A
    for q in range(nlayers):
        v = torch.zeros_like(A)
        if first and q == 0:
            val = taylor_fma_field(prev1, f0, variant) * m
        elif q <= 1:
            val = leap_fma_field(prev1, prev2, f1, None, variant) * m
        else:
            val = leap_fma_field(prev1, prev2, f1, m, variant)
        v[1:-1, 1:-1, 1:-1] = val
        out.append(v)
        prev2, prev1 = prev1, v
    return out


def chained_delta_layers_fma(A, Dm1, nlayers: int, *, first: bool, mask, hx2, hy2, hz2, coefs, variant=None):
    """``chained_delta_layers`` in FMA form (k_tbn ``delta=True, fma=True``): ``d_l = d_{l-1} + coef_lap_fma
    (U_{l-1})`` (layer 0 of the first sweep: coef_lap_fma alone, from ``coefs[0]``), then ``d_l = d_l m`` and
    ``U_l = (U_{l-1} + d_l) m``. Returns ([U_0 .. U_{n-1}], d_{n-1})."""
    dt = A.dtype
    m = _cmask(mask, dt)
    f0 = fma_coefs(coefs[0], hx2, hy2, hz2, dt)
    f1 = fma_coefs(coefs[1], hx2, hy2, hz2, dt)
    inner = (slice(1, -1),) * 3
    out, u, d = [], A, Dm1
    for q in range(nlayers):
        t = first and q == 0
        l_ = coef_lap_fma_field(u, f0 if t else f1, variant)
        dn = torch.zeros_like(A)
        dn[inner] = (l_ if t else d[inner] + l_) * m
        un = torch.zeros_like(A)
        un[inner] = (u[inner] + dn[inner]) * m
        out.append(un)
        u, d = un, dn
    return out, d


def div_const(a: torch.Tensor, h2: float) -> torch.Tensor:
    """The kernels' division by a constant (csrc/stencil_math.hpp div_const), operation for operation:
    ``b = T(h2)``, ``y = RN(1 / b)``, ``q = a y``, ``r = fma(-q, b, a)``, ``q' = fma(r, y, q)``. Equal to ``a / b`` on
    ``tests/bits.py division_range``; an infinite numerator gives NaN (true division: the infinity) and
    ``-0`` gives ``+0``, which is why the oracle of non-finite fields divides like the kernels."""
    b = torch.tensor(h2, dtype=a.dtype)
    y = torch.ones((), dtype=a.dtype) / b
    q = a * y
    return fma(fma(-q, b, a), y, q)


def laplace7_cr(u: torch.Tensor, hx2, hy2, hz2) -> torch.Tensor:
    """``laplace7`` with ``div_const`` in place of the three divisions (laplace7_cr in stencil_math.hpp)."""
    c = u[1:-1, 1:-1, 1:-1]
    two_c = 2 * c
    ans = torch.zeros_like(c)
    ans = ans + div_const(u[:-2, 1:-1, 1:-1] - two_c + u[2:, 1:-1, 1:-1], hx2)
    ans = ans + div_const(u[1:-1, :-2, 1:-1] - two_c + u[1:-1, 2:, 1:-1], hy2)
    ans = ans + div_const(u[1:-1, 1:-1, :-2] - two_c + u[1:-1, 1:-1, 2:], hz2)
    return ans


def chained_layers_kernel(A, B, nlayers: int, *, first: bool, mask, hx2, hy2, hz2, coefs):
    """``chained_layers`` (exact form) with the two things k_tbn does differently on fields that are not
    finite or not in range: the constant division (``laplace7_cr``) and the mask as a product, ``upd`` in
    csrc/hip_tbn.hip: layers 0 and 1 ``value m``, later layers ``(2c - u2) + (coef m) lap``. So ``0 * NaN`` is
    NaN on a masked node, and an infinite numerator gives NaN, as on the device. On finite in-range
    fields it equals ``chained_layers`` up to the sign of a masked zero."""
    dt = A.dtype
    m = _cmask(mask, dt)
    out, prev2, prev1 = [], B, A
    inner = (slice(1, -1),) * 3
    for q in range(nlayers):
        lap = laplace7_cr(prev1, hx2, hy2, hz2)
        c = prev1[inner]
        coef = torch.tensor(coefs[q], dtype=dt)
        if first and q == 0:
            val = (c + coef * lap) * m
        elif q <= 1:
            val = ((2 * c - prev2[inner]) + coef * lap) * m
        else:
            val = (2 * c - prev2[inner]) + (coef * m) * lap
        v = torch.zeros_like(A)
        v[inner] = val
        out.append(v)
        prev2, prev1 = prev1, v
    return out


def rel_key_fma(d: torch.Tensor, tx, ty, tz, ct: float, init: float = -100.0) -> float:
    """The --math fma relative-error key (RelMax in csrc/device_common.hpp), operation for operation:
    ``w = (1 / |sx sy|) (1 / |sz|)`` from the reciprocal tables (each a correctly rounded quotient of 1),
    the NaN-ignoring maximum of ``|d w|``, then times ``T(1 / |ct|)`` (the quotient in double, cast). ``d`` =
    ``u - f`` on the error nodes, tx / ty / tz their table slices; the initial value comes back untouched."""
    dt = d.dtype
    one = torch.ones((), dtype=dt)
    w = (one / (tx[:, None, None] * ty[None, :, None]).abs()) * (one / tz.abs())[None, None, :]
    p = (d * w).abs()
    neg = torch.tensor(-math.inf, dtype=dt)
    mx = torch.where(torch.isnan(p), neg, p).max() if p.numel() else neg
    if not bool(mx > init):
        return float(init)
    return (mx * torch.tensor(1.0 / abs(float(ct)), dtype=torch.float64).to(dt)).item()


def solve_fma(N: int, K: int, L=("pi", "pi", "pi"), T: float = 1.0, pi: str = "ref", phase: float = 0.0,
              dtype=torch.float64, scheme: str = "leapfrog", variant=None):
    """``solve`` in FMA form (the ``cpu`` backend's ``math="fma"``): the Taylor start ``c + coef_lap_fma`` with
    the coefficients of ``coef_first``, then leap_fm; scheme "delta": ``d = d + coef_lap_fma``, ``u = c + d``."""
    sx, sy, sz, ct, c = tables(N, K, L, T, pi, phase, dtype)
    g = [torch.zeros(N + 3, N + 1, N + 1, dtype=dtype) for _ in range(3)]

    def wrap(u):
        u[0] = u[N]
        u[N + 2] = u[2]

    f0 = analytic(sx, sy, sz, ct[0])
    g[0][1:N + 2] = f0
    wrap(g[0])
    ma, mr = max_errors(f0, f0)
    abs_e, rel_e = [ma], [mr]
    fc1 = fma_coefs(c["coef_first"], c["hx2"], c["hy2"], c["hz2"], dtype)
    fcn = fma_coefs(c["coef"], c["hx2"], c["hy2"], c["hz2"], dtype)
    d = None
    box = (slice(0, N + 1), slice(0, N - 1), slice(0, N - 1))  # interior index of x all, y/z 1..N-1
    for n in range(1, K + 1):
        u1, u2, u = g[(n + 2) % 3], g[(n + 1) % 3], g[n % 3]
        u.zero_()
        if scheme == "delta":
            l_ = coef_lap_fma_field(u1, fc1 if n == 1 else fcn, variant)[box]
            d = l_ if n == 1 else d + l_
            vals = u1[1:N + 2, 1:N, 1:N] + d
        elif n == 1:
            vals = taylor_fma_field(u1, fc1, variant)[box]
        else:
            vals = leap_fma_field(u1, u2, fcn, None, variant)[box]
        u[1:N + 2, 1:N, 1:N] = vals
        wrap(u)
        f = analytic(sx[1:N], sy[1:N], sz[1:N], torch.tensor(ct[n], dtype=dtype).item())
        ma, mr = max_errors(u[2:N + 1, 1:N, 1:N], f)
        abs_e.append(ma)
        rel_e.append(mr)
    return abs_e, rel_e, g[K % 3]


# ---- heterogeneous medium: u_tt = c^2 (lap u + f) -----------------------------------------

STAR_WEIGHTS = {
    2: ((-2, 1), (1, 1)),
    4: ((-5, 2), (4, 3), (-1, 12)),
    8: ((-205, 72), (8, 5), (-1, 5), (8, 315), (-1, 560)),
}


def star_weights(order: int) -> list[float]:
    """Central second-derivative weights c_0 .. c_M of the star stencil of ``order`` (2, 4, 8;
    M = order / 2): each the Python float quotient of its two integers."""
    if order not in STAR_WEIGHTS:
        raise ValueError(f"space order must be 2, 4 or 8, not {order!r}")
    return [a / b for a, b in STAR_WEIGHTS[order]]


def cfl_limit(order: int = 2) -> float:
    """Largest stable Courant number ``c tau / h_min`` of the leapfrog with the star Laplacian of
    ``order``: ``2 / sqrt(3 S)``, ``S = |c_0| + 2 sum |c_d|`` (order 2: 1/sqrt(3), 4: 0.5, 8: 0.4528...)."""
    w = star_weights(order)
    if order == 2:
        return 1.0 / math.sqrt(3.0)  # the constant-speed solver's CFL_LIMIT, bit for bit
    return 2.0 / math.sqrt(3.0 * (abs(w[0]) + 2.0 * sum(abs(v) for v in w[1:])))


def _check_star_box(shape, box, M: int, mirror) -> tuple:
    """The box and mirror contract of the high-order step (the same checks as the HIP launcher);
    returns the mirror as a 4-tuple."""
    mirror = (None,) * 4 if mirror is None else tuple(mirror)
    if len(mirror) != 4:
        raise ValueError("mirror = (j_lo, j_hi, k_lo, k_hi), an entry may be None")
    nx, ny, nz = shape
    i0, i1, j0, j1, k0, k1 = box
    if not (M <= i0 and i1 <= nx - 1 - M):
        raise ValueError(f"box {tuple(box)} nearer than {M} to the storage edge in x ({nx} planes)")
    for name, lo, hi, n, f_lo, f_hi in (("y", j0, j1, ny, mirror[0], mirror[1]), ("z", k0, k1, nz, mirror[2], mirror[3])):
        for f, inside in ((f_lo, lambda f: f + (M - 1) <= n - 1), (f_hi, lambda f: f - (M - 1) >= 0)):
            if f is not None and not (0 <= f <= n - 1 and inside(f)):
                raise ValueError(f"mirror face {f} in {name}: outside the storage of {n} nodes, or a reflected "
                                 f"node would leave it")
        if f_lo is not None and f_hi is not None and f_hi - f_lo < M:
            raise ValueError(f"mirror faces {f_lo}, {f_hi} in {name} are nearer than {M}")
        if not (lo > f_lo if f_lo is not None else lo >= M) or not (hi < f_hi if f_hi is not None else hi <= n - 1 - M):
            raise ValueError(f"box {tuple(box)} in {name}: not strictly inside its mirror faces {f_lo}, {f_hi}, or "
                             f"nearer than {M} to an unmirrored storage edge ({n} nodes)")
    return mirror


def laplace_star(u, box, hx2, hy2, hz2, *, order: int, mirror=None) -> torch.Tensor:
    """Star Laplacian of ``order`` (half-width M = order / 2) on the nodes of ``box`` (storage
    indices, inclusive) of the grid ``u``. Per axis, with centre v and neighbours p_-d, p_+d:
    ``t = c_0 v``, then ``t = t + c_d (p_-d + p_+d)`` for d = 1 .. M, every operation rounded on its
    own, and ``lap = ((0 + t_x / hx2) + t_y / hy2) + t_z / hz2``.

    The x neighbours come from storage (the box keeps M planes from both ends). ``mirror = (j_lo,
    j_hi, k_lo, k_hi)``: storage indices of reflecting (Dirichlet) faces in y and z, an entry may be
    None. A neighbour beyond a face f is read as ``-u[2 f - j]`` (odd reflection), the face itself as
    stored; the box lies strictly inside its faces and a pair of faces is at least M apart. On a
    side without a face the neighbours come from storage and the box keeps M nodes from its edge."""
    w = [torch.tensor(v, dtype=u.dtype, device=u.device) for v in star_weights(order)]
    M = order // 2
    i0, i1, j0, j1, k0, k1 = (int(v) for v in box)
    mirror = _check_star_box(u.shape, (i0, i1, j0, j1, k0, k1), M, mirror)
    si, sj, sk = slice(i0, i1 + 1), slice(j0, j1 + 1), slice(k0, k1 + 1)
    c = u[si, sj, sk]

    def shifted(axis, lo, hi, off, f_lo, f_hi):
        idx = torch.arange(lo + off, hi + off + 1, device=u.device)
        neg = torch.zeros_like(idx, dtype=torch.bool)
        if f_lo is not None:
            neg = neg | (idx < f_lo)
            idx = torch.where(idx < f_lo, 2 * f_lo - idx, idx)
        if f_hi is not None:
            neg = neg | (idx > f_hi)
            idx = torch.where(idx > f_hi, 2 * f_hi - idx, idx)
        sl = [si, sj, sk]
        sl[axis] = slice(None)
        v = u[tuple(sl)].index_select(axis, idx)
        shape = [1, 1, 1]
        shape[axis] = -1
        return torch.where(neg.reshape(shape), -v, v)

    ans = torch.zeros_like(c)
    for axis, (lo, hi, f_lo, f_hi, h2) in enumerate(((i0, i1, None, None, hx2), (j0, j1, mirror[0], mirror[1], hy2),
                                                     (k0, k1, mirror[2], mirror[3], hz2))):
        t = w[0] * c
        for d in range(1, M + 1):
            t = t + w[d] * (shifted(axis, lo, hi, -d, f_lo, f_hi) + shifted(axis, lo, hi, d, f_lo, f_hi))
        ans = ans + t / h2
    return ans


def laplace_density(u: torch.Tensor, b: torch.Tensor, hx2, hy2, hz2) -> torch.Tensor:
    """Variable-density operator ``D_b u = div(b grad u)`` on all interior nodes ``u[1:-1, 1:-1, 1:-1]``,
    with the node-centred buoyancy ``b = 1 / rho`` (a grid like ``u``). A face value is the arithmetic
    mean of the two adjacent nodes' buoyancies (the harmonic mean of the densities). Per axis, with
    centre c, neighbours u_-, u_+ and buoyancies b_c, b_-, b_+:
    ``f_+ = (0.5 (b_c + b_+)) (u_+ - c)``, ``f_- = (0.5 (b_c + b_-)) (c - u_-)``, ``t = f_+ - f_-``,
    and ``D_b u = ((0 + t_x / hx2) + t_y / hy2) + t_z / hz2``, every operation rounded on its own.
    The operator is symmetric on the unique nodes; ``b == 1`` gives the 7-point Laplacian up to
    rounding."""
    if b.shape != u.shape or b.dtype != u.dtype:
        raise ValueError(f"buoyancy must match the grid: {tuple(u.shape)} {u.dtype}, not {tuple(b.shape)} {b.dtype}")
    inner = slice(1, -1)
    c = u[inner, inner, inner]
    bc = b[inner, inner, inner]
    ans = torch.zeros_like(c)
    for axis, h2 in enumerate((hx2, hy2, hz2)):
        lo, hi = [inner] * 3, [inner] * 3
        lo[axis], hi[axis] = slice(None, -2), slice(2, None)
        lo, hi = tuple(lo), tuple(hi)
        fp = (0.5 * (bc + b[hi])) * (u[hi] - c)
        fm = (0.5 * (bc + b[lo])) * (c - u[lo])
        ans = ans + (fp - fm) / h2
    return ans


def face_correlation(a: torch.Tensor, v: torch.Tensor, box, hx2, hy2, hz2) -> torch.Tensor:
    """Face correlation ``C(a, v)`` of two grids on the nodes of ``box`` (storage indices, inclusive):
    the sum over a node's six faces of the products of the two fields' differences across the face.
    Per axis, with centre values a_c, v_c and neighbours a_-, a_+, v_-, v_+:
    ``p_+ = (a_+ - a_c) (v_+ - v_c)``, ``p_- = (a_c - a_-) (v_c - v_-)``, ``t = p_+ + p_-``, and
    ``C = ((0 + t_x / hx2) + t_y / hy2) + t_z / hz2``, every operation rounded on its own. Symmetric
    in (a, v) bit for bit, and a face's product is the same number seen from either of its nodes.

    It is the derivative of ``laplace_density`` with respect to the buoyancy: for a vanishing on the
    boundary of the box's neighbourhood, ``d <a, D_b v> / d b_l = -C(a, v)_l / 2``. The box contract is
    ``step_medium``'s at order 2: every box node has its six neighbours inside the storage."""
    if a.dim() != 3 or v.shape != a.shape or v.dtype != a.dtype:
        raise ValueError(f"the two grids must match: {tuple(a.shape)} {a.dtype}, not {tuple(v.shape)} {v.dtype}")
    i0, i1, j0, j1, k0, k1 = (int(x) for x in box)
    nx, ny, nz = a.shape
    if not (1 <= i0 <= i1 <= nx - 2 and 1 <= j0 <= j1 <= ny - 2 and 1 <= k0 <= k1 <= nz - 2):
        raise ValueError(f"box {tuple(box)} is empty or touches an edge of the {nx}x{ny}x{nz} storage")
    ctr = [slice(i0, i1 + 1), slice(j0, j1 + 1), slice(k0, k1 + 1)]
    ac, vc = a[tuple(ctr)], v[tuple(ctr)]
    ans = torch.zeros_like(ac)
    for axis, h2 in enumerate((hx2, hy2, hz2)):
        lo, hi = list(ctr), list(ctr)
        lo[axis] = slice(ctr[axis].start - 1, ctr[axis].stop - 1)
        hi[axis] = slice(ctr[axis].start + 1, ctr[axis].stop + 1)
        lo, hi = tuple(lo), tuple(hi)
        pp = (a[hi] - ac) * (v[hi] - vc)
        pm = (ac - a[lo]) * (vc - v[lo])
        ans = ans + (pp + pm) / h2
    return ans


def _lap_box(u1, box, hx2, hy2, hz2, order: int, mirror, buoyancy=None):
    """lap(u1) on the nodes of ``box``: order 2 is ``laplace7`` (today's operations), 4 and 8
    ``laplace_star``; with ``buoyancy`` (order 2 only) ``laplace_density``."""
    if buoyancy is not None:
        if order != 2:
            raise ValueError(f"variable density exists for space order 2 only, not {order!r}")
        i0, i1, j0, j1, k0, k1 = box
        return laplace_density(u1, buoyancy, hx2, hy2, hz2)[i0 - 1:i1, j0 - 1:j1, k0 - 1:k1]
    if order == 2:
        i0, i1, j0, j1, k0, k1 = box
        return laplace7(u1, hx2, hy2, hz2)[i0 - 1:i1, j0 - 1:j1, k0 - 1:k1]
    return laplace_star(u1, box, hx2, hy2, hz2, order=order, mirror=mirror)


def step_medium(u1, u2, m, box, *, first: bool, hx2, hy2, hz2, taper=None, order: int = 2,
                mirror=None, buoyancy=None, born=None, born_add=None) -> torch.Tensor:
    """Layer update on ``box`` with the per-node coefficient ``m = c^2 tau^2``: the Taylor start
    ``c + (0.5 m) lap`` or ``(2c - u2) + m lap``; returns the updated box values.

    order = 2: the 7-point Laplacian (``mirror`` is not used); 4 or 8: ``laplace_star`` with its box
    and ``mirror`` contract.

    buoyancy: a grid ``b = 1 / rho`` like ``u1`` (order 2 only): ``laplace_density`` takes the place of
    the Laplacian in every form below, and ``m = rho c^2 tau^2``. None: today's operations.

    taper = (gx, gy, gz), 1-D factors in (0, 1] per axis in storage indexing (the lengths of the
    grid's axes): the damped leapfrog of an absorbing sponge with ``G = gx (gy gz)`` per node,
    ``G (c + (0.5 m) lap)`` or ``G ((2c - G u2) + m lap)``, every operation rounded on its own.

    born = (q_box, dm): the step of Born (linearised) modelling on a perturbation field, leapfrog
    steps only: ``((2c - u2) + m lap) + dm q`` or ``G (((2c - G u2) + m lap) + dm q)``, the product
    rounded before its add. ``q_box`` = the Laplacian of the background field on the box, as
    ``_lap_box`` returns it; ``dm`` = the perturbation of m, a grid like m.

    born_add = s_box: the same step with the scattering term already formed, on the box (leapfrog steps
    only, not together with ``born``): ``((2c - u2) + m lap) + s`` or ``G (((2c - G u2) + m lap) + s)``.
    Born modelling with a density perturbation uses it (``born_medium``): there s has two terms."""
    if order not in STAR_WEIGHTS:
        raise ValueError(f"space order must be 2, 4 or 8, not {order!r}")
    i0, i1, j0, j1, k0, k1 = box
    sc = None
    if born_add is not None:
        if born is not None:
            raise ValueError("born_add cannot be combined with born")
        if first:
            raise ValueError("Born-add mode: not on the Taylor start (first=True)")
        want = (i1 - i0 + 1, j1 - j0 + 1, k1 - k0 + 1)
        if tuple(born_add.shape) != want:
            raise ValueError(f"born_add must have the box's shape {want}, not {tuple(born_add.shape)}")
        sc = born_add
    if born is not None:
        if first:
            raise ValueError("Born mode: not on the Taylor start (first=True)")
        q_box, dm = born
        want = (i1 - i0 + 1, j1 - j0 + 1, k1 - k0 + 1)
        if tuple(q_box.shape) != want or tuple(dm.shape) != tuple(u1.shape):
            raise ValueError(f"born = (q_box, dm): q_box must have the box's shape {want} and dm the grid's "
                             f"{tuple(u1.shape)}, not {tuple(q_box.shape)} and {tuple(dm.shape)}")
        sc = dm[i0:i1 + 1, j0:j1 + 1, k0:k1 + 1] * q_box
    lap = _lap_box(u1, box, hx2, hy2, hz2, order, mirror, buoyancy)
    c = u1[i0:i1 + 1, j0:j1 + 1, k0:k1 + 1]
    mb = m[i0:i1 + 1, j0:j1 + 1, k0:k1 + 1]
    if taper is None:
        if first:
            return c + (0.5 * mb) * lap
        v = (2 * c - u2[i0:i1 + 1, j0:j1 + 1, k0:k1 + 1]) + mb * lap
        return v if sc is None else v + sc
    gx, gy, gz = taper
    for t, n in zip(taper, u1.shape):
        if t.dim() != 1 or t.numel() != n or t.dtype != u1.dtype:
            raise ValueError(f"taper tables must be 1-D {u1.dtype} tensors of lengths {tuple(u1.shape)}")
    G = gx[i0:i1 + 1, None, None] * (gy[None, j0:j1 + 1, None] * gz[None, None, k0:k1 + 1])
    if first:
        return G * (c + (0.5 * mb) * lap)
    v = (2 * c - G * u2[i0:i1 + 1, j0:j1 + 1, k0:k1 + 1]) + mb * lap
    return G * (v if sc is None else v + sc)


def max_abs_field(u: torch.Tensor, init: float = -100.0) -> float:
    """max |u| with the NaN-ignoring rule of ``max_errors``."""
    a = u.abs()
    neg = torch.tensor(-math.inf, dtype=u.dtype, device=u.device)
    return max(torch.where(torch.isnan(a), neg, a).max().item() if a.numel() else -math.inf, init)


def _wrap_x(u, N: int, ghost: int = 1) -> None:
    """Fill the ``ghost`` periodic x planes per side of a level (local i = global + ghost)."""
    for g in range(1, ghost + 1):
        u[ghost - g] = u[N + ghost - g]
        u[N + ghost + g] = u[ghost + g]


def _node_field(v, N: int, name: str) -> torch.Tensor:
    s = torch.as_tensor(v, dtype=torch.float64)
    if s.dim() == 0:
        s = s.expand(N + 1, N + 1, N + 1)
    if tuple(s.shape) != (N + 1, N + 1, N + 1):
        raise ValueError(f"{name} must be a scalar or have shape {(N + 1,) * 3}, not {tuple(s.shape)}")
    return s


def medium_coefficient(speed2, tau: float, N: int, dtype, ghost: int = 1, density=None) -> torch.Tensor:
    """m = ((speed2 * tau) * tau), left to right in float64, then cast: ``[N+1+2 ghost][N+1][N+1]``
    in ``solve()``'s storage with ``ghost`` x ghost planes per side, filled periodically. With
    ``density`` (a scalar or ``(N+1)^3``): m = (((speed2 * rho) * tau) * tau), the bulk modulus
    ``rho c^2`` times ``tau^2``."""
    s = _node_field(speed2, N, "speed2")
    if density is not None:
        s = s * _node_field(density, N, "density")
    m = torch.zeros(N + 1 + 2 * ghost, N + 1, N + 1, dtype=dtype)
    m[ghost:N + 1 + ghost] = ((s * tau) * tau).to(dtype)
    _wrap_x(m, N, ghost)
    return m


def buoyancy_field(density, N: int, dtype, ghost: int = 1) -> torch.Tensor:
    """b = 1 / rho in float64, then cast, for ``density`` a scalar or ``(N+1)^3``: stored like
    ``medium_coefficient`` with the x ghost planes filled periodically."""
    r = _node_field(density, N, "density")
    b = torch.zeros(N + 1 + 2 * ghost, N + 1, N + 1, dtype=dtype)
    b[ghost:N + 1 + ghost] = (1.0 / r).to(dtype)
    _wrap_x(b, N, ghost)
    return b


def dbuoyancy_field(ddensity, density, N: int, dtype, ghost: int = 1) -> torch.Tensor:
    """The first-order change of the buoyancy for a perturbation ``ddensity`` of ``density`` (each a
    scalar or ``(N+1)^3``): db = -(drho / (rho rho)) in float64, then cast; stored like
    ``buoyancy_field`` with the x ghost planes filled periodically."""
    r = _node_field(density, N, "density")
    d = _node_field(ddensity, N, "ddensity")
    db = torch.zeros(N + 1 + 2 * ghost, N + 1, N + 1, dtype=dtype)
    db[ghost:N + 1 + ghost] = (-(d / (r * r))).to(dtype)
    _wrap_x(db, N, ghost)
    return db


def _buoyancy(density, N: int, dtype, order: int, ghost: int):
    """The buoyancy grid of ``density`` for the medium solver, None without one."""
    if density is None:
        return None
    if order != 2:
        raise ValueError(f"variable density exists for space order 2 only, not {order!r}")
    return buoyancy_field(density, N, dtype, ghost)


def source_table(wavelet, K: int, S: int, hx: float, hy: float, hz: float, dtype) -> torch.Tensor:
    """g[n-1, s] = f_s(t_{n-1}) / (hx*hy*hz) in float64, row 0 halved (Taylor start), then cast."""
    if S == 0:
        return torch.zeros(K, 0, dtype=dtype)
    if wavelet is None:
        raise ValueError("sources need a wavelet of shape [K, S]")
    w = torch.as_tensor(wavelet, dtype=torch.float64)
    if tuple(w.shape) != (K, S):
        raise ValueError(f"wavelet must have shape {(K, S)} (timesteps x sources), not {tuple(w.shape)}")
    g = w / (hx * hy * hz)
    if K > 0:
        g[0] = g[0] * 0.5
    return g.to(dtype)


def source_entries(sources, N: int, ghost: int = 1) -> list[tuple[tuple[int, int, int], int]]:
    """Storage nodes of the sources, ((local i, j, k), column of the source table): local =
    global + ghost in x; a source on the periodic plane 0 or N acts on both planes."""
    out = []
    for s, (i, j, k) in enumerate(sources):
        for gi in ((0, N) if i in (0, N) else (i,)):
            out.append(((gi + ghost, j, k), s))
    return out


def taper_tables(taper, N: int, dtype, ghost: int = 1) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Sponge factors (gx, gy, gz), each ``N+1`` values in global indexing (an entry may be None:
    ones), cast to ``dtype`` in ``solve()``'s storage: gx ``[N+1+2 ghost]`` with the x ghosts filled
    periodically like ``medium_coefficient``, gy and gz ``[N+1]``."""
    if len(taper) != 3:
        raise ValueError("taper = (gx, gy, gz)")
    out = []
    for name, t in zip("xyz", taper):
        t = torch.ones(N + 1, dtype=torch.float64) if t is None else torch.as_tensor(t, dtype=torch.float64).cpu()
        if t.dim() != 1 or t.numel() != N + 1:
            raise ValueError(f"taper g{name} must have {N + 1} values, not shape {tuple(t.shape)}")
        out.append(t.to(dtype))
    gx = torch.empty(N + 1 + 2 * ghost, dtype=dtype)
    gx[ghost:N + 1 + ghost] = out[0]
    _wrap_x(gx, N, ghost)
    return gx, out[1].contiguous(), out[2].contiguous()


# ---- off-grid sources and receivers ------------------------------------------------------------
#
# A position is given in fractional node coordinates (xi, eta, zeta) = (x / hx, y / hy, z / hz) and acts
# through 8 slots per axis: slot a is node floor(p) - 3 + a with the offset x = node - p and a weight
# w(x). The slots carry the boundary conditions: in x the node is taken modulo N onto the unique planes
# 0 .. N-1, in y and z a node beyond a face is reflected oddly (node -n -> n, node N + n -> N - n, the
# weight negated; laplace_star's convention) and a node on a face gets the weight 0. A position on a
# node gives a Kronecker delta, so the node lists are the special case. The tables below are built on
# the host once, shared by the oracle and the HIP front-end (models/medium.py), and the oracle ops
# (record_weighted, rows_values, inject_rows, rows_dot) have the kernels' arithmetic operation for
# operation (csrc/hip_medium_points.hip).

INTERP_KINDS = ("sinc8", "linear")
SINC8_B = 6.31  # the Kaiser window's shape parameter for the 8-point sinc
MIN_POSITION_N = 8


def interp_weight(x, kind: str = "sinc8") -> torch.Tensor:
    """The interpolation weight w(x) of a node at the offset ``x = node - position`` (float64).
    "sinc8": ``sinc(x) I0(b sqrt(1 - (x / 4)^2)) / I0(b)`` with b = 6.31 for |x| < 4, 0 beyond, exactly
    1 at x == 0 and exactly 0 at every other integer; "linear": ``max(0, 1 - |x|)``."""
    x = torch.as_tensor(x, dtype=torch.float64)
    if kind == "linear":
        return (1 - x.abs()).clamp(min=0)
    if kind != "sinc8":
        raise ValueError(f"interp must be one of {INTERP_KINDS}, not {kind!r}")
    b = torch.tensor(SINC8_B, dtype=torch.float64)
    w = torch.sinc(x) * torch.special.i0(b * (1 - (x / 4) ** 2).clamp(min=0).sqrt()) / torch.special.i0(b)
    w = torch.where(x.abs() >= 4, torch.zeros_like(w), w)
    return torch.where(x == x.round(), (x == 0).to(torch.float64), w)


def check_positions(positions, N: int, what: str) -> torch.Tensor:
    """Positions as a float64 ``[P, 3]`` CPU tensor of fractional node coordinates, validated: finite,
    ``0 <= xi <= N``; a "source" needs ``0 < eta, zeta < N`` (off the Dirichlet faces), a "receiver"
    ``0 <= eta, zeta <= N``; N >= 8."""
    p = torch.as_tensor(positions, dtype=torch.float64).detach().cpu()
    if p.dim() == 1 and p.numel() == 3:
        p = p.reshape(1, 3)
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f"{what} positions must have shape [count, 3] (xi, eta, zeta), not {tuple(p.shape)}")
    if N < MIN_POSITION_N:
        raise ValueError(f"{what} positions need N >= {MIN_POSITION_N}, not N = {N}")
    if not bool(torch.isfinite(p).all()):
        raise ValueError(f"{what} positions must be finite")
    for q in range(p.shape[0]):
        xi, eta, zeta = (float(v) for v in p[q])
        if not (0 <= xi <= N and 0 <= eta <= N and 0 <= zeta <= N):
            raise ValueError(f"{what} position {(xi, eta, zeta)} outside the grid 0..{N}")
        if what == "source" and not (0 < eta < N and 0 < zeta < N):
            raise ValueError(f"source position {(xi, eta, zeta)} lies on a Dirichlet face")
    return p


def _axis_intervals(N) -> tuple[int, int, int]:
    """N as (Nx, Ny, Nz): the solver's grids have one N; the kernels' tests also use other boxes."""
    return (int(N),) * 3 if isinstance(N, int) else tuple(int(v) for v in N)


def _interp_axes(pos: torch.Tensor, N, kind: str, ghost: int):
    """The slots of ``[P, 3]`` positions: (ix, iy, iz) int64 ``[P, 8]`` storage indices and (wx, wy, wz)
    float64 ``[P, 8]`` weights (see ``interp_tables``)."""
    if kind not in INTERP_KINDS:
        raise ValueError(f"interp must be one of {INTERP_KINDS}, not {kind!r}")
    NN = _axis_intervals(N)
    node = (torch.floor(pos).to(torch.int64) - 3)[:, :, None] + torch.arange(8)  # [P, 3, 8]
    w = interp_weight(node.to(torch.float64) - pos[:, :, None], kind)
    idx, wt = [torch.remainder(node[:, 0], NN[0]) + ghost], [w[:, 0]]
    for axis in (1, 2):
        N = NN[axis]
        n, v = node[:, axis], w[:, axis]
        lo, hi = n < 0, n > N
        n = torch.where(lo, -n, torch.where(hi, 2 * N - n, n))
        v = torch.where(lo | hi, -v, v)
        v = torch.where((n == 0) | (n == N), torch.zeros_like(v), v)
        idx.append(n)
        wt.append(v)
    return (*idx, *wt)


def interp_tables(position, N, kind: str = "sinc8", ghost: int = 1):
    """The 8-slot tables of one position (xi, eta, zeta) in fractional node coordinates: three int64
    index tables ``ix, iy, iz`` (storage indices; local i = global + ``ghost`` in x) and three float64
    weight tables ``wx, wy, wz``, 8 values each (``[P, 8]`` each for ``[P, 3]`` positions).

    Slot a of an axis is node ``floor(p) - 3 + a`` with the weight ``interp_weight(node - p, kind)``.
    x: the node modulo N, on the unique planes 0 .. N-1. y and z: a node n < 0 becomes -n and a node
    n > N becomes 2N - n, the weight negated (odd reflection); a node that lands on 0 or N gets the
    weight 0. Two slots may name the same node; they stay separate slots. ``N``: the intervals per axis,
    one number or (Nx, Ny, Nz)."""
    pos = torch.as_tensor(position, dtype=torch.float64)
    single = pos.dim() == 1
    out = _interp_axes(pos.reshape(-1, 3), N, kind, int(ghost))
    return tuple(t[0] for t in out) if single else out


def receiver_tables(positions, N, dtype, kind: str = "sinc8", ghost: int = 1, over_taper=None):
    """The gather tables of ``record_weighted`` for ``[R, 3]`` positions: (index int32 ``[R, 3, 8]``,
    weight ``[R, 3, 8]`` of ``dtype``; x, y, z slots). ``over_taper`` = the ``taper_tables``: every
    weight is divided, in ``dtype``, by the per-axis sponge factor of its slot's node, so that the
    gather returns ``sum W u / G`` with the separable G (the wavelet gradient's tables)."""
    pos = torch.as_tensor(positions, dtype=torch.float64).reshape(-1, 3)
    ix, iy, iz, wx, wy, wz = _interp_axes(pos, N, kind, ghost)
    index = torch.stack([ix, iy, iz], 1).to(torch.int32).contiguous()
    weight = torch.stack([wx, wy, wz], 1).to(dtype)
    if over_taper is not None:
        for axis, (t, i) in enumerate(zip(over_taper, (ix, iy, iz))):
            weight[:, axis] = weight[:, axis] / t[i]
    return index, weight.contiguous()


class PointRows:
    """A CSR list of the nodes a set of points touches: ``nodes`` int32 ``[rows, 3]`` storage nodes,
    ``rowptr`` int32 ``[rows + 1]``, and per entry the point ``col`` (int32) and the weight ``w``.
    ``unique``: the leading rows without the plane-N duplicates; ``ncols``: the number of points."""

    def __init__(self, nodes, rowptr, col, w, unique: int, ncols: int):
        self.nodes, self.rowptr, self.col, self.w = nodes, rowptr, col, w
        self.unique, self.ncols = int(unique), int(ncols)
        self._pad = None

    def __len__(self):
        return int(self.nodes.shape[0])

    @property
    def entries(self) -> int:
        return int(self.col.numel())

    def ijk(self):
        n = self.nodes.long()
        return n[:, 0], n[:, 1], n[:, 2]

    def padded(self):
        """(col, w, mask), each ``[rows, longest row]``: the entries of every row in order, padded."""
        if self._pad is None:
            ptr = self.rowptr.long()
            cnt = ptr[1:] - ptr[:-1]
            width = int(cnt.max()) if len(cnt) else 0
            e = ptr[:-1, None] + torch.arange(width)[None, :]
            mask = torch.arange(width)[None, :] < cnt[:, None]
            e = torch.where(mask, e, torch.zeros_like(e))
            if self.entries:
                self._pad = (self.col.long()[e], self.w[e], mask)
            else:
                self._pad = (e, torch.zeros(e.shape, dtype=self.w.dtype), mask)
        return self._pad


def point_rows(positions, N, dtype, kind: str = "sinc8", ghost: int = 1, tt=None) -> PointRows:
    """The row list of ``[P, 3]`` points (sources, or receivers acting as adjoint sources): all 8^3 slot
    triples of each point with the weight ``(wx[a] wy[b]) wz[c]``, every factor cast to ``dtype`` first
    and the products formed in it; entries whose weight is exactly 0 are dropped and the rest grouped
    by storage node. Rows are sorted by (i, j, k), the entries of a row by point, then (a, b, c); entries
    of one point that fold onto the same node stay separate. A row on the unique plane 0 is emitted for
    both storage planes, ``ghost`` and ``N + ghost``, like ``source_entries``; these duplicates are the
    last rows. ``tt`` = the ``taper_tables``: each weight is multiplied once more, in ``dtype``, by
    ``taper_at(tt, node)`` (the ``G rho`` of ``adjoint_source_table``)."""
    pos = torch.as_tensor(positions, dtype=torch.float64).reshape(-1, 3)
    P = pos.shape[0]
    ix, iy, iz, wx, wy, wz = _interp_axes(pos, N, kind, ghost)
    wx, wy, wz = wx.to(dtype), wy.to(dtype), wz.to(dtype)
    W = ((wx[:, :, None, None] * wy[:, None, :, None]) * wz[:, None, None, :]).reshape(-1)
    full = (P, 8, 8, 8)
    I = ix[:, :, None, None].expand(full).reshape(-1)
    J = iy[:, None, :, None].expand(full).reshape(-1)
    Kk = iz[:, None, None, :].expand(full).reshape(-1)
    col = torch.arange(P)[:, None].expand(P, 512).reshape(-1)
    keep = W != 0
    W, I, J, Kk, col = W[keep], I[keep], J[keep], Kk[keep], col[keep]
    if tt is not None:
        W = W * (tt[0][I] * (tt[1][J] * tt[2][Kk]))
    Nx, ny1, nz1 = (v + d for v, d in zip(_axis_intervals(N), (0, 1, 1)))
    key, order = torch.sort((I * ny1 + J) * nz1 + Kk, stable=True)  # keeps (point, a, b, c) within a node
    W, col = W[order], col[order]
    rows, cnt = torch.unique_consecutive(key, return_counts=True)
    nodes = torch.stack([rows // (ny1 * nz1), (rows // nz1) % ny1, rows % nz1], 1)
    ptr = torch.zeros(len(rows) + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(cnt, 0)
    unique = len(rows)
    dup = (nodes[:, 0] == ghost).nonzero().flatten()  # the unique plane 0 acts on plane N too
    if len(dup):
        e = torch.cat([torch.arange(int(ptr[r]), int(ptr[r + 1])) for r in dup])
        twin = nodes[dup].clone()
        twin[:, 0] = Nx + ghost
        nodes = torch.cat([nodes, twin])
        ptr = torch.cat([ptr, ptr[-1] + torch.cumsum(cnt[dup], 0)])
        W, col = torch.cat([W, W[e]]), torch.cat([col, col[e]])
    return PointRows(nodes.to(torch.int32).contiguous(), ptr.to(torch.int32), col.to(torch.int32).contiguous(),
                     W.contiguous(), unique, P)


def record_weighted(u: torch.Tensor, index: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """The weighted gather of ``k_record_w``: ``[R]`` values from the ``receiver_tables``. Per receiver
    and slot pair (a, b): ``s = s + wz[c] u[ix[a], iy[b], iz[c]]`` for c = 0 .. 7 from s = 0, then
    ``t = (wx[a] wy[b]) s``; the 64 values, l = 8a + b, are summed by ``v = v[:h] + v[h:2h]`` for
    h = 32, 16, 8, 4, 2, 1, the kernel's xor butterfly as lane 0 sees it."""
    idx = index.long()
    ix, iy, iz = idx[:, 0], idx[:, 1], idx[:, 2]
    U = u[ix[:, :, None, None], iy[:, None, :, None], iz[:, None, None, :]]  # [R, 8, 8, 8]
    wx, wy, wz = weight[:, 0], weight[:, 1], weight[:, 2]
    s = torch.zeros(U.shape[:3], dtype=u.dtype, device=u.device)
    for c in range(8):
        s = s + wz[:, None, None, c] * U[:, :, :, c]
    v = ((wx[:, :, None] * wy[:, None, :]) * s).reshape(-1, 64)
    for h in (32, 16, 8, 4, 2, 1):
        v = v[:, :h] + v[:, h:2 * h]
    return v[:, 0]


def rows_values(rows: PointRows, g: torch.Tensor) -> torch.Tensor:
    """``val[row] = val + w[e] g[col[e]]`` over the entries of every row in order, from 0: the row loop
    of ``k_inject_rows``. ``g``: one value per point."""
    colp, wp, mask = rows.padded()
    val = torch.zeros(len(rows), dtype=rows.w.dtype)
    for e in range(colp.shape[1]):
        val = torch.where(mask[:, e], val + wp[:, e] * g[colp[:, e]], val)
    return val


def inject_rows(u: torch.Tensor, m: torch.Tensor, rows: PointRows, g: torch.Tensor) -> None:
    """``u[node] = u[node] + m[node] val`` at the nodes of ``rows`` (in place), val = ``rows_values``."""
    if len(rows) == 0:
        return
    i, j, k = rows.ijk()
    u[i, j, k] = u[i, j, k] + m[i, j, k] * rows_values(rows, g)


def rows_dot(u: torch.Tensor, rows: PointRows, g: torch.Tensor, sacc: torch.Tensor) -> torch.Tensor:
    """``sacc[row] + u[node] val`` over the unique rows (``k_rows_dot``); returns the new ``[unique]`` sums."""
    n = rows.unique
    i, j, k = rows.ijk()
    return sacc[:n] + u[i[:n], j[:n], k[:n]] * rows_values(rows, g)[:n]


class _Points:
    """The sources and receivers of an oracle run, node lists or positions on either side."""

    def __init__(self, N: int, M: int, dtype, sources, receivers, source_positions, receiver_positions, interp):
        if source_positions is not None and len(sources):
            raise ValueError("give sources or source_positions, not both")
        if receiver_positions is not None and len(receivers):
            raise ValueError("give receivers or receiver_positions, not both")
        if interp not in INTERP_KINDS:
            raise ValueError(f"interp must be one of {INTERP_KINDS}, not {interp!r}")
        self.N, self.M, self.dtype, self.interp = N, M, dtype, interp
        self.spos = None if source_positions is None else check_positions(source_positions, N, "source")
        self.rpos = None if receiver_positions is None else check_positions(receiver_positions, N, "receiver")
        self.sources, self.receivers = sources, receivers
        self.ent = source_entries(sources, N, M) if self.spos is None else None
        self.rows = None if self.spos is None else point_rows(self.spos, N, dtype, interp, M)
        self.rec = [(i + M, j, k) for i, j, k in receivers] if self.rpos is None else None
        self.rtab = None if self.rpos is None else receiver_tables(self.rpos, N, dtype, interp, M)
        self.S = len(sources) if self.spos is None else int(self.spos.shape[0])
        self.R = len(receivers) if self.rpos is None else int(self.rpos.shape[0])

    def inject(self, u, m, g) -> None:
        """The source terms of one step: ``g`` = the step's row of the source table."""
        if self.rows is not None:
            inject_rows(u, m, self.rows, g)
            return
        for nd, s in self.ent:
            u[nd] = u[nd] + m[nd] * g[s]

    def sample(self, u) -> torch.Tensor:
        if self.rtab is not None:
            return record_weighted(u, *self.rtab)
        return torch.stack([u[nd] for nd in self.rec]) if self.rec else torch.zeros(0, dtype=u.dtype, device=u.device)


# ---- on-the-fly discrete Fourier transform (csrc/hip_medium_dft.hip) -------------------------
#
# While a time loop runs, a few monochromatic components of a field are summed up level by level:
# U_f = sum_p u^p exp(-i 2 pi f p tau) over the sampled indices p, as the two real sums
#   re_f = re_f + u c[p, f],   im_f = im_f + u s[p, f],   c = cos(2 pi f p tau),  s = -sin(2 pi f p tau),
# every product rounded before its add. The twiddle tables are formed in float64 and cast once.

def check_frequencies(frequencies) -> torch.Tensor:
    """The frequencies in Hz as a float64 tensor: a non-empty 1-D list of finite values >= 0."""
    try:
        f = torch.as_tensor(frequencies, dtype=torch.float64).cpu()
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"frequencies must be a 1-D list of numbers: {e}") from None
    if f.dim() != 1 or f.numel() == 0:
        raise ValueError(f"frequencies must be a non-empty 1-D list, not shape {tuple(f.shape)}")
    bad = ~(torch.isfinite(f) & (f >= 0))
    if bool(bad.any()):
        raise ValueError(f"frequencies must be finite and >= 0, found {f[bad][0].item()}")
    return f


def check_dft_every(dft_every) -> int:
    if isinstance(dft_every, bool) or not isinstance(dft_every, int) or dft_every < 1:
        raise ValueError(f"dft_every must be an integer >= 1, not {dft_every!r}")
    return dft_every


def dft_tables(frequencies, indices, tau: float, dtype) -> tuple[torch.Tensor, torch.Tensor]:
    """Twiddle tables ``(c, s)``, ``[len(indices), F]`` each: ``c[r, f] = cos(a)``, ``s[r, f] = -sin(a)`` with
    ``a = ((2 pi f) p) tau`` for the integer sample index ``p = indices[r]``, evaluated in float64 and then
    cast once to ``dtype``."""
    f = check_frequencies(frequencies)
    p = torch.as_tensor(list(indices), dtype=torch.int64)
    if p.dim() != 1:
        raise ValueError("indices must be a 1-D list of integers")
    a = ((2 * math.pi * f)[None, :] * p.to(torch.float64)[:, None]) * float(tau)
    return torch.cos(a).to(dtype), (-torch.sin(a)).to(dtype)


def dft_accumulate(re, im, u: torch.Tensor, box, c_row, s_row) -> None:
    """One accumulation, in place on the lists ``re`` / ``im`` of F tensors shaped like ``u``: at the
    nodes of ``box`` = (i0, i1, j0, j1, k0, k1), for f ascending, ``re[f] = re[f] + u c_row[f]`` and
    ``im[f] = im[f] + u s_row[f]``, the product rounded before the add. ``u`` is never written and the
    nodes outside the box keep their values (``k_dft_acc``)."""
    if len(re) != len(im) or len(re) == 0 or len(c_row) != len(re) or len(s_row) != len(re):
        raise ValueError("re, im, c_row and s_row must have one entry per frequency, at least one")
    i0, i1, j0, j1, k0, k1 = box
    sl = (slice(i0, i1 + 1), slice(j0, j1 + 1), slice(k0, k1 + 1))
    for f in range(len(re)):
        if re[f].shape != u.shape or im[f].shape != u.shape or re[f].dtype != u.dtype or im[f].dtype != u.dtype:
            raise ValueError("re and im levels must match u in shape and dtype")
        re[f][sl] = re[f][sl] + u[sl] * torch.as_tensor(c_row[f]).to(u.dtype)
        im[f][sl] = im[f][sl] + u[sl] * torch.as_tensor(s_row[f]).to(u.dtype)


def finish_gradient_dft(Qre, Qim, Mre, Mim, weights, dtype) -> torch.Tensor:
    """``acc = sum_f w_f (Qre_f Mre_f + Qim_f Mim_f)``, the correlation of the spectra of q and mu that
    takes the place of ``sum_n mu^{n+1} q^n``: from ``acc = 0``, for f ascending ``t = Qre_f Mre_f``,
    ``t = t + Qim_f Mim_f``, ``acc = acc + w_f t``, every operation rounded on its own in ``dtype``.
    ``weights`` None: ones. The host-side step shared by both backends (CPU tensors)."""
    F = len(Qre)
    w = torch.ones(F, dtype=torch.float64) if weights is None else torch.as_tensor(weights, dtype=torch.float64)
    if w.dim() != 1 or w.numel() != F or not bool(torch.isfinite(w).all()):
        raise ValueError(f"weights must be {F} finite values, one per frequency")
    w = w.to(dtype)
    acc = torch.zeros_like(Qre[0], dtype=dtype)
    for f in range(F):
        t = Qre[f] * Mre[f]
        t = t + Qim[f] * Mim[f]
        acc = acc + w[f] * t
    return acc


def solve_medium(N: int, K: int, speed2, *, u0=None, sources=(), wavelet=None, receivers=(),
                 L=("pi", "pi", "pi"), T: float = 1.0, pi: str = "ref", dtype=torch.float64, device="cpu",
                 taper=None, order: int = 2, density=None, source_positions=None, receiver_positions=None,
                 interp: str = "sinc8", frequencies=None, dft_every: int = 1):
    """Whole single-domain solve of ``(1/c^2) u_tt = lap u + f`` from rest in PyTorch, in
    ``solve()``'s storage (x ghosts, local = global + 1).

    order: the space order, 2 (the 7-point Laplacian), 4 or 8 (``laplace_star``: the levels then
    carry order / 2 x ghost planes per side, local = global + order / 2, and the Dirichlet faces
    reflect oddly); the results keep their shapes.

    speed2: c^2, a scalar or ``(N+1)^3``; u0: the initial field (``(N+1)^3``, default 0), used as
    given, face values included; sources / receivers: global (i, j, k) nodes; wavelet ``[K, S]``:
    f_s at t_n = n tau, n = 0..K-1. Step n adds ``m[x_s] * g[n-1, s]`` after the stencil and before
    the periodic wrap. Returns (traces ``[K+1, R]`` with row 0 the initial field, u_K ``(N+1)^3``,
    max |u| per layer ``[K+1]``: over the stencil nodes, of the step's result before its source term).

    taper = (gx, gy, gz): sponge factors per axis, ``N+1`` values each in global indexing
    (``taper_tables``); every step is then the damped one of ``step_medium`` (the source term is
    not tapered in its own step). None: the undamped scheme.

    density: rho, a scalar or ``(N+1)^3`` (order 2 only): ``(1/kappa) u_tt = div(b grad u) + f`` with
    ``kappa = rho c^2`` and ``b = 1 / rho``; m becomes ``kappa tau^2`` (``medium_coefficient``) and every
    step uses ``laplace_density``. None: the constant-density operations, unchanged.

    source_positions / receiver_positions: ``[S, 3]`` / ``[R, 3]`` fractional node coordinates in place of
    ``sources`` / ``receivers`` (each side exclusive with its node list; CPU only), acting through the
    ``interp`` slots ("sinc8" or "linear"; ``interp_tables``): step n adds ``m[p] val_p(g[n-1])`` at every
    touched node p (``inject_rows``) and a trace is the weighted gather ``record_weighted``.

    frequencies (Hz; a non-empty list of finite values >= 0) / dft_every = e >= 1: the on-the-fly Fourier
    transform. For n = 0, e, 2e, ... <= K the level u^n, after its source term and the x wrap (n = 0: the
    initial field), is accumulated with the twiddle row p = n (``dft_tables``, ``dft_accumulate``) on the
    step box. The result then has a fourth entry, the spectra ``sum_n u^n exp(-i 2 pi f n tau)`` as a
    complex ``[F, N+1, N+1, N+1]`` tensor (the Dirichlet faces 0); the first three do not change by a bit.
    """
    c = tables(N, K, L, T, pi)[4]
    M, box, mirror = _medium_layout(N, order)
    pts = _Points(N, M, dtype, sources, receivers, source_positions, receiver_positions, interp)
    spec = None
    if frequencies is not None:
        e = check_dft_every(dft_every)
        ctab, stab = dft_tables(frequencies, range(K + 1), c["tau"], dtype)
        F = ctab.shape[1]
        spec = tuple([torch.zeros(N + 1 + 2 * M, N + 1, N + 1, dtype=dtype, device=device) for _ in range(F)]
                     for _ in range(2))

    def transform(n, u):
        if spec is not None and n % e == 0:
            dft_accumulate(spec[0], spec[1], u, box, ctab[n], stab[n])

    if (pts.rows is not None or pts.rtab is not None) and torch.device(device).type != "cpu":
        raise ValueError("positions exist on the CPU oracle only")
    if taper is not None:
        taper = tuple(t.to(device) for t in taper_tables(taper, N, dtype, M))
    m = medium_coefficient(speed2, c["tau"], N, dtype, M, density).to(device)
    bu = _buoyancy(density, N, dtype, order, M)
    if bu is not None:
        bu = bu.to(device)
    g = source_table(wavelet, K, pts.S, c["hx"], c["hy"], c["hz"], dtype).to(device)
    lv = [torch.zeros(N + 1 + 2 * M, N + 1, N + 1, dtype=dtype, device=device) for _ in range(3)]

    def wrap(u):
        _wrap_x(u, N, M)

    if u0 is not None:
        u0 = torch.as_tensor(u0)
        if tuple(u0.shape) != (N + 1, N + 1, N + 1):
            raise ValueError(f"u0 must have shape {(N + 1,) * 3}, not {tuple(u0.shape)}")
        lv[0][M:N + 1 + M] = u0.to(dtype).to(device)
        wrap(lv[0])
    traces = torch.zeros(K + 1, pts.R, dtype=dtype, device=device)

    def sample(n, u):
        traces[n] = pts.sample(u)

    sample(0, lv[0])
    transform(0, lv[0])
    mx = [max_abs_field(lv[0][M:N + 1 + M, 1:N, 1:N])]
    for n in range(1, K + 1):
        u1, u2, u = lv[(n + 2) % 3], lv[(n + 1) % 3], lv[n % 3]
        u.zero_()
        vals = step_medium(u1, u2, m, box, first=n == 1, hx2=c["hx2"], hy2=c["hy2"], hz2=c["hz2"], taper=taper,
                           order=order, mirror=mirror, buoyancy=bu)
        mx.append(max_abs_field(vals))
        u[M:N + 1 + M, 1:N, 1:N] = vals
        pts.inject(u, m, g[n - 1])
        wrap(u)
        sample(n, u)
        transform(n, u)
    out = (traces, lv[K % 3][M:N + 1 + M].clone(), mx)
    if spec is not None:
        out += (spectra_tensor(spec[0], spec[1], N, M),)
    return out


def spectra_tensor(re, im, N: int, ghost: int = 1) -> torch.Tensor:
    """The storage-shaped accumulators of ``dft_accumulate`` as one complex ``[F, N+1, N+1, N+1]`` tensor
    on the CPU: the planes ``ghost .. N + ghost`` of every level."""
    return torch.complex(torch.stack([t[ghost:N + 1 + ghost].cpu() for t in re]),
                         torch.stack([t[ghost:N + 1 + ghost].cpu() for t in im]))


# ---- misfit gradients of the medium solver (adjoint state) ---------------------------------
#
# From rest, on the unique nodes (plane N is plane 0, Dirichlet faces 0), solve_medium is
#   u^1 = m g[0] e_s,   u^{n+1} = G ((2 u^n - G u^{n-1}) + m L u^n) + m g[n] e_s,
# with L symmetric. With J = 1/2 sum_{n=1..K} sum_r (u^n[x_r] - d[n, r])^2, lambda the adjoint state
# and mu = m G lambda, the adjoint recurrence is the forward step run backwards in time,
#   mu^K = m (G rho^K),   mu^n = G ((2 mu^{n+1} - G mu^{n+2}) + m L mu^{n+1}) + m (G rho^n),
# rho^n the residuals scattered to the receiver nodes, and with q^n = L u^n
#   dJ/dm = (sum_{n=K-1..1} mu^{n+1} q^n) / m + e_s (sum_n mu^{n+1}[x_s] g[n, s]) / (m[x_s] G[x_s]),
#   dJ/dg[n, s] = mu^{n+1}[x_s] / G[x_s].
# With a density, m = rho c^2 tau^2 and L = D_b with b = 1 / rho; summation by parts (mu is 0 on the
# Dirichlet faces, x is periodic) gives dJ/db = -1/2 sum_{n=K-1..1} C(mu^{n+1}, u^n), C the
# face_correlation, and dJ/drho at fixed c^2 = dJ/dm c^2 tau^2 + (1/2 sum_n C) / rho^2
# (gradient_medium_density, finish_gradient_density).
# The helpers below are the host-side arithmetic shared by gradient_medium and the HIP front-end
# (models/medium.py): both call them on CPU tensors, so they round alike.

def _medium_box(N: int, ghost: int = 1):
    return (ghost, N + ghost, 1, N - 1, 1, N - 1)


def _medium_layout(N: int, order: int):
    """(x ghost depth M = order / 2, the step box, the mirror faces or None) of the medium solver's
    storage for a space order."""
    if order not in STAR_WEIGHTS:
        raise ValueError(f"space order must be 2, 4 or 8, not {order!r}")
    M = order // 2
    if N < 2 * M:
        raise ValueError(f"space order {order} needs N >= {2 * M}, not N = {N}")
    return M, _medium_box(N, M), (None if order == 2 else (0, N, 0, N))


def taper_at(tt, node):
    """G = gx[i] (gy[j] gz[k]) at a storage node, rounded like ``step_medium``; ``tt`` = the
    ``taper_tables`` (None: 1)."""
    if tt is None:
        return 1.0
    i, j, k = node
    return tt[0][i] * (tt[1][j] * tt[2][k])


def forward_medium_autograd(N: int, K: int, speed2, *, sources=(), wavelet=None, receivers=(), taper=None,
                            L=("pi", "pi", "pi"), T: float = 1.0, pi: str = "ref", dtype=torch.float64,
                            keep_lap: bool = False, order: int = 2, density=None, keep_levels: bool = False,
                            source_positions=None, receiver_positions=None, interp: str = "sinc8", points=None):
    """``solve_medium`` from rest, restated out of place: every level is a new tensor, so
    ``torch.autograd`` can differentiate the traces with respect to ``speed2`` (an ``(N+1)^3``
    tensor) and ``wavelet``. The operations and their order are those of ``solve_medium``: the traces
    ``[K+1, R]`` are equal bit for bit. ``keep_lap``: also return [q^1 .. q^{K-1}], q^n = lap u^n on
    the stencil nodes (the value step n+1 uses). ``density``: as in ``solve_medium`` (a scalar, an
    ``(N+1)^3`` tensor or a leaf to differentiate with respect to; q^n is then ``laplace_density`` of
    u^n). ``keep_levels``: also return [u^1 .. u^{K-1}], whole levels in storage with their x ghosts
    (after ``keep_lap``'s list if both are asked for). ``source_positions`` / ``receiver_positions`` /
    ``interp``: as in ``solve_medium``."""
    c = tables(N, K, L, T, pi)[4]
    M, box, mirror = _medium_layout(N, order)
    pts = points or _Points(N, M, dtype, sources, receivers, source_positions, receiver_positions, interp)
    shape = (N + 1 + 2 * M, N + 1, N + 1)
    tt = None if taper is None else taper_tables(taper, N, dtype, M)
    m = medium_coefficient(speed2, c["tau"], N, dtype, M, density)
    bu = _buoyancy(density, N, dtype, order, M)
    g = source_table(wavelet, K, pts.S, c["hx"], c["hy"], c["hz"], dtype)
    u2 = torch.zeros(shape, dtype=dtype)
    u1 = torch.zeros(shape, dtype=dtype)
    rows = [pts.sample(u1)]
    laps, levels = [], []
    for n in range(1, K + 1):
        if keep_lap and n >= 2:
            laps.append(_lap_box(u1, box, c["hx2"], c["hy2"], c["hz2"], order, mirror, bu))
        if keep_levels and n >= 2:
            levels.append(u1)
        vals = step_medium(u1, u2, m, box, first=n == 1, hx2=c["hx2"], hy2=c["hy2"], hz2=c["hz2"], taper=tt,
                           order=order, mirror=mirror, buoyancy=bu)
        u = torch.zeros(shape, dtype=dtype)
        u[M:N + 1 + M, 1:N, 1:N] = vals
        pts.inject(u, m, g[n - 1])
        _wrap_x(u, N, M)
        rows.append(pts.sample(u))
        u2, u1 = u1, u
    traces = torch.stack(rows)
    out = (traces,) + ((laps,) if keep_lap else ()) + ((levels,) if keep_levels else ())
    return out if len(out) > 1 else traces


def misfit_medium(traces, observed):
    """J = 1/2 sum_{n=1..K} sum_r (traces[n, r] - observed[n, r])^2 in the dtype of ``traces`` (row
    0 does not enter); returns (J as a float, the residuals ``[K+1, R]`` with row 0 zeroed)."""
    if tuple(observed.shape) != tuple(traces.shape):
        raise ValueError(f"observed must have shape {tuple(traces.shape)} (timesteps + 1 x receivers), "
                         f"not {tuple(observed.shape)}")
    res = traces - torch.as_tensor(observed).to(traces.dtype).cpu()
    res[0] = 0
    return (0.5 * (res * res).sum()).item(), res


def adjoint_source_table(res, receivers, N: int, tt, ghost: int = 1):
    """Adjoint sources of the residuals ``res`` ``[K+1, R]``: ([storage nodes], table ``[K+1, E]``).

    Receivers that share a unique node (planes 0 and N are one plane) are summed in list order;
    a receiver on a Dirichlet face injects nothing; a node on the periodic plane yields entries on
    both storage planes, like ``source_entries``. Column e of the table is ``G[node] * rho`` rounded
    in the dtype of ``res`` (``tt`` = the ``taper_tables``, None: G = 1). ``ghost``: the x ghost depth
    of the storage (local i = global + ghost)."""
    rho = {}
    for r, (i, j, k) in enumerate(receivers):
        if j in (0, N) or k in (0, N):
            continue
        key = (i % N, j, k)
        rho[key] = rho[key] + res[:, r] if key in rho else res[:, r].clone()
    nodes, cols = [], []
    for (i, j, k), v in rho.items():
        for gi in ((0, N) if i == 0 else (i,)):
            nd = (gi + ghost, j, k)
            nodes.append(nd)
            cols.append(taper_at(tt, nd) * v)
    tab = torch.stack(cols, 1).contiguous() if cols else torch.zeros(res.shape[0], 0, dtype=res.dtype)
    return nodes, tab


def source_unique_nodes(sources, N: int, ghost: int = 1):
    """One storage node per source for sampling the adjoint field: plane N is read on plane 0."""
    return [((i % N) + ghost, j, k) for i, j, k in sources]


def _gradient_wrt_m(acc, a, g, m, tt, sources, N: int, ghost: int, source_rows=None):
    """dJ/dm on the planes 0 .. N: ``acc / m`` plus the source term at the source nodes; also returns
    the sources' unique storage nodes. ``source_rows = (rows, sacc)`` (off-grid sources): the source
    term is ``sacc[p] / (m[p] G[p])`` at the unique rows p instead, sacc the time sums of ``rows_dot``."""
    gm = acc[ghost:N + 1 + ghost] / m[ghost:N + 1 + ghost]
    if source_rows is not None:
        rows, sacc = source_rows
        n = rows.unique
        i, j, k = (v[:n] for v in rows.ijk())
        G = 1.0 if tt is None else tt[0][i] * (tt[1][j] * tt[2][k])
        gm[i - ghost, j, k] = gm[i - ghost, j, k] + sacc[:n] / (m[i, j, k] * G)
        return gm, []
    nodes = source_unique_nodes(sources, N, ghost)
    if nodes:
        dots = (a * g).sum(0)
        for s, nd in enumerate(nodes):
            at = (nd[0] - ghost, nd[1], nd[2])
            gm[at] = gm[at] + dots[s] / (m[nd] * taper_at(tt, nd))
    return gm, nodes


def _unique_node_convention(grad, N: int):
    """In place: plane N a copy of plane 0, the Dirichlet faces 0."""
    grad[N] = grad[0]
    grad[:, 0, :] = 0
    grad[:, N, :] = 0
    grad[:, :, 0] = 0
    grad[:, :, N] = 0
    return grad


def finish_gradient_medium(acc, a, g, m, tt, sources, N: int, tau: float, hx: float, hy: float, hz: float,
                           ghost: int = 1, density=None, source_rows=None):
    """The host-side end of the gradient. acc ``[N+1+2 ghost][N+1][N+1]`` = sum mu^{n+1} q^n in storage
    (faces 0), a ``[K, S]`` with ``a[n, s] = mu^{n+1}[x_s]``, g = the ``source_table``, m = the
    ``medium_coefficient``, all CPU tensors of the working dtype. Returns (dJ/dspeed2 ``(N+1)^3``
    with respect to the unique nodes: plane N a copy of plane 0, faces 0; dJ/dwavelet ``[K, S]``).
    ``density`` (a scalar or ``(N+1)^3``): m = rho speed2 tau^2, so the gradient is multiplied by rho as
    its last arithmetic operation: dJ/dspeed2 at fixed rho.
    ``source_rows = (rows, sacc)``: off-grid sources. ``a[n, s]`` is then the weighted gather
    ``sum_p W[p, s] mu^{n+1}[p] / G[p]`` (``receiver_tables(over_taper=tt)``), so dJ/dwavelet only divides
    it by ``hx hy hz``, and the source term of dJ/dm comes from ``sacc`` (``_gradient_wrt_m``)."""
    gm, nodes = _gradient_wrt_m(acc, a, g, m, tt, sources, N, ghost, source_rows)
    grad = (gm * tau) * tau  # m = (speed2 tau) tau
    if density is not None:
        grad = grad * _node_field(density, N, "density").to(grad.dtype)
    _unique_node_convention(grad, N)
    gw = torch.zeros_like(a) if source_rows is None else a / (hx * hy * hz)
    for s, nd in enumerate(nodes):
        gw[:, s] = a[:, s] / taper_at(tt, nd) / (hx * hy * hz)
    if gw.shape[0] > 0:
        gw[0] = gw[0] * 0.5
    return grad, gw


def finish_gradient_density(acc, accb, a, g, m, tt, sources, N: int, tau: float, speed2, density,
                            ghost: int = 1, source_rows=None):
    """The host-side end of the density gradient, shared by both backends. acc, a, g, m, tt, sources as
    in ``finish_gradient_medium``; accb ``[N+1+2 ghost][N+1][N+1]`` = sum_{n=K-1..1} C(mu^{n+1}, u^n)
    (``face_correlation``) in storage. rho enters the step through ``m = rho speed2 tau^2`` and through
    the buoyancy ``b = 1 / rho`` of ``laplace_density``; with gm = dJ/dm, in the working dtype and with
    rho and speed2 cast to it:

        dJ/drho = ((gm tau) tau) speed2 + (0.5 accb) / (rho rho)

    at fixed speed2. Returns it as ``(N+1)^3`` with respect to the densities of the stencil nodes, the
    unique x planes and j, k in 1 .. N-1: plane N a copy of plane 0 and the Dirichlet faces 0 (the wall
    nodes' densities do enter the adjacent half-face averages; they are held fixed and reported as 0,
    like the faces of dJ/dspeed2, which keeps the accumulation on ``step_medium``'s box)."""
    gm, _ = _gradient_wrt_m(acc, a, g, m, tt, sources, N, ghost, source_rows)
    rho = _node_field(density, N, "density").to(gm.dtype)
    part1 = ((gm * tau) * tau) * _node_field(speed2, N, "speed2").to(gm.dtype)
    part2 = (0.5 * accb[ghost:N + 1 + ghost]) / (rho * rho)
    return _unique_node_convention(part1 + part2, N)


def finish_illumination(h, tt, N: int, tau: float, ghost: int = 1, density=None):
    """The host-side end of the source illumination, shared by both backends. h
    ``[N+1+2 ghost][N+1][N+1]`` = sum_{n=1..K-1} q^n q^n in storage, a CPU tensor of the working dtype;
    tt = the ``taper_tables`` (None: G = 1). Returns (illumination, pseudo_hessian_speed2), both
    ``(N+1)^3`` in the convention of dJ/dspeed2 (plane N a copy of plane 0, the Dirichlet faces 0).

    The Born step injects ``G dm q^n`` for a perturbation of speed2 at a node, ``dm = rho tau^2 dspeed2``
    (rho = 1 without a density), so the diagonal of Shin's pseudo-Hessian for speed2 is
    ``illumination * (w * w)`` with ``w = (G tau) tau [rho]``, G = gx[i] (gy[j] gz[k]) rounded like
    ``step_medium``, every operation in the working dtype. The source term of dJ/dm at the source nodes
    is not part of it."""
    illum = h[ghost:N + 1 + ghost].clone()
    if tt is None:
        G = torch.ones((), dtype=h.dtype)
    else:
        G = tt[0][ghost:N + 1 + ghost, None, None] * (tt[1][None, :, None] * tt[2][None, None, :])
    w = (G * tau) * tau
    if density is not None:
        w = w * _node_field(density, N, "density").to(h.dtype)
    ph = illum * (w * w)
    return _unique_node_convention(illum, N), _unique_node_convention(ph, N)


def _adjoint_medium(N: int, K: int, speed2, observed, *, sources, wavelet, receivers, taper, L, T, pi, dtype,
                    order: int, density, wrt_density: bool, illumination: bool = False, source_positions=None,
                    receiver_positions=None, interp: str = "sinc8", dft=None):
    """The forward run and the adjoint loop shared by ``gradient_medium`` and
    ``gradient_medium_density``: everything their host-side ends need, as a dict. ``illumination``: also
    ``h = h + q^n q^n`` over the forward run's q^1 .. q^{K-1} in that order, the product rounded before
    the add, on the stencil nodes in storage (``finish_illumination`` has the rest).

    Off-grid receivers: the residuals ``[K+1, R]`` are injected through ``point_rows(.., tt)``, whose
    weights carry G. Off-grid sources: ``a[n-1, s]`` is the weighted gather of mu^n with the
    ``receiver_tables(over_taper=tt)`` and ``sacc = sacc + mu^n[p] val_p(g[n-1])`` is accumulated per
    unique source row in the loop's order, n = K .. 1 (``rows_dot``).

    ``dft = (frequencies, dft_every)`` (``gradient_medium_dft``): no ``acc``; the spectra of q and mu at the
    indices p = e, 2e, ... <= K - 1 instead, as ``spectra = (Qre, Qim, Mre, Mim)``, lists of F levels in
    storage. q^p goes into Q with the twiddle row p in ascending p, after the forward run; mu^{n+1},
    injected and wrapped, goes into M with the row n before the step that produces mu^n, in the loop's
    descending order (``dft_accumulate`` on the step box)."""
    M0 = _medium_layout(N, order)[0]
    pts = _Points(N, M0, dtype, sources, receivers, source_positions, receiver_positions, interp)
    fwd = forward_medium_autograd(N, K, speed2, wavelet=wavelet, taper=taper, L=L, T=T, pi=pi, dtype=dtype,
                                  keep_lap=True, order=order, density=density, keep_levels=wrt_density, points=pts)
    traces, laps = fwd[0], fwd[1]
    J, res = misfit_medium(traces, observed)
    c = tables(N, K, L, T, pi)[4]
    M, box, mirror = _medium_layout(N, order)
    tt = None if taper is None else taper_tables(taper, N, dtype, M)
    m = medium_coefficient(speed2, c["tau"], N, dtype, M, density)
    bu = _buoyancy(density, N, dtype, order, M)
    g = source_table(wavelet, K, pts.S, c["hx"], c["hy"], c["hz"], dtype)
    arows = gtab = sacc = None
    anodes, atab, snodes = [], None, []
    if pts.rpos is None:
        anodes, atab = adjoint_source_table(res, receivers, N, tt, M)
    else:
        arows = point_rows(pts.rpos, N, dtype, interp, M, tt)
    if pts.spos is None:
        snodes = source_unique_nodes(sources, N, M)
    else:
        gtab = receiver_tables(pts.spos, N, dtype, interp, M, over_taper=tt)
        sacc = torch.zeros(pts.rows.unique, dtype=dtype)
    shape = (N + 1 + 2 * M, N + 1, N + 1)
    own = (slice(M, N + 1 + M), slice(1, N), slice(1, N))
    a = torch.zeros(K, pts.S, dtype=dtype)
    h = None
    if illumination:  # ascending n, the q^n the adjoint loop correlates with mu^{n+1}
        h = torch.zeros(shape, dtype=dtype)
        for q in laps:
            h[own] = h[own] + q * q

    def finish_level(mu, n):  # inject G rho^n, wrap, sample mu^n at the sources
        nonlocal sacc
        if arows is not None:
            inject_rows(mu, m, arows, res[n])
        for e, nd in enumerate(anodes):
            mu[nd] = mu[nd] + m[nd] * atab[n, e]
        _wrap_x(mu, N, M)
        if gtab is not None:
            a[n - 1] = record_weighted(mu, *gtab)
            sacc = rows_dot(mu, pts.rows, g[n - 1], sacc)
        for s, nd in enumerate(snodes):
            a[n - 1, s] = mu[nd]

    spectra = None
    if dft is not None:
        every = check_dft_every(dft[1])
        ctab, stab = dft_tables(dft[0], range(K), c["tau"], dtype)
        spectra = tuple([torch.zeros(shape, dtype=dtype) for _ in range(ctab.shape[1])] for _ in range(4))
        ql = torch.zeros(shape, dtype=dtype)
        for p in range(every, K, every):  # q^p = laps[p - 1], what forward step p + 1 used
            ql[own] = laps[p - 1]
            dft_accumulate(spectra[0], spectra[1], ql, box, ctab[p], stab[p])

    mu2 = torch.zeros(shape, dtype=dtype)
    mu1 = torch.zeros(shape, dtype=dtype)
    finish_level(mu1, K)
    acc = torch.zeros(shape, dtype=dtype) if dft is None else None
    accb = torch.zeros(shape, dtype=dtype) if wrt_density else None
    for n in range(K - 1, 0, -1):
        vals = step_medium(mu1, mu2, m, box, first=False, hx2=c["hx2"], hy2=c["hy2"], hz2=c["hz2"], taper=tt,
                           order=order, mirror=mirror, buoyancy=bu)
        if dft is None:
            acc[own] = acc[own] + mu1[own] * laps[n - 1]
        elif n % every == 0:
            dft_accumulate(spectra[2], spectra[3], mu1, box, ctab[n], stab[n])
        if wrt_density:  # mu1 = mu^{n+1}, injected and wrapped; fwd[2][n - 1] = u^n
            accb[own] = accb[own] + face_correlation(mu1, fwd[2][n - 1], box, c["hx2"], c["hy2"], c["hz2"])
        mu = torch.zeros(shape, dtype=dtype)
        mu[own] = vals
        finish_level(mu, n)
        mu2, mu1 = mu1, mu
    return dict(J=J, traces=traces, acc=acc, accb=accb, a=a, g=g, m=m, tt=tt, c=c, M=M, h=h, spectra=spectra,
                source_rows=None if gtab is None else (pts.rows, sacc))


def gradient_medium(N: int, K: int, speed2, observed, *, sources=(), wavelet=None, receivers=(), taper=None,
                    L=("pi", "pi", "pi"), T: float = 1.0, pi: str = "ref", dtype=torch.float64, order: int = 2,
                    density=None, illumination: bool = False, source_positions=None, receiver_positions=None,
                    interp: str = "sinc8"):
    """Misfit J of the traces against ``observed`` ``[K+1, R]`` (row 0 ignored) and its gradients by
    the hand-written adjoint above: (J, dJ/dspeed2 ``(N+1)^3``, dJ/dwavelet ``[K, S]``, traces).

    The adjoint field runs on ``step_medium(first=False)`` itself, each step followed by the
    injection of ``G rho``; ``acc = acc + mu q`` is accumulated for n = K-1 .. 1 in that order.
    dJ/dspeed2 is taken with respect to the unique nodes: entry [0] is the derivative with respect
    to the shared value of planes 0 and N (autograd's ``g[0] + g[N]`` for an ``(N+1)^3`` leaf) and
    entry [N] a copy of it; for a periodic perturbation d the directional derivative is
    ``(grad[:N] * d[:N]).sum()``.

    order: the space order of ``solve_medium``; the star Laplacian with periodic wrap and odd
    reflection is symmetric on the unique nodes, so the adjoint recurrence keeps its form.

    density: rho of ``solve_medium`` (order 2), held fixed: ``laplace_density`` is symmetric on the
    unique nodes too, so the adjoint field runs on the same density step, and dJ/dspeed2 is the
    derivative at fixed rho (``finish_gradient_medium``). dJ/drho: ``gradient_medium_density``.

    illumination: two more results, (source illumination, pseudo-Hessian diagonal for speed2), both
    ``(N+1)^3`` (``finish_illumination``): sum_{n=1..K-1} q^n q^n over the q^n above, added in ascending
    n, the product rounded before the add. The other results do not change.

    source_positions / receiver_positions / interp: off-grid points as in ``solve_medium``. With W the
    row weights, ``dJ/dg[n, s] = sum_p W[p, s] mu^{n+1}[p] / G[p]`` and the source term of dJ/dm at a touched
    node p is ``(sum_n mu^{n+1}[p] val_p(g[n])) / (m[p] G[p])`` (``_adjoint_medium``)."""
    with torch.no_grad():
        r = _adjoint_medium(N, K, speed2, observed, sources=sources, wavelet=wavelet, receivers=receivers,
                            taper=taper, L=L, T=T, pi=pi, dtype=dtype, order=order, density=density,
                            wrt_density=False, illumination=illumination, source_positions=source_positions,
                            receiver_positions=receiver_positions, interp=interp)
        c = r["c"]
        grad, gw = finish_gradient_medium(r["acc"], r["a"], r["g"], r["m"], r["tt"], sources, N, c["tau"], c["hx"],
                                          c["hy"], c["hz"], r["M"], density, r["source_rows"])
        out = (r["J"], grad, gw, r["traces"])
        if illumination:
            out += finish_illumination(r["h"], r["tt"], N, c["tau"], r["M"], density)
        return out


def gradient_medium_dft(N: int, K: int, speed2, observed, frequencies, *, weights=None, dft_every: int = 1,
                        sources=(), wavelet=None, receivers=(), taper=None, L=("pi", "pi", "pi"), T: float = 1.0,
                        pi: str = "ref", dtype=torch.float64, order: int = 2, density=None, source_positions=None,
                        receiver_positions=None, interp: str = "sinc8"):
    """``gradient_medium`` with the time sum ``sum_n mu^{n+1} q^n`` replaced by a sum over frequencies of the
    on-the-fly spectra of q and mu: (J, dJ/dspeed2, dJ/dwavelet, traces), J, dJ/dwavelet and the traces
    those of ``gradient_medium`` bit for bit.

    With e = ``dft_every`` the pairs p = e, 2e, ... <= K - 1 are transformed: Q_f = sum_p q^p w_p and
    M_f = sum_p mu^{p+1} w_p with w_p = exp(-i 2 pi f p tau) (``_adjoint_medium``'s ``dft``), and
    ``acc = sum_f weights_f (Re Q_f Re M_f + Im Q_f Im M_f)`` (``finish_gradient_dft``) goes through
    ``finish_gradient_medium`` unchanged. With every bin of the half spectrum of the P = (K - 1) // e pairs,
    f_k = k / (P e tau) for k = 0 .. P // 2 and the weights 2 / P (1 / P for k = 0 and, P even, k = P / 2),
    Parseval's identity makes ``acc`` the time sum over those pairs up to rounding: ``gradient_medium``'s
    for e = 1. Fewer bins give the band-limited gradient. Neither pass keeps a level of the other: the
    memory is that of 4 F levels whatever K is."""
    f = check_frequencies(frequencies)
    every = check_dft_every(dft_every)
    if every > K - 1:
        raise ValueError(f"dft_every = {every} leaves no pair to correlate: the pairs are p = e, 2e, ... <= K - 1 = "
                         f"{K - 1}")
    with torch.no_grad():
        r = _adjoint_medium(N, K, speed2, observed, sources=sources, wavelet=wavelet, receivers=receivers,
                            taper=taper, L=L, T=T, pi=pi, dtype=dtype, order=order, density=density,
                            wrt_density=False, source_positions=source_positions,
                            receiver_positions=receiver_positions, interp=interp, dft=(f, every))
        c = r["c"]
        acc = finish_gradient_dft(*r["spectra"], weights, dtype)
        grad, gw = finish_gradient_medium(acc, r["a"], r["g"], r["m"], r["tt"], sources, N, c["tau"], c["hx"],
                                          c["hy"], c["hz"], r["M"], density, r["source_rows"])
        return r["J"], grad, gw, r["traces"]


def gradient_medium_density(N: int, K: int, speed2, observed, *, sources=(), wavelet=None, receivers=(), taper=None,
                            L=("pi", "pi", "pi"), T: float = 1.0, pi: str = "ref", dtype=torch.float64,
                            order: int = 2, density=None, illumination: bool = False, source_positions=None,
                            receiver_positions=None, interp: str = "sinc8"):
    """``gradient_medium`` of a problem with a ``density`` (required; order 2), plus the gradient with
    respect to it: (J, dJ/dspeed2 at fixed rho, dJ/dwavelet, traces, dJ/drho at fixed speed2). The
    first four are those of ``gradient_medium`` bit for bit. ``illumination``: ``gradient_medium``'s two
    more results, after the five.

    Beside ``acc`` the adjoint loop accumulates ``accb = accb + C(mu^{n+1}, u^n)`` (``face_correlation``)
    for n = K-1 .. 1 in that order, mu^{n+1} injected and wrapped; by summation by parts (mu is 0 on
    the Dirichlet faces and x is periodic) ``dJ/db_l = -accb_l / 2``. ``finish_gradient_density`` has the
    rest and the face convention: the derivative with respect to the densities of the stencil nodes,
    entry [0] for the shared value of planes 0 and N (autograd's ``g[0] + g[N]`` for a density leaf),
    the Dirichlet faces reported as 0. Other parametrisations follow by the chain rule from the pair
    (dJ/dspeed2 at fixed rho, dJ/drho at fixed speed2)."""
    if density is None:
        raise ValueError("gradient_medium_density needs a density (a scalar or an (N+1)^3 field)")
    with torch.no_grad():
        r = _adjoint_medium(N, K, speed2, observed, sources=sources, wavelet=wavelet, receivers=receivers,
                            taper=taper, L=L, T=T, pi=pi, dtype=dtype, order=order, density=density,
                            wrt_density=True, illumination=illumination, source_positions=source_positions,
                            receiver_positions=receiver_positions, interp=interp)
        c = r["c"]
        grad, gw = finish_gradient_medium(r["acc"], r["a"], r["g"], r["m"], r["tt"], sources, N, c["tau"], c["hx"],
                                          c["hy"], c["hz"], r["M"], density, r["source_rows"])
        gd = finish_gradient_density(r["acc"], r["accb"], r["a"], r["g"], r["m"], r["tt"], sources, N, c["tau"],
                                     speed2, density, r["M"], r["source_rows"])
        out = (r["J"], grad, gw, r["traces"], gd)
        if illumination:
            out += finish_illumination(r["h"], r["tt"], N, c["tau"], r["M"], density)
        return out


# ---- Born (linearised) modelling of the medium solver ---------------------------------------
#
# The Jacobian itself, where the adjoint above is its transpose. With the forward scheme
#   u^1 = m g[0] e_s,   u^n = G ((2 u^{n-1} - G u^{n-2}) + m L u^{n-1}) + m g[n-1] e_s,
# a perturbation ds of speed2 at fixed density changes m by dm = medium_coefficient(ds, ...) (m is
# linear in speed2) and a perturbation dw of the wavelet changes g by dg = source_table(dw, ...).
# To first order, with q^{n-1} = L u^{n-1} (q^0 = 0 from rest),
#   du^1 = dm g[0] e_s + m dg[0] e_s,
#   du^n = G (((2 du^{n-1} - G du^{n-2}) + m L du^{n-1}) + dm q^{n-1}) + dm g[n-1] e_s + m dg[n-1] e_s:
# the forward step on du with the scattering term dm q inside the sponge factor (step_medium's
# ``born``) and the perturbed source terms outside, like the source term itself. dtraces[n, r] =
# du^n[x_r] is the directional derivative of the traces, and for any r [K+1, R]
#   (dtraces[1:] * r[1:]).sum() == (grad_speed2[:N] * ds[:N]).sum() + (grad_wavelet * dw).sum()
# with the gradients of gradient_medium(observed = traces - r), in exact arithmetic.
#
# A perturbation drho of the density at fixed speed2 changes the step in two places: m = rho c^2 tau^2 by
# dm_rho = medium_coefficient(speed2, density=drho) (added to the dm above in the working dtype; one
# term alone is used as it is), and the buoyancy b = 1 / rho by db = -drho / rho^2 (dbuoyancy_field).
# D_b is linear in b, so with r^{n-1} = D_db u^{n-1} (laplace_density with db in b's place) the
# scattering term becomes s^{n-1} = dm q^{n-1} + m r^{n-1}, both products rounded, then the add, and
#   du^n = G (((2 du^{n-1} - G du^{n-2}) + m D_b du^{n-1}) + s^{n-1}) + dm g[n-1] e_s + m dg[n-1] e_s
# (step_medium's ``born_add``); du^1 has no db term, u^0 being 0. The wall nodes' db enters the
# adjacent half-face averages exactly as their b does, so dtraces is the true directional derivative
# for any drho. gradient_medium_density holds the wall densities fixed and reports 0 there, so the
# adjoint identity gains the term (grad_density[:N] * drho[:N]).sum() for drho that vanishes on the
# y/z faces.

def perturbation_field(v, N: int, name: str) -> torch.Tensor:
    """A model perturbation as a float64 CPU tensor: a scalar or ``(N+1)^3``, finite, of any sign,
    periodic in x."""
    s = torch.as_tensor(v, dtype=torch.float64).cpu()
    n1 = N + 1
    if s.dim() != 0 and tuple(s.shape) != (n1, n1, n1):
        raise ValueError(f"{name} must be a scalar or have shape {(n1, n1, n1)}, not {tuple(s.shape)}")
    bad = ~torch.isfinite(s)
    if bool(bad.any()):
        v = s[bad].flatten()[0].item() if s.dim() else s.item()
        raise ValueError(f"{name} must be finite, found {v}")
    if s.dim() != 0 and not torch.equal(s[0], s[N]):
        j, k = (int(x) for x in (s[0] != s[N]).nonzero()[0])
        raise ValueError(f"{name} must be periodic in x: {name}[0,{j},{k}] = {s[0, j, k].item()} but "
                         f"{name}[{N},{j},{k}] = {s[N, j, k].item()}")
    return s


def born_medium(N: int, K: int, speed2, dspeed2=None, dwavelet=None, *, sources=(), wavelet=None, receivers=(),
                taper=None, L=("pi", "pi", "pi"), T: float = 1.0, pi: str = "ref", dtype=torch.float64,
                order: int = 2, density=None, ddensity=None, source_positions=None, receiver_positions=None,
                interp: str = "sinc8"):
    """Born modelling from rest: ``solve_medium``'s run and, in lock step, the first-order change of
    its field for the perturbations ``dspeed2`` of speed2 (a scalar or ``(N+1)^3``, finite, periodic
    in x, of any sign; the density stays fixed), ``dwavelet`` ``[K, S]`` of the wavelet and ``ddensity``
    of the density (like ``dspeed2``, at fixed speed2, wall nodes included; needs ``density``); at
    least one of the three. Returns (traces ``[K+1, R]``, those of ``solve_medium`` bit for bit; dtraces
    ``[K+1, R]``, row 0 zero; du^K ``(N+1)^3``; max |du| per layer ``[K+1]`` like ``solve_medium``'s).

    Per step: the background step, the Born step ``step_medium(born=(q, dm))`` with q the Laplacian
    of the background level it started from, then per source node ``du += dm g[n-1, s]`` and
    ``du += m dg[n-1, s]`` (each a rounded product, then the add), the wrap, the sample. Step 1 has
    no Born term. With ``ddensity`` the Born step is ``step_medium(born_add=s)`` with
    ``s = dm q + m r``, r = ``laplace_density`` of the same background level with the buoyancy
    perturbation in b's place; without it every operation is the one above.
    ``source_positions`` / ``receiver_positions`` / ``interp``: off-grid points as in ``solve_medium``; the
    perturbed source terms are then ``inject_rows`` with dm and g, and with m and dg."""
    if dspeed2 is None and dwavelet is None and ddensity is None:
        raise ValueError("born_medium needs a perturbation: dspeed2, dwavelet, ddensity or any of them together")
    if ddensity is not None and density is None:
        raise ValueError("ddensity needs a density model: density=... (a scalar such as 1.0 is fine)")
    c = tables(N, K, L, T, pi)[4]
    M, box, mirror = _medium_layout(N, order)
    tt = None if taper is None else taper_tables(taper, N, dtype, M)
    m = medium_coefficient(speed2, c["tau"], N, dtype, M, density)
    if dspeed2 is None:
        dm = torch.zeros_like(m)
    else:
        dm = medium_coefficient(perturbation_field(dspeed2, N, "dspeed2"), c["tau"], N, dtype, M, density)
    bu = _buoyancy(density, N, dtype, order, M)
    db = None
    if ddensity is not None:
        dr = perturbation_field(ddensity, N, "ddensity")
        dmr = medium_coefficient(speed2, c["tau"], N, dtype, M, dr)
        dm = dmr if dspeed2 is None else dm + dmr
        db = dbuoyancy_field(dr, density, N, dtype, M)
    pts = _Points(N, M, dtype, sources, receivers, source_positions, receiver_positions, interp)
    S = pts.S
    g = source_table(wavelet, K, S, c["hx"], c["hy"], c["hz"], dtype)
    dg = None
    if dwavelet is not None:
        dw = torch.as_tensor(dwavelet, dtype=torch.float64)
        if tuple(dw.shape) != (K, S):
            raise ValueError(f"dwavelet must have shape {(K, S)} (timesteps x sources), not {tuple(dw.shape)}")
        dg = source_table(dw, K, S, c["hx"], c["hy"], c["hz"], dtype)
    shape = (N + 1 + 2 * M, N + 1, N + 1)
    own = (slice(M, N + 1 + M), slice(1, N), slice(1, N))
    lv = [torch.zeros(shape, dtype=dtype) for _ in range(3)]
    dl = [torch.zeros(shape, dtype=dtype) for _ in range(3)]
    traces = torch.zeros(K + 1, pts.R, dtype=dtype)
    dtraces = torch.zeros(K + 1, pts.R, dtype=dtype)
    kw = dict(hx2=c["hx2"], hy2=c["hy2"], hz2=c["hz2"], taper=tt, order=order, mirror=mirror, buoyancy=bu)
    mx = [0.0]  # du^0 = 0
    for n in range(1, K + 1):
        u1, u2, u = lv[(n + 2) % 3], lv[(n + 1) % 3], lv[n % 3]
        d1, d2, d = dl[(n + 2) % 3], dl[(n + 1) % 3], dl[n % 3]
        q = _lap_box(u1, box, c["hx2"], c["hy2"], c["hz2"], order, mirror, bu) if n >= 2 else None
        u.zero_()
        u[own] = step_medium(u1, u2, m, box, first=n == 1, **kw)
        pts.inject(u, m, g[n - 1])
        _wrap_x(u, N, M)
        if db is None or n == 1:
            dvals = step_medium(d1, d2, m, box, first=n == 1, born=None if n == 1 else (q, dm), **kw)
        else:  # q and r of the level u1 the background step above started from
            r = _lap_box(u1, box, c["hx2"], c["hy2"], c["hz2"], order, mirror, db)
            dvals = step_medium(d1, d2, m, box, first=False, born_add=dm[own] * q + m[own] * r, **kw)
        mx.append(max_abs_field(dvals))
        d.zero_()
        d[own] = dvals
        if pts.rows is not None:
            inject_rows(d, dm, pts.rows, g[n - 1])
            if dg is not None:
                inject_rows(d, m, pts.rows, dg[n - 1])
        else:
            for nd, s in pts.ent:
                d[nd] = d[nd] + dm[nd] * g[n - 1, s]
                if dg is not None:
                    d[nd] = d[nd] + m[nd] * dg[n - 1, s]
        _wrap_x(d, N, M)
        traces[n] = pts.sample(u)
        dtraces[n] = pts.sample(d)
    return traces, dtraces, dl[K % 3][M:N + 1 + M].clone(), mx
