"""The FMA-form oracle (ops/reference.py: ``fma``, ``chained_layers_fma``, ``chained_delta_layers_fma``,
``solve(math="fma")``) checked without a GPU:

* ``fma`` against exact rational arithmetic, float64 and float32, on uniform operands, on ``c = -RN(ab)``
  cancellation, on addends up to 2^59 times larger or smaller than the product, and on exact ties of
  the final rounding;
* whole FMA-form solves against the OpenMP ``cpu`` backend with ``math="fma"``, final field and
  per-layer maxima bit for bit, both types and both schemes;
* sensitivity on the very inputs of the GPU kernel tests (tests/test_gpu_tb_kernels.py): a subtly
  different arithmetic changes bits inside the boxes while staying inside the tolerance those tests
  used to allow, so the bitwise comparison sees what the tolerance let through.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

import sweep_cases as sc
from bits import assert_same_bits, round_fraction

P = {torch.float32: 24, torch.float64: 53}
EMIN = {torch.float32: -126, torch.float64: -1022}
SAMPLES = 10000


def _exact(t: torch.Tensor) -> list:
    return [Fraction(v) for v in t.double().tolist()]  # float -> Fraction is exact; fp32 -> fp64 too


def _family(name: str, dtype, n: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    r = lambda: (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1)  # noqa: E731
    p = P[dtype]
    a, b = r().to(dtype), r().to(dtype)
    if name == "uniform":
        c = r().to(dtype)
    elif name == "cancel":
        c = -(a * b)
    elif name == "exponents":
        k = torch.randint(-59, 60, (n,), generator=g)
        c = torch.ldexp((a * b).double() * (1 + r().abs()), k).to(dtype)
    else:
        raise AssertionError(name)
    return a, b, c


def _ties(dtype, n: int, g):
    """Exact ties of the final rounding: a = an odd integer A below 2^(p-2), either sign, b = 1/2, and
    c = an integer C of either sign and parity with 2^(p-1) <= |C| < 2^(p-1) + 2^(p-2). Then a b + c =
    C + A/2 is a half-integer between two p-bit integers: a tie, to be broken to even."""
    p = P[dtype]
    A = torch.randint(0, 2 ** (p - 3), (n,), generator=g) * 2 + 1
    Cm = torch.randint(2 ** (p - 1), 2 ** (p - 1) + 2 ** (p - 2), (n,), generator=g)
    sa = torch.randint(0, 2, (n,), generator=g) * 2 - 1
    sc_ = torch.randint(0, 2, (n,), generator=g) * 2 - 1
    a = (A * sa).to(torch.float64).to(dtype)
    b = torch.full((n,), 0.5, dtype=dtype)
    c = (Cm * sc_).to(torch.float64).to(dtype)
    return a, b, c


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("family", ["uniform", "cancel", "exponents", "ties"])
def test_fma_against_rationals(dtype, family):
    """``reference.fma`` equals the exact rational ``a b + c`` rounded once to p bits, on 10,000 samples per
    family; the unfused ``a * b + c`` does not (counted: it must differ somewhere in every family but the
    one where the product is exact)."""
    from wave3d.ops import reference

    g = torch.Generator().manual_seed(7)
    a, b, c = _ties(dtype, SAMPLES, g) if family == "ties" else _family(family, dtype, SAMPLES, 11)
    got = reference.fma(a, b, c)
    p, emin = P[dtype], EMIN[dtype]
    exp = [round_fraction(x * y + z, p, emin) for x, y, z in zip(_exact(a), _exact(b), _exact(c))]
    if family == "ties":  # the cases are ties: the exact sum is half-way between two p-bit numbers
        x, y, z = _exact(a)[0], _exact(b)[0], _exact(c)[0]
        s = x * y + z
        assert (s * 2).denominator == 1 and s.denominator == 2 and abs(s) >= 2 ** (p - 1)
    want = torch.tensor([float(v) for v in exp], dtype=torch.float64).to(dtype)  # exact: p-bit values
    assert [Fraction(v) for v in want.double().tolist()] == exp
    assert_same_bits(got, want, f"fma {family} {dtype}")
    plain = a * b + c
    differ = int((plain != want).sum())
    if family in ("uniform", "cancel"):
        assert differ > SAMPLES // 10, differ  # the unfused form is another function


def test_fma_special_values():
    from wave3d.ops import reference

    inf, nan = float("inf"), float("nan")
    for dtype in (torch.float64, torch.float32):
        t = lambda *v: torch.tensor(v, dtype=dtype)  # noqa: E731
        got = reference.fma(t(0.0, 2.0, inf, 0.0, nan, 1.5, -0.0), t(3.0, 0.0, 0.0, inf, 1.0, 2.0, 5.0),
                            t(-0.0, 7.0, 1.0, 1.0, 1.0, inf, -0.0))
        assert_same_bits(got, t(0.0, 7.0, nan, nan, nan, inf, -0.0))


@pytest.mark.parametrize("dtype,name", [(torch.float64, "fp64"), (torch.float32, "fp32")])
@pytest.mark.parametrize("scheme", ["leapfrog", "delta"])
def test_solve_fma_equals_cpu_backend(C, dtype, name, scheme):
    """``reference.solve(math="fma")``: the final field and the per-layer maxima of the OpenMP oracle with
    ``math="fma"``, bit for bit (shifted initial condition, non-cubic lengths, small N). In these runs
    the FMA and the exact fields differ, so the comparison tells the two forms apart."""
    import wave3d
    from wave3d.ops import reference

    N, K = 14, 7
    p = wave3d.WaveProblem(N, Lx=1.3, Ly="pi", Lz=2.0, timesteps=K, ic="shifted", dtype=name, scheme=scheme, math="fma")
    res, field = wave3d.WaveSolver(p, "cpu", threads=2).solve_field()
    a, r, uK = reference.solve(N, K, L=(1.3, "pi", 2.0), phase=0.7, dtype=dtype, scheme=scheme, math="fma")
    got = torch.from_numpy(np.ascontiguousarray(field))
    assert_same_bits(got, uK[1:N + 2].double(), f"final field {name} {scheme}")  # (fp32 fields come back widened)
    assert res.max_abs == [float(v) for v in a]
    assert res.max_rel == [float(v) for v in r]
    _, _, uE = reference.solve(N, K, L=(1.3, "pi", 2.0), phase=0.7, dtype=dtype, scheme=scheme)
    assert int((uE != uK).sum()) > 100


# ---- sensitivity on the inputs of the GPU kernel tests -------------------------------------------

def _changed(exp, var, boxes, G):
    n = 0
    for b in boxes:
        s = sc.sl(b, G)
        for e, v in zip(exp, var):
            n += int((e[s] != v[s]).sum())
    return n


def _inside_old_tolerance(exp, var, boxes, G, dtype, kind):
    t32 = 2e-5 if kind == "tb3" else 4e-5
    tol = dict(rtol=1e-12, atol=1e-12) if dtype == torch.float64 else dict(rtol=t32, atol=t32)
    for b in boxes:
        s = sc.sl(b, G)
        for e, v in zip(exp, var):
            torch.testing.assert_close(v[s], e[s], **tol)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("kind,variant", [(k, v) for k in ("tb3", "tbn4", "tbn4_delta") for v in ("unfused", "swap", "fold2c")
                                          if (k, v) != ("tbn4_delta", "fold2c")])  # no leapfrog chain to fold there
def test_variants_change_bits_inside_the_old_tolerance(dtype, first, variant, kind):
    """On every case of the GPU kernel tests, each of these changes the stored layers inside the boxes
    and still passes the tolerance those tests had (1e-12 in fp64; 2e-5 (tb3) / 4e-5 (tbn) in fp32): (a) every fma
    unfused, (b) the fp32 composition on fp64 data and the reverse, (c) the rejected chain with 2c
    folded into kc (it rewrites the leapfrog only: the increment form has none, and a first sweep's
    layer 0 is the Taylor start).

    Changed stored values, summed over the cases, of 141,568 (tb3) / 332,340 (tbn4) compared; columns:
    fp64 leapfrog sweep, fp64 first sweep, fp32 leapfrog sweep, fp32 first sweep (measured on the CPU):

        tb3        unfused   24,213   18,748   12,915    8,082
        tb3        swap      27,432   17,758   35,845   24,563
        tb3        fold2c   100,179   81,444   95,668   83,045
        tbn4       unfused   75,840   66,686   44,676   22,000
        tbn4       swap      87,138   60,239  113,635   88,284
        tbn4       fold2c   270,307  257,813  256,494  251,215
        tbn4_delta unfused   67,795   69,433   66,725   69,244
        tbn4_delta swap      92,831   93,419   97,613   97,749

    The smallest share in any single case is 6 % (tb3, fp32, first sweep, unfused); the floor asserted
    per case is 2 %. (fold2c on fp32 data swaps the fp64 chain in as well: there is no fp32 form of it.)"""
    from wave3d.ops import reference

    cases = sc.CASES if kind == "tb3" else sc.TBN_CASES
    for case in range(len(cases)):
        if kind == "tb3":
            inp = sc.tb3_fma_inputs(case, dtype, first)
        elif kind == "tbn4":
            inp = sc.tbn4_fma_inputs(case, dtype, first)
        else:
            inp = sc.tbn4_delta_fma_inputs(case, dtype, first)
        kw = dict(first=first, mask=inp["mask"], coefs=inp["coefs"], **sc.H2)
        if kind == "tbn4_delta":
            fn = lambda v: (lambda L, d: [d, L[-1]])(*reference.chained_delta_layers_fma(  # noqa: E731
                inp["A"], inp["B"], 4, variant=v, **kw))
        else:
            n = 3 if kind == "tb3" else 4
            fn = lambda v: reference.chained_layers_fma(inp["A"], inp["B"], n, variant=v, **kw)[-2:]  # noqa: E731
        exp, var = fn(None), fn(variant)
        n = _changed(exp, var, inp["boxes"], inp["G"])
        total = 2 * sum(exp[0][sc.sl(b, inp["G"])].numel() for b in inp["boxes"])
        assert n > total // 50, f"{kind} case {case}: only {n} of {total} stored values change"
        _inside_old_tolerance(exp, var, inp["boxes"], inp["G"], dtype, kind)
