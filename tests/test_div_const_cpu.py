"""The range of the kernels' constant division: ``div_const`` (csrc/stencil_math.hpp), compiled for the
host, against true division over every binade of fp32 and fp64 (tests/native/div_const_sweep.cpp).

Figures of the sweep (1e5 random numerators of both signs per binade, h^2 = 0.011, 0.013, 0.017, 2.75):

* inside ``bits.division_range`` no quotient differs from ``a / b``;
* below it, for the three h^2 < 1, quotients differ in the binades 2^-137 .. 2^-109 (fp32: up to 45 % of
  a binade around 2^-131, a few of 1e5 from 2^-114 up, none from 2^-108 on; the promise starts at 2^-101)
  and 2^-1033 .. 2^-1006 (fp64: up to 58 % of a binade; none from 2^-1005 on; the promise starts at
  2^-968), and never by more than **D = 1** unit in the last place of the true quotient;
* above it, from 2^121 (fp32) and 2^1017 (fp64), ``a y`` overflows and the result is NaN for a finite
  quotient (the promise ends at 2^120 and 2^1016 for these h^2);
* h^2 = 2.75 has no differing quotient anywhere: its range reaches the largest finite value, and
  below it the sweep found no mismatch;
* ``-0 -> +0`` (true division: ``-0``), ``+-inf -> NaN`` (true division: ``+-inf``), ``NaN -> NaN``.
"""
import math
import os
import shutil
import subprocess

import pytest
import torch

from bits import division_range

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d-wave-equation-mpi-cuda_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "div_const_sweep.cpp")
H2 = (0.011, 0.013, 0.017, 2.75)  # kH2 of the sweep
GPU_H2 = (0, 1, 2)                # the divisors the GPU tests use: the caveat must show for them
D = 1                             # largest distance to true division outside the range, in ulp
SAMPLES = 100000
DTYPES = {"f32": torch.float32, "f64": torch.float64}


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("div_const") / "div_const_sweep")
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-I", CSRC, SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(SAMPLES)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    binades, special, consts = {}, {}, {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "B":
            binades.setdefault((f[1], int(f[2])), []).append(tuple(int(v) for v in f[3:]))
        elif f[0] == "S":
            special[(f[1], int(f[2]), f[3])] = (f[4], f[5])
        elif f[0] == "H":
            consts[(f[1], int(f[2]))] = (float.fromhex(f[3]), float.fromhex(f[4]))
    return binades, special, consts


EXPONENTS = {"f32": (23, -126, 127), "f64": (52, -1022, 1023)}  # explicit significand bits, emin, emax


def _inside(e, lo, hi, tn):
    """the binade [2^e, 2^(e+1)) lies inside [lo, hi]; the top binade ends at the largest finite value"""
    top = math.ldexp(1.0, e + 1) if e < EXPONENTS[tn][2] else torch.finfo(DTYPES[tn]).max
    return math.ldexp(1.0, e) >= lo and top <= hi


@pytest.mark.parametrize("tn", ["f32", "f64"])
def test_sweep_covers_every_binade_with_the_tests_divisors(sweep, tn):
    binades, _, consts = sweep
    dt = DTYPES[tn]
    mant, emin, emax = EXPONENTS[tn]
    for h, h2 in enumerate(H2):
        b, y = consts[(tn, h)]
        assert b == torch.tensor(h2, dtype=dt).item()
        assert y == (torch.ones((), dtype=dt) / torch.tensor(h2, dtype=dt)).item()
        rows = binades[(tn, h)]
        assert [r[0] for r in rows] == list(range(emin - mant, emax + 1))
        assert all(r[1] >= 100000 for r in rows)


@pytest.mark.parametrize("tn", ["f32", "f64"])
def test_div_const_is_true_division_inside_its_range_and_within_D_outside(sweep, tn):
    binades, _, _ = sweep
    dt = DTYPES[tn]
    for h, h2 in enumerate(H2):
        lo, hi = division_range(dt, h2)
        rows = binades[(tn, h)]
        bad_in = [(e, mism) for e, _, mism, _, _ in rows if _inside(e, lo, hi, tn) and mism]
        assert not bad_in, f"{tn} h2={h2}: mismatches inside [{lo!r}, {hi!r}]: {bad_in[:8]}"
        below = [(e, mism, ulp) for e, _, mism, _, ulp in rows if math.ldexp(1.0, e) < lo and mism]
        above = [(e, mism, nf) for e, _, mism, nf, _ in rows if not _inside(e, lo, hi, tn) and math.ldexp(1.0, e) >= lo
                 and mism]
        print(f"{tn} h2={h2}: range [2^{math.log2(lo):.0f}, {'max' if hi == torch.finfo(dt).max else '2^%.0f' % math.log2(hi)}]; "
              f"below: {len(below)} binades 2^{below[0][0] if below else '-'} .. 2^{below[-1][0] if below else '-'}, "
              f"worst {max((m for _, m, _ in below), default=0)} of {SAMPLES}, "
              f"max ulp {max((u for _, _, u in below), default=0)}; above: first 2^{above[0][0] if above else '-'}, "
              f"{sum(m for _, m, _ in above)} mismatches, {sum(n for _, _, n in above)} of them non-finite")
        # never further than D from true division where both are finite, anywhere
        assert max(ulp for *_, ulp in rows) <= D
        # above the range the only failure is the overflow of a y: NaN (or inf) for a finite quotient
        assert all(m == nf for _, m, nf in above)
        if h in GPU_H2:
            assert below and above, f"{tn} h2={h2}: the sweep sees no mismatch outside the range"
            assert max(u for _, _, u in below) == D  # D is what the sweep finds, not a loose cap
        elif h2 >= 2:
            assert hi == torch.finfo(dt).max and not above


@pytest.mark.parametrize("tn", ["f32", "f64"])
def test_div_const_special_numerators(sweep, tn):
    _, special, _ = sweep
    for h in range(len(H2)):
        got = {name: special[(tn, h, name)] for name in ("+0", "-0", "+inf", "-inf", "nan")}
        assert got == {"+0": ("+0", "+0"), "-0": ("+0", "-0"), "+inf": ("+nan", "+inf"), "-inf": ("+nan", "-inf"),
                       "nan": ("+nan", "+nan")}, (tn, h, got)


def test_division_range_figures():
    assert division_range(torch.float32, 0.011) == (2.0 ** -101, 2.0 ** 120)
    assert division_range(torch.float64, 0.011) == (2.0 ** -968, 2.0 ** 1016)
    assert division_range(torch.float32, 0.017) == (2.0 ** -101, 2.0 ** 121)
    assert division_range(torch.float32, 2.75)[1] == torch.finfo(torch.float32).max
    assert division_range(torch.float32, 1.0)[1] == 2.0 ** 127
    with pytest.raises(ValueError):
        division_range(torch.float32, 0.0)


def test_bits_helpers():
    from bits import assert_same_bits, numerators, spacing, ulp_distance
    from wave3d.ops import reference

    for dt, tiny in ((torch.float32, 2.0 ** -149), (torch.float64, 2.0 ** -1074)):
        a = torch.tensor([0.0, -0.0, tiny, -tiny, 1.0, torch.finfo(dt).tiny, math.inf, -math.inf], dtype=dt)
        b = torch.tensor([-0.0, 0.0, -tiny, 3 * tiny, 1.0 + torch.finfo(dt).eps, torch.finfo(dt).tiny - tiny,
                          torch.finfo(dt).max, math.inf], dtype=dt)
        d = ulp_distance(a, b)
        assert d[:7].tolist() == [0, 0, 2, 4, 1, 1, 1]
        assert d[7].item() == (2 * 0x7F800000 if dt == torch.float32 else 2 ** 63 - 1)
        with pytest.raises(ValueError):
            ulp_distance(a, torch.full_like(a, math.nan))
        assert spacing(torch.tensor([0.0, tiny, 1.0, -1.5, 2.0], dtype=dt)).tolist() == \
            [tiny, tiny, torch.finfo(dt).eps, torch.finfo(dt).eps, 2 * torch.finfo(dt).eps]
        assert_same_bits(torch.tensor([math.nan, -0.0, 1.0], dtype=dt), torch.tensor([math.nan, -0.0, 1.0], dtype=dt))
        with pytest.raises(AssertionError, match="1 of 2 values differ"):
            assert_same_bits(torch.tensor([0.0, 1.0], dtype=dt), torch.tensor([-0.0, 1.0], dtype=dt))
        with pytest.raises(AssertionError, match="in being NaN"):
            assert_same_bits(torch.tensor([math.nan], dtype=dt), torch.tensor([1.0], dtype=dt))
        # the numerators are the oracle's own: dividing and summing them gives its Laplacian back
        g = torch.Generator().manual_seed(5)
        u = (torch.rand((12, 13, 14), generator=g, dtype=torch.float64) - 0.5).to(dt)
        bu = (0.5 + torch.rand((12, 13, 14), generator=g, dtype=torch.float64)).to(dt)
        h2 = [torch.tensor(v, dtype=dt).item() for v in (0.011, 0.013, 0.017)]
        for order, box, mirror, buo in ((2, (1, 10, 1, 11, 1, 12), None, None), (2, (2, 9, 1, 11, 3, 12), None, bu),
                                        (8, (4, 7, 1, 11, 4, 9), (0, 12, None, None), None)):
            (tx, ty, tz), ok = numerators(u, box, h2, order, mirror, buo)
            assert bool(ok.all())
            lap = reference._lap_box(u, box, *h2, order, mirror, buo)
            assert_same_bits(((torch.zeros_like(tx) + tx / h2[0]) + ty / h2[1]) + tz / h2[2], lap)
        (tx, ty, tz), ok = numerators(u, (1, 10, 1, 11, 1, 12), h2, correlate=bu)
        assert_same_bits(((torch.zeros_like(tx) + tx / h2[0]) + ty / h2[1]) + tz / h2[2],
                         reference.face_correlation(u, bu, (1, 10, 1, 11, 1, 12), *h2))
        # a node whose numerators are tiny but not zero is outside the range, its order-one neighbours inside
        u[4:7, 4:7, 4:7] = 0
        u[5, 5, 5] = 2.0 ** -110 if dt == torch.float32 else 2.0 ** -980
        _, ok = numerators(u, (1, 10, 1, 11, 1, 12), h2)
        assert not bool(ok[4, 4, 4]) and int((~ok).sum()) == 1
