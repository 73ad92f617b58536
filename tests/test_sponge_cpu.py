"""Absorbing sponge of the variable-speed medium solver on the CPU: the PyTorch oracle
(ops/reference.py step_medium / solve_medium with ``taper``), ``wave3d.sponge_taper`` and the
front-end's validation.

The scheme is the damped leapfrog u^{n+1} = G ((2 u^n - G u^{n-1}) + m lap u^n) with a separable
G = gx (gy gz): G == 1 is the undamped scheme bit for bit, and a constant G = gamma gives
u^n = gamma^n v^n with v the undamped solution, exactly in floating point for gamma a power of two.
"""
import math

import pytest
import torch

DT = {"fp64": torch.float64, "fp32": torch.float32}


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_ones_are_a_noop(dtype):
    from test_medium_cpu import A, B, K, N, hetero_case
    from wave3d.ops import reference

    speed2, w = hetero_case()
    ones = torch.ones(N + 1, dtype=torch.float64)
    kw = dict(sources=[A], wavelet=w, receivers=[B, (0, 6, 7), (8, 8, 8)], dtype=DT[dtype])
    tr0, uf0, mx0 = reference.solve_medium(N, K, speed2, **kw)
    tr1, uf1, mx1 = reference.solve_medium(N, K, speed2, taper=(ones, ones, ones), **kw)
    assert float(tr0.abs().max()) > 1e-3
    assert torch.equal(tr1, tr0) and torch.equal(uf1, uf0) and mx1 == mx0


def decay_case(dtype):
    """The source-free run of test_uniform_medium_reproduces_constant_speed_oracle (N = 16, K = 20)
    and the two constant tapers of the exact decay law, each with its G per node."""
    import wave3d
    from wave3d.ops import reference

    n, k = 16, 20
    sx, sy, sz, ct, c = reference.tables(n, k, dtype=DT[dtype])
    u0 = reference.analytic(sx, sy, sz, ct[0])
    prob = wave3d.MediumProblem(n, c["a2"], timesteps=k, dtype=dtype)
    full = lambda v: torch.full((n + 1,), v, dtype=torch.float64)  # noqa: E731
    return prob, u0, [((full(0.5), None, None), 0.5), ((full(0.5), full(0.25), full(0.5)), 0.0625)]


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_exact_decay_law(dtype):
    import wave3d

    prob, u0, tapers = decay_case(dtype)
    base = wave3d.MediumSolver(prob, "cpu", u0=u0).run()
    assert float(base.u_final.abs().max()) > 0.1
    for taper, g in tapers:
        res = wave3d.MediumSolver(prob, "cpu", u0=u0, taper=taper).run()
        assert res.u_final.dtype == DT[dtype]
        assert torch.equal(res.u_final, base.u_final * g ** 20)  # 2^-20, 2^-80
        assert res.max_abs_u == [v * g ** n for n, v in enumerate(base.max_abs_u)]


def test_sponge_taper_profile():
    import wave3d

    N, K = 32, 64
    prob = wave3d.MediumProblem(N, 2.25, Lx=4.0, Ly=2.0, Lz=8.0, T=0.5, timesteps=K)
    W, sig, pw = 6, 3.0, 2
    gx, gy, gz = wave3d.sponge_taper(prob, W, sigma_max=sig, power=pw)
    for g in (gx, gy, gz):
        assert g.dtype == torch.float64 and tuple(g.shape) == (N + 1,)
        assert bool((g[W:N - W + 1] == 1).all())
        assert bool(((g > 0) & (g <= 1)).all()) and float(g.min()) < 1
        assert torch.equal(g, g.flip(0)) and g[0] == g[N]
        assert bool((g[1:W + 1] >= g[:W]).all()) and bool((g[:W] < 1).all())
        for q in range(N + 1):
            d = min(q, N - q)
            want = math.exp(-sig * ((W - d) / W) ** pw * prob.tau) if d < W else 1.0
            assert math.isclose(g[q].item(), want, rel_tol=1e-14)
    assert torch.equal(gx, gy) and torch.equal(gx, gz)

    # default sigma_max: two-way travel through the layer at the fastest speed, reflection 0.02
    for pw, refl in ((2, 0.02), (3, 0.001)):
        sig = (pw + 1) * 1.5 * math.log(1 / refl) / (2 * W * (2.0 / N))
        a = wave3d.sponge_taper(prob, W, power=pw, reflection=refl)
        b = wave3d.sponge_taper(prob, W, sigma_max=sig, power=pw)
        for ga, gb in zip(a, b):
            torch.testing.assert_close(ga, gb, rtol=1e-14, atol=0)
    assert torch.equal(wave3d.sponge_taper(prob, W)[0], wave3d.sponge_taper(prob, W, reflection=0.02)[0])

    gx, gy, gz = wave3d.sponge_taper(prob, W, axes="yz")
    assert bool((gx == 1).all()) and float(gy.min()) < 1 and torch.equal(gy, gz)

    with pytest.raises(ValueError, match="width"):
        wave3d.sponge_taper(prob, 0)
    with pytest.raises(ValueError, match="fit"):
        wave3d.sponge_taper(prob, N // 2 + 1)
    g = wave3d.sponge_taper(prob, N // 2)[0]  # 2 width == N is allowed: only the middle node is free
    assert g[N // 2] == 1 and float(g[N // 2 - 1]) < 1 and float(g[N // 2 + 1]) < 1
    for refl in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="reflection"):
            wave3d.sponge_taper(prob, W, reflection=refl)


def test_taper_validation():
    import wave3d

    N = 16
    prob = wave3d.MediumProblem(N, 0.5, timesteps=12)
    ok = torch.linspace(0.5, 1.0, N + 1, dtype=torch.float64)
    sym = torch.minimum(ok, ok.flip(0))
    wave3d.MediumSolver(prob, "cpu", taper=(sym, ok, None))  # accepted
    wave3d.MediumSolver(prob, "cpu", taper=(None, None, None))

    def bad(q, v):
        t = sym.clone()
        t[q] = v
        return t

    cases = [
        ("17 values", (sym[:-1], None, None)),
        ("17 values", (None, torch.ones(N + 2, dtype=torch.float64), None)),
        ("17 values", (None, None, torch.ones(N + 1, 2, dtype=torch.float64))),
        (r"gy\[3\] = 0", (None, bad(3, 0.0), None)),
        (r"gz\[5\] = 1.25", (None, None, bad(5, 1.25))),
        (r"gy\[7\] = nan", (None, bad(7, math.nan), None)),
        (r"gx\[2\] = -0.5", (bad(2, -0.5), None, None)),
        (r"periodic in x: gx\[0\] = 0.5 but gx\[16\] = 0.75", (bad(N, 0.75), None, None)),
    ]
    for match, taper in cases:
        for backend in ("cpu", "hip"):
            with pytest.raises(ValueError, match=match):
                wave3d.MediumSolver(prob, backend, taper=taper)
    with pytest.raises(ValueError, match="gx, gy, gz"):
        wave3d.MediumSolver(prob, "cpu", taper=(sym, ok))


def absorb_traces(N, K, f0, off, dtype, backend, width, sigma_max):
    """One Ricker shot at the centre of a box of N unit cells (h = 1, c = 1, tau = 0.5), heard
    ``off`` nodes away along j: (trace without sponge, trace with sponge)."""
    import wave3d

    prob = wave3d.MediumProblem(N, 1.0, Lx=N, Ly=N, Lz=N, T=K / 2, timesteps=K, dtype=dtype)
    w = wave3d.ricker(f0, 1.2 / f0, K, prob.tau).reshape(K, 1)
    c = N // 2
    kw = dict(sources=[(c, c, c)], wavelet=w, receivers=[(c, c + off, c)])
    plain = wave3d.MediumSolver(prob, backend, **kw).run().traces[:, 0]
    taper = wave3d.sponge_taper(prob, width, sigma_max=sigma_max)
    return plain, wave3d.MediumSolver(prob, backend, taper=taper, **kw).run().traces[:, 0]


def absorb_truth(N, K, f0, off, dtype="fp64", backend="cpu"):
    """The echo-free trace: the same shot in a box of 2N cells, whose walls (and periodic seam) are
    N nodes from the source, 2N - off > K/2 nodes of travel from the receiver."""
    import wave3d

    prob = wave3d.MediumProblem(2 * N, 1.0, Lx=2 * N, Ly=2 * N, Lz=2 * N, T=K / 2, timesteps=K, dtype=dtype)
    w = wave3d.ricker(f0, 1.2 / f0, K, prob.tau).reshape(K, 1)
    return wave3d.MediumSolver(prob, backend, sources=[(N, N, N)], wavelet=w,
                               receivers=[(N, N + off, N)]).run().traces[:, 0]


def absorb_ratio(plain, sponge, truth):
    truth = truth.to(torch.float64)
    e0 = float((plain.to(torch.float64) - truth).abs().max())
    e1 = float((sponge.to(torch.float64) - truth).abs().max())
    return e1 / e0, e0 / float(truth.abs().max())


# measured with this oracle (fp64): e(sponge) / e(no sponge) = 0.173559 (fp32: 0.173560), the undamped
# echo 0.321 of the direct arrival's peak; the bound is 1.5 x that (profiles/medium_sponge.txt)
ABSORB_CPU_RATIO = 0.173559
ABSORB_CPU_BOUND = 1.5 * ABSORB_CPU_RATIO


def test_sponge_absorbs_the_wall_echo():
    N, K, f0, off = 48, 150, 0.08, 12
    assert 2 * N - off > K / 2  # no echo in the truth run: c tau = 0.5 nodes per step
    plain, sponge = absorb_traces(N, K, f0, off, "fp64", "cpu", width=10, sigma_max=0.3)
    truth = absorb_truth(N, K, f0, off)
    ratio, echo = absorb_ratio(plain, sponge, truth)
    print(f"absorption N={N}: e(sponge)/e(no sponge) = {ratio:.6g}, undamped echo / peak = {echo:.6g}")
    assert echo >= 0.1
    assert ratio <= ABSORB_CPU_BOUND
