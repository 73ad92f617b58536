"""Source illumination and the pseudo-Hessian diagonal of the medium solver on the CPU: the oracle's
accumulation (ops/reference.py _adjoint_medium, finish_illumination) against the sum formed from
forward_medium_autograd(keep_lap=True) in the stated order, the conventions, the finite reach,
precondition(), the level counts and the argument checks of MediumSolver.gradient(illumination=True).
"""
import pytest
import torch

from test_medium_gradient_cpu import RECEIVERS, SOURCES, N, K, _case, _kw


def _density():
    g = torch.Generator().manual_seed(23)
    rho = 1 + torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64)
    rho[N] = rho[0]
    return rho


def _setup(order, sponge, density):
    """speed2, the oracle's keywords and the observed traces (those of a perturbed speed2)."""
    from wave3d.ops import reference

    speed2, pert, w, taper = _case()
    kw = dict(_kw(w, taper if sponge else None), order=order, density=_density() if density else None)
    observed = reference.solve_medium(N, K, pert, **kw)[0]
    return speed2, kw, observed


def _weight(kw, tau, dtype=torch.float64):
    """w = (G tau) tau [rho] on the planes 0 .. N, as the issue defines it."""
    from wave3d.ops import reference

    M = kw["order"] // 2
    if kw["taper"] is None:
        G = torch.ones((N + 1,) * 3, dtype=dtype)
    else:
        gx, gy, gz = reference.taper_tables(kw["taper"], N, dtype, M)
        G = gx[M:N + 1 + M, None, None] * (gy[None, :, None] * gz[None, None, :])
    w = (G * tau) * tau
    if kw["density"] is not None:
        w = w * kw["density"].to(dtype)
    return w


CASES = [(2, False, False), (2, True, False), (4, False, False), (4, True, False), (8, False, False),
         (8, True, False), (2, False, True), (2, True, True)]


@pytest.mark.parametrize("order,sponge,density", CASES)
def test_illumination_is_the_ordered_sum_of_squared_laplacians(order, sponge, density):
    from wave3d.ops import reference

    speed2, kw, observed = _setup(order, sponge, density)
    plain = reference.gradient_medium(N, K, speed2, observed, **kw)
    out = reference.gradient_medium(N, K, speed2, observed, illumination=True, **kw)
    assert len(plain) == 4 and len(out) == 6
    for a, b in zip(plain[1:], out[1:4]):  # the flag changes nothing else
        assert torch.equal(a, b)
    assert plain[0] == out[0]
    illum, ph = out[4], out[5]
    _, laps = reference.forward_medium_autograd(N, K, speed2, keep_lap=True, **kw)
    assert len(laps) == K - 1
    h = torch.zeros(N + 1, N - 1, N - 1, dtype=torch.float64)
    for q in laps:  # ascending n; the product rounded, then the add
        h = h + q * q
    want = torch.zeros((N + 1,) * 3, dtype=torch.float64)
    want[:, 1:N, 1:N] = h
    want[N] = want[0]
    assert float(want.max()) > 0
    assert torch.equal(illum, want)
    # conventions
    assert tuple(illum.shape) == tuple(ph.shape) == (N + 1,) * 3
    assert bool((illum >= 0).all()) and bool((ph >= 0).all())
    for f in (illum, ph):
        assert torch.equal(f[N], f[0])
        for face in (f[:, 0], f[:, N], f[:, :, 0], f[:, :, N]):
            assert not bool(face.any())
    w = _weight(kw, 1.0 / K)
    assert torch.equal(ph, illum * (w * w))


def test_density_gradient_oracle_carries_the_same_illumination():
    from wave3d.ops import reference

    speed2, kw, observed = _setup(2, True, True)
    a = reference.gradient_medium(N, K, speed2, observed, illumination=True, **kw)
    b = reference.gradient_medium_density(N, K, speed2, observed, illumination=True, **kw)
    assert len(b) == 7
    assert torch.equal(a[4], b[5]) and torch.equal(a[5], b[6])
    assert torch.equal(b[4], reference.gradient_medium_density(N, K, speed2, observed, **kw)[4])


def test_illumination_has_finite_reach():
    import wave3d

    n, k, M = 20, 4, 1
    src = (3, 9, 12)
    prob = wave3d.MediumProblem(n, 1.0, T=0.2, timesteps=k)
    sol = wave3d.MediumSolver(prob, "cpu", sources=[src], wavelet=torch.ones(k, 1), receivers=[(5, 5, 5)])
    r = sol.gradient(torch.zeros(k + 1, 1), illumination=True)
    reach = (k - 1) * M
    q = torch.arange(n + 1)
    dx = torch.minimum((q - src[0]) % n, (src[0] - q) % n)  # periodic in x
    dy, dz = (q - src[1]).abs(), (q - src[2]).abs()
    far = (dx[:, None, None] > reach) | (dy[None, :, None] > reach) | (dz[None, None, :] > reach)
    assert bool(far.any()) and not bool(far.all())
    assert not bool(r.illumination[far].any())
    assert not bool(r.pseudo_hessian_speed2[far].any())
    assert float(r.illumination[src]) > 0
    # the farthest nodes along an axis are reached by q^{K-1} alone
    assert float(r.illumination[src[0] + reach, src[1], src[2]]) > 0
    assert float(r.illumination[src[0] - reach, src[1], src[2]]) > 0


def test_precondition():
    import wave3d

    speed2, kw, observed = _setup(2, True, False)
    kw = {k: v for k, v in kw.items() if k not in ("order", "density")}
    sol = wave3d.MediumSolver(wave3d.MediumProblem(N, speed2, timesteps=K), "cpu", **kw)
    r = sol.gradient(observed, illumination=True)
    g, ph = r.grad_speed2, r.pseudo_hessian_speed2
    for eps in (1e-3, 0.5):
        p = wave3d.precondition(g, ph, eps)
        assert torch.equal(p, g / (ph + eps * ph.max()))
        assert torch.equal(p[N], p[0])
        for face in (p[:, 0], p[:, N], p[:, :, 0], p[:, :, N]):
            assert not bool(face.any())
        assert bool(torch.isfinite(p).all()) and float(p.abs().max()) > 0
    assert torch.equal(wave3d.precondition(g, ph), wave3d.precondition(g, ph, 1e-3))
    for eps in (0, -1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            wave3d.precondition(g, ph, eps)
    with pytest.raises(ValueError, match="maximum"):
        wave3d.precondition(g, torch.zeros_like(ph))
    with pytest.raises(ValueError, match="maximum"):
        wave3d.precondition(g, -ph - 1)
    with pytest.raises(ValueError, match="shape"):
        wave3d.precondition(g, ph[:-1])


def test_front_end_flag():
    import wave3d

    speed2, kw, observed = _setup(2, True, False)
    kw = {k: v for k, v in kw.items() if k not in ("order", "density")}
    sol = wave3d.MediumSolver(wave3d.MediumProblem(N, speed2, timesteps=K), "cpu", **kw)
    off = sol.gradient(observed)
    assert off.illumination is None and off.pseudo_hessian_speed2 is None
    assert off.extra["illumination"] is False
    on = sol.gradient(observed, illumination=True)
    assert on.extra["illumination"] is True
    assert on.misfit == off.misfit
    assert torch.equal(on.grad_speed2, off.grad_speed2)
    assert torch.equal(on.grad_wavelet, off.grad_wavelet)
    assert torch.equal(on.traces, off.traces)
    assert on.illumination.dtype == torch.float64 and float(on.illumination.max()) > 0
    # the illumination peaks at a source, where the forward field is strongest
    peak = tuple(int(v) for v in (on.illumination == on.illumination.max()).nonzero()[0])
    assert (peak[0] % N, peak[1], peak[2]) in {(s[0] % N, s[1], s[2]) for s in SOURCES}
    # gauss_newton passes the flag through
    d = 0.01 * speed2
    gn = sol.gauss_newton(d, illumination=True)
    assert torch.equal(gn.illumination, on.illumination)
    assert torch.equal(gn.pseudo_hessian_speed2, on.pseudo_hessian_speed2)
    assert sol.gauss_newton(d).illumination is None
    # with a density and its gradient
    rho = _density()
    sd = wave3d.MediumSolver(wave3d.MediumProblem(N, speed2, timesteps=K, density=rho), "cpu", **kw)
    both = sd.gradient(observed, wrt_density=True, illumination=True)
    assert torch.equal(both.grad_density, sd.gradient(observed, wrt_density=True).grad_density)
    assert torch.equal(both.illumination, sd.gradient(observed, illumination=True).illumination)
    assert len(RECEIVERS) == observed.shape[1]


def test_fp32_illumination_is_accumulated_in_the_working_dtype():
    import wave3d

    speed2, kw, observed = _setup(2, True, False)
    kw = {k: v for k, v in kw.items() if k not in ("order", "density")}
    r = wave3d.MediumSolver(wave3d.MediumProblem(N, speed2, timesteps=K, dtype="fp32"), "cpu", **kw).gradient(
        observed, illumination=True)
    assert r.illumination.dtype == torch.float32 and r.pseudo_hessian_speed2.dtype == torch.float32
    w = _weight(dict(kw, order=2, density=None), 1.0 / K, torch.float32)
    assert torch.equal(r.pseudo_hessian_speed2, r.illumination * (w * w))


def test_gradient_levels_count_the_illumination_level():
    import wave3d

    for k in (1, 2, 3, 16, 24, 100):
        for seg in (1, 2, 5, 7, k - 1, k, k + 5):
            if seg < 1:
                continue
            for kw in ({}, dict(density=True), dict(density=True, wrt_density=True)):
                assert (wave3d.gradient_levels(k, seg, illumination=True, **kw)
                        == wave3d.gradient_levels(k, seg, **kw) + 1)
        # one level more for every segment: the best segment does not move
        assert wave3d.best_gradient_segment(k, illumination=True) == wave3d.best_gradient_segment(k)
        assert (wave3d.best_gradient_segment(k, wrt_density=True, illumination=True)
                == wave3d.best_gradient_segment(k, wrt_density=True))


def test_illumination_with_a_variant_raises():
    import wave3d

    speed2, kw, observed = _setup(2, True, False)
    kw = {k: v for k, v in kw.items() if k not in ("order", "density")}
    prob = wave3d.MediumProblem(N, speed2, timesteps=K)
    for backend in ("cpu", "hip"):  # refused before any device is touched
        for variant in ("nt", "plain", "r2", "r2nt"):
            sol = wave3d.MediumSolver(prob, backend, variant=variant, **kw)
            with pytest.raises(ValueError, match="variant"):
                sol.gradient(observed, illumination=True)
