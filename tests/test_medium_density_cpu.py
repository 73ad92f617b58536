"""Variable density in the medium solver on the CPU: the operator div(b grad u) of ops/reference.py
(laplace_density: symmetry, consistency order), solve_medium / gradient_medium with ``density`` against
the constant-density solver, exact scalings and torch.autograd, and the density model of
MediumProblem (Courant number, stability, validation).
"""
import math

import pytest
import torch

F64 = torch.float64


def _rand(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(shape, generator=g, dtype=F64)


def _periodic(v):
    v[-1] = v[0]
    return v


def _storage(v, N):
    """(N+1)^3 -> the solver's storage with one periodic x ghost plane per side."""
    return torch.cat([v[N - 1:N], v, v[1:2]])


def test_operator_is_symmetric_on_the_unique_nodes():
    """<D_b a, c> = <a, D_b c> for fields that are periodic in x and 0 on the Dirichlet faces."""
    from wave3d.ops import reference

    N = 16
    h2 = (0.011, 0.013, 0.017)
    rho = _periodic(_rand((N + 1,) * 3, 1, 0.5, 3.0))
    b = reference.buoyancy_field(rho, N, F64)

    def field(seed):
        v = _periodic(_rand((N + 1,) * 3, seed, -1.0, 1.0))
        v[:, 0], v[:, N], v[:, :, 0], v[:, :, N] = 0, 0, 0, 0
        return _storage(v, N)

    a, c = field(2), field(3)
    uniq = (slice(1, N + 1), slice(1, N), slice(1, N))  # planes 0 .. N-1, interior j and k
    Da = torch.zeros_like(a)
    Dc = torch.zeros_like(c)
    Da[1:-1, 1:-1, 1:-1] = reference.laplace_density(a, b, *h2)
    Dc[1:-1, 1:-1, 1:-1] = reference.laplace_density(c, b, *h2)
    lhs, rhs = float((Da[uniq] * c[uniq]).sum()), float((a[uniq] * Dc[uniq]).sum())
    rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    print("symmetry: relative difference", rel, "of", lhs)
    assert abs(lhs) > 1 and rel <= 1e-12


def test_operator_is_second_order_consistent():
    """D_b u against div(b grad u) by autograd for smooth u and b on L = pi: order >= 1.9."""
    from wave3d.ops import reference

    def fields(x, y, z):
        u = torch.sin(2 * x + 0.3) * torch.sin(3 * y) * torch.sin(2 * z)
        b = 1 / (1.5 + 0.8 * torch.sin(2 * x + 1) * torch.cos(y) * torch.cos(2 * z))
        return u, b

    def error(N):
        h = math.pi / N
        ax = torch.arange(-1, N + 2, dtype=F64) * h  # one node beyond the box on every side
        X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
        u, b = fields(X, Y, Z)
        got = reference.laplace_density(u, b, h * h, h * h, h * h)
        pts = [t[1:-1, 1:-1, 1:-1].clone().requires_grad_(True) for t in (X, Y, Z)]
        ue, be = fields(*pts)
        grads = torch.autograd.grad(ue.sum(), pts, create_graph=True)
        exact = sum(torch.autograd.grad((be * g).sum(), p, retain_graph=True)[0] for g, p in zip(grads, pts))
        return float((got - exact).abs().max())

    e32, e64 = error(32), error(64)
    order = math.log2(e32 / e64)
    print("consistency: errors", e32, e64, "order", order)
    assert order >= 1.9


def _model(N, seed=4):
    u0 = _periodic(_rand((N + 1,) * 3, seed, -1.0, 1.0))
    speed2 = _periodic(_rand((N + 1,) * 3, seed + 1, 0.5, 1.5))
    return u0, speed2


@pytest.fixture(scope="module")
def plain16():
    from wave3d.ops import reference

    N, K = 16, 40
    u0, speed2 = _model(N)
    return N, K, u0, speed2, reference.solve_medium(N, K, speed2, u0=u0)


@pytest.mark.parametrize("rho0", [1.0, 2.0, 3.0])
def test_uniform_density_is_todays_solver(plain16, rho0):
    from wave3d.ops import reference

    N, K, u0, speed2, (_, want, wmx) = plain16
    tr, got, mx = reference.solve_medium(N, K, speed2, u0=u0, density=torch.full((N + 1,) * 3, rho0, dtype=F64))
    rel = float((got - want).abs().max() / want.abs().max())
    print("uniform density", rho0, "relative L-inf", rel)
    assert float(want.abs().max()) > 0.1 and rel <= 1e-12
    assert max(abs(a - b) for a, b in zip(mx, wmx)) <= 1e-12 * max(wmx)


def test_scalar_density_is_the_filled_array():
    from wave3d.ops import reference

    N, K = 8, 6
    u0, speed2 = _model(N)
    a = reference.solve_medium(N, K, speed2, u0=u0, density=1.7, receivers=[(3, 4, 5)])
    b = reference.solve_medium(N, K, speed2, u0=u0, density=torch.full((N + 1,) * 3, 1.7, dtype=F64),
                               receivers=[(3, 4, 5)])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert float(a[1].abs().max()) > 0.1
    assert torch.equal(reference.buoyancy_field(1.7, N, F64),
                       reference.buoyancy_field(torch.full((N + 1,) * 3, 1.7, dtype=F64), N, F64))


def _scaling_solver(backend, density):
    import wave3d

    N, K = 12, 16
    g = torch.Generator().manual_seed(21)
    speed2 = _periodic(0.5 + torch.rand((N + 1,) * 3, generator=g, dtype=F64))
    prob = wave3d.MediumProblem(N, speed2, timesteps=K, density=density)
    w = torch.stack([wave3d.ricker(3.0, 0.3, K, prob.tau), -0.5 * wave3d.ricker(2.0, 0.2, K, prob.tau)], 1)
    return wave3d.MediumSolver(prob, backend, sources=[(0, 4, 6), (6, 3, 5)], wavelet=w,
                               receivers=[(N, 7, 3), (4, 5, 5), (6, 3, 5)], taper=wave3d.sponge_taper(prob, 3))


def test_power_of_two_density_scales_the_field_exactly():
    """m doubles, D_b halves and the source term doubles, all exactly: density 2 gives 2 x density 1."""
    one, two = _scaling_solver("cpu", 1.0).run(), _scaling_solver("cpu", 2.0).run()
    assert float(one.traces.abs().max()) > 1e-3
    assert torch.equal(two.traces, 2 * one.traces) and torch.equal(two.u_final, 2 * one.u_final)
    assert two.extra["density"] is True and one.courant == two.courant


def _layered(N):
    """Layered rho and c^2 (in k), periodic in x by construction."""
    rho = torch.ones((N + 1,) * 3, dtype=F64)
    rho[:, :, N // 2:] = 2.5
    rho[:, N // 2:, :] *= 1.3
    speed2 = torch.full((N + 1,) * 3, 1.0, dtype=F64)
    speed2[:, :, N // 3:] = 1.8
    return rho, speed2


def test_gradient_matches_autograd():
    import wave3d
    from wave3d.ops import reference

    N, K = 8, 10
    rho, speed2 = _layered(N)
    prob = wave3d.MediumProblem(N, speed2, timesteps=K, density=rho)
    w = wave3d.ricker(3.0, 0.3, K, prob.tau)[:, None].clone()
    kw = dict(sources=[(0, 4, 5)], wavelet=w, receivers=[(3, 2, 6), (N, 5, 3)], taper=wave3d.sponge_taper(prob, 2),
              density=rho)
    observed = reference.solve_medium(N, K, speed2 * 1.1, **kw)[0]
    s = speed2.clone().requires_grad_(True)
    wl = w.clone().requires_grad_(True)
    tr = reference.forward_medium_autograd(N, K, s, **dict(kw, wavelet=wl))
    assert torch.equal(tr.detach(), reference.solve_medium(N, K, speed2, **kw)[0])
    J = 0.5 * ((tr[1:] - observed[1:]) ** 2).sum()
    gs, gw = torch.autograd.grad(J, (s, wl))
    Jh, grad, gwh, traces = reference.gradient_medium(N, K, speed2, observed, **kw)
    fold = gs.clone()  # plane-0 convention: the unique node gets both leaves
    fold[0] = gs[0] + gs[N]
    fold[N] = fold[0]
    e_s = float((grad - fold).abs().max() / fold.abs().max())
    e_w = float((gwh - gw).abs().max() / gw.abs().max())
    print("gradient against autograd: speed2", e_s, "wavelet", e_w)
    assert float(fold.abs().max()) > 0 and float(gw.abs().max()) > 0
    assert e_s <= 1e-12 and e_w <= 1e-12
    assert abs(Jh - J.item()) <= 1e-12 * J.item() and torch.equal(traces, tr.detach())
    # density matters: the constant-density gradient is another one
    plain = reference.gradient_medium(N, K, speed2, observed, **{k: v for k, v in kw.items() if k != "density"})[1]
    assert float((plain - grad).abs().max()) > 1e-3 * float(grad.abs().max())
    # the front-end's cpu backend is the same call
    r = wave3d.MediumSolver(prob, "cpu", **{k: v for k, v in kw.items() if k != "density"}).gradient(observed)
    assert r.misfit == Jh and torch.equal(r.grad_speed2, grad) and torch.equal(r.grad_wavelet, gwh)
    assert r.extra["density"] is True


def _courant_formula(speed2, rho, N, tau, h_min):
    """sqrt(max_i kappa_i bhat_i) tau / h_min with plain loops over the stencil nodes."""
    b = (1.0 / rho).tolist()
    kap = (speed2 * rho).tolist()
    best = 0.0
    for i in range(N + 1):
        im, ip = (i - 1) % N, (i + 1) % N  # planes 0 and N are one plane
        for j in range(1, N):
            for k in range(1, N):
                nb = (b[im][j][k], b[ip][j][k], b[i][j - 1][k], b[i][j + 1][k], b[i][j][k - 1], b[i][j][k + 1])
                best = max(best, kap[i][j][k] * max(0.5 * (b[i][j][k] + v) for v in nb))
    return math.sqrt(best) * tau / h_min


def test_courant_number_with_density():
    import wave3d

    N, K = 6, 40
    _, speed2 = _model(N)
    plain = wave3d.MediumProblem(N, speed2, timesteps=K)
    scalar = wave3d.MediumProblem(N, speed2, timesteps=K, density=2.7)
    assert scalar.courant == plain.courant and scalar.min_stable_timesteps() == plain.min_stable_timesteps()
    assert plain.density is None and scalar.density.dtype == F64 and scalar.density.dim() == 0
    rho = _periodic(_rand((N + 1,) * 3, 9, 0.5, 4.0))
    prob = wave3d.MediumProblem(N, speed2, timesteps=K, density=rho)
    want = _courant_formula(speed2, rho, N, prob.tau, min(prob.lengths()) / N)
    assert math.isclose(prob.courant, want, rel_tol=1e-14) and prob.courant != plain.courant
    assert torch.equal(prob.density, rho) and prob.density.device.type == "cpu" and prob.stable()
    k = prob.min_stable_timesteps()
    assert wave3d.MediumProblem(N, speed2, timesteps=k, density=rho).stable()
    with pytest.raises(ValueError, match="Courant"):  # a model above the limit raises
        wave3d.MediumProblem(N, speed2, timesteps=k - 1, density=rho)
    assert wave3d.gradient_levels(9, 3, density=True) == wave3d.gradient_levels(9, 3) + 1


def _band_limited(N, seed, M=5):
    """Random data on the lowest modes: random coefficients in [-1, 1] on the Fourier modes |ix| <= M in
    x and the sine modes 1 .. M in y and z (periodic in x, 0 on the Dirichlet faces)."""
    q = torch.arange(N + 1, dtype=F64) / N
    a = _rand((2 * M + 1, M, M), seed, -1.0, 1.0)
    fx = torch.stack([torch.cos(2 * math.pi * ix * q) if ix >= 0 else torch.sin(2 * math.pi * ix * q)
                      for ix in range(-M, M + 1)])
    fs = torch.stack([torch.sin(math.pi * m * q) for m in range(1, M + 1)])
    u = torch.einsum("abc,ai,bj,ck->ijk", a, fx, fs, fs)
    u[N] = u[0]
    u[:, 0], u[:, N], u[:, :, 0], u[:, :, N] = 0, 0, 0, 0
    return u


@pytest.mark.parametrize("data", ["white", "band"])
def test_stable_at_the_limit_with_a_two_valued_density(data):
    """A random two-valued rho in {1, 4} at 0.98 of the limit, N = 16, 200 steps from random data:
    max |u| <= 2 max |u0| (a blow-up grows by orders of magnitude).

    "band": random coefficients on the lowest modes; the bound holds on every layer (measured 1.05).
    "white": uniform noise in [-1, 1] on every node, which excites every mode of the operator. There
    the bound holds on the field after the 200 steps (measured 1.77) but cannot hold on every layer:
    the constant-density solver itself reaches 2.0 to 2.5 on such data at 0.98 of its own limit, and
    the density solver 2.76, by the statistics of the maximum of 17^3 mixed values, not by growth (1000
    steps give 3.2, 200 steps 2.76). For the white data the test therefore adds the bound that a stable
    scheme obeys exactly: from rest with the Taylor start every eigenmode of kappa D_b is u^n =
    cos(n theta) u^0, and the modes are orthogonal under the weight 1 / kappa on the unique nodes, so the
    weighted L2 norm of no layer exceeds that of u0."""
    import wave3d

    N, K = 16, 200
    rho = _periodic(1.0 + 3.0 * (_rand((N + 1,) * 3, 12) < 0.5).to(F64))
    assert sorted(set(rho.flatten().tolist())) == [1.0, 4.0]
    u0, speed2 = _model(N, 13)
    if data == "band":
        u0 = _band_limited(N, 6)
    u0[:, 0], u0[:, N], u0[:, :, 0], u0[:, :, N] = 0, 0, 0, 0
    probe = wave3d.MediumProblem(N, speed2, timesteps=K, T=1e-3, density=rho)
    T = 1e-3 * 0.98 * probe.cfl_limit / probe.courant  # the Courant number is linear in T at fixed K
    prob = wave3d.MediumProblem(N, speed2, timesteps=K, T=T, density=rho)
    assert math.isclose(prob.courant, 0.98 * prob.cfl_limit, rel_tol=1e-12)
    r = wave3d.MediumSolver(prob, "cpu", u0=u0).run()
    m0 = float(u0.abs().max())
    layers, final = max(r.max_abs_u) / m0, float(r.u_final.abs().max()) / m0
    print(data, "max |u| / max |u0| at 0.98 of the limit: every layer", layers, "after 200 steps", final)
    assert final <= 2.0
    if data == "band":
        assert layers <= 2.0
    else:
        w = 1.0 / (speed2 * rho)
        uniq = (slice(0, N), slice(1, N), slice(1, N))
        n0 = float((w[uniq] * u0[uniq] ** 2).sum())
        nK = float((w[uniq] * r.u_final[uniq] ** 2).sum())
        print("weighted L2 norm squared: u0", n0, "u_K", nK)
        assert nK <= n0 * (1 + 1e-10)


def test_validation_errors():
    import wave3d
    from wave3d.ops import reference

    N = 6
    ok = torch.ones((N + 1,) * 3, dtype=F64)
    with pytest.raises(ValueError, match="density must be a scalar or have shape"):
        wave3d.MediumProblem(N, 0.5, density=torch.ones(N, N, N))
    for bad in (0.0, -1.0, math.inf):
        v = ok.clone()
        v[2, 3, 4] = bad
        with pytest.raises(ValueError, match="density must be finite and > 0"):
            wave3d.MediumProblem(N, 0.5, density=v)
    with pytest.raises(ValueError, match="density must be finite and > 0"):
        wave3d.MediumProblem(N, 0.5, density=-2.0)
    v = ok.clone()
    v[N, 2, 3] = 2.0
    with pytest.raises(ValueError, match="density must be periodic in x"):
        wave3d.MediumProblem(N, 0.5, density=v)
    with pytest.raises(ValueError, match="space_order 2"):
        wave3d.MediumProblem(N, 0.5, density=ok, space_order=4, timesteps=40)
    u = _rand((N + 5, N + 1, N + 1), 3)
    with pytest.raises(ValueError, match="order 2"):
        reference.step_medium(u, u, u, (2, N + 2, 2, N - 2, 2, N - 2), first=False, hx2=0.1, hy2=0.1, hz2=0.1,
                              order=4, buoyancy=torch.ones_like(u))
    with pytest.raises(ValueError, match="order 2"):
        reference.solve_medium(N, 40, 0.5, order=4, density=ok)
