"""Space orders 4 and 8 of the variable-speed medium solver on the CPU: the star Laplacian of the
PyTorch oracle (ops/reference.py laplace_star), its consistency order and symmetry, the adjoint
against torch.autograd, the order-dependent CFL limit, stability at that limit and the argument
checks. Order 2 must stay what it was bit for bit.
"""
import math

import pytest
import torch

from test_medium_gradient_cpu import K, N, _case, _kw, _rel  # that file's case: N = 10, K = 16

ORDERS = (4, 8)


def test_default_path_is_unchanged():
    """order=2 is the call without the keyword, bit for bit (the case of test_medium_gradient_cpu)."""
    from wave3d.ops import reference

    speed2, pert, w, taper = _case()
    kw = _kw(w, taper)
    a = reference.solve_medium(N, K, speed2, **kw)
    b = reference.solve_medium(N, K, speed2, order=2, **kw)
    assert float(a[0].abs().max()) > 1e-3
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    observed = reference.solve_medium(N, K, pert, **kw)[0]
    ga = reference.gradient_medium(N, K, speed2, observed, **kw)
    gb = reference.gradient_medium(N, K, speed2, observed, order=2, **kw)
    assert ga[0] == gb[0] and float(ga[1].abs().max()) > 0
    assert all(torch.equal(x, y) for x, y in zip(ga[1:], gb[1:]))


def _mode_error(n, order):
    """L-inf error of the discrete Laplacian of sin(2x + 0.3) sin(3y) sin(2z) on the pi-box."""
    from wave3d.ops import reference

    h, M = math.pi / n, order // 2
    x = torch.arange(-M, n + 1 + M, dtype=torch.float64) * h
    y = torch.arange(n + 1, dtype=torch.float64) * h
    f = torch.sin(2 * x + 0.3)[:, None, None] * torch.sin(3 * y)[None, :, None] * torch.sin(2 * y)[None, None, :]
    lap = reference.laplace_star(f, (M, n + M, 1, n - 1, 1, n - 1), h * h, h * h, h * h, order=order,
                                 mirror=(0, n, 0, n))
    return float((lap + 17 * f[M:n + 1 + M, 1:n, 1:n]).abs().max())


@pytest.mark.parametrize("order", ORDERS)
def test_consistency_order(order):
    rate = math.log2(_mode_error(16, order) / _mode_error(32, order))
    print("order", order, "observed", rate)  # numpy: 3.97 (order 4), 7.92 (order 8)
    assert rate >= order - 0.25


def test_star_laplacian_is_symmetric():
    """<La, b> = <a, Lb> on the unique nodes (x periodic, odd reflection at the y/z faces), unequal h."""
    from wave3d.ops import reference

    n, M = 8, 4
    g = torch.Generator().manual_seed(3)
    h2 = (1.0, 1.3, 0.7)

    def field():
        u = torch.zeros(n + 1 + 2 * M, n + 1, n + 1, dtype=torch.float64)
        u[M:n + M, 1:n, 1:n] = torch.rand(n, n - 1, n - 1, generator=g, dtype=torch.float64) - 0.5
        u[n + M] = u[M]  # plane N is plane 0
        reference._wrap_x(u, n, M)
        return u

    def lap(u):
        return reference.laplace_star(u, (M, n + M - 1, 1, n - 1, 1, n - 1), *h2, order=8, mirror=(0, n, 0, n))

    a, b = field(), field()
    own = (slice(M, n + M), slice(1, n), slice(1, n))
    lab, alb = float((lap(a) * b[own]).sum()), float((a[own] * lap(b)).sum())
    print("<La,b>", lab, "<a,Lb>", alb)
    assert abs(lab) > 1.0  # not a tiny number that would make the bound empty
    assert abs(lab - alb) <= 1e-12 * abs(lab)


@pytest.fixture(scope="module")
def grads():
    """Per order: autograd's gradients of the existing case and the hand-written adjoint's."""
    from wave3d.ops import reference

    speed2, pert, w, taper = _case()
    out = {}
    for order in ORDERS:
        kw = dict(order=order, **_kw(w, taper))
        observed = reference.solve_medium(N, K, pert, **kw)[0]
        s = speed2.clone().requires_grad_(True)
        wl = w.clone().requires_grad_(True)
        tr = reference.forward_medium_autograd(N, K, s, **dict(kw, wavelet=wl))
        J = 0.5 * ((tr[1:] - observed[1:]) ** 2).sum()
        gs, gw = torch.autograd.grad(J, (s, wl))
        hand = reference.gradient_medium(N, K, speed2, observed, **kw)
        out[order] = dict(J=J.item(), gs=gs, gw=gw, hand=hand, traces=reference.solve_medium(N, K, speed2, **kw)[0])
    return out


# measured relative max-norm differences (speed2, wavelet); 100x that covers other summation orders
# (cap 1e-9), the rule of test_medium_gradient_cpu.test_adjoint_matches_autograd
ADJOINT_MEASURED = {4: (2.44e-15, 1.09e-15), 8: (2.46e-15, 1.83e-15)}


@pytest.mark.parametrize("order", ORDERS)
def test_adjoint_matches_autograd(grads, order):
    c = grads[order]
    J, grad, gw, traces = c["hand"]
    fold = c["gs"].clone()  # planes 0 and N are two leaves of autograd: the unique node gets both
    fold[0] = c["gs"][0] + c["gs"][N]
    fold[N] = fold[0]
    assert float(fold.abs().max()) > 0 and float(c["gw"].abs().max()) > 0
    e_s, e_w = _rel(grad, fold), _rel(gw, c["gw"])
    print("order", order, "relative max-norm difference: speed2", e_s, "wavelet", e_w)
    b_s, b_w = (min(100 * v, 1e-9) for v in ADJOINT_MEASURED[order])
    assert e_s <= b_s
    assert e_w <= b_w
    assert abs(J - c["J"]) <= 1e-14 * c["J"]
    assert torch.equal(traces, c["traces"])
    for f in (grad[:, 0], grad[:, N], grad[:, :, 0], grad[:, :, N]):
        assert float(f.abs().max()) == 0.0


def test_cfl_limits():
    import wave3d

    for order, want in ((2, 1 / math.sqrt(3)), (4, 0.5), (8, 0.45285552331841994)):
        assert abs(wave3d.cfl_limit(order) - want) <= 1e-12
    # 2 / sqrt(3 S), S = |c_0| + 2 sum |c_d|
    S8 = 205 / 72 + 2 * (8 / 5 + 1 / 5 + 8 / 315 + 1 / 560)
    assert abs(wave3d.cfl_limit(8) - 2 / math.sqrt(3 * S8)) <= 1e-12
    with pytest.raises(ValueError):
        wave3d.cfl_limit(6)

    n, k = 16, 20
    h, tau = wave3d.models.wave.PI_REF / n, 1.0 / k

    def problem(courant, order, **kw):
        return wave3d.MediumProblem(n, (courant * h / tau) ** 2, timesteps=k, space_order=order, **kw)

    assert abs(problem(0.55, 2).courant - 0.55) < 1e-12
    for courant, good, bad in ((0.55, (2,), (4, 8)), (0.48, (2, 4), (8,))):
        for order in good:
            assert problem(courant, order).stable()
        for order in bad:
            with pytest.raises(ValueError, match="Courant"):
                problem(courant, order)
            with pytest.warns(RuntimeWarning):
                p = problem(courant, order, strict_cfl=False)
            assert not p.stable()
            q = wave3d.MediumProblem(n, p.speed2, timesteps=p.min_stable_timesteps(), space_order=order)
            assert q.stable() and q.timesteps > k


@pytest.mark.parametrize("order", (2, 4, 8))
def test_oracle_is_stable_just_below_the_limit(order):
    """200 steps at 0.98 of the limit from random data: max |u| stays within 2x its initial value
    (numpy at N = 16: at most 1.03x; at 1.05 of the limit it exceeds 1e70).

    The data are normal deviates: from rest every eigenmode evolves as cos(n theta) times its
    initial amplitude, so a stable run only re-phases the modes, the field stays a normal one of at
    most the initial variance, and its maximum stays at the extreme-value scale it started on.
    (A uniform field would turn normal and its maximum grow about twofold without any instability.)"""
    import wave3d
    from wave3d.ops import reference

    n, k = 12, 200
    h = wave3d.models.wave.PI_REF / n
    T = k * 0.98 * wave3d.cfl_limit(order) * h  # speed 1: Courant = tau / h
    g = torch.Generator().manual_seed(order)
    u0 = torch.zeros((n + 1,) * 3, dtype=torch.float64)
    u0[:n, 1:n, 1:n] = torch.randn(n, n - 1, n - 1, generator=g, dtype=torch.float64)
    u0[n] = u0[0]
    prob = wave3d.MediumProblem(n, 1.0, T=T, timesteps=k, space_order=order)
    assert abs(prob.courant / prob.cfl_limit - 0.98) < 1e-9
    mx = reference.solve_medium(n, k, 1.0, u0=u0, T=T, order=order)[2]
    print("order", order, "max |u| growth", max(mx) / mx[0])
    assert max(mx) <= 2 * mx[0]


def test_argument_checks():
    import wave3d
    from wave3d.ops import reference

    u = torch.zeros(14, 12, 12, dtype=torch.float64)
    kw = dict(first=False, hx2=1.0, hy2=1.0, hz2=1.0)
    ok = (4, 9, 4, 7, 4, 7)
    assert reference.step_medium(u, u, u, ok, order=8, **kw).shape == (6, 4, 4)
    with pytest.raises(ValueError, match="order"):
        reference.step_medium(u, u, u, ok, order=6, **kw)
    for box in ((3, 9, 4, 7, 4, 7), (4, 10, 4, 7, 4, 7), (4, 9, 3, 7, 4, 7), (4, 9, 4, 8, 4, 7), (4, 9, 4, 7, 4, 8)):
        with pytest.raises(ValueError, match="nearer than 4"):  # too near an unmirrored edge
            reference.step_medium(u, u, u, box, order=8, **kw)
    # the same box is fine with a face there, but not on or beyond the face
    assert reference.step_medium(u, u, u, (4, 9, 1, 7, 4, 7), order=8, mirror=(0, None, None, None), **kw).shape[1] == 7
    with pytest.raises(ValueError, match="mirror"):
        reference.step_medium(u, u, u, (4, 9, 1, 7, 4, 7), order=8, mirror=(1, None, None, None), **kw)
    with pytest.raises(ValueError, match="mirror"):  # faces nearer than M
        reference.step_medium(u, u, u, (4, 9, 1, 2, 4, 7), order=8, mirror=(0, 3, None, None), **kw)
    with pytest.raises(ValueError, match="space_order"):
        wave3d.MediumProblem(16, 1.0, timesteps=40, space_order=6)
    with pytest.raises(ValueError, match="N >= 8"):
        wave3d.MediumProblem(7, 1.0, timesteps=40, space_order=8)
    with pytest.raises(ValueError, match="N >= 4"):
        reference.solve_medium(3, 4, 0.01, order=4)
    assert wave3d.MediumProblem(8, 1.0, timesteps=40, space_order=8).space_order == 8
    assert wave3d.MediumProblem(8, 1.0, timesteps=40).space_order == 2


def test_front_end_cpu_passes_the_order():
    import wave3d
    from wave3d.ops import reference

    speed2, pert, w, taper = _case()
    for order in ORDERS:
        prob = wave3d.MediumProblem(N, speed2, timesteps=K, space_order=order)
        sol = wave3d.MediumSolver(prob, "cpu", **_kw(w, taper))
        r = sol.run()
        want = reference.solve_medium(N, K, speed2, order=order, **_kw(w, taper))
        assert torch.equal(r.traces, want[0]) and torch.equal(r.u_final, want[1]) and r.max_abs_u == want[2]
        assert r.extra["space_order"] == order and tuple(r.u_final.shape) == (N + 1,) * 3
        assert not torch.equal(r.traces, reference.solve_medium(N, K, speed2, **_kw(w, taper))[0])
        observed = reference.solve_medium(N, K, pert, order=order, **_kw(w, taper))[0]
        g = sol.gradient(observed)
        hand = reference.gradient_medium(N, K, speed2, observed, order=order, **_kw(w, taper))
        assert g.misfit == hand[0] and torch.equal(g.grad_speed2, hand[1]) and torch.equal(g.grad_wavelet, hand[2])
        assert g.extra["space_order"] == order
