"""Misfit gradients of the variable-speed medium solver on the CPU: the hand-written adjoint
(ops/reference.py gradient_medium) against torch.autograd of the out-of-place forward restatement
(forward_medium_autograd), the plane-0 convention, the level planning and the argument checks of
MediumSolver.gradient.
"""
import pytest
import torch

N, K = 10, 16
SOURCES = [(0, 4, 6), (6, 3, 5)]                              # one on the periodic plane, one interior
RECEIVERS = [(N, 7, 3), (4, 5, 5), (4, 5, 5), (3, 0, 4), (7, 6, 2)]  # plane N, two on one node, a face


def _case():
    import wave3d

    g = torch.Generator().manual_seed(11)
    speed2 = 2 + 2 * torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64)
    speed2[N] = speed2[0]
    pert = speed2 * (1 + 0.1 * torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64))
    pert[N] = pert[0]
    tau = 1.0 / K
    w = torch.stack([wave3d.ricker(3.0, 0.3, K, tau), -0.5 * wave3d.ricker(2.0, 0.2, K, tau)], 1)
    prob = wave3d.MediumProblem(N, speed2, timesteps=K)
    taper = wave3d.sponge_taper(prob, 3)
    return speed2, pert, w, taper


def _kw(w, taper):
    return dict(sources=SOURCES, wavelet=w, receivers=RECEIVERS, taper=taper)


@pytest.fixture(scope="module")
def case():
    """The shared case: observed = the traces of a perturbed speed2; autograd's and the adjoint's gradients."""
    from wave3d.ops import reference

    speed2, pert, w, taper = _case()
    observed = reference.solve_medium(N, K, pert, **_kw(w, taper))[0]
    s = speed2.clone().requires_grad_(True)
    wl = w.clone().requires_grad_(True)
    tr = reference.forward_medium_autograd(N, K, s, **_kw(wl, taper))
    J = 0.5 * ((tr[1:] - observed[1:]) ** 2).sum()
    gs, gw = torch.autograd.grad(J, (s, wl))
    hand = reference.gradient_medium(N, K, speed2, observed, **_kw(w, taper))
    return dict(speed2=speed2, w=w, taper=taper, observed=observed, J=J.item(), gs=gs, gw=gw, hand=hand)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("sponge", [True, False])
def test_forward_restatement_is_solve_medium_bit_for_bit(sponge):
    from wave3d.ops import reference

    speed2, _, w, taper = _case()
    kw = _kw(w, taper if sponge else None)
    a = reference.forward_medium_autograd(N, K, speed2, **kw)
    b = reference.solve_medium(N, K, speed2, **kw)[0]
    assert float(b.abs().max()) > 1e-3
    assert torch.equal(a, b)


def test_adjoint_matches_autograd(case):
    J, grad, gw, traces = case["hand"]
    gs = case["gs"]
    fold = gs.clone()          # autograd treats planes 0 and N as two leaves: the unique node gets both
    fold[0] = gs[0] + gs[N]
    fold[N] = fold[0]
    assert float(fold.abs().max()) > 0 and float(case["gw"].abs().max()) > 0
    e_s, e_w = _rel(grad, fold), _rel(gw, case["gw"])
    print("relative max-norm difference: speed2", e_s, "wavelet", e_w, "misfit", abs(J - case["J"]) / case["J"])
    # measured: 4.02e-16 (speed2), 5.66e-16 (wavelet); 100x that covers other summation orders (cap 1e-9)
    assert e_s <= 4.02e-14
    assert e_w <= 5.66e-14
    assert abs(J - case["J"]) <= 1e-14 * case["J"]
    assert torch.equal(traces, reference_traces(case))
    # the faces carry no gradient, and autograd agrees
    for f in (grad[:, 0], grad[:, N], grad[:, :, 0], grad[:, :, N]):
        assert float(f.abs().max()) == 0.0
    assert float(gs[:, 0].abs().max()) == 0.0


def reference_traces(case):
    from wave3d.ops import reference

    return reference.solve_medium(N, K, case["speed2"], **_kw(case["w"], case["taper"]))[0]


def test_directional_derivative_convention(case):
    grad = case["hand"][1]
    g = torch.Generator().manual_seed(5)
    d = torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64) - 0.5
    d[N] = d[0]
    want = float((case["gs"] * d).sum())
    got = float((grad[:N] * d[:N]).sum())
    scale = float(case["gs"].abs().max()) * float(d.abs().sum())
    print("directional derivative", got, want, abs(got - want) / scale)
    # the bound of the gradient itself, on every term of the sum (measured: the two sums are equal)
    assert abs(got - want) <= 4.02e-14 * scale
    assert abs(want) > 1e-3 * float(case["gs"].abs().max())


def test_front_end_cpu_gradient(case):
    import wave3d

    prob = wave3d.MediumProblem(N, case["speed2"], timesteps=K)
    sol = wave3d.MediumSolver(prob, "cpu", **_kw(case["w"], case["taper"]))
    r = sol.gradient(case["observed"])
    assert isinstance(r, wave3d.MediumGradient)
    J, grad, gw, traces = case["hand"]
    assert r.misfit == J and torch.equal(r.grad_speed2, grad) and torch.equal(r.grad_wavelet, gw)
    assert torch.equal(r.traces, sol.run().traces)
    assert tuple(r.grad_speed2.shape) == (N + 1,) * 3 and tuple(r.grad_wavelet.shape) == (K, 2)
    assert r.total_ms > 0 and r.extra["recomputed_steps"] == 0
    # zero residual: zero misfit and gradients
    z = sol.gradient(r.traces)
    assert z.misfit == 0 and not bool(z.grad_speed2.any()) and not bool(z.grad_wavelet.any())


def test_gradient_levels():
    import wave3d

    # forward ring, m, acc (5) + q buffer; with more than one segment a second ring (3) and a
    # checkpoint pair per segment but the last
    assert wave3d.gradient_levels(24, 23) == 5 + 23          # all q stored
    assert wave3d.gradient_levels(24, 24) == 5 + 23
    assert wave3d.gradient_levels(24, 100) == 5 + 23
    assert wave3d.gradient_levels(24, 1) == 8 + 1 + 2 * 22   # 23 segments of one step
    assert wave3d.gradient_levels(24, 5) == 8 + 5 + 2 * 4    # 5 segments
    assert wave3d.gradient_levels(24, 7) == 8 + 7 + 2 * 3    # 4 segments, the last of 2 steps
    assert wave3d.gradient_levels(100, 10) == 8 + 10 + 2 * 9
    assert wave3d.gradient_levels(1, 1) == 5                 # no leapfrog step at all
    assert wave3d.gradient_levels(2, 1) == 6
    with pytest.raises(ValueError):
        wave3d.gradient_levels(24, 0)


def test_gradient_argument_checks(case):
    import wave3d

    prob = wave3d.MediumProblem(N, case["speed2"], timesteps=K)
    kw = _kw(case["w"], case["taper"])
    obs = case["observed"]
    for backend in ("cpu", "hip"):  # refused before any device is touched
        sol = wave3d.MediumSolver(prob, backend, **kw)
        with pytest.raises(ValueError, match="shape"):
            sol.gradient(obs[:-1])
        with pytest.raises(ValueError, match="shape"):
            sol.gradient(obs[:, :-1])
        with pytest.raises(ValueError, match="segment"):
            sol.gradient(obs, segment=0)
        with pytest.raises(ValueError, match="u0"):
            wave3d.MediumSolver(prob, backend, u0=torch.zeros((N + 1,) * 3), **kw).gradient(obs)
        with pytest.raises(ValueError, match="receiver"):
            wave3d.MediumSolver(prob, backend, sources=SOURCES, wavelet=case["w"]).gradient(obs[:, :0])
