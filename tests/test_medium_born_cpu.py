"""Born (linearised) modelling of the medium solver on the CPU: ops/reference.py born_medium against
torch.autograd's forward-mode derivative of forward_medium_autograd, its linearity, the adjoint dot
test against gradient_medium, the Gauss-Newton product of MediumSolver.gauss_newton and the
argument checks of MediumSolver.born.

The shared case is that of test_medium_gradient_cpu.py (N = 10, its sources and receivers, sponge
width 3) at the space orders 2, 4 and 8 and at order 2 with a random density in [1, 2], each with
and without the sponge; K is large enough for the order's Courant limit.
"""
import pytest
import torch

from test_medium_gradient_cpu import N, RECEIVERS, SOURCES

# name -> (space order, K, density?)
CONFIGS = {"order2": (2, 16, False), "order4": (4, 32, False), "order8": (8, 32, False), "density": (2, 24, True)}
CASES = [(name, sponge) for name in CONFIGS for sponge in (True, False)]

# Relative max-norm differences measured per case: (dtraces against autograd's jvp; born(ds, dw) against
# born(ds) + born(0 ds, dw); the adjoint dot test, |lhs - rhs| / |lhs|; the symmetry of the Gauss-Newton
# product, |<H d1, d2> - <d1, H d2>| / |<H d1, d2>|; |<H d, d> - |dtraces|^2| / |dtraces|^2). The bounds are
# 100 times these, which covers other summation orders, capped at 1e-9; a measured 0 gets the floor
# 100 * 2^-52 (one rounding of the compared quantity).
MEASURED = {
    ("order2", True): (8.608e-16, 1.23e-16, 0.0, 6.006e-16, 1.393e-16),
    ("order2", False): (7.516e-16, 5.261e-16, 1.277e-15, 6.357e-16, 3.345e-16),
    ("order4", True): (2.086e-16, 5.215e-16, 8.466e-16, 5.139e-15, 5.637e-16),
    ("order4", False): (3.832e-16, 1.259e-15, 8.097e-15, 1.036e-14, 1.533e-16),
    ("order8", True): (6.311e-16, 5.86e-16, 2.161e-15, 1.048e-15, 0.0),
    ("order8", False): (1.804e-15, 1.017e-15, 1.421e-15, 1.407e-15, 8.205e-16),
    ("density", True): (1.295e-15, 5.394e-16, 8.078e-16, 1.134e-15, 4.033e-16),
    ("density", False): (1.721e-15, 7.374e-16, 6.143e-16, 5.621e-16, 0.0),
}
EPS = 2.0 ** -52


def _bound(case, which):
    return min(100 * max(MEASURED[case][which], EPS), 1e-9)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _periodic(g, lo, hi):
    v = lo + (hi - lo) * torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64)
    v[N] = v[0]
    return v


def _setup(name, sponge):
    """The problem of a case and its perturbations: (problem, solver keywords, ds, dw, ds2, dw2, r)."""
    import wave3d

    order, K, dens = CONFIGS[name]
    g = torch.Generator().manual_seed(11)
    speed2 = _periodic(g, 2.0, 4.0)
    rho = _periodic(g, 1.0, 2.0) if dens else None
    tau = 1.0 / K
    w = torch.stack([wave3d.ricker(3.0, 0.3, K, tau), -0.5 * wave3d.ricker(2.0, 0.2, K, tau)], 1)
    prob = wave3d.MediumProblem(N, speed2, timesteps=K, space_order=order, density=rho)
    kw = dict(sources=SOURCES, wavelet=w, receivers=RECEIVERS, taper=wave3d.sponge_taper(prob, 3) if sponge else None)
    ds, ds2 = _periodic(g, -0.5, 0.5), _periodic(g, -0.5, 0.5)
    dw = torch.rand(K, len(SOURCES), generator=g, dtype=torch.float64) - 0.5
    dw2 = torch.rand(K, len(SOURCES), generator=g, dtype=torch.float64) - 0.5
    r = torch.rand(K + 1, len(RECEIVERS), generator=g, dtype=torch.float64) - 0.5
    return prob, kw, ds, dw, ds2, dw2, r


def _ref_kw(prob, kw):
    return dict(kw, order=prob.space_order, density=prob.density)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{'sponge' if c[1] else 'plain'}")
def case(request):
    from wave3d.ops import reference

    name, sponge = request.param
    prob, kw, ds, dw, ds2, dw2, r = _setup(name, sponge)
    K = prob.timesteps
    born = reference.born_medium(N, K, prob.speed2, ds, dw, **_ref_kw(prob, kw))
    return dict(id=request.param, prob=prob, kw=kw, K=K, ds=ds, dw=dw, ds2=ds2, dw2=dw2, r=r, born=born)


def test_traces_are_solve_medium_bit_for_bit(case):
    from wave3d.ops import reference

    prob, kw = case["prob"], case["kw"]
    tr, dtr, duf, mx = case["born"]
    want = reference.solve_medium(N, case["K"], prob.speed2, **_ref_kw(prob, kw))[0]
    assert float(want.abs().max()) > 1e-3
    assert torch.equal(tr, want)
    assert tuple(dtr.shape) == tuple(tr.shape) and not bool(dtr[0].any()) and float(dtr.abs().max()) > 0
    assert tuple(duf.shape) == (N + 1,) * 3 and torch.equal(duf[N], duf[0]) and len(mx) == case["K"] + 1
    assert mx[0] == 0.0 and max(mx) > 0
    # the face receiver sees nothing
    assert float(dtr[:, 3].abs().max()) == 0.0


def test_dtraces_match_autograd_jvp(case):
    from wave3d.ops import reference

    prob, kw, K = case["prob"], case["kw"], case["K"]
    rest = {k: v for k, v in _ref_kw(prob, kw).items() if k != "wavelet"}

    def fwd(s, w):
        return reference.forward_medium_autograd(N, K, s, wavelet=w, **rest)

    full = prob.speed2.expand(N + 1, N + 1, N + 1).clone()
    tr, jv = torch.autograd.functional.jvp(fwd, (full, kw["wavelet"].clone()), (case["ds"], case["dw"]))
    assert torch.equal(tr, case["born"][0])
    e = _rel(case["born"][1], jv)
    print(f"{case['id']}: dtraces against jvp, relative max-norm difference {e:.3e}")
    assert float(jv.abs().max()) > 0
    assert e <= _bound(case["id"], 0)


def test_linearity(case):
    from wave3d.ops import reference

    prob, K, ds, dw = case["prob"], case["K"], case["ds"], case["dw"]
    kw = _ref_kw(prob, case["kw"])
    both = case["born"][1]
    only_s = reference.born_medium(N, K, prob.speed2, ds, None, **kw)[1]
    only_w = reference.born_medium(N, K, prob.speed2, 0 * ds, dw, **kw)[1]
    assert float(only_s.abs().max()) > 0 and float(only_w.abs().max()) > 0
    e = _rel(only_s + only_w, both)
    print(f"{case['id']}: born(ds, dw) against born(ds) + born(0, dw), relative max-norm difference {e:.3e}")
    assert e <= _bound(case["id"], 1)
    # dwavelet alone (dm = 0) is the same run
    assert torch.equal(reference.born_medium(N, K, prob.speed2, None, dw, **kw)[1], only_w)
    # scaling by 2 is exact
    two = reference.born_medium(N, K, prob.speed2, 2 * ds, None, **kw)
    assert torch.equal(two[1], 2 * only_s) and torch.equal(two[0], case["born"][0])


def test_adjoint_dot_test(case):
    from wave3d.ops import reference

    prob, K, ds, dw, r = case["prob"], case["K"], case["ds"], case["dw"], case["r"]
    tr, dtr = case["born"][:2]
    _, gs, gw, _ = reference.gradient_medium(N, K, prob.speed2, tr - r, **_ref_kw(prob, case["kw"]))
    lhs = float((dtr[1:] * r[1:]).sum())
    rhs = float((gs[:N] * ds[:N]).sum() + (gw * dw).sum())
    e = abs(lhs - rhs) / abs(lhs)
    print(f"{case['id']}: <J d, r> = {lhs!r}, <d, J^T r> = {rhs!r}, relative difference {e:.3e}")
    assert abs(lhs) > 1e-3 * float(dtr[1:].norm() * r[1:].norm())
    assert e <= _bound(case["id"], 2)


def test_gauss_newton_cpu(case):
    import wave3d

    prob, ds, dw, ds2, dw2 = case["prob"], case["ds"], case["dw"], case["ds2"], case["dw2"]
    sol = wave3d.MediumSolver(prob, "cpu", **case["kw"])
    h1, h2 = sol.gauss_newton(ds, dw), sol.gauss_newton(ds2, dw2)
    assert isinstance(h1, wave3d.MediumGradient)
    assert torch.equal(h1.extra["dtraces"], case["born"][1]) and torch.equal(h1.traces, case["born"][0])

    def dot(h, s, w):
        return float((h.grad_speed2[:N] * s[:N]).sum() + (h.grad_wavelet * w).sum())

    a, b = dot(h1, ds2, dw2), dot(h2, ds, dw)
    e_sym = abs(a - b) / abs(a)
    quad, nrm = dot(h1, ds, dw), float((h1.extra["dtraces"][1:] ** 2).sum())
    e_quad = abs(quad - nrm) / nrm
    print(f"{case['id']}: <H d1, d2> = {a!r}, <d1, H d2> = {b!r}, relative difference {e_sym:.3e}; "
          f"<H d, d> = {quad!r}, |dtraces|^2 = {nrm!r}, relative difference {e_quad:.3e}")
    assert nrm > 0 and h1.misfit > 0
    assert e_sym <= _bound(case["id"], 3)
    assert e_quad <= _bound(case["id"], 4)


def test_front_end_cpu_born():
    import wave3d
    from wave3d.ops import reference

    prob, kw, ds, dw, _, _, _ = _setup("order2", True)
    sol = wave3d.MediumSolver(prob, "cpu", **kw)
    r = sol.born(ds, dw)
    assert isinstance(r, wave3d.MediumBorn)
    want = reference.born_medium(N, prob.timesteps, prob.speed2, ds, dw, **kw)
    assert torch.equal(r.traces, want[0]) and torch.equal(r.dtraces, want[1]) and torch.equal(r.du_final, want[2])
    assert r.max_abs_du == want[3] and r.total_ms > 0
    assert torch.equal(r.traces, sol.run().traces)
    # a scalar perturbation is the constant field
    assert torch.equal(sol.born(0.25).dtraces, sol.born(torch.full((N + 1,) * 3, 0.25)).dtraces)
    assert wave3d.born_levels() == 9 and wave3d.born_levels(density=True) == 10


def test_born_argument_checks():
    import wave3d
    from wave3d.ops import reference

    prob, kw, ds, dw, _, _, _ = _setup("order2", True)
    K = prob.timesteps
    for backend in ("cpu", "hip"):  # refused before any device is touched
        sol = wave3d.MediumSolver(prob, backend, **kw)
        with pytest.raises(ValueError, match="u0"):
            wave3d.MediumSolver(prob, backend, u0=torch.zeros((N + 1,) * 3), **kw).born(ds)
        with pytest.raises(ValueError, match="receiver"):
            wave3d.MediumSolver(prob, backend, sources=SOURCES, wavelet=kw["wavelet"]).born(ds)
        with pytest.raises(ValueError, match="perturbation"):
            sol.born()
        with pytest.raises(ValueError, match="perturbation"):
            sol.gauss_newton()
        with pytest.raises(ValueError, match="shape"):
            sol.born(ds[:-1])
        with pytest.raises(ValueError, match="shape"):
            sol.born(ds, dw[:-1])
        with pytest.raises(ValueError, match="shape"):
            sol.born(None, dw[:, :1])
        bad = ds.clone()
        bad[3, 4, 5] = float("nan")
        with pytest.raises(ValueError, match="finite"):
            sol.born(bad)
        bad = ds.clone()
        bad[2, 2, 2] = float("inf")
        with pytest.raises(ValueError, match="finite"):
            sol.born(bad)
        bad = ds.clone()
        bad[N, 2, 3] += 1.0
        with pytest.raises(ValueError, match="periodic"):
            sol.born(bad)
        bad = dw.clone()
        bad[1, 0] = float("nan")
        with pytest.raises(ValueError, match="finite"):
            sol.born(None, bad)
    # the oracle checks its own arguments
    rkw = _ref_kw(prob, kw)
    with pytest.raises(ValueError, match="perturbation"):
        reference.born_medium(N, K, prob.speed2, **rkw)
    with pytest.raises(ValueError, match="periodic"):
        reference.born_medium(N, K, prob.speed2, bad_periodic(ds), **rkw)
    with pytest.raises(ValueError, match="shape"):
        reference.born_medium(N, K, prob.speed2, None, dw[:-1], **rkw)
    shape = (N + 3, N + 1, N + 1)
    z = torch.zeros(shape, dtype=torch.float64)
    box = reference._medium_box(N)
    q = torch.zeros(N + 1, N - 1, N - 1, dtype=torch.float64)
    with pytest.raises(ValueError, match="first"):
        reference.step_medium(z, z, z, box, first=True, hx2=1.0, hy2=1.0, hz2=1.0, born=(q, z))
    with pytest.raises(ValueError, match="shape"):
        reference.step_medium(z, z, z, box, first=False, hx2=1.0, hy2=1.0, hz2=1.0, born=(q[1:], z))


def bad_periodic(ds):
    bad = ds.clone()
    bad[0, 1, 1] -= 1.0
    return bad
