"""Density perturbations in Born modelling on the CPU: ops/reference.py born_medium(ddensity=...) against
torch.autograd's forward-mode derivative of forward_medium_autograd(..., density=leaf), its linearity, the
adjoint dot test against gradient_medium_density, the Gauss-Newton product of MediumSolver.gauss_newton
over the three blocks (speed2, wavelet, density) and the argument checks.

The case is the "density" configuration of test_medium_born_cpu.py (N = 10, K = 24, its sources and
receivers, a random density in [1, 2]), with and without the sponge; the density perturbation is random
in [-0.5, 0.5] and periodic in x. born_medium honours it on the Dirichlet wall nodes (the jvp tests use
the full field); gradient_medium_density holds the wall densities fixed, so the adjoint identity is
stated for a perturbation that vanishes on the y/z faces.
"""
import pytest
import torch

from test_medium_born_cpu import N, _periodic, _ref_kw, _rel, _setup

CASES = [True, False]  # with and without the sponge

# Relative differences measured per case: (dtraces of born(drho) against autograd's jvp, max-norm; the same for
# born(ds, dw, drho); born(ds, dw, drho) against born(ds, dw) + born(drho); the adjoint dot test,
# |lhs - rhs| / |lhs|; the symmetry of the Gauss-Newton product, |<H d1, d2> - <d1, H d2>| / |<H d1, d2>|;
# |<H d, d> - |dtraces|^2| / |dtraces|^2; the dot test of the density block alone). Measured against autograd
# and against the oracle's own sums (max |dtraces| is 1.6e-2 to 2.0e-2; <H d1, d2> of the case without the
# sponge is small, 4.4e-4 against |<H d, d>| = 3.0e-3, hence its larger relative difference). The bounds are 100 times these, which covers other summation orders, capped at 1e-9; a measured 0 gets the
# floor 100 * 2^-52 (one rounding of the compared quantity).
MEASURED = {
    True: (5.385e-16, 1.514e-15, 4.732e-16, 1.539e-15, 2.733e-15, 9.062e-16, 3.441e-16),
    False: (8.873e-16, 7.366e-16, 7.800e-16, 7.571e-16, 3.139e-14, 4.399e-16, 8.220e-16),
}
EPS = 2.0 ** -52


def _bound(sponge, which):
    return min(100 * max(MEASURED[sponge][which], EPS), 1e-9)


def _inner(v):
    """v with the Dirichlet (y/z) faces zeroed: the perturbations grad_density is defined for."""
    v = v.clone()
    v[:, 0, :] = 0
    v[:, N, :] = 0
    v[:, :, 0] = 0
    v[:, :, N] = 0
    return v


@pytest.fixture(scope="module", params=CASES, ids=lambda s: "sponge" if s else "plain")
def case(request):
    from wave3d.ops import reference

    sponge = request.param
    prob, kw, ds, dw, ds2, dw2, r = _setup("density", sponge)
    g = torch.Generator().manual_seed(23)
    dr, dr2 = _periodic(g, -0.5, 0.5), _periodic(g, -0.5, 0.5)
    K = prob.timesteps
    rkw = _ref_kw(prob, kw)
    alone = reference.born_medium(N, K, prob.speed2, ddensity=dr, **rkw)
    joint = reference.born_medium(N, K, prob.speed2, ds, dw, ddensity=dr, **rkw)
    return dict(id=sponge, prob=prob, kw=kw, rkw=rkw, K=K, ds=ds, dw=dw, ds2=ds2, dw2=dw2, r=r, dr=dr, dr2=dr2,
                alone=alone, joint=joint)


def test_traces_are_solve_medium_bit_for_bit(case):
    from wave3d.ops import reference

    prob = case["prob"]
    want = reference.solve_medium(N, case["K"], prob.speed2, **case["rkw"])[0]
    assert float(want.abs().max()) > 1e-3
    for tr, dtr, duf, mx in (case["alone"], case["joint"]):
        assert torch.equal(tr, want)
        assert tuple(dtr.shape) == tuple(tr.shape) and not bool(dtr[0].any()) and float(dtr.abs().max()) > 0
        assert tuple(duf.shape) == (N + 1,) * 3 and torch.equal(duf[N], duf[0]) and len(mx) == case["K"] + 1
        assert mx[0] == 0.0 and max(mx) > 0
        assert float(dtr[:, 3].abs().max()) == 0.0  # the face receiver sees nothing


@pytest.mark.parametrize("joint", [False, True], ids=["drho", "ds-dw-drho"])
def test_dtraces_match_autograd_jvp(case, joint):
    """The full density perturbation, wall nodes included, against the jvp with a density leaf."""
    from wave3d.ops import reference

    prob, kw, K = case["prob"], case["kw"], case["K"]
    rest = {k: v for k, v in case["rkw"].items() if k not in ("wavelet", "density")}

    def fwd(s, w, rho):
        return reference.forward_medium_autograd(N, K, s, wavelet=w, density=rho, **rest)

    full = prob.speed2.expand(N + 1, N + 1, N + 1).clone()
    zero_s, zero_w = torch.zeros_like(full), torch.zeros_like(kw["wavelet"])
    tang = (case["ds"], case["dw"], case["dr"]) if joint else (zero_s, zero_w, case["dr"])
    tr, jv = torch.autograd.functional.jvp(fwd, (full, kw["wavelet"].clone(), prob.density.clone()), tang)
    born = case["joint"] if joint else case["alone"]
    assert torch.equal(tr, born[0])
    e = _rel(born[1], jv)
    print(f"sponge={case['id']} joint={joint}: dtraces against jvp, relative max-norm difference {e:.3e}, "
          f"max |dtraces| {float(jv.abs().max()):.3e}")
    assert float(jv.abs().max()) > 0
    assert e <= _bound(case["id"], 1 if joint else 0)


def test_wall_nodes_matter(case):
    """born_medium honours ddensity on the Dirichlet faces: dropping it there changes the traces."""
    from wave3d.ops import reference

    inner = reference.born_medium(N, case["K"], case["prob"].speed2, ddensity=_inner(case["dr"]), **case["rkw"])
    assert not torch.equal(inner[1], case["alone"][1])


def test_linearity(case):
    from wave3d.ops import reference

    prob, K, ds, dw, dr, rkw = case["prob"], case["K"], case["ds"], case["dw"], case["dr"], case["rkw"]
    sw = reference.born_medium(N, K, prob.speed2, ds, dw, **rkw)
    only_r = case["alone"][1]
    assert float(sw[1].abs().max()) > 0 and float(only_r.abs().max()) > 0
    e = _rel(sw[1] + only_r, case["joint"][1])
    print(f"sponge={case['id']}: born(ds, dw, drho) against born(ds, dw) + born(drho), relative max-norm "
          f"difference {e:.3e}")
    assert e <= _bound(case["id"], 2)
    # scaling by 2 is exact
    two = reference.born_medium(N, K, prob.speed2, ddensity=2 * dr, **rkw)
    assert torch.equal(two[1], 2 * only_r) and torch.equal(two[0], case["alone"][0])
    # a zero density perturbation is the run without one
    zero = reference.born_medium(N, K, prob.speed2, ds, dw, ddensity=0 * dr, **rkw)
    for a, b in zip(zero[:3], sw[:3]):
        assert torch.equal(a, b)
    assert zero[3] == sw[3]
    # a scalar is the constant field
    assert torch.equal(reference.born_medium(N, K, prob.speed2, ddensity=0.25, **rkw)[1],
                       reference.born_medium(N, K, prob.speed2, ddensity=torch.full((N + 1,) * 3, 0.25), **rkw)[1])


def test_adjoint_dot_test(case):
    """<J d, r> = <d, J^T r> over the three blocks, for a density perturbation that vanishes on the y/z faces."""
    from wave3d.ops import reference

    prob, K, ds, dw, r, rkw = case["prob"], case["K"], case["ds"], case["dw"], case["r"], case["rkw"]
    dr = _inner(case["dr"])
    tr, dtr = reference.born_medium(N, K, prob.speed2, ds, dw, ddensity=dr, **rkw)[:2]
    _, gs, gw, _, gd = reference.gradient_medium_density(N, K, prob.speed2, tr - r, **rkw)
    lhs = float((dtr[1:] * r[1:]).sum())
    parts = [float((gs[:N] * ds[:N]).sum()), float((gd[:N] * dr[:N]).sum()), float((gw * dw).sum())]
    rhs = parts[0] + parts[1] + parts[2]
    e = abs(lhs - rhs) / abs(lhs)
    print(f"sponge={case['id']}: <J d, r> = {lhs!r}, <d, J^T r> = {rhs!r} (speed2 {parts[0]!r}, density "
          f"{parts[1]!r}, wavelet {parts[2]!r}), relative difference {e:.3e}")
    assert abs(lhs) > 1e-3 * float(dtr[1:].norm() * r[1:].norm())
    assert abs(parts[1]) > 1e-3 * abs(lhs)  # the density block takes part
    assert e <= _bound(case["id"], 3)
    # the density block alone
    dtr_r = reference.born_medium(N, K, prob.speed2, ddensity=dr, **rkw)[1]
    lhs_r = float((dtr_r[1:] * r[1:]).sum())
    e_r = abs(lhs_r - parts[1]) / abs(lhs_r)
    print(f"sponge={case['id']}: density block alone: {lhs_r!r} against {parts[1]!r}, relative difference {e_r:.3e}")
    assert e_r <= _bound(case["id"], 6)


def test_gauss_newton_cpu(case):
    import wave3d

    prob, ds, dw, ds2, dw2 = case["prob"], case["ds"], case["dw"], case["ds2"], case["dw2"]
    dr, dr2 = _inner(case["dr"]), _inner(case["dr2"])
    sol = wave3d.MediumSolver(prob, "cpu", **case["kw"])
    h1, h2 = sol.gauss_newton(ds, dw, dr), sol.gauss_newton(ds2, dw2, dr2)
    assert isinstance(h1, wave3d.MediumGradient) and h1.grad_density is not None
    assert h1.extra["wrt_density"] and tuple(h1.grad_density.shape) == (N + 1,) * 3
    assert float(h1.grad_density.abs().max()) > 0
    # without ddensity nothing changes, and wrt_density can be asked for on its own
    assert sol.gauss_newton(ds, dw).grad_density is None
    assert sol.gauss_newton(ds, dw, wrt_density=True).grad_density is not None
    assert sol.gauss_newton(ds, dw, dr, wrt_density=False).grad_density is None

    def dot(h, s, w, d):
        return float((h.grad_speed2[:N] * s[:N]).sum() + (h.grad_wavelet * w).sum() + (h.grad_density[:N] * d[:N]).sum())

    a, b = dot(h1, ds2, dw2, dr2), dot(h2, ds, dw, dr)
    e_sym = abs(a - b) / abs(a)
    quad, nrm = dot(h1, ds, dw, dr), float((h1.extra["dtraces"][1:] ** 2).sum())
    e_quad = abs(quad - nrm) / nrm
    print(f"sponge={case['id']}: <H d1, d2> = {a!r}, <d1, H d2> = {b!r}, relative difference {e_sym:.3e}; "
          f"<H d, d> = {quad!r}, |dtraces|^2 = {nrm!r}, relative difference {e_quad:.3e}")
    assert nrm > 0 and h1.misfit > 0
    assert e_sym <= _bound(case["id"], 4)
    assert e_quad <= _bound(case["id"], 5)


def test_front_end_cpu_born(case):
    import wave3d

    prob, ds, dw, dr = case["prob"], case["ds"], case["dw"], case["dr"]
    sol = wave3d.MediumSolver(prob, "cpu", **case["kw"])
    r = sol.born(ds, dw, dr)
    want = case["joint"]
    assert isinstance(r, wave3d.MediumBorn) and r.extra["ddensity"] is True
    assert torch.equal(r.traces, want[0]) and torch.equal(r.dtraces, want[1]) and torch.equal(r.du_final, want[2])
    assert r.max_abs_du == want[3]
    assert torch.equal(sol.born(ddensity=dr).dtraces, case["alone"][1])
    assert sol.born(ds).extra["ddensity"] is False
    assert wave3d.born_levels() == 9 and wave3d.born_levels(density=True) == 10
    assert wave3d.born_levels(density=True, ddensity=True) == 11
    # a scalar density model takes a density perturbation too
    flat = wave3d.MediumProblem(N, prob.speed2, timesteps=prob.timesteps, density=1.5)
    assert float(wave3d.MediumSolver(flat, "cpu", **case["kw"]).born(ddensity=dr).dtraces.abs().max()) > 0


def test_argument_checks():
    import wave3d
    from wave3d.ops import reference

    prob, kw, ds, dw, _, _, _ = _setup("density", True)
    bare, bkw, _, _, _, _, _ = _setup("order2", True)
    K = prob.timesteps
    dr = _periodic(torch.Generator().manual_seed(5), -0.5, 0.5)
    for backend in ("cpu", "hip"):  # refused before any device is touched
        sol = wave3d.MediumSolver(prob, backend, **kw)
        with pytest.raises(ValueError, match="needs a density model"):
            wave3d.MediumSolver(bare, backend, **bkw).born(ddensity=dr)
        with pytest.raises(ValueError, match="needs a density model"):
            wave3d.MediumSolver(bare, backend, **bkw).gauss_newton(ds, ddensity=dr)
        with pytest.raises(ValueError, match="perturbation"):
            sol.born()
        with pytest.raises(ValueError, match="perturbation"):
            sol.gauss_newton()
        with pytest.raises(ValueError, match="ddensity must be a scalar or have shape"):
            sol.born(ddensity=dr[:-1])
        for v in (float("nan"), float("inf")):
            bad = dr.clone()
            bad[3, 4, 5] = v
            with pytest.raises(ValueError, match="ddensity must be finite"):
                sol.born(ds, ddensity=bad)
        bad = dr.clone()
        bad[N, 2, 3] += 1.0
        with pytest.raises(ValueError, match="ddensity must be periodic"):
            sol.born(ddensity=bad)
    # the oracle checks its own arguments
    rkw = _ref_kw(prob, kw)
    with pytest.raises(ValueError, match="perturbation"):
        reference.born_medium(N, K, prob.speed2, **rkw)
    with pytest.raises(ValueError, match="needs a density model"):
        reference.born_medium(N, bare.timesteps, bare.speed2, ddensity=dr, **_ref_kw(bare, bkw))
    with pytest.raises(ValueError, match="periodic"):
        reference.born_medium(N, K, prob.speed2, ddensity=bad, **rkw)
    with pytest.raises(ValueError, match="shape"):
        reference.born_medium(N, K, prob.speed2, ddensity=dr[:, 1:], **rkw)
    shape = (N + 3, N + 1, N + 1)
    z = torch.zeros(shape, dtype=torch.float64)
    box = reference._medium_box(N)
    s = torch.zeros(N + 1, N - 1, N - 1, dtype=torch.float64)
    with pytest.raises(ValueError, match="first"):
        reference.step_medium(z, z, z, box, first=True, hx2=1.0, hy2=1.0, hz2=1.0, born_add=s)
    with pytest.raises(ValueError, match="shape"):
        reference.step_medium(z, z, z, box, first=False, hx2=1.0, hy2=1.0, hz2=1.0, born_add=s[1:])
    with pytest.raises(ValueError, match="combined"):
        reference.step_medium(z, z, z, box, first=False, hx2=1.0, hy2=1.0, hz2=1.0, born_add=s, born=(s, z))
    # born_add with the scattering term formed by hand is Born mode
    g = torch.Generator().manual_seed(3)
    u1, u2, m, dm = (torch.rand(shape, generator=g, dtype=torch.float64) for _ in range(4))
    q = torch.rand(N + 1, N - 1, N - 1, generator=g, dtype=torch.float64)
    own = (slice(1, N + 2), slice(1, N), slice(1, N))
    assert torch.equal(reference.step_medium(u1, u2, m, box, first=False, hx2=1.0, hy2=1.0, hz2=1.0, born=(q, dm)),
                       reference.step_medium(u1, u2, m, box, first=False, hx2=1.0, hy2=1.0, hz2=1.0,
                                             born_add=dm[own] * q))
    # the buoyancy perturbation: -(drho / rho^2), x ghosts periodic
    db = reference.dbuoyancy_field(dr, prob.density, N, torch.float64)
    assert tuple(db.shape) == shape and torch.equal(db[1:N + 2], -(dr / (prob.density * prob.density)))
    assert torch.equal(db[0], db[N]) and torch.equal(db[N + 2], db[2])
