"""Density gradients (dJ/drho) of the medium solver on the CPU: the hand-written adjoint
(ops/reference.py gradient_medium_density, face_correlation, finish_gradient_density) against
torch.autograd through forward_medium_autograd with a density leaf, the properties of the face
correlation, the level planning with ``wrt_density`` and the front-end keyword.
"""
import pytest
import torch

F64 = torch.float64
N, K = 10, 9
BOX = (3.0, 3.4, 2.8)                                           # not a cube: three different h
SOURCES = [(0, 4, 6), (6, 3, 5)]                                # one on the periodic plane, one interior
RECEIVERS = [(N, 7, 3), (4, 5, 5), (5, 1, 1), (2, N - 1, 4), (7, 6, 2)]  # two of them next to the walls


def _layered(seed):
    """Layered rho and c^2 with a little noise, periodic in x."""
    g = torch.Generator().manual_seed(seed)
    rho = torch.ones((N + 1,) * 3, dtype=F64)
    rho[:, :, N // 2:] = 2.5
    rho[:, N // 3:, :] *= 1.3
    rho = rho * (1 + 0.1 * torch.rand((N + 1,) * 3, generator=g, dtype=F64))
    speed2 = torch.full((N + 1,) * 3, 0.3, dtype=F64)
    speed2[:, :, 2 * N // 3:] = 0.6
    speed2 = speed2 * (1 + 0.1 * torch.rand((N + 1,) * 3, generator=g, dtype=F64))
    rho[N], speed2[N] = rho[0], speed2[0]
    return rho, speed2


def _problem(density):
    import wave3d

    _, speed2 = _layered(31)
    return wave3d.MediumProblem(N, speed2, *BOX, timesteps=K, density=density)


def _solver(backend, density):
    import wave3d

    prob = _problem(density)
    w = 1e4 * torch.stack([wave3d.ricker(3.0, 0.3, K, prob.tau), -0.5 * wave3d.ricker(2.0, 0.2, K, prob.tau)], 1)
    return wave3d.MediumSolver(prob, backend, sources=SOURCES, wavelet=w, receivers=RECEIVERS,
                               taper=wave3d.sponge_taper(prob, 3))


@pytest.fixture(scope="module")
def case():
    """The shared case: observed = the traces of a perturbed model; autograd's and the adjoint's gradients."""
    from wave3d.ops import reference

    rho, speed2 = _layered(31)
    sol = _solver("cpu", rho)
    kw = dict(sources=SOURCES, wavelet=sol.wavelet, receivers=RECEIVERS, taper=sol.taper, L=BOX)
    observed = reference.solve_medium(N, K, speed2 * 1.1, density=rho * 0.9, **kw)[0]
    r = rho.clone().requires_grad_(True)
    s = speed2.clone().requires_grad_(True)
    tr = reference.forward_medium_autograd(N, K, s, density=r, **kw)
    J = 0.5 * ((tr[1:] - observed[1:]) ** 2).sum()
    g_rho, g_s = torch.autograd.grad(J, (r, s))
    hand = reference.gradient_medium_density(N, K, speed2, observed, density=rho, **kw)
    plain = reference.gradient_medium(N, K, speed2, observed, density=rho, **kw)
    return dict(rho=rho, speed2=speed2, kw=kw, observed=observed, J=J.item(), g_rho=g_rho, g_s=g_s, hand=hand,
                plain=plain)


def _fold(g):
    """autograd treats planes 0 and N as two leaves: the unique node gets both."""
    f = g.clone()
    f[0] = g[0] + g[N]
    f[N] = f[0]
    return f


def test_grad_density_matches_autograd(case):
    J, gs, gw, traces, gd = case["hand"]
    fr, fs = _fold(case["g_rho"]), _fold(case["g_s"])
    own = (slice(None), slice(1, N), slice(1, N))  # the stencil nodes: every x plane, j and k in 1..N-1
    scale = float(fr.abs().max())
    e_rho = float((gd[own] - fr[own]).abs().max()) / scale
    e_s = float((gs[own] - fs[own]).abs().max()) / float(fs.abs().max())
    wall = torch.cat([fr[:, 0].flatten(), fr[:, N].flatten(), fr[:, :, 0].flatten(), fr[:, :, N].flatten()])
    print("relative max-norm deviation from autograd: grad_density", e_rho, "grad_speed2", e_s,
          "max |autograd dJ/drho|", scale, "on the wall nodes", float(wall.abs().max()))
    assert scale > 1e-3 and case["J"] > 0
    # the bound of test_gradient_matches_autograd for dJ/dspeed2 with a density; measured here:
    # 7.9e-16 (grad_density), 2.4e-16 (grad_speed2), of max |dJ/drho| = 5.5e-3
    assert e_rho <= 1e-12
    assert e_s <= 1e-12
    assert abs(J - case["J"]) <= 1e-14 * case["J"]
    # the wall nodes' densities are held fixed: reported as exactly 0 (what autograd has there is printed)
    for f in (gd[:, 0], gd[:, N], gd[:, :, 0], gd[:, :, N]):
        assert float(f.abs().max()) == 0.0
    assert torch.equal(gd[N], gd[0]) and float(gd[0].abs().max()) > 0
    assert tuple(gd.shape) == (N + 1,) * 3 and gd.dtype == F64


def test_first_four_outputs_are_gradient_medium_bit_for_bit(case):
    assert len(case["hand"]) == 5 and len(case["plain"]) == 4
    assert case["hand"][0] == case["plain"][0]
    for a, b in zip(case["hand"][1:4], case["plain"][1:4]):
        assert torch.equal(a, b)


def test_gradient_medium_density_needs_a_density(case):
    from wave3d.ops import reference

    with pytest.raises(ValueError, match="density"):
        reference.gradient_medium_density(N, K, case["speed2"], case["observed"], **case["kw"])


def test_directional_derivative_in_density(case):
    """(grad[:N] * d[:N]).sum() is the derivative along a periodic perturbation d that leaves the walls alone."""
    gd = case["hand"][4]
    g = torch.Generator().manual_seed(5)
    d = torch.rand((N + 1,) * 3, generator=g, dtype=F64) - 0.5
    d[N] = d[0]
    d[:, 0], d[:, N], d[:, :, 0], d[:, :, N] = 0, 0, 0, 0
    want = float((case["g_rho"] * d).sum())
    got = float((gd[:N] * d[:N]).sum())
    scale = float(case["g_rho"].abs().max()) * float(d.abs().sum())
    print("directional derivative", got, want, abs(got - want) / scale)
    assert abs(got - want) <= 1e-12 * scale  # the bound of the gradient itself, on every term of the sum
    assert abs(want) > 1e-3 * float(case["g_rho"].abs().max())


# ---- the face correlation ----------------------------------------------------------------------

H2 = (0.011, 0.013, 0.017)
SHAPE = (9, 12, 14)
INNER = (1, SHAPE[0] - 2, 1, SHAPE[1] - 2, 1, SHAPE[2] - 2)


def _rand(seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(SHAPE, generator=g, dtype=F64)


def _zero_rings(v, rings):
    for r in range(rings):
        v[r], v[-1 - r], v[:, r], v[:, -1 - r], v[:, :, r], v[:, :, -1 - r] = 0, 0, 0, 0, 0, 0
    return v


def test_face_correlation_is_symmetric_bit_for_bit():
    from wave3d.ops import reference

    a, v = _rand(1), _rand(2)
    box = (2, 6, 1, 9, 3, 12)
    c = reference.face_correlation(a, v, box, *H2)
    assert tuple(c.shape) == (5, 9, 10) and float(c.abs().max()) > 1
    assert torch.equal(c, reference.face_correlation(v, a, box, *H2))
    c32 = reference.face_correlation(a.float(), v.float(), box, *H2)
    assert c32.dtype == torch.float32 and torch.equal(c32, reference.face_correlation(v.float(), a.float(), box, *H2))
    for bad in ((0, 6, 1, 9, 3, 12), (2, 8, 1, 9, 3, 12), (2, 6, 0, 9, 3, 12), (2, 6, 1, 11, 3, 12),
                (2, 6, 1, 9, 0, 12), (2, 6, 1, 9, 3, 13)):
        with pytest.raises(ValueError, match="edge"):
            reference.face_correlation(a, v, bad, *H2)
    with pytest.raises(ValueError, match="match"):
        reference.face_correlation(a, v[:, :, :-1], box, *H2)


def test_a_face_is_seen_alike_from_both_of_its_nodes():
    """Every face with a non-zero product lies between two box nodes: sum_box C = 2 sum_faces."""
    from wave3d.ops import reference

    a, v = _zero_rings(_rand(3), 2), _zero_rings(_rand(4), 2)
    total = float(reference.face_correlation(a, v, INNER, *H2).sum())
    faces = sum(float((torch.diff(a, dim=ax) * torch.diff(v, dim=ax)).sum()) / H2[ax] for ax in range(3))
    print("sum_box C", total, "2 sum_faces", 2 * faces)
    assert abs(faces) > 1 and abs(total - 2 * faces) <= 1e-12 * abs(total)


def test_face_correlation_is_the_derivative_with_respect_to_the_buoyancy():
    """d <a, D_b v> / d b = -C(a, v) / 2 on the stencil nodes, for a vanishing on the faces (unequal h)."""
    from wave3d.ops import reference

    a, v = _zero_rings(_rand(5), 1), _rand(6)
    b = _rand(7, 0.3, 2.0).requires_grad_(True)
    inner = (slice(1, -1),) * 3
    dot = (a[inner] * reference.laplace_density(v, b, *H2)).sum()
    gb, = torch.autograd.grad(dot, b)
    want = -0.5 * reference.face_correlation(a, v, INNER, *H2)
    scale = float(want.abs().max())
    err = float((gb[inner] - want).abs().max()) / scale
    print("d<a, D_b v>/db against -C/2: relative max-norm deviation", err, "of", scale)
    assert scale > 1 and err <= 1e-12


# ---- level planning ----------------------------------------------------------------------------

def test_gradient_levels_with_wrt_density():
    import wave3d

    for k in (1, 2, 3, 9, 24, 100):
        counts = {}
        for s in range(1, k + 3):
            base = wave3d.gradient_levels(k, s, density=True)
            counts[s] = wave3d.gradient_levels(k, s, density=True, wrt_density=True)
            assert counts[s] == base + min(s, k - 1) + 1
            # the defaults are today's
            assert wave3d.gradient_levels(k, s, density=True, wrt_density=False) == base
            assert wave3d.gradient_levels(k, s, wrt_density=False) == wave3d.gradient_levels(k, s) == base - 1
        best = wave3d.best_gradient_segment(k, wrt_density=True)
        assert 1 <= best <= max(k - 1, 1) and counts[best] == min(counts.values())
        assert wave3d.best_gradient_segment(k, wrt_density=False) == wave3d.best_gradient_segment(k)
    assert wave3d.gradient_levels(24, 5) == 8 + 5 + 2 * 4
    assert wave3d.gradient_levels(24, 5, wrt_density=True) == 8 + 5 + 2 * 4 + 5 + 1
    assert wave3d.gradient_levels(100, 10, density=True, wrt_density=True) == 9 + 10 + 2 * 9 + 10 + 1
    assert wave3d.best_gradient_segment(100) == min(range(1, 100), key=lambda s: (wave3d.gradient_levels(100, s), -s))


# ---- the front-end -----------------------------------------------------------------------------

def test_front_end_cpu_grad_density(case):
    import wave3d

    sol = _solver("cpu", case["rho"])
    r = sol.gradient(case["observed"], wrt_density=True)
    J, gs, gw, traces, gd = case["hand"]
    assert isinstance(r, wave3d.MediumGradient) and r.extra["wrt_density"] is True
    assert r.misfit == J and torch.equal(r.grad_speed2, gs) and torch.equal(r.grad_wavelet, gw)
    assert torch.equal(r.traces, traces) and torch.equal(r.grad_density, gd)
    assert tuple(r.grad_density.shape) == (N + 1,) * 3
    off = sol.gradient(case["observed"])
    assert off.grad_density is None and off.extra["wrt_density"] is False
    assert torch.equal(off.grad_speed2, gs) and torch.equal(off.grad_wavelet, gw)


def test_front_end_scalar_density(case):
    """A scalar density is a model too: the gradient is that of the constant field."""
    sol = _solver("cpu", 1.7)
    r = sol.gradient(case["observed"], wrt_density=True)
    full = _solver("cpu", torch.full((N + 1,) * 3, 1.7, dtype=F64)).gradient(case["observed"], wrt_density=True)
    assert float(r.grad_density.abs().max()) > 0 and torch.equal(r.grad_density, full.grad_density)


def test_wrt_density_needs_a_density_model(case):
    for backend in ("cpu", "hip"):  # refused before any device is touched
        sol = _solver(backend, None)
        with pytest.raises(ValueError, match="density="):
            sol.gradient(case["observed"], wrt_density=True)
