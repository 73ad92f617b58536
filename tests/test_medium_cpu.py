"""Variable-speed medium: the PyTorch oracle (ops/reference.py solve_medium) and the front-end
(models/medium.py) on the CPU.

A uniform medium must reproduce the constant-speed oracle bit for bit; a heterogeneous one must
obey source-receiver reciprocity (the operator of (1/c^2) u_tt = lap u + f is symmetric) and the
x periodicity of the grid.
"""
import math
import warnings

import pytest
import torch

N, K = 16, 48
A, B, C3 = (3, 5, 11), (12, 9, 4), (7, 7, 7)


def _analytic0(n, k, dtype):
    from wave3d.ops import reference

    sx, sy, sz, ct, c = reference.tables(n, k, dtype=dtype)
    return reference.analytic(sx, sy, sz, ct[0]), c


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_uniform_medium_reproduces_constant_speed_oracle(dtype):
    import wave3d
    from wave3d.ops import reference

    dt = {"fp64": torch.float64, "fp32": torch.float32}[dtype]
    u0, c = _analytic0(16, 20, dt)
    prob = wave3d.MediumProblem(16, c["a2"], timesteps=20, dtype=dtype)
    res = wave3d.MediumSolver(prob, "cpu", u0=u0).run()
    exp = reference.solve(16, 20, dtype=dt)[2]
    assert res.u_final.dtype == dt and tuple(res.u_final.shape) == (17, 17, 17)
    assert torch.equal(res.u_final, exp[1:18])
    assert len(res.max_abs_u) == 21 and not res.aborted
    if dtype == "fp64":
        sx, sy, sz, ct, _ = reference.tables(16, 20)
        f = reference.analytic(sx[1:16], sy[1:16], sz[1:16], ct[20])
        assert f"{reference.max_errors(res.u_final[1:16, 1:16, 1:16], f)[0]:.4e}" == "7.0844e-04"


def hetero_case():
    """The heterogeneous case shared with the GPU tests: speed2 in [4, 8), Ricker source."""
    import wave3d

    g = torch.Generator().manual_seed(3)
    speed2 = 4 + 4 * torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64)
    speed2[N] = speed2[0]
    tau = 1.0 / K
    return speed2, wave3d.ricker(4.0, 0.25, K, tau).reshape(K, 1)


def _trace(speed2, w, src, rec, dtype="fp64"):
    import wave3d

    prob = wave3d.MediumProblem(N, speed2, T=1.0, timesteps=K, dtype=dtype)
    return wave3d.MediumSolver(prob, "cpu", sources=[src], wavelet=w, receivers=[rec]).run()


def test_reciprocity():
    speed2, w = hetero_case()
    ab = _trace(speed2, w, A, B)
    ba = _trace(speed2, w, B, A)
    cb = _trace(speed2, w, C3, B)
    assert tuple(ab.traces.shape) == (K + 1, 1)
    # sqrt(8) (1/48) / (pi/16) = 0.30, i.e. 0.52 of the stability limit 1/sqrt(3)
    assert 0.25 < ab.courant < 1 / math.sqrt(3)
    peak = float(ab.traces.abs().max())
    assert peak > 1e-3 and max(ab.max_abs_u) < 2
    assert float((ab.traces - ba.traces).abs().max()) <= 1e-12 * peak
    # not vacuous: another source position is heard differently at B
    assert float((cb.traces - ab.traces).abs().max()) > 1e-3 * peak


def test_periodic_plane():
    import wave3d

    speed2, w = hetero_case()
    prob = wave3d.MediumProblem(N, speed2, timesteps=K)
    res = wave3d.MediumSolver(prob, "cpu", sources=[(0, 5, 7)], wavelet=w,
                              receivers=[(0, 6, 7), (N, 6, 7)]).run()
    assert float(res.traces.abs().max()) > 0
    assert torch.equal(res.traces[:, 0], res.traces[:, 1])
    assert torch.equal(res.u_final[0], res.u_final[N])


def test_ricker():
    import wave3d

    w = wave3d.ricker(4.0, 0.25, 48, 1 / 48)
    assert tuple(w.shape) == (48,) and w.dtype == torch.float64
    assert w[12].item() == 1.0  # t = t0
    a = (math.pi * 4.0 * (5 / 48 - 0.25)) ** 2
    assert math.isclose(w[5].item(), (1 - 2 * a) * math.exp(-a), rel_tol=1e-14)


def test_validation():
    import wave3d

    speed2, w = hetero_case()
    with pytest.raises(ValueError, match="Courant"):
        wave3d.MediumProblem(N, speed2, timesteps=10)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        p = wave3d.MediumProblem(N, speed2, timesteps=10, strict_cfl=False)
    assert any("Courant" in str(r.message) for r in rec) and not p.stable()
    assert p.min_stable_timesteps() > 10
    assert wave3d.MediumProblem(N, speed2, timesteps=p.min_stable_timesteps()).stable()

    bad = speed2.clone()
    bad[N, 2, 3] += 1.0
    with pytest.raises(ValueError, match="periodic"):
        wave3d.MediumProblem(N, bad, timesteps=K)
    neg = speed2.clone()
    neg[1, 2, 3] = -2.5
    with pytest.raises(ValueError, match="-2.5"):
        wave3d.MediumProblem(N, neg, timesteps=K)
    with pytest.raises(ValueError, match="nan"):
        wave3d.MediumProblem(N, float("nan"), timesteps=K)

    prob = wave3d.MediumProblem(N, speed2, timesteps=K)
    with pytest.raises(ValueError, match="Dirichlet"):
        wave3d.MediumSolver(prob, "cpu", sources=[(3, 0, 5)], wavelet=w)
    with pytest.raises(ValueError, match="Dirichlet"):
        wave3d.MediumSolver(prob, "cpu", sources=[(3, 4, N)], wavelet=w)
    w2 = torch.cat([w, w], dim=1)
    with pytest.raises(ValueError, match="more than once"):
        wave3d.MediumSolver(prob, "cpu", sources=[A, A], wavelet=w2)
    with pytest.raises(ValueError, match="more than once"):  # planes 0 and N are one plane
        wave3d.MediumSolver(prob, "cpu", sources=[(0, 5, 7), (N, 5, 7)], wavelet=w2)
    with pytest.raises(ValueError, match="wavelet"):
        wave3d.MediumSolver(prob, "cpu", sources=[A], wavelet=w2)
    with pytest.raises(ValueError, match="wavelet"):
        wave3d.MediumSolver(prob, "cpu", sources=[A], wavelet=w[:-1])
    with pytest.raises(ValueError, match="wavelet"):
        wave3d.MediumSolver(prob, "cpu", sources=[A])
