"""Misfit gradients on the GPU: the save / image modes of k_march_m (csrc/hip_medium.hip) against
the plain-PyTorch oracle, and MediumSolver.gradient ("hip": checkpoint / recompute schedule, the
adjoint field on k_march_m itself) against ops/reference.py gradient_medium.

fp64 results must be *bitwise* equal: both sides round every operation in the same order and share
the host-side arithmetic (reference.adjoint_source_table, finish_gradient_medium); a single fp32 step in
save or image mode is bitwise equal too.
"""
import warnings

import pytest
import torch

from bits import assert_same_bits
from test_gpu_medium import CASES, H2, _cast, _inputs, _rand

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -7.0


def _taper(shape, dtype, on):
    if not on:
        return None
    return tuple(_rand((n,), dtype, 20 + a, 0.5, 1.0) for a, n in enumerate(shape))


def _dense(t, padded):
    """A device copy of the CPU tensor t: dense, or an alloc_level padded view."""
    from wave3d.ops import kernels

    if not padded:
        return t.to(DEV)
    v = kernels.alloc_level(*t.shape, t.dtype)
    v.copy_(t)
    return v


def _mode_case(shape, box, chunk, dtype, sponge, padded, mode):
    """Run the plain step and the step in `mode`; returns everything the checks need."""
    from wave3d.ops import kernels, reference

    u1, u2, m = _inputs(shape, dtype)
    q = _rand(shape, dtype, 4, -1.0, 1.0)
    acc0 = _rand(shape, dtype, 5, -1.0, 1.0)
    tp = _taper(shape, dtype, sponge)
    d = [_dense(t, padded) for t in (u1, u2, m)]
    tpd = None if tp is None else tuple(t.to(DEV) for t in tp)
    ei = (box[0], box[1])
    plain = _dense(torch.full(shape, SENT, dtype=dtype), padded)
    sp = kernels.new_err(1)
    kernels.step_medium(*d, plain, box, first=False, h2=H2, stat=sp, stat_i=ei, chunk=chunk, taper=tpd)
    u = _dense(torch.full(shape, SENT, dtype=dtype), padded)
    sm = kernels.new_err(1)
    if mode == "save":
        x = _dense(torch.full(shape, SENT, dtype=dtype), padded)
        kernels.step_medium(*d, u, box, first=False, h2=H2, stat=sm, stat_i=ei, chunk=chunk, taper=tpd, lap_out=x)
    else:
        x = _dense(acc0, padded)
        qd = _dense(q, padded)
        kernels.step_medium(*d, u, box, first=False, h2=H2, stat=sm, stat_i=ei, chunk=chunk, taper=tpd,
                            image=(qd, x))
    torch.cuda.synchronize()
    i0, i1, j0, j1, k0, k1 = box
    sl = (slice(i0, i1 + 1), slice(j0, j1 + 1), slice(k0, k1 + 1))
    if mode == "save":
        h = [_cast(v, dtype) for v in H2]
        exp = reference.laplace7(u1, *h)[i0 - 1:i1, j0 - 1:j1, k0 - 1:k1]
        outside = torch.full(shape, SENT, dtype=dtype)
    else:
        exp = acc0[sl] + u1[sl] * q[sl]
        outside = acc0.clone()
    # u and the statistic are those of the plain call, bit for bit
    assert torch.equal(u.cpu(), plain.cpu())
    assert kernels.decode_err(sm) == kernels.decode_err(sp)
    got = x.cpu()
    if dtype == torch.float64:
        assert torch.equal(got[sl], exp)
    assert_same_bits(got[sl], exp)
    mask = torch.ones(shape, dtype=torch.bool)
    mask[sl] = False
    assert torch.equal(got[mask], outside[mask])  # nothing outside the box is written
    if padded:  # nor the padding between the rows
        base = x._base
        inside = torch.zeros(base.shape, dtype=torch.bool, device=DEV)
        inside.as_strided(x.shape, x.stride(), x.storage_offset()).fill_(True)
        assert bool((base[~inside] == 0).all())


@pytest.mark.parametrize("mode", ["save", "image"])
@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("shape,box,chunk", CASES)
def test_step_medium_modes(C, shape, box, chunk, dtype, sponge, mode):
    _mode_case(shape, box, chunk, dtype, sponge, False, mode)


@pytest.mark.parametrize("mode", ["save", "image"])
@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_step_medium_modes_on_padded_views(C, dtype, sponge, mode):
    _mode_case(*CASES[2], dtype, sponge, True, mode)


def test_step_medium_modes_rejected_combinations(C):
    from wave3d.ops import kernels

    shape, box, _ = CASES[3]
    dt = torch.float64
    u1, u2, m = (t.to(DEV) for t in _inputs(shape, dt))
    u, x, q = (torch.zeros(shape, dtype=dt, device=DEV) for _ in range(3))
    kw = dict(h2=H2, stat=kernels.new_err(1), stat_i=(1, 4))
    with pytest.raises(ValueError, match="first"):
        kernels.step_medium(u1, u2, m, u, box, first=True, lap_out=x, **kw)
    with pytest.raises(ValueError, match="first"):
        kernels.step_medium(u1, u2, m, u, box, first=True, image=(q, x), **kw)
    with pytest.raises(ValueError, match="combined"):
        kernels.step_medium(u1, u2, m, u, box, first=False, lap_out=x, image=(q, x), **kw)
    for v in ("plain", "r2", "r2nt"):
        with pytest.raises(ValueError, match="variant"):
            kernels.step_medium(u1, u2, m, u, box, first=False, lap_out=x, variant=v, **kw)
        with pytest.raises(ValueError, match="variant"):
            kernels.step_medium(u1, u2, m, u, box, first=False, image=(q, x), variant=v, **kw)
    with pytest.raises(ValueError):  # image = (q, acc)
        kernels.step_medium(u1, u2, m, u, box, first=False, image=(q,), **kw)
    with pytest.raises(ValueError):  # another dtype
        kernels.step_medium(u1, u2, m, u, box, first=False, lap_out=x.float(), **kw)
    with pytest.raises(ValueError):  # another shape
        kernels.step_medium(u1, u2, m, u, box, first=False, image=(q, x[:-1]), **kw)
    with pytest.raises(ValueError):  # other strides
        kernels.step_medium(u1, u2, m, u, box, first=False, lap_out=kernels.alloc_level(*shape, dt), **kw)
    with pytest.raises(ValueError):  # not on the device
        kernels.step_medium(u1, u2, m, u, box, first=False, image=(q.cpu(), x), **kw)
    # the launcher refuses them as well (the native entry point, past the Python checks)
    gv = [*shape, shape[2], shape[1] * shape[2]]
    args = [u1.data_ptr(), u2.data_ptr(), m.data_ptr(), u.data_ptr(), gv, [list(box)], 1, 4, [], list(H2),
            kw["stat"].data_ptr(), 0, torch.cuda.current_stream().cuda_stream]
    X, Q = x.data_ptr(), q.data_ptr()
    for first, mode, variant, grids in ((True, "save", 1, dict(lap_out=X)),               # the Taylor start
                                        (False, "save", 0, dict(lap_out=X)),              # another variant
                                        (False, "image", 3, dict(q=Q, acc=X)),
                                        (False, "save", 1, dict(lap_out=X, q=Q, acc=X)),  # both modes' grids
                                        (False, "image", 1, dict(lap_out=X, q=Q, acc=X)),
                                        (False, "image", 1, dict(q=Q))):                  # q without acc
        with pytest.raises(C.Wave3dError):
            C.k_step_medium_f64(first, *args, C.medium_modes[mode], variant=variant, **grids)
    torch.cuda.synchronize()
    assert not bool(u.any()) and not bool(x.any())  # nothing was launched


# ---- end to end ------------------------------------------------------------------------------

def _problem(N, K, sponge, dtype="fp64", seed=3):
    """Heterogeneous speed2 <= 0.04 with T chosen for a Courant number near 0.28 (T = 1 at N = 70,
    K = 16); sources and receivers within 3 nodes of each other on both sides of the tile seams
    j = 16/17 and k = 64/65 (where N reaches them) and on the periodic plane; a duplicate receiver
    and a face receiver."""
    import wave3d

    g = torch.Generator().manual_seed(seed)
    T = (70 / 16) * K / N
    speed2 = 0.04 * (0.5 + 0.5 * torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64))
    speed2[N] = speed2[0]
    pert = speed2 * (1 + 0.1 * torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64))
    pert[N] = pert[0]
    prob = wave3d.MediumProblem(N, speed2, T=T, timesteps=K, dtype=dtype)
    ka, kb = (64, 65) if N > 66 else (N // 2, N // 2 + 1)
    sources = [(0, 16, ka), (N // 2, 17, kb), (3, 15, ka - 1)]
    receivers = [(N, 17, kb), (1, 16, ka + 1), (1, 16, ka + 1), (N // 2 + 1, 16, ka), (N // 2, 18, kb + 1),
                 (2, 0, ka), (2, 17, kb), (N - 1, 15, kb)]
    tau = T / K
    w = torch.stack([wave3d.ricker(3.0 / T, 0.3 * T, K, tau), -0.5 * wave3d.ricker(2.0 / T, 0.2 * T, K, tau),
                     0.7 * wave3d.ricker(4.0 / T, 0.25 * T, K, tau)], 1)
    taper = wave3d.sponge_taper(prob, 4) if sponge else None
    kw = dict(sources=sources, wavelet=w, receivers=receivers, taper=taper)
    observed = wave3d.MediumSolver(wave3d.MediumProblem(N, pert, T=T, timesteps=K, dtype=dtype), "cpu", **kw).run().traces
    return prob, kw, observed


def _assert_same(a, b):
    assert a.misfit == b.misfit
    assert torch.equal(a.traces, b.traces)
    assert torch.equal(a.grad_speed2, b.grad_speed2)
    assert torch.equal(a.grad_wavelet, b.grad_wavelet)


@pytest.fixture(scope="module")
def n20():
    """N = 20, K = 24 with sponge: the problem and the oracle's gradient, computed once."""
    import wave3d

    prob, kw, obs = _problem(20, 24, True)
    return prob, kw, obs, wave3d.MediumSolver(prob, "cpu", **kw).gradient(obs)


@pytest.mark.parametrize("N,K,sponge", [(20, 24, True), (20, 24, False), (70, 16, True)])
def test_gradient_matches_oracle_fp64(C, N, K, sponge):
    import wave3d

    prob, kw, obs = _problem(N, K, sponge)
    assert 0.2 < prob.courant < 0.35
    ref = wave3d.MediumSolver(prob, "cpu", **kw).gradient(obs)
    sol = wave3d.MediumSolver(prob, "hip", **kw)
    got = sol.gradient(obs)
    assert ref.misfit > 0 and float(ref.grad_speed2.abs().max()) > 0 and float(ref.grad_wavelet.abs().max()) > 0
    _assert_same(got, ref)
    assert torch.equal(got.traces, sol.run().traces)
    assert torch.equal(got.grad_speed2[N], got.grad_speed2[0])
    assert got.total_ms > 0 and got.extra["levels"] == wave3d.gradient_levels(K, got.extra["segment"])


def test_gradient_segment_invariance(C, n20):
    import wave3d

    prob, kw, obs, ref = n20
    K = prob.timesteps
    sol = wave3d.MediumSolver(prob, "hip", **kw)
    for seg in (K, 1, 5, 7):
        got = sol.gradient(obs, segment=seg)
        _assert_same(got, ref)
        last = (K - 1) % seg or min(seg, K - 1)
        assert got.extra["recomputed_steps"] == (0 if seg == K else (K - 1) - last)
        assert got.extra["segment"] == seg and got.extra["levels"] == wave3d.gradient_levels(K, seg)


def test_gradient_fp32(C, n20):
    import wave3d

    prob, kw, obs, ref = n20
    p32 = wave3d.MediumProblem(prob.N, prob.speed2, T=prob.T, timesteps=prob.timesteps, dtype="fp32")
    cpu = wave3d.MediumSolver(p32, "cpu", **kw).gradient(obs)
    hip = wave3d.MediumSolver(p32, "hip", **kw).gradient(obs)
    assert hip.grad_speed2.dtype == torch.float32 and hip.grad_wavelet.dtype == torch.float32

    def rel(a, b):
        return float((a.double() - b).abs().max() / b.abs().max())

    for name in ("grad_speed2", "grad_wavelet"):
        e_cpu, e_hip = rel(getattr(cpu, name), getattr(ref, name)), rel(getattr(hip, name), getattr(ref, name))
        print(f"fp32 {name}: oracle error {e_cpu:.3e}, hip error {e_hip:.3e}")
        assert e_cpu > 0
        assert e_hip <= 4 * e_cpu


def test_gradient_zero_residual(C, n20):
    import wave3d

    prob, kw, _, _ = n20
    sol = wave3d.MediumSolver(prob, "hip", **kw)
    got = sol.gradient(sol.run().traces, segment=6)
    assert got.misfit == 0
    assert not bool(got.grad_speed2.any()) and not bool(got.grad_wavelet.any())


def test_gradient_nonfinite_names_the_pass(C):
    import wave3d

    N, K = 16, 60
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        prob = wave3d.MediumProblem(N, 1e8, timesteps=K, strict_cfl=False)  # Courant number 849
    assert not prob.stable()
    sol = wave3d.MediumSolver(prob, "hip", sources=[(8, 8, 8)], wavelet=torch.ones(K, 1), receivers=[(5, 5, 5)])
    with pytest.raises(RuntimeError, match=r"forward pass at layer \d+"):
        sol.gradient(torch.zeros(K + 1, 1), segment=20)
