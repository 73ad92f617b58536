"""Variable density on the GPU: k_march_mb (csrc/hip_medium.hip) against the PyTorch oracle
(ops/reference.py laplace_density, step_medium / solve_medium / gradient_medium with a buoyancy or a
density).

A single step must be bitwise equal in fp64 and in fp32: both sides round every operation in the same
order (the inputs keep every numerator inside the constant division's range). fp32 solves stay inside the
bound of test_gpu_medium_order.py, measured on the oracle and never on the kernel:
|got - exp32| <= 4 max |exp32 - exp64|. Inputs: u1, u2 in [0, 1], m in [1e-4, 6e-4], b in [0.3, 2].
"""
import math

import pytest
import torch

from test_gpu_medium import CASES, H2, _cast, _inputs, _rand
from test_gpu_medium_order import _at, _box_mask, _check
from test_gpu_sponge import _tapers

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = (torch.float64, torch.float32)


def _buoyancy(shape, dtype):
    return _rand(shape, dtype, 4, 0.3, 2.0)


def _oracle(u1, u2, m, b, box, first, taper, dtype=None):
    """reference.step_medium with a buoyancy in ``dtype`` (default: that of the inputs) on the same values."""
    from wave3d.ops import reference

    h2 = [_cast(v, u1.dtype) for v in H2]  # the kernel casts h2 to the working type
    if dtype is not None:
        u1, u2, m, b = (t.to(dtype) for t in (u1, u2, m, b))
        taper = None if taper is None else tuple(t.to(dtype) for t in taper)
    return reference.step_medium(u1, u2, m, box, first=first, hx2=h2[0], hy2=h2[1], hz2=h2[2], taper=taper,
                                 buoyancy=b)


@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_step_matches_reference(C, case, dtype, first, sponge):
    from wave3d.ops import kernels, reference

    shape, box, chunk = CASES[case]
    u1, u2, m = _inputs(shape, dtype)
    b = _buoyancy(shape, dtype)
    taper = _tapers(shape, dtype) if sponge else None
    u = torch.full(shape, -7.0, dtype=dtype, device=DEV)
    stat = kernels.new_err(1)
    ei = (box[0] + 1, box[1])  # exclude the first box plane from the statistic
    kernels.step_medium(u1.to(DEV), u2.to(DEV), m.to(DEV), u, box, first=first, h2=H2, stat=stat, stat_i=ei,
                        chunk=chunk, taper=None if taper is None else tuple(t.to(DEV) for t in taper),
                        buoyancy=b.to(DEV))
    torch.cuda.synchronize()
    exp = _oracle(u1, u2, m, b, box, first, taper)
    exp64 = _oracle(u1, u2, m, b, box, first, taper, torch.float64)
    # the density matters: the constant-density values differ
    h2 = [_cast(v, dtype) for v in H2]
    assert not torch.equal(exp, reference.step_medium(u1, u2, m, box, first=first, hx2=h2[0], hy2=h2[1], hz2=h2[2],
                                                      taper=taper))
    uc = u.cpu()
    _check(_at(uc, box), exp, exp64)
    assert bool((uc[_box_mask(shape, box)] == -7.0).all())  # every node outside the box keeps its sentinel
    want = reference.max_abs_field(exp[ei[0] - box[0]:].double())
    (ga, gr, bad), = kernels.decode_err(stat)
    assert ga == want
    assert gr == -100.0 and not bad


@pytest.mark.parametrize("dtype", DTYPES)
def test_flags_nonfinite(C, dtype):
    from wave3d.ops import kernels, reference

    shape, box, _ = CASES[0]
    u1, u2, m = _inputs(shape, dtype)
    b = _buoyancy(shape, dtype)
    u1[5, 7, 33] = math.nan
    u = torch.zeros(shape, dtype=dtype, device=DEV)
    stat = kernels.new_err(1)
    kernels.step_medium(u1.to(DEV), u2.to(DEV), m.to(DEV), u, box, first=False, h2=H2, stat=stat,
                        stat_i=(box[0], box[1]), buoyancy=b.to(DEV))
    torch.cuda.synchronize()
    (ga, _, bad), = kernels.decode_err(stat)
    assert bad
    exp = _oracle(u1, u2, m, b, box, False, None)
    want = reference.max_abs_field(exp.double())  # the maximum ignores the NaN nodes
    assert int(torch.isnan(exp).sum()) == 7 and math.isfinite(ga)
    assert ga == want


@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_padded_views(C, dtype, first):
    """alloc_level views, b included, give the dense tensors' bits."""
    from wave3d.ops import kernels

    shape, box, chunk = CASES[2]
    cpu = [*_inputs(shape, dtype), _buoyancy(shape, dtype)]
    d = [t.to(DEV) for t in cpu]
    ud = torch.full(shape, -7.0, dtype=dtype, device=DEV)
    sd = kernels.new_err(1)
    kw = dict(first=first, h2=H2, stat_i=(1, 7), chunk=chunk)
    kernels.step_medium(d[0], d[1], d[2], ud, box, stat=sd, buoyancy=d[3], **kw)
    views = [kernels.alloc_level(*shape, dtype) for _ in range(5)]
    assert views[0].stride(1) > shape[2]  # padded pitch
    for v, t in zip(views, cpu):
        v.copy_(t)
    views[4].fill_(-7.0)
    sv = kernels.new_err(1)
    kernels.step_medium(views[0], views[1], views[2], views[4], box, stat=sv, buoyancy=views[3], **kw)
    torch.cuda.synchronize()
    assert torch.equal(views[4].cpu(), ud.cpu()) and kernels.decode_err(sv) == kernels.decode_err(sd)
    assert torch.equal(views[3].cpu(), cpu[3])  # b is never written
    for v in views:  # the padding between rows and in front of the view is still zero
        base = v._base
        inside = torch.zeros(base.shape, dtype=torch.bool, device=DEV)
        inside.as_strided(v.shape, v.stride(), v.storage_offset()).fill_(True)
        assert int(inside.sum()) == v.numel() and bool((base[~inside] == 0).all())


@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_save_and_image_modes(C, dtype, sponge):
    from wave3d.ops import kernels, reference

    shape, box, chunk = CASES[1]
    u1, u2, m = _inputs(shape, dtype)
    b = _buoyancy(shape, dtype)
    taper = _tapers(shape, dtype) if sponge else None
    g = torch.Generator().manual_seed(9)
    q = (torch.rand(shape, generator=g, dtype=torch.float64) - 0.5).to(dtype)
    acc0 = (torch.rand(shape, generator=g, dtype=torch.float64) - 0.5).to(dtype)
    dev = [t.to(DEV) for t in (u1, u2, m)]
    kw = dict(first=False, h2=H2, stat_i=(box[0], box[1]), chunk=chunk, buoyancy=b.to(DEV),
              taper=None if taper is None else tuple(t.to(DEV) for t in taper))

    def run(**mode):
        u = torch.full(shape, -7.0, dtype=dtype, device=DEV)
        st = kernels.new_err(1)
        kernels.step_medium(*dev, u, box, stat=st, **kw, **mode)
        return u, kernels.decode_err(st)

    plain, pstat = run()
    lap = torch.full(shape, -7.0, dtype=dtype, device=DEV)
    saved, sstat = run(lap_out=lap)
    acc = acc0.to(DEV)
    imaged, istat = run(image=(q.to(DEV), acc))
    torch.cuda.synchronize()
    _check(_at(plain.cpu(), box), _oracle(u1, u2, m, b, box, False, taper),
           _oracle(u1, u2, m, b, box, False, taper, torch.float64))
    # u and stat are the plain density step's bits; nothing outside the box is written
    assert torch.equal(saved, plain) and torch.equal(imaged, plain) and sstat == pstat and istat == pstat
    assert bool((plain.cpu()[_box_mask(shape, box)] == -7.0).all())
    h2 = [_cast(v, dtype) for v in H2]
    i0, i1, j0, j1, k0, k1 = box
    want = reference.laplace_density(u1, b, *h2)[i0 - 1:i1, j0 - 1:j1, k0 - 1:k1]
    want64 = reference.laplace_density(u1.double(), b.double(), *h2)[i0 - 1:i1, j0 - 1:j1, k0 - 1:k1]
    lc = lap.cpu()
    _check(_at(lc, box), want, want64)
    assert bool((lc[_box_mask(shape, box)] == -7.0).all())
    # acc = acc + u1 q, the product rounded first: elementwise, the same bits in either dtype
    exp_acc = acc0.clone()
    _at(exp_acc, box).copy_(_at(acc0, box) + _at(u1, box) * _at(q, box))
    assert torch.equal(acc.cpu(), exp_acc)


def test_rejected_calls(C):
    """Every one a ValueError before any launch: the output keeps its sentinel."""
    from wave3d.ops import kernels

    shape, box, _ = CASES[0]
    dt = torch.float64
    u1, u2, m = (t.to(DEV) for t in _inputs(shape, dt))
    b = _buoyancy(shape, dt).to(DEV)
    u = torch.full(shape, -7.0, dtype=dt, device=DEV)
    kw = dict(first=False, h2=H2, stat=kernels.new_err(1), stat_i=(1, 11))
    with pytest.raises(ValueError, match="order 2"):
        kernels.step_medium(u1, u2, m, u, (4, 8, 4, 16, 4, 60), order=4, buoyancy=b, **kw)
    with pytest.raises(ValueError, match="default variant"):
        kernels.step_medium(u1, u2, m, u, box, variant="r2", buoyancy=b, **kw)
    with pytest.raises(ValueError, match="dtypes"):
        kernels.step_medium(u1, u2, m, u, box, buoyancy=b.float(), **kw)
    with pytest.raises(ValueError, match="strides"):
        padded = kernels.alloc_level(*shape, dt)
        padded.copy_(b)
        kernels.step_medium(u1, u2, m, u, box, buoyancy=padded, **kw)
    with pytest.raises(ValueError):
        kernels.step_medium(u1, u2, m, u, box, buoyancy=b[:, :, :-1], **kw)
    torch.cuda.synchronize()
    assert bool((u == -7.0).all())


# ---- the front-end: MediumSolver with a density model, "hip" against "cpu" --------------------

def _layered(N, seed):
    """Layered rho and c^2 with a little noise, periodic in x."""
    g = torch.Generator().manual_seed(seed)
    rho = torch.ones((N + 1,) * 3, dtype=torch.float64)
    rho[:, :, N // 2:] = 2.5
    rho[:, N // 3:, :] *= 1.3
    rho = rho * (1 + 0.1 * torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64))
    speed2 = torch.full((N + 1,) * 3, 0.3, dtype=torch.float64)
    speed2[:, :, 2 * N // 3:] = 0.6
    speed2 = speed2 * (1 + 0.1 * torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64))
    rho[N], speed2[N] = rho[0], speed2[0]
    return rho, speed2


def _solver(backend, N, K, sponge, receivers):
    import wave3d

    rho, speed2 = _layered(N, 31)
    prob = wave3d.MediumProblem(N, speed2, timesteps=K, density=rho)
    w = torch.stack([wave3d.ricker(3.0, 0.3, K, prob.tau), -0.5 * wave3d.ricker(2.0, 0.2, K, prob.tau)], 1)
    return wave3d.MediumSolver(prob, backend, sources=[(0, 4, 6), (6, 3, 5)], wavelet=w, receivers=receivers,
                               taper=wave3d.sponge_taper(prob, 3) if sponge else None)


@pytest.mark.parametrize("sponge", [True, False])
def test_run_matches_oracle(C, sponge):
    N, K = 12, 12
    rec = [(N, 7, 3), (4, 5, 5), (6, 3, 5), (3, 0, 4)]
    want = _solver("cpu", N, K, sponge, rec).run()
    got = _solver("hip", N, K, sponge, rec).run()
    assert float(want.traces.abs().max()) > 1e-3 and got.extra["density"] is True and not got.aborted
    assert torch.equal(got.traces, want.traces) and torch.equal(got.u_final, want.u_final)
    assert got.max_abs_u == want.max_abs_u and got.courant == want.courant


def test_power_of_two_density_scales_the_field_exactly(C):
    from test_medium_density_cpu import _scaling_solver

    one, two = _scaling_solver("hip", 1.0).run(), _scaling_solver("hip", 2.0).run()
    assert float(one.traces.abs().max()) > 1e-3
    assert torch.equal(two.traces, 2 * one.traces) and torch.equal(two.u_final, 2 * one.u_final)
    assert torch.equal(one.traces, _scaling_solver("cpu", 1.0).run().traces)


@pytest.fixture(scope="module")
def gradient_case():
    import wave3d
    from wave3d.ops import reference

    N, K = 10, 9
    rec = [(N, 7, 3), (4, 5, 5), (6, 3, 5)]
    cpu = _solver("cpu", N, K, True, rec)
    p = cpu.problem
    observed = reference.solve_medium(N, K, p.speed2 * 1.1, sources=cpu.sources, wavelet=cpu.wavelet, receivers=rec,
                                      taper=cpu.taper, density=p.density)[0]
    assert isinstance(cpu.gradient(observed), wave3d.MediumGradient)
    return N, K, rec, observed, cpu.gradient(observed)


@pytest.mark.parametrize("segment", [1, 3, 8, None])  # 8 = K - 1
def test_gradient_matches_oracle(C, gradient_case, segment):
    import wave3d

    N, K, rec, observed, want = gradient_case
    got = _solver("hip", N, K, True, rec).gradient(observed, segment=segment)
    assert want.misfit > 0 and float(want.grad_speed2.abs().max()) > 0 and float(want.grad_wavelet.abs().max()) > 0
    assert got.misfit == want.misfit and torch.equal(got.traces, want.traces)
    assert torch.equal(got.grad_speed2, want.grad_speed2) and torch.equal(got.grad_wavelet, want.grad_wavelet)
    seg = got.extra["segment"]
    assert seg == (segment if segment is not None else wave3d.models.medium.best_gradient_segment(K))
    assert got.extra["levels"] == wave3d.gradient_levels(K, seg, density=True) == wave3d.gradient_levels(K, seg) + 1
    assert got.extra["density"] is True
