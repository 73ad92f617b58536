"""Born (linearised) modelling on the GPU: the Born mode of k_march_m, k_march_mh and k_march_mb
(csrc/hip_medium.hip) against ops/reference.py step_medium(born=...), and MediumSolver.born /
gauss_newton ("hip": the background step in save mode, the perturbation step in Born mode, in lock
step) against the "cpu" backend (ops/reference.py born_medium).

fp64 results must be *bitwise* equal: both sides round every operation in the same order and share
the host-side arithmetic; a single fp32 step is bitwise equal too, fp32 solves within the bounds the existing
tests use.
"""
import math
import warnings

import pytest
import torch

from bits import assert_same_bits
from test_gpu_medium import CASES, H2, _cast, _inputs, _rand
from test_gpu_medium_density import _buoyancy
from test_gpu_medium_gradient import _dense, _problem
from test_gpu_medium_order import CASES as ORDER_CASES
from test_gpu_sponge import _tapers

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -7.0
DTYPES = (torch.float64, torch.float32)
# the adjoint dot test's |lhs - rhs| / |lhs| of the N = 20 case, measured on the "cpu" backend (whose fp64
# results are those of "hip" bit for bit); on the GPU: the same 1.301e-15
DOT_MEASURED = 1.301e-15
# (name, storage shape, box, chunk, step keywords): order 2, orders 4 and 8 with their mirrors, order 2 with a density
STEP_CASES = ([(f"o2-{i}", s, b, c, {}) for i, (s, b, c) in enumerate(CASES)]
              + [(f"o{o}-{i}", s, b, c, dict(order=o, mirror=mir)) for o in (4, 8)
                 for i, (s, b, c, mir) in enumerate(ORDER_CASES)]
              + [(f"rho-{i}", s, b, c, dict(density=True)) for i, (s, b, c) in enumerate(CASES)])


def _at(t, box):
    i0, i1, j0, j1, k0, k1 = box
    return t[i0:i1 + 1, j0:j1 + 1, k0:k1 + 1]


def _step_inputs(shape, dtype, kw, sponge):
    """CPU tensors: (u1, u2, m, q, dm, taper or None, buoyancy or None) and the keywords without `density`."""
    u1, u2, m = _inputs(shape, dtype)
    q = _rand(shape, dtype, 6, -1.0, 1.0)
    dm = _rand(shape, dtype, 7, -1.0, 1.0)
    tp = _tapers(shape, dtype) if sponge else None
    kw = dict(kw)
    b = _buoyancy(shape, dtype) if kw.pop("density", False) else None
    return (u1, u2, m, q, dm, tp, b), kw


def _oracle(cpu, box, kw, born=True):
    from wave3d.ops import reference

    u1, u2, m, q, dm, tp, b = cpu
    h = [_cast(v, u1.dtype) for v in H2]  # the kernel casts h2 to the working type
    return reference.step_medium(u1, u2, m, box, first=False, hx2=h[0], hy2=h[1], hz2=h[2], taper=tp, buoyancy=b,
                                 born=(_at(q, box).clone(), dm) if born else None, **kw)


def _run(cpu, box, chunk, kw, padded=False, born=True, dm=None):
    """The device step on copies of the CPU inputs: (u, stat, q, dm on the device)."""
    from wave3d.ops import kernels

    u1, u2, m, q, dm0, tp, b = cpu
    d = [_dense(t, padded) for t in (u1, u2, m)]
    qd, dmd = _dense(q, padded), _dense(dm0 if dm is None else dm, padded)
    u = _dense(torch.full(u1.shape, SENT, dtype=u1.dtype), padded)
    stat = kernels.new_err(1)
    kernels.step_medium(*d, u, box, first=False, h2=H2, stat=stat, stat_i=(box[0] + 1, box[1]), chunk=chunk,
                        taper=None if tp is None else tuple(t.to(DEV) for t in tp),
                        buoyancy=None if b is None else _dense(b, padded), born=(qd, dmd) if born else None, **kw)
    torch.cuda.synchronize()
    return u, stat, qd, dmd


@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,shape,box,chunk,kw", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_born_step_matches_reference(C, name, shape, box, chunk, kw, dtype, sponge):
    from wave3d.ops import kernels, reference

    cpu, kw = _step_inputs(shape, dtype, kw, sponge)
    u, stat, qd, dmd = _run(cpu, box, chunk, kw)
    exp = _oracle(cpu, box, kw)
    assert not torch.equal(exp, _oracle(cpu, box, kw, born=False))  # the scattering term matters
    uc = u.cpu()
    if dtype == torch.float64:
        assert torch.equal(_at(uc, box), exp)
    assert_same_bits(_at(uc, box), exp)
    mask = torch.ones(shape, dtype=torch.bool)
    _at(mask, box)[...] = False
    assert bool((uc[mask] == SENT).all())  # nothing outside the box is written
    # slot 0: max |u| of the Born-updated values over the planes after the first; flag clear
    want = reference.max_abs_field(exp[1:].double())
    (ga, gr, bad), = kernels.decode_err(stat)
    assert ga == want
    assert gr == -100.0 and not bad
    # q and dm are read only
    assert torch.equal(qd.cpu(), cpu[3]) and torch.equal(dmd.cpu(), cpu[4])


@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("name,shape,box,chunk,kw", [STEP_CASES[2], STEP_CASES[5], STEP_CASES[9], STEP_CASES[14]],
                         ids=["o2", "o4", "o8", "rho"])
def test_born_step_with_zero_dm_is_the_plain_step(C, name, shape, box, chunk, kw, sponge):
    from wave3d.ops import kernels

    cpu, kw = _step_inputs(shape, torch.float64, kw, sponge)
    u, stat, _, _ = _run(cpu, box, chunk, kw, dm=torch.zeros(shape, dtype=torch.float64))
    plain, pstat, _, _ = _run(cpu, box, chunk, kw, born=False)
    assert torch.equal(u, plain)  # x + 0 q with finite q
    assert kernels.decode_err(stat) == kernels.decode_err(pstat)


@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_born_step_on_padded_views(C, dtype, sponge):
    """alloc_level views give the dense tensors' bits, and the padding between the rows stays zero."""
    from wave3d.ops import kernels

    _, shape, box, chunk, kw = STEP_CASES[2]
    cpu, kw = _step_inputs(shape, dtype, kw, sponge)
    u, stat, qd, dmd = _run(cpu, box, chunk, kw, padded=True)
    dense, dstat, _, _ = _run(cpu, box, chunk, kw)
    assert torch.equal(u.cpu(), dense.cpu())
    assert kernels.decode_err(stat) == kernels.decode_err(dstat)
    if dtype == torch.float64:
        assert torch.equal(_at(u.cpu(), box), _oracle(cpu, box, kw))
    for v in (u, qd, dmd):
        base = v._base
        inside = torch.zeros(base.shape, dtype=torch.bool, device=DEV)
        inside.as_strided(v.shape, v.stride(), v.storage_offset()).fill_(True)
        assert bool((base[~inside] == 0).all())
    assert torch.equal(qd.cpu(), cpu[3]) and torch.equal(dmd.cpu(), cpu[4])


def test_born_step_fused_wrap_and_nonfinite_flag(C):
    """The periodic wrap carries the Born-updated planes, and a NaN in dm sets the flag (a value check)."""
    from wave3d.ops import kernels

    _, shape, box, chunk, kw = STEP_CASES[0]
    dt = torch.float64
    cpu, kw = _step_inputs(shape, dt, kw, True)
    u1, u2, m, q, dm, tp, _ = cpu
    nx = shape[0]
    wrap = (nx - 2, 0, 1, nx - 1)
    u = torch.full(shape, SENT, dtype=dt, device=DEV)
    stat = kernels.new_err(1)
    args = [t.to(DEV) for t in (u1, u2, m)]
    tpd = tuple(t.to(DEV) for t in tp)
    kernels.step_medium(*args, u, box, first=False, h2=H2, stat=stat, stat_i=(1, nx - 2), wrap=wrap, taper=tpd,
                        born=(q.to(DEV), dm.to(DEV)))
    torch.cuda.synchronize()
    exp = _oracle(cpu, box, kw)
    sl = (slice(box[2], box[3] + 1), slice(box[4], box[5] + 1))
    uc = u.cpu()
    assert torch.equal(_at(uc, box), exp)
    assert torch.equal(uc[0][sl], exp[-1]) and torch.equal(uc[nx - 1][sl], exp[0])
    assert not kernels.decode_err(stat)[0][2]
    bad = dm.clone()
    bad[5, 7, 33] = math.nan
    kernels.step_medium(*args, u, box, first=False, h2=H2, stat=stat, stat_i=(1, nx - 2), wrap=wrap, taper=tpd,
                        born=(q.to(DEV), bad.to(DEV)))
    torch.cuda.synchronize()
    assert kernels.decode_err(stat)[0][2]
    assert bool(torch.isnan(u[5, 7, 33])) and int(torch.isnan(u).sum()) == 1


def test_born_step_rejected_calls(C):
    """Every refusal is a ValueError from ops.kernels before any launch; the native entry point refuses
    the same calls on its own (past the Python checks). The output keeps its sentinel."""
    from wave3d.ops import kernels

    shape, box, _ = CASES[3]
    dt = torch.float64
    u1, u2, m = (t.to(DEV) for t in _inputs(shape, dt))
    u = torch.full(shape, SENT, dtype=dt, device=DEV)
    x, q, dm = (torch.zeros(shape, dtype=dt, device=DEV) for _ in range(3))
    kw = dict(h2=H2, stat=kernels.new_err(1), stat_i=(1, 4))
    with pytest.raises(ValueError, match="first"):
        kernels.step_medium(u1, u2, m, u, box, first=True, born=(q, dm), **kw)
    for v in ("plain", "r2", "r2nt"):
        with pytest.raises(ValueError, match="variant"):
            kernels.step_medium(u1, u2, m, u, box, first=False, born=(q, dm), variant=v, **kw)
    with pytest.raises(ValueError, match="combined"):
        kernels.step_medium(u1, u2, m, u, box, first=False, born=(q, dm), lap_out=x, **kw)
    with pytest.raises(ValueError, match="combined"):
        kernels.step_medium(u1, u2, m, u, box, first=False, born=(q, dm), image=(q, x), **kw)
    with pytest.raises(ValueError):  # born = (q, dm): dm without q, q without dm
        kernels.step_medium(u1, u2, m, u, box, first=False, born=(dm,), **kw)
    with pytest.raises(ValueError):
        kernels.step_medium(u1, u2, m, u, box, first=False, born=(None, dm), **kw)
    with pytest.raises(ValueError):
        kernels.step_medium(u1, u2, m, u, box, first=False, born=(q, None), **kw)
    with pytest.raises(ValueError, match="shares memory"):
        kernels.step_medium(u1, u2, m, u, box, first=False, born=(u, dm), **kw)
    with pytest.raises(ValueError, match="shares memory"):
        kernels.step_medium(u1, u2, m, u, box, first=False, born=(q, u), **kw)
    with pytest.raises(ValueError):  # another dtype
        kernels.step_medium(u1, u2, m, u, box, first=False, born=(q, dm.float()), **kw)
    with pytest.raises(ValueError):  # another shape
        kernels.step_medium(u1, u2, m, u, box, first=False, born=(q[:-1], dm), **kw)
    with pytest.raises(ValueError):  # other strides
        kernels.step_medium(u1, u2, m, u, box, first=False, born=(kernels.alloc_level(*shape, dt), dm), **kw)
    with pytest.raises(ValueError):  # not on the device
        kernels.step_medium(u1, u2, m, u, box, first=False, born=(q, dm.cpu()), **kw)
    # the launcher refuses them as well
    gv = [*shape, shape[2], shape[1] * shape[2]]
    args = [u1.data_ptr(), u2.data_ptr(), m.data_ptr(), u.data_ptr(), gv, [list(box)], 1, 4, [], list(H2),
            kw["stat"].data_ptr(), 0, torch.cuda.current_stream().cuda_stream]
    Q, D, X, U = q.data_ptr(), dm.data_ptr(), x.data_ptr(), u.data_ptr()
    born, image = C.medium_modes["born"], C.medium_modes["image"]
    for first, mode, variant, grids in ((False, born, 1, dict(dm=D)),                  # dm without q
                                        (True, born, 1, dict(q=Q, dm=D)),              # the Taylor start
                                        (False, born, 0, dict(q=Q, dm=D)),             # another variant
                                        (False, born, 3, dict(q=Q, dm=D)),
                                        (False, born, 1, dict(q=Q, dm=D, lap_out=X)),  # with save
                                        (False, born, 1, dict(q=Q, dm=D, acc=X)),      # with image
                                        (False, born, 1, dict(q=U, dm=D)),             # q is u
                                        (False, born, 1, dict(q=Q, dm=U)),             # dm is u
                                        (False, born, 1, dict(q=Q)),                   # q alone: an incomplete Born mode
                                        (False, image, 1, dict(q=Q))):                 # and an incomplete image mode
        with pytest.raises(C.Wave3dError):
            C.k_step_medium_f64(first, *args, mode, variant=variant, **grids)
    torch.cuda.synchronize()
    assert bool((u == SENT).all()) and not bool(x.any())  # nothing was launched
    # the plain step of the same arguments runs
    C.k_step_medium_f64(False, *args, C.medium_modes["plain"], variant=1)
    torch.cuda.synchronize()
    assert not bool((_at(u, box) == SENT).any())


# ---- the front-end: MediumSolver.born and gauss_newton, "hip" against "cpu" -------------------

def _perturbations(prob, kw, seed=9):
    """(dspeed2 periodic in x, dwavelet, r) for a problem: random, of both signs."""
    N, K = prob.N, prob.timesteps
    g = torch.Generator().manual_seed(seed)
    ds = 0.02 * (torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64) - 0.5)
    ds[N] = ds[0]
    dw = torch.rand(K, len(kw["sources"]), generator=g, dtype=torch.float64) - 0.5
    r = torch.rand(K + 1, len(kw["receivers"]), generator=g, dtype=torch.float64) - 0.5
    return ds, dw, r


def _front_end_case(N, K, sponge, order=2, density=False, dtype="fp64"):
    """`_problem`'s case (sources and receivers on both sides of the tile seams j = 16/17 and k = 64/65
    where N reaches them, and on the periodic plane) at a space order or with a random density in [1, 2]."""
    import wave3d

    base, kw, _ = _problem(N, K, sponge)
    rho = None
    if density:
        g = torch.Generator().manual_seed(17)
        rho = 1 + torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64)
        rho[N] = rho[0]
    prob = wave3d.MediumProblem(N, base.speed2, T=base.T, timesteps=K, dtype=dtype, space_order=order, density=rho)
    return prob, kw


FRONT_END = [(20, 24, True, 2, False), (20, 24, False, 2, False), (70, 16, True, 2, False), (20, 24, True, 4, False),
             (20, 24, False, 8, False), (20, 24, True, 2, True)]


@pytest.mark.parametrize("N,K,sponge,order,density", FRONT_END)
def test_born_matches_oracle_fp64(C, N, K, sponge, order, density):
    import wave3d

    prob, kw = _front_end_case(N, K, sponge, order, density)
    assert prob.stable()
    ds, dw, _ = _perturbations(prob, kw)
    want = wave3d.MediumSolver(prob, "cpu", **kw).born(ds, dw)
    sol = wave3d.MediumSolver(prob, "hip", **kw)
    got = sol.born(ds, dw)
    assert float(want.dtraces.abs().max()) > 0 and not bool(want.dtraces[0].any())
    assert torch.equal(got.traces, want.traces)
    assert torch.equal(got.dtraces, want.dtraces)
    assert torch.equal(got.du_final, want.du_final)
    assert got.max_abs_du == want.max_abs_du
    assert torch.equal(got.traces, sol.run().traces)
    assert got.total_ms > 0 and got.extra["levels"] == wave3d.born_levels(density=density) == 9 + density
    assert isinstance(got, wave3d.MediumBorn)


@pytest.fixture(scope="module")
def n20():
    """N = 20, K = 24 with sponge: the problem, its perturbations and the oracle's Born run, computed once."""
    import wave3d

    prob, kw = _front_end_case(20, 24, True)
    ds, dw, r = _perturbations(prob, kw)
    return prob, kw, ds, dw, r, wave3d.MediumSolver(prob, "cpu", **kw).born(ds, dw)


def test_born_one_perturbation_at_a_time(C, n20):
    import wave3d

    prob, kw, ds, dw, _, _ = n20
    for a, b in ((ds, None), (None, dw), (0.01, None)):
        want = wave3d.MediumSolver(prob, "cpu", **kw).born(a, b)
        got = wave3d.MediumSolver(prob, "hip", **kw).born(a, b)
        assert float(want.dtraces.abs().max()) > 0
        assert torch.equal(got.dtraces, want.dtraces) and torch.equal(got.du_final, want.du_final)


def test_born_fp32(C, n20):
    import wave3d

    prob, kw, ds, dw, _, ref = n20
    p32 = wave3d.MediumProblem(prob.N, prob.speed2, T=prob.T, timesteps=prob.timesteps, dtype="fp32")
    cpu = wave3d.MediumSolver(p32, "cpu", **kw).born(ds, dw)
    hip = wave3d.MediumSolver(p32, "hip", **kw).born(ds, dw)
    assert hip.dtraces.dtype == torch.float32 and hip.du_final.dtype == torch.float32

    def rel(a, b):
        return float((a.double() - b).abs().max() / b.abs().max())

    # both sides accumulate fp32 rounding over the same K steps in different orders: the bound is the
    # fp32 oracle's own error against the fp64 oracle, times 4 (measured: that error is 2.40e-7 on dtraces,
    # 2.14e-7 on du_final and 4.94e-7 on traces, and the hip backend's errors equal it to the digits printed)
    for name in ("dtraces", "du_final", "traces"):
        e_cpu, e_hip = rel(getattr(cpu, name), getattr(ref, name)), rel(getattr(hip, name), getattr(ref, name))
        print(f"fp32 {name}: oracle error {e_cpu:.3e}, hip error {e_hip:.3e}")
        assert e_cpu > 0
        assert e_hip <= 4 * e_cpu


def test_gauss_newton_matches_oracle(C, n20):
    import wave3d

    prob, kw, ds, dw, _, ref = n20
    want = wave3d.MediumSolver(prob, "cpu", **kw).gauss_newton(ds, dw)
    assert want.misfit > 0 and float(want.grad_speed2.abs().max()) > 0 and float(want.grad_wavelet.abs().max()) > 0
    assert torch.equal(want.extra["dtraces"], ref.dtraces)
    sol = wave3d.MediumSolver(prob, "hip", **kw)
    for seg in (5, None):  # the result does not depend on the checkpoint schedule
        got = sol.gauss_newton(ds, dw, segment=seg)
        assert got.misfit == want.misfit
        assert torch.equal(got.grad_speed2, want.grad_speed2)
        assert torch.equal(got.grad_wavelet, want.grad_wavelet)
        assert torch.equal(got.traces, want.traces) and torch.equal(got.extra["dtraces"], ref.dtraces)


def test_adjoint_dot_test_on_the_gpu(C, n20):
    """<J d, r> from born() against <d, J^T r> from gradient(traces - r), both on the GPU."""
    import wave3d

    prob, kw, ds, dw, r, _ = n20
    N = prob.N
    sol = wave3d.MediumSolver(prob, "hip", **kw)
    b = sol.born(ds, dw)
    g = sol.gradient(b.traces - r)
    lhs = float((b.dtraces[1:] * r[1:]).sum())
    rhs = float((g.grad_speed2[:N] * ds[:N]).sum() + (g.grad_wavelet * dw).sum())
    e = abs(lhs - rhs) / abs(lhs)
    print(f"<J d, r> = {lhs!r}, <d, J^T r> = {rhs!r}, relative difference {e:.3e}")
    assert abs(lhs) > 1e-3 * float(b.dtraces[1:].norm() * r[1:].norm())
    # the CPU test's bound: 100 times the difference measured for this case (on the "cpu" backend, whose
    # fp64 results are those of "hip" bit for bit: DOT_MEASURED), capped at 1e-9
    assert e <= min(100 * max(DOT_MEASURED, 2.0 ** -52), 1e-9)



def test_born_nonfinite_names_the_field(C, n20):
    """Non-finite values must not crash: a NaN in dspeed2 is refused by the argument check before any
    launch, and a finite perturbation whose source term overflows raises the non-finite error of the
    one flag read-back, naming the perturbation field; a diverging background run names the background."""
    import wave3d

    prob, kw, ds, _, _, _ = n20
    N = prob.N
    sol = wave3d.MediumSolver(prob, "hip", **kw)
    bad = ds.clone()
    bad[3, 4, 5] = math.nan
    with pytest.raises(ValueError, match="dspeed2 must be finite"):
        sol.born(bad)
    huge = ds.clone()
    i, j, k = kw["sources"][0]  # on the periodic plane
    assert i == 0
    huge[0, j, k] = huge[N, j, k] = 1e308  # dm g overflows at the source node
    with pytest.raises(RuntimeError, match=r"non-finite values in the perturbation field at layer \d+"):
        sol.born(huge)
    K = 60
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        wild = wave3d.MediumProblem(16, 1e8, timesteps=K, strict_cfl=False)  # Courant number 849
    sol = wave3d.MediumSolver(wild, "hip", sources=[(8, 8, 8)], wavelet=torch.ones(K, 1), receivers=[(5, 5, 5)])
    with pytest.raises(RuntimeError, match=r"non-finite values in the background field at layer \d+"):
        sol.born(1.0)
