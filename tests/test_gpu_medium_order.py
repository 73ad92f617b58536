"""Space orders 4 and 8 on the GPU: k_march_mh (csrc/hip_medium.hip) against the PyTorch oracle
(ops/reference.py laplace_star / step_medium / solve_medium / gradient_medium with ``order``).

A single step must be bitwise equal in fp64 and in fp32: both sides round every operation in the same
order, and the inputs keep every numerator inside the range of the kernels' constant division
(tests/test_div_const_cpu.py). The fp32 bound of the solver-level tests is measured on the oracle, never
on the kernel: |got - exp32| <= 4 max |exp32 - exp64|, both expectations computed on the CPU from the
same fp32-representable inputs.
"""
import math

import pytest
import torch

from bits import assert_same_bits
from test_gpu_medium import H2, _cast, _inputs
from test_gpu_sponge import _tapers

pytestmark = pytest.mark.gpu

DEV = "cuda"
ORDERS = (4, 8)
DTYPES = (torch.float64, torch.float32)
# (storage shape, box, chunk, mirror)
CASES = [
    ((20, 21, 70), (4, 15, 1, 19, 1, 68), 0, (0, 20, 0, 69)),          # whole region, faces at the storage edges
    ((20, 40, 140), (5, 13, 6, 30, 60, 133), 3, None),                 # all from storage; across tiles; chunk < M
    ((11, 5, 6), (4, 6, 1, 3, 1, 4), 0, (0, 4, 0, 5)),                 # N = M: reflections reach the far side
    ((14, 30, 80), (4, 9, 4, 25, 4, 69), 0, (3, None, None, 70)),      # one-sided faces off the storage edge
]


def _oracle(u1, u2, m, box, first, taper, order, mirror, dtype=None):
    """reference.step_medium in ``dtype`` (default: that of the inputs) on the same input values."""
    from wave3d.ops import reference

    dt = u1.dtype
    h2 = [_cast(v, dt) for v in H2]  # the kernel casts h2 to the working type
    if dtype is not None:
        u1, u2, m = (t.to(dtype) for t in (u1, u2, m))
        taper = None if taper is None else tuple(t.to(dtype) for t in taper)
    return reference.step_medium(u1, u2, m, box, first=first, hx2=h2[0], hy2=h2[1], hz2=h2[2], taper=taper,
                                 order=order, mirror=mirror)


def _check(got, exp, exp64):
    """Bitwise in fp64 and in fp32; exp64 only shows that the fp32 comparison is not a trivial one."""
    if got.dtype == torch.float64:
        assert torch.equal(got, exp)
    else:
        assert float((exp.double() - exp64).abs().max()) > 0
    assert_same_bits(got, exp)


def _box_mask(shape, box):
    i0, i1, j0, j1, k0, k1 = box
    mask = torch.ones(shape, dtype=torch.bool)
    mask[i0:i1 + 1, j0:j1 + 1, k0:k1 + 1] = False
    return mask


def _at(u, box):
    i0, i1, j0, j1, k0, k1 = box
    return u[i0:i1 + 1, j0:j1 + 1, k0:k1 + 1]


@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_step_matches_reference(C, case, order, dtype, first, sponge):
    from wave3d.ops import kernels, reference

    shape, box, chunk, mirror = CASES[case]
    u1, u2, m = _inputs(shape, dtype)
    taper = _tapers(shape, dtype) if sponge else None
    u = torch.full(shape, -7.0, dtype=dtype, device=DEV)
    stat = kernels.new_err(1)
    ei = (box[0] + 1, box[1])  # exclude the first box plane from the statistic
    kernels.step_medium(u1.to(DEV), u2.to(DEV), m.to(DEV), u, box, first=first, h2=H2, stat=stat, stat_i=ei,
                        chunk=chunk, taper=None if taper is None else tuple(t.to(DEV) for t in taper),
                        order=order, mirror=mirror)
    torch.cuda.synchronize()
    exp = _oracle(u1, u2, m, box, first, taper, order, mirror)
    exp64 = _oracle(u1, u2, m, box, first, taper, order, mirror, torch.float64)
    # the order matters: the 7-point values differ
    if mirror is None:
        assert not torch.equal(exp, _oracle(u1, u2, m, box, first, taper, 2, None))
    uc = u.cpu()
    _check(_at(uc, box), exp, exp64)
    assert bool((uc[_box_mask(shape, box)] == -7.0).all())  # nothing outside the box is written
    want = reference.max_abs_field(exp[ei[0] - box[0]:].double())
    (ga, gr, bad), = kernels.decode_err(stat)
    assert ga == want
    assert gr == -100.0 and not bad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ORDERS)
def test_nonfinite_flag_reaches_the_stencil_width(C, order, dtype):
    """A NaN M nodes outside the box in j enters the stencil and sets the flag; one node further out
    it does not."""
    from wave3d.ops import kernels

    shape, box, chunk, mirror = CASES[1]
    M = order // 2
    for dist, flagged in ((M, True), (M + 1, False)):
        u1, u2, m = _inputs(shape, dtype)
        u1[8, box[2] - dist, 70] = math.nan
        u = torch.zeros(shape, dtype=dtype, device=DEV)
        stat = kernels.new_err(1)
        kernels.step_medium(u1.to(DEV), u2.to(DEV), m.to(DEV), u, box, first=False, h2=H2, stat=stat,
                            stat_i=(box[0], box[1]), chunk=chunk, order=order, mirror=mirror)
        torch.cuda.synchronize()
        (ga, _, bad), = kernels.decode_err(stat)
        assert bad == flagged and math.isfinite(ga)
        assert bool(torch.isnan(u.cpu()).any()) == flagged


@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ORDERS)
def test_save_and_image_modes(C, order, dtype, sponge):
    from wave3d.ops import kernels, reference

    shape, box, chunk, mirror = CASES[1]
    u1, u2, m = _inputs(shape, dtype)
    taper = _tapers(shape, dtype) if sponge else None
    g = torch.Generator().manual_seed(9)
    q = (torch.rand(shape, generator=g, dtype=torch.float64) - 0.5).to(dtype)
    acc0 = (torch.rand(shape, generator=g, dtype=torch.float64) - 0.5).to(dtype)
    dev = [t.to(DEV) for t in (u1, u2, m)]
    kw = dict(first=False, h2=H2, stat_i=(box[0], box[1]), chunk=chunk, order=order, mirror=mirror,
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
    _check(_at(plain.cpu(), box), _oracle(u1, u2, m, box, False, taper, order, mirror),
           _oracle(u1, u2, m, box, False, taper, order, mirror, torch.float64))
    # u and stat are the plain step's bits
    assert torch.equal(saved, plain) and torch.equal(imaged, plain) and sstat == pstat and istat == pstat
    h2 = [_cast(v, dtype) for v in H2]
    want = reference.laplace_star(u1, box, *h2, order=order, mirror=mirror)
    want64 = reference.laplace_star(u1.double(), box, *h2, order=order, mirror=mirror)
    lc = lap.cpu()
    _check(_at(lc, box), want, want64)
    assert bool((lc[_box_mask(shape, box)] == -7.0).all())
    # acc = acc + u1 q, the product rounded first: elementwise, the same bits in either dtype
    exp_acc = acc0.clone()
    _at(exp_acc, box).copy_(_at(acc0, box) + _at(u1, box) * _at(q, box))
    assert torch.equal(acc.cpu(), exp_acc)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ORDERS)
def test_padded_views_and_fused_wrap(C, order, dtype):
    """alloc_level views with M ghost planes per side and the 2M wrap pairs of the solver."""
    from wave3d.ops import kernels

    n, M = 9, order // 2
    shape = (n + 1 + 2 * M, 12, 70)
    box, mirror = (M, n + M, 1, 10, 1, 68), (0, 11, 0, 69)
    wrap = []
    for g in range(1, M + 1):
        wrap += [n + M - g, M - g, M + g, n + M + g]
    cpu = _inputs(shape, dtype)
    dense = [t.to(DEV) for t in cpu]
    ud = torch.zeros(shape, dtype=dtype, device=DEV)
    sd = kernels.new_err(1)
    kw = dict(first=False, h2=H2, stat_i=(M, n + M), wrap=wrap, order=order, mirror=mirror)
    kernels.step_medium(*dense, ud, box, stat=sd, **kw)
    views = [kernels.alloc_level(*shape, dtype) for _ in range(4)]
    for v, t in zip(views, cpu):
        v.copy_(t)
    sv = kernels.new_err(1)
    kernels.step_medium(*views, box, stat=sv, **kw)
    torch.cuda.synchronize()
    uc = views[3].cpu()
    assert torch.equal(uc, ud.cpu()) and kernels.decode_err(sv) == kernels.decode_err(sd)
    assert float(uc[n].abs().sum()) > 0
    for q in range(0, len(wrap), 2):  # the ghost planes equal their sources
        assert torch.equal(uc[wrap[q + 1]], uc[wrap[q]]) and float(uc[wrap[q]].abs().sum()) > 0
    assert sorted(wrap[1::2]) == list(range(M)) + list(range(n + M + 1, n + 2 * M + 1))  # every ghost plane
    for v in views:  # the padding between rows and in front of the view is still zero
        base = v._base
        inside = torch.zeros(base.shape, dtype=torch.bool, device=DEV)
        inside.as_strided(v.shape, v.stride(), v.storage_offset()).fill_(True)
        assert int(inside.sum()) == v.numel() and bool((base[~inside] == 0).all())


def test_rejected_calls(C):
    """Every refusal of the launcher is a ValueError from ops.kernels before any launch; the native
    entry point refuses the same calls on its own."""
    from wave3d.ops import kernels

    shape = (14, 30, 80)
    dt = torch.float64
    u1, u2, m = (t.to(DEV) for t in _inputs(shape, dt))
    u = torch.full(shape, -7.0, dtype=dt, device=DEV)
    stat = kernels.new_err(1)
    good = dict(box=(4, 9, 4, 25, 4, 69), order=8, mirror=(3, None, None, 70), wrap=None)
    bad = [
        dict(order=3), dict(order=6), dict(order=16),
        dict(box=(3, 9, 4, 25, 4, 69)), dict(box=(4, 10, 4, 25, 4, 69)),        # x: nearer than M to the storage edge
        dict(box=(4, 9, 4, 26, 4, 69)), dict(box=(4, 9, 4, 25, 3, 69)),         # y high / z low: no face, nearer than M
        dict(box=(4, 9, 3, 25, 4, 69)), dict(box=(4, 9, 4, 25, 4, 70)),         # on a face
        dict(box=(4, 9, 2, 25, 4, 69)), dict(box=(4, 9, 4, 25, 4, 71)),         # beyond a face
        dict(box=(4, 9, 4, 5, 4, 69), mirror=(3, 6, None, 70)),                 # faces nearer than M
        dict(mirror=(3, None, None, 80)), dict(mirror=(-1, None, None, 70)),    # a face outside the storage
        dict(box=(4, 9, 28, 28, 4, 69), mirror=(27, None, None, 70)),           # a reflected node would leave it
        dict(mirror=(3, None, 70)),                                             # not four entries
        dict(wrap=(9, 14, 4, 0)), dict(wrap=(13, 0)),                           # wrap planes outside the storage
        dict(variant="r2"),
    ]
    for change in bad:
        kw = dict(good, **change)
        box = kw.pop("box")
        with pytest.raises(ValueError):
            kernels.step_medium(u1, u2, m, u, box, first=False, h2=H2, stat=stat, stat_i=(4, 9), **kw)
    # the launcher's own checks, without the Python ones in front
    gv = [*shape, u.stride(1), u.stride(0)]
    no = C.no_mirror

    def native(box, order, mirror, wrap=()):
        C.k_step_medium_f64(False, u1.data_ptr(), u2.data_ptr(), m.data_ptr(), u.data_ptr(), gv, [list(box)], 4, 9,
                            list(wrap), list(H2), stat.data_ptr(), 0, torch.cuda.current_stream().cuda_stream,
                            C.medium_modes["plain"], order=order, mirror=mirror)

    for box, order, mirror, wrap in (
            (good["box"], 6, [3, no, no, 70], ()),
            ((3, 9, 4, 25, 4, 69), 8, [3, no, no, 70], ()),
            ((4, 9, 4, 26, 4, 69), 8, [3, no, no, 70], ()),
            ((4, 9, 3, 25, 4, 69), 8, [3, no, no, 70], ()),
            ((4, 9, 4, 5, 4, 69), 8, [3, 6, no, 70], ()),
            ((4, 9, 28, 28, 4, 69), 8, [27, no, no, 70], ()),
            (good["box"], 8, [3, no, no, 80], ()),
            (good["box"], 8, [3, no, no, 70], (9, 14))):
        with pytest.raises(C.Wave3dError):
            native(box, order, mirror, wrap)
    torch.cuda.synchronize()
    assert bool((u == -7.0).all())  # nothing was launched
    native(good["box"], 8, [3, no, no, 70])  # and the accepted call runs
    torch.cuda.synchronize()
    assert not bool((_at(u, good["box"]) == -7.0).any())


# ---- the solver ------------------------------------------------------------------------------

N, K = 20, 12
SOURCES = [(0, 1, 10), (7, 19, 3)]                               # the periodic plane next to a face; next to a face
RECEIVERS = [(N, 2, 10), (7, N, 3), (8, 19, 4), (6, 18, 2)]      # plane N next to a face, on a face, next to a face


def _solver_case():
    import wave3d

    g = torch.Generator().manual_seed(21)
    # fp32-representable inputs, so that fp32 and fp64 runs start from the same values
    speed2 = (0.2 + 0.4 * torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64)).float().double()
    speed2[N] = speed2[0]
    pert = (speed2 * (1 - 0.1 * torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64))).float().double()
    pert[N] = pert[0]
    tau = 1.0 / K
    w = torch.stack([wave3d.ricker(3.0, 0.3, K, tau), -0.5 * wave3d.ricker(2.0, 0.2, K, tau)], 1).float().double()
    return speed2, pert, w


def _solver(order, sponge, backend, dtype="fp64", speed2=None):
    import wave3d

    s, _, w = _solver_case()
    prob = wave3d.MediumProblem(N, s if speed2 is None else speed2, timesteps=K, dtype=dtype, space_order=order)
    assert prob.courant <= 0.42
    taper = wave3d.sponge_taper(prob, 4) if sponge else None
    return wave3d.MediumSolver(prob, backend, sources=SOURCES, wavelet=w, receivers=RECEIVERS, taper=taper)


@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("order", ORDERS)
def test_solver_matches_oracle(C, order, sponge):
    got = _solver(order, sponge, "hip").run()
    want = _solver(order, sponge, "cpu").run()
    assert float(want.traces.abs().max()) > 1e-3 and float(want.traces[:, 1].abs().max()) == 0  # the face receiver
    assert torch.equal(got.traces, want.traces)
    assert torch.equal(got.u_final, want.u_final)
    assert got.max_abs_u == want.max_abs_u
    assert got.extra["space_order"] == order and not got.aborted
    # fp32: the rule of the module docstring on the traces
    got32 = _solver(order, sponge, "hip", "fp32").run().traces
    want32 = _solver(order, sponge, "cpu", "fp32").run().traces
    bound = 4 * float((want32.double() - want.traces).abs().max())
    err = float((got32.double() - want32.double()).abs().max())
    print("fp32 traces: max |hip - cpu|", err, "bound", bound)
    assert got32.dtype == torch.float32 and bound > 0 and err <= bound


@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("order", ORDERS)
def test_gradient_matches_oracle(C, order, sponge):
    _, pert, _ = _solver_case()
    observed = _solver(order, sponge, "cpu", speed2=pert).run().traces
    want = _solver(order, sponge, "cpu").gradient(observed)
    assert want.misfit > 0 and float(want.grad_speed2.abs().max()) > 0 and float(want.grad_wavelet.abs().max()) > 0
    sol = _solver(order, sponge, "hip")
    for seg in (1, 4, None):  # the result does not depend on the checkpoint schedule
        got = sol.gradient(observed, segment=seg)
        assert got.misfit == want.misfit
        assert torch.equal(got.grad_speed2, want.grad_speed2)
        assert torch.equal(got.grad_wavelet, want.grad_wavelet)
        assert torch.equal(got.traces, want.traces)
        assert got.extra["space_order"] == order


@pytest.fixture(scope="module")
def accuracy():
    """L-inf error of the analytic mode at N = 32, K = 320, T = 1 per order on the GPU, and the CPU
    oracle's at order 2."""
    import wave3d
    from wave3d.ops import reference

    n, k = 32, 320
    sx, sy, sz, ct, c = reference.tables(n, k)
    u0 = reference.analytic(sx, sy, sz, ct[0])
    exact = reference.analytic(sx, sy, sz, ct[k])
    speed2 = 1 / (4 * wave3d.models.wave.PI_REF ** 2)
    err = {}
    for order in (2, 4, 8):
        prob = wave3d.MediumProblem(n, speed2, timesteps=k, space_order=order)
        r = wave3d.MediumSolver(prob, "hip", u0=u0).run()
        err[order] = float((r.u_final - exact).abs().max())
    cpu2 = float((reference.solve_medium(n, k, speed2, u0=u0)[1] - exact).abs().max())
    return err, cpu2


def test_accuracy_on_the_gpu(C, accuracy):
    err, cpu2 = accuracy
    print("L-inf errors at N=32 K=320:", err, "cpu order 2:", cpu2)
    # numpy: 1.78e-4, 8.3e-7, 9.1e-9 (ratios 215 and 1.9e4; the margins leave a factor 4 to 20)
    assert err[8] <= err[2] / 1000
    assert err[4] <= err[2] / 50
    assert abs(err[2] - cpu2) <= 0.05 * cpu2
