"""Density perturbations in Born modelling on the GPU: the scatter and Born-add modes of k_march_mb
(csrc/hip_medium.hip) against ops/reference.py (laplace_density with the buoyancy perturbation in b's place,
step_medium(born_add=...)), and MediumSolver.born(ddensity=...) / gauss_newton(..., ddensity) ("hip": the
background step in scatter mode, the perturbation step in Born-add mode, in lock step) against the "cpu"
backend (ops/reference.py born_medium).

fp64 results must be *bitwise* equal: both sides round every operation in the same order and share the
host-side arithmetic; a single fp32 step is bitwise equal too. fp32 solves stay inside the bound of the sibling
tests, measured on the oracle and never on the kernel: |got - exp32| <= 4 max |exp32 - exp64|. Inputs: u1, u2 in [0, 1], m in [1e-4, 6e-4], b in
[0.3, 2], db, dm and s in [-1, 1].
"""
import math

import pytest
import torch

from test_gpu_medium import CASES, H2, _cast, _inputs, _rand
from test_gpu_medium_born import _front_end_case, _perturbations
from test_gpu_medium_density import _buoyancy
from test_gpu_medium_gradient import _dense
from test_gpu_medium_order import _at, _box_mask, _check
from test_gpu_sponge import _tapers

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -7.0
DTYPES = (torch.float64, torch.float32)
# the adjoint dot test's |lhs - rhs| / |lhs| of the N = 20 case over the three blocks, measured on the "cpu"
# backend (whose fp64 results are those of "hip" bit for bit)
DOT_MEASURED = 1.037e-15


def _step_inputs(shape, dtype, sponge):
    """CPU tensors (u1, u2, m, b, db, dm, s, taper or None): db, dm and s of both signs."""
    u1, u2, m = _inputs(shape, dtype)
    return (u1, u2, m, _buoyancy(shape, dtype), _rand(shape, dtype, 8, -1.0, 1.0), _rand(shape, dtype, 7, -1.0, 1.0),
            _rand(shape, dtype, 9, -1.0, 1.0), _tapers(shape, dtype) if sponge else None)


def _h(dtype):
    return [_cast(v, dtype) for v in H2]  # the kernel casts h2 to the working type


def _oracle_scatter(cpu, box, dtype=None):
    """(u, s) of the scatter step from the oracle's pieces, in ``dtype`` (default: that of the inputs)."""
    from wave3d.ops import reference

    u1, u2, m, b, db, dm, _, tp = cpu
    h = _h(u1.dtype)
    if dtype is not None:
        u1, u2, m, b, db, dm = (t.to(dtype) for t in (u1, u2, m, b, db, dm))
        tp = None if tp is None else tuple(t.to(dtype) for t in tp)
    u = reference.step_medium(u1, u2, m, box, first=False, hx2=h[0], hy2=h[1], hz2=h[2], taper=tp, buoyancy=b)
    q = reference._lap_box(u1, box, h[0], h[1], h[2], 2, None, b)
    r = reference._lap_box(u1, box, h[0], h[1], h[2], 2, None, db)
    return u, _at(dm, box) * q + _at(m, box) * r


def _oracle_add(cpu, box, s=None, dtype=None, **kw):
    from wave3d.ops import reference

    u1, u2, m, b, _, _, s0, tp = cpu
    s = s0 if s is None else s
    h = _h(u1.dtype)
    if dtype is not None:
        u1, u2, m, b, s = (t.to(dtype) for t in (u1, u2, m, b, s))
        tp = None if tp is None else tuple(t.to(dtype) for t in tp)
    return reference.step_medium(u1, u2, m, box, first=False, hx2=h[0], hy2=h[1], hz2=h[2], taper=tp, buoyancy=b,
                                 born_add=_at(s, box).clone(), **kw)


def _run(cpu, box, chunk, mode, padded=False, s=None, stat_i=None, wrap=None, **over):
    """The device step on copies of the CPU inputs. mode: "scatter", "add", "plain", "save" or "born" (the
    last with q = s and dm). Returns (u, stat, the mode's device grids)."""
    from wave3d.ops import kernels

    u1, u2, m, b, db, dm, s0, tp = cpu
    d = [_dense(t, padded) for t in (u1, u2, m)]
    u = _dense(torch.full(u1.shape, SENT, dtype=u1.dtype), padded)
    stat = kernels.new_err(1)
    if mode == "scatter":
        grids = (_dense(torch.full(u1.shape, SENT, dtype=u1.dtype), padded), _dense(dm, padded), _dense(db, padded))
        kw = dict(scatter=grids)
    elif mode == "add":
        grids = (_dense(s0 if s is None else s, padded),)
        kw = dict(born_add=grids[0])
    elif mode == "save":
        grids = (_dense(torch.full(u1.shape, SENT, dtype=u1.dtype), padded),)
        kw = dict(lap_out=grids[0])
    elif mode == "born":
        grids = (_dense(s0 if s is None else s, padded), _dense(dm, padded))
        kw = dict(born=grids)
    else:
        grids, kw = (), {}
    kw.update(over)
    kernels.step_medium(*d, u, box, first=False, h2=H2, stat=stat, stat_i=stat_i or (box[0] + 1, box[1]), chunk=chunk,
                        taper=None if tp is None else tuple(t.to(DEV) for t in tp), buoyancy=_dense(b, padded),
                        wrap=wrap, **kw)
    torch.cuda.synchronize()
    return u, stat, grids


def _padding_is_zero(v):
    base = v._base
    inside = torch.zeros(base.shape, dtype=torch.bool, device=DEV)
    inside.as_strided(v.shape, v.stride(), v.storage_offset()).fill_(True)
    return bool((base[~inside] == 0).all())


# ---- single steps ---------------------------------------------------------------------------------

@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_scatter_step_matches_reference(C, case, dtype, sponge):
    from wave3d.ops import kernels

    shape, box, chunk = CASES[case]
    cpu = _step_inputs(shape, dtype, sponge)
    u, stat, (s, dmd, dbd) = _run(cpu, box, chunk, "scatter")
    plain, pstat, _ = _run(cpu, box, chunk, "plain")
    # u and the statistic are the plain density step's, bit for bit, in both types
    assert torch.equal(u, plain) and kernels.decode_err(stat) == kernels.decode_err(pstat)
    assert not kernels.decode_err(stat)[0][2]
    exp_u, exp_s = _oracle_scatter(cpu, box)
    exp_u64, exp_s64 = _oracle_scatter(cpu, box, torch.float64)
    # both terms of s matter
    _, only_q = _oracle_scatter(cpu[:4] + (torch.zeros_like(cpu[4]),) + cpu[5:], box)
    _, only_r = _oracle_scatter(cpu[:5] + (torch.zeros_like(cpu[5]),) + cpu[6:], box)
    assert not torch.equal(exp_s, only_q) and not torch.equal(exp_s, only_r)
    uc, sc = u.cpu(), s.cpu()
    _check(_at(uc, box), exp_u, exp_u64)
    _check(_at(sc, box), exp_s, exp_s64)
    mask = _box_mask(shape, box)
    assert bool((uc[mask] == SENT).all()) and bool((sc[mask] == SENT).all())  # nothing outside the box is written
    assert torch.equal(dmd.cpu(), cpu[5]) and torch.equal(dbd.cpu(), cpu[4])  # dm and db are read only


@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_born_add_step_matches_reference(C, case, dtype, sponge):
    from wave3d.ops import kernels, reference

    shape, box, chunk = CASES[case]
    cpu = _step_inputs(shape, dtype, sponge)
    u, stat, (sd,) = _run(cpu, box, chunk, "add")
    exp, exp64 = _oracle_add(cpu, box), _oracle_add(cpu, box, dtype=torch.float64)
    uc = u.cpu()
    _check(_at(uc, box), exp, exp64)
    assert bool((uc[_box_mask(shape, box)] == SENT).all())
    want = reference.max_abs_field(exp[1:].double())  # of the updated values, over the planes after the first
    (ga, gr, bad), = kernels.decode_err(stat)
    assert ga == want
    assert gr == -100.0 and not bad
    assert torch.equal(sd.cpu(), cpu[6])  # s is read only


@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("case", [0, 2])
def test_born_add_step_against_the_plain_and_the_born_step(C, case, sponge):
    from wave3d.ops import kernels

    shape, box, chunk = CASES[case]
    dt = torch.float64
    cpu = _step_inputs(shape, dt, sponge)
    # s = 0: the plain step (x + 0)
    u, stat, _ = _run(cpu, box, chunk, "add", s=torch.zeros(shape, dtype=dt))
    plain, pstat, _ = _run(cpu, box, chunk, "plain")
    assert torch.equal(u, plain) and kernels.decode_err(stat) == kernels.decode_err(pstat)
    # s = dm q formed on the host: today's Born mode
    q, dm = cpu[6], cpu[5]
    u, stat, _ = _run(cpu, box, chunk, "add", s=dm * q)
    born, bstat, _ = _run(cpu, box, chunk, "born")
    assert torch.equal(u, born) and kernels.decode_err(stat) == kernels.decode_err(bstat)
    assert not torch.equal(born, plain)
    # and scatter mode with db = 0 stores dm D_b u1, save mode's value times dm
    zero_db = cpu[:4] + (torch.zeros(shape, dtype=dt),) + cpu[5:]
    _, _, (s, _, _) = _run(zero_db, box, chunk, "scatter")
    _, _, (lap,) = _run(cpu, box, chunk, "save")
    assert torch.equal(_at(s, box), _at(dm.to(DEV) * lap, box))


@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["scatter", "add"])
def test_padded_views(C, mode, dtype, sponge):
    """alloc_level views give the dense tensors' bits, and the padding between the rows stays zero."""
    from wave3d.ops import kernels

    shape, box, chunk = CASES[2]
    cpu = _step_inputs(shape, dtype, sponge)
    u, stat, grids = _run(cpu, box, chunk, mode, padded=True)
    dense, dstat, dgrids = _run(cpu, box, chunk, mode)
    assert u.stride(1) > shape[2]  # padded pitch
    assert torch.equal(u.cpu(), dense.cpu()) and kernels.decode_err(stat) == kernels.decode_err(dstat)
    for a, b in zip(grids, dgrids):
        assert torch.equal(a.cpu(), b.cpu())
    if dtype == torch.float64:
        if mode == "scatter":
            exp_u, exp_s = _oracle_scatter(cpu, box)
            assert torch.equal(_at(u.cpu(), box), exp_u) and torch.equal(_at(grids[0].cpu(), box), exp_s)
        else:
            assert torch.equal(_at(u.cpu(), box), _oracle_add(cpu, box))
    for v in (u, *grids):
        assert _padding_is_zero(v)


def test_fused_wrap(C):
    """The periodic wrap carries the updated planes of u in both modes, and never s."""
    _, box, chunk = CASES[0]
    shape = CASES[0][0]
    cpu = _step_inputs(shape, torch.float64, True)
    nx = shape[0]
    wrap = (nx - 2, 0, 1, nx - 1)
    sl = (slice(box[2], box[3] + 1), slice(box[4], box[5] + 1))
    u, _, _ = _run(cpu, box, chunk, "add", wrap=wrap, stat_i=(1, nx - 2))
    exp = _oracle_add(cpu, box)
    uc = u.cpu()
    assert torch.equal(_at(uc, box), exp)
    assert torch.equal(uc[0][sl], exp[-1]) and torch.equal(uc[nx - 1][sl], exp[0])
    u, _, (s, _, _) = _run(cpu, box, chunk, "scatter", wrap=wrap, stat_i=(1, nx - 2))
    exp_u, exp_s = _oracle_scatter(cpu, box)
    uc, sc = u.cpu(), s.cpu()
    assert torch.equal(_at(uc, box), exp_u) and torch.equal(_at(sc, box), exp_s)
    assert torch.equal(uc[0][sl], exp_u[-1]) and torch.equal(uc[nx - 1][sl], exp_u[0])
    assert bool((sc[0] == SENT).all()) and bool((sc[nx - 1] == SENT).all())


def test_nonfinite_values_reach_the_flag_of_their_field(C):
    """A NaN in db next to the box enters s through the half-face average and leaves u and the background
    step's flag alone; the Born-add step that reads that s raises the flag of the perturbation field."""
    from wave3d.ops import kernels

    shape, box, chunk = CASES[1]  # an interior sub-box: (2, 10, 3, 17, 2, 66)
    dt = torch.float64
    cpu = _step_inputs(shape, dt, False)
    bad_db = cpu[4].clone()
    bad_db[5, 2, 33] = math.nan  # j = 2 lies outside the box, next to the box node (5, 3, 33)
    u, stat, (s, _, _) = _run(cpu[:4] + (bad_db,) + cpu[5:], box, chunk, "scatter")
    plain, pstat, _ = _run(cpu, box, chunk, "plain")
    assert torch.equal(u, plain) and kernels.decode_err(stat) == kernels.decode_err(pstat)
    assert not kernels.decode_err(stat)[0][2]
    assert bool(torch.isnan(s[5, 3, 33])) and int(torch.isnan(s).sum()) == 1
    u, stat, _ = _run(cpu, box, chunk, "add", s=s.cpu())
    assert kernels.decode_err(stat)[0][2]
    assert bool(torch.isnan(u[5, 3, 33])) and int(torch.isnan(u).sum()) == 1
    # a NaN in s at a box node does the same, one outside the box is never read
    bad_s = cpu[6].clone()
    bad_s[4, 9, 20] = math.nan
    u, stat, _ = _run(cpu, box, chunk, "add", s=bad_s)
    assert kernels.decode_err(stat)[0][2] and bool(torch.isnan(u[4, 9, 20])) and int(torch.isnan(u).sum()) == 1
    bad_s = cpu[6].clone()
    bad_s[4, 2, 20] = math.nan
    u, stat, _ = _run(cpu, box, chunk, "add", s=bad_s)
    assert not kernels.decode_err(stat)[0][2] and not bool(torch.isnan(u).any())


def test_rejected_calls(C):
    """Every refusal is a ValueError from ops.kernels before any launch; the native entry point refuses
    the same calls on its own (past the Python checks). The outputs keep their sentinels."""
    from wave3d.ops import kernels

    shape, box, _ = CASES[3]
    dt = torch.float64
    u1, u2, m = (t.to(DEV) for t in _inputs(shape, dt))
    b = _buoyancy(shape, dt).to(DEV)
    u = torch.full(shape, SENT, dtype=dt, device=DEV)
    so = torch.full(shape, SENT, dtype=dt, device=DEV)
    x, dm, db, s = (torch.zeros(shape, dtype=dt, device=DEV) for _ in range(4))
    kw = dict(h2=H2, stat=kernels.new_err(1), stat_i=(1, 4))

    def step(first=False, **more):
        kernels.step_medium(u1, u2, m, u, box, first=first, **{**kw, "buoyancy": b, **more})

    sc, ad = dict(scatter=(so, dm, db)), dict(born_add=s)
    for mode in (sc, ad):
        with pytest.raises(ValueError, match="buoyancy"):
            step(buoyancy=None, **mode)
        with pytest.raises(ValueError, match="order"):  # density at orders 4 and 8 does not exist
            step(order=4, **mode)
        with pytest.raises(ValueError, match="buoyancy"):
            step(buoyancy=None, order=4, **mode)
        for v in ("plain", "r2", "r2nt"):
            with pytest.raises(ValueError, match="variant"):
                step(variant=v, **mode)
        with pytest.raises(ValueError, match="first"):
            step(first=True, **mode)
        with pytest.raises(ValueError, match="combined"):
            step(lap_out=x, **mode)
        with pytest.raises(ValueError, match="combined"):
            step(image=(x, dm), **mode)
        with pytest.raises(ValueError, match="combined"):
            step(born=(x, dm), **mode)
    with pytest.raises(ValueError, match="combined"):
        step(**sc, **ad)
    for g in (u, u1, u2, m, b):
        with pytest.raises(ValueError, match="shares memory"):
            step(scatter=(g, dm, db))
    with pytest.raises(ValueError, match="shares memory"):
        step(scatter=(so, so, db))
    with pytest.raises(ValueError, match="shares memory"):
        step(scatter=(so, dm, so))
    with pytest.raises(ValueError, match="shares memory"):
        step(born_add=u)
    with pytest.raises(ValueError):
        step(scatter=(so, dm))
    with pytest.raises(ValueError):
        step(scatter=(so, None, db))
    for bad in (dm.float(), dm[:-1], kernels.alloc_level(*shape, dt), dm.cpu()):  # dtype, shape, strides, device
        for pos in range(3):
            grids = [so, dm, db]
            grids[pos] = bad
            with pytest.raises(ValueError):
                step(scatter=tuple(grids))
        with pytest.raises(ValueError):
            step(born_add=bad)
    # the launcher refuses them as well
    gv = [*shape, shape[2], shape[1] * shape[2]]
    args = [u1.data_ptr(), u2.data_ptr(), m.data_ptr(), u.data_ptr(), gv, [list(box)], 1, 4, [], list(H2),
            kw["stat"].data_ptr(), 0, torch.cuda.current_stream().cuda_stream]
    B, SO, D, DB, S, X, U = (t.data_ptr() for t in (b, so, dm, db, s, x, u))
    SC, AD = C.medium_modes["scatter"], C.medium_modes["born_add"]
    scg, adg = dict(b=B, s_out=SO, dm=D, db=DB), dict(b=B, sadd=S)  # the grids of the two modes, with b

    def without(grids, name):
        return {k: v for k, v in grids.items() if k != name}

    for first, mode, variant, order, grids in (
            (False, SC, 1, 2, without(scg, "b")),            # scatter without b
            (False, AD, 1, 2, without(adg, "b")),            # Born-add without b
            (False, SC, 1, 4, scg),                          # another order
            (False, AD, 1, 8, adg),
            (False, SC, 0, 2, scg),                          # another variant
            (False, AD, 3, 2, adg),
            (True, SC, 1, 2, scg),                           # the Taylor start
            (True, AD, 1, 2, adg),
            (False, SC, 1, 2, without(scg, "s_out")),        # scatter without s_out
            (False, SC, 1, 2, without(scg, "dm")),           # scatter without dm
            (False, SC, 1, 2, dict(scg, q=X)),               # with q (Born / image)
            (False, SC, 1, 2, dict(scg, q=X, acc=X)),
            (False, AD, 1, 2, dict(adg, lap_out=X)),         # Born-add with save
            (False, AD, 1, 2, dict(adg, q=X, acc=X)),        # with image
            (False, AD, 1, 2, dict(adg, q=X, dm=D)),         # with Born
            (False, SC, 1, 2, dict(scg, sadd=S)),            # both modes
            (False, AD, 1, 2, dict(scg, sadd=S)),
            (False, SC, 1, 2, dict(scg, s_out=U)),           # s_out is u, u1, m, b, dm, db
            (False, SC, 1, 2, dict(scg, s_out=u1.data_ptr())),
            (False, SC, 1, 2, dict(scg, s_out=m.data_ptr())),
            (False, SC, 1, 2, dict(scg, s_out=B)),
            (False, SC, 1, 2, dict(scg, s_out=D)),
            (False, SC, 1, 2, dict(scg, s_out=DB)),
            (False, AD, 1, 2, dict(adg, sadd=U))):           # s is u
        with pytest.raises(C.Wave3dError):
            C.k_step_medium_f64(first, *args, mode, variant=variant, order=order, **grids)
    torch.cuda.synchronize()
    assert bool((u == SENT).all()) and bool((so == SENT).all()) and not bool(x.any())  # nothing was launched
    # both modes do run with these grids
    step(**sc)
    torch.cuda.synchronize()
    assert not bool((_at(u, box) == SENT).any()) and not bool((_at(so, box) == SENT).any())
    u.fill_(SENT)
    step(**ad)
    torch.cuda.synchronize()
    assert not bool((_at(u, box) == SENT).any())


# ---- the front-end: MediumSolver.born(ddensity=...) and gauss_newton, "hip" against "cpu" ---------------

def _ddensity(prob, seed=13, walls=True):
    """A density perturbation of both signs, periodic in x; ``walls=False``: zero on the y/z faces."""
    N = prob.N
    g = torch.Generator().manual_seed(seed)
    dr = 0.2 * (torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64) - 0.5)
    dr[N] = dr[0]
    if not walls:
        dr[:, 0, :] = 0
        dr[:, N, :] = 0
        dr[:, :, 0] = 0
        dr[:, :, N] = 0
    return dr


def _same_born(got, want):
    assert torch.equal(got.traces, want.traces)
    assert torch.equal(got.dtraces, want.dtraces)
    assert torch.equal(got.du_final, want.du_final)
    assert got.max_abs_du == want.max_abs_du


# (N, K, sponge, with ds and dw): N = 70 has two k tiles, five j tiles and a partial tile on both axes
FRONT_END = [(20, 24, True, True), (20, 24, False, False), (20, 12, False, True), (20, 12, True, False),
             (70, 8, True, True), (70, 6, False, False)]


@pytest.mark.parametrize("N,K,sponge,joint", FRONT_END)
def test_born_matches_oracle_fp64(C, N, K, sponge, joint):
    import wave3d

    prob, kw = _front_end_case(N, K, sponge, density=True)
    assert prob.stable()
    ds, dw, _ = _perturbations(prob, kw)
    dr = _ddensity(prob)
    args = (ds, dw, dr) if joint else (None, None, dr)
    want = wave3d.MediumSolver(prob, "cpu", **kw).born(*args)
    sol = wave3d.MediumSolver(prob, "hip", **kw)
    got = sol.born(*args)
    assert float(want.dtraces.abs().max()) > 0 and not bool(want.dtraces[0].any())
    _same_born(got, want)
    assert isinstance(got, wave3d.MediumBorn) and got.extra["ddensity"] is True and got.extra["density"] is True
    assert got.extra["levels"] == wave3d.born_levels(density=True, ddensity=True) == 11


@pytest.fixture(scope="module")
def n20():
    """N = 20, K = 24 with sponge and a random density: the problem, its perturbations (the density's zero
    on the y/z faces) and the oracle's Born run, computed once."""
    import wave3d

    prob, kw = _front_end_case(20, 24, True, density=True)
    ds, dw, r = _perturbations(prob, kw)
    dr = _ddensity(prob, walls=False)
    return prob, kw, ds, dw, dr, r, wave3d.MediumSolver(prob, "cpu", **kw).born(ds, dw, dr)


def test_born_with_a_scalar_density(C):
    import wave3d

    base, kw = _front_end_case(20, 12, True)
    prob = wave3d.MediumProblem(20, base.speed2, T=base.T, timesteps=12, density=1.5)
    ds, dw, _ = _perturbations(prob, kw)
    for args in ((None, None, _ddensity(prob)), (ds, dw, 0.05)):
        want = wave3d.MediumSolver(prob, "cpu", **kw).born(*args)
        assert float(want.dtraces.abs().max()) > 0
        _same_born(wave3d.MediumSolver(prob, "hip", **kw).born(*args), want)


def test_born_with_zero_ddensity_is_born_without(C, n20):
    """The scatter and Born-add kernels against the save and Born kernels."""
    import wave3d

    prob, kw, ds, dw, dr, _, _ = n20
    sol = wave3d.MediumSolver(prob, "hip", **kw)
    old = sol.born(ds, dw)
    new = sol.born(ds, dw, 0 * dr)
    assert old.extra["levels"] == 10 and old.extra["ddensity"] is False and new.extra["levels"] == 11
    _same_born(new, old)
    _same_born(sol.born(ds, dw, 0.0), old)


def test_born_fp32(C, n20):
    import wave3d

    prob, kw, ds, dw, dr, _, ref = n20
    p32 = wave3d.MediumProblem(prob.N, prob.speed2, T=prob.T, timesteps=prob.timesteps, dtype="fp32",
                               density=prob.density)
    cpu = wave3d.MediumSolver(p32, "cpu", **kw).born(ds, dw, dr)
    hip = wave3d.MediumSolver(p32, "hip", **kw).born(ds, dw, dr)
    assert hip.dtraces.dtype == torch.float32 and hip.du_final.dtype == torch.float32

    def rel(a, b):
        return float((a.double() - b).abs().max() / b.abs().max())

    # both sides accumulate fp32 rounding over the same K steps in different orders: the bound is the fp32
    # oracle's own error against the fp64 oracle, times 4, as in test_gpu_medium_born.py
    for name in ("dtraces", "du_final", "traces"):
        e_cpu, e_hip = rel(getattr(cpu, name), getattr(ref, name)), rel(getattr(hip, name), getattr(ref, name))
        print(f"fp32 {name}: oracle error {e_cpu:.3e}, hip error {e_hip:.3e}")
        assert e_cpu > 0
        assert e_hip <= 4 * e_cpu


@pytest.mark.parametrize("segment", [1, 3, 23, None])
def test_gauss_newton_matches_oracle(C, n20, segment):
    import wave3d

    prob, kw, ds, dw, dr, _, ref = n20
    assert prob.timesteps - 1 == 23
    want = _gn_oracle(n20)
    got = wave3d.MediumSolver(prob, "hip", **kw).gauss_newton(ds, dw, dr, segment=segment)
    assert got.misfit == want.misfit and got.extra["wrt_density"] is True
    assert torch.equal(got.grad_speed2, want.grad_speed2)
    assert torch.equal(got.grad_wavelet, want.grad_wavelet)
    assert torch.equal(got.grad_density, want.grad_density)
    assert torch.equal(got.traces, want.traces) and torch.equal(got.extra["dtraces"], ref.dtraces)


_GN = {}


def _gn_oracle(n20):
    """The "cpu" backend's Gauss-Newton product of the n20 case, computed once."""
    import wave3d

    if "want" not in _GN:
        prob, kw, ds, dw, dr, _, ref = n20
        want = wave3d.MediumSolver(prob, "cpu", **kw).gauss_newton(ds, dw, dr)
        assert want.misfit > 0 and float(want.grad_density.abs().max()) > 0
        assert float(want.grad_speed2.abs().max()) > 0 and float(want.grad_wavelet.abs().max()) > 0
        assert torch.equal(want.extra["dtraces"], ref.dtraces)
        _GN["want"] = want
    return _GN["want"]


def test_adjoint_dot_test_on_the_gpu(C, n20):
    """<J d, r> from born(ds, dw, drho) against <d, J^T r> from gradient(traces - r, wrt_density=True), both
    on the GPU, drho zero on the y/z faces."""
    import wave3d

    prob, kw, ds, dw, dr, r, _ = n20
    N = prob.N
    sol = wave3d.MediumSolver(prob, "hip", **kw)
    b = sol.born(ds, dw, dr)
    g = sol.gradient(b.traces - r, wrt_density=True)
    lhs = float((b.dtraces[1:] * r[1:]).sum())
    rho_part = float((g.grad_density[:N] * dr[:N]).sum())
    rhs = float((g.grad_speed2[:N] * ds[:N]).sum() + rho_part + (g.grad_wavelet * dw).sum())
    e = abs(lhs - rhs) / abs(lhs)
    print(f"<J d, r> = {lhs!r}, <d, J^T r> = {rhs!r} (density block {rho_part!r}), relative difference {e:.3e}")
    assert abs(lhs) > 1e-3 * float(b.dtraces[1:].norm() * r[1:].norm())
    assert abs(rho_part) > 1e-3 * abs(lhs)  # the density block takes part
    # the CPU test's bound: 100 times the difference measured for this case (on the "cpu" backend, whose
    # fp64 results are those of "hip" bit for bit: DOT_MEASURED), capped at 1e-9
    assert e <= min(100 * max(DOT_MEASURED, 2.0 ** -52), 1e-9)


def test_born_argument_checks_on_the_hip_backend(C, n20):
    import wave3d

    prob, kw, ds, _, dr, _, _ = n20
    bare, bkw = _front_end_case(20, 24, True)
    with pytest.raises(ValueError, match="needs a density model"):
        wave3d.MediumSolver(bare, "hip", **bkw).born(ds, ddensity=dr)
    sol = wave3d.MediumSolver(prob, "hip", **kw)
    bad = dr.clone()
    bad[3, 4, 5] = math.nan
    with pytest.raises(ValueError, match="ddensity must be finite"):
        sol.born(ddensity=bad)
    with pytest.raises(ValueError, match="perturbation"):
        sol.born()
