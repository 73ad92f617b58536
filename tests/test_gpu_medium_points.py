"""Off-grid sources and receivers on the GPU: k_record_w, k_inject_rows and k_rows_dot
(csrc/hip_medium_points.hip) against the oracle ops of ops/reference.py, and MediumSolver with
source_positions / receiver_positions on "hip" against the "cpu" backend.

The point kernels are rounded multiplies and adds in a fixed order, so fp64 and fp32 results are
bitwise those of PyTorch on the CPU.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float64, torch.float32]
SHAPE = (13, 12, 11)          # [Nx + 1 + 2][Ny + 1][Nz + 1] with one x ghost plane per side
NN = (10, 11, 10)             # intervals per axis
WRAP = (10, 0, 2, 12)         # ghost -1 <- global 9, ghost 11 <- global 1
# on a node; folded at the low y face; folded at the high z face; across the x seam; two 1.5 nodes apart
POINTS = torch.tensor([[4.0, 5.0, 6.0], [3.3, 0.4, 4.2], [5.6, 6.3, 9.7], [9.8, 5.5, 5.5], [5.2, 5.2, 5.2],
                       [6.7, 5.2, 5.2]], dtype=torch.float64)


def _rand(shape, dtype, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64)).to(dtype)


def _level(t, padded):
    """A device copy of the CPU tensor t: dense, or an alloc_level padded view."""
    from wave3d.ops import kernels

    if not padded:
        return t.to(DEV)
    v = kernels.alloc_level(*t.shape, t.dtype)
    v.copy_(t)
    return v


def _padding_is_zero(x):
    base = x._base
    inside = torch.zeros(base.shape, dtype=torch.bool, device=DEV)
    inside.as_strided(x.shape, x.stride(), x.storage_offset()).fill_(True)
    return bool((base[~inside] == 0).all())


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_record_weighted_is_the_oracle_bit_for_bit(C, dtype, padded):
    from wave3d.ops import kernels, reference

    u = _rand(SHAPE, dtype, 1)
    index, weight = reference.receiver_tables(POINTS, NN, dtype)
    exp = reference.record_weighted(u, index, weight)
    assert exp[0] == u[5, 5, 6]  # the on-node receiver reads its node (x storage = global + 1)
    assert float(exp.abs().min()) > 0
    ud = _level(u, padded)
    out = torch.full((len(POINTS) + 2,), -7.0, dtype=dtype, device=DEV)
    kernels.record_weighted(ud, kernels.point_tables(index, weight, ud), out)
    got = out.cpu()
    assert torch.equal(got[:len(POINTS)], exp)
    assert bool((got[len(POINTS):] == -7.0).all())
    assert torch.equal(ud.cpu(), u)


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_inject_rows_and_rows_dot_are_the_oracle_bit_for_bit(C, dtype, padded):
    from wave3d.ops import kernels, reference

    u, m = _rand(SHAPE, dtype, 2), _rand(SHAPE, dtype, 3, 0.5, 1.5)
    g = _rand((len(POINTS),), dtype, 4)
    rows = reference.point_rows(POINTS, NN, dtype)
    assert rows.unique < len(rows)                       # the seam point touches plane 0: twin rows on plane N
    assert int((rows.rowptr[1:] - rows.rowptr[:-1]).max()) > 1  # overlapping supports share rows
    exp = u.clone()
    reference.inject_rows(exp, m, rows, g)
    i, j, k = rows.ijk()
    for src, dst in ((WRAP[0], WRAP[1]), (WRAP[2], WRAP[3])):  # the ghost copies of the touched nodes alone
        on = i == src
        exp[dst, j[on], k[on]] = exp[src, j[on], k[on]]
        assert bool(on.any())
    sacc0 = _rand((rows.unique,), dtype, 5)
    exp_dot = reference.rows_dot(u, rows, g, sacc0)

    ud, md = _level(u, padded), _level(m, padded)
    rl = kernels.row_list(rows, ud)
    sacc = sacc0.to(DEV)
    kernels.rows_dot(ud, rl, g.to(DEV), sacc)
    assert torch.equal(ud.cpu(), u)                      # the dot writes sacc alone
    assert torch.equal(sacc.cpu(), exp_dot)
    kernels.inject_rows(ud, md, rl, g.to(DEV), WRAP)
    got = ud.cpu()
    assert torch.equal(got, exp)                         # the rows, their wrap copies, and nothing else
    touched = got != u
    assert 0 < int(touched.sum()) <= len(rows) + int(((i == WRAP[0]) | (i == WRAP[2])).sum())
    assert torch.equal(md.cpu(), m)
    if padded:
        assert _padding_is_zero(ud)


@pytest.mark.parametrize("dtype", DTYPES)
def test_single_on_node_entry_is_inject(C, dtype):
    from wave3d.ops import kernels, reference

    u, m = _rand(SHAPE, dtype, 6), _rand(SHAPE, dtype, 7, 0.5, 1.5)
    g = _rand((2,), dtype, 8)
    nodes = [(2, 5, 6), (10, 3, 4)]  # both on wrap source planes
    rows = reference.point_rows(torch.tensor([[1.0, 5.0, 6.0], [9.0, 3.0, 4.0]], dtype=torch.float64), NN, dtype)
    assert rows.nodes.tolist() == [list(nd) for nd in nodes] and rows.w.tolist() == [1.0, 1.0]
    a, b = u.to(DEV), u.to(DEV)
    kernels.inject(a, m.to(DEV), nodes, g.to(DEV), WRAP)
    kernels.inject_rows(b, m.to(DEV), kernels.row_list(rows, b), g.to(DEV), WRAP)
    assert torch.equal(a, b) and not torch.equal(a.cpu(), u)
    assert a[12, 5, 6] == a[2, 5, 6] and a[0, 3, 4] == a[10, 3, 4]


def test_wrappers_refuse_bad_calls_before_any_launch(C):
    from wave3d.ops import kernels, reference

    dt = torch.float64
    u, m = torch.zeros(SHAPE, dtype=dt, device=DEV), torch.ones(SHAPE, dtype=dt, device=DEV)
    index, weight = reference.receiver_tables(POINTS, NN, dt)
    rows = reference.point_rows(POINTS, NN, dt)
    tb, rl = kernels.point_tables(index, weight, u), kernels.row_list(rows, u)
    out = torch.full((len(POINTS),), -7.0, dtype=dt, device=DEV)
    g = torch.ones(len(POINTS), dtype=dt, device=DEV)
    sacc = torch.zeros(rows.unique, dtype=dt, device=DEV)

    bad = index.clone()
    bad[1, 2, 3] = SHAPE[2]
    with pytest.raises(ValueError, match="outside the storage"):
        kernels.point_tables(bad, weight, u)
    with pytest.raises(ValueError):
        kernels.point_tables(index[:, :, :7], weight[:, :, :7], u)
    with pytest.raises(ValueError):
        kernels.point_tables(index, weight.float(), u)
    kw = dict(ncols=rows.ncols, unique=rows.unique, shape=u.shape, device=u.device, dtype=dt)
    nodes = rows.nodes.clone()
    nodes[0, 1] = 0  # on a face: outside the owned region
    with pytest.raises(ValueError, match="owned region"):
        kernels.RowList(nodes, rows.rowptr, rows.col, rows.w, **kw)
    nodes = rows.nodes.clone()
    nodes[1] = nodes[0]
    with pytest.raises(ValueError, match="more than one row"):
        kernels.RowList(nodes, rows.rowptr, rows.col, rows.w, **kw)
    ptr = rows.rowptr.clone()
    ptr[2] = ptr[1] - 1
    with pytest.raises(ValueError, match="rowptr"):
        kernels.RowList(rows.nodes, ptr, rows.col, rows.w, **kw)
    col = rows.col.clone()
    col[0] = rows.ncols
    with pytest.raises(ValueError, match="col"):
        kernels.RowList(rows.nodes, rows.rowptr, col, rows.w, **kw)
    with pytest.raises(ValueError):
        kernels.RowList(rows.nodes, rows.rowptr, rows.col, rows.w.float(), **kw)

    other = torch.zeros(SHAPE[0] + 1, *SHAPE[1:], dtype=dt, device=DEV)
    for call in (lambda: kernels.record_weighted(other, tb, out),            # tables of another grid
                 lambda: kernels.record_weighted(u, rl, out),                # not a table
                 lambda: kernels.record_weighted(u, tb, out[:-1]),           # too short
                 lambda: kernels.record_weighted(u, tb, out.float()),        # another dtype
                 lambda: kernels.record_weighted(u, tb, out.cpu()),          # not on the device
                 lambda: kernels.record_weighted(u, tb, u[3, 3, :len(POINTS)]),  # shares memory with u
                 lambda: kernels.inject_rows(other, other, rl, g),
                 lambda: kernels.inject_rows(u, m.float(), rl, g),
                 lambda: kernels.inject_rows(u, m, tb, g),
                 lambda: kernels.inject_rows(u, m, rl, g[:-1]),              # col would leave g
                 lambda: kernels.inject_rows(u, m, rl, g[::2]),
                 lambda: kernels.inject_rows(u, m, rl, g, (1, 2, 3)),        # wrap pairs
                 lambda: kernels.rows_dot(u, rl, g, sacc[:-1]),
                 lambda: kernels.rows_dot(u, rl, g, u[2, 2, :])):            # shares memory with u
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    assert not bool(u.any()) and bool((out == -7.0).all()) and not bool(sacc.any())  # nothing ran


# ---- MediumSolver with positions: "hip" against "cpu" ---------------------------------------

N, K, T = 16, 12, 0.3
SOURCE_POS = torch.tensor([[0.3, 4.2, 6.7], [6.5, 0.4, 5.1], [15.6, 8.0, 15.7]], dtype=torch.float64)
RECEIVER_POS = POINTS * (N / 10.0)  # the six receivers above, scaled to the grid
CONFIGS = {"order2": (2, False, False), "order2-density-sponge": (2, True, True), "order8-sponge": (8, False, True)}


def _problem(name, dtype="fp64"):
    import wave3d

    order, density, sponge = CONFIGS[name]
    g = torch.Generator().manual_seed(31)

    def field(lo, hi):
        v = lo + (hi - lo) * torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64)
        v[N] = v[0]
        return v

    speed2, pert, rho, ds = field(2, 4), field(1.0, 1.1), field(1, 2), field(-0.2, 0.2)
    prob = wave3d.MediumProblem(N, speed2, T=T, timesteps=K, dtype=dtype, space_order=order,
                                density=rho if density else None)
    tau = T / K
    w = torch.stack([wave3d.ricker(3.0 / T, 0.3 * T, K, tau), -0.5 * wave3d.ricker(2.0 / T, 0.2 * T, K, tau),
                     0.7 * wave3d.ricker(4.0 / T, 0.25 * T, K, tau)], 1)
    kw = dict(source_positions=SOURCE_POS, wavelet=w, receiver_positions=RECEIVER_POS, interp="sinc8",
              taper=wave3d.sponge_taper(prob, 4) if sponge else None)
    return prob, kw, speed2 * pert, ds, 0.3 * w.flip(1)


@pytest.fixture(scope="module", params=list(CONFIGS))
def case(request):
    """One configuration: the problem, and the fp64 oracle's run, gradient and Born run, computed once."""
    import wave3d

    name = request.param
    prob, kw, pert, ds, dw = _problem(name)
    density = CONFIGS[name][1]
    pp = wave3d.MediumProblem(N, pert, T=T, timesteps=K, space_order=prob.space_order, density=prob.density)
    obs = wave3d.MediumSolver(pp, "cpu", **kw).run().traces
    cpu = wave3d.MediumSolver(prob, "cpu", **kw)
    return dict(name=name, prob=prob, kw=kw, obs=obs, ds=ds, dw=dw, density=density, run=cpu.run(),
                grad=cpu.gradient(obs, wrt_density=density, illumination=True), born=cpu.born(ds, dw))


GRAD_FIELDS = ("traces", "grad_speed2", "grad_wavelet", "illumination", "pseudo_hessian_speed2")


def test_solver_matches_the_oracle_fp64(C, case):
    import wave3d

    prob, kw, density = case["prob"], case["kw"], case["density"]
    sol = wave3d.MediumSolver(prob, "hip", **kw)
    run = sol.run()
    assert float(case["run"].traces[1:].abs().max()) > 0
    assert torch.equal(run.traces, case["run"].traces) and torch.equal(run.u_final, case["run"].u_final)
    assert run.extra["interp"] == "sinc8" and run.extra["source_rows"] > 0
    assert run.extra["source_entries"] >= run.extra["source_rows"]

    ref = case["grad"]
    got = sol.gradient(case["obs"], segment=3, wrt_density=density, illumination=True)
    free = sol.gradient(case["obs"], wrt_density=density, illumination=True)  # the default schedule
    assert got.extra["recomputed_steps"] > 0 and got.extra["segment"] == 3
    assert got.extra["receiver_rows"] > 0
    for name in GRAD_FIELDS + (("grad_density",) if density else ()):
        r = getattr(ref, name)
        assert float(r.abs().max()) > 0, name
        assert torch.equal(getattr(got, name), r), name
        assert torch.equal(getattr(free, name), r), name   # gradient() does not depend on the segment
    assert got.misfit == ref.misfit == free.misfit

    born = sol.born(case["ds"], case["dw"])
    assert float(case["born"].dtraces.abs().max()) > 0
    for name in ("traces", "dtraces", "du_final"):
        assert torch.equal(getattr(born, name), getattr(case["born"], name)), name


def test_solver_fp32(C, case):
    """fp32 on "hip" against the fp64 oracle, bounded like tests/test_gpu_medium_gradient.py and
    test_gpu_medium_born.py: at most 4 times the fp32 oracle's own error."""
    import wave3d

    prob, kw, density = case["prob"], case["kw"], case["density"]
    p32 = wave3d.MediumProblem(N, prob.speed2, T=T, timesteps=K, dtype="fp32", space_order=prob.space_order,
                               density=prob.density)
    cpu, hip = wave3d.MediumSolver(p32, "cpu", **kw), wave3d.MediumSolver(p32, "hip", **kw)

    def rel(a, b):
        return float((a.double() - b).abs().max() / b.abs().max())

    def check(c, h, ref, names):
        for name in names:
            assert getattr(h, name).dtype == torch.float32
            e_cpu, e_hip = rel(getattr(c, name), getattr(ref, name)), rel(getattr(h, name), getattr(ref, name))
            print(f"{case['name']} fp32 {name}: oracle error {e_cpu:.3e}, hip error {e_hip:.3e}")
            assert e_cpu > 0
            assert e_hip <= 4 * e_cpu

    check(cpu.run(), hip.run(), case["run"], ("traces",))
    gkw = dict(wrt_density=density, illumination=True)
    check(cpu.gradient(case["obs"], **gkw), hip.gradient(case["obs"], segment=3, **gkw), case["grad"],
          ("grad_speed2", "grad_wavelet") + (("grad_density",) if density else ()))
    check(cpu.born(case["ds"], case["dw"]), hip.born(case["ds"], case["dw"]), case["born"],
          ("dtraces", "du_final", "traces"))
