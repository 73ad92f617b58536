"""Off-grid sources and receivers of the medium solver on the CPU: the interpolation tables
(ops/reference.py interp_tables), the on-node identity with the node lists, the adjoint against
torch.autograd and finite differences, the Born / gradient dot-product identity, sub-cell consistency
and reciprocity of the 8-point windowed sinc, and the argument checks of MediumSolver.
"""
import pytest
import torch

from test_medium_born_cpu import EPS, MEASURED
from test_medium_gradient_cpu import N, _case

K = 16
SOURCES = [(0, 4, 6), (6, 3, 5)]                       # one on the periodic plane, one interior
RECEIVERS = [(N, 7, 3), (4, 5, 5), (3, 0, 4), (7, 6, 2)]  # plane N, interior, a face: all distinct
SOURCE_POS = torch.tensor([[0.3, 4.2, 6.7], [6.5, 0.4, 5.1], [9.6, 8.0, 9.7]], dtype=torch.float64)
RECEIVER_POS = torch.tensor([[4.0, 5.0, 5.0], [3.3, 0.4, 4.2], [7.1, 6.2, 9.7], [0.3, 8.5, 8.5], [9.6, 3.3, 5.1],
                             [5.2, 5.2, 5.2], [6.7, 5.2, 5.2]], dtype=torch.float64)


def _f64(nodes):
    return torch.tensor(nodes, dtype=torch.float64)


def _wavelets(S, K, tau):
    import wave3d

    cols = [wave3d.ricker(3.0, 0.3, K, tau), -0.5 * wave3d.ricker(2.0, 0.2, K, tau),
            0.7 * wave3d.ricker(2.5, 0.25, K, tau)]
    return torch.stack(cols[:S], 1)


# ---- tables ------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["sinc8", "linear"])
def test_on_node_position_is_a_kronecker_delta(kind):
    import wave3d

    ix, iy, iz, wx, wy, wz = wave3d.interp_tables((5.0, 3.0, 16.0), 16, kind, ghost=2)
    for idx, w, node in ((ix, wx, 5 + 2), (iy, wy, 3), (iz, wz, 16)):
        assert idx.dtype == torch.int64 and w.dtype == torch.float64 and idx.shape == w.shape == (8,)
        assert int(idx[3]) == node
    assert wx.tolist() == wy.tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    assert not bool(wz.any())  # on the Dirichlet face: the node carries no weight
    # x = N is the periodic plane 0
    assert int(wave3d.interp_tables((16.0, 3.0, 3.0), 16)[0][3]) == 0 + 1


def test_weights_sum_to_one():
    import wave3d

    for f in (0.25, 0.5, 0.9):
        p = (8 + f,) * 3
        lin = wave3d.interp_tables(p, 16, "linear")[3:]
        sinc = wave3d.interp_tables(p, 16, "sinc8")[3:]
        print(f"fraction {f}: sinc8 weights sum to {float(sinc[0].sum())!r}")
        for w in lin:
            assert abs(float(w.sum()) - 1) <= 4 * EPS and int((w != 0).sum()) == 2
        for w in sinc:
            assert abs(float(w.sum()) - 1) <= 1e-3 and int((w != 0).sum()) == 8
    from wave3d.ops import reference

    x = torch.tensor([-4.0, -3.5, 0.0, 1.0, 3.999, 4.0, 4.5], dtype=torch.float64)
    w = reference.interp_weight(x)
    assert w[0] == 0 and w[2] == 1 and w[3] == 0 and w[5] == 0 and w[6] == 0 and w[1] != 0 and w[4] != 0


def test_fold_and_wrap_indices():
    import wave3d

    n = 16
    ix, iy, iz, wx, wy, wz = wave3d.interp_tables((0.3, 0.4, n - 0.3), n, "sinc8", ghost=1)
    # the same fractions away from the edges; the offsets node - p round differently there (p is larger), by
    # at most 2 ulp(16) = 7e-15, and |w'| < 4: the weights agree to 1e-13
    plain = wave3d.interp_tables((8.3, 8.4, 8.7), n, "sinc8")[3:]

    def same(a, b):
        return bool(((a - b).abs() <= 1e-13).all())

    # xi = 0.3: nodes -3 .. 4 modulo N, plus the ghost
    assert ix.tolist() == [v % n + 1 for v in range(-3, 5)] and same(wx, plain[0])
    # eta = 0.4: nodes -3, -2, -1 fold onto 3, 2, 1 with the weight negated, node 0 carries none
    assert iy.tolist() == [3, 2, 1, 0, 1, 2, 3, 4]
    assert same(wy[:3], -plain[1][:3]) and wy[3] == 0 and same(wy[4:], plain[1][4:])
    # zeta = N - 0.3: nodes N-4 .. N+3; N+1 .. N+3 fold onto N-1 .. N-3 negated, node N carries none
    assert iz.tolist() == [n - 4, n - 3, n - 2, n - 1, n, n - 1, n - 2, n - 3]
    assert same(wz[:4], plain[2][:4]) and wz[4] == 0 and same(wz[5:], -plain[2][5:])
    assert float(plain[1][:3].abs().min()) > 1e-3 and float(plain[2][5:].abs().min()) > 1e-3
    # xi = N - 0.4: nodes N-4 .. N+3 wrap onto N-4 .. N-1, 0 .. 3
    ix = wave3d.interp_tables((n - 0.4, 5.0, 5.0), n, ghost=4)[0]
    assert ix.tolist() == [v % n + 4 for v in range(n - 4, n + 4)]


def test_row_list_layout():
    from wave3d.ops import reference

    n = 16
    pos = torch.tensor([[0.3, 0.4, 5.5], [0.3, 0.4, 5.5], [8.0, 8.0, 8.0]], dtype=torch.float64)
    rows = reference.point_rows(pos, n, torch.float64, ghost=1)
    nodes = rows.nodes.tolist()
    assert nodes[:rows.unique] == sorted(nodes[:rows.unique]) and len(set(map(tuple, nodes))) == len(nodes)
    assert all(1 <= j <= n - 1 and 1 <= k <= n - 1 for _, j, k in nodes)
    twins = [nd for nd in nodes if nd[0] == n + 1]
    assert nodes[rows.unique:] == twins == [[n + 1, j, k] for i, j, k in nodes if i == 1]
    ptr, col = rows.rowptr.tolist(), rows.col.tolist()
    assert ptr[0] == 0 and ptr[-1] == rows.entries and all(a <= b for a, b in zip(ptr, ptr[1:]))
    for r in range(len(rows)):  # entries sorted by point; two equal points give equal pairs of entries
        assert col[ptr[r]:ptr[r + 1]] == sorted(col[ptr[r]:ptr[r + 1]])
    r = nodes.index([9, 8, 8])
    assert col[ptr[r]:ptr[r + 1]] == [2] and rows.w[ptr[r]] == 1
    r = nodes.index([2, 1, 5])  # eta = 0.4: slots 2 (node -1, negated) and 4 (node 1) fold onto j = 1: separate entries
    assert col[ptr[r]:ptr[r + 1]] == [0, 0, 1, 1]
    ix, iy, iz, wx, wy, wz = reference.interp_tables(pos[0], n)
    assert int(ix[4]) == 2 and int(iy[2]) == int(iy[4]) == 1 and int(iz[3]) == 5
    assert rows.w[ptr[r]:ptr[r] + 2].tolist() == [float((wx[4] * wy[2]) * wz[3]), float((wx[4] * wy[4]) * wz[3])]
    assert not bool((rows.w == 0).any())


# ---- on-node identity ---------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("sponge", [False, True])
def test_integer_positions_are_the_node_lists(sponge, dtype):
    """== on everything but two places: the source-node entries of grad_speed2, whose time sum runs in
    the adjoint loop's order instead of the host's sum(0) (rtol 1e-13 in fp64), and, with a sponge,
    grad_wavelet, whose 1 / G is the product of three per-axis quotients instead of one."""
    import wave3d

    speed2, pert, _, _ = _case()
    prob = wave3d.MediumProblem(N, speed2, timesteps=K, dtype=dtype)
    w = _wavelets(2, K, prob.tau)
    taper = wave3d.sponge_taper(prob, 3) if sponge else None
    a = wave3d.MediumSolver(prob, "cpu", sources=SOURCES, receivers=RECEIVERS, wavelet=w, taper=taper)
    b = wave3d.MediumSolver(prob, "cpu", source_positions=_f64(SOURCES), receiver_positions=_f64(RECEIVERS),
                            wavelet=w, taper=taper)
    ra, rb = a.run(), b.run()
    assert float(ra.traces.abs().max()) > 0
    assert torch.equal(ra.traces, rb.traces) and torch.equal(ra.u_final, rb.u_final)
    obs = wave3d.MediumSolver(wave3d.MediumProblem(N, pert, timesteps=K, dtype=dtype), "cpu", sources=SOURCES,
                              receivers=RECEIVERS, wavelet=w, taper=taper).run().traces
    ga, gb = a.gradient(obs), b.gradient(obs)
    assert ga.misfit == gb.misfit > 0 and torch.equal(ga.traces, gb.traces)
    at_source = torch.zeros((N + 1,) * 3, dtype=torch.bool)
    for i, j, k in SOURCES:
        at_source[i, j, k] = True
        if i in (0, N):
            at_source[N - i, j, k] = True
    assert torch.equal(ga.grad_speed2[~at_source], gb.grad_speed2[~at_source])
    assert float(ga.grad_speed2[at_source].abs().min()) > 0
    if dtype == "fp64":
        torch.testing.assert_close(gb.grad_speed2[at_source], ga.grad_speed2[at_source], rtol=1e-13, atol=0)
    if sponge:  # three quotients and two products against one quotient: a few roundings of the working dtype
        torch.testing.assert_close(gb.grad_wavelet, ga.grad_wavelet, rtol=1e-13 if dtype == "fp64" else 16 * 2.0 ** -24,
                                   atol=0)
    else:
        assert torch.equal(ga.grad_wavelet, gb.grad_wavelet)
    ds, dw = 0.1 * speed2, 0.3 * w.flip(1)
    ba, bb = a.born(ds, dw), b.born(ds, dw)
    assert float(ba.dtraces.abs().max()) > 0
    assert torch.equal(ba.dtraces, bb.dtraces) and torch.equal(ba.traces, bb.traces)
    assert torch.equal(ba.du_final, bb.du_final)
    assert rb.extra["interp"] == "sinc8" and "interp" not in ra.extra


# ---- gradient -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def grad_case():
    """Off-grid sources and receivers with a sponge: autograd's and the adjoint's gradients."""
    import wave3d
    from wave3d.ops import reference

    speed2, pert, _, taper = _case()
    w = _wavelets(3, K, 1.0 / K)
    kw = dict(source_positions=SOURCE_POS, receiver_positions=RECEIVER_POS, taper=taper)
    observed = reference.solve_medium(N, K, pert, wavelet=w, **kw)[0]
    s = speed2.clone().requires_grad_(True)
    wl = w.clone().requires_grad_(True)
    tr = reference.forward_medium_autograd(N, K, s, wavelet=wl, **kw)
    assert torch.equal(tr.detach(), reference.solve_medium(N, K, speed2, wavelet=w, **kw)[0])
    J = 0.5 * ((tr[1:] - observed[1:]) ** 2).sum()
    gs, gw = torch.autograd.grad(J, (s, wl))
    hand = reference.gradient_medium(N, K, speed2, observed, wavelet=w, **kw)
    prob = wave3d.MediumProblem(N, speed2, timesteps=K)
    return dict(speed2=speed2, w=w, kw=kw, observed=observed, J=J.item(), gs=gs, gw=gw, hand=hand, prob=prob)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_adjoint_matches_autograd_with_positions(grad_case):
    J, grad, gw, _ = grad_case["hand"]
    gs = grad_case["gs"]
    fold = gs.clone()  # autograd treats planes 0 and N as two leaves: the unique node gets both
    fold[0] = gs[0] + gs[N]
    fold[N] = fold[0]
    assert float(fold.abs().max()) > 0 and float(grad_case["gw"].abs().min(0).values.max()) > 0
    e_s, e_w = _rel(grad, fold), _rel(gw, grad_case["gw"])
    print("relative max-norm difference: speed2", e_s, "wavelet", e_w, "misfit", abs(J - grad_case["J"]) / J)
    # the bounds of tests/test_medium_gradient_cpu.py
    assert e_s <= 4.02e-14
    assert e_w <= 5.66e-14
    assert abs(J - grad_case["J"]) <= 1e-14 * grad_case["J"]


def test_grad_wavelet_by_central_differences(grad_case):
    """The traces are linear in the wavelet, so J is quadratic in it and the central difference is exact
    but for the cancellation in J+ - J-: two sums of ~100 squares, each within ~1e-14 J of its value,
    divided by 2 eps |dJ|. With eps = 1e-2 and J / |dJ| < 10 (asserted) that stays below 1e-10."""
    import wave3d

    prob, w, kw, obs = grad_case["prob"], grad_case["w"], grad_case["kw"], grad_case["observed"]
    g = torch.Generator().manual_seed(3)
    dw = torch.rand(w.shape, generator=g, dtype=torch.float64) - 0.5
    eps = 1e-2
    Jp, Jm = (wave3d.MediumSolver(prob, "cpu", wavelet=w + s * eps * dw, **kw).gradient(obs).misfit for s in (1, -1))
    fd = (Jp - Jm) / (2 * eps)
    want = float((grad_case["hand"][2] * dw).sum())
    print("central difference", fd, "gradient", want, "relative", abs(fd - want) / abs(want))
    assert grad_case["J"] < 10 * abs(want)
    assert abs(fd - want) <= 1e-10 * abs(want)


# ---- adjoint identity ---------------------------------------------------------------------

@pytest.mark.parametrize("order,K_,density,sponge", [(2, 24, True, False), (8, 32, False, True)],
                         ids=["order2-density", "order8-sponge"])
def test_born_gradient_dot_product_identity(order, K_, density, sponge):
    """<J d, r> against <d, J^T r> with off-grid sources and receivers. The bound is that of the dot test of
    tests/test_medium_born_cpu.py, 100 times a measured difference capped at 1e-9; these cases have other
    geometries than that file's, so its largest measured value stands in for a per-case one."""
    import wave3d

    speed2, _, _, _ = _case()
    g = torch.Generator().manual_seed(17)

    def field(lo, hi):
        v = lo + (hi - lo) * torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64)
        v[N] = v[0]
        return v

    prob = wave3d.MediumProblem(N, speed2, timesteps=K_, space_order=order, density=field(1, 2) if density else None)
    w = _wavelets(3, K_, prob.tau)
    sol = wave3d.MediumSolver(prob, "cpu", source_positions=SOURCE_POS, receiver_positions=RECEIVER_POS, wavelet=w,
                              taper=wave3d.sponge_taper(prob, 3) if sponge else None)
    ds, dw = field(-0.3, 0.3), torch.rand(w.shape, generator=g, dtype=torch.float64) - 0.5
    b = sol.born(ds, dw)
    r = torch.rand(b.traces.shape, generator=g, dtype=torch.float64) - 0.5
    gr = sol.gradient(b.traces - r)
    lhs = float((b.dtraces[1:] * r[1:]).sum())
    rhs = float((gr.grad_speed2[:N] * ds[:N]).sum() + (gr.grad_wavelet * dw).sum())
    e = abs(lhs - rhs) / abs(lhs)
    print(f"<J d, r> = {lhs!r}, <d, J^T r> = {rhs!r}, relative difference {e:.3e}")
    assert abs(lhs) > 1e-3 * float(b.dtraces[1:].norm() * r[1:].norm())
    assert e <= min(100 * max(max(v[2] for v in MEASURED.values()), EPS), 1e-9)
    # gauss_newton() is born() followed by gradient(traces - dtraces): the residuals are dtraces
    h = sol.gauss_newton(ds, dw)
    assert torch.equal(h.extra["dtraces"], b.dtraces) and h.misfit == pytest.approx(float(0.5 * (b.dtraces[1:] ** 2).sum()), rel=1e-9)
    assert float(h.grad_speed2.abs().max()) > 0 and h.extra["interp"] == "sinc8"


# ---- sub-cell consistency and reciprocity --------------------------------------------------

@pytest.fixture(scope="module")
def uniform():
    """N = 32, speed2 = 1, T = 1.2, K = 80, one Ricker source (f0 = 1, t0 = 0.35): trace(source, receiver, interp)."""
    import wave3d

    prob = wave3d.MediumProblem(32, 1.0, T=1.2, timesteps=80)
    w = wave3d.ricker(1.0, 0.35, 80, prob.tau)[:, None]

    def trace(src, rec, interp="sinc8"):
        sol = wave3d.MediumSolver(prob, "cpu", source_positions=[src], receiver_positions=[rec], wavelet=w,
                                  interp=interp)
        return sol.run().traces[:, 0]

    return trace


def test_sub_cell_consistency(uniform):
    """Source (16, 16, 12) and receiver (16, 16, 22.5) against both moved by (0.3, -0.4, 0.2), which changes
    nothing in the continuum. Measured relative L2 change of the trace: 0.02336 with sinc8 (0.1335 with
    linear, so sinc8's is 0.175 of it); asserted at twice the measured value, the margin for the
    implementation's rounding choices, and at one third of linear's."""
    a, b = (16.0, 16.0, 12.0), (16.0, 16.0, 22.5)
    a2, b2 = (16.3, 15.6, 12.2), (16.3, 15.6, 22.7)
    change = {}
    for interp in ("sinc8", "linear"):
        t0, t1 = uniform(a, b, interp), uniform(a2, b2, interp)
        assert float(t0.abs().max()) > 0
        change[interp] = float((t0 - t1).norm() / t0.norm())
    print("relative L2 change of the trace:", change)
    assert change["sinc8"] <= 2 * 0.02336
    assert change["sinc8"] <= change["linear"] / 3


def test_reciprocity(uniform):
    """Uniform medium: source z = 12, receiver z = 22.5 against source z = 12.5, receiver z = 23: the two
    supports are mirror images, the traces equal to rounding (where nearest-node rounding gives 11
    against 10 cells)."""
    t0 = uniform((16.0, 16.0, 12.0), (16.0, 16.0, 22.5))
    t1 = uniform((16.0, 16.0, 12.5), (16.0, 16.0, 23.0))
    e = float((t0 - t1).abs().max() / t0.abs().max())
    print("reciprocity: relative max difference", e)
    assert float(t0.abs().max()) > 0
    assert e <= 1e-12


# ---- argument checks ------------------------------------------------------------------------

def test_position_argument_checks():
    import wave3d

    prob = wave3d.MediumProblem(N, 1.0, timesteps=K)
    w = _wavelets(1, K, prob.tau)
    S = wave3d.MediumSolver
    for backend in ("cpu", "hip"):  # refused before any device is touched
        with pytest.raises(ValueError, match="not both"):
            S(prob, backend, sources=[(1, 2, 3)], source_positions=[(1.5, 2, 3)], wavelet=w)
        with pytest.raises(ValueError, match="not both"):
            S(prob, backend, receivers=[(1, 2, 3)], receiver_positions=[(1.5, 2, 3)])
        for bad in ((3.0, 0.0, 4.0), (3.0, 4.0, float(N)), (3.0, -0.5, 4.0), (N + 0.5, 4.0, 4.0)):
            with pytest.raises(ValueError, match="face|outside"):
                S(prob, backend, source_positions=[bad], wavelet=w)
        S(prob, backend, receiver_positions=[(3.0, 0.0, float(N))])  # a receiver may sit on a face
        with pytest.raises(ValueError, match="outside"):
            S(prob, backend, receiver_positions=[(3.0, N + 0.1, 4.0)])
        with pytest.raises(ValueError, match="N >= 8"):
            S(wave3d.MediumProblem(6, 1.0, timesteps=K), backend, receiver_positions=[(3.0, 3.0, 3.0)])
        with pytest.raises(ValueError, match="interp"):
            S(prob, backend, receiver_positions=[(3.0, 3.0, 3.0)], interp="cubic")
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match="finite"):
                S(prob, backend, source_positions=[(3.0, bad, 3.0)], wavelet=w)
            with pytest.raises(ValueError, match="finite"):
                S(prob, backend, receiver_positions=[(bad, 3.0, 3.0)])
        with pytest.raises(ValueError, match="shape"):
            S(prob, backend, receiver_positions=[(3.0, 3.0)])
        with pytest.raises(ValueError, match="wavelet"):
            S(prob, backend, source_positions=[(3.0, 3.0, 3.0), (3.0, 3.0, 3.0)], wavelet=w)
        # two sources at one position are fine: their rows have two entries
        S(prob, backend, source_positions=[(3.5, 3.0, 3.0), (3.5, 3.0, 3.0)], wavelet=torch.cat([w, w], 1))


def test_grid_position():
    import wave3d

    prob = wave3d.MediumProblem(16, 1.0, Lx=2.0, Ly=4.0, Lz=8.0, timesteps=40)
    p = wave3d.grid_position(prob, [[1.0, 1.0, 1.0], [0.25, 4.0, 0.0]])
    assert p.dtype == torch.float64 and p.tolist() == [[8.0, 4.0, 2.0], [2.0, 16.0, 0.0]]
    assert wave3d.grid_position(prob, (2.0, 2.0, 2.0)).tolist() == [16.0, 8.0, 4.0]
    with pytest.raises(ValueError):
        wave3d.grid_position(prob, [1.0, 2.0])
