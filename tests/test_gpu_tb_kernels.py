"""Isolated temporal-blocking sweeps (k_tb3, k_tbn) vs the plain-PyTorch oracles, bit for bit.

One launch on random fields: C = u^m and D = u^{m+1} (tb3: C errors only, D, E) over boxes
that cross 64-lane k tiles, TJ-row j tiles and short i chunks, with a Dirichlet column inside
the ring (C = 0 outside ``cdom``). The shapes and fields live in tests/sweep_cases.py, shared with
the CPU tests that examine them.

What is compared, and how (``bits.assert_same_bits``: equal integer views, so no tolerance at all):

* exact form, fp64 and fp32: the stored layers against ``reference.chained_layers`` /
  ``chained_delta_layers`` evaluated in the grid's own type. The one operation the kernels do
  differently, the constant division ``div_const``, equals true division on the numerators of these
  cases (tests/test_sweep_bits_cpu.py checks every one of them against ``bits.division_range``).
* --math fma, fp64 and fp32: the stored layers against ``reference.chained_layers_fma`` /
  ``chained_delta_layers_fma``, written out from csrc/stencil_math.hpp's FMA section with a correctly
  rounded software ``fma`` (tests/test_fma_oracle_cpu.py checks it against rationals, against the
  OpenMP oracle, and shows that an unfused, a swapped or a folded chain changes bits on these inputs).
* the fused error keys of every layer: ``max |u - f|`` equal to the oracle's in the grid's type in both
  math modes; ``max |u - f| / |f|`` equal to ``reference.max_errors`` (exact form: RelArg is the maximum
  of the rounded quotients) and to ``reference.rel_key_fma`` (--math fma: RelMax's chain of reciprocal
  tables, product, maximum and ``1 / |ct|``; the device's reciprocals are correctly rounded quotients, so
  the chain is reproducible and the comparison is for equality as well).
* nodes outside the boxes stay untouched.

The end-to-end solves are covered against the OpenMP oracle in test_gpu_solver.py.
"""
import pytest
import torch

import sweep_cases as sc
from bits import assert_same_bits
from sweep_cases import CASES, COEFS, CT, TBN_CASES

pytestmark = pytest.mark.gpu

DEV = "cuda"
COEF = sc.H2
_rand, _tables, _mask, _sl = sc.rand, sc.tables, sc.mask, sc.sl


def _check(got, exp, dtype):
    """Stored values: the same bits in either type."""
    assert got.dtype == dtype
    assert_same_bits(got, exp)


def _err_nodes(vals, box, ei, tx, ty, tz, ct, dtype):
    """(u, f, table slices) on the error nodes of ``box``, f in the grid's type."""
    from wave3d.ops import reference

    i0, i1, j0, j1, k0, k1 = box
    t = (tx[ei[0]:ei[1] + 1], ty[j0:j1 + 1], tz[k0:k1 + 1])
    f = reference.analytic(*t, sc.cast(ct, dtype))
    return vals[ei[0] - i0:ei[1] - i0 + 1], f, t


def _check_err(err, vals, box, ei, tx, ty, tz, ct, dtype):
    """Exact form: both keys equal the oracle's, formed in the grid's type (``d = u - f``, ``|d| / |f|``,
    NaN-ignoring maxima)."""
    from wave3d.ops import kernels, reference

    u, f, _ = _err_nodes(vals, box, ei, tx, ty, tz, ct, dtype)
    assert u.dtype == dtype and f.dtype == dtype
    ea, er = reference.max_errors(u, f)
    (ga, gr, bad), = kernels.decode_err(err)
    assert ga == ea and gr == er, (ga, ea, gr, er)
    assert not bad


def _check_err_fma(err, vals, box, ei, tx, ty, tz, ct, dtype):
    """--math fma: the abs key equals ``max |u - f|`` of the oracle's values; the rel key equals RelMax's
    chain, reproduced operation for operation (``reference.rel_key_fma``)."""
    from wave3d.ops import kernels, reference

    u, f, t = _err_nodes(vals, box, ei, tx, ty, tz, ct, dtype)
    assert u.dtype == dtype and f.dtype == dtype
    ea, _ = reference.max_errors(u, f)
    er = reference.rel_key_fma(u - f, *t, ct)
    (ga, gr, bad), = kernels.decode_err(err)
    assert ga == ea and gr == er, (ga, ea, gr, er)
    assert not bad


def _h(dtype):
    return {k: sc.cast(v, dtype) for k, v in COEF.items()}


def _untouched(outs, fills, boxes, G):
    touched = torch.zeros(outs[0].shape, dtype=torch.bool)
    for b in boxes:
        touched[_sl(b, G)] = True
    for g, v in zip(outs, fills):
        assert bool((g[~touched] == v).all())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("rows,waves", [(2, 8), (2, 4), (1, 16), (1, 8)])
@pytest.mark.parametrize("case", [0, 2, 3])
def test_tb3_sweep_matches_reference(C, dtype, first, rows, waves, case):
    from wave3d.ops import kernels, reference

    (X, Y, Z), boxes, cdom, chunk = CASES[case]
    G = 3
    shape = (X + 2 * G, Y + 2 * G, Z + 2 * G)
    A, B = _rand(shape, dtype, 4), _rand(shape, dtype, 5)
    tx, ty, tz = _tables(max(shape), dtype, 6)
    dD, dE = torch.full(shape, -7.0, dtype=dtype, device=DEV), torch.full(shape, -9.0, dtype=dtype, device=DEV)
    errs = [kernels.new_err(1) for _ in range(3)]
    ei = (min(b[0] for b in boxes), max(b[1] for b in boxes))
    co = [(*COEF.values(), COEFS[q], CT[q]) for q in range(3)]
    kernels.tb3_sweep(A.to(DEV), B.to(DEV), dD, dE, boxes, first=first, cdom=cdom, err_i=ei,
                      tx=tx.to(DEV), ty=ty.to(DEV), tz=tz.to(DEV), coefs_c=co[0], coefs_d=co[1],
                      coefs_e=co[2], err_c=errs[0], err_d=errs[1], err_e=errs[2], rows=rows,
                      waves=waves, chunk=chunk)
    torch.cuda.synchronize()
    cast = lambda v: torch.tensor(v, dtype=dtype).item()  # noqa: E731
    h = {k: cast(v) for k, v in COEF.items()}
    Cf, Df, Ef = reference.chained_layers(A, B, 3, first=first, mask=_mask(shape, G, cdom),
                                          coefs=[cast(c) for c in COEFS], **h)
    gD, gE = dD.cpu(), dE.cpu()
    for b in boxes:
        s = _sl(b, G)
        _check(gD[s], Df[s], dtype)
        _check(gE[s], Ef[s], dtype)
    if len(boxes) == 1:
        s = _sl(boxes[0], G)
        for err, vals, q in ((errs[0], Cf[s], 0), (errs[1], gD[s], 1), (errs[2], gE[s], 2)):
            _check_err(err, vals, boxes[0], ei, tx, ty, tz, CT[q], dtype)


def test_tb_sweep_shape_checks(C):
    from wave3d.ops import kernels

    G = 3
    shape = (7 + 2 * G, 6 + 2 * G, 7 + 2 * G)
    u = torch.zeros(shape, dtype=torch.float64, device=DEV)
    t = torch.zeros(max(shape), dtype=torch.float64, device=DEV)
    e = kernels.new_err(1)
    kw = dict(first=False, cdom=(1, 7, 1, 6, 1, 7), err_i=(1, 7), tx=t, ty=t, tz=t,
              coefs_c=(1, 1, 1, 1, 1), coefs_d=(1, 1, 1, 1, 1), coefs_e=(1, 1, 1, 1, 1), err_c=e, err_d=e, err_e=e)
    with pytest.raises(ValueError):
        kernels.tb3_sweep(u, u, u, u, (0, 7, 1, 6, 1, 7), **kw)   # i outside the owned region
    with pytest.raises(ValueError):
        kernels.tb3_sweep(u, u, u, u, (1, 7, 1, 6, 1, 7), rows=3, waves=4, **kw)  # no such tile


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("rows,waves", [(2, 8), (1, 16), (1, 8)])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_tb3_fma_sweep_close_to_reference(C, dtype, first, rows, waves, case):
    """--math fma: the same three-layer sweep with coef/h^2 folded into FMAs. The FMA form is a fixed
    sequence of rounded operations, so D, E and the error keys of all three layers equal the FMA-form
    oracle bit for bit, in fp64 and fp32 (the name is from the time this was a comparison within
    1e-12 / 2e-5 of the exact-form oracle)."""
    from wave3d.ops import kernels, reference

    inp = sc.tb3_fma_inputs(case, dtype, first)
    boxes, shape, G, ei = inp["boxes"], inp["shape"], inp["G"], inp["ei"]
    tx, ty, tz = inp["tx"], inp["ty"], inp["tz"]
    dD, dE = torch.full(shape, -7.0, dtype=dtype, device=DEV), torch.full(shape, -9.0, dtype=dtype, device=DEV)
    errs = [kernels.new_err(1) for _ in range(3)]
    co = [(*COEF.values(), inp["coefs"][q], CT[q]) for q in range(3)]
    kernels.tb3_sweep(inp["A"].to(DEV), inp["B"].to(DEV), dD, dE, boxes, first=first, cdom=inp["cdom"], err_i=ei,
                      tx=tx.to(DEV), ty=ty.to(DEV), tz=tz.to(DEV), coefs_c=co[0], coefs_d=co[1],
                      coefs_e=co[2], err_c=errs[0], err_d=errs[1], err_e=errs[2], rows=rows,
                      waves=waves, chunk=inp["chunk"], fma=True)
    torch.cuda.synchronize()
    Cf, Df, Ef = reference.chained_layers_fma(inp["A"], inp["B"], 3, first=first, mask=inp["mask"],
                                              coefs=inp["coefs"], **COEF)
    gD, gE = dD.cpu(), dE.cpu()
    for b in boxes:
        s = _sl(b, G)
        _check(gD[s], Df[s], dtype)
        _check(gE[s], Ef[s], dtype)
    _untouched((gD, gE), (-7.0, -9.0), boxes, G)
    if len(boxes) == 1:  # the fused error keys of all three layers
        s = _sl(boxes[0], G)
        for err, vals, q in ((errs[0], Cf[s], 0), (errs[1], Df[s], 1), (errs[2], Ef[s], 2)):
            _check_err_fma(err, vals, boxes[0], ei, tx, ty, tz, CT[q], dtype)


@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("case", range(len(TBN_CASES)))
def test_tbn_depth3_bitwise_equal_to_tb3(C, first, fma, case):
    """The generic deep sweep at depth 3 is the three-layer sweep: k_tbn<3> and k_tb3 on the
    same fields give bitwise identical D, E and error keys (fp64, exact and --math fma)."""
    from wave3d.ops import kernels

    (X, Y, Z), boxes, cdom, chunk = TBN_CASES[case]
    G, dtype = 4, torch.float64
    shape = (X + 2 * G, Y + 2 * G, Z + 2 * G)
    A, B = _rand(shape, dtype, 14).to(DEV), _rand(shape, dtype, 15).to(DEV)
    tx, ty, tz = (t.to(DEV) for t in _tables(max(shape), dtype, 16))
    ei = (min(b[0] for b in boxes), max(b[1] for b in boxes))
    coefs = (COEFS[0] if first or not fma else COEFS[1], COEFS[1], COEFS[2] if not fma else COEFS[1])
    co = [(*COEF.values(), coefs[q], CT[q]) for q in range(3)]
    outs = []
    for tbn in (False, True):
        dD, dE = (torch.full(shape, v, dtype=dtype, device=DEV) for v in (-7.0, -9.0))
        errs = [kernels.new_err(1) for _ in range(3)]
        kw = dict(first=first, cdom=cdom, err_i=ei, tx=tx, ty=ty, tz=tz, rows=2, waves=8, chunk=chunk,
                  ghost=G, fma=fma)
        if tbn:
            kernels.tbn_sweep(A, B, dD, dE, boxes, depth=3, coefs=co, errs=errs, **kw)
        else:
            kernels.tb3_sweep(A, B, dD, dE, boxes, coefs_c=co[0], coefs_d=co[1], coefs_e=co[2], err_c=errs[0],
                              err_d=errs[1], err_e=errs[2], **kw)
        torch.cuda.synchronize()
        outs.append((dD.cpu(), dE.cpu(), [e.cpu() for e in errs]))
    (d0, e0, k0), (d1, e1, k1) = outs
    assert torch.equal(d0, d1) and torch.equal(e0, e1)
    for a, b in zip(k0, k1):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("case", range(len(TBN_CASES)))
def test_tbn_depth4_sweep_matches_reference(C, dtype, first, case):
    """Four layers per sweep (k_tbn<4>, exact arithmetic): the stored layers u^{m+2}, u^{m+3} and
    the error keys of all four layers against the chained plain-PyTorch oracle — bitwise in fp64;
    nodes outside the boxes untouched."""
    from wave3d.ops import kernels, reference

    (X, Y, Z), boxes, cdom, chunk = TBN_CASES[case]
    G = 4
    shape = (X + 2 * G, Y + 2 * G, Z + 2 * G)
    A, B = _rand(shape, dtype, 24), _rand(shape, dtype, 25)
    tx, ty, tz = _tables(max(shape), dtype, 26)
    c4 = (3.1e-4, 2.9e-4, 2.7e-4, 2.6e-4)
    ct4 = (-0.83, 0.47, 0.21, -0.66)
    dO0, dO1 = (torch.full(shape, v, dtype=dtype, device=DEV) for v in (-7.0, -9.0))
    errs = [kernels.new_err(1) for _ in range(4)]
    ei = (min(b[0] for b in boxes), max(b[1] for b in boxes))
    co = [(*COEF.values(), c4[q], ct4[q]) for q in range(4)]
    kernels.tbn_sweep(A.to(DEV), B.to(DEV), dO0, dO1, boxes, depth=4, first=first, cdom=cdom, err_i=ei,
                      tx=tx.to(DEV), ty=ty.to(DEV), tz=tz.to(DEV), coefs=co, errs=errs, chunk=chunk)
    torch.cuda.synchronize()
    cast = lambda v: torch.tensor(v, dtype=dtype).item()  # noqa: E731
    h = {k: cast(v) for k, v in COEF.items()}
    L = reference.chained_layers(A, B, 4, first=first, mask=_mask(shape, G, cdom), coefs=[cast(c) for c in c4], **h)
    g0, g1 = dO0.cpu(), dO1.cpu()
    touched = torch.zeros(shape, dtype=torch.bool)
    for b in boxes:
        s = _sl(b, G)
        _check(g0[s], L[2][s], dtype)
        _check(g1[s], L[3][s], dtype)
        touched[s] = True
    assert bool((g0[~touched] == -7.0).all()) and bool((g1[~touched] == -9.0).all())
    if len(boxes) == 1:
        s = _sl(boxes[0], G)
        for q in range(4):
            _check_err(errs[q], L[q][s], boxes[0], ei, tx, ty, tz, ct4[q], dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("case", range(len(TBN_CASES)))
def test_tbn_depth4_delta_matches_reference(C, dtype, first, case):
    """The increment form on four-layer sweeps (k_tbn DELTA, exact arithmetic; fp64 since round 6):
    O0 = d of the last layer, O1 = u of the last layer, and the error keys of all four layers,
    against the chained plain-PyTorch increment-form oracle; nodes outside the boxes untouched."""
    from wave3d.ops import kernels, reference

    (X, Y, Z), boxes, cdom, chunk = TBN_CASES[case]
    G = 4
    shape = (X + 2 * G, Y + 2 * G, Z + 2 * G)
    A = _rand(shape, dtype, 31)
    Dm1 = (_rand(shape, dtype, 32) - 0.5) * 1e-3  # increments are small
    tx, ty, tz = _tables(max(shape), dtype, 33)
    c4 = (3.1e-4, 2.9e-4, 2.7e-4, 2.6e-4)
    ct4 = (-0.83, 0.47, 0.21, -0.66)
    dO0, dO1 = (torch.full(shape, v, dtype=dtype, device=DEV) for v in (-7.0, -9.0))
    errs = [kernels.new_err(1) for _ in range(4)]
    ei = (min(b[0] for b in boxes), max(b[1] for b in boxes))
    co = [(*COEF.values(), c4[q], ct4[q]) for q in range(4)]
    kernels.tbn_sweep(A.to(DEV), Dm1.to(DEV), dO0, dO1, boxes, depth=4, first=first, cdom=cdom, err_i=ei,
                      tx=tx.to(DEV), ty=ty.to(DEV), tz=tz.to(DEV), coefs=co, errs=errs, chunk=chunk, delta=True)
    torch.cuda.synchronize()
    cast = lambda v: torch.tensor(v, dtype=dtype).item()  # noqa: E731
    h = {k: cast(v) for k, v in COEF.items()}
    L, dl = reference.chained_delta_layers(A, Dm1, 4, first=first, mask=_mask(shape, G, cdom),
                                           coefs=[cast(c) for c in c4], **h)
    g0, g1 = dO0.cpu(), dO1.cpu()
    touched = torch.zeros(shape, dtype=torch.bool)
    for b in boxes:
        s = _sl(b, G)
        _check(g0[s], dl[s], dtype)
        _check(g1[s], L[3][s], dtype)
        touched[s] = True
    assert bool((g0[~touched] == -7.0).all()) and bool((g1[~touched] == -9.0).all())
    if len(boxes) == 1:
        s = _sl(boxes[0], G)
        for q in range(4):
            _check_err(errs[q], L[q][s], boxes[0], ei, tx, ty, tz, ct4[q], dtype)


def _run_tbn_fma(inp, depth, first, dtype, delta=False):
    """One k_tbn ``fma=True`` launch on ``inp``; returns (O0, O1 on the host, error slots)."""
    from wave3d.ops import kernels

    shape = inp["shape"]
    dO0, dO1 = (torch.full(shape, v, dtype=dtype, device=DEV) for v in (-7.0, -9.0))
    errs = [kernels.new_err(1) for _ in range(depth)]
    co = [(*COEF.values(), inp["coefs"][q], inp["cts"][q]) for q in range(depth)]
    kernels.tbn_sweep(inp["A"].to(DEV), inp["B"].to(DEV), dO0, dO1, inp["boxes"], depth=depth, first=first,
                      cdom=inp["cdom"], err_i=inp["ei"], tx=inp["tx"].to(DEV), ty=inp["ty"].to(DEV),
                      tz=inp["tz"].to(DEV), coefs=co, errs=errs, chunk=inp["chunk"], fma=True, delta=delta,
                      ghost=inp["G"])
    torch.cuda.synchronize()
    return dO0.cpu(), dO1.cpu(), errs


def _check_tbn_fma(inp, layers, stored, got, errs, dtype):
    boxes, G = inp["boxes"], inp["G"]
    for b in boxes:
        s = _sl(b, G)
        _check(got[0][s], stored[0][s], dtype)
        _check(got[1][s], stored[1][s], dtype)
    _untouched(got, (-7.0, -9.0), boxes, G)
    if len(boxes) == 1:
        s = _sl(boxes[0], G)
        for q, L in enumerate(layers):
            _check_err_fma(errs[q], L[s], boxes[0], inp["ei"], inp["tx"], inp["ty"], inp["tz"], inp["cts"][q], dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("case", range(len(TBN_CASES)))
def test_tbn_depth4_fma_close_to_reference(C, dtype, first, case):
    """The --math fma four-layer sweep (k_tbn<double, 4, fma> is the bench kernel): the stored layers
    u^{m+2}, u^{m+3} and the error keys of all four layers equal the FMA-form oracle bit for bit, fp64
    and fp32; nodes outside the boxes untouched (the name is from the time this was a comparison
    within 1e-12 / 4e-5 of the exact-form oracle)."""
    from wave3d.ops import reference

    inp = sc.tbn4_fma_inputs(case, dtype, first)
    g0, g1, errs = _run_tbn_fma(inp, 4, first, dtype)
    L = reference.chained_layers_fma(inp["A"], inp["B"], 4, first=first, mask=inp["mask"], coefs=inp["coefs"], **COEF)
    _check_tbn_fma(inp, L, (L[2], L[3]), (g0, g1), errs, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("case", range(len(TBN_CASES)))
def test_tbn_depth3_fma_matches_reference(C, dtype, first, case):
    """k_tbn at depth 3 with ``fma=True`` against the FMA-form oracle itself (the test above compares it
    with k_tb3 only, and only in fp64): stored layers and error keys bit for bit."""
    from wave3d.ops import reference

    inp = sc.tbn3_fma_inputs(case, dtype, first)
    g0, g1, errs = _run_tbn_fma(inp, 3, first, dtype)
    L = reference.chained_layers_fma(inp["A"], inp["B"], 3, first=first, mask=inp["mask"], coefs=inp["coefs"], **COEF)
    _check_tbn_fma(inp, L, (L[1], L[2]), (g0, g1), errs, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("case", range(len(TBN_CASES)))
def test_tbn_depth4_delta_fma_matches_reference(C, dtype, first, case):
    """The FMA increment form at depth 4 (``delta=True, fma=True``; in fp32 the ``--scheme delta --math fma``
    auto kernel): O0 = d of the last layer, O1 = u of the last layer and the error keys of all four
    layers equal the FMA increment-form oracle bit for bit. Both types have the instantiation."""
    from wave3d.ops import reference

    assert C.tbn_delta_supported(4, 2, 8, True, dtype == torch.float32)
    inp = sc.tbn4_delta_fma_inputs(case, dtype, first)
    g0, g1, errs = _run_tbn_fma(inp, 4, first, dtype, delta=True)
    L, dl = reference.chained_delta_layers_fma(inp["A"], inp["B"], 4, first=first, mask=inp["mask"],
                                               coefs=inp["coefs"], **COEF)
    _check_tbn_fma(inp, L, (dl, L[3]), (g0, g1), errs, dtype)
