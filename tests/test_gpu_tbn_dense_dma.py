"""The fp64 deep sweeps' dense LDS-DMA staging (k_tbn: DenseDma / dma_dense2 in csrc/hip_tbn.hip).

The A / B frames of a plane are filled by 16-byte chunks that run across the frame's row ends:
two pieces per wave and fill, each lane with its own source offset, a chunk that starts in a row's
pad fetching the cell before the next row's first frame column. A misplaced chunk puts a wrong
value into a frame cell, so every check here is bitwise:

  * one sweep through ``ops.kernels.tbn_sweep`` on random finite fields, exact math, against
    ``reference.chained_layers``: the stored layers and the error keys of every layer, ``first`` on
    and off, depth 4 and 3 — one tile clipped on both sides; a grid whose row length 16 + Z + G is a
    multiple of 16 with the box reaching Y and Z (the plane's last value is then the node
    (jmax, kmax), the one cell a chunk may lose to the descriptor's range); three k-tiles by three
    j-tiles with one-plane work items (checked planes only) and with the steady loop;
  * whole solves through ``WaveSolver`` against the OpenMP oracle, the per-layer max_abs tables bit
    for bit in ``math="exact"`` and ``"fma"``, K = 9 (two sweeps and a tail layer): one rank, 2x2x2
    and 1x2x2 simulated ranks (the y/z ghosts then hold the neighbours' data, so a misplaced ring
    cell changes the table).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
H2 = dict(hx2=0.011, hy2=0.013, hz2=0.017)
COEFS = (3.1e-4, 2.9e-4, 2.7e-4, 2.6e-4)
CT = (-0.83, 0.47, 0.21, -0.66)
G = 4

SWEEPS = {
    # (X, Y, Z), box, cdom, chunk
    "one_tile_clipped": ((9, 9, 11), (1, 9, 2, 8, 2, 10), (1, 9, 2, 8, 2, 10), 0),
    "row_multiple_of_16": ((11, 21, 60), (1, 11, 1, 21, 1, 60), (1, 11, 1, 21, 1, 60), 0),
    "tiles_3x3_checked": ((11, 40, 131), (1, 11, 1, 40, 1, 130), (1, 11, 1, 40, 1, 130), 1),
    "tiles_3x3_steady": ((11, 40, 131), (1, 11, 1, 40, 1, 130), (1, 11, 1, 40, 1, 130), 0),
}


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64)


@pytest.fixture(scope="module")
def fields():
    """per case: A, B, the analytic tables and the Dirichlet mask (computed once, never changed)"""
    out = {}
    for n, (name, ((X, Y, Z), _, cdom, _)) in enumerate(SWEEPS.items()):
        shape = (X + 2 * G, Y + 2 * G, Z + 2 * G)
        g = torch.Generator().manual_seed(300 + n)
        tabs = [torch.rand(max(shape), generator=g, dtype=torch.float64) * 2 - 1 for _ in range(3)]
        mask = torch.zeros(shape, dtype=torch.bool)
        _, _, j0, j1, k0, k1 = cdom
        mask[:, j0 + G - 1:j1 + G, k0 + G - 1:k1 + G] = True
        out[name] = (_rand(shape, 100 + n), _rand(shape, 200 + n), tabs, mask)
    return out


@pytest.fixture(scope="module")
def oracle(fields):
    """reference.chained_layers per (case, first): four layers (depth 3 takes the first three)"""
    from wave3d.ops import reference

    out = {}
    for name, (A, B, _, mask) in fields.items():
        for first in (False, True):
            out[name, first] = reference.chained_layers(A, B, 4, first=first, mask=mask, coefs=list(COEFS), **H2)
    return out


@pytest.mark.parametrize("depth", [4, 3])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("name", list(SWEEPS))
def test_dense_dma_sweep_bitwise(C, fields, oracle, name, first, depth):
    from wave3d.ops import kernels, reference

    (X, Y, Z), box, cdom, chunk = SWEEPS[name]
    A, B, (tx, ty, tz), _ = fields[name]
    L = oracle[name, first]
    shape = A.shape
    O0, O1 = (torch.full(shape, v, dtype=torch.float64, device=DEV) for v in (-7.0, -9.0))
    errs = [kernels.new_err(1) for _ in range(depth)]
    co = [(*H2.values(), COEFS[q], CT[q]) for q in range(depth)]
    ei = (box[0], box[1])
    kernels.tbn_sweep(A.to(DEV), B.to(DEV), O0, O1, [box], depth=depth, first=first, cdom=cdom, err_i=ei,
                      tx=tx.to(DEV), ty=ty.to(DEV), tz=tz.to(DEV), coefs=co, errs=errs, chunk=chunk, ghost=G)
    torch.cuda.synchronize()
    i0, i1, j0, j1, k0, k1 = box
    o = G - 1
    s = (slice(i0 + o, i1 + o + 1), slice(j0 + o, j1 + o + 1), slice(k0 + o, k1 + o + 1))
    g0, g1 = O0.cpu(), O1.cpu()
    assert torch.equal(g0[s], L[depth - 2][s])
    assert torch.equal(g1[s], L[depth - 1][s])
    touched = torch.zeros(shape, dtype=torch.bool)
    touched[s] = True
    assert bool((g0[~touched] == -7.0).all()) and bool((g1[~touched] == -9.0).all())
    for q in range(depth):
        f = reference.analytic(tx[i0:i1 + 1], ty[j0:j1 + 1], tz[k0:k1 + 1], CT[q])
        ea, er = reference.max_errors(L[q][s], f)
        (ga, gr, bad), = kernels.decode_err(errs[q])
        assert (ga, gr) == (ea, er), (q, ga, ea, gr, er)
        assert not bad


SOLVES = {
    "n20_one_rank": (20, {}),
    "n48_2x2x2": (48, dict(ranks=8, dims=[2, 2, 2])),
    "n70_1x2x2": (70, dict(ranks=4, dims=[1, 2, 2])),
}


@pytest.mark.parametrize("math_", ["exact", "fma"])
@pytest.mark.parametrize("name", list(SOLVES))
def test_dense_dma_solve_bitwise(C, name, math_):
    import wave3d

    N, kw = SOLVES[name]
    p = wave3d.WaveProblem(N, timesteps=9, math=math_)
    base = wave3d.WaveSolver(p, "cpu", threads=8).run()
    r = wave3d.WaveSolver(p, "hip", kernel="tb4", **kw).run()
    assert r.kernel == "tb4" and r.extra["math"] == math_
    assert r.max_abs == base.max_abs
