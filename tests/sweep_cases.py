"""The shapes, boxes and fields of the isolated-sweep kernel tests (tests/test_gpu_tb_kernels.py), in one
place so that the CPU tests (tests/test_fma_oracle_cpu.py, tests/test_sweep_bits_cpu.py) examine the very
inputs the GPU tests launch.

A plain helper module (``import sweep_cases``): no fixtures, no pytest hooks.
"""
import torch

H2 = dict(hx2=0.011, hy2=0.013, hz2=0.017)
CT = (-0.83, 0.47, 0.21)
COEFS = (3.1e-4, 2.9e-4, 2.7e-4)
C4 = (3.1e-4, 2.9e-4, 2.7e-4, 2.6e-4)
CT4 = (-0.83, 0.47, 0.21, -0.66)

CASES = [
    # (X, Y, Z), boxes, cdom (j/k part used), chunk
    ((9, 40, 131), [(2, 8, 3, 37, 60, 130)], (1, 9, 1, 40, 1, 130), 3),
    ((9, 40, 131), [(1, 9, 1, 40, 1, 130)], (1, 9, 1, 40, 1, 130), 0),
    ((12, 21, 70), [(1, 2, 1, 21, 1, 69), (3, 12, 5, 9, 2, 66)], (1, 12, 1, 21, 1, 69), 4),
    ((7, 9, 11), [(1, 7, 2, 8, 2, 10)], (1, 7, 2, 8, 2, 10), 0),
]

TBN_CASES = [
    # (X, Y, Z), boxes, cdom, chunk — as CASES, with a box that starts past the first plane and
    # chunks short enough that every work item runs its prologue / epilogue planes
    ((11, 40, 131), [(2, 10, 3, 37, 60, 130)], (1, 11, 1, 40, 1, 130), 3),
    ((11, 40, 131), [(1, 11, 1, 40, 1, 130)], (1, 11, 1, 40, 1, 130), 0),
    ((13, 21, 70), [(1, 2, 1, 21, 1, 69), (3, 13, 5, 9, 2, 66)], (1, 13, 1, 21, 1, 69), 5),
    ((9, 9, 11), [(1, 9, 2, 8, 2, 10)], (1, 9, 2, 8, 2, 10), 0),
    # one- and two-plane work items: shorter than the steady window's start (only checked planes)
    ((11, 40, 131), [(2, 10, 3, 37, 60, 130)], (1, 11, 1, 40, 1, 130), 1),
    ((11, 40, 131), [(1, 11, 1, 40, 1, 130)], (1, 11, 1, 40, 1, 130), 2),
]


def rand(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64).to(dtype)


def tables(n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1).to(dtype) for _ in range(3)]


def mask(shape, G, cdom):
    """j/k inside cdom (logical) as a tensor-index mask."""
    m = torch.zeros(shape, dtype=torch.bool)
    _, _, j0, j1, k0, k1 = cdom
    m[:, j0 + G - 1:j1 + G, k0 + G - 1:k1 + G] = True
    return m


def sl(box, G):
    i0, i1, j0, j1, k0, k1 = box
    o = G - 1
    return (slice(i0 + o, i1 + o + 1), slice(j0 + o, j1 + o + 1), slice(k0 + o, k1 + o + 1))


def cast(v, dtype) -> float:
    return torch.tensor(v, dtype=dtype).item()


def _inputs(cases, case, G, dtype, seeds, coefs, cts, B=None):
    (X, Y, Z), boxes, cdom, chunk = cases[case]
    shape = (X + 2 * G, Y + 2 * G, Z + 2 * G)
    A = rand(shape, dtype, seeds[0])
    B = rand(shape, dtype, seeds[1]) if B is None else B(shape)
    tx, ty, tz = tables(max(shape), dtype, seeds[2])
    return dict(A=A, B=B, tx=tx, ty=ty, tz=tz, boxes=boxes, cdom=cdom, chunk=chunk, G=G, shape=shape,
                mask=mask(shape, G, cdom), coefs=list(coefs), cts=list(cts),
                ei=(min(b[0] for b in boxes), max(b[1] for b in boxes)))


def exact_inputs(kind, case, dtype):
    """The fields of the exact-form tests: "tb3" (k_tb3, G = 3), "tbn4" (k_tbn depth 4), "tbn4_delta"
    (B = d^{m-1}: small increments)."""
    if kind == "tb3":
        return _inputs(CASES, case, 3, dtype, (4, 5, 6), COEFS, CT)
    if kind == "tbn4":
        return _inputs(TBN_CASES, case, 4, dtype, (24, 25, 26), C4, CT4)
    if kind == "tbn4_delta":
        return _inputs(TBN_CASES, case, 4, dtype, (31, 32, 33), C4, CT4,
                       B=lambda shape: (rand(shape, dtype, 32) - 0.5) * 1e-3)
    raise ValueError(kind)


def tb3_fma_inputs(case, dtype, first):
    """k_tb3 ``fma=True``: one coefficient triple for the non-first layers (as in a solve, where every
    layer but the Taylor start has the same a2 tau^2)."""
    coefs = (COEFS[0] if first else COEFS[1], COEFS[1], COEFS[1])
    return _inputs(CASES, case, 3, dtype, (4, 5, 6), coefs, CT)


def tbn3_fma_inputs(case, dtype, first):
    coefs = (COEFS[0] if first else COEFS[1], COEFS[1], COEFS[1])
    return _inputs(TBN_CASES, case, 4, dtype, (14, 15, 16), coefs, CT)


def tbn4_fma_inputs(case, dtype, first):
    c = 2.9e-4
    return _inputs(TBN_CASES, case, 4, dtype, (34, 35, 36), (3.1e-4 if first else c, c, c, c), CT4)


def tbn4_delta_fma_inputs(case, dtype, first):
    c = 2.9e-4
    return _inputs(TBN_CASES, case, 4, dtype, (44, 45, 46), (3.1e-4 if first else c, c, c, c), CT4,
                   B=lambda shape: (rand(shape, dtype, 45) - 0.5) * 1e-3)


# ---- the single-step kernel tests (tests/test_gpu_kernels.py) ---------------------------------------

STEP_CASES = [
    ((13, 21, 70), (1, 11, 1, 19, 1, 68), 0),      # whole owned region
    ((13, 21, 70), (2, 10, 3, 17, 2, 66), 3),      # interior sub-box, short chunks
    ((9, 40, 131), (1, 7, 5, 33, 60, 129), 2),     # k box across 64-lane tiles
    ((6, 7, 9), (1, 4, 1, 5, 1, 7), 0),            # tiny
]
STEP_COEFS = (0.011, 0.013, 0.017, 3.1e-4, -0.83)  # hx2, hy2, hz2, coef, ct


def step_inputs(shape, dtype):
    """(u1, u2, tx, ty, tz) of the step tests on the host (the CPU tests examine the same fields)."""
    g = lambda seed: torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype)  # noqa: E731
    t = torch.Generator().manual_seed(103)
    return (g(1), g(2), *[(torch.rand(n, generator=t, dtype=torch.float64) * 2 - 1).to(dtype) for n in shape])
