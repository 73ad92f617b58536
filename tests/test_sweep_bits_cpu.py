"""Why the exact-form sweep and step kernels can be compared bit for bit in fp32 (no GPU needed).

The kernels divide by h^2 with ``div_const`` (csrc/stencil_math.hpp), the oracle with true division;
the two agree on ``bits.division_range`` and may differ by one unit in the last place below it. So every
Laplacian numerator that the GPU tests meet, in every chained layer of every case of
tests/test_gpu_tb_kernels.py and tests/test_gpu_kernels.py, must be zero or inside that range. And the
bitwise comparison must see the change a tolerance let through on the medium kernels: ``coef * lap``
contracted into the following add.
"""
import pytest
import torch

import sweep_cases as sc
from bits import numerators

DTYPES = [torch.float64, torch.float32]
H2 = tuple(sc.H2.values())


def _all_in_range(u, dtype):
    nx, ny, nz = u.shape
    _, ok = numerators(u, (1, nx - 2, 1, ny - 2, 1, nz - 2), [sc.cast(h, dtype) for h in H2])
    return bool(ok.all())


def _layers(kind, case, dtype, first):
    """The fields whose Laplacian a sweep takes: the input and every layer but the last."""
    from wave3d.ops import reference

    inp = sc.exact_inputs(kind, case, dtype)
    n = 3 if kind == "tb3" else 4
    kw = dict(first=first, mask=inp["mask"], coefs=[sc.cast(c, dtype) for c in inp["coefs"]],
              **{k: sc.cast(v, dtype) for k, v in sc.H2.items()})
    if kind == "tbn4_delta":
        L, _ = reference.chained_delta_layers(inp["A"], inp["B"], n, **kw)
    else:
        L = reference.chained_layers(inp["A"], inp["B"], n, **kw)
    return inp, [inp["A"]] + L[:-1], L


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("kind", ["tb3", "tbn4", "tbn4_delta"])
def test_sweep_numerators_inside_division_range(kind, dtype, first):
    """Every numerator of every chained layer, on every interior node of the grid (a superset of the
    nodes the kernels compute), is zero or inside ``division_range`` for the three h^2."""
    cases = sc.CASES if kind == "tb3" else sc.TBN_CASES
    for case in range(len(cases)):
        _, fields, _ = _layers(kind, case, dtype, first)
        for q, u in enumerate(fields):
            assert _all_in_range(u, dtype), f"{kind} case {case} layer {q}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_step_numerators_inside_division_range(dtype):
    for shape, _, _ in sc.STEP_CASES:
        assert _all_in_range(sc.step_inputs(shape, dtype)[0], dtype), shape


def _contracted(A, B, n, first, m, h, coefs, delta):
    """The exact-form chain with ``coef * lap`` contracted into the add that follows it (what a compiler
    does to ``x + coef * lap`` with contraction on): the one deviation this test plants."""
    from wave3d.ops import reference

    inner = (slice(1, -1),) * 3
    zero = torch.zeros((), dtype=A.dtype)
    mi = m.clone()
    mi[0], mi[-1], mi[:, 0], mi[:, -1], mi[:, :, 0], mi[:, :, -1] = (False,) * 6
    out, u, prev = [], A, B
    for q in range(n):
        lap = reference.laplace7(u, *h)
        c = torch.tensor(coefs[q], dtype=A.dtype)
        v = torch.zeros_like(A)
        if delta:
            d = torch.zeros_like(A)
            d[inner] = c * lap if (first and q == 0) else reference.fma(c, lap, prev[inner])
            d = torch.where(mi, d, zero)
            v = torch.where(mi, u + d, zero)
            u, prev = v, d
        else:
            base = u[inner] if (first and q == 0) else 2 * u[inner] - prev[inner]
            v[inner] = torch.where(mi[inner], reference.fma(c, lap, base), zero)
            u, prev = v, u
        out.append(v)
    return out, prev


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["tb3", "tbn4", "tbn4_delta"])
def test_contracted_multiply_add_changes_bits(kind, dtype):
    """Contracting ``coef * lap`` into the add changes stored values inside the boxes of every case and
    stays inside the tolerance the fp32 comparison used to have (4e-6), so only the bitwise comparison
    sees it. Changed stored values, summed over the cases (leapfrog sweeps; measured on the CPU):
    tb3 fp64 20,010 of 141,568, fp32 19,730; tbn4 fp64 66,475 of 332,340, fp32 66,482; tbn4_delta
    (d and u of the last layer) fp64 86,103, fp32 83,965. The floor asserted per case is 5 %."""
    cases = sc.CASES if kind == "tb3" else sc.TBN_CASES
    total_changed = 0
    for case in range(len(cases)):
        inp, _, L = _layers(kind, case, dtype, False)
        n = 3 if kind == "tb3" else 4
        h = [sc.cast(v, dtype) for v in H2]
        Lc, dc = _contracted(inp["A"], inp["B"], n, False, inp["mask"], h, [sc.cast(c, dtype) for c in inp["coefs"]],
                             kind == "tbn4_delta")
        if kind == "tbn4_delta":
            from wave3d.ops import reference

            _, d = reference.chained_delta_layers(inp["A"], inp["B"], n, first=False, mask=inp["mask"],
                                                  coefs=[sc.cast(c, dtype) for c in inp["coefs"]],
                                                  **{k: sc.cast(v, dtype) for k, v in sc.H2.items()})
            pairs = [(d, dc), (L[-1], Lc[-1])]
        else:
            pairs = [(L[-2], Lc[-2]), (L[-1], Lc[-1])]
        changed = compared = 0
        for b in inp["boxes"]:
            s = sc.sl(b, inp["G"])
            for e, v in pairs:
                changed += int((e[s] != v[s]).sum())
                compared += e[s].numel()
                torch.testing.assert_close(v[s], e[s], rtol=4e-6, atol=4e-6)
        assert changed > compared // 20, f"{kind} case {case}: {changed} of {compared}"
        total_changed += changed
    print(f"{kind} {dtype}: {total_changed} stored values change")  # (shown with pytest -s)
