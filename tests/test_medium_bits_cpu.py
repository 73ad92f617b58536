"""What the bit-for-bit GPU step tests rest on, checked on the CPU: their inputs keep every numerator of
the Laplacian zero or inside the range of the kernels' constant division (bits.division_range), and the
comparison would see a kernel that contracts one product of the update into an FMA."""
import pytest
import torch

from bits import numerators
from test_gpu_medium import CASES, H2, _cast, _inputs, _rand
from test_gpu_medium_order import CASES as STAR_CASES

DTYPES = (torch.float64, torch.float32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_inputs_of_the_step_tests_keep_every_numerator_in_range(dtype):
    h2 = [_cast(v, dtype) for v in H2]
    for shape, box, _ in CASES:
        u1, _, _ = _inputs(shape, dtype)
        assert bool(numerators(u1, box, h2)[1].all())
        b = _rand(shape, dtype, 4, 0.3, 2.0)  # test_gpu_medium_density._buoyancy
        assert bool(numerators(u1, box, h2, buoyancy=b)[1].all())
        db = _rand(shape, dtype, 8, -1.0, 1.0)  # test_gpu_medium_born_density._step_inputs
        assert bool(numerators(u1, box, h2, buoyancy=db)[1].all())
        a, v = _rand(shape, dtype, 1), _rand(shape, dtype, 2)  # test_gpu_medium_density_gradient._inputs
        assert bool(numerators(a, box, h2, correlate=v)[1].all())
    for order in (4, 8):
        for shape, box, _, mirror in STAR_CASES:
            u1, _, _ = _inputs(shape, dtype)
            assert bool(numerators(u1, box, h2, order, mirror)[1].all())


def test_a_contracted_product_changes_fp32_bits_on_the_step_tests_data():
    """(2 u1 - u2) + m lap with the product contracted into the add (one rounding, formed here in fp64:
    the product of two fp32 values is exact there) differs from the oracle's two roundings at 940 of the
    11 * 19 * 68 = 14212 box nodes of the first case of test_gpu_medium.py: a kernel that contracted it
    would fail the bit-for-bit comparison, where the earlier 2e-6 tolerance let it pass."""
    from wave3d.ops import reference

    dt = torch.float32
    shape, box, _ = CASES[0]
    u1, u2, m = _inputs(shape, dt)
    h2 = [_cast(v, dt) for v in H2]
    i0, i1, j0, j1, k0, k1 = box
    sl = (slice(i0, i1 + 1), slice(j0, j1 + 1), slice(k0, k1 + 1))
    exp = reference.step_medium(u1, u2, m, box, first=False, hx2=h2[0], hy2=h2[1], hz2=h2[2])
    lap = reference._lap_box(u1, box, *h2, 2, None)
    fused = ((2 * u1[sl] - u2[sl]).double() + m[sl].double() * lap.double()).to(dt)
    n = int((fused != exp).sum())
    print("contracted m lap: differing nodes", n, "of", exp.numel())
    torch.testing.assert_close(fused, exp, rtol=2e-6, atol=2e-6)  # the old bound does not see it
    assert n >= exp.numel() // 100  # measured: 940
