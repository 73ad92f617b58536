"""Absorbing sponge on the GPU: the TAPER instantiations of k_march_m (csrc/hip_medium.hip) against
the PyTorch oracle (ops/reference.py step_medium / solve_medium with ``taper``), against the undamped
kernels (tables of ones) and against the exact decay law of a constant power-of-two taper.

A single step must be bitwise equal in fp64 and in fp32; chained fp32 steps of a solve within the bounds of
the undamped medium tests.
"""
import math

import pytest
import torch

from bits import assert_same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _tapers(shape, dtype, seed=11):
    """Random factors in (0.5, 1] per axis, storage indexing (CPU)."""
    g = torch.Generator().manual_seed(seed)
    return tuple((1.0 - 0.5 * torch.rand(n, generator=g, dtype=torch.float64)).to(dtype) for n in shape)


def _expected(u1, u2, m, box, first, taper):
    from test_gpu_medium import H2, _cast
    from wave3d.ops import reference

    dt = u1.dtype
    return reference.step_medium(u1, u2, m, box, first=first, hx2=_cast(H2[0], dt), hy2=_cast(H2[1], dt),
                                 hz2=_cast(H2[2], dt), taper=taper)


def _cases():
    from test_gpu_medium import CASES

    return CASES


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("case", range(4))
def test_tapered_step_matches_reference(C, dtype, first, case):
    from test_gpu_medium import H2, _inputs
    from wave3d.ops import kernels, reference

    shape, box, chunk = _cases()[case]
    u1, u2, m = _inputs(shape, dtype)
    taper = _tapers(shape, dtype)
    assert all(0.5 < float(t.min()) and float(t.max()) <= 1 for t in taper)
    u = torch.full(shape, -7.0, dtype=dtype, device=DEV)
    stat = kernels.new_err(1)
    ei = (box[0] + 1, box[1])  # exclude the first box plane from the statistic
    kernels.step_medium(u1.to(DEV), u2.to(DEV), m.to(DEV), u, box, first=first, h2=H2, stat=stat, stat_i=ei,
                        chunk=chunk, taper=tuple(t.to(DEV) for t in taper))
    torch.cuda.synchronize()
    exp = _expected(u1, u2, m, box, first, taper)
    i0, i1, j0, j1, k0, k1 = box
    got = u[i0:i1 + 1, j0:j1 + 1, k0:k1 + 1].cpu()
    if dtype == torch.float64:
        assert torch.equal(got, exp)
    assert_same_bits(got, exp)
    # the taper acts: the undamped values differ
    assert not torch.equal(exp, _expected(u1, u2, m, box, first, None))
    mask = torch.ones(shape, dtype=torch.bool)
    mask[i0:i1 + 1, j0:j1 + 1, k0:k1 + 1] = False
    assert bool((u.cpu()[mask] == -7.0).all())
    # slot 0: max |v| over the planes ei; slot 1 untouched; flag clear
    want = reference.max_abs_field(exp[ei[0] - i0:].double())
    (ga, gr, bad), = kernels.decode_err(stat)
    assert ga == want
    assert gr == -100.0 and not bad


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("first", [False, True])
def test_ones_equal_the_untapered_kernel_and_variants_agree(C, dtype, first):
    from test_gpu_medium import H2, _inputs
    from wave3d.ops import kernels

    shape, box, chunk = _cases()[2]
    u1, u2, m = (t.to(DEV) for t in _inputs(shape, dtype))

    def run(variant, taper):
        u = torch.full(shape, -7.0, dtype=dtype, device=DEV)
        st = kernels.new_err(1)
        kernels.step_medium(u1, u2, m, u, box, first=first, h2=H2, stat=st, stat_i=(1, 7), chunk=chunk,
                            variant=variant, taper=taper)
        return u, kernels.decode_err(st)

    ones = tuple(torch.ones(n, dtype=dtype, device=DEV) for n in shape)
    rnd = tuple(t.to(DEV) for t in _tapers(shape, dtype))
    variants = (None, "nt", "plain", "r2", "r2nt")
    base = run(None, None)
    same = [run(v, ones) for v in variants]
    damped = [run(v, rnd) for v in variants]
    torch.cuda.synchronize()
    for u, st in same:
        assert torch.equal(u, base[0]) and st == base[1]
    assert not torch.equal(damped[0][0], base[0])
    for u, st in damped[1:]:
        assert torch.equal(u, damped[0][0]) and st == damped[0][1]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("first", [False, True])
def test_tapered_step_on_padded_views_with_fused_wrap(C, dtype, first):
    from test_gpu_medium import H2, _inputs
    from wave3d.ops import kernels

    N = 9
    shape = (N + 3, N + 1, 70)  # solve_medium's storage in x and y, k across two 64-lane tiles
    cpu = _inputs(shape, dtype)
    taper = _tapers(shape, dtype)
    views = [kernels.alloc_level(*shape, dtype) for _ in range(4)]
    assert views[0].stride(1) > shape[2]  # padded pitch
    for v, t in zip(views, cpu):
        v.copy_(t)
    views[3].fill_(-7.0)
    box = (1, N + 1, 1, shape[1] - 2, 1, shape[2] - 2)
    st = kernels.new_err(1)
    kernels.step_medium(*views, box, first=first, h2=H2, stat=st, stat_i=(1, N + 1), wrap=(N, 0, 2, N + 2),
                        taper=tuple(t.to(DEV) for t in taper))
    torch.cuda.synchronize()
    u = views[3].cpu()
    exp = _expected(*cpu, box, first, taper)
    own = u[1:N + 2, 1:-1, 1:-1]
    if dtype == torch.float64:
        assert torch.equal(own, exp)
    assert_same_bits(own, exp)
    # ghost planes: the fused wrap stored the tapered values of their source planes
    assert torch.equal(u[0, 1:-1, 1:-1], u[N, 1:-1, 1:-1]) and torch.equal(u[N + 2, 1:-1, 1:-1], u[2, 1:-1, 1:-1])
    assert float(u[N, 1:-1, 1:-1].abs().sum()) > 0
    # faces untouched, padding still zero
    assert bool((u[:, 0] == -7).all() and (u[:, -1] == -7).all() and (u[:, :, 0] == -7).all()
                and (u[:, :, -1] == -7).all())
    for v in views[:3]:
        base = v._base
        inside = torch.zeros(base.shape, dtype=torch.bool, device=DEV)
        inside.as_strided(v.shape, v.stride(), v.storage_offset()).fill_(True)
        assert bool((base[~inside] == 0).all())


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_exact_decay_law_end_to_end(C, dtype):
    import wave3d
    from test_sponge_cpu import decay_case

    prob, u0, tapers = decay_case(dtype)
    base = wave3d.MediumSolver(prob, "hip", u0=u0).run()
    assert float(base.u_final.abs().max()) > 0.1
    for taper, g in tapers:
        res = wave3d.MediumSolver(prob, "hip", u0=u0, taper=taper).run()
        assert torch.equal(res.u_final, base.u_final * g ** 20)  # 2^-20, 2^-80
        assert res.max_abs_u == [v * g ** n for n, v in enumerate(base.max_abs_u)]


def _hetero(backend, dtype):
    import wave3d
    from test_medium_cpu import A, B, K, N, hetero_case

    speed2, w = hetero_case()
    prob = wave3d.MediumProblem(N, speed2, T=1.0, timesteps=K, dtype=dtype)
    return wave3d.MediumSolver(prob, backend, sources=[A], wavelet=w, taper=wave3d.sponge_taper(prob, 4),
                               receivers=[B, (0, 6, 7), (N, 6, 7), (8, 8, 8)]).run()


def test_end_to_end_sponge_fp64(C):
    ref, got = _hetero("cpu", "fp64"), _hetero("hip", "fp64")
    assert float(ref.traces.abs().max()) > 1e-3
    assert torch.equal(got.traces, ref.traces)
    assert torch.equal(got.u_final, ref.u_final)
    assert got.max_abs_u == ref.max_abs_u
    assert not got.aborted


def test_end_to_end_sponge_fp32(C):
    ref, got = _hetero("cpu", "fp32"), _hetero("hip", "fp32")
    print("fp32 max |trace dev|", float((got.traces - ref.traces).abs().max()),
          "max |field dev|", float((got.u_final - ref.u_final).abs().max()), "max |u|", max(ref.max_abs_u))
    torch.testing.assert_close(got.traces, ref.traces, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(got.u_final, ref.u_final, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(torch.tensor(got.max_abs_u), torch.tensor(ref.max_abs_u), rtol=2e-5, atol=2e-5)


# measured once with the fp64 CPU oracle (bitwise the fp64 GPU run): e(sponge) / e(no sponge) =
# 0.0419517 (fp32 oracle: 0.0419514), the undamped echo 0.227 of the direct arrival's peak; the bound
# is 1.5 x that (profiles/medium_sponge.txt)
ABSORB_GPU_RATIO = 0.0419517
ABSORB_GPU_BOUND = 1.5 * ABSORB_GPU_RATIO


@pytest.fixture(scope="module")
def absorb_truth_trace(C):
    from test_sponge_cpu import absorb_truth

    return absorb_truth(64, 190, 0.15, 14, "fp64", "hip")  # the box of 128 cells


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_sponge_absorbs_the_wall_echo_on_the_gpu(C, absorb_truth_trace, dtype):
    from test_sponge_cpu import absorb_ratio, absorb_traces

    N, K, f0, off = 64, 190, 0.15, 14
    assert 2 * N - off > K / 2
    plain, sponge = absorb_traces(N, K, f0, off, dtype, "hip", width=16, sigma_max=0.35)
    ratio, echo = absorb_ratio(plain, sponge, absorb_truth_trace)
    print(f"absorption N={N} {dtype}: e(sponge)/e(no sponge) = {ratio:.6g}, undamped echo / peak = {echo:.6g}")
    assert echo >= 0.1
    assert ratio <= ABSORB_GPU_BOUND


def test_taper_is_validated_before_launch(C):
    from test_gpu_medium import H2, _inputs
    from wave3d.ops import kernels

    shape, box, _ = _cases()[3]
    dt = torch.float64
    u1, u2, m = (t.to(DEV) for t in _inputs(shape, dt))
    u = torch.full(shape, -7.0, dtype=dt, device=DEV)
    stat = kernels.new_err(1)
    good = tuple(torch.ones(n, dtype=dt, device=DEV) for n in shape)

    def swap(q, t):
        return tuple(t if a == q else g for a, g in enumerate(good))

    bad = [
        swap(0, torch.ones(shape[0] + 1, dtype=dt, device=DEV)),            # too long
        swap(1, torch.ones(shape[1] - 1, dtype=dt, device=DEV)),            # too short
        swap(2, torch.ones(shape[2], dtype=torch.float32, device=DEV)),     # wrong dtype
        swap(1, torch.ones(shape[1], dtype=dt)),                            # on the CPU
        swap(2, torch.ones(2 * shape[2], dtype=dt, device=DEV)[::2]),       # not contiguous
        swap(0, torch.ones(shape[0], 1, dtype=dt, device=DEV)),             # not 1-D
        good[:2],
    ]
    for taper in bad:
        with pytest.raises(ValueError, match="taper"):
            kernels.step_medium(u1, u2, m, u, box, first=False, h2=H2, stat=stat, stat_i=(1, 4), taper=taper)
    torch.cuda.synchronize()
    assert bool((u == -7.0).all())  # nothing was launched
    kernels.step_medium(u1, u2, m, u, box, first=False, h2=H2, stat=stat, stat_i=(1, 4), taper=good)
    torch.cuda.synchronize()
    assert not bool((u == -7.0).all())
