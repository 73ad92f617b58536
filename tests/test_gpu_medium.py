"""Variable-speed medium on the GPU: k_march_m / k_inject / k_record (csrc/hip_medium.hip) against
the plain-PyTorch oracle (ops/reference.py step_medium, solve_medium) and against k_march.

A single step must be *bitwise* equal in fp64 and in fp32 (both sides round every operation in the
same order, no FMA contraction; the inputs keep every numerator of the Laplacian inside the range of
the kernels' constant division, tests/test_div_const_cpu.py); chained fp32 steps of a solve within the
bounds the constant-speed kernels' tests use.
"""
import math

import pytest
import torch

from bits import assert_same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
H2 = (0.011, 0.013, 0.017)
CASES = [
    ((13, 21, 70), (1, 11, 1, 19, 1, 68), 0),      # whole owned region
    ((13, 21, 70), (2, 10, 3, 17, 2, 66), 3),      # interior sub-box, short chunks
    ((9, 40, 131), (1, 7, 5, 33, 60, 129), 2),     # k box across 64-lane tiles
    ((6, 7, 9), (1, 4, 1, 5, 1, 7), 0),            # tiny
]


def _rand(shape, dtype, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64)).to(dtype)


def _inputs(shape, dtype):
    """CPU tensors u1, u2, m (m in [1e-4, 6e-4])."""
    return _rand(shape, dtype, 1), _rand(shape, dtype, 2), _rand(shape, dtype, 3, 1e-4, 6e-4)


def _cast(v, dtype):
    return torch.tensor(v, dtype=dtype).item()


def _expected(u1, u2, m, box, first):
    from wave3d.ops import reference

    dt = u1.dtype
    return reference.step_medium(u1, u2, m, box, first=first, hx2=_cast(H2[0], dt), hy2=_cast(H2[1], dt),
                                 hz2=_cast(H2[2], dt))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("shape,box,chunk", CASES)
def test_step_medium_matches_reference(C, dtype, first, shape, box, chunk):
    from wave3d.ops import kernels, reference

    u1, u2, m = _inputs(shape, dtype)
    u = torch.full(shape, -7.0, dtype=dtype, device=DEV)
    stat = kernels.new_err(1)
    ei = (box[0] + 1, box[1])  # exclude the first box plane from the statistic
    kernels.step_medium(u1.to(DEV), u2.to(DEV), m.to(DEV), u, box, first=first, h2=H2, stat=stat, stat_i=ei,
                        chunk=chunk)
    torch.cuda.synchronize()
    exp = _expected(u1, u2, m, box, first)
    i0, i1, j0, j1, k0, k1 = box
    got = u[i0:i1 + 1, j0:j1 + 1, k0:k1 + 1].cpu()
    if dtype == torch.float64:
        assert torch.equal(got, exp)
    assert_same_bits(got, exp)
    mask = torch.ones(shape, dtype=torch.bool)
    mask[i0:i1 + 1, j0:j1 + 1, k0:k1 + 1] = False
    assert bool((u.cpu()[mask] == -7.0).all())
    # slot 0: max |u| over the planes ei; slot 1 untouched; flag clear
    want = reference.max_abs_field(exp[ei[0] - i0:].double())
    (ga, gr, bad), = kernels.decode_err(stat)
    assert ga == want
    assert gr == -100.0 and not bad


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_step_medium_flags_nonfinite(C, dtype):
    from wave3d.ops import kernels, reference

    shape, box, _ = CASES[0]
    u1, u2, m = _inputs(shape, dtype)
    u1[5, 7, 33] = math.nan
    u = torch.zeros(shape, dtype=dtype, device=DEV)
    stat = kernels.new_err(1)
    kernels.step_medium(u1.to(DEV), u2.to(DEV), m.to(DEV), u, box, first=False, h2=H2, stat=stat,
                        stat_i=(box[0], box[1]))
    torch.cuda.synchronize()
    (ga, _, bad), = kernels.decode_err(stat)
    assert bad
    # the maximum ignores the NaN nodes
    want = reference.max_abs_field(_expected(u1, u2, m, box, False).double())
    assert math.isfinite(ga) and ga == want


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("first", [False, True])
def test_step_medium_on_padded_views(C, dtype, first):
    from wave3d.ops import kernels

    shape, box, chunk = CASES[2]
    cpu = _inputs(shape, dtype)
    dense = [t.to(DEV) for t in cpu]
    ud = torch.full(shape, -7.0, dtype=dtype, device=DEV)
    sd = kernels.new_err(1)
    kernels.step_medium(*dense, ud, box, first=first, h2=H2, stat=sd, stat_i=(1, 7), chunk=chunk)

    views = [kernels.alloc_level(*shape, dtype) for _ in range(4)]
    es = views[0].element_size()
    assert views[0].stride(1) * es % 128 == 0 and views[0].stride(1) > shape[2]  # padded pitch
    assert (views[0].data_ptr() + es) % 128 == 0                                   # k = 1 aligned
    assert all(float(v.abs().sum()) == 0.0 for v in views)
    for v, t in zip(views, cpu):
        v.copy_(t)
    views[3].fill_(-7.0)
    sv = kernels.new_err(1)
    kernels.step_medium(*views, box, first=first, h2=H2, stat=sv, stat_i=(1, 7), chunk=chunk)
    torch.cuda.synchronize()
    assert torch.equal(views[3].cpu(), ud.cpu())
    assert kernels.decode_err(sv) == kernels.decode_err(sd)
    for v in views:  # the padding between rows and in front of the view is still zero
        base = v._base
        inside = torch.zeros(base.shape, dtype=torch.bool, device=DEV)
        inside.as_strided(v.shape, v.stride(), v.storage_offset()).fill_(True)
        assert int(inside.sum()) == v.numel() and bool((base[~inside] == 0).all())
    # mixed layouts are refused before any launch
    with pytest.raises(ValueError):
        kernels.step_medium(dense[0], views[1], views[2], views[3], box, first=first, h2=H2, stat=sv,
                            stat_i=(1, 7))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("first", [False, True])
def test_uniform_medium_is_k_march(C, dtype, first):
    from wave3d.ops import kernels

    shape, box, chunk = CASES[2]
    u1, u2, _ = (t.to(DEV) for t in _inputs(shape, dtype))
    coef = 3.1e-4
    m = torch.full(shape, coef, dtype=dtype, device=DEV)
    a = torch.full(shape, -7.0, dtype=dtype, device=DEV)
    b = torch.full(shape, -7.0, dtype=dtype, device=DEV)
    kernels.step_medium(u1, u2, m, a, box, first=first, h2=H2, stat=kernels.new_err(1), stat_i=(1, 7), chunk=chunk)
    tabs = [torch.ones(n, dtype=dtype, device=DEV) for n in shape]
    # the Taylor start of k_march takes coef_first = 0.5 coef (an exact halving) from the host
    c_step = 0.5 * _cast(coef, dtype) if first else coef
    kernels.step(u1, u2, b, box, first=first, err_i=(1, 7), tx=tabs[0], ty=tabs[1], tz=tabs[2],
                 coefs=(*H2, c_step, 1.0), err=kernels.new_err(1), kernel="march", chunk=chunk)
    torch.cuda.synchronize()
    assert torch.equal(a.cpu(), b.cpu())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("first", [False, True])
def test_step_medium_variants_agree(C, dtype, first):
    """The ablation variants (cache policy of the m loads, rows per lane) compute the same bits."""
    from wave3d.ops import kernels

    shape, box, chunk = CASES[2]
    u1, u2, m = (t.to(DEV) for t in _inputs(shape, dtype))
    outs, stats = [], []
    for v in (None, "nt", "plain", "r2", "r2nt"):
        u = torch.full(shape, -7.0, dtype=dtype, device=DEV)
        st = kernels.new_err(1)
        kernels.step_medium(u1, u2, m, u, box, first=first, h2=H2, stat=st, stat_i=(1, 7), chunk=chunk, variant=v)
        outs.append(u)
        stats.append(kernels.decode_err(st))
    torch.cuda.synchronize()
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    assert all(s == stats[0] for s in stats[1:])
    with pytest.raises(ValueError):
        kernels.step_medium(u1, u2, m, outs[0], box, first=first, h2=H2, stat=kernels.new_err(1), stat_i=(1, 7),
                            variant="r3")


def test_step_medium_fused_wrap(C):
    from wave3d.ops import kernels

    shape = (12, 10, 75)
    dt = torch.float64
    u1, u2, m = (t.to(DEV) for t in _inputs(shape, dt))
    u = torch.zeros(shape, dtype=dt, device=DEV)
    X, Y, Z = (n - 2 for n in shape)
    kernels.step_medium(u1, u2, m, u, (1, X, 1, Y, 1, Z), first=False, h2=H2, stat=kernels.new_err(1),
                        stat_i=(1, X), wrap=(X - 1, 0, 2, X + 1))
    torch.cuda.synchronize()
    uc = u.cpu()
    assert float(uc[X - 1].abs().sum()) > 0
    assert torch.equal(uc[0], uc[X - 1])
    assert torch.equal(uc[X + 1], uc[2])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_inject_and_record(C, dtype):
    from wave3d.ops import kernels

    shape = (9, 8, 70)
    X = shape[0] - 2
    u0, _, m = _inputs(shape, dtype)
    nodes = [(3, 4, 5), (X - 1, 2, 66), (1, 6, 1)]  # the second one sits on a wrap source plane
    g = torch.tensor([0.75, -1.25, 3.5], dtype=dtype)
    u, md = u0.to(DEV), m.to(DEV)
    kernels.inject(u, md, nodes, g.to(DEV), wrap=(X - 1, 0, 2, X + 1))
    rec_nodes = nodes + [(0, 2, 66), (4, 4, 4), (X + 1, 7, 69)]
    out = torch.zeros(len(rec_nodes), dtype=dtype, device=DEV)
    kernels.record(u, rec_nodes, out)
    torch.cuda.synchronize()
    exp = u0.clone()
    for nd, gv in zip(nodes, g):
        exp[nd] = u0[nd] + m[nd] * gv
    exp[0, 2, 66] = exp[X - 1, 2, 66]
    assert torch.equal(u.cpu(), exp)
    assert torch.equal(out.cpu(), torch.stack([exp[nd] for nd in rec_nodes]))
    # node lists are validated before any launch
    with pytest.raises(ValueError):
        kernels.inject(u, md, [(3, 4, 5), (3, 4, 5)], g.to(DEV))
    with pytest.raises(ValueError):
        kernels.inject(u, md, [(0, 4, 5)], g.to(DEV))
    with pytest.raises(ValueError):
        kernels.record(u, [(3, 4, shape[2])], out)
    with pytest.raises(ValueError):
        kernels.inject(u, md, nodes, g[:2].to(DEV))
    assert torch.equal(u.cpu(), exp)


def _hetero(backend, dtype):
    import wave3d
    from test_medium_cpu import A, B, K, N, hetero_case

    speed2, w = hetero_case()
    prob = wave3d.MediumProblem(N, speed2, T=1.0, timesteps=K, dtype=dtype)
    return wave3d.MediumSolver(prob, backend, sources=[A], wavelet=w,
                               receivers=[B, (0, 6, 7), (N, 6, 7), (8, 8, 8)]).run()


def test_end_to_end_heterogeneous_fp64(C):
    ref, got = _hetero("cpu", "fp64"), _hetero("hip", "fp64")
    assert float(ref.traces.abs().max()) > 1e-3
    assert torch.equal(got.traces, ref.traces)
    assert torch.equal(got.u_final, ref.u_final)
    assert got.max_abs_u == ref.max_abs_u
    assert not got.aborted and got.total_ms > 0 and got.mpts_per_s > 0


def test_end_to_end_heterogeneous_fp32(C):
    # measured on MI355X: max |trace deviation| = 0.0 and max |field deviation| = 0.0 (max |u| = 1.44):
    # the fp32 kernel rounds like the fp32 oracle here; the bound is the one for chained fp32 steps
    ref, got = _hetero("cpu", "fp32"), _hetero("hip", "fp32")
    print("fp32 max |trace dev|", float((got.traces - ref.traces).abs().max()),
          "max |field dev|", float((got.u_final - ref.u_final).abs().max()),
          "max |u|", max(ref.max_abs_u))
    torch.testing.assert_close(got.traces, ref.traces, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(got.u_final, ref.u_final, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(torch.tensor(got.max_abs_u), torch.tensor(ref.max_abs_u), rtol=2e-5, atol=2e-5)


def test_end_to_end_uniform_matches_constant_speed_solver(C):
    import numpy as np

    import wave3d
    from wave3d.ops import reference
    from wave3d.utils import GOLDEN_N32_K20, fmt6

    n, k = 32, 20
    sx, sy, sz, ct, c = reference.tables(n, k)
    u0 = reference.analytic(sx, sy, sz, ct[0])
    res = wave3d.MediumSolver(wave3d.MediumProblem(n, c["a2"], timesteps=k), "hip", u0=u0).run()
    assert torch.equal(res.u_final, reference.solve(n, k)[2][1:n + 2])
    _, field = wave3d.WaveSolver(wave3d.WaveProblem(n, timesteps=k), "hip", kernel="march").solve_field()
    assert np.array_equal(res.u_final.numpy(), field)
    f = reference.analytic(sx[1:n], sy[1:n], sz[1:n], ct[k])
    ea, er = reference.max_errors(res.u_final[1:n, 1:n, 1:n], f)
    assert (fmt6(ea), fmt6(er)) == GOLDEN_N32_K20[-1]


def test_check_every_stops_on_nonfinite(C):
    import wave3d

    n, k = 16, 12
    u0 = torch.zeros((n + 1,) * 3, dtype=torch.float64)
    u0[5, 6, 7] = math.inf
    res = wave3d.MediumSolver(wave3d.MediumProblem(n, 0.5, timesteps=k), "hip", u0=u0, check_every=4).run()
    assert res.aborted and 1 <= res.abort_layer <= 4
    assert res.abort_reason == "non-finite values"
    assert len(res.max_abs_u) == 5  # layers 0..4: the run stopped at the first check
