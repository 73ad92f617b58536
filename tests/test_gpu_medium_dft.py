"""On-the-fly Fourier transforms on the GPU: k_dft_acc (csrc/hip_medium_dft.hip) against the PyTorch
oracle (ops/reference.py dft_accumulate), and MediumSolver.run(frequencies=) / gradient_dft, "hip"
against "cpu".

A launch must be bitwise equal in fp64 and in fp32: both sides round every product before its add. The
fp64 front-end results are bitwise equal too; the fp32 ones stay inside the bound of
test_gpu_medium_order.py, measured on the oracle and never on the kernel:
|got - exp32| <= 4 max |exp32 - exp64|. Inputs of the single launches: u, re, im in [-0.5, 0.5].

Measured on one MI355X: in all 72 fp32 comparisons of the front-end tests (spectra, traces, u_final,
grad_speed2, grad_wavelet over the six cases and dft_every 1 and 2) max |hip - oracle32| is 0, the bounds
lying between 2e-8 and 1.1e-6; on the device Parseval's identity holds to 2.4e-16 of max |grad|.
"""
import math

import pytest
import torch

from bits import assert_same_bits
from test_gpu_medium import CASES, _rand
from test_gpu_medium_density import _layered
from test_gpu_medium_order import _at, _box_mask

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = (torch.float64, torch.float32)


def _nf():
    from wave3d.ops import kernels

    return kernels.dft_frequencies_per_launch()


def _inputs(shape, dtype, F):
    """CPU tensors u, [re_f], [im_f]."""
    return (_rand(shape, dtype, 1, -0.5, 0.5), [_rand(shape, dtype, 10 + f, -0.5, 0.5) for f in range(F)],
            [_rand(shape, dtype, 50 + f, -0.5, 0.5) for f in range(F)])


def _rows(F, dtype, p=3):
    from wave3d.ops import reference

    c, s = reference.dft_tables([0.7 * f for f in range(F)], [0, p, p + 4], 0.031, dtype)
    return c, s  # row 0 = (1, -0): the first frequency is 0 as well


def _oracle(u, re, im, box, c_row, s_row):
    from wave3d.ops import reference

    re, im = [t.clone() for t in re], [t.clone() for t in im]
    reference.dft_accumulate(re, im, u, box, c_row, s_row)
    return re, im


def _same(got, exp):
    for g, e in zip(got, exp):
        if e.dtype == torch.float64 and not bool(torch.isnan(e).any()):
            assert torch.equal(g.cpu(), e)
        assert_same_bits(g.cpu(), e)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fcount", ["1", "NF", "NF+1", "2NF+1"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_dft_accumulate_matches_reference(C, case, fcount, dtype):
    from wave3d.ops import kernels

    NF = _nf()
    assert NF == C.dft_nf and NF >= 1
    F = {"1": 1, "NF": NF, "NF+1": NF + 1, "2NF+1": 2 * NF + 1}[fcount]
    shape, box, chunk = CASES[case]
    u, re0, im0 = _inputs(shape, dtype, F)
    c, s = _rows(F, dtype)
    ud, cd, sd = u.to(DEV), c.to(DEV), s.to(DEV)
    re, im = [t.to(DEV) for t in re0], [t.to(DEV) for t in im0]
    kernels.dft_accumulate(ud, re, im, box, cd[1], sd[1], chunk=chunk)
    torch.cuda.synchronize()
    exp_re, exp_im = _oracle(u, re0, im0, box, c[1], s[1])
    assert all(not torch.equal(e, t) for e, t in zip(exp_re + exp_im[1:], re0 + im0[1:]))  # something happened
    _same(re, exp_re)
    _same(im, exp_im)
    # a second call, another row, accumulates on top of the first
    kernels.dft_accumulate(ud, re, im, box, cd[2], sd[2], chunk=chunk)
    torch.cuda.synchronize()
    exp_re, exp_im = _oracle(u, exp_re, exp_im, box, c[2], s[2])
    _same(re, exp_re)
    _same(im, exp_im)
    # every node outside the box keeps its bits, and u is never written
    mask = _box_mask(shape, box)
    for t, t0 in zip(re + im, re0 + im0):
        assert torch.equal(t.cpu()[mask], t0[mask])
    assert torch.equal(ud.cpu(), u)


def test_several_boxes_in_one_launch(C):
    from wave3d.ops import kernels

    shape = CASES[2][0]
    boxes = [(1, 3, 5, 33, 60, 129), (4, 7, 1, 20, 1, 70), (4, 7, 21, 38, 3, 64)]
    F = _nf() + 1
    u, re0, im0 = _inputs(shape, torch.float64, F)
    c, s = _rows(F, torch.float64)
    re, im = [t.to(DEV) for t in re0], [t.to(DEV) for t in im0]
    kernels.dft_accumulate(u.to(DEV), re, im, boxes, c[1].to(DEV), s[1].to(DEV))
    torch.cuda.synchronize()
    exp_re, exp_im = re0, im0
    for b in boxes:
        exp_re, exp_im = _oracle(u, exp_re, exp_im, b, c[1], s[1])
    _same(re, exp_re)
    _same(im, exp_im)


@pytest.mark.parametrize("dtype", DTYPES)
def test_padded_views(C, dtype):
    """alloc_level views give the dense tensors' bits and leave the padding alone."""
    from wave3d.ops import kernels

    shape, box, chunk = CASES[2]
    F = _nf() + 1
    u, re0, im0 = _inputs(shape, dtype, F)
    c, s = _rows(F, dtype)
    cd, sd = c.to(DEV), s.to(DEV)
    views = [kernels.alloc_level(*shape, dtype) for _ in range(1 + 2 * F)]
    assert views[0].stride(1) > shape[2]  # padded pitch
    for w, t in zip(views, [u] + re0 + im0):
        w.copy_(t)
    kernels.dft_accumulate(views[0], views[1:1 + F], views[1 + F:], box, cd[1], sd[1], chunk=chunk)
    torch.cuda.synchronize()
    exp_re, exp_im = _oracle(u, re0, im0, box, c[1], s[1])
    _same(views[1:1 + F], exp_re)
    _same(views[1 + F:], exp_im)
    assert torch.equal(views[0].cpu(), u)
    for w in views:  # the padding between rows and in front of the view is still zero
        base = w._base
        inside = torch.zeros(base.shape, dtype=torch.bool, device=DEV)
        inside.as_strided(w.shape, w.stride(), w.storage_offset()).fill_(True)
        assert int(inside.sum()) == w.numel() and bool((base[~inside] == 0).all())
    with pytest.raises(ValueError, match="strides"):  # mixed layouts are refused before any launch
        kernels.dft_accumulate(u.to(DEV), views[1:1 + F], views[1 + F:], box, cd[1], sd[1])


def _specials(dtype):
    fi = torch.finfo(dtype)
    tiny = fi.smallest_normal * fi.eps  # the smallest subnormal
    return [0.0, -0.0, tiny, -tiny, 3 * tiny, -fi.smallest_normal / 2, fi.smallest_normal, math.inf, -math.inf,
            math.nan, fi.max, -fi.max]


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values_in_one_launch(C, dtype):
    """+-0, subnormals, +-inf and NaN in u change re / im exactly where the oracle changes them, and
    identically (inf times a zero twiddle is NaN on both sides); a NaN at a masked lane, past the row end
    or outside the box, changes nothing."""
    from wave3d.ops import kernels

    shape, box, chunk = CASES[1]  # an interior sub-box: masked lanes on every side
    i0, i1, j0, j1, k0, k1 = box
    F = 3
    u, re0, im0 = _inputs(shape, dtype, F)
    sp = _specials(dtype)
    g = torch.Generator().manual_seed(9)
    flat = _at(u, box).reshape(-1)
    where = torch.randperm(flat.numel(), generator=g)[:8 * len(sp)]
    vals = torch.tensor(sp * 8, dtype=dtype)
    bu = _at(u, box).clone().reshape(-1)
    bu[where] = vals
    _at(u, box).copy_(bu.reshape(_at(u, box).shape))
    for t in re0 + im0:  # accumulators that are zero, so that a -0 product shows
        _at(t, box)[::2, ::3, ::5] = 0.0
    # NaN at masked lanes: past the row end and in front of it, rows and planes beside the box
    outside = [(i0, j0, k1 + 1), (i1, j1, k0 - 1), (i0, j0 - 1, k0), (i1, j1 + 1, k1), (i0 - 1, j0, k0), (i1 + 1, j1, k1),
               (i0, j0, shape[2] - 1), (0, 0, 0)]
    for nd in outside:
        u[nd] = math.nan
    # twiddles with an exact zero, a negative one and a subnormal
    c = torch.tensor([0.0, -1.0, 0.37], dtype=dtype)
    s = torch.tensor([-0.0, torch.finfo(dtype).smallest_normal / 4, -0.93], dtype=dtype)
    re, im = [t.to(DEV) for t in re0], [t.to(DEV) for t in im0]
    ud = u.to(DEV)
    kernels.dft_accumulate(ud, re, im, box, c.to(DEV), s.to(DEV), chunk=chunk)
    torch.cuda.synchronize()
    exp_re, exp_im = _oracle(u, re0, im0, box, c, s)
    assert bool(torch.isnan(_at(exp_re[0], box)).any()) and bool(torch.isinf(_at(exp_re[1], box)).any())
    _same(re, exp_re)
    _same(im, exp_im)
    mask = _box_mask(shape, box)
    for t, t0 in zip(re + im, re0 + im0):
        assert_same_bits(t.cpu()[mask], t0[mask])
        assert not bool(torch.isnan(t.cpu()[mask]).any())
    assert_same_bits(ud.cpu(), u)


def test_rejected_calls(C):
    """Every one refused before any launch, as a ValueError: the accumulators keep their values."""
    from wave3d.ops import kernels

    shape, box, _ = CASES[0]
    nx, ny, nz = shape
    dt = torch.float64
    F = 2
    u0, re0, im0 = _inputs(shape, dt, F)
    u, re, im = u0.to(DEV), [t.to(DEV) for t in re0], [t.to(DEV) for t in im0]
    c, s = (t[1].contiguous().to(DEV) for t in _rows(F, dt))

    def unchanged():
        torch.cuda.synchronize()
        assert torch.equal(u.cpu(), u0)
        assert all(torch.equal(t.cpu(), t0) for t, t0 in zip(re + im, re0 + im0))

    edges = [(0, 11, 1, 19, 1, 68), (1, nx - 1, 1, 19, 1, 68), (1, 11, 0, 19, 1, 68), (1, 11, 1, ny - 1, 1, 68),
             (1, 11, 1, 19, 0, 68), (1, 11, 1, 19, 1, nz - 1)]
    for bad in edges:  # a box on a storage edge, one per side
        with pytest.raises(ValueError, match="owned region"):
            kernels.dft_accumulate(u, re, im, bad, c, s)
    with pytest.raises(ValueError, match="strides"):
        kernels.dft_accumulate(u, [kernels.alloc_level(*shape, dt), re[1]], im, box, c, s)
    with pytest.raises(ValueError, match="dtypes"):
        kernels.dft_accumulate(u, re, [im[0], im[1].float()], box, c, s)
    with pytest.raises(ValueError, match="shapes"):
        kernels.dft_accumulate(u, [re[0][:, :, :-1], re[1]], im, box, c, s)
    with pytest.raises(ValueError, match="device tensors"):
        kernels.dft_accumulate(u, re, [im[0].cpu(), im[1]], box, c, s)
    with pytest.raises(ValueError, match="device tensors"):
        kernels.dft_accumulate(u.cpu(), re, im, box, c, s)
    with pytest.raises(ValueError, match="one level per frequency"):
        kernels.dft_accumulate(u, re, im[:1], box, c, s)
    with pytest.raises(ValueError, match="at least one frequency"):
        kernels.dft_accumulate(u, [], [], box, c[:0], s[:0])
    for bad in (c[:1], torch.cat([c, c]), c.float(), c.cpu(), torch.stack([c, c]), torch.cat([c, c])[::2]):
        with pytest.raises(ValueError, match="c_row"):  # length, dtype, device, rank, stride
            kernels.dft_accumulate(u, re, im, box, bad, s)
        with pytest.raises(ValueError, match="s_row"):
            kernels.dft_accumulate(u, re, im, box, c, bad)
    unchanged()
    # an accumulator aliasing u or another accumulator
    with pytest.raises(ValueError, match=r"re\[1\] shares memory with u"):
        kernels.dft_accumulate(u, [re[0], u], im, box, c, s)
    with pytest.raises(ValueError, match=r"im\[0\] shares memory with u"):
        kernels.dft_accumulate(u, re, [u, im[1]], box, c, s)
    with pytest.raises(ValueError, match=r"re\[1\] shares memory with re\[0\]"):
        kernels.dft_accumulate(u, [re[0], re[0]], im, box, c, s)
    with pytest.raises(ValueError, match=r"im\[1\] shares memory with re\[0\]"):
        kernels.dft_accumulate(u, re, [im[0], re[0]], box, c, s)
    # two views of one buffer that overlap without starting at the same address
    buf = torch.zeros(2 * nx * ny * nz, dtype=dt, device=DEV)
    lo, hi = buf[:nx * ny * nz].view(shape), buf[ny * nz:ny * nz + nx * ny * nz].view(shape)
    with pytest.raises(ValueError, match="shares memory"):
        kernels.dft_accumulate(u, [lo, re[1]], [hi, im[1]], box, c, s)
    unchanged()
    # the launcher has its own checks behind the wrapper's, ValueErrors as well
    gv = [nx, ny, nz, nz, ny * nz]
    P = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    for args in ((u.data_ptr(), P(re), P([im[0], u]), c.data_ptr(), s.data_ptr(), gv, [list(box)]),
                 (u.data_ptr(), P(re), P([im[0], re[1]]), c.data_ptr(), s.data_ptr(), gv, [list(box)]),
                 (u.data_ptr(), P([lo, re[1]]), P([hi, im[1]]), c.data_ptr(), s.data_ptr(), gv, [list(box)]),
                 (u.data_ptr(), P(re), P(im), c.data_ptr(), s.data_ptr(), gv, [list(edges[1])]),
                 (u.data_ptr(), P(re), P(im), c.data_ptr(), s.data_ptr(), [nx, ny, nz, nz - 1, ny * nz], [list(box)]),
                 (u.data_ptr(), P(re), P(im[:1]), c.data_ptr(), s.data_ptr(), gv, [list(box)]),
                 (u.data_ptr(), [], [], c.data_ptr(), s.data_ptr(), gv, [list(box)]),
                 (u.data_ptr(), P(re), P(im), 0, s.data_ptr(), gv, [list(box)])):
        with pytest.raises(ValueError):
            C.k_dft_acc_f64(*args, 0, st)
    unchanged()
    assert not bool(buf.any())


# ---- the front end: run(frequencies=) and gradient_dft, "hip" against "cpu" ------------------------

N, K = 12, 9
SOURCES = [(0, 4, 6), (6, 3, 5)]
REC = [(N, 7, 3), (4, 5, 5), (6, 3, 5)]
FREQS = [0.0, 0.9, 2.6]
WEIGHTS = [1.0, 0.5, 2.0]
FRONT = ["order2", "order4", "order8", "density", "sponge", "offgrid"]


def _solver(backend, name, dtype="fp64"):
    import wave3d

    rho, speed2 = _layered(N, 31)
    order = {"order4": 4, "order8": 8}.get(name, 2)
    prob = wave3d.MediumProblem(N, speed2, timesteps=K, dtype=dtype, space_order=order,
                                density=rho if name == "density" else None)
    w = torch.stack([wave3d.ricker(3.0, 0.3, K, prob.tau), -0.5 * wave3d.ricker(2.0, 0.2, K, prob.tau)], 1)
    kw = dict(wavelet=w, taper=wave3d.sponge_taper(prob, 3) if name == "sponge" else None)
    if name == "offgrid":
        kw.update(source_positions=torch.tensor([[0.3, 4.2, 6.5], [6.0, 3.0, 5.0]], dtype=torch.float64),
                  receiver_positions=torch.tensor([[11.7, 7.1, 3.4], [4.5, 5.5, 5.5], [6.0, 3.0, 5.0]],
                                                  dtype=torch.float64))
    else:
        kw.update(sources=SOURCES, receivers=REC)
    return wave3d.MediumSolver(prob, backend, **kw)


_ORACLE = {}


def _oracle_run(name, every, dtype):
    """The "cpu" run, computed once per (case, dft_every, dtype) and never changed."""
    key = ("run", name, every, dtype)
    if key not in _ORACLE:
        _ORACLE[key] = _solver("cpu", name, dtype).run(frequencies=FREQS, dft_every=every)
    return _ORACLE[key]


def _observed(name):
    key = ("obs", name)
    if key not in _ORACLE:
        import wave3d

        sol = _solver("cpu", name)
        p = sol.problem
        prob = wave3d.MediumProblem(N, p.speed2 * 1.1, timesteps=K, space_order=p.space_order,
                                    density=None if p.density is None else p.density * 0.9)
        pert = wave3d.MediumSolver(prob, "cpu", wavelet=sol.wavelet, taper=sol.taper, sources=sol.sources,
                                   receivers=sol.receivers, source_positions=sol.source_positions,
                                   receiver_positions=sol.receiver_positions)
        _ORACLE[key] = pert.run().traces
    return _ORACLE[key]


def _oracle_gradient(name, every, dtype):
    key = ("grad", name, every, dtype)
    if key not in _ORACLE:
        _ORACLE[key] = _solver("cpu", name, dtype).gradient_dft(_observed(name), FREQS, weights=WEIGHTS,
                                                               dft_every=every)
    return _ORACLE[key]


def _within(what, got, want32, want64):
    """fp32 "hip" against the fp32 oracle, inside 4 max |oracle32 - oracle64|; prints what it measured."""
    if torch.is_complex(got):
        got, want32, want64 = (torch.view_as_real(t) for t in (got, want32, want64))
    bound = 4 * float((want32.double() - want64.double()).abs().max())
    err = float((got.double() - want32.double()).abs().max())
    print(f"{what} fp32: max |hip - oracle32| {err:.3e} bound {bound:.3e} max |oracle| "
          f"{float(want64.abs().max()):.3e}")
    assert got.dtype == want32.dtype and bound > 0 and err <= bound


@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("name", FRONT)
def test_run_with_frequencies_matches_oracle(C, name, every):
    want = _oracle_run(name, every, "fp64")
    sol = _solver("hip", name)
    got = sol.run(frequencies=FREQS, dft_every=every)
    assert got.spectra.dtype == torch.complex128 and got.spectra.device.type == "cpu"
    assert tuple(got.spectra.shape) == (len(FREQS),) + (N + 1,) * 3
    assert float(want.spectra.abs().max()) > 0 and float(want.spectra[1].imag.abs().max()) > 0
    assert torch.equal(torch.view_as_real(got.spectra), torch.view_as_real(want.spectra))
    assert torch.equal(got.traces, want.traces) and torch.equal(got.u_final, want.u_final)
    for key in ("frequencies", "dft_every", "dft_samples"):
        assert got.extra[key] == want.extra[key]
    assert got.extra["dft_samples"] == K // every + 1
    # the non-spectral results are those of a run without frequencies, bit for bit
    plain = sol.run()
    assert plain.spectra is None and "dft_every" not in plain.extra
    assert torch.equal(plain.traces, got.traces) and torch.equal(plain.u_final, got.u_final)
    assert plain.max_abs_u == got.max_abs_u


@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("name", FRONT)
def test_run_with_frequencies_fp32(C, name, every):
    want, want64 = _oracle_run(name, every, "fp32"), _oracle_run(name, every, "fp64")
    sol = _solver("hip", name, "fp32")
    got = sol.run(frequencies=FREQS, dft_every=every)
    assert got.spectra.dtype == torch.complex64
    _within(f"{name} every {every} spectra", got.spectra, want.spectra, want64.spectra)
    _within(f"{name} every {every} traces", got.traces, want.traces, want64.traces)
    _within(f"{name} every {every} u_final", got.u_final, want.u_final, want64.u_final)
    plain = sol.run()
    assert torch.equal(plain.traces, got.traces) and torch.equal(plain.u_final, got.u_final)
    assert plain.max_abs_u == got.max_abs_u


@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("name", FRONT)
def test_gradient_dft_matches_oracle(C, name, every):
    import wave3d

    want = _oracle_gradient(name, every, "fp64")
    got = _solver("hip", name).gradient_dft(_observed(name), FREQS, weights=WEIGHTS, dft_every=every)
    assert want.misfit > 0 and float(want.grad_speed2.abs().max()) > 0 and float(want.grad_wavelet.abs().max()) > 0
    assert got.misfit == want.misfit and torch.equal(got.traces, want.traces)
    assert torch.equal(got.grad_speed2, want.grad_speed2) and torch.equal(got.grad_wavelet, want.grad_wavelet)
    assert got.extra["levels"] == wave3d.gradient_dft_levels(len(FREQS), density=name == "density")
    assert got.extra["levels"] == 17 + (name == "density")
    assert got.extra["recomputed_steps"] == 0 and got.extra["dft_every"] == every
    assert got.extra["dft_samples"] == (K - 1) // every and got.extra["frequencies"] == FREQS
    assert got.extra["forward_ms"] > 0 and got.extra["reverse_ms"] > 0


@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("name", FRONT)
def test_gradient_dft_fp32(C, name, every):
    want, want64 = _oracle_gradient(name, every, "fp32"), _oracle_gradient(name, every, "fp64")
    got = _solver("hip", name, "fp32").gradient_dft(_observed(name), FREQS, weights=WEIGHTS, dft_every=every)
    _within(f"{name} every {every} grad_speed2", got.grad_speed2, want.grad_speed2, want64.grad_speed2)
    _within(f"{name} every {every} grad_wavelet", got.grad_wavelet, want.grad_wavelet, want64.grad_wavelet)
    _within(f"{name} every {every} traces", got.traces, want.traces, want64.traces)
    assert abs(got.misfit - want.misfit) <= 4 * abs(want.misfit - want64.misfit) and want.misfit != want64.misfit


def test_full_spectrum_on_the_gpu_is_the_time_domain_gradient(C):
    """Parseval on the device: every bin of the pairs' half spectrum gives gradient()'s grad_speed2 up to
    rounding (the cap of tests/test_medium_dft_cpu.py), and the band-limited one differs."""
    import wave3d

    sol = _solver("hip", "sponge")
    f, w = wave3d.dft_bins(sol.problem, every=1, pairs=True)
    time = sol.gradient(_observed("sponge"))
    full = sol.gradient_dft(_observed("sponge"), f, weights=w)
    scale = float(time.grad_speed2.abs().max())
    dev = float((full.grad_speed2 - time.grad_speed2).abs().max()) / scale
    print("max |delta| / max |grad| =", dev)
    assert scale > 0 and dev <= 1e-12
    assert torch.equal(full.grad_wavelet, time.grad_wavelet) and full.misfit == time.misfit
    low = sol.gradient_dft(_observed("sponge"), f[:2], weights=w[:2])
    assert float((low.grad_speed2 - time.grad_speed2).abs().max()) > 1e-3 * scale


def test_memory_is_checked_before_any_allocation(C):
    """An absurd number of frequencies on a tiny grid: the RuntimeError comes before a level exists."""
    sol = _solver("hip", "order2")
    many = torch.zeros(20_000_000, dtype=torch.float64)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(RuntimeError, match="levels"):
        sol.run(frequencies=many)
    assert torch.cuda.memory_allocated() == before
    with pytest.raises(RuntimeError, match="levels"):
        sol.gradient_dft(_observed("order2"), many)
    assert torch.cuda.memory_allocated() == before
