"""Density gradients on the GPU: k_face_corr (csrc/hip_medium_corr.hip) against the PyTorch oracle
(ops/reference.py face_correlation), and MediumSolver.gradient(wrt_density=True), "hip" against "cpu".

fp64 results must be bitwise equal: both sides round every operation in the same order; a single fp32
launch of k_face_corr is bitwise equal too. The fp32 gradient stays inside the bound of
test_gpu_medium_order.py, measured on the oracle and never on the kernel:
|got - exp32| <= 4 max |exp32 - exp64|. Inputs: a, v in [0, 1], acc in [-0.5, 0.5].
"""
import pytest
import torch

from test_gpu_medium import CASES, H2, _cast, _rand
from test_gpu_medium_density import _layered
from test_gpu_medium_order import _at, _box_mask, _check

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = (torch.float64, torch.float32)


def _inputs(shape, dtype):
    """CPU tensors a, v, acc."""
    return _rand(shape, dtype, 1), _rand(shape, dtype, 2), _rand(shape, dtype, 3, -0.5, 0.5)


def _corr(a, v, box, dtype=None):
    """reference.face_correlation in ``dtype`` (default: that of the inputs), h2 cast like the kernel's."""
    from wave3d.ops import reference

    h2 = [_cast(x, a.dtype) for x in H2]
    if dtype is not None:
        a, v = a.to(dtype), v.to(dtype)
    return reference.face_correlation(a, v, box, *h2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_face_correlation_matches_reference(C, case, dtype):
    from wave3d.ops import kernels

    shape, box, chunk = CASES[case]
    a, v, acc0 = _inputs(shape, dtype)
    ad, vd, acc = a.to(DEV), v.to(DEV), acc0.to(DEV)
    kernels.face_correlation(ad, vd, acc, box, h2=H2, chunk=chunk)
    torch.cuda.synchronize()
    once = acc.cpu()
    kernels.face_correlation(ad, vd, acc, box, h2=H2, chunk=chunk)
    torch.cuda.synchronize()
    twice = acc.cpu()
    c, c64 = _corr(a, v, box), _corr(a, v, box, torch.float64)
    assert float(c.abs().max()) > 1
    exp1, exp1_64 = _at(acc0, box) + c, _at(acc0, box).double() + c64
    _check(_at(once, box), exp1, exp1_64)
    # a second call accumulates on top of the first
    _check(_at(twice, box), exp1 + c, exp1_64 + c64)
    # every node outside the box keeps its value, and the inputs are never written
    mask = _box_mask(shape, box)
    assert torch.equal(once[mask], acc0[mask]) and torch.equal(twice[mask], acc0[mask])
    assert torch.equal(ad.cpu(), a) and torch.equal(vd.cpu(), v)
    # symmetric in its two fields bit for bit
    sym = acc0.to(DEV)
    kernels.face_correlation(vd, ad, sym, box, h2=H2, chunk=chunk)
    torch.cuda.synchronize()
    assert torch.equal(sym.cpu(), once)


def test_several_boxes_in_one_launch(C):
    from wave3d.ops import kernels

    shape = CASES[2][0]
    boxes = [(1, 3, 5, 33, 60, 129), (4, 7, 1, 20, 1, 70), (4, 7, 21, 38, 3, 64)]
    a, v, acc0 = _inputs(shape, torch.float64)
    acc = acc0.to(DEV)
    kernels.face_correlation(a.to(DEV), v.to(DEV), acc, boxes, h2=H2)
    torch.cuda.synchronize()
    exp = acc0.clone()
    for b in boxes:
        _at(exp, b).copy_(_at(acc0, b) + _corr(a, v, b))
    assert torch.equal(acc.cpu(), exp)


@pytest.mark.parametrize("dtype", DTYPES)
def test_padded_views(C, dtype):
    """alloc_level views give the dense tensors' bits and leave the padding alone."""
    from wave3d.ops import kernels

    shape, box, chunk = CASES[2]
    cpu = _inputs(shape, dtype)
    d = [t.to(DEV) for t in cpu]
    kernels.face_correlation(*d, box, h2=H2, chunk=chunk)
    views = [kernels.alloc_level(*shape, dtype) for _ in range(3)]
    assert views[0].stride(1) > shape[2]  # padded pitch
    for w, t in zip(views, cpu):
        w.copy_(t)
    kernels.face_correlation(*views, box, h2=H2, chunk=chunk)
    torch.cuda.synchronize()
    assert torch.equal(views[2].cpu(), d[2].cpu()) and not torch.equal(views[2].cpu(), cpu[2])
    assert torch.equal(views[0].cpu(), cpu[0]) and torch.equal(views[1].cpu(), cpu[1])
    for w in views:  # the padding between rows and in front of the view is still zero
        base = w._base
        inside = torch.zeros(base.shape, dtype=torch.bool, device=DEV)
        inside.as_strided(w.shape, w.stride(), w.storage_offset()).fill_(True)
        assert int(inside.sum()) == w.numel() and bool((base[~inside] == 0).all())
    with pytest.raises(ValueError, match="strides"):  # mixed layouts are refused before any launch
        kernels.face_correlation(d[0], views[1], views[2], box, h2=H2)


def test_rejected_calls(C):
    """Every one refused before any launch: acc keeps its values."""
    from wave3d.ops import kernels

    shape, box, _ = CASES[0]
    nx, ny, nz = shape
    dt = torch.float64
    a, v, acc0 = (t.to(DEV) for t in _inputs(shape, dt))
    acc = acc0.clone()
    edges = [(0, 11, 1, 19, 1, 68), (1, nx - 1, 1, 19, 1, 68), (1, 11, 0, 19, 1, 68), (1, 11, 1, ny - 1, 1, 68),
             (1, 11, 1, 19, 0, 68), (1, 11, 1, 19, 1, nz - 1)]
    for bad in edges:  # a box on a storage edge, one per side
        with pytest.raises(ValueError, match="owned region"):
            kernels.face_correlation(a, v, acc, bad, h2=H2)
    with pytest.raises(ValueError, match="strides"):
        padded = kernels.alloc_level(*shape, dt)
        kernels.face_correlation(a, padded, acc, box, h2=H2)
    with pytest.raises(ValueError, match="dtypes"):
        kernels.face_correlation(a, v.float(), acc, box, h2=H2)
    with pytest.raises(ValueError, match="shapes"):
        kernels.face_correlation(a, v[:, :, :-1], acc, box, h2=H2)
    with pytest.raises(ValueError, match="device tensors"):
        kernels.face_correlation(a, v.cpu(), acc, box, h2=H2)
    with pytest.raises(ValueError, match="h2"):
        kernels.face_correlation(a, v, acc, box, h2=(H2[0], 0.0, H2[2]))
    torch.cuda.synchronize()
    assert torch.equal(acc, acc0)
    # acc aliasing an input: the aliased grid is untouched as well
    keep = a.clone()
    with pytest.raises(ValueError, match="shares memory with a"):
        kernels.face_correlation(a, v, a, box, h2=H2)
    with pytest.raises(ValueError, match="shares memory with v"):
        kernels.face_correlation(v, a, a, box, h2=H2)
    # two views of one buffer that overlap without starting at the same address
    buf = torch.zeros(2 * nx * ny * nz, dtype=dt, device=DEV)
    lo, hi = buf[:nx * ny * nz].view(shape), buf[ny * nz:ny * nz + nx * ny * nz].view(shape)
    with pytest.raises(ValueError, match="shares memory"):
        kernels.face_correlation(lo, v, hi, box, h2=H2)
    # the launcher has its own checks behind the wrapper's
    gv = [nx, ny, nz, nz, ny * nz]
    for args in ((a.data_ptr(), v.data_ptr(), a.data_ptr(), gv, [list(box)]),
                 (a.data_ptr(), v.data_ptr(), acc.data_ptr(), gv, [list(edges[1])]),
                 (a.data_ptr(), v.data_ptr(), acc.data_ptr(), [nx, ny, nz, nz - 1, ny * nz], [list(box)])):
        with pytest.raises(C.Wave3dError):
            C.k_face_corr_f64(*args, list(H2), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(a, keep) and torch.equal(acc, acc0) and not bool(buf.any())


# ---- the front-end: gradient(wrt_density=True), "hip" against "cpu" ---------------------------

N, K = 10, 9
REC = [(N, 7, 3), (4, 5, 5), (6, 3, 5)]


def _solver(backend, dtype="fp64"):
    """The density suite's gradient case (test_gpu_medium_density._solver), in either dtype."""
    import wave3d

    rho, speed2 = _layered(N, 31)
    prob = wave3d.MediumProblem(N, speed2, timesteps=K, density=rho, dtype=dtype)
    w = torch.stack([wave3d.ricker(3.0, 0.3, K, prob.tau), -0.5 * wave3d.ricker(2.0, 0.2, K, prob.tau)], 1)
    return wave3d.MediumSolver(prob, backend, sources=[(0, 4, 6), (6, 3, 5)], wavelet=w, receivers=REC,
                               taper=wave3d.sponge_taper(prob, 3))


@pytest.fixture(scope="module")
def gradient_case():
    from wave3d.ops import reference

    cpu = _solver("cpu")
    p = cpu.problem
    observed = reference.solve_medium(N, K, p.speed2 * 1.1, sources=cpu.sources, wavelet=cpu.wavelet, receivers=REC,
                                      taper=cpu.taper, density=p.density * 0.9)[0]
    return observed, cpu.gradient(observed, wrt_density=True)


@pytest.mark.parametrize("segment", [1, 3, 8, None])  # 8 = K - 1
def test_gradient_matches_oracle(C, gradient_case, segment):
    import wave3d

    observed, want = gradient_case
    sol = _solver("hip")
    got = sol.gradient(observed, segment=segment, wrt_density=True)
    assert want.misfit > 0 and float(want.grad_density.abs().max()) > 0 and float(want.grad_speed2.abs().max()) > 0
    assert got.misfit == want.misfit and torch.equal(got.traces, want.traces)
    assert torch.equal(got.grad_speed2, want.grad_speed2) and torch.equal(got.grad_wavelet, want.grad_wavelet)
    assert torch.equal(got.grad_density, want.grad_density)
    seg = got.extra["segment"]
    assert seg == (segment if segment is not None else wave3d.best_gradient_segment(K, wrt_density=True))
    assert got.extra["levels"] == wave3d.gradient_levels(K, seg, density=True, wrt_density=True)
    assert got.extra["levels"] == wave3d.gradient_levels(K, seg, density=True) + min(seg, K - 1) + 1
    assert got.extra["wrt_density"] is True
    # the keyword changes nothing else
    off = sol.gradient(observed, segment=segment)
    assert off.grad_density is None and off.extra["wrt_density"] is False
    assert off.extra["levels"] == wave3d.gradient_levels(K, off.extra["segment"], density=True)
    assert torch.equal(off.grad_speed2, got.grad_speed2) and torch.equal(off.grad_wavelet, got.grad_wavelet)
    assert torch.equal(off.traces, got.traces) and off.misfit == got.misfit


def test_gradient_fp32(C, gradient_case):
    """fp32 "hip" against the fp32 oracle, inside 4 max |oracle32 - oracle64|."""
    observed, want64 = gradient_case
    want = _solver("cpu", "fp32").gradient(observed, wrt_density=True)
    got = _solver("hip", "fp32").gradient(observed, wrt_density=True)
    assert got.grad_density.dtype == torch.float32 and float(got.grad_density.abs().max()) > 0
    g, w, w64 = got.grad_density, want.grad_density, want64.grad_density
    bound = 4 * float((w.double() - w64).abs().max())
    err = float((g.double() - w.double()).abs().max())
    print("grad_density fp32: max |hip - oracle32|", err, "bound", bound, "max |oracle|", float(w64.abs().max()))
    assert bound > 0 and err <= bound
