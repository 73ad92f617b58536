"""Source illumination on the GPU: the illum and save+illum modes of k_march_m, k_march_mh and
k_march_mb (csrc/hip_medium.hip) against the plain-PyTorch oracle, and
MediumSolver.gradient(illumination=True) ("hip": the forward pass proper accumulates, the recomputed
steps do not) against ops/reference.py.

fp64 results must be *bitwise* equal: h = h + lap * lap, the product rounded before the add, with the
oracle's Laplacian; a single fp32 step is bitwise equal too. The fp32 bound of the solver-level test is
measured on the oracle, never on the kernel: |got - exp64| <= 4 max |exp32 - exp64|, both expectations
computed on the CPU from the same fp32-representable inputs.
"""
import pytest
import torch

from bits import assert_same_bits
from test_gpu_medium import CASES, H2, _cast, _inputs, _rand
from test_gpu_medium_gradient import _dense, _problem
from test_gpu_medium_order import CASES as STAR_CASES
from test_gpu_medium_order import _at, _box_mask
from test_gpu_sponge import _tapers

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -7.0
DTYPES = (torch.float64, torch.float32)
# (kernel, storage shape, box, chunk, order, mirror, with a buoyancy)
STEPS = ([("m", s, b, c, 2, None, False) for s, b, c in CASES]
         + [("mh", s, b, c, o, mi, False) for o in (4, 8) for s, b, c, mi in STAR_CASES]
         + [("mb", s, b, c, 2, None, True) for s, b, c in CASES])


def _lap(u1, b, box, order, mirror, dtype):
    """The oracle's Laplacian on the box in ``dtype``, h2 cast to the working type like the kernel's."""
    from wave3d.ops import reference

    h2 = [_cast(v, u1.dtype) for v in H2]
    return reference._lap_box(u1.to(dtype), box, *h2, order, mirror, None if b is None else b.to(dtype))


def _step_case(shape, box, chunk, order, mirror, density, dtype, sponge, padded):
    from wave3d.ops import kernels

    u1, u2, m = _inputs(shape, dtype)
    b = _rand(shape, dtype, 4, 0.3, 2.0) if density else None
    h0 = _rand(shape, dtype, 6, -1.0, 1.0)
    tp = _tapers(shape, dtype) if sponge else None
    d = [_dense(t, padded) for t in (u1, u2, m)]
    kw = dict(first=False, h2=H2, stat_i=(box[0], box[1]), chunk=chunk, order=order, mirror=mirror,
              taper=None if tp is None else tuple(t.to(DEV) for t in tp),
              buoyancy=None if b is None else _dense(b, padded))

    def run(save, illum):
        u = _dense(torch.full(shape, SENT, dtype=dtype), padded)
        lap = _dense(torch.full(shape, SENT, dtype=dtype), padded) if save else None
        h = _dense(h0, padded) if illum else None
        st = kernels.new_err(1)
        kernels.step_medium(*d, u, box, stat=st, lap_out=lap, illum=h, **kw)
        return u, kernels.decode_err(st), lap, h

    plain, pstat, _, _ = run(False, False)
    saved, sstat, slap, _ = run(True, False)
    iu, istat, _, ih = run(False, True)
    su, sistat, silap, sih = run(True, True)
    torch.cuda.synchronize()
    # u, the statistic and lap_out are those of the plain step and of save mode, bit for bit
    assert float(_at(plain.cpu(), box).abs().max()) > 0
    assert torch.equal(saved, plain) and torch.equal(iu, plain) and torch.equal(su, plain)
    assert sstat == pstat and istat == pstat and sistat == pstat
    assert torch.equal(silap, slap)
    lap64 = _lap(u1, b, box, order, mirror, torch.float64)
    exp64 = _at(h0, box).double() + lap64 * lap64
    lap = _lap(u1, b, box, order, mirror, dtype)
    exp = _at(h0, box) + lap * lap
    mask = _box_mask(shape, box)
    for h in (ih, sih):
        got = h.cpu()
        if dtype == torch.float64:
            assert torch.equal(_at(got, box), exp)
        else:
            assert float((exp.double() - exp64).abs().max()) > 0  # fp32 rounds: the comparison is not trivial
        assert_same_bits(_at(got, box), exp)
        assert torch.equal(got[mask], h0[mask])  # outside the box h keeps its values: no wrap either
        if padded:  # and the padding between the rows its zeros
            base = h._base
            inside = torch.zeros(base.shape, dtype=torch.bool, device=DEV)
            inside.as_strided(h.shape, h.stride(), h.storage_offset()).fill_(True)
            assert bool((base[~inside] == 0).all())
    assert torch.equal(ih, sih)


@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(STEPS)), ids=[f"{s[0]}{s[4]}-{i}" for i, s in enumerate(STEPS)])
def test_illum_and_save_illum_steps(C, case, dtype, sponge):
    _step_case(*STEPS[case][1:], dtype, sponge, False)


@pytest.mark.parametrize("sponge", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_steps_on_padded_views(C, dtype, sponge):
    _step_case(*STEPS[2][1:], dtype, sponge, True)


def test_rejected_combinations(C):
    from wave3d.ops import kernels

    shape, box, _ = CASES[3]
    dt = torch.float64
    u1, u2, m = (t.to(DEV) for t in _inputs(shape, dt))
    b = _rand(shape, dt, 4, 0.3, 2.0).to(DEV)
    u, x, q, h, dm, db = (torch.zeros(shape, dtype=dt, device=DEV) for _ in range(6))
    kw = dict(h2=H2, stat=kernels.new_err(1), stat_i=(1, 4))

    def bad(match=None, first=False, **more):
        with pytest.raises(ValueError, match=match):
            kernels.step_medium(u1, u2, m, u, box, first=first, **kw, **more)

    bad("first", first=True, illum=h)
    bad("first", first=True, illum=h, lap_out=x)
    for v in ("plain", "r2", "r2nt"):
        bad("variant", illum=h, variant=v)
        bad("variant", illum=h, lap_out=x, variant=v)
    bad("combined", illum=h, image=(q, x))
    bad("combined", illum=h, born=(q, dm))
    bad("combined", illum=h, buoyancy=b, scatter=(x, dm, db))
    bad("combined", illum=h, buoyancy=b, born_add=q)
    for name, t in (("u", u), ("u1", u1), ("u2", u2), ("m", m)):
        bad(f"shares memory with {name}$", illum=t)
    bad("shares memory with buoyancy", illum=b, buoyancy=b)
    bad("shares memory with lap_out", illum=x, lap_out=x)
    bad(illum=h.float())                             # another dtype
    bad(illum=h[:-1])                                # another shape
    bad(illum=kernels.alloc_level(*shape, dt))       # other strides
    bad(illum=h.cpu())                               # not on the device
    bad(illum=[h])                                   # not a tensor
    # the launcher refuses them as well (the native entry point, past the Python checks)
    gv = [*shape, shape[2], shape[1] * shape[2]]
    args = [u1.data_ptr(), u2.data_ptr(), m.data_ptr(), u.data_ptr(), gv, [list(box)], 1, 4, [], list(H2),
            kw["stat"].data_ptr(), 0, torch.cuda.current_stream().cuda_stream]
    P = torch.Tensor.data_ptr
    IL, SI = C.medium_modes["illum"], C.medium_modes["save_illum"]
    native = [
        (True, IL, 1, dict(illum=P(h))),                                               # first
        (True, SI, 1, dict(illum=P(h), lap_out=P(x))),
        (False, IL, 0, dict(illum=P(h))),                                              # variants
        (False, IL, 2, dict(illum=P(h))),
        (False, SI, 3, dict(illum=P(h), lap_out=P(x))),
        (False, IL, 1, dict(illum=P(h), q=P(q), acc=P(x))),                            # image
        (False, IL, 1, dict(illum=P(h), q=P(q), dm=P(dm))),                            # Born
        (False, IL, 1, dict(illum=P(h), b=P(b), s_out=P(x), dm=P(dm), db=P(db))),      # scatter
        (False, IL, 1, dict(illum=P(h), b=P(b), sadd=P(q))),                           # Born-add
        (False, C.medium_modes["image"], 1, dict(illum=P(h), q=P(q), acc=P(x))),       # the same under their modes
        (False, C.medium_modes["born"], 1, dict(illum=P(h), q=P(q), dm=P(dm))),
        (False, C.medium_modes["scatter"], 1, dict(illum=P(h), b=P(b), s_out=P(x), dm=P(dm), db=P(db))),
        (False, C.medium_modes["born_add"], 1, dict(illum=P(h), b=P(b), sadd=P(q))),
        (False, IL, 1, dict(illum=P(u))),                                              # shared memory
        (False, IL, 1, dict(illum=P(u1))),
        (False, IL, 1, dict(illum=P(u2))),
        (False, IL, 1, dict(illum=P(m))),
        (False, IL, 1, dict(illum=P(b), b=P(b))),
        (False, SI, 1, dict(illum=P(x), lap_out=P(x))),
        (False, IL, 1, dict(illum=P(u1) + 8 * shape[2])),                              # partly
    ]
    for first, mode, variant, grids in native:
        with pytest.raises(C.Wave3dError):
            C.k_step_medium_f64(first, *args, mode, variant=variant, **grids)
    torch.cuda.synchronize()
    assert not bool(u.any()) and not bool(x.any()) and not bool(h.any())  # nothing was launched


# ---- end to end ------------------------------------------------------------------------------

def _variant(prob, kind, dtype="fp64"):
    """The problem of _problem() at another space order, with a density, or in another dtype."""
    import wave3d

    N = prob.N
    kw = dict(T=prob.T, timesteps=prob.timesteps, dtype=dtype)
    if kind == "order8":
        kw["space_order"] = 8
    if kind == "density":
        g = torch.Generator().manual_seed(29)
        rho = 1 + 0.5 * torch.rand((N + 1,) * 3, generator=g, dtype=torch.float64)
        rho[N] = rho[0]
        kw["density"] = rho
    return wave3d.MediumProblem(N, prob.speed2, **kw)


E2E = [(20, 24, True, "order2"), (70, 16, False, "order2"), (20, 24, True, "order8"), (20, 24, True, "density")]
_cache = {}


def _oracle(N, K, sponge, kind):
    """The problem, its keywords, the observed traces and the "cpu" results, computed once."""
    import wave3d

    key = (N, K, sponge, kind)
    if key not in _cache:
        prob, kw, obs = _problem(N, K, sponge)
        prob = _variant(prob, kind)
        ref = wave3d.MediumSolver(prob, "cpu", **kw).gradient(obs, illumination=True)
        _cache[key] = prob, kw, obs, ref
    return _cache[key]


@pytest.mark.parametrize("N,K,sponge,kind", E2E)
def test_gradient_illumination_matches_oracle_fp64(C, N, K, sponge, kind):
    import wave3d

    prob, kw, obs, ref = _oracle(N, K, sponge, kind)
    sol = wave3d.MediumSolver(prob, "hip", **kw)
    got = sol.gradient(obs, illumination=True)
    off = sol.gradient(obs)
    assert float(ref.illumination.max()) > 0 and float(ref.pseudo_hessian_speed2.max()) > 0
    assert torch.equal(got.illumination, ref.illumination)
    assert torch.equal(got.pseudo_hessian_speed2, ref.pseudo_hessian_speed2)
    assert torch.equal(got.illumination[N], got.illumination[0])
    # the flag changes nothing else
    assert off.illumination is None and off.pseudo_hessian_speed2 is None
    assert got.misfit == off.misfit
    assert torch.equal(got.grad_speed2, off.grad_speed2) and torch.equal(got.grad_speed2, ref.grad_speed2)
    assert torch.equal(got.grad_wavelet, off.grad_wavelet)
    assert torch.equal(got.traces, off.traces)
    assert got.extra["illumination"] is True and off.extra["illumination"] is False
    dens = kind == "density"
    assert got.extra["levels"] == wave3d.gradient_levels(K, got.extra["segment"], density=dens, illumination=True)
    assert got.extra["levels"] == off.extra["levels"] + 1 and got.extra["segment"] == off.extra["segment"]


def test_illumination_segment_invariance(C):
    import wave3d

    N, K = 20, 24
    prob, kw, obs, ref = _oracle(N, K, True, "order2")
    sol = wave3d.MediumSolver(prob, "hip", **kw)
    for seg in (1, 5, 23, None):
        got = sol.gradient(obs, segment=seg, illumination=True)
        assert torch.equal(got.illumination, ref.illumination)
        assert torch.equal(got.pseudo_hessian_speed2, ref.pseudo_hessian_speed2)
        assert torch.equal(got.grad_speed2, ref.grad_speed2)
        s = got.extra["segment"]
        assert seg is None or s == seg
        assert got.extra["levels"] == wave3d.gradient_levels(K, s, illumination=True)
        last = (K - 1) % s or min(s, K - 1)
        assert got.extra["recomputed_steps"] == (K - 1) - last


def test_density_gradient_and_gauss_newton_carry_the_illumination(C):
    import wave3d

    N, K = 20, 24
    prob, kw, obs, ref = _oracle(N, K, True, "density")
    sol = wave3d.MediumSolver(prob, "hip", **kw)
    both = sol.gradient(obs, wrt_density=True, illumination=True, segment=5)
    assert torch.equal(both.illumination, ref.illumination)
    assert torch.equal(both.grad_density, sol.gradient(obs, wrt_density=True, segment=5).grad_density)
    assert both.extra["levels"] == wave3d.gradient_levels(K, 5, density=True, wrt_density=True, illumination=True)
    gn = sol.gauss_newton(0.01 * prob.speed2, illumination=True)
    assert torch.equal(gn.illumination, ref.illumination)  # the background field's, whatever the residuals
    assert torch.equal(gn.pseudo_hessian_speed2, ref.pseudo_hessian_speed2)


def test_illumination_fp32(C):
    import wave3d

    prob, kw, obs, ref = _oracle(20, 24, True, "order2")
    p32 = _variant(prob, "order2", "fp32")
    cpu = wave3d.MediumSolver(p32, "cpu", **kw).gradient(obs, illumination=True)
    hip = wave3d.MediumSolver(p32, "hip", **kw).gradient(obs, illumination=True)
    for name in ("illumination", "pseudo_hessian_speed2"):
        g, c, r = getattr(hip, name), getattr(cpu, name), getattr(ref, name)
        assert g.dtype == torch.float32
        bound = 4 * float((c.double() - r).abs().max())
        err = float((g.double() - r).abs().max())
        print(f"fp32 {name}: max |hip - oracle64| {err:.3e}, bound {bound:.3e}")
        assert bound > 0 and err <= bound


def test_variant_is_refused(C):
    import wave3d

    prob, kw, obs, _ = _oracle(20, 24, True, "order2")
    with pytest.raises(ValueError, match="variant"):
        wave3d.MediumSolver(prob, "hip", variant="plain", **kw).gradient(obs, illumination=True)
