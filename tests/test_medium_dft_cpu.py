"""On-the-fly Fourier transforms of the medium solver on the CPU (ops/reference.py dft_tables,
dft_accumulate, solve_medium(frequencies=), gradient_medium_dft, finish_gradient_dft) and their front end
(MediumSolver.run(frequencies=), gradient_dft, dft_bins, gradient_dft_levels): the twiddle tables
against math.cos / math.sin, the spectra against their definition from a run that keeps every level,
Parseval's identity against gradient_medium, the band limit, the input checks and the level count.
"""
import math

import pytest
import torch

F64, F32 = torch.float64, torch.float32
EPS = 2.0 ** -53


def _ulp_apart(a: float, b: float) -> bool:
    """Equal, or neighbours in float64."""
    return a == b or b in (math.nextafter(a, math.inf), math.nextafter(a, -math.inf))


# ---- twiddle tables ------------------------------------------------------------------------------

def test_twiddles_match_libm():
    from wave3d.ops import reference

    freqs, idx, tau = [0.0, 0.37, 2.5, 11.0], [0, 1, 2, 7, 40, 1000], 0.0123
    c, s = reference.dft_tables(freqs, idx, tau, F64)
    assert c.shape == s.shape == (len(idx), len(freqs)) and c.dtype == s.dtype == F64
    for r, p in enumerate(idx):
        for q, f in enumerate(freqs):
            a = ((2 * math.pi * f) * p) * tau
            assert _ulp_apart(c[r, q].item(), math.cos(a)), (p, f)
            assert _ulp_apart(s[r, q].item(), -math.sin(a)), (p, f)
    # row 0 and the zero frequency: (1, -0) or (1, 0)
    assert bool((c[0] == 1).all()) and bool((s[0] == 0).all())
    assert bool((c[:, 0] == 1).all()) and bool((s[:, 0] == 0).all())
    # the cast comes after the float64 evaluation
    c32, s32 = reference.dft_tables(freqs, idx, tau, F32)
    assert c32.dtype == s32.dtype == F32
    assert torch.equal(c32, c.to(F32)) and torch.equal(s32, s.to(F32))
    a32 = ((2 * math.pi * torch.tensor(freqs, dtype=F32))[None, :] * torch.tensor(idx, dtype=F32)[:, None]) * tau
    assert not torch.equal(c32, torch.cos(a32))  # an evaluation in float32 differs


def test_accumulate_keeps_everything_outside_the_box():
    from wave3d.ops import reference

    g = torch.Generator().manual_seed(3)
    shape, box = (6, 7, 9), (1, 4, 2, 5, 1, 6)
    u = torch.rand(shape, generator=g, dtype=F64)
    re = [torch.rand(shape, generator=g, dtype=F64) for _ in range(2)]
    im = [torch.rand(shape, generator=g, dtype=F64) for _ in range(2)]
    re0, im0, u0 = [t.clone() for t in re], [t.clone() for t in im], u.clone()
    c, s = reference.dft_tables([1.0, 3.0], [5], 0.01, F64)
    reference.dft_accumulate(re, im, u, box, c[0], s[0])
    sl = (slice(1, 5), slice(2, 6), slice(1, 7))
    mask = torch.ones(shape, dtype=torch.bool)
    mask[sl] = False
    for f in range(2):
        assert torch.equal(re[f][sl], re0[f][sl] + u[sl] * c[0, f]) and torch.equal(re[f][mask], re0[f][mask])
        assert torch.equal(im[f][sl], im0[f][sl] + u[sl] * s[0, f]) and torch.equal(im[f][mask], im0[f][mask])
    assert torch.equal(u, u0)
    with pytest.raises(ValueError):
        reference.dft_accumulate(re, im[:1], u, box, c[0], s[0])
    with pytest.raises(ValueError):
        reference.dft_accumulate([], [], u, box, c[0, :0], s[0, :0])


# ---- the spectra against their definition ----------------------------------------------------------

N, K = 8, 12
SOURCES = [(0, 4, 5), (5, 3, 2)]
RECEIVERS = [(N, 6, 3), (4, 5, 5)]
FREQS = [0.0, 0.8, 2.3]


def _speed2(n, seed=7):
    g = torch.Generator().manual_seed(seed)
    s = 0.3 * (1 + 0.2 * torch.rand((n + 1,) * 3, generator=g, dtype=F64))
    s[:, :, n // 2:] *= 1.5
    s[n] = s[0]
    return s


def _solve_kw(n=N, k=K):
    import wave3d

    prob = wave3d.MediumProblem(n, _speed2(n), timesteps=k)
    w = torch.stack([wave3d.ricker(3.0, 0.3, k, prob.tau), -0.5 * wave3d.ricker(2.0, 0.2, k, prob.tau)], 1)
    return prob, dict(sources=SOURCES, wavelet=w, receivers=RECEIVERS, taper=wave3d.sponge_taper(prob, 2))


def _all_levels(prob, kw, dtype):
    """u^0 .. u^K on the planes 0 .. N, from a run that keeps every level."""
    from wave3d.ops import reference

    n, k = prob.N, prob.timesteps
    _, levels = reference.forward_medium_autograd(n, k, prob.speed2, dtype=dtype, keep_levels=True, **kw)
    final = reference.solve_medium(n, k, prob.speed2, dtype=dtype, **kw)[1]
    return [torch.zeros((n + 1,) * 3, dtype=dtype)] + [lv[1:n + 2] for lv in levels] + [final]


@pytest.mark.parametrize("every", [1, 3])
def test_spectra_match_the_definition_fp64(every):
    from wave3d.ops import reference

    prob, kw = _solve_kw()
    tr, uf, mx, spec = reference.solve_medium(N, K, prob.speed2, frequencies=FREQS, dft_every=every, **kw)
    assert spec.shape == (len(FREQS),) + (N + 1,) * 3 and spec.dtype == torch.complex128
    levels = _all_levels(prob, kw, F64)
    assert len(levels) == K + 1 and torch.equal(levels[K], uf)
    want = torch.zeros_like(spec)
    for n in range(0, K + 1, every):
        for q, f in enumerate(FREQS):
            a = 2 * math.pi * f * n * prob.tau
            want[q] += levels[n] * complex(math.cos(a), -math.sin(a))
    umax = max(float(lv.abs().max()) for lv in levels)
    tol = 4 * (K + 1) * EPS * umax  # each of the at most K + 1 adds and products rounds once
    dre, dim = float((spec.real - want.real).abs().max()), float((spec.imag - want.imag).abs().max())
    print("every", every, "max |u|", umax, "deviation re", dre, "im", dim, "tolerance", tol)
    assert umax > 0 and float(want.abs().max()) > 0.1 * umax
    assert dre <= tol and dim <= tol
    # the Dirichlet faces are 0, and the zero frequency has no imaginary part
    for face in (spec[:, :, 0], spec[:, :, N], spec[:, :, :, 0], spec[:, :, :, N]):
        assert float(face.abs().max()) == 0.0
    assert float(spec[0].imag.abs().max()) == 0.0
    # the other results do not change by a bit
    tr0, uf0, mx0 = reference.solve_medium(N, K, prob.speed2, **kw)
    assert torch.equal(tr, tr0) and torch.equal(uf, uf0) and mx == mx0


@pytest.mark.parametrize("every", [1, 3])
def test_spectra_fp32_are_the_fp32_definition_bit_for_bit(every):
    from wave3d.ops import reference

    prob, kw = _solve_kw()
    spec = reference.solve_medium(N, K, prob.speed2, dtype=F32, frequencies=FREQS, dft_every=every, **kw)[3]
    assert spec.dtype == torch.complex64
    levels = _all_levels(prob, kw, F32)
    c, s = reference.dft_tables(FREQS, range(K + 1), prob.tau, F32)
    own = (slice(None), slice(1, N), slice(1, N))
    for q in range(len(FREQS)):
        re, im = torch.zeros((N + 1,) * 3, dtype=F32), torch.zeros((N + 1,) * 3, dtype=F32)
        for n in range(0, K + 1, every):
            re[own] = re[own] + levels[n][own] * c[n, q]
            im[own] = im[own] + levels[n][own] * s[n, q]
        assert torch.equal(spec[q].real, re) and torch.equal(spec[q].imag, im)
    assert float(spec.abs().max()) > 0


def test_level_zero_is_the_initial_field():
    """K = 1 with a given u0: the spectrum is u^0 + u^1 w."""
    from wave3d.ops import reference

    n, f = 8, 1.7
    g = torch.Generator().manual_seed(11)
    u0 = torch.zeros((n + 1,) * 3, dtype=F64)
    u0[:, 1:n, 1:n] = torch.rand((n + 1, n - 1, n - 1), generator=g, dtype=F64)
    u0[n] = u0[0]
    _, uf, _, spec = reference.solve_medium(n, 1, 0.01, u0=u0, frequencies=[f], T=0.05)
    tau = reference.tables(n, 1, T=0.05)[4]["tau"]
    c, s = reference.dft_tables([f], [0, 1], tau, F64)
    own = (slice(None), slice(1, n), slice(1, n))
    assert torch.equal(spec[0].real[own], (0 + u0[own] * c[0, 0]) + uf[own] * c[1, 0])
    assert torch.equal(spec[0].imag[own], (0 + u0[own] * s[0, 0]) + uf[own] * s[1, 0])


# ---- dft_bins and Parseval's identity ----------------------------------------------------------------

@pytest.mark.parametrize("k,every,pairs,P", [(8, 1, True, 7), (8, 1, False, 9), (9, 1, True, 8), (20, 1, True, 19),
                                             (13, 2, True, 6), (13, 3, False, 5)])
def test_dft_bins_satisfy_parseval(k, every, pairs, P):
    import wave3d

    prob = wave3d.MediumProblem(8, 0.01, timesteps=k)
    f, w = wave3d.dft_bins(prob, every=every, pairs=pairs)
    assert f.dtype == w.dtype == F64 and f.shape == w.shape == (P // 2 + 1,)
    assert torch.equal(f, torch.arange(P // 2 + 1, dtype=F64) / (P * every * prob.tau))
    want = torch.full((P // 2 + 1,), 2.0 / P, dtype=F64)
    want[0] = 1.0 / P
    if P % 2 == 0:
        want[-1] = 1.0 / P
    assert torch.equal(w, want)
    idx = list(range(every, k, every)) if pairs else list(range(0, k + 1, every))
    assert len(idx) == P
    g = torch.Generator().manual_seed(P)
    a, b = torch.rand(P, generator=g, dtype=F64) - 0.5, torch.rand(P, generator=g, dtype=F64) - 0.5
    from wave3d.ops import reference

    c, s = reference.dft_tables(f, idx, prob.tau, F64)
    A, B = torch.complex(a @ c, a @ s), torch.complex(b @ c, b @ s)
    lhs, rhs = float((a * b).sum()), float((w * (A.real * B.real + A.imag * B.imag)).sum())
    assert abs(lhs - rhs) <= 1e-13 * float(a.abs().sum())


KP = 13
PARSEVAL_TOL = min(4 * 1.25e-15, 1e-12)  # four times the oracle-side measurement, capped (see the Parseval test)
OFFGRID = [[2.4, 5.1, 3.3], [7.6, 2.0, 6.5]]


def _layered_density(n):
    rho = torch.ones((n + 1,) * 3, dtype=F64)
    rho[:, :, n // 2:] = 2.5
    rho[:, n // 3:, :] *= 1.3
    return rho


def _parseval_case(name):
    import wave3d

    n, order, density, offgrid = dict(plain=(8, 2, None, False), density=(8, 2, _layered_density(8), True),
                                      order8=(10, 8, None, False))[name]
    speed2 = _speed2(n)
    if order == 8:
        speed2 = speed2 * 0.5
    prob = wave3d.MediumProblem(n, speed2, timesteps=KP, space_order=order, density=density)
    w = torch.stack([wave3d.ricker(3.0, 0.3, KP, prob.tau), -0.5 * wave3d.ricker(2.0, 0.2, KP, prob.tau)], 1)
    kw = dict(sources=SOURCES, wavelet=w, taper=wave3d.sponge_taper(prob, 2), order=order, density=density)
    if offgrid:
        kw["receiver_positions"] = torch.tensor(OFFGRID, dtype=F64)
    else:
        kw["receivers"] = [(n, 6, 3), (4, 5, 5), (2, 1, n - 1)]
    return prob, kw


@pytest.fixture(scope="module", params=["plain", "density", "order8"])
def parseval(request):
    from wave3d.ops import reference

    prob, kw = _parseval_case(request.param)
    n = prob.N
    observed = reference.solve_medium(n, KP, prob.speed2 * 1.1, **kw)[0]
    return dict(name=request.param, prob=prob, kw=kw, observed=observed,
                time=reference.gradient_medium(n, KP, prob.speed2, observed, **kw))


def test_full_spectrum_reproduces_the_time_domain_gradient(parseval):
    """Parseval: with every bin of the half spectrum of the K - 1 = 12 pairs, gradient_medium_dft gives
    gradient_medium's grad_speed2 up to rounding, and its other results bit for bit.

    Measured on this oracle in fp64, max |delta| / max |grad|: 1.25e-15 (plain), 5.7e-17 (layered density,
    off-grid receivers), 6.4e-16 (order 8); with dft_every = 2 against the restricted time sum 5.9e-16
    (the test below). The assertion is four times the largest, PARSEVAL_TOL = 5.0e-15, far inside the cap
    of 1e-12 above which the pairing index or the weights would be wrong."""
    import wave3d
    from wave3d.ops import reference

    prob, kw = parseval["prob"], parseval["kw"]
    f, w = wave3d.dft_bins(prob, every=1, pairs=True)
    assert f.numel() == (KP - 1) // 2 + 1
    J, gs, gw, tr = reference.gradient_medium_dft(prob.N, KP, prob.speed2, parseval["observed"], f, weights=w, **kw)
    J0, gs0, gw0, tr0 = parseval["time"]
    dev = float((gs - gs0).abs().max()) / float(gs0.abs().max())
    print(parseval["name"], "max |delta| / max |grad| =", dev, "max |grad|", float(gs0.abs().max()))
    assert J0 > 0 and float(gs0.abs().max()) > 0
    assert dev <= PARSEVAL_TOL
    assert J == J0 and torch.equal(gw, gw0) and torch.equal(tr, tr0)
    assert torch.equal(gs[prob.N], gs[0]) and float(gs[:, 0].abs().max()) == 0.0


def test_every_second_pair_matches_the_restricted_time_sum():
    """dft_every = 2: the identity holds against the time-domain sum over the even pair indices, formed
    here from forward_medium_autograd(keep_lap=True) and an adjoint loop written out."""
    import wave3d
    from wave3d.ops import reference

    prob, kw = _parseval_case("plain")
    n = prob.N
    observed = reference.solve_medium(n, KP, prob.speed2 * 1.1, **kw)[0]
    f, w = wave3d.dft_bins(prob, every=2, pairs=True)
    assert f.numel() == 4  # P = 6 pairs: p = 2, 4, .., 12
    J, gs, gw, tr = reference.gradient_medium_dft(n, KP, prob.speed2, observed, f, weights=w, dft_every=2, **kw)

    c = reference.tables(n, KP)[4]
    traces, laps = reference.forward_medium_autograd(n, KP, prob.speed2, keep_lap=True, **kw)
    _, res = reference.misfit_medium(traces, observed)
    tt = reference.taper_tables(kw["taper"], n, F64)
    m = reference.medium_coefficient(prob.speed2, c["tau"], n, F64)
    g = reference.source_table(kw["wavelet"], KP, 2, c["hx"], c["hy"], c["hz"], F64)
    anodes, atab = reference.adjoint_source_table(res, kw["receivers"], n, tt)
    snodes = reference.source_unique_nodes(SOURCES, n)
    shape, box = (n + 3, n + 1, n + 1), (1, n + 1, 1, n - 1, 1, n - 1)
    own = (slice(1, n + 2), slice(1, n), slice(1, n))
    a = torch.zeros(KP, 2, dtype=F64)

    def finish(mu, k):
        for e, nd in enumerate(anodes):
            mu[nd] = mu[nd] + m[nd] * atab[k, e]
        reference._wrap_x(mu, n)
        for q, nd in enumerate(snodes):
            a[k - 1, q] = mu[nd]

    mu2, mu1 = torch.zeros(shape, dtype=F64), torch.zeros(shape, dtype=F64)
    finish(mu1, KP)
    acc = torch.zeros(shape, dtype=F64)
    for k in range(KP - 1, 0, -1):
        if k % 2 == 0:
            acc[own] = acc[own] + mu1[own] * laps[k - 1]
        vals = reference.step_medium(mu1, mu2, m, box, first=False, hx2=c["hx2"], hy2=c["hy2"], hz2=c["hz2"], taper=tt)
        mu = torch.zeros(shape, dtype=F64)
        mu[own] = vals
        finish(mu, k)
        mu2, mu1 = mu1, mu
    want, gw0 = reference.finish_gradient_medium(acc, a, g, m, tt, SOURCES, n, c["tau"], c["hx"], c["hy"], c["hz"])
    dev = float((gs - want).abs().max()) / float(want.abs().max())
    print("every 2: max |delta| / max |grad| =", dev)
    assert dev <= PARSEVAL_TOL and torch.equal(gw, gw0)
    # and it is not the full sum
    full = reference.gradient_medium(n, KP, prob.speed2, observed, **kw)[1]
    assert float((gs - full).abs().max()) > 1e-3 * float(full.abs().max())


def test_band_limit_and_default_weights(parseval):
    import wave3d
    from wave3d.ops import reference

    prob, kw, obs = parseval["prob"], parseval["kw"], parseval["observed"]
    f, w = wave3d.dft_bins(prob, every=1, pairs=True)
    h = f.numel() // 2
    low = reference.gradient_medium_dft(prob.N, KP, prob.speed2, obs, f[:h], weights=w[:h], **kw)
    full = parseval["time"]
    # half of the bins: another gradient, so `frequencies` cannot be ignored
    assert float((low[1] - full[1]).abs().max()) > 1e-3 * float(full[1].abs().max())
    assert low[0] == full[0] and torch.equal(low[2], full[2]) and torch.equal(low[3], full[3])
    # weights=None is explicit ones, bit for bit
    ones = reference.gradient_medium_dft(prob.N, KP, prob.speed2, obs, f[:h], weights=torch.ones(h), **kw)
    none = reference.gradient_medium_dft(prob.N, KP, prob.speed2, obs, f[:h], **kw)
    assert torch.equal(ones[1], none[1]) and not torch.equal(none[1], low[1])


# ---- the front end on the "cpu" backend ---------------------------------------------------------------

def _front(backend="cpu", **kw):
    import wave3d

    prob, skw = _solve_kw()
    return wave3d.MediumSolver(prob, backend, **skw, **kw)


def test_run_with_frequencies_on_the_cpu_backend():
    from wave3d.ops import reference

    sol = _front()
    plain = sol.run()
    assert plain.spectra is None and "frequencies" not in plain.extra
    r = sol.run(frequencies=FREQS, dft_every=3)
    prob, kw = _solve_kw()
    want = reference.solve_medium(N, K, prob.speed2, frequencies=FREQS, dft_every=3, **kw)
    assert torch.equal(r.spectra, want[3]) and r.spectra.device.type == "cpu"
    assert torch.equal(r.traces, plain.traces) and torch.equal(r.u_final, plain.u_final)
    assert r.max_abs_u == plain.max_abs_u
    assert r.extra["frequencies"] == FREQS and r.extra["dft_every"] == 3 and r.extra["dft_samples"] == 5


def test_gradient_dft_on_the_cpu_backend():
    import wave3d
    from wave3d.ops import reference

    sol = _front()
    prob, kw = _solve_kw()
    observed = reference.solve_medium(N, K, prob.speed2 * 1.1, **kw)[0]
    f, w = wave3d.dft_bins(prob, every=1, pairs=True)
    got = sol.gradient_dft(observed, f, weights=w)
    want = reference.gradient_medium_dft(N, K, prob.speed2, observed, f, weights=w, **kw)
    time = sol.gradient(observed)
    assert got.misfit == want[0] == time.misfit
    assert torch.equal(got.grad_speed2, want[1]) and torch.equal(got.grad_wavelet, want[2])
    assert torch.equal(got.grad_wavelet, time.grad_wavelet) and torch.equal(got.traces, time.traces)
    assert float((got.grad_speed2 - time.grad_speed2).abs().max()) <= 1e-12 * float(time.grad_speed2.abs().max())
    e = got.extra
    assert e["recomputed_steps"] == 0 and e["dft_every"] == 1 and e["dft_samples"] == K - 1
    assert e["frequencies"] == f.tolist() and e["levels"] is None
    assert got.grad_density is None and got.illumination is None


def test_input_checks():
    import wave3d

    sol = _front()
    obs = torch.zeros(K + 1, len(RECEIVERS), dtype=F64)
    bad_freqs = ([], [[1.0, 2.0]], 1.0, [1.0, -0.5], [math.nan], [math.inf], ["a"])
    for bad in bad_freqs:
        with pytest.raises(ValueError, match="frequencies"):
            sol.run(frequencies=bad)
        with pytest.raises(ValueError, match="frequencies"):
            sol.gradient_dft(obs, bad)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="dft_every"):
            sol.run(frequencies=[1.0], dft_every=bad)
        with pytest.raises(ValueError, match="dft_every"):
            sol.gradient_dft(obs, [1.0], dft_every=bad)
        with pytest.raises(ValueError, match="dft_every"):
            wave3d.dft_bins(sol.problem, every=bad)
    for bad in ([1.0], [1.0, 2.0, 3.0], [1.0, math.nan], [1.0, math.inf], [[1.0, 1.0]]):
        with pytest.raises(ValueError, match="weights"):
            sol.gradient_dft(obs, [1.0, 2.0], weights=bad)
    # no pair to correlate: the pairs are p = e, 2e, ... <= K - 1
    sol.gradient_dft(obs, [1.0], dft_every=K - 1)
    with pytest.raises(ValueError, match="no pair"):
        sol.gradient_dft(obs, [1.0], dft_every=K)
    with pytest.raises(ValueError, match="dft_every"):
        wave3d.dft_bins(sol.problem, every=K, pairs=True)
    assert wave3d.dft_bins(sol.problem, every=K)[0].numel() == 2  # run() samples n = 0 and K
    # gradient()'s preconditions, and variant None
    with pytest.raises(ValueError, match="observed"):
        sol.gradient_dft(obs[:-1], [1.0])
    with pytest.raises(ValueError, match="variant"):
        _front(variant="plain").gradient_dft(obs, [1.0])
    prob, kw = _solve_kw()
    with pytest.raises(ValueError, match="receiver"):
        wave3d.MediumSolver(prob, "cpu", sources=SOURCES, wavelet=kw["wavelet"]).gradient_dft(obs[:, :0], [1.0])
    with pytest.raises(ValueError, match="rest"):
        _front(u0=torch.zeros((N + 1,) * 3)).gradient_dft(obs, [1.0])
    with pytest.raises(TypeError):
        sol.gradient_dft(obs, [1.0], wrt_density=True)
    with pytest.raises(TypeError):
        sol.gradient_dft(obs, [1.0], illumination=True)


def test_level_count():
    import wave3d

    assert wave3d.gradient_dft_levels(1) == 9
    assert wave3d.gradient_dft_levels(2, density=False) == 13
    assert wave3d.gradient_dft_levels(4, density=True) == 22
    with pytest.raises(ValueError):
        wave3d.gradient_dft_levels(0)
