"""Variable-speed medium front-end: ``(1/c^2) u_tt = lap u + f`` with point sources and receivers,
or with a density model ``(1/(rho c^2)) u_tt = div((1/rho) grad u) + f``.

``MediumProblem`` describes the box, the grid and the squared wave speed c^2(x, y, z) on the
constant-speed solver's grid (``N+1`` nodes per axis, periodic in x with planes 0 and N both
stencil points, Dirichlet 0 on the y/z faces, zero initial velocity); ``MediumSolver`` runs it on
one GPU through the HIP kernels of ``csrc/hip_medium.hip`` or on the PyTorch oracle
(``ops.reference.solve_medium``).
"""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass, field
from typing import Any

import torch

from .wave import PI_REF

_DTYPES = {"fp64": torch.float64, "fp32": torch.float32}
_ORDERS = (2, 4, 8)


def cfl_limit(order: int = 2) -> float:
    """Largest stable Courant number ``c_max tau / h_min`` of the leapfrog with the star Laplacian
    of space ``order`` (2, 4 or 8): ``2 / sqrt(3 S)`` with ``S = |c_0| + 2 sum |c_d|`` over the
    stencil weights: 1/sqrt(3) = 0.5774 (order 2), 0.5 (4), 0.4529 (8)."""
    from ..ops import reference

    return reference.cfl_limit(order)


class MediumProblem:
    """N intervals per axis, ``speed2`` = c^2 as a float or an ``(N+1)^3`` array/tensor.

    ``space_order``: 2 (the 7-point Laplacian, the default), 4 or 8 (star stencils of half-width
    M = order / 2 with odd reflection at the Dirichlet faces; needs N >= 2 M). The stability limit
    of the Courant number depends on it (:func:`cfl_limit`).

    ``density``: rho as a float or an ``(N+1)^3`` array/tensor, finite, > 0 and periodic in x
    (``space_order`` 2 only). The equation becomes ``(1/kappa) u_tt = div(b grad u) + f`` with the bulk
    modulus ``kappa = rho c^2`` and the buoyancy ``b = 1/rho`` (``ops.reference.laplace_density``), so
    impedance contrasts reflect. The Courant number is then ``sqrt(max_i kappa_i bhat_i) tau / h_min``
    over the stencil nodes, ``bhat_i`` the largest of node i's six face buoyancies; by Gershgorin the
    limit 1/sqrt(3) stays sufficient. A scalar density leaves it at ``c_max tau / h_min``. None: the
    constant-density solver, unchanged."""

    def __init__(self, N: int, speed2, Lx: Any = "pi", Ly: Any = "pi", Lz: Any = "pi", T: float = 1.0,
                 timesteps: int = 20, dtype: str = "fp64", pi: str = "ref", strict_cfl: bool = True,
                 space_order: int = 2, density=None):
        if dtype not in _DTYPES:
            raise ValueError(f"dtype must be fp64 or fp32, not {dtype!r}")
        if N < 2 or timesteps < 1:
            raise ValueError(f"need N >= 2 and timesteps >= 1, not N={N} timesteps={timesteps}")
        if space_order not in _ORDERS:
            raise ValueError(f"space_order must be 2, 4 or 8, not {space_order!r}")
        if N < space_order:
            raise ValueError(f"space_order {space_order} needs N >= {space_order}, not N={N}")
        self.space_order = int(space_order)
        self.cfl_limit = cfl_limit(self.space_order)
        self.N, self.Lx, self.Ly, self.Lz = int(N), Lx, Ly, Lz
        self.T, self.timesteps, self.dtype, self.pi = float(T), int(timesteps), dtype, pi
        s = self._field(speed2, "speed2")
        self.speed2 = s
        self.max_speed2 = float(s.max())
        self.density = None
        self._cfl_speed2 = self.max_speed2  # (Courant number h_min / tau)^2
        if density is not None:
            if self.space_order != 2:
                raise ValueError(f"density needs space_order 2, not {self.space_order}")
            self.density = self._field(density, "density")
            if self.density.dim() != 0:
                self._cfl_speed2 = self._max_kappa_bhat()
        if self.courant > self.cfl_limit:
            msg = (f"Courant number {self.courant:.4g} exceeds the stability limit {self.cfl_limit:.4g} of space "
                   f"order {self.space_order}: "
                   f"needs timesteps >= {self.min_stable_timesteps()}")
            if strict_cfl:
                raise ValueError(msg)
            warnings.warn(msg, RuntimeWarning, stacklevel=2)

    def _field(self, v, name: str) -> torch.Tensor:
        """A model field as a float64 CPU tensor: a scalar or ``(N+1)^3``, finite, > 0, periodic in x."""
        s = torch.as_tensor(v, dtype=torch.float64).cpu()
        n1 = self.N + 1
        if s.dim() != 0 and tuple(s.shape) != (n1, n1, n1):
            raise ValueError(f"{name} must be a scalar or have shape {(n1, n1, n1)}, not {tuple(s.shape)}")
        bad = ~(torch.isfinite(s) & (s > 0))
        if bool(bad.any()):
            v = s[bad].flatten()[0].item() if s.dim() else s.item()
            raise ValueError(f"{name} must be finite and > 0, found {v}")
        if s.dim() != 0 and not torch.equal(s[0], s[self.N]):
            j, k = (int(x) for x in (s[0] != s[self.N]).nonzero()[0])
            raise ValueError(f"{name} must be periodic in x: {name}[0,{j},{k}] = {s[0, j, k].item()} but "
                             f"{name}[{self.N},{j},{k}] = {s[self.N, j, k].item()}")
        return s

    def _max_kappa_bhat(self) -> float:
        """``max_i kappa_i bhat_i`` over the stencil nodes (every x plane, j and k in 1..N-1): kappa =
        speed2 rho, bhat_i = the largest of node i's six face buoyancies, a face buoyancy being the mean
        of its two nodes' 1/rho (x periodic: planes 0 and N are one plane)."""
        N = self.N
        rho = self.density
        b = 1.0 / rho
        bs = torch.cat([b[N - 1:N], b, b[1:2]])  # x ghost planes
        own = (slice(1, N + 2), slice(1, N), slice(1, N))
        nb = None
        for axis in range(3):
            for d in (-1, 1):
                sl = list(own)
                sl[axis] = slice(own[axis].start + d, own[axis].stop + d)
                nb = bs[tuple(sl)] if nb is None else torch.maximum(nb, bs[tuple(sl)])
        bhat = 0.5 * (bs[own] + nb)
        kappa = (self.speed2 * rho).expand(N + 1, N + 1, N + 1)[:, 1:N, 1:N]
        return float((kappa * bhat).max())

    def _pi(self) -> float:
        return PI_REF if self.pi == "ref" else math.pi

    def lengths(self) -> tuple[float, float, float]:
        p = self._pi()
        return tuple(p if v == "pi" else float(v) for v in (self.Lx, self.Ly, self.Lz))

    @property
    def tau(self) -> float:
        return self.T / self.timesteps

    @property
    def courant(self) -> float:
        return math.sqrt(self._cfl_speed2) * self.tau / (min(self.lengths()) / self.N)

    def stable(self) -> bool:
        return self.courant <= self.cfl_limit

    def min_stable_timesteps(self) -> int:
        k = math.ceil(math.sqrt(self._cfl_speed2) * self.T * self.N / (min(self.lengths()) * self.cfl_limit))
        # the quotient may round down onto the limit while the Courant number rounds up past it
        while math.sqrt(self._cfl_speed2) * (self.T / k) / (min(self.lengths()) / self.N) > self.cfl_limit:
            k += 1
        return k

    @property
    def points(self) -> int:
        return (self.N + 1) ** 3

    @property
    def torch_dtype(self):
        return _DTYPES[self.dtype]


def ricker(f0: float, t0: float, K: int, tau: float) -> torch.Tensor:
    """Ricker wavelet (1 - 2a) exp(-a), a = (pi f0 (t - t0))^2, at t_n = n tau for n = 0..K-1."""
    t = torch.arange(K, dtype=torch.float64) * tau
    a = (math.pi * f0 * (t - t0)) ** 2
    return (1 - 2 * a) * torch.exp(-a)


def grid_position(problem: MediumProblem, xyz) -> torch.Tensor:
    """Physical coordinates ``(x, y, z)`` (``[3]`` or ``[count, 3]``) as the fractional node coordinates
    ``(x / hx, y / hy, z / hz)`` that ``MediumSolver(source_positions=..., receiver_positions=...)`` takes
    (float64; h = L / N per axis)."""
    p = torch.as_tensor(xyz, dtype=torch.float64)
    if p.shape[-1:] != (3,) or p.dim() > 2:
        raise ValueError(f"xyz must have shape [3] or [count, 3], not {tuple(p.shape)}")
    h = torch.tensor([v / problem.N for v in problem.lengths()], dtype=torch.float64)
    return p / h


def sponge_taper(problem: MediumProblem, width: int, sigma_max: float | None = None, power: float = 2,
                 reflection: float = 0.02, axes: str = "xyz"):
    """Per-axis factors ``(gx, gy, gz)`` of an absorbing sponge layer for :class:`MediumSolver`.

    ``g[q] = exp(-sigma_max ((width - d) / width)^power tau)`` with d = min(q, N - q) nodes from the
    nearer end of the axis, 1 where d >= width; axes not named in ``axes`` are ones. Without
    ``sigma_max`` the damping follows from the two-way travel through the layer at the fastest
    speed for a nominal ``reflection``: ``(power + 1) c_max ln(1 / reflection) / (2 width h_min)``.
    Each is a float64 tensor of N+1 values in global indexing; the profile is symmetric, so
    ``gx[0] == gx[N]`` on the periodic axis.
    """
    N = problem.N
    width = int(width)
    if width < 1:
        raise ValueError(f"sponge width must be >= 1 node, not {width}")
    if 2 * width > N:
        raise ValueError(f"two sponge layers of {width} nodes do not fit in N = {N} intervals")
    if not 0 < reflection < 1:
        raise ValueError(f"reflection must lie in (0, 1), not {reflection}")
    if not set(axes) <= set("xyz"):
        raise ValueError(f"axes must name x, y, z, not {axes!r}")
    if sigma_max is None:
        h_min = min(problem.lengths()) / N
        sigma_max = (power + 1) * math.sqrt(problem.max_speed2) * math.log(1 / reflection) / (2 * width * h_min)
    if not (math.isfinite(sigma_max) and sigma_max >= 0):
        raise ValueError(f"sigma_max must be finite and >= 0, not {sigma_max}")
    q = torch.arange(N + 1, dtype=torch.float64)
    d = torch.minimum(q, N - q)
    g = torch.exp(-sigma_max * ((width - d) / width).clamp(min=0) ** power * problem.tau)
    g[d >= width] = 1.0
    return tuple(g.clone() if a in axes else torch.ones(N + 1, dtype=torch.float64) for a in "xyz")


@dataclass
class MediumResult:
    traces: torch.Tensor     # [K+1, R], row 0 = the initial field
    u_final: torch.Tensor    # (N+1)^3
    max_abs_u: list          # [K+1]: max |u| over the stencil nodes, before the step's source term
    courant: float
    total_ms: float
    mpts_per_s: float
    aborted: bool = False
    abort_layer: int = -1
    abort_reason: str = ""
    extra: dict = field(default_factory=dict)
    # run(frequencies=...): complex [F, N+1, N+1, N+1] on the CPU, sum_n u^n exp(-i 2 pi f n tau) over the
    # sampled layers (the Dirichlet faces 0)
    spectra: torch.Tensor | None = None


def dft_bins(problem: MediumProblem, every: int = 1, pairs: bool = False):
    """``(frequencies, weights)``, float64 tensors, of the half spectrum of the sequence the on-the-fly
    transform samples with ``dft_every = every``: p = 0, e, 2e, ... <= K, what
    :meth:`MediumSolver.run` transforms, or with ``pairs=True`` p = e, 2e, ... <= K - 1, what
    :meth:`MediumSolver.gradient_dft` pairs. With P samples ``f_k = k / (P e tau)`` for k = 0 .. P // 2 and
    the weights ``2 / P``, except ``1 / P`` for k = 0 and, when P is even, for k = P / 2. For real sequences
    a, b over those samples and their transforms A, B at these bins
    ``sum_p a_p b_p = sum_k w_k (Re A_k Re B_k + Im A_k Im B_k)``."""
    from ..ops import reference

    e = reference.check_dft_every(every)
    K = problem.timesteps
    P = (K - 1) // e if pairs else K // e + 1
    if P < 1:
        raise ValueError(f"dft_every = {e} leaves no sample: the pairs are p = e, 2e, ... <= K - 1 = {K - 1}")
    k = torch.arange(P // 2 + 1, dtype=torch.float64)
    w = torch.full((P // 2 + 1,), 2.0 / P, dtype=torch.float64)
    w[0] = 1.0 / P
    if P % 2 == 0:
        w[P // 2] = 1.0 / P
    return k / (P * e * problem.tau), w


class MediumSolver:
    """Run a :class:`MediumProblem` from rest.

    backend     "hip" (MI355X kernels, one GPU) or "cpu" (the PyTorch oracle)
    u0          initial field, ``(N+1)^3`` (default 0); used as given, face values included
    sources     global (i, j, k) nodes off the Dirichlet faces, all distinct (planes 0 and N are
                the same periodic plane)
    wavelet     ``[timesteps, len(sources)]``: f_s(t_n), n = 0..K-1 (see :func:`ricker`)
    receivers   global (i, j, k) nodes
    check_every >0 ("hip"): read the non-finite flag every that many steps and stop early
    variant     ablation only: k_march_m variant ("nt", "plain", "r2", "r2nt"; ops.kernels.step_medium)
    taper       absorbing sponge: ``(gx, gy, gz)``, N+1 factors in (0, 1] per axis in global indexing
                (an entry may be None: ones; see :func:`sponge_taper`). With G = gx[i] (gy[j] gz[k]) the
                step becomes ``u = G ((2 u1 - G u2) + m lap u1)``; the source term is not damped in
                its own step. gx[0] must equal gx[N] (one periodic plane).

    source_positions / receiver_positions
                off-grid points in place of ``sources`` / ``receivers`` (each side exclusive with its
                node list): ``[S, 3]`` / ``[R, 3]`` fractional node coordinates (xi, eta, zeta) = (x / hx,
                y / hy, z / hz) (:func:`grid_position`), ``0 <= xi <= N``; a source needs ``0 < eta, zeta < N``,
                a receiver ``0 <= eta, zeta <= N``; needs N >= 8. Two sources may share a position. A
                point acts through 8 x 8 x 8 nodes (``ops.reference.interp_tables``): periodic wrap in x,
                odd reflection at the y/z faces, and a position on a node is that node alone, so
                integer positions reproduce the node lists. The wavelet stays ``[timesteps, S]``.
    interp      "sinc8" (8-point Kaiser-windowed sinc, b = 6.31; the default) or "linear"

    With ``problem.density`` every step, forward, recomputed and adjoint, uses the density operator;
    the source term stays ``m g`` with ``m = rho c^2 tau^2``, so f is a rate of volume injection.
    """

    def __init__(self, problem: MediumProblem, backend: str = "hip", *, u0=None, sources=(), wavelet=None,
                 receivers=(), check_every: int = 0, device: int | None = None, variant: str | None = None,
                 taper=None, source_positions=None, receiver_positions=None, interp: str = "sinc8"):
        from ..ops import reference

        if backend not in ("hip", "cpu"):
            raise ValueError(f"unknown backend {backend!r}")
        N, K = problem.N, problem.timesteps
        if interp not in reference.INTERP_KINDS:
            raise ValueError(f"interp must be one of {reference.INTERP_KINDS}, not {interp!r}")
        self.interp = interp
        if source_positions is not None and len(sources):
            raise ValueError("give sources or source_positions, not both")
        if receiver_positions is not None and len(receivers):
            raise ValueError("give receivers or receiver_positions, not both")
        self.source_positions = self.receiver_positions = None
        if source_positions is not None and len(source_positions):
            self.source_positions = reference.check_positions(source_positions, N, "source")
        if receiver_positions is not None and len(receiver_positions):
            self.receiver_positions = reference.check_positions(receiver_positions, N, "receiver")
        self.problem, self.backend, self.check_every, self.device = problem, backend, int(check_every), device
        self.variant = variant
        self.sources = [tuple(int(v) for v in s) for s in sources]
        self.receivers = [tuple(int(v) for v in r) for r in receivers]
        seen = set()
        for s in self.sources:
            if len(s) != 3 or not all(0 <= v <= N for v in s):
                raise ValueError(f"source {s} outside the grid 0..{N}")
            if s[1] in (0, N) or s[2] in (0, N):
                raise ValueError(f"source {s} lies on a Dirichlet face")
            key = (s[0] % N, s[1], s[2])  # planes 0 and N are one plane
            if key in seen:
                raise ValueError(f"source {s} given more than once")
            seen.add(key)
        for r in self.receivers:
            if len(r) != 3 or not all(0 <= v <= N for v in r):
                raise ValueError(f"receiver {r} outside the grid 0..{N}")
        self.nsrc = len(self.sources) if self.source_positions is None else int(self.source_positions.shape[0])
        self.nrec = len(self.receivers) if self.receiver_positions is None else int(self.receiver_positions.shape[0])
        if self.nsrc:
            if wavelet is None:
                raise ValueError("sources need a wavelet of shape [timesteps, len(sources)]")
            w = torch.as_tensor(wavelet, dtype=torch.float64)
            if tuple(w.shape) != (K, self.nsrc):
                raise ValueError(f"wavelet must have shape {(K, self.nsrc)} (timesteps x sources), "
                                 f"not {tuple(w.shape)}")
            self.wavelet = w
        else:
            self.wavelet = None
        if u0 is not None:
            u0 = torch.as_tensor(u0)
            if tuple(u0.shape) != (N + 1, N + 1, N + 1):
                raise ValueError(f"u0 must have shape {(N + 1,) * 3}, not {tuple(u0.shape)}")
        self.u0 = u0
        self.taper = None if taper is None else self._check_taper(taper, N)

    @staticmethod
    def _check_taper(taper, N):
        if len(taper) != 3:
            raise ValueError("taper = (gx, gy, gz)")
        out = []
        for name, t in zip("xyz", taper):
            t = torch.ones(N + 1, dtype=torch.float64) if t is None else torch.as_tensor(t, dtype=torch.float64).cpu()
            if t.dim() != 1 or t.numel() != N + 1:
                raise ValueError(f"taper g{name} must have {N + 1} values, not shape {tuple(t.shape)}")
            bad = ~(torch.isfinite(t) & (t > 0) & (t <= 1))
            if bool(bad.any()):
                q = int(bad.nonzero()[0])
                raise ValueError(f"taper g{name} must be finite and in (0, 1], found g{name}[{q}] = {t[q].item()}")
            out.append(t)
        gx = out[0]
        if gx[0] != gx[N]:
            raise ValueError(f"taper gx must be periodic in x: gx[0] = {gx[0].item()} but gx[{N}] = {gx[N].item()}")
        return tuple(out)

    def _layout(self):
        """Storage of the "hip" levels for the problem's space order: (x ghost depth M = order / 2
        with local i = global + M, the step box, the 2M periodic wrap pairs, the order / mirror
        keywords of ``kernels.step_medium``)."""
        N, order = self.problem.N, self.problem.space_order
        M = order // 2
        box = (M, N + M, 1, N - 1, 1, N - 1)
        wrap = []
        for g in range(1, M + 1):  # ghost -g <- global N - g, ghost N + g <- global g
            wrap += [N + M - g, M - g, M + g, N + M + g]
        kw = {} if order == 2 else dict(order=order, mirror=(0, N, 0, N))
        return M, box, tuple(wrap), kw

    def _points_kw(self) -> dict:
        """The source / receiver keywords of the ``ops.reference`` oracles."""
        return dict(sources=self.sources, receivers=self.receivers, source_positions=self.source_positions,
                    receiver_positions=self.receiver_positions, interp=self.interp)

    def _points_extra(self, **counts) -> dict:
        """``extra`` entries of a run with positions (none without): the interpolation and the row and
        entry counts given."""
        if self.source_positions is None and self.receiver_positions is None:
            return {}
        return dict(interp=self.interp, **counts)

    def run(self, frequencies=None, dft_every: int = 1) -> MediumResult:
        """The solve. ``frequencies`` (Hz; a non-empty 1-D list of finite values >= 0) also gives
        ``spectra``, the on-the-fly discrete Fourier transform ``sum_n u^n exp(-i 2 pi f n tau)`` over the
        layers n = 0, e, 2e, ... <= K with e = ``dft_every`` (n = 0: the initial field; every other level
        after its source term), a complex ``[F, N+1, N+1, N+1]`` tensor with the Dirichlet faces 0
        (``ops.reference.solve_medium`` has the definition; :func:`dft_bins` the bins of the half spectrum).
        Every other result keeps its bits. "hip": 2 F more levels, checked against the free device memory
        first, and one ``k_dft_acc`` pass over them per sampled layer (``ops.kernels.dft_accumulate``).
        None: the plain run."""
        from ..ops import reference

        if frequencies is None:
            if dft_every != 1:
                reference.check_dft_every(dft_every)
            dft = None
        else:
            dft = (reference.check_frequencies(frequencies), reference.check_dft_every(dft_every))
        return self._run_cpu(dft) if self.backend == "cpu" else self._run_hip(dft)

    @staticmethod
    def _dft_extra(dft, samples: int) -> dict:
        return {} if dft is None else dict(frequencies=dft[0].tolist(), dft_every=dft[1], dft_samples=samples)

    def _result(self, traces, u_final, mx, ms, **kw) -> MediumResult:
        p = self.problem
        rate = p.points * (len(mx) - 1) / (ms * 1e3) if ms > 0 else 0.0  # Mpoints/s over the layers done
        return MediumResult(traces=traces, u_final=u_final, max_abs_u=mx, courant=p.courant, total_ms=ms,
                            mpts_per_s=rate, **kw)

    def _run_cpu(self, dft=None) -> MediumResult:
        import time

        from ..ops import reference

        p = self.problem
        t0 = time.perf_counter()
        kw = {} if dft is None else dict(frequencies=dft[0], dft_every=dft[1])
        tr, uf, mx, *spec = reference.solve_medium(p.N, p.timesteps, p.speed2, u0=self.u0, wavelet=self.wavelet,
                                                   L=(p.Lx, p.Ly, p.Lz), T=p.T, pi=p.pi, dtype=p.torch_dtype,
                                                   taper=self.taper, order=p.space_order, density=p.density,
                                                   **self._points_kw(), **kw)
        return self._result(tr, uf, mx, (time.perf_counter() - t0) * 1e3, spectra=spec[0] if spec else None,
                            extra=dict(space_order=p.space_order, density=p.density is not None,
                                       **self._points_extra(),
                                       **self._dft_extra(dft, dft and p.timesteps // dft[1] + 1)))

    def _run_hip(self, dft=None) -> MediumResult:
        from ..ops import kernels, reference

        p = self.problem
        N, K, dt = p.N, p.timesteps, p.torch_dtype
        s = _HipSetup(self)
        dev, M, box = s.dev, s.M, s.box
        with torch.cuda.device(dev):
            if dft is not None:
                F = dft[0].numel()
                s.require_levels(4 + 2 * F + (p.density is not None), f"run() with {F} frequencies")
            lv = [s.level() for _ in range(3)]
            m = s.level()
            s.medium(m, lv[0])
            step, g = s.bind_step(m), s.g
            if self.u0 is not None:
                lv[0][M:N + 1 + M] = self.u0.to(dt).to(dev)
                reference._wrap_x(lv[0], N, M)
            traces = torch.zeros(K + 1, self.nrec, dtype=dt, device=dev)
            stat = kernels.new_err(K + 1, device=dev)
            mx0 = reference.max_abs_field(lv[0][M:N + 1 + M, 1:N, 1:N])
            s.record(lv[0], traces[0])
            samples = 0
            if dft is not None:  # the twiddle table goes up once; a sampled layer passes one of its rows
                every = dft[1]
                ctab, stab = (t.contiguous().to(dev) for t in reference.dft_tables(dft[0], range(K + 1), s.c["tau"], dt))
                sre, sim = [s.level() for _ in range(F)], [s.level() for _ in range(F)]
                kernels.dft_accumulate(lv[0], sre, sim, box, ctab[0], stab[0])
                samples = 1
            abort = {}
            done = K
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for n in range(1, K + 1):
                u1, u2, u = lv[(n + 2) % 3], lv[(n + 1) % 3], lv[n % 3]
                if n == 3:  # level 0 comes round: the faces of the given u0 become Dirichlet zeros
                    u[:, 0, :] = 0
                    u[:, N, :] = 0
                    u[:, :, 0] = 0
                    u[:, :, N] = 0
                step(u1, u2, u, first=n == 1, stat=stat[3 * n:3 * n + 3], variant=self.variant)
                s.inject(u, m, g[n - 1])
                s.record(u, traces[n])
                if dft is not None and n % every == 0:
                    kernels.dft_accumulate(u, sre, sim, box, ctab[n], stab[n])
                    samples += 1
                if self.check_every > 0 and n % self.check_every == 0:
                    bad = _nonfinite_layer(stat, n)  # one read-back: the flags of layers 0..n
                    if bad is not None:
                        abort = dict(aborted=True, abort_layer=bad, abort_reason="non-finite values")
                        done = n
                        break
            ev1.record()
            ev1.synchronize()
            ms = ev0.elapsed_time(ev1)
            dec = kernels.decode_err(stat)  # the one read-back of the statistics
            mx = [mx0] + [dec[n][0] for n in range(1, done + 1)]
            extra = dict(space_order=p.space_order, density=p.density is not None, **s.points_extra(),
                         **self._dft_extra(dft, samples))
            if not abort and any(d[2] for d in dec[1:]):  # ran to the end, but not on finite values
                extra["nonfinite_layer"] = next(n for n in range(1, K + 1) if dec[n][2])
            uf = lv[done % 3][M:N + 1 + M].cpu()
            spectra = None if dft is None else reference.spectra_tensor(sre, sim, N, M)
            return self._result(traces.cpu(), uf, mx, ms, extra=extra, spectra=spectra, **abort)

    # ---- misfit gradients (adjoint state; ops/reference.py has the mathematics) ------------

    def gradient(self, observed, *, segment: int | None = None, wrt_density: bool = False,
                 illumination: bool = False) -> "MediumGradient":
        """Misfit ``J = 1/2 sum_{n=1..K} sum_r (trace[n, r] - observed[n, r])^2`` and its gradients
        with respect to ``speed2`` and the wavelet (full-waveform-inversion gradient / reverse-time
        migration image). ``observed``: ``[timesteps + 1, len(receivers)]``, row 0 is ignored.

        ``grad_speed2`` is taken with respect to the unique nodes: entry [0] is the derivative with
        respect to the shared value of planes 0 and N, entry [N] a copy of it, the Dirichlet faces
        are 0; for a periodic perturbation d the directional derivative is ``(grad[:N] * d[:N]).sum()``.

        "hip": the forward history does not stay in memory; steps 2..K are cut into segments of
        ``segment`` steps, the two newest levels are checkpointed before each segment and the
        reverse pass recomputes one segment at a time (``segment >= K - 1``: nothing is
        recomputed). The result does not depend on ``segment`` bit for bit. None: the segment
        with the fewest levels (:func:`gradient_levels`), checked against the free device memory.

        ``wrt_density=True`` (needs ``problem.density``, a scalar is fine) also returns ``grad_density``,
        dJ/drho at fixed ``speed2``, with the convention of ``grad_speed2``: the derivative with respect
        to the densities of the stencil nodes (the unique x planes, j and k in 1..N-1), entry [0] for
        the shared value of planes 0 and N, entry [N] a copy of it. The densities of the Dirichlet wall
        nodes do enter the adjacent half-face averages; they are held fixed and reported as 0, like
        the faces of ``grad_speed2``. ``grad_speed2`` stays the derivative at fixed rho, so any other
        parametrisation follows from the pair by the chain rule (impedance and speed, bulk modulus
        and density, ...). "hip": each segment then also keeps the levels u^n of its steps beside q,
        ``min(segment, K - 1)`` more levels plus one accumulator, and every adjoint step is followed
        by one ``k_face_corr`` call; the other results do not change by a bit.

        ``illumination=True`` also returns the source illumination and the diagonal of Shin's
        pseudo-Hessian for ``speed2``, the usual scaling of the gradient (:func:`precondition`) and
        preconditioner of a Gauss-Newton iteration: ``illumination = sum_{n=1..K-1} q^n q^n`` at the
        stencil nodes, q^n the Laplacian (``div(b grad u^n)`` with a density) that entered forward step
        n + 1, the very values the gradient correlates with the adjoint field; each product is rounded,
        then added, in ascending n. ``pseudo_hessian_speed2 = illumination (w w)`` with
        ``w = (G tau) tau [rho]``, G the sponge factor of the node, finished on the host in the working
        dtype (``ops.reference.finish_illumination``). Both follow the convention of ``grad_speed2``
        (plane N a copy of plane 0, the Dirichlet faces 0). The pseudo-Hessian ignores the source term
        of dJ/dm at the source nodes. ``variant`` must be None. "hip": one more level; the forward pass
        proper runs its steps 2..K in the illum mode of ``ops.kernels.step_medium`` (save+illum in the
        last segment) and the recomputed steps stay in save mode, so every q^n is added exactly once,
        in ascending n, and the result does not depend on ``segment`` by a bit; the other results do not
        change by a bit either.
        """
        p = self.problem
        K = p.timesteps
        if self.u0 is not None:
            raise ValueError("gradient() starts from rest: u0 is not supported")
        if not self.nrec:
            raise ValueError("gradient() needs at least one receiver")
        obs = torch.as_tensor(observed)
        if tuple(obs.shape) != (K + 1, self.nrec):
            raise ValueError(f"observed must have shape {(K + 1, self.nrec)} (timesteps + 1 x receivers), "
                             f"not {tuple(obs.shape)}")
        if segment is not None and int(segment) < 1:
            raise ValueError(f"segment must be >= 1 step, not {segment}")
        wrt_density, illumination = bool(wrt_density), bool(illumination)
        if illumination and self.variant is not None:
            raise ValueError(f"gradient(illumination=True) exists for the default kernel variant only: build the "
                             f"MediumSolver with variant=None, not {self.variant!r}")
        if wrt_density and p.density is None:
            raise ValueError("gradient(wrt_density=True) needs a density model: build the MediumProblem with "
                             "density=... (a scalar such as 1.0 is fine)")
        obs = obs.detach().cpu()
        if self.backend == "cpu":
            return self._gradient_cpu(obs, wrt_density, illumination)
        return self._gradient_hip(obs, segment, wrt_density, illumination)

    def _gradient_cpu(self, obs, wrt_density: bool = False, illumination: bool = False) -> "MediumGradient":
        import time

        from ..ops import reference

        p = self.problem
        t0 = time.perf_counter()
        fn = reference.gradient_medium_density if wrt_density else reference.gradient_medium
        kw = dict(illumination=True) if illumination else {}
        J, gs, gw, tr, *more = fn(p.N, p.timesteps, p.speed2, obs, wavelet=self.wavelet, taper=self.taper,
                                  L=(p.Lx, p.Ly, p.Lz), T=p.T, pi=p.pi, dtype=p.torch_dtype, order=p.space_order,
                                  density=p.density, **self._points_kw(), **kw)
        il, ph = more[-2:] if illumination else (None, None)
        return MediumGradient(misfit=J, grad_speed2=gs, grad_wavelet=gw, traces=tr,
                              total_ms=(time.perf_counter() - t0) * 1e3,
                              grad_density=more[0] if wrt_density else None, illumination=il,
                              pseudo_hessian_speed2=ph,
                              extra=dict(segment=None, levels=None, recomputed_steps=0, space_order=p.space_order,
                                         density=p.density is not None, wrt_density=wrt_density,
                                         illumination=illumination, **self._points_extra()))

    def _gradient_hip(self, obs, segment, wrt_density: bool = False, illumination: bool = False) -> "MediumGradient":
        import time

        from ..ops import kernels, reference

        p = self.problem
        N, K, dt = p.N, p.timesteps, p.torch_dtype
        s = _HipSetup(self)
        dev, c, M, box, h2, level = s.dev, s.c, s.M, s.box, s.h2, s.level
        with torch.cuda.device(dev):
            if segment is None:
                segment = best_gradient_segment(K, wrt_density=wrt_density, illumination=illumination)
                what = "the smallest schedule"
            else:
                segment = int(segment)
                what = f"the schedule of segment = {segment}"
            nlev = gradient_levels(K, segment, density=p.density is not None, wrt_density=wrt_density,
                                   illumination=illumination)
            s.require_levels(nlev, f"gradient(): {what}")
            # forward steps 2..K in segments [a, b]; the last one keeps its q, the others a checkpoint
            segs = [(a, min(a + segment - 1, K)) for a in range(2, K + 1, segment)]
            qlen = min(segment, K - 1)
            t0 = time.perf_counter()
            lv = [level() for _ in range(3)]
            ad = [level() for _ in range(3)] if len(segs) > 1 else lv  # the adjoint's ring
            m, acc = level(), level()
            qb = [level() for _ in range(qlen)]
            # wrt_density: ub[n - (a - 1)] = u^n for the steps n = a-1 .. b-1 of the segment [a, b] at hand
            # (its own data: with one segment the adjoint ring overwrites the forward ring), and accb
            ub = [level() for _ in range(qlen)] if wrt_density else None
            accb = level() if wrt_density else None
            hl = level() if illumination else None  # h = sum q^n q^n, added to by the forward pass proper alone
            ck = [(level(), level()) for _ in segs[:-1]]
            mc = s.medium(m, lv[0])
            step, tt, gsrc, g = s.bind_step(m), s.tt, s.gsrc, s.g
            traces = torch.zeros(K + 1, self.nrec, dtype=dt, device=dev)
            stat = kernels.new_err(K + 1, device=dev)
            scratch = kernels.new_err(1, device=dev)  # statistics of the recomputed steps (those of `stat` again)

            def keep_level(n, a):  # u^n, injected and wrapped, into the history of the segment from a
                if wrt_density:
                    ub[n - (a - 1)]._base.copy_(lv[n % 3]._base)

            def forward_step(n, slot, save, illum=None):
                u1, u2, u = lv[(n + 2) % 3], lv[(n + 1) % 3], lv[n % 3]
                step(u1, u2, u, first=n == 1, stat=slot, variant=None if save is not None else self.variant,
                     lap_out=save, illum=illum)
                s.inject(u, m, g[n - 1])

            # forward pass: run()'s steps; checkpoints before the segments, q of the last segment
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            s.record(lv[0], traces[0])
            forward_step(1, stat[3:6], None)
            s.record(lv[1], traces[1])
            for si, (a, b) in enumerate(segs):
                last = si == len(segs) - 1
                if not last:
                    ck[si][0]._base.copy_(lv[(a - 1) % 3]._base)
                    ck[si][1]._base.copy_(lv[(a - 2) % 3]._base)
                if last:
                    keep_level(a - 1, a)
                for n in range(a, b + 1):
                    forward_step(n, stat[3 * n:3 * n + 3], qb[n - a] if last else None, hl)
                    s.record(lv[n % 3], traces[n])
                    if last and n < b:
                        keep_level(n, a)
            ev[1].record()
            _require_finite(stat, "gradient()", "forward pass")
            tr = traces.cpu()
            J, res = reference.misfit_medium(tr, obs)
            finish_level = s.adjoint_points(res, lv[0], m)  # injects G rho^n, samples mu^n at the sources
            a_dev = torch.zeros(K, self.nsrc, dtype=dt, device=dev)
            astat = kernels.new_err(K + 1, device=dev)

            # reverse pass: mu^K into zero levels, then mu^n for n = K-1 .. 1, level mu^n in ad[n % 3]
            ev[2].record()
            ad[(K + 1) % 3].zero_()
            ad[K % 3].zero_()
            finish_level(ad[K % 3], K, a_dev[K - 1])
            recomputed = 0
            for si in range(len(segs) - 1, -1, -1):
                a, b = segs[si]
                if si != len(segs) - 1:
                    lv[(a - 1) % 3]._base.copy_(ck[si][0]._base)
                    lv[(a - 2) % 3]._base.copy_(ck[si][1]._base)
                    keep_level(a - 1, a)
                    for n in range(a, b + 1):
                        forward_step(n, scratch, qb[n - a])
                        if n < b:
                            keep_level(n, a)
                    recomputed += b - a + 1
                for n in range(b - 1, a - 2, -1):  # q^n is what forward step n + 1 saved
                    u1, u2, u = ad[(n + 1) % 3], ad[(n + 2) % 3], ad[n % 3]
                    step(u1, u2, u, first=False, stat=astat[3 * n:3 * n + 3], image=(qb[n + 1 - a], acc))
                    finish_level(u, n, a_dev[n - 1])
                    if wrt_density:  # u1 = mu^{n+1}, injected and wrapped; its level is reused two steps on
                        kernels.face_correlation(u1, ub[n - (a - 1)], accb, box, h2=h2)
            ev[3].record()
            _require_finite(astat, "gradient()", "adjoint pass")
            acc_c, a_c = acc.cpu(), a_dev.cpu()
            srows = s.source_rows_host()  # off-grid sources: (rows, the time sums of rows_dot)
            gs, gw = reference.finish_gradient_medium(acc_c, a_c, gsrc, mc, tt, self.sources, N, c["tau"],
                                                      c["hx"], c["hy"], c["hz"], M, p.density, srows)
            gd = None
            if wrt_density:
                gd = reference.finish_gradient_density(acc_c, accb.cpu(), a_c, gsrc, mc, tt, self.sources, N,
                                                       c["tau"], p.speed2, p.density, M, srows)
            il = ph = None
            if illumination:
                il, ph = reference.finish_illumination(hl.cpu(), tt, N, c["tau"], M, p.density)
            torch.cuda.synchronize(dev)
            ms = (time.perf_counter() - t0) * 1e3
            return MediumGradient(misfit=J, grad_speed2=gs, grad_wavelet=gw, traces=tr, total_ms=ms, grad_density=gd,
                                  illumination=il, pseudo_hessian_speed2=ph,
                                  extra=dict(segment=segment, levels=nlev, recomputed_steps=recomputed,
                                             space_order=p.space_order, density=p.density is not None,
                                             wrt_density=wrt_density, illumination=illumination,
                                             forward_ms=ev[0].elapsed_time(ev[1]), reverse_ms=ev[2].elapsed_time(ev[3]),
                                             **s.points_extra()))

    # ---- the checkpoint-free spectral gradient ------------------------------------------------

    def gradient_dft(self, observed, frequencies, *, weights=None, dft_every: int = 1) -> "MediumGradient":
        """:meth:`gradient` with the time sum ``sum_n mu^{n+1} q^n`` replaced by a sum over a few
        frequencies of the on-the-fly spectra of q and mu (``ops.reference.gradient_medium_dft`` has the
        definition): ``acc = sum_f weights_f (Re Q_f Re M_f + Im Q_f Im M_f)`` with
        ``Q_f = sum_p q^p exp(-i 2 pi f p tau)``, ``M_f = sum_p mu^{p+1} exp(-i 2 pi f p tau)`` over the pairs
        p = e, 2e, ... <= K - 1, e = ``dft_every``. Neither pass keeps a level of the other, so there are no
        checkpoints and nothing is recomputed: :func:`gradient_dft_levels` levels whatever K is.

        With ``dft_bins(problem, every=e, pairs=True)`` as ``frequencies`` and ``weights`` Parseval's identity
        makes ``grad_speed2`` the time-domain sum over those pairs up to rounding (for e = 1 that of
        :meth:`gradient`); a few bins give the band-limited gradient of multiscale inversion. ``misfit``,
        ``grad_wavelet`` and ``traces`` are those of :meth:`gradient` bit for bit. ``weights`` None: ones.

        Preconditions: those of :meth:`gradient` (from rest, at least one receiver, ``observed`` of shape
        ``[timesteps + 1, receivers]``), ``variant`` None and ``dft_every <= K - 1``. Every space order, a
        density model, the sponge and off-grid points work; ``wrt_density`` and ``illumination`` are not
        offered. "hip": the forward pass runs its steps 2 .. K in save mode into one scratch level, followed
        by ``k_dft_acc`` at the sampled indices; the adjoint field runs in the same ring with the plain step,
        mu^{n+1} accumulated before each sampled step."""
        from ..ops import reference

        p = self.problem
        K = p.timesteps
        if self.u0 is not None:
            raise ValueError("gradient_dft() starts from rest: u0 is not supported")
        if not self.nrec:
            raise ValueError("gradient_dft() needs at least one receiver")
        if self.variant is not None:
            raise ValueError(f"gradient_dft() exists for the default kernel variant only: build the MediumSolver "
                             f"with variant=None, not {self.variant!r}")
        obs = torch.as_tensor(observed)
        if tuple(obs.shape) != (K + 1, self.nrec):
            raise ValueError(f"observed must have shape {(K + 1, self.nrec)} (timesteps + 1 x receivers), "
                             f"not {tuple(obs.shape)}")
        f = reference.check_frequencies(frequencies)
        every = reference.check_dft_every(dft_every)
        if every > K - 1:
            raise ValueError(f"dft_every = {every} leaves no pair to correlate: the pairs are p = e, 2e, ... <= "
                             f"K - 1 = {K - 1}")
        if weights is not None:
            try:
                w = torch.as_tensor(weights, dtype=torch.float64).cpu()
            except (TypeError, ValueError, RuntimeError) as e:
                raise ValueError(f"weights must be a 1-D list of numbers: {e}") from None
            if w.dim() != 1 or w.numel() != f.numel() or not bool(torch.isfinite(w).all()):
                raise ValueError(f"weights must be {f.numel()} finite values, one per frequency")
            weights = w
        obs = obs.detach().cpu()
        if self.backend == "cpu":
            return self._gradient_dft_cpu(obs, f, weights, every)
        return self._gradient_dft_hip(obs, f, weights, every)

    def _gradient_dft_extra(self, f, every: int, levels) -> dict:
        p = self.problem
        return dict(segment=None, levels=levels, recomputed_steps=0, space_order=p.space_order,
                    density=p.density is not None, wrt_density=False, illumination=False, frequencies=f.tolist(),
                    dft_every=every, dft_samples=(p.timesteps - 1) // every)

    def _gradient_dft_cpu(self, obs, f, weights, every: int) -> "MediumGradient":
        import time

        from ..ops import reference

        p = self.problem
        t0 = time.perf_counter()
        J, gs, gw, tr = reference.gradient_medium_dft(p.N, p.timesteps, p.speed2, obs, f, weights=weights,
                                                      dft_every=every, wavelet=self.wavelet, taper=self.taper,
                                                      L=(p.Lx, p.Ly, p.Lz), T=p.T, pi=p.pi, dtype=p.torch_dtype,
                                                      order=p.space_order, density=p.density, **self._points_kw())
        return MediumGradient(misfit=J, grad_speed2=gs, grad_wavelet=gw, traces=tr,
                              total_ms=(time.perf_counter() - t0) * 1e3,
                              extra=dict(**self._gradient_dft_extra(f, every, None), **self._points_extra()))

    def _gradient_dft_hip(self, obs, f, weights, every: int) -> "MediumGradient":
        import time

        from ..ops import kernels, reference

        p = self.problem
        N, K, dt = p.N, p.timesteps, p.torch_dtype
        F = f.numel()
        s = _HipSetup(self)
        dev, c, M, box, level = s.dev, s.c, s.M, s.box, s.level
        with torch.cuda.device(dev):
            nlev = gradient_dft_levels(F, density=p.density is not None)
            s.require_levels(nlev, f"gradient_dft() with {F} frequencies")
            t0 = time.perf_counter()
            lv = [level() for _ in range(3)]  # the forward ring, then the adjoint's
            m, ql = level(), level()          # ql: the q^p of the step at hand
            spec = [[level() for _ in range(F)] for _ in range(4)]  # Qre, Qim, Mre, Mim
            mc = s.medium(m, lv[0])
            step, tt, gsrc, g = s.bind_step(m), s.tt, s.gsrc, s.g
            ctab, stab = (t.contiguous().to(dev) for t in reference.dft_tables(f, range(K), c["tau"], dt))
            traces = torch.zeros(K + 1, self.nrec, dtype=dt, device=dev)
            stat = kernels.new_err(K + 1, device=dev)

            # forward pass: run()'s steps; step n >= 2 saves q^{n-1}, the Laplacian it used
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            s.record(lv[0], traces[0])
            for n in range(1, K + 1):
                u1, u2, u = lv[(n + 2) % 3], lv[(n + 1) % 3], lv[n % 3]
                step(u1, u2, u, first=n == 1, stat=stat[3 * n:3 * n + 3], lap_out=ql if n >= 2 else None)
                s.inject(u, m, g[n - 1])
                s.record(u, traces[n])
                if n >= 2 and (n - 1) % every == 0:
                    kernels.dft_accumulate(ql, spec[0], spec[1], box, ctab[n - 1], stab[n - 1])
            ev[1].record()
            _require_finite(stat, "gradient_dft()", "forward pass")
            tr = traces.cpu()
            J, res = reference.misfit_medium(tr, obs)
            finish_level = s.adjoint_points(res, lv[0], m)  # injects G rho^n, samples mu^n at the sources
            a_dev = torch.zeros(K, self.nsrc, dtype=dt, device=dev)
            astat = kernels.new_err(K + 1, device=dev)

            # reverse pass in the same ring: mu^K into zero levels, then mu^n for n = K-1 .. 1 in lv[n % 3]
            ev[2].record()
            lv[(K + 1) % 3].zero_()
            lv[K % 3].zero_()
            finish_level(lv[K % 3], K, a_dev[K - 1])
            for n in range(K - 1, 0, -1):
                u1, u2, u = lv[(n + 1) % 3], lv[(n + 2) % 3], lv[n % 3]
                if n % every == 0:  # u1 = mu^{n+1}, injected and wrapped
                    kernels.dft_accumulate(u1, spec[2], spec[3], box, ctab[n], stab[n])
                step(u1, u2, u, first=False, stat=astat[3 * n:3 * n + 3])
                finish_level(u, n, a_dev[n - 1])
            ev[3].record()
            _require_finite(astat, "gradient_dft()", "adjoint pass")
            acc = reference.finish_gradient_dft(*([t.cpu() for t in ts] for ts in spec), weights, dt)
            gs, gw = reference.finish_gradient_medium(acc, a_dev.cpu(), gsrc, mc, tt, self.sources, N, c["tau"],
                                                      c["hx"], c["hy"], c["hz"], M, p.density, s.source_rows_host())
            torch.cuda.synchronize(dev)
            ms = (time.perf_counter() - t0) * 1e3
            return MediumGradient(misfit=J, grad_speed2=gs, grad_wavelet=gw, traces=tr, total_ms=ms,
                                  extra=dict(**self._gradient_dft_extra(f, every, nlev),
                                             forward_ms=ev[0].elapsed_time(ev[1]),
                                             reverse_ms=ev[2].elapsed_time(ev[3]), **s.points_extra()))

    # ---- Born (linearised) modelling and Gauss-Newton products -------------------------------

    def born(self, dspeed2=None, dwavelet=None, ddensity=None) -> "MediumBorn":
        """Born (linearised) modelling, the Jacobian that :meth:`gradient` transposes: the change of the
        traces, to first order, for a perturbation ``dspeed2`` of ``speed2`` (a scalar or ``(N+1)^3``,
        finite, periodic in x, of any sign; the density stays fixed), ``dwavelet``
        ``[timesteps, len(sources)]`` of the wavelet and ``ddensity`` of the density (like ``dspeed2``, at
        fixed ``speed2``; needs ``problem.density``, a scalar is fine). At least one of the three.

        The background field and the perturbation field ``du`` run in lock step from rest
        (``ops.reference.born_medium`` has the recurrence): ``dtraces[n, r] = du^n[x_r]``, row 0 is 0.
        For any ``r`` of the traces' shape, ``(dtraces[1:] * r[1:]).sum()`` equals
        ``(grad_speed2[:N] * dspeed2[:N]).sum() + (grad_wavelet * dwavelet).sum()`` of
        ``gradient(traces - r)`` up to rounding. ``ddensity`` is honoured on the Dirichlet wall nodes too
        (their buoyancy enters the adjacent half-face averages), so ``dtraces`` is the true directional
        derivative; ``grad_density`` holds the wall densities fixed, so for a ``ddensity`` that vanishes
        on the y/z faces the identity gains ``(grad_density[:N] * ddensity[:N]).sum()`` of
        ``gradient(traces - r, wrt_density=True)``.

        "hip": nine levels (the rings of u and du, m, dm and one q level; ten with a density), checked
        against the free device memory. Per step the background step runs in save mode into q and
        the step of du reads it back in Born mode (``ops.kernels.step_medium``). With ``ddensity``:
        eleven levels (one more, the buoyancy perturbation), the background step runs in scatter mode
        and stores the whole scattering term ``s = dm q + m D_db u`` where q went, and the step of du
        adds it in Born-add mode. Without ``ddensity`` nothing changes: the same kernels, levels and bits."""
        from ..ops import reference

        p = self.problem
        N, K = p.N, p.timesteps
        if self.u0 is not None:
            raise ValueError("born() starts from rest: u0 is not supported")
        if not self.nrec:
            raise ValueError("born() needs at least one receiver")
        if dspeed2 is None and dwavelet is None and ddensity is None:
            raise ValueError("born() needs a perturbation: dspeed2, dwavelet, ddensity or any of them together")
        if ddensity is not None and p.density is None:
            raise ValueError("born(ddensity=...) needs a density model: build the MediumProblem with "
                             "density=... (a scalar such as 1.0 is fine)")
        ds = None if dspeed2 is None else reference.perturbation_field(dspeed2, N, "dspeed2")
        dr = None if ddensity is None else reference.perturbation_field(ddensity, N, "ddensity")
        dw = None
        if dwavelet is not None:
            if not self.nsrc:
                raise ValueError("dwavelet needs sources")
            dw = torch.as_tensor(dwavelet, dtype=torch.float64).detach().cpu()
            if tuple(dw.shape) != (K, self.nsrc):
                raise ValueError(f"dwavelet must have shape {(K, self.nsrc)} (timesteps x sources), "
                                 f"not {tuple(dw.shape)}")
            if not bool(torch.isfinite(dw).all()):
                raise ValueError("dwavelet must be finite")
        return self._born_cpu(ds, dw, dr) if self.backend == "cpu" else self._born_hip(ds, dw, dr)

    def _born_cpu(self, ds, dw, dr=None) -> "MediumBorn":
        import time

        from ..ops import reference

        p = self.problem
        t0 = time.perf_counter()
        tr, dtr, duf, mx = reference.born_medium(p.N, p.timesteps, p.speed2, ds, dw, wavelet=self.wavelet,
                                                 taper=self.taper, L=(p.Lx, p.Ly, p.Lz), T=p.T, pi=p.pi,
                                                 dtype=p.torch_dtype, order=p.space_order, density=p.density,
                                                 ddensity=dr, **self._points_kw())
        return MediumBorn(traces=tr, dtraces=dtr, du_final=duf, max_abs_du=mx,
                          total_ms=(time.perf_counter() - t0) * 1e3,
                          extra=dict(levels=None, space_order=p.space_order, density=p.density is not None,
                                     ddensity=dr is not None, **self._points_extra()))

    def _born_hip(self, ds, dw, dr=None) -> "MediumBorn":
        import time

        from ..ops import kernels, reference

        p = self.problem
        N, K, dt = p.N, p.timesteps, p.torch_dtype
        s = _HipSetup(self)
        dev, c, M, level = s.dev, s.c, s.M, s.level
        with torch.cuda.device(dev):
            nlev = born_levels(density=p.density is not None, ddensity=dr is not None)
            s.require_levels(nlev, "born(): the schedule")
            t0 = time.perf_counter()
            lv = [level() for _ in range(3)]
            dl = [level() for _ in range(3)]
            m, dm, q = level(), level(), level()  # with ddensity, q holds s = dm q + m D_db u instead
            db = None if dr is None else level()
            s.medium(m, lv[0], dwavelet=dw)
            step, g, dg = s.bind_step(m), s.g, s.dg
            if ds is not None:  # None: dm = 0, the scattering term adds zeros
                dm.copy_(reference.medium_coefficient(ds, c["tau"], N, dt, M, p.density))
            if dr is not None:  # born_medium's dm and db
                dmr = reference.medium_coefficient(p.speed2, c["tau"], N, dt, M, dr)
                if ds is not None:
                    dmr = reference.medium_coefficient(ds, c["tau"], N, dt, M, p.density) + dmr
                dm.copy_(dmr)
                db.copy_(reference.dbuoyancy_field(dr, p.density, N, dt, M))
            traces = torch.zeros(K + 1, self.nrec, dtype=dt, device=dev)
            dtraces = torch.zeros(K + 1, self.nrec, dtype=dt, device=dev)
            stat = kernels.new_err(K + 1, device=dev)
            dstat = kernels.new_err(K + 1, device=dev)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for n in range(1, K + 1):
                u1, u2, u = lv[(n + 2) % 3], lv[(n + 1) % 3], lv[n % 3]
                d1, d2, d = dl[(n + 2) % 3], dl[(n + 1) % 3], dl[n % 3]
                first = n == 1
                # the background step, saving q = lap u^{n-1} (save mode: the default variant), or with
                # ddensity the scattering term s (scatter mode); the step of du reads it back
                if first:
                    save, read = {}, {}
                elif db is None:
                    save, read = dict(lap_out=q), dict(born=(q, dm))
                else:
                    save, read = dict(scatter=(q, dm, db)), dict(born_add=q)
                variant = self.variant if first else None
                step(u1, u2, u, first=first, stat=stat[3 * n:3 * n + 3], variant=variant, **save)
                s.inject(u, m, g[n - 1])
                # the step of du with the scattering term, then the perturbed source terms
                step(d1, d2, d, first=first, stat=dstat[3 * n:3 * n + 3], variant=variant, **read)
                s.inject(d, dm, g[n - 1])
                if dg is not None:
                    s.inject(d, m, dg[n - 1])
                s.record(u, traces[n])
                s.record(d, dtraces[n])
            ev1.record()
            ev1.synchronize()
            _require_finite(stat, "born()", "background field")
            _require_finite(dstat, "born()", "perturbation field")
            dec = kernels.decode_err(dstat)
            mx = [0.0] + [dec[n][0] for n in range(1, K + 1)]  # du^0 = 0
            duf = dl[K % 3][M:N + 1 + M].cpu()
            tr, dtr = traces.cpu(), dtraces.cpu()
            return MediumBorn(traces=tr, dtraces=dtr, du_final=duf, max_abs_du=mx,
                              total_ms=(time.perf_counter() - t0) * 1e3,
                              extra=dict(levels=nlev, space_order=p.space_order, density=p.density is not None,
                                         ddensity=dr is not None, loop_ms=ev0.elapsed_time(ev1),
                                         **s.points_extra()))

    def gauss_newton(self, dspeed2=None, dwavelet=None, ddensity=None, *, segment: int | None = None,
                     wrt_density: bool | None = None, illumination: bool = False) -> "MediumGradient":
        """The Gauss-Newton Hessian applied to a perturbation: one :meth:`born` run, then
        :meth:`gradient` with ``observed = traces - dtraces``, so that the residuals are ``dtraces`` and
        ``grad_speed2``, ``grad_wavelet`` are ``J^T J [dspeed2; dwavelet]`` (``misfit`` is
        ``1/2 |dtraces[1:]|^2``). ``segment``: the checkpoint schedule of :meth:`gradient`. ``extra``
        also carries the Born run's ``dtraces``. Both backends form ``observed`` on the host alike.

        ``ddensity``: the density block of the perturbation (:meth:`born`). ``wrt_density`` (default:
        whether ``ddensity`` is given) also returns ``grad_density``, the density row of
        ``J^T J [dspeed2; dwavelet; ddensity]``, with the wall convention of :meth:`gradient`.
        ``illumination``: passed through to :meth:`gradient` (the pseudo-Hessian diagonal, the usual
        preconditioner of a conjugate-gradient iteration on these products)."""
        b = self.born(dspeed2, dwavelet, ddensity)
        if wrt_density is None:
            wrt_density = ddensity is not None
        r = self.gradient(b.traces - b.dtraces, segment=segment, wrt_density=wrt_density, illumination=illumination)
        r.extra["dtraces"] = b.dtraces
        r.extra["born_ms"] = b.total_ms
        return r


class _HipSetup:
    """What run(), gradient() and born() share on the "hip" backend: the device, the grid constants
    ``c`` / ``h2``, the storage layout of :meth:`MediumSolver._layout`, the level allocator, and
    (:meth:`medium`) the model and source data on the device. The drivers allocate their levels
    themselves, in their own order."""

    def __init__(self, solver: MediumSolver):
        from ..ops import reference

        p = solver.problem
        if not torch.cuda.is_available():
            raise RuntimeError("the hip backend needs a HIP device")
        self.solver = solver
        self.dev = torch.device("cuda", torch.cuda.current_device() if solver.device is None else solver.device)
        self.c = reference.tables(p.N, p.timesteps, (p.Lx, p.Ly, p.Lz), p.T, p.pi)[4]
        self.h2 = (self.c["hx2"], self.c["hy2"], self.c["hz2"])
        self.M, self.box, self.wrap, self.step_kw = solver._layout()
        self.shape = (p.N + 1 + 2 * self.M, p.N + 1, p.N + 1)

    def level(self):
        from ..ops import kernels

        return kernels.alloc_level(*self.shape, self.solver.problem.torch_dtype, self.dev)

    def require_levels(self, nlev: int, what: str) -> None:
        """Raises unless ``nlev`` levels fit into the free device memory; ``what`` names the schedule."""
        from ..ops import kernels

        dev = self.dev
        level_bytes = kernels.level_bytes(*self.shape, self.solver.problem.torch_dtype)
        free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        if nlev * level_bytes > free:
            raise RuntimeError(f"{what} holds {nlev} levels = {nlev * level_bytes} bytes, but only "
                               f"{free} bytes of device memory are free")

    def medium(self, m, lv0, dwavelet=None):
        """Fills the level ``m`` with the coefficient field and returns its host copy; allocates the
        buoyancy level of a density model into ``step_kw``; then the taper tables (``tt`` on the host,
        ``taper`` on the device, None without a sponge), the source entries, the source table of the
        wavelet (``gsrc`` on the host, ``g`` its columns on the device, one per storage node; ``dg``
        those of ``dwavelet``) and the source and receiver nodes ``src`` / ``rec`` in the strides of
        the level ``lv0``. With positions the tables stay compact, ``g`` ``[K, S]``, and ``src_rows`` (the CSR
        row list of the sources) / ``rec_tab`` (the receivers' gather tables) take the node lists' place;
        :meth:`inject` and :meth:`record` dispatch on them."""
        from ..ops import kernels, reference

        sv, c, M, dev = self.solver, self.c, self.M, self.dev
        p = sv.problem
        N, K, dt = p.N, p.timesteps, p.torch_dtype
        mc = reference.medium_coefficient(p.speed2, c["tau"], N, dt, M, p.density)
        m.copy_(mc)
        if p.density is not None:
            bu = self.level()
            bu.copy_(reference.buoyancy_field(p.density, N, dt, M))
            self.step_kw = dict(self.step_kw, buoyancy=bu)
        self.tt = None if sv.taper is None else reference.taper_tables(sv.taper, N, dt, M)
        self.taper = None if self.tt is None else tuple(t.to(dev) for t in self.tt)
        def table(w):
            return reference.source_table(w, K, sv.nsrc, c["hx"], c["hy"], c["hz"], dt)

        self.gsrc = table(sv.wavelet)
        self.src = self.rec = self.src_rows = self.rec_tab = self.host_rows = None
        self.counts = {}
        if sv.source_positions is None:
            ent = reference.source_entries(sv.sources, N, M)
            cols = [s for _, s in ent]  # one column per storage node
            self.g = self.gsrc[:, cols].contiguous().to(dev)
            self.dg = None if dwavelet is None else table(dwavelet)[:, cols].contiguous().to(dev)
            self.src = kernels.source_nodes([nd for nd, _ in ent], lv0)
        else:  # the compact [K, S] tables; the rows carry the weights
            self.host_rows = reference.point_rows(sv.source_positions, N, dt, sv.interp, M)
            self.src_rows = kernels.row_list(self.host_rows, lv0)
            self.g = self.gsrc.contiguous().to(dev)
            self.dg = None if dwavelet is None else table(dwavelet).contiguous().to(dev)
            self.counts.update(source_rows=len(self.host_rows), source_entries=self.host_rows.entries)
        if sv.receiver_positions is None:
            self.rec = kernels.receiver_nodes([(i + M, j, k) for i, j, k in sv.receivers], lv0)
        else:
            self.rec_tab = kernels.point_tables(*reference.receiver_tables(sv.receiver_positions, N, dt, sv.interp, M),
                                                lv0)
        return mc

    def bind_step(self, m):
        """``step(u1, u2, u, *, first, stat, variant=None, **mode)``: ``ops.kernels.step_medium`` on the coefficient
        level ``m`` with what every step of a driver shares bound (the box, ``h2``, the statistic's planes, the
        wrap, the sponge and ``step_kw``), so that a call names what varies: the three levels, ``first``, the
        stat slot, the variant and the mode keyword. Call it after :meth:`medium`, which completes
        ``step_kw`` and ``taper``."""
        from ..ops import kernels

        N, box = self.solver.problem.N, self.box
        bound = dict(h2=self.h2, stat_i=(self.M, N + self.M), wrap=self.wrap, taper=self.taper, **self.step_kw)

        def step(u1, u2, u, **varies):
            kernels.step_medium(u1, u2, m, u, box, **bound, **varies)

        return step

    def inject(self, u, m, g) -> None:
        """The source terms of one step into ``u``: ``g`` = the step's row of ``self.g`` / ``self.dg``."""
        from ..ops import kernels

        if self.src_rows is not None:
            kernels.inject_rows(u, m, self.src_rows, g, self.wrap)
        else:
            kernels.inject(u, m, self.src, g, self.wrap)

    def record(self, u, out) -> None:
        from ..ops import kernels

        if self.rec_tab is not None:
            kernels.record_weighted(u, self.rec_tab, out)
        else:
            kernels.record(u, self.rec, out)

    def points_extra(self) -> dict:
        return self.solver._points_extra(**self.counts)

    def adjoint_points(self, res, lv0, m):
        """The adjoint pass's end of a level for the residuals ``res`` ``[K+1, R]`` (host): returns
        ``finish_level(mu, n, a_row)``, which injects ``G rho^n`` into the stepped level mu^n (wrap copies
        included) and samples it at the sources into ``a_row``; with off-grid sources it also adds
        ``mu^n[p] val_p(g[n-1])`` to the time sums of the unique source rows (:meth:`source_rows_host`)."""
        from ..ops import kernels, reference

        sv, M, dev, wrap = self.solver, self.M, self.dev, self.wrap
        N, dt = sv.problem.N, sv.problem.torch_dtype
        if sv.receiver_positions is None:
            anodes, atab = reference.adjoint_source_table(res, sv.receivers, N, self.tt, M)
            adj, ag = kernels.source_nodes(anodes, lv0), atab.to(dev)
            inject = lambda mu, n: kernels.inject(mu, m, adj, ag[n], wrap)  # noqa: E731
        else:  # the compact [K+1, R] residual table; the rows' weights carry G
            arows = reference.point_rows(sv.receiver_positions, N, dt, sv.interp, M, self.tt)
            adj, ag = kernels.row_list(arows, lv0), res.contiguous().to(dev)
            self.counts.update(receiver_rows=len(arows), receiver_entries=arows.entries)
            inject = lambda mu, n: kernels.inject_rows(mu, m, adj, ag[n], wrap)  # noqa: E731
        self.sacc = None
        if sv.source_positions is None:
            snodes = kernels.receiver_nodes(reference.source_unique_nodes(sv.sources, N, M), lv0)
            sample = lambda mu, n, a_row: kernels.record(mu, snodes, a_row)  # noqa: E731
        else:
            gtab = kernels.point_tables(*reference.receiver_tables(sv.source_positions, N, dt, sv.interp, M,
                                                                   over_taper=self.tt), lv0)
            self.sacc = torch.zeros(self.src_rows.unique, dtype=dt, device=dev)

            def sample(mu, n, a_row):
                kernels.record_weighted(mu, gtab, a_row)
                kernels.rows_dot(mu, self.src_rows, self.g[n - 1], self.sacc)

        def finish_level(mu, n, a_row):
            inject(mu, n)
            sample(mu, n, a_row)

        return finish_level

    def source_rows_host(self):
        """(rows, sacc) for ``ops.reference.finish_gradient_medium`` after the adjoint pass, None with a
        node list of sources."""
        return None if self.sacc is None else (self.host_rows, self.sacc.cpu())


def _nonfinite_layer(stat, upto: int | None = None):
    """The first layer whose non-finite flag is set in the statistics ``stat`` (of the layers
    0..``upto``; None: all), or None: one read-back of the flags."""
    flags = (stat[2::3] if upto is None else stat[2:3 * upto + 3:3]).cpu()
    bad = (flags != 0).nonzero()
    return int(bad[0]) if len(bad) else None


def _require_finite(stat, who: str, what: str) -> None:
    n = _nonfinite_layer(stat)
    if n is not None:
        raise RuntimeError(f"{who}: non-finite values in the {what} at layer {n}")


@dataclass
class MediumBorn:
    traces: torch.Tensor     # [K+1, R], those of run()
    dtraces: torch.Tensor    # [K+1, R], the first-order change of the traces; row 0 is 0
    du_final: torch.Tensor   # (N+1)^3, the perturbation field at the last layer
    max_abs_du: list         # [K+1]: max |du| over the stencil nodes, before the step's source terms
    total_ms: float          # wall time of the whole call
    extra: dict = field(default_factory=dict)  # levels; "hip" also loop_ms, the device time of the time loop


def born_levels(density: bool = False, ddensity: bool = False) -> int:
    """Number of grid levels the "hip" schedule of :meth:`MediumSolver.born` holds: the rings of the
    background and the perturbation field (3 each), m, dm and one q level; ``density``: one more, the
    buoyancy; ``ddensity`` (a density perturbation, which needs a density model): 11, the buoyancy and
    its perturbation, the scattering term taking q's place."""
    return 11 if ddensity else 9 + bool(density)


@dataclass
class MediumGradient:
    misfit: float               # J = 1/2 sum_{n >= 1} sum_r (trace - observed)^2
    grad_speed2: torch.Tensor   # (N+1)^3, dJ/dspeed2 on the unique nodes (plane N = plane 0, faces 0)
    grad_wavelet: torch.Tensor  # [K, S]
    traces: torch.Tensor        # [K+1, R], those of run()
    total_ms: float             # wall time of the whole call
    # segment, levels, recomputed_steps, wrt_density; "hip" also forward_ms / reverse_ms, the device time of the
    # two passes
    extra: dict = field(default_factory=dict)
    # gradient(wrt_density=True): (N+1)^3, dJ/drho at fixed speed2 on the stencil nodes (plane N = plane 0, faces 0)
    grad_density: torch.Tensor | None = None
    # gradient(illumination=True): (N+1)^3 each, sum_n q^n q^n and the pseudo-Hessian diagonal for speed2
    # (plane N = plane 0, faces 0)
    illumination: torch.Tensor | None = None
    pseudo_hessian_speed2: torch.Tensor | None = None


def precondition(grad, pseudo_hessian, eps: float = 1e-3):
    """``grad / (pseudo_hessian + eps * pseudo_hessian.max())``: a gradient such as ``grad_speed2`` scaled
    by the diagonal ``pseudo_hessian_speed2`` of :meth:`MediumSolver.gradient` (``illumination=True``),
    the water level ``eps > 0`` keeping the nodes the sources hardly reach finite. The pseudo-Hessian
    must have a positive maximum. The output follows the convention of the two inputs (plane N a
    copy of plane 0, the Dirichlet faces 0)."""
    g, ph = torch.as_tensor(grad), torch.as_tensor(pseudo_hessian)
    if tuple(g.shape) != tuple(ph.shape):
        raise ValueError(f"grad and pseudo_hessian must have the same shape, not {tuple(g.shape)} and "
                         f"{tuple(ph.shape)}")
    if not (isinstance(eps, (int, float)) and math.isfinite(eps) and eps > 0):
        raise ValueError(f"eps must be finite and > 0, not {eps!r}")
    top = ph.max() if ph.numel() else None
    if top is None or not bool(torch.isfinite(top)) or not bool(top > 0):
        raise ValueError("pseudo_hessian must have a finite, positive maximum")
    return g / (ph + eps * top)


def gradient_levels(K: int, segment: int, density: bool = False, wrt_density: bool = False,
                    illumination: bool = False) -> int:
    """Number of grid levels the "hip" schedule of :meth:`MediumSolver.gradient` holds for K
    timesteps cut into segments of ``segment`` steps (steps 2..K): the forward ring (3), m, acc, the
    q buffer (one level per step of a segment), a checkpoint pair per segment but the last, and,
    when there is anything to recompute, a second ring for the adjoint field. ``density``: one more
    level, the buoyancy of a problem with a density model. ``wrt_density``: the levels u^n of a segment's
    steps beside its q buffer and the accumulator of the density gradient, ``min(segment, K - 1) + 1`` more.
    ``illumination``: one more level, the accumulator of the source illumination."""
    K, segment = int(K), int(segment)
    if K < 1 or segment < 1:
        raise ValueError(f"need K >= 1 and segment >= 1, not K={K} segment={segment}")
    nseg = -(-(K - 1) // segment)
    nq = min(segment, K - 1)
    return (5 + bool(density) + bool(illumination) + nq + (nq + 1 if wrt_density else 0)
            + (2 * (nseg - 1) + 3 if nseg > 1 else 0))


def gradient_dft_levels(F: int, density: bool = False) -> int:
    """Number of grid levels the "hip" schedule of :meth:`MediumSolver.gradient_dft` holds for F
    frequencies, whatever K is: one ring (3) that the forward and then the adjoint field run in, m, the
    scratch level of q, and the real and imaginary parts of the spectra of q and of mu (4 F).
    ``density``: one more level, the buoyancy."""
    F = int(F)
    if F < 1:
        raise ValueError(f"need F >= 1 frequencies, not {F}")
    return 5 + 4 * F + bool(density)


def best_gradient_segment(K: int, wrt_density: bool = False, illumination: bool = False) -> int:
    """The segment length with the fewest levels (``wrt_density``: of the schedule with the density
    gradient; ``illumination``: with the illumination's level, the same for every segment); every schedule
    recomputes less than one extra forward pass, and of equal level counts the longer segment (less
    recomputation) wins."""
    return min(range(1, max(K - 1, 1) + 1),
               key=lambda s: (gradient_levels(K, s, wrt_density=wrt_density, illumination=illumination), -s))
