#!/usr/bin/env python3
"""Throughput of the variable-speed medium step (k_march_m) beside its yardstick, k_march.

    python tools/bench_medium.py [--N 512] [--steps 100] [--dtypes fp64,fp32]
                                 [--variants default,plain,r2,r2nt] [--repeat 3] [--no-yardstick]
                                 [--taper WIDTH] [--order 2,4,8] [--density]
    python tools/bench_medium.py --gradient [--N 512] [--steps 100] [--dtypes fp64,fp32] [--segment 10]
                                 [--order 2,8] [--kernels-only] [--density] [--illum]
    python tools/bench_medium.py --gradient --density --wrt-density [--N 512] [--steps 100] [--segment 10]
    python tools/bench_medium.py --born [--N 512] [--steps 100] [--dtypes fp64,fp32] [--order 2,4,8]
                                 [--kernels-only] [--density]
    python tools/bench_medium.py --born --density --ddensity [--N 512] [--steps 100] [--kernels-only]
    python tools/bench_medium.py --positions R [--N 256] [--steps 100] [--dtypes fp64,fp32] [--repeat 3]
    python tools/bench_medium.py --dft F[,F...] [--N 512] [--steps 100] [--dtypes fp64,fp32] [--segment 10]
                                 [--kernels-only]

For each dtype: a random smooth speed2, one source, one receiver; per variant one warm-up run()
and `--repeat` timed ones (device events around the time loop: step + inject + record per layer),
the variants alternating inside each repeat. The yardstick is the constant-speed solver with
`--kernel march --math exact` at the same N and steps in the same process. Effective bandwidth
counts the bytes the algorithm needs: u1, u2, m read and u written once per node (32 B in fp64,
16 B in fp32) for the medium step, 24 B / 12 B for the yardstick. `--taper WIDTH` adds, per dtype
and variant, the same run with the absorbing sponge `sponge_taper(prob, WIDTH)` (the TAPER
instantiation of k_march_m, the same bytes), alternating with the untapered one inside each
repeat, and reports its ms/step and the ratio tapered / untapered. Prints one JSON line.

`--gradient` measures the adjoint-state gradient instead (MediumSolver.gradient), per dtype in one
process: ms/step of the plain step, the save step (+ lap_out: 40 B per node in fp64 against 32) and
the image step (+ q, acc read, acc written: 56 B), `--repeat` rounds of 20 launches each, the three
alternating inside each round, with and without a sponge of 16 nodes; then, alternating as well,
one forward run() and gradient() with every q stored (segment = steps) and with `--segment`: the
device time of the passes beside run()'s time loop, and the wall time of the whole call. `--illum`
adds the illum step (+ h read and written: 48 B per node in fp64, 1.5 times the plain step) and the
save+illum step (56 B, 1.4 times the save step: `ratio_to_save`) to the alternating kernel rounds, and
gradient(illumination=True) beside each schedule (`passes_vs_without`: its two passes over those of
the same schedule without the flag, in the same job).

`--born` measures Born (linearised) modelling instead (MediumSolver.born), with `--gradient`'s layout:
ms/step of the plain step, the save step and the Born step (+ q, dm read: 48 B per node in fp64
against 32, so the byte count predicts 1.5 times the plain step), the three alternating inside each
round, with and without the sponge; then, alternating as well, one forward run() and one born()
(per step a save step, a Born step, the injections and two records): the device time of the time
loops. `--kernels-only` skips the runs; `--order` and `--density` as for `--gradient`.

`--order 2,4,8` runs every configuration at each of the space orders (4 and 8: k_march_mh), the
orders alternating inside each repeat in the one job, and reports per row the order and the ratio
of its time to order 2's (`vs_order2`, when 2 is among the orders). The byte count per node does
not depend on the order; the speed keeps the Courant number at 0.9 of the smallest limit among
the orders. The ablation variants exist for order 2 only. With `--gradient` the kernel rounds and
the schedules run at each order; `--kernels-only` skips the schedules.

`--density` (order 2 must be among the orders) adds the variable-density step (k_march_mb) with a
two-layer rho (1 above, 2 below the plane k = N / 2), alternating with the constant-density step
inside each repeat. It reads one more stream, the buoyancy: 40 B per node in fp64 (20 B in fp32)
against 32 (16), so the byte count predicts 1.25 times the constant-density time (`vs_constant`
beside `expected_ratio`); with `--gradient` 48 B (save) and 64 B (image) against 40 and 56. The speed
is lowered by the factor 1.5 that the two-layer interface adds to the Courant number's
max kappa bhat. Works with `--taper` and `--gradient --kernels-only`.

`--gradient --density --wrt-density` measures the density gradient dJ/drho (order 2), per dtype in
one process: ms per call of k_face_corr (a, v read, acc read and written: 32 B per node in fp64, 16 B
in fp32) beside the plain constant-density step k_march_m (the same byte count) and the plain density
step k_march_mb, `--repeat` rounds of 20 launches each, the three alternating inside each round; then
gradient() of the two-layer density problem with and without `wrt_density`, with every level stored
(segment = steps) and with `--segment`, the four alternating inside each repeat: the device time of
the two passes, the wall time, the levels held and their size. A schedule that does not fit the free
device memory is reported as such.

`--born --density --ddensity` measures Born modelling with a density perturbation (order 2), per dtype in
one process, three arms alternating inside each round: the scatter step (u1, u2, m, b, db, dm read, u and
s written: 64 B per node in fp64) and the Born-add step (u1, u2, m, b, s read, u written: 48 B); the save
step (48 B) and the Born step (56 B) of the same density problem; the plain density step k_march_mb
(40 B), the yardstick, with and without the sponge. Then, alternating as well, the time loops of
born(ddensity=...), born(dspeed2=...) and run() of the two-layer density problem. `--kernels-only` skips
the loops.

`--positions R` measures off-grid sources and receivers (k_inject_rows, k_record_w, k_rows_dot), per dtype
in one process at N = 256 unless `--N` says otherwise: R receivers on a square array in the plane
z = N / 8, each jittered by up to half a cell per axis, and one off-grid source, against the same
problem with every point rounded to its nearest node (k_inject, k_record). Inside each repeat run() and
gradient() (every q stored, so the reverse pass recomputes nothing) of the two alternate; reported are
ms per step of run()'s time loop (step + inject + record) and of gradient()'s reverse pass (image step
+ the injection of R residuals + the record at the source, with positions also the row dot), the
difference positions - nodes, and that difference over the node-list step.

`--dft F[,F...]` (frequencies in Hz) measures the on-the-fly Fourier transform, per dtype in one process:
ms per call of k_dft_acc with one frequency (u read, re and im read and written: 40 B per node in fp64)
and with a full launch of NF (8 + 32 NF B), beside the plain step k_march_m and k_face_corr (32 B each),
`--repeat` rounds of 20 launches each, the four alternating inside each round. Then run() without
frequencies, with them, and with them at dft_every = 4, alternating inside each repeat: the device time of
the time loop. Then gradient_dft() with the frequencies beside gradient(segment=`--segment`) and gradient()
with every q stored, alternating as well: the levels held, their size, and the device time of the two
passes. `--kernels-only` skips the runs.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def smooth_speed2(N: int, lo: float, hi: float, seed: int = 7):
    """Random 9^3 control values, trilinearly interpolated to (N+1)^3, periodic in x."""
    import torch
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(seed)
    ctl = torch.rand(1, 1, 9, 9, 9, generator=g, dtype=torch.float64)
    ctl[:, :, -1] = ctl[:, :, 0]
    s = F.interpolate(ctl, size=(N + 1,) * 3, mode="trilinear", align_corners=True)[0, 0]
    s = lo + (hi - lo) * s
    s[N] = s[0]
    return s.contiguous()


def two_layer_density(N: int):
    """rho = 1 above and 2 below the plane k = N / 2."""
    import torch

    rho = torch.ones((N + 1,) * 3, dtype=torch.float64)
    rho[:, :, N // 2:] = 2.0
    return rho


def positions_bench(a) -> int:
    import math

    import torch

    import wave3d

    N, K, R = a.N, a.steps, a.positions
    h = 3.1415926535 / N
    hi = (0.9 * wave3d.cfl_limit(2) * h * K) ** 2
    speed2 = smooth_speed2(N, 0.5 * hi, hi)
    side = max(1, math.isqrt(R))
    g = torch.Generator().manual_seed(5)
    q = torch.arange(R)
    lo, span = 0.1 * N, 0.8 * N / max(side - 1, 1)
    rpos = torch.stack([lo + span * (q % side), lo + span * ((q // side) % side),
                        torch.full((R,), N / 8.0, dtype=torch.float64)], 1).to(torch.float64)
    rpos = rpos + (torch.rand(R, 3, generator=g, dtype=torch.float64) - 0.5)
    mid = N // 2
    spos = torch.tensor([[mid + 0.3, mid - 0.4, mid + 0.2]], dtype=torch.float64)
    out = {"N": N, "steps": K, "receivers": R, "device": torch.cuda.get_device_name(0), "runs": []}
    for dtype in a.dtypes.split(","):
        prob = wave3d.MediumProblem(N, speed2, timesteps=K, dtype=dtype)
        w = wave3d.ricker(4.0, 0.25, K, prob.tau).reshape(K, 1)
        sol = {"nodes": wave3d.MediumSolver(prob, "hip", sources=[tuple(int(v) for v in spos[0].round())], wavelet=w,
                                            receivers=[tuple(int(v) for v in r) for r in rpos.round()]),
               "positions": wave3d.MediumSolver(prob, "hip", source_positions=spos, wavelet=w,
                                                receiver_positions=rpos)}
        obs = 0.9 * sol["nodes"].run().traces  # warm-up as well
        fwd, rev, extra = {k: [] for k in sol}, {k: [] for k in sol}, {}
        for k in sol:
            sol[k].gradient(obs, segment=K)
        for _ in range(a.repeat):
            for k in sol:
                r = sol[k].run()
                assert not r.aborted and math.isfinite(max(r.max_abs_u)), "the benchmark run diverged"
                fwd[k].append(r.total_ms / K)
            for k in sol:
                gr = sol[k].gradient(obs, segment=K)
                rev[k].append(gr.extra["reverse_ms"] / K)
                extra[k] = gr.extra
            print(f"bench_medium: {dtype} forward {fwd['nodes'][-1]:.4f} / {fwd['positions'][-1]:.4f} ms per step, "
                  f"reverse {rev['nodes'][-1]:.4f} / {rev['positions'][-1]:.4f} (nodes / positions)",
                  file=sys.stderr, flush=True)
        row = {"dtype": dtype, "courant": round(prob.courant, 4)}
        for name, t in (("forward", fwd), ("reverse", rev)):
            a0, b0 = min(t["nodes"]), min(t["positions"])
            row[name] = {"nodes_ms_per_step": round(a0, 4), "positions_ms_per_step": round(b0, 4),
                         "extra_ms_per_step": round(b0 - a0, 4), "extra_over_nodes": round((b0 - a0) / a0, 4),
                         "all_nodes": [round(v, 4) for v in t["nodes"]],
                         "all_positions": [round(v, 4) for v in t["positions"]]}
        row.update({k: extra["positions"][k] for k in ("interp", "source_rows", "source_entries", "receiver_rows",
                                                      "receiver_entries")})
        out["runs"].append(row)
    print(json.dumps(out))
    return 0


def dft_bench(a) -> int:
    import math

    import torch

    import wave3d
    from wave3d.ops import kernels, reference

    N, K = a.N, a.steps
    freqs = [float(v) for v in a.dft.split(",")]
    F = len(freqs)
    h = 3.1415926535 / N
    hi = (0.9 * wave3d.cfl_limit(2) * h * K) ** 2
    speed2 = smooth_speed2(N, 0.5 * hi, hi)
    nodes = float(N + 1) ** 3
    NF = kernels.dft_frequencies_per_launch()
    out = {"N": N, "steps": K, "device": torch.cuda.get_device_name(0), "frequencies": freqs,
           "frequencies_per_launch": NF, "kernels": [], "run": [], "gradient": []}
    dev = torch.device("cuda", 0)
    for dtype in a.dtypes.split(","):
        es = 8 if dtype == "fp64" else 4
        prob = wave3d.MediumProblem(N, speed2, timesteps=K, dtype=dtype)
        dt = prob.torch_dtype
        c = reference.tables(N, K)[4]
        h2 = (c["hx2"], c["hy2"], c["hz2"])
        box, wrap = (1, N + 1, 1, N - 1, 1, N - 1), [N, 0, 2, N + 2]

        # the kernels on one set of levels (smooth values, nothing denormal)
        g = torch.Generator().manual_seed(1)
        seed = torch.rand(N + 1, N + 1, generator=g, dtype=torch.float64).to(dt).to(dev)
        u1, u2, m, u, acc = (kernels.alloc_level(N + 3, N + 1, N + 1, dt, dev) for _ in range(5))
        re = [kernels.alloc_level(N + 3, N + 1, N + 1, dt, dev) for _ in range(NF)]
        im = [kernels.alloc_level(N + 3, N + 1, N + 1, dt, dev) for _ in range(NF)]
        m.copy_(reference.medium_coefficient(speed2, c["tau"], N, dt))
        for t in (u1, u2):
            t[:, 1:N, 1:N] = seed[1:N, 1:N]
        ctab, stab = (t.contiguous().to(dev) for t in reference.dft_tables([1.0 + f for f in range(NF)], range(K), c["tau"], dt))
        stat = kernels.new_err(1, device=dev)
        step = dict(first=False, h2=h2, stat=stat, stat_i=(1, N + 1), wrap=wrap)
        # (bytes per node / element size, call); k_dft_acc with 1 and with NF frequencies per launch
        arms = {"k_march_m": (4, lambda: kernels.step_medium(u1, u2, m, u, box, **step)),
                "k_face_corr": (4, lambda: kernels.face_correlation(u1, u2, acc, box, h2=h2)),
                "k_dft_acc_1": (5, lambda: kernels.dft_accumulate(u1, re[:1], im[:1], box, ctab[7, :1], stab[7, :1])),
                f"k_dft_acc_{NF}": (1 + 4 * NF, lambda: kernels.dft_accumulate(u1, re, im, box, ctab[7], stab[7]))}
        reps = 20
        ms = {k: [] for k in arms}
        for rnd in range(a.repeat + 1):  # round 0 warms up
            for name, (_, fn) in arms.items():  # the arms alternate inside each round
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                acc.zero_()
                for t in re + im:
                    t.zero_()
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                if rnd:
                    ms[name].append(e0.elapsed_time(e1) / reps)
        for name, (bpn, _) in arms.items():
            best = min(ms[name])
            out["kernels"].append({"dtype": dtype, "kernel": name, "ms_per_call": round(best, 4),
                                   "all_ms": [round(v, 4) for v in ms[name]], "bytes_per_node": bpn * es,
                                   "eff_tb_per_s": round(bpn * es * nodes / (best * 1e-3) / 1e12, 3),
                                   "vs_k_march_m": round(best / min(ms["k_march_m"]), 4),
                                   "expected_vs_k_march_m": bpn / 4})
            print(f"bench_medium: {dtype} {name}: {best:.4f} ms/call", file=sys.stderr, flush=True)
        del u1, u2, m, u, acc, re, im, arms, step
        torch.cuda.empty_cache()
        if a.kernels_only:
            continue

        w = wave3d.ricker(4.0, 0.25, K, prob.tau).reshape(K, 1)
        mid = N // 2
        sol = wave3d.MediumSolver(prob, "hip", sources=[(mid, mid, mid)], wavelet=w,
                                  receivers=[(mid - K // 5, mid, mid), (mid, mid - K // 4, mid + 3)],
                                  taper=wave3d.sponge_taper(prob, 16))
        obs = 0.9 * sol.run().traces  # warm-up
        lb = kernels.level_bytes(N + 3, N + 1, N + 1, dt)

        # run() with and without the frequencies, at dft_every 1 and 4, alternating inside each repeat
        runs = {"plain": {}, "dft_every_1": dict(frequencies=freqs), "dft_every_4": dict(frequencies=freqs, dft_every=4)}
        loop = {k: [] for k in runs}
        for rnd in range(a.repeat + 1):  # round 0 warms up
            for name, kw in runs.items():
                r = sol.run(**kw)
                assert not r.aborted and math.isfinite(max(r.max_abs_u)), "the benchmark run diverged"
                assert (r.spectra is not None) == bool(kw)
                if rnd:
                    loop[name].append(round(r.total_ms, 2))
                print(f"bench_medium: {dtype} run {name}: {r.total_ms:.2f} ms", file=sys.stderr, flush=True)
                del r
                torch.cuda.empty_cache()
        for name in runs:
            best = min(loop[name])
            out["run"].append({"dtype": dtype, "run": name, "loop_ms": best, "ms_per_step": round(best / K, 4),
                               "vs_plain": round(best / min(loop["plain"]), 3), "loop_ms_all": loop[name],
                               "levels": 4 + (2 * F if name != "plain" else 0)})

        # gradient_dft beside gradient(segment) and gradient() with every q stored
        cfgs = {"gradient_dft": lambda: sol.gradient_dft(obs, freqs),
                f"segment_{a.segment}": lambda: sol.gradient(obs, segment=a.segment),
                "all_q": lambda: sol.gradient(obs, segment=K)}
        rows = {n: [] for n in cfgs}
        for _ in range(a.repeat):
            for name, fn in cfgs.items():
                r = fn()
                assert math.isfinite(r.misfit) and r.misfit > 0 and float(r.grad_speed2.abs().max()) > 0
                rows[name].append({"wall_ms": round(r.total_ms, 1), "forward_ms": round(r.extra["forward_ms"], 2),
                                   "reverse_ms": round(r.extra["reverse_ms"], 2), "levels": r.extra["levels"],
                                   "gb": round(r.extra["levels"] * lb / 1e9, 1),
                                   "recomputed_steps": r.extra["recomputed_steps"]})
                print(f"bench_medium: {dtype} {name}: {rows[name][-1]}", file=sys.stderr, flush=True)
                del r
                torch.cuda.empty_cache()
        run_ms = min(loop["plain"])
        for name in cfgs:
            best = min(rows[name], key=lambda v: v["forward_ms"] + v["reverse_ms"])
            passes = best["forward_ms"] + best["reverse_ms"]
            out["gradient"].append({"dtype": dtype, "schedule": name, **best, "passes_ms": round(passes, 2),
                                    "run_loop_ms": run_ms, "passes_vs_run": round(passes / run_ms, 3),
                                    "wall_ms_all": [v["wall_ms"] for v in rows[name]]})
        del sol
        torch.cuda.empty_cache()
    print(json.dumps(out))
    return 0


def density_gradient_bench(a) -> int:
    import math

    import torch

    import wave3d
    from wave3d.ops import kernels, reference

    N, K = a.N, a.steps
    h = 3.1415926535 / N
    hi = (0.9 * wave3d.cfl_limit(2) * h * K) ** 2 / 1.5
    speed2 = smooth_speed2(N, 0.5 * hi, hi)
    rho = two_layer_density(N)
    nodes = float(N + 1) ** 3
    out = {"N": N, "steps": K, "device": torch.cuda.get_device_name(0), "density": "two layers: 1, 2",
           "kernels": [], "gradient": []}
    dev = torch.device("cuda", 0)
    for dtype in a.dtypes.split(","):
        es = 8 if dtype == "fp64" else 4
        prob = wave3d.MediumProblem(N, speed2, timesteps=K, dtype=dtype, density=rho)
        dt = prob.torch_dtype
        c = reference.tables(N, K)[4]
        h2 = (c["hx2"], c["hy2"], c["hz2"])
        box, wrap = (1, N + 1, 1, N - 1, 1, N - 1), [N, 0, 2, N + 2]

        # the kernels on one set of levels (smooth values, nothing denormal)
        g = torch.Generator().manual_seed(1)
        seed = torch.rand(N + 1, N + 1, generator=g, dtype=torch.float64).to(dt).to(dev)
        u1, u2, m, u, acc, bu = (kernels.alloc_level(N + 3, N + 1, N + 1, dt, dev) for _ in range(6))
        m.copy_(reference.medium_coefficient(speed2, c["tau"], N, dt, 1, rho))
        bu.copy_(reference.buoyancy_field(rho, N, dt))
        for t in (u1, u2):
            t[:, 1:N, 1:N] = seed[1:N, 1:N]
        stat = kernels.new_err(1, device=dev)
        step = dict(first=False, h2=h2, stat=stat, stat_i=(1, N + 1), wrap=wrap)
        arms = {"k_march_m": (4, lambda: kernels.step_medium(u1, u2, m, u, box, **step)),
                "k_march_mb": (5, lambda: kernels.step_medium(u1, u2, m, u, box, buoyancy=bu, **step)),
                "k_face_corr": (4, lambda: kernels.face_correlation(u1, u2, acc, box, h2=h2))}
        reps = 20
        ms = {k: [] for k in arms}
        for rnd in range(a.repeat + 1):  # round 0 warms up
            for name, (_, fn) in arms.items():  # the arms alternate inside each round
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                acc.zero_()
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                if rnd:
                    ms[name].append(e0.elapsed_time(e1) / reps)
        for name, (bpn, _) in arms.items():
            best = min(ms[name])
            out["kernels"].append({"dtype": dtype, "kernel": name, "ms_per_call": round(best, 4),
                                   "all_ms": [round(v, 4) for v in ms[name]], "bytes_per_node": bpn * es,
                                   "eff_tb_per_s": round(bpn * es * nodes / (best * 1e-3) / 1e12, 3),
                                   "vs_k_march_m": round(best / min(ms["k_march_m"]), 4),
                                   "expected_vs_k_march_m": bpn / 4})
            print(f"bench_medium: {dtype} {name}: {best:.4f} ms/call", file=sys.stderr, flush=True)
        del u1, u2, m, u, acc, bu, arms, step
        torch.cuda.empty_cache()
        if a.kernels_only:
            continue

        w = wave3d.ricker(4.0, 0.25, K, prob.tau).reshape(K, 1)
        mid = N // 2
        sol = wave3d.MediumSolver(prob, "hip", sources=[(mid, mid, mid)], wavelet=w,
                                  receivers=[(mid - K // 5, mid, mid), (mid, mid - K // 4, mid + 3)],
                                  taper=wave3d.sponge_taper(prob, 16))
        obs = 0.9 * sol.run().traces  # warm-up
        lb = kernels.level_bytes(N + 3, N + 1, N + 1, dt)
        cfgs = [(f"{n}{'_wrt_density' if wd else ''}", seg, wd) for n, seg in (("all_stored", K), (f"segment_{a.segment}",
                a.segment)) for wd in (False, True)]
        rows = {n: [] for n, _, _ in cfgs}
        for _ in range(a.repeat):
            for name, seg, wd in cfgs:
                levels = wave3d.gradient_levels(K, seg, density=True, wrt_density=wd)
                try:
                    r = sol.gradient(obs, segment=seg, wrt_density=wd)
                except RuntimeError as e:
                    if "bytes of device memory are free" not in str(e):
                        raise
                    rows[name].append({"levels": levels, "gb": round(levels * lb / 1e9, 1), "fits": False})
                    print(f"bench_medium: {dtype} {name}: does not fit", file=sys.stderr, flush=True)
                    continue
                assert math.isfinite(r.misfit) and r.misfit > 0 and r.extra["levels"] == levels
                assert (r.grad_density is not None) == wd
                rows[name].append({"wall_ms": round(r.total_ms, 1), "forward_ms": round(r.extra["forward_ms"], 2),
                                   "reverse_ms": round(r.extra["reverse_ms"], 2), "levels": levels,
                                   "gb": round(levels * lb / 1e9, 1), "recomputed_steps": r.extra["recomputed_steps"],
                                   "fits": True})
                print(f"bench_medium: {dtype} {name}: {rows[name][-1]}", file=sys.stderr, flush=True)
                del r
                torch.cuda.empty_cache()
        for name, seg, wd in cfgs:
            ok = [v for v in rows[name] if v["fits"]]
            if not ok:
                out["gradient"].append({"dtype": dtype, "schedule": name, **rows[name][0]})
                continue
            best = min(ok, key=lambda v: v["forward_ms"] + v["reverse_ms"])
            row = {"dtype": dtype, "schedule": name, **best, "passes_ms": round(best["forward_ms"] + best["reverse_ms"], 2),
                   "wall_ms_all": [v["wall_ms"] for v in ok]}
            base = [x for x in out["gradient"] if x["dtype"] == dtype and x["schedule"] == name[:-len("_wrt_density")]]
            if wd and base and base[0]["fits"]:
                row["passes_vs_without"] = round(row["passes_ms"] / base[0]["passes_ms"], 3)
            out["gradient"].append(row)
        del sol
        torch.cuda.empty_cache()
    print(json.dumps(out))
    return 0


def born_density_bench(a) -> int:
    import math

    import torch

    import wave3d
    from wave3d.ops import kernels, reference

    N, K = a.N, a.steps
    h = 3.1415926535 / N
    hi = (0.9 * wave3d.cfl_limit(2) * h * K) ** 2 / 1.5
    speed2 = smooth_speed2(N, 0.5 * hi, hi)
    rho = two_layer_density(N)
    drho = 0.01 * smooth_speed2(N, -1.0, 1.0, seed=11)
    nodes = float(N + 1) ** 3
    out = {"N": N, "steps": K, "device": torch.cuda.get_device_name(0), "density": "two layers: 1, 2",
           "kernels": [], "born": []}
    dev = torch.device("cuda", 0)
    for dtype in a.dtypes.split(","):
        es = 8 if dtype == "fp64" else 4
        prob = wave3d.MediumProblem(N, speed2, timesteps=K, dtype=dtype, density=rho)
        dt = prob.torch_dtype
        c = reference.tables(N, K)[4]
        h2 = (c["hx2"], c["hy2"], c["hz2"])
        box, wrap = (1, N + 1, 1, N - 1, 1, N - 1), [N, 0, 2, N + 2]
        sponge = wave3d.sponge_taper(prob, 16)
        taper = tuple(t.to(dev) for t in reference.taper_tables(sponge, N, dt))

        # the kernels on one set of levels (smooth values, nothing denormal)
        g = torch.Generator().manual_seed(1)
        seed = torch.rand(N + 1, N + 1, generator=g, dtype=torch.float64).to(dt).to(dev)
        u1, u2, m, u, x, q, dm, bu, db = (kernels.alloc_level(N + 3, N + 1, N + 1, dt, dev) for _ in range(9))
        m.copy_(reference.medium_coefficient(speed2, c["tau"], N, dt, 1, rho))
        dm.copy_(reference.medium_coefficient(speed2, c["tau"], N, dt, 1, drho))
        bu.copy_(reference.buoyancy_field(rho, N, dt))
        db.copy_(reference.dbuoyancy_field(drho, rho, N, dt))
        for t in (u1, u2, q):
            t[:, 1:N, 1:N] = seed[1:N, 1:N]
        stat = kernels.new_err(1, device=dev)
        # (bytes per node / element size, keywords); the three arms in the order they alternate
        arms = {"scatter": (8, dict(scatter=(x, dm, db))), "born_add": (6, dict(born_add=q)),
                "save": (6, dict(lap_out=x)), "born": (7, dict(born=(q, dm))), "plain": (5, {})}
        reps = 20
        for tp_name in ("", "sponge"):
            ms = {k: [] for k in arms}
            for rnd in range(a.repeat + 1):  # round 0 warms up
                for name, (_, kw) in arms.items():  # the arms alternate inside each round
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        kernels.step_medium(u1, u2, m, u, box, first=False, h2=h2, stat=stat, stat_i=(1, N + 1),
                                            wrap=wrap, buoyancy=bu, taper=taper if tp_name else None, **kw)
                    e1.record()
                    e1.synchronize()
                    if rnd:
                        ms[name].append(e0.elapsed_time(e1) / reps)
            for name, (bpn, _) in arms.items():
                best = min(ms[name])
                out["kernels"].append({"dtype": dtype, "mode": name, "sponge": bool(tp_name),
                                       "ms_per_step": round(best, 4), "all_ms": [round(v, 4) for v in ms[name]],
                                       "bytes_per_node": bpn * es, "expected_ratio": bpn / 5,
                                       "ratio_to_plain": round(best / min(ms["plain"]), 4),
                                       "eff_tb_per_s": round(bpn * es * nodes / (best * 1e-3) / 1e12, 3)})
                print(f"bench_medium: {dtype} {name} {tp_name}: {best:.4f} ms/step", file=sys.stderr, flush=True)
        del u1, u2, m, u, x, q, dm, bu, db, arms, taper
        torch.cuda.empty_cache()
        if a.kernels_only:
            continue

        w = wave3d.ricker(4.0, 0.25, K, prob.tau).reshape(K, 1)
        mid = N // 2
        sol = wave3d.MediumSolver(prob, "hip", sources=[(mid, mid, mid)], wavelet=w,
                                  receivers=[(mid - K // 5, mid, mid), (mid, mid - K // 4, mid + 3)], taper=sponge)
        ds = 0.01 * speed2
        loops = {"born_ddensity": lambda: sol.born(ddensity=drho), "born": lambda: sol.born(ds),
                 "run": lambda: sol.run()}
        rows = {n: [] for n in loops}
        for rnd in range(a.repeat + 1):  # round 0 warms up
            for name, fn in loops.items():
                r = fn()
                if name == "run":
                    ms_loop = r.total_ms
                else:
                    assert math.isfinite(float(r.dtraces.abs().max())) and float(r.dtraces.abs().max()) > 0
                    ms_loop = r.extra["loop_ms"]
                del r
                if rnd:
                    rows[name].append(round(ms_loop, 2))
                print(f"bench_medium: {dtype} {name}: {ms_loop:.2f} ms", file=sys.stderr, flush=True)
                torch.cuda.empty_cache()
        best = {n: min(v) for n, v in rows.items()}
        out["born"].append({"dtype": dtype, "run_loop_ms": best["run"], "born_loop_ms": best["born"],
                            "born_ddensity_loop_ms": best["born_ddensity"],
                            "born_vs_run": round(best["born"] / best["run"], 3),
                            "born_ddensity_vs_run": round(best["born_ddensity"] / best["run"], 3),
                            "born_ddensity_vs_born": round(best["born_ddensity"] / best["born"], 3),
                            "levels": wave3d.born_levels(density=True),
                            "levels_ddensity": wave3d.born_levels(density=True, ddensity=True),
                            "born_ddensity_loop_ms_all": rows["born_ddensity"], "born_loop_ms_all": rows["born"]})
        del sol
        torch.cuda.empty_cache()
    print(json.dumps(out))
    return 0


def gradient_bench(a) -> int:
    import math

    import torch

    import wave3d
    from wave3d.ops import kernels, reference

    N, K = a.N, a.steps
    h = 3.1415926535 / N
    orders = [int(v) for v in a.order.split(",")]
    hi = (0.9 * min(wave3d.cfl_limit(o) for o in orders) * h * K) ** 2 / (1.5 if a.density else 1.0)
    speed2 = smooth_speed2(N, 0.5 * hi, hi)
    rho = two_layer_density(N) if a.density else None
    nodes = float(N + 1) ** 3
    out = {"N": N, "steps": K, "orders": orders, "device": torch.cuda.get_device_name(0), "kernels": [],
           "born" if a.born else "gradient": []}
    third = "born" if a.born else "image"
    illum = a.illum and not a.born
    if a.density:
        out["density"] = "two layers: 1, 2"
        if not a.kernels_only:
            raise SystemExit("--gradient / --born with --density: the kernel rounds only (add --kernels-only)")
        orders = orders + ["2d"]  # the density step at order 2, a configuration of its own
    dev = torch.device("cuda", 0)
    for dtype in a.dtypes.split(","):
        es = 8 if dtype == "fp64" else 4
        probs = {o: wave3d.MediumProblem(N, speed2, timesteps=K, dtype=dtype, space_order=o) for o in orders
                 if o != "2d"}
        dt = probs[orders[0]].torch_dtype
        c = reference.tables(N, K)[4]
        h2 = (c["hx2"], c["hy2"], c["hz2"])
        sponge = wave3d.sponge_taper(probs[orders[0]], 16)

        # the three kernels on one set of levels per order (values of a short run, so nothing is denormal)
        g = torch.Generator().manual_seed(1)
        seed = torch.rand(N + 1, N + 1, generator=g, dtype=torch.float64).to(dt).to(dev)
        sets = {}
        for o in orders:
            M = 1 if o == "2d" else o // 2
            lv = [kernels.alloc_level(N + 1 + 2 * M, N + 1, N + 1, dt, dev) for _ in range(7 if illum else 6)]
            lv[2].copy_(reference.medium_coefficient(speed2, c["tau"], N, dt, M, rho if o == "2d" else None))
            for t in (lv[0], lv[1], lv[5]):
                t[:, 1:N, 1:N] = seed[1:N, 1:N]
            wrap = []
            for gh in range(1, M + 1):
                wrap += [N + M - gh, M - gh, M + gh, N + M + gh]
            sets[o] = dict(lv=lv, box=(M, N + M, 1, N - 1, 1, N - 1), wrap=wrap, stat_i=(M, N + M),
                           kw={} if o in (2, "2d") else dict(order=o, mirror=(0, N, 0, N)),
                           taper=tuple(t.to(dev) for t in reference.taper_tables(sponge, N, dt, M)))
            if o == "2d":
                sets[o]["kw"] = dict(buoyancy=kernels.alloc_level(N + 3, N + 1, N + 1, dt, dev))
                sets[o]["kw"]["buoyancy"].copy_(reference.buoyancy_field(rho, N, dt))
        stat = kernels.new_err(1, device=dev)
        reps = 20
        for tp_name in ("", "sponge"):
            modes = ("plain", "save", third) + (("illum", "save_illum") if illum else ())
            ms = {(k, o): [] for k in modes for o in orders}
            for rnd in range(a.repeat + 1):  # round 0 warms up
                for name in modes:
                    for o in orders:  # the orders alternate inside each round
                        S = sets[o]
                        u1, u2, m, u, x, q = S["lv"][:6]
                        hl = S["lv"][6] if illum else None
                        kw = {"plain": {}, "save": {"lap_out": x}, "image": {"image": (q, x)},
                              "born": {"born": (q, x)}, "illum": {"illum": hl},
                              "save_illum": {"lap_out": x, "illum": hl}}[name]
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        x.zero_()
                        if illum:
                            hl.zero_()
                        if name == "born":  # x is dm here: smooth values instead of zeros
                            x.copy_(q)
                        e0.record()
                        for _ in range(reps):
                            kernels.step_medium(u1, u2, m, u, S["box"], first=False, h2=h2, stat=stat,
                                                stat_i=S["stat_i"], wrap=S["wrap"],
                                                taper=S["taper"] if tp_name else None, **kw, **S["kw"])
                        e1.record()
                        e1.synchronize()
                        if rnd:
                            ms[(name, o)].append(e0.elapsed_time(e1) / reps)
            for o in orders:
                for name, bpn in ((("plain", 4), ("save", 5), ("born", 6) if a.born else ("image", 7))
                                  + ((("illum", 6), ("save_illum", 7)) if illum else ())):
                    best = min(ms[(name, o)])
                    if o == "2d":
                        bpn += 1  # the buoyancy stream
                    row = {"dtype": dtype, "order": 2 if o == "2d" else o, "mode": name, "sponge": bool(tp_name),
                           "ms_per_step": round(best, 4), "all_ms": [round(v, 4) for v in ms[(name, o)]],
                           "bytes_per_node": bpn * es, "expected_ratio": bpn / (5 if o == "2d" else 4),
                           "ratio_to_plain": round(best / min(ms[("plain", o)]), 4),
                           "eff_tb_per_s": round(bpn * es * nodes / (best * 1e-3) / 1e12, 3)}
                    if o == "2d":
                        row["density"] = True
                        row["vs_constant"] = round(best / min(ms[(name, 2)]), 4)
                        row["expected_vs_constant"] = round(bpn / (bpn - 1), 4)
                    elif 2 in orders:
                        row["vs_order2"] = round(best / min(ms[(name, 2)]), 4)
                    if name == "save_illum":
                        row["ratio_to_save"] = round(best / min(ms[("save", o)]), 4)
                        row["expected_ratio_to_save"] = round(bpn / (bpn - 2), 4)
                    out["kernels"].append(row)
                    print(f"bench_medium: {dtype} order {o} {name} {tp_name}: {best:.4f} ms/step", file=sys.stderr,
                          flush=True)
        del sets, lv, u1, u2, m, u, x, q, S, hl
        torch.cuda.empty_cache()
        if a.kernels_only:
            continue

        if a.born:  # born() beside one forward run(), per order
            w = wave3d.ricker(4.0, 0.25, K, probs[orders[0]].tau).reshape(K, 1)
            mid = N // 2
            sols = {o: wave3d.MediumSolver(probs[o], "hip", sources=[(mid, mid, mid)], wavelet=w,
                                           receivers=[(mid - K // 5, mid, mid), (mid, mid - K // 4, mid + 3)],
                                           taper=sponge) for o in orders}
            ds = 0.01 * speed2
            rows = {(n, o): [] for n in ("run", "born") for o in orders}
            for rnd in range(a.repeat + 1):  # round 0 warms up
                for name in ("run", "born"):
                    for o in orders:
                        if name == "run":
                            ms_loop = sols[o].run().total_ms
                        else:
                            r = sols[o].born(ds)
                            assert math.isfinite(float(r.dtraces.abs().max())) and float(r.dtraces.abs().max()) > 0
                            ms_loop = r.extra["loop_ms"]
                            del r
                        if rnd:
                            rows[(name, o)].append(round(ms_loop, 2))
                        print(f"bench_medium: {dtype} order {o} {name}: {ms_loop:.2f} ms", file=sys.stderr, flush=True)
                        torch.cuda.empty_cache()
            for o in orders:
                run_ms, born_ms = min(rows[("run", o)]), min(rows[("born", o)])
                out["born"].append({"dtype": dtype, "order": o, "run_loop_ms": run_ms, "born_loop_ms": born_ms,
                                    "born_vs_run": round(born_ms / run_ms, 3), "levels": wave3d.born_levels(),
                                    "born_loop_ms_all": rows[("born", o)]})
            continue

        # gradient() beside one forward run(), per order
        w = wave3d.ricker(4.0, 0.25, K, probs[orders[0]].tau).reshape(K, 1)
        mid = N // 2
        sols = {o: wave3d.MediumSolver(probs[o], "hip", sources=[(mid, mid, mid)], wavelet=w,
                                       receivers=[(mid - K // 5, mid, mid), (mid, mid - K // 4, mid + 3)],
                                       taper=sponge) for o in orders}
        obs = {o: 0.9 * sols[o].run().traces for o in orders}  # warm-up
        cfgs = [("run", None, False), ("all_q", K, False), (f"segment_{a.segment}", a.segment, False)]
        if illum:  # each schedule is followed by the same one with the illumination
            cfgs = [d for c in cfgs for d in ((c, (c[0] + "_illum", c[1], True)) if c[1] is not None else (c,))]
        rows = {(n, o): [] for n, _, _ in cfgs for o in orders}
        for _ in range(a.repeat):
            for name, seg, il in cfgs:
                for o in orders:
                    if seg is None:
                        r = sols[o].run()
                        rows[(name, o)].append({"loop_ms": round(r.total_ms, 2)})
                    else:
                        r = sols[o].gradient(obs[o], segment=seg, illumination=il)
                        assert math.isfinite(r.misfit) and r.misfit > 0
                        assert (r.illumination is not None) == il and (not il or float(r.illumination.max()) > 0)
                        rows[(name, o)].append({"wall_ms": round(r.total_ms, 1),
                                                "forward_ms": round(r.extra["forward_ms"], 2),
                                                "reverse_ms": round(r.extra["reverse_ms"], 2),
                                                "levels": r.extra["levels"],
                                                "recomputed_steps": r.extra["recomputed_steps"]})
                    print(f"bench_medium: {dtype} order {o} {name}: {rows[(name, o)][-1]}", file=sys.stderr, flush=True)
                    del r
                    torch.cuda.empty_cache()
        for o in orders:
            run_ms = min(v["loop_ms"] for v in rows[("run", o)])
            for name, seg, il in cfgs[1:]:
                best = min(rows[(name, o)], key=lambda v: v["forward_ms"] + v["reverse_ms"])
                passes = best["forward_ms"] + best["reverse_ms"]
                row = {"dtype": dtype, "order": o, "schedule": name, **best, "passes_ms": round(passes, 2),
                       "run_loop_ms": run_ms, "passes_vs_run": round(passes / run_ms, 3),
                       "wall_ms_all": [v["wall_ms"] for v in rows[(name, o)]]}
                if il:  # against the row of the same schedule without the flag, just before it
                    base = out["gradient"][-1]
                    row["passes_vs_without"] = round(passes / base["passes_ms"], 3)
                    row["forward_vs_without"] = round(best["forward_ms"] / base["forward_ms"], 3)
                out["gradient"].append(row)
    print(json.dumps(out))
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--N", type=int, default=None, help="default 512 (--positions: 256)")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--dtypes", default="fp64,fp32")
    ap.add_argument("--variants", default="default")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--taper", type=int, default=0, metavar="WIDTH",
                    help="also time the step with sponge_taper(prob, WIDTH)")
    ap.add_argument("--gradient", action="store_true", help="time the gradient's kernels and schedules instead")
    ap.add_argument("--born", action="store_true", help="time the Born step and born() instead")
    ap.add_argument("--segment", type=int, default=10, help="--gradient: steps per checkpoint segment")
    ap.add_argument("--order", default="2", help="space orders to time, e.g. 2,4,8 (alternating inside each repeat)")
    ap.add_argument("--kernels-only", action="store_true", help="--gradient: the kernel rounds without the schedules")
    ap.add_argument("--density", action="store_true",
                    help="also time the variable-density step (two-layer rho), alternating with the constant-density one")
    ap.add_argument("--wrt-density", action="store_true",
                    help="--gradient --density: time k_face_corr and gradient(wrt_density=True) instead")
    ap.add_argument("--illum", action="store_true",
                    help="--gradient: also time the illum and save+illum steps and gradient(illumination=True)")
    ap.add_argument("--ddensity", action="store_true",
                    help="--born --density: time the scatter and Born-add steps and born(ddensity=...) instead")
    ap.add_argument("--positions", type=int, default=0, metavar="R",
                    help="time off-grid sources and receivers instead: R receivers and one source, run() and gradient()")
    ap.add_argument("--dft", default="", metavar="F[,F...]",
                    help="time k_dft_acc, run(frequencies=...) and gradient_dft() with these frequencies (Hz) instead")
    a = ap.parse_args(argv)
    if a.N is None:
        a.N = 256 if a.positions else 512

    import math

    import torch

    import wave3d

    if not torch.cuda.is_available():
        print("bench_medium: no HIP device (timings are only taken on the GPU)", file=sys.stderr)
        return 2
    N, K = a.N, a.steps
    orders = [int(v) for v in a.order.split(",")]
    if not orders or any(o not in (2, 4, 8) for o in orders):
        ap.error("--order: a comma-separated list of 2, 4, 8")
    if a.density and 2 not in orders:
        ap.error("--density: order 2 must be among the orders")
    if a.illum and (not a.gradient or a.wrt_density):
        ap.error("--illum goes with --gradient (without --wrt-density)")
    if a.dft:
        if a.gradient or a.born or a.density or a.positions or orders != [2]:
            ap.error("--dft is a measurement of its own (order 2, no other mode)")
        return dft_bench(a)
    if a.positions:
        if a.positions < 1 or a.gradient or a.born or a.density or orders != [2]:
            ap.error("--positions R >= 1 is a measurement of its own (order 2, no other mode)")
        return positions_bench(a)
    if a.wrt_density:
        if not (a.gradient and a.density) or orders != [2]:
            ap.error("--wrt-density goes with --gradient --density at order 2")
        return density_gradient_bench(a)
    if a.born and a.gradient:
        ap.error("--born and --gradient are separate measurements")
    if a.ddensity:
        if not (a.born and a.density) or orders != [2]:
            ap.error("--ddensity goes with --born --density at order 2")
        return born_density_bench(a)
    if a.gradient or a.born:
        return gradient_bench(a)
    variants = a.variants.split(",")
    # speed2 <= hi keeps the Courant number at 0.9 of the limit for T = 1 (order 2: 1/sqrt(3); the
    # smallest limit among the orders)
    h = 3.1415926535 / N
    # (--density: the two-layer interface raises max kappa bhat by the factor 1.5)
    hi = (0.9 * min(wave3d.cfl_limit(o) for o in orders) * h * K) ** 2 / (1.5 if a.density else 1.0)
    speed2 = smooth_speed2(N, 0.5 * hi, hi)
    rho = two_layer_density(N) if a.density else None
    nodes = float(N + 1) ** 3
    out = {"N": N, "steps": K, "orders": orders, "device": torch.cuda.get_device_name(0), "runs": []}
    for dtype in a.dtypes.split(","):
        es = 8 if dtype == "fp64" else 4
        probs = {o: wave3d.MediumProblem(N, speed2, timesteps=K, dtype=dtype, space_order=o) for o in orders}
        prob = probs[orders[0]]
        dprob = wave3d.MediumProblem(N, speed2, timesteps=K, dtype=dtype, density=rho) if a.density else None
        w = wave3d.ricker(4.0, 0.25, K, prob.tau).reshape(K, 1)
        mid = N // 2

        sponge = wave3d.sponge_taper(prob, a.taper) if a.taper > 0 else None

        def solver(v, tapered, order, dens=False):
            return wave3d.MediumSolver(dprob if dens else probs[order], "hip", sources=[(mid, mid, mid)], wavelet=w,
                                       receivers=[(mid // 2, mid, mid)], variant=None if v == "default" else v,
                                       taper=sponge if tapered else None)

        # the ablation variants are k_march_m's: order 2 only
        cfgs = [(v, t, o, False) for v in variants for t in ((False, True) if sponge is not None else (False,))
                for o in orders if o == 2 or v == "default"]
        # the density step follows its constant-density counterpart inside each repeat
        cfgs = [d for c in cfgs for d in ((c, c[:3] + (True,)) if a.density and c[2] == 2 and c[0] == "default" else (c,))]
        ms = {c: [] for c in cfgs}
        for c in cfgs:
            solver(*c).run()  # warm-up
        for _ in range(a.repeat):
            for c in cfgs:
                r = solver(*c).run()
                assert not r.aborted and math.isfinite(max(r.max_abs_u)), "the benchmark run diverged"
                ms[c].append(r.total_ms)
                print(f"bench_medium: {dtype} order {c[2]} {c[0]}{' taper' if c[1] else ''}{' density' if c[3] else ''}: "
                      f"{r.total_ms:.2f} ms",
                      file=sys.stderr, flush=True)
        for c in cfgs:
            best = min(ms[c])
            bpn = 5 if c[3] else 4
            row = {"kernel": "k_march_mb" if c[3] else "k_march_m" if c[2] == 2 else "k_march_mh", "order": c[2],
                   "variant": c[0], "dtype": dtype, "courant": round((dprob if c[3] else prob).courant, 4),
                   "loop_ms": [round(t, 3) for t in ms[c]], "ms_per_step": round(best / K, 4),
                   "mpts_per_s": round(nodes * K / best / 1e3, 1), "bytes_per_node": bpn * es,
                   "eff_tb_per_s": round(bpn * es * nodes * K / (best * 1e-3) / 1e12, 3)}
            if c[1]:
                row["taper"] = a.taper
                row["vs_untapered"] = round(best / min(ms[(c[0], False, c[2], c[3])]), 4)
            if c[3]:
                row["density"] = True
                row["vs_constant"] = round(best / min(ms[c[:3] + (False,)]), 4)
                row["expected_vs_constant"] = 1.25
            elif (c[0], c[1], 2, False) in ms:
                row["vs_order2"] = round(best / min(ms[(c[0], c[1], 2, False)]), 4)
            out["runs"].append(row)
        if not a.no_yardstick:
            yp = wave3d.WaveProblem(N, timesteps=K, dtype=dtype)
            r = wave3d.WaveSolver(yp, "hip", kernel="march", device=0).run(repeat=a.repeat, warmup=1)
            mp = r.mpts_per_s_best
            out["runs"].append({"kernel": "k_march", "variant": r.kernel, "dtype": dtype,
                                "solve_ms": [round(t, 3) for t in r.solve_ms],
                                "ms_per_step": round(nodes / mp / 1e3, 4), "mpts_per_s": round(mp, 1),
                                "bytes_per_node": 3 * es, "eff_tb_per_s": round(3 * es * mp * 1e6 / 1e12, 3)})
    for d in (x for x in out["runs"] if x["kernel"] in ("k_march_m", "k_march_mh", "k_march_mb")):
        y = [x for x in out["runs"] if x["kernel"] == "k_march" and x["dtype"] == d["dtype"]]
        if y:
            d["bw_vs_k_march"] = round(d["eff_tb_per_s"] / y[0]["eff_tb_per_s"], 3)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
