"""The two mode tables of the medium step held together on the GPU: every keyword combination of
tests/test_medium_modes_cpu.py through ops.kernels.step_medium, and every mode through the native entry point
with the mode named and exactly its grids, one grid too few, one grid too many.

Everything refused is refused on the host, before any launch: the outputs are filled with a sentinel and
must keep it. What is accepted runs on a dense 12 x 12 x 12 level and the box (4, 7, 4, 7, 4, 7), which
every space order accepts without mirror faces; the other medium tests check what the kernels compute.
"""
import itertools

import pytest
import torch

from test_gpu_medium import H2, _rand
from test_medium_modes_cpu import MODES, ORDERS, VARIANTS, cases, expected

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -7.0
SHAPE = (12, 12, 12)
BOX = (4, 7, 4, 7, 4, 7)
# the native entry point's grids of each mode, and which grids a step writes
GRIDS = dict(plain=(), save=("lap_out",), image=("q", "acc"), born=("q", "dm"), scatter=("s_out", "dm", "db"),
             born_add=("sadd",), illum=("illum",), save_illum=("lap_out", "illum"))
ALL_GRIDS = ("lap_out", "q", "acc", "dm", "db", "s_out", "sadd", "illum")
WRITTEN = ("u", "lap_out", "acc", "s_out", "illum")
VARIANT_CODES = {None: -1, "plain": 0, "nt": 1, "r2": 2, "r2nt": 3}


class _Grids:
    """The levels and one grid per name of the native entry point; the written ones hold the sentinel."""

    def __init__(self, dtype):
        self.t = {name: _rand(SHAPE, dtype, seed, -1.0, 1.0).to(DEV)
                  for seed, name in enumerate(("u1", "u2", "q", "dm", "db", "sadd"), 1)}
        self.t["m"] = _rand(SHAPE, dtype, 11, 1e-4, 6e-4).to(DEV)
        self.t["b"] = _rand(SHAPE, dtype, 12, 0.3, 2.0).to(DEV)
        for name in WRITTEN:
            self.t[name] = torch.full(SHAPE, SENT, dtype=dtype, device=DEV)

    def __getitem__(self, name):
        return self.t[name]

    def keywords(self, given):
        """The mode keywords ``given`` of ops.kernels.step_medium with their grids."""
        t = self.t
        kw = dict(lap_out=t["lap_out"], image=(t["q"], t["acc"]), born=(t["q"], t["dm"]),
                  scatter=(t["s_out"], t["dm"], t["db"]), born_add=t["sadd"], illum=t["illum"])
        return {k: kw[k] for k in given}

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((self.t[name] == SENT).all()) for name in WRITTEN)

    def ran(self, written):
        """Whether the step wrote u and the grids ``written`` at every box node and nothing else; the
        sentinels return."""
        torch.cuda.synchronize()
        i0, i1, j0, j1, k0, k1 = BOX
        ok = True
        for name in ("u",) + tuple(written):
            box = self.t[name][i0:i1 + 1, j0:j1 + 1, k0:k1 + 1]
            ok = ok and not bool((box == SENT).any())
            box.fill_(SENT)
        return ok and self.untouched()


def _written(mode):
    return [g for g in GRIDS[mode] if g in WRITTEN]


def test_step_medium_keyword_cases(C):
    """All 3840 cases through the Python wrapper: a refused one raises ValueError and writes nothing, an
    accepted one runs."""
    from wave3d.ops import kernels

    g = _Grids(torch.float64)
    stat = kernels.new_err(1)
    accepted = 0
    for case in cases():
        given, first, buoyancy, order, variant = case
        mode = expected(*case)
        kw = dict(first=first, h2=H2, stat=stat, stat_i=(BOX[0], BOX[1]), order=order, variant=variant,
                  buoyancy=g["b"] if buoyancy else None, **g.keywords(given))
        if mode is None:
            with pytest.raises(ValueError):
                kernels.step_medium(g["u1"], g["u2"], g["m"], g["u"], BOX, **kw)
            continue
        assert g.untouched(), f"a refused call before {case} wrote to an output"
        kernels.step_medium(g["u1"], g["u2"], g["m"], g["u"], BOX, **kw)
        assert g.ran(_written(mode)), case
        accepted += 1
    assert g.untouched() and accepted == 52


def _native_args(g, stat):
    gv = [*SHAPE, SHAPE[2], SHAPE[1] * SHAPE[2]]
    return [g["u1"].data_ptr(), g["u2"].data_ptr(), g["m"].data_ptr(), g["u"].data_ptr(), gv, [list(BOX)], BOX[0],
            BOX[1], [], list(H2), stat.data_ptr(), 0, torch.cuda.current_stream().cuda_stream]


def test_launcher_mode_cases(C):
    """Every mode x first x buoyancy x order x variant through the native entry point, the mode named and
    exactly its grids given. The launcher's rules, written out: a mode other than plain is a leapfrog step
    and at order 2 of variant 1; scatter and Born-add need b; b needs order 2 and variant 1; at orders 4 and
    8 the variant is ignored. So it accepts everything that step_medium accepts."""
    from wave3d.ops import kernels

    g = _Grids(torch.float64)
    stat = kernels.new_err(1)
    args = _native_args(g, stat)
    accepted = 0
    for given, mode in MODES.items():
        grids = {name: g[name].data_ptr() for name in GRIDS[mode]}
        for first, buoyancy, order, variant in itertools.product((True, False), (False, True), ORDERS, VARIANTS):
            code = VARIANT_CODES[variant]
            runs = C.medium_variant() if code < 0 else code
            ok = ((mode == "plain" or not first)
                  and (mode not in ("scatter", "born_add") or buoyancy)
                  and (not buoyancy or (order == 2 and runs == 1))
                  and (mode == "plain" or order != 2 or runs == 1))
            assert ok or expected(given, first, buoyancy, order, variant) is None
            kw = dict(variant=code, order=order, b=g["b"].data_ptr() if buoyancy else 0, **grids)
            if not ok:
                with pytest.raises(C.Wave3dError):
                    C.k_step_medium_f64(first, *args, C.medium_modes[mode], **kw)
                continue
            assert g.untouched(), f"a refused call before {mode, first, buoyancy, order, variant} wrote to an output"
            C.k_step_medium_f64(first, *args, C.medium_modes[mode], **kw)
            assert g.ran(_written(mode)), (mode, first, buoyancy, order, variant)
            accepted += 1
    assert g.untouched() and accepted > 52


def test_launcher_wants_exactly_the_modes_grids(C):
    """A grid of the mode's set missing, each in turn, and a grid outside it given, each in turn: refused. A
    mode value that names no mode: refused."""
    from wave3d.ops import kernels

    g = _Grids(torch.float64)
    stat = kernels.new_err(1)
    args = _native_args(g, stat)
    assert C.medium_modes == {name: q for q, name in enumerate(MODES.values())}
    for mode, names in GRIDS.items():
        grids = {name: g[name].data_ptr() for name in names}
        kw = dict(variant=1, b=g["b"].data_ptr() if mode in ("scatter", "born_add") else 0)
        for missing in names:
            with pytest.raises(C.Wave3dError):
                C.k_step_medium_f64(False, *args, C.medium_modes[mode], **kw,
                                    **{k: v for k, v in grids.items() if k != missing})
        for extra in ALL_GRIDS:
            if extra not in names:
                with pytest.raises(C.Wave3dError):
                    C.k_step_medium_f64(False, *args, C.medium_modes[mode], **kw, **grids,
                                        **{extra: g[extra].data_ptr()})
    for mode in (-1, len(MODES), 1 << 20):
        with pytest.raises(C.Wave3dError):
            C.k_step_medium_f64(False, *args, mode, variant=1)
    with pytest.raises(TypeError):  # the grids go by keyword alone
        C.k_step_medium_f64(False, *args, C.medium_modes["save"], 1, 2, [], 0, 0, 0, 0, g["lap_out"].data_ptr())
    assert g.untouched()


def test_every_mode_runs_in_fp32(C):
    from wave3d.ops import kernels

    g = _Grids(torch.float32)
    stat = kernels.new_err(1)
    for given, mode in MODES.items():
        kernels.step_medium(g["u1"], g["u2"], g["m"], g["u"], BOX, first=False, h2=H2, stat=stat,
                            stat_i=(BOX[0], BOX[1]), buoyancy=g["b"] if mode in ("scatter", "born_add") else None,
                            **g.keywords(given))
        assert g.ran(_written(mode)), mode
