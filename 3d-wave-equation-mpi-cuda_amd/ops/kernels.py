"""Tensor-level access to the hand-written HIP kernels (for numerics tests and tools).

Tensors are dense ``[nx][ny][nz]`` (k contiguous, one ghost layer) on the current HIP
device; they are passed to the native kernels as raw pointers on torch's current stream.
Shapes are validated here *before* any launch (the kernels index with the boxes given).
The solver itself uses an aligned, padded layout (``csrc/hip_kernels.hpp``); these entry
points use pitch = nz, which the kernels accept as well; the medium ops (``step_medium``,
``face_correlation``, ``dft_accumulate``, ``inject``, ``record``, ``inject_rows``, ``record_weighted``, ``rows_dot``) also take
views in that padded layout (``alloc_level``).

The sweep kernels behind ``step``, ``tb3_sweep`` and ``tbn_sweep`` are tested bit for bit, stored values and
both error keys, in fp64 and fp32 and in both math modes, against ``ops.reference`` (the exact-form chains,
and the FMA-form chains built on its software ``fma``); nothing there is compared within a tolerance. What
is not bitwise: the FMA form against the exact form (the same scheme rounded differently), and fp32
against fp64.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import torch

from .._native import load

_U64 = (1 << 64) - 1


def _C():
    return load()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _sfx(t: torch.Tensor) -> str:
    if t.dtype == torch.float64:
        return "f64"
    if t.dtype == torch.float32:
        return "f32"
    raise TypeError(f"unsupported dtype {t.dtype}")


def _check_grid(*ts: torch.Tensor) -> list[int]:
    u = ts[0]
    for t in ts:
        if not t.is_cuda:
            raise ValueError("wave3d kernels need HIP device tensors")
        if t.dim() != 3 or not t.is_contiguous():
            raise ValueError("grids must be contiguous 3-D [nx][ny][nz] tensors")
        if t.shape != u.shape or t.dtype != u.dtype:
            raise ValueError("grid shapes/dtypes differ")
    nx, ny, nz = u.shape
    if min(nx, ny, nz) < 3:
        raise ValueError("grid needs at least one owned node plus ghosts per axis")
    return [nx, ny, nz, nz, ny * nz]


def _check_box(box, gv) -> list[int]:
    i0, i1, j0, j1, k0, k1 = map(int, box)
    nx, ny, nz = gv[0], gv[1], gv[2]
    if not (1 <= i0 and i1 <= nx - 2 and 1 <= j0 and j1 <= ny - 2 and 1 <= k0 and k1 <= nz - 2):
        raise ValueError(f"box {box} outside the owned region of a {nx}x{ny}x{nz} grid")
    return [i0, i1, j0, j1, k0, k1]


def _check_boxes(boxes, gv) -> list[list[int]]:
    """``boxes``: a single box or 1..7 of them, each inside the owned region of the grid view ``gv``."""
    if isinstance(boxes[0], int):
        boxes = [boxes]
    if not 1 <= len(boxes) <= 7:
        raise ValueError("1..7 boxes per launch")
    return [_check_box(b, gv) for b in boxes]


def _check_tables(u, tx, ty, tz):
    nx, ny, nz = u.shape
    for t, n, name in ((tx, nx, "tx"), (ty, ny, "ty"), (tz, nz, "tz")):
        if not t.is_cuda or t.dtype != u.dtype or t.numel() < n or not t.is_contiguous():
            raise ValueError(f"table {name} must be a contiguous {u.dtype} device tensor of >= {n}")


def new_err(layers: int = 1, device=None) -> torch.Tensor:
    """Per-layer error slots (abs key, rel key, non-finite flag), initialised on device."""
    e = torch.empty(layers * 3, dtype=torch.int64, device=device or "cuda")
    _C().k_init_err(e.data_ptr(), layers, _stream())
    return e


def decode_err(err: torch.Tensor) -> list[tuple[float, float, bool]]:
    C = _C()
    v = [int(x) & _U64 for x in err.cpu().tolist()]
    return [(C.decode_max_key(v[q]), C.decode_max_key(v[q + 1]), v[q + 2] != 0)
            for q in range(0, len(v), 3)]


def step(u1, u2, u, boxes, *, first: bool, err_i, tx, ty, tz, coefs, err,
         kernel: str = "march", wrap=None, chunk: int = 0, pack=None) -> None:
    """One leapfrog layer over ``boxes`` (list of (i0,i1,j0,j1,k0,k1), local indices). fp64 and fp32
    results and error keys are bitwise those of ``ops.reference.step``; ``kernel="marchf"`` / ``"march2f"``: the
    --math fma instantiation, bitwise ``ops.reference.taylor_fma_field`` / ``leap_fma_field``.

    coefs = (hx2, hy2, hz2, coef, ct); err_i = (ei0, ei1) rows entering the error;
    wrap = (src0, dst0, src1, dst1) periodic self-wrap planes; pack = ([zbuf0, zbuf1,
    ybuf0, ybuf1] tensors or None, [zk0, zk1, yj0, yj1]).
    """
    gv = _check_grid(u1, u2, u)
    bl = _check_boxes(boxes, gv)
    _check_tables(u, tx, ty, tz)
    if err.dtype != torch.int64 or err.numel() < 3 or not err.is_cuda:
        raise ValueError("err must be >= 3 int64 device slots (new_err())")
    if wrap is not None:
        w = [int(v) for v in wrap]
        for q in range(0, 4, 2):
            if w[q] >= 0 and not (0 <= w[q + 1] < gv[0] and 1 <= w[q] <= gv[0] - 2):
                raise ValueError("bad wrap planes")
    else:
        w = []
    pb, pi = [], []
    if pack is not None:
        bufs, idx = pack
        pb = [b.data_ptr() if b is not None else 0 for b in bufs]
        pi = [int(v) for v in idx]
        nx, ny, nz = u.shape
        for q, b in enumerate(bufs):
            if b is None:
                continue
            need = (nx - 2) * (ny if q < 2 else nz)
            if b.numel() < need or b.dtype != u.dtype:
                raise ValueError("pack buffer too small")
    fn = getattr(_C(), "k_step_" + _sfx(u))
    fn(kernel, bool(first), u1.data_ptr(), u2.data_ptr(), u.data_ptr(), gv, bl, int(err_i[0]),
       int(err_i[1]), w, tx.data_ptr(), ty.data_ptr(), tz.data_ptr(), [float(c) for c in coefs],
       err.data_ptr(), int(chunk), _stream(), pb, pi)


def init(u, box, *, tx, ty, tz, ct0: float, err, wrap=None) -> None:
    gv = _check_grid(u)
    b = _check_box(box, gv)
    _check_tables(u, tx, ty, tz)
    getattr(_C(), "k_init_" + _sfx(u))(u.data_ptr(), gv, b, list(wrap or []), tx.data_ptr(),
                                      ty.data_ptr(), tz.data_ptr(), float(ct0), err.data_ptr(),
                                      _stream())


def zero_faces(u, mask: int) -> None:
    gv = _check_grid(u)
    getattr(_C(), "k_zero_faces_" + _sfx(u))(u.data_ptr(), gv, int(mask), _stream())


def faces(u, ops, to_buf: bool) -> None:
    """ops: list of (buffer, axis in {1,2}, plane index). Pack (to_buf) or unpack."""
    gv = _check_grid(u)
    nx, ny, nz = u.shape
    lst = []
    for buf, axis, index in ops:
        if axis not in (1, 2):
            raise ValueError("faces: axis must be 1 (y) or 2 (z)")
        lim = ny if axis == 1 else nz
        if not 0 <= index < lim:
            raise ValueError("faces: plane index out of range")
        need = (nx - 2) * (nz if axis == 1 else ny)
        if buf.numel() < need or buf.dtype != u.dtype or not buf.is_cuda:
            raise ValueError("faces: buffer too small")
        lst.append((buf.data_ptr(), int(axis), int(index)))
    if len(lst) > 4:
        raise ValueError("at most 4 faces per launch")
    getattr(_C(), "k_faces_" + _sfx(u))(u.data_ptr(), gv, lst, bool(to_buf), _stream())


def _check_grid_g(G: int, *ts: torch.Tensor) -> list[int]:
    """Dense [nx][ny][nz] grids with G ghost layers per side (logical 1..X owned)."""
    u = ts[0]
    for t in ts:
        if not t.is_cuda or t.dim() != 3 or not t.is_contiguous():
            raise ValueError("grids must be contiguous 3-D HIP device tensors")
        if t.shape != u.shape or t.dtype != u.dtype:
            raise ValueError("grid shapes/dtypes differ")
    nx, ny, nz = u.shape
    if min(nx, ny, nz) < 2 * G + 1:
        raise ValueError(f"grid needs at least one owned node plus {G} ghosts per side")
    return [nx, ny, nz, G]


def _check_box_g(box, gv) -> list[int]:
    i0, i1, j0, j1, k0, k1 = (int(v) for v in box)
    X, Y, Z = (gv[a] - 2 * gv[3] for a in range(3))
    if not (1 <= i0 <= i1 <= X and 1 <= j0 <= j1 <= Y and 1 <= k0 <= k1 <= Z):
        raise ValueError(f"box {box} outside the owned region 1..{X} x 1..{Y} x 1..{Z}")
    return [i0, i1, j0, j1, k0, k1]


def tbn_sweep(A, B, O0, O1, boxes, *, depth: int, first: bool, cdom, err_i, tx, ty, tz, coefs, errs,
              rows: int = 2, waves: int = 8, chunk: int = 0, ghost: int | None = None, fma: bool = False,
              delta: bool = False, check_finite: bool = True) -> None:
    """One deep sweep (k_tbn, ``depth`` layers u^m .. u^{m+depth-1}): the first depth-2 layers
    errors only, O0 = u^{m+depth-2}, O1 = u^{m+depth-1}. ``coefs[l]`` = (hx2, hy2, hz2, coef, ct)
    and ``errs[l]`` the error slot of layer m+l. ``delta``: the increment form (depth 4):
    B = d^{m-1}, O0 = d^{m+depth-1}, O1 = u^{m+depth-1}.
    A and B must be finite everywhere, ghosts included: the LDS-DMA staging reads whole frame
    rows (a row's neighbours past the box), and a masked Dirichlet node computes 0 * value, so a
    NaN there would spread into the interior (the solver's levels are zeroed at
    allocation). ``check_finite=False`` skips that one check and nothing else: for the tests that plant
    a non-finite value on purpose and compare where it goes with the oracle (non-finite values are
    data to the kernel, not faults; tests/test_gpu_sweep_bits.py). Leave it on everywhere else.

    What is bitwise (tests/test_gpu_tb_kernels.py): the stored layers and both error keys, in fp64 and
    fp32, equal ``ops.reference.chained_layers`` / ``chained_delta_layers`` (exact form) and
    ``chained_layers_fma`` / ``chained_delta_layers_fma`` with ``rel_key_fma`` (``fma=True``)."""
    ghost = depth if ghost is None else ghost
    gv = _check_grid_g(ghost, A, B, O0, O1)
    if check_finite and not (bool(torch.isfinite(A).all()) and bool(torch.isfinite(B).all())):
        raise ValueError("k_tbn: A and B must be finite everywhere (ghost and padding cells included)")
    if ghost < depth:
        raise ValueError("k_tbn needs ghost depth >= depth")
    if isinstance(boxes[0], int):
        boxes = [boxes]
    bl = [_check_box_g(b, gv) for b in boxes]
    ok = (_C().tbn_delta_supported(int(depth), int(rows), int(waves), bool(fma), A.dtype == torch.float32)
          if delta else _C().tbn_supported(int(depth), int(rows), int(waves), bool(fma), A.dtype == torch.float32))
    if not ok:
        raise ValueError(f"unsupported depth={depth} tile rows={rows} waves={waves} fma={fma} delta={delta}")
    if len(coefs) != depth or len(errs) != depth:
        raise ValueError("one coefficient set and one error slot per layer")
    for t in (tx, ty, tz):
        if not t.is_cuda or t.dtype != A.dtype or t.numel() < max(gv[:3]):
            raise ValueError("analytic tables must be device tensors covering the grid")
    fn = getattr(_C(), "k_tbn_" + _sfx(A))
    fn(int(depth), int(rows), int(waves), bool(fma), bool(first), A.data_ptr(), B.data_ptr(), O0.data_ptr(),
       O1.data_ptr(), gv, bl, [int(v) for v in cdom], int(err_i[0]), int(err_i[1]), tx.data_ptr(), ty.data_ptr(),
       tz.data_ptr(), [[float(c) for c in co] for co in coefs], [e.data_ptr() for e in errs], int(chunk), _stream(),
       bool(delta))


def tb3_sweep(A, B, D, E, boxes, *, first: bool, cdom, err_i, tx, ty, tz, coefs_c, coefs_d,
              coefs_e, err_c, err_d, err_e, rows: int = 2, waves: int = 8, chunk: int = 0,
              ghost: int = 3, fma: bool = False) -> None:
    """One three-layer sweep (k_tb3): C = u^m (errors only), D = u^{m+1}, E = u^{m+2}.
    ``fma``: the --math fma instantiation (coef/h^2 folded; not bitwise with the exact form, but a fixed
    sequence of rounded operations of its own: bitwise equal to ``ops.reference.chained_layers_fma``)."""
    gv = _check_grid_g(ghost, A, B, D, E)
    if ghost < 3:
        raise ValueError("k_tb3 needs ghost depth >= 3")
    if isinstance(boxes[0], int):
        boxes = [boxes]
    bl = [_check_box_g(b, gv) for b in boxes]
    if not _C().tb_supported(3, rows, waves, fm=bool(fma)):
        raise ValueError(f"unsupported tile rows={rows} waves={waves} fma={fma}")
    for t in (tx, ty, tz):
        if not t.is_cuda or t.dtype != A.dtype or t.numel() < max(gv[:3]):
            raise ValueError("analytic tables must be device tensors covering the grid")
    fn = getattr(_C(), "k_tb3_" + _sfx(A))
    fn(int(rows), int(waves), bool(fma), bool(first), A.data_ptr(), B.data_ptr(), D.data_ptr(), E.data_ptr(),
       gv, bl, [int(v) for v in cdom], int(err_i[0]), int(err_i[1]), tx.data_ptr(),
       ty.data_ptr(), tz.data_ptr(), [float(c) for c in coefs_c], [float(c) for c in coefs_d],
       [float(c) for c in coefs_e], err_c.data_ptr(), err_d.data_ptr(), err_e.data_ptr(),
       int(chunk), _stream())


# ---- heterogeneous medium (csrc/hip_medium.hip) -----------------------------------------

def alloc_level(nx: int, ny: int, nz: int, dtype, device=None) -> torch.Tensor:
    """A zeroed ``[nx][ny][nz]`` level in the solver's aligned layout (``csrc/hip_kernels.hpp``):
    a view into a padded allocation whose row pitch is a multiple of 128 B and whose elements
    ``(., ., k=1)`` are 128-B aligned, so every 64-lane k-tile (k = 1 + 64 t) is whole cache lines."""
    if min(nx, ny, nz) < 3:
        raise ValueError("grid needs at least one owned node plus ghosts per axis")
    es = torch.empty((), dtype=dtype).element_size()
    line = 128 // es
    sj = -(-nz // line) * line
    si = ny * sj
    off = line - 1  # the k = 0 column sits in front of the aligned k = 1
    buf = torch.zeros(off + nx * si, dtype=dtype, device=device or "cuda")
    if buf.data_ptr() % 128:
        raise RuntimeError("allocator returned a buffer that is not 128-B aligned")
    return buf.as_strided((nx, ny, nz), (si, sj, 1), off)


def level_bytes(nx: int, ny: int, nz: int, dtype) -> int:
    """Size of the allocation behind one :func:`alloc_level` view."""
    es = torch.empty((), dtype=dtype).element_size()
    line = 128 // es
    return (line - 1 + nx * ny * (-(-nz // line) * line)) * es


def _check_grid_strided(*ts: torch.Tensor) -> list[int]:
    """Grids that are dense or padded views (last stride 1), all with the same strides."""
    u = ts[0]
    for t in ts:
        if not t.is_cuda:
            raise ValueError("wave3d kernels need HIP device tensors")
        if t.dim() != 3:
            raise ValueError("grids must be 3-D [nx][ny][nz] tensors")
        if t.shape != u.shape or t.dtype != u.dtype or t.device != u.device:
            raise ValueError("grid shapes/dtypes/devices differ")
        if t.stride() != u.stride():
            raise ValueError(f"grid strides differ: {t.stride()} vs {u.stride()}")
    nx, ny, nz = u.shape
    if min(nx, ny, nz) < 3:
        raise ValueError("grid needs at least one owned node plus ghosts per axis")
    si, sj, sk = u.stride()
    if sk != 1 or sj < nz or si < ny * sj:
        raise ValueError(f"grid strides {u.stride()}: k must be contiguous, rows and planes must not overlap")
    if si * u.element_size() >= 1 << 31:
        raise ValueError("a plane must be smaller than 2 GiB")
    _sfx(u)
    return [nx, ny, nz, sj, si]


def _check_wrap(wrap, gv) -> list[int]:
    if wrap is None:
        return []
    w = [int(v) for v in wrap]
    if len(w) % 2 or len(w) > 16:
        raise ValueError("wrap = (src, dst, ...) pairs, at most 8")
    for q in range(0, len(w), 2):
        if w[q] >= 0 and not (0 <= w[q + 1] < gv[0] and 1 <= w[q] <= gv[0] - 2):
            raise ValueError(f"bad wrap planes {w[q]} -> {w[q + 1]}")
    return w


class NodeList:
    """Validated (i, j, k) nodes of a grid, uploaded once (int32 ``[n][3]`` on the device)."""

    def __init__(self, nodes, shape, device, *, owned: bool, distinct: bool):
        nx, ny, nz = shape
        lst = [tuple(int(v) for v in nd) for nd in nodes]
        lo, hi = (1, 2) if owned else (0, 1)
        for nd in lst:
            if len(nd) != 3 or not all(lo <= v <= n - hi for v, n in zip(nd, (nx, ny, nz))):
                raise ValueError(f"node {nd} outside the {'owned region' if owned else 'storage'} of a "
                                 f"{nx}x{ny}x{nz} grid")
        if distinct and len(set(lst)) != len(lst):
            dup = sorted(nd for nd in set(lst) if lst.count(nd) > 1)
            raise ValueError(f"node {dup[0]} named more than once")
        self.shape, self.nodes, self.owned, self.distinct = (nx, ny, nz), lst, owned, distinct
        self.dev = torch.tensor(lst, dtype=torch.int32).reshape(len(lst), 3).to(device)

    def __len__(self):
        return len(self.nodes)


def _node_list(nodes, u, *, owned: bool, distinct: bool) -> NodeList:
    if isinstance(nodes, NodeList):
        if nodes.shape != tuple(u.shape) or nodes.dev.device != u.device:
            raise ValueError("node list was built for another grid")
        if (owned and not nodes.owned) or (distinct and not nodes.distinct):
            raise ValueError("node list was not validated for this use")
        return nodes
    return NodeList(nodes, u.shape, u.device, owned=owned, distinct=distinct)


def source_nodes(nodes, u) -> NodeList:
    """Nodes for :func:`inject`: inside the owned region of ``u`` and distinct."""
    return NodeList(nodes, u.shape, u.device, owned=True, distinct=True)


def receiver_nodes(nodes, u) -> NodeList:
    """Nodes for :func:`record`: anywhere in the storage of ``u``."""
    return NodeList(nodes, u.shape, u.device, owned=False, distinct=False)


_MEDIUM_VARIANTS = {None: -1, "plain": 0, "nt": 1, "r2": 2, "r2nt": 3}


def _check_taper(taper, u) -> list[int]:
    if taper is None:
        return [0, 0, 0]
    if len(taper) != 3:
        raise ValueError("taper = (gx, gy, gz)")
    for t, n, name in zip(taper, u.shape, ("gx", "gy", "gz")):
        if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != u.device or t.dtype != u.dtype
                or t.dim() != 1 or t.numel() != n or not t.is_contiguous()):
            raise ValueError(f"taper table {name} must be a contiguous 1-D {u.dtype} tensor of {n} values "
                             f"on {u.device}")
    return [t.data_ptr() for t in taper]


class _MediumMode(NamedTuple):
    """One row of the mode table of :func:`step_medium` (``csrc/hip_medium.hpp`` describes the modes)."""
    name: str                  # its key in the binding's ``medium_modes``
    grids: dict                # the keywords that select it -> the name(s) of the grid(s) each one carries
    taylor: bool = False       # runs on the Taylor start (``first``)
    any_variant: bool = False  # every variant has it; otherwise, at order 2, the default one alone
    buoyancy: bool = False     # needs a buoyancy (k_march_mb alone has it)
    apart: tuple = ()          # (grid, the grids it must not share memory with): written, or read while u is


_LEVELS = ("u", "u1", "u2", "m", "buoyancy")
_MEDIUM_MODES = (
    _MediumMode("plain", {}, taylor=True, any_variant=True),
    _MediumMode("save", dict(lap_out="lap_out")),
    _MediumMode("image", dict(image=("q", "acc"))),
    _MediumMode("born", dict(born=("q", "dm")), apart=(("q", ("u",)), ("dm", ("u",)))),
    _MediumMode("scatter", dict(scatter=("s_out", "dm", "dbuoyancy")), buoyancy=True,
                apart=(("s_out", _LEVELS + ("dm", "dbuoyancy")),)),
    _MediumMode("born_add", dict(born_add="s"), buoyancy=True, apart=(("s", ("u",)),)),
    _MediumMode("illum", dict(illum="illum"), apart=(("illum", _LEVELS),)),
    _MediumMode("save_illum", dict(lap_out="lap_out", illum="illum"), apart=(("illum", _LEVELS + ("lap_out",)),)),
)
_MODE_KEYWORDS = ("lap_out", "image", "born", "scatter", "born_add", "illum")
_MODE_OF_KEYWORDS = {frozenset(r.grids): r for r in _MEDIUM_MODES}
_NATIVE_NAMES = dict(dbuoyancy="db", s="sadd")  # where the native entry point names a mode grid differently


@functools.lru_cache(maxsize=None)  # small-N runs are host-bound; measured in profiles/medium_step_modes.txt
def medium_mode(present: tuple, first: bool, order: int, variant: str | None, buoyancy: bool):
    """The mode of a :func:`step_medium` call and the variant it runs. ``present``: one flag per mode
    keyword, in the order ``lap_out``, ``image``, ``born``, ``scatter``, ``born_add``, ``illum``, saying
    whether it is given; ``buoyancy``: whether one is given. Returns ``(row of the mode table, variant)``
    or raises ``ValueError``. Pure: no tensor and no native module is touched."""
    given = [k for k, flag in zip(_MODE_KEYWORDS, present) if flag]
    if order not in (2, 4, 8):
        raise ValueError(f"space order must be 2, 4 or 8, not {order!r}")
    if variant not in _MEDIUM_VARIANTS:
        raise ValueError(f"unknown variant {variant!r}")
    if order != 2 and variant is not None:
        raise ValueError("the ablation variants exist for order 2 only")
    if buoyancy:
        if order != 2:
            raise ValueError(f"variable density (buoyancy) exists for space order 2 only, not {order!r}")
        if variant not in (None, "nt"):
            raise ValueError(f"variable density (buoyancy) exists for the default variant only, not {variant!r}")
    mode = _MODE_OF_KEYWORDS.get(frozenset(given))
    if mode is None:
        raise ValueError(f"{', '.join(sorted(given))} cannot be combined: a step runs in one mode, selected by "
                         "no mode keyword, by one of them, or by lap_out with illum")
    if mode.buoyancy and not buoyancy:
        raise ValueError(f"{mode.name} mode needs a buoyancy (variable density)")
    if first and not mode.taylor:
        raise ValueError(f"{mode.name} mode: not on the Taylor start (first=True)")
    if not mode.any_variant and variant not in (None, "nt"):
        raise ValueError(f"{mode.name} mode exists for the default variant only, not {variant!r}")
    if order == 2 and (buoyancy or not mode.any_variant):
        variant = "nt"  # by name: the default may have been changed for an ablation run
    return mode, variant


def step_medium(u1, u2, m, u, boxes, *, first: bool, h2, stat, stat_i, wrap=None, chunk: int = 0,
                variant: str | None = None, taper=None, lap_out=None, image=None, order: int = 2,
                mirror=None, buoyancy=None, born=None, scatter=None, born_add=None, illum=None) -> None:
    """One layer of ``u_tt = c^2 (lap u + f)`` over ``boxes``: ``u = (2 u1 - u2) + m lap(u1)``, on
    the Taylor start (``first``) ``u = u1 + (0.5 m) lap(u1)``, with ``m = c^2 tau^2`` per node.
    ``csrc/hip_medium.hpp`` has the arithmetic of every form named here, operation by operation.

    The grids are dense ``[nx][ny][nz]`` tensors or :func:`alloc_level` views with identical
    strides. h2 = (hx2, hy2, hz2); stat = >= 3 int64 slots (``new_err()``): slot 0 receives the
    key of max |u| over the planes stat_i = (ei0, ei1), slot 2 the non-finite flag; wrap as in
    :func:`step`. ``variant`` (ablation; the results are the same bit for bit): "nt" non-temporal
    loads of m with 4 rows per lane (the default, None), "plain" ordinary loads of m, "r2" / "r2nt"
    the same with 2 rows per lane.

    ``taper`` = (gx, gy, gz): the absorbing sponge, 1-D device tensors of exactly nx, ny, nz factors
    in (0, 1] (storage indexing); tables of ones give the undamped bits. None: the undamped kernels.

    ``order`` = 2 (the 7-point Laplacian; ``mirror`` is not used), 4 or 8: the star stencil of half-width
    M = order / 2 (``ops.reference.laplace_star`` has the scheme); ``variant`` must then be None. The box
    and mirror contract, checked here before any launch: the boxes keep M planes from both ends of the
    storage in x. ``mirror = (j_lo, j_hi, k_lo, k_hi)`` names the storage indices of reflecting (Dirichlet)
    faces in y and z, an entry or the whole tuple may be None. The boxes lie strictly inside their faces,
    a pair of faces is at least M apart, every reflected node exists in storage, and on a side without a
    face the boxes keep M nodes from the storage edge.

    ``buoyancy``: a grid ``b = 1 / rho`` (variable density): ``lap(u1)`` becomes ``div(b grad u1)``
    (``ops.reference.laplace_density`` has the scheme) in every form and mode, and ``m = rho c^2 tau^2``.
    Its ghost planes are filled like those of ``u1``; it is never written. For ``order`` 2 and the default
    variant only.

    The mode keywords: a step runs in one mode, selected by none of them (the plain step), by one of them,
    or by ``lap_out`` together with ``illum``. Every mode but the plain one is a leapfrog step
    (``first=False``) of the default variant.
      * ``lap_out`` (save): a grid that receives the Laplacian that entered the update, at the box nodes.
      * ``image = (q, acc)``: ``acc = acc + u1 * q`` at the box nodes (the adjoint-state imaging condition).
      * ``born = (q, dm)``: the step of linearised modelling, ``u`` also receives ``+ dm q``; ``q`` is what
        ``lap_out`` received in the background step, ``dm`` the perturbation of ``m``.
      * ``scatter = (s_out, dm, dbuoyancy)`` (needs ``buoyancy``): the background step that also stores the
        scattering term ``s_out = dm D_b u1 + m D_db u1`` of a density perturbation.
      * ``born_add = s`` (needs ``buoyancy``): the step of the perturbation field, ``u`` also receives ``+ s``.
      * ``illum = h``, alone or with ``lap_out``: also ``h = h + lap * lap`` (the source illumination).
    In save, image, scatter and the illum modes ``u`` and ``stat`` are those of the plain step bit for bit.
    Mode grids match ``u`` in shape, dtype, device and strides; they are read or written at the box nodes
    alone and the wrap applies to ``u`` alone. ``q`` and ``dm`` of ``born`` and ``s`` must not share memory with
    ``u``; ``s_out`` not with any other grid of the call; ``h`` not with ``u``, ``u1``, ``u2``, ``m``, ``buoyancy``
    or ``lap_out``.

    Every violation is a ``ValueError`` before any launch."""
    values = (lap_out, image, born, scatter, born_add, illum)  # in the order of _MODE_KEYWORDS
    mode, variant = medium_mode((lap_out is not None, image is not None, born is not None, scatter is not None,
                                 born_add is not None, illum is not None), first, order, variant, buoyancy is not None)
    grids, native = {}, {}  # the mode's grids by name; their pointers under the native entry point's names
    for key, names in mode.grids.items():
        value = values[_MODE_KEYWORDS.index(key)]
        if isinstance(names, str):
            grids[names] = value
        elif len(value) != len(names):
            raise ValueError(f"{key} = ({', '.join(names)})")
        else:
            grids.update(zip(names, value))
    for name, t in grids.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
        native[_NATIVE_NAMES.get(name, name)] = t.data_ptr()
    if buoyancy is None:
        gv = _check_grid_strided(u1, u2, m, u, *grids.values())
    elif not isinstance(buoyancy, torch.Tensor):
        raise ValueError("buoyancy must be a tensor")
    else:
        gv = _check_grid_strided(u1, u2, m, u, buoyancy, *grids.values())
    if mode.apart:
        named = dict(grids, u=u, u1=u1, u2=u2, m=m)
        if buoyancy is not None:
            named["buoyancy"] = buoyancy
        for name, others in mode.apart:
            _check_spans_apart(name, _grid_span(named[name]), [(o, _grid_span(named[o])) for o in others if o in named],
                               mode.name)
    bl = _check_boxes(boxes, gv)
    mir = []
    if order != 2:
        from .reference import _check_star_box

        no = _C().no_mirror
        for b in bl:
            mir = [no if f is None else int(f) for f in _check_star_box(gv[:3], b, order // 2, mirror)]
    h2 = [float(v) for v in h2]
    if len(h2) != 3 or not all(v > 0 for v in h2):
        raise ValueError("h2 = (hx2, hy2, hz2), all > 0")
    if stat.dtype != torch.int64 or stat.numel() < 3 or not stat.is_cuda or not stat.is_contiguous():
        raise ValueError("stat must be >= 3 contiguous int64 device slots (new_err())")
    w = _check_wrap(wrap, gv)
    C = _C()
    getattr(C, "k_step_medium_" + _sfx(u))(
        bool(first), u1.data_ptr(), u2.data_ptr(), m.data_ptr(), u.data_ptr(), gv, bl, int(stat_i[0]),
        int(stat_i[1]), w, h2, stat.data_ptr(), int(chunk), _stream(), C.medium_modes[mode.name],
        _MEDIUM_VARIANTS[variant], int(order), mir, *_check_taper(taper, u),
        0 if buoyancy is None else buoyancy.data_ptr(), **native)


def _grid_span(t: torch.Tensor) -> tuple[int, int]:
    """[first byte, one past the last byte) of the memory a grid view covers."""
    n = sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1
    return t.data_ptr(), t.data_ptr() + n * t.element_size()


def _check_spans_apart(name: str, span, others, mode: str | None = None) -> None:
    """Raises if the grid ``name`` with the :func:`_grid_span` ``span`` shares memory with one of ``others``,
    (name, span) pairs; ``mode`` names the mode of :func:`step_medium` in the message."""
    t0, t1 = span
    for other, (o0, o1) in others:
        if t0 < o1 and o0 < t1:
            where = "" if mode is None else f"{mode} mode: "
            raise ValueError(f"{where}{name} shares memory with {other}")


def face_correlation(a, v, acc, boxes, *, h2, chunk: int = 0) -> None:
    """``acc = acc + C(a, v)`` at the nodes of ``boxes`` (``k_face_corr``), the accumulation behind the
    density gradient of the adjoint pass: ``C`` is the sum over a node's six faces of the products of
    the two fields' differences across the face, per axis divided by h2 = (hx2, hy2, hz2)
    (``ops.reference.face_correlation`` has the scheme; fp64 results are bitwise equal to it).

    The grids are dense ``[nx][ny][nz]`` tensors or :func:`alloc_level` views with identical shapes,
    dtypes, devices and strides; the boxes lie inside the owned region (``step_medium``'s contract at
    order 2), so every box node has its six neighbours in storage. ``a`` and ``v`` are never written,
    ``acc`` only at the box nodes, and it must not share memory with ``a`` or ``v``. Every violation is
    a ``ValueError`` before any launch."""
    if not all(isinstance(t, torch.Tensor) for t in (a, v, acc)):
        raise ValueError("a, v and acc must be tensors")
    gv = _check_grid_strided(a, v, acc)
    _check_spans_apart("acc", _grid_span(acc), (("a", _grid_span(a)), ("v", _grid_span(v))))
    bl = _check_boxes(boxes, gv)
    if len(h2) != 3 or not all(float(x) > 0 for x in h2):
        raise ValueError("h2 = (hx2, hy2, hz2), all > 0")
    getattr(_C(), "k_face_corr_" + _sfx(a))(a.data_ptr(), v.data_ptr(), acc.data_ptr(), gv, bl,
                                           [float(x) for x in h2], int(chunk), _stream())


def dft_frequencies_per_launch() -> int:
    """NF, the number of frequencies one ``k_dft_acc`` launch carries on a single read of ``u``."""
    return int(_C().dft_nf)


def dft_accumulate(u, re, im, boxes, c_row, s_row, *, chunk: int = 0) -> None:
    """On-the-fly Fourier accumulation (``k_dft_acc``): ``re[f] = re[f] + u c_row[f]`` and
    ``im[f] = im[f] + u s_row[f]`` at the nodes of ``boxes`` for every frequency f, each product rounded
    before its add (``ops.reference.dft_accumulate`` has the scheme; fp64 and fp32 results are bitwise
    equal to it). ``re`` / ``im``: lists of F levels; ``c_row`` / ``s_row``: contiguous 1-D device tensors of
    exactly F values of the levels' dtype, one row of the ``ops.reference.dft_tables`` uploaded once (a
    row of a ``[rows, F]`` table is such a tensor), so nothing synchronises. A launch carries up to
    :func:`dft_frequencies_per_launch` frequencies on one read of ``u``; a longer list is split.

    The grids are dense ``[nx][ny][nz]`` tensors or :func:`alloc_level` views with identical shapes,
    dtypes, devices and strides; the boxes lie inside the owned region (``step_medium``'s contract).
    ``u`` is never written, the accumulators only at the box nodes, and none of them may share memory
    with ``u`` or with another of them. Every violation is a ``ValueError`` before any launch."""
    if not isinstance(u, torch.Tensor) or not isinstance(re, (list, tuple)) or not isinstance(im, (list, tuple)):
        raise ValueError("u must be a tensor, re and im lists of tensors")
    re, im = list(re), list(im)
    if len(re) != len(im):
        raise ValueError(f"re and im must have one level per frequency each, not {len(re)} and {len(im)}")
    F = len(re)
    if F == 0:
        raise ValueError("dft_accumulate needs at least one frequency")
    if not all(isinstance(t, torch.Tensor) for t in re + im):
        raise ValueError("re and im must be lists of tensors")
    gv = _check_grid_strided(u, *re, *im)
    for t, name in ((c_row, "c_row"), (s_row, "s_row")):
        if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != u.device or t.dtype != u.dtype
                or t.dim() != 1 or not t.is_contiguous() or t.numel() != F):
            raise ValueError(f"{name} must be a contiguous 1-D {u.dtype} tensor of {F} values on {u.device}")
    spans = [("u", _grid_span(u))] + [(f"{n}[{f}]", _grid_span(t)) for n, ts in (("re", re), ("im", im))
                                      for f, t in enumerate(ts)]
    for q, (name, span) in enumerate(spans):
        _check_spans_apart(name, span, spans[:q])
    bl = _check_boxes(boxes, gv)
    getattr(_C(), "k_dft_acc_" + _sfx(u))(u.data_ptr(), [t.data_ptr() for t in re], [t.data_ptr() for t in im],
                                         c_row.data_ptr(), s_row.data_ptr(), gv, bl, int(chunk), _stream())


def inject(u, m, nodes, g, wrap=None) -> None:
    """Point sources: ``u[node_s] += m[node_s] * g[s]`` (the product rounded, then the add); a node
    on a wrap source plane is also copied to its ghost plane. ``nodes``: (i, j, k) tuples inside
    the owned region, all distinct, or a :func:`source_nodes` list; ``g``: one value per node."""
    gv = _check_grid_strided(u, m)
    nl = _node_list(nodes, u, owned=True, distinct=True)
    if not g.is_cuda or g.device != u.device or g.dtype != u.dtype or not g.is_contiguous() or g.numel() < len(nl):
        raise ValueError(f"g must be a contiguous {u.dtype} device tensor of >= {len(nl)} values")
    w = _check_wrap(wrap, gv)
    if len(nl) == 0:
        return
    getattr(_C(), "k_inject_" + _sfx(u))(u.data_ptr(), m.data_ptr(), gv, nl.dev.data_ptr(), g.data_ptr(),
                                        len(nl), w, _stream())


def record(u, nodes, out) -> None:
    """Receivers: ``out[r] = u[node_r]``. ``nodes``: (i, j, k) tuples anywhere in the storage, or a
    :func:`receiver_nodes` list."""
    gv = _check_grid_strided(u)
    nl = _node_list(nodes, u, owned=False, distinct=False)
    if (not out.is_cuda or out.device != u.device or out.dtype != u.dtype or not out.is_contiguous()
            or out.numel() < len(nl)):
        raise ValueError(f"out must be a contiguous {u.dtype} device tensor of >= {len(nl)} values")
    if len(nl) == 0:
        return
    getattr(_C(), "k_record_" + _sfx(u))(u.data_ptr(), gv, nl.dev.data_ptr(), out.data_ptr(), len(nl), _stream())


# ---- off-grid sources and receivers (csrc/hip_medium_points.hip) ---------------------------

class PointTables:
    """Validated gather tables of :func:`record_weighted`, uploaded once: ``index`` int ``[R, 3, 8]``
    (x, y, z slots, storage indices of the grid ``shape``) and ``weight`` ``[R, 3, 8]`` of ``dtype``
    (``ops.reference.receiver_tables`` builds them). Every index must lie inside the storage."""

    def __init__(self, index, weight, shape, device, dtype):
        nx, ny, nz = (int(v) for v in shape)
        if not isinstance(index, torch.Tensor) or not isinstance(weight, torch.Tensor):
            raise ValueError("index and weight must be tensors")
        if index.dtype not in (torch.int32, torch.int64) or index.dim() != 3 or tuple(index.shape[1:]) != (3, 8):
            raise ValueError(f"index must be an integer [R, 3, 8] tensor, not {index.dtype} {tuple(index.shape)}")
        if weight.dtype != dtype or tuple(weight.shape) != tuple(index.shape):
            raise ValueError(f"weight must be a {dtype} tensor of shape {tuple(index.shape)}, not {weight.dtype} "
                             f"{tuple(weight.shape)}")
        ic = index.detach().cpu().long()
        for axis, n in enumerate((nx, ny, nz)):
            bad = (ic[:, axis] < 0) | (ic[:, axis] >= n)
            if bool(bad.any()):
                r = int(bad.any(1).nonzero()[0])
                raise ValueError(f"receiver {r}: index outside the storage of a {nx}x{ny}x{nz} grid on axis {axis}")
        if not bool(torch.isfinite(weight).all()):
            raise ValueError("weights must be finite")
        self.shape, self.dtype, self.n = (nx, ny, nz), dtype, int(index.shape[0])
        self.index = ic.to(torch.int32).contiguous().to(device)
        self.weight = weight.detach().contiguous().to(device)
        self.device = self.index.device

    def __len__(self):
        return self.n


class RowList:
    """A validated CSR list of touched nodes for :func:`inject_rows` / :func:`rows_dot`, uploaded once
    (``ops.reference.point_rows`` builds it): ``nodes`` ``[rows, 3]`` distinct storage nodes inside the
    owned region of the grid ``shape``, ``rowptr`` ``[rows + 1]`` non-decreasing from 0 to the number
    of entries, per entry a column ``col`` in 0 .. ``ncols`` - 1 and a weight ``w`` of ``dtype``.
    ``unique``: the leading rows :func:`rows_dot` runs on (the rest are plane-N duplicates)."""

    def __init__(self, nodes, rowptr, col, w, *, ncols: int, unique: int | None, shape, device, dtype):
        nx, ny, nz = (int(v) for v in shape)
        for t, name in ((nodes, "nodes"), (rowptr, "rowptr"), (col, "col")):
            if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"{name} must be an integer tensor")
        if nodes.dim() != 2 or nodes.shape[1] != 3:
            raise ValueError(f"nodes must have shape [rows, 3], not {tuple(nodes.shape)}")
        nrows = int(nodes.shape[0])
        if rowptr.dim() != 1 or rowptr.numel() != nrows + 1:
            raise ValueError(f"rowptr must have {nrows + 1} values, not shape {tuple(rowptr.shape)}")
        if not isinstance(w, torch.Tensor) or w.dtype != dtype or w.dim() != 1 or col.dim() != 1 \
                or w.numel() != col.numel():
            raise ValueError(f"col and w must be 1-D with one value per entry, w of {dtype}")
        nnz = int(col.numel())
        nc, pc, cc = nodes.detach().cpu().long(), rowptr.detach().cpu().long(), col.detach().cpu().long()
        for axis, n in enumerate((nx, ny, nz)):
            bad = (nc[:, axis] < 1) | (nc[:, axis] > n - 2)
            if bool(bad.any()):
                nd = tuple(int(v) for v in nc[int(bad.nonzero()[0])])
                raise ValueError(f"row node {nd} outside the owned region of a {nx}x{ny}x{nz} grid")
        key = (nc[:, 0] * ny + nc[:, 1]) * nz + nc[:, 2]
        if torch.unique(key).numel() != nrows:
            raise ValueError("a node is named by more than one row")
        if int(pc[0]) != 0 or int(pc[-1]) != nnz or bool((pc[1:] < pc[:-1]).any()):
            raise ValueError(f"rowptr must not decrease and must run from 0 to the {nnz} entries")
        ncols = int(ncols)
        if nnz and (int(cc.min()) < 0 or int(cc.max()) >= ncols):
            raise ValueError(f"col must lie in 0..{ncols - 1}")
        if not bool(torch.isfinite(w).all()):
            raise ValueError("weights must be finite")
        unique = nrows if unique is None else int(unique)
        if not 0 <= unique <= nrows:
            raise ValueError(f"unique = {unique} outside 0..{nrows}")
        self.shape, self.dtype, self.nrows, self.nnz, self.ncols, self.unique = (nx, ny, nz), dtype, nrows, nnz, ncols, unique
        self.nodes = nc.to(torch.int32).contiguous().to(device)
        self.rowptr = pc.to(torch.int32).contiguous().to(device)
        self.col = cc.to(torch.int32).contiguous().to(device)
        self.w = w.detach().contiguous().to(device)
        self.device = self.nodes.device

    def __len__(self):
        return self.nrows


def point_tables(index, weight, u) -> PointTables:
    """Tables for :func:`record_weighted` in the storage of the grid ``u``."""
    return PointTables(index, weight, u.shape, u.device, u.dtype)


def row_list(rows, u) -> RowList:
    """An ``ops.reference.PointRows`` list for :func:`inject_rows` / :func:`rows_dot` on the grid ``u``."""
    return RowList(rows.nodes, rows.rowptr, rows.col, rows.w, ncols=rows.ncols, unique=rows.unique, shape=u.shape,
                   device=u.device, dtype=u.dtype)


def _check_points(t, u, cls, what: str):
    if not isinstance(t, cls):
        raise ValueError(f"{what} must be a {cls.__name__}")
    if t.shape != tuple(u.shape) or t.dtype != u.dtype or t.device != u.device:
        raise ValueError(f"{what} was built for another grid")
    return t


def _check_values(t, u, n: int, name: str):
    if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != u.device or t.dtype != u.dtype
            or t.dim() != 1 or not t.is_contiguous() or t.numel() < n):
        raise ValueError(f"{name} must be a contiguous 1-D {u.dtype} tensor of >= {n} values on {u.device}")


def _check_apart(t, u, name: str):
    u0, u1 = _grid_span(u)
    t0, t1 = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
    if u0 < t1 and t0 < u1:
        raise ValueError(f"{name} shares memory with u")


def record_weighted(u, tables: PointTables, out) -> None:
    """Off-grid receivers (``k_record_w``): ``out[r]`` = the weighted sum of ``u`` over the 8 x 8 x 8 slots
    of receiver r, one wave per receiver, in the fixed order of ``ops.reference.record_weighted`` (fp64
    and fp32 results are bitwise equal to it). ``tables``: :func:`point_tables`; ``out``: one value per
    receiver, not sharing memory with ``u``. Every violation is a ``ValueError`` before any launch."""
    gv = _check_grid_strided(u)
    tb = _check_points(tables, u, PointTables, "tables")
    _check_values(out, u, len(tb), "out")
    _check_apart(out, u, "out")
    if len(tb) == 0:
        return
    getattr(_C(), "k_record_w_" + _sfx(u))(u.data_ptr(), gv, tb.index.data_ptr(), tb.weight.data_ptr(),
                                          out.data_ptr(), len(tb), _stream())


def inject_rows(u, m, rows: RowList, g, wrap=None) -> None:
    """Off-grid sources (``k_inject_rows``): per row (touched node) ``val = val + w[e] g[col[e]]`` over its
    entries in order, then ``u[node] += m[node] val`` and the ghost-plane copy of a node on a wrap source
    plane, like :func:`inject`. ``rows``: :func:`row_list`; ``g``: one value per column (one time row of
    the compact ``[K, S]`` / ``[K+1, R]`` table). A single entry of weight 1 gives :func:`inject`'s bits."""
    gv = _check_grid_strided(u, m)
    rl = _check_points(rows, u, RowList, "rows")
    _check_values(g, u, rl.ncols, "g")
    _check_apart(g, u, "g")
    w = _check_wrap(wrap, gv)
    if len(rl) == 0:
        return
    getattr(_C(), "k_inject_rows_" + _sfx(u))(u.data_ptr(), m.data_ptr(), gv, rl.nodes.data_ptr(), rl.rowptr.data_ptr(),
                                             rl.col.data_ptr(), rl.w.data_ptr(), g.data_ptr(), len(rl), rl.nnz,
                                             rl.ncols, w, _stream())


def rows_dot(u, rows: RowList, g, sacc) -> None:
    """``sacc[row] += u[node] val`` with the ``val`` of :func:`inject_rows`, for the ``rows.unique`` leading
    rows (``k_rows_dot``); nothing else is written. The per-node time sum behind the source term of
    dJ/dm. ``sacc``: one value per unique row, not sharing memory with ``u``."""
    gv = _check_grid_strided(u)
    rl = _check_points(rows, u, RowList, "rows")
    _check_values(g, u, rl.ncols, "g")
    _check_values(sacc, u, rl.unique, "sacc")
    _check_apart(sacc, u, "sacc")
    if rl.unique == 0:
        return
    getattr(_C(), "k_rows_dot_" + _sfx(u))(u.data_ptr(), gv, rl.nodes.data_ptr(), rl.rowptr.data_ptr(),
                                          rl.col.data_ptr(), rl.w.data_ptr(), g.data_ptr(), rl.unique, rl.nnz,
                                          rl.ncols, sacc.data_ptr(), _stream())
