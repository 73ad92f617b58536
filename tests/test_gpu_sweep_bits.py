"""The sweep kernels' fused error reduction and non-finite flag on chosen values (k_tbn depth 4 and 3,
k_tb3, k_step; fp64 and fp32), bit for bit against the oracle.

The other kernel tests feed uniform random fields, on which the relative-error argmax (RelArg,
csrc/device_common.hpp) never meets a tie, a zero of f or a NaN, and the flag is never set. Here:

* chosen (u, f) pairs. With every coef = 0 and B = A each layer of a sweep equals A on the computed
  nodes (``2A - A`` and ``A + 0 lap`` are exact; the oracle is still evaluated), and with ty = tz = 1 and
  ct = -1/2 the analytic value is ``f[i, j, k] = -tx[i] / 2`` exactly. So a test chooses f per plane and u
  per node: the tie pairs of tests/relarg_ties.py (cross products that round to the same number; RelArg
  must break the tie on the exact FMA residuals), in one column at two planes and in both orders, in
  the first and the last wave and k lane of a tile; a field mirrored in k (exact ties between lanes);
  zeros of f (0/0 is ignored, x/0 is inf); errors that are all NaN (the keys keep their initial
  value); and the pairs scaled down to the magnitude to which the tie-break is exact, and below it.
* non-finite inputs of k_tbn (``check_finite=False``): one +inf, -inf or NaN planted in A or in B at a
  box corner, at k = 64 / 65, at a j tile seam, on the first and the last plane of a work item, on ring
  nodes at every distance, on a masked node beside the box and outside the frame. The oracle divides
  and masks like the kernel (``reference.chained_layers_kernel``, ``chained_layers_fma``), so the very nodes
  that are non-finite must agree, the finite ones bit for bit, the maxima (NaN ignored, an infinity
  wins) and the flag.

Shapes: (9, 9, 11) one clipped tile; (11, 21, 60); (11, 40, 131) 3 x 3 tiles, as one work item per tile
and as one-plane work items.
"""
import math
from fractions import Fraction

import pytest
import torch

import relarg_ties
import sweep_cases as sc
from bits import assert_same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float64, torch.float32]
TIES = {torch.float64: "F64", torch.float32: "F32"}
KINDS = {"tbn4": (4, 4), "tbn3": (3, 3), "tb3": (3, 3), "step": (1, 1)}  # layers, ghost
SHAPES = [((9, 9, 11), 0), ((11, 21, 60), 0), ((11, 40, 131), 0), ((11, 40, 131), 1)]
H2 = tuple(sc.H2.values())
CT = -0.5


def _launch(kind, A, B, tx, ty, tz, box, cdom, coefs, cts, chunk, fma=False, check_finite=True):
    """One launch of ``kind`` on host tensors; returns ([stored layers on the host, by layer index],
    [(abs key, rel key, flag) per layer])."""
    from wave3d.ops import kernels

    n, G = KINDS[kind]
    dtype = A.dtype
    dev = [t.to(DEV) for t in (A, B, tx, ty, tz)]
    o0, o1 = (torch.full(A.shape, v, dtype=dtype, device=DEV) for v in (-7.0, -9.0))
    errs = [kernels.new_err(1) for _ in range(n)]
    co = [(*H2, coefs[q], cts[q]) for q in range(n)]
    ei = (box[0], box[1])
    if kind == "step":
        kernels.step(dev[0], dev[1], o0, box, first=False, err_i=ei, tx=dev[2], ty=dev[3], tz=dev[4],
                     coefs=co[0], err=errs[0], chunk=chunk)
        stored = {0: o0}
    elif kind == "tb3":
        kernels.tb3_sweep(dev[0], dev[1], o0, o1, box, first=False, cdom=cdom, err_i=ei, tx=dev[2], ty=dev[3],
                          tz=dev[4], coefs_c=co[0], coefs_d=co[1], coefs_e=co[2], err_c=errs[0], err_d=errs[1],
                          err_e=errs[2], chunk=chunk, fma=fma)
        stored = {1: o0, 2: o1}
    else:
        kernels.tbn_sweep(dev[0], dev[1], o0, o1, box, depth=n, first=False, cdom=cdom, err_i=ei, tx=dev[2],
                          ty=dev[3], tz=dev[4], coefs=co, errs=errs, chunk=chunk, fma=fma, ghost=G,
                          check_finite=check_finite)
        stored = {n - 2: o0, n - 1: o1}
    torch.cuda.synchronize()
    return {q: t.cpu() for q, t in stored.items()}, [kernels.decode_err(e)[0] for e in errs]


def _oracle(kind, A, B, cdom, coefs):
    """The layers of ``kind`` (exact form) on the full grid, in the grid's type."""
    from wave3d.ops import reference

    n, G = KINDS[kind]
    h = {k: sc.cast(v, A.dtype) for k, v in sc.H2.items()}
    if kind == "step":
        v = torch.zeros_like(A)
        v[1:-1, 1:-1, 1:-1] = reference.stencil_field(A, B, first=False, coef=sc.cast(coefs[0], A.dtype), **h)
        return [v]
    return reference.chained_layers(A, B, n, first=False, mask=sc.mask(A.shape, G, cdom),
                                    coefs=[sc.cast(c, A.dtype) for c in coefs], **h)


class Field:
    """A grid of ``kind`` on ``(X, Y, Z)`` owned nodes with f chosen per plane and u per node (logical
    indices 1 .. X, as the kernels' boxes): coef = 0, B = A, ty = tz = 1, ct = -1/2."""

    def __init__(self, kind, dims, dtype, seed=3, exact=False):
        self.kind, self.dtype = kind, dtype
        self.n, self.G = KINDS[kind]
        X, Y, Z = dims
        self.dims = dims
        G = self.G
        self.shape = (X + 2 * G, Y + 2 * G, Z + 2 * G)
        self.box = (1, X, 1, Y, 1, Z)
        g = torch.Generator().manual_seed(seed)
        n = max(self.shape)
        self.F = (1 + torch.rand(n, generator=g, dtype=torch.float64)).to(dtype)  # |f| per table index
        eps = (torch.rand(self.shape, generator=g, dtype=torch.float64) - 0.5) * 2.0 ** -5
        self.eps = torch.zeros(self.shape, dtype=torch.float64) if exact else eps
        self.ty = torch.ones(n, dtype=dtype)
        self.tz = torch.ones(n, dtype=dtype)
        self.plants = []

    def at(self, i, j, k):
        o = self.G - 1
        return (i + o, j + o, k + o)

    def plant(self, node, d, f):
        """|f| of the node's plane becomes f and the node's error d: u = -(f + d)."""
        self.plants.append((node, d, f))

    def build(self):
        """(A, tx): tx[i] = 2 |f| of the logical plane i (ct = -1/2, so f = -|f|), A = f (1 + eps) with the
        planted nodes u = -(|f| + d); the ghost planes below logical 0 take |f| = 1.5."""
        F = self.F.clone()
        for (i, _, _), _, f in self.plants:
            F[i] = f
        logical = torch.arange(self.shape[0]) - (self.G - 1)
        Fg = torch.where(logical >= 0, F[logical.clamp(min=0)], torch.full((), 1.5, dtype=self.dtype))
        A = -(Fg[:, None, None].double() * (1 + self.eps)).to(self.dtype)
        for (i, j, k), d, f in self.plants:
            A[self.at(i, j, k)] = -(f + d)
        return A, 2 * F

    def run(self, chunk, A=None, tx=None):
        from wave3d.ops import reference

        if A is None:
            A, tx = self.build()
        zero = [0.0] * self.n
        stored, keys = _launch(self.kind, A, A.clone(), tx, self.ty, self.tz, self.box, self.box, zero,
                               [CT] * self.n, chunk)
        L = _oracle(self.kind, A, A, self.box, zero)
        s = sc.sl(self.box, self.G)
        X, Y, Z = self.dims
        f = reference.analytic(tx[1:X + 1], self.ty[1:Y + 1], self.tz[1:Z + 1], CT)
        exp = []
        for q in range(self.n):
            assert_same_bits(L[q][s], A[s])  # the identity the construction rests on, evaluated
            if q in stored:
                assert_same_bits(stored[q][s], L[q][s])
            exp.append(reference.max_errors(L[q][s], f))
        return keys, exp


def _positions(dims):
    """(j, k) columns: the first and the last wave of the first j tile (16 rows), the last row; the
    first k lane, lane 63, lane 0 of the next tile, the last column."""
    X, Y, Z = dims
    js = sorted({1, min(16, Y), Y})
    ks = sorted({1, min(64, Z), min(65, Z), Z})
    return [(j, k) for j in js for k in ks]


def _ties(dtype):
    return [tuple(float.fromhex(v) for v in row) for row in getattr(relarg_ties, TIES[dtype])]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("cfg", range(len(SHAPES)))
@pytest.mark.parametrize("kind", list(KINDS))
def test_relarg_breaks_ties_exactly(C, kind, cfg, dtype):
    """Each tie pair as the field's largest relative error, at two planes of one column, in both
    orders: both keys of every layer equal ``reference.max_errors``. A RelArg that compared the rounded
    products alone would keep the pair it met first: the smaller quotient in one of the two orders
    (tests/test_relarg_ties_cpu.py). The 64 pairs of a type are dealt over the four shapes; the column
    moves through the first and last wave and k lane with the pair's index."""
    dims, chunk = SHAPES[cfg]
    rows = _ties(dtype)
    pos = _positions(dims)
    for q in range(cfg, len(rows), len(SHAPES)):
        d1, f1, d2, f2 = rows[q]
        j, k = pos[(q // len(SHAPES)) % len(pos)]
        for a, b in (((d1, f1), (d2, f2)), ((d2, f2), (d1, f1))):
            fld = Field(kind, dims, dtype)
            fld.plant((3, j, k), *a)
            fld.plant((4, j, k), *b)
            keys, exp = fld.run(chunk)
            want = max(Fraction(d1) / Fraction(f1), Fraction(d2) / Fraction(f2))
            for (ga, gr, bad), (ea, er) in zip(keys, exp):
                assert (ga, gr) == (ea, er) and not bad, (q, j, k, a, b, ga, ea, gr, er)
                # the oracle's key is the planted maximum: the larger exact quotient, rounded once
                assert abs(Fraction(gr) / want - 1) < Fraction(1, 2 ** 20)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("cfg", range(len(SHAPES)))
@pytest.mark.parametrize("kind", list(KINDS))
def test_mirror_symmetric_field(C, kind, cfg, dtype):
    """A field mirrored in k (u, and f through a mirrored tz): every error occurs twice, in two lanes,
    as an exact tie. The keys equal the oracle's."""
    from wave3d.ops import reference

    dims, chunk = SHAPES[cfg]
    n, G = KINDS[kind]
    X, Y, Z = dims
    shape = (X + 2 * G, Y + 2 * G, Z + 2 * G)
    box = (1, X, 1, Y, 1, Z)
    A = sc.rand(shape, dtype, 51) * 2 - 1
    A = torch.where(torch.arange(shape[2]) <= (shape[2] - 1) // 2, A, A.flip(2))
    assert_same_bits(A, A.flip(2))
    tx, ty, tz = sc.tables(max(shape), dtype, 52)
    tz[1:Z + 1] = torch.where(torch.arange(Z) <= (Z - 1) // 2, tz[1:Z + 1], tz[1:Z + 1].flip(0))
    zero, cts = [0.0] * n, list(sc.CT4[:n])
    stored, keys = _launch(kind, A, A.clone(), tx, ty, tz, box, box, zero, cts, chunk)
    L = _oracle(kind, A, A, box, zero)
    s = sc.sl(box, G)
    for q in range(n):
        f = reference.analytic(tx[1:X + 1], ty[1:Y + 1], tz[1:Z + 1], sc.cast(cts[q], dtype))
        assert_same_bits(f, f.flip(2))
        ea, er = reference.max_errors(L[q][s], f)
        assert keys[q] == (ea, er, False), (q, keys[q], ea, er)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("cfg", range(len(SHAPES)))
@pytest.mark.parametrize("kind", list(KINDS))
def test_zeros_of_f(C, kind, cfg, dtype):
    """A plane with f = 0 and u = 0: every quotient there is 0/0 = NaN and is ignored, the rel key comes
    from the other planes. One node of it with u != 0: x/0, the rel key is inf and the abs key
    finite. f = NaN everywhere: every error is NaN and both keys keep their initial value."""
    dims, chunk = SHAPES[cfg]
    X, Y, Z = dims
    fld = Field(kind, dims, dtype)
    A, tx = fld.build()
    i = 5
    A[fld.at(i, 1, 1)[0]] = 0.0
    tx[i] = 0.0
    keys, exp = fld.run(chunk, A, tx)
    for got, (ea, er) in zip(keys, exp):
        assert got == (ea, er, False) and 0 < er < 1 and 0 < ea < 1, (got, ea, er)
    j, k = _positions(dims)[-1]
    A[fld.at(i, j, k)] = 0.25
    keys, exp = fld.run(chunk, A, tx)
    for got, (ea, er) in zip(keys, exp):
        assert got == (ea, er, False) and er == math.inf and ea == 0.25, (got, ea, er)
    tx[:] = math.nan
    keys, exp = fld.run(chunk, A, tx)
    for got, (ea, er) in zip(keys, exp):
        assert got == (ea, er, False) and (ea, er) == (-100.0, -100.0), (got, ea, er)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_small_magnitudes(C, kind, dtype):
    """The tie pairs scaled by 2^SAFE, where every product RelArg forms still has an exact FMA residual
    (exponent >= emin + p - 1; fp64 |d|, |f| ~ 1e-146, fp32 ~ 1e-15): the keys equal the oracle's. And
    scaled by 2^LOW, where the products are subnormal: the tie-break no longer sees the difference, and
    the kernel returns what RelArg's arithmetic returns there (``relarg_ties.relarg``, in rationals): the
    smaller quotient in 62 of the 128 orders of a type (tests/test_relarg_ties_cpu.py has the figures).
    One work item (chunk = X), so that one lane meets both planes."""
    dims = (9, 9, 11)
    name = TIES[dtype]
    p, emin = relarg_ties.FORMATS[name]
    rows = _ties(dtype)
    pos = _positions(dims)
    wrong = 0
    for q in range(0, len(rows), 4):
        d1, f1, d2, f2 = rows[q]
        j, k = pos[(q // 4) % len(pos)]
        for a, b in (((d1, f1), (d2, f2)), ((d2, f2), (d1, f1))):
            for scale, exact in ((relarg_ties.SAFE[name], True), (relarg_ties.LOW[name], False)):
                s = 2.0 ** scale
                fld = Field(kind, dims, dtype, exact=True)
                fld.F[:] = s
                fld.plant((3, j, k), a[0] * s, a[1] * s)
                fld.plant((4, j, k), b[0] * s, b[1] * s)
                keys, exp = fld.run(dims[0])
                for (ga, gr, bad), (ea, er) in zip(keys, exp):
                    assert ga == ea and not bad
                    if exact:
                        assert gr == er, (q, scale, gr, er)
                    else:
                        seq = [(Fraction(0), Fraction(s))] * 2 + [tuple(Fraction(v * s) for v in a),
                                                                  tuple(Fraction(v * s) for v in b)]
                        num, den = relarg_ties.relarg(seq, p, emin)
                        assert Fraction(gr) == relarg_ties.round_fraction(num / den, p, emin), (q, scale, gr, er)
                        wrong += gr != er
    print(f"{kind} {name}: below the bound the key is the smaller quotient in {wrong} launches x layers")


# ---- non-finite inputs of k_tbn -------------------------------------------------------------------

NF_DIMS = (11, 24, 72)             # the smallest grid with all of: k = 64 / 65 and a j tile seam inside the box,
NF_BOX = (2, 10, 3, 21, 58, 70)    # ring and frame nodes on every side, three work items
NF_CDOM = (1, 11, 3, 24, 1, 72)    # j = 2 is a masked node beside the box
NF_CHUNK = 3                       # work items of planes 2-4, 5-7, 8-10


def _nf_plants(depth):
    """(name, logical node) of the planted value."""
    i0, i1, j0, j1, k0, k1 = NF_BOX
    out = [("box corner", (i0, j0, k0)), ("box corner far", (i1, j1, k1)), ("k = 64", (5, 10, 64)),
           ("k = 65", (5, 10, 65)), ("j tile seam, last row", (5, j0 + 15, 66)), ("j tile seam, first row", (5, j0 + 16, 66)),
           ("first plane of a work item", (5, 20, 68)), ("last plane of a work item", (7, 20, 68)),
           ("masked node beside the box", (5, j0 - 1, 68)),
           ("frame corner", (5, j0 - depth, k0 - depth)), ("frame, diagonal", (5, j0 - 2, k0 - (depth - 1))),
           ("outside, k", (5, 10, k0 - depth - 1)), ("outside, j", (5, j1 + depth + 1, 68)),
           ("outside, i", (i1 + depth + 1, 10, 68)), ("outside, corner", (i0 - depth - 1, j0 - depth - 1, k0 - depth - 1))]
    for r in range(1, depth + 1):
        out += [(f"ring k, distance {r}", (5, 10, k0 - r)), (f"ring i, distance {r}", (i0 - r, 10, 68))]
        if r in (1, depth):
            out.append((f"ring j high, distance {r}", (5, j1 + r, 68)))
    return out


def _l1_chebyshev(node):
    gaps = [max(lo - v, 0, v - hi) for v, lo, hi in zip(node, NF_BOX[0::2], NF_BOX[1::2])]
    return sum(gaps), max(gaps)


def _nf_fields():
    """The clean fields per (depth, dtype, fma), built once and left unchanged."""
    cache = {}

    def get(depth, dtype, fma):
        key = (depth, dtype, fma)
        if key not in cache:
            G = depth
            X, Y, Z = NF_DIMS
            shape = (X + 2 * G, Y + 2 * G, Z + 2 * G)
            A, B = sc.rand(shape, dtype, 61), sc.rand(shape, dtype, 62)
            tx, ty, tz = sc.tables(max(shape), dtype, 63)
            c = 2.9e-4
            coefs = [c] * depth if fma else list(sc.C4[:depth])
            cache[key] = dict(A=A, B=B, tx=tx, ty=ty, tz=tz, coefs=coefs, cts=list(sc.CT4[:depth]), G=G, shape=shape)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def nf_base():
    return _nf_fields()


def _nf_oracle(base, A, B, depth, fma):
    from wave3d.ops import reference

    m = sc.mask(base["shape"], base["G"], NF_CDOM)
    if fma:
        return reference.chained_layers_fma(A, B, depth, first=False, mask=m, coefs=base["coefs"], **sc.H2)
    dt = A.dtype
    return reference.chained_layers_kernel(A, B, depth, first=False, mask=m, coefs=[sc.cast(c, dt) for c in base["coefs"]],
                                           **{k: sc.cast(v, dt) for k, v in sc.H2.items()})


def _nf_keys(base, L, depth, fma, dtype):
    from wave3d.ops import reference

    i0, i1, j0, j1, k0, k1 = NF_BOX
    s = sc.sl(NF_BOX, base["G"])
    out = []
    for q in range(depth):
        t = (base["tx"][i0:i1 + 1], base["ty"][j0:j1 + 1], base["tz"][k0:k1 + 1])
        f = reference.analytic(*t, sc.cast(base["cts"][q], dtype))
        ea, er = reference.max_errors(L[q][s], f)
        if fma:
            er = reference.rel_key_fma(L[q][s] - f, *t, base["cts"][q])
        out.append((ea, er))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("fma", [False, True], ids=["exact", "fma"])
@pytest.mark.parametrize("depth", [4, 3])
def test_nonfinite_inputs_of_tbn(C, nf_base, depth, fma, dtype):
    """One non-finite value in A or B, one place at a time. Where the value lies decides what must
    happen; the oracle, not a rule, says which stored nodes and keys change:

    * anywhere: the stored layers are non-finite at the oracle's nodes and nowhere else, finite nodes
      are equal bit for bit, both keys of every layer equal the NaN-ignoring oracle's, and the flag of
      the last layer is set exactly when the oracle's last layer holds a non-finite value inside the
      box. The slots of the earlier layers never carry a flag (chk is summed on the last layer).
    * outside the frame (Chebyshev distance > depth from every box node): nothing changes, flag clear.
    * inside the frame but outside the L1 cone: stored layers and keys are those of the clean fields
      (asserted through the oracle, which is unchanged there); what the flag does is collected and
      pinned below."""
    kind = f"tbn{depth}"
    base = nf_base(depth, dtype, fma)
    G = base["G"]
    s = sc.sl(NF_BOX, G)
    o = G - 1

    def run(A, B):
        return _launch(kind, A, B, base["tx"], base["ty"], base["tz"], NF_BOX, NF_CDOM, base["coefs"], base["cts"],
                       NF_CHUNK, fma=fma, check_finite=False)

    clean_stored, clean_keys = run(base["A"], base["B"])
    Lc = _nf_oracle(base, base["A"], base["B"], depth, fma)
    for q, t in clean_stored.items():
        assert_same_bits(t[s], Lc[q][s])
    exp_clean = _nf_keys(base, Lc, depth, fma, dtype)
    assert [k[:2] for k in clean_keys] == exp_clean and not any(k[2] for k in clean_keys)

    problems, frame_flags, hits = [], {}, 0
    values = (math.inf, -math.inf, math.nan)
    for n_plant, (name, node) in enumerate(_nf_plants(depth)):
        l1, cheb = _l1_chebyshev(node)
        for stream in ("A", "B"):
            value = None if name in ("box corner", "k = 64") else values[(n_plant + (stream == "B")) % 3]
            for v in (values if value is None else (value,)):
                what = f"{stream}{node} = {v} ({name})"
                t = {"A": base["A"], "B": base["B"]}
                t[stream] = t[stream].clone()
                t[stream][node[0] + o, node[1] + o, node[2] + o] = v
                stored, keys = run(t["A"], t["B"])
                L = _nf_oracle(base, t["A"], t["B"], depth, fma)
                for q, got in stored.items():
                    gn, en = ~torch.isfinite(got[s]), ~torch.isfinite(L[q][s])
                    if not torch.equal(gn, en):
                        problems.append(f"{what}: layer {q} non-finite at {int(gn.sum())} nodes, oracle {int(en.sum())}")
                        continue
                    hits += int(en.sum())
                    try:
                        assert_same_bits(got[s][~en], L[q][s][~en], what)
                        full = got.clone()
                        full[s] = -7.0 if q == depth - 2 else -9.0
                        assert bool((full == (-7.0 if q == depth - 2 else -9.0)).all()), "a node outside the box written"
                    except AssertionError as e:
                        problems.append(f"{what}: layer {q}: {str(e)[:300]}")
                exp = _nf_keys(base, L, depth, fma, dtype)
                if [k[:2] for k in keys] != exp:
                    problems.append(f"{what}: keys {[k[:2] for k in keys]} oracle {exp}")
                want_bad = bool((~torch.isfinite(L[depth - 1][s])).any())
                flags = [k[2] for k in keys]
                if any(flags[:-1]):
                    problems.append(f"{what}: an earlier layer's slot carries a flag: {flags}")
                reaches = any(bool((~torch.isfinite(L[q][s])).any()) for q in range(depth))
                if cheb > depth:
                    if flags[-1] or reaches or exp != exp_clean:
                        problems.append(f"{what}: outside the frame, flag {flags[-1]}, oracle touched {reaches}")
                elif not reaches:  # inside the frame, outside the cone
                    if exp != exp_clean:
                        problems.append(f"{what}: outside the cone but the oracle's keys moved")
                    frame_flags[what] = flags[-1]
                elif flags[-1] != want_bad:
                    problems.append(f"{what}: flag {flags[-1]}, oracle's last layer non-finite in the box: {want_bad}")
    print(f"tbn{depth} {'fma' if fma else 'exact'} {dtype}: {hits} non-finite stored values compared; flag between "
          f"cone and frame: {frame_flags}")
    assert not problems, f"{len(problems)} problems:\n" + "\n".join(problems[:40])
    assert hits > 0
    # Between cone and frame (ring nodes the sweep computes or stages but whose values never reach the
    # box): the flag stays clear, like the outputs. chk is summed over the box nodes of the last layer
    # alone (csrc/hip_tbn.hip), so a non-finite value that reaches no box node is not reported.
    assert frame_flags and not any(frame_flags.values()), frame_flags
