"""The medium kernels bit for bit, in fp64 and fp32, on the values real fields are made of: zero regions
with signed zeros, subnormals, products that underflow, a front that decays through the whole
subnormal range, and non-finite values. k_march_m / k_march_mh / k_march_mb, k_face_corr
(csrc/hip_medium.hip, hip_medium_corr.hip) and the point kernels (k_inject, k_record, k_record_w,
k_inject_rows, k_rows_dot) against the PyTorch oracle (ops/reference.py).

Three input families, each from a seeded generator below:

* quiescent: u1, u2 exactly zero (some zeros negative) but for a compact blob of order-one values that
  straddles a 64-lane k tile, a row seam and a chunk boundary; every side stream mixes normal values
  with subnormals, signed zeros and magnitudes whose products underflow. Every numerator of the
  Laplacian is zero or inside the range of the kernels' constant division (bits.division_range), so
  everything is bit-equal to the oracle, the signs of the zeros included.
* front: u1 = +-2^(-g distance) from a box corner, through the range bound and the subnormals down to
  zero. In-range nodes are bit-equal; at the others the constant division may be off by D = 1 ulp per
  quotient (tests/test_div_const_cpu.py) and the Laplacian lies within ``_lap_bound``.
* non-finite: +-inf and NaN, one at a time, at a box corner, k = 64 / 65, a row seam, next to a mirror
  face and on an x ghost plane. The constant division turns an infinite numerator into NaN where
  true division keeps the infinity, so the *masks* of non-finite nodes must agree, and all finite
  nodes bit for bit.
"""
import math
from collections import namedtuple

import pytest
import torch

from bits import _FORMAT, assert_same_bits, numerators, spacing
from test_div_const_cpu import D
from test_gpu_medium import H2, _cast, _rand

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -7.0
DTYPES = (torch.float64, torch.float32)
FAMILIES = ("quiescent", "front", "nonfinite")
# decay of the front in bits per node of (L1) distance: (g, d0, g_far), g up to the distance d0 and g_far
# beyond it. Chosen on the CPU so that at least half of the box nodes keep every numerator zero or in
# range and at least a tenth do not (asserted in the test). In fp64 the out-of-range band, 2^-968 down to
# 2^-1074, is a tenth of the way to zero: one slope cannot put a tenth of the nodes there, so the front
# falls steeply to the range bound and more gently through the band.
FRONT_G = {torch.float32: (2.25, 0.0, 2.25), torch.float64: (22.0, 44.0, 5.0)}

Cfg = namedtuple("Cfg", "name shape box chunk order mirror density wrap")


def _wrap_pairs(i0, i1, M):
    """the solver's periodic pairs for a box that spans the owned planes: i1 - g -> i0 - g, i0 + g -> i1 + g"""
    w = []
    for g in range(1, M + 1):
        w += [i1 - g, i0 - g, i0 + g, i1 + g]
    return tuple(w)


# the shapes, boxes, chunks and mirrors of test_gpu_medium.py (order 2, density) and test_gpu_medium_order.py
CONFIGS = [Cfg(f"{k}-whole", (13, 21, 70), (1, 11, 1, 19, 1, 68), 0, 2, None, k == "mb", _wrap_pairs(1, 11, 1))
           for k in ("m", "mb")]
CONFIGS += [Cfg(f"{k}-tiles", (9, 40, 131), (1, 7, 5, 33, 60, 129), 2, 2, None, k == "mb", None) for k in ("m", "mb")]
for _o in (4, 8):
    CONFIGS.append(Cfg(f"mh{_o}-faces", (20, 21, 70), (4, 15, 1, 19, 1, 68), 0, _o, (0, 20, 0, 69), False,
                       _wrap_pairs(4, 15, _o // 2)))
    CONFIGS.append(Cfg(f"mh{_o}-storage", (20, 40, 140), (5, 13, 6, 30, 60, 133), 3, _o, None, False, None))


def _modes(cfg):
    """(mode, first): every legal combination of the kernel's modes with the Taylor start / leapfrog"""
    modes = [("plain", True)] + [(m, False) for m in ("plain", "save", "image", "born", "illum", "save_illum")]
    if cfg.density:
        modes += [("scatter", False), ("add", False)]
    return modes


STEPS = [(c, m, f) for c in CONFIGS for m, f in _modes(c)]
STEP_IDS = [f"{c.name}-{m}{'-first' if f else ''}" for c, m, f in STEPS]
# the side streams a mode reads (non-finite family), beside u1, u2, m and the buoyancy
SIDE = {"plain": (), "save": (), "image": ("q", "acc"), "born": ("q", "dm"), "illum": ("h",), "save_illum": ("h",),
        "scatter": ("dm", "db"), "add": ("s",)}


def _at(t, box):
    i0, i1, j0, j1, k0, k1 = box
    return t[i0:i1 + 1, j0:j1 + 1, k0:k1 + 1]


# ---- the generators ----------------------------------------------------------------------------------

def _specials(dtype):
    """signed zeros, subnormals, the smallest normal, and magnitudes whose products are subnormal or 0"""
    p, emin, _ = _FORMAT[dtype]
    tiny = math.ldexp(1.0, emin - p + 1)
    half = emin // 2
    return torch.tensor([0.0, -0.0, tiny, -tiny, 3 * tiny, math.ldexp(1.25, emin - 3), -math.ldexp(1.0, emin - 1),
                         math.ldexp(1.0, emin), math.ldexp(1.0, half), -math.ldexp(1.5, half - 9),
                         math.ldexp(1.0, half + 2), -math.ldexp(1.75, emin + 5)], dtype=torch.float64).to(dtype)


def _mix(shape, dtype, seed, lo, hi, frac=0.4, positive=False, keep=None):
    """uniform values of [lo, hi] with a fraction ``frac`` of special values (``keep``: a mask of nodes that
    stay ordinary; ``positive``: magnitudes only and no zero, for the sponge's factors in (0, 1])"""
    g = torch.Generator().manual_seed(seed)
    v = (lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64)).to(dtype)
    sp = _specials(dtype)
    pick = sp[torch.randint(len(sp), shape, generator=g)]
    if positive:
        pick = pick.abs()
        pick = torch.where(pick == 0, sp[2].expand(shape), pick)
    use = torch.rand(shape, generator=g, dtype=torch.float64) < frac
    if keep is not None:
        use &= ~keep
    return torch.where(use, pick, v)


def _blob(cfg):
    """index ranges of the quiescent blob: across the chunk boundary after the box's 2nd (3rd) plane, the
    row seam j0 + 15 | j0 + 16 and the k tile seam 64 | 65"""
    i0, _, j0, _, _, _ = cfg.box
    return (i0 + 1, i0 + 4), (j0 + 13, j0 + 18), (62, 67)


def _quiescent_field(cfg, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.zeros(cfg.shape, dtype=dtype)
    u = torch.where(torch.rand(cfg.shape, generator=g, dtype=torch.float64) < 0.3, torch.tensor(-0.0, dtype=dtype), u)
    (a0, a1), (b0, b1), (c0, c1) = _blob(cfg)
    n = (a1 - a0 + 1, b1 - b0 + 1, c1 - c0 + 1)
    mag = 0.25 + 0.75 * torch.rand(n, generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand(n, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
    u[a0:a1 + 1, b0:b1 + 1, c0:c1 + 1] = (mag * sign).to(dtype)
    return u


def _front_field(cfg, dtype, seed, scale=1.0):
    """+-(1 + f) 2^(-g d), d = L1 distance from the box corner (i0, j0, k0) and g = FRONT_G, formed in fp64
    and rounded to ``dtype``: normal, then subnormal, then exactly zero"""
    g = torch.Generator().manual_seed(seed)
    i0, _, j0, _, k0, _ = cfg.box
    ax = [torch.arange(n, dtype=torch.float64) for n in cfg.shape]
    d = (ax[0] - i0).abs()[:, None, None] + (ax[1] - j0).abs()[None, :, None] + (ax[2] - k0).abs()[None, None, :]
    rate, d0, rate_far = FRONT_G[dtype]
    e = torch.floor(-(rate * torch.clamp(d, max=d0) + rate_far * torch.clamp(d - d0, min=0.0)))
    mant = scale * (1.0 + 0.999 * torch.rand(cfg.shape, generator=g, dtype=torch.float64))
    sign = torch.where(torch.rand(cfg.shape, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
    return torch.ldexp(mant * sign, e.to(torch.int32)).to(dtype)


def _streams(cfg, dtype, family, sponge):
    """CPU tensors of every stream any mode reads: u1 u2 m q acc dm h s b db and the sponge tables"""
    shape = cfg.shape
    st = {}
    if family == "quiescent":
        st["u1"], st["u2"] = _quiescent_field(cfg, dtype, 31), _quiescent_field(cfg, dtype, 32)
        st["m"] = _mix(shape, dtype, 33, 1e-4, 6e-4)
        for n, (name, lo, hi) in enumerate((("q", -1, 1), ("acc", -1, 1), ("dm", -1, 1), ("h", -1, 1), ("s", -1, 1))):
            st[name] = _mix(shape, dtype, 34 + n, lo, hi)
        # b and db multiply differences of u1: special values only where those are all zero (two nodes
        # from the blob), or the numerators would leave the range
        near = torch.zeros(shape, dtype=torch.bool)
        (a0, a1), (b0, b1), (c0, c1) = _blob(cfg)
        near[a0 - 2:a1 + 3, b0 - 2:b1 + 3, c0 - 2:c1 + 3] = True
        st["b"] = _mix(shape, dtype, 40, 0.3, 2.0, keep=near)
        st["db"] = _mix(shape, dtype, 41, -1.0, 1.0, keep=near)
        st["taper"] = tuple(_mix((n,), dtype, 42 + a, 0.5, 1.0, positive=True) for a, n in enumerate(shape)) \
            if sponge else None
        return st
    if family == "front":
        st["u1"], st["u2"] = _front_field(cfg, dtype, 51), _front_field(cfg, dtype, 52, 0.5)
    else:
        st["u1"], st["u2"] = _rand(shape, dtype, 61), _rand(shape, dtype, 62)
    st["m"] = _rand(shape, dtype, 63, 1e-4, 6e-4)
    for n, name in enumerate(("q", "acc", "dm", "h", "s", "db")):
        st[name] = _rand(shape, dtype, 64 + n, -1.0, 1.0)
    st["b"] = _rand(shape, dtype, 70, 0.3, 2.0)
    st["taper"] = tuple(_rand((n,), dtype, 71 + a, 0.5, 1.0) for a, n in enumerate(shape)) if sponge else None
    return st


# ---- the kernel and the oracle ----------------------------------------------------------------------------

def _launch(cfg, st, mode, first):
    """One step on the device; returns the full grids the step writes (CPU) and the decoded statistic."""
    from wave3d.ops import kernels

    dt = st["u1"].dtype
    reads = ["u1", "u2", "m"] + list(SIDE[mode]) + (["b"] if cfg.density else [])
    d = {k: st[k].to(DEV) for k in reads}
    out = {"u": torch.full(cfg.shape, SENT, dtype=dt, device=DEV)}
    kw = {}
    if mode in ("save", "save_illum"):
        out["lap_out"] = kw["lap_out"] = torch.full(cfg.shape, SENT, dtype=dt, device=DEV)
    if mode in ("illum", "save_illum"):
        out["h"] = kw["illum"] = d.pop("h")
    if mode == "image":
        out["acc"] = d.pop("acc")
        kw["image"] = (d["q"], out["acc"])
    if mode == "born":
        kw["born"] = (d["q"], d["dm"])
    if mode == "scatter":
        out["s_out"] = torch.full(cfg.shape, SENT, dtype=dt, device=DEV)
        kw["scatter"] = (out["s_out"], d["dm"], d["db"])
    if mode == "add":
        kw["born_add"] = d["s"]
    stat = kernels.new_err(1)
    kernels.step_medium(d["u1"], d["u2"], d["m"], out["u"], cfg.box, first=first, h2=H2, stat=stat,
                        stat_i=(cfg.box[0] + 1, cfg.box[1]), wrap=cfg.wrap, chunk=cfg.chunk,
                        taper=None if st["taper"] is None else tuple(t.to(DEV) for t in st["taper"]),
                        order=cfg.order, mirror=cfg.mirror, buoyancy=d["b"] if cfg.density else None, **kw)
    torch.cuda.synchronize()
    (ga, gr, bad), = kernels.decode_err(stat)
    assert gr == -100.0  # slot 1 is never touched
    for k, v in d.items():  # the inputs are read only
        assert_same_bits(v.cpu(), st[k], k)
    return {k: v.cpu() for k, v in out.items()}, ga, bad


def _oracle(cfg, st, mode, first, lap=None):
    """The expected full grids, and the oracle's Laplacian on the box. ``lap``: a Laplacian to use in the
    update of u instead of the oracle's own (the front family's bound)."""
    from wave3d.ops import reference

    dt = st["u1"].dtype
    h = [_cast(v, dt) for v in H2]  # the kernel casts h2 to the working type
    box = cfg.box
    b = st["b"] if cfg.density else None
    L = reference._lap_box(st["u1"], box, *h, cfg.order, cfg.mirror, b)
    kw = {}
    if mode == "born":
        kw["born"] = (_at(st["q"], box).clone(), st["dm"])
    if mode == "add":
        kw["born_add"] = _at(st["s"], box).clone()
    own = reference._lap_box
    if lap is not None:
        reference._lap_box = lambda *a, **k: lap
    try:
        ubox = reference.step_medium(st["u1"], st["u2"], st["m"], box, first=first, hx2=h[0], hy2=h[1], hz2=h[2],
                                     taper=st["taper"], order=cfg.order, mirror=cfg.mirror, buoyancy=b, **kw)
    finally:
        reference._lap_box = own
    exp = {"u": torch.full(cfg.shape, SENT, dtype=dt)}
    _at(exp["u"], box).copy_(ubox)
    w = cfg.wrap or ()
    for src, dst in zip(w[0::2], w[1::2]):  # the fused periodic wrap: the box nodes of plane src, copied
        _at(exp["u"], (dst, dst) + tuple(box[2:])).copy_(_at(exp["u"], (src, src) + tuple(box[2:])))
    if mode in ("save", "save_illum"):
        exp["lap_out"] = torch.full(cfg.shape, SENT, dtype=dt)
        _at(exp["lap_out"], box).copy_(L)
    if mode in ("illum", "save_illum"):
        exp["h"] = st["h"].clone()
        _at(exp["h"], box).copy_(_at(st["h"], box) + L * L)
    if mode == "image":
        exp["acc"] = st["acc"].clone()
        _at(exp["acc"], box).copy_(_at(st["acc"], box) + _at(st["u1"], box) * _at(st["q"], box))
    if mode == "scatter":
        R = reference._lap_box(st["u1"], box, *h, 2, None, st["db"])
        exp["s_out"] = torch.full(cfg.shape, SENT, dtype=dt)
        _at(exp["s_out"], box).copy_(_at(st["dm"], box) * L + _at(st["m"], box) * R)
    return exp, ubox, L


def _numerators(cfg, st, field="b"):
    return numerators(st["u1"], cfg.box, H2_CAST[st["u1"].dtype], cfg.order, cfg.mirror,
                      st[field] if cfg.density else None)


H2_CAST = {dt: [_cast(v, dt) for v in H2] for dt in DTYPES}


def _lap_bound(ts, dtype):
    """Largest |lap_kernel - lap_oracle| at a node whose numerators t_x, t_y, t_z are outside the division's
    range (fp64 tensor). The oracle forms lap = ((0 + q_x) + q_y) + q_z with q = t / h2. Each of the
    kernel's quotients is at most D units in the last place of its own magnitude from q (the sweep of
    tests/test_div_const_cpu.py): |dq| <= D spacing(q). 0 + q_x is exact. Each of the two remaining adds
    rounds once on either side, by half a spacing of its result; the kernel's result may lie in the binade
    above the oracle's, where the spacing is twice as large, so the two roundings together are below
    2 spacing(oracle's partial sum). Hence
    |d lap| <= D (spacing(q_x) + spacing(q_y) + spacing(q_z)) + 2 spacing(s_2) + 2 spacing(lap)."""
    h = H2_CAST[dtype]
    q = [t / hv for t, hv in zip(ts, h)]
    s2 = (torch.zeros_like(q[0]) + q[0]) + q[1]
    s3 = s2 + q[2]
    return (D * sum(spacing(v).double() for v in q) + 2 * spacing(s2).double() + 2 * spacing(s3).double())


def _check_stat(ga, bad, ubox, flagged=False):
    from wave3d.ops import reference

    assert ga == reference.max_abs_field(ubox[1:].double())  # the planes after the box's first
    assert bad == flagged


# ---- the march kernels ----------------------------------------------------------------------------------

@pytest.mark.parametrize("sponge", [False, True], ids=["", "sponge"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("cfg,mode,first", STEPS, ids=STEP_IDS)
def test_quiescent_step_is_the_oracle_bit_for_bit(C, cfg, mode, first, dtype, sponge):
    st = _streams(cfg, dtype, "quiescent", sponge)
    ts, ok = _numerators(cfg, st)
    assert bool(ok.all()) and int(sum((t != 0).sum() for t in ts)) > 100
    if mode == "scatter":
        assert bool(_numerators(cfg, st, "db")[1].all())
    got, ga, bad = _launch(cfg, st, mode, first)
    exp, ubox, _ = _oracle(cfg, st, mode, first)
    assert sorted(got) == sorted(exp)
    for name in exp:  # the box, the wrap planes, and everything else untouched; the signs of the zeros too
        assert_same_bits(got[name], exp[name], name)
    # the data is what the family promises: zeros of both signs, subnormals, underflowing products
    u = _at(exp["u"], cfg.box)
    assert int((u != 0).sum()) > 100
    if mode not in ("born", "add"):  # their scattering term fills the box
        assert int((u == 0).sum()) > u.numel() // 2
    _check_stat(ga, bad, ubox)


@pytest.mark.parametrize("sponge", [False, True], ids=["", "sponge"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("cfg,mode,first", STEPS, ids=STEP_IDS)
def test_front_step_inside_and_outside_the_division_range(C, cfg, mode, first, dtype, sponge):
    st = _streams(cfg, dtype, "front", sponge)
    ts, ok = _numerators(cfg, st)
    frac_in, out = float(ok.double().mean()), ~ok
    assert frac_in >= 0.5 and 1.0 - frac_in >= 0.1, frac_in
    got, ga, bad = _launch(cfg, st, mode, first)
    exp, ubox, L = _oracle(cfg, st, mode, first)
    box = cfg.box
    # outside the box: untouched; the wrap planes: copies of the kernel's own source planes
    mask = torch.ones(cfg.shape, dtype=torch.bool)
    _at(mask, box)[...] = False
    w = cfg.wrap or ()
    for src, dst in zip(w[0::2], w[1::2]):
        assert_same_bits(_at(got["u"], (dst, dst) + tuple(box[2:])), _at(got["u"], (src, src) + tuple(box[2:])), "wrap")
        _at(mask, (dst, dst) + tuple(box[2:]))[...] = False
    for name in exp:
        assert_same_bits(got[name][mask], exp[name][mask], name + " outside the box")
        # in range: bit for bit, every output
        assert_same_bits(_at(got[name], box)[ok], _at(exp[name], box)[ok], name + " in range")
    if "acc" in exp:  # no division behind it
        assert_same_bits(got["acc"], exp["acc"], "acc")
    # out of range: the Laplacian within _lap_bound, u between the oracle's updates of lap -+ the bound (the
    # update is a chain of rounded monotone operations of lap, so this is "the bound times |m|", rounded
    # as the update rounds it)
    tol = _lap_bound(ts, dtype)
    assert bool(torch.isfinite(tol).all())
    if "lap_out" in exp:
        dl = (_at(got["lap_out"], box).double() - L.double()).abs()
        print(f"lap_out: {int((dl[out] != 0).sum())} of {int(out.sum())} out-of-range nodes differ")
        assert bool((dl[out] <= tol[out]).all())
    ends = [_oracle(cfg, st, mode, first, lap=(L.double() + s * tol).to(dtype))[1] for s in (-1.0, 1.0)]
    lo, hi = torch.minimum(*ends), torch.maximum(*ends)
    gu = _at(got["u"], box)
    print(f"u: {int((gu[out] != ubox[out]).sum())} of {int(out.sum())} out-of-range nodes differ; "
          f"{100 * frac_in:.0f} % of the box in range")
    assert bool(((gu >= lo) & (gu <= hi))[out].all())
    # the statistic is that of the stored field; where the oracle's maximum sits at in-range nodes (near the
    # corner, unless a scattering term fills the box) it is the oracle's too
    _check_stat(ga, bad, gu)
    a = ubox[1:].abs()
    if bool(ok[1:][a == a.max()].all()):
        _check_stat(ga, bad, ubox)


def _places(cfg):
    i0, i1, j0, j1, k0, k1 = cfg.box
    im = (i0 + i1) // 2
    p = {"corner": (i0, j0, k0), "k64": (im, j0 + 2, 64), "k65": (im + 1, j0 + 3, 65),
         "row seam": (im, j0 + 16, (k0 + k1) // 2), "row seam-1": (i1, j0 + 15, k1), "x ghost": (i0 - 1, j0 + 5, k0 + 7)}
    if cfg.mirror is not None:
        p["mirror"] = (im + 1, j1, k1 - 9)  # next to the face j_hi = j1 + 1
    return p


@pytest.mark.parametrize("sponge", [False, True], ids=["", "sponge"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("cfg,mode,first", STEPS, ids=STEP_IDS)
def test_nonfinite_values_reach_the_same_nodes_as_in_the_oracle(C, cfg, mode, first, dtype, sponge):
    from wave3d.ops import reference

    base = _streams(cfg, dtype, "nonfinite", sponge)
    streams = ["u1", "m"] + ([] if first else ["u2"]) + list(SIDE[mode]) + (["b"] if cfg.density else [])
    ei0 = cfg.box[0] + 1
    runs = 0
    for stream in streams:
        stencil = stream in ("u1", "b", "db")  # read at the neighbours too: the ghost plane matters
        for place, node in _places(cfg).items():
            if place == "x ghost" and not stencil:
                continue
            for value in (math.inf, -math.inf, math.nan):
                st = dict(base)
                st[stream] = base[stream].clone()
                st[stream][node] = value
                got, ga, bad = _launch(cfg, st, mode, first)
                exp, ubox, _ = _oracle(cfg, st, mode, first)
                what = f"{stream}{node} = {value} ({place})"
                hit = 0
                for name in exp:
                    gn, en = ~torch.isfinite(got[name]), ~torch.isfinite(exp[name])
                    assert torch.equal(gn, en), f"{what}: {name} is non-finite at other nodes than the oracle's"
                    assert_same_bits(got[name][~en], exp[name][~en], f"{what}: {name}")
                    hit += int(en.sum())
                assert hit > 0, what
                assert bad == bool((~torch.isfinite(ubox)).any()), what
                # the statistic is that of the field the kernel stored (NaN ignored, an infinity wins)
                assert ga == reference.max_abs_field(_at(got["u"], cfg.box)[ei0 - cfg.box[0]:].double()), what
                runs += 1
    assert runs >= 3 * len(streams) * 5


# ---- face correlation ------------------------------------------------------------------------------------

CORR = [((13, 21, 70), (1, 11, 1, 19, 1, 68), 0), ((9, 40, 131), (1, 7, 5, 33, 60, 129), 2)]
CORR_CFG = [Cfg(f"corr-{i}", s, b, c, 2, None, False, None) for i, (s, b, c) in enumerate(CORR)]


def _corr(cfg, a, v, acc0):
    from wave3d.ops import kernels, reference

    dt = a.dtype
    acc = acc0.to(DEV)
    ad, vd = a.to(DEV), v.to(DEV)
    kernels.face_correlation(ad, vd, acc, cfg.box, h2=H2, chunk=cfg.chunk)
    torch.cuda.synchronize()
    assert_same_bits(ad.cpu(), a, "a")
    assert_same_bits(vd.cpu(), v, "v")
    Cav = reference.face_correlation(a, v, cfg.box, *H2_CAST[dt])
    exp = acc0.clone()
    _at(exp, cfg.box).copy_(_at(acc0, cfg.box) + Cav)
    return acc.cpu(), exp, Cav


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("cfg", CORR_CFG, ids=[c.name for c in CORR_CFG])
def test_face_correlation_quiescent(C, cfg, dtype):
    a, v = _quiescent_field(cfg, dtype, 81), _quiescent_field(cfg, dtype, 82)
    acc0 = _mix(cfg.shape, dtype, 83, -1.0, 1.0)
    ts, ok = numerators(a, cfg.box, H2_CAST[dtype], correlate=v)
    assert bool(ok.all()) and int(sum((t != 0).sum() for t in ts)) > 100
    got, exp, _ = _corr(cfg, a, v, acc0)
    assert_same_bits(got, exp)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("cfg", CORR_CFG, ids=[c.name for c in CORR_CFG])
def test_face_correlation_front(C, cfg, dtype):
    # the numerators are products of two differences: an order-one field against the front
    a, v = _front_field(cfg, dtype, 84), _rand(cfg.shape, dtype, 85, -1.0, 1.0)
    acc0 = _front_field(cfg, dtype, 86, 0.25)
    ts, ok = numerators(a, cfg.box, H2_CAST[dtype], correlate=v)
    frac_in, out = float(ok.double().mean()), ~ok
    assert frac_in >= 0.5 and 1.0 - frac_in >= 0.1, frac_in
    got, exp, Cav = _corr(cfg, a, v, acc0)
    mask = torch.ones(cfg.shape, dtype=torch.bool)
    _at(mask, cfg.box)[...] = False
    assert_same_bits(got[mask], exp[mask], "outside the box")
    g, e, a0 = _at(got, cfg.box), _at(exp, cfg.box), _at(acc0, cfg.box)
    assert_same_bits(g[ok], e[ok], "in range")
    # out of range: C within _lap_bound (the same three quotients and two adds), acc between acc0 + (C -+ bound)
    tol = _lap_bound(ts, dtype)
    ends = [a0 + (Cav.double() + s * tol).to(dtype) for s in (-1.0, 1.0)]
    lo, hi = torch.minimum(*ends), torch.maximum(*ends)
    print(f"acc: {int((g[out] != e[out]).sum())} of {int(out.sum())} out-of-range nodes differ; "
          f"{100 * frac_in:.0f} % of the box in range")
    assert bool(((g >= lo) & (g <= hi))[out].all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("cfg", CORR_CFG, ids=[c.name for c in CORR_CFG])
def test_face_correlation_nonfinite(C, cfg, dtype):
    base = {"a": _rand(cfg.shape, dtype, 87, -1.0, 1.0), "v": _rand(cfg.shape, dtype, 88, -1.0, 1.0),
            "acc": _rand(cfg.shape, dtype, 89, -1.0, 1.0)}
    for stream in base:
        for place, node in _places(cfg).items():
            if place == "x ghost" and stream == "acc":
                continue
            for value in (math.inf, -math.inf, math.nan):
                t = dict(base)
                t[stream] = base[stream].clone()
                t[stream][node] = value
                got, exp, _ = _corr(cfg, t["a"], t["v"], t["acc"])
                gn, en = ~torch.isfinite(got), ~torch.isfinite(exp)
                what = f"{stream}{node} = {value} ({place})"
                assert int(en.sum()) > 0 and torch.equal(gn, en), what
                assert_same_bits(got[~en], exp[~en], what)


# ---- the point kernels: no division, so everything finite is bit-equal ---------------------------------------

SHAPE = (13, 12, 11)
NN = (10, 11, 10)
WRAP = (10, 0, 2, 12)
PT = Cfg("points", SHAPE, (1, 11, 1, 10, 1, 9), 0, 2, None, False, WRAP)


def _point_field(dtype, family, seed):
    if family == "quiescent":  # zeros of both signs and special values; a few order-one nodes
        u = _mix(SHAPE, dtype, seed, -1.0, 1.0, frac=0.7)
        return torch.where(_rand(SHAPE, dtype, seed + 100, 0.0, 1.0) < 0.5, torch.zeros((), dtype=dtype), u)
    if family == "front":
        i = torch.arange(SHAPE[0], dtype=torch.float64)[:, None, None]
        j = torch.arange(SHAPE[1], dtype=torch.float64)[None, :, None]
        k = torch.arange(SHAPE[2], dtype=torch.float64)[None, None, :]
        _, emin, _ = _FORMAT[dtype]
        e = torch.floor((i + j + k) * (emin - 40) / 24.0)  # through the subnormals to zero within the grid
        return torch.ldexp(_rand(SHAPE, torch.float64, seed, -2.0, 2.0), e.to(torch.int32)).to(dtype)
    return _rand(SHAPE, dtype, seed, -1.0, 1.0)


def _same_or_both_nonfinite(got, exp, what):
    gn, en = ~torch.isfinite(got), ~torch.isfinite(exp)
    assert torch.equal(gn, en), what
    assert_same_bits(got[~en], exp[~en], what)
    # without a division the kind of non-finite value is the oracle's too
    assert_same_bits(got, exp, what)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_inject_and_record(C, dtype, family):
    from wave3d.ops import kernels

    u0, m = _point_field(dtype, family, 91), _point_field(dtype, family, 92)
    nodes = [(3, 4, 5), (10, 2, 9), (1, 6, 1), (2, 10, 3), (7, 7, 7), (6, 1, 8)]  # two on wrap source planes
    g = torch.tensor([0.75, -1.25, 3.5, -0.0, 2.0 ** -70, -(2.0 ** -20)], dtype=dtype)
    variants = [(None, None)]
    if family == "nonfinite":
        variants = [(s, v) for s in ("u", "m", "g") for v in (math.inf, -math.inf, math.nan)]
    for stream, value in variants:
        u, mm, gg = u0.clone(), m.clone(), g.clone()
        if stream == "g":
            gg[1] = value
        elif stream is not None:
            (u if stream == "u" else mm)[nodes[1]] = value
        ud = u.to(DEV)
        kernels.inject(ud, mm.to(DEV), nodes, gg.to(DEV), wrap=WRAP)
        rec = nodes + [(0, 2, 9), (12, 10, 3), (4, 4, 4)]
        out = torch.zeros(len(rec), dtype=dtype, device=DEV)
        kernels.record(ud, rec, out)
        torch.cuda.synchronize()
        exp = u.clone()
        for nd, gv in zip(nodes, gg):
            exp[nd] = u[nd] + mm[nd] * gv
        exp[0, 2, 9], exp[12, 10, 3] = exp[10, 2, 9], exp[2, 10, 3]
        what = f"{stream} = {value}"
        _same_or_both_nonfinite(ud.cpu(), exp, what)
        _same_or_both_nonfinite(out.cpu(), torch.stack([exp[nd] for nd in rec]), what)
        if stream is not None:
            assert not bool(torch.isfinite(exp[nodes[1]]))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_record_weighted(C, dtype, family):
    from test_gpu_medium_points import POINTS
    from wave3d.ops import kernels, reference

    u0 = _point_field(dtype, family, 93)
    index, weight = reference.receiver_tables(POINTS, NN, dtype)
    # receiver 0 sits on the node (5, 5, 6): every other slot of it has the weight 0
    assert int((weight[0] == 0).sum()) == 21
    variants = [None]
    if family == "nonfinite":  # under a non-zero weight, and under a zero weight of receiver 0 alone
        variants = [(nd, v) for nd in ((5, 5, 6), (5, 5, 7), (2, 2, 2)) for v in (math.inf, -math.inf, math.nan)]
    for var in variants:
        u = u0.clone()
        if var is not None:
            u[var[0]] = var[1]
        ud = u.to(DEV)
        out = torch.full((len(POINTS),), SENT, dtype=dtype, device=DEV)
        kernels.record_weighted(ud, kernels.point_tables(index, weight, ud), out)
        exp = reference.record_weighted(u, index, weight)
        _same_or_both_nonfinite(out.cpu(), exp, str(var))
        if var is not None and var[0] != (2, 2, 2):
            assert not bool(torch.isfinite(exp[0]))  # 0 * NaN and 0 * inf are NaN, in the kernel as in the oracle


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
def test_inject_rows_and_rows_dot(C, dtype, family):
    from test_gpu_medium_points import POINTS
    from wave3d.ops import kernels, reference

    u0, m0 = _point_field(dtype, family, 94), _point_field(dtype, family, 95)
    g0 = torch.tensor([0.75, -1.25, 2.0 ** -70, -0.0, 3.5, -(2.0 ** -30)], dtype=dtype)
    rows = reference.point_rows(POINTS, NN, dtype)
    sacc0 = _mix((rows.unique,), dtype, 96, -1.0, 1.0)
    i, j, k = rows.ijk()
    node = (int(i[7]), int(j[7]), int(k[7]))  # a touched node
    variants = [(None, None)]
    if family == "nonfinite":
        variants = [(s, v) for s in ("u", "m", "g", "sacc") for v in (math.inf, -math.inf, math.nan)]
    for stream, value in variants:
        u, m, g, sacc_c = u0.clone(), m0.clone(), g0.clone(), sacc0.clone()
        if stream in ("u", "m"):
            (u if stream == "u" else m)[node] = value
        elif stream == "g":
            g[4] = value
        elif stream == "sacc":
            sacc_c[7] = value
        exp = u.clone()
        reference.inject_rows(exp, m, rows, g)
        for src, dst in ((WRAP[0], WRAP[1]), (WRAP[2], WRAP[3])):
            on = i == src
            exp[dst, j[on], k[on]] = exp[src, j[on], k[on]]
        exp_dot = reference.rows_dot(u, rows, g, sacc_c)
        ud = u.to(DEV)
        rl = kernels.row_list(rows, ud)
        sacc = sacc_c.to(DEV)
        kernels.rows_dot(ud, rl, g.to(DEV), sacc)
        what = f"{stream} = {value}"
        _same_or_both_nonfinite(sacc.cpu(), exp_dot, what)
        kernels.inject_rows(ud, m.to(DEV), rl, g.to(DEV), WRAP)
        _same_or_both_nonfinite(ud.cpu(), exp, what)
        if stream is not None:
            assert not bool(torch.isfinite(exp_dot).all() and torch.isfinite(exp).all()), what
