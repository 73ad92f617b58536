"""The mode table of ops.kernels.step_medium, host-only: the pure resolver ``medium_mode`` against the rules
written out here, over every subset of the six mode keywords x first x buoyancy x order x variant (3840
cases). tests/test_gpu_medium_modes.py runs the same cases through step_medium and the native launcher."""
import itertools

import pytest

KEYWORDS = ("lap_out", "image", "born", "scatter", "born_add", "illum")
# the keyword sets that name a mode, and the mode
MODES = {
    frozenset(): "plain",
    frozenset({"lap_out"}): "save",
    frozenset({"image"}): "image",
    frozenset({"born"}): "born",
    frozenset({"scatter"}): "scatter",
    frozenset({"born_add"}): "born_add",
    frozenset({"illum"}): "illum",
    frozenset({"lap_out", "illum"}): "save_illum",
}
ORDERS = (2, 4, 8)
VARIANTS = (None, "nt", "plain", "r2", "r2nt")


def cases():
    """(keywords given, first, buoyancy given, order, variant) of all 3840 cases."""
    for r in range(len(KEYWORDS) + 1):
        for given in itertools.combinations(KEYWORDS, r):
            for first, buoyancy, order, variant in itertools.product((True, False), (False, True), ORDERS, VARIANTS):
                yield given, first, buoyancy, order, variant


def _present(given):
    """The resolver's presence flags for the keywords ``given``."""
    return tuple(k in given for k in KEYWORDS)


def expected(given, first, buoyancy, order, variant):
    """The mode's name if the call is accepted, None if it is refused."""
    given = frozenset(given)
    default = variant in (None, "nt")
    ok = (given in MODES
          and (not given or (not first and default))              # a mode: a leapfrog step of the default variant
          and (not given & {"scatter", "born_add"} or buoyancy)   # the two modes of the density kernel alone
          and (not buoyancy or (order == 2 and default))          # the density kernel: order 2, default variant
          and (order == 2 or variant is None))                    # orders 4 and 8 have no variants
    return MODES[given] if ok else None


def test_case_count():
    assert sum(1 for _ in cases()) == 3840
    assert sum(1 for c in cases() if expected(*c) is not None) == 52


def test_medium_mode_resolver_against_the_rules():
    from wave3d.ops.kernels import medium_mode

    wrong = []
    for case in cases():
        given, first, buoyancy, order, variant = case
        try:
            mode, run_variant = medium_mode(_present(given), first, order, variant, buoyancy)
            got = mode.name
            # the variant that runs: the one asked for, or by name the default one where the mode or the
            # density kernel has no other (an ablation run may have changed the process's default)
            pinned = order == 2 and (bool(given) or buoyancy)
            assert run_variant == ("nt" if pinned else variant), case
        except ValueError:
            got = None
        if got != expected(*case):
            wrong.append((case, got))
    assert not wrong, wrong[:10]


@pytest.mark.parametrize("kw, word", [
    (dict(given=("lap_out",), first=True), "first"),
    (dict(given=("illum", "lap_out"), first=True), "first"),
    (dict(given=("born",), variant="r2"), "variant"),
    (dict(given=("lap_out", "image")), "combined"),
    (dict(given=("illum", "born")), "combined"),
    (dict(given=("scatter", "born_add"), buoyancy=True), "combined"),
    (dict(given=("scatter",)), "buoyancy"),
    (dict(given=("born_add",), order=4), "buoyancy"),
    (dict(given=("scatter",), buoyancy=True, order=4), "order"),
    (dict(given=(), buoyancy=True, order=8), "order 2"),
    (dict(given=(), order=6), "order"),
    (dict(given=(), order=4, variant="nt"), "variant"),
    (dict(given=(), variant="fast"), "variant"),
])
def test_medium_mode_messages(kw, word):
    """The words that callers and the GPU tests match in a refusal."""
    from wave3d.ops.kernels import medium_mode

    kw = dict(dict(first=False, order=2, variant=None, buoyancy=False), **kw)
    with pytest.raises(ValueError, match=word):
        medium_mode(_present(kw.pop("given")), **kw)


def test_mode_table_rows():
    """One row per mode, under the names of the native entry point's grids after renaming."""
    from wave3d.ops import kernels

    assert [r.name for r in kernels._MEDIUM_MODES] == list(MODES.values())
    assert {frozenset(r.grids): r.name for r in kernels._MEDIUM_MODES} == MODES
    for r in kernels._MEDIUM_MODES:
        own = [n for names in r.grids.values() for n in ([names] if isinstance(names, str) else names)]
        for grid, others in r.apart:  # a no-shared-memory rule: a grid the step writes, against own grids and levels
            assert grid in own + ["u"]
            assert set(others) <= set(own) | {"u", "u1", "u2", "m", "buoyancy"} and grid not in others
