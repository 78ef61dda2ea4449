"""SBR_HETERO_INVALID on the GPU: sbr_hetero_equilibrium_on_knots on the knot sets of
tests/hetero_invalid_cases.py, whose bisection root comes after an earlier above → not-above knot
pair, with the pair moved through the kernels' 64-knot blocks (inside one, across a boundary,
starting one, in the last partial block, ending a block whose successor the bounds alone put not
above κ),
a dip that stays above κ, K = 5, 9, 16 by splitting groups, a non-monotone tail, a NaN that forces
the per-knot path, and launches that mix invalid, run, no-run and below points.  Every case runs on
the specialised and the group-looped kernel, pruned and exhaustive, and must give the numpy
restatement's class — invalid there and nowhere else — and the oracle's result bit for bit."""
import numpy as np
import pytest

import hetero_invalid_cases as H

pytestmark = pytest.mark.gpu

FIELDS = ("xi", "aw_max", "tol", "tau_in_unc", "tau_out_unc")


@pytest.fixture(scope="module")
def cases(oracle):
    built = H.build(oracle.hetero_equilibrium_knots)
    return [(c, H.solve(oracle.hetero_equilibrium_knots, c)) for c in built]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check(c, g, o, what):
    for f in FIELDS:
        assert same(g[f], o[f]), (what, c["name"], f, g[f], o[f])
    assert np.array_equal(g["status"], o["status"]), (what, c["name"], g["status"], o["status"])
    assert np.array_equal(g["iters"], o["iters"]), (what, c["name"])
    inv = (np.asarray(g["status"]) & ~np.uint32(H.INFO_BITS)) == H.INVALID
    assert np.isnan(g["xi"][inv]).all() and np.isnan(g["aw_max"][inv]).all() and np.isinf(g["tol"][inv]).all()
    assert np.isfinite(g["tau_in_unc"][inv]).all() and np.isfinite(g["tau_out_unc"][inv]).all()
    if not c.get("no_numpy"):
        cls = H.check_against_numpy(c, g, what)
        assert [k == "invalid" for k in cls] == list(inv), (what, c["name"], cls)
    return int(inv.sum())


@pytest.mark.parametrize("exhaustive", [False, True], ids=["pruned", "exhaustive"])
@pytest.mark.parametrize("wide", [False, True], ids=["specialised", "group-looped"])
def test_every_variant(engine, cases, wide, exhaustive):
    n_inv = 0
    for c, o in cases:
        g = H.solve(engine.hetero_equilibrium_on_knots, c, paths=False, wide=wide, exhaustive=exhaustive)
        n_inv += check(c, g, o, f"wide={wide} exhaustive={exhaustive}")
    assert n_inv >= 25


def test_same_knots_twice_and_single_points(engine, cases):
    """Residency: a launch that mixes invalid, run, no-run and below points, then the same knots
    again (resident), then its points one per call with paths: all equal."""
    for c, o in [(c, o) for c, o in cases if c["name"].endswith("mixed u")]:
        call = lambda **kw: H.solve(engine.hetero_equilibrium_on_knots, c, **kw)  # noqa: E731
        a, b = call(paths=False), call(paths=False)
        check(c, a, o, "first")
        check(c, b, o, "again")
        for j, u in enumerate(c["u"]):
            one = H.solve(engine.hetero_equilibrium_on_knots, dict(c, u=np.array([u])), paths=True)
            for f in FIELDS:
                assert same(one[f][0], o[f][j]), (c["name"], j, f)
            assert int(one["status"][0]) == int(o["status"][j]) and int(one["iters"][0]) == int(o["iters"][j])
            if int(o["status"][j]) & ~H.INFO_BITS == H.INVALID:
                assert np.isnan(one["aw_total"]).all()
