"""The seeded draws of tests/random_cases.py on the oracle alone (CPU): every family's draw holds what it
is drawn for — the outcome classes, the column shapes, the mixed waves, the long value functions, the
fixed points that converge and those that do not — so that a change in numpy's stream or an edit to the
ranges fails here and does not silently thin tests/test_gpu_random.py.  And a point's result is a
function of the point: the oracle gives the same bits whether a column's u come as drawn, sorted,
reversed or shuffled."""
import numpy as np
import pytest

import random_cases as R


@pytest.mark.parametrize("family", R.FAMILIES)
def test_premise(oracle, family):
    facts, fails = R.premise(oracle, family)
    print(family, facts)
    assert not fails, (family, fails, facts)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_draw_shapes_and_invalid_lanes(family):
    for c in R.calls_of(family):
        if family == "points":
            n = len(c["args"]["u"])
            assert n == 130 and len(c["bad"]) == 6 and 100 * len(c["bad"]) <= 5 * n
            changed = sum(int((~((c["args"][k] == c["args_bad"][k]))).sum()) for k in c["args"])
            assert changed == 6
            continue
        u = c["u"]
        assert (u >= 0).all() and (u == 0).sum() >= 1 and len(np.unique(u)) < len(u), c["name"]
        assert not (np.diff(u) >= 0).all() and not (np.diff(u) <= 0).all(), c["name"]  # not sorted
        assert (c["eta"] <= c["t_end"]).all() and (c["beta"] > 0).all()
        if family == "social":
            assert c["cmp"].shape == (8, 1000) and len(u) == 9 and c["max_iter"] <= 6 and c["tol"] == 1e-4
            continue
        bad = c["bad"]
        assert 1 <= len(bad) and (100 * len(bad) <= 5 * len(u) or len(u) < 20), c["name"]
        ok = np.ones(len(u), bool)
        ok[bad] = False
        assert np.array_equal(c["u_bad"][ok], u[ok]) and not (c["u_bad"][bad] >= 0).any(), c["name"]
        if family.endswith("econ"):
            assert (len(c["u"]), len(c["kappa"]), len(c["p"]), len(c["lam"])) == (5, 13, 2, 2)
            # a κ × u plane is κ-major: its 65 points are one full wave holding all 13 κ and a one-lane wave
            assert len(set(np.repeat(np.arange(13), 5)[:64].tolist())) == 13 >= 3
            for q, mask in R.spoil_axes(c):
                assert 0 < mask.sum() < mask.size
        if "K" in c:
            assert c["betas"].shape == (len(c["beta"]), c["K"]) and abs(c["dist"].sum() - 1.0) < 1e-10
            assert 1 <= c["K"] <= 16 and (c["dist"] >= 0).all()
    if family in ("baseline", "interest"):
        shapes = {(len(c["beta"]), len(c["u"])) for c in R.calls_of(family)}
        assert {(70, 65), (6, 33)} <= shapes and ((193, 65) in shapes) == (family == "baseline")
    if family == "hetero":
        cs = R.calls_of(family)
        assert sum(len(c["beta"]) for c in cs) == 16 and len({c["K"] for c in cs}) == len(cs)


@pytest.mark.parametrize("family,name", [("baseline", "pair1"), ("baseline", "high0"), ("interest", "pair0"),
                                         ("hetero", None)])
def test_oracle_result_is_a_function_of_the_point(oracle, family, name):
    calls, refs = R.reference(oracle, family)
    i = 0 if name is None else [c["name"] for c in calls].index(name)
    c, ref = calls[i], refs[i]
    n = len(c["u"])
    rng = np.random.default_rng(0)
    fields = [k for k in ref if k != "n_knots"]
    for what, perm in (("sorted", np.argsort(c["u"], kind="stable")), ("reversed", np.arange(n)[::-1]),
                       ("shuffled", rng.permutation(n))):
        o = R.oracle_call(oracle, dict(c, u=c["u"][perm]))
        want = {k: ref[k][:, perm] for k in fields}
        R.assert_equal(o, want, c, f"oracle, u {what}", fields, u=c["u"][perm])
