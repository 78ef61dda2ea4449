"""The oracle's is_valid_equilibrium_hetero on caller knots against the numpy restatement of
tests/hetero_invalid_cases.py (heterogeneity_solver.jl:175-210): the two recorded knot sets whose
bisection root comes after an earlier above → not-above knot pair, and every variant the GPU test
(tests/test_gpu_hetero_invalid.py) runs.  The seeds' verdicts are found again here, so a changed
oracle cannot silently lose the invalid class."""
import numpy as np
import pytest

import hetero_invalid_cases as H


@pytest.fixture(scope="module")
def cases(oracle):
    return H.build(oracle.hetero_equilibrium_knots)


def test_the_seeds_are_invalid_where_recorded(oracle):
    for seed, ok_u in ((H.SEED_A, H.U_GRID), (H.SEED_B, np.array(H.SEED_B["u_invalid"]))):
        c = dict(H.seed_case(seed, "seed"), u=np.ascontiguousarray(ok_u[:8]))
        res = H.solve(oracle.hetero_equilibrium_knots, c)
        cls = H.check_against_numpy(c, res, "seed")
        for j, u in enumerate(c["u"]):
            assert (cls[j] == "invalid") == (float(u) in seed["u_invalid"]), (j, u, cls[j])
        j = list(c["u"]).index(seed["u_invalid"][0])
        e = H.expected(c, res["tau_in_unc"][j], res["tau_out_unc"][j])
        assert (e["pairs"][0], e["pairs"][0] + 1) == seed["pair"] and len(e["pairs"]) == 1 and e["m"] == seed["m_knots"]
        assert int(res["status"][j]) & ~H.INFO_BITS == H.INVALID
    # ξ ≈ 7.0614 and 6.7834 (the root the bisection found before the validity check refused it)
    a = H.seed_case(H.SEED_A, "A")
    r = H.solve(oracle.hetero_equilibrium_knots, a)
    assert abs(H.expected(a, r["tau_in_unc"][0], r["tau_out_unc"][0])["xi"] - 7.0614) < 1e-4
    b = H.seed_case(H.SEED_B, "B")
    r = H.solve(oracle.hetero_equilibrium_knots, b)
    assert abs(H.expected(b, r["tau_in_unc"][0], r["tau_out_unc"][0])["xi"] - 6.7834) < 1e-4


def test_the_restatement_sees_one_knot(oracle):
    """The numpy verdict is decided by single knots: lifting the first not-above knot after the pair
    back above κ (one G value of one group) moves the pair on by exactly one knot."""
    c = H.seed_case(H.SEED_A, "A")
    i, e = H.the_pair(oracle.hetero_equilibrium_knots, c)
    r = H.solve(oracle.hetero_equilibrium_knots, c)
    lift = (c["kappa"] - e["path"][i + 1]) / c["dist"][1] + 1e-6
    G = c["G"].copy()
    G[i + 1, 1] += lift
    e2 = H.expected(dict(c, G=G), r["tau_in_unc"][0], r["tau_out_unc"][0])
    assert e2["pairs"][0] == i + 1


def test_oracle_on_every_variant(oracle, cases):
    seen = {}
    assert len(cases) >= 20
    for c in cases:
        res = H.solve(oracle.hetero_equilibrium_knots, c)
        if c.get("no_numpy"):
            cls = ["invalid" if int(s) & ~H.INFO_BITS == H.INVALID else "other" for s in res["status"]]
        else:
            cls = H.check_against_numpy(c, res, "oracle")
        for k in cls:
            seen[k] = seen.get(k, 0) + 1
        inv = np.array([k == "invalid" for k in cls])
        assert np.isnan(res["xi"][inv]).all() and np.isnan(res["aw_max"][inv]).all() and np.isinf(res["tol"][inv]).all()
    assert seen["invalid"] >= 25 and seen["run"] >= 4 and seen["below"] >= 3 and seen["norun"] >= 2
    assert {len(c["dist"]) for c in cases} == {2, 3, 5, 9, 16}
    # four cases whose verdict the kernels' block bounds give without evaluating a knot after the pair
    # (the builder restates the bounds and asserts it): after an above block and after an evaluated one
    assert sum("bounds decide after an above block" in c["name"] for c in cases) == 2
    assert sum("bounds decide after an evaluated block" in c["name"] for c in cases) == 2
