"""The CPU oracle against the continuum model of the run (tests/continuum.py): an independent
float64 reference — the logistic in closed form, the hazard and the value function by scipy's
DOP853, ξ and AW_max in closed form — that shares no code and no reading of the reference with
oracle/sbr_oracle.c.  Its expected values are recorded in tests/golden/continuum.json by
tools/make_continuum_golden.py, away from the figures' p = 0.5, κ = 0.6, λ = 0.01, x0 = 1e-4.

Tolerances are the project's knot-grid sensitivity, 2e-5 on ξ, τ̄_IN, τ̄_OUT and 1e-5 on AW_max
(tests/test_oracle_golden.py); the oracle alone must stay within half of each, so that the GPU test
(tests/test_gpu_continuum.py) has the other half."""
import numpy as np
import pytest

import continuum as C
import continuum_cases as CC

VALUES = ("tau_in", "tau_out", "xi", "aw_max")


@pytest.fixture(scope="module")
def fix():
    return CC.load()


def _within_half(dev, recorded):
    assert dev["time"] <= CC.TOL_TIME / 2 and dev["aw"] <= CC.TOL_AW / 2, dev
    assert dev == recorded  # the maxima the fixture and DESIGN.md §2 state


def test_the_fixture_is_what_the_issue_asks(fix):
    m = fix["meta"]
    assert m["dropped"] <= 0.10 * m["drawn"] and m["dropped_share"] == m["dropped"] / m["drawn"]
    assert len(fix["points"]["cls"]) == 96  # more than one learning wave, the second partial
    assert fix["econ"]["shape"] == [3, 2, 2, 3, 8] and fix["interest_econ"]["shape"] == [2, 2, 1, 2, 2, 6]
    assert fix["interest_econ"]["r"][0] == 0.0 and fix["interest_econ"]["r"][1] > 0.0
    assert {c["K"] for c in fix["hetero"]} == {1, 2, 3, 5, 8, 12, 16} and len(fix["hetero"]) == 21
    for c in fix["hetero"]:
        assert len(set(c["dist"])) == c["K"] and abs(sum(c["dist"]) - 1.0) < 1e-15
    seen = list(fix["points"]["cls"]) + [c["cls"] for c in fix["hetero"]]
    for name in ("econ", "interest_econ"):
        seen += [c for c, ok in zip(fix[name]["cls"], fix[name]["ok"]) if ok]
    assert all(seen.count(c) >= 1 for c in C.CLASSES) and seen.count("false") >= 2
    assert fix["points"]["cls"].count("false") >= 2
    assert {c: seen.count(c) for c in C.CLASSES} == m["classes"]
    # float64 against mpmath: at least 1000 times below the tolerances, one point per class and more
    mp = m["mpmath"]
    assert mp["digits"] >= 40 and len(mp["points"]) >= 6
    assert all(any(c in p for p in mp["points"]) for c in C.CLASSES)
    assert mp["max_time_diff"] <= CC.TOL_TIME / 1000 and mp["max_aw_diff"] <= CC.TOL_AW / 1000


def test_oracle_points(oracle, fix):
    P = fix["points"]
    dev = CC.compare(CC.oracle_points(oracle, P), P["cls"], P, P["t_end"], what="oracle points")
    _within_half(dev, fix["meta"]["oracle"]["points"])


@pytest.mark.parametrize("name", ["econ", "interest_econ"])
def test_oracle_grids(oracle, fix, name):
    """sweep_baseline / sweep_interest per (p, λ, [rate,] κ) against every well-conditioned element."""
    E = fix[name]
    dev = CC.compare(CC.oracle_grid(oracle, E), *CC.grid_want(E), what=f"oracle {name}")
    _within_half(dev, fix["meta"]["oracle"][name])


def test_oracle_hetero_with_equal_rates(oracle, fix):
    """K groups at one rate are the baseline model (ω = G: the shares sum to 1) — with the two
    differences the reference has (heterogeneity_solver.jl:316-375): AW_max without + G(0), and taken
    over the learning grid up to t_end.  Every group's buffers must be the continuum's pair."""
    worst = {"time": 0.0, "aw": 0.0}
    past_eta = 0
    for n, case in enumerate(fix["hetero"]):
        res = CC.oracle_hetero(oracle, case)
        if case["cls"] == "run":  # the peak lies past η: only the t_end clip gives the right AW_max
            th = np.log((1 - case["x0"]) / case["x0"]) / case["beta"]
            past_eta += th + (case["xi"] - case["tau_in"]) / 2 > case["eta"]
        for got in CC.hetero_got(res, case["K"]):
            d = CC.compare(got, [case["cls"]], CC.hetero_want(case), [case["t_end"]], what=f"oracle hetero {n}")
            worst = {k: max(worst[k], d[k]) for k in worst}
    _within_half(worst, fix["meta"]["oracle"]["hetero"])
    assert past_eta >= 1


def test_solve_hetero_with_equal_rates_is_solve(fix):
    """The K-group model (DOP853 on (G_k, I_k), brentq for ξ, scans for the validity path and AW_max)
    at equal rates against the closed-form model it must collapse to: every field to 1e-9."""
    for case in fix["hetero"]:
        a = C.solve(*[case[k] for k in CC.PARAMS], case["x0"], hetero=True)
        b = C.solve_hetero([case["beta"]] * case["K"], case["dist"], case["eta"], case["t_end"], case["u"], case["p"],
                           case["kappa"], case["lam"], case["x0"])
        assert a["cls"] == b["cls"] == case["cls"] and b["ok"], (case["K"], a["cls"], b["cls"], b["reason"])
        assert np.shape(b["tau_in"]) == np.shape(b["tau_out"]) == (case["K"],)
        for k in VALUES:
            if a[k] != a[k]:
                assert np.isnan(b[k]).all(), k
            else:
                assert float(np.max(np.abs(np.asarray(b[k]) - a[k]))) <= 1e-9, (case["K"], k, b[k], a[k])


def test_the_unequal_rate_list_is_what_the_issue_asks(fix):
    H, m = fix["hetero_unequal"], fix["meta"]["hetero_unequal"]
    assert len(H) == 48
    assert {c["K"] for c in H} == {2, 3, 5, 8, 12, 16}
    for c in H:
        b, d = np.array(c["betas"]), np.array(c["dist"])
        assert len(b) == len(d) == c["K"] and abs(d.sum() - 1.0) < 1e-15 and len(set(c["dist"])) == c["K"]
        assert 1.5 * (1 - 1e-12) <= b.max() / b.min() <= 30.0 * (1 + 1e-12) and 1.0 <= b.min() and b.max() <= 60.0
        rise = np.log((1 - c["x0"]) / c["x0"]) / float(d @ b)
        assert 1.2 * rise <= c["eta"] * (1 + 1e-12) and c["eta"] <= 4.0 * rise * (1 + 1e-12)
        assert 1.2 * c["eta"] * (1 - 1e-12) <= c["t_end"] <= 2.0 * c["eta"] * (1 + 1e-8)
        assert 0 <= c["t_end_redraws"] <= 3
        below = np.array(c["tau_in"]) == np.array(c["tau_out"])
        assert c["mixed"] == bool(below.any() and not below.all())
        assert (c["cls"] == "below") == bool(below.all())
    assert all(c["betas"] != sorted(c["betas"]) for c in H if c["K"] > 3)  # shuffled: not in rate order
    seen = [c["cls"] for c in H]
    assert {k: seen.count(k) for k in set(seen)} == m["classes"]
    assert sum(c["mixed"] for c in H) == m["mixed"] >= 6
    assert seen.count("norun") >= 2 and seen.count("below") >= 2 and seen.count("false") >= 2
    assert sum(c["t_end_redraws"] for c in H) == m["t_end_redraws"]
    # drops, from conditioning and from the rounding BoundsError, within 10 % of all drawn points
    M = fix["meta"]
    assert m["dropped"] + M["dropped"] <= 0.10 * (m["drawn"] + M["drawn"])
    assert m["dropped_share_all_lists"] == (m["dropped"] + M["dropped"]) / (m["drawn"] + M["drawn"])
    mp = M["mpmath"]["hetero_unequal"]
    assert mp["digits"] >= 30 and H[mp["case"]]["K"] == 2 and H[mp["case"]]["cls"] == "run"
    assert mp["max_time_diff"] <= 1e-8 and mp["max_aw_diff"] <= 1e-9


def test_oracle_hetero_with_unequal_rates(oracle, fix):
    """Every group's own buffers, ξ, AW_max, the class and the sentinels of the oracle against the
    K-group continuum model: what is specific to heterogeneity — the dist-weighted AW(ξ) with
    per-group clipping, hazards from different pdf_k, groups below u beside groups with a window,
    the maximum of a multi-humped AW_total."""
    worst = {"time": 0.0, "aw": 0.0}
    for n, case in enumerate(fix["hetero_unequal"]):
        d = CC.hetero_compare(CC.oracle_hetero(oracle, case), case, f"oracle hetero_unequal {n}")
        worst = {k: max(worst[k], d[k]) for k in worst}
    _within_half(worst, fix["meta"]["oracle"]["hetero_unequal"])


def test_the_fixture_is_reproducible(fix):
    """A seeded subset recomputed with tests/continuum.py: classes and verdicts equal, values to 1e-10."""
    rng = np.random.default_rng(5)

    def same(res, cls, want, ok):
        assert res["cls"] == cls and res["ok"] == ok
        for k in ("tau_in", "tau_out", "xi", "aw_max"):
            assert (res[k] != res[k] and want[k] != want[k]) or abs(res[k] - want[k]) <= 1e-10, (k, res[k], want[k])

    P = fix["points"]
    for i in rng.choice(96, 12, replace=False):
        res = C.solve(*[P[k][i] for k in CC.PARAMS], P["x0"])
        same(res, P["cls"][i], {k: P[k][i] for k in VALUES}, True)
    for name in ("econ", "interest_econ"):
        E = fix[name]
        shape = tuple(E["shape"])
        for n in rng.choice(int(np.prod(shape)), 10, replace=False):
            ix = np.unravel_index(n, shape)
            i, a, b, c, j = ix[0], ix[1], ix[2], ix[-2], ix[-1]
            r, delta = (E["r"][ix[3]], E["delta"][ix[3]]) if "r" in E else (0.0, 0.1)
            res = C.solve(E["beta"][i], E["eta"][i], E["t_end"][i], E["u"][j], E["p"][a], E["kappa"][c], E["lam"][b],
                          E["x0"], r, delta)
            same(res, E["cls"][n], {k: E[k][n] for k in VALUES}, bool(E["ok"][n]))
    for case in fix["hetero"][::5]:
        res = C.solve(*[case[k] for k in CC.PARAMS], case["x0"], hetero=True)
        same(res, case["cls"], {k: np.nan if case[k] is None else case[k] for k in VALUES}, True)
    for case in fix["hetero_unequal"][::7]:
        res = C.solve_hetero(case["betas"], case["dist"], *[case[k] for k in CC.PARAMS[1:]], case["x0"])
        assert res["cls"] == case["cls"] and res["ok"]
        for k in ("tau_in", "tau_out"):
            assert float(np.max(np.abs(res[k] - np.array(case[k])))) <= 1e-10, k
        for k in ("xi", "aw_max"):
            assert (res[k] != res[k] and case[k] is None) or abs(res[k] - case[k]) <= 1e-10, k


@pytest.mark.parametrize("K", [2, 3, 5, 8, 16])
def test_hetero_learning_with_unequal_rates(oracle, K):
    """dG_k = (1 − G_k) β_k Σ_j dist_j G_j at the oracle's own knots against DOP853 at rtol 1e-13:
    relative difference ≤ 1e-10 (measured: ≤ 5.2e-12), on condition that a second scipy solve (Radau)
    agrees with the first to ≤ 1e-11."""
    rng = np.random.default_rng(100 + K)
    betas = 0.5 * 20.0 ** rng.random(K)
    d = rng.random(K) + 0.2
    d /= d.sum()
    d[-1] = 1.0 - d[:-1].sum()
    t_end, x0 = 24.0, 1e-4
    t, G, info = oracle.learn_hetero(betas, d, t_end, x0)
    assert info["status"] & ~0x800 == 0 and G.shape == (len(t), K) and t[-1] == t_end
    ref = C.hetero_learning(betas, d, t_end, x0, t)
    ref2 = C.hetero_learning(betas, d, t_end, x0, t, method="Radau", rtol=3e-14, atol=1e-20)
    cond = float(np.max(np.abs(ref2 - ref) / ref))
    got = float(np.max(np.abs(G - ref) / ref))
    print(f"hetero learning K={K}: {len(t)} knots, scipy DOP853 vs Radau {cond:.2e}, oracle vs DOP853 {got:.2e}")
    assert cond <= 1e-11
    assert got <= 1e-10
