"""The AW_max scan's slope-monotone window (csrc/sbr_solve_dev.h aw_scan, found in eq_column's
summary pass), restated in tools/aw_scan_sim.py: on learning CDFs the scan stops at the peak and
still returns the exhaustive maximum bit for bit; where the CDF's shape fails near the peak the
window ends before the failure and the maximum is still the exhaustive one.  CPU only."""
import bisect
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import aw_scan_sim as sim  # noqa: E402

import sbr  # noqa: E402

O = sim.O


@pytest.fixture(scope="module")
def columns():
    """Three config-3 columns (β = 1e4 carries ulp-sized decreases in its tail: dd > 0) and 16 u."""
    g = sbr.fig5_grid(2048)
    cols = [(float(g.beta[ci]),) + tuple(O.learn_logistic(float(g.beta[ci]), 30.0)[:2]) for ci in (0, 1024, 2047)]
    return cols, g.u[np.linspace(0, 2047, 16).astype(int)]


def exhaustive_max(col, o):
    """get_AW's maximum over every τ̄ knot, the reference's operations (solver.jl:553-576)"""
    T, G, n, nle, ntau, eta = col["T"], col["G"], col["n"], col["nle"], col["ntau"], col["eta"]
    xi, tin, tout = o["xi"], o["tau_in_unc"], o["tau_out_unc"]
    icc = xi if tin >= xi else tin
    occ = xi if tout > xi else tout

    def lerp(x):
        k = min(bisect.bisect_right(T, x) - 1, n - 2)
        d = (x - T[k]) / (T[k + 1] - T[k])
        return G[k] * (1.0 - d) + G[k + 1] * d

    G0 = lerp(0.0)
    mx = -np.inf
    for i in range(ntau):
        ti = T[i] if i < nle else eta
        av, bv = (ti - xi) + icc, (ti - xi) + occ
        awin = lerp(av if av > 0 else 0.0) if av >= 0 else 0.0
        awout = lerp(bv if bv > 0 else 0.0) if bv >= 0 else 0.0
        v = (awout - awin) + G0
        mx = v if v > mx else mx
    return mx


def test_learning_columns_stop_at_the_peak(columns):
    cols, us = columns
    r = sim.window_counts(cols, us, check=exhaustive_max)  # asserts every maximum == the oracle's
    assert any(w[4] > 0 for w in r["windows"]), "no drawdown column in the sample"
    assert all(w[3] != sim.EMPTY_WINDOW and w[1] >= w[2] - 20 for w in r["windows"]), r["windows"]
    assert r["points"] >= 12
    print(f"{r['points']} run points: exact evaluations {r['exact'][0]} shipped, {r['exact'][1]} with the window")
    # a cap that a silently disabled window fails (the simulation gives ≈0.10), not a performance claim
    assert 4 * r["exact"][1] <= r["exact"][0], r["exact"]


def half_knot(G):
    return bisect.bisect_right(list(G), 0.5) - 1


def bump(t, G):
    """+δ on four knots just past the CDF's inflection (G stays nondecreasing): AW_cum gets a
    second hump for every point whose peak lies before them"""
    G = G.copy()
    k = half_knot(G) + 4
    G[k:k + 4] += 0.5 * min(G[k] - G[k - 1], G[k + 4] - G[k + 3])
    return G, k


def equal_slopes(t, G):
    """five knots put on one line: a run of equal slopes"""
    G = G.copy()
    k = half_knot(G) + 4
    G[k:k + 5] = G[k] + (G[k + 4] - G[k]) * (t[k:k + 5] - t[k]) / (t[k + 4] - t[k])
    return G, k


def decrease(t, G):
    """one decrease of 1e-13 (within Summ::scan's drawdown bound, so the scan still runs)"""
    G = G.copy()
    k = half_knot(G) + 4
    G[k + 1] = G[k] - 1e-13
    return G, k


@pytest.mark.parametrize("perturb", [bump, equal_slopes, decrease])
def test_window_ends_before_a_shape_failure(columns, perturb):
    cols, us = columns
    pert, where = [], []
    for beta, t, G in cols:
        Gp, k = perturb(t, G)
        assert np.all(np.diff(Gp) >= -2e-13)  # Summ::scan's drawdown bound (1e-12) holds
        pert.append((beta, t, Gp))
        where.append(k)
    r = sim.window_counts(pert, us, check=exhaustive_max)
    assert r["points"] >= 12
    for (kc, wb, n, win, dd), k in zip(r["windows"], where):
        # the window shrinks to end at the failure (or vanishes)
        assert win == sim.EMPTY_WINDOW or wb <= k + 4, (perturb.__name__, wb, k, n)
