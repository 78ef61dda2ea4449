"""GPU parity of the AW_max scan's slope-monotone window (aw_scan: the scan stops at the peak where
the CDF's knot-to-knot slopes rise and then fall).  Every comparison is bitwise (xi, tau_in_unc,
tau_out_unc, aw_max, tol, status, iters) against the oracle and against the same call with
SBR_FLAG_EXHAUSTIVE; the evaluation counts show that the shortcut is taken."""
import bisect

import numpy as np
import pytest

import sbr
from sbr import _lib

pytestmark = pytest.mark.gpu

FIELDS = ("xi", "tau_in_unc", "tau_out_unc", "aw_max", "tol")
RUN = sbr.STATUS["SBR_RUN"]
# fig5 columns: β = 1e4 (column 0) and β = 11.49 (column 178) carry ulp-sized decreases in the tail of G
BETAS = [1.0, 1.376, 2.05, 11.49, 22.95, 1e4]
U128 = sbr.julia_range("0.001", "1", 128)
P, KAPPA, LAM, X0 = 0.5, 0.6, 0.01, 1e-4


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check_sweep(g, o, name, iters=True):
    for f in FIELDS:
        assert same(g[f], o[f]), (name, f)
    assert np.array_equal(g["status"], o["status"]), name
    if iters:
        assert np.array_equal(g["iters"], o["iters"]), name


def check_vector(g, os, name):
    for j, o in enumerate(os):
        for f in FIELDS:
            assert same(g[f][j], o[f]), (name, j, f, g[f][j], o[f])
        assert int(g["status"][j]) == o["status"], (name, j, hex(int(g["status"][j])), hex(o["status"]))
        assert int(g["iters"][j]) == o["iters"], (name, j, int(g["iters"][j]), o["iters"])


def t_half(beta):
    return np.log(1.0 / X0 - 1.0) / beta  # the logistic's G = 1/2


def sweep_grid(kind):
    beta = np.array(BETAS)
    if kind == "eta15":
        return sbr.BaselineGrid(beta, U128, 15.0, 30.0)
    if kind == "eta_below_t_half":  # τ* = t_half + ... lies beyond the last τ̄: the scan is not used (and no point runs)
        return sbr.BaselineGrid(beta, U128, 0.9 * t_half(beta), 30.0)
    if kind == "eta_above_t_half":  # G(η) = 0.82: run points with τ* beyond the last τ̄ and others with τ* on the grid
        return sbr.BaselineGrid(beta, U128, t_half(beta) + 1.5 / beta, 30.0)
    return sbr.BaselineGrid(beta, U128, 30.0, 30.0)  # η = t_end


@pytest.mark.parametrize("kind", ["eta15", "eta_below_t_half", "eta_above_t_half", "eta_t_end"])
def test_sweeps_equal_oracle_and_exhaustive(engine, oracle, kind):
    grid = sweep_grid(kind)
    o = oracle.sweep_baseline(grid.beta, grid.eta, grid.t_end, grid.u, grid.p, grid.kappa, grid.lam, grid.x0)
    g = engine.sweep_baseline(grid)
    check_sweep(g, o, kind)
    check_sweep(engine.sweep_baseline(grid, exhaustive=True), o, kind + " exhaustive")
    run = (o["status"] & RUN) > 0
    if kind != "eta_below_t_half":
        # u spans the run boundary: run points and others in the β = 1 column, runs in every column
        assert 0 < run[0].sum() < 128 and np.all(run.sum(axis=1) > 0), run.sum(axis=1)


def logistic(t, beta, t0):
    return 1.0 / (1.0 + np.exp(-beta * (t - t0)))


def half_knot(G):
    return bisect.bisect_right(list(G), 0.5) - 1


def with_bump(G, k):
    """+δ on knots k..k+3, G still nondecreasing (tests/test_aw_window_sim.py's bump)"""
    G = G.copy()
    G[k:k + 4] += 0.5 * min(G[k] - G[k - 1], G[k + 4] - G[k + 3])
    return G


def knot_cases(oracle):
    """(name, t, G, β, η, u): shapes the learning ODE never produces, through the sweep kernel on
    the caller's knots (n_u >= 2)"""
    u64 = sbr.julia_range("0.001", "0.3", 64)
    cases = []
    for n in (3, 4, 9):
        t = np.linspace(0.0, 30.0, n)
        cases.append((f"{n} knots", t, logistic(t, 1.0, t_half(1.0)), 1.0, 15.0, u64))
    t = np.linspace(0.0, 30.0, 401)
    two = 0.5 * logistic(t, 2.0, 6.0) + 0.5 * logistic(t, 2.0, 14.0)  # two slope maxima
    cases.append(("two logistics", t, two, 2.0, 25.0, sbr.julia_range("0.001", "0.6", 128)))
    ramp = np.clip((t - 4.0) / 10.0, 1e-4, 1.0)  # slopes 0, 1/10 (equal, 133 times), 0
    cases.append(("equal slopes", t, ramp, 1.0, 15.0, u64))
    tl, Gl, _ = oracle.learn_logistic(1.0, 30.0)
    # the peak knot of a middle run point of the learned β = 1 column, as the kernel predicts it
    mid = oracle.equilibrium(tl, Gl, 1.0, 15.0, 30.0, 0.05, P, KAPPA, LAM)
    assert mid["status"] & RUN
    xi, tin, tout = mid["xi"], mid["tau_in_unc"], mid["tau_out_unc"]
    icc, occ = (xi if tin >= xi else tin), (xi if tout > xi else tout)
    k = half_knot(Gl)
    th = tl[k] + (0.5 - Gl[k]) * (tl[k + 1] - tl[k]) / (Gl[k + 1] - Gl[k])
    c = bisect.bisect_right(list(tl), th + 0.5 * ((xi - icc) + (xi - occ))) - 1
    u_near = np.linspace(0.03, 0.07, 64)  # peaks around knot c
    cases.append(("bump at the peak's right neighbour", tl, with_bump(Gl, c + 1), 1.0, 15.0, u_near))
    cases.append(("bump past the stopping knot", tl, with_bump(Gl, c + 2), 1.0, 15.0, u_near))
    # η on a knot inside the window: the τ̄ grid ends there (no extra η entry), right of most peaks / at them
    for teta in (12.0, 10.5):
        kw = bisect.bisect_right(list(tl), teta)
        cases.append((f"eta on the knot after t = {teta}", tl, Gl, 1.0, float(tl[kw]), u64))
    return cases


@pytest.fixture(scope="module")
def cases(oracle):
    return {c[0]: c for c in knot_cases(oracle)}


@pytest.mark.parametrize("name", ["3 knots", "4 knots", "9 knots", "two logistics", "equal slopes",
                                  "bump at the peak's right neighbour", "bump past the stopping knot",
                                  "eta on the knot after t = 12.0", "eta on the knot after t = 10.5"])
def test_caller_knots_equal_oracle_and_exhaustive(engine, oracle, cases, name):
    _, t, G, beta, eta, u = cases[name]
    os = [oracle.equilibrium(t, G, beta, eta, 30.0, float(x), P, KAPPA, LAM) for x in u]
    g = engine.equilibrium_on_knots(t, G, beta, eta, 30.0, u, P, KAPPA, LAM, paths=False)
    check_vector(g, os, name)
    ge = engine.equilibrium_on_knots(t, G, beta, eta, 30.0, u, P, KAPPA, LAM, paths=False, exhaustive=True)
    check_vector(ge, os, name + " exhaustive")


def test_the_window_cuts_the_exact_evaluations(engine, oracle):
    """SBR_FLAG_DIAG_COUNT_AW_BLOCKS returns a run point's exact AW_cum evaluations in `iters`;
    SBR_FLAG_DIAG_NO_AW_WINDOW makes the scan ignore the window.  Same results, and at most a
    quarter of the evaluations with the window (a cap that a silently disabled window fails; the
    simulator gives a tenth)."""
    grid = sweep_grid("eta15")
    o = oracle.sweep_baseline(grid.beta, grid.eta, grid.t_end, grid.u, grid.p, grid.kappa, grid.lam, grid.x0)
    count = _lib.SBR_FLAG_DIAG_COUNT_AW_BLOCKS
    gw = engine.sweep_baseline(grid, flags=count)
    gn = engine.sweep_baseline(grid, flags=count | _lib.SBR_FLAG_DIAG_NO_AW_WINDOW)
    check_sweep(gw, o, "window", iters=False)
    check_sweep(gn, o, "no window", iters=False)
    run = (o["status"] & RUN) > 0
    nw, nn = int(gw["iters"][run].sum()), int(gn["iters"][run].sum())
    print(f"{int(run.sum())} run points: {nw} exact evaluations with the window, {nn} without")
    assert np.all(gw["iters"][run] >= 1)
    assert 4 * nw <= nn, (nw, nn)
    # without the flag the kernel does not look at the bit: plain results carry the bisection count
    check_sweep(engine.sweep_baseline(grid, flags=_lib.SBR_FLAG_DIAG_NO_AW_WINDOW), o, "no window, plain")
