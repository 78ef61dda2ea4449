"""GPU parity of the two-loop bisection (solve_from_buffers): loop A, the reference's
iteration with bracketed lookups, and loop B, which a wave enters once every lane still
iterating has its bracket inside one knot interval and which iterates on registers alone.
Every comparison is bitwise against the oracle: xi, tau_in_unc, tau_out_unc, aw_max, tol,
status and iters."""
import numpy as np
import pytest

import sbr

pytestmark = pytest.mark.gpu

FIELDS = ("xi", "tau_in_unc", "tau_out_unc", "aw_max", "tol")
RUN = sbr.STATUS["SBR_RUN"]
MAXITER = sbr.STATUS["SBR_NO_RUN_MAXITER"]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check_sweep(g, o, name):
    for f in FIELDS:
        assert same(g[f], o[f]), (name, f)
    assert np.array_equal(g["status"], o["status"]), name
    assert np.array_equal(g["iters"], o["iters"]), name


def check_vector(g, os, name):
    for j, o in enumerate(os):
        for f in FIELDS:
            assert same(g[f][j], o[f]), (name, j, f, g[f][j], o[f])
        assert int(g["status"][j]) == o["status"], (name, j, hex(int(g["status"][j])), hex(o["status"]))
        assert int(g["iters"][j]) == o["iters"], (name, j, int(g["iters"][j]), o["iters"])


@pytest.mark.parametrize("cap", [5, 12, 14, 20, 48, 100])
def test_iteration_caps_across_the_loop_switch(engine, oracle, cap):
    """bisect_max_iters below, at and above the iterations (10-17) at which lanes enter loop B,
    70 u per column (a full wave and a partial one).  Caps <= 20 end every bisected point at
    iters = cap - 1 with the max-iteration status; 48 splits them (22 run, 228 capped); 100 gives
    235 run points of 280."""
    grid = sbr.BaselineGrid([1.0, 3.0, 10.0, 40.0], sbr.julia_range("0.001", "0.3", 70), 15.0, 30.0)
    o = oracle.sweep_baseline(grid.beta, grid.eta, grid.t_end, grid.u, grid.p, grid.kappa, grid.lam, grid.x0,
                              max_iters=cap)
    g = engine.sweep_baseline(grid, max_iters=cap)
    check_sweep(g, o, cap)
    run = (o["status"] & RUN) > 0
    capped = (o["status"] & MAXITER) > 0
    if cap <= 20:
        assert run.sum() == 0 and capped.sum() == 250 and np.all(o["iters"][capped] == cap - 1)
    elif cap == 48:
        assert run.sum() == 22 and capped.sum() == 228
    else:
        assert run.sum() == 235


def test_lanes_that_never_enter_loop_b(engine, oracle):
    """η = t_end: brackets at the end of the grid fail ξmax + ε <= t[n−1], so their lanes (and
    the waves holding them) stay in loop A; β = 0.4 has a run point whose τ* is off the τ̄ grid.
    The oracle gives 11, 16 and 26 run points."""
    grid = sbr.BaselineGrid([0.4, 0.6, 1.0], sbr.julia_range("0.001", "0.4", 96), 30.0, 30.0)
    o = oracle.sweep_baseline(grid.beta, grid.eta, grid.t_end, grid.u, grid.p, grid.kappa, grid.lam, grid.x0)
    g = engine.sweep_baseline(grid)
    check_sweep(g, o, "eta = t_end")
    assert list(((o["status"] & RUN) > 0).sum(axis=1)) == [11, 16, 26]


def test_coarse_knots_switch_early(engine, oracle):
    """A column learned at tol = 1e-6 (43 knots, wide intervals): brackets are inside one knot
    interval within 2-3 iterations, so nearly the whole bisection runs in loop B."""
    t, G, _ = oracle.learn_logistic(1.0, 30.0, rtol=1e-6, atol=1e-6)
    assert len(t) < 100
    u = sbr.julia_range("0.001", "0.3", 64)
    g = engine.equilibrium_on_knots(t, G, 1.0, 15.0, 30.0, u, 0.5, 0.6, 0.01, paths=False)
    os = [oracle.equilibrium(t, G, 1.0, 15.0, 30.0, float(x), 0.5, 0.6, 0.01) for x in u]
    check_vector(g, os, "coarse")
    assert sum((o["status"] & RUN) > 0 for o in os) >= 16


def test_reversed_brackets_take_the_unspecialised_loop(engine, oracle):
    """An explicit pdf with a bump at t = 1 and η = 9: HR starts above a small u, dips below it
    and stays above it to the end, so the last 1→0 crossing precedes the first 0→1 one and
    τ̄_IN > τ̄_OUT.  Loop A's ordered-bracket form does not apply to a wave holding such a lane
    (it never enters loop B either).  128 u in one call: a wave of 64 ordered points, which at
    this η find no run and bisect until the bracket collapses (loop B's collapse exit,
    iterations 51-53), then a wave of 24 reversed points (collapse or iteration cap) with 40
    ordered ones."""
    t, G, _ = oracle.learn_logistic(1.0, 30.0)
    pdf = G * (1.0 - G) + 0.03 * np.exp(-((t - 1.0) / 1.0) ** 2)
    u = np.concatenate([sbr.julia_range("0.06", "0.24", 64), np.linspace(0.0047, 0.0199, 24),
                        sbr.julia_range("0.07", "0.23", 40)])
    g = engine.equilibrium_on_knots(t, G, 1.0, 9.0, 30.0, u, 0.5, 0.6, 0.01, paths=False, pdf=pdf)
    os = [oracle.equilibrium_paths_pdf(t, G, pdf, 9.0, 30.0, float(x), 0.5, 0.6, 0.01) for x in u]
    check_vector(g, os, "reversed")
    assert sum(o["tau_in_unc"] > o["tau_out_unc"] for o in os) >= 20
    collapse = sbr.STATUS["SBR_NO_RUN_COLLAPSE"]
    assert sum(o["tau_in_unc"] < o["tau_out_unc"] and (o["status"] & collapse) > 0 for o in os) >= 100


def test_fine_knots_past_the_lds_slab(engine, oracle):
    """Knots refined by midpoints past the LDS slab: the global-memory instantiation of the
    same two loops (a knots-in vector call, n_u = 64)."""
    t, G, _ = oracle.learn_logistic(1.0, 30.0)
    tm = np.empty(2 * len(t) - 1)
    tm[0::2], tm[1::2] = t, 0.5 * (t[:-1] + t[1:])
    Gm = np.empty_like(tm)
    Gm[0::2], Gm[1::2] = G, 0.5 * (G[:-1] + G[1:])
    info = engine.device_info()
    assert len(tm) > info["lds_knot_capacity"] // 2 or len(tm) > 4432
    u = sbr.julia_range("0.001", "0.2", 64)
    g = engine.equilibrium_on_knots(tm, Gm, 1.0, 15.0, 30.0, u, 0.5, 0.6, 0.01, paths=False)
    os = [oracle.equilibrium(tm, Gm, 1.0, 15.0, 30.0, float(x), 0.5, 0.6, 0.01) for x in u]
    check_vector(g, os, "refined")
    assert sum((o["status"] & RUN) > 0 for o in os) >= 16
