"""The HIP social-learning kernels against the continuum model of the fixed point: the recorded values
of tests/golden/continuum_social.json (tools/make_continuum_golden.py --social; the model is
tests/continuum_social.py, of which this file uses only the comparison), one sweep_social call per
group of 2 β columns × 4 u, away from p = 0.99, κ = 0.25, λ = 0.25, η = 30/0.9, x0 = 1e-4, tol = 1e-4,
under the built-in schedule and with one point per lane.  Every field, status and fp_iters must be the
recorded oracle's bit for bit, and the model's in class, fp_iters and value (2e-5 on times, 1e-5 on
AW_max).  Needs neither scipy nor an oracle run."""
import numpy as np
import pytest

import continuum_social as CS

pytestmark = pytest.mark.gpu

FIX = CS.load()
GROUPS = [pytest.param(n, id=f"{n}-{g['kind']}") for n, g in enumerate(FIX["groups"])]


@pytest.mark.parametrize("lanes", [False, True], ids=["default-schedule", "point-per-lane"])
@pytest.mark.parametrize("n", GROUPS)
def test_sweep_social(engine, n, lanes):
    g = FIX["groups"][n]
    a, kw = CS.group_args(g)
    if lanes:
        with engine.social_schedule(coop_max=0, waves=1):
            r = engine.sweep_social(*a, **kw)
            stats = engine.social_schedule_stats()
        assert stats[0] > 0, stats  # multi-point waves ran (a point that outgrows its lane may still move to a wave of its own)
    else:
        r = engine.sweep_social(*a, **kw)
    CS.assert_recorded(r, g, f"gpu group {n}")
    dev = CS.compare(r, g, f"gpu group {n} ({g['kind']})")
    assert dev["time"] <= FIX["meta"]["oracle"]["time"] and dev["aw"] <= FIX["meta"]["oracle"]["aw"]


@pytest.mark.parametrize("k", range(len(FIX["meta"]["path_points"])), ids=["run", "below", "cap"])
def test_forced_ode_against_its_closed_form(engine, k):
    """The returned iterate's (t, G, aw_old) must satisfy G = 1 − (1 − x0)·exp(−β ∫ aw_old), ∫ by the
    trapezoid rule on the returned knots: the kernel's forced ODE without any oracle.  The bound is twice
    the residual that the oracle's own knots show on the same point."""
    pp = FIX["meta"]["path_points"][k]
    g = FIX["groups"][pp["group"]]
    q, pt = CS.point_of(g, pp["point"]), g["points"][pp["point"]]
    r = engine.social_point_paths(q["beta"], q["eta"], q["u"], q["p"], q["kappa"], q["lam"], x0=q["x0"], tol=q["tol"],
                                  max_iter=q["max_iter"])
    assert r["fp_iters"] == pt["fp_iters"] and r["status"] == pt["oracle"]["status"]
    assert r["t"][0] == 0.0 and r["t"][-1] == q["eta"] and np.all(np.diff(r["t"]) > 0) and r["G"][0] == q["x0"]
    res = CS.forced_ode_residual(r["t"], r["G"], r["aw_old"], q["beta"], q["x0"])
    print(f"forced ODE residual {res:.3e} (oracle {pp['oracle_residual']:.3e})")
    assert res <= pp["bound"]
