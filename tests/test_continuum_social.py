"""The CPU oracle against the continuum model of the social-learning fixed point
(tests/continuum_social.py): an independent float64 restatement of solve_equilibrium_social_learning
on a fixed fine grid — the forced ODE in closed form, the hazard, the buffers, ξ, the sup-norm test,
the damping and the no-run branch — that shares no code and no reading of the reference with
oracle/sbr_oracle.c.  Its expected values are recorded per group (one sweep_social call each) in
tests/golden/continuum_social.json by tools/make_continuum_golden.py --social, over a box of
(β, η, x0, p, κ, λ, u, tol, max_iter) instead of the single triple p = 0.99, κ = 0.25, λ = 0.25.

Classes and fp_iters are asserted exactly, values within the project's tolerances, 2e-5 on ξ, τ̄_IN,
τ̄_OUT and 1e-5 on AW_max; for a predicted BoundsError ("throws") the iterate and the two status bits.
"""
import numpy as np
import pytest

pytest.importorskip("scipy")

import continuum_social as CS  # noqa: E402
import sbr  # noqa: E402

VALUES = ("tau_in", "tau_out", "xi", "aw_max")


@pytest.fixture(scope="module")
def fix():
    return CS.load()


@pytest.fixture(scope="module")
def results(oracle, fix):
    """The oracle on every group, once."""
    out = []
    for g in fix["groups"]:
        a, kw = CS.group_args(g)
        cmp = np.stack([sbr.julia_range(0.0, float(e), 1000) for e in g["eta"]])
        out.append(oracle.sweep_social(*a, cmp, **kw))
    return out


def test_the_fixture_is_what_the_issue_asks(fix):
    m, groups = fix["meta"], fix["groups"]
    pts = [pt for g in groups for pt in g["points"]]
    assert all(len(g["beta"]) == 2 and len(g["u"]) == 4 and len(g["points"]) == 8 for g in groups)
    assert sum(g["kind"] == "seeded" for g in groups) == 12 and groups[0]["kind"] == "script"
    assert {g["tol"] for g in groups if g["kind"] == "seeded"} == {1e-3, 1e-4, 1e-5}
    assert m["drawn"] == len(pts) and m["dropped"] == sum(not pt["ok"] for pt in pts)
    assert m["dropped"] <= 0.10 * m["drawn"]
    seen = [pt["cls"] for pt in pts if pt["ok"]]
    assert {c: seen.count(c) for c in set(seen)} == m["classes"]
    assert seen.count("throws") >= 4 and seen.count("below") >= 6 and seen.count("run") >= 40
    assert any(g["max_iter"] == 7 and pt["ok"] and pt["cls"] == "cap" for g in groups for pt in g["points"])
    assert any(g["max_iter"] == 600 and pt["ok"] and pt["cls"] == "past_eta" and pt["fp_iters"] == 501
               for g in groups for pt in g["points"])
    assert seen.count("false") >= 2 or m["false_statement"]
    # the model's own accuracy: the closed form against DOP853 and the grid cell halved
    assert m["closed_form_vs_dop853"] <= CS.TOL_AW / 100
    assert m["halved_cell"]["time"] <= CS.TOL_TIME / 100 and m["halved_cell"]["aw"] <= CS.TOL_AW / 100
    assert m["halved_cell"]["class_or_iterate_changed"] == 0
    assert 2 * m["stop_margin_measurement"]["smallest_agreeing_margin"] <= CS.STOP_MARGIN
    assert m["cells"] == CS.CELLS and m["stop_margin"] == CS.STOP_MARGIN


def test_oracle_equals_the_recorded_oracle(results, fix):
    for n, (r, g) in enumerate(zip(results, fix["groups"])):
        CS.assert_recorded(r, g, f"oracle group {n}")


def test_oracle_agrees_with_the_model(results, fix):
    worst = {"time": 0.0, "aw": 0.0}
    for n, (r, g) in enumerate(zip(results, fix["groups"])):
        d = CS.compare(r, g, f"oracle group {n} ({g['kind']})")
        worst = {k: max(worst[k], d[k]) for k in worst}
    print(f"social continuum: max |Δtime| {worst['time']:.3e}, max |ΔAW_max| {worst['aw']:.3e}")
    assert worst == fix["meta"]["oracle"]  # the maxima the fixture and DESIGN.md §2 state


@pytest.fixture(scope="module")
def self_points(fix):
    out = []
    for gi, i in fix["meta"]["self_points"]:
        g = fix["groups"][gi]
        out.append((CS.point_of(g, i), g["points"][i]))
    return out


def test_model_reproduces_its_recorded_values(self_points):
    """Three points (a run, a below, a cap): guards tests/continuum_social.py against drift."""
    assert [pt["cls"] for _, pt in self_points] == ["run", "below", "cap"]
    for q, pt in self_points:
        r = CS.solve_social(**q)
        assert (r["cls"], r["inner"], r["fp_iters"]) == (pt["cls"], pt["inner"], pt["fp_iters"])
        for k in VALUES:
            if pt[k] is None:
                assert r[k] != r[k], k
            else:
                assert abs(r[k] - pt[k]) <= 1e-9, (k, r[k], pt[k])


def test_model_at_half_the_cell(self_points):
    """The same three points at CELLS and at 2·CELLS cells: a hundredth of the comparison tolerances
    (the model is second order in the cell once the jump cells are integrated exactly: the script point's
    τ̄_IN moves 6.3e-9, 1.6e-9, 3.9e-10 from 200k to 1.6M cells)."""
    for q, pt in self_points:
        r = CS.solve_social(**q, cells=2 * CS.CELLS)
        assert (r["cls"], r["fp_iters"]) == (pt["cls"], pt["fp_iters"])
        for k in VALUES:
            if pt[k] is not None:
                d = abs(r[k] - pt[k])
                print(f"{pt['cls']} {k}: {d:.2e}")
                assert d <= (CS.TOL_AW if k == "aw_max" else CS.TOL_TIME) / 100, (k, d)
