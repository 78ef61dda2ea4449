"""The HIP kernels against the continuum model of the run: the recorded expected values of
tests/golden/continuum.json (tools/make_continuum_golden.py; the model is tests/continuum.py, which
this file does not need), away from the figures' p = 0.5, κ = 0.6, λ = 0.01, x0 = 1e-4 and without
the oracle.  Classes are asserted on status bits and on the NaN / Inf sentinels, values within 2e-5
(ξ, τ̄_IN, τ̄_OUT) and 1e-5 (AW_max); the product sweeps are compared element by element at their
documented index, which pins the layout too.  The kernels are bit-identical to the oracle, so
their largest deviations must be the ones the fixture records for the oracle."""
import numpy as np
import pytest

import continuum_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    return CC.load()


def test_solve_points(engine, fix):
    P = fix["points"]
    assert len(P["cls"]) == 96  # one full learning wave and a partial one
    r = engine.solve_points(*[np.array(P[k]) for k in ("beta", "u", "eta", "t_end", "p", "kappa", "lam")], x0=P["x0"])
    dev = CC.compare(r, P["cls"], P, P["t_end"], what="gpu solve_points")
    assert dev == fix["meta"]["oracle"]["points"]


def test_sweep_econ_at_its_documented_index(engine, fix):
    E = fix["econ"]
    r = engine.sweep_econ(*[np.array(E[k]) for k in ("beta", "eta", "t_end", "u", "p", "kappa", "lam")], x0=E["x0"])
    assert r["xi"].shape == tuple(E["shape"])  # (i, a, b, c, j) = (β, p, λ, κ, u)
    dev = CC.compare(r, *CC.grid_want(E), what="gpu sweep_econ")
    assert dev == fix["meta"]["oracle"]["econ"]


def test_sweep_interest_econ_at_its_documented_index(engine, fix):
    E = fix["interest_econ"]
    r = engine.sweep_interest_econ(*[np.array(E[k]) for k in ("beta", "eta", "t_end", "u", "p", "kappa", "lam", "r",
                                                             "delta")], x0=E["x0"])
    assert r["xi"].shape == tuple(E["shape"])  # (i, a, b, d, c, j) = (β, p, λ, rate, κ, u)
    assert (r["rk_steps"][:, :, :, 0] == 0).all() and (r["rk_steps"][:, :, :, 1] > 0).all()  # r = 0, r > 0
    dev = CC.compare(r, *CC.grid_want(E), what="gpu sweep_interest_econ")
    assert dev == fix["meta"]["oracle"]["interest_econ"]


def test_sweep_interest_on_one_line(engine, fix):
    E = fix["interest_econ"]
    i, a, b, d, c = 1, 0, 0, 1, 1
    sl = np.arange(len(E["cls"])).reshape(E["shape"])[i, a, b, d, c, :]
    cls = [E["cls"][n] for n in sl]
    assert E["r"][d] > 0 and {"run", "norun", "below"} <= set(cls) and E["ok"][sl].all()
    r = engine.sweep_interest(E["beta"][i:i + 1], E["eta"][i], E["t_end"][i], np.array(E["u"]), E["p"][a],
                              E["kappa"][c], E["lam"][b], E["r"][d], E["delta"][d], x0=E["x0"])
    want = {k: E[k][sl] for k in ("tau_in", "tau_out", "xi", "aw_max")}
    dev = CC.compare(r, cls, want, E["t_end"][i], what="gpu sweep_interest")
    assert dev["time"] <= CC.TOL_TIME / 2 and dev["aw"] <= CC.TOL_AW / 2


@pytest.mark.parametrize("wide", [False, True], ids=["specialised", "group-looped"])
def test_sweep_hetero_with_equal_rates(engine, fix, wide):
    """K groups at one rate and unequal shares are the baseline model, with AW_max over the learning
    grid up to t_end and without + G(0); every group's buffers must be the continuum's pair.  Without
    the flag K = 1, 2, 3, 8 run the specialised kernels and 5, 12, 16 the group-looped one; with
    SBR_FLAG_HETERO_WIDE every K runs the group-looped one."""
    worst = {"time": 0.0, "aw": 0.0}
    assert {c["K"] for c in fix["hetero"]} == {1, 2, 3, 5, 8, 12, 16}
    for n, case in enumerate(fix["hetero"]):
        K = case["K"]
        r = engine.sweep_hetero(np.full((1, K), case["beta"]), np.array(case["dist"]), case["eta"], case["t_end"],
                                [case["u"]], case["p"], case["kappa"], case["lam"], x0=case["x0"], wide=wide)
        for got in CC.hetero_got(r, K):
            d = CC.compare(got, [case["cls"]], CC.hetero_want(case), [case["t_end"]], what=f"gpu hetero {n} K={K}")
            worst = {k: max(worst[k], d[k]) for k in worst}
    print(f"gpu hetero wide={wide}: max |Δtime| {worst['time']:.3e}, max |ΔAW_max| {worst['aw']:.3e}")
    assert worst == fix["meta"]["oracle"]["hetero"]


@pytest.mark.parametrize("wide", [False, True], ids=["specialised", "group-looped"])
def test_sweep_hetero_with_unequal_rates(engine, fix, wide):
    """Genuinely different group rates: every group's own buffers, ξ, AW_max, the class and the
    sentinels against the K-group continuum model (tests/continuum.py, solve_hetero), one 1 × 1
    sweep per case.  Without the flag K = 2, 3, 8 run the specialised kernels and 5, 12, 16 the
    group-looped one."""
    worst = {"time": 0.0, "aw": 0.0}
    H = fix["hetero_unequal"]
    assert {c["K"] for c in H} == {2, 3, 5, 8, 12, 16} and sum(c["mixed"] for c in H) >= 6
    for n, case in enumerate(H):
        r = engine.sweep_hetero(CC.hetero_betas(case), np.array(case["dist"]), case["eta"], case["t_end"], [case["u"]],
                                case["p"], case["kappa"], case["lam"], x0=case["x0"], wide=wide)
        d = CC.hetero_compare(r, case, f"gpu hetero_unequal {n}")
        worst = {k: max(worst[k], d[k]) for k in worst}
    print(f"gpu hetero_unequal wide={wide}: max |Δtime| {worst['time']:.3e}, max |ΔAW_max| {worst['aw']:.3e}")
    assert worst == fix["meta"]["oracle"]["hetero_unequal"]
