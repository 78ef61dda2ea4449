"""The continuum fixture (tests/golden/continuum.json, written by tools/make_continuum_golden.py) and
the comparison that tests/test_continuum.py (oracle) and tests/test_gpu_continuum.py (GPU) share
(not a test module).  json and numpy only: the model itself is tests/continuum.py.

A result is compared in class — on status bits and on the NaN / Inf sentinels — and in value, within
the project's knot-grid tolerances: 2e-5 on ξ, τ̄_IN, τ̄_OUT and 1e-5 on AW_max."""
import json
from pathlib import Path

import numpy as np

PATH = Path(__file__).resolve().parent / "golden" / "continuum.json"
TOL_TIME, TOL_AW = 2e-5, 1e-5
PARAMS = ("beta", "eta", "t_end", "u", "p", "kappa", "lam")
TIMES = (("xi", "xi"), ("tau_in", "tau_in_unc"), ("tau_out", "tau_out_unc"))
# status bits that say how the ODE was integrated, not how the point ended (include/sbr_status.h)
INFO_BITS = 0x0800  # SBR_STIFF_SWITCH
RUN, BELOW, COLLAPSE, MAXITER, FALSE_EQ = 0x3, 0x6, 0x8, 0x10, 0x20
STATUS_OF = {"run": (RUN,), "below": (BELOW,), "norun": (COLLAPSE, MAXITER), "false": (FALSE_EQ,),
             "invalid": (0x40,)}  # SBR_HETERO_INVALID


def _arr(v):
    return np.array([np.nan if x is None else x for x in v], float)


def load(text: str | None = None) -> dict:
    fix = json.loads(PATH.read_text() if text is None else text)
    assert fix["meta"]["tol_time"] == TOL_TIME and fix["meta"]["tol_aw"] == TOL_AW
    for name in ("points", "econ", "interest_econ"):
        lst = fix[name]
        for k in ("tau_in", "tau_out", "xi", "aw_max"):
            lst[k] = _arr(lst[k])
        lst["ok"] = np.array(lst.get("ok", [True] * len(lst["cls"])), bool)
    return fix


def compare(got: dict, cls, want: dict, t_end, ok=None, what: str = "") -> dict:
    """Assert that flat result arrays ``got`` (xi, tau_in_unc, tau_out_unc, aw_max, tol, status) are
    the continuum's: element n of class cls[n] with the values want[...][n]; t_end[n] is the
    point's horizon; elements with ok[n] false are ill-conditioned and not compared.  Returns the
    largest deviations {"time", "aw"}; prints them before it asserts."""
    n = len(cls)
    ok = np.ones(n, bool) if ok is None else np.asarray(ok, bool)
    st = np.asarray(got["status"]).reshape(-1) & ~np.uint32(INFO_BITS)
    g = {k: np.asarray(got[k], float).reshape(-1) for k in ("xi", "tau_in_unc", "tau_out_unc", "aw_max", "tol")}
    assert all(v.shape == (n,) for v in g.values()) and st.shape == (n,), what
    t_end = np.broadcast_to(np.asarray(t_end, float), (n,))
    cls = np.asarray(cls)
    bad = [(i, cls[i], hex(int(st[i]))) for i in np.flatnonzero(ok) if int(st[i]) not in STATUS_OF[cls[i]]]
    dev = {"time": 0.0, "aw": 0.0}
    for i in np.flatnonzero(ok):
        for k, a in TIMES:
            if want[k][i] == want[k][i]:
                dev["time"] = max(dev["time"], abs(g[a][i] - want[k][i]))
        if want["aw_max"][i] == want["aw_max"][i]:
            dev["aw"] = max(dev["aw"], abs(g["aw_max"][i] - want["aw_max"][i]))
    print(f"continuum {what}: {int(ok.sum())} of {n} compared, class mismatches {len(bad)}, "
          f"max |Δtime| {dev['time']:.3e}, max |ΔAW_max| {dev['aw']:.3e}")
    assert not bad, (what, bad[:8])
    for i in np.flatnonzero(ok):
        c, w = cls[i], f"{what}[{i}] {cls[i]}"
        if c == "run":
            assert np.isfinite([g[k][i] for k in g]).all(), w
        else:
            assert np.isnan(g["xi"][i]) and np.isnan(g["aw_max"][i]), w
            assert g["tol"][i] == (0.0 if c == "below" else np.inf), w
        if c == "below":  # the fallback is tspan[2] itself, not a crossing
            assert g["tau_in_unc"][i] == t_end[i] and g["tau_out_unc"][i] == t_end[i], w
        for k, a in TIMES:
            if want[k][i] == want[k][i]:
                assert abs(g[a][i] - want[k][i]) <= TOL_TIME, (w, k, g[a][i], want[k][i])
        if c == "run":
            assert abs(g["aw_max"][i] - want["aw_max"][i]) <= TOL_AW, (w, g["aw_max"][i], want["aw_max"][i])
    return dev


def grid_want(lst: dict) -> tuple:
    """(cls, want, t_end per element, ok) of a product grid, flat in its documented C order."""
    shape = lst["shape"]
    t_end = np.broadcast_to(np.asarray(lst["t_end"]).reshape(-1, *[1] * (len(shape) - 1)), shape).reshape(-1)
    return lst["cls"], lst, t_end, lst["ok"]


def hetero_got(res: dict, K: int) -> list:
    """A one-point hetero result as K flat results, one per group's buffers."""
    out = []
    for k in range(K):
        out.append(dict(xi=res["xi"].reshape(-1), aw_max=res["aw_max"].reshape(-1), tol=res["tol"].reshape(-1),
                        status=res["status"].reshape(-1), tau_in_unc=res["tau_in_unc"].reshape(-1, K)[:, k],
                        tau_out_unc=res["tau_out_unc"].reshape(-1, K)[:, k]))
    return out


def hetero_want(case: dict, k: int | None = None) -> dict:
    """The expected values of a hetero case for one group: the shared pair of an equal-rate case, or
    group k's own pair of an unequal-rate one."""
    pick = (lambda v: v) if k is None else (lambda v: v[k] if isinstance(v, list) else v)
    return {f: _arr([pick(case[f])]) for f in ("tau_in", "tau_out", "xi", "aw_max")}


# ---------------------------------------------------------------------------------------------
# the oracle on the fixture's lists (oracle/oracle.py passed in as O), flat in the lists' order
_KEYS = ("xi", "tau_in_unc", "tau_out_unc", "aw_max", "tol", "status")


def oracle_points(O, P: dict) -> dict:
    rows = [O.sweep_baseline([P["beta"][i]], P["eta"][i], P["t_end"][i], [P["u"][i]], P["p"][i], P["kappa"][i],
                             P["lam"][i], P["x0"]) for i in range(len(P["cls"]))]
    return {k: np.array([r[k][0, 0] for r in rows]) for k in _KEYS}


def oracle_grid(O, E: dict) -> dict:
    """One oracle sweep per (p, λ, [rate,] κ), stacked at (i, a, b, [d,] c, j)."""
    shape = tuple(E["shape"])
    out = {k: np.empty(shape, np.uint32 if k == "status" else float) for k in _KEYS}
    for a, p in enumerate(E["p"]):
        for b, lam in enumerate(E["lam"]):
            for c, kappa in enumerate(E["kappa"]):
                if "r" in E:
                    for d, (r, delta) in enumerate(zip(E["r"], E["delta"])):
                        res = O.sweep_interest(E["beta"], E["eta"], E["t_end"], E["u"], p, kappa, lam, r, delta,
                                               E["x0"])
                        for k in _KEYS:
                            out[k][:, a, b, d, c, :] = res[k]
                else:
                    res = O.sweep_baseline(E["beta"], E["eta"], E["t_end"], E["u"], p, kappa, lam, E["x0"])
                    for k in _KEYS:
                        out[k][:, a, b, c, :] = res[k]
    return out


def hetero_betas(case: dict) -> np.ndarray:
    return np.array([case["betas"]]) if "betas" in case else np.full((1, case["K"]), case["beta"])


def oracle_hetero(O, case: dict) -> dict:
    return O.sweep_hetero(hetero_betas(case), case["dist"], case["eta"], case["t_end"],
                          [case["u"]], case["p"], case["kappa"], case["lam"], case["x0"])


def hetero_compare(res: dict, case: dict, what: str) -> dict:
    """``compare`` on every group of a one-point result of an unequal-rate case; the largest deviations."""
    worst = {"time": 0.0, "aw": 0.0}
    for k, got in enumerate(hetero_got(res, case["K"])):
        d = compare(got, [case["cls"]], hetero_want(case, k), [case["t_end"]], what=f"{what} K={case['K']} group {k}")
        worst = {m: max(worst[m], d[m]) for m in worst}
    return worst


def oracle_maxima(O, fix: dict) -> dict:
    """{list: {"time", "aw"}}: the oracle's largest deviations from the fixture (asserting, as
    ``compare`` does, classes, sentinels and the full tolerances on the way)."""
    P, E, IE = fix["points"], fix["econ"], fix["interest_econ"]
    out = {"points": compare(oracle_points(O, P), P["cls"], P, P["t_end"], what="oracle points"),
           "econ": compare(oracle_grid(O, E), *grid_want(E), what="oracle econ"),
           "interest_econ": compare(oracle_grid(O, IE), *grid_want(IE), what="oracle interest_econ")}
    h = {"time": 0.0, "aw": 0.0}
    for n, case in enumerate(fix["hetero"]):
        for got in hetero_got(oracle_hetero(O, case), case["K"]):
            d = compare(got, [case["cls"]], hetero_want(case), [case["t_end"]], what=f"oracle hetero {n} K={case['K']}")
            h = {k: max(h[k], d[k]) for k in h}
    out["hetero"] = h
    h = {"time": 0.0, "aw": 0.0}
    for n, case in enumerate(fix["hetero_unequal"]):
        d = hetero_compare(oracle_hetero(O, case), case, f"oracle hetero_unequal {n}")
        h = {k: max(h[k], d[k]) for k in h}
    out["hetero_unequal"] = h
    return {k: {m: float(v) for m, v in d.items()} for k, d in out.items()}
