"""The continuum model of a run (not a test module, not a conftest).

An independent float64 reference for the baseline, the interest-rate extension and the
heterogeneity extension with equal group rates, restated from the reference's source and not from
the oracle.  The learning curve is the logistic in closed form; everything else follows from it in
the limit of an infinitely fine knot grid:

    G(t) = 1/(1 + A e^{-βt}), A = (1 - x0)/x0,  g = βG(1 - G),  t½ = ln A / β
    I(τ) = ∫₀^τ e^{λs} g(s) ds
    h(τ) = p e^{λτ} g(τ) / (p I(τ) + (1 - p) I(η))            on [0, η]   (solver.jl:153-185)
    V'   = (h + δ)(1 - V) + max(u + rV - h, 0),  V(0) = (u + δ)/(r + δ)   (r > 0 only)
    f    = h - rV - u  (r > 0)   or   h - u

    buffers (optimal_buffer, solver.jl:211-264): f ≤ 0 everywhere → τ̄_IN = τ̄_OUT = t_end, class
    "below"; else τ̄_IN = the first up-crossing of f (0 if there is none), τ̄_OUT = the last
    down-crossing (η if there is none).
    ξ = G⁻¹(κ + G(τ̄_IN)); class "norun" if κ + G(τ̄_IN) ≥ 1 or ξ > τ̄_OUT; class "false" if
    g(ξ) < g(τ̄_IN) (the slope test, solver.jl:339-362); else class "run".
    AW_max (get_AW): d = ξ - τ̄_IN, t* = min(t½ + d/2, η), AW_max = G(t*) - [t* ≥ d] G(t* - d) + x0;
    heterogeneity with equal rates (heterogeneity_solver.jl:316-375): the same with min(…, t_end)
    and without + x0.

Heterogeneity with unequal group rates has no closed form: ``solve_hetero`` (below) integrates the
K-group learning ODE and finds ξ, the validity path and AW_max numerically.

I and V come from scipy's DOP853 with dense output at rtol 1e-13, the crossings from brentq after a
sign scan.  Each point also carries the conditioning verdict ``ok`` (see ``verdict``): a point is
ill-conditioned if a relative ±1e-4 on u or κ changes its class, or a relative ±1e-7 on u moves a
predicted time by more than a quarter of the time tolerance, or the bisection's acceptance window
10·eps(κ) is narrower than AW's float resolution at the root, or the hazard crosses u so flatly that
the reference's own trapezoid error (relative 5e-6) would move a time by half the tolerance.
"""
from __future__ import annotations

import functools
import math

import numpy as np
from scipy.integrate import solve_ivp
from scipy.optimize import brentq, minimize_scalar

TOL_TIME = 2e-5  # ξ, τ̄_IN, τ̄_OUT: the project's knot-grid sensitivity (tests/test_oracle_golden.py)
TOL_AW = 1e-5    # AW_max
CLASSES = ("run", "below", "norun", "false")
RTOL = 1e-13
N_SCAN = 4097
XTOL = 1e-14
H_REL = 5e-6  # relative error of the reference's trapezoid hazard on its own knots (see ``verdict``)


def G_of(t, beta, x0):
    A = (1.0 - x0) / x0
    return 1.0 / (1.0 + A * np.exp(-beta * np.asarray(t, float)))


def g_of(t, beta, x0):
    G = G_of(t, beta, x0)
    return beta * G * (1.0 - G)


def G_inv(y, beta, x0):
    A = (1.0 - x0) / x0
    return math.log(y * A / (1.0 - y)) / beta


class Hazard:
    """I(τ) on [0, η] for one (β, η, λ, x0), and the sign-scan grid: uniform on [0, η] plus a
    cluster of the same size across the logistic's rise at t½ (width ~ 1/β)."""

    def __init__(self, beta, eta, lam, x0):
        self.beta, self.eta, self.lam, self.x0 = beta, eta, lam, x0
        self.t_half = math.log((1.0 - x0) / x0) / beta
        self._atol_I = 1e-16 * beta * x0
        s = solve_ivp(self._dI, (0.0, eta), [0.0], method="DOP853", rtol=RTOL, atol=self._atol_I,
                      dense_output=True)
        assert s.success, s.message
        self._I = s.sol
        self.I_eta = float(s.y[0, -1])
        w = 40.0 / beta
        near = np.clip(self.t_half + np.linspace(-w, w, N_SCAN), 0.0, eta)
        self.scan = np.unique(np.concatenate([np.linspace(0.0, eta, N_SCAN), near]))

    def _dI(self, t, y):
        return [math.exp(self.lam * t) * float(g_of(t, self.beta, self.x0))]

    def eg(self, t):
        return np.exp(self.lam * np.asarray(t, float)) * g_of(t, self.beta, self.x0)

    def h_from_I(self, t, I, p):
        return p * self.eg(t) / (p * I + (1.0 - p) * self.I_eta)

    def h(self, t, p):
        return self.h_from_I(t, self._I(t)[0], p)

    def value_function(self, p, u, r, delta):
        """Dense (I, V) on [0, η]: I is carried along so that h needs no lookup inside the RHS."""
        def rhs(t, y):
            e = math.exp(self.lam * t) * float(g_of(t, self.beta, self.x0))
            h = p * e / (p * y[0] + (1.0 - p) * self.I_eta)
            return [e, (h + delta) * (1.0 - y[1]) + max(u + r * y[1] - h, 0.0)]

        s = solve_ivp(rhs, (0.0, self.eta), [0.0, (u + delta) / (r + delta)], method="DOP853", rtol=RTOL,
                      atol=[self._atol_I, 1e-15], dense_output=True)
        assert s.success, s.message
        return s.sol


@functools.lru_cache(maxsize=256)
def hazard(beta, eta, lam, x0) -> Hazard:
    return Hazard(beta, eta, lam, x0)


def _f_of(hz: Hazard, u, p, r, delta):
    """f(τ) (vectorised) whose sign decides the buffers."""
    if r > 0.0:
        sol = hz.value_function(p, u, r, delta)

        def f(t):
            y = sol(t)
            return hz.h_from_I(t, y[0], p) - r * y[1] - u
    else:
        def f(t):
            return hz.h(t, p) - u
    return f


def _buffers(hz: Hazard, f):
    """(τ̄_IN, τ̄_OUT) of optimal_buffer in the continuum, or None if f ≤ 0 on [0, η]."""
    s = hz.scan
    above = f(s) > 0.0
    if not above.any():
        return None
    up = np.flatnonzero(~above[:-1] & above[1:])
    dn = np.flatnonzero(above[:-1] & ~above[1:])
    fs = lambda x: float(f(x))  # noqa: E731
    tin = brentq(fs, s[up[0]], s[up[0] + 1], xtol=XTOL, rtol=8.9e-16) if len(up) else 0.0
    tout = brentq(fs, s[dn[-1]], s[dn[-1] + 1], xtol=XTOL, rtol=8.9e-16) if len(dn) else hz.eta
    return tin, tout


def _finish(hz: Hazard, buf, t_end, kappa, hetero):
    """Class, ξ and AW_max from the buffers: all closed form."""
    nan = float("nan")
    if buf is None:
        return dict(cls="below", tau_in=t_end, tau_out=t_end, xi=nan, aw_max=nan)
    tin, tout = buf
    beta, x0 = hz.beta, hz.x0
    out = dict(cls="norun", tau_in=tin, tau_out=tout, xi=nan, aw_max=nan)
    if not tin < tout:
        out["cls"] = "unmodelled"  # an up-crossing after the last down-crossing: not in the model
        return out
    y = kappa + float(G_of(tin, beta, x0))
    if y >= 1.0:
        return out
    xi = G_inv(y, beta, x0)
    if xi > tout:
        return out
    out["xi_root"] = xi
    # compute_ξ accepts |AW − κ| ≤ 10·eps(κ) (solver.jl:310); one float step of ξ moves AW by g(ξ)·eps(ξ)
    out["bisect_ratio"] = 0.0 if hetero else (float(g_of(xi, beta, x0)) * float(np.spacing(xi))
                                              / (10.0 * float(np.spacing(kappa))))
    if float(g_of(xi, beta, x0)) < float(g_of(tin, beta, x0)):
        out["cls"] = "false"
        return out
    d = xi - tin
    ts = min(hz.t_half + d / 2.0, t_end if hetero else hz.eta)
    aw = float(G_of(ts, beta, x0)) - (float(G_of(ts - d, beta, x0)) if ts >= d else 0.0)
    out.update(cls="run", xi=xi, aw_max=aw if hetero else aw + x0)
    return out


def _core(hz, t_end, u, p, kappa, r, delta, hetero, buf="compute"):
    if buf == "compute":
        buf = _buffers(hz, _f_of(hz, u, p, r, delta))
    res = _finish(hz, buf, t_end, kappa, hetero)
    res["_buf"] = buf
    return res


def verdict(hz, base, t_end, u, p, kappa, r, delta, hetero):
    """(ok, reason): the conditioning rule.  ok is False if a relative ±1e-4 on u or on κ changes
    the class, or a relative ±1e-7 on u moves τ̄_IN, τ̄_OUT or ξ by more than TOL_TIME / 4, or the
    root of the baseline bisection is not resolvable in floating point: the reference accepts ξ only
    where |AW(ξ) − κ| ≤ 10·eps(κ), and where one float step of ξ moves AW by more than that
    (g(ξ)·eps(ξ) > 10·eps(κ), half the acceptance window; small κ, mostly below 0.25) rounding
    decides between a run and the iteration cap, which no continuum predicts.  Last, a relative
    ±H_REL on u, the size of the reference's own discretisation error in h, must not move a time by
    more than TOL_TIME / 2: where the hazard crosses u at a log-slope below about 0.5 per unit
    time, the reference's knot grid and not the model decides the fifth digit."""
    if base["cls"] == "unmodelled":
        return False, "unmodelled"
    if base.get("bisect_ratio", 0.0) > 1.0:
        return False, f"bisection resolution {base['bisect_ratio']:.2f}"
    for s in (-1e-4, 1e-4):
        if _core(hz, t_end, u, p, kappa * (1.0 + s), r, delta, hetero, buf=base["_buf"])["cls"] != base["cls"]:
            return False, f"class changes at kappa*(1{s:+g})"
        if _core(hz, t_end, u * (1.0 + s), p, kappa, r, delta, hetero)["cls"] != base["cls"]:
            return False, f"class changes at u*(1{s:+g})"
    for s in (-1e-7, 1e-7):
        q = _core(hz, t_end, u * (1.0 + s), p, kappa, r, delta, hetero)
        if q["cls"] != base["cls"]:
            return False, f"class changes at u*(1{s:+g})"
        for k in ("tau_in", "tau_out", "xi"):
            if abs(q[k] - base[k]) > TOL_TIME / 4:  # NaN compares False: both NaN in one class
                return False, f"{k} moves {abs(q[k] - base[k]):.2e} at u*(1{s:+g})"
    # the reference's own hazard: trapezoid rule on ODE knots spaced βΔ ≈ 0.0085 through the rise,
    # a relative error of (βΔ)²/12 ≈ 6e-6 in I and h; it must not cost more than half the tolerance
    for s in (-H_REL, H_REL):
        q = _core(hz, t_end, u * (1.0 + s), p, kappa, r, delta, hetero)
        for k in ("tau_in", "tau_out", "xi"):
            if q["cls"] == base["cls"] and abs(q[k] - base[k]) > TOL_TIME / 2:
                return False, f"{k} moves {abs(q[k] - base[k]):.2e} at u*(1{s:+g})"
    return True, ""


def solve(beta, eta, t_end, u, p, kappa, lam, x0, r=0.0, delta=0.1, hetero=False, with_verdict=True) -> dict:
    """One point of the continuum model: cls in CLASSES (or "unmodelled"), tau_in, tau_out, xi, aw_max
    (NaN where the class has none) and, with ``with_verdict``, ok / reason."""
    args = [float(v) for v in (beta, eta, t_end, u, p, kappa, lam, x0, r, delta)]
    beta, eta, t_end, u, p, kappa, lam, x0, r, delta = args
    hz = hazard(beta, eta, lam, x0)
    res = _core(hz, t_end, u, p, kappa, r, delta, hetero)
    if with_verdict:
        res["ok"], res["reason"] = verdict(hz, res, t_end, u, p, kappa, r, delta, hetero)
    res.pop("_buf")
    res.pop("xi_root", None)
    res.pop("bisect_ratio", None)
    return res


def hetero_learning(betas, dist, t_end, x0, t_eval, method="DOP853", rtol=RTOL, atol=1e-18):
    """The K-group learning ODE dG_k = (1 - G_k) β_k Σ_j dist_j G_j, G_k(0) = x0, at t_eval: [n, K]."""
    betas, dist = np.asarray(betas, float), np.asarray(dist, float)

    def rhs(t, G):
        return (1.0 - G) * betas * float(dist @ G)

    kw = {}
    if method == "Radau":
        def jac(t, G):
            J = np.outer((1.0 - G) * betas, dist)
            J[np.diag_indices(len(G))] -= betas * float(dist @ G)
            return J
        kw["jac"] = jac
    s = solve_ivp(rhs, (0.0, float(t_end)), np.full(len(betas), float(x0)), method=method, rtol=rtol, atol=atol,
                  t_eval=np.asarray(t_eval, float), **kw)
    assert s.success, s.message
    return s.y.T


# ------------------------------------------------------------------------------------------------
# heterogeneity with unequal group rates (heterogeneity_learning.jl, heterogeneity_solver.jl)
HETERO_CLASSES = CLASSES + ("invalid",)


class HeteroLearning:
    """G_k and I_k(τ) = ∫₀^τ e^{λs} g_k of the K-group learning ODE in one DOP853 solve to t_end:

        G_k' = g_k = (1 − G_k) β_k ω,  ω = Σ_j dist_j G_j,  G_k(0) = x0
        h_k(τ) = p e^{λτ} g_k(τ) / (p I_k(τ) + (1 − p) I_k(η))     on [0, η]

    The sign-scan grids are uniform plus the integrator's own steps, which cluster where any group
    rises."""

    def __init__(self, betas, dist, eta, t_end, lam, x0):
        self.betas, self.dist = np.asarray(betas, float), np.asarray(dist, float)
        self.K, self.eta, self.t_end, self.lam, self.x0 = len(self.betas), eta, t_end, lam, x0
        K, b, d = self.K, self.betas, self.dist

        def rhs(t, y):
            g = (1.0 - y[:K]) * b * float(d @ y[:K])
            return np.concatenate([g, math.exp(lam * t) * g])

        atol = np.concatenate([np.full(K, 1e-18), 1e-16 * b * x0])
        s = solve_ivp(rhs, (0.0, t_end), np.concatenate([np.full(K, x0), np.zeros(K)]), method="DOP853", rtol=RTOL,
                      atol=atol, dense_output=True)
        assert s.success, s.message
        self.sol, self.steps = s.sol, s.t
        self.I_eta = s.sol(eta)[K:]
        self.scan = self.grid(eta, N_SCAN)

    def grid(self, hi, n):
        return np.unique(np.concatenate([np.linspace(0.0, hi, n), self.steps[self.steps <= hi]]))

    def G(self, k, t):
        return self.sol(t)[k]

    def g(self, k, t):
        Y = self.sol(t)[:self.K]
        return (1.0 - Y[k]) * self.betas[k] * (self.dist @ Y)

    def h(self, k, t, p):
        Y = self.sol(t)
        g = (1.0 - Y[k]) * self.betas[k] * (self.dist @ Y[:self.K])
        return p * np.exp(self.lam * np.asarray(t, float)) * g / (p * Y[self.K + k] + (1.0 - p) * self.I_eta[k])

    @functools.cached_property
    def h_over_p_scan(self):
        """[K, n]: e^{λτ} g_k and I_k on the scan grid, from which h_k follows for any p."""
        Y = self.sol(self.scan)
        g = (1.0 - Y[:self.K]) * self.betas[:, None] * (self.dist @ Y[:self.K])[None, :]
        return np.exp(self.lam * self.scan)[None, :] * g, Y[self.K:]


@functools.lru_cache(maxsize=64)
def _hetero_learning(betas, dist, eta, t_end, lam, x0) -> HeteroLearning:
    return HeteroLearning(betas, dist, eta, t_end, lam, x0)


def _hetero_buffers(L: HeteroLearning, u, p):
    """(τ̄_IN [K], τ̄_OUT [K], below [K]): each group's pair from the sign of h_k − u, as ``_buffers``;
    a group that never exceeds u gets t_end twice (optimal_buffer's fallback)."""
    s = L.scan
    eg, I = L.h_over_p_scan
    tin, tout, below = np.empty(L.K), np.empty(L.K), np.zeros(L.K, bool)
    for k in range(L.K):
        above = p * eg[k] / (p * I[k] + (1.0 - p) * L.I_eta[k]) - u > 0.0
        if not above.any():
            tin[k] = tout[k] = L.t_end
            below[k] = True
            continue
        up = np.flatnonzero(~above[:-1] & above[1:])
        dn = np.flatnonzero(above[:-1] & ~above[1:])
        fs = lambda x, k=k: float(L.h(k, x, p)) - u  # noqa: E731
        tin[k] = brentq(fs, s[up[0]], s[up[0] + 1], xtol=XTOL, rtol=8.9e-16) if len(up) else 0.0
        tout[k] = brentq(fs, s[dn[-1]], s[dn[-1] + 1], xtol=XTOL, rtol=8.9e-16) if len(dn) else L.eta
    return tin, tout, below


def _hetero_finish(L: HeteroLearning, buf, kappa, with_aw=True):
    """Class, ξ and AW_max from the groups' buffers.  Also the quantities the verdict needs: aw_cap =
    AW(max τ̄_OUT), slope, and path_gap, the smallest |path − κ| over the validity path's interior
    local extrema."""
    tin, tout, below = buf
    K, dist, nan = L.K, L.dist, float("nan")
    out = dict(cls="norun", tau_in=tin, tau_out=tout, xi=nan, aw_max=nan)
    if below.all():
        out["cls"] = "below"
        return out
    if not (tin[~below] < tout[~below]).all():
        out["cls"] = "unmodelled"  # an up-crossing after the last down-crossing: not in the model
        return out
    ks = np.arange(K)

    def AW(x):  # Σ dist_k [G_k(min(ξ, τ̄_OUT_k)) − G_k(min(ξ, τ̄_IN_k))], nondecreasing
        Y = L.sol(np.concatenate([np.minimum(x, tout), np.minimum(x, tin)]))[:K]
        return float(dist @ (Y[ks, ks] - Y[ks, K + ks]))

    hi = float(tout[~below].max())
    out["aw_cap"] = AW(hi)
    if out["aw_cap"] < kappa:
        return out
    xi = hi if out["aw_cap"] == kappa else brentq(lambda x: AW(x) - kappa, 0.0, hi, xtol=XTOL, rtol=8.9e-16)
    out["xi_root"] = xi
    Y = L.sol(np.concatenate([np.minimum(xi, tout), np.minimum(xi, tin)]))[:K]
    gY = (1.0 - Y) * L.betas[:, None] * (dist @ Y)[None, :]
    out["slope"] = float(dist @ (gY[ks, ks] - gY[ks, K + ks]))
    if out["slope"] < 0.0:
        out["cls"] = "false"
        return out
    # is_valid_equilibrium_hetero: the path on [0, ξ] must not go from above κ to not above κ
    tg = L.grid(xi, N_SCAN)
    path = np.zeros(len(tg))
    for k in range(K):
        path += dist[k] * (L.G(k, tg) - L.G(k, np.maximum(0.0, tg - max(0.0, xi - tin[k]))))
    above = path > kappa
    d = np.diff(path)
    ext = 1 + np.flatnonzero(d[:-1] * d[1:] < 0.0)
    out["path_gap"] = float(np.abs(path[ext] - kappa).min()) if len(ext) else float("inf")
    if (above[:-1] & ~above[1:]).any():
        out["cls"] = "invalid"
        return out
    out.update(cls="run", xi=xi)
    if not with_aw:
        return out
    # get_AW_hetero: the maximum over [0, t_end] of the summed shifted curves, without + x0
    tinc, toutc = np.minimum(tin, xi), np.minimum(tout, xi)

    def total(t):
        t = np.asarray(t, float)
        a = np.zeros_like(t)
        for k in range(K):
            so, si = t - xi + toutc[k], t - xi + tinc[k]
            if toutc[k] == tinc[k]:
                continue
            a += dist[k] * (np.where(so >= 0.0, L.G(k, np.maximum(so, 0.0)), 0.0)
                            - np.where(si >= 0.0, L.G(k, np.maximum(si, 0.0)), 0.0))
        return a

    tg = L.grid(L.t_end, 4 * N_SCAN)
    v = total(tg)
    i = int(np.argmax(v))
    m = minimize_scalar(lambda t: -float(total(np.array([t]))[0]), bounds=(tg[max(i - 1, 0)], tg[min(i + 1, len(tg) - 1)]),
                        method="bounded", options=dict(xatol=1e-11))
    out["aw_max"] = max(float(v[i]), -float(m.fun))
    out["aw_argmax"] = float(tg[i]) if float(v[i]) >= -float(m.fun) else float(m.x)
    return out


def _hetero_core(L, u, p, kappa, buf=None, with_aw=False):
    buf = _hetero_buffers(L, u, p) if buf is None else buf
    res = _hetero_finish(L, buf, kappa, with_aw)
    res["_buf"] = buf
    return res


def verdict_hetero(L, base, u, p, kappa):
    """``verdict``'s rules per group, and three of heterogeneity's own: AW(max τ̄_OUT) within a
    relative 1e-4 of κ (below that the reference's interval collapse and its iteration cap are not
    separable from a root), a slope that a relative 1e-4 on κ moves across 0, and a validity path
    whose interior extrema come within 1e-4·κ of κ."""
    if base["cls"] == "unmodelled":
        return False, "unmodelled"
    if "aw_cap" in base and abs(base["aw_cap"] - kappa) <= 1e-4 * kappa:
        return False, "AW(max tau_out) within 1e-4 of kappa"
    if base.get("path_gap", float("inf")) <= 1e-4 * kappa:
        return False, "path within 1e-4 kappa of kappa"
    for s in (-1e-4, 1e-4):
        q = _hetero_core(L, u, p, kappa * (1.0 + s), buf=base["_buf"])
        if q["cls"] != base["cls"]:
            return False, f"class changes at kappa*(1{s:+g})"
        if "slope" in base and "slope" in q and (q["slope"] < 0.0) != (base["slope"] < 0.0):
            return False, f"slope changes sign at kappa*(1{s:+g})"
        if _hetero_core(L, u * (1.0 + s), p, kappa)["cls"] != base["cls"]:
            return False, f"class changes at u*(1{s:+g})"
    for s, lim in ((-1e-7, TOL_TIME / 4), (1e-7, TOL_TIME / 4), (-H_REL, TOL_TIME / 2), (H_REL, TOL_TIME / 2)):
        q = _hetero_core(L, u * (1.0 + s), p, kappa)
        if q["cls"] != base["cls"]:
            if abs(s) == 1e-7:
                return False, f"class changes at u*(1{s:+g})"
            continue
        for k in ("tau_in", "tau_out", "xi"):
            move = float(np.max(np.abs(np.asarray(q[k]) - np.asarray(base[k]))))  # NaN: both NaN in one class
            if move > lim:
                return False, f"{k} moves {move:.2e} at u*(1{s:+g})"
    return True, ""


def solve_hetero(betas, dist, eta, t_end, u, p, kappa, lam, x0, with_verdict=True, internals=False) -> dict:
    """One point of the K-group continuum model: cls in HETERO_CLASSES (or "unmodelled"), tau_in and
    tau_out per group [K], xi, aw_max (NaN where the class has none) and, with ``with_verdict``,
    ok / reason; with ``internals`` also below [K], aw_cap, slope, path_gap and aw_argmax where the
    class has them."""
    eta, t_end, u, p, kappa, lam, x0 = (float(v) for v in (eta, t_end, u, p, kappa, lam, x0))
    L = _hetero_learning(tuple(float(b) for b in betas), tuple(float(d) for d in dist), eta, t_end, lam, x0)
    res = _hetero_core(L, u, p, kappa, with_aw=True)
    if with_verdict:
        res["ok"], res["reason"] = verdict_hetero(L, res, u, p, kappa)
    res["below"] = res.pop("_buf")[2]
    for k in () if internals else ("below", "xi_root", "aw_cap", "slope", "path_gap", "aw_argmax"):
        res.pop(k, None)
    return res
