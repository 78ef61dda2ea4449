#!/usr/bin/env python3
"""Write tests/golden/continuum.json: seeded parameter lists with the continuum model's expected
values (tests/continuum.py), for tests/test_continuum.py (oracle) and tests/test_gpu_continuum.py.

    python tools/make_continuum_golden.py            # rewrites the fixture (about six minutes)
    python tools/make_continuum_golden.py --check    # regenerates and compares with the committed file
    python tools/make_continuum_golden.py --social   # tests/golden/continuum_social.json: the social-learning fixed
                                                     # point (tests/continuum_social.py), about ten minutes on 8 cores;
                                                     # with --check it compares, with --margin it measures the stopping
                                                     # margin again on 200 random points

Needs numpy, scipy and mpmath.  The lists and their expected values are the model alone; the built
oracle is run on them afterwards only to record its largest deviations (meta.oracle), which must
stay within half of each tolerance.

The box (the issue's, narrowed twice for a stated reason):
  β log-uniform [1, 60] (asked: from 0.3; the reference's trapezoid / linear-interpolation error in
  a time scales like 1e-5/β and passes half the tolerance below β ≈ 1), η [3, 30], t_end [η, 2η],
  p [.05, .95], κ [.1, .95], λ log-uniform [.002, .5], u log-uniform [.005, 2], x0 log-uniform
  [1e-6, 1e-2], and G(η) ≥ 0.1 (where learning has not started by η the reference's knots, spaced by
  its absolute tolerance, are ten times coarser).
The list hetero_unequal (C.solve_hetero, K groups at different rates) has ranges of its own (UNEQUAL)
and one oracle-informed step, the t_end redraw on the reference's rounding BoundsError
(make_hetero_unequal).
A drawn point that fails the conditioning verdict is dropped (lists) or masked (grids: ok = false);
at most 10 % of all drawn points may be, or the tool fails.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import math
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "tests"), str(REPO / "oracle")]
import continuum as C  # noqa: E402
import continuum_cases as CC  # noqa: E402

OUT = REPO / "tests" / "golden" / "continuum.json"
BOX = dict(beta=(1.0, 60.0), eta=(3.0, 30.0), t_end_over_eta=(1.0, 2.0), p=(0.05, 0.95), kappa=(0.1, 0.95),
           lam=(0.002, 0.5), u=(0.005, 2.0), x0=(1e-6, 1e-2), G_eta_min=0.1)
SEEDS = dict(points=101, false_eq=102, econ=103, interest_econ=104, hetero=105)
SEED_HETERO_UNEQUAL = 106
N_POINTS, N_FALSE = 96, 3
HETERO_K = (1, 2, 3, 5, 8, 12, 16)
UNEQUAL_K = (2, 3, 5, 8, 12, 16)
N_UNEQUAL, N_UNEQUAL_MIXED, N_UNEQUAL_FALSE = 48, 4, 2
UNEQUAL = dict(mean_beta=(1.0, 20.0), spread=(1.5, 30.0), eta_over_rise=(1.2, 4.0), t_end_over_eta=(1.2, 2.0),
               u_high=(0.1, 4.0), need=dict(mixed=6, norun=2, below=2, false=1))
OOB_STATUS, MAX_REDRAWS, REDRAW = 0x80, 3, 1.0 + 2.0 ** -30
MP_DIGITS_HETERO = 30
MP_DIGITS = 45
FIELDS = ("tau_in", "tau_out", "xi", "aw_max")


def logu(rng, lo, hi):
    return float(math.exp(rng.uniform(math.log(lo), math.log(hi))))


def draw_x0(rng):
    return logu(rng, *BOX["x0"])


def draw_column(rng, x0):
    """(β, η, t_end) inside the box, G(η) ≥ G_eta_min."""
    while True:
        beta, eta = logu(rng, *BOX["beta"]), float(rng.uniform(*BOX["eta"]))
        t_end = eta * float(rng.uniform(*BOX["t_end_over_eta"]))
        if float(C.G_of(eta, beta, x0)) >= BOX["G_eta_min"]:
            return beta, eta, t_end


def strata(rng, lo, hi, n, log=False):
    """An axis of n increasing values: one draw from each of n equal parts of [lo, hi]."""
    if log:
        return [math.exp(v) for v in strata(rng, math.log(lo), math.log(hi), n)]
    w = (hi - lo) / n
    return [float(rng.uniform(lo + k * w, lo + (k + 1) * w)) for k in range(n)]


def draw_econ(rng, kappa=None):
    return dict(u=logu(rng, *BOX["u"]), p=float(rng.uniform(*BOX["p"])),
                kappa=float(rng.uniform(*(kappa or BOX["kappa"]))), lam=logu(rng, *BOX["lam"]))


def jnum(x):
    x = float(x)
    return None if x != x else x


class Tally:
    def __init__(self):
        self.drawn = self.dropped = 0
        self.reasons = {}

    def add(self, res):
        self.drawn += 1
        if not res["ok"]:
            self.dropped += 1
            key = res["reason"].split(" at ")[0].split(" moves")[0].rstrip(" .0123456789")
            self.reasons[key] = self.reasons.get(key, 0) + 1
        return res["ok"]


def make_points(tally):
    rng = np.random.default_rng(SEEDS["points"])
    x0 = draw_x0(rng)
    pts, exp = [], []
    while len(pts) < N_POINTS - N_FALSE:
        beta, eta, t_end = draw_column(rng, x0)
        q = dict(beta=beta, eta=eta, t_end=t_end, **draw_econ(rng))
        res = C.solve(**q, x0=x0)
        if tally.add(res):
            pts.append(q)
            exp.append(res)
    # false equilibria need G(τ̄_IN) > (1 − κ)/2: a search of its own at κ ≥ 0.8; only its well-conditioned
    # false equilibria are kept, and the draws it throws away for their class are not conditioning drops
    rng = np.random.default_rng(SEEDS["false_eq"])
    searched = 0
    while len(pts) < N_POINTS:
        beta, eta, t_end = draw_column(rng, x0)
        q = dict(beta=beta, eta=eta, t_end=t_end, **draw_econ(rng, kappa=(0.8, BOX["kappa"][1])))
        searched += 1
        res = C.solve(**q, x0=x0, with_verdict=False)
        if res["cls"] != "false":
            continue
        res = C.solve(**q, x0=x0)
        if tally.add(res):
            pts.append(q)
            exp.append(res)
    out = dict(x0=x0, false_eq_search_draws=searched)
    for k in ("beta", "eta", "t_end", "u", "p", "kappa", "lam"):
        out[k] = [q[k] for q in pts]
    out["cls"] = [e["cls"] for e in exp]
    for k in FIELDS:
        out[k] = [jnum(e[k]) for e in exp]
    return out


def make_grid(tally, seed, n_beta, n_p, n_lam, n_kappa, n_u, rates=None):
    """A product grid in sbr_sweep_econ's layout (i, a, b, c, j) or, with rate pairs, in
    sbr_sweep_interest_econ's (i, a, b, d, c, j); flat C-order lists."""
    rng = np.random.default_rng(seed)
    x0 = draw_x0(rng)
    cols = [draw_column(rng, x0) for _ in range(n_beta)]
    ax = dict(p=strata(rng, *BOX["p"], n_p), lam=strata(rng, *BOX["lam"], n_lam, log=True),
              kappa=strata(rng, *BOX["kappa"], n_kappa), u=strata(rng, *BOX["u"], n_u, log=True))
    out = dict(x0=x0, beta=[c[0] for c in cols], eta=[c[1] for c in cols], t_end=[c[2] for c in cols], **ax)
    if rates is not None:
        out["r"], out["delta"] = [r for r, _ in rates], [d for _, d in rates]
    out["cls"], out["ok"] = [], []
    for k in FIELDS:
        out[k] = []
    for beta, eta, t_end in cols:
        for p in ax["p"]:
            for lam in ax["lam"]:
                for r, delta in (rates or [(0.0, 0.1)]):
                    for kappa in ax["kappa"]:
                        for u in ax["u"]:
                            res = C.solve(beta, eta, t_end, u, p, kappa, lam, x0, r, delta)
                            out["ok"].append(bool(tally.add(res)))
                            out["cls"].append(res["cls"])
                            for k in FIELDS:
                                out[k].append(jnum(res[k]))
    shape = [n_beta, n_p, n_lam] + ([len(rates)] if rates else []) + [n_kappa, n_u]
    out["shape"] = shape
    assert len(out["cls"]) == int(np.prod(shape))
    return out


def make_hetero(tally):
    """Equal group rates: K groups with one β and random unequal shares collapse to the baseline
    model (ω = G because the shares sum to 1), with AW_max over the learning grid up to t_end and
    without + G(0)."""
    rng = np.random.default_rng(SEEDS["hetero"])
    cases = []
    while len(cases) < 3 * len(HETERO_K):
        K = HETERO_K[len(cases) % len(HETERO_K)]
        x0 = draw_x0(rng)
        beta, eta, t_end = draw_column(rng, x0)
        d = rng.random(K) + 0.2
        d /= d.sum()
        d[-1] = 1.0 - d[:-1].sum()
        q = dict(beta=beta, eta=eta, t_end=t_end, **draw_econ(rng))
        res = C.solve(**q, x0=x0, hetero=True)
        if tally.add(res):
            cases.append(dict(K=K, dist=[float(v) for v in d], x0=x0, **q, cls=res["cls"],
                              **{k: jnum(res[k]) for k in FIELDS}))
    return cases


def draw_unequal(rng, n, kappa=None, high_u=None):
    """Case n's parameters: K cycles; rates log-uniform around a (geometric) mean with a spread ratio, shuffled;
    unequal shares; η a multiple of the mean-rate logistic's rise time; every third case at high u."""
    K = UNEQUAL_K[n % len(UNEQUAL_K)]
    x0 = draw_x0(rng)
    while True:  # every group's rate inside the box's β range, for the reason the box gives for its floor
        mean, spread = logu(rng, *UNEQUAL["mean_beta"]), float(rng.uniform(*UNEQUAL["spread"]))
        x = rng.uniform(-0.5, 0.5, K)
        x[0], x[1] = -0.5, 0.5  # the slowest and the fastest group: max β / min β is the spread ratio itself
        betas = mean * spread ** x
        if BOX["beta"][0] <= betas.min() and betas.max() <= BOX["beta"][1]:
            break
    rng.shuffle(betas)
    d = rng.random(K) + 0.2
    d /= d.sum()
    d[-1] = 1.0 - d[:-1].sum()
    eta = float(rng.uniform(*UNEQUAL["eta_over_rise"])) * math.log((1.0 - x0) / x0) / float(d @ betas)
    t_end = eta * float(rng.uniform(*UNEQUAL["t_end_over_eta"]))
    econ = draw_econ(rng, kappa)
    u_high = logu(rng, *UNEQUAL["u_high"])
    if n % 3 == 2 if high_u is None else high_u:
        econ["u"] = u_high
    return dict(K=K, betas=[float(b) for b in betas], dist=[float(v) for v in d], x0=x0, eta=eta, t_end=t_end, **econ)


def make_hetero_unequal(O):
    """Unequal group rates (C.solve_hetero).  The model alone fixes each case and its verdict; the
    oracle is then asked one thing: whether a predicted run ends in SBR_OOB, the reference's
    BoundsError where (t_grid[end] − ξ) + ξ rounds one ulp above t_end.  Such a case is evaluated
    again with t_end·(1 + 2⁻³⁰), at most three times, and dropped after that."""
    rng = np.random.default_rng(SEED_HETERO_UNEQUAL)
    tally = Tally()
    cases, n_draw, oob_dropped, redraws, searched = [], 0, 0, 0, dict(mixed=0, false=0)
    while len(cases) < N_UNEQUAL:
        model = lambda q, **kw: C.solve_hetero(**{k: v for k, v in q.items() if k != "K"}, **kw)  # noqa: E731
        if len(cases) < N_UNEQUAL - N_UNEQUAL_MIXED - N_UNEQUAL_FALSE:
            q = draw_unequal(rng, n_draw)
        elif len(cases) < N_UNEQUAL - N_UNEQUAL_FALSE:
            # groups below u beside groups with a window, and false equilibria, are rare in the box: as for
            # `points`, searches of their own, whose draws of another kind are not conditioning drops
            q = draw_unequal(rng, n_draw, high_u=True)
            searched["mixed"] += 1
            below = model(q, with_verdict=False, internals=True)["below"]
            if not below.any() or below.all():
                n_draw += 1
                continue
        else:
            q = draw_unequal(rng, n_draw, kappa=(0.8, BOX["kappa"][1]), high_u=False)
            searched["false"] += 1
            if model(q, with_verdict=False)["cls"] != "false":
                n_draw += 1
                continue
        n_draw += 1
        for redraw in range(MAX_REDRAWS + 1):
            res = model(q, internals=True)
            if not res["ok"] or res["cls"] != "run":
                break
            st = int(O.sweep_hetero(np.array([q["betas"]]), q["dist"], q["eta"], q["t_end"], [q["u"]], q["p"],
                                    q["kappa"], q["lam"], q["x0"])["status"][0, 0]) & ~CC.INFO_BITS
            if st != OOB_STATUS:
                break
            if redraw < MAX_REDRAWS:
                q["t_end"] *= REDRAW
        else:
            res = dict(res, ok=False, reason="BoundsError after redraws")
            oob_dropped += 1
        if not tally.add(res):
            continue
        redraws += redraw
        assert res["cls"] in C.HETERO_CLASSES
        mixed = bool(res["below"].any() and not res["below"].all())
        cases.append(dict(**q, cls=res["cls"], mixed=mixed, t_end_redraws=redraw,
                          tau_in=[float(v) for v in res["tau_in"]], tau_out=[float(v) for v in res["tau_out"]],
                          xi=jnum(res["xi"]), aw_max=jnum(res["aw_max"])))
    classes = {}
    for c in cases:
        classes[c["cls"]] = classes.get(c["cls"], 0) + 1
    n_mixed = sum(c["mixed"] for c in cases)
    need = UNEQUAL["need"]
    assert n_mixed >= need["mixed"] and all(classes.get(k, 0) >= need[k] for k in ("norun", "below", "false")), (
        n_mixed, classes)
    meta = dict(seed=SEED_HETERO_UNEQUAL, ranges={k: list(v) if isinstance(v, tuple) else v for k, v in UNEQUAL.items()},
                drawn=tally.drawn, dropped=tally.dropped, dropped_reasons=tally.reasons, oob_dropped=oob_dropped,
                search_draws=searched, t_end_redraws=redraws, classes=classes, mixed=n_mixed)
    return cases, meta


def mp_hetero(case):
    """One K = 2 unequal-rate run with mpmath: Taylor integration (odefun) of (G_k, I_k) at
    MP_DIGITS_HETERO digits; the crossings, ξ, the validity path and AW_max's hump are found by mpmath
    scans of its own; returns the largest differences from the float64 model in a time and in AW_max."""
    import mpmath as mp

    mp.mp.dps = MP_DIGITS_HETERO
    M = mp.mpf
    K = case["K"]
    b, d = [M(v) for v in case["betas"]], [M(v) for v in case["dist"]]
    eta, t_end, u, p, kappa, lam, x0 = (M(case[k]) for k in ("eta", "t_end", "u", "p", "kappa", "lam", "x0"))

    def F(t, y):
        om = mp.fsum(d[j] * y[j] for j in range(K))
        g = [(1 - y[k]) * b[k] * om for k in range(K)]
        e = mp.exp(lam * t)
        return g + [e * v for v in g]

    sol = mp.odefun(F, 0, [x0] * K + [M(0)] * K)
    sol(t_end)
    I_eta = sol(eta)[K:]

    def h(k, t):
        y = sol(t)
        return p * F(t, y)[K + k] / (p * y[K + k] + (1 - p) * I_eta[k])

    # mpmath's own choices: a coarse scan of h_k − u names the first up-crossing and the last down-crossing,
    # AW(ξ) = κ is bracketed by [0, max τ̄_OUT], and a coarse scan of AW_total names the hump; the float64
    # model is only compared at the end
    N = 400
    root = lambda f, lo, hi: mp.findroot(f, (lo, hi), solver="illinois", tol=M(10) ** -50, maxsteps=300,  # noqa: E731
                                         verify=False)
    tin, tout = [], []
    for k in range(K):
        ts = [eta * j / N for j in range(N + 1)]
        above = [h(k, t) - u > 0 for t in ts]
        assert any(above)
        ups = [j for j in range(N) if not above[j] and above[j + 1]]
        dns = [j for j in range(N) if above[j] and not above[j + 1]]
        tin.append(root(lambda t: h(k, t) - u, ts[ups[0]], ts[ups[0] + 1]) if ups else M(0))
        tout.append(root(lambda t: h(k, t) - u, ts[dns[-1]], ts[dns[-1] + 1]) if dns else eta)

    def AW(x):
        return mp.fsum(d[k] * (sol(min(x, tout[k]))[k] - sol(min(x, tin[k]))[k]) for k in range(K))

    assert AW(max(tout)) > kappa
    xi = root(lambda x: AW(x) - kappa, M(0), max(tout))
    slope = mp.fsum(d[k] * (F(min(xi, tout[k]), sol(min(xi, tout[k])))[k] - F(min(xi, tin[k]), sol(min(xi, tin[k])))[k])
                    for k in range(K))
    assert slope >= 0
    tI = [max(0, xi - tin[k]) for k in range(K)]
    path = [mp.fsum(d[k] * (sol(t)[k] - sol(max(0, t - tI[k]))[k]) for k in range(K)) for t in (xi * j / N for j in range(N))]
    assert not any(path[j] > kappa and not path[j + 1] > kappa for j in range(N - 1))

    def total(t):
        a = M(0)
        for k in range(K):
            so, si = t - xi + min(tout[k], xi), t - xi + min(tin[k], xi)
            a += d[k] * ((sol(max(so, 0))[k] if so >= 0 else 0) - (sol(max(si, 0))[k] if si >= 0 else 0))
        return a

    ts = [t_end * j / N for j in range(N + 1)]
    v = [total(t) for t in ts]
    j = max(range(N + 1), key=lambda q: v[q])
    lo, hi = ts[max(j - 1, 0)], ts[min(j + 1, N)]
    for _ in range(120):  # ternary search of the hump's cell pair: 1e-20 in t
        a, b = lo + (hi - lo) / 3, hi - (hi - lo) / 3
        lo, hi = (a, hi) if total(a) < total(b) else (lo, b)
    aw = max(v[j], total((lo + hi) / 2))
    want = C.solve_hetero(**{k: v for k, v in case.items() if k in ("betas", "dist", "eta", "t_end", "u", "p", "kappa",
                                                                    "lam", "x0")}, with_verdict=False)
    assert want["cls"] == "run"
    dt = max(abs(float(a) - float(v)) for a, v in zip(tin + tout + [xi], [*want["tau_in"], *want["tau_out"], want["xi"]]))
    return dt, abs(float(aw) - float(want["aw_max"]))


# ------------------------------------------------------------------------------------------------
# the same model at MP_DIGITS digits: quadrature for I, bracketed root finding for the crossings,
# and the value function in closed form between its switch points
def mp_point(q, x0, r=0.0, delta=0.1, hetero=False):
    import mpmath as mp

    mp.mp.dps = MP_DIGITS
    M = mp.mpf
    beta, eta, t_end, u, p, kappa, lam = (M(q[k]) for k in ("beta", "eta", "t_end", "u", "p", "kappa", "lam"))
    x0m, rm, dm = M(x0), M(r), M(delta)
    A = (1 - x0m) / x0m
    G = lambda t: 1 / (1 + A * mp.exp(-beta * t))  # noqa: E731
    g = lambda t: beta * G(t) * (1 - G(t))  # noqa: E731
    eg = lambda t: mp.exp(lam * t) * g(t)  # noqa: E731
    th = mp.log(A) / beta

    def quad(fn, a, b):
        if a == b:
            return M(0)
        cuts = sorted({a, b, *[c for c in (th - 10 / beta, th, th + 10 / beta) if a < c < b]})
        return mp.quad(fn, cuts)

    I_eta = quad(eg, M(0), eta)
    D = lambda I: p * I + (1 - p) * I_eta  # noqa: E731
    # the float64 model's sign scan only names the brackets; every value below is mpmath's own
    hz = C.hazard(float(q["beta"]), float(q["eta"]), float(q["lam"]), float(x0))
    f64 = C._f_of(hz, float(q["u"]), float(q["p"]), float(r), float(delta))
    s = hz.scan
    above = f64(s) > 0.0
    flips = np.flatnonzero(above[:-1] != above[1:])
    c = dm - rm
    # state at the left end a of the current piece: I(a), V(a)
    a, Ia, Va = M(0), M(0), (u + dm) / (rm + dm)
    ups, downs = [], []

    def f_at(t, a, Ia, Va, in_B):
        """f = h − rV − u at t ≥ a, V continued from (a, Va) with the piece's own formula."""
        It = Ia + quad(eg, a, t)
        h = p * eg(t) / D(It)
        if rm == 0:
            return h - u, It, None
        if in_B:  # u + rV − h > 0: (V·D·e^{cτ})' = (δ + u)·D·e^{cτ}; ∫ I e^{cs} by parts
            J = (It * mp.exp(c * t) - Ia * mp.exp(c * a)) / c - quad(lambda x: eg(x) * mp.exp(c * x), a, t) / c
            K = p * J + (1 - p) * I_eta * (mp.exp(c * t) - mp.exp(c * a)) / c
            V = (Va * D(Ia) * mp.exp(c * a) + (dm + u) * K) / (D(It) * mp.exp(c * t))
        else:  # (1 − V)' = −(h + δ)(1 − V), exp(∫h) = D
            V = 1 - (1 - Va) * D(Ia) / D(It) * mp.exp(-dm * (t - a))
        return h - rm * V - u, It, V

    in_B = not bool(above[0])  # f ≤ 0 ⇔ u + rV − h ≥ 0
    f0 = f_at(M(0), a, Ia, Va, in_B)[0]
    assert (f0 > 0) == bool(above[0])
    for i in flips:
        lo, hi = M(float(s[i])), M(float(s[i + 1]))
        root = mp.findroot(lambda t: f_at(t, a, Ia, Va, in_B)[0], (lo, hi), solver="illinois", tol=M(10) ** -50,
                           maxsteps=300, verify=False)
        _, Ir, Vr = f_at(root, a, Ia, Va, in_B)
        (ups if in_B else downs).append(root)
        a, Ia, Va, in_B = root, Ir, Vr, not in_B
    nan = float("nan")
    if not above.any():
        # the class itself at high precision: f at the float64 scan's maximum and at its neighbours
        i = int(np.argmax(f64(s)))
        assert all(f_at(M(float(s[j])), M(0), M(0), (u + dm) / (rm + dm), True)[0] < 0
                   for j in (max(i - 1, 0), i, min(i + 1, len(s) - 1)))
        return dict(cls="below", tau_in=float(t_end), tau_out=float(t_end), xi=nan, aw_max=nan)
    tin = ups[0] if ups else M(0)
    tout = downs[-1] if downs else eta
    out = dict(cls="norun", tau_in=float(tin), tau_out=float(tout), xi=nan, aw_max=nan)
    y = kappa + G(tin)
    if y >= 1:
        return out
    xi = mp.log(y * A / (1 - y)) / beta
    if xi > tout:
        return out
    if g(xi) < g(tin):
        out["cls"] = "false"
        return out
    d = xi - tin
    ts = min(th + d / 2, t_end if hetero else eta)
    aw = G(ts) - (G(ts - d) if ts >= d else 0)
    out.update(cls="run", xi=float(xi), aw_max=float(aw if hetero else aw + x0m))
    return out


def mp_check(fix):
    """One point per class from `points`, an r > 0 run of the interest grid and a hetero run against
    mpmath: the largest differences in a time and in AW_max."""
    P, IE, H = fix["points"], fix["interest_econ"], fix["hetero"]
    todo = []
    for cls in C.CLASSES:
        i = P["cls"].index(cls)
        todo.append((f"points[{i}] {cls}", {k: P[k][i] for k in ("beta", "eta", "t_end", "u", "p", "kappa", "lam")},
                     P["x0"], 0.0, 0.1, False, {k: P[k][i] for k in ("cls", *FIELDS)}))
    sh = IE["shape"]
    idx = np.arange(int(np.prod(sh))).reshape(sh)
    for want in ("run", "norun"):
        cand = [n for n in idx[:, :, :, [d for d, r in enumerate(IE["r"]) if r > 0]].ravel()
                if IE["cls"][n] == want and IE["ok"][n] and IE["tau_in"][n] > 0]
        if cand:
            i, a_, b_, d_, c_, j_ = np.unravel_index(cand[len(cand) // 2], sh)
            q = dict(beta=IE["beta"][i], eta=IE["eta"][i], t_end=IE["t_end"][i], u=IE["u"][j_], p=IE["p"][a_],
                     kappa=IE["kappa"][c_], lam=IE["lam"][b_])
            n = cand[len(cand) // 2]
            todo.append((f"interest_econ[{i},{a_},{b_},{d_},{c_},{j_}] {want}", q, IE["x0"], IE["r"][d_],
                         IE["delta"][d_], False, {k: IE[k][n] for k in ("cls", *FIELDS)}))
    h = next(c for c in H if c["cls"] == "run")
    todo.append(("hetero run", h, h["x0"], 0.0, 0.1, True, h))
    dt = da = 0.0
    names = []
    for name, q, x0, r, delta, het, want in todo:
        m = mp_point(q, x0, r, delta, het)
        assert m["cls"] == want["cls"], (name, m["cls"], want["cls"])
        for k in FIELDS:
            w = want[k]
            if w is None:
                assert m[k] != m[k], (name, k)
                continue
            if k == "aw_max":
                da = max(da, abs(m[k] - w))
            else:
                dt = max(dt, abs(m[k] - w))
        names.append(name)
    assert dt <= C.TOL_TIME / 1000 and da <= C.TOL_AW / 1000, (dt, da)
    out = dict(digits=MP_DIGITS, points=names, max_time_diff=dt, max_aw_diff=da)
    # the first two-group run in which every buffer is a crossing, none a fallback (0, η or t_end)
    n, h = next((n, c) for n, c in enumerate(fix["hetero_unequal"]) if c["K"] == 2 and c["cls"] == "run"
                and min(c["tau_in"]) > 0.0 and max(c["tau_out"]) < c["eta"])
    dt, da = mp_hetero(h)
    assert dt <= 1e-8 and da <= 1e-9, (dt, da)
    out["hetero_unequal"] = dict(digits=MP_DIGITS_HETERO, case=n, max_time_diff=dt, max_aw_diff=da)
    return out


# ------------------------------------------------------------------------------------------------
# the social-learning fixed point (tests/continuum_social.py): tests/golden/continuum_social.json
OUT_SOCIAL = REPO / "tests" / "golden" / "continuum_social.json"
SOCIAL_BOX = dict(beta=(0.5, 20.0), x0=(1e-5, 1e-2), eta_over_rise=(1.2, 4.0), p=(0.05, 0.99), kappa=(0.1, 0.9),
                  lam=(0.002, 0.5), u=(0.005, 2.0))
SOCIAL_TOLS = (1e-3, 1e-4, 1e-5)
SOCIAL_SEEDS = dict(groups=201, cap=202, past_eta=203, throws=204, below=205, false=206, margin=207)
N_SOCIAL_GROUPS, SOCIAL_NB, SOCIAL_NU = 12, 2, 4
SOCIAL_NEED = dict(throws=4, below=6, false=2)
SOCIAL_FALSE_SEARCH = 400  # points searched for a false equilibrium of the returned iterate
SOCIAL_SCRIPT = dict(p=0.99, kappa=0.25, lam=0.25, x0=1e-4, tol=1e-4, max_iter=500, beta=[0.9, 0.9], eta=[30 / 0.9] * 2,
                     u=[0.5, 0.1, 0.3, 0.6])
SOCIAL_SELF = 3  # points on which the tests repeat the model
N_MARGIN = 200


def draw_social_group(rng, n, max_iter=500, u_range=None, kappa=None):
    x0 = logu(rng, *SOCIAL_BOX["x0"])
    beta = [logu(rng, *SOCIAL_BOX["beta"]) for _ in range(SOCIAL_NB)]
    eta = [float(rng.uniform(*SOCIAL_BOX["eta_over_rise"])) * math.log((1.0 - x0) / x0) / b for b in beta]
    return dict(p=float(rng.uniform(*SOCIAL_BOX["p"])), kappa=float(rng.uniform(*(kappa or SOCIAL_BOX["kappa"]))),
                lam=logu(rng, *SOCIAL_BOX["lam"]), x0=x0, tol=SOCIAL_TOLS[n % len(SOCIAL_TOLS)], max_iter=max_iter,
                beta=beta, eta=eta, u=sorted(logu(rng, *(u_range or SOCIAL_BOX["u"])) for _ in range(SOCIAL_NU)))


def social_points(grp):
    return [dict(beta=grp["beta"][b], eta=grp["eta"][b], u=u, **{k: grp[k] for k in ("p", "kappa", "lam", "x0", "tol",
                                                                                       "max_iter")})
            for b in range(len(grp["beta"])) for u in grp["u"]]


def social_model(q):
    """The model alone on one point: its class (searches)."""
    import continuum_social as CS

    r = CS.solve_social(**q)
    return r["cls"], r["fp_iters"]


def social_oracle(q, stats=True):
    import oracle as O
    from sbr import julia_range

    o = O.sweep_social([q["beta"]], q["eta"], [q["u"]], q["p"], q["kappa"], q["lam"], julia_range(0.0, q["eta"], 1000),
                       x0=q["x0"], tol=q["tol"], max_iter=q["max_iter"], nthreads=1, stats=stats)
    return {k: (int(v[0, 0]) if v.dtype.kind in "iu" else jnum(v[0, 0])) for k, v in o.items()}


def social_knots(q):
    """The oracle's learning knots of the returned iterate: rule (ii) takes the reference's knot spacing
    at a jump from them."""
    import oracle as O
    from sbr import julia_range

    return O.social_point(q["beta"], q["eta"], q["u"], q["p"], q["kappa"], q["lam"], julia_range(0.0, q["eta"], 1000),
                          x0=q["x0"], tol=q["tol"], max_iter=q["max_iter"])["t"]


def social_eval_group(pool, grp):
    """Every point of a group; a column in which any point asks for the η redraw is evaluated again as a
    whole at the new η (the sweep takes one η per β column), at most three times."""
    grp = dict(grp, beta=list(grp["beta"]), eta=list(grp["eta"]), eta_redraws=[0] * len(grp["beta"]))
    nu = len(grp["u"])
    for _ in range(MAX_REDRAWS + 1):
        pts = pool.map(social_eval_fixed, social_points(grp))
        again = False
        for b in range(len(grp["beta"])):
            if any(pt["wants_redraw"] for pt in pts[b * nu:(b + 1) * nu]) and grp["eta_redraws"][b] < MAX_REDRAWS:
                grp["eta"][b] *= REDRAW
                grp["eta_redraws"][b] += 1
                again = True
        if not again:
            break
    for pt in pts:
        if pt.pop("wants_redraw"):
            pt.update(ok=False, reason="BoundsError after redraws")
    grp["points"] = pts
    return grp


def social_eval_fixed(q):
    """``social_eval`` without the redraw loop: wants_redraw says that the point asks for one."""
    import continuum_social as CS

    res = CS.solve_social(**q)
    o = social_oracle(q)
    ok, reason = CS.verdict_social(res, q["eta"], q["kappa"], q["tol"], social_knots(q))
    oob = (o["status"] & (CS.OOB | CS.NOTCONV | 0x1)) == (CS.OOB | CS.NOTCONV)
    wants = bool(ok and oob and (res["cls"] != "throws" or o["fp_iters"] < res["fp_iters"]))
    margins = [abs(e - q["tol"]) / q["tol"] for e in res["errs"]]
    return dict(cls=res["cls"], inner=res["inner"], fp_iters=res["fp_iters"], tau_in=jnum(res["tau_in"]),
                tau_out=jnum(res["tau_out"]), xi=jnum(res["xi"]), aw_max=jnum(res["aw_max"]), ok=bool(ok), reason=reason,
                wants_redraw=wants, min_margin=min(margins) if margins else None, n_knots=o["n_knots"],
                oracle={k: o[k] for k in ("xi", "tau_in_unc", "tau_out_unc", "aw_max", "tol", "status", "iters",
                                          "fp_iters")})


def social_halved(q):
    """(a): the model at CELLS and at 2·CELLS cells on one point: the largest change of a time and of AW_max
    (None where the class or the iterate count changes)."""
    import continuum_social as CS

    a, b = CS.solve_social(**q), CS.solve_social(**q, cells=2 * CS.CELLS)
    if (a["cls"], a["fp_iters"]) != (b["cls"], b["fp_iters"]):
        return None
    if a["cls"] == "throws":
        return 0.0, 0.0
    dt = max([abs(a[k] - b[k]) for k in ("tau_in", "tau_out", "xi") if a[k] == a[k]] or [0.0])
    return dt, abs(a["aw_max"] - b["aw_max"]) if a["aw_max"] == a["aw_max"] else 0.0


def social_closed_form(q):
    """(b): G_n of the first three iterates from the closed form against DOP853 at rtol 1e-13 on
    dG/dt = (1 − G) β AW_{n−1}(t), with the model's own AW_{n−1}: the largest difference on the grid."""
    import continuum_social as CS
    from scipy.integrate import solve_ivp

    worst = [0.0]

    def hook(n, t, A, G):
        if n > 3:
            return
        te = t[::len(t) // 2000]
        sol = solve_ivp(lambda x, y: (1.0 - y) * q["beta"] * np.interp(x, t, A), (0.0, float(t[-1])), [q["x0"]],
                        method="DOP853", rtol=1e-13, atol=1e-16, t_eval=te, max_step=float(t[-1]) / 2000)
        assert sol.success, sol.message
        worst[0] = max(worst[0], float(np.abs(sol.y[0] - G[::len(t) // 2000][:len(te)]).max()))

    CS.solve_social(**dict(q, max_iter=min(q["max_iter"], 3)), hook=hook)
    return worst[0]


def social_residual(q):
    """The forced ODE's closed form on the oracle's own knots of the returned iterate."""
    import continuum_social as CS
    import oracle as O
    from sbr import julia_range

    r = O.social_point(q["beta"], q["eta"], q["u"], q["p"], q["kappa"], q["lam"], julia_range(0.0, q["eta"], 1000),
                       x0=q["x0"], tol=q["tol"], max_iter=q["max_iter"])
    return CS.forced_ode_residual(r["t"], r["G"], r["aw_old"], q["beta"], q["x0"])


def make_social(margin=False) -> dict:
    """tests/golden/continuum_social.json: a list of groups, each one sweep_social call of 2 β columns
    (with their own η) × 4 u at one (p, κ, λ, x0, tol, max_iter)."""
    import multiprocessing as mp

    import continuum_social as CS

    with mp.Pool(8) as pool:
        groups, searched = [], {}

        def add(grp, kind):
            g = social_eval_group(pool, grp)
            g["kind"] = kind
            groups.append(g)
            print(f"group {len(groups) - 1} {kind}: " + " ".join(f"{pt['cls']}/{pt['fp_iters']}{'' if pt['ok'] else '!'}"
                                                                 for pt in g["points"]), file=sys.stderr)
            return g

        def count(cls):
            return sum(pt["ok"] and pt["cls"] == cls and (cls != "past_eta" or pt["fp_iters"] == 501)
                       for g in groups for pt in g["points"])

        def search(name, want, need, limit, fp_iters=None, **kw):
            """Groups from a seeded search of its own until ``need`` well-conditioned points of class ``want``
            stand in the fixture; a drawn group without a candidate is of another kind, not a drop."""
            rng = np.random.default_rng(SOCIAL_SEEDS[name])
            n = searched.setdefault(name, 0)
            while count(want) < need and n < limit:
                grp = draw_social_group(rng, n, **kw)
                n += 1
                if any(c == want and (fp_iters is None or f == fp_iters)
                       for c, f in pool.map(social_model, social_points(grp))):
                    add(grp, name)
            searched[name] = n

        add(SOCIAL_SCRIPT, "script")
        rng = np.random.default_rng(SOCIAL_SEEDS["groups"])
        for n in range(N_SOCIAL_GROUPS):
            add(draw_social_group(rng, n), "seeded")
        rng = np.random.default_rng(SOCIAL_SEEDS["cap"])
        add(draw_social_group(rng, 2, max_iter=7), "cap")
        search("past_eta", "past_eta", 1, 40, fp_iters=501, max_iter=600, kappa=(0.6, 0.9), u_range=(0.1, 2.0))
        search("throws", "throws", SOCIAL_NEED["throws"], 40)
        search("below", "below", SOCIAL_NEED["below"], 40, u_range=(0.5, 2.0))
        # a false equilibrium of the returned iterate needs g(ξ) < g(τ̄_IN): as in `points`, a search at κ ≥ 0.8
        rng = np.random.default_rng(SOCIAL_SEEDS["false"])
        n_false, false_groups = 0, []
        while n_false < SOCIAL_FALSE_SEARCH and count("false") < SOCIAL_NEED["false"]:
            grp = draw_social_group(rng, n_false // 8, kappa=(0.8, SOCIAL_BOX["kappa"][1]))
            n_false += 8
            if any(c == "false" for c, _ in pool.map(social_model, social_points(grp))):
                add(grp, "false")
        searched["false_points"] = n_false

        pts = [(g, i, pt) for g in groups for i, pt in enumerate(g["points"])]
        drawn, dropped, reasons, classes = len(pts), 0, {}, {}
        for g, i, pt in pts:
            if pt["ok"]:
                classes[pt["cls"]] = classes.get(pt["cls"], 0) + 1
                continue
            dropped += 1
            key = pt["reason"].split(" at ")[0].split(" moves")[0]
            reasons[key] = reasons.get(key, 0) + 1
        if dropped > 0.10 * drawn:
            raise SystemExit(f"social: {dropped} of {drawn} drawn points dropped ({reasons}): more than 10 %")
        assert classes.get("cap", 0) >= 1 and classes.get("past_eta", 0) >= 1, classes
        assert all(classes.get(k, 0) >= v for k, v in SOCIAL_NEED.items() if k != "false"), classes
        assert any(pt["cls"] == "past_eta" and pt["fp_iters"] == 501 and pt["ok"] for _, _, pt in pts)

        # the oracle against the model, as the tests compare them
        import oracle as O
        from sbr import julia_range

        worst = {"time": 0.0, "aw": 0.0}
        for n, g in enumerate(groups):
            a, kw = CS.group_args(g)
            cmp = np.stack([julia_range(0.0, float(e), 1000) for e in g["eta"]])
            d = CS.compare(O.sweep_social(*a, cmp, **kw), g, f"oracle group {n}")
            worst = {k: max(worst[k], d[k]) for k in worst}
        # (a) the grid cell halved, on every ok point; (b) the closed form against DOP853 on three points
        ok_q = [CS.point_of(g, i) for g, i, pt in pts if pt["ok"]]
        halves = pool.map(social_halved, ok_q, chunksize=1)
        changed = sum(h is None for h in halves)
        half = dict(time=max(h[0] for h in halves if h), aw=max(h[1] for h in halves if h), class_or_iterate_changed=changed)
        pick = {}
        for gi, g in enumerate(groups):
            for i, pt in enumerate(g["points"]):
                if pt["ok"] and pt["cls"] in ("run", "below", "cap") and pt["cls"] not in pick and pt["fp_iters"] <= 60:
                    pick[pt["cls"]] = (gi, i)
        self_pts = [pick[k] for k in ("run", "below", "cap")]
        self_q = [CS.point_of(groups[gi], i) for gi, i in self_pts]
        closed = max(pool.map(social_closed_form, self_q))
        resid = pool.map(social_residual, self_q)
        assert half["time"] <= C.TOL_TIME / 100 and half["aw"] <= C.TOL_AW / 100 and closed <= C.TOL_AW / 100, (half, closed)
        meta = dict(tol_time=CS.TOL_TIME, tol_aw=CS.TOL_AW, cells=CS.CELLS, stop_margin=CS.STOP_MARGIN,
                    knot_factor=CS.KNOT_FACTOR, throw_margin=CS.THROW_MARGIN,
                    box={k: list(v) for k, v in SOCIAL_BOX.items()}, tols=list(SOCIAL_TOLS), seeds=SOCIAL_SEEDS,
                    drawn=drawn, dropped=dropped, dropped_share=dropped / drawn, dropped_reasons=reasons,
                    eta_redraws=sum(sum(g["eta_redraws"]) for g in groups), classes=classes, searched=searched,
                    false_statement=(None if classes.get("false", 0) >= SOCIAL_NEED["false"] else
                                     f"a search of {n_false} points at kappa >= 0.8 found {classes.get('false', 0)} "
                                     "well-conditioned false equilibria of the returned iterate"),
                    oracle=worst, halved_cell=half, closed_form_vs_dop853=closed,
                    max_beta_knot_spacing=max(g["beta"][i // len(g["u"])] * g["eta"][i // len(g["u"])] / pt["n_knots"]
                                              for g, i, pt in pts),
                    self_points=[list(v) for v in self_pts],
                    path_points=[dict(group=gi, point=i, oracle_residual=r, bound=2.0 * r)
                                 for (gi, i), r in zip(self_pts, resid)])
        if margin:
            meta["stop_margin_measurement"] = social_margin(pool)
    return dict(meta=meta, groups=groups)


def social_margin(pool):
    """Rule (i)'s margin: on N_MARGIN random points of the box, the largest min_n |err_n − tol| / tol among the
    points that no other rule drops and on which model and oracle differ in fp_iters (none of them a BoundsError)."""
    rng = np.random.default_rng(SOCIAL_SEEDS["margin"])
    qs, k = [], 0
    while len(qs) < N_MARGIN:
        pts = social_points(draw_social_group(rng, k))
        k += 1
        qs += [pts[0], pts[5]]
    out = pool.map(social_eval_fixed, qs, chunksize=1)
    differ = [r for r in out if r["oracle"]["fp_iters"] != r["fp_iters"] and not r["oracle"]["status"] & 0x80]
    by_margin = [r["min_margin"] for r in differ if r["ok"] or "stopping margin" in r["reason"]]
    return dict(points=N_MARGIN, fp_iters_differ=len(differ), explained_by_other_rules=len(differ) - len(by_margin),
                smallest_agreeing_margin=max(by_margin, default=0.0))


def build() -> dict:
    import oracle as O

    tally = Tally()
    fix = dict(points=make_points(tally),
               econ=make_grid(tally, SEEDS["econ"], 3, 2, 2, 3, 8),
               interest_econ=make_grid(tally, SEEDS["interest_econ"], 2, 2, 1, 2, 6, rates=[(0.0, 0.1), (0.05, 0.1)]),
               hetero=make_hetero(tally))
    share = tally.dropped / tally.drawn
    if share > 0.10:
        raise SystemExit(f"{tally.dropped} of {tally.drawn} drawn points are ill-conditioned: more than 10 %")
    classes = {}
    for lst in (fix["points"]["cls"], [c for c, ok in zip(fix["econ"]["cls"], fix["econ"]["ok"]) if ok],
                [c for c, ok in zip(fix["interest_econ"]["cls"], fix["interest_econ"]["ok"]) if ok],
                [c["cls"] for c in fix["hetero"]]):
        for c in lst:
            classes[c] = classes.get(c, 0) + 1
    assert all(classes.get(c, 0) >= (2 if c == "false" else 1) for c in C.CLASSES), classes
    fix["hetero_unequal"], unequal = make_hetero_unequal(O)
    share_all = (tally.dropped + unequal["dropped"]) / (tally.drawn + unequal["drawn"])
    if share_all > 0.10 or unequal["dropped"] > 0.10 * unequal["drawn"]:
        raise SystemExit(f"{unequal['dropped']} of {unequal['drawn']} unequal-rate draws dropped; {share_all:.3f} of all")
    unequal["dropped_share_all_lists"] = share_all
    fix["meta"] = dict(tol_time=C.TOL_TIME, tol_aw=C.TOL_AW, box={k: list(v) if isinstance(v, tuple) else v
                                                                  for k, v in BOX.items()},
                       seeds=SEEDS, drawn=tally.drawn, dropped=tally.dropped, dropped_share=share,
                       dropped_reasons=tally.reasons, classes=classes, hetero_unequal=unequal, mpmath=mp_check(fix))
    with contextlib.redirect_stdout(io.StringIO()):
        worst = CC.oracle_maxima(O, CC.load(json.dumps(fix)))
    for name, d in worst.items():
        if d["time"] > C.TOL_TIME / 2 or d["aw"] > C.TOL_AW / 2:
            raise SystemExit(f"the oracle leaves half the tolerance on {name}: {d}")
    fix["meta"]["oracle"] = worst
    return fix


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="regenerate and compare with the committed fixture")
    ap.add_argument("--social", action="store_true", help="the social fixed point's fixture (continuum_social.json)")
    ap.add_argument("--margin", action="store_true", help="with --social: measure the stopping margin again (200 points)")
    a = ap.parse_args()
    if a.social:
        sys.path.insert(0, str(REPO / "replication-social-bank-runs_amd"))
        fix = make_social(a.margin)
        if not a.margin and OUT_SOCIAL.exists():  # the measurement is kept from the run that made it
            old = json.loads(OUT_SOCIAL.read_text())["meta"].get("stop_margin_measurement")
            if old:
                fix["meta"]["stop_margin_measurement"] = old
        text = json.dumps(fix, indent=1) + "\n"
        if a.check:
            same = OUT_SOCIAL.read_text() == text
            print("identical" if same else "DIFFERENT")
            raise SystemExit(0 if same else 1)
        OUT_SOCIAL.write_text(text)
        print(f"{OUT_SOCIAL.relative_to(REPO)}: {len(text)} bytes; " + json.dumps({k: v for k, v in fix["meta"].items()
                                                                                  if k not in ("box", "seeds")}))
        return
    text = json.dumps(build(), indent=1) + "\n"
    if a.check:
        same = OUT.read_text() == text
        print("identical" if same else "DIFFERENT")
        raise SystemExit(0 if same else 1)
    OUT.write_text(text)
    m = json.loads(text)["meta"]
    print(f"{OUT.relative_to(REPO)}: {len(text)} bytes; drawn {m['drawn']}, dropped {m['dropped']} "
          f"({100 * m['dropped_share']:.1f} %: {m['dropped_reasons']}); classes {m['classes']}; mpmath {m['mpmath']}; oracle {m['oracle']}")


if __name__ == "__main__":
    main()
