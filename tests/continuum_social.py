"""The continuum model of the social-learning fixed point (not a test module, not a conftest).

An independent float64 reference for solve_equilibrium_social_learning, restated from the reference's
source (social_learning_solver.jl:63-263, social_learning_dynamics.jl:58-114 and solver.jl's
hazard_rate, optimal_buffer, compute_ξ, get_AW) and not from the oracle.  Functions on [0, η] live on
a fixed uniform grid of CELLS cells; integrals are trapezoid sums, exact across the jumps of AW_{n−1}
(``_jump_terms``), and look-ups are linear.  Iterate n
follows from AW_{n−1} in closed form:

    G_n(t) = 1 − (1 − x0)·exp(−β ∫₀ᵗ AW_{n−1})            (dG/dt = (1 − G) β AW_{n−1}, solved exactly)
    g_n = (1 − G_n) β AW_{n−1},  I = ∫ e^{λs} g_n,  h = p e^{λτ} g_n / (p I(τ) + (1 − p) I(η))
    buffers: h ≤ u everywhere → τ̄_IN = τ̄_OUT = η ("below"); else the first up-crossing (or 0) and the
    last down-crossing (or η)
    ξ_n = G_n⁻¹(κ + G_n(τ̄_IN)) if G_n(τ̄_OUT) − G_n(τ̄_IN) ≥ κ, and g_n(ξ) ≥ g_n(τ̄_IN) (else "false")
    run:     AW_n(t) = G_n(t) − [t ≥ ξ − τ̄_IN]·G_n(t − ξ + τ̄_IN) + G_n(0);  AW_max = sup AW_n
    no run:  ξ_n = ξ_{n−1} + η/500; past η the iteration stops; AW_n from get_AW with τ̄ constrained to ξ_n
    err_n = max over range(0, η, length = 1000) of |AW_n − AW_{n−1}|;  err_n < tol → converged
    else AW_n ← ½ AW_{n−1} + ½ AW_n;   AW_0 = the logistic G (no + x0)

Classes: the returned iterate's own ("run", "below", "norun", "false") where the fixed point
converged, else "cap" (max_iter reached), "past_eta" (the ξ search left [0, η]) or "throws": at some
iterate the hazard is still above u at η, so τ̄_OUT = η is the last learning knot, and G_n(η) −
G_n(τ̄_IN) < κ; the bisection then walks into the last knot interval and the reference's look-up at
ξ + ε raises a BoundsError.  For "throws" the model predicts the iterate and nothing else.

AW_n has jumps: the IN term switches on with the value G(0) = x0 at t = ξ − τ̄_IN, and damping keeps
earlier jumps at halved weight.  The model records every jump (place, size) so that ``verdict_social``
can tell where the reference's knot grid, and not the model, decides the sup-norm test.

numpy only.  ``compare`` is what tests/test_continuum_social.py (oracle) and
tests/test_gpu_continuum_social.py (GPU) share.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

PATH = Path(__file__).resolve().parent / "golden" / "continuum_social.json"
TOL_TIME, TOL_AW = 2e-5, 1e-5  # tests/continuum.py
CELLS = 400_000                # the model's grid: η / CELLS per cell (DESIGN.md §2 "Social fixed point")
N_CMP = 1000
INNER = ("run", "below", "norun", "false")
CLASSES = INNER + ("cap", "past_eta", "throws")
STOP_MARGIN = 3.3e-4   # rule (i): |err_n − tol| > STOP_MARGIN·tol at every iterate (measured)
KNOT_FACTOR = 1.0     # rule (ii): a jump blurs one knot interval of its neighbourhood (``knot_width``)
THROW_MARGIN = 1e-4   # rule (iii): |κ + G(τ̄_IN) − G(η)| > 1e-4·κ wherever τ̄_OUT = η
JUMP_FLOOR = 1e-12    # jumps smaller than this are forgotten

INFO_BITS = 0x0800    # SBR_STIFF_SWITCH (include/sbr_status.h)
RUN, BELOW, COLLAPSE, MAXITER, FALSE_EQ, OOB, NOTCONV = 0x3, 0x6, 0x8, 0x10, 0x20, 0x80, 0x1000
STATUS_OF = {"run": (RUN,), "below": (BELOW,), "norun": (COLLAPSE, MAXITER), "false": (FALSE_EQ,)}
FIELDS = ("xi", "tau_in_unc", "tau_out_unc", "aw_max", "tol")
TIMES = (("xi", "xi"), ("tau_in", "tau_in_unc"), ("tau_out", "tau_out_unc"))


def _cumtrapz(y, h):
    out = np.empty_like(y)
    out[0] = 0.0
    np.cumsum(0.5 * h * (y[1:] + y[:-1]), out=out[1:])
    return out


def _jump_terms(n, h, jumps, weight=None):
    """What the trapezoid sum misses across the cells that hold a jump: a step of size s at fraction f of
    its cell (t_i, t_{i+1}] integrates to s·(1 − f)·h over the cell, the trapezoid rule gives s·h/2; the
    difference, cumulated like the integral itself.  Without it the model is first order in the cell."""
    d = np.zeros(n)
    for loc, size in jumps:
        i = min(max(int(np.ceil(loc / h)) - 1, 0), n - 2)
        d[i + 1] += (size if weight is None else size * weight(loc)) * h * (0.5 - (loc / h - i))
    return np.cumsum(d)


def _shifted(G, t, s, h):
    """[t + s ≥ 0]·G(max(t + s, 0)) on the grid, s ≤ 0 (get_AW's truncated look-up, solver.jl:511-520)."""
    x = t + s
    return np.where(x >= 0.0, np.interp(np.maximum(x, 0.0), t, G), 0.0)


def _equilibrium(t, h, G, g, hz, u, kappa, jcells) -> dict:
    """The baseline equilibrium on one iterate's learning curve: inner class, τ̄_IN, τ̄_OUT, ξ and what the
    verdict needs (optimal_buffer, compute_ξ in the continuum)."""
    eta, nan = float(t[-1]), float("nan")
    it = dict(inner=None, tau_in=eta, tau_out=eta, xi=nan, at_eta=False, gap_eta=nan, buffer_at_jump=False,
              bisect_ratio=0.0)
    above = hz > u
    if not above.any():
        it["inner"] = "below"
        return it
    up = np.flatnonzero(~above[:-1] & above[1:])
    dn = np.flatnonzero(above[:-1] & ~above[1:])
    if len(up):
        i = int(up[0])
        tin = float(t[i] + (u - hz[i]) * h / (hz[i + 1] - hz[i]))
        it["buffer_at_jump"] |= i in jcells
    else:
        tin = float(t[np.argmax(above)])
    if len(dn):
        i = int(dn[-1])
        tout = float(t[i] + (u - hz[i]) * h / (hz[i + 1] - hz[i]))
        it["buffer_at_jump"] |= i in jcells
    else:
        tout = float(t[len(above) - 1 - np.argmax(above[::-1])])
    it.update(tau_in=tin, tau_out=tout)
    G_in, G_out = float(np.interp(tin, t, G)), float(np.interp(tout, t, G))
    if tout == eta:
        it["at_eta"], it["gap_eta"] = True, kappa + G_in - G_out
    if not tin < tout:
        it["inner"] = "unmodelled"
    elif G_out - G_in < kappa:
        it["inner"] = "throws" if tout == eta else "norun"
    else:
        xi = float(np.interp(kappa + G_in, G, t))
        g_xi, g_in = float(np.interp(xi, t, g)), float(np.interp(tin, t, g))
        it["slope"] = (g_xi, g_in)
        it["bisect_ratio"] = g_xi * float(np.spacing(xi)) / (10.0 * float(np.spacing(kappa)))
        it["inner"] = "run" if g_xi >= g_in else "false"
        if it["inner"] == "run":
            it["xi"] = xi
    return it


def solve_social(beta, eta, u, p, kappa, lam, x0, tol=1e-4, max_iter=500, cells=CELLS, hook=None) -> dict:
    """One fixed point.  Returns cls, inner (the returned iterate's own class), fp_iters, tau_in,
    tau_out, xi, aw_max (NaN where the class has none), errs [fp_iters] and ``iterates``: per iterate
    what ``verdict_social`` needs."""
    beta, eta, u, p, kappa, lam, x0, tol = (float(v) for v in (beta, eta, u, p, kappa, lam, x0, tol))
    nan = float("nan")
    t = np.linspace(0.0, eta, cells + 1)
    h = eta / cells
    cmp_t = np.linspace(0.0, eta, N_CMP)
    elam = np.exp(lam * t)
    A = 1.0 / (1.0 + (1.0 - x0) / x0 * np.exp(-beta * t))  # AW_0: the logistic learning curve, no + x0
    jumps = []  # (place, size) of AW_{n−1}'s jumps
    xi_prev = 0.0
    errs, its = [], []
    out = dict(cls="cap", inner=None, u=u, fp_iters=int(max_iter), tau_in=nan, tau_out=nan, xi=nan, aw_max=nan)
    for n in range(1, int(max_iter) + 1):
        S = _cumtrapz(A, h)
        if jumps:
            S += _jump_terms(len(t), h, jumps)
        G = 1.0 - (1.0 - x0) * np.exp(-beta * S)
        if hook is not None:
            hook(n, t, A, G)
        g = (1.0 - G) * beta * A
        eg = elam * g
        I = _cumtrapz(eg, h)
        if jumps:  # g_n jumps with AW_{n−1}: by (1 − G_n)·β·e^{λt} times the jump
            I += _jump_terms(len(t), h, jumps, lambda x: (1.0 - float(np.interp(x, t, G))) * beta * np.exp(lam * x))
        hz = p * eg / (p * I + (1.0 - p) * I[-1])
        it = dict(n=n, aw_sup_at_jump=0.0, **_equilibrium(t, h, G, g, hz, u, kappa, {int(loc / h) for loc, _ in jumps}))
        new_jumps = []
        inner, tin, tout, xi = it["inner"], it["tau_in"], it["tau_out"], it["xi"]
        out["_last"] = (t, h, G, g, hz, {int(loc / h) for loc, _ in jumps})
        out.update(inner=inner, fp_iters=n, tau_in=tin, tau_out=tout, xi=nan, aw_max=nan)
        if inner in ("throws", "unmodelled"):
            its.append(it)
            out["cls"] = inner
            break
        if inner == "run":
            d = xi - tin
            AW = G - _shifted(G, t, -d, h) + x0
            sup = float(AW.max())
            if 0.0 < d <= eta:
                new_jumps.append((d, -x0))
                left = float(np.interp(d, t, G)) + x0  # the limit from the left of the IN term's switch
                if left > sup:
                    it["aw_sup_at_jump"], sup = float(np.interp(d, t, g)), left
            out.update(xi=xi, aw_max=sup)
            xi_new = xi
        else:
            xi_new = xi_prev + eta / 500.0
            if xi_new > eta:
                its.append(it)
                out["cls"] = "past_eta"
                break
            # get_AW with τ̄ constrained to ξ (solver.jl:500-501)
            s_in = (xi_new if tin >= xi_new else tin) - xi_new
            s_out = (xi_new if tout > xi_new else tout) - xi_new
            AW = _shifted(G, t, s_out, h) - _shifted(G, t, s_in, h) + x0
            if s_out < 0.0:
                new_jumps.append((-s_out, x0))
            if s_in < 0.0:
                new_jumps.append((-s_in, -x0))
        diff = np.interp(cmp_t, t, AW) - np.interp(cmp_t, t, A)
        err = float(np.abs(diff).max())
        errs.append(err)
        it.update(err=err, _near=_near_table(cmp_t, diff, jumps, new_jumps))
        its.append(it)
        if err < tol:
            out["cls"] = inner
            break
        xi_prev = xi_new
        A = 0.5 * A + 0.5 * AW
        jumps = [(loc, 0.5 * s) for loc, s in [*jumps, *new_jumps] if abs(0.5 * s) >= JUMP_FLOOR]
    out["errs"], out["iterates"] = errs, its
    return out


def _near_table(cmp_t, diff, old_jumps, new_jumps):
    """For err_n's conditioning, without keeping 1000 numbers for each of 500 iterates: per jump, the two
    comparison points that bracket it (the only ones that a ramp narrower than the comparison spacing
    can reach) with diff = AW_n − AW_{n−1} there, and the largest |diff| over all other points.  A jump of
    size s at d, ramped over a knot interval that also holds the comparison point c, moves the function
    at c towards its value on the other side of d: by −s·θ where c ≥ d, by +s·θ where c < d, θ in [0, 1];
    AW_{n−1} enters diff with a minus sign."""
    step = cmp_t[1] - cmp_t[0]
    near = {}
    for sign, jumps in ((-1.0, old_jumps), (1.0, new_jumps)):
        for loc, size in jumps:
            k = int(loc / step)
            for j in (k, k + 1):
                if 0 <= j < len(cmp_t):
                    e = near.setdefault(j, [float(diff[j]), []])
                    e[1].append((abs(cmp_t[j] - loc), sign * size * (-1.0 if cmp_t[j] >= loc else 1.0), loc))
    mask = np.ones(len(cmp_t), bool)
    mask[list(near)] = False
    rest = float(np.abs(diff[mask]).max()) if mask.any() else 0.0
    return dict(rest=rest, near=list(near.values()))


def err_range(it, width_at):
    """(lowest, highest) err_n if a comparison point closer than ``width_at(place)`` to a jump may take any
    value between the jump's two sides."""
    lo = hi = it["_near"]["rest"]
    for d, js in it["_near"]["near"]:
        a = d + sum(min(0.0, s) for dist, s, loc in js if dist < width_at(loc))
        b = d + sum(max(0.0, s) for dist, s, loc in js if dist < width_at(loc))
        lo = max(lo, 0.0 if a <= 0.0 <= b else min(abs(a), abs(b)))
        hi = max(hi, abs(a), abs(b))
    return lo, hi


def knot_width(knots, factor=None):
    """place → KNOT_FACTOR × the longest knot interval within one comparison step of it: the interval in
    which the reference's linear AW ramps across a new jump is an ordinary one of that neighbourhood (the
    integrator refines only around the kinks of earlier iterates)."""
    knots = np.asarray(knots, float)
    gaps = np.diff(knots)
    step = float(knots[-1]) / (N_CMP - 1)
    factor = KNOT_FACTOR if factor is None else factor

    def width_at(loc):
        i = max(int(np.searchsorted(knots, loc - step, side="right")) - 1, 0)
        j = min(int(np.searchsorted(knots, loc + step, side="left")), len(gaps))
        return factor * float(gaps[i:max(j, i + 1)].max())
    return width_at


def verdict_social(res, eta, kappa, tol, knots, tol_time=TOL_TIME, tol_aw=TOL_AW, factor=None):
    """(ok, reason): is the fixed point's outcome the model's to predict?  On the returned iterate and on
    every one before it:
      (i)   err_n is away from tol by a relative STOP_MARGIN;
      (ii)  the comparison points closer to a jump of AW_n or AW_{n−1} than KNOT_FACTOR × the reference's
            knot spacing there (``knots``: the oracle's learning knots of the returned iterate) cannot
            move err_n across tol;
      (iii) wherever τ̄_OUT = η, κ + G(τ̄_IN) − G(η) is away from 0 by THROW_MARGIN·κ;
    and, as in ``continuum.verdict``: the bisection resolves its root in floating point, no buffer sits in
    the cell of a jump, and where AW's supremum is the left limit of a jump the knot spacing times the
    slope there stays below half the AW tolerance."""
    if res["cls"] == "unmodelled":
        return False, "unmodelled"
    width_at = knot_width(knots, factor)
    for it in res["iterates"]:
        n = it["n"]
        if it["at_eta"] and abs(it["gap_eta"]) <= THROW_MARGIN * kappa:
            return False, f"kappa + G(tau_in) - G(eta) within margin at iterate {n}"
        if it["buffer_at_jump"]:
            return False, f"buffer at a jump at iterate {n}"
        if it["bisect_ratio"] > 1.0:
            return False, f"bisection resolution at iterate {n}"
        if "slope" in it:
            a, b = it["slope"]
            if abs(a - b) <= 1e-4 * max(abs(a), abs(b)):
                return False, f"slope test within 1e-4 at iterate {n}"
        if "err" not in it:
            continue
        if abs(it["err"] - tol) <= STOP_MARGIN * tol:
            return False, f"err within the stopping margin at iterate {n}"
        lo, hi = err_range(it, width_at)
        if (lo < tol) != (hi < tol):
            return False, f"a jump decides the stopping test at iterate {n}"
    last = res["iterates"][-1]
    # continuum.verdict's rules on the returned iterate: a relative ±1e-4 on u or κ keeps the class and ±1e-7 on u
    # moves no time by more than TOL_TIME / 4.  Its fourth rule (±5e-6 on u, the baseline's trapezoid error in
    # h on ~2,300 knots) has no counterpart: the forced ODE leaves 25 times as many knots, (βΔ)²/12 < 1e-7
    if res["cls"] != "throws":
        for du, dk, lim in ((-1e-4, 0, None), (1e-4, 0, None), (0, -1e-4, None), (0, 1e-4, None), (-1e-7, 0, tol_time / 4),
                            (1e-7, 0, tol_time / 4)):
            q = _equilibrium(*res["_last"][:5], res["u"] * (1.0 + du), kappa * (1.0 + dk), res["_last"][5])
            if q["inner"] != last["inner"]:
                return False, f"class changes at u*(1{du:+g}), kappa*(1{dk:+g})"
            if lim is not None:
                for k in ("tau_in", "tau_out", "xi"):
                    if abs(q[k] - last[k]) > lim:  # NaN compares False: both NaN in one class
                        return False, f"{k} moves {abs(q[k] - last[k]):.2e} at u*(1{du:+g})"
    if res["inner"] == "run" and last["aw_sup_at_jump"] * width_at(res["xi"] - res["tau_in"]) > tol_aw / 2:
        return False, "AW_max at a jump"
    return True, ""


# ---------------------------------------------------------------------------------------------
# the fixture and the comparison shared by the oracle test and the GPU test
def load() -> dict:
    fix = json.loads(PATH.read_text())
    assert fix["meta"]["tol_time"] == TOL_TIME and fix["meta"]["tol_aw"] == TOL_AW
    return fix


def _num(x):
    return float("nan") if x is None else float(x)


def group_args(grp: dict) -> tuple:
    """(positional, keyword) arguments of sweep_social (oracle and engine alike) for one group."""
    return ((np.array(grp["beta"]), np.array(grp["eta"]), np.array(grp["u"]), grp["p"], grp["kappa"], grp["lam"]),
            dict(x0=grp["x0"], tol=grp["tol"], max_iter=grp["max_iter"]))


def assert_recorded(got: dict, grp: dict, what: str):
    """``got`` [n_beta, n_u] equals the group's recorded oracle result bit for bit: seven fields, status
    and fp_iters."""
    for k in (*FIELDS, "status", "iters", "fp_iters"):
        a = np.asarray(got[k]).reshape(-1)
        b = np.array([_num(pt["oracle"][k]) for pt in grp["points"]])
        if k in ("status", "iters", "fp_iters"):
            same = a.astype(np.int64) == b.astype(np.int64)
        else:
            same = (a == b) | (np.isnan(a) & np.isnan(b))
        assert same.all(), (what, k, [(int(i), a[i], b[i]) for i in np.flatnonzero(~same)[:4]])


def compare(got: dict, grp: dict, what: str = "") -> dict:
    """Assert that ``got`` [n_beta, n_u] is the model's on every ok point of the group: class (status
    bits, NaN / Inf sentinels, τ̄ = η exactly in "below"), fp_iters exactly, values within TOL_TIME and
    TOL_AW; for "throws", fp_iters and the two status bits only.  Returns the largest deviations."""
    st = np.asarray(got["status"]).reshape(-1) & ~np.uint32(INFO_BITS)
    g = {k: np.asarray(got[k], float).reshape(-1) for k in FIELDS}
    fp = np.asarray(got["fp_iters"]).reshape(-1)
    dev = {"time": 0.0, "aw": 0.0}
    n_beta, n_u = len(grp["beta"]), len(grp["u"])
    assert st.shape == (n_beta * n_u,) == (len(grp["points"]),), what
    for i, pt in enumerate(grp["points"]):
        if not pt["ok"]:
            continue
        w, cls, inner = f"{what}[{i}] {pt['cls']}", pt["cls"], pt["inner"]
        eta = grp["eta"][i // n_u]
        assert int(fp[i]) == pt["fp_iters"], (w, "fp_iters", int(fp[i]), pt["fp_iters"])
        if cls == "throws":
            assert int(st[i]) == OOB | NOTCONV, (w, hex(int(st[i])))
            continue
        notconv = NOTCONV if cls in ("cap", "past_eta") else 0
        assert int(st[i]) in [s | notconv for s in STATUS_OF[inner]], (w, hex(int(st[i])))
        if inner == "run":
            assert np.isfinite([g[k][i] for k in g]).all(), w
        else:
            assert np.isnan(g["xi"][i]) and np.isnan(g["aw_max"][i]), w
            assert g["tol"][i] == (0.0 if inner == "below" else np.inf), w
        if inner == "below":
            assert g["tau_in_unc"][i] == eta and g["tau_out_unc"][i] == eta, w
        for k, a in TIMES:
            if pt[k] is not None:
                d = abs(g[a][i] - pt[k])
                dev["time"] = max(dev["time"], d)
                assert d <= TOL_TIME, (w, k, g[a][i], pt[k])
        if inner == "run":
            d = abs(g["aw_max"][i] - pt["aw_max"])
            dev["aw"] = max(dev["aw"], d)
            assert d <= TOL_AW, (w, g["aw_max"][i], pt["aw_max"])
    return dev


def forced_ode_residual(t, G, aw_old, beta, x0) -> float:
    """max |G − (1 − (1 − x0)·exp(−β ∫ aw_old))| with ∫ by the trapezoid rule on the knots t: the forced
    ODE's closed form on the returned iterate's own knots."""
    t, G, aw_old = (np.asarray(v, float) for v in (t, G, aw_old))
    S = np.concatenate([[0.0], np.cumsum(0.5 * np.diff(t) * (aw_old[1:] + aw_old[:-1]))])
    return float(np.max(np.abs(G - (1.0 - (1.0 - x0) * np.exp(-beta * S)))))


def point_of(grp: dict, i: int) -> dict:
    n_u = len(grp["u"])
    return dict(beta=grp["beta"][i // n_u], eta=grp["eta"][i // n_u], u=grp["u"][i % n_u], p=grp["p"],
                kappa=grp["kappa"], lam=grp["lam"], x0=grp["x0"], tol=grp["tol"], max_iter=grp["max_iter"])

