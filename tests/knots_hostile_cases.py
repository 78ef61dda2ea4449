"""Caller knots that put the equilibrium kernel's pruning guards (csrc/sbr_eq_column_body.h: s_nonmono,
s_noscan, s_near1, the drawdown product, the G range test, the slope window, Summ::bnb, the crossing
tables, `moderate`, `rcp_ok`) on the side the learned logistic CDFs never reach (not a test module).

Every case is a legal input of sbr_equilibrium_on_knots[_pdf] whose answer the oracle defines: the
clean column learn_logistic(1, 30) (2,848 knots, 2,308 hazard entries at η = 15) with knots inserted,
values replaced, times repeated, an explicit pdf, u tied to hazard values, or the time axis rescaled.
``stats`` restates the kernel's summary pass in numpy and ``branch`` the AW_max dispatch that follows
from it; each case carries the ``premise`` on those statistics it is named for and the dispatch it
must take (``expect``).  tests/test_knots_hostile.py checks premises and class counts on the oracle
alone, tests/test_gpu_knots_hostile.py holds the kernels to the oracle bit for bit."""
import numpy as np

P0 = dict(beta=1.0, eta=15.0, t_end=30.0, p=0.5, kappa=0.6, lam=0.01)
U0 = np.linspace(0.001, 0.3, 64)
FIELDS = ("xi", "tau_in_unc", "tau_out_unc", "aw_max", "tol")

RUN, CONVERGED, BELOW, COLLAPSE, MAXITER, FALSE_EQ, OOB = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x80


# ------------------------------------------------------------------------------------------------
# the summary pass and the dispatch, restated
def stats(t, G) -> dict:
    """The equilibrium kernel's per-column statistics, as its summary pass computes them."""
    t, G = np.asarray(t, float), np.asarray(G, float)
    n = len(t)
    with np.errstate(invalid="ignore"):
        dec = G[1:] < G[:-1]  # false on NaN, as in the kernel
        drop = np.where(dec, G[:-1] - G[1:], 0.0)
    ndec = int(dec.sum())
    maxdec = float(drop.max()) if n > 1 else 0.0
    sep = 1e-15 * t[-1]
    nan = bool(np.isnan(G).any())
    return dict(n=n, ndec=ndec, maxdec=maxdec, dd=ndec * maxdec, sep=sep, nan=nan,
                nonmono=ndec > 0 or nan,
                noscan=nan or bool(n > 2 and (t[2:] - t[:-2] <= sep).any()),
                near1=bool(n > 1 and (t[1:] - t[:-1] <= sep).any()),
                range_ok=bool(n >= 2 and G[0] >= 0.0 and G[-1] <= 2.0))


def branch(s: dict) -> str:
    """AW_max's dispatch for a column that fits the LDS slab (sbr_eq_dev.h, `!(scan || S.bnb)`):
    "exhaustive" where the column's statistics alone send every run point through eval_range(0, ntau),
    "pruned" where they admit the scan or the branch and bound."""
    bnb = (not s["nonmono"]) or s["noscan"]
    scan = s["n"] >= 2 and not s["noscan"] and s["dd"] <= 1e-12 and s["range_ok"]
    return "pruned" if (bnb or scan) else "exhaustive"


# ------------------------------------------------------------------------------------------------
# knot surgery
def insert_after(t, G, picks, make):
    """t / G with the knots make(k) = [(time, value), ...] after each index k in ``picks``.  Returns t, G
    and, per pick, the index of its first new knot."""
    picks = set(int(k) for k in picks)
    tn, Gn, idx = [], [], []
    for k in range(len(t)):
        tn.append(t[k])
        Gn.append(G[k])
        if k in picks:
            idx.append(len(tn))
            for tv, gv in make(k):
                tn.append(tv)
                Gn.append(gv)
    return np.asarray(tn), np.asarray(Gn), np.asarray(idx)


def decreases(t, G, picks, d):
    """One real decrease of d per pick: a knot halfway to the next one with the value G[k] − d."""
    tn, Gn, _ = insert_after(t, G, picks, lambda k: [(t[k] + 0.5 * (t[k + 1] - t[k]), G[k] - d)])
    return tn, Gn


def crowd(t, G, picks, sep, extra=1):
    """tests/test_gpu_knots._crowd with ``extra`` knots per pick, the last one sep·t[n−1] after it, G
    just above its left neighbour's, and the index of each pick's first new knot.  One extra knot
    below the 1e-15·t[n−1] separation sets s_near1 only; two put knots i and i + 2 within it (s_noscan)."""
    return insert_after(t, G, picks, lambda k: [(t[k] + (r / extra) * sep * t[-1], G[k] + (G[k + 1] - G[k]) * 1e-3 * r)
                                                for r in range(1, extra + 1)])


def refine(t, G, pdf=None):
    """The grid with every interval's midpoint added (2n − 1 knots: past the LDS slab)."""
    def mid(v):
        out = np.empty(2 * len(v) - 1)
        out[0::2], out[1::2] = v, 0.5 * (v[:-1] + v[1:])
        return out

    return mid(t), mid(G), None if pdf is None else mid(pdf)


# ------------------------------------------------------------------------------------------------
def solve(O, c: dict, u: float, t=None, G=None, pdf=None) -> dict:
    """The oracle's answer with paths for one u of case c (on other knots where given)."""
    t = c["t"] if t is None else t
    G = c["G"] if G is None else G
    pdf = c["pdf"] if pdf is None else pdf
    a = (c["eta"], c["t_end"], float(u), c["p"], c["kappa"], c["lam"])
    if pdf is None:
        return O.equilibrium_paths(t, G, c["beta"], *a)
    return O.equilibrium_paths_pdf(t, G, pdf, *a)


def classes(status) -> tuple:
    """(run or false equilibrium, HR below u, collapse, iteration cap, anything else) counts."""
    st = np.asarray(status, np.uint32)
    run = ((st & (RUN | FALSE_EQ)) != 0)
    below = (st & BELOW) != 0
    col = (st & COLLAPSE) != 0
    mxi = (st & MAXITER) != 0
    other = ~(run | below | col | mxi)
    return tuple(int(x.sum()) for x in (run, below, col, mxi, other))


def run_spacings(O, c: dict, refined=False) -> np.ndarray:
    """ε = the knot spacing at ξ of every run point of case c (the divisor of the bisection's register
    loop B, which takes the refined reciprocal only for ε in [2^-64, 2^64])."""
    knots = refine(c["t"], c["G"], c["pdf"]) if refined else (c["t"], c["G"], c["pdf"])
    xi = np.array([solve(O, c, u, *knots)["xi"] for u in c["u"]])
    j = np.searchsorted(knots[0], xi[~np.isnan(xi)], side="right") - 1
    return knots[0][j + 1] - knots[0][j]


def bisect_marks(t, G, tin, tout, kappa, stop=90) -> tuple:
    """compute_ξ on an ordered bracket tin <= tout, restated far enough to date two events of a lane:
    S, the iteration whose update first leaves [ξmin, ξmax] inside one knot interval with ξmax + ε on the
    grid (the kernel's `single`), and K, the iteration whose update makes the next iterate 0.5·(ξ + ξmax)
    infinite.  None where the lane ends first (within ``stop`` iterations)."""
    import bisect
    t, G = [float(x) for x in t], [float(x) for x in G]
    n = len(t)

    def ssl(x):
        return bisect.bisect_right(t, x) - 1

    def lerp(x):
        j = min(max(ssl(x), 0), n - 2)
        d = (x - t[j]) / (t[j + 1] - t[j])
        return G[j] * (1.0 - d) + G[j + 1] * d

    tin, tout = float(tin), float(tout)
    xmin, xmax, xo = tin, tout, (tin + tout) / 2.0
    jlo, jhi, Gin, S = ssl(xmin), ssl(xmax), lerp(tin), None
    for it in range(1, stop + 1):
        j = ssl(xo)
        if xmin == xmax or j + 1 >= n:
            break
        eps = t[j + 1] - t[j]
        err = (lerp(min(tout, xo)) - Gin) - kappa
        if abs(err) <= 10.0 * np.spacing(kappa):
            break
        if err > 0:
            xmax, jhi, xo = xo, j, 0.5 * (xo + xmin)
        else:
            xmin, jlo, xo = xo, j, 0.5 * (xo + xmax)
        if S is None and jlo == jhi and eps > 0.0 and xmax + eps <= t[-1]:
            S = it
        if xo == float("inf"):
            return S, it
    return S, None


def late_overflows(O, c: dict) -> list:
    """The points of case c (one wave: 64 consecutive u) whose midpoint overflows only after every lane
    of the wave still iterating holds its bracket inside one knot interval — where a wave that took the
    grid for one of moderate size would already iterate on registers.  Each must end in the reference's
    BoundsError in the iterate after the overflow."""
    res = [solve(O, c, u) for u in c["u"]]
    marks = [bisect_marks(c["t"], c["G"], r["tau_in_unc"], r["tau_out_unc"], c["kappa"]) if r["iters"] else (None, None)
             for r in res]
    late = []
    for j, (r, (S, K)) in enumerate(zip(res, marks)):
        if K is None:
            continue
        assert r["status"] == OOB and r["iters"] == K + 1, (j, hex(r["status"]), r["iters"], K)
        # the wave leaves the reference's loop after the first iteration W at which every lane that has not
        # ended (iters > W) is `single`
        W = next((w for w in range(1, K + 1)
                  if all(s is not None and s <= w for (s, _), q in zip(marks, res) if q["iters"] > w)), None)
        if W is not None:
            late.append(j)
    return late


def cases(O) -> list:
    t, G, _ = O.learn_logistic(1.0, 30.0)
    n = len(t)
    m = int(np.searchsorted(t, P0["eta"], side="right"))  # knots <= η
    sym = (1.0 * G) * (1.0 - G)
    out = []

    def add(name, tv=t, Gv=G, pdf=None, premise=lambda s: True, expect="any", cap=True, gmem=False, **kw):
        c = dict(P0, name=name, t=np.ascontiguousarray(tv, float), G=np.ascontiguousarray(Gv, float),
                 pdf=None if pdf is None else np.ascontiguousarray(pdf, float), u=U0.copy(), premise=premise,
                 expect=expect, cap=cap, gmem=gmem)
        c.update(kw)
        out.append(c)
        return c

    add("clean", premise=lambda s: s["ndec"] == 0 and not s["noscan"] and not s["near1"], expect="pruned")

    # ---- the drawdown bound dd = ndec·maxdec <= 1e-12, both sides
    k = n // 2
    for name, d, above in (("dd_below", 0.9e-12, False), ("dd_above", 1.1e-12, True)):
        tv, Gv = decreases(t, G, [k], d)
        add(name, tv, Gv, gmem=above, expect="exhaustive" if above else "pruned",
            premise=lambda s, above=above: s["ndec"] == 1 and (s["dd"] > 1e-12) == above and not s["noscan"])

    # ---- many decreases, each below the bound, their product above it
    many = list(range(200, n - 200, 4))[:600]
    tm, Gm = decreases(t, G, many, 1e-11)
    # (G[k] − (G[k] − d) is d up to one rounding of G <= 1)
    add("small_decs", tm, Gm, expect="exhaustive", premise=lambda s: s["ndec"] == 600
        and s["maxdec"] <= 1e-12 * 10 + 2.0 ** -52 and s["dd"] > 1e-12 and not s["noscan"])
    Gd = Gm.copy()
    Gd[1300:1500] -= 0.05  # a dip inside the slope window
    add("small_decs_dip", tm, Gd, expect="exhaustive",
        premise=lambda s: s["ndec"] == 601 and s["dd"] > 1e-12 and not s["noscan"])

    # ---- non-monotone and no-scan: the 8-knot prefix-max / suffix-min tables.  One crowded knot per pick
    # (test_gpu_knots._crowd) sets s_near1 alone: knots i and i + 2 of a sorted grid are never closer than
    # i and i + 1, so s_noscan by spacing needs two (and "noscan without near1" exists only through a NaN)
    picks = range(200, n - 200, 37)
    for name, sep, extra in (("nonmono_crowded", 0.5e-15, 2), ("nonmono_near1", 0.5e-15, 1),
                             ("nonmono_spaced", 2e-15, 1)):
        tc, Gc, idx = crowd(t, G, picks, sep, extra)
        Gc[idx[::11]] -= 1e-6
        near, nosc = sep < 1e-15, extra == 2
        add(name, tc, Gc, gmem=nosc, expect="pruned" if nosc else "exhaustive",
            premise=lambda s, near=near, nosc=nosc: s["ndec"] > 0 and s["noscan"] == nosc and s["near1"] == near
            and s["dd"] > 1e-12)
    # the same with every 13th 8-knot block of G halved: there a block's own min is far from the suffix min
    # over the blocks, so tables left as block extremes would bound AW_cum below its value
    tc, Gs, idx = crowd(t, G, picks, 0.5e-15, 2)
    Gs[idx[::11]] -= 1e-6
    for g in np.arange(40, len(tc) // 8 - 40, 13):
        Gs[8 * g:8 * g + 8] *= 0.5
    add("nonmono_crowded_notches", tc, Gs, expect="pruned",
        premise=lambda s: s["ndec"] >= 20 and s["noscan"] and s["near1"] and s["maxdec"] > 0.25)

    # ---- NaN in G: beyond every lookup, at the tail, in the middle; alone and with the decreases above
    for base, tb, Gb in (("", t, G), ("_decs", tm, Gm)):
        mb = int(np.searchsorted(tb, P0["eta"], side="right"))
        for name, i, runs in (("nan_past_eta", mb + 50, True), ("nan_tail", len(tb) - 3, True),
                              ("nan_mid", len(tb) // 2, False)):
            Gn = Gb.copy()
            Gn[i] = np.nan
            add(name + base, tb, Gn, cap=runs, gmem=(name == "nan_past_eta" and not base),
                premise=lambda s: s["nan"] and s["noscan"] and s["nonmono"], expect="pruned")

    # ---- the G range test sG[0] >= 0 && sG[n−1] <= 2
    add("G_minus", Gv=G - 0.01, premise=lambda s: not s["range_ok"] and s["ndec"] == 0, expect="pruned")
    add("G_times_2p5", Gv=2.5 * G, premise=lambda s: not s["range_ok"] and s["ndec"] == 0, expect="pruned")
    Gh = G.copy()
    Gh[0] = 0.6  # one decrease of 0.6 at the first knot, G[0] > 1/2: no t_half
    add("G0_high", Gv=Gh, premise=lambda s: s["ndec"] == 1 and s["dd"] > 0.5 and not s["noscan"], expect="exhaustive")
    # never reaches 1/2: t_half is NaN, the branch and bound descends its 256/64/8 hierarchy unpredicted
    # (κ = 0.2: AW_cum cannot reach 0.6 on a G below 0.45)
    add("G_capped", Gv=np.minimum(G, 0.45), kappa=0.2, expect="pruned",
        premise=lambda s: s["ndec"] == 0 and s["range_ok"] and not s["noscan"])

    # ---- repeated knot times (zero-width intervals), flat G
    def rep(name, pairs, **kw):
        tv = t.copy()
        for dst, src in pairs:
            tv[dst] = t[src]
        assert np.all(np.diff(tv) >= 0)
        add(name, tv, premise=lambda s: s["near1"] and not s["noscan"] and s["ndec"] == 0, expect="pruned", **kw)

    kp = int(np.searchsorted(t, 11.0))
    rep("t_rep_300", [(300, 301)])
    rep("t_rep_first", [(1, 0)])
    rep("t_rep_last", [(n - 2, n - 1)], gmem=True)
    tv = t.copy()
    tv[kp + 1] = tv[kp + 2] = t[kp]
    add("t_rep3_peak", tv, premise=lambda s: s["near1"] and s["noscan"] and s["ndec"] == 0, expect="pruned")
    Gp = G.copy()
    Gp[1400:1420] = G[1400]
    add("G_plateau", Gv=Gp, premise=lambda s: s["ndec"] == 0 and not s["near1"], expect="pruned")

    # ---- hazard shapes by an explicit pdf
    add("pdf_fast_sin", pdf=sym * (1.0 + 0.9 * np.sin(40.0 * t)), gmem=True, expect="pruned")
    # the hazard starts above the low u and dips below within the first period: optimal_buffer's scans from
    # an interior start (the first 0→1 pair after the first drop, the last 1→0 pair before the last rise)
    add("pdf_starts_high", pdf=(sym + 0.03) * (1.0 + 0.9 * np.cos(40.0 * t)), expect="pruned")
    add("pdf_slow_sin", pdf=sym * (1.0 + 0.5 * np.sin(3.0 * t)), expect="pruned")
    pn = sym.copy()
    pn[:200] = -pn[:200]
    add("pdf_neg_head", pdf=pn, expect="pruned")
    for name, i, runs in (("pdf_nan_past_eta", m + 50, True), ("pdf_nan_before_eta", m // 2, False)):
        pv = sym.copy()
        pv[i] = np.nan
        add(name, pdf=pv, cap=runs, expect="pruned")
    pv = sym.copy()
    pv[[400, 1200, m - 5]] = np.inf
    add("pdf_inf3", pdf=pv, cap=False, expect="pruned")

    # ---- u equal to hazard values, and one ulp either side
    hr = solve(O, out[0], 0.1)["hr"]
    ties = hr[np.linspace(50, len(hr) - 2, 64).astype(int)].copy()
    add("ties", u=ties, gmem=True, expect="pruned", premise=lambda s, hr=hr, ties=ties: np.isin(ties, hr).all())
    add("ties_up", u=np.nextafter(ties, np.inf), expect="pruned")
    add("ties_down", u=np.nextafter(ties, -np.inf), expect="pruned")
    # u equal to a 64-entry block's largest / smallest hazard value: the equalities the block summaries
    # (hmax > u, hmin > u and their prefix / suffix tables) decide, not only the in-block scans
    nbh = (len(hr) + 63) // 64
    ext = [64 * b + int(np.argmax(hr[64 * b:64 * b + 64])) for b in range(nbh)]
    ext += [64 * b + int(np.argmin(hr[64 * b:64 * b + 64])) for b in np.linspace(0, nbh - 1, 64 - nbh).astype(int)]
    tb = hr[ext].copy()
    add("ties_blocks", u=tb, expect="pruned", premise=lambda s, tb=tb: len(tb) == 64 and np.isin(tb, hr).all())

    # ---- the time axis rescaled by 2^e (an explicit pdf scales as 1/s): out of rcp_ok, out of moderate,
    # down to the 2^-840 / 2^-900 tests.  The knot spacing at the run points' ξ is 0.0053 to 0.0118, half
    # that on the refined grid: ε·2^70 stays below 2^64 (the last scale inside rcp_ok), ε·2^74 is above it
    # on both grids, ε·2^-70 below 2^-64
    def scaled(e, inside, **kw):
        s = 2.0 ** e if e < 1000 else 2.0 ** 1000 * 2.0 ** (e - 1000)
        c = add(f"scale_2^{e}", t * s, G, pdf=sym / s, eta=P0["eta"] * s, t_end=P0["t_end"] * s, u=U0 / s,
                lam=P0["lam"] / s, expect="pruned", **kw)

        def premise(st):
            eps = [run_spacings(O, c)] + ([run_spacings(O, c, refined=True)] if c["gmem"] and not inside else [])
            return (np.isfinite(c["t"]).all() and (np.diff(c["t"]) > 0).all() and all(len(x) >= 16 for x in eps)
                    and all((((x >= 2.0 ** -64) & (x <= 2.0 ** 64)) == inside).all() for x in eps))

        c["premise"] = premise

    scaled(-1000, False)
    scaled(-70, False)
    scaled(70, True, gmem=True)
    scaled(74, False, gmem=True)
    scaled(1001, False)

    # a grid near the top of the number range: 2^1019·30 is finite, the sum of two times past 16·2^1020 is
    # not, so ξ = (τ̄_IN + τ̄_OUT)/2 or a later midpoint 0.5·(ξ + ξmax) is +Inf where the buffers end late
    # (the reference's searchsortedlast(grid, Inf) + 1 is its BoundsError).  A pdf that stays high up to
    # t = 24 keeps τ̄_OUT there; the low u enter early and bisect downward (they run), the others enter at
    # the step at 9.5 and overflow in iterate 1, 2, 3 or 5
    s = 2.0 ** 1019
    pv = np.where(t < 9.5, np.minimum(sym, 0.1), 0.4)
    pv[t > 24.0] = 0.0
    uv = np.concatenate([np.linspace(0.0005, 0.012, 32), np.linspace(0.0125, 0.055, 32)])
    add("scale_2^1019_overflow", t * s, G, pdf=pv / s, eta=25.0 * s, t_end=P0["t_end"] * s, u=uv / s,
        lam=P0["lam"] / s, expect="pruned", premise=lambda st, s=s: np.isfinite(t * s).all() and t[-1] * s >= 2.0 ** 1023)
    # the same grid with the overflow late: the hazard drops to 0 across the knot interval [t0, t1) that
    # holds 16 (2^1023 after scaling), so τ̄_OUT = t1 − (u/h0)·(t1 − t0) and the u below place it at 16 + δ,
    # δ from 2^-30 to 2^-9.  These points enter at the step (τ̄_IN ≈ 9.5, G(τ̄_IN) > 1 − κ: no root), every
    # iterate moves up, and ξ + ξmax reaches 2^1024 only once ξ >= 16 − δ, iterations after [ξmin, ξmax] has
    # come to lie inside [t0, t1).  A wave that took this grid for one of moderate size would by then
    # iterate on registers (loop B), where nothing looks the infinite iterate up; the reference does, and
    # throws.  24 low u enter early and run, 12 high u leave before 16 and climb to the iteration cap
    k = int(np.searchsorted(t, 16.0, side="right")) - 1
    pv = np.where(t < 9.5, np.minimum(sym, 0.1), 0.4)
    pv[k + 1:] = 0.0
    h0 = solve(O, dict(P0, t=t, G=G, pdf=pv, eta=25.0), 0.01)["hr"][k]
    delta = 2.0 ** np.linspace(-30.0, -9.0, 28)
    uv = np.concatenate([np.linspace(0.0005, 0.029, 24), h0 * ((t[k + 1] - 16.0 - delta) / (t[k + 1] - t[k])),
                         np.linspace(0.0505, 0.11, 12)])
    c = add("scale_2^1019_late_overflow", t * s, G, pdf=pv / s, eta=25.0 * s, t_end=P0["t_end"] * s, u=uv / s,
            lam=P0["lam"] / s, expect="pruned")
    c["premise"] = lambda st, c=c, s=s, k=k: t[k] * s < 2.0 ** 1023 < t[k + 1] * s and len(late_overflows(O, c)) >= 8

    # ---- tiny grids.  On two knots ε is the whole grid, so ξ + ε leaves it for every ξ > t[0]: no point
    # can run.  The class cap is therefore lifted for n = 2 as it is for n = 1 (for which alone it was
    # lifted when these cases were specified); the CPU test asserts that none of their points runs
    add("n1", t[:1], G[:1], cap=False, premise=lambda s: s["n"] == 1)
    add("n2", np.array([0.0, 30.0]), np.array([1e-4, 1.0]), cap=False, eta=30.0, premise=lambda s: s["n"] == 2)
    add("n2_equal", np.array([15.0, 15.0]), np.array([1e-4, 1.0]), cap=False, premise=lambda s: s["near1"])

    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


NAMES = ["clean", "dd_below", "dd_above", "small_decs", "small_decs_dip", "nonmono_crowded", "nonmono_near1",
         "nonmono_spaced", "nonmono_crowded_notches", "nan_past_eta", "nan_tail", "nan_mid",
         "nan_past_eta_decs", "nan_tail_decs", "nan_mid_decs", "G_minus", "G_times_2p5", "G0_high", "G_capped",
         "t_rep_300", "t_rep_first", "t_rep_last", "t_rep3_peak", "G_plateau", "pdf_fast_sin", "pdf_starts_high", "pdf_slow_sin",
         "pdf_neg_head", "pdf_nan_past_eta", "pdf_nan_before_eta", "pdf_inf3", "ties", "ties_up", "ties_down", "ties_blocks",
         "scale_2^-1000", "scale_2^-70", "scale_2^70", "scale_2^74", "scale_2^1001", "scale_2^1019_overflow",
         "scale_2^1019_late_overflow", "n1", "n2", "n2_equal"]
