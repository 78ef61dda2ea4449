"""Counts aw_scan's exact AW evaluations per run point (csrc/sbr_baseline.hip) on the oracle's
knots of config-3 columns, for the shipped bounds and a variant, and checks that every variant's
maximum equals the exhaustive maximum bit for bit.  Test infrastructure / design tool (CPU).

`python tools/aw_scan_sim.py window [columns [u per column]]` compares the shipped bounds with
the scan that also stops at the peak inside the CDF's slope-monotone window (slope_window, as
the kernel's staging finds it; drawdown columns included); window_counts takes any (β, t, G)
columns, so a perturbed G can be tried before the kernel is touched."""
import bisect
import math
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "oracle"), str(REPO / "replication-social-bank-runs_amd")]
import oracle as O  # noqa: E402
import sbr  # noqa: E402


def ssl(T, x, lo=0, hi=None):
    hi = len(T) - 1 if hi is None else hi
    j = bisect.bisect_right(T, x, lo, hi + 1) - 1
    return max(j, lo)


def first_ge_down(key, hi, x):
    top, lo, step = hi, hi - 1, 1
    while lo >= 0 and key(lo) >= x:
        top = lo
        step <<= 1
        lo = top - step
    lo = max(lo, -1)
    while top - lo > 1:
        mid = (lo + top) >> 1
        if key(mid) >= x:
            top = mid
        else:
            lo = mid
    return top


def ssl_range(t, lo, hi, x):
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if t[mid] <= x:
            lo = mid
        else:
            hi = mid - 1
    return lo


def ssl_gallop(t, n, j0, x):
    """sbr_device.h's search, step for step: G is not sorted on a drawdown column"""
    lo, step = j0, 1
    while lo + step < n and t[lo + step] <= x:
        lo += step
        step <<= 1
    return ssl_range(t, lo, min(lo + step - 1, n - 1), x)


EMPTY_WINDOW = (math.inf, -math.inf, 0.0)


def slope_window(T, G):
    """The slope-monotone window as eq_column's summary pass finds it (csrc/sbr_baseline.hip):
    knots [0, wb] over which the knot-to-knot slopes d_k strictly rise (k < kc) and then strictly
    fall, each comparison strict by 2^-50 of the larger slope, so that the slopes in real
    arithmetic are monotone too.  Returns (kc, wb, (wlo, whi, wm)): the time window, shrunk by
    the rounding of a shifted argument, and the margin the scan adds to M."""
    n = len(T)
    d = []
    for k in range(n - 1):
        h = T[k + 1] - T[k]
        g = G[k + 1] - G[k]
        d.append(g / h if h != 0.0 else (math.nan if g == 0.0 or g != g else math.copysign(math.inf, g)))
    kc, wb, dmax = n - 1, n - 1, 0.0
    for k in range(n - 1):
        ad = abs(d[k])
        dmax = ad if (ad != ad or ad > dmax) and dmax == dmax else dmax
    inc_prev = True
    for k in range(1, n - 1):
        m = max(abs(d[k]), abs(d[k - 1]))
        ok = 2.0 ** -900 <= m <= 1e300
        inc = ok and d[k] - d[k - 1] > 2.0 ** -50 * m
        dec = ok and d[k - 1] - d[k] > 2.0 ** -50 * m
        if not inc:
            kc = min(kc, k)
        if (not inc and not dec) or (k >= 2 and inc and not inc_prev):
            wb = min(wb, k)
        inc_prev = inc
    if n < 2 or not dmax <= 1e300:
        return kc, wb, EMPTY_WINDOW
    span = (T[wb] + 2.0 * max(abs(T[0]), abs(T[n - 1]))) * (1.0 + 2.0 ** -40)
    du = 2.0 ** -52 * span
    wm = 2.0 ** -46 + dmax * (2.0 ** -50 * span)
    if not wm <= 1e-9:
        return kc, wb, EMPTY_WINDOW
    return kc, wb, (max(T[0], 0.0) + du, T[wb] - du, wm)


def aw_scan(T, G, n, ntau, nle, ETA, xi, icc, occ, G0, dd, c, koff, variant, win=EMPTY_WINDOW):
    """variant 0: the shipped bounds; 1, 2: the own-knot bounds of DESIGN §4d (monotone G only).
    win: slope_window's (wlo, whi, wm); the empty window is the scan without the shortcut."""
    M = 1e-14 + 4.0 * dd
    wlo, whi, wm = win
    Mw = M + wm
    wuse = occ >= icc and wlo <= whi
    tau = lambda i: T[i] if i < nle else ETA  # noqa: E731
    av_of = lambda i: (tau(i) - xi) + icc  # noqa: E731
    st = dict(ka=0, ta0=0., ta1=0., ga0=0., ga1=0., awin=0., awout=0., nev=0, mx=-np.inf, trips=0,
              inw=False, mxin=False)
    own_ok = occ == xi

    def in_own(i):
        """b_i = (t_i − ξ) + ξ is t_i exactly (Sterbenz: t_i in [ξ/2, 2ξ])"""
        return own_ok and i < nle and 0.5 * xi <= T[i] <= 2.0 * xi

    def koff_of(i):
        return 0 if (variant == 2 and in_own(i)) else koff

    def seek(x):
        k = min(ssl(T, x), n - 2)
        st.update(ka=k, ta0=T[k], ta1=T[k + 1], ga0=G[k], ga1=G[k + 1])

    def fwd(x):
        while st["ka"] < n - 2 and st["ta1"] <= x:
            k = st["ka"] + 1
            st.update(ka=k, ta0=st["ta1"], ga0=st["ga1"], ta1=T[k + 1], ga1=G[k + 1])

    def bwd(x):
        while st["ka"] > 0 and st["ta0"] > x:
            k = st["ka"] - 1
            st.update(ka=k, ta1=st["ta0"], ga1=st["ga0"], ta0=T[k], ga0=G[k])

    def exact(i, av, xa):
        ti = tau(i)
        bv = (ti - xi) + occ
        xb = bv if bv > 0 else 0.0
        kb = i if (i < nle and xb == ti) else ssl(T, xb)
        kb = min(kb, n - 2)
        tb0, tb1, gb0, gb1 = T[kb], T[kb + 1], G[kb], G[kb + 1]
        da = (xa - st["ta0"]) / (st["ta1"] - st["ta0"])
        gi = st["ga0"] * (1.0 - da) + st["ga1"] * da
        if xb == tb0:
            go = gb0 * 1.0 + gb1 * 0.0
        else:
            db = (xb - tb0) / (tb1 - tb0)
            go = gb0 * (1.0 - db) + gb1 * db
        st["inw"] = wuse and av >= wlo and bv <= whi
        st["awin"] = gi if av >= 0 else 0.0
        st["awout"] = go if bv >= 0 else 0.0
        st["nev"] += 1
        return (st["awout"] - st["awin"]) + G0

    def upd(v):
        """folds v into the maximum; True when the window's stopping rule fires: v and the
        maximum's holder both inside the window, v below it by more than the margin"""
        if v > st["mx"]:
            st["mx"] = v
            st["mxin"] = st["inw"]
            return False
        return st["inw"] and st["mxin"] and v < st["mx"] - Mw

    bv_of = lambda i: (tau(i) - xi) + occ  # noqa: E731

    def hi_own(i):
        """the variant's bound of AW_OUT(b_i) for knot i alone: G[i] when b_i = t_i exactly"""
        k2 = min(i + koff, n - 1)
        if variant == 1 and i < nle and occ == xi:
            bv = (tau(i) - xi) + occ
            if bv == tau(i):
                return G[i], k2
        return G[k2], k2

    av = av_of(c)
    xa = av if av > 0 else 0.0
    seek(xa)
    upd(exact(c, av, xa))
    kc = st["ka"]
    ub_left = st["awout"]
    LA = st["awin"]
    i = c + 1
    while i < ntau:
        st["trips"] += 1
        av = av_of(i)
        xa = av if av > 0 else 0.0
        fwd(xa)
        lb = st["ga0"] if av >= 0 else 0.0
        LA = LA if LA > lb else lb
        V = (((st["mx"] - G0) + LA) - M) - dd
        hi, k2 = hi_own(i)
        if variant == 2:
            k2 = min(i + koff_of(i), n - 1)
            hi = G[k2]
        if hi > V:
            drop = upd(exact(i, av, xa))
            LA = st["awin"]
            if drop:
                # every further knot whose b is still inside the window is below the maximum
                if bv_of(ntau - 1) <= whi:
                    break
                lo_, hi_ = i, ntau - 1  # bv_of(lo_) <= whi < bv_of(hi_)
                while hi_ - lo_ > 1:
                    mid = (lo_ + hi_) >> 1
                    if bv_of(mid) <= whi:
                        lo_ = mid
                    else:
                        hi_ = mid
                an = av_of(hi_)
                seek(an if an > 0 else 0.0)
                i = hi_
                continue
            i += 1
            continue
        if variant == 1 and G[k2] > V:  # knot i pruned by its own bound only: step past it
            i += 1
            continue
        # skip every j with G[j + koff] <= V (gallop)
        kl = ssl_gallop(G, n, k2, V)
        if kl >= n - 1:
            break
        inext = kl + 1 - koff_of(i)
        if variant == 2 and koff_of(i) == 0 and not (T[kl] <= 2.0 * xi):
            inext = max(kl + 1 - koff, i + 1)
        an = av_of(inext)
        seek(an if an > 0 else 0.0)
        i = inext
    UB = ub_left
    av = av_of(c)
    seek(av if av > 0 else 0.0)
    i = c - 1
    while i >= 0:
        st["trips"] += 1
        k2 = min(i + koff_of(i), n - 1)
        g2 = G[k2] if G[k2] > 0.0 else 0.0
        UB = UB if UB < g2 else g2
        Vp = (((UB + G0) + M) - st["mx"]) + dd
        if not (Vp - dd > 0.0):
            break
        av = av_of(i)
        xa = av if av > 0 else 0.0
        bwd(xa)
        lb = st["ga0"] if av >= 0 else 0.0
        Vi = Vp
        if variant == 1:
            h, _ = hi_own(i)
            h = h if h > 0.0 else 0.0
            ui = UB if UB < h else h
            Vi = (((ui + G0) + M) - st["mx"]) + dd
        if not (lb >= Vi):
            drop = upd(exact(i, av, xa))
            UB = UB if UB < st["awout"] else st["awout"]
            if drop:
                # every further knot whose a is still inside the window is below the maximum
                j = first_ge_down(av_of, i, wlo)
                if j == 0:
                    break
                an = av_of(j - 1)
                seek(an if an > 0 else 0.0)
                i = j - 1
                continue
            i -= 1
            continue
        if not (lb >= Vp):  # pruned by knot i's own bound only
            i -= 1
            continue
        ks = first_ge_down(lambda k: G[k], st["ka"], Vp)
        tk = T[ks]
        j = first_ge_down(av_of, i, tk)
        if j == 0:
            break
        inext = j - 1
        an = av_of(inext)
        seek(an if an > 0 else 0.0)
        i = inext
    return st["mx"], st["nev"], st["trips"]


def main(ncol=16, ustride=8):
    g = sbr.fig5_grid(2048)
    cols = np.linspace(0, 2047, ncol).astype(int)
    tot = {0: 0, 1: 0, 2: 0}
    trips = {0: 0, 1: 0, 2: 0}
    npts = 0
    for ci in cols:
        beta = g.beta[ci]
        t, G, _ = O.learn_logistic(beta, 30.0)
        n = len(t)
        if np.any(np.diff(G) < 0):
            continue  # drawdown columns: dd > 0 (kept simple here)
        T, Gl = t.tolist(), G.tolist()
        nle = bisect.bisect_right(T, 15.0)
        ntau = nle if T[nle - 1] == 15.0 else nle + 1
        lo = bisect.bisect_right(Gl, 0.5) - 1
        thalf = T[lo] + (0.5 - Gl[lo]) * (T[lo + 1] - T[lo]) / (Gl[lo + 1] - Gl[lo])
        koff = 1 if all(T[i + 1] - T[i] > 1e-15 * T[-1] for i in range(n - 1)) else 2
        for uj in range(0, 2048, ustride):
            o = O.equilibrium_paths(t, G, beta, 15.0, 30.0, g.u[uj], 0.5, 0.6, 0.01)
            if not (o["status"] & sbr.STATUS["SBR_RUN"]):
                continue
            xi, tin, tout = o["xi"], o["tau_in_unc"], o["tau_out_unc"]
            icc = xi if tin >= xi else tin
            occ = xi if tout > xi else tout
            tstar = thalf + 0.5 * ((xi - icc) + (xi - occ))
            c = ssl(T, max(tstar, T[0]), 0, max(nle, 1) - 1)
            c = min(c, ntau - 1)
            for v in (0, 1, 2):
                mx, nev, tr = aw_scan(T, Gl, n, ntau, nle, 15.0, xi, icc, occ, Gl[0], 0.0, c, koff, v)
                assert mx == o["aw_max"], (ci, uj, v, mx, o["aw_max"])
                tot[v] += nev
                trips[v] += tr
            npts += 1
    print(f"{npts} run points: exact evaluations per point shipped {tot[0] / npts:.2f}, "
          f"own-knot bound {tot[1] / npts:.2f}, own-knot run bounds {tot[2] / npts:.2f}; loop trips "
          f"{trips[0] / npts:.2f} / {trips[1] / npts:.2f} / {trips[2] / npts:.2f}")


def column_setup(t, G, eta=15.0):
    """What the kernel's staging derives from a column's knots: the τ̄ grid, t_half, the scan's
    preconditions and drawdown bound (Summ::scan, dd, koff) and the slope-monotone window."""
    T, Gl = [float(x) for x in t], [float(x) for x in G]
    n = len(T)
    nle = bisect.bisect_right(T, eta)
    ntau = nle if nle > 0 and T[nle - 1] == eta else nle + 1
    thalf = math.nan
    if n >= 2 and Gl[0] <= 0.5 < Gl[-1]:
        lo, hi = 0, n - 1
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if Gl[mid] <= 0.5:
                lo = mid
            else:
                hi = mid
        thalf = T[lo] + (0.5 - Gl[lo]) * (T[hi] - T[lo]) / (Gl[hi] - Gl[lo])
    sep = 1e-15 * T[-1]
    far = all(T[i + 2] - T[i] > sep for i in range(n - 2))
    koff = 1 if all(T[i + 1] - T[i] > sep for i in range(n - 1)) else 2
    decs = [Gl[i] - Gl[i + 1] for i in range(n - 1) if Gl[i + 1] < Gl[i]]
    dd = len(decs) * max(decs) if decs else 0.0
    scan = n >= 2 and far and dd <= 1e-12 and Gl[0] >= 0.0 and Gl[-1] <= 2.0 and not any(g != g for g in Gl)
    kc, wb, win = slope_window(T, Gl)
    return dict(T=T, G=Gl, n=n, nle=nle, ntau=ntau, eta=eta, thalf=thalf, koff=koff, dd=dd, scan=scan, kc=kc, wb=wb,
                win=win)


def scan_point(col, xi, tin, tout, win):
    """aw_scan as solve_from_buffers calls it for a run point (ξ and the buffer times are the
    oracle's); None where the kernel takes another path (τ* off the τ̄ grid, Summ::scan false)."""
    T, n, ntau, nle, eta = col["T"], col["n"], col["ntau"], col["nle"], col["eta"]
    icc = xi if tin >= xi else tin
    occ = xi if tout > xi else tout
    tau = lambda i: T[i] if i < nle else eta  # noqa: E731
    tstar = col["thalf"] + 0.5 * ((xi - icc) + (xi - occ))
    if not (col["scan"] and tstar == tstar and tau(0) <= tstar <= tau(ntau - 1)):
        return None
    c = min(ssl(T, max(tstar, T[0]), 0, max(nle, 1) - 1), ntau - 1)
    G0 = col["G"][0] if T[0] == 0.0 else float(np.interp(0.0, T, col["G"]))
    return aw_scan(T, col["G"], n, ntau, nle, eta, xi, icc, occ, G0, col["dd"], c, col["koff"], 0, win)


def window_counts(columns, us, eta=15.0, t_end=30.0, check=None):
    """Runs the shipped scan and the windowed one over (β, t, G) columns x the u values.  Every
    maximum is asserted equal to the oracle's on the same knots (and to check(col, o), if given).
    Returns the totals: points, exact evaluations and bound trips of each scan, and the windows."""
    r = dict(points=0, exact=[0, 0], bound=[0, 0], windows=[])
    for beta, t, G in columns:
        col = column_setup(t, G, eta)
        r["windows"].append((col["kc"], col["wb"], col["n"], col["win"], col["dd"]))
        ta, Ga = np.asarray(col["T"]), np.asarray(col["G"])
        for u in us:
            o = O.equilibrium_paths(ta, Ga, beta, eta, t_end, u, 0.5, 0.6, 0.01)
            if not (o["status"] & sbr.STATUS["SBR_RUN"]):
                continue
            res = [scan_point(col, o["xi"], o["tau_in_unc"], o["tau_out_unc"], w) for w in (EMPTY_WINDOW, col["win"])]
            if res[0] is None:
                continue
            for k, (mx, nev, tr) in enumerate(res):
                assert mx == o["aw_max"], (beta, u, k, mx, o["aw_max"])
                if check is not None:
                    assert mx == check(col, o), (beta, u, k)
                r["exact"][k] += nev
                r["bound"][k] += tr - (nev - 1)
            r["points"] += 1
    return r


def main_window(ncol=24, nu=64):
    """Shipped scan against the windowed one on config-3 columns, drawdown columns included."""
    g = sbr.fig5_grid(2048)
    cols = np.linspace(0, 2047, ncol).astype(int)
    columns = [(g.beta[ci],) + tuple(O.learn_logistic(g.beta[ci], 30.0)[:2]) for ci in cols]
    us = g.u[np.linspace(0, 2047, nu).astype(int)]
    r = window_counts(columns, us)
    n = max(r["points"], 1)
    short = [w[2] - 1 - w[1] for w in r["windows"]]
    print(f"{r['points']} run points on {ncol} columns ({sum(w[4] > 0 for w in r['windows'])} with dd > 0): "
          f"exact evaluations per point shipped {r['exact'][0] / n:.2f}, window {r['exact'][1] / n:.2f}; bound trips "
          f"{r['bound'][0] / n:.2f} / {r['bound'][1] / n:.2f}; window ends {min(short)}-{max(short)} knots short of "
          f"the last knot, margin up to {max(w[3][2] for w in r['windows']):.2e}")
    return r


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "window":
        main_window(*(int(a) for a in sys.argv[2:]))
    else:
        main(*(int(a) for a in sys.argv[1:]))
