// sbr_eq_dev.h — the equilibrium stage of one learning column by one workgroup: solve_point /
// solve_from_buffers (optimal_buffer, compute_ξ, get_AW + AW_max per lane), the interest-rate
// extension's value function, and eq_column (knots staged in LDS, block summaries, the point loop),
// shared by the sweep kernels (sbr_baseline.hip) and the economic-parameter sweep (sbr_econ.hip).
// Device code; include from a .hip file.
#pragma once

#include "sbr_device.h"
#include "sbr_hazard_dev.h"
#include "sbr_kernels.h"
#include "sbr_ode.h"
#include "sbr_scan.h"
#include "sbr_solve_dev.h"

namespace sbr {

template <class P>
__device__ __forceinline__ void solve_point(P T, P G, P H, const Summ& S, const int n, const int ntau,
                                            const int nle, const double ETA, const double T1, const bool trunc,
                                            const double u, const double kappa, const int max_iters,
                                            const uint32_t lbits, PointResult& r, double* __restrict__ aw_path,
                                            const int diag)
{
    r.xi = NAN; r.aw = NAN; r.tol = INFINITY; r.iters = 0; r.status = 0;
    (void)0;

    // ---------------- optimal_buffer: crossings of HR(τ̄) with u ----------------
    bool any, all;
    int fa, la, cin, cout;
    if (S.hpm) {
        buffer_scan_bs(H, S, S.hpm, S.hpn, S.hsm, S.hsn, S.nbh, ntau, u, any, all, fa, la, cin, cout);
    } else if (S.hmax) {
        buffer_scan_blocked(H, S, ntau, u, any, all, fa, la, cin, cout);
    } else {
        any = false; all = true;
        bool prev = false;
        fa = la = cin = cout = -1;
        for (int i = 0; i < ntau; i++) {
            const bool ab = H[i] > u;
            any |= ab;
            all &= ab;
            if (ab) { if (fa < 0) fa = i; la = i; }
            if (i > 0) {
                if (!prev && ab && cin < 0) cin = i - 1;
                if (prev && !ab) cout = i - 1;
            }
            prev = ab;
        }
    }
    auto tau = [&](int i) -> double { return i < nle ? T[i] : ETA; };
    double tin, tout;
    if (!any) {
        tin = T1; tout = T1;
    } else if (all) {
        tin = tau(0); tout = tau(ntau - 1);
    } else {
        tin = T1; tout = T1;
        if (cin >= 0) {
            const double t0 = tau(cin), t1 = tau(cin + 1), h0 = H[cin], h1 = H[cin + 1];
            tin = t0 + ((u - h0) * (t1 - t0)) / (h1 - h0);
        }
        if (cout >= 0) {
            const double t0 = tau(cout), t1 = tau(cout + 1), h0 = H[cout], h1 = H[cout + 1];
            tout = t0 + ((u - h0) * (t1 - t0)) / (h1 - h0);
        }
        if (tin == T1) tin = tau(fa);
        if (tout == T1) tout = tau(la);
    }
    r.tin = tin;
    r.tout = tout;
    if (diag & 1) return;
    solve_from_buffers(T, G, H, S, n, ntau, nle, ETA, T1, trunc, u, kappa, max_iters, lbits, r, aw_path, diag,
                       tin, tout);
}

// solve_equilibrium_baseline from the buffer times on (solver.jl:429-462) + get_AW / AW_max:
// no run if τ̄_IN == τ̄_OUT, else compute_ξ on G and AW_max on the τ̄ grid.
template <class P>
__device__ __forceinline__ void solve_from_buffers(P T, P G, P H, const Summ& S, const int n, const int ntau,
                                                   const int nle, const double ETA, const double T1, const bool trunc,
                                                   const double u, const double kappa, const int max_iters,
                                                   const uint32_t lbits, PointResult& r, double* __restrict__ aw_path,
                                                   const int diag, const double tin, const double tout)
{
    const double tlo = T[0], thi = T[n - 1];
    auto tau = [&](int i) -> double { return i < nle ? T[i] : ETA; };
    if (tin == tout) {
        r.status = SBR_NO_RUN_HR_BELOW_U | SBR_CONVERGED | lbits;
        r.tol = 0.0;
        return;
    }

    // ---------------- compute_ξ: bisection with bracketed lookups ----------------
    uint32_t flag = 0;
    const double tolerance = 10.0 * sbr_jl_eps(kappa);
    double xnew = (tin + tout) / 2.0, xmin = tin, xmax = tout;
    const bool okmin = in_range(xmin, tlo, thi, trunc, flag);
    const bool okmax = in_range(xmax, tlo, thi, trunc, flag);
    if (!okmin || !okmax) {
        // a buffer outside the grid (NaN from a NaN or zero-width hazard bracket): the BoundsError of the
        // reference's first iteration, after that iteration's collapse and iteration-cap tests
        if (max_iters >= 1) {
            r.iters = 1;
            r.status = (collapsed(xmin - xmax) ? SBR_NO_RUN_COLLAPSE : max_iters == 2 ? SBR_NO_RUN_MAXITER : flag) | lbits;
        } else {
            r.status = SBR_NO_RUN_MAXITER | lbits;
        }
        return;
    }
    int jlo = ssl_range(T, 0, n - 1, xmin);
    int jhi = ssl_range(T, 0, n - 1, xmax);
    const int jtin = jlo;
    double c_ic_x = NAN, c_ic_v = 0.0;
    uint32_t s = SBR_NO_RUN_MAXITER;
    double xi = NAN, tolr = INFINITY;
    // The bisection runs in two loops.
    // Loop A is the reference's iteration, every lookup bracketed by [jlo, jhi].  Once a lane's
    // bracket is one knot interval [t0, t1) (jlo == jhi) and the tests below hold, every later
    // iterate of that lane is decided by constants (`single`): ξmin and ξmax only move inward,
    // so tin ≤ ξmin ≤ ξ ≤ ξmax ≤ tout gives ic = tin and oc = ξ (in range, as tin and tout are),
    // the search over [jlo, jhi] returns j = jlo, ε = t1 − t0, G(ic) is the cached G(tin), and the
    // BoundsError tests pass: tin + ε was tested by the iteration that set `single`, and
    // tlo ≤ ξ + ε ≤ ξmax + ε ≤ thi because rounding is monotone.  A `single` lane that stays in
    // loop A runs the same operations as before.
    // When every lane of the wave still iterating is `single`, the wave moves to loop B, which
    // iterates on registers alone: δ = (ξ − t0)/ε, G(ξ) = g0·(1 − δ) + g1·δ, err = (G(ξ) − G(tin)) − κ,
    // the same operations in the reference's order, without the search, the range tests or LDS.
    // A wave holding a lane that never becomes `single` (a bracket at the end of the grid, NaN
    // buffers) stays in loop A until that lane terminates.  Iteration counts, ξ and every status
    // bit are the reference's.
    // Both arguments need midpoints that stay inside [ξmin, ξmax]: 0.5·(a + b) does for a <= b
    // (monotone rounding) unless a + b overflows, so the grid has to be of moderate size.
    // Loop A itself is specialised for an ordered bracket (ORD: tin <= tout on a moderate grid,
    // every lane of the wave): there tin = ξmin <= ξ <= ξmax = tout from the first iterate on, so
    // ic = tin and oc = ξ, both pass their range tests (tin and tout did), G(oc) is looked up
    // at j and G(ic) = G(tin) once; the ε probes' range tests stay (they fail near the end of the
    // grid).  Any other wave (a last 1→0 crossing before the first 0→1 one) runs the iteration as
    // the reference writes it.
    const bool moderate = tlo >= -0x1p1000 && thi <= 0x1p1000;
    bool single = false, live = false;
    int iter = 1;
    auto loop_a = [&](auto spec) {
        constexpr bool ORD = decltype(spec)::value;
        if constexpr (ORD) c_ic_v = lerp_at(T, G, n, jtin, tin);
        for (; iter <= max_iters; iter++) {
            r.iters = iter;
            const double dd = xmin - xmax;
            if (collapsed(dd)) { s = SBR_NO_RUN_COLLAPSE; break; }
            if (iter == max_iters - 1) { s = SBR_NO_RUN_MAXITER; break; }
            const double xo = xnew;
            // t[jlo] <= ξmin <= xo <= ξmax < t[jhi+1]; on a grid that is not moderate a midpoint may overflow
            // past ξmax, and the reference's search is over the whole grid (±Inf and NaN end in its BoundsError)
            const int j = (ORD || moderate) ? ssl_range(T, jlo, jhi, xo) : ssl_range(T, 0, n - 1, xo);
            double ic, oc, Goc, Gic = 0.0;
            int joc, jic = 0;
            if constexpr (ORD) {
                ic = tin; oc = xo; joc = j; jic = jtin;
                Goc = lerp_at(T, G, n, j, xo);
                Gic = c_ic_v;
            } else {
                ic = dmin(tin, xo); oc = dmin(tout, xo);
                // G(oc)
                const bool ok = in_range(oc, tlo, thi, trunc, flag);
                joc = (oc == xo) ? j : (ok ? ssl_range(T, 0, n - 1, oc) : 0);
                Goc = ok ? lerp_at(T, G, n, joc, oc) : 0.0;
                // G(ic) — ic == tin for every iterate of a valid bracket; cached by value
                if (in_range(ic, tlo, thi, trunc, flag)) {
                    jic = (ic == tin) ? jtin : (ic == xo ? j : ssl_range(T, 0, n - 1, ic));
                    if (ic == c_ic_x) Gic = c_ic_v;
                    else { Gic = lerp_at(T, G, n, jic, ic); c_ic_x = ic; c_ic_v = Gic; }
                }
            }
            // ε = local knot spacing at ξ_old (solver.jl:336-338)
            if (j + 1 >= n) { flag |= trunc ? SBR_ENGINE_TRUNC : SBR_OOB; break; }
            const double eps = T[j + 1] - T[j];
            const double xoe = oc + eps, xie = ic + eps;
            // the slope probe AW(ξ + ε) only decides the terminal iterate (solver.jl:345-352);
            // its lookups' BoundsError checks still run every iterate, in the reference's order
            const bool oke = in_range(xoe, tlo, thi, trunc, flag);
            const bool oki = in_range(xie, tlo, thi, trunc, flag);
            if (flag) break;
            const double AW = Goc - Gic;
            const double err = AW - kappa;
            if (fabs(err) <= tolerance) {
                double Goce = 0.0, Gice = 0.0;
                if (oke) Goce = lerp_at(T, G, n, ssl_gallop(T, n, joc, xoe), xoe);
                if (oki) Gice = lerp_at(T, G, n, ssl_gallop(T, n, jic, xie), xie);
                const double AWe = Goce - Gice;
                if (AWe >= AW) { s = SBR_RUN; xi = xo; tolr = fabs(err); }
                else s = SBR_FALSE_EQ;
                break;
            } else if (err > 0) {
                xmax = xo; jhi = j; xnew = 0.5 * (xo + xmin);
            } else {
                xmin = xo; jlo = j; xnew = 0.5 * (xo + xmax);
            }
            // j + 1 < n and ξ + ε, tin + ε in range were tested by this iteration (ε > 0: t[j] <= ξ < t[j+1])
            const bool inside = ORD || (moderate && ic == tin && tin <= xmin && xmax <= tout);
            single = single || (inside && jlo == jhi && xmax + eps <= thi && eps > 0.0);
            if (__ballot(!single) == 0) { live = true; iter++; break; }
        }
    };
    if (__ballot(!(moderate && tin <= tout)) == 0) loop_a(BoolC<true>{});
    else loop_a(BoolC<false>{});
    if (live) {
        const int j = jlo;
        const double t0 = T[j], g0 = G[j], g1 = G[j + 1], eps = T[j + 1] - t0, Gic = c_ic_v;
        // ε is the same for every iterate, so its reciprocal is refined once and the quotient
        // takes div_rcp's three operations.  That is the IEEE quotient (sbr_device.h) where
        // v_div_scale and v_div_fixup are identities: here the divisor ε is in [2^-64, 2^64] and the
        // dividend a = ξ − t0 is 0 or in [2^-900, ε] (a <= ξmax − t0 <= t1 − t0 by monotone
        // rounding), so the quotient and the remainder term are normal numbers or 0.  a >= 2^-900
        // when nonzero: for |t0| >= 2^-840 either |ξ| < |t0|/2 or the signs differ (a >= |t0|/2),
        // or ξ − t0 is exact (Sterbenz) and a multiple of ulp(t0)/2 >= 2^-894; for t0 = 0, a = ξ >=
        // ξmin, which must already be >= 2^-900 — a bracket [0, ·) can halve towards 0 for as many
        // iterations as the caller's bisect_max_iters allows, and then keeps `/`.  One lane
        // outside these ranges sends its wave through the loop with `/`.
        // (The estimate e0 + s·(ξ − t0) that used to skip the exact body of decided midpoints does
        // not pay any more: in this loop it was slower, as was `/` for every wave —
        // profiles/experiments/r07_bisect_loops.json.)
        const bool rcp_ok = eps >= 0x1p-64 && eps <= 0x1p64 &&
                            (fabs(t0) >= 0x1p-840 || (t0 == 0.0 && xmin >= 0x1p-900));
        const bool use_rcp = __ballot(!rcp_ok) == 0;
        const double rinv = rcp_refined(eps);
        const int last = max_iters - 1;
        int ex = 0; // 1 collapse, 2 iteration cap, 3 terminal iterate; 0: the loop ran out
        double xo = xnew, err = 0.0, Goc = 0.0;
        auto trips = [&](auto quot) {
            for (; iter <= max_iters; iter++) {
                r.iters = iter;
                const bool col = collapsed(xmin - xmax);
                xo = xnew;
                const double d = quot(xo - t0);
                Goc = g0 * (1.0 - d) + g1 * d;
                err = (Goc - Gic) - kappa;
                const bool ter = fabs(err) <= tolerance;
                if (col || iter == last || ter) { ex = col ? 1 : (iter == last ? 2 : 3); break; }
                const bool up = err > 0;
                const double other = up ? xmin : xmax;
                xmax = up ? xo : xmax;
                xmin = up ? xmin : xo;
                xnew = 0.5 * (xo + other);
            }
        };
        if (use_rcp) trips([&](double a) { return div_rcp(a, eps, rinv); });
        else trips([&](double a) { return a / eps; });
        if (ex == 1) s = SBR_NO_RUN_COLLAPSE;
        else if (ex == 3) {
            // the terminal iterate's slope probe (both arguments in range, see above)
            const double xoe = xo + eps, xie = tin + eps, AW = Goc - Gic;
            const double Goce = lerp_at(T, G, n, ssl_gallop(T, n, j, xoe), xoe);
            const double Gice = lerp_at(T, G, n, ssl_gallop(T, n, jtin, xie), xie);
            if (Goce - Gice >= AW) { s = SBR_RUN; xi = xo; tolr = fabs(err); }
            else s = SBR_FALSE_EQ;
        }
    }
    if (flag) { r.status = flag | lbits; return; }
    if (s != SBR_RUN) { r.status = s | lbits; return; }
    if (diag & 2) return;
    int nblk_eval = 0;

    // ---------------- get_AW on the HR grid + AW_max ----------------
    const double icc = (tin >= xi) ? xi : tin;
    const double occ = (tout > xi) ? xi : tout;
    if (!in_range(0.0, tlo, thi, trunc, flag)) { r.status = flag | lbits; return; }
    const double G0 = lerp_at(T, G, n, ssl_range(T, 0, n - 1, 0.0), 0.0);
    double mx = -INFINITY;
    auto xa_of = [&](int i) { const double v = (tau(i) - xi) + icc; return v > 0 ? v : 0.0; };
    auto xb_of = [&](int i) { const double v = (tau(i) - xi) + occ; return v > 0 ? v : 0.0; };
    // Brackets of a(τ̄_i) and b(τ̄_i) are searched from the last one found, moved by
    // the τ̄ distance (both are τ̄_i shifted by a constant, so they advance with i).
    int ra_i = 0, ra_j = 0, rb_i = 0, rb_j = 0;
    auto brk_a = [&](int i) { ra_j = ssl_near(T, n, ra_j + (i - ra_i), xa_of(i)); ra_i = i; return ra_j; };
    auto brk_b = [&](int i) { rb_j = ssl_near(T, n, rb_j + (i - rb_i), xb_of(i)); rb_i = i; return rb_j; };
    // exact AW_cum(τ̄_i) for i in [i0, i1), folded into the NaN-propagating max
    auto eval_range = [&](int i0, int i1) {
        // The brackets of a(τ̄_i) and b(τ̄_i) only move forward with i: keep each bracket's
        // two knots (t, G) in registers and slide them, so a knot costs the LDS loads of
        // the knots the brackets pass (≈1 per argument) instead of a fresh search + 4 lerp
        // operands each.  Bracket k = min(searchsortedlast, n − 2), as lerp_at clamps it.
        int ka = brk_a(i0), kb = brk_b(i0);
        ka = ka < n - 2 ? ka : n - 2;
        kb = kb < n - 2 ? kb : n - 2;
        double ta0 = T[ka], ta1 = T[ka + 1], ga0 = G[ka], ga1 = G[ka + 1];
        double tb0 = T[kb], tb1 = T[kb + 1], gb0 = G[kb], gb1 = G[kb + 1];
        for (int i = i0; i < i1; i++) {
            const double ti = tau(i);
            const double av = (ti - xi) + icc;
            const double bv = (ti - xi) + occ;
            const double xa = av > 0 ? av : 0.0;
            const double xb = bv > 0 ? bv : 0.0;
            if (!(xa <= thi) || !(xb <= thi)) { flag |= trunc ? SBR_ENGINE_TRUNC : SBR_OOB; return; }
            while (ka < n - 2 && ta1 <= xa) { ka++; ta0 = ta1; ga0 = ga1; ta1 = T[ka + 1]; ga1 = G[ka + 1]; }
            while (kb < n - 2 && tb1 <= xb) { kb++; tb0 = tb1; gb0 = gb1; tb1 = T[kb + 1]; gb1 = G[kb + 1]; }
            const double da = (xa - ta0) / (ta1 - ta0);
            const double gi = ga0 * (1.0 - da) + ga1 * da;
            // b(τ̄_i) = (τ̄_i − ξ) + ξ is τ̄_i itself whenever τ̄_i − ξ is exact (Sterbenz):
            // then δ = 0 and the lerp is G[j]·(1 − 0) + G[j+1]·0, no division
            double go;
            if (xb == tb0) go = gb0 * 1.0 + gb1 * 0.0;
            else { const double db = (xb - tb0) / (tb1 - tb0); go = gb0 * (1.0 - db) + gb1 * db; }
            const double awin = av >= 0 ? gi : 0.0;
            const double awout = bv >= 0 ? go : 0.0;
            const double v = (awout - awin) + G0;
            if (diag & 4) nblk_eval++;
            if (aw_path) aw_path[i] = v;
            if (mx == mx && (v != v || v > mx)) mx = v;
        }
        ra_j = ka; ra_i = i1 - 1;
        rb_j = kb; rb_i = i1 - 1;
    };
    // AW peak predictor (a logistic-shaped CDF): the continuous maximiser of
    // G(τ − s_out) − G(τ − s_in) sits where G(τ − s_out) + G(τ − s_in) = 1, i.e. at
    // τ* = t_half + (s_in + s_out)/2
    const double tstar = S.t_half + 0.5 * ((xi - icc) + (xi - occ));
    const bool predicted = tstar == tstar && tstar >= tau(0) && tstar <= tau(ntau - 1);
    const bool scan = S.scan && predicted;
    if (!S.pmc || aw_path || !(scan || S.bnb)) {
        eval_range(0, ntau); // exhaustive (single-point path mode, or summaries unavailable)
    } else {
        // Branch and bound over a 256/64/8 hierarchy of τ̄ ranges — the same maximum,
        // far fewer evaluations.  Every argument sequence is nondecreasing in i, so the
        // range check of the last τ̄ covers the whole path.
        const double al = (tau(ntau - 1) - xi) + icc, bl = (tau(ntau - 1) - xi) + occ;
        if (!((al > 0 ? al : 0.0) <= thi) || !((bl > 0 ? bl : 0.0) <= thi)) {
            flag |= trunc ? SBR_ENGINE_TRUNC : SBR_OOB;
        } else {
            // Upper bound of AW_cum over τ̄ indices [i0, i1]: AW_OUT ≤ max G over knots
            // ≤ bracket(b(τ̄_i1)) + 1, AW_IN ≥ min G over knots ≥ bracket(a(τ̄_i0)) (8-knot
            // prefix-max / suffix-min tables), plus a rounding margin far above the
            // ≈2e-15 the exact path can add.
            // When G is nondecreasing (every learning CDF of the configs) the prefix max up to
            // knot k is G[k] and the suffix min from k is G[k]: knot-exact bounds, loose by one
            // knot interval instead of an 8-knot block on each side.
            auto ub_rng = [&](int i0, int i1) -> double {
                const int ja = brk_a(i0), jb = brk_b(i1);
                const int kh = jb + 1 < n - 1 ? jb + 1 : n - 1, kl = ja < n - 2 ? ja : n - 2;
                const double hi = S.mono ? G[kh] : S.pmc[kh >> 3];
                const double lo = S.mono ? G[kl] : S.smc[kl >> 3];
                const double ub_out = hi > 0.0 ? hi : 0.0;
                const double lb_in = ((tau(i0) - xi) + icc) >= 0 ? lo : (lo < 0.0 ? lo : 0.0);
                return ((ub_out - lb_in) + G0) + 1e-14;
            };
            auto end_of = [&](int i0, int w) { return i0 + w < ntau ? i0 + w : ntau; };
            // pass 1: a first running maximum.  For a logistic-shaped CDF the continuous
            // maximiser of G(τ − s_out) − G(τ − s_in) sits where G(τ − s_out) + G(τ − s_in) = 1,
            // i.e. at τ* = t_half + (s_in + s_out)/2: evaluate the 8-blocks around it
            // (a heuristic — exactness comes from pass 2's bounds).  Otherwise descend the
            // bound hierarchy to the most promising 8-block.
            const int ic = predicted ? ssl_range(T, 0, (nle > 0 ? nle : 1) - 1, tstar < T[0] ? T[0] : tstar) : 0;
            if (scan) {
                aw_scan(T, G, n, ntau, nle, ETA, xi, icc, occ, G0, S.dd, ic < ntau ? ic : ntau - 1, mx, nblk_eval,
                        S.koff, S.wlo, S.whi, S.wm);
            } else
            {
            int b8 = -1, w0 = 0, w1 = 0;
            if (predicted) {
                const int c8 = (ic < ntau ? ic : ntau - 1) & ~7;
                w0 = c8 - 8 * kAwWin > 0 ? c8 - 8 * kAwWin : 0;
                w1 = end_of(c8, 8 * (kAwWin + 1));
                eval_range(w0, w1);
            } else {
                int bs = 0;
                double bu = -INFINITY;
                for (int i0 = 0; i0 < ntau; i0 += 256) {
                    const double ub = ub_rng(i0, end_of(i0, 256) - 1);
                    if (!(ub <= bu)) { bu = ub; bs = i0; }
                }
                int bb = bs;
                bu = -INFINITY;
                for (int i0 = bs; i0 < end_of(bs, 256); i0 += 64) {
                    const double ub = ub_rng(i0, end_of(i0, 64) - 1);
                    if (!(ub <= bu)) { bu = ub; bb = i0; }
                }
                b8 = bb;
                bu = -INFINITY;
                for (int i0 = bb; i0 < end_of(bb, 64); i0 += 8) {
                    const double ub = ub_rng(i0, end_of(i0, 8) - 1);
                    if (!(ub <= bu)) { bu = ub; b8 = i0; }
                }
                eval_range(b8, end_of(b8, 8));
            }
            // pass 2: every range whose bound beats the running max is refined
            for (int s0 = 0; s0 < ntau && !flag && mx == mx; s0 += 256) {
                const int se = end_of(s0, 256);
                if (ub_rng(s0, se - 1) <= mx) continue;
                for (int k0 = s0; k0 < se && !flag && mx == mx; k0 += 64) {
                    const int ke = end_of(k0, 64);
                    if (ub_rng(k0, ke - 1) <= mx) continue;
                    for (int i0 = k0; i0 < ke && !flag && mx == mx; i0 += 8) {
                        const int ie = end_of(i0, 8);
                        if (i0 == b8 || (i0 >= w0 && ie <= w1) || ub_rng(i0, ie - 1) <= mx) continue;
                        eval_range(i0, ie);
                    }
                }
            }
            }
        }
    }
    if (flag) { r.status = flag | lbits; return; }
    r.xi = xi;
    r.tol = tolr;
    r.aw = mx;
    r.status = SBR_RUN | SBR_CONVERGED | lbits;
    if (diag & 4) r.iters = nblk_eval;
}

// ============================================================================
// Interest-rate extension (src/extensions/interest_rates/)
// ============================================================================
// τ̄ grid view: knots ≤ η, then η (hazard_rate's grid, solver.jl:155-161)
template <class P>
struct TauView {
    P T;
    int nle;
    double eta;
    __device__ __forceinline__ double operator[](int i) const { return i < nle ? T[i] : eta; }
};

// Tsit5 dense-output coefficients (OrdinaryDiffEqTsit5 Tsit5Interp) — as oracle tsit5_dense
constexpr double R11 = 1.0, R12 = -2.763706197274826, R13 = 2.9132554618219126, R14 = -1.0530884977290216;
constexpr double R22 = 0.13169999999999998, R23 = -0.2234, R24 = 0.1017;
constexpr double R32 = 3.9302962368947516, R33 = -5.941033872131505, R34 = 2.490627285651253;
constexpr double R42 = -12.411077166933676, R43 = 30.33818863028232, R44 = -16.548102889244902;
constexpr double R52 = 37.50931341651104, R53 = -88.1789048947664, R54 = 47.37952196281928;
constexpr double R62 = -27.896526289197286, R63 = 65.09189467479366, R64 = -34.87065786149660;
constexpr double R72 = 1.5, R73 = -4.0, R74 = 2.5;

// the step's interpolant at Θ (saveat): Horner b_i(Θ), nested muladd sum
__device__ __forceinline__ double tsit5_dense(double th, double dt, double y0, double k1, double k2, double k3,
                                              double k4, double k5, double k6, double k7)
{
    const double th2 = th * th;
    const double b1 = th * fma(th, fma(th, fma(th, R14, R13), R12), R11);
    const double b2 = th2 * fma(th, fma(th, R24, R23), R22);
    const double b3 = th2 * fma(th, fma(th, R34, R33), R32);
    const double b4 = th2 * fma(th, fma(th, R44, R43), R42);
    const double b5 = th2 * fma(th, fma(th, R54, R53), R52);
    const double b6 = th2 * fma(th, fma(th, R64, R63), R62);
    const double b7 = th2 * fma(th, fma(th, R74, R73), R72);
    const double sum = fma(k1, b1, fma(k2, b2, fma(k3, b3, fma(k4, b4, fma(k5, b5, fma(k6, b6, k7 * b7))))));
    return fma(dt, sum, y0);
}

// hjb_equation! (value_function_solver.jl:86-95): dV = (h + δ)(1 − V) + max(u + rV − h, 0)
// with h = HR(τ̄) (gridded linear, Throw()); brackets galloped from the step's own.
template <class P>
struct ValueRhs {
    TauView<P> tau;
    P H;
    int ntau;
    double delta, r, u, tlo, thi;
    int jb;
    bool oob;
    __device__ __forceinline__ double hr(double t)
    {
        if (ntau < 2 || !(t >= tlo && t <= thi)) { oob = true; return (double)NAN; }
        const int j = (tau[jb] <= t) ? ssl_gallop(tau, ntau, jb, t) : ssl_range(tau, 0, jb, t);
        return lerp_at(tau, H, ntau, j, t);
    }
    __device__ __forceinline__ double eval(double t, double V)
    {
        const double h = hr(t);
        const double x = (u + r * V) - h;
        const double re = (x != x) ? x : (x > 0.0 ? x : 0.0); // Julia max(x, 0.0)
        return (h + delta) * (1.0 - V) + re;
    }
    __device__ __forceinline__ void prepare(double, double) {}
    __device__ __forceinline__ double stage(int, double ts, double V) { return eval(ts, V); }
    // ForwardDiff (oracle jac_value): max(x, 0.0) on a Dual keeps x iff 0 < x (or NaN);
    // J = −(h + δ) + (r | 0), ∂f/∂τ̄ = h'·(1 − V) + (−h' | 0), h' the HR interpolant's slope
    __device__ __forceinline__ void jac(double t, double V, double& J, double& dT)
    {
        double h = (double)NAN, hp = (double)NAN;
        if (ntau < 2 || !(t >= tlo && t <= thi)) {
            oob = true;
        } else {
            int j = (tau[jb] <= t) ? ssl_gallop(tau, ntau, jb, t) : ssl_range(tau, 0, jb, t);
            j = j > ntau - 2 ? ntau - 2 : (j < 0 ? 0 : j);
            const double t0 = tau[j], t1 = tau[j + 1], h0 = H[j], h1 = H[j + 1];
            const double d = (t - t0) / (t1 - t0);
            h = h0 * (1.0 - d) + h1 * d;
            const double rr = 1.0 / (t1 - t0);
            hp = h0 * (-rr) + h1 * rr;
        }
        const double x = (u + r * V) - h;
        const bool keep = (x != x) || (x > 0.0);
        J = (h + delta) * (-1.0) + (keep ? r : 0.0);
        dT = hp * (1.0 - V) + (keep ? -hp : 0.0);
    }
    __device__ __forceinline__ void accepted(double t)
    {
        if (ntau >= 2 && t >= tlo && t <= thi) jb = ssl_gallop(tau, ntau, jb, t);
    }
    static constexpr bool kFsalExact = false;
    static constexpr int kPinTableau = 0;
};

// The value function saved on the HR grid (saveat) streamed into optimal_buffer
// on h − rV (interest_rate_solver.jl:84-93, solver.jl:211-264): V(τ̄_i) and HR(τ̄_i)
// are their interpolants at their own knots (v_i·(1−0) + v_{i+1}·0, the last knot
// v_{n−2}·0 + v_{n−1}·1), so knot i is scanned once V_{i+1} is known.
template <class P>
struct SaveScan {
    TauView<P> tau;
    P H;
    int ntau;
    double r, u;
    double* vpath;   // single-point mode: every saved V (may be null)
    int next;        // grid index of the next saved value
    double vprev;    // V at knot next − 1 (its h − rV waits for V_next)
    double vprev2;   // V at knot next − 2
    int nh;          // h − rV values scanned
    double hprev;    // h − rV at knot nh − 1
    bool any, all;
    int fa, la, cin, cout;
    double tin_x, tout_x; // crossing lerps (valid when cin / cout ≥ 0)
    __device__ __forceinline__ void init(double V0)
    {
        next = 1; vprev = V0; vprev2 = 0.0; nh = 0; hprev = 0.0;
        if (vpath) vpath[0] = V0;
        any = false; all = true; fa = la = cin = cout = -1; tin_x = tout_x = 0.0;
    }
    __device__ __forceinline__ void scan(double hv)
    {
        const int i = nh;
        const bool ab = hv > u;
        any |= ab;
        all &= ab;
        if (ab) { if (fa < 0) fa = i; la = i; }
        if (i > 0) {
            const bool pab = hprev > u;
            const double t0 = tau[i - 1], t1 = tau[i];
            if (!pab && ab && cin < 0) { cin = i - 1; tin_x = t0 + ((u - hprev) * (t1 - t0)) / (hv - hprev); }
            if (pab && !ab) { cout = i - 1; tout_x = t0 + ((u - hprev) * (t1 - t0)) / (hv - hprev); }
        }
        hprev = hv;
        nh = i + 1;
    }
    // V_k saved (k = next): knot k − 1 is interior to V's grid now
    __device__ __forceinline__ void save(double v)
    {
        const int i = next - 1;
        if (vpath) vpath[next] = v;
        const double ti = tau[i], t1 = tau[i + 1];
        const double d = (ti - ti) / (t1 - ti);
        const double Vi = vprev * (1.0 - d) + v * d;
        scan(lerp_at(tau, H, ntau, i, ti) - r * Vi);
        vprev2 = vprev;
        vprev = v;
        next++;
    }
    // after the solve: the last saved knot (j = n − 2, δ = 1)
    __device__ __forceinline__ void finish()
    {
        const int i = next - 1;
        const double t0 = tau[i - 1], ti = tau[i];
        const double d = (ti - t0) / (ti - t0);
        const double Vi = vprev2 * (1.0 - d) + vprev * d;
        scan(lerp_at(tau, H, ntau, i, ti) - r * Vi);
    }
};

// solve_equilibrium_interest (interest_rate_solver.jl:51-150) for one u with r > 0:
// V on the HR grid, optimal_buffer on h − rV, then the baseline's compute_ξ / AW.
// sbr_interest_econ.hip holds a copy of this function in two parts — interest_value_stage (down to
// τ̄_IN, τ̄_OUT) and the κ loop of interest_econ_lane (the preamble and the three ways out below) —
// because a shared stage changes equilibrium_kernel's machine code.  Edit one, edit the other.
template <class P>
__device__ __forceinline__ void solve_interest_point(P T, P G, P H, const Summ& S, const int n, const int ntau,
                                                     const int nle, const double ETA, const double T1,
                                                     const bool trunc, const double u, const double kappa,
                                                     const int max_iters, const uint32_t lbits,
                                                     const InterestArgs& ia, PointResult& r, int64_t& nsteps,
                                                     double* __restrict__ aw_path, const int diag)
{
    r.xi = NAN; r.aw = NAN; r.tol = INFINITY; r.iters = 0; r.status = 0;
    nsteps = 0;
    const TauView<P> tau{T, nle, ETA};
    ValueRhs<P> f{tau, H, ntau, ia.delta, ia.r, u, ntau > 0 ? tau[0] : 0.0, ntau > 0 ? tau[ntau - 1] : 0.0, 0, false};
    const double V0 = (u + ia.delta) / (ia.r + ia.delta);
    SaveScan<P> sv{tau, H, ntau, ia.r, u, ia.v_path};
    sv.init(V0);
    // savevalues! with saveat = the HR grid: each pending grid point ≤ the new t is the
    // step's dense output at Θ = (s − tprev)/dt (Tsit5's or Rosenbrock23's), or u itself at t
    struct Saver {
        SaveScan<P>& sv;
        const TauView<P>& tau;
        int ntau;
        __device__ __forceinline__ bool start(double, double) { return true; }
        __device__ __forceinline__ bool step(bool acc, double tprev, double tn, double dt, double y0, double y1,
                                             const StepK& K, bool)
        {
            while (acc && sv.next < ntau && tau[sv.next] <= tn) {
                const double ts = tau[sv.next];
                const double th = (ts - tprev) / dt;
                sv.save(ts != tn ? (K.stiff ? ros23_dense(th, dt, y0, K.k[0], K.k[1])
                                            : tsit5_dense(th, dt, y0, K.k[0], K.k[1], K.k[2], K.k[3], K.k[4],
                                                          K.k[5], K.k[6]))
                                 : y1);
            }
            return true;
        }
    } saver{sv, tau, ntau};
    OdeOut vo;
    ode_scalar(f, saver, ntau > 0 ? tau[ntau - 1] : 0.0, V0, ia.rtol, ia.atol, ia.maxiters, vo);
    uint32_t vbits = vo.status;
    nsteps = vo.naccept + vo.nreject;
    if (ia.v_count) *ia.v_count = sv.next;
    if (f.oob) vbits |= SBR_OOB;
    const uint32_t bits = lbits | (vbits & (SBR_ODE_MAXITERS | SBR_STIFF_SWITCH | SBR_ODE_FAILED));
    if ((vbits & SBR_OOB) || sv.next < 2) { // HR lookup past the grid / a 1-knot V interpolant: BoundsError
        r.status = SBR_OOB | bits;
        r.tin = NAN; r.tout = NAN;
        return;
    }
    sv.finish();
    const int ns = sv.nh;
    double tin, tout;
    if (!sv.any) {
        tin = T1; tout = T1;
    } else if (sv.all) {
        tin = tau[0]; tout = tau[ns - 1];
    } else {
        tin = sv.cin >= 0 ? sv.tin_x : T1;
        tout = sv.cout >= 0 ? sv.tout_x : T1;
        if (tin == T1) tin = tau[sv.fa];
        if (tout == T1) tout = tau[sv.la];
    }
    r.tin = tin;
    r.tout = tout;
    if (diag & 1) { r.status = bits; return; }
    solve_from_buffers(T, G, H, S, n, ntau, nle, ETA, T1, trunc, u, kappa, max_iters, bits, r, aw_path, diag, tin,
                       tout);
}

// The equilibria of u values [j0, j1) of column b by one workgroup of BLOCK threads (smem:
// the dynamic LDS slab of launch_equilibrium's size).  Starts and ends uniformly; the caller
// puts a barrier between two calls on the same workgroup (the LDS slab and flags are reused).
template <int BLOCK, bool INTEREST, int MODE = 0>
__device__ __forceinline__ void eq_column(const int b, const int j0, const int j1, const LearnBufs& L,
                                          const double* __restrict__ eta, const double* __restrict__ t_end,
                                          const double* __restrict__ u, const EqArgs& a, const InterestArgs& ia,
                                          const ResultSoA& out, double* smem)
// point j of the β×u sweeps: u[j] with the launch's κ, result (b, j) of an n_beta × n_u grid
#define SBR_EQ_U(j) u[j]
#define SBR_EQ_KAPPA(j) a.kappa
#define SBR_EQ_BAD(uj, j) !(uj >= 0.0)
#define SBR_EQ_OUT(b, j) (size_t)b * (size_t)a.n_u + j
#include "sbr_eq_column_body.h"
#undef SBR_EQ_U
#undef SBR_EQ_KAPPA
#undef SBR_EQ_BAD
#undef SBR_EQ_OUT

}  // namespace sbr
