// sbr_solve_dev.h — the per-point equilibrium pieces every baseline solve shares: PointResult, the
// interpolant range checks, the block summaries, the AW scan and the plain ξ iteration.
// Device code; include from a .hip file after sbr_hazard_dev.h.
#pragma once

#include "sbr_device.h"
#include "sbr_kernels.h"
#include "sbr_scan.h"
#include "sbr_hazard_dev.h"

namespace sbr {

struct PointResult {
    double xi, tin, tout, aw, tol;
    uint32_t status;
    int iters;
};

// Learning bits of a knot grid that ends early for a reason other than the engine's own stop after η
// (DESIGN.md §Truncated learning): the integrator's iteration cap, the knot capacity, a failed step.
// The reference's interpolant ends where such a grid ends, so a lookup past its last knot is the
// BoundsError (SBR_OOB), never SBR_ENGINE_TRUNC.
constexpr uint32_t kLearnCutBits = SBR_ODE_MAXITERS | SBR_KNOT_OVERFLOW | SBR_ODE_FAILED;

// range check of an interpolation argument; returns false (and flags) when
// Interpolations' Throw() extrapolation would raise.
__device__ __forceinline__ bool in_range(double x, double tlo, double thi, bool trunc, uint32_t& flag)
{
    if (x >= tlo && x <= thi) return true;
    flag |= (trunc && x > thi) ? SBR_ENGINE_TRUNC : SBR_OOB;
    return false;
}

// Per-workgroup summaries staged in LDS next to the knot grid (null = unavailable):
//   hmax/hmin  per 64-entry block of HR(τ̄): max over non-NaN entries / min with NaN as −∞,
//              i.e. "some entry > u" ⇔ hmax > u and "every entry > u" ⇔ hmin > u;
//   pmc/smc    per 64-knot block of G: prefix max / suffix min over blocks (NaN-propagating).
struct Summ {
    const double* hmax;
    const double* hmin;
    const double* pmc;
    const double* smc;
    bool mono; // G nondecreasing over the knots (no NaN): prefix max / suffix min are knot values
    double t_half; // time where G crosses 1/2 (lerp inverse), NaN if it does not: AW peak predictor
    // aw_scan's preconditions: no NaN in G, 0 <= G[0], G[n−1] <= 2 (the 1e-14 rounding margin),
    // t[k+2] − t[k] > 1e-15·t[n−1] (a shifted τ̄ argument stays below the knot after next) and a
    // drawdown bound dd <= 1e-12 (Tsit5 at eps() leaves ulp-sized decreases in the saturated tail
    // of G on ≈20 % of the Fig 5 columns: G[k] <= G[k'] + dd for every k < k')
    bool scan;
    double dd;
    bool bnb; // the branch-and-bound bounds are available (mono, or the prefix/suffix tables built)
    // aw_scan's knot offset for AW_OUT(b_j) <= G[j + koff]: 1 when consecutive knots are more than
    // 1e-15·t[n−1] apart (b_j then lies below t[j + 1]: bracket <= j), else 2 (knots 2 apart)
    int koff;
    // prefix / suffix extremes of the HR block summaries: hpm = prefix max of hmax,
    // hpn = prefix min of hmin, hsm = suffix max of hmax, hsn = suffix min of hmin, over nbh
    // blocks; null: the linear block scans
    const double* hpm;
    const double* hpn;
    const double* hsm;
    const double* hsn;
    int nbh;
    // aw_scan's slope-monotone window, as times: the knot-to-knot slopes of G rise strictly from
    // knot 0 and then fall strictly up to knot wb, so AW_cum is quasi-concave in τ̄ while both its
    // arguments lie in [wlo, whi] = [max(t[0], 0) + δ, t[wb] − δ] (δ: the rounding of a shifted
    // argument); wm is what rounding can add to a comparison of two AW_cum values there.  Empty
    // (wlo > whi) where no summaries are built: the scan then prunes with its bounds alone.
    double wlo = INFINITY, whi = -INFINITY, wm = 0.0;
};

template <class P>
__device__ __forceinline__ void solve_from_buffers(P T, P G, P H, const Summ& S, const int n, const int ntau,
                                                   const int nle, const double ETA, const double T1, const bool trunc,
                                                   const double u, const double kappa, const int max_iters,
                                                   const uint32_t lbits, PointResult& r, double* __restrict__ aw_path,
                                                   const int diag, const double tin, const double tout);

// smallest k in [0, hi] with key(k) >= x, for a nondecreasing key with key(hi) >= x: gallop
// down from hi, then bisect
template <class F>
__device__ __forceinline__ int first_ge_down(F key, int hi, double x)
{
    int top = hi, lo = hi - 1, step = 1; // key(top) >= x; answer in (lo, top]
    while (lo >= 0 && key(lo) >= x) {
        top = lo;
        step <<= 1;
        lo = top - step;
    }
    if (lo < -1) lo = -1;
    while (top - lo > 1) {
        const int mid = (lo + top) >> 1;
        if (key(mid) >= x) top = mid;
        else lo = mid;
    }
    return top;
}

// AW_max (solver.jl:553-576) over τ̄ knots [0, ntau) by an outward scan from the predicted
// peak knot c, for a G with Summ::scan's preconditions (nondecreasing up to the drawdown dd:
// every bound below is widened by dd, and the margin is 1e-14 + 4·dd).  AW_cum(τ̄_i) =
// AW_OUT(b_i) − AW_IN(a_i) + G(0) with a_i = (τ̄_i − ξ) + icc ≤ b_i = (τ̄_i − ξ) + occ ≤ τ̄_i + ulp,
// both nondecreasing in i, so
//   right of the last evaluated knot i:  AW_OUT(b_j) ≤ G[j + 2] and AW_IN(a_j) ≥ AW_IN(a_i);
//   left of it:                         AW_OUT(b_j) ≤ AW_OUT(b_i) and AW_IN(a_j) ≥ G[bracket(a_j)].
// A knot is evaluated exactly (the same operations as eval_range) only where these bounds
// (+ the 1e-14 rounding margin) do not already put it at or below the running maximum; runs
// of knots the bounds dismiss are skipped with one search in G (right) or in G and τ̄ (left).
// The maximum equals the exhaustive one bit for bit (G has no NaN here).
// (A knot offset 0 for the AW_OUT bound inside [ξ/2, 2ξ], where b_i = t[i] exactly, halved the exact
// evaluations and was slower: an exact evaluation costs about what a bounded trip costs,
// profiles/experiments/r05_d_*)
//
// The slope-monotone window (Summ::wlo, whi, wm).  Over the window's knots the
// slopes of the interpolant Ĝ rise and then fall, so for s_out = ξ − occ ≤ s_in = ξ − icc the function
// F(τ) = Ĝ(τ − s_out) − Ĝ(τ − s_in) has F′ = slope(b) − slope(a) ≥ 0 while both arguments are in the
// convex part, nonincreasing while a is in the convex and b in the concave part, and ≤ 0 once both
// are in the concave part: F is quasi-concave on the τ interval whose arguments stay in the
// window.  Hence, for evaluated knots c′ and i and any knot j beyond i on the side away from c′,
// all three inside the window:  F(τ̄_i) < F(τ̄_c′)  ⇒  F(τ̄_j) ≤ F(τ̄_i).
// The computed v_i differs from F(τ̄_i) + G(0) by at most E = E_arg + E_op:
//   E_arg  the computed a_i = fl(fl(τ̄_i − ξ) + icc) is off by at most u·(|τ̄_i − ξ| + |a_i|) ≤ u·(2·t[wb] + |icc|)
//          (u = 2^-53; |τ̄_i − ξ| ≤ |a_i| + |icc| and 0 ≤ a_i ≤ t[wb] inside the window), b_i alike with occ; icc, occ
//          and ξ lie on the grid, so both are within δ = 2^-52·(t[wb] + 2·max|t|), and Ĝ moves by at most
//          D·δ per argument, D the largest |slope| of the column: E_arg ≤ 2·D·δ.  The window's ends
//          are moved inward by δ, so the exact arguments are inside it whenever the computed are.
//   E_op   the two lerps (δ_a, 1 − δ_a, two products, a sum: ≤ 12·u·max|G| each, max|G| ≤ 2 + dd) and the two
//          last operations (≤ 10·u): E_op ≤ 58·u·(1 + dd) < 2^-47.
// With wm = 2^-46 + D·2^-50·(t[wb] + 2·max|t|) ≥ 2·E, the test  v_i < mx − (M + wm)  on computed values, mx
// held by a knot c′ inside the window, gives F(τ̄_i) < F(τ̄_c′) and so v_j ≤ F(τ̄_j) + G(0) + E ≤ v_i + 2·E < mx for
// every such j: none of them can raise the maximum, and they are dismissed unvisited.  The scan
// goes on with its bounds from the first knot outside the window (LA / UB hold the last
// exact AW_IN / AW_OUT, valid bounds as before).  a_i > 0 inside the window (wlo > 0), so AW_IN and AW_OUT
// are the two lerps there.  M itself is not loosened: the bounds use it as before.
template <class P>
__device__ __forceinline__ void aw_scan(P T, P G, const int n, const int ntau, const int nle, const double ETA,
                                        const double xi, const double icc, const double occ, const double G0,
                                        const double dd, const int c, double& mx, int& nev, const int koff = 2,
                                        const double wlo = INFINITY, const double whi = -INFINITY,
                                        const double wm = 0.0)
{
    const double M = 1e-14 + 4.0 * dd;
    const double Mw = M + wm;
    const bool wuse = occ >= icc && wlo <= whi;
    auto tau = [&](int i) -> double { return i < nle ? T[i] : ETA; };
    auto bv_of = [&](int i) -> double { return (tau(i) - xi) + occ; };
    auto av_of = [&](int i) -> double { return (tau(i) - xi) + icc; };
    // a(τ̄_i)'s bracket window: k = min(searchsortedlast(t, x), n − 2), its two knots (t, G)
    int ka;
    double ta0, ta1, ga0, ga1;
    auto seek = [&](int hint, double x) {
        ka = ssl_near(T, n, hint, x);
        ka = ka < n - 2 ? ka : n - 2;
        ta0 = T[ka]; ta1 = T[ka + 1]; ga0 = G[ka]; ga1 = G[ka + 1];
    };
    auto fwd = [&](double x) {
        while (ka < n - 2 && ta1 <= x) { ka++; ta0 = ta1; ga0 = ga1; ta1 = T[ka + 1]; ga1 = G[ka + 1]; }
    };
    auto bwd = [&](double x) {
        while (ka > 0 && ta0 > x) { ka--; ta1 = ta0; ga1 = ga0; ta0 = T[ka]; ga0 = G[ka]; }
    };
    // exact AW_cum(τ̄_i) with the a window at a_i's bracket; b's bracket is searched from i
    double awin = 0.0, awout = 0.0;
    auto exact = [&](int i, double av, double xa) -> double {
        const double ti = tau(i);
        const double bv = (ti - xi) + occ;
        const double xb = bv > 0 ? bv : 0.0;
        // b(τ̄_i) is τ̄_i = t[i] itself whenever τ̄_i − ξ is exact: bracket i, no search
        int kb = (i < nle && xb == ti) ? i : ssl_near(T, n, i, xb);
        kb = kb < n - 2 ? kb : n - 2;
        const double tb0 = T[kb], tb1 = T[kb + 1], gb0 = G[kb], gb1 = G[kb + 1];
        const double da = (xa - ta0) / (ta1 - ta0);
        const double gi = ga0 * (1.0 - da) + ga1 * da;
        double go;
        if (xb == tb0) go = gb0 * 1.0 + gb1 * 0.0;
        else { const double db = (xb - tb0) / (tb1 - tb0); go = gb0 * (1.0 - db) + gb1 * db; }
        awin = av >= 0 ? gi : 0.0;
        awout = bv >= 0 ? go : 0.0;
        nev++;
        return (awout - awin) + G0;
    };
    bool mxin; // the running maximum is held by a knot inside the window
    // knot c
    {
        const double av = av_of(c), xa = av > 0 ? av : 0.0;
        seek(c, xa);
        const double v = exact(c, av, xa);
        if (v > mx) mx = v;
        mxin = wuse && av >= wlo && bv_of(c) <= whi;
    }
    const int kc = ka;
    const double ub_left = awout;
    // right of c
    double LA = awin; // lower bound of AW_IN(a_j) for every j >= i
    for (int i = c + 1; i < ntau;) {
        const double ti = tau(i);
        const double av = (ti - xi) + icc, xa = av > 0 ? av : 0.0;
        fwd(xa);
        const double lb = av >= 0 ? ga0 : 0.0;
        LA = LA > lb ? LA : lb;
        const double V = (((mx - G0) + LA) - M) - dd; // G[k] <= V: every knot up to k is <= V + dd
        const int k2 = i + koff < n - 1 ? i + koff : n - 1;
        int inext;
        if (G[k2] > V) {
            const double v = exact(i, av, xa);
            LA = awin;
            const double bv = (ti - xi) + occ;
            bool drop = false;
            if (v > mx) {
                mx = v;
                mxin = wuse && av >= wlo && bv <= whi;
            } else {
                drop = mxin && bv <= whi && v < mx - Mw;
            }
            if (!drop) {
                i++;
                continue;
            }
            // dropped inside the window (a_i >= a_c′ >= wlo): every further knot with b_j <= whi is
            // below the maximum; go on from the first one outside
            if (bv_of(ntau - 1) <= whi) break;
            int lo = i;
            inext = ntau - 1; // b_lo <= whi < b_inext
            while (inext - lo > 1) {
                const int mid = (lo + inext) >> 1;
                if (bv_of(mid) <= whi) lo = mid;
                else inext = mid;
            }
        } else {
            // every knot j with G[min(j + 2, n − 1)] <= V is at or below mx: skip to the first other
            const int kl = ssl_gallop(G, n, k2, V);
            if (kl >= n - 1) break;
            // G[kl + 1] > V: the first knot whose bound is not dismissed
            inext = kl + 1 - koff;
        }
        const double an = av_of(inext);
        seek(ka + (inext - i), an > 0 ? an : 0.0);
        i = inext;
    }
    // left of c
    double UB = ub_left; // upper bound of AW_OUT(b_j) for every j <= i
    {
        const double av = av_of(c);
        seek(kc, av > 0 ? av : 0.0);
    }
    for (int i = c - 1; i >= 0;) {
        const double ti = tau(i);
        const int k2 = i + koff < n - 1 ? i + koff : n - 1;
        const double g2 = G[k2] > 0.0 ? G[k2] : 0.0;
        UB = UB < g2 ? UB : g2;
        const double Vp = (((UB + G0) + M) - mx) + dd; // AW_IN(a_j) >= G[bracket(a_j)] − dd
        if (!(Vp - dd > 0.0)) break; // AW_IN(a_j) >= 0 for every j: all pruned
        const double av = (ti - xi) + icc, xa = av > 0 ? av : 0.0;
        bwd(xa);
        const double lb = av >= 0 ? ga0 : 0.0;
        int ks;
        double tk;
        if (!(lb >= Vp)) {
            const double v = exact(i, av, xa);
            UB = UB < awout ? UB : awout;
            bool drop = false;
            if (v > mx) {
                mx = v;
                mxin = wuse && av >= wlo && (ti - xi) + occ <= whi;
            } else {
                drop = mxin && av >= wlo && v < mx - Mw;
            }
            if (!drop) {
                i--;
                continue;
            }
            // dropped inside the window (b_i <= b_c′ <= whi): every further knot with a_j >= wlo is
            // below the maximum; go on from the first one outside
            ks = ka;
            tk = wlo;
        } else {
            // knots j <= i with a_j >= t[k*] (k* = first knot with G >= Vp) are pruned
            ks = first_ge_down([&](int k) { return G[k]; }, ka, Vp);
            tk = T[ks];
        }
        const int j = first_ge_down(av_of, i, tk);
        if (j == 0) break;
        const int inext = j - 1;
        const double an = av_of(inext);
        seek(ks, an > 0 ? an : 0.0);
        i = inext;
    }
}

// compute_ξ (solver.jl:308-376) from an arbitrary first iterate ξ_guess (the single-point kernel's
// knots-in calls only: the sweep kernel carries none of this): the reference's iteration as
// written, every lookup bracketed by a search over the whole grid (the oracle's compute_xi).  A
// lookup outside [t[0], t[n−1]] — G at a constrained time, searchsortedlast(grid, ξ_old) below the
// first knot or at the last, the ε probes — is the interpolant's BoundsError.
template <class P>
__device__ __forceinline__ void bisect_plain(P T, P G, const int n, const double tlo, const double thi,
                                             const bool trunc, const double tin, const double tout,
                                             const double guess, const double kappa, const double tolerance,
                                             const int max_iters, PointResult& r, uint32_t& flag, uint32_t& s,
                                             double& xi, double& tolr)
{
    double xnew = guess, xmin = tin, xmax = tout;
    for (int iter = 1; iter <= max_iters; iter++) {
        r.iters = iter;
        if (collapsed(xmin - xmax)) { s = SBR_NO_RUN_COLLAPSE; return; }
        if (iter == max_iters - 1) { s = SBR_NO_RUN_MAXITER; return; }
        const double xo = xnew;
        const double ic = dmin(tin, xo), oc = dmin(tout, xo);
        double Goc = 0.0, Gic = 0.0;
        if (in_range(oc, tlo, thi, trunc, flag)) Goc = lerp_at(T, G, n, ssl_range(T, 0, n - 1, oc), oc);
        if (in_range(ic, tlo, thi, trunc, flag)) Gic = lerp_at(T, G, n, ssl_range(T, 0, n - 1, ic), ic);
        if (!(xo >= tlo)) { flag |= SBR_OOB; return; } // searchsortedlast = 0: grid[0]
        const int j = ssl_range(T, 0, n - 1, xo);
        if (j + 1 >= n) { flag |= trunc ? SBR_ENGINE_TRUNC : SBR_OOB; return; }
        const double eps = T[j + 1] - T[j];
        const double xoe = oc + eps, xie = ic + eps;
        const bool oke = in_range(xoe, tlo, thi, trunc, flag);
        const bool oki = in_range(xie, tlo, thi, trunc, flag);
        if (flag) return;
        const double AW = Goc - Gic;
        const double err = AW - kappa;
        if (fabs(err) <= tolerance) {
            double Goce = 0.0, Gice = 0.0;
            if (oke) Goce = lerp_at(T, G, n, ssl_range(T, 0, n - 1, xoe), xoe);
            if (oki) Gice = lerp_at(T, G, n, ssl_range(T, 0, n - 1, xie), xie);
            if (Goce - Gice >= AW) { s = SBR_RUN; xi = xo; tolr = fabs(err); }
            else s = SBR_FALSE_EQ;
            return;
        } else if (err > 0) {
            xmax = xo; xnew = 0.5 * (xo + xmin);
        } else {
            xmin = xo; xnew = 0.5 * (xo + xmax);
        }
    }
}

}  // namespace sbr
