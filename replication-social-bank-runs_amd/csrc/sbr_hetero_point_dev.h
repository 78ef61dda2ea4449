// sbr_hetero_point_dev.h — the heterogeneity extension's per-point solve for a compile-time group
// count K: HCol (one column's knots, group CDFs and hazard rows) and solve_hetero_point<K> (K
// crossing scans, compute_ξ_hetero, the validity check, AW_max), moved here verbatim from
// sbr_hetero.hip and shared by two translation units:
//   sbr_hetero.hip        equilibrium_hetero_kernel<K, BLOCK, MODE>        one lane per (column, u)
//   sbr_hetero_econ.hip   equilibrium_hetero_econ_kernel<K, BLOCK, MODE>   one lane per (column, class, κ, u)
// κ and u are by-value arguments of the solve, so both kernels run the same operations per point.
#pragma once

#include "sbr_device.h"
#include "sbr_kernels.h"
#include "sbr_scan.h"

namespace sbr {

// ---------------------------------------------------------------------------
// per-point solve
// ---------------------------------------------------------------------------
template <int K, class PT>
struct HCol {
    PT T;                       // knot times (LDS or global)
    const double* __restrict__ G;   // [n][K]
    const double* __restrict__ H;   // [K][cap]
    int n, ntau, nle;
    size_t cap;
    double ETA, T1;
    const double* __restrict__ hsum; // [2][K][nblk] per-64 HR block max / min (LDS), or null
    int nblk;
    __device__ __forceinline__ double tau(int i) const { return i < nle ? T[i] : ETA; }
    __device__ __forceinline__ double g(int j, int k) const { return G[(size_t)j * K + k]; }
    // Interpolations gridded-linear value of group k on bracket j (clamped)
    __device__ __forceinline__ double lerp(int j, int k, double x) const
    {
        if (j > n - 2) j = n - 2;
        if (j < 0) j = 0;
        const double d = (x - T[j]) / (T[j + 1] - T[j]);
        return g(j, k) * (1.0 - d) + g(j + 1, k) * d;
    }
};

constexpr int kHetUbcBits = 16; // bound-code width (8: 29.8 ms alone, the 1/256 window recomputes)
typedef unsigned short ubc_t;
template <int K, class PT>
__device__ __forceinline__ void solve_hetero_point(const HCol<K, PT>& C, const double* __restrict__ dist,
                                                   const double u, const double kappa, const int max_iters,
                                                   const double tolerance, const uint32_t lbits, double& xi_o,
                                                   double& aw_o, double& tol_o, uint32_t& st_o, int& it_o,
                                                   double* tin, double* tout, const bool mono, const int diag,
                                                   double* __restrict__ aw_path, const double env, const bool sep,
                                                   const int koff,
                                                   double* __restrict__ tin_g, double* __restrict__ tout_g,
                                                   ubc_t* __restrict__ ubc = nullptr, const int ubc_stride = 0,
                                                   const int ubc_rows = 0)
{
    xi_o = NAN; aw_o = NAN; tol_o = INFINITY; it_o = 0;
    const int n = C.n;
    const double tlo = C.T[0], thi = C.T[n - 1];
    // ---------------- K crossing scans (optimal_buffer per group) ----------------
    bool all_eq = true;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const double* __restrict__ Hk = C.H + (size_t)k * C.cap;
        bool any = false, all = true, prev = false;
        int fa = -1, la = -1, cin = -1, cout = -1;
        if (C.hsum) {
            struct { const double* hmax; const double* hmin; } S{C.hsum + (size_t)k * C.nblk,
                                                                 C.hsum + (size_t)(K + k) * C.nblk};
            buffer_scan_blocked(Hk, S, C.ntau, u, any, all, fa, la, cin, cout);
        } else {
            for (int i = 0; i < C.ntau; i++) {
                const bool ab = Hk[i] > u;
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
        double a, b;
        if (!any) {
            a = C.T1; b = C.T1;
        } else if (all) {
            a = C.tau(0); b = C.tau(C.ntau - 1);
        } else {
            a = C.T1; b = C.T1;
            if (cin >= 0) {
                const double t0 = C.tau(cin), t1 = C.tau(cin + 1), h0 = Hk[cin], h1 = Hk[cin + 1];
                a = t0 + ((u - h0) * (t1 - t0)) / (h1 - h0);
            }
            if (cout >= 0) {
                const double t0 = C.tau(cout), t1 = C.tau(cout + 1), h0 = Hk[cout], h1 = Hk[cout + 1];
                b = t0 + ((u - h0) * (t1 - t0)) / (h1 - h0);
            }
            if (a == C.T1) a = C.tau(fa);
            if (b == C.T1) b = C.tau(la);
        }
        tin[k] = a;
        tout[k] = b;
        all_eq = all_eq && (a == b);
    }
    // the buffers are final here: store them now, so that they need no registers through the
    // validity check and the AW phase (only min(τ_k, ξ) is live there)
    if (tin_g)
#pragma unroll
        for (int k = 0; k < K; k++) tin_g[k] = tin[k];
    if (tout_g)
#pragma unroll
        for (int k = 0; k < K; k++) tout_g[k] = tout[k];
    if (all_eq) {
        st_o = SBR_NO_RUN_HR_BELOW_U | SBR_CONVERGED | lbits;
        tol_o = 0.0;
        return;
    }
    if (diag & 1) return; // timing diagnostics: stop after the crossing scans
    // ---------------- compute_ξ_hetero ----------------
    uint32_t flag = 0;
    double guess = (dist[0] * (tin[0] + tout[0])) / 2.0;
    double mo = tout[0];
#pragma unroll
    for (int k = 1; k < K; k++) { guess = guess + (dist[k] * (tin[k] + tout[k])) / 2.0; mo = dmax(mo, tout[k]); }
    double xmin = 0.0, xmax = mo * 2.0, xnew = guess;
    // exact brackets and values of the constant lookup points tin_k, tout_k
    int jin[K], jout[K];
    double gin[K], gout[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        jin[k] = -1; jout[k] = -1; gin[k] = 0.0; gout[k] = 0.0;
        if (tin[k] >= tlo && tin[k] <= thi) { jin[k] = ssl_range(C.T, 0, n - 1, tin[k]); gin[k] = C.lerp(jin[k], k, tin[k]); }
        if (tout[k] >= tlo && tout[k] <= thi) { jout[k] = ssl_range(C.T, 0, n - 1, tout[k]); gout[k] = C.lerp(jout[k], k, tout[k]); }
    }
    int jlo = 0, jhi = n - 1;
    uint32_t s = SBR_NO_RUN_MAXITER;
    double xi = NAN, tolr = INFINITY;
    bool term = false;
    double xt = 0.0, et = 0.0, awt = 0.0, errt = 0.0;
    int jt = 0;
    for (int iter = 1; iter <= max_iters; iter++) {
        it_o = iter;
        const double dd = xmin - xmax;
        if (collapsed(dd)) { s = SBR_NO_RUN_COLLAPSE; break; }
        if (iter == max_iters - 1) { s = SBR_NO_RUN_MAXITER; break; }
        const double xo = xnew;
        if (!(xo >= tlo)) { flag |= SBR_OOB; break; }  // searchsortedlast = 0: BoundsError
        const int j = ssl_range(C.T, jlo, jhi, xo); // t[jlo] <= ξmin <= xo <= ξmax < t[jhi+1]
        const int i2 = j + 1 < n - 1 ? j + 1 : n - 1;
        const double eps = C.T[i2] - C.T[j];
        double AW = 0.0;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const double ic = dmin(tin[k], xo), oc = dmin(tout[k], xo);
            // value and bracket of oc, ic (each is either xo or the group constant)
            int joc, jic;
            double Goc, Gic;
            if (oc == xo) { joc = xo <= thi ? j : -1; Goc = joc >= 0 ? C.lerp(j, k, xo) : 0.0; }
            else { joc = jout[k]; Goc = gout[k]; }
            if (ic == xo) { jic = xo <= thi ? j : -1; Gic = jic >= 0 ? C.lerp(j, k, xo) : 0.0; }
            else { jic = jin[k]; Gic = gin[k]; }
            if (joc < 0 || jic < 0) flag |= SBR_OOB;
            // the slope probe only decides the terminal iterate: range checks every
            // iterate (BoundsError order of heterogeneity_solver.jl:81-95), lerps later
            const double xoe = oc + eps, xie = ic + eps;
            if (!(xoe <= thi && joc >= 0)) flag |= SBR_OOB;
            if (!(xie <= thi && jic >= 0)) flag |= SBR_OOB;
            AW = AW + dist[k] * (Goc - Gic);
        }
        if (flag) break;
        const double err = AW - kappa;
        if (fabs(err) <= tolerance) {
            // the terminal iterate: its slope probe runs after the loop, where the bracket state and
            // the constant lookups are dead (inside the loop it spilled them to scratch)
            term = true;
            xt = xo;
            jt = j;
            et = eps;
            awt = AW;
            errt = err;
            break;
        } else if (err > 0) {
            xmax = xo;
            jhi = j;
            xnew = 0.5 * (xo + xmin);
        } else {
            xmin = xo;
            jlo = j;
            xnew = 0.5 * (xo + xmax);
        }
    }
    if (flag) { st_o = flag | lbits; return; }
    if (term) {
        double AWe = 0.0;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const double ic = dmin(tin[k], xt), oc = dmin(tout[k], xt);
            const int joc = oc == xt ? jt : jout[k], jic = ic == xt ? jt : jin[k];
            const double xoe = oc + et, xie = ic + et;
            const double Goce = C.lerp(ssl_gallop(C.T, n, joc, xoe), k, xoe);
            const double Gice = C.lerp(ssl_gallop(C.T, n, jic, xie), k, xie);
            AWe = AWe + dist[k] * (Goce - Gice);
        }
        if (AWe >= awt) { s = SBR_RUN; xi = xt; tolr = fabs(errt); }
        else s = SBR_FALSE_EQ;
    }
    if (s != SBR_RUN) { st_o = s | lbits; return; }
    if (diag & 2) return; // ... after the bisection

    // ---------------- is_valid_equilibrium_hetero ----------------
    // valid ⇔ no knot pair (t_{i−1}, t_i), t_i ≤ ξ, with AW(t_{i−1}) > κ ≥ AW(t_i), where
    // AW(t) = Σ dist_k (G_k(t) − G_k(max(0, t − τ_I,k))) (heterogeneity_solver.jl:190-207).
    {
        double tI[K];
        int jp[K];
#pragma unroll
        for (int k = 0; k < K; k++) { tI[k] = dmax(0.0, xi - tin[k]); jp[k] = 0; }
        bool prev = false, valid = true;
        // the reference's per-knot test on knots [i0, i1) with walkers jp at x(t_i0)'s bracket
        auto exact = [&](int i0, int i1) {
            for (int i = i0; i < i1; i++) {
                const double ti = C.T[i];
                double aw = 0.0;
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const double a = C.lerp(i, k, ti);
                    const double x = dmax(0.0, ti - tI[k]);
                    while (jp[k] + 1 < n && C.T[jp[k] + 1] <= x) jp[k]++;
                    const double bb = C.lerp(jp[k], k, x);
                    aw = aw + dist[k] * (a - bb);
                }
                const bool above = aw > kappa;
                if (i > 0 && prev && !above) { valid = false; return; }
                prev = above;
            }
        };
        const int m = ssl_range(C.T, 0, n - 1, xi) + 1; // knots with t ≤ ξ (ξ ≥ t_0 here)
        if (!mono) {
            exact(0, m);
        } else {
            // 64-knot blocks bounded as in AW_max (G_k nondecreasing up to Δ_k): a block whose
            // bounds put every knot on one side of κ is decided without evaluating it; only
            // blocks straddling κ (near the crossing) are evaluated knot by knot.
            int hl[K], hh[K];
#pragma unroll
            for (int k = 0; k < K; k++) { hl[k] = 0; hh[k] = 0; }
            for (int i0 = 0; i0 < m && valid; i0 += 64) {
                const int i1 = (i0 + 64 < m ? i0 + 64 : m) - 1;
                double lb = 0.0, ub = 0.0;
#pragma unroll
                for (int k = 0; k < K; k++) {
                    // hints: the previous block's last bracket, then this block's first + its width
                    hl[k] = ssl_near(C.T, n, hh[k], dmax(0.0, C.T[i0] - tI[k]));
                    hh[k] = ssl_near(C.T, n, hl[k] + (i1 - i0), dmax(0.0, C.T[i1] - tI[k]));
                    const int kh = hh[k] + 1 < n - 1 ? hh[k] + 1 : n - 1;
                    lb = lb + dist[k] * (C.g(i0, k) - C.g(kh, k));
                    ub = ub + dist[k] * (C.g(i1, k) - C.g(hl[k], k));
                }
                lb = (lb - env) - 1e-14;
                ub = (ub + env) + 1e-14;
                if (ub <= kappa) {        // every knot not above κ
                    if (i0 > 0 && prev) valid = false;
                    prev = false;
                } else if (lb > kappa) {  // every knot above κ
                    prev = true;
                } else {
#pragma unroll
                    for (int k = 0; k < K; k++) jp[k] = hl[k];
                    exact(i0, i1 + 1);
                }
            }
        }
        if (!valid) { st_o = SBR_HETERO_INVALID | lbits; return; }
    }
    if (diag & 4) return; // ... after the validity check
    // ---------------- AW_max over the whole learning grid ----------------
    double icc[K], occ[K];
#pragma unroll
    for (int k = 0; k < K; k++) { icc[k] = dmin(tin[k], xi); occ[k] = dmin(tout[k], xi); }
    double mx = -INFINITY;
    // exact AW_total(t_i) for i in [i0, i1), walkers started by searches from per-group hints
    int ha[K], hb[K];
#pragma unroll
    for (int k = 0; k < K; k++) { ha[k] = 0; hb[k] = 0; }
    // the knot index each hint set was found for: a later search for knot i starts from
    // hint + (i − that index) (the shifted arguments move with the knots), not from the hint
    int ia = 0, ib = 0;
    auto eval_range = [&](int i0, int i1) {
        int ja[K], jb[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const double av = (C.T[i0] - xi) + icc[k], bv = (C.T[i0] - xi) + occ[k];
            ha[k] = ssl_near(C.T, n, ha[k] + (i0 - ia), av > 0 ? av : 0.0);
            hb[k] = ssl_near(C.T, n, hb[k] + (i0 - ib), bv > 0 ? bv : 0.0);
            ja[k] = ha[k];
            jb[k] = hb[k];
        }
        ia = i0;
        ib = i0;
        for (int i = i0; i < i1; i++) {
            const double ti = C.T[i];
            double cum = 0.0;
            // Interpolation weights shared between groups: groups with the same shift
            // (occ_k = ξ for most, equal icc_k where τ_IN,k ≥ ξ) have the same argument, bracket and
            // weight δ, so δ is divided out once; and a b argument on a knot (t_i − ξ + ξ == t_i)
            // has δ = 0 exactly — the same operands and operations as C.lerp, fewer divisions
            double xa_p = NAN, da_p = 0.0, xb_p = NAN, db_p = 0.0;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const double av = (ti - xi) + icc[k];
                const double bv = (ti - xi) + occ[k];
                const double xa = av > 0 ? av : 0.0;
                const double xb = bv > 0 ? bv : 0.0;
                if (!(xa <= thi) || !(xb <= thi)) flag |= SBR_OOB;
                while (ja[k] + 1 < n && C.T[ja[k] + 1] <= xa) ja[k]++;
                while (jb[k] + 1 < n && C.T[jb[k] + 1] <= xb) jb[k]++;
                const int qa = ja[k] > n - 2 ? n - 2 : (ja[k] < 0 ? 0 : ja[k]);
                const int qb = jb[k] > n - 2 ? n - 2 : (jb[k] < 0 ? 0 : jb[k]);
                double da = da_p, db = db_p;
                if (!(xa == xa_p)) da = (xa - C.T[qa]) / (C.T[qa + 1] - C.T[qa]);
                if (!(xb == xb_p)) {
                    const double t0 = C.T[qb], t1 = C.T[qb + 1];
                    db = (xb == t0 && t1 > t0) ? 0.0 : (xb - t0) / (t1 - t0);
                }
                xa_p = xa; da_p = da; xb_p = xb; db_p = db;
                const double gi = C.g(qa, k) * (1.0 - da) + C.g(qa + 1, k) * da;
                const double go = C.g(qb, k) * (1.0 - db) + C.g(qb + 1, k) * db;
                const double awin = av >= 0 ? gi : 0.0;
                const double awout = bv >= 0 ? go : 0.0;
                cum = cum + dist[k] * (awout - awin);
            }
            if (aw_path) aw_path[i] = cum;
            if (mx == mx && (cum != cum || cum > mx)) mx = cum;
        }
    };
    if (!mono) {
        eval_range(0, n);
    } else {
        // Every group CDF is nondecreasing on the knots up to its drawdown Δ_k, so over knots
        // [i0, i1] AW_OUT,k is at most G_k at the knot after b_k(t_i1)'s bracket + Δ_k and AW_IN,k
        // at least G_k at a_k(t_i0)'s bracket − Δ_k (0 where masked; `env` = Σ dist_k·2Δ_k):
        // branch and bound over 256/64/8-knot ranges,
        // the same maximum with a fraction of the K·2 lerps per knot.  Arguments are
        // nondecreasing in i, so the last knot's range check covers the whole path.
#pragma unroll
        for (int k = 0; k < K; k++) {
            const double av = (C.T[n - 1] - xi) + icc[k], bv = (C.T[n - 1] - xi) + occ[k];
            if (!((av > 0 ? av : 0.0) <= thi) || !((bv > 0 ? bv : 0.0) <= thi)) flag |= SBR_OOB;
        }
        auto ub_rng = [&](int i0, int i1) -> double {
            double sum = 0.0;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const double bv = (C.T[i1] - xi) + occ[k];
                double hi = 0.0;
                if (sep && occ[k] == xi) {
                    // b_k(t_i1) = (t_i1 − ξ) + ξ lies within an ulp of t_i1, below t[i1 + koff] (knots
                    // koff apart are farther apart than that, `sep`): G_k at the knot after its
                    // bracket is G_k at a knot <= i1 + koff, no search
                    const double g = C.g(i1 + koff < n - 1 ? i1 + koff : n - 1, k);
                    hi = g > 0.0 ? g : 0.0;
                    hb[k] = i1; // with ib = i1 below, the next hint hb + (i − ib) is i itself
                } else if (bv >= 0) {
                    hb[k] = ssl_near(C.T, n, hb[k] + (i1 - ib), bv);
                    const double g = C.g(hb[k] + 1 < n - 1 ? hb[k] + 1 : n - 1, k);
                    hi = g > 0.0 ? g : 0.0;
                }
                const double av = (C.T[i0] - xi) + icc[k];
                double lo = 0.0;
                if (av >= 0) {
                    ha[k] = ssl_near(C.T, n, ha[k] + (i0 - ia), av);
                    lo = C.g(ha[k], k);
                } else {
                    lo = C.g(0, k) < 0.0 ? C.g(0, k) : 0.0;
                }
                sum = sum + dist[k] * (hi - lo);
            }
            ia = i0;
            ib = i1;
            return (sum + 1e-14) + env;
        };
        auto end_of = [&](int i0, int w) { return i0 + w < n ? i0 + w : n; };
        if (!flag) {
            // pass 1 keeps every range bound as a code in LDS (this lane's column of ubc rows:
            // the 256-knot ranges, then the best one's four 64-knot and its eight 8-knot ranges),
            // c = ceil(S·ub) clamped to [0, S − 2] — c/S >= ub exactly (S = 2^bits: ×S is exact) —
            // or S − 1 (ub > (S − 2)/S: unknown).  Pass 2: c/S <= mx prunes, (c − 1)/S >= mx
            // descends (ub > mx), in between — and for rows past ubc_rows, the LDS left — the bound
            // is recomputed (ub_rng's value does not depend on the hints).
            constexpr double S = (double)(1 << kHetUbcBits), rS = 1.0 / S;
            constexpr int unk = (1 << kHetUbcBits) - 1;
            const int nr = (n + 255) >> 8;
            auto put = [&](int row, double ub) {
                if (row >= ubc_rows) return;
                const double q = ceil(ub * S);
                ubc[row * ubc_stride] = (ubc_t)(q != q || q > S - 2.0 ? unk : (q < 0.0 ? 0 : (int)q));
            };
            auto pruned = [&](int row, int i0, int i1) -> bool {
                if (row < ubc_rows) {
                    const int cv = ubc[row * ubc_stride];
                    if (cv != unk) {
                        if ((double)cv * rS <= mx) return true;
                        if ((double)(cv - 1) * rS >= mx) return false;
                    }
                }
                return ub_rng(i0, i1) <= mx;
            };
            int bs = 0;
            double bu = -INFINITY;
            for (int i0 = 0; i0 < n; i0 += 256) {
                const double ub = ub_rng(i0, end_of(i0, 256) - 1);
                put(i0 >> 8, ub);
                if (!(ub <= bu)) { bu = ub; bs = i0; }
            }
            int bb = bs;
            bu = -INFINITY;
            for (int i0 = bs; i0 < end_of(bs, 256); i0 += 64) {
                const double ub = ub_rng(i0, end_of(i0, 64) - 1);
                put(nr + ((i0 - bs) >> 6), ub);
                if (!(ub <= bu)) { bu = ub; bb = i0; }
            }
            int b8 = bb;
            bu = -INFINITY;
            for (int i0 = bb; i0 < end_of(bb, 64); i0 += 8) {
                const double ub = ub_rng(i0, end_of(i0, 8) - 1);
                put(nr + 4 + ((i0 - bb) >> 3), ub);
                if (!(ub <= bu)) { bu = ub; b8 = i0; }
            }
            eval_range(b8, end_of(b8, 8));
            for (int s0 = 0; s0 < n && mx == mx; s0 += 256) {
                const int se = end_of(s0, 256);
                if (pruned(s0 >> 8, s0, se - 1)) continue;
                for (int k0 = s0; k0 < se && mx == mx; k0 += 64) {
                    const int ke = end_of(k0, 64);
                    if (s0 == bs ? pruned(nr + ((k0 - bs) >> 6), k0, ke - 1) : (ub_rng(k0, ke - 1) <= mx)) continue;
                    for (int i0 = k0; i0 < ke && mx == mx; i0 += 8) {
                        const int ie = end_of(i0, 8);
                        if (i0 == b8) continue;
                        if (k0 == bb ? pruned(nr + 4 + ((i0 - bb) >> 3), i0, ie - 1) : (ub_rng(i0, ie - 1) <= mx))
                            continue;
                        eval_range(i0, ie);
                    }
                }
            }
        }
    }
    if (flag) { st_o = flag | lbits; return; }
    xi_o = xi;
    tol_o = tolr;
    aw_o = mx;
    st_o = SBR_RUN | SBR_CONVERGED | lbits;
}

constexpr int kHetBlock = 256; // u points per hetero equilibrium workgroup (512 was slower)
constexpr int kHetMinW = 2; // waves per SIMD: two 4-wave workgroups per CU (LDS slab: kHetLds in sbr_ctx.h)

}  // namespace sbr
