// sbr_hetero_wide_dev.h — the heterogeneity extension's per-point solve with the group count K a
// runtime argument: HColW, WideState and solve_hetero_point_wide<BLOCK>, moved here verbatim from
// sbr_hetero_wide.hip and shared by two translation units:
//   sbr_hetero_wide.hip        equilibrium_hetero_wide_kernel<BLOCK, MODE>        one lane per (column, u)
//   sbr_hetero_econ_wide.hip   equilibrium_hetero_econ_wide_kernel<BLOCK, MODE>   one lane per (column, class, κ, u)
#pragma once

#include "sbr_device.h"
#include "sbr_kernels.h"
#include "sbr_scan.h"

namespace sbr {

template <class PT>
struct HColW {
    PT T;                           // knot times (LDS or global)
    const double* __restrict__ G;   // [n][K]
    const double* __restrict__ H;   // [K][cap]
    int K, n, ntau, nle;
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

// this lane's columns of the per-group LDS arrays (group k at [k·BLOCK])
struct WideState {
    double *tin, *tout, *gin, *gout;
    int *jin, *jout;
};
constexpr int kWideStateBytes = 4 * 8 + 2 * 4; // per group and lane

template <int BLOCK, class PT>
__device__ __forceinline__ void solve_hetero_point_wide(const HColW<PT>& C, const double* __restrict__ dist,
                                                        const double u, const double kappa, const int max_iters,
                                                        const double tolerance, const uint32_t lbits, double& xi_o,
                                                        double& aw_o, double& tol_o, uint32_t& st_o, int& it_o,
                                                        const WideState& S, const int diag,
                                                        double* __restrict__ aw_path, double* __restrict__ tin_g,
                                                        double* __restrict__ tout_g)
{
    xi_o = NAN; aw_o = NAN; tol_o = INFINITY; it_o = 0;
    const int K = C.K;
    const int n = C.n;
    const double tlo = C.T[0], thi = C.T[n - 1];
    // ---------------- K crossing scans (optimal_buffer per group) ----------------
    bool all_eq = true;
    for (int k = 0; k < K; k++) {
        const double* __restrict__ Hk = C.H + (size_t)k * C.cap;
        bool any = false, all = true, prev = false;
        int fa = -1, la = -1, cin = -1, cout = -1;
        if (C.hsum) {
            struct { const double* hmax; const double* hmin; } SU{C.hsum + (size_t)k * C.nblk,
                                                                  C.hsum + (size_t)(K + k) * C.nblk};
            buffer_scan_blocked(Hk, SU, C.ntau, u, any, all, fa, la, cin, cout);
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
        S.tin[k * BLOCK] = a;
        S.tout[k * BLOCK] = b;
        if (tin_g) tin_g[k] = a;
        if (tout_g) tout_g[k] = b;
        all_eq = all_eq && (a == b);
    }
    if (all_eq) {
        st_o = SBR_NO_RUN_HR_BELOW_U | SBR_CONVERGED | lbits;
        tol_o = 0.0;
        return;
    }
    if (diag & 1) return; // timing diagnostics: stop after the crossing scans
    // ---------------- compute_ξ_hetero ----------------
    uint32_t flag = 0;
    double guess = (dist[0] * (S.tin[0] + S.tout[0])) / 2.0;
    double mo = S.tout[0];
    for (int k = 1; k < K; k++) {
        const double a = S.tin[k * BLOCK], b = S.tout[k * BLOCK];
        guess = guess + (dist[k] * (a + b)) / 2.0;
        mo = dmax(mo, b);
    }
    double xmin = 0.0, xmax = mo * 2.0, xnew = guess;
    // exact brackets and values of the constant lookup points tin_k, tout_k
    for (int k = 0; k < K; k++) {
        const double a = S.tin[k * BLOCK], b = S.tout[k * BLOCK];
        int ji = -1, jo = -1;
        double gi = 0.0, go = 0.0;
        if (a >= tlo && a <= thi) { ji = ssl_range(C.T, 0, n - 1, a); gi = C.lerp(ji, k, a); }
        if (b >= tlo && b <= thi) { jo = ssl_range(C.T, 0, n - 1, b); go = C.lerp(jo, k, b); }
        S.jin[k * BLOCK] = ji; S.jout[k * BLOCK] = jo;
        S.gin[k * BLOCK] = gi; S.gout[k * BLOCK] = go;
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
        for (int k = 0; k < K; k++) {
            const double ic = dmin(S.tin[k * BLOCK], xo), oc = dmin(S.tout[k * BLOCK], xo);
            // value and bracket of oc, ic (each is either xo or the group constant)
            int joc, jic;
            double Goc, Gic;
            if (oc == xo) { joc = xo <= thi ? j : -1; Goc = joc >= 0 ? C.lerp(j, k, xo) : 0.0; }
            else { joc = S.jout[k * BLOCK]; Goc = S.gout[k * BLOCK]; }
            if (ic == xo) { jic = xo <= thi ? j : -1; Gic = jic >= 0 ? C.lerp(j, k, xo) : 0.0; }
            else { jic = S.jin[k * BLOCK]; Gic = S.gin[k * BLOCK]; }
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
            term = true; // the terminal iterate: its slope probe runs after the loop
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
        for (int k = 0; k < K; k++) {
            const double ic = dmin(S.tin[k * BLOCK], xt), oc = dmin(S.tout[k * BLOCK], xt);
            const int joc = oc == xt ? jt : S.jout[k * BLOCK], jic = ic == xt ? jt : S.jin[k * BLOCK];
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
    // AW(t) = Σ dist_k (G_k(t) − G_k(max(0, t − τ_I,k))) (heterogeneity_solver.jl:190-207):
    // the reference's per-knot test, one walker per group (in the jin slots)
    {
        for (int k = 0; k < K; k++) S.jin[k * BLOCK] = 0;
        bool prev = false, valid = true;
        const int m = ssl_range(C.T, 0, n - 1, xi) + 1; // knots with t ≤ ξ (ξ ≥ t_0 here)
        for (int i = 0; i < m; i++) {
            const double ti = C.T[i];
            double aw = 0.0;
            for (int k = 0; k < K; k++) {
                const double a = C.lerp(i, k, ti);
                const double tI = dmax(0.0, xi - S.tin[k * BLOCK]);
                const double x = dmax(0.0, ti - tI);
                int jp = S.jin[k * BLOCK];
                while (jp + 1 < n && C.T[jp + 1] <= x) jp++;
                S.jin[k * BLOCK] = jp;
                const double bb = C.lerp(jp, k, x);
                aw = aw + dist[k] * (a - bb);
            }
            const bool above = aw > kappa;
            if (i > 0 && prev && !above) { valid = false; break; }
            prev = above;
        }
        if (!valid) { st_o = SBR_HETERO_INVALID | lbits; return; }
    }
    if (diag & 4) return; // ... after the validity check
    // ---------------- AW_max over the whole learning grid ----------------
    // exact AW_total(t_i) at every knot; the walkers (jin / jout slots) start at the brackets of
    // the first knot's arguments
    double mx = -INFINITY;
    {
        const double t0 = C.T[0];
        for (int k = 0; k < K; k++) {
            const double icc = dmin(S.tin[k * BLOCK], xi), occ = dmin(S.tout[k * BLOCK], xi);
            const double av = (t0 - xi) + icc, bv = (t0 - xi) + occ;
            S.jin[k * BLOCK] = ssl_near(C.T, n, 0, av > 0 ? av : 0.0);
            S.jout[k * BLOCK] = ssl_near(C.T, n, 0, bv > 0 ? bv : 0.0);
        }
    }
    for (int i = 0; i < n; i++) {
        const double ti = C.T[i];
        double cum = 0.0;
        // Interpolation weights shared between groups: groups with the same shift have the same
        // argument, bracket and weight δ, so δ is divided out once; and a b argument on a knot
        // (t_i − ξ + ξ == t_i) has δ = 0 exactly — the same operands and operations as C.lerp
        double xa_p = NAN, da_p = 0.0, xb_p = NAN, db_p = 0.0;
        for (int k = 0; k < K; k++) {
            const double icc = dmin(S.tin[k * BLOCK], xi), occ = dmin(S.tout[k * BLOCK], xi);
            const double av = (ti - xi) + icc;
            const double bv = (ti - xi) + occ;
            const double xa = av > 0 ? av : 0.0;
            const double xb = bv > 0 ? bv : 0.0;
            if (!(xa <= thi) || !(xb <= thi)) flag |= SBR_OOB;
            int ja = S.jin[k * BLOCK], jb = S.jout[k * BLOCK];
            while (ja + 1 < n && C.T[ja + 1] <= xa) ja++;
            while (jb + 1 < n && C.T[jb + 1] <= xb) jb++;
            S.jin[k * BLOCK] = ja;
            S.jout[k * BLOCK] = jb;
            const int qa = ja > n - 2 ? n - 2 : (ja < 0 ? 0 : ja);
            const int qb = jb > n - 2 ? n - 2 : (jb < 0 ? 0 : jb);
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
    if (flag) { st_o = flag | lbits; return; }
    xi_o = xi;
    tol_o = tolr;
    aw_o = mx;
    st_o = SBR_RUN | SBR_CONVERGED | lbits;
}

constexpr size_t kWideLdsBytes = 160 * 1024; // LDS of a gfx950 CU, all of it one workgroup's

}  // namespace sbr
