// sbr_point_dev.h — one point by a whole workgroup: wave-wide searches (wave_ssl), the solve on one
// wave (point_wave) and get_AW over every τ̄ knot by the block (co_eval), shared by
// point_coop_kernel and points_kernel.  Device code; include from a .hip file.
#pragma once

#include "sbr_device.h"
#include "sbr_kernels.h"
#include "sbr_scan.h"
#include "sbr_solve_dev.h"

namespace sbr {

constexpr int CO_BLOCK = 256;

// searchsortedlast in [lo, hi] (ssl_range's result for sorted t: lo + #{j in (lo, hi] : t[j] <= x})
// by the 64 lanes of a wave; every lane returns the same index.  Call with the whole wave active.
template <class P>
__device__ __forceinline__ int wave_ssl(P t, int lo, int hi, double x)
{
    const int lane = threadIdx.x & 63;
    if (lo >= hi) return lo; // a one-knot bracket (most bisection iterates once narrowed)
    while (hi - lo > 64) {
        const int step = (hi - lo + 63) >> 6; // probes lo + k·step, k = 1..64 (those <= hi)
        const int pk = lo + (lane + 1) * step;
        const bool pr = pk <= hi && t[pk <= hi ? pk : hi] <= x;
        const int c = __popcll(__ballot(pr)); // the true probes are a prefix (t sorted)
        const int nhi = lo + (c + 1) * step - 1;
        hi = nhi < hi ? nhi : hi;
        lo = lo + c * step;
    }
    const int pk = lo + 1 + lane;
    const bool pr = pk <= hi && t[pk <= hi ? pk : hi] <= x;
    return lo + __popcll(__ballot(pr));
}

// lane k's double (k wave-uniform)
__device__ __forceinline__ double co_rl(double x, int k)
{
    const uint64_t u = sbr_dbits(x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, k);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), k);
    return sbr_bitsd(((uint64_t)hi << 32) | lo);
}

// wave-uniform in_range (the flag as solve_from_buffers sets it)
__device__ __forceinline__ bool co_in_range(double x, double tlo, double thi, bool trunc, uint32_t& flag)
{
    if (x >= tlo && x <= thi) return true;
    flag |= (trunc && x > thi) ? SBR_ENGINE_TRUNC : SBR_OOB;
    return false;
}

template <class P>
__device__ __forceinline__ void point_wave(P T, P G, P H, const int n, const int ntau, const int nle,
                                           const double ETA, const double T1, const bool trunc, const double u,
                                           const double kappa, const int max_iters, const uint32_t lbits,
                                           PointResult& r, const double guess)
{
    const int lane = threadIdx.x & 63;
    r.xi = NAN; r.aw = NAN; r.tol = INFINITY; r.iters = 0; r.status = 0;
    // ---------------- optimal_buffer (solver.jl:211-264), 64 τ̄ entries per round ----------------
    bool any = false, all = true;
    int fa = -1, la = -1, cin = -1, cout = -1;
    for (int b0 = 0; b0 < ntau; b0 += 64) {
        const int i = b0 + lane;
        const bool in = i < ntau;
        const bool ab = in && H[in ? i : 0] > u;
        const bool pv = in && i > 0 && H[i > 0 && in ? i - 1 : 0] > u;
        const unsigned long long mab = __ballot(ab), min_ = __ballot(in);
        any |= mab != 0ull;
        all &= (mab & min_) == min_;
        if (mab) {
            if (fa < 0) fa = b0 + __ffsll((long long)mab) - 1;
            la = b0 + 63 - __clzll((long long)mab);
        }
        const unsigned long long mi = __ballot(in && i > 0 && !pv && ab); // 0 → 1 at i: cin = i − 1
        const unsigned long long mo = __ballot(in && i > 0 && pv && !ab); // 1 → 0 at i: cout = i − 1
        if (cin < 0 && mi) cin = b0 + __ffsll((long long)mi) - 2;
        if (mo) cout = b0 + 63 - __clzll((long long)mo) - 1;
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
    const double tlo = T[0], thi = T[n - 1];
    if (tin == tout) {
        r.status = SBR_NO_RUN_HR_BELOW_U | SBR_CONVERGED | lbits;
        r.tol = 0.0;
        return;
    }
    // ---------------- compute_ξ (solver.jl:308-376): the exact iteration ----------------
    uint32_t flag = 0;
    const double tolerance = 10.0 * sbr_jl_eps(kappa);
    uint32_t s = SBR_NO_RUN_MAXITER;
    double xi = NAN, tolr = INFINITY;
    if (guess == guess) { // ξ_guess: the plain iteration (solve_from_buffers), wave-uniform
        bisect_plain(T, G, n, tlo, thi, trunc, tin, tout, guess, kappa, tolerance, max_iters, r, flag, s, xi, tolr);
    } else {
    double xnew = (tin + tout) / 2.0, xmin = tin, xmax = tout;
    const bool okmin = co_in_range(xmin, tlo, thi, trunc, flag);
    const bool okmax = co_in_range(xmax, tlo, thi, trunc, flag);
    if (!okmin || !okmax) { // the BoundsError of the reference's first iteration (solve_from_buffers)
        if (max_iters >= 1) {
            r.iters = 1;
            r.status = (collapsed(xmin - xmax) ? SBR_NO_RUN_COLLAPSE : max_iters == 2 ? SBR_NO_RUN_MAXITER : flag) | lbits;
        } else {
            r.status = SBR_NO_RUN_MAXITER | lbits;
        }
        return;
    }
    // brackets [jlo, jhi] hold the iterates of a moderate grid; elsewhere a midpoint may overflow past ξmax
    const bool moderate = tlo >= -0x1p1000 && thi <= 0x1p1000;
    int jlo = wave_ssl(T, 0, n - 1, xmin);
    int jhi = wave_ssl(T, 0, n - 1, xmax);
    const int jtin = jlo;
    // Rounds of six bisection levels at once: lane ℓ < 63 evaluates node k = ℓ + 1 of the
    // depth-6 tree below the current state (heap order; child 2k follows err > 0, 2k + 1
    // err < 0), replaying its path's midpoint arithmetic exactly, then the wave walks the tree
    // with the nodes' signs.  Each node runs the serial iteration's tests in its order; the walk
    // stops at the first terminal node on the path — the iteration where the serial loop breaks,
    // with its counters, flags and (for |err| <= tol) the slope probe, done by the whole wave.
    int iter0 = 1;
    for (;;) {
        const int k = lane + 1;
        const int d = 31 - __builtin_clz(k);
        double nmin = xmin, nmax = xmax, xo = xnew;
        for (int b = d - 1; b >= 0; b--) {
            if (((k >> b) & 1) == 0) { nmax = xo; xo = 0.5 * (xo + nmin); }
            else { nmin = xo; xo = 0.5 * (xo + nmax); }
        }
        const int it = iter0 + d;
        int term = 0; // 1 collapse, 2 max_iters − 1, 3 range flag, 4 |err| <= tol, 5 past max_iters
        uint32_t nflag = 0;
        double err = 0.0, AW = 0.0, oc = 0.0, ic = 0.0, xoe = 0.0, xie = 0.0;
        int j = 0, joc = 0, jic = 0;
        bool oke = false, oki = false;
        if (lane < 63) {
            if (it > max_iters) term = 5;
            else if (collapsed(nmin - nmax)) term = 1;
            else if (it == max_iters - 1) term = 2;
            else {
                ic = dmin(tin, xo); oc = dmin(tout, xo);
                j = moderate ? ssl_range(T, jlo, jhi, xo) : ssl_range(T, 0, n - 1, xo);
                const bool ok = co_in_range(oc, tlo, thi, trunc, nflag);
                joc = (oc == xo) ? j : (ok ? ssl_range(T, 0, n - 1, oc) : 0);
                const double Goc = ok ? lerp_at(T, G, n, joc, oc) : 0.0;
                double Gic = 0.0;
                if (co_in_range(ic, tlo, thi, trunc, nflag)) {
                    jic = (ic == tin) ? jtin : (ic == xo ? j : ssl_range(T, 0, n - 1, ic));
                    Gic = lerp_at(T, G, n, jic, ic);
                }
                if (j + 1 >= n) {
                    nflag |= trunc ? SBR_ENGINE_TRUNC : SBR_OOB;
                    term = 3;
                } else {
                    const double eps = T[j + 1] - T[j];
                    xoe = oc + eps; xie = ic + eps;
                    oke = co_in_range(xoe, tlo, thi, trunc, nflag);
                    oki = co_in_range(xie, tlo, thi, trunc, nflag);
                    if (nflag) term = 3;
                    else {
                        AW = Goc - Gic;
                        err = AW - kappa;
                        if (fabs(err) <= tolerance) term = 4;
                    }
                }
            }
        }
        int node = 1, stop = 0;
        for (int lev = 0; lev < 6 && !stop; lev++) {
            const int src = node - 1;
            const int t_ = __builtin_amdgcn_readlane(term, src);
            if (t_) {
                stop = 1;
                r.iters = t_ == 5 ? max_iters : iter0 + lev;
                if (t_ == 1) s = SBR_NO_RUN_COLLAPSE;
                else if (t_ == 2) s = SBR_NO_RUN_MAXITER;
                else if (t_ == 3) flag |= (uint32_t)__builtin_amdgcn_readlane((int)nflag, src);
                else if (t_ == 4) {
                    const double xo_t = co_rl(xo, src), AW_t = co_rl(AW, src), err_t = co_rl(err, src);
                    const double xoe_t = co_rl(xoe, src), xie_t = co_rl(xie, src);
                    const int joc_t = __builtin_amdgcn_readlane(joc, src), jic_t = __builtin_amdgcn_readlane(jic, src);
                    const bool oke_t = __builtin_amdgcn_readlane(oke ? 1 : 0, src) != 0;
                    const bool oki_t = __builtin_amdgcn_readlane(oki ? 1 : 0, src) != 0;
                    double Goce = 0.0, Gice = 0.0;
                    if (oke_t) Goce = lerp_at(T, G, n, wave_ssl(T, joc_t, n - 1, xoe_t), xoe_t);
                    if (oki_t) Gice = lerp_at(T, G, n, wave_ssl(T, jic_t, n - 1, xie_t), xie_t);
                    const double AWe = Goce - Gice;
                    if (AWe >= AW_t) { s = SBR_RUN; xi = xo_t; tolr = fabs(err_t); }
                    else s = SBR_FALSE_EQ;
                }
                break;
            }
            const double e_ = co_rl(err, src);
            const int j_ = __builtin_amdgcn_readlane(j, src);
            if (e_ > 0) jhi = j_; else jlo = j_;
            if (lev == 5) { // the next round's state: the child of this depth-5 node
                const double xs = co_rl(xo, src), mn = co_rl(nmin, src), mxv = co_rl(nmax, src);
                if (e_ > 0) { xmin = mn; xmax = xs; xnew = 0.5 * (xs + mn); }
                else { xmin = xs; xmax = mxv; xnew = 0.5 * (xs + mxv); }
            }
            node = 2 * node + (e_ > 0 ? 0 : 1);
        }
        if (stop) break;
        iter0 += 6;
    }
    } // default first iterate
    if (flag) { r.status = flag | lbits; return; }
    if (s != SBR_RUN) { r.status = s | lbits; return; }
    // the AW stage's own range checks (solve_from_buffers: G(0), then the path's last τ̄ — the
    // shifted arguments are nondecreasing, so the first failing knot fails there too)
    if (!co_in_range(0.0, tlo, thi, trunc, flag)) { r.status = flag | lbits; return; }
    const double icc = (tin >= xi) ? xi : tin;
    const double occ = (tout > xi) ? xi : tout;
    const double al = (tau(ntau - 1) - xi) + icc, bl = (tau(ntau - 1) - xi) + occ;
    if (!((al > 0 ? al : 0.0) <= thi) || !((bl > 0 ? bl : 0.0) <= thi)) {
        r.status = (trunc ? SBR_ENGINE_TRUNC : SBR_OOB) | lbits;
        return;
    }
    r.xi = xi;
    r.tol = tolr;
    r.status = SBR_RUN | SBR_CONVERGED | lbits; // r.aw: the block's get_AW pass
}

// get_AW on τ̄ entries [i0, i1) with brackets slid along (eval_range's arithmetic); NaN-latching
// max into mx (Julia maximum), paths written when given
template <class P>
__device__ __forceinline__ void co_eval(P T, P G, const int n, const int nle, const double ETA, const double xi,
                                        const double icc, const double occ, const double G0, const int i0,
                                        const int i1, double& mx, double* __restrict__ aw_cum,
                                        double* __restrict__ aw_out, double* __restrict__ aw_in)
{
    if (i0 >= i1) return;
    auto tau = [&](int i) -> double { return i < nle ? T[i] : ETA; };
    auto x_of = [&](int i, double c) { const double v = (tau(i) - xi) + c; return v > 0 ? v : 0.0; };
    int ka = ssl_range(T, 0, n - 1, x_of(i0, icc)), kb = ssl_range(T, 0, n - 1, x_of(i0, occ));
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
        while (ka < n - 2 && ta1 <= xa) { ka++; ta0 = ta1; ga0 = ga1; ta1 = T[ka + 1]; ga1 = G[ka + 1]; }
        while (kb < n - 2 && tb1 <= xb) { kb++; tb0 = tb1; gb0 = gb1; tb1 = T[kb + 1]; gb1 = G[kb + 1]; }
        const double da = (xa - ta0) / (ta1 - ta0);
        const double gi = ga0 * (1.0 - da) + ga1 * da;
        double go;
        if (xb == tb0) go = gb0 * 1.0 + gb1 * 0.0; // eval_range's δ = 0 form (the same value)
        else { const double db = (xb - tb0) / (tb1 - tb0); go = gb0 * (1.0 - db) + gb1 * db; }
        const double awin = av >= 0 ? gi : 0.0;
        const double awout = bv >= 0 ? go : 0.0;
        const double v = (awout - awin) + G0;
        if (aw_cum) aw_cum[i] = v;
        if (aw_out) aw_out[i] = awout;
        if (aw_in) aw_in[i] = awin;
        if (mx == mx && (v != v || v > mx)) mx = v;
    }
}

}  // namespace sbr
