// sbr_eq_column_body.h — the body of eq_column (sbr_eq_dev.h), included once per kind of point.
// No include guard: the including function supplies its signature (b, j0, j1, L, eta, t_end, u, a, ia,
// out, smem and the template parameters BLOCK, INTEREST, MODE) and these macros:
//   SBR_EQ_U(j), SBR_EQ_KAPPA(j)   the u and κ of point j
//   SBR_EQ_BAD(uj, j)              the point's own ArgumentError (EconomicParameters, model.jl:71-76)
//   SBR_EQ_OUT(b, j)               the index of its result
// or, in place of the four, SBR_EQ_LANE(j): a statement that solves and stores everything lane j of
// the tile stands for, on the body's locals (sbr_interest_econ.hip: one value function, every κ).
// The β×u sweeps' expansion is the text eq_column had before the body was shared, token for
// token, so their machine code does not depend on the other users.
{
    const int n = L.n_knots[b], ntau = L.n_tau[b], nle = L.n_le[b];
    const uint32_t lst = L.status[b];
    const size_t row = (size_t)b * (size_t)L.cap;
    const double* __restrict__ gT = L.t + row;
    const double* __restrict__ gG = L.G + row;
    const double* __restrict__ gH = L.hr + row;
    // Baseline: t and G staged (HR is read once per point by the blocked crossing scan, from
    // L2, with its block summaries in LDS) so that two workgroups fit a CU's LDS; the
    // interest mode stages HR too (its value functions look it up every RK stage).
    constexpr int NS = INTEREST ? 3 : 2;
    const bool fits = n <= a.lds_cap && (!INTEREST || ntau <= a.lds_cap);
    // MODE 1: the columns whose knots fit the LDS slab, MODE 2: the others, MODE 0: both.  The
    // sweeps launch 1 then 2, so the hot kernel carries no copy of the global-memory path (half
    // the machine code, no VGPR spills); a MODE-2 workgroup of a fitting column exits at once.
    if ((MODE == 1 && !fits) || (MODE == 2 && fits)) return;
    double* sT = smem;
    double* sG = smem + a.lds_cap;
    double* sH = INTEREST ? smem + 2 * a.lds_cap : nullptr;
    const double* __restrict__ cH = INTEREST ? sH : gH;
    // block summaries behind the three knot arrays (lds_cap/64 + 1 entries each)
    const int nsum = (a.lds_cap >> 6) + 1, nsum8 = (a.lds_cap >> 3) + 1;
    double* hmax = smem + NS * a.lds_cap;
    double* hmin = hmax + nsum;
    double* pmc = hmin + nsum;
    double* smc = pmc + nsum8;
    double* hpm = smc + nsum8; // crossing-scan tables (launch_equilibrium sizes the slab for them)
    double* hpn = hpm + nsum;
    double* hsm = hpn + nsum;
    double* hsn = hsm + nsum;
    const int nbh_s = (ntau + 63) >> 6;
    __shared__ int eq_next;
    __shared__ int s_nonmono;
    __shared__ int s_noscan;
    __shared__ int s_near1;                // two consecutive knots within 1e-15·t[n−1]
    __shared__ int s_ndec;                 // decreases of G between consecutive knots
    __shared__ unsigned long long s_maxdec; // largest decrease (bits of a nonnegative double)
    __shared__ double s_thalf;
    __shared__ int s_wb;                   // last knot of the slope-monotone window (Summ::whi)
    __shared__ unsigned long long s_dmax;  // largest |slope| of G (bits of a nonnegative double)
    // every shared flag is initialised before the first barrier: lanes >= nq set
    // s_nonmono right after it, so a later store by thread 0 could clear their flag
    if (threadIdx.x == 0) { eq_next = 0; s_nonmono = 0; s_noscan = 0; s_near1 = 0; s_ndec = 0; s_maxdec = 0; s_thalf = NAN; s_wb = 0x7fffffff; s_dmax = 0; }
    if (fits) {
        for (int i = threadIdx.x; i < n; i += BLOCK) { sT[i] = gT[i]; sG[i] = gG[i]; }
        if (INTEREST)
            for (int i = threadIdx.x; i < ntau; i += BLOCK) sH[i] = gH[i];
    }
    __syncthreads();
    Summ S{nullptr, nullptr, nullptr, nullptr, false, (double)NAN, false, 0.0, false, 2, nullptr, nullptr, nullptr,
           nullptr, 0};
    if (fits && !a.exhaustive) {
        const int nbh = (ntau + 63) >> 6, nbg = (n + 7) >> 3;
        // HR summaries: 8 lanes per 64-entry block, 8 independent loads each (HR is read from
        // L2), combined across the 8 lanes; then one lane per 8-knot G block
        const int nq = nbh << 3;
        for (int bk = threadIdx.x; bk < nq + nbg; bk += BLOCK) {
            if (bk < nq) {
                double mx = -INFINITY, mn = INFINITY;
                const int i0 = bk << 3;
                double h[8];
#pragma unroll
                for (int k = 0; k < 8; k++) h[k] = i0 + k < ntau ? cH[i0 + k] : -INFINITY;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    if (i0 + k >= ntau) continue;
                    if (h[k] > mx) mx = h[k];                                 // NaN never > u: ignore it
                    mn = (h[k] != h[k]) ? -INFINITY : (h[k] < mn ? h[k] : mn); // NaN is "not above"
                }
#pragma unroll
                for (int off = 1; off < 8; off <<= 1) { // the 8 lanes of a block are aligned in one wave
                    const double omx = __shfl_xor(mx, off, 8), omn = __shfl_xor(mn, off, 8);
                    mx = omx > mx ? omx : mx;
                    mn = omn < mn ? omn : mn;
                }
                if ((bk & 7) == 0) {
                    hmax[bk >> 3] = mx;
                    hmin[bk >> 3] = mn;
                }
            } else {
                const int g = bk - nq;
                double mx = -INFINITY, mn = INFINITY;
                const int e = (g << 3) + 8 < n ? (g << 3) + 8 : n;
                double prev = g > 0 ? sG[(g << 3) - 1] : -INFINITY;
                bool mono = true, nan = false;
                int ndec = 0;
                double maxdec = 0.0;
                for (int i = g << 3; i < e; i++) {
                    const double v = sG[i];
                    if (v != v) { mx = NAN; mn = NAN; mono = false; nan = true; break; }
                    if (v > mx) mx = v;
                    if (v < mn) mn = v;
                    const bool dec = v < prev;
                    mono &= !dec;
                    ndec += dec ? 1 : 0;
                    maxdec = dec && prev - v > maxdec ? prev - v : maxdec;
                    prev = v;
                }
                if (!mono) s_nonmono = 1;
                if (nan) s_noscan = 1;
                if (ndec) {
                    atomicAdd(&s_ndec, ndec);
                    atomicMax(&s_maxdec, (unsigned long long)sbr_dbits(maxdec));
                }
                // aw_scan's knot separation (Summ::scan)
                const double sep = 1e-15 * sT[n - 1];
                bool far = true, far1 = true;
                for (int i = g << 3; i < e; i++) {
                    far &= i + 2 >= n || sT[i + 2] - sT[i] > sep;
                    far1 &= i + 1 >= n || sT[i + 1] - sT[i] > sep;
                }
                if (!far) s_noscan = 1;
                if (!far1) s_near1 = 1;
                pmc[g] = mx; // block max for now
                smc[g] = mn; // block min for now
            }
        }
        // aw_scan's slope-monotone window: slopes d_k = (G[k+1] − G[k])/(t[k+1] − t[k]).  With inc(k) ⇔
        // d_k > d_(k−1) and dec(k) ⇔ d_k < d_(k−1), both strict, and kc the first k without inc(k), the slopes
        // rise over [0, kc) and fall from kc up to the first k that has neither inc nor dec or has
        // inc(k) after a k − 1 without it (that k − 1 is >= kc, and the first inc after kc follows a
        // k − 1 without inc): wb is the smallest such k, a local test, so one atomicMin finds it.
        // A computed slope is within 3.01·u of the real one (two differences, a quotient; u = 2^-53), so
        // a computed difference above 2^-50 = 8·u times the larger magnitude implies the same order in
        // real arithmetic; slopes below 2^-900 (where the quotient may round as a subnormal), infinite
        // or NaN end the window.  A wave takes 62 slopes per trip, one division per lane: lanes 0 and 1
        // recompute the two slopes before them, and the neighbours' values come by shuffles.
        {
            auto rises = [](double lo, double hi) { // hi > lo in real arithmetic
                const double m = fabs(lo) > fabs(hi) ? fabs(lo) : fabs(hi);
                return m >= 0x1p-900 && m <= 1e300 && hi - lo > 0x1p-50 * m;
            };
            const int ln = threadIdx.x & 63;
            for (int q = threadIdx.x >> 6; q * 62 < n - 1; q += BLOCK >> 6) {
                const int k = q * 62 + ln - 2;
                const bool valid = k >= 0 && k <= n - 2;
                const double d = valid ? (sG[k + 1] - sG[k]) / (sT[k + 1] - sT[k]) : 0.0;
                const double d1 = __shfl_up(d, 1, 64);
                const bool inc = rises(d1, d), dec = rises(d, d1);
                const bool incp = __shfl_up((int)inc, 1, 64) != 0;
                const bool mine = valid && ln >= 2;
                const bool fail = mine && k >= 1 && ((!inc && !dec) || (k >= 2 && inc && !incp));
                double ad = mine ? fabs(d) : 0.0;
                ad = ad <= 1e300 ? ad : (double)INFINITY; // NaN too
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const double o = __shfl_xor(ad, off, 64);
                    ad = o > ad ? o : ad;
                }
                const unsigned long long fm = __ballot(fail);
                if (ln == 0) {
                    if (fm) atomicMin(&s_wb, q * 62 + (int)__builtin_ctzll(fm) - 2);
                    atomicMax(&s_dmax, (unsigned long long)sbr_dbits(ad));
                }
            }
        }
        __syncthreads();
        // prefix max / suffix min over blocks (NaN-propagating), two waves at once
        if (threadIdx.x == 0) {
            // t_half: first knot interval with G[k] <= 1/2 < G[k+1] (heuristic only)
            int lo = 0, hi = n - 1;
            if (n >= 2 && sG[0] <= 0.5 && sG[n - 1] > 0.5) {
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (sG[mid] <= 0.5) lo = mid;
                    else hi = mid;
                }
                s_thalf = sT[lo] + (0.5 - sG[lo]) * (sT[hi] - sT[lo]) / (sG[hi] - sG[lo]);
            }
            // the tables are read only when G is not monotone (Summ::mono) and aw_scan's
            // preconditions fail (the scan's points never read them): skip the serial scans
            if (s_nonmono && s_noscan)
            for (int g = 1; g < nbg; g++) {
                const double a0 = pmc[g - 1], b0 = pmc[g];
                pmc[g] = (a0 != a0 || b0 != b0) ? NAN : (a0 > b0 ? a0 : b0);
            }
        } else if (threadIdx.x == (BLOCK > 64 ? 64 : 1) && s_nonmono && s_noscan) {
            for (int g = nbg - 2; g >= 0; g--) {
                const double a0 = smc[g + 1], b0 = smc[g];
                smc[g] = (a0 != a0 || b0 != b0) ? NAN : (a0 < b0 ? a0 : b0);
            }
        }
        // the crossing scans' prefix / suffix tables over the HR blocks (hmax has no NaN, hmin has
        // NaN as −∞): a wave each way, 64 blocks per shuffle scan; small blocks: one lane each way
        if (BLOCK >= 256 && (threadIdx.x >> 6) >= 2 && (threadIdx.x >> 6) <= 3) {
            const bool fwd = (threadIdx.x >> 6) == 2;
            const int ln = threadIdx.x & 63;
            double ca = -INFINITY, cb = INFINITY;
            for (int c0 = 0; c0 < nbh; c0 += 64) {
                const int g = fwd ? c0 + ln : nbh - 1 - c0 - ln;
                const bool in = fwd ? g < nbh : g >= 0;
                double a = in ? hmax[g] : -INFINITY, b = in ? hmin[g] : INFINITY;
                for (int off = 1; off < 64; off <<= 1) {
                    const double oa = __shfl_up(a, off, 64), ob = __shfl_up(b, off, 64);
                    if (ln >= off) { a = oa > a ? oa : a; b = ob < b ? ob : b; }
                }
                a = ca > a ? ca : a;
                b = cb < b ? cb : b;
                if (in) {
                    if (fwd) { hpm[g] = a; hpn[g] = b; }
                    else { hsm[g] = a; hsn[g] = b; }
                }
                ca = __shfl(a, 63, 64);
                cb = __shfl(b, 63, 64);
            }
        }
        if (BLOCK < 256 && threadIdx.x == 2) {
            double a0 = -INFINITY, b0 = INFINITY;
            for (int g = 0; g < nbh; g++) {
                a0 = hmax[g] > a0 ? hmax[g] : a0;
                b0 = hmin[g] < b0 ? hmin[g] : b0;
                hpm[g] = a0;
                hpn[g] = b0;
            }
        }
        if (BLOCK < 256 && threadIdx.x == 3) {
            double a0 = -INFINITY, b0 = INFINITY;
            for (int g = nbh - 1; g >= 0; g--) {
                a0 = hmax[g] > a0 ? hmax[g] : a0;
                b0 = hmin[g] < b0 ? hmin[g] : b0;
                hsm[g] = a0;
                hsn[g] = b0;
            }
        }
        __syncthreads();
        // (values every lane reads from LDS are the same in all of them: kept in scalar registers,
        // not in lane registers that stay live across a point's solve)
        auto uni = [](double x) {
            const unsigned long long v = sbr_dbits(x);
            const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
            const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
            return sbr_bitsd(((unsigned long long)hi << 32) | lo);
        };
        const double dd = uni((double)s_ndec * sbr_bitsd(s_maxdec)); // ≥ the largest drawdown
        S = Summ{hmax, hmin, pmc, smc, s_nonmono == 0, uni(s_thalf),
                 n >= 2 && !s_noscan && dd <= 1e-12 && sG[0] >= 0.0 && sG[n - 1] <= 2.0, dd,
                 s_nonmono == 0 || s_noscan != 0, s_near1 == 0 ? 1 : 2,
                 hpm, hpn, hsm, hsn, nbh_s};
        // the window as times, and the scan's extra margin (aw_scan's comment derives both)
        const double dmax = sbr_bitsd(s_dmax);
        if (n >= 2 && dmax <= 1e300 && !(a.diag & 16)) {
            const int wb = s_wb < n - 1 ? s_wb : n - 1;
            const double e0 = fabs(sT[0]), e1 = fabs(sT[n - 1]);
            const double span = (sT[wb] + 2.0 * (e0 > e1 ? e0 : e1)) * (1.0 + 0x1p-40);
            const double du = 0x1p-52 * span;
            const double wm = 0x1p-46 + dmax * (0x1p-50 * span);
            if (wm <= 1e-9) { // a larger margin would rarely let the scan stop: no window
                S.wlo = uni((sT[0] > 0.0 ? sT[0] : 0.0) + du);
                S.whi = uni(sT[wb] - du);
                S.wm = uni(wm);
            }
        }
    }
    // Points are handed out to waves 64 at a time from an LDS counter, so a
    // wave that drew cheap no-run points goes back for more instead of idling
    // at the end of the block while the run points (bisection + AW_max) of its
    // neighbours finish.  Consecutive u in one wave keep its lanes on similar
    // control paths (runs form a prefix in u on the paper's grids).
    const int lane = threadIdx.x & 63;
    const double ETA = eta[b], T1 = t_end[b];
    const uint32_t lbits = lst & (SBR_ODE_MAXITERS | SBR_STIFF_SWITCH | SBR_ODE_FAILED | SBR_KNOT_OVERFLOW);
    const bool bad_col = (lst & (SBR_ARG_INVALID | SBR_OOB)) || n < 2;
    const bool trunc = !a.full_grid && n >= 2 && gT[n - 1] < T1 && !(lst & kLearnCutBits);
    for (;;) {
        int base = 0;
        if (lane == 0) base = atomicAdd(&eq_next, 64);
        base = __builtin_amdgcn_readfirstlane(base);
        if (j0 + base >= j1) break;
        const int j = j0 + base + lane;
        if (j >= j1) continue;
#ifdef SBR_EQ_LANE
        SBR_EQ_LANE(j);
#else
        const double uj = SBR_EQ_U(j);
        PointResult r;
        int64_t vsteps = 0;
        if (bad_col || SBR_EQ_BAD(uj, j)) {
            r.xi = NAN; r.aw = NAN; r.tol = INFINITY; r.iters = 0;
            r.tin = NAN; r.tout = NAN;
            r.status = ((lst & SBR_ARG_INVALID) || SBR_EQ_BAD(uj, j)) ? SBR_ARG_INVALID : (SBR_OOB | lbits);
        } else if (INTEREST && ia.r > 0.0) {
            if (MODE != 2 && fits)
                solve_interest_point(sT, sG, sH, S, n, ntau, nle, ETA, T1, trunc, uj, SBR_EQ_KAPPA(j), a.max_iters, lbits, ia,
                                     r, vsteps, a.aw_path, a.diag);
            else if (MODE != 1)
                solve_interest_point(gT, gG, gH, S, n, ntau, nle, ETA, T1, trunc, uj, SBR_EQ_KAPPA(j), a.max_iters, lbits, ia,
                                     r, vsteps, a.aw_path, a.diag);
        } else if (MODE != 2 && fits) {
            solve_point((const double*)sT, (const double*)sG, cH, S, n, ntau, nle, ETA, T1, trunc, uj, SBR_EQ_KAPPA(j),
                        a.max_iters, lbits, r, a.aw_path, a.diag);
        } else if (MODE != 1) {
            solve_point(gT, gG, gH, S, n, ntau, nle, ETA, T1, trunc, uj, SBR_EQ_KAPPA(j), a.max_iters, lbits, r, a.aw_path, a.diag);
        }
        const size_t o = SBR_EQ_OUT(b, j);
        if (INTEREST && ia.steps) ia.steps[o] = vsteps;
        out.xi[o] = r.xi;
        out.tau_in_unc[o] = r.tin;
        out.tau_out_unc[o] = r.tout;
        out.aw_max[o] = r.aw;
        out.tol[o] = r.tol;
        out.status[o] = r.status;
        if (out.iters) out.iters[o] = r.iters;
#endif
    }
}
