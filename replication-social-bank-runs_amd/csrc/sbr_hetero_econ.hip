// sbr_hetero_econ.hip — the gfx950 kernels of sbr_sweep_hetero_econ: K groups × p × λ × κ × u in
// one call.
//
// solve_SInetwork_hetero depends on (βs, dist, tspan, x0) only, the K hazard paths on (column, η,
// p, λ), the per-group buffers on (hazard paths, u), and κ enters only compute_ξ_hetero, the
// validity check and the AW pass.  So the learning kernel runs once per column (launch_hetero's
// phase 0, launched by the caller; its streamed hazard rows are a by-product nobody reads), then
// per chunk of hazard classes (p[a], λ[b]):
//   hazard_hetero_econ_kernel<K>        one wave per (column, class), lane k = group k:
//                                       hazard_hetero_kernel's loop (sbr_hetero_learn_dev.h),
//                                       operation for operation, with the class's p, λ read from
//                                       the axes, into the class's own HR / running-integral rows,
//                                       τ̄ counters and status word.
//   equilibrium_hetero_econ_kernel<K>   one workgroup per (column, class, tile of the κ × u
//                                       plane): equilibrium_hetero_kernel's staging (knot slab,
//                                       drawdown prologue, knot-separation checks, HR block sums,
//                                       bound cache) on the column's t / G and the class's HR rows,
//                                       lane e solving (kappa[e / n_u], u[e % n_u]) with
//                                       solve_hetero_point<K> (sbr_hetero_point_dev.h).
// The same operations as the sweep's hazard and equilibrium kernels, so the same bits.
// K = 1, 2, 3, 4, 8 here; every other K and SBR_FLAG_HETERO_WIDE: sbr_hetero_econ_wide.hip.
//
// A translation unit of its own: sbr_hetero.hip's compile time and its kernels' machine code do
// not depend on these kernels.
#include "sbr_device.h"
#include "sbr_hetero_econ_dev.h"
#include "sbr_hetero_learn_dev.h"
#include "sbr_hetero_point_dev.h"
#include "sbr_kernels.h"
#include "sbr_scan.h"

namespace sbr {

// The loop of hazard_hetero_kernel<K> (copied: as a shared __device__ function the existing kernel
// compiled to other machine code, sbr_hetero_learn_dev.h) over the knots of column c, writing class
// k's rows.  The class's status starts as the learning kernel's — whose streamed hazard may have set
// SBR_OOB already (η against the knots: the same for every class) — and only the class's words are
// written.
template <int K>
__global__ __launch_bounds__(64) void hazard_hetero_econ_kernel(const double* __restrict__ betas,
                                                               const double* __restrict__ dist,
                                                               const double* __restrict__ eta, HeteroBufs L,
                                                               HeteroEconArgs e)
{
    const int c = blockIdx.x, kc = blockIdx.y, cls = e.class0 + kc;
    const int lane = threadIdx.x;
    const bool act = lane < K;
    const size_t row = (size_t)kc * (size_t)e.n_col + (size_t)c;
    const double p = e.p[cls / e.n_lam], lam = e.lam[cls % e.n_lam];
    uint32_t st = L.status[c];
    if (hetero_econ_class_bad(p, lam)) { // every point of the class is SBR_ARG_INVALID (wave-uniform)
        if (lane == 0) { e.n_tau[row] = 0; e.n_le[row] = 0; e.status[row] = st; }
        return;
    }
    const WaveRow<K> R(lane, betas + (size_t)c * K, dist);
    const double ETA = eta[c];
    const size_t cap = (size_t)L.cap;
    const double* __restrict__ T = L.t + (size_t)c * cap;
    const double* __restrict__ Gv = L.G + (size_t)c * cap * K;
    double* __restrict__ H = e.hr + (row * K + R.kk) * cap;
    double* __restrict__ HI = e.hrI + (row * K + R.kk) * cap;
    const int n = L.n_knots[c];
    int m = 0;
    double tprev = 0.0, Ik = 0.0, eprev = 0.0, gprev = 0.0;
    bool past = false;
    for (int i = 0; i < n && !past; i++) {
        const double t = T[i];
        const double g = R.rhs(Gv[(size_t)i * K + R.kk]);
        if (t <= ETA) {
            const double E = sbr_exp(lam * t);
            const double ev = E * g;
            Ik = (m == 0) ? 0.0 : Ik + (0.5 * (eprev + ev)) * (t - tprev);
            if (act) { H[m] = (p * E) * g; HI[m] = Ik; }
            eprev = ev;
            gprev = g;
            m++;
            tprev = t;
        } else if (m == 0) {
            st |= SBR_OOB; // η before the first knot
            break;
        } else {
            past = true; // pdf(η) on bracket [i-1, i]
            const double d = (ETA - tprev) / (t - tprev);
            const double E = sbr_exp(lam * ETA);
            const double pe = gprev * (1.0 - d) + g * d;
            const double ev = E * pe;
            Ik = Ik + (0.5 * (eprev + ev)) * (ETA - tprev);
            if (act) { H[m] = (p * E) * pe; HI[m] = Ik; }
            m++;
        }
    }
    int n_le = m;
    if (past) {
        n_le = m - 1;
    } else if (!(st & SBR_OOB)) {
        if (n >= 2 && tprev == ETA) { // η is the last knot: pdf(η) = its value
            const double E = sbr_exp(lam * ETA);
            const double pe = 0.0 + gprev * 1.0;
            if (act) { H[m] = (p * E) * pe; HI[m] = Ik; }
            m++;
        } else {
            st |= SBR_OOB;
        }
    }
    if (m > 0 && !(st & SBR_OOB)) {
        __threadfence_block();
        const double omp = 1.0 - p;
        double* __restrict__ Hc = e.hr + row * K * cap;
        const double* __restrict__ HIc = e.hrI + row * K * cap;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const double Ieta = HIc[(size_t)k * cap + m - 1];
            for (int i = lane; i < m; i += 64)
                Hc[(size_t)k * cap + i] = Hc[(size_t)k * cap + i] / ((p * HIc[(size_t)k * cap + i]) + (omp * Ieta));
        }
    }
    if (lane == 0) {
        e.n_tau[row] = (st & SBR_OOB) ? 0 : m;
        e.n_le[row] = (st & SBR_OOB) ? 0 : n_le;
        e.status[row] = st;
    }
}

// equilibrium_hetero_kernel<K, BLOCK, MODE> over (column, class, tile of the κ × u plane): the
// column's knots and group CDFs, the class's hazard rows, counters and status word, κ per lane.
template <int K, int BLOCK, int MODE>
__global__ __launch_bounds__(BLOCK, kHetMinW)
void equilibrium_hetero_econ_kernel(HeteroBufs L, const double* __restrict__ dist, const double* __restrict__ eta,
                                    const double* __restrict__ t_end, const double* __restrict__ u, HeteroEqArgs a,
                                    HeteroEconArgs e, ResultSoA out, double* __restrict__ tin_out,
                                    double* __restrict__ tout_out)
{
    extern __shared__ double smem[];
    __builtin_amdgcn_s_setprio(2);
    // XCD-aware tile order (1-D grid): workgroup w runs on XCD w mod 8, so the tiles of one
    // (column, class) pair are given to consecutive workgroups of the same XCD — they share that
    // XCD's L2 copy of the column's G and the class's HR rows — and consecutive pairs go round the
    // eight XCDs.
    const int plane = e.n_kappa * e.n_u;
    const int ntile = (plane + BLOCK - 1) / BLOCK;
    const int wid = blockIdx.x, xcd = wid & 7, seq = wid >> 3;
    const int pair = (seq / ntile) * 8 + xcd;
    const int tile = seq - (seq / ntile) * ntile;
    if (pair >= a.n_col * e.n_class) return;
    const int c = pair / e.n_class, kc = pair - c * e.n_class, cls = e.class0 + kc;
    const size_t row = (size_t)kc * (size_t)e.n_col + (size_t)c;
    const int n = L.n_knots[c];
    const uint32_t lst = e.status[row];
    const size_t cap = (size_t)L.cap;
    const double* __restrict__ gT = L.t + (size_t)c * cap;
    const double* __restrict__ Hc = e.hr + row * K * cap;
    const bool fits = n <= a.lds_cap;
    // MODE 1: columns whose knot times fit the LDS slab; MODE 2: the others (global-memory path,
    // launched second without a slab)
    if ((MODE == 1 && !fits) || (MODE == 2 && fits)) return;
    __shared__ int s_nonmono;
    __shared__ int s_close; // two knots 2 apart closer than 1e-15·t[n−1] (the AW bounds then search)
    __shared__ int s_close1; // two consecutive knots that close (the AW bounds then use knot + 2)
    if (threadIdx.x == 0) { s_nonmono = a.exhaustive || a.aw_path; s_close = 0; s_close1 = 0; }
    if (fits)
        for (int i = threadIdx.x; i < n; i += BLOCK) smem[i] = gT[i];
    __syncthreads();

    // group CDF drawdown for the AW_max branch and bound, as in equilibrium_hetero_kernel
    __shared__ int s_dcnt[K];
    __shared__ unsigned long long s_dmax[K];
    if (threadIdx.x < K) { s_dcnt[threadIdx.x] = 0; s_dmax[threadIdx.x] = 0ull; }
    __syncthreads();
    {
        const double* __restrict__ Gc = L.G + (size_t)c * cap * K;
        bool nan = false;
        int cnt[K];
        double dm[K];
#pragma unroll
        for (int k = 0; k < K; k++) { cnt[k] = 0; dm[k] = 0.0; }
        for (int i = 1 + threadIdx.x; i < n; i += BLOCK)
#pragma unroll
            for (int k = 0; k < K; k++) {
                const double g1 = Gc[(size_t)i * K + k], g0 = Gc[(size_t)(i - 1) * K + k];
                if (!(fabs(g0) < INFINITY) || !(fabs(g1) < INFINITY)) nan = true; // NaN or ±Inf
                else if (g1 < g0) { cnt[k]++; dm[k] = dmax(dm[k], g0 - g1); }
            }
        if (nan) s_nonmono = 1;
        if (fits) {
            bool close = false, close1 = false;
            const double sepd = n > 0 ? 1e-15 * smem[n - 1] : 0.0; // n == 0: an ARG_INVALID column
            for (int i = threadIdx.x; i + 2 < n; i += BLOCK) close |= !(smem[i + 2] - smem[i] > sepd);
            for (int i = threadIdx.x; i + 1 < n; i += BLOCK) close1 |= !(smem[i + 1] - smem[i] > sepd);
            if (close) s_close = 1;
            if (close1) s_close1 = 1;
        }
#pragma unroll
        for (int k = 0; k < K; k++)
            if (cnt[k]) {
                atomicAdd(&s_dcnt[k], cnt[k]);
                atomicMax(&s_dmax[k], (unsigned long long)__double_as_longlong(dm[k])); // dm > 0: ordered as bits
            }
    }
    // per-group 64-entry block max / min of HR (sbr_scan.h) at the top of the LDS slab
    const int ntau = e.n_tau[row];
    const int nblk = (ntau + 63) >> 6;
    const bool sums = fits && n + 2 * K * nblk <= a.lds_cap;
    double* hsum = smem + (a.lds_cap - 2 * K * nblk);
    if (sums) {
        for (int q = threadIdx.x; q < K * nblk; q += BLOCK) {
            const int k = q / nblk, bk = q - k * nblk;
            const double* __restrict__ Hk = Hc + (size_t)k * cap;
            double mx = -INFINITY, mn = INFINITY;
            const int en = (bk << 6) + 64 < ntau ? (bk << 6) + 64 : ntau;
            for (int i = bk << 6; i < en; i++) {
                const double h = Hk[i];
                if (h > mx) mx = h;                            // NaN never > u: ignore it
                mn = (h != h) ? -INFINITY : (h < mn ? h : mn);  // NaN is "not above"
            }
            hsum[(size_t)k * nblk + bk] = mx;
            hsum[(size_t)(K + k) * nblk + bk] = mn;
        }
    }
    __syncthreads();
    const bool mono = s_nonmono == 0;
    double env = 0.0; // Σ_k dist_k · 2Δ_k, added to every branch-and-bound bound
#pragma unroll
    for (int k = 0; k < K; k++)
        env = env + dist[k] * (2.0 * ((double)s_dcnt[k] * __longlong_as_double((long long)s_dmax[k])));
    const int j = tile * BLOCK + threadIdx.x;
    if (j >= plane) return;
    double dl[K];
#pragma unroll
    for (int k = 0; k < K; k++) dl[k] = dist[k];
    const double uj = u[j % e.n_u];
    const double kap = e.kappa[j / e.n_u];
    // a point whose own u, κ or class (p, λ) breaks its rule: sbr_solve_points' sentinel
    const bool bad = hetero_econ_class_bad(e.p[cls / e.n_lam], e.lam[cls % e.n_lam]) || !(uj >= 0.0) ||
                     !(kap > 0.0 && kap < 1.0);
    const uint32_t lbits = lst & (SBR_ODE_MAXITERS | SBR_STIFF_SWITCH | SBR_ODE_FAILED | SBR_KNOT_OVERFLOW);
    double xi, aw, tol, tin[K], tout[K];
    uint32_t st;
    int it;
    const size_t o = ((size_t)c * (size_t)(e.n_p * e.n_lam) + (size_t)cls) * (size_t)plane + (size_t)j;
    double* const tin_g = tin_out ? tin_out + o * K : nullptr;
    double* const tout_g = tout_out ? tout_out + o * K : nullptr;
    if ((lst & (SBR_ARG_INVALID | SBR_OOB)) || n < 2 || bad) {
        xi = NAN; aw = NAN; tol = INFINITY; it = 0;
#pragma unroll
        for (int k = 0; k < K; k++) {
            if (tin_g) tin_g[k] = NAN;
            if (tout_g) tout_g[k] = NAN;
        }
        st = ((lst & SBR_ARG_INVALID) || bad) ? SBR_ARG_INVALID : (SBR_OOB | lbits);
    } else if constexpr (MODE == 1) {
        HCol<K, const double*> C{smem, L.G + (size_t)c * cap * K, Hc, n, ntau, e.n_le[row], cap, eta[c], t_end[c],
                                 sums && !a.exhaustive ? hsum : nullptr, nblk};
        // AW_max's bound cache: rows of BLOCK codes (one per lane) between the knot times and the
        // HR block sums
        const int ubc_rows = ((sums ? a.lds_cap - 2 * K * nblk : a.lds_cap) - n) * 8 / (BLOCK * (int)sizeof(ubc_t));
        ubc_t* const ubc = (ubc_t*)(smem + n) + threadIdx.x;
        solve_hetero_point<K>(C, dl, uj, kap, a.max_iters, a.tolerance, lbits, xi, aw, tol, st, it, tin, tout, mono,
                              a.diag, a.aw_path, env, fits && s_close == 0, s_close1 == 0 ? 1 : 2, tin_g, tout_g, ubc,
                              BLOCK, ubc_rows);
    } else {
        HCol<K, const double*> C{gT, L.G + (size_t)c * cap * K, Hc, n, ntau, e.n_le[row], cap, eta[c], t_end[c],
                                 nullptr, 0};
        solve_hetero_point<K>(C, dl, uj, kap, a.max_iters, a.tolerance, lbits, xi, aw, tol, st, it, tin, tout, mono,
                              a.diag, a.aw_path, env, fits && s_close == 0, s_close1 == 0 ? 1 : 2, tin_g, tout_g);
    }
    out.xi[o] = xi;
    out.aw_max[o] = aw;
    out.tol[o] = tol;
    out.status[o] = st;
    if (out.iters) out.iters[o] = it;
}

// the 1-D grid of an equilibrium launch: tiles × the (column, class) pairs rounded up to the eight
// XCDs; 0 if it does not fit a launch
unsigned hetero_econ_grid(int64_t n_col, int64_t n_class, int64_t plane, int bs)
{
    const int64_t pairs8 = ((n_col * n_class + 7) / 8) * 8;
    const int64_t g = ((plane + bs - 1) / bs) * pairs8;
    return g > 0 && g <= 0x7fffffff ? (unsigned)g : 0u;
}

template <int K>
static hipError_t launch_eq_hetero_econ_k(const double* dist, const double* eta, const double* t_end, const double* u,
                                          const HeteroEqArgs& ea, const HeteroBufs& L, const HeteroEconArgs& e,
                                          const ResultSoA& out, double* tin, double* tout, hipStream_t s)
{
    const size_t lds = (size_t)ea.lds_cap * sizeof(double);
    const int64_t plane = (int64_t)e.n_kappa * e.n_u;
    const int bs = plane >= kHetBlock ? kHetBlock : 64;
    const unsigned grid = hetero_econ_grid(e.n_col, e.n_class, plane, bs);
    if (!grid) return hipErrorInvalidValue;
    // the LDS-resident columns, then (no slab, exiting at once where the knots fit) the others
    auto go = [&](auto k1, auto k2) {
        hipLaunchKernelGGL(k1, dim3(grid), dim3(bs), lds, s, L, dist, eta, t_end, u, ea, e, out, tin, tout);
        hipLaunchKernelGGL(k2, dim3(grid), dim3(bs), 0, s, L, dist, eta, t_end, u, ea, e, out, tin, tout);
    };
    if (bs == kHetBlock)
        go(equilibrium_hetero_econ_kernel<K, kHetBlock, 1>, equilibrium_hetero_econ_kernel<K, kHetBlock, 2>);
    else
        go(equilibrium_hetero_econ_kernel<K, 64, 1>, equilibrium_hetero_econ_kernel<K, 64, 2>);
    return hipGetLastError();
}

hipError_t launch_equilibrium_hetero_econ(int K, const double* dist, const double* eta, const double* t_end,
                                          const double* u, const HeteroEqArgs& ea_in, const HeteroBufs& L,
                                          const HeteroEconArgs& e, const ResultSoA& out, double* tin, double* tout,
                                          hipStream_t s, bool wide)
{
    if (e.n_col <= 0 || e.n_class <= 0 || e.n_kappa <= 0 || e.n_u <= 0) return hipErrorInvalidValue;
    HeteroEqArgs ea = ea_in;
    ea.n_col = e.n_col;
    const bool spec = K == 1 || K == 2 || K == 3 || K == 4 || K == 8;
    if (wide || !spec) return launch_equilibrium_hetero_econ_wide(K, dist, eta, t_end, u, ea, L, e, out, tin, tout, s);
    switch (K) {
    case 1: return launch_eq_hetero_econ_k<1>(dist, eta, t_end, u, ea, L, e, out, tin, tout, s);
    case 2: return launch_eq_hetero_econ_k<2>(dist, eta, t_end, u, ea, L, e, out, tin, tout, s);
    case 3: return launch_eq_hetero_econ_k<3>(dist, eta, t_end, u, ea, L, e, out, tin, tout, s);
    case 4: return launch_eq_hetero_econ_k<4>(dist, eta, t_end, u, ea, L, e, out, tin, tout, s);
    case 8: return launch_eq_hetero_econ_k<8>(dist, eta, t_end, u, ea, L, e, out, tin, tout, s);
    default: return hipErrorInvalidValue;
    }
}

template <int K>
static void launch_hz(const double* betas, const double* dist, const double* eta, const HeteroBufs& L,
                      const HeteroEconArgs& e, hipStream_t s)
{
    hipLaunchKernelGGL(hazard_hetero_econ_kernel<K>, dim3(e.n_col, e.n_class), dim3(64), 0, s, betas, dist, eta, L, e);
}

hipError_t launch_hazard_hetero_econ(int K, const double* betas, const double* dist, const double* eta,
                                     const HeteroBufs& L, const HeteroEconArgs& e, hipStream_t s)
{
    if (e.n_col <= 0 || e.n_class <= 0 || e.n_class > 65535) return hipErrorInvalidValue;
    switch (K) {
    case 1: launch_hz<1>(betas, dist, eta, L, e, s); break;
    case 2: launch_hz<2>(betas, dist, eta, L, e, s); break;
    case 3: launch_hz<3>(betas, dist, eta, L, e, s); break;
    case 4: launch_hz<4>(betas, dist, eta, L, e, s); break;
    case 5: launch_hz<5>(betas, dist, eta, L, e, s); break;
    case 6: launch_hz<6>(betas, dist, eta, L, e, s); break;
    case 7: launch_hz<7>(betas, dist, eta, L, e, s); break;
    case 8: launch_hz<8>(betas, dist, eta, L, e, s); break;
    case 9: launch_hz<9>(betas, dist, eta, L, e, s); break;
    case 10: launch_hz<10>(betas, dist, eta, L, e, s); break;
    case 11: launch_hz<11>(betas, dist, eta, L, e, s); break;
    case 12: launch_hz<12>(betas, dist, eta, L, e, s); break;
    case 13: launch_hz<13>(betas, dist, eta, L, e, s); break;
    case 14: launch_hz<14>(betas, dist, eta, L, e, s); break;
    case 15: launch_hz<15>(betas, dist, eta, L, e, s); break;
    case 16: launch_hz<16>(betas, dist, eta, L, e, s); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace sbr
