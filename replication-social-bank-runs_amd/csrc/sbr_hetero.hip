// sbr_hetero.hip — gfx950 kernels for the heterogeneity extension (K coupled
// learning groups), src/extensions/heterogeneity/.
//
//   learn_hetero_wave_kernel<K>   one wave per parameter column (lane k = group k):
//                                 FP64 AutoTsit5(Rosenbrock23()) on
//                                 dG_k/dt = (1−G_k) β_k Σ_j dist_j G_j with the
//                                 RMS error norm over K components
//                                 (heterogeneity_learning.jl:49-94), pdfs
//                                 (compute_pdf_hetero :114-134) and the K hazard
//                                 rates on the explicit-grid τ̄ (solver.jl:163-164:
//                                 η always appended) streamed per knot.
//   equilibrium_hetero_kernel<K>  one lane per (column, u): K crossing scans,
//                                 the dist-weighted ξ bisection on [0, 2 max τ̄_OUT]
//                                 (compute_ξ_hetero :48-144), the multimodality
//                                 validity check (:175-210) and AW_max over the
//                                 whole learning grid (get_AW_hetero :316-375).
// Knot times are staged in LDS; G (AoS [knot][K]) and HR ([K][τ̄]) stay in HBM/L2.
// Bit-exact against oracle/sbr_oracle.c (sbro_sweep_hetero).
#include "sbr_device.h"
#include "sbr_hetero_learn_dev.h"
#include "sbr_hetero_point_dev.h"
#include "sbr_kernels.h"
#include "sbr_ode.h"
#include "sbr_scan.h"

namespace sbr {

template <int K>
__device__ __forceinline__ double omega(const double* __restrict__ dist, const double* I)
{
    double w = dist[0] * I[0];
#pragma unroll
    for (int j = 1; j < K; j++) w = w + dist[j] * I[j];
    return w;
}

template <int K>
__device__ __forceinline__ void rhs(const double* __restrict__ dist, const double* b, const double* I, double* du)
{
    const double w = omega<K>(dist, I);
#pragma unroll
    for (int k = 0; k < K; k++) du[k] = ((1.0 - I[k]) * b[k]) * w;
}

template <int K>
__device__ __forceinline__ double rms(const double* v)
{
    if (K == 1) return fabs(v[0]);
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < K; i++) s = s + v[i] * v[i];
    return sqrt(s / (double)K);
}

// ForwardDiff jacobian of rhs (oracle jac_hetero): b_k = (1 − I_k)·β_k,
// J_kj = dist_j·b_k (j ≠ k), J_kk = (−β_k)·ω + dist_k·b_k; autonomous (∂f/∂t = 0)
template <int K>
__device__ __forceinline__ void jac(const double* __restrict__ dist, const double* b, const double* I, double* J)
{
    const double w = omega<K>(dist, I);
#pragma unroll
    for (int k = 0; k < K; k++) {
        const double bk = (1.0 - I[k]) * b[k];
#pragma unroll
        for (int j = 0; j < K; j++) J[k * K + j] = (j == k) ? (-b[k]) * w + dist[k] * bk : dist[j] * bk;
    }
}

// opnorm(J, Inf) (NaN-propagating max of the row sums): Rosenbrock23's eigen_est
template <int K>
__device__ __forceinline__ double opnorm_inf(const double* J)
{
    double nrm = 0.0;
#pragma unroll
    for (int i = 0; i < K; i++) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < K; j++) s = s + fabs(J[i * K + j]);
        nrm = (nrm != nrm || s != s) ? (double)NAN : (s > nrm ? s : nrm);
    }
    return nrm;
}

// learn_hetero_wave_kernel<K> (one wave per column, lane k = group k) and hazard_hetero_kernel<K> (the
// K hazards of a column whose knots are already in L): sbr_hetero_learn_dev.h
// HCol and solve_hetero_point<K> (the per-point solve): sbr_hetero_point_dev.h

template <int K, int BLOCK, int MODE>
__global__ __launch_bounds__(BLOCK, kHetMinW)
void equilibrium_hetero_kernel(HeteroBufs L, const double* __restrict__ dist,
                                                                   const double* __restrict__ eta,
                                                                   const double* __restrict__ t_end,
                                                                   const double* __restrict__ u, HeteroEqArgs a,
                                                                   ResultSoA out, double* __restrict__ tin_out,
                                                                   double* __restrict__ tout_out)
{
    extern __shared__ double smem[];
    __builtin_amdgcn_s_setprio(2); // issue priority over co-resident learning waves (step 49.7 -> 47.9 ms)
    // XCD-aware tile order (1-D grid): workgroup w runs on XCD w mod 8, so the u-tiles of one
    // column are given to consecutive workgroups of the same XCD — they share that XCD's L2
    // copy of the column's G and HR rows instead of fetching four copies into four L2s.
    const int ntile = (a.n_u + BLOCK - 1) / BLOCK;
    const int wid = blockIdx.x, xcd = wid & 7, seq = wid >> 3;
    const int c = (seq / ntile) * 8 + xcd;
    const int tile = seq - (seq / ntile) * ntile;
    if (c >= a.n_col) return;
    const int n = L.n_knots[c];
    const uint32_t lst = L.status[c];
    const size_t cap = (size_t)L.cap;
    const double* __restrict__ gT = L.t + (size_t)c * cap;
    const bool fits = n <= a.lds_cap;
    // MODE 1: columns whose knot times fit the LDS slab; MODE 2: the others (global-memory path,
    // launched second without a slab); the hot launch carries one copy of the point solve
    if ((MODE == 1 && !fits) || (MODE == 2 && fits)) return;
    __shared__ int s_nonmono;
    __shared__ int s_close; // two knots 2 apart closer than 1e-15·t[n−1] (the AW bounds then search)
    __shared__ int s_close1; // two consecutive knots that close (the AW bounds then use knot + 2)
    if (threadIdx.x == 0) { s_nonmono = a.exhaustive || a.aw_path; s_close = 0; s_close1 = 0; } // path mode: every knot
    if (fits)
        for (int i = threadIdx.x; i < n; i += BLOCK) smem[i] = gT[i];
    __syncthreads();

    // Group CDF drawdown for the AW_max branch and bound: Tsit5 at eps() leaves ulp-sized
    // decreases in the saturated tail (G_k = 1 − 2^-53 after 1.0: most config-4 columns), so
    // the bounds take G_k[j] ± Δ_k for the prefix max / suffix min, with
    // Δ_k = (#decreases)·(largest decrease) ≥ the largest drawdown max_{j<j'} G_k[j] − G_k[j'].
    // NaN or ±Inf anywhere -> exhaustive evaluation.
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
    const int ntau = L.n_tau[c];
    const int nblk = (ntau + 63) >> 6;
    const bool sums = fits && n + 2 * K * nblk <= a.lds_cap;
    double* hsum = smem + (a.lds_cap - 2 * K * nblk);
    if (sums) {
        const double* __restrict__ Hc = L.hr + (size_t)c * K * cap;
        for (int q = threadIdx.x; q < K * nblk; q += BLOCK) {
            const int k = q / nblk, bk = q - k * nblk;
            const double* __restrict__ Hk = Hc + (size_t)k * cap;
            double mx = -INFINITY, mn = INFINITY;
            const int e = (bk << 6) + 64 < ntau ? (bk << 6) + 64 : ntau;
            for (int i = bk << 6; i < e; i++) {
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
    if (j >= a.n_u) return;
    double dl[K];
#pragma unroll
    for (int k = 0; k < K; k++) dl[k] = dist[k];
    const double uj = u[j];
    const uint32_t lbits = lst & (SBR_ODE_MAXITERS | SBR_STIFF_SWITCH | SBR_ODE_FAILED | SBR_KNOT_OVERFLOW);
    double xi, aw, tol, tin[K], tout[K];
    uint32_t st;
    int it;
    const size_t o = (size_t)c * (size_t)a.n_u + j;
    double* const tin_g = tin_out ? tin_out + o * K : nullptr;
    double* const tout_g = tout_out ? tout_out + o * K : nullptr;
    if ((lst & (SBR_ARG_INVALID | SBR_OOB)) || n < 2 || !(uj >= 0.0)) {
        xi = NAN; aw = NAN; tol = INFINITY; it = 0;
#pragma unroll
        for (int k = 0; k < K; k++) {
            if (tin_g) tin_g[k] = NAN;
            if (tout_g) tout_g[k] = NAN;
        }
        st = ((lst & SBR_ARG_INVALID) || !(uj >= 0.0)) ? SBR_ARG_INVALID : (SBR_OOB | lbits);
    } else if constexpr (MODE == 1) {
        HCol<K, const double*> C{smem, L.G + (size_t)c * cap * K, L.hr + (size_t)c * K * cap, n, L.n_tau[c],
                                 L.n_le[c], cap, eta[c], t_end[c], sums && !a.exhaustive ? hsum : nullptr, nblk};
        // AW_max's byte bound cache: rows of BLOCK bytes (one per lane) between the knot times
        // and the HR block sums
        const int ubc_rows = ((sums ? a.lds_cap - 2 * K * nblk : a.lds_cap) - n) * 8 / (BLOCK * (int)sizeof(ubc_t));
        ubc_t* const ubc = (ubc_t*)(smem + n) + threadIdx.x;
        solve_hetero_point<K>(C, dl, uj, a.kappa, a.max_iters, a.tolerance, lbits, xi, aw, tol, st, it, tin, tout,
                              mono, a.diag, a.aw_path, env, fits && s_close == 0, s_close1 == 0 ? 1 : 2,
                              tin_g, tout_g, ubc, BLOCK, ubc_rows);
    } else {
        HCol<K, const double*> C{gT, L.G + (size_t)c * cap * K, L.hr + (size_t)c * K * cap, n, L.n_tau[c],
                                 L.n_le[c], cap, eta[c], t_end[c], nullptr, 0};
        solve_hetero_point<K>(C, dl, uj, a.kappa, a.max_iters, a.tolerance, lbits, xi, aw, tol, st, it, tin, tout,
                              mono, a.diag, a.aw_path, env, fits && s_close == 0, s_close1 == 0 ? 1 : 2,
                              tin_g, tout_g);
    }
    out.xi[o] = xi;
    out.aw_max[o] = aw;
    out.tol[o] = tol;
    out.status[o] = st;
    if (out.iters) out.iters[o] = it;
}

template <int K>
static hipError_t launch_hetero_k(const double* betas, const double* dist, const double* eta, const double* t_end,
                                  const double* u, const LearnArgs& la, const HeteroEqArgs& ea_in, const HeteroBufs& L,
                                  const ResultSoA& out, double* tin, double* tout, hipStream_t s, int phase)
{
    if (phase == 2) { // hazards of knots already in L (caller knots)
        hipLaunchKernelGGL(hazard_hetero_kernel<K>, dim3(la.n_beta), dim3(64), 0, s, betas, dist, eta, la, L);
        return hipGetLastError();
    }
    if (phase == 0) {
        hipLaunchKernelGGL(learn_hetero_wave_kernel<K>, dim3((la.n_beta + kHetLearnWG - 1) / kHetLearnWG),
                           dim3(64 * kHetLearnWG), 0, s, betas, dist, eta, t_end, la, L);
        return hipGetLastError();
    }
    const size_t lds = (size_t)ea_in.lds_cap * sizeof(double);
    HeteroEqArgs ea = ea_in;
    ea.n_col = la.n_beta;
    // the LDS-resident columns, then (no slab, exiting at once where the knots fit) the others
    auto go = [&](auto k1, auto k2, dim3 grid, int bs) {
        hipLaunchKernelGGL(k1, grid, dim3(bs), lds, s, L, dist, eta, t_end, u, ea, out, tin, tout);
        hipLaunchKernelGGL(k2, grid, dim3(bs), 0, s, L, dist, eta, t_end, u, ea, out, tin, tout);
    };
    const unsigned ncol8 = (unsigned)((la.n_beta + 7) / 8) * 8;
    if (ea.n_u >= kHetBlock)
        go(equilibrium_hetero_kernel<K, kHetBlock, 1>, equilibrium_hetero_kernel<K, kHetBlock, 2>,
           dim3(((ea.n_u + kHetBlock - 1) / kHetBlock) * ncol8), kHetBlock);
    else
        go(equilibrium_hetero_kernel<K, 64, 1>, equilibrium_hetero_kernel<K, 64, 2>, dim3(((ea.n_u + 63) / 64) * ncol8), 64);
    return hipGetLastError();
}

hipError_t launch_hetero(int K, const double* betas, const double* dist, const double* eta, const double* t_end,
                         const double* u, const LearnArgs& la, const HeteroEqArgs& ea, const HeteroBufs& L,
                         const ResultSoA& out, double* tin, double* tout, hipStream_t s, int phase, bool wide)
{
    // K = 1, 2, 3, 4, 8: the kernels specialised here; every other K up to SBR_HETERO_MAX_K (and the
    // equilibria of any K with `wide`, SBR_FLAG_HETERO_WIDE): the group-looped equilibrium kernel
    // (sbr_hetero_wide.hip) and the learning / hazard instantiations of sbr_hetero_learn_wide.hip
    const bool spec = K == 1 || K == 2 || K == 3 || K == 4 || K == 8;
    if (phase == 1 && (wide || !spec)) return launch_hetero_wide(K, dist, eta, t_end, u, la, ea, L, out, tin, tout, s);
    if (!spec) return launch_hetero_learn_wide(K, betas, dist, eta, t_end, la, L, s, phase);
    switch (K) {
    case 1: return launch_hetero_k<1>(betas, dist, eta, t_end, u, la, ea, L, out, tin, tout, s, phase);
    case 2: return launch_hetero_k<2>(betas, dist, eta, t_end, u, la, ea, L, out, tin, tout, s, phase);
    case 3: return launch_hetero_k<3>(betas, dist, eta, t_end, u, la, ea, L, out, tin, tout, s, phase);
    case 4: return launch_hetero_k<4>(betas, dist, eta, t_end, u, la, ea, L, out, tin, tout, s, phase);
    case 8: return launch_hetero_k<8>(betas, dist, eta, t_end, u, la, ea, L, out, tin, tout, s, phase);
    default: return hipErrorInvalidValue;
    }
}

// ---------------------------------------------------------------------------
// hetero_aw_groups_kernel<K>: get_AW_hetero's per-group curves (heterogeneity_solver.jl:335-362)
// of one solved point on its learning knots, one lane per knot i:
//   AW_OUT_k(t_i) = t_i − ξ + min(τ̄_OUT,k, ξ) >= 0 ? G_k(max(that, 0)) : 0, AW_IN_k alike,
// G_k the gridded-linear interpolant on the knots (bracket = searchsortedlast, clamped to
// [0, n−2]) — the operations of equilibrium_hetero_kernel's AW pass, so the same bits.  Runs
// after the equilibrium on the same stream (ξ, τ̄ and status read on the device); writes nothing
// without a run (the host fills NaN rows).  Rows: AW_OUT_k at out + k·ld, AW_IN_k at out + (K+k)·ld.
// ---------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(256) void hetero_aw_groups_kernel(const double* __restrict__ T,
                                                               const double* __restrict__ G,
                                                               const int32_t* __restrict__ n_p,
                                                               const double* __restrict__ xi_p,
                                                               const double* __restrict__ tin,
                                                               const double* __restrict__ tout,
                                                               const uint32_t* __restrict__ status,
                                                               double* __restrict__ out, size_t ld)
{
    const int n = *n_p;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || n < 2 || !(status[0] & SBR_RUN)) return;
    const double xi = *xi_p, ti = T[i];
    auto at = [&](int k, double x) {
        int q = ssl_range(T, 0, n - 1, x);
        q = q > n - 2 ? n - 2 : (q < 0 ? 0 : q);
        const double d = (x - T[q]) / (T[q + 1] - T[q]);
        return G[(size_t)q * K + k] * (1.0 - d) + G[(size_t)(q + 1) * K + k] * d;
    };
#pragma unroll
    for (int k = 0; k < K; k++) {
        const double av = (ti - xi) + dmin(tin[k], xi);
        const double bv = (ti - xi) + dmin(tout[k], xi);
        const double gi = at(k, av > 0 ? av : 0.0);
        const double go = at(k, bv > 0 ? bv : 0.0);
        out[(size_t)k * ld + i] = bv >= 0 ? go : 0.0;
        out[(size_t)(K + k) * ld + i] = av >= 0 ? gi : 0.0;
    }
}

hipError_t launch_hetero_aw_groups(int K, const double* T, const double* G, const int32_t* n_dev, int n_max,
                                   const double* xi, const double* tin, const double* tout, const uint32_t* status,
                                   double* out, size_t ld, hipStream_t s)
{
    if (n_max < 1) return hipSuccess;
    const dim3 grid((unsigned)((n_max + 255) / 256)), block(256);
    switch (K) {
    case 1: hipLaunchKernelGGL(hetero_aw_groups_kernel<1>, grid, block, 0, s, T, G, n_dev, xi, tin, tout, status, out, ld); break;
    case 2: hipLaunchKernelGGL(hetero_aw_groups_kernel<2>, grid, block, 0, s, T, G, n_dev, xi, tin, tout, status, out, ld); break;
    case 3: hipLaunchKernelGGL(hetero_aw_groups_kernel<3>, grid, block, 0, s, T, G, n_dev, xi, tin, tout, status, out, ld); break;
    case 4: hipLaunchKernelGGL(hetero_aw_groups_kernel<4>, grid, block, 0, s, T, G, n_dev, xi, tin, tout, status, out, ld); break;
    case 8: hipLaunchKernelGGL(hetero_aw_groups_kernel<8>, grid, block, 0, s, T, G, n_dev, xi, tin, tout, status, out, ld); break;
    default: return launch_hetero_aw_groups_wide(K, T, G, n_dev, n_max, xi, tin, tout, status, out, ld, s);
    }
    return hipGetLastError();
}

}  // namespace sbr
