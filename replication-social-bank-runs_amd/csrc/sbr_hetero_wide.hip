// sbr_hetero_wide.hip — the heterogeneity equilibrium for any number of groups K (a runtime
// argument, 1 <= K <= SBR_HETERO_MAX_K) on gfx950.
//
//   equilibrium_hetero_wide_kernel  one lane per (column, u): the operations of
//                                   solve_hetero_point<K> (sbr_hetero.hip) in the same order —
//                                   K crossing scans, the dist-weighted ξ bisection, the validity
//                                   check, AW_max with the left fold Σ dist_k·(…) in group order —
//                                   with the group loops as real loops: code size and register
//                                   use do not grow with K.
//   hetero_aw_groups_wide_kernel    get_AW_hetero's per-group curves, one lane per knot.
//
// equilibrium_hetero_kernel<K> keeps every group's buffers, constant-lookup brackets and values
// and search hints unrolled in registers (K = 8: 253 VGPRs).  Here that per-lane per-group state
// lives in lane-strided LDS arrays behind the knot slab (entry k of lane l at [k·BLOCK + l]: a
// wave's accesses to one group are consecutive, no bank conflicts):
//     tin_k, tout_k        the buffers (doubles)
//     gin_k, gout_k        G_k at the constant lookup points tin_k / tout_k (doubles)
//     jin_k, jout_k        their brackets (ints); after the bisection the same slots hold the
//                          walkers of the validity check and of the AW pass
// 40 bytes per group and lane.  AW_max and the validity check evaluate every knot (the
// SBR_FLAG_EXHAUSTIVE path of the specialised kernel: the branch and bound there needs four more
// hint arrays per group); the crossing scans use the per-64 HR block summaries when they fit the
// slab and SBR_FLAG_EXHAUSTIVE is not set.
#include "sbr_device.h"
#include "sbr_hetero_wide_dev.h"
#include "sbr_kernels.h"
#include "sbr_scan.h"

namespace sbr {

// HColW, WideState and solve_hetero_point_wide<BLOCK> (the per-point solve): sbr_hetero_wide_dev.h

// One workgroup per CU: the knot slab (a.lds_cap doubles, MODE 1) and BLOCK·K·40 bytes of group
// state share the CU's 160 KB of LDS.  MODE as in equilibrium_hetero_kernel: 1 = columns whose
// knot times fit the slab, 2 = the others, from global memory (no slab, the state alone).
template <int BLOCK, int MODE>
__global__ __launch_bounds__(BLOCK)
void equilibrium_hetero_wide_kernel(HeteroBufs L, const int K, const double* __restrict__ dist,
                                    const double* __restrict__ eta, const double* __restrict__ t_end,
                                    const double* __restrict__ u, HeteroEqArgs a, ResultSoA out,
                                    double* __restrict__ tin_out, double* __restrict__ tout_out)
{
    extern __shared__ double smem[];
    // XCD-aware tile order (1-D grid), as in equilibrium_hetero_kernel
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
    if ((MODE == 1 && !fits) || (MODE == 2 && fits)) return;
    const int slab = MODE == 1 ? a.lds_cap : 0; // doubles in front of the group state
    if (MODE == 1)
        for (int i = threadIdx.x; i < n; i += BLOCK) smem[i] = gT[i];
    // per-group 64-entry block max / min of HR (sbr_scan.h) at the top of the slab
    const int ntau = L.n_tau[c];
    const int nblk = (ntau + 63) >> 6;
    const bool sums = MODE == 1 && !a.exhaustive && n + 2 * K * nblk <= a.lds_cap;
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
    const int j = tile * BLOCK + threadIdx.x;
    if (j >= a.n_u) return;
    const double uj = u[j];
    const uint32_t lbits = lst & (SBR_ODE_MAXITERS | SBR_STIFF_SWITCH | SBR_ODE_FAILED | SBR_KNOT_OVERFLOW);
    double xi, aw, tol;
    uint32_t st;
    int it;
    const size_t o = (size_t)c * (size_t)a.n_u + j;
    double* const tin_g = tin_out ? tin_out + o * K : nullptr;
    double* const tout_g = tout_out ? tout_out + o * K : nullptr;
    if ((lst & (SBR_ARG_INVALID | SBR_OOB)) || n < 2 || !(uj >= 0.0)) {
        xi = NAN; aw = NAN; tol = INFINITY; it = 0;
        for (int k = 0; k < K; k++) {
            if (tin_g) tin_g[k] = NAN;
            if (tout_g) tout_g[k] = NAN;
        }
        st = ((lst & SBR_ARG_INVALID) || !(uj >= 0.0)) ? SBR_ARG_INVALID : (SBR_OOB | lbits);
    } else {
        double* const sd = smem + slab + threadIdx.x;
        int* const si = (int*)(smem + slab + 4 * K * BLOCK) + threadIdx.x;
        const WideState S{sd, sd + K * BLOCK, sd + 2 * K * BLOCK, sd + 3 * K * BLOCK, si, si + K * BLOCK};
        HColW<const double*> C{MODE == 1 ? (const double*)smem : gT, L.G + (size_t)c * cap * K,
                               L.hr + (size_t)c * K * cap, K, n, ntau, L.n_le[c], cap, eta[c], t_end[c],
                               sums ? hsum : nullptr, nblk};
        solve_hetero_point_wide<BLOCK>(C, dist, uj, a.kappa, a.max_iters, a.tolerance, lbits, xi, aw, tol, st, it, S,
                                       a.diag, a.aw_path, tin_g, tout_g);
    }
    out.xi[o] = xi;
    out.aw_max[o] = aw;
    out.tol[o] = tol;
    out.status[o] = st;
    if (out.iters) out.iters[o] = it;
}

hipError_t launch_hetero_wide(int K, const double* dist, const double* eta, const double* t_end, const double* u,
                              const LearnArgs& la, const HeteroEqArgs& ea_in, const HeteroBufs& L,
                              const ResultSoA& out, double* tin, double* tout, hipStream_t s)
{
    if (K < 1 || K > 16) return hipErrorInvalidValue;
    HeteroEqArgs ea = ea_in;
    ea.n_col = la.n_beta;
    const size_t slab = (size_t)ea.lds_cap * sizeof(double);
    // the widest workgroup (256, 128 or 64 lanes) that the u count fills and whose group state
    // fits behind the slab
    int bs = 256;
    while (bs > 64 && (ea.n_u < bs || slab + (size_t)K * bs * kWideStateBytes > kWideLdsBytes)) bs >>= 1;
    const size_t state = (size_t)K * bs * kWideStateBytes;
    if (slab + state > kWideLdsBytes) return hipErrorInvalidValue;
    const unsigned ncol8 = (unsigned)((la.n_beta + 7) / 8) * 8;
    const dim3 grid(((ea.n_u + bs - 1) / bs) * ncol8);
    // the LDS-resident columns, then (no slab, exiting at once where the knots fit) the others
    auto go = [&](auto k1, auto k2) {
        hipLaunchKernelGGL(k1, grid, dim3(bs), slab + state, s, L, K, dist, eta, t_end, u, ea, out, tin, tout);
        hipLaunchKernelGGL(k2, grid, dim3(bs), state, s, L, K, dist, eta, t_end, u, ea, out, tin, tout);
    };
    if (bs == 256) go(equilibrium_hetero_wide_kernel<256, 1>, equilibrium_hetero_wide_kernel<256, 2>);
    else if (bs == 128) go(equilibrium_hetero_wide_kernel<128, 1>, equilibrium_hetero_wide_kernel<128, 2>);
    else go(equilibrium_hetero_wide_kernel<64, 1>, equilibrium_hetero_wide_kernel<64, 2>);
    return hipGetLastError();
}

// hetero_aw_groups_kernel<K> (sbr_hetero.hip) with K a runtime argument: the same operations per
// group, so the same bits.
__global__ __launch_bounds__(256) void hetero_aw_groups_wide_kernel(const int K, const double* __restrict__ T,
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
    for (int k = 0; k < K; k++) {
        const double av = (ti - xi) + dmin(tin[k], xi);
        const double bv = (ti - xi) + dmin(tout[k], xi);
        const double gi = at(k, av > 0 ? av : 0.0);
        const double go = at(k, bv > 0 ? bv : 0.0);
        out[(size_t)k * ld + i] = bv >= 0 ? go : 0.0;
        out[(size_t)(K + k) * ld + i] = av >= 0 ? gi : 0.0;
    }
}

hipError_t launch_hetero_aw_groups_wide(int K, const double* T, const double* G, const int32_t* n_dev, int n_max,
                                        const double* xi, const double* tin, const double* tout,
                                        const uint32_t* status, double* out, size_t ld, hipStream_t s)
{
    if (n_max < 1) return hipSuccess;
    hipLaunchKernelGGL(hetero_aw_groups_wide_kernel, dim3((unsigned)((n_max + 255) / 256)), dim3(256), 0, s, K, T, G,
                       n_dev, xi, tin, tout, status, out, ld);
    return hipGetLastError();
}

}  // namespace sbr
