// sbr_hetero_econ_wide.hip — sbr_sweep_hetero_econ's equilibria for any number of groups K (a
// runtime argument, 1 <= K <= SBR_HETERO_MAX_K) on gfx950: every K without a specialised kernel,
// and any K under SBR_FLAG_HETERO_WIDE.
//
//   equilibrium_hetero_econ_wide_kernel   one workgroup per (column, class, tile of the κ × u
//                                         plane): equilibrium_hetero_wide_kernel's staging on the
//                                         column's knots and the class's hazard rows, lane e
//                                         solving (kappa[e / n_u], u[e % n_u]) with
//                                         solve_hetero_point_wide (sbr_hetero_wide_dev.h) — the
//                                         same operations per point, so the same bits.
#include "sbr_device.h"
#include "sbr_hetero_econ_dev.h"
#include "sbr_hetero_wide_dev.h"
#include "sbr_kernels.h"
#include "sbr_scan.h"

namespace sbr {

// MODE as in equilibrium_hetero_wide_kernel: 1 = columns whose knot times fit the slab (a.lds_cap
// doubles in front of the BLOCK·K·40 bytes of group state), 2 = the others, from global memory.
template <int BLOCK, int MODE>
__global__ __launch_bounds__(BLOCK)
void equilibrium_hetero_econ_wide_kernel(HeteroBufs L, const int K, const double* __restrict__ dist,
                                         const double* __restrict__ eta, const double* __restrict__ t_end,
                                         const double* __restrict__ u, HeteroEqArgs a, HeteroEconArgs e,
                                         ResultSoA out, double* __restrict__ tin_out,
                                         double* __restrict__ tout_out)
{
    extern __shared__ double smem[];
    // XCD-aware tile order (1-D grid), as in equilibrium_hetero_econ_kernel
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
    if ((MODE == 1 && !fits) || (MODE == 2 && fits)) return;
    const int slab = MODE == 1 ? a.lds_cap : 0; // doubles in front of the group state
    if (MODE == 1)
        for (int i = threadIdx.x; i < n; i += BLOCK) smem[i] = gT[i];
    // per-group 64-entry block max / min of HR (sbr_scan.h) at the top of the slab
    const int ntau = e.n_tau[row];
    const int nblk = (ntau + 63) >> 6;
    const bool sums = MODE == 1 && !a.exhaustive && n + 2 * K * nblk <= a.lds_cap;
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
    const int j = tile * BLOCK + threadIdx.x;
    if (j >= plane) return;
    const double uj = u[j % e.n_u];
    const double kap = e.kappa[j / e.n_u];
    // a point whose own u, κ or class (p, λ) breaks its rule: sbr_solve_points' sentinel
    const bool bad = hetero_econ_class_bad(e.p[cls / e.n_lam], e.lam[cls % e.n_lam]) || !(uj >= 0.0) ||
                     !(kap > 0.0 && kap < 1.0);
    const uint32_t lbits = lst & (SBR_ODE_MAXITERS | SBR_STIFF_SWITCH | SBR_ODE_FAILED | SBR_KNOT_OVERFLOW);
    double xi, aw, tol;
    uint32_t st;
    int it;
    const size_t o = ((size_t)c * (size_t)(e.n_p * e.n_lam) + (size_t)cls) * (size_t)plane + (size_t)j;
    double* const tin_g = tin_out ? tin_out + o * K : nullptr;
    double* const tout_g = tout_out ? tout_out + o * K : nullptr;
    if ((lst & (SBR_ARG_INVALID | SBR_OOB)) || n < 2 || bad) {
        xi = NAN; aw = NAN; tol = INFINITY; it = 0;
        for (int k = 0; k < K; k++) {
            if (tin_g) tin_g[k] = NAN;
            if (tout_g) tout_g[k] = NAN;
        }
        st = ((lst & SBR_ARG_INVALID) || bad) ? SBR_ARG_INVALID : (SBR_OOB | lbits);
    } else {
        double* const sd = smem + slab + threadIdx.x;
        int* const si = (int*)(smem + slab + 4 * K * BLOCK) + threadIdx.x;
        const WideState S{sd, sd + K * BLOCK, sd + 2 * K * BLOCK, sd + 3 * K * BLOCK, si, si + K * BLOCK};
        HColW<const double*> C{MODE == 1 ? (const double*)smem : gT, L.G + (size_t)c * cap * K, Hc, K, n, ntau,
                               e.n_le[row], cap, eta[c], t_end[c], sums ? hsum : nullptr, nblk};
        solve_hetero_point_wide<BLOCK>(C, dist, uj, kap, a.max_iters, a.tolerance, lbits, xi, aw, tol, st, it, S,
                                       a.diag, a.aw_path, tin_g, tout_g);
    }
    out.xi[o] = xi;
    out.aw_max[o] = aw;
    out.tol[o] = tol;
    out.status[o] = st;
    if (out.iters) out.iters[o] = it;
}

hipError_t launch_equilibrium_hetero_econ_wide(int K, const double* dist, const double* eta, const double* t_end,
                                               const double* u, const HeteroEqArgs& ea_in, const HeteroBufs& L,
                                               const HeteroEconArgs& e, const ResultSoA& out, double* tin,
                                               double* tout, hipStream_t s)
{
    if (K < 1 || K > 16 || e.n_col <= 0 || e.n_class <= 0 || e.n_kappa <= 0 || e.n_u <= 0) return hipErrorInvalidValue;
    HeteroEqArgs ea = ea_in;
    ea.n_col = e.n_col;
    const size_t slab = (size_t)ea.lds_cap * sizeof(double);
    const int64_t plane = (int64_t)e.n_kappa * e.n_u;
    // the widest workgroup (256, 128 or 64 lanes) that the plane fills and whose group state fits
    // behind the slab
    int bs = 256;
    while (bs > 64 && (plane < bs || slab + (size_t)K * bs * kWideStateBytes > kWideLdsBytes)) bs >>= 1;
    const size_t state = (size_t)K * bs * kWideStateBytes;
    if (slab + state > kWideLdsBytes) return hipErrorInvalidValue;
    const unsigned grid = hetero_econ_grid(e.n_col, e.n_class, plane, bs);
    if (!grid) return hipErrorInvalidValue;
    // the LDS-resident columns, then (no slab, exiting at once where the knots fit) the others
    auto go = [&](auto k1, auto k2) {
        hipLaunchKernelGGL(k1, dim3(grid), dim3(bs), slab + state, s, L, K, dist, eta, t_end, u, ea, e, out, tin, tout);
        hipLaunchKernelGGL(k2, dim3(grid), dim3(bs), state, s, L, K, dist, eta, t_end, u, ea, e, out, tin, tout);
    };
    if (bs == 256) go(equilibrium_hetero_econ_wide_kernel<256, 1>, equilibrium_hetero_econ_wide_kernel<256, 2>);
    else if (bs == 128) go(equilibrium_hetero_econ_wide_kernel<128, 1>, equilibrium_hetero_econ_wide_kernel<128, 2>);
    else go(equilibrium_hetero_econ_wide_kernel<64, 1>, equilibrium_hetero_econ_wide_kernel<64, 2>);
    return hipGetLastError();
}

}  // namespace sbr
