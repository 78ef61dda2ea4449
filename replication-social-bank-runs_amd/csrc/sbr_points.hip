// sbr_points.hip — the gfx950 kernel of sbr_solve_points: a list of models, each with its own
// (β, η, t_end, u, p, κ, λ).
//
// One workgroup per point j of the chunk, row j of the learning buffers its column.  The
// workgroup runs the point's hazard_rate with its own p, λ (hazard_column on a workgroup-local
// copy of the learning arguments, as eq_ready_kernel's tile-0 taker runs a column's hazard
// before its equilibria), stages t, G and HR in LDS when they fit the slab (global memory
// otherwise, as point_coop_kernel), wave 0 solves with point_wave on the point's u, κ, and the
// block runs get_AW over every τ̄ knot.  The same operations as the sweep's hazard and
// equilibrium kernels, so the same bits.
//
// A translation unit of its own: the sweep kernels' machine code (and with it the code hashes
// bench.py keys its PMC counters on) does not depend on this kernel.
#include "sbr_device.h"
#include "sbr_hazard_dev.h"
#include "sbr_kernels.h"
#include "sbr_point_dev.h"
#include "sbr_scan.h"
#include "sbr_solve_dev.h"

namespace sbr {

__global__ __launch_bounds__(CO_BLOCK) void points_kernel(LearnBufs L, LearnArgs la, PointArgs pa, ResultSoA out)
{
    static_assert(CO_BLOCK == HZ_BLOCK, "points_kernel runs hazard_column with the whole workgroup");
    extern __shared__ double smem[];
    __shared__ double s_r[5];
    __shared__ uint32_t s_st;
    __shared__ int s_it;
    __shared__ double s_mx[CO_BLOCK / 64];
    const int jb = blockIdx.x;
    const double BETA = pa.beta[jb], ETA = pa.eta[jb], T1 = pa.t_end[jb], uj = pa.u[jb];
    const double pj = pa.p[jb], kj = pa.kappa[jb], lj = pa.lam[jb];
    // LearningParameters / EconomicParameters checks (model.jl:31-35, 71-76), per point; a NaN
    // fails its rule.  Uniform over the workgroup.
    const bool bad_arg = !(BETA > 0.0) || !(T1 > 0.0) || !(ETA > 0.0) || !(uj >= 0.0) || !(pj >= 0.0 && pj <= 1.0) ||
                         !(kj > 0.0 && kj < 1.0) || !(lj > 0.0);
    if (bad_arg) {
        if (threadIdx.x == 0) {
            out.xi[jb] = NAN;
            out.tau_in_unc[jb] = NAN;
            out.tau_out_unc[jb] = NAN;
            out.aw_max[jb] = NAN;
            out.tol[jb] = INFINITY;
            out.status[jb] = SBR_ARG_INVALID;
            if (out.iters) out.iters[jb] = 0;
        }
        return;
    }
    la.p = pj;
    la.lam = lj;
    // hazard scratch at the head of the slab (launch_points sizes it for both uses)
    hazard_column<CO_BLOCK>(jb, BETA, ETA, la, L, smem, smem + (HZ_LDS + 1), smem + 2 * (HZ_LDS + 1),
                            smem + 3 * HZ_LDS + 2);
    __syncthreads(); // HR, n_tau, n_le and the status of row jb are the workgroup's own writes
    const int n = L.n_knots[jb], ntau = L.n_tau[jb], nle = L.n_le[jb];
    const uint32_t lst = L.status[jb];
    const size_t row = (size_t)jb * (size_t)L.cap;
    const double* gT = L.t + row;
    const double* gG = L.G + row;
    const double* gH = L.hr + row;
    const bool fits = n <= pa.lds_cap && ntau <= pa.lds_cap;
    double* sT = smem;
    double* sG = smem + pa.lds_cap;
    double* sH = smem + 2 * pa.lds_cap;
    if (fits) {
        for (int i = threadIdx.x; i < n; i += CO_BLOCK) { sT[i] = gT[i]; sG[i] = gG[i]; }
        for (int i = threadIdx.x; i < ntau; i += CO_BLOCK) sH[i] = gH[i];
    }
    __syncthreads();
    const double* T = fits ? (const double*)sT : gT;
    const double* G = fits ? (const double*)sG : gG;
    const double* H = fits ? (const double*)sH : gH;
    const uint32_t lbits = lst & (SBR_ODE_MAXITERS | SBR_STIFF_SWITCH | SBR_ODE_FAILED | SBR_KNOT_OVERFLOW);
    const bool bad_col = (lst & (SBR_ARG_INVALID | SBR_OOB)) || n < 2;
    const bool trunc = n >= 2 && gT[n - 1] < T1 && !(lst & kLearnCutBits);
    if (threadIdx.x < 64) {
        PointResult r;
        if (bad_col) {
            r.xi = NAN; r.aw = NAN; r.tol = INFINITY; r.iters = 0; r.tin = NAN; r.tout = NAN;
            r.status = (lst & SBR_ARG_INVALID) ? SBR_ARG_INVALID : (SBR_OOB | lbits);
        } else {
            point_wave(T, G, H, n, ntau, nle, ETA, T1, trunc, uj, kj, pa.max_iters, lbits, r, (double)NAN);
        }
        if (threadIdx.x == 0) {
            s_r[0] = r.xi; s_r[1] = r.tin; s_r[2] = r.tout; s_r[3] = r.aw; s_r[4] = r.tol;
            s_st = r.status;
            s_it = r.iters;
        }
    }
    __syncthreads();
    const uint32_t st = s_st;
    double mx = -INFINITY;
    if (st & SBR_RUN) {
        const double xi = s_r[0], tin = s_r[1], tout = s_r[2];
        const double icc = (tin >= xi) ? xi : tin;
        const double occ = (tout > xi) ? xi : tout;
        const double G0 = lerp_at(T, G, n, ssl_range(T, 0, n - 1, 0.0), 0.0);
        // contiguous τ̄ ranges per thread (the brackets slide), a NaN-latching max per thread
        const int per = (ntau + CO_BLOCK - 1) / CO_BLOCK;
        const int i0 = threadIdx.x * per, i1 = i0 + per < ntau ? i0 + per : ntau;
        co_eval(T, G, n, nle, ETA, xi, icc, occ, G0, i0, i1, mx, nullptr, nullptr, nullptr);
        // block reduction in thread order (NaN latches: any NaN gives NaN, else the max)
        for (int off = 32; off >= 1; off >>= 1) {
            const double o = __shfl_down(mx, off, 64);
            mx = (mx != mx || o != o) ? (double)NAN : (o > mx ? o : mx);
        }
        if ((threadIdx.x & 63) == 0) s_mx[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double aw = s_r[3];
        if (st & SBR_RUN) {
            aw = s_mx[0];
            for (int w = 1; w < CO_BLOCK / 64; w++) aw = (aw != aw || s_mx[w] != s_mx[w]) ? (double)NAN : (s_mx[w] > aw ? s_mx[w] : aw);
        }
        out.xi[jb] = s_r[0];
        out.tau_in_unc[jb] = s_r[1];
        out.tau_out_unc[jb] = s_r[2];
        out.aw_max[jb] = aw;
        out.tol[jb] = s_r[4];
        out.status[jb] = st;
        if (out.iters) out.iters[jb] = s_it;
    }
}

hipError_t launch_points(const LearnBufs& L, const LearnArgs& la, const PointArgs& pa, const ResultSoA& out,
                         int n_points, hipStream_t s)
{
    if (n_points <= 0) return hipSuccess;
    size_t lds = (size_t)3 * pa.lds_cap * sizeof(double);
    const size_t hz = (size_t)(3 * HZ_LDS + 3) * sizeof(double); // hazard scratch shares the slab
    if (lds < hz) lds = hz;
    hipLaunchKernelGGL(points_kernel, dim3(n_points), dim3(CO_BLOCK), lds, s, L, la, pa, out);
    return hipGetLastError();
}

}  // namespace sbr
