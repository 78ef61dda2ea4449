// sbr_econ.hip — the gfx950 kernels of sbr_sweep_econ: β × p × λ × κ × u in one call.
//
// The learning solve depends on (β, t_end, x0) only, the hazard path on (column, η, p, λ), and κ
// and u enter only the per-point solve.  So the learning kernel runs once per column (the single
// sweep's learn_logistic_kernel, launched by the caller), then per chunk of hazard classes
// (p[a], λ[b]):
//   hazard_econ_kernel        one workgroup per (column, class): hazard_column on a
//                             workgroup-local copy of the learning arguments with the class's
//                             p, λ, as points_kernel runs it, into the class's own HR row,
//                             τ̄ counters and status word.
//   equilibrium_econ_kernel   one workgroup per (column, class, tile of the κ × u plane): the
//                             baseline column solve (eq_plane: eq_column's body, sbr_eq_column_body.h
//                             — t and G staged in LDS, the HR and G summaries, solve_point per
//                             lane) on the class's HR row, lane e of the plane solving
//                             (kappa[e / n_u], u[e % n_u]).
// The same operations as the sweep's hazard and equilibrium kernels, so the same bits.
//
// A translation unit of its own: the sweep kernels' machine code (and with it the code hashes
// bench.py keys its PMC counters on) does not depend on these kernels.
#include "sbr_device.h"
#include "sbr_econ_dev.h"
#include "sbr_eq_dev.h"
#include "sbr_hazard_dev.h"
#include "sbr_kernels.h"
#include "sbr_scan.h"
#include "sbr_solve_dev.h"

namespace sbr {

__global__ __launch_bounds__(HZ_BLOCK) void hazard_econ_kernel(const double* __restrict__ beta,
                                                               const double* __restrict__ eta, LearnArgs a,
                                                               LearnBufs L, EconArgs e)
{
    __shared__ double s_eg[HZ_LDS + 1];
    __shared__ double s_t[HZ_LDS + 1];
    __shared__ double s_I[HZ_LDS];
    __shared__ double s_Ieta;
    __builtin_amdgcn_s_setprio(3);
    const int b = blockIdx.x, k = blockIdx.y, g = e.class0 + k;
    const LearnBufs C = econ_class_bufs(L, e, k);
    // hazard_column reads the column's n_le and status and stores its own n_tau, n_le and SBR_OOB:
    // the class's words start as the learning kernel's (n_tau = 0: an invalid column or class has
    // no τ̄ grid), and hazard_column then reads and writes the class's words only
    if (threadIdx.x == 0) {
        C.n_tau[b] = 0;
        C.n_le[b] = L.n_le[b];
        C.status[b] = L.status[b];
    }
    __syncthreads();
    a.p = e.p[g / e.n_lam];
    a.lam = e.lam[g % e.n_lam];
    if (econ_class_bad(a.p, a.lam)) return; // every point of the class is SBR_ARG_INVALID (uniform)
    hazard_column<HZ_BLOCK>(b, beta[b], eta[b], a, C, s_eg, s_t, s_I, &s_Ieta);
}

// point j of a (column, class) plane: κ-major, u-fastest
struct EconPoints {
    const double* __restrict__ kappa;
    int n_u;
    bool bad_class;
    size_t out0; // the plane's first result
};

// eq_column on the plane's points [j0, j1): lane j solves (kappa[j / n_u], u[j % n_u]) on the HR row,
// counters and status of L (econ_class_bufs), κ per lane, tolerance = 10·eps(κ) included
template <int BLOCK, bool INTEREST, int MODE>
__device__ __forceinline__ void eq_plane(const int b, const int j0, const int j1, const LearnBufs& L,
                                         const double* __restrict__ eta, const double* __restrict__ t_end,
                                         const double* __restrict__ u, const EqArgs& a, const InterestArgs& ia,
                                         const ResultSoA& out, double* smem, const EconPoints pt)
#define SBR_EQ_U(j) u[(j) % pt.n_u]
#define SBR_EQ_KAPPA(j) pt.kappa[(j) / pt.n_u]
#define SBR_EQ_BAD(uj, j) (pt.bad_class || !(uj >= 0.0) || !(SBR_EQ_KAPPA(j) > 0.0 && SBR_EQ_KAPPA(j) < 1.0))
#define SBR_EQ_OUT(b, j) pt.out0 + (size_t)(j)
#include "sbr_eq_column_body.h"
#undef SBR_EQ_U
#undef SBR_EQ_KAPPA
#undef SBR_EQ_BAD
#undef SBR_EQ_OUT

template <int BLOCK, int MODE>
__global__ __launch_bounds__(BLOCK, kEqMinW) void equilibrium_econ_kernel(LearnBufs L, const double* __restrict__ eta,
                                                                          const double* __restrict__ t_end,
                                                                          const double* __restrict__ u, EqArgs a,
                                                                          EconArgs e, ResultSoA out)
{
    extern __shared__ double smem[];
    const int plane = e.n_kappa * e.n_u;
    const int tiles = (plane + EQ_TILE - 1) / EQ_TILE;
    const int k = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - k * tiles;
    const int b = (int)blockIdx.y, g = e.class0 + k;
    const int j0 = tile * EQ_TILE;
    const int j1 = j0 + EQ_TILE < plane ? j0 + EQ_TILE : plane;
    const LearnBufs C = econ_class_bufs(L, e, k);
    const InterestArgs none{0.0, 1.0, 0.0, 0.0, 0, nullptr, nullptr, nullptr};
    const EconPoints pt{e.kappa, e.n_u, econ_class_bad(e.p[g / e.n_lam], e.lam[g % e.n_lam]),
                        ((size_t)b * (size_t)(e.n_p * e.n_lam) + (size_t)g) * (size_t)plane};
    eq_plane<BLOCK, false, MODE>(b, j0, j1, C, eta, t_end, u, a, none, out, smem, pt);
}

hipError_t launch_hazard_econ(const double* beta, const double* eta, const LearnArgs& la, const LearnBufs& L,
                              const EconArgs& e, hipStream_t s)
{
    if (e.n_beta <= 0 || e.n_class <= 0 || e.n_class > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hazard_econ_kernel, dim3(e.n_beta, e.n_class), dim3(HZ_BLOCK), 0, s, beta, eta, la, L, e);
    return hipGetLastError();
}

hipError_t launch_equilibrium_econ(const LearnBufs& L, const double* eta, const double* t_end, const double* u,
                                   const EqArgs& a, const EconArgs& e, const ResultSoA& out, hipStream_t s)
{
    // the slab of launch_equilibrium: t, G and the block summaries
    const size_t lds = ((size_t)2 * a.lds_cap + 6 * ((a.lds_cap >> 6) + 1) + 2 * ((a.lds_cap >> 3) + 1)) * sizeof(double);
    const int64_t plane = (int64_t)e.n_kappa * e.n_u;
    const int64_t tiles = (plane + EQ_TILE - 1) / EQ_TILE;
    if (plane <= 0 || plane > (1 << 30) || tiles * e.n_class > 0x7fffffff || e.n_beta > 65535) return hipErrorInvalidValue;
    const int w = plane < EQ_TILE ? (int)plane : EQ_TILE;
    dim3 grid((unsigned)(tiles * e.n_class), e.n_beta);
    // the LDS-resident columns, then the columns beyond the slab on the global-memory path
    auto go = [&](auto k1, auto k2, int bs) {
        hipLaunchKernelGGL(k1, grid, dim3(bs), lds, s, L, eta, t_end, u, a, e, out);
        hipLaunchKernelGGL(k2, grid, dim3(bs), 0, s, L, eta, t_end, u, a, e, out);
    };
    if (w > 256)
        go(equilibrium_econ_kernel<kEqWide, 1>, equilibrium_econ_kernel<kEqWide, 2>, kEqWide);
    else if (w > 64)
        go(equilibrium_econ_kernel<256, 1>, equilibrium_econ_kernel<256, 2>, 256);
    else
        go(equilibrium_econ_kernel<64, 1>, equilibrium_econ_kernel<64, 2>, 64);
    return hipGetLastError();
}

}  // namespace sbr
