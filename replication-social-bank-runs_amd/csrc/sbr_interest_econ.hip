// sbr_interest_econ.hip — the gfx950 kernel of sbr_sweep_interest_econ: β × p × λ × (r, δ) × κ × u
// of the interest-rate extension in one call.
//
// The learning solve depends on (β, t_end, x0), the hazard path on (column, η, p, λ), and the value
// function V with the buffers τ̄_IN, τ̄_OUT taken from h − rV > u on (HR, r, δ, u).  κ enters only
// compute_ξ and the AW pass.  So after sbr_sweep_econ's learning and hazard launches (sbr_econ.hip),
//   interest_econ_kernel      one workgroup per (column, class, tile of the rate × u plane): the
//                             interest column solve (eq_column's body, sbr_eq_column_body.h — t, G
//                             and HR staged in LDS, the summaries behind them) on the class's HR
//                             row.  Lane e of the plane takes ((r, δ)[e / n_u], u[e % n_u]): it
//                             integrates its value function once (≈ 5·10⁴ Tsit5 steps at eps()) and
//                             then runs the baseline's bisection and AW pass on those buffers for
//                             every kappa[c] (≈ 10⁻⁴ of the integration each).
// The same operations per point as equilibrium_kernel<…, true, …>, so the same bits.
//
// A translation unit of its own: the other kernels' machine code does not depend on this one.
#include "sbr_device.h"
#include "sbr_econ_dev.h"
#include "sbr_eq_dev.h"
#include "sbr_hazard_dev.h"
#include "sbr_kernels.h"
#include "sbr_scan.h"
#include "sbr_solve_dev.h"

namespace sbr {

// Lanes of the rate × u plane per workgroup, and the widest block.  launch_interest goes on to
// 1,024-thread blocks over EQ_TILE-point tiles; a 1,024-thread block is held to 128 VGPRs and the value
// function spills there (equilibrium_kernel<1024, true, 1>: 136 bytes of scratch per lane, this kernel
// 140), while at 512 threads it has the 185 registers it wants.  The slab admits one workgroup per
// CU either way, and 512 threads are the two waves per SIMD that 185 registers allow: a plane wider
// than 512 lanes is cut into more workgroups instead, each lane still drawn exactly once.
constexpr int kRateTile = 512;

// what a lane needs beside the column: the axes, and where the (column, class)'s results start
struct InterestEconPoints {
    const double* __restrict__ kappa;
    const double* __restrict__ r;
    const double* __restrict__ delta;
    int n_u, n_kappa;
    bool bad_class;
    size_t out0;   // first result: [n_rate][n_kappa][n_u] from here
    size_t steps0; // first step count: [n_rate][n_u] from here
};

// The value-function stage of solve_interest_point (sbr_eq_dev.h; interest_rate_solver.jl:51-93) for
// one u with r > 0: V on the HR grid, optimal_buffer on h − rV.  Everything in it depends on
// (HR, r, δ, u), never on κ.  Returns false for the BoundsError case (an HR lookup past the grid, a
// 1-knot V interpolant: tin = tout = NaN); bits = the learning bits with the value-function solve's.
// The statements are solve_interest_point's own, in its order, and that function keeps them too: a
// stage shared with it changes equilibrium_kernel<…, true, …>'s machine code.  Edit
// one, edit the other.
template <class P>
__device__ __forceinline__ bool interest_value_stage(P T, P H, const int ntau, const int nle, const double ETA,
                                                     const double T1, const double u, const uint32_t lbits,
                                                     const InterestArgs& ia, uint32_t& bits, int64_t& nsteps,
                                                     double& tin, double& tout)
{
    nsteps = 0;
    const TauView<P> tau{T, nle, ETA};
    ValueRhs<P> f{tau, H, ntau, ia.delta, ia.r, u, ntau > 0 ? tau[0] : 0.0, ntau > 0 ? tau[ntau - 1] : 0.0, 0, false};
    const double V0 = (u + ia.delta) / (ia.r + ia.delta);
    SaveScan<P> sv{tau, H, ntau, ia.r, u, nullptr};
    sv.init(V0);
    // savevalues! with saveat = the HR grid: each pending grid point ≤ the new t is the
    // step's dense output at Θ = (s − tprev)/dt (Tsit5's or Rosenbrock23's), or u itself at t
    struct Saver {
        SaveScan<P>& sv;
        const TauView<P>& tau;
        int ntau;
        __device__ __forceinline__ bool start(double, double) { return true; }
        __device__ __forceinline__ bool step(bool acc, double tprev, double tn, double dt, double y0, double y1,
                                             const StepK& K, bool)
        {
            while (acc && sv.next < ntau && tau[sv.next] <= tn) {
                const double ts = tau[sv.next];
                const double th = (ts - tprev) / dt;
                sv.save(ts != tn ? (K.stiff ? ros23_dense(th, dt, y0, K.k[0], K.k[1])
                                            : tsit5_dense(th, dt, y0, K.k[0], K.k[1], K.k[2], K.k[3], K.k[4],
                                                          K.k[5], K.k[6]))
                                 : y1);
            }
            return true;
        }
    } saver{sv, tau, ntau};
    OdeOut vo;
    ode_scalar(f, saver, ntau > 0 ? tau[ntau - 1] : 0.0, V0, ia.rtol, ia.atol, ia.maxiters, vo);
    uint32_t vbits = vo.status;
    nsteps = vo.naccept + vo.nreject;
    if (f.oob) vbits |= SBR_OOB;
    bits = lbits | (vbits & (SBR_ODE_MAXITERS | SBR_STIFF_SWITCH | SBR_ODE_FAILED));
    if ((vbits & SBR_OOB) || sv.next < 2) {
        tin = NAN; tout = NAN;
        return false;
    }
    sv.finish();
    const int ns = sv.nh;
    if (!sv.any) {
        tin = T1; tout = T1;
    } else if (sv.all) {
        tin = tau[0]; tout = tau[ns - 1];
    } else {
        tin = sv.cin >= 0 ? sv.tin_x : T1;
        tout = sv.cout >= 0 ? sv.tout_x : T1;
        if (tin == T1) tin = tau[sv.fa];
        if (tout == T1) tout = tau[sv.la];
    }
    return true;
}

// Lane j of a (column, class)'s rate × u plane, u-fastest: the value-function stage of
// solve_interest_point once, its tail per κ (r = 0: solve_point per κ, the baseline).  A lane whose own
// u, rate pair or class breaks its rule stores the SBR_ARG_INVALID sentinel for every κ and 0 steps; a
// κ outside (0, 1) is skipped with the sentinel, its neighbours untouched.
template <class P>
__device__ __forceinline__ void interest_econ_lane(const int j, P T, P G, P H, const Summ& S, const int n,
                                                   const int ntau, const int nle, const double ETA,
                                                   const double T1, const bool trunc, const uint32_t lbits,
                                                   const uint32_t lst, const bool bad_col,
                                                   const double* __restrict__ u, const EqArgs& a,
                                                   const InterestEconArgs& ie, const InterestEconPoints& pt,
                                                   const ResultSoA& out)
{
    const int d = j / pt.n_u, ju = j - d * pt.n_u;
    const double uj = u[ju], rr = pt.r[d], dl = pt.delta[d];
    // EconomicParametersInterest (interest_rate_model.jl:40-50); a NaN breaks its rule
    const bool bad = pt.bad_class || !(uj >= 0.0) || !(rr >= 0.0 && dl > 0.0 && rr < dl);
    const bool valued = !bad_col && !bad && rr > 0.0;
    uint32_t bits = lbits;
    int64_t vsteps = 0;
    double tin = NAN, tout = NAN;
    bool ok = false;
    if (valued) {
        const InterestArgs ia{rr, dl, ie.rtol, ie.atol, ie.maxiters, nullptr, nullptr, nullptr};
        ok = interest_value_stage(T, H, ntau, nle, ETA, T1, uj, lbits, ia, bits, vsteps, tin, tout);
    }
    if (ie.steps) ie.steps[pt.steps0 + (size_t)d * (size_t)pt.n_u + (size_t)ju] = vsteps;
    size_t o = pt.out0 + (size_t)d * (size_t)pt.n_kappa * (size_t)pt.n_u + (size_t)ju;
    for (int c = 0; c < pt.n_kappa; c++, o += (size_t)pt.n_u) {
        const double kap = pt.kappa[c];
        const bool bad_k = !(kap > 0.0 && kap < 1.0);
        PointResult r;
        // solve_interest_point's preamble: solve_from_buffers leaves the status as it is where a
        // diagnostic flag stops it after the bisection
        r.xi = NAN; r.aw = NAN; r.tol = INFINITY; r.iters = 0; r.status = 0;
        r.tin = tin; r.tout = tout;
        if (bad_col || bad || bad_k) {
            r.tin = NAN; r.tout = NAN;
            r.status = ((lst & SBR_ARG_INVALID) || bad || bad_k) ? SBR_ARG_INVALID : (SBR_OOB | lbits);
        } else if (!valued) {
            solve_point(T, G, H, S, n, ntau, nle, ETA, T1, trunc, uj, kap, a.max_iters, lbits, r, nullptr, a.diag);
        } else if (!ok) {
            r.status = SBR_OOB | bits;
        } else if (a.diag & 1) {
            r.status = bits;
        } else {
            solve_from_buffers(T, G, H, S, n, ntau, nle, ETA, T1, trunc, uj, kap, a.max_iters, bits, r, nullptr,
                               a.diag, tin, tout);
        }
        out.xi[o] = r.xi;
        out.tau_in_unc[o] = r.tin;
        out.tau_out_unc[o] = r.tout;
        out.aw_max[o] = r.aw;
        out.tol[o] = r.tol;
        out.status[o] = r.status;
        if (out.iters) out.iters[o] = r.iters;
    }
}

// eq_column on the plane's lanes [j0, j1): the interest slab (t, G, HR) and summaries of the class's
// column, then interest_econ_lane per lane — from LDS in the MODE-1 launch, from global memory in MODE 2
template <int BLOCK, bool INTEREST, int MODE>
__device__ __forceinline__ void interest_plane(const int b, const int j0, const int j1, const LearnBufs& L,
                                               const double* __restrict__ eta, const double* __restrict__ t_end,
                                               const double* __restrict__ u, const EqArgs& a,
                                               const InterestEconArgs& ie, const ResultSoA& out, double* smem,
                                               const InterestEconPoints pt)
#define SBR_EQ_LANE(j)                                                                                              \
    if (MODE != 2 && fits)                                                                                          \
        interest_econ_lane((j), (const double*)sT, (const double*)sG, (const double*)sH, S, n, ntau, nle, ETA, T1,  \
                           trunc, lbits, lst, bad_col, u, a, ie, pt, out);                                          \
    else if (MODE != 1)                                                                                             \
        interest_econ_lane((j), gT, gG, gH, S, n, ntau, nle, ETA, T1, trunc, lbits, lst, bad_col, u, a, ie, pt, out)
#include "sbr_eq_column_body.h"
#undef SBR_EQ_LANE

template <int BLOCK, int MODE>
__global__ __launch_bounds__(BLOCK, 1) void interest_econ_kernel(LearnBufs L, const double* __restrict__ eta,
                                                                 const double* __restrict__ t_end,
                                                                 const double* __restrict__ u, EqArgs a, EconArgs e,
                                                                 InterestEconArgs ie, ResultSoA out)
{
    extern __shared__ double smem[];
    const int plane = ie.n_rate * e.n_u;
    const int tiles = (plane + kRateTile - 1) / kRateTile;
    const int k = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - k * tiles;
    const int b = (int)blockIdx.y, g = e.class0 + k;
    const int j0 = tile * kRateTile;
    const int j1 = j0 + kRateTile < plane ? j0 + kRateTile : plane;
    const LearnBufs C = econ_class_bufs(L, e, k);
    const size_t cls = (size_t)b * (size_t)(e.n_p * e.n_lam) + (size_t)g;
    const InterestEconPoints pt{e.kappa, ie.r, ie.delta, e.n_u, e.n_kappa,
                                econ_class_bad(e.p[g / e.n_lam], e.lam[g % e.n_lam]),
                                cls * (size_t)plane * (size_t)e.n_kappa, cls * (size_t)plane};
    interest_plane<BLOCK, true, MODE>(b, j0, j1, C, eta, t_end, u, a, ie, out, smem, pt);
}

hipError_t launch_interest_econ(const LearnBufs& L, const double* eta, const double* t_end, const double* u,
                                const EqArgs& a, const EconArgs& e, const InterestEconArgs& ie,
                                const ResultSoA& out, hipStream_t s)
{
    // the slab of launch_interest: t, G, HR and the block summaries
    const size_t lds = ((size_t)3 * a.lds_cap + 6 * ((a.lds_cap >> 6) + 1) + 2 * ((a.lds_cap >> 3) + 1)) * sizeof(double);
    const int64_t plane = (int64_t)ie.n_rate * e.n_u;
    const int64_t tiles = (plane + kRateTile - 1) / kRateTile;
    if (plane <= 0 || plane > (1 << 30) || e.n_kappa <= 0 || e.n_class <= 0 || tiles * e.n_class > 0x7fffffff ||
        e.n_beta <= 0 || e.n_beta > 65535)
        return hipErrorInvalidValue;
    // every lane integrates its own value function: one wave per 64 lanes of the tile so that all of
    // them run at once
    const int w = plane < kRateTile ? (int)plane : kRateTile;
    dim3 grid((unsigned)(tiles * e.n_class), e.n_beta);
    // the LDS-resident columns, then the columns beyond the slab on the global-memory path
    auto go = [&](auto k1, auto k2, int bs) {
        hipLaunchKernelGGL(k1, grid, dim3(bs), lds, s, L, eta, t_end, u, a, e, ie, out);
        hipLaunchKernelGGL(k2, grid, dim3(bs), 0, s, L, eta, t_end, u, a, e, ie, out);
    };
    if (w > 256)
        go(interest_econ_kernel<kRateTile, 1>, interest_econ_kernel<kRateTile, 2>, kRateTile);
    else if (w > 64)
        go(interest_econ_kernel<256, 1>, interest_econ_kernel<256, 2>, 256);
    else
        go(interest_econ_kernel<64, 1>, interest_econ_kernel<64, 2>, 64);
    return hipGetLastError();
}

}  // namespace sbr
