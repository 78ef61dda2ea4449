// sbr_baseline.hip — gfx950 kernels for the baseline β×u sweep.
//
//   learn_logistic_kernel   one lane per β column: FP64 Tsit5 with
//                           OrdinaryDiffEq's PI step control on
//                           dx/dt = βx(1−x) (learning.jl:41-54), every
//                           accepted step a knot (save_everystep), hazard
//                           numerator / cumulative trapezoid streamed as the
//                           knots are produced (solver.jl:153-185), HR
//                           finalised in a second pass.
//   equilibrium_kernel      one workgroup per (β, u-tile), one lane per grid
//                           point: knot grid + HR staged once per workgroup
//                           in LDS, then per lane the crossing scan
//                           (solver.jl:211-264), the ξ bisection with the
//                           slope check (solver.jl:308-376) and the AW path
//                           maximum (solver.jl:495-532, 565).  Results are
//                           written as coalesced SoA rows.
//
// Bit-exact against oracle/sbr_oracle.c (see sbr_device.h).
#include "sbr_device.h"
#include "sbr_eq_dev.h"
#include "sbr_hazard_dev.h"
#include "sbr_kernels.h"
#include "sbr_ode.h"
#include "sbr_point_dev.h"
#include "sbr_scan.h"
#include "sbr_solve_dev.h"

namespace sbr {

// ============================================================================
// Learning kernel
// ============================================================================
// lanes per learning workgroup of the pipelined batch's streamed-hazard launches (learning that
// runs beside the equilibrium kernel): two waves per workgroup.  Same-call A/Bs (r05_oo, r05_pp):
// the co-running equilibrium kernel 1.39 -> 1.36 ms, config-3 step 1.487-1.507 -> 1.455 ms at 50
// steps; 256 lanes slower (1.524 ms).  Latency-critical launches (single sweeps, the batch's
// first group, config 1) keep one wave per workgroup: with two, config 1 took 2.24 instead of
// 2.15 ms and a single sweep 4.20 instead of 4.01 ms (r05_qq)
constexpr int kLearnBlock = 128;
constexpr int kLearnBlockLat = 64;

// readiness sweeps: column b is complete (knots, counters, status written by this lane) —
// release it to the equilibrium workgroups (agent scope: they run on other CUs / XCDs)
__device__ __forceinline__ void publish_column(const LearnArgs& a, int b)
{
    const int k = atomicAdd(a.ready_tail, 1);
    __hip_atomic_store(a.ready_q + k, b + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
// one lane's knot-row store of the learning kernel (the nontemporal hint was neutral, r05_ee)
#define st_knot(p, v) (*(p) = (v))
// STAGE (a batch's wide learning launch, the chip otherwise idle; fused hazard): the knot rows
// (t, G) and the hazard rows (numerator, running integral) go through a per-lane ring of
// kStageSlots slots in LDS, [array][slot][lane], and leave as whole 128-B lines — eight 16-B
// stores per array — on every 8th attempted step (the same step for every live lane), the rest
// when the lane's solve ends.  With hundreds of learning waves the direct 8-B knot stores (one
// line per lane per store instruction) made the launch twice the chain alone
// (tools/ubench_wide.hip: 640 waves 3.74 ms without stores, 6.48 direct, 4.43 staged).  Between
// two flushes a lane accepts at most 8 knots and holds fewer than 16 unflushed after one, so 24
// slots never overwrite an unflushed entry; 48 KiB per wave lets three waves share a CU.
constexpr int kStageSlots = 24;
constexpr size_t kStageLdsPerWave = (size_t)4 * kStageSlots * 64 * sizeof(double); // 48 KiB
template <int LB, bool STAGE = false>
__global__ __launch_bounds__(LB) void learn_logistic_kernel(const double* __restrict__ beta,
                                                            const double* __restrict__ eta,
                                                            const double* __restrict__ t_end, LearnArgs a,
                                                            LearnBufs L)
{
    extern __shared__ double stage_lds[];
    // latency-bound (one serial ODE per lane): take issue priority over co-resident
    // equilibrium waves of a previous batch
    __builtin_amdgcn_s_setprio(3);
    // one column per lane (a knot store or load of the wave touches one row per active lane).
    // Heads first (a.wpg, one-wave blocks): the workgroup dispatcher deals consecutive blocks
    // round-robin over the XCDs and their CUs, so every grid's first wave — block g·32 of a
    // 2048-column grid — landed on one of only 8 CUs, three heads per CU, and those waves hold
    // the longest columns of a β-descending grid (config 3: column 22, 4.45k steps against a
    // 2.9k median).  Dealt first, each head has a CU to itself: a 20-grid launch 4.2-4.7 →
    // 3.0-3.2 ms (tools/ubench_fill.hip).
    int blk = blockIdx.x;
    if (LB == 64 && a.wpg) {
        const int nh = (a.n_beta / (64 * a.wpg)) * a.head, per = a.wpg - a.head;
        blk = blk < nh ? (blk / a.head) * a.wpg + blk % a.head
                       : ((blk - nh) / per) * a.wpg + a.head + (blk - nh) % per;
    }
    const int b = blk * LB + threadIdx.x;
    const bool live = b < a.n_beta;
    const double BETA = live ? beta[b] : 1.0, ETA = live ? eta[b] : 1.0, T1 = live ? t_end[b] : 1.0, T0 = 0.0;
    const size_t row = (size_t)(live ? b : 0) * (size_t)L.cap;
    double* __restrict__ T = L.t + row;
    double* __restrict__ Gv = L.G + row;
    uint32_t st = 0;
    const bool fuse = a.fuse_hazard != 0; // wave-uniform

    if (live && (!(BETA > 0.0) || !(T1 > T0) || !(ETA > 0.0))) { // LearningParameters / EconomicParameters checks
        L.status[b] = SBR_ARG_INVALID;
        L.n_knots[b] = 0; L.n_tau[b] = 0; L.n_le[b] = 0; L.n_accept[b] = 0; L.n_reject[b] = 0;
        if (a.ready_q) publish_column(a, b);
    } else if (live) {
    // ---- knot sink: store (t, G).  Branch-free: every attempted step writes its candidate
    // knot at the fill index n (a rejected one is overwritten by the next accepted step) and the
    // counters advance by select.  Fused hazard (a.fuse_hazard, the pipelined batch): each
    // accepted knot ≤ η is also a τ̄ entry of hazard_rate (solver.jl:153-185) — its numerator
    // (p·e^{λτ̄})·g and the running trapezoid integral I are formed as the knot is accepted
    // (g = βG(1−G), the sequential sum in the reference's order), the η entry at the first
    // knot past η; the normalisation by p·I + (1−p)·I_η is hazard_norm_kernel's.  The same
    // operations as hazard_kernel, so the same bits. ----
    struct Sink {
        double* __restrict__ T;
        double* __restrict__ Gv;
        double* __restrict__ H;
        double* __restrict__ HI;
        double* SL;       // STAGE: this lane's ring, slot k of array a at SL[(a·kStageSlots + k)·64]
        int fl, tick;     // STAGE: entries flushed (a multiple of 16), attempted steps
        int ws, fs;       // STAGE: the ring slots of entry n and of entry fl
        int n, cap, m; // m: knots ≤ η (the hazard stage's τ̄ prefix), set at the first knot past η
        double tlast, bound, eta;
        int past, done, stop_after_eta; // 0 / 1 (ints: loop-carried bools cost mask conversions)
        uint32_t& st;
        int fuse, hm;            // hm: τ̄ entries written
        double beta, lam, p;
        double hI, he, ht, hg;   // I, e and τ̄ of the last τ̄ entry, pdf of the last knot ≤ η
        __device__ __forceinline__ bool push(bool acc, double t, double x)
        {
            const bool room = n < cap;
            const int w = room ? n : cap - 1;
            if (STAGE) {
                if (room) { SL[ws * 64] = t; SL[(kStageSlots + ws) * 64] = x; }
            } else if (room) {
                st_knot(T + w, t); st_knot(Gv + w, x); // a rejected candidate is overwritten later
            }
            // bitwise (not short-circuit) logic: selects, no branches
            const bool pushed = acc & room;
            const bool over = acc & !room;
            st |= over ? SBR_KNOT_OVERFLOW : 0u;
            // furthest point any lookup of the equilibrium stage can reach (DESIGN.md
            // §Truncation): max of t_j + (t_j − t_{j−1}) over the knots j ≥ 1 up to and
            // including the first knot past η
            const bool upd = pushed & (n >= 1) & (past == 0);
            const double reach = dmax(bound, t + (t - tlast));
            bound = upd ? reach : bound;
            const bool cross = pushed & (past == 0) & (t > eta);
            if (fuse) {
                const double g = (beta * x) * (1.0 - x);
                const bool le = pushed & (past == 0) & (t <= eta);
                const double E = sbr_exp(lam * t);
                const double e = E * g;
                const double In = hm == 0 ? 0.0 : hI + (0.5 * (he + e)) * (t - ht);
                if (STAGE) {
                    if (le) { SL[(2 * kStageSlots + ws) * 64] = (p * E) * g; SL[(3 * kStageSlots + ws) * 64] = In; }
                } else if (le) {
                    st_knot(H + n, (p * E) * g); st_knot(HI + n, In);
                }
                hI = le ? In : hI;
                he = le ? e : he;
                ht = le ? t : ht;
                hg = le ? g : hg;
                hm += le ? 1 : 0;
                if (cross && ht != eta) {
                    // τ̄ = η on bracket [m-1, m]: pdf interpolated, pushed unless η is a knot
                    const double d = (eta - ht) / (t - ht);
                    const double pe = hg * (1.0 - d) + g * d;
                    const double E2 = sbr_exp(lam * eta);
                    const double e2 = E2 * pe;
                    hI = hI + (0.5 * (he + e2)) * (eta - ht);
                    if (STAGE) { // hm == n here: every earlier knot is ≤ η
                        SL[(2 * kStageSlots + ws) * 64] = (p * E2) * pe;
                        SL[(3 * kStageSlots + ws) * 64] = hI;
                    } else {
                        H[hm] = (p * E2) * pe;
                        HI[hm] = hI;
                    }
                    hm++;
                }
            }
            m = cross ? n : m;
            past |= cross ? 1 : 0;
            tlast = pushed ? t : tlast;
            n += pushed ? 1 : 0;
            if (STAGE) {
                ws = pushed ? (ws == kStageSlots - 1 ? 0 : ws + 1) : ws;
                if ((++tick & 7) == 0 && n - fl >= 16) flush_line();
            }
            done |= (over | (pushed & (stop_after_eta != 0) & (past != 0) & (t >= bound))) ? 1 : 0;
            return done == 0;
        }
        // STAGE: entries [fl, fl + 16) from the ring to the rows, as 16-B pairs (hazard entries
        // past the τ̄ grid carry stale slots: never read)
        __device__ __forceinline__ void flush_line()
        {
            typedef double d2 __attribute__((ext_vector_type(2)));
            double* const R[4] = {T, Gv, H, HI};
#pragma unroll
            for (int k = 0; k < 16; k += 2) {
                const int s0 = fs + k < kStageSlots ? fs + k : fs + k - kStageSlots; // pairs never straddle the wrap
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    d2 v;
                    v.x = SL[(q * kStageSlots + s0) * 64];
                    v.y = SL[(q * kStageSlots + s0 + 1) * 64];
                    *(d2*)(R[q] + fl + k) = v;
                }
            }
            fl += 16;
            fs = fs + 16 < kStageSlots ? fs + 16 : fs + 16 - kStageSlots;
        }
        __device__ __forceinline__ bool start(double t, double x) { return push(true, t, x); }
        __device__ __forceinline__ bool step(bool acc, double, double tn, double, double, double y1, const StepK&, bool)
        {
            return push(acc, tn, y1);
        }
        // the column is learned: counters and status, then (readiness sweeps) its
        // publication — called by ode_scalar the moment this lane's solve ends, while the
        // other columns of the wave may still be integrating
        const LearnBufs* Lp;
        const LearnArgs* ap;
        int b;
        int ntau_out; // the τ̄ entries of the column, set by finish
        __device__ __forceinline__ void finish(const OdeOut& o)
        {
            if (STAGE) // the entries not flushed yet: knots [fl, n), τ̄ entries [fl, hm)
                for (int i = fl, sl = fs; i < n; i++, sl = sl == kStageSlots - 1 ? 0 : sl + 1) {
                    T[i] = SL[sl * 64];
                    Gv[i] = SL[(kStageSlots + sl) * 64];
                    if (i < hm) {
                        H[i] = SL[(2 * kStageSlots + sl) * 64];
                        HI[i] = SL[(3 * kStageSlots + sl) * 64];
                    }
                }
            st |= o.status;
            int n_le = m < 0 ? n : m; // every knot ≤ η when none passed it
            int n_tau = 0;
            if (fuse) {
                // hazard_kernel's η rule: with no knot past η, pdf(η) exists only if η is the last knot
                if (m < 0 && ht != eta) {
                    st |= SBR_OOB;
                    n_le = 0;
                } else {
                    n_tau = hm;
                }
            }
            Lp->n_knots[b] = n;
            Lp->n_le[b] = n_le;
            if (fuse) Lp->n_tau[b] = n_tau;
            ntau_out = n_tau;
            Lp->status[b] = st;
            Lp->n_accept[b] = (int)o.naccept;
            Lp->n_reject[b] = (int)o.nreject;
            if (ap->ready_q) publish_column(*ap, b);
        }
    } sink{T, Gv, fuse ? L.hr + row : nullptr, fuse ? L.hrI + row : nullptr,
           stage_lds + (size_t)(threadIdx.x >> 6) * (4 * kStageSlots * 64) + (threadIdx.x & 63), 0, 0, 0, 0,
           0, L.lim, -1, 0.0, -INFINITY, ETA,
           0, 0, a.stop_after_eta != 0 ? 1 : 0, st, fuse ? 1 : 0, 0, BETA, a.lam, a.p, 0.0, 0.0, 0.0, 0.0,
           &L, &a, b, 0};
    LogisticSys f{BETA};
    OdeOut o;
    ode_scalar(f, sink, T1, a.x0, a.rtol, a.atol, a.maxiters, o);
    if (STAGE && a.fuse_hazard == 2 && a.wpg && (blk % a.wpg) >= a.head && sink.ntau_out > 0) {
        // A tail wave (not a grid's head wave) normalises its columns' hazard rows itself once
        // every lane has solved — hazard_norm_kernel's operation, the same bits.  The tail waves
        // end long before the head waves that set the launch's length, so the pass (≈1 ms of
        // latency-bound loads per lane) is hidden; the head waves' columns are left to a small
        // hazard_norm_kernel launch after the learning (LearnArgs::part 1).  Eight entries per
        // round keep eight loads of each row in flight.
        double* __restrict__ H = L.hr + row;
        const double* __restrict__ HI = L.hrI + row;
        const int nt = sink.ntau_out;
        const double p = a.p, omp = 1.0 - p, ie = HI[nt - 1];
        for (int i0 = 0; i0 < nt; i0 += 8) {
            double h[8], q[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                h[k] = i0 + k < nt ? H[i0 + k] : 0.0;
                q[k] = i0 + k < nt ? HI[i0 + k] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (i0 + k < nt) H[i0 + k] = h[k] / ((p * q[k]) + (omp * ie));
        }
    }
    }
}

// Fused hazard, second half: HR_i = num_i / (p·I_i + (1 − p)·I_η) over every τ̄ entry the
// learning kernel streamed (num_i in the HR row, I_i in the hrI row; I_η = the last I).  Fully
// parallel and HBM-streaming (≈20 µs per 2048-column grid) — unlike hazard_kernel, whose
// workgroups hold CU slots for the length of a serial scan while equilibria are running.
constexpr int HN_BLOCK = 256, HN_UNROLL = 4;
__global__ __launch_bounds__(HN_BLOCK) void hazard_norm_kernel(LearnArgs a, LearnBufs L)
{
    // a.part == 1: only the columns of each grid's head waves (the rest normalised by their
    // learning waves, learn_logistic_kernel with fuse_hazard 2): block → grid's head column
    const int hc = 64 * a.head;
    const int b = a.part == 1 ? (int)(blockIdx.x / hc) * 64 * a.wpg + (int)(blockIdx.x % hc) : (int)blockIdx.x;
    const int nt = L.n_tau[b];
    if (nt <= 0) return;
    const size_t row = (size_t)b * (size_t)L.cap;
    double* __restrict__ H = L.hr + row;
    const double* __restrict__ HI = L.hrI + row;
    const double p = a.p, omp = 1.0 - p, ie = HI[nt - 1];
    for (int i0 = threadIdx.x; i0 < nt; i0 += HN_BLOCK * HN_UNROLL) {
        double h[HN_UNROLL], q[HN_UNROLL];
#pragma unroll
        for (int k = 0; k < HN_UNROLL; k++) {
            const int i = i0 + k * HN_BLOCK;
            h[k] = i < nt ? H[i] : 0.0;
            q[k] = i < nt ? HI[i] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < HN_UNROLL; k++) {
            const int i = i0 + k * HN_BLOCK;
            if (i < nt) H[i] = h[k] / ((p * q[k]) + (omp * ie));
        }
    }
}

// ============================================================================
// Hazard kernel — hazard_rate (solver.jl:153-185) for one β column per
// workgroup: τ̄ = knots ≤ η (+ η), pdf g = βG(1−G) (learning.jl:170), then
// e = exp(λτ̄)·g, the cumulative trapezoid (sequential, in the reference's
// order) and HR = (p·exp(λτ̄))·g / (p·I + (1−p)·I_η).
// ============================================================================
__global__ __launch_bounds__(HZ_BLOCK) void hazard_kernel(const double* __restrict__ beta,
                                                          const double* __restrict__ eta, LearnArgs a, LearnBufs L)
{
    // 24 KiB of LDS per block, so hazard blocks of the next batch still fit beside two
    // equilibrium blocks on a CU
    __shared__ double s_eg[HZ_LDS + 1]; // s_eg[k + 1] = e·g of knot c0 + k; s_eg[0] that of knot c0 − 1
    __shared__ double s_t[HZ_LDS + 1];  // τ̄ likewise
    __shared__ double s_I[HZ_LDS];
    __shared__ double s_Ieta;
    __builtin_amdgcn_s_setprio(3);
    const int b = blockIdx.x;
    hazard_column<HZ_BLOCK>(b, beta[b], eta[b], a, L, s_eg, s_t, s_I, &s_Ieta);
}

// ============================================================================
// Equilibrium kernel
// ============================================================================
#ifdef SBR_EQ_WGTIME
// diagnostic build only (tools/wgtime.py): per-workgroup start / end (100 MHz realtime clock)
// and hardware ids of the last equilibrium_kernel launch
constexpr size_t kWgTimeMax = 65536;
__device__ unsigned long long g_wgtime[2 * kWgTimeMax];
__device__ unsigned int g_wghw[2 * kWgTimeMax];
#endif

template <int BLOCK, bool INTEREST, int MODE>
__global__ __launch_bounds__(BLOCK, INTEREST ? 1 : kEqMinW) void equilibrium_kernel(LearnBufs L, const double* __restrict__ eta,
                                                            const double* __restrict__ t_end,
                                                            const double* __restrict__ u, EqArgs a, InterestArgs ia,
                                                            ResultSoA out)
{
    extern __shared__ double smem[];
    int b = (int)blockIdx.y;
    if (a.group > 1) { // grouped launch: the copies of a column back to back
        const int per = (int)gridDim.y / a.group;
        b = (b % a.group) * per + b / a.group;
    }
    const int j0 = blockIdx.x * EQ_TILE;
    const int j1 = j0 + EQ_TILE < a.n_u ? j0 + EQ_TILE : a.n_u;
#ifdef SBR_EQ_WGTIME
    const unsigned long long wt0 = __builtin_amdgcn_s_memrealtime();
#endif
    eq_column<BLOCK, INTEREST, MODE>(b, j0, j1, L, eta, t_end, u, a, ia, out, smem);
#ifdef SBR_EQ_WGTIME
    __syncthreads();
    const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (threadIdx.x == 0 && wg < kWgTimeMax) {
        g_wgtime[2 * wg] = wt0;
        g_wgtime[2 * wg + 1] = __builtin_amdgcn_s_memrealtime();
        // HW_ID (SE / CU / SIMD of wave 0) and XCC_ID: where the workgroup ran
        g_wghw[2 * wg] = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));
        g_wghw[2 * wg + 1] = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11));
    }
#endif
}

// ============================================================================
// Readiness sweep, equilibrium side: workgroups take (column, u-tile) items in the order the
// learning kernel publishes the columns (ReadyArgs), so that a column's equilibria start as
// soon as its own ODE is solved instead of after the slowest column of the grid.  The
// tile-0 taker runs the column's hazard_rate first.
// ============================================================================
// poll *p (acquire) until it is set; 0 after `limit` polls or once another workgroup has
// given up (*err set): a stuck schedule drains in one timeout, not one per workgroup
__device__ __forceinline__ int ready_wait(const int32_t* p, const int32_t* err, int limit)
{
    int v = 0;
    for (int k = 0; k < limit; k++) {
        v = __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if (v) break;
        if ((k & 63) == 63 && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        __builtin_amdgcn_s_sleep(8);
    }
    return v;
}

// One workgroup per item, n_items in the grid: a workgroup draws its item ticket when it
// starts (tickets follow the publication order, so resident workgroups wait for the columns
// that come next), rather than persistent workgroups looping over items — a loop around the
// equilibrium body lets the compiler hoist its invariants and spill the 80-VGPR budget.
__global__ __launch_bounds__(kEqWide, kEqMinW) void eq_ready_kernel(LearnBufs L, const double* __restrict__ beta,
                                                                            const double* __restrict__ eta,
                                                                            const double* __restrict__ t_end,
                                                                            const double* __restrict__ u, LearnArgs la,
                                                                            EqArgs a, ReadyArgs ra, ResultSoA out)
{
    extern __shared__ double smem[];
    __shared__ int s_col, s_tile;
    const InterestArgs none{0.0, 1.0, 0.0, 0.0, 0, nullptr, nullptr, nullptr};
    if (threadIdx.x == 0) {
        const int it = atomicAdd(ra.head, 1);
        int col = -1, tile = 0;
        if (it < ra.n_items) {
            const int slot = it / ra.tiles;
            tile = it - slot * ra.tiles;
            const int v = ready_wait(ra.q + slot, ra.head + 1, ra.spin_limit);
            col = v ? v - 1 : -2;
            if (col >= 0 && tile > 0 && !ready_wait(ra.hz_flag + col, ra.head + 1, ra.spin_limit)) col = -2;
        }
        s_col = col;
        s_tile = tile;
    }
    __syncthreads();
    const int col = __builtin_amdgcn_readfirstlane(s_col), tile = __builtin_amdgcn_readfirstlane(s_tile);
    if (col == -1) return;
    if (col == -2) { // gave up waiting (a bug guard): the grid still drains
        if (threadIdx.x == 0) atomicOr(ra.head + 1, 1);
        return;
    }
    if (tile == 0) {
        // (the LDS-chunked path: the register-resident one needs 5 × 16 doubles per thread,
        // which the equilibrium's 80-VGPR budget would spill)
        hazard_column<kEqWide, false>(col, beta[col], eta[col], la, L, smem, smem + (HZ_LDS + 1),
                                          smem + 2 * (HZ_LDS + 1), smem + 3 * HZ_LDS + 2);
        __syncthreads();
        if (threadIdx.x == 0 && ra.tiles > 1)
            __hip_atomic_store(ra.hz_flag + col, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    const int j0 = tile * ra.tile_u;
    const int j1 = j0 + ra.tile_u < a.n_u ? j0 + ra.tile_u : a.n_u;
    eq_column<kEqWide, false>(col, j0, j1, L, eta, t_end, u, a, none, out, smem);
}

// ============================================================================
// One point by a whole workgroup (sbr_equilibrium_on_knots / sbr_solve_point_paths with
// n_u = 1: the drop-in's per-u calls).  The throughput kernel gives each point one lane, so a
// lone point pays every dependent LDS round trip of its searches (≈12 per lookup, ≈4 lookups
// per bisection iteration) and its staging runs on one wave.  Here the knots are staged by
// the whole block, wave 0 runs the point with wave-wide searches — searchsortedlast over [lo,
// hi] by 64-ary probing: one LDS load per lane and a ballot per round, two rounds for a
// Fig 5 column — and the block evaluates get_AW on every τ̄ knot (the exhaustive path), so
// AW_max and the three paths come from one pass.  The same operations as solve_point /
// solve_from_buffers' exact iteration and eval_range (each lookup lands on the bracket
// ssl_range finds: the knots are sorted), so the same bits.
// ============================================================================
__global__ __launch_bounds__(CO_BLOCK) void point_coop_kernel(LearnBufs L, const double* __restrict__ eta,
                                                              const double* __restrict__ t_end,
                                                              const double* __restrict__ u, EqArgs a, ResultSoA out)
{
    extern __shared__ double smem[];
    __shared__ double s_r[5];
    __shared__ uint32_t s_st;
    __shared__ int s_it;
    __shared__ double s_mx[CO_BLOCK / 64];
    const int n = L.n_knots[0], ntau = L.n_tau[0], nle = L.n_le[0];
    const uint32_t lst = L.status[0];
    const bool fits = n <= a.lds_cap && ntau <= a.lds_cap;
    double* sT = smem;
    double* sG = smem + a.lds_cap;
    double* sH = smem + 2 * a.lds_cap;
    if (fits) {
        for (int i = threadIdx.x; i < n; i += CO_BLOCK) { sT[i] = L.t[i]; sG[i] = L.G[i]; }
        for (int i = threadIdx.x; i < ntau; i += CO_BLOCK) sH[i] = L.hr[i];
    }
    __syncthreads();
    const double* T = fits ? (const double*)sT : (const double*)L.t;
    const double* G = fits ? (const double*)sG : (const double*)L.G;
    const double* H = fits ? (const double*)sH : (const double*)L.hr;
    // one workgroup per u value (a ξ_guess call over n_u values; paths only with one workgroup)
    const int jb = blockIdx.x;
    const double ETA = eta[0], T1 = t_end[0], uj = u[jb];
    const uint32_t lbits = lst & (SBR_ODE_MAXITERS | SBR_STIFF_SWITCH | SBR_ODE_FAILED | SBR_KNOT_OVERFLOW);
    const bool bad_col = (lst & (SBR_ARG_INVALID | SBR_OOB)) || n < 2;
    const bool trunc = !a.full_grid && n >= 2 && L.t[n - 1] < T1 && !(lst & kLearnCutBits);
    if (threadIdx.x < 64) {
        PointResult r;
        if (bad_col || !(uj >= 0.0)) {
            r.xi = NAN; r.aw = NAN; r.tol = INFINITY; r.iters = 0; r.tin = NAN; r.tout = NAN;
            r.status = ((lst & SBR_ARG_INVALID) || !(uj >= 0.0)) ? SBR_ARG_INVALID : (SBR_OOB | lbits);
        } else {
            point_wave(T, G, H, n, ntau, nle, ETA, T1, trunc, uj, a.kappa, a.max_iters, lbits, r, a.xi_guess);
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
        double* sc = a.path_scratch;
        if (sc && a.aw_path)
            co_eval(T, G, n, nle, ETA, xi, icc, occ, G0, i0, i1, mx, sc, a.aw_out_path ? sc + ntau : nullptr,
                    a.aw_in_path ? sc + 2 * ntau : nullptr);
        else
            co_eval(T, G, n, nle, ETA, xi, icc, occ, G0, i0, i1, mx, a.aw_path, a.aw_out_path, a.aw_in_path);
        // block reduction in thread order (NaN latches: any NaN gives NaN, else the max)
        for (int off = 32; off >= 1; off >>= 1) {
            const double o = __shfl_down(mx, off, 64);
            mx = (mx != mx || o != o) ? (double)NAN : (o > mx ? o : mx);
        }
        if ((threadIdx.x & 63) == 0) s_mx[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if ((st & SBR_RUN) && a.path_scratch && a.aw_path) {
        // the rows formed per thread in scratch, copied out with consecutive lanes on consecutive
        // entries (a mapped-host destination then takes whole-line writes)
        const double* sc = a.path_scratch;
        for (int i = threadIdx.x; i < ntau; i += CO_BLOCK) {
            a.aw_path[i] = sc[i];
            if (a.aw_out_path) a.aw_out_path[i] = sc[ntau + i];
            if (a.aw_in_path) a.aw_in_path[i] = sc[2 * ntau + i];
        }
    }
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

hipError_t launch_point_coop(const LearnBufs& L, const double* eta, const double* t_end, const double* u,
                             const EqArgs& a, const ResultSoA& out, hipStream_t s, int n_points)
{
    if (n_points > 1 && (a.aw_path || a.aw_out_path || a.aw_in_path || a.path_scratch)) return hipErrorInvalidValue;
    const size_t lds = (size_t)3 * a.lds_cap * sizeof(double);
    hipLaunchKernelGGL(point_coop_kernel, dim3(n_points), dim3(CO_BLOCK), lds, s, L, eta, t_end, u, a, out);
    return hipGetLastError();
}

// ============================================================================
// launchers
// ============================================================================
hipError_t launch_learn_kernel(const double* beta, const double* eta, const double* t_end, const LearnArgs& a,
                               const LearnBufs& L, hipStream_t s, int mode)
{
    const unsigned waves = (unsigned)((a.n_beta + 63) / 64);
    // heads first: whole grids of one-wave blocks only
    if (a.wpg && (mode == 0 || a.wpg < 2 || a.head < 1 || a.head >= a.wpg || a.n_beta % (64 * a.wpg) != 0))
        return hipErrorInvalidValue;
    if (mode == 2) { // LDS-staged rows with the fused hazard (launch_hazard_norm after)
        if (!a.fuse_hazard) return hipErrorInvalidValue;
        hipLaunchKernelGGL((learn_logistic_kernel<64, true>), dim3(waves), dim3(64), kStageLdsPerWave, s,
                           beta, eta, t_end, a, L);
    } else if (mode == 0) {
        hipLaunchKernelGGL(learn_logistic_kernel<kLearnBlock>, dim3((a.n_beta + kLearnBlock - 1) / kLearnBlock),
                           dim3(kLearnBlock), 0, s, beta, eta, t_end, a, L);
    } else {
        static_assert(kLearnBlockLat == 64, "mode 1 runs one-wave blocks");
        hipLaunchKernelGGL(learn_logistic_kernel<kLearnBlockLat>, dim3(waves), dim3(kLearnBlockLat), 0, s, beta, eta,
                           t_end, a, L);
    }
    return hipGetLastError();
}

hipError_t launch_hazard_norm(const LearnArgs& a, const LearnBufs& L, int n_cols, hipStream_t s)
{
    hipLaunchKernelGGL(hazard_norm_kernel, dim3(n_cols), dim3(HN_BLOCK), 0, s, a, L);
    return hipGetLastError();
}

hipError_t launch_learn_logistic(const double* beta, const double* eta, const double* t_end, const LearnArgs& a,
                                 const LearnBufs& L, hipStream_t s)
{
    hipError_t e = launch_learn_kernel(beta, eta, t_end, a, L, s, (a.fuse_hazard && !a.ready_q) ? 0 : 1);
    if (e != hipSuccess) return e;
    if (a.ready_q) return hipSuccess; // readiness sweep: eq_ready_kernel runs each column's hazard
    if (a.fuse_hazard) return launch_hazard_norm(a, L, a.n_beta, s);
    hipLaunchKernelGGL(hazard_kernel, dim3(a.n_beta), dim3(HZ_BLOCK), 0, s, beta,
                       eta, a, L);
    return hipGetLastError();
}

hipError_t launch_hazard(const double* beta, const double* eta, const LearnArgs& a, const LearnBufs& L, int n_beta,
                         hipStream_t s)
{
    hipLaunchKernelGGL(hazard_kernel, dim3(n_beta), dim3(HZ_BLOCK), 0, s, beta, eta, a, L);
    return hipGetLastError();
}

hipError_t launch_equilibrium(const LearnBufs& L, const double* eta, const double* t_end, const double* u,
                              const EqArgs& a, const ResultSoA& out, int n_beta, hipStream_t s, int only_mode)
{
    const size_t lds = ((size_t)2 * a.lds_cap + 6 * ((a.lds_cap >> 6) + 1) + 2 * ((a.lds_cap >> 3) + 1)) * sizeof(double);
    // one block per (β column, tile of EQ_TILE u values); block size by tile width.  Wide
    // tiles use 12-wave blocks: two per CU (LDS holds two columns' t and G) = 6 waves/SIMD.
    const int tiles = (a.n_u + EQ_TILE - 1) / EQ_TILE;
    const int w = a.n_u < EQ_TILE ? a.n_u : EQ_TILE;
    dim3 grid(tiles, n_beta);
    const InterestArgs none{0.0, 1.0, 0.0, 0.0, 0, nullptr, nullptr, nullptr};
    // the LDS-resident columns, then (a workgroup per column, exiting at once where it fits, no
    // LDS slab) the columns beyond the slab on the global-memory path
    auto go = [&](auto k1, auto k2, int bs) {
        if (only_mode != 2) hipLaunchKernelGGL(k1, grid, dim3(bs), lds, s, L, eta, t_end, u, a, none, out);
        if (only_mode != 1) hipLaunchKernelGGL(k2, grid, dim3(bs), 0, s, L, eta, t_end, u, a, none, out);
    };
    if (w > 256)
        go(equilibrium_kernel<kEqWide, false, 1>, equilibrium_kernel<kEqWide, false, 2>, kEqWide);
    else if (w > 64)
        go(equilibrium_kernel<256, false, 1>, equilibrium_kernel<256, false, 2>, 256);
    else
        go(equilibrium_kernel<64, false, 1>, equilibrium_kernel<64, false, 2>, 64);
    return hipGetLastError();
}

hipError_t launch_eq_ready(const LearnBufs& L, const double* beta, const double* eta, const double* t_end,
                           const double* u, const LearnArgs& la, const EqArgs& a, const ReadyArgs& ra,
                           const ResultSoA& out, int n_blocks, hipStream_t s)
{
    size_t lds = ((size_t)2 * a.lds_cap + 6 * ((a.lds_cap >> 6) + 1) + 2 * ((a.lds_cap >> 3) + 1)) * sizeof(double);
    const size_t hz = (size_t)(3 * HZ_LDS + 3) * sizeof(double); // hazard scratch shares the slab
    if (lds < hz) lds = hz;
    (void)n_blocks; // one workgroup per item
    hipLaunchKernelGGL(eq_ready_kernel, dim3(ra.n_items), dim3(kEqWide), lds, s, L, beta, eta, t_end, u, la, a, ra,
                       out);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void ready_fail_kernel(const int32_t* __restrict__ gave_up, ResultSoA out,
                                                          int64_t n_pts)
{
    if (__hip_atomic_load(gave_up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_pts; i += (int64_t)gridDim.x * 256) {
        out.xi[i] = NAN;
        out.tau_in_unc[i] = NAN;
        out.tau_out_unc[i] = NAN;
        out.aw_max[i] = NAN;
        out.tol[i] = INFINITY;
        out.status[i] = SBR_ENGINE_SCHED;
        if (out.iters) out.iters[i] = 0;
    }
}

hipError_t launch_ready_fail(const int32_t* gave_up, const ResultSoA& out, int64_t n_pts, hipStream_t s)
{
    hipLaunchKernelGGL(ready_fail_kernel, dim3(256), dim3(256), 0, s, gave_up, out, n_pts);
    return hipGetLastError();
}

hipError_t launch_interest(const LearnBufs& L, const double* eta, const double* t_end, const double* u,
                           const EqArgs& a, const InterestArgs& ia, const ResultSoA& out, int n_beta, hipStream_t s)
{
    const size_t lds = ((size_t)3 * a.lds_cap + 6 * ((a.lds_cap >> 6) + 1) + 2 * ((a.lds_cap >> 3) + 1)) * sizeof(double);
    // every lane integrates its own value function (~5·10⁴ Tsit5 steps): one wave per 64 u
    // of the column so that all of them run at once (the LDS slab allows one block per CU)
    const int tiles = (a.n_u + EQ_TILE - 1) / EQ_TILE;
    const int w = a.n_u < EQ_TILE ? a.n_u : EQ_TILE;
    dim3 grid(tiles, n_beta);
    auto go = [&](auto k1, auto k2, int bs) {
        hipLaunchKernelGGL(k1, grid, dim3(bs), lds, s, L, eta, t_end, u, a, ia, out);
        hipLaunchKernelGGL(k2, grid, dim3(bs), 0, s, L, eta, t_end, u, a, ia, out);
    };
    if (w > 512)
        go(equilibrium_kernel<1024, true, 1>, equilibrium_kernel<1024, true, 2>, 1024);
    else if (w > 256)
        go(equilibrium_kernel<512, true, 1>, equilibrium_kernel<512, true, 2>, 512);
    else if (w > 64)
        go(equilibrium_kernel<256, true, 1>, equilibrium_kernel<256, true, 2>, 256);
    else
        go(equilibrium_kernel<64, true, 1>, equilibrium_kernel<64, true, 2>, 64);
    return hipGetLastError();
}

}  // namespace sbr

#ifdef SBR_EQ_WGTIME
// diagnostic build only: copy the workgroup timeline of the last equilibrium launch (n entries)
extern "C" int sbr_diag_wgtime_read(unsigned long long* t2, unsigned int* hw2, int n)
{
    if (n < 0 || (size_t)n > sbr::kWgTimeMax) return -1;
    if (hipMemcpyFromSymbol(t2, HIP_SYMBOL(sbr::g_wgtime), sizeof(unsigned long long) * 2 * n) != hipSuccess) return -2;
    if (hipMemcpyFromSymbol(hw2, HIP_SYMBOL(sbr::g_wghw), sizeof(unsigned int) * 2 * n) != hipSuccess) return -2;
    return 0;
}
#endif
