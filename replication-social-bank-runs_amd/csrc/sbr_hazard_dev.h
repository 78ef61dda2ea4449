// sbr_hazard_dev.h — launch constants of the baseline kernels and hazard_rate (solver.jl:153-185) of one
// learning column by one workgroup (hazard_column), shared by the hazard kernel, the readiness
// sweep and the per-point kernel.  Device code; include from a .hip file.
#pragma once

#include "sbr_device.h"
#include "sbr_kernels.h"

namespace sbr {

constexpr int kEqWide = 768; // lanes per equilibrium workgroup on wide u tiles
constexpr int kEqMinW = 6;    // waves per SIMD the baseline equilibrium kernel must fit (two 12-wave blocks per CU)
constexpr int HZ_BLOCK = 256;
constexpr int HZ_LDS = 1024; // τ̄ knots per LDS chunk of the hazard kernel
constexpr int HZ_REG = 16;   // τ̄ knots per thread held in registers (ntau <= 4096: one pass over HBM)
constexpr int EQ_TILE = 4096; // u values per equilibrium block (one block per β column up to this)
constexpr int kAwWin = 6;     // 8-blocks each side of the predicted AW peak evaluated first

// I_k = I_{k-1} + term_k over s_I[0, cn) in place, left to right (the reference's rounding
// order), by the 64 lanes of one wave: lane l holds terms [16l, 16l + 16) in registers and
// the running integral passes from lane to lane — in round r only lane r adds (16 dependent
// adds), then v_readlane broadcasts its I.  The chain is the adds plus one broadcast per 16
// terms; a one-lane scan out of LDS waits on an LDS round trip every few terms instead.
// Call with all 64 lanes of the wave active; I must be wave-uniform (and is on return).
constexpr int HZ_LANE = HZ_LDS / 64; // terms per lane (16)
__device__ __forceinline__ double hz_bcast(double x, int lane)
{
    const uint64_t u = sbr_dbits(x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), lane);
    return sbr_bitsd(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ void hz_scan_wave(double* s_I, int cn, double& I)
{
    const int lane = threadIdx.x & 63, base = lane * HZ_LANE;
    double v[HZ_LANE];
#pragma unroll
    for (int j = 0; j < HZ_LANE; j++) v[j] = base + j < cn ? s_I[base + j] : 0.0;
    const int rounds = (cn + HZ_LANE - 1) / HZ_LANE;
    double acc = I;
    for (int r = 0; r < rounds; r++) {
        if (lane == r) {
            // the tail past cn adds +0.0, which leaves I (>= +0) unchanged
#pragma unroll
            for (int j = 0; j < HZ_LANE; j++) { acc = acc + v[j]; v[j] = acc; }
        }
        acc = hz_bcast(acc, r);
    }
    I = acc;
#pragma unroll
    for (int j = 0; j < HZ_LANE; j++)
        if (base + j < cn) s_I[base + j] = v[j];
}

#ifdef SBR_HZ_PROF // per-block phase cycles of the hazard kernel (tools/ubench_hazard.hip)
__device__ long long g_hzprof[8192 * 6];
#define HZ_T0 long long hz_tp = __builtin_amdgcn_s_memtime()
#define HZ_STAMP(ph)                                                                                  \
    do {                                                                                              \
        const long long hz_now = __builtin_amdgcn_s_memtime();                                        \
        if (threadIdx.x == 0) g_hzprof[(size_t)blockIdx.x * 6 + (ph)] += hz_now - hz_tp;              \
        hz_tp = hz_now;                                                                               \
    } while (0)
#else
#define HZ_T0
#define HZ_STAMP(ph)
#endif
// hazard_rate of column b by one workgroup of NT >= HZ_BLOCK threads (threads past HZ_BLOCK
// only take part in the barriers): the τ̄ grid in chunks of HZ_LDS knots, e_i·g_i and the
// trapezoid terms formed in parallel into LDS, one wave adds the terms left to right (the
// reference's rounding order), and a last parallel pass turns the partial integrals into
// HR_i.  LDS scratch: s_eg, s_t [HZ_LDS + 1], s_I [HZ_LDS], s_Ieta [1].  Every early
// return is uniform over the workgroup.
template <int NT, bool REGS = true>
__device__ __forceinline__ void hazard_column(const int b, const double BETA, const double ETA, const LearnArgs& a,
                                              const LearnBufs& L, double* s_eg, double* s_t, double* s_I,
                                              double* s_Ieta)
{
    static_assert(NT >= HZ_BLOCK, "hazard_column needs HZ_BLOCK threads");
    const int tid = threadIdx.x;
    const bool act = tid < HZ_BLOCK;
    HZ_T0;
    const int n = L.n_knots[b];
    const uint32_t st = L.status[b];
    if (st & SBR_ARG_INVALID) return; // learn kernel already wrote the row
    const size_t row = (size_t)b * (size_t)L.cap;
    const double* __restrict__ T = L.t + row;
    const double* __restrict__ Gv = L.G + row;
    double* __restrict__ H = L.hr + row;
    const double p = a.p, lam = a.lam;
    const int m = L.n_le[b]; // #knots ≤ η (searchsortedlast + 1), counted by the learning kernel
    bool oob = false, push;
    if (m < n) {
        push = (m == 0) || T[m - 1] != ETA; // solver.jl:159
        oob = (m == 0);                       // pdf(η) with η < t_0
    } else {
        push = (m == 0) || T[m - 1] != ETA;
        oob = push;                           // no knot beyond η to interpolate pdf(η)
    }
    const int ntau = m + (push ? 1 : 0);
    if (oob) {
        if (tid == 0) {
            L.status[b] = st | SBR_OOB;
            L.n_tau[b] = 0;
            L.n_le[b] = 0;
        }
        return;
    }
    // the pdf at knot i: compute_pdf_symbolic_baseline's βG(1 − G) (learning.jl:161-173), or the
    // caller's values (a.pdf: the interpolant of another pdf on the same knots)
    const double* __restrict__ PD = a.pdf ? a.pdf + row : nullptr; // the caller's pdf rows, laid out like G
    auto pdf_k = [&](int i) -> double {
        if (PD) return PD[i];
        const double x = Gv[i];
        return (BETA * x) * (1.0 - x);
    };
    auto pdf_at = [&](int i) -> double {
        if (i < m) return pdf_k(i);
        // η on bracket [m-1, m]
        const double g0 = pdf_k(m - 1);
        const double g1 = pdf_k(m);
        const double d = (ETA - T[m - 1]) / (T[m] - T[m - 1]);
        return g0 * (1.0 - d) + g1 * d;
    };
    auto tau_at = [&](int i) -> double { return i < m ? T[i] : ETA; };
    // Global reads are batched (unrolled loops, every load of a batch in flight before the
    // first use): the knots were written by another XCD's learning wave, so each one costs an
    // L2 miss, and one dependent miss per knot per thread would dominate the kernel.
    HZ_STAMP(0);
    if (REGS && ntau <= HZ_BLOCK * HZ_REG) {
        // Every τ̄ knot of the column in registers (thread tid owns knots tid + 256·j): one
        // batch of global loads, the chunks fed to LDS from registers, I_i read back into
        // registers, HR written once.
        double tv[HZ_REG], egv[HZ_REG], numv[HZ_REG], iv[HZ_REG], gk[HZ_REG];
        if (act) {
            // loads first, unconditionally (indices clamped into the knots ≤ η), so that all of
            // them are in flight at once; τ̄ = η and its interpolated pdf are selected after
            const double pdf_eta = m < n ? pdf_at(m) : 0.0; // m == n: η is a knot, not pushed
#pragma unroll
            for (int j = 0; j < HZ_REG; j++) {
                const int i = tid + HZ_BLOCK * j;
                const int ic = i < m ? i : m - 1;
                tv[j] = T[ic];
                gk[j] = PD ? PD[ic] : Gv[ic];
            }
#pragma unroll
            for (int j = 0; j < HZ_REG; j++) {
                const int i = tid + HZ_BLOCK * j;
                const double x = gk[j];
                const double ti = i < m ? tv[j] : ETA;
                const double g = i < m ? (PD ? x : (BETA * x) * (1.0 - x)) : pdf_eta;
                const double E = sbr_exp(lam * ti);
                tv[j] = ti;
                egv[j] = E * g;        // e_i = exp(λτ̄_i)·pdf_i
                numv[j] = (p * E) * g; // the HR numerator (p·exp(λτ̄_i))·pdf_i
                iv[j] = 0.0;
            }
        }
        double I = 0.0;
        constexpr int RPC = HZ_LDS / HZ_BLOCK; // register slots per LDS chunk
#pragma unroll
        for (int c = 0; c < HZ_REG / RPC; c++) {
            const int c0 = c * HZ_LDS;
            if (c0 < ntau) { // uniform
                const int cn = ntau - c0 < HZ_LDS ? ntau - c0 : HZ_LDS;
                if (act) {
#pragma unroll
                    for (int r = 0; r < RPC; r++) {
                        const int k = tid + HZ_BLOCK * r;
                        s_t[k + 1] = tv[c * RPC + r];
                        s_eg[k + 1] = egv[c * RPC + r];
                    }
                    if (c > 0 && tid == HZ_BLOCK - 1) { // knot c0 − 1 is this thread's last slot
                        s_t[0] = tv[c * RPC - 1];
                        s_eg[0] = egv[c * RPC - 1];
                    }
                }
                __syncthreads();
                HZ_STAMP(1);
                if (act)
                    for (int k = tid; k < cn; k += HZ_BLOCK)
                        s_I[k] = c0 + k == 0 ? 0.0 : (0.5 * (s_eg[k] + s_eg[k + 1])) * (s_t[k + 1] - s_t[k]);
                __syncthreads();
                HZ_STAMP(2);
                if (tid < 64) hz_scan_wave(s_I, cn, I);
                __syncthreads();
                HZ_STAMP(3);
                if (act) {
#pragma unroll
                    for (int r = 0; r < RPC; r++) {
                        const int k = tid + HZ_BLOCK * r;
                        if (k < cn) iv[c * RPC + r] = s_I[k];
                    }
                }
                __syncthreads(); // the chunk's LDS is reused
                HZ_STAMP(4);
            }
        }
        if (tid == 0) {
            s_Ieta[0] = I;
            L.n_tau[b] = ntau;
            L.n_le[b] = m;
        }
        __syncthreads();
        const double Ieta = s_Ieta[0], omp = 1.0 - p;
        if (act) {
#pragma unroll
            for (int j = 0; j < HZ_REG; j++) {
                const int i = tid + HZ_BLOCK * j;
                if (i < ntau) H[i] = numv[j] / ((p * iv[j]) + (omp * Ieta));
            }
        }
        HZ_STAMP(5);
        return;
    }
    double I = 0.0, egprev = 0.0, tprev = 0.0; // thread 0: running integral; the chunk's last e·g, τ̄
    for (int c0 = 0; c0 < ntau; c0 += HZ_LDS) {
        const int cn = ntau - c0 < HZ_LDS ? ntau - c0 : HZ_LDS;
        if (tid == 0) { s_eg[0] = egprev; s_t[0] = tprev; }
        if (act) {
#pragma unroll 4
            for (int k = tid; k < cn; k += HZ_BLOCK) {
                const int i = c0 + k;
                const double ti = tau_at(i);
                s_t[k + 1] = ti;
                s_eg[k + 1] = sbr_exp(lam * ti) * pdf_at(i); // e_i = exp(λτ̄_i)·pdf_i
            }
        }
        __syncthreads();
        HZ_STAMP(1);
        // trapezoid term of i pairs e_{i-1}, e_i (solver.jl:173-175); term_0 = 0
        if (act)
            for (int k = tid; k < cn; k += HZ_BLOCK)
                s_I[k] = c0 + k == 0 ? 0.0 : (0.5 * (s_eg[k] + s_eg[k + 1])) * (s_t[k + 1] - s_t[k]);
        __syncthreads();
        HZ_STAMP(2);
        if (tid < 64) hz_scan_wave(s_I, cn, I); // I_i = I_{i-1} + term_i, left to right
        if (tid == 0) {
            egprev = s_eg[cn];
            tprev = s_t[cn];
        }
        __syncthreads();
        HZ_STAMP(3);
        if (act)
            for (int k = tid; k < cn; k += HZ_BLOCK) H[c0 + k] = s_I[k]; // I_i parked in the HR row
        __syncthreads(); // the chunk's LDS is reused
        HZ_STAMP(4);
    }
    if (tid == 0) {
        s_Ieta[0] = I;
        L.n_tau[b] = ntau;
        L.n_le[b] = m;
    }
    __syncthreads();
    // HR_i = (p·exp(λτ̄_i))·pdf_i / (p·I_i + (1 − p)·I_η); each thread reads back the I_i it parked
    const double Ieta = s_Ieta[0], omp = 1.0 - p;
    if (act) {
#pragma unroll 4
        for (int i = tid; i < ntau; i += HZ_BLOCK) {
            const double E = sbr_exp(lam * tau_at(i));
            H[i] = ((p * E) * pdf_at(i)) / ((p * H[i]) + (omp * Ieta));
        }
    }
    HZ_STAMP(5);
}

}  // namespace sbr
