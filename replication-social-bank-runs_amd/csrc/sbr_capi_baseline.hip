// sbr_capi_baseline.hip — the baseline model's entry points of the C API: the learning workspaces,
// single sweeps (chunked and readiness schedules), the pipelined batch, lists of models
// (sbr_solve_points), β × p × λ × κ × u (sbr_sweep_econ), the interest-rate extension and its product
// with the economic parameters (sbr_sweep_interest_econ).
#include "sbr_hostio.h"

using namespace sbr_capi;

namespace sbr_capi {

void free_learn(sbr_ctx* c, int slot)
{
    sbr::LearnBufs& L = c->LW[slot];
    free_dev(L.t, L.G, L.hr, L.hrI, L.n_knots, L.n_tau, L.n_le, L.status, L.n_accept, L.n_reject);
    L = sbr::LearnBufs{};
    c->ws_beta[slot] = c->ws_cap[slot] = 0;
}

// Row stride of a learning workspace for a knot capacity: the capacity rounded up to a 128-B line
// plus one line.  A wave's 64 lanes each stream their own column's row; with a power-of-two
// stride (65536 knots = 512 KiB) all 64 rows map to the same L2 set and channel, the partial
// lines are evicted before they fill, and every 8-B knot store costs a memory write.
size_t learn_ld(size_t cap) { return ((cap + 15) & ~(size_t)15) + 16; }

int ensure_learn(sbr_ctx* c, size_t n_beta, size_t cap, int slot, bool hri)
{
    if (n_beta <= c->ws_beta[slot] && cap == c->ws_cap[slot] && (!hri || c->LW[slot].hrI)) return SBR_OK;
    free_learn(c, slot);
    sbr::LearnBufs& L = c->LW[slot];
    const size_t ld = learn_ld(cap);
    const size_t slab = n_beta * ld * sizeof(double);
    // hrI: the hazard kernel scans in LDS; the fused hazard (batch) parks I here
    const int rc = alloc_dev(c, {{L.t, slab}, {L.G, slab}, {L.hr, slab}, {L.hrI, hri ? slab : 0},
                                 {L.n_knots, n_beta * 4}, {L.n_tau, n_beta * 4}, {L.n_le, n_beta * 4},
                                 {L.status, n_beta * 4}, {L.n_accept, n_beta * 4}, {L.n_reject, n_beta * 4}});
    if (rc) return rc;
    L.cap = (int32_t)ld;
    L.lim = (int32_t)cap;
    c->ws_beta[slot] = n_beta;
    c->ws_cap[slot] = cap;
    return SBR_OK;
}

// The learning-only entry points return the learning solve's status (solve_learning has no
// hazard): a column's status word also holds the hazard stage's SBR_OOB — no knot at η, as after a
// solve that maxiters or the knot capacity cut short — which is no outcome of the learning solve.
void strip_hazard_status(uint32_t* status, int64_t n)
{
    for (int64_t i = 0; status && i < n; i++) status[i] &= ~(uint32_t)SBR_OOB;
}

// highest-priority learning streams + events of the pipelined batch sweeps
int ensure_pipe_streams(sbr_ctx* c)
{
    if (c->lstream[0]) return SBR_OK;
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi); // hi = greatest priority
    for (int k = 0; k < sbr_ctx::kLearnStreams; k++)
        HIP_TRY(c, hipStreamCreateWithPriority(&c->lstream[k], hipStreamNonBlocking, hi), SBR_EDEVICE);
    for (int k = 0; k < sbr_ctx::kLearnSlots; k++) {
        HIP_TRY(c, hipEventCreateWithFlags(&c->ev_learned[k], kSyncEventFlags), SBR_EDEVICE);
        HIP_TRY(c, hipEventCreateWithFlags(&c->ev_eq[k], kSyncEventFlags), SBR_EDEVICE);
    }
    HIP_TRY(c, hipEventCreateWithFlags(&c->ev_in, kSyncEventFlags), SBR_EDEVICE);
    return SBR_OK;
}

void free_econ(sbr_ctx* c)
{
    free_dev(c->ec_hr, c->ec_cnt);
    c->ec_rows = c->ec_ld = 0;
}

int ensure_econ(sbr_ctx* c, size_t rows, size_t ld)
{
    if (rows <= c->ec_rows && ld == c->ec_ld) return SBR_OK;
    free_econ(c);
    const int rc = alloc_dev(c, {{c->ec_hr, rows * ld * sizeof(double)}, {c->ec_cnt, rows * 3 * sizeof(int32_t)}});
    if (rc) return rc;
    c->ec_rows = rows;
    c->ec_ld = ld;
    return SBR_OK;
}

}  // namespace sbr_capi

namespace {

// Truncated learning (DESIGN.md §Truncated learning) stores a bit-exact prefix of the full solve,
// but its status is the prefix's too: an SBR_ODE_MAXITERS or SBR_STIFF_SWITCH bit that the
// reference's solve to t_end sets after the stop point would be lost.  With integrator options
// of the caller's (a cap that the tail can reach, a tolerance at which Tsit5 hands over late) the
// sweeps therefore integrate to t_end; the equilibrium stage reads the same knots either way.
int32_t stop_after_eta(const sbr_opts& o)
{
    const double e = 2.220446049250313e-16;
    return (o.ode_reltol == e && o.ode_abstol == e && o.ode_maxiters >= SBR_DEFAULT_ODE_MAXITERS) ? 1 : 0;
}

int launch_eq(sbr_ctx* c, hipStream_t s, const sbr::LearnBufs& L, const double* eta, const double* t_end,
              const double* u, int64_t n_beta, int64_t n_u, double kappa, const sbr_opts& o,
              const sbr::ResultSoA& out, double* aw_path, int group = 1, bool timed = true)
{
    sbr::EqArgs ea{kappa, (int32_t)n_u, o.bisect_max_iters, c->lds_cap_b, aw_path,
                   (o.flags & SBR_FLAG_EXHAUSTIVE) ? 1 : 0, (o.flags >> 8) & 0x17};
    ea.group = group;
    hipEvent_t t0 = timed ? tstart(c, s) : nullptr;
    if (aw_path && n_beta == 1 && n_u == 1) { // single point with its path: the whole workgroup on it
        ea.lds_cap = c->lds_cap;
        HIP_TRY(c, sbr::launch_point_coop(L, eta, t_end, u, ea, out, s), SBR_EDEVICE);
        tend(c, s, 1, t0);
        return SBR_OK;
    }
    HIP_TRY(c, sbr::launch_equilibrium(L, eta, t_end, u, ea, out, (int)n_beta, s), SBR_EDEVICE);
    tend(c, s, 1, t0);
    return SBR_OK;
}

// Pipelined batch plan (sbr_sweep_baseline_batch_dev).  The learning kernel is latency-bound
// (one serial ODE per lane, ≈32 waves per 2048-column grid) and a launch lasts as long as its
// slowest column whatever its width; run beside the equilibrium kernel a learning wave holds
// an equilibrium workgroup slot of its CU (169 VGPRs next to 6 × 80) and issues ahead of it.
// So the batch learns as many grids as it can in ONE launch — up to SBR_BATCH_LEARN_WAVES waves,
// at most one per SIMD — while the chip has nothing else to do, and then runs the equilibria
// back to back with nothing beside them; a batch longer than that learns its next group into
// the second workspace beside the first group's equilibria.
#ifndef SBR_BATCH_LEARN_WAVES
#define SBR_BATCH_LEARN_WAVES 768 // learning waves per batch learning launch (of 1,024 SIMDs)
#endif
#ifndef SBR_BATCH_EQ_COLS
#define SBR_BATCH_EQ_COLS 4096 // columns per equilibrium launch of a batch (two full grids: one tail per two)
#endif
struct BatchPlan {
    int64_t L = 1;  // grids per learning launch (and workspace slot)
    int64_t E = 1;  // grids per equilibrium launch
    int nslot = 1;  // workspace slots in rotation (1 when one group holds the batch, else 2)
};

// bytes of one learning column of a batch workspace: t, G, the HR numerators and the running
// integrals (cap doubles each) and six counters
size_t batch_col_bytes(size_t cap) { return learn_ld(cap) * 4 * sizeof(double) + 6 * sizeof(int32_t); }

// Size the plan and its workspaces.  L is capped by the wave budget and by the memory budget
// (c->bt_budget, default 40 % of the free plus the already held HBM); if an allocation fails
// anyway the slots are released and L is halved, down to one grid (then SBR_ENOMEM).
int batch_alloc(sbr_ctx* c, int64_t n_batch, int64_t n_beta, size_t cap, BatchPlan& P)
{
    const int64_t wpg = (n_beta + 63) / 64; // learning waves per grid
    int64_t L = SBR_BATCH_LEARN_WAVES / wpg;
    if (L < 1) L = 1;
    if (L > n_batch) L = n_batch;
    size_t freeb = 0, total = 0;
    (void)hipMemGetInfo(&freeb, &total);
    size_t held = 0;
    for (int k = 0; k < 2; k++) held += c->ws_beta[k] * batch_col_bytes(c->ws_cap[k]);
    const double budget = c->bt_budget > 0 ? (double)c->bt_budget : 0.4 * (double)(freeb + held);
    const double per_grid = (double)n_beta * (double)batch_col_bytes(cap);
    for (;;) {
        int nslot = n_batch > L ? 2 : 1;
        while (L > 1 && (double)(L * nslot) * per_grid > budget) {
            L = L > 2 ? (L + 1) / 2 : 1;
            nslot = n_batch > L ? 2 : 1;
        }
        // balanced groups: ⌈n_batch / L⌉ groups of (nearly) equal size
        const int64_t ng = (n_batch + L - 1) / L;
        L = (n_batch + ng - 1) / ng;
        nslot = ng > 1 ? 2 : 1;
        // launch columns are int32 in the kernels' arguments
        if (L * n_beta > INT32_MAX) return fail(c, SBR_EARG, "batch: n_beta too large for one learning launch");
        int rc = SBR_OK;
        for (int k = 0; k < nslot && rc == SBR_OK; k++) rc = ensure_learn(c, (size_t)(L * n_beta), cap, k, true);
        if (rc == SBR_OK) {
            P.L = L;
            P.nslot = nslot;
            int64_t E = (SBR_BATCH_EQ_COLS + n_beta - 1) / n_beta;
            P.E = E < 1 ? 1 : (E > L ? L : E);
            return SBR_OK;
        }
        for (int k = 0; k < sbr_ctx::kLearnSlots; k++) free_learn(c, k);
        if (L == 1) return rc;
        // the failed hipMalloc left hipErrorOutOfMemory as the thread's last error: clear it, or
        // the next launch check (hipGetLastError) would report it against a good launch
        (void)hipGetLastError();
        L = (L + 1) / 2;
    }
}

// the learning buffers / results of columns [c0, ...) of a sweep (row views)
sbr::LearnBufs learn_rows(const sbr::LearnBufs& L, size_t c0)
{
    const size_t k = c0 * (size_t)L.cap;
    return {L.t + k,        L.G + k,        L.hr + k,     L.hrI + k,         L.n_knots + c0, L.n_tau + c0,
            L.n_le + c0,    L.status + c0,  L.n_accept + c0, L.n_reject + c0, L.cap, L.lim};
}
sbr::ResultSoA result_rows(const sbr::ResultSoA& r, size_t off)
{
    auto at = [off](auto* p) { return p ? p + off : p; };
    return {at(r.xi), at(r.tau_in_unc), at(r.tau_out_unc), at(r.aw_max), at(r.tol), at(r.status), at(r.iters)};
}

// One sweep.  Every learning column is a serial ODE on one lane, and the launch lasts as long
// as its slowest column (config 3: one column takes 4.4k steps where the median takes 2.9k),
// while the equilibrium stage is a throughput kernel over the whole chip.  Wide sweeps are
// therefore cut into kSweepChunks column chunks, each learned and solved on its own learning
// stream: the equilibria of the chunks that finish learning early run while the slowest
// chunk is still integrating.  Timing records: kind 0 = the learning stage of all chunks
// (fork to the last chunk learned), kind 1 = the equilibrium tail after it.
constexpr int kSweepChunks = sbr_ctx::kLearnStreams;
// pipelined batch: hazard_rate streamed by the learning kernel (no separate hazard launch
// competing with the equilibrium kernel for CU slots); single sweeps keep the hazard kernel
constexpr int kSweepFront = 32;       // the front chunk of a single sweep: 1/32 of the waves (halving only: 4.44 vs 4.25 ms)
constexpr int kReadyLearnCus = 64;    // CUs reserved for the learning waves (8 / 16 / 32 / 64: 13.3 / 9.2 / 3.5 / 3.0 ms of learning)
constexpr int kReadyTileU = 4096;     // u values per equilibrium workgroup (768: three tiles of a config-3 column, 6.7 vs 5.5 ms)
constexpr int kReadySpin = 1 << 24;   // polls (≈ 0.5 µs each) before a waiting workgroup gives up: a bug guard

// the streams with disjoint CU masks and the queue of a readiness sweep
int ensure_ready(sbr_ctx* c, size_t n_beta)
{
    if (c->rs_state == 0) {
        c->rs_state = -1;
        int ncu = 0;
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device);
        if (ncu >= 4 * kReadyLearnCus) {
            std::vector<uint32_t> ml((size_t)(ncu + 31) / 32, 0u), me(ml.size(), 0u);
            for (int i = 0; i < ncu; i++) (i < kReadyLearnCus ? ml : me)[(size_t)i / 32] |= 1u << (i % 32);
            if (hipExtStreamCreateWithCUMask(&c->rs_learn, (uint32_t)ml.size(), ml.data()) == hipSuccess &&
                hipExtStreamCreateWithCUMask(&c->rs_eq, (uint32_t)me.size(), me.data()) == hipSuccess &&
                hipEventCreateWithFlags(&c->ev_rin, kSyncEventFlags) == hipSuccess &&
                hipEventCreateWithFlags(&c->ev_rq, kSyncEventFlags) == hipSuccess &&
                hipEventCreateWithFlags(&c->ev_rl, kSyncEventFlags) == hipSuccess &&
                hipEventCreateWithFlags(&c->ev_re, kSyncEventFlags) == hipSuccess)
                c->rs_state = 1;
        }
    }
    if (c->rs_state != 1) return SBR_EDEVICE;
    const size_t need = 4 + 2 * n_beta;
    if (need > c->rq_cap) {
        if (c->rq) (void)hipFree(c->rq);
        c->rq = nullptr;
        c->rq_cap = 0;
        HIP_TRY(c, hipMalloc(&c->rq, need * 4), SBR_ENOMEM);
        c->rq_cap = need;
    }
    return SBR_OK;
}

// One sweep, readiness schedule (SBR_FLAG_READY_SWEEP): the learning kernel publishes every
// column the moment its lane has solved it (release), and one equilibrium workgroup per
// (column, u-tile) — in publication order, on the CUs the learning waves do not use — runs
// the column's hazard (tile 0) and equilibria (acquire).  Measured on config 3 it is slower
// than the chunked schedule (5.5 vs 4.3 ms): most columns' learning ends late (≈2.8k steps of
// a ≈4.4k-step maximum), so the equilibria cannot start much earlier, and they lose the
// learning CUs.  Timing records: kind 0 = the learning kernel, kind 1 = the equilibrium
// kernel (concurrent).
int run_baseline_ready(sbr_ctx* c, hipStream_t s, const double* beta, const double* eta, const double* t_end,
                       const double* u, int64_t n_beta, int64_t n_u, double kappa, const sbr_opts& o,
                       sbr::LearnArgs la, const sbr::ResultSoA& out)
{
    const int tiles = (int)((n_u + kReadyTileU - 1) / kReadyTileU);
    int32_t* q = c->rq;
    HIP_TRY(c, hipEventRecord(c->ev_rin, s), SBR_EDEVICE);
    HIP_TRY(c, hipStreamWaitEvent(c->rs_learn, c->ev_rin, 0), SBR_EDEVICE);
    HIP_TRY(c, hipMemsetAsync(q, 0, (4 + 2 * (size_t)n_beta) * 4, c->rs_learn), SBR_EDEVICE);
    HIP_TRY(c, hipEventRecord(c->ev_rq, c->rs_learn), SBR_EDEVICE);
    HIP_TRY(c, hipStreamWaitEvent(c->rs_eq, c->ev_rq, 0), SBR_EDEVICE);
    la.fuse_hazard = 0;
    la.ready_tail = q + 2;
    la.ready_q = q + 4;
    hipEvent_t t0 = tstart(c, c->rs_learn);
    HIP_TRY(c, sbr::launch_learn_logistic(beta, eta, t_end, la, c->LW[0], c->rs_learn), SBR_EDEVICE);
    tend(c, c->rs_learn, 0, t0);
    sbr::EqArgs ea{kappa, (int32_t)n_u, o.bisect_max_iters, c->lds_cap_b, nullptr,
                   (o.flags & SBR_FLAG_EXHAUSTIVE) ? 1 : 0, (o.flags >> 8) & 0x17};
    sbr::ReadyArgs ra{q, q + 4, q + 4 + n_beta, (int32_t)(n_beta * tiles), tiles, kReadyTileU, kReadySpin};
    hipEvent_t t1 = tstart(c, c->rs_eq);
    HIP_TRY(c, sbr::launch_eq_ready(c->LW[0], beta, eta, t_end, u, la, ea, ra, out, 0, c->rs_eq), SBR_EDEVICE);
    tend(c, c->rs_eq, 1, t1);
    HIP_TRY(c, hipEventRecord(c->ev_rl, c->rs_learn), SBR_EDEVICE);
    HIP_TRY(c, hipEventRecord(c->ev_re, c->rs_eq), SBR_EDEVICE);
    HIP_TRY(c, hipStreamWaitEvent(s, c->ev_rl, 0), SBR_EDEVICE);
    HIP_TRY(c, hipStreamWaitEvent(s, c->ev_re, 0), SBR_EDEVICE);
    // a workgroup that gave up left its tile unwritten: mark the whole sweep on the device, so a
    // *_dev caller sees it in the results (the host-pointer entry point also returns SBR_EDEVICE)
    HIP_TRY(c, sbr::launch_ready_fail(q + 1, out, n_beta * n_u, s), SBR_EDEVICE);
    return SBR_OK;
}

int run_baseline(sbr_ctx* c, hipStream_t s, const double* beta, const double* eta, const double* t_end, double x0,
                 const double* u, int64_t n_beta, int64_t n_u, double p, double kappa, double lambda,
                 const sbr_opts& o, const sbr::ResultSoA& out, double* aw_path)
{
    int rc = ensure_learn(c, (size_t)n_beta, (size_t)o.knot_capacity);
    if (rc) return rc;
    c->last_slot = 0;
    c->last_off = 0;
    sbr::LearnArgs la{x0, o.ode_reltol, o.ode_abstol, p, lambda, o.ode_maxiters, (int32_t)n_beta, stop_after_eta(o), 0};
    // per-column readiness on request (SBR_FLAG_READY_SWEEP): see above
    c->rs_used = !aw_path && n_beta >= 64 && (o.flags & SBR_FLAG_READY_SWEEP) &&
                 ensure_ready(c, (size_t)n_beta) == SBR_OK;
    if (c->rs_used) return run_baseline_ready(c, s, beta, eta, t_end, u, n_beta, n_u, kappa, o, la, out);
    if (aw_path || n_beta < 64 * kSweepChunks) {
        hipEvent_t t0 = tstart(c, s);
        HIP_TRY(c, sbr::launch_learn_logistic(beta, eta, t_end, la, c->LW[0], s), SBR_EDEVICE);
        tend(c, s, 0, t0);
        return launch_eq(c, s, c->LW[0], eta, t_end, u, n_beta, n_u, kappa, o, out, aw_path);
    }
    rc = ensure_pipe_streams(c);
    if (rc) return rc;
    // chunk boundaries on whole waves (64 columns), halving towards the front: the last chunk
    // gets half of the columns, the others 1/4, 1/8, ...  The longest learning columns of a
    // β-descending grid (Fig 5: large β, outliers of up to 1.5x the median steps) sit in the
    // front chunks, whose equilibria, last to start, then fill one round of workgroups.
    const int64_t waves = (n_beta + 63) / 64;
    int64_t lo[kSweepChunks + 1];
    lo[0] = 0;
    lo[kSweepChunks] = n_beta;
    for (int k = kSweepChunks - 1; k >= 1; k--) {
        const int64_t wk = waves >> (kSweepChunks - k); // waves before chunk k
        lo[k] = std::min<int64_t>(n_beta, std::max<int64_t>(wk * 64, (int64_t)k * 64));
    }
    // the front chunk is 1/kSweepFront of the waves (the Fig 5 grid's outliers sit in
    // its first wave: 1.25x the steps of the next slowest)
    lo[1] = std::min<int64_t>(lo[2] - 64, std::max<int64_t>(64, (waves / kSweepFront) * 64));
    HIP_TRY(c, hipEventRecord(c->ev_in, s), SBR_EDEVICE);
    hipEvent_t t0 = tstart(c, s);
    c->ck_start = c->timing ? t0 : nullptr;
    c->ck_ev.assign(c->timing ? 2 * kSweepChunks : 0, nullptr);
    for (int k = 0; k < kSweepChunks; k++) {
        hipStream_t ls = c->lstream[k];
        const int64_t c0 = lo[k], nb = lo[k + 1] - lo[k];
        HIP_TRY(c, hipStreamWaitEvent(ls, c->ev_in, 0), SBR_EDEVICE);
        if (nb <= 0) continue;
        sbr::LearnArgs lk = la;
        lk.n_beta = (int32_t)nb;
        const sbr::LearnBufs Lk = learn_rows(c->LW[0], (size_t)c0);
        HIP_TRY(c, sbr::launch_learn_logistic(beta + c0, eta + c0, t_end + c0, lk, Lk, ls), SBR_EDEVICE);
        if (c->timing) {
            c->ck_ev[2 * k] = next_event(c);
            if (c->ck_ev[2 * k]) (void)hipEventRecord(c->ck_ev[2 * k], ls);
        }
        HIP_TRY(c, hipEventRecord(c->ev_learned[k], ls), SBR_EDEVICE);
        sbr::EqArgs ea{kappa, (int32_t)n_u, o.bisect_max_iters, c->lds_cap_b, nullptr,
                       (o.flags & SBR_FLAG_EXHAUSTIVE) ? 1 : 0, (o.flags >> 8) & 0x17};
        HIP_TRY(c, sbr::launch_equilibrium(Lk, eta + c0, t_end + c0, u, ea, result_rows(out, (size_t)(c0 * n_u)),
                                           (int)nb, ls), SBR_EDEVICE);
        if (c->timing) {
            c->ck_ev[2 * k + 1] = next_event(c);
            if (c->ck_ev[2 * k + 1]) (void)hipEventRecord(c->ck_ev[2 * k + 1], ls);
        }
        HIP_TRY(c, hipEventRecord(c->ev_eq[k], ls), SBR_EDEVICE);
    }
    for (int k = 0; k < kSweepChunks; k++)
        if (lo[k + 1] > lo[k]) HIP_TRY(c, hipStreamWaitEvent(s, c->ev_learned[k], 0), SBR_EDEVICE);
    hipEvent_t t1 = tstart(c, s);
    tend(c, s, 0, t0);
    for (int k = 0; k < kSweepChunks; k++)
        if (lo[k + 1] > lo[k]) HIP_TRY(c, hipStreamWaitEvent(s, c->ev_eq[k], 0), SBR_EDEVICE);
    tend(c, s, 1, t1);
    return SBR_OK;
}

// workspace bytes a point of a list counts for against the budget (sbr.h: sbr_set_points_workspace)
size_t point_bytes(size_t cap) { return 4 * cap * sizeof(double) + 6 * sizeof(int32_t); }

// A list of models (sbr_solve_points): n points, each with its own seven parameters, in chunks
// of at most n_chunk points through learning slot 0, all in stream order on s — the learning
// launch of a single sweep (one lane per point, truncated after η, no hazard), then one
// points_kernel workgroup per point.  A chunk's learning starts after the previous chunk's
// equilibria (they share the rows); no host synchronisation.  Timing records: kind 0 = the
// learning launches, kind 1 = the points kernel.
int run_points(sbr_ctx* c, hipStream_t s, const double* beta, const double* eta, const double* t_end, double x0,
               const double* u, const double* p, const double* kappa, const double* lambda, int64_t n,
               const sbr_opts& o, const sbr::ResultSoA& out)
{
    const size_t cap = (size_t)o.knot_capacity;
    size_t freeb = 0, total = 0;
    (void)hipMemGetInfo(&freeb, &total);
    const size_t held = c->ws_beta[0] * batch_col_bytes(c->ws_cap[0]);
    const double budget = c->pt_budget > 0 ? (double)c->pt_budget : 0.4 * (double)(freeb + held);
    int64_t n_chunk = (int64_t)(budget / (double)point_bytes(cap));
    if (n_chunk > 64) n_chunk &= ~(int64_t)63; // whole learning waves
    n_chunk = std::max<int64_t>(1, std::min<int64_t>(n_chunk, n));
    // a workspace that already holds enough rows of this capacity is used as it is
    for (;;) {
        const int rc = ensure_learn(c, (size_t)n_chunk, cap);
        if (rc == SBR_OK) break;
        free_learn(c, 0);
        if (n_chunk == 1) return rc;
        (void)hipGetLastError(); // the failed hipMalloc's error must not surface at the next launch check
        n_chunk = (n_chunk + 1) / 2;
    }
    c->last_slot = 0;
    c->last_off = 0;
    c->rs_used = false;
    const sbr::LearnBufs& L = c->LW[0];
    for (int64_t c0 = 0; c0 < n; c0 += n_chunk) {
        const int64_t nc = std::min<int64_t>(n_chunk, n - c0);
        // p and λ are per point: the hazard runs in points_kernel, not in the learning launch
        sbr::LearnArgs la{x0, o.ode_reltol, o.ode_abstol, 0.0, 0.0, o.ode_maxiters, (int32_t)nc, stop_after_eta(o), 0};
        hipEvent_t t0 = tstart(c, s);
        HIP_TRY(c, sbr::launch_learn_kernel(beta + c0, eta + c0, t_end + c0, la, L, s, 1), SBR_EDEVICE);
        tend(c, s, 0, t0);
        const sbr::PointArgs pa{beta + c0, eta + c0,    t_end + c0,         u + c0,    p + c0,
                                kappa + c0, lambda + c0, o.bisect_max_iters, c->lds_cap};
        t0 = tstart(c, s);
        HIP_TRY(c, sbr::launch_points(L, la, pa, result_rows(out, (size_t)c0), (int)nc, s), SBR_EDEVICE);
        tend(c, s, 1, t0);
    }
    return SBR_OK;
}

// workspace bytes a (column, class) pair counts for against the budget (sbr.h: sbr_sweep_econ)
size_t econ_class_bytes(size_t cap) { return cap * sizeof(double) + 3 * sizeof(int32_t); }

// β × p × λ × κ × u (sbr_sweep_econ), all in stream order on s: the learning launch of a single
// sweep once (one lane per column, truncated after η at default opts, no hazard), then per chunk
// of hazard classes (p[a], λ[b]) the hazard launch — one workgroup per (column, class) — and the
// equilibrium launches over the κ × u planes.  A chunk's hazards start after the previous
// chunk's equilibria (they share the class rows); no host synchronisation.  Timing records:
// kind 0 = the learning launch, kind 1 = the hazard and equilibrium launches.
// With `rates` (sbr_sweep_interest_econ) the equilibrium launches are the interest-rate model's over
// the rate × u planes, every κ solved on one value function (sbr_interest_econ.hip); out then has a
// rate axis outside κ.
struct RateAxis {
    const double *r, *delta; // n pairs, on the device
    int64_t n;
    int64_t* steps;          // value-function steps, no κ axis (may be null)
};
int run_econ(sbr_ctx* c, hipStream_t s, const double* beta, const double* eta, const double* t_end, double x0,
             const double* u, int64_t n_beta, int64_t n_u, const double* p, int64_t n_p, const double* lambda,
             int64_t n_lambda, const double* kappa, int64_t n_kappa, const sbr_opts& o, const sbr::ResultSoA& out,
             const RateAxis* rates = nullptr)
{
    const size_t cap = (size_t)o.knot_capacity;
    const int64_t n_class = n_p * n_lambda;
    size_t freeb = 0, total = 0;
    (void)hipMemGetInfo(&freeb, &total);
    const size_t held = c->ws_beta[0] * batch_col_bytes(c->ws_cap[0]) + c->ec_rows * c->ec_ld * sizeof(double);
    const double budget = c->ec_budget > 0 ? (double)c->ec_budget : 0.4 * (double)(freeb + held);
    const double left = budget - (double)n_beta * (double)point_bytes(cap);
    int64_t per = left > 0.0 ? (int64_t)std::min(left / ((double)n_beta * (double)econ_class_bytes(cap)), 65535.0) : 1;
    per = std::max<int64_t>(1, std::min<int64_t>(per, n_class));
    int rc = ensure_learn(c, (size_t)n_beta, cap);
    if (rc) return rc;
    c->last_slot = 0;
    c->last_off = 0;
    c->rs_used = false;
    const sbr::LearnBufs& L = c->LW[0];
    // a workspace that already holds enough rows of this stride is used as it is
    for (;;) {
        rc = ensure_econ(c, (size_t)(per * n_beta), (size_t)L.cap);
        if (rc == SBR_OK) break;
        free_econ(c);
        if (per == 1) return rc;
        (void)hipGetLastError(); // the failed hipMalloc's error must not surface at the next launch check
        per = (per + 1) / 2;
    }
    // p and λ are per class: the hazard runs in hazard_econ_kernel, not in the learning launch
    sbr::LearnArgs la{x0, o.ode_reltol, o.ode_abstol, 0.0, 0.0, o.ode_maxiters, (int32_t)n_beta, stop_after_eta(o), 0};
    hipEvent_t t0 = tstart(c, s);
    HIP_TRY(c, sbr::launch_learn_kernel(beta, eta, t_end, la, L, s, 1), SBR_EDEVICE);
    tend(c, s, 0, t0);
    // (the interest slab stages HR too: its knot capacity is the three-array one, as in run_interest)
    sbr::EqArgs ea{0.0, (int32_t)(n_kappa * n_u), o.bisect_max_iters, rates ? c->lds_cap : c->lds_cap_b, nullptr,
                   (o.flags & SBR_FLAG_EXHAUSTIVE) ? 1 : 0, (o.flags >> 8) & 0x17};
    const sbr::InterestEconArgs ie{rates ? rates->r : nullptr, rates ? rates->delta : nullptr,
                                   (int32_t)(rates ? rates->n : 0), o.ode_reltol, o.ode_abstol, o.ode_maxiters,
                                   rates ? rates->steps : nullptr};
    t0 = tstart(c, s);
    int launches = 0;
    for (int64_t g0 = 0; g0 < n_class; g0 += per) {
        const int64_t ng = std::min<int64_t>(per, n_class - g0);
        const size_t rows = (size_t)(per * n_beta);
        const sbr::EconArgs e{p, lambda, kappa, (int32_t)n_p, (int32_t)n_lambda, (int32_t)n_kappa, (int32_t)n_u,
                              (int32_t)n_beta, (int32_t)g0, (int32_t)ng, c->ec_hr, c->ec_cnt, c->ec_cnt + rows,
                              (uint32_t*)(c->ec_cnt + 2 * rows)};
        HIP_TRY(c, sbr::launch_hazard_econ(beta, eta, la, L, e, s), SBR_EDEVICE);
        if (rates) HIP_TRY(c, sbr::launch_interest_econ(L, eta, t_end, u, ea, e, ie, out, s), SBR_EDEVICE);
        else HIP_TRY(c, sbr::launch_equilibrium_econ(L, eta, t_end, u, ea, e, out, s), SBR_EDEVICE);
        launches += 3;
    }
    tend(c, s, 1, t0, launches);
    return SBR_OK;
}

// the checks sbr_sweep_econ and sbr_sweep_econ_dev share, before any array is looked at
int econ_checks(sbr_ctx* c, const sbr_opts* opts, double x0, int64_t n_beta, int64_t n_u, int64_t n_p,
                int64_t n_lambda, int64_t n_kappa)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    if (!c) return SBR_EARG;
    const int64_t lim = 1 << 30;
    if (n_beta <= 0 || n_u <= 0 || n_p <= 0 || n_lambda <= 0 || n_kappa <= 0 || n_beta > lim || n_u > lim ||
        n_p > lim || n_lambda > lim || n_kappa > lim || n_p * n_lambda > lim || n_kappa * n_u > lim)
        return fail(c, SBR_EARG, "grid size");
    if (!(x0 >= 0.0)) return fail(c, SBR_EARG, "ArgumentError: x0");
    return SBR_OK;
}

int run_interest(sbr_ctx* c, hipStream_t s, const double* beta, const double* eta, const double* t_end, double x0,
                 const double* u, int64_t n_beta, int64_t n_u, double p, double kappa, double lambda, double r,
                 double delta, const sbr_opts& o, const sbr::ResultSoA& out, int64_t* steps, double* aw_path = nullptr,
                 double* v_path = nullptr, int32_t* v_count = nullptr)
{
    int rc = ensure_learn(c, (size_t)n_beta, (size_t)o.knot_capacity);
    if (rc) return rc;
    c->last_slot = 0;
    c->last_off = 0;
    sbr::LearnArgs la{x0, o.ode_reltol, o.ode_abstol, p, lambda, o.ode_maxiters, (int32_t)n_beta, stop_after_eta(o), 0};
    hipEvent_t t0 = tstart(c, s);
    HIP_TRY(c, sbr::launch_learn_logistic(beta, eta, t_end, la, c->LW[0], s), SBR_EDEVICE);
    tend(c, s, 0, t0);
    sbr::EqArgs ea{kappa, (int32_t)n_u, o.bisect_max_iters, c->lds_cap, aw_path,
                   (o.flags & SBR_FLAG_EXHAUSTIVE) ? 1 : 0, (o.flags >> 8) & 0x17};
    sbr::InterestArgs ia{r, delta, o.ode_reltol, o.ode_abstol, o.ode_maxiters, steps, v_path, v_count};
    t0 = tstart(c, s);
    HIP_TRY(c, sbr::launch_interest(c->LW[0], eta, t_end, u, ea, ia, out, (int)n_beta, s), SBR_EDEVICE);
    tend(c, s, 1, t0);
    return SBR_OK;
}

// EconomicParametersInterest / solve_value_function checks (interest_rate_model.jl:40-50,
// value_function_solver.jl:67-69)
bool interest_valid(double r, double delta) { return r >= 0.0 && delta > 0.0 && r < delta; }

}  // namespace

extern "C" {

int sbr_sweep_baseline_dev(sbr_ctx* c, void* stream, const double* beta, const double* eta, const double* t_end,
                           double x0, const double* u, int64_t n_beta, int64_t n_u, double p, double kappa,
                           double lambda, const sbr_opts* opts, sbr_result_soa* out)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    SBR_SINGLE_DEVICE(c);
    if (!c || !has_fields(out)) return SBR_EARG;
    if (n_beta <= 0 || n_u <= 0 || n_beta > (1 << 30) || n_u > (1 << 30)) return fail(c, SBR_EARG, "grid size");
    if (!scalars_valid(x0, p, kappa, lambda)) return fail(c, SBR_EARG, "ArgumentError: x0/p/kappa/lambda");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    sbr_opts o = resolve(opts);
    const sbr::ResultSoA r = device_soa(out);
    return fenced(c, stream, true, [&](hipStream_t s) {
        return run_baseline(c, s, beta, eta, t_end, x0, u, n_beta, n_u, p, kappa, lambda, o, r, nullptr);
    });
}

int sbr_sweep_baseline_batch_dev(sbr_ctx* c, void* stream, int64_t n_batch, const double* beta, const double* eta,
                                 const double* t_end, double x0, const double* u, int64_t n_beta, int64_t n_u,
                                 double p, double kappa, double lambda, const sbr_opts* opts, sbr_result_soa* out)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    SBR_SINGLE_DEVICE(c);
    if (!c || !out || !beta || !eta || !t_end || !u) return SBR_EARG;
    if (!has_fields(out)) return SBR_EARG;
    if (n_batch <= 0 || n_beta <= 0 || n_u <= 0 || n_beta > (1 << 30) || n_u > (1 << 30))
        return fail(c, SBR_EARG, "grid size");
    if (!scalars_valid(x0, p, kappa, lambda)) return fail(c, SBR_EARG, "ArgumentError: x0/p/kappa/lambda");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    sbr_opts o = resolve(opts);
    BatchPlan P;
    int rc = batch_alloc(c, n_batch, n_beta, (size_t)o.knot_capacity, P);
    if (rc) return rc;
    rc = ensure_pipe_streams(c);
    if (rc) return rc;
    const int64_t n_group = (n_batch + P.L - 1) / P.L;
    const int64_t n_eq_per_group = (P.L + P.E - 1) / P.E;
    while ((int64_t)c->ev_grid.size() < n_batch) {
        hipEvent_t e = nullptr;
        HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming), SBR_EDEVICE);
        c->ev_grid.push_back(e);
    }
    while ((int64_t)c->ev_hn.size() < n_group * n_eq_per_group) {
        hipEvent_t e = nullptr;
        HIP_TRY(c, hipEventCreateWithFlags(&e, kSyncEventFlags), SBR_EDEVICE);
        c->ev_hn.push_back(e);
    }
    c->n_grid = 0;
    return fenced(c, stream, true, [&](hipStream_t s) -> int {
        const size_t np = (size_t)n_beta * (size_t)n_u;
        // learning on lstream[0] (greatest priority), the hazard normalisations on lstream[1],
        // the equilibrium launches on the caller's stream
        hipStream_t ls = c->lstream[0], hs = c->lstream[1], es = s;
        HIP_TRY(c, hipEventRecord(c->ev_in, s), SBR_EDEVICE);
        HIP_TRY(c, hipStreamWaitEvent(ls, c->ev_in, 0), SBR_EDEVICE);
        int64_t k_hn = 0;
        for (int64_t m = 0; m < n_group; m++) {
            const int slot = (int)(m % P.nslot);
            const int64_t g0 = m * P.L, gn = (n_batch - g0) < P.L ? (n_batch - g0) : P.L;
            const sbr::LearnBufs& W = c->LW[slot];
            // the slot's previous readers (the equilibria of group m - nslot) must be done
            if (m >= P.nslot) HIP_TRY(c, hipStreamWaitEvent(ls, c->ev_eq[slot], 0), SBR_EDEVICE);
            // every grid of the group in ONE learning launch (the hazard numerators and running
            // integrals streamed with the knots, normalised by launch_hazard_norm): the launch
            // lasts as long as its slowest column whatever its width, so up to
            // SBR_BATCH_LEARN_WAVES waves learn together.  The first group has the chip to itself:
            // its rows leave through LDS as whole lines (mode 2).  Later groups run beside the
            // equilibrium launches and store directly (no LDS taken from the equilibrium slabs).
            const bool wide = m == 0;
            sbr::LearnArgs la{x0, o.ode_reltol, o.ode_abstol, p, lambda, o.ode_maxiters, (int32_t)(gn * n_beta),
                              stop_after_eta(o), 1};
            hipEvent_t t0 = tstart(c, ls);
            // (a narrow first group — under 256 waves, e.g. a strong-scaled shard — stores directly:
            // the staging's flush instructions cost more than the stores' contention there)
            const int lmode = !wide ? 0 : ((gn * n_beta + 63) / 64 >= 256 ? 2 : 1);
            // every grid's first wave dealt first (learn_logistic_kernel: the long columns of a
            // β-descending grid sit there; 20 grids 4.2-4.7 → 3.0-3.2 ms)
            if (lmode && n_beta % 64 == 0 && n_beta >= 128) {
                la.head = 1;
                la.wpg = (int32_t)(n_beta / 64);
            }
            // the staged heads-first launch normalises its tail waves' hazard rows itself; one small
            // hazard_norm_kernel launch takes the head waves' columns (no normalisation launches
            // beside the first equilibrium launch)
            const bool norm_in_learn = lmode == 2 && la.wpg;
            if (norm_in_learn) la.fuse_hazard = 2;
            HIP_TRY(c, sbr::launch_learn_kernel(beta + g0 * n_beta, eta + g0 * n_beta, t_end + g0 * n_beta, la, W, ls,
                                                lmode), SBR_EDEVICE);
            tend(c, ls, 0, t0);
            if (norm_in_learn) {
                sbr::LearnArgs lh = la;
                lh.part = 1;
                HIP_TRY(c, sbr::launch_hazard_norm(lh, W, (int)(gn * 64 * la.head), ls), SBR_EDEVICE);
            }
            HIP_TRY(c, hipEventRecord(c->ev_learned[slot], ls), SBR_EDEVICE);
            if (norm_in_learn) HIP_TRY(c, hipStreamWaitEvent(es, c->ev_learned[slot], 0), SBR_EDEVICE);
            else HIP_TRY(c, hipStreamWaitEvent(hs, c->ev_learned[slot], 0), SBR_EDEVICE);
            // the group's equilibria in launches of E grids (balanced).  Without the learning
            // kernel's own normalisation each launch follows a hazard_norm_kernel launch for its
            // columns on hs, run ahead and overlapped with the previous equilibrium launch — all of
            // them beside the first one, which they slowed from 2.28 to 2.71 ms (20 grids)
            const int64_t ne = (gn + P.E - 1) / P.E, Eg = (gn + ne - 1) / ne;
            // timing (sbr_timing_enable): one span over the group's equilibrium launches, from
            // the first one's start to the last one's end, counted as ne launches — two timing
            // events per launch between back-to-back launches cost ≈1 % of the step
            hipEvent_t te = nullptr;
            for (int64_t e0 = 0; e0 < gn; e0 += Eg) {
                const int64_t en = (gn - e0) < Eg ? (gn - e0) : Eg;
                const sbr::LearnBufs We = learn_rows(W, (size_t)(e0 * n_beta));
                const int64_t gg = g0 + e0;
                if (!norm_in_learn) {
                    HIP_TRY(c, sbr::launch_hazard_norm(la, We, (int)(en * n_beta), hs), SBR_EDEVICE);
                    hipEvent_t eh = c->ev_hn[(size_t)k_hn++];
                    HIP_TRY(c, hipEventRecord(eh, hs), SBR_EDEVICE);
                    HIP_TRY(c, hipStreamWaitEvent(es, eh, 0), SBR_EDEVICE);
                }
                if (e0 == 0) te = tstart(c, es);
                // column i·n_beta + j of the launch is grid g0+e0+i's column j: eta / t_end and
                // every out field are [n_batch × n_beta (× n_u)] contiguous
                sbr::ResultSoA r{out->xi + gg * np, out->tau_in_unc + gg * np, out->tau_out_unc + gg * np,
                                 out->aw_max + gg * np, out->tol + gg * np, out->status + gg * np,
                                 out->iters ? out->iters + gg * np : nullptr};
                rc = launch_eq(c, es, We, eta + gg * n_beta, t_end + gg * n_beta, u, en * n_beta, n_u, kappa, o, r,
                               nullptr, (int)en, false);
                if (rc) return rc;
                for (int64_t i = 0; i < en; i++) HIP_TRY(c, hipEventRecord(c->ev_grid[gg + i], es), SBR_EDEVICE);
                c->n_grid = gg + en;
            }
            tend(c, es, 1, te, (int)ne);
            HIP_TRY(c, hipEventRecord(c->ev_eq[slot], es), SBR_EDEVICE);
            c->last_slot = slot;
            c->last_off = (gn - 1) * n_beta;
        }
        return SBR_OK;
    });
}

int sbr_batch_reserve(sbr_ctx* c, int64_t n_batch, int64_t n_beta, const sbr_opts* opts)
{
    SBR_SINGLE_DEVICE(c);
    if (!c) return SBR_EARG;
    if (n_batch <= 0 || n_beta <= 0 || n_beta > (1 << 30)) return fail(c, SBR_EARG, "grid size");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    const sbr_opts o = resolve(opts);
    // the workspaces are replaced only once nothing enqueued earlier can still read them
    if (c->have_last) HIP_TRY(c, hipEventSynchronize(c->ev_last), SBR_EDEVICE);
    BatchPlan P;
    return batch_alloc(c, n_batch, n_beta, (size_t)o.knot_capacity, P);
}

int sbr_set_batch_workspace(sbr_ctx* c, int64_t bytes)
{
    SBR_SINGLE_DEVICE(c);
    if (!c || bytes < 0) return SBR_EARG;
    c->bt_budget = bytes;
    return SBR_OK;
}

int sbr_batch_wait(sbr_ctx* c, void* stream, int64_t k)
{
    SBR_SINGLE_DEVICE(c);
    if (!c) return SBR_EARG;
    if (k < 0 || k >= c->n_grid) return fail(c, SBR_EARG, "sbr_batch_wait: no such grid in the last batch");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    HIP_TRY(c, hipStreamWaitEvent((hipStream_t)stream, c->ev_grid[k], 0), SBR_EDEVICE);
    return SBR_OK;
}

static int multi_sweep_baseline(sbr_ctx* c, const Inputs& in, double x0, int64_t n_beta, int64_t n_u, double p,
                                double kappa, double lambda, const sbr_opts& o, sbr_result_soa* out)
{
    auto run = [&](sbr_ctx* kid, hipStream_t s, int64_t nc, const DevInputs& d, const std::vector<void*>& f) -> int {
        sbr_result_soa ro = rank_results(f);
        return sbr_sweep_baseline_dev(kid, s, d[0], d[1], d[2], x0, d[3], nc, n_u, p, kappa, lambda, &o, &ro);
    };
    const int rc = fan_out(c, in, n_beta, n_u, result_fields(out), o, run);
    if (rc == SBR_OK) early_exit(o, n_beta, n_u, out);
    return rc;
}

int sbr_sweep_baseline(sbr_ctx* c, const double* beta, const double* eta, const double* t_end, double x0,
                       const double* u, int64_t n_beta, int64_t n_u, double p, double kappa, double lambda,
                       const sbr_opts* opts, sbr_result_soa* out)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    if (!c || !out || !beta || !eta || !t_end || !u) return SBR_EARG;
    if (n_beta <= 0 || n_u <= 0) return fail(c, SBR_EARG, "grid size");
    if (!scalars_valid(x0, p, kappa, lambda)) return fail(c, SBR_EARG, "ArgumentError: x0/p/kappa/lambda");
    int rc = check_positive(c, n_beta, {beta, t_end, eta}, "ArgumentError: beta/eta/t_end must be positive");
    if (!rc) rc = check_u(c, u, n_u);
    if (rc) return rc;
    const Inputs in{cols(beta), cols(eta), cols(t_end), shared(u, (size_t)n_u)};
    if (c->multi) return multi_sweep_baseline(c, in, x0, n_beta, n_u, p, kappa, lambda, resolve(opts), out);
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    sbr_opts o = resolve(opts);
    const size_t np = (size_t)n_beta * (size_t)n_u;
    void* dres;
    rc = ensure_io(c, in, (size_t)n_beta, result_bytes(np), &dres);
    if (!rc) rc = ensure_res_pin(c, result_bytes(np));
    if (rc) return rc;
    const auto d = in.dev(c->stage, (size_t)n_beta);
    const sbr::ResultSoA r = carve_results(dres, np);
    const auto h0 = std::chrono::steady_clock::now();
    hipEvent_t pe[4] = {};
    return fenced(c, nullptr, false, [&](hipStream_t s) -> int {
        if (c->timing)
            for (hipEvent_t& e : pe) e = next_event(c);
        auto mark = [&](int k) { if (pe[k]) (void)hipEventRecord(pe[k], s); };
        mark(0);
        rc = in.stage(c, c->stage, (size_t)n_beta, s);
        if (rc) return rc;
        mark(1);
        rc = run_baseline(c, s, d[0], d[1], d[2], x0, d[3], n_beta, n_u, p, kappa, lambda, o, r, nullptr);
        if (rc) return rc;
        mark(2);
        int32_t gave_up = 0;
        if (c->rs_used) HIP_TRY(c, hipMemcpyAsync(&gave_up, c->rq + 1, 4, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        rc = readback_enqueue(c, dres, np, out->iters != nullptr, s);
        if (rc) return rc;
        mark(3);
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        if (gave_up) return fail(c, SBR_EDEVICE, "readiness schedule: an equilibrium workgroup timed out");
        const auto h1 = std::chrono::steady_clock::now();
        scatter_results(c->res_pin, np, out);
        early_exit(o, n_beta, n_u, out);
        if (pe[3]) {
            float a = 0.f;
            for (int k = 0; k < 3; k++)
                c->ph_ms[k] = hipEventElapsedTime(&a, pe[k], pe[k + 1]) == hipSuccess ? (double)a : -1.0;
            const auto h2 = std::chrono::steady_clock::now();
            c->ph_ms[3] = std::chrono::duration<double, std::milli>(h2 - h1).count();
            c->ph_ms[4] = std::chrono::duration<double, std::milli>(h2 - h0).count();
        }
        return SBR_OK;
    });
}

// the checks sbr_solve_points and sbr_solve_points_dev share, before any array is looked at;
// *done: nothing to do (n == 0)
static int points_checks(sbr_ctx* c, const sbr_opts* opts, double x0, int64_t n, bool* done)
{
    *done = false;
    if (int rc = refuse_guess(c, opts)) return rc;
    if (!c) return SBR_EARG;
    if (n < 0 || n > (1 << 30)) return fail(c, SBR_EARG, "list size");
    if (!(x0 >= 0.0)) return fail(c, SBR_EARG, "ArgumentError: x0");
    *done = n == 0;
    return SBR_OK;
}

int sbr_solve_points_dev(sbr_ctx* c, void* stream, const double* beta, const double* eta, const double* t_end,
                         double x0, const double* u, const double* p, const double* kappa, const double* lambda,
                         int64_t n, const sbr_opts* opts, sbr_result_soa* out)
{
    bool done;
    int rc = points_checks(c, opts, x0, n, &done);
    if (rc) return rc;
    SBR_SINGLE_DEVICE(c);
    if (done) return SBR_OK;
    if (!beta || !eta || !t_end || !u || !p || !kappa || !lambda || !has_fields(out))
        return fail(c, SBR_EARG, "null array");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    const sbr_opts o = resolve(opts);
    const sbr::ResultSoA r = device_soa(out);
    return fenced(c, stream, true, [&](hipStream_t s) {
        return run_points(c, s, beta, eta, t_end, x0, u, p, kappa, lambda, n, o, r);
    });
}

// a list of models on n devices: point i to rank i mod N (the columns of an n × 1 grid)
static int multi_solve_points(sbr_ctx* c, const Inputs& in, double x0, int64_t n, const sbr_opts& o,
                              sbr_result_soa* out)
{
    auto run = [&](sbr_ctx* kid, hipStream_t s, int64_t nc, const DevInputs& d, const std::vector<void*>& f) -> int {
        sbr_result_soa ro = rank_results(f);
        return sbr_solve_points_dev(kid, s, d[0], d[1], d[2], x0, d[3], d[4], d[5], d[6], nc, &o, &ro);
    };
    return fan_out(c, in, n, 1, result_fields(out), o, run);
}

int sbr_solve_points(sbr_ctx* c, const double* beta, const double* eta, const double* t_end, double x0,
                     const double* u, const double* p, const double* kappa, const double* lambda, int64_t n,
                     const sbr_opts* opts, sbr_result_soa* out)
{
    bool done;
    int rc = points_checks(c, opts, x0, n, &done);
    if (rc || done) return rc;
    if (!beta || !eta || !t_end || !u || !p || !kappa || !lambda || !out) return fail(c, SBR_EARG, "null array");
    // per-point ArgumentErrors are per-point results (SBR_ARG_INVALID), found on the device
    const Inputs in{cols(beta), cols(eta), cols(t_end), cols(u), cols(p), cols(kappa), cols(lambda)};
    if (c->multi) return multi_solve_points(c, in, x0, n, resolve(opts), out);
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    const sbr_opts o = resolve(opts);
    const size_t np = (size_t)n;
    void* dres;
    rc = ensure_io(c, in, np, result_bytes(np), &dres);
    if (!rc) rc = ensure_res_pin(c, result_bytes(np));
    if (rc) return rc;
    const auto d = in.dev(c->stage, np);
    const sbr::ResultSoA r = carve_results(dres, np);
    return fenced(c, nullptr, false, [&](hipStream_t s) -> int {
        rc = in.stage(c, c->stage, np, s);
        if (!rc) rc = run_points(c, s, d[0], d[1], d[2], x0, d[3], d[4], d[5], d[6], n, o, r);
        if (!rc) rc = readback_enqueue(c, dres, np, out->iters != nullptr, s);
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        scatter_results(c->res_pin, np, out);
        return SBR_OK;
    });
}

int sbr_set_points_workspace(sbr_ctx* c, int64_t bytes)
{
    if (!c || bytes < 0) return SBR_EARG;
    for (int r = 0; c->multi && r < sbr_multi_size(c); r++) sbr_multi_child(c, r)->pt_budget = bytes; // every rank's own
    c->pt_budget = bytes;
    return SBR_OK;
}

int sbr_sweep_econ_dev(sbr_ctx* c, void* stream, const double* beta, const double* eta, const double* t_end,
                       double x0, const double* u, int64_t n_beta, int64_t n_u, const double* p, int64_t n_p,
                       const double* lambda, int64_t n_lambda, const double* kappa, int64_t n_kappa,
                       const sbr_opts* opts, sbr_result_soa* out)
{
    int rc = econ_checks(c, opts, x0, n_beta, n_u, n_p, n_lambda, n_kappa);
    if (rc) return rc;
    SBR_SINGLE_DEVICE(c);
    if (!beta || !eta || !t_end || !u || !p || !lambda || !kappa || !has_fields(out))
        return fail(c, SBR_EARG, "null array");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    const sbr_opts o = resolve(opts);
    const sbr::ResultSoA r = device_soa(out);
    return fenced(c, stream, true, [&](hipStream_t s) {
        return run_econ(c, s, beta, eta, t_end, x0, u, n_beta, n_u, p, n_p, lambda, n_lambda, kappa, n_kappa, o, r);
    });
}

// β × p × λ × κ × u on n devices: column i to rank i mod N with its n_p·n_lambda·n_kappa·n_u
// points, the four axes to every rank
static int multi_sweep_econ(sbr_ctx* c, const Inputs& in, double x0, int64_t n_beta, int64_t n_u, int64_t n_p,
                            int64_t n_lambda, int64_t n_kappa, const sbr_opts& o, sbr_result_soa* out)
{
    auto run = [&](sbr_ctx* kid, hipStream_t s, int64_t nc, const DevInputs& d, const std::vector<void*>& f) -> int {
        sbr_result_soa ro = rank_results(f);
        return sbr_sweep_econ_dev(kid, s, d[0], d[1], d[2], x0, d[3], nc, n_u, d[4], n_p, d[5], n_lambda, d[6],
                                  n_kappa, &o, &ro);
    };
    const int rc = fan_out(c, in, n_beta, n_p * n_lambda * n_kappa * n_u, result_fields(out), o, run);
    if (rc == SBR_OK) early_exit(o, n_beta * n_p * n_lambda * n_kappa, n_u, out);
    return rc;
}

int sbr_sweep_econ(sbr_ctx* c, const double* beta, const double* eta, const double* t_end, double x0,
                   const double* u, int64_t n_beta, int64_t n_u, const double* p, int64_t n_p, const double* lambda,
                   int64_t n_lambda, const double* kappa, int64_t n_kappa, const sbr_opts* opts, sbr_result_soa* out)
{
    int rc = econ_checks(c, opts, x0, n_beta, n_u, n_p, n_lambda, n_kappa);
    if (rc) return rc;
    if (!beta || !eta || !t_end || !u || !p || !lambda || !kappa || !out) return fail(c, SBR_EARG, "null array");
    rc = check_positive(c, n_beta, {beta, t_end, eta}, "ArgumentError: beta/eta/t_end must be positive");
    if (!rc) rc = check_u(c, u, n_u);
    if (rc) return rc;
    for (int64_t a = 0; a < n_p; a++)
        if (!(p[a] >= 0.0 && p[a] <= 1.0)) return fail(c, SBR_EARG, "ArgumentError: p must be in [0, 1]");
    rc = check_positive(c, n_lambda, {lambda}, "ArgumentError: lambda must be positive");
    if (rc) return rc;
    for (int64_t k = 0; k < n_kappa; k++)
        if (!(kappa[k] > 0.0 && kappa[k] < 1.0)) return fail(c, SBR_EARG, "ArgumentError: kappa must be in (0, 1)");
    const sbr_opts o = resolve(opts);
    const int64_t n_line = n_beta * n_p * n_lambda * n_kappa;
    const Inputs in{cols(beta), cols(eta), cols(t_end), shared(u, (size_t)n_u), shared(p, (size_t)n_p),
                    shared(lambda, (size_t)n_lambda), shared(kappa, (size_t)n_kappa)};
    if (c->multi) return multi_sweep_econ(c, in, x0, n_beta, n_u, n_p, n_lambda, n_kappa, o, out);
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    const size_t np = (size_t)n_line * (size_t)n_u;
    void* dres;
    rc = ensure_io(c, in, (size_t)n_beta, result_bytes(np), &dres);
    if (!rc) rc = ensure_res_pin(c, result_bytes(np));
    if (rc) return rc;
    const auto d = in.dev(c->stage, (size_t)n_beta);
    const sbr::ResultSoA r = carve_results(dres, np);
    return fenced(c, nullptr, false, [&](hipStream_t s) -> int {
        rc = in.stage(c, c->stage, (size_t)n_beta, s);
        if (!rc) rc = run_econ(c, s, d[0], d[1], d[2], x0, d[3], n_beta, n_u, d[4], n_p, d[5], n_lambda, d[6], n_kappa, o, r);
        if (!rc) rc = readback_enqueue(c, dres, np, out->iters != nullptr, s);
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        scatter_results(c->res_pin, np, out);
        early_exit(o, n_line, n_u, out);
        return SBR_OK;
    });
}

int sbr_set_econ_workspace(sbr_ctx* c, int64_t bytes)
{
    if (!c || bytes < 0) return SBR_EARG;
    for (int r = 0; c->multi && r < sbr_multi_size(c); r++) sbr_multi_child(c, r)->ec_budget = bytes; // every rank's own
    c->ec_budget = bytes;
    return SBR_OK;
}

int sbr_sweep_interest_dev(sbr_ctx* c, void* stream, const double* beta, const double* eta, const double* t_end,
                           double x0, const double* u, int64_t n_beta, int64_t n_u, double p, double kappa,
                           double lambda, double r, double delta, const sbr_opts* opts, sbr_result_soa* out,
                           int64_t* rk_steps)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    SBR_SINGLE_DEVICE(c);
    if (!c || !has_fields(out)) return SBR_EARG;
    if (n_beta <= 0 || n_u <= 0 || n_beta > (1 << 30) || n_u > (1 << 30)) return fail(c, SBR_EARG, "grid size");
    if (!scalars_valid(x0, p, kappa, lambda)) return fail(c, SBR_EARG, "ArgumentError: x0/p/kappa/lambda");
    if (!interest_valid(r, delta)) return fail(c, SBR_EARG, "ArgumentError: need 0 <= r < delta");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    sbr_opts o = resolve(opts);
    const sbr::ResultSoA rs = device_soa(out);
    return fenced(c, stream, true, [&](hipStream_t s) {
        return run_interest(c, s, beta, eta, t_end, x0, u, n_beta, n_u, p, kappa, lambda, r, delta, o, rs, rk_steps);
    });
}

static int multi_sweep_interest(sbr_ctx* c, const Inputs& in, double x0, int64_t n_beta, int64_t n_u, double p,
                                double kappa, double lambda, double r, double delta, const sbr_opts& o,
                                sbr_result_soa* out, int64_t* rk_steps)
{
    std::vector<FieldSpec> fs = result_fields(out);
    fs.push_back({rk_steps, 8, 1});
    auto run = [&](sbr_ctx* kid, hipStream_t s, int64_t nc, const DevInputs& d, const std::vector<void*>& f) -> int {
        sbr_result_soa ro = rank_results(f);
        return sbr_sweep_interest_dev(kid, s, d[0], d[1], d[2], x0, d[3], nc, n_u, p, kappa, lambda, r, delta, &o,
                                      &ro, (int64_t*)f[7]);
    };
    return fan_out(c, in, n_beta, n_u, fs, o, run);
}

int sbr_sweep_interest(sbr_ctx* c, const double* beta, const double* eta, const double* t_end, double x0,
                       const double* u, int64_t n_beta, int64_t n_u, double p, double kappa, double lambda, double r,
                       double delta, const sbr_opts* opts, sbr_result_soa* out, int64_t* rk_steps)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    if (!c || !out || !beta || !eta || !t_end || !u) return SBR_EARG;
    if (n_beta <= 0 || n_u <= 0) return fail(c, SBR_EARG, "grid size");
    if (!scalars_valid(x0, p, kappa, lambda)) return fail(c, SBR_EARG, "ArgumentError: x0/p/kappa/lambda");
    if (!interest_valid(r, delta)) return fail(c, SBR_EARG, "ArgumentError: need 0 <= r < delta");
    int rc = check_positive(c, n_beta, {beta, t_end, eta}, "ArgumentError: beta/eta/t_end must be positive");
    if (!rc) rc = check_u(c, u, n_u);
    if (rc) return rc;
    const Inputs in{cols(beta), cols(eta), cols(t_end), shared(u, (size_t)n_u)};
    if (c->multi)
        return multi_sweep_interest(c, in, x0, n_beta, n_u, p, kappa, lambda, r, delta, resolve(opts), out, rk_steps);
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    sbr_opts o = resolve(opts);
    const size_t np = (size_t)n_beta * (size_t)n_u;
    void* dres;
    rc = ensure_io(c, in, (size_t)n_beta, result_bytes(np, true), &dres);
    if (rc) return rc;
    const auto d = in.dev(c->stage, (size_t)n_beta);
    int64_t* dsteps;
    const sbr::ResultSoA rs = carve_results(dres, np, &dsteps);
    return fenced(c, nullptr, false, [&](hipStream_t s) -> int {
        rc = in.stage(c, c->stage, (size_t)n_beta, s);
        if (!rc) rc = run_interest(c, s, d[0], d[1], d[2], x0, d[3], n_beta, n_u, p, kappa, lambda, r, delta, o, rs, dsteps);
        if (!rc) rc = copy_out(c, s, out, rs, np);
        if (!rc) rc = copy_out(c, s, {{rk_steps, dsteps, np * 8}});
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        return SBR_OK;
    });
}

// the checks sbr_sweep_interest_econ and sbr_sweep_interest_econ_dev share, before any array is looked at
static int interest_econ_checks(sbr_ctx* c, const sbr_opts* opts, double x0, int64_t n_beta, int64_t n_u,
                                int64_t n_p, int64_t n_lambda, int64_t n_rate, int64_t n_kappa)
{
    if (int rc = econ_checks(c, opts, x0, n_beta, n_u, n_p, n_lambda, n_kappa)) return rc;
    const int64_t lim = 1 << 30;
    if (n_rate <= 0 || n_rate > lim || n_rate * n_u > lim) return fail(c, SBR_EARG, "grid size");
    // at most 2^40 results in all, so that no index of the call can wrap: each factor is within 2^30,
    // and the quotients keep every intermediate product below 2^61
    const int64_t total = (int64_t)1 << 40, plane = n_rate * n_u, per_col = n_p * n_lambda;
    if (plane > total / n_kappa || per_col > total / (plane * n_kappa) || n_beta > total / (plane * n_kappa * per_col))
        return fail(c, SBR_EARG, "grid size: more than 2^40 points");
    return SBR_OK;
}

// one device's launch takes a column per grid row (launch_hazard_econ, launch_interest_econ)
static int interest_econ_cols(sbr_ctx* c, int64_t n_beta)
{
    return n_beta > 65535 ? fail(c, SBR_EARG, "grid size: more than 65,535 columns on one device") : SBR_OK;
}

int sbr_sweep_interest_econ_dev(sbr_ctx* c, void* stream, const double* beta, const double* eta, const double* t_end,
                                double x0, const double* u, int64_t n_beta, int64_t n_u, const double* p,
                                int64_t n_p, const double* lambda, int64_t n_lambda, const double* r,
                                const double* delta, int64_t n_rate, const double* kappa, int64_t n_kappa,
                                const sbr_opts* opts, sbr_result_soa* out, int64_t* rk_steps)
{
    int rc = interest_econ_checks(c, opts, x0, n_beta, n_u, n_p, n_lambda, n_rate, n_kappa);
    if (rc) return rc;
    SBR_SINGLE_DEVICE(c);
    if ((rc = interest_econ_cols(c, n_beta))) return rc;
    if (!beta || !eta || !t_end || !u || !p || !lambda || !r || !delta || !kappa || !has_fields(out))
        return fail(c, SBR_EARG, "null array");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    const sbr_opts o = resolve(opts);
    const sbr::ResultSoA rs = device_soa(out);
    const RateAxis rates{r, delta, n_rate, rk_steps};
    return fenced(c, stream, true, [&](hipStream_t s) {
        return run_econ(c, s, beta, eta, t_end, x0, u, n_beta, n_u, p, n_p, lambda, n_lambda, kappa, n_kappa, o, rs,
                        &rates);
    });
}

// β × p × λ × (r, δ) × κ × u on n devices: column i to rank i mod N with its n_p·n_lambda·n_rate·n_u
// shard points of n_kappa results and one step count each, the five axes to every rank
static int multi_sweep_interest_econ(sbr_ctx* c, const Inputs& in, double x0, int64_t n_beta, int64_t n_u,
                                     int64_t n_p, int64_t n_lambda, int64_t n_rate, int64_t n_kappa,
                                     const sbr_opts& o, sbr_result_soa* out, int64_t* rk_steps)
{
    std::vector<FieldSpec> fs = result_fields(out);
    for (FieldSpec& f : fs) f.per_pt = (size_t)n_kappa;
    fs.push_back({rk_steps, 8, 1});
    auto run = [&](sbr_ctx* kid, hipStream_t s, int64_t nc, const DevInputs& d, const std::vector<void*>& f) -> int {
        sbr_result_soa ro = rank_results(f);
        return sbr_sweep_interest_econ_dev(kid, s, d[0], d[1], d[2], x0, d[3], nc, n_u, d[4], n_p, d[5], n_lambda,
                                           d[6], d[7], n_rate, d[8], n_kappa, &o, &ro, (int64_t*)f[7]);
    };
    return fan_out(c, in, n_beta, n_p * n_lambda * n_rate * n_u, fs, o, run);
}

int sbr_sweep_interest_econ(sbr_ctx* c, const double* beta, const double* eta, const double* t_end, double x0,
                            const double* u, int64_t n_beta, int64_t n_u, const double* p, int64_t n_p,
                            const double* lambda, int64_t n_lambda, const double* r, const double* delta,
                            int64_t n_rate, const double* kappa, int64_t n_kappa, const sbr_opts* opts,
                            sbr_result_soa* out, int64_t* rk_steps)
{
    int rc = interest_econ_checks(c, opts, x0, n_beta, n_u, n_p, n_lambda, n_rate, n_kappa);
    if (rc) return rc;
    if (!beta || !eta || !t_end || !u || !p || !lambda || !r || !delta || !kappa || !out)
        return fail(c, SBR_EARG, "null array");
    rc = check_positive(c, n_beta, {beta, t_end, eta}, "ArgumentError: beta/eta/t_end must be positive");
    if (!rc) rc = check_u(c, u, n_u);
    if (rc) return rc;
    for (int64_t a = 0; a < n_p; a++)
        if (!(p[a] >= 0.0 && p[a] <= 1.0)) return fail(c, SBR_EARG, "ArgumentError: p must be in [0, 1]");
    rc = check_positive(c, n_lambda, {lambda}, "ArgumentError: lambda must be positive");
    if (rc) return rc;
    for (int64_t d = 0; d < n_rate; d++)
        if (!interest_valid(r[d], delta[d])) return fail(c, SBR_EARG, "ArgumentError: need 0 <= r < delta");
    for (int64_t k = 0; k < n_kappa; k++)
        if (!(kappa[k] > 0.0 && kappa[k] < 1.0)) return fail(c, SBR_EARG, "ArgumentError: kappa must be in (0, 1)");
    const sbr_opts o = resolve(opts);
    const Inputs in{cols(beta), cols(eta), cols(t_end), shared(u, (size_t)n_u), shared(p, (size_t)n_p),
                    shared(lambda, (size_t)n_lambda), shared(r, (size_t)n_rate), shared(delta, (size_t)n_rate),
                    shared(kappa, (size_t)n_kappa)};
    if (c->multi)
        return multi_sweep_interest_econ(c, in, x0, n_beta, n_u, n_p, n_lambda, n_rate, n_kappa, o, out, rk_steps);
    if ((rc = interest_econ_cols(c, n_beta))) return rc;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    // the result block of np points, then the step counts, one per value function
    const size_t ns = (size_t)(n_beta * n_p * n_lambda * n_rate) * (size_t)n_u, np = ns * (size_t)n_kappa;
    void* dres;
    rc = ensure_io(c, in, (size_t)n_beta, result_bytes(np) + ns * 8, &dres);
    if (!rc) rc = ensure_res_pin(c, result_bytes(np));
    if (rc) return rc;
    const auto d = in.dev(c->stage, (size_t)n_beta);
    const sbr::ResultSoA rs = carve_results(dres, np);
    int64_t* dsteps = (int64_t*)((char*)dres + result_bytes(np));
    const RateAxis rates{d[6], d[7], n_rate, dsteps};
    return fenced(c, nullptr, false, [&](hipStream_t s) -> int {
        rc = in.stage(c, c->stage, (size_t)n_beta, s);
        if (!rc) rc = run_econ(c, s, d[0], d[1], d[2], x0, d[3], n_beta, n_u, d[4], n_p, d[5], n_lambda, d[8], n_kappa, o, rs, &rates);
        if (!rc) rc = readback_enqueue(c, dres, np, out->iters != nullptr, s);
        if (rc) return rc;
        // the step counts reach the caller only after the sweep itself has succeeded
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        if (rk_steps) HIP_TRY(c, hipMemcpy(rk_steps, dsteps, ns * 8, hipMemcpyDeviceToHost), SBR_EDEVICE);
        scatter_results(c->res_pin, np, out);
        return SBR_OK;
    });
}

// One point with its paths.  rd = nullptr: sbr_solve_point_paths; rd = {r, delta}: the interest-rate
// model's point, with the value function's path V (n_v values; none at r = 0).
// Stage: [β, η, t_end, u | xi … tol | status | n_v | AW_cum path (kc) | V path (kc)]
static int point_paths(sbr_ctx* c, double beta, double eta, double t_end, double x0, double u, double p, double kappa,
                       double lambda, const double* rd, const sbr_opts* opts, double* res, uint32_t* status,
                       double* tau, double* hr, double* V, double* aw_cum, int64_t cap, int64_t* n_tau, int64_t* n_v)
{
    if (!c || !res || !status) return SBR_EARG;
    if (!scalars_valid(x0, p, kappa, lambda) || !(beta > 0) || !(eta > 0) || !(t_end > 0) || !(u >= 0))
        return fail(c, SBR_EARG, "ArgumentError");
    if (rd && !interest_valid(rd[0], rd[1])) return fail(c, SBR_EARG, "ArgumentError: need 0 <= r < delta");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    sbr_opts o = resolve(opts);
    const size_t kc = (size_t)o.knot_capacity;
    int rc = ensure_stage(c, (4 + 5 + 1 + 1 + 2 * kc) * 8 + 512);
    if (rc) return rc;
    double* d = (double*)c->stage;
    double hin[4] = {beta, eta, t_end, u};
    return fenced(c, nullptr, false, [&](hipStream_t s) -> int {
        HIP_TRY(c, hipMemcpyAsync(d, hin, 32, hipMemcpyHostToDevice, s), SBR_EDEVICE);
        double* dres = d + 4;
        uint32_t* dst = (uint32_t*)(dres + 5);
        int32_t* dnv = (int32_t*)(dres + 6);
        double* dpath = dres + 7;
        double* dv = dpath + kc;
        sbr::ResultSoA rs{dres, dres + 1, dres + 2, dres + 3, dres + 4, dst, nullptr};
        if (rd) {
            HIP_TRY(c, hipMemsetAsync(dnv, 0, 4, s), SBR_EDEVICE);
            rc = run_interest(c, s, d, d + 1, d + 2, x0, d + 3, 1, 1, p, kappa, lambda, rd[0], rd[1], o, rs, nullptr,
                              dpath, rd[0] > 0.0 ? dv : nullptr, dnv);
        } else {
            rc = run_baseline(c, s, d, d + 1, d + 2, x0, d + 3, 1, 1, p, kappa, lambda, o, rs, dpath);
        }
        if (rc) return rc;
        int32_t nt = 0, nle = 0, nv = 0;
        rc = copy_out(c, s, {{res, dres, 40}, {status, dst, 4}, {&nt, c->LW[0].n_tau, 4}, {&nle, c->LW[0].n_le, 4},
                             {rd ? &nv : nullptr, dnv, 4}});
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        if (!rd || rd[0] <= 0.0) nv = 0;
        if (n_tau) *n_tau = nt;
        if (n_v) *n_v = nv;
        if (nt > cap) return fail(c, SBR_EARG, "path capacity too small");
        if (tau) {
            HIP_TRY(c, hipMemcpy(tau, c->LW[0].t, (size_t)nle * 8, hipMemcpyDeviceToHost), SBR_EDEVICE);
            if (nt > nle) tau[nle] = eta;
        }
        if (hr) HIP_TRY(c, hipMemcpy(hr, c->LW[0].hr, (size_t)nt * 8, hipMemcpyDeviceToHost), SBR_EDEVICE);
        if (V && nv > 0) HIP_TRY(c, hipMemcpy(V, dv, (size_t)nv * 8, hipMemcpyDeviceToHost), SBR_EDEVICE);
        if (aw_cum) {
            if (*status & SBR_RUN) HIP_TRY(c, hipMemcpy(aw_cum, dpath, (size_t)nt * 8, hipMemcpyDeviceToHost), SBR_EDEVICE);
            else for (int i = 0; i < nt; i++) aw_cum[i] = NAN;
        }
        return SBR_OK;
    });
}

int sbr_solve_point_paths(sbr_ctx* c, double beta, double eta, double t_end, double x0, double u, double p,
                          double kappa, double lambda, const sbr_opts* opts, double* res, uint32_t* status,
                          double* tau, double* hr, double* aw_cum, int64_t cap, int64_t* n_tau)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    SBR_ON_RANK0(c, sbr_solve_point_paths(c, beta, eta, t_end, x0, u, p, kappa, lambda, opts, res, status, tau, hr, aw_cum, cap, n_tau));
    return point_paths(c, beta, eta, t_end, x0, u, p, kappa, lambda, nullptr, opts, res, status, tau, hr, nullptr, aw_cum,
                       cap, n_tau, nullptr);
}

int sbr_interest_point_paths(sbr_ctx* c, double beta, double eta, double t_end, double x0, double u, double p,
                             double kappa, double lambda, double r, double delta, const sbr_opts* opts, double* res,
                             uint32_t* status, double* tau, double* hr, double* V, double* aw_cum, int64_t cap,
                             int64_t* n_tau, int64_t* n_v)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    SBR_ON_RANK0(c, sbr_interest_point_paths(c, beta, eta, t_end, x0, u, p, kappa, lambda, r, delta, opts, res, status, tau, hr, V, aw_cum, cap, n_tau, n_v));
    const double rd[2] = {r, delta};
    return point_paths(c, beta, eta, t_end, x0, u, p, kappa, lambda, rd, opts, res, status, tau, hr, V, aw_cum, cap, n_tau,
                       n_v);
}

int sbr_learn_baseline(sbr_ctx* c, const double* beta, const double* eta, const double* t_end, double x0,
                       int64_t n_beta, int32_t stop_after_eta, const sbr_opts* opts, double* t_out, double* G_out,
                       int64_t cap, int32_t* n_knots, uint32_t* status)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    SBR_ON_RANK0(c, sbr_learn_baseline(c, beta, eta, t_end, x0, n_beta, stop_after_eta, opts, t_out, G_out, cap, n_knots, status));
    if (!c || !beta || !eta || !t_end || n_beta <= 0 || cap <= 0) return SBR_EARG;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    sbr_opts o = resolve(opts);
    if (cap < o.knot_capacity) o.knot_capacity = (int32_t)cap;
    int rc = ensure_learn(c, (size_t)n_beta, (size_t)o.knot_capacity);
    if (rc) return rc;
    const Inputs in{cols(beta), cols(eta), cols(t_end)};
    rc = ensure_stage(c, in.bytes((size_t)n_beta));
    if (rc) return rc;
    const auto d = in.dev(c->stage, (size_t)n_beta);
    return fenced(c, nullptr, false, [&](hipStream_t s) -> int {
        rc = in.stage(c, c->stage, (size_t)n_beta, s);
        if (rc) return rc;
        sbr::LearnArgs la{x0, o.ode_reltol, o.ode_abstol, 0.5, 1.0, o.ode_maxiters, (int32_t)n_beta, stop_after_eta, 0};
        HIP_TRY(c, sbr::launch_learn_logistic(d[0], d[1], d[2], la, c->LW[0], s), SBR_EDEVICE);
        const size_t w = (size_t)o.knot_capacity, ld = (size_t)c->LW[0].cap;
        if (t_out)
            HIP_TRY(c, hipMemcpy2DAsync(t_out, cap * 8, c->LW[0].t, ld * 8, w * 8, n_beta, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        if (G_out)
            HIP_TRY(c, hipMemcpy2DAsync(G_out, cap * 8, c->LW[0].G, ld * 8, w * 8, n_beta, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        if (n_knots) HIP_TRY(c, hipMemcpyAsync(n_knots, c->LW[0].n_knots, n_beta * 4, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        if (status) HIP_TRY(c, hipMemcpyAsync(status, c->LW[0].status, n_beta * 4, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        strip_hazard_status(status, n_beta);
        return SBR_OK;
    });
}

}  // extern "C"
