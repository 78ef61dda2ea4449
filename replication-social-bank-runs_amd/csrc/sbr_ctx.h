// sbr_ctx.h — the context behind the opaque sbr_ctx of include/sbr.h and what every file of the
// C API (sbr_capi*.hip) shares: error reporting, the call fence, option defaults, argument checks
// and the workspaces' ensure_* / free_* functions.  Private to csrc/: not installed.
#pragma once

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <initializer_list>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sbr.h"
#include "../../include/sbr_detmath.h"
#include "sbr_kernels.h"
#include "sbr_multi.h"
#include "sbr_social_plan.h"

// Event flags. Timing events only time (no system-scope cache writeback/invalidate when they
// complete); dependency events between this device's queues release to device scope.
constexpr unsigned kTimingEventFlags = hipEventDisableSystemFence;
constexpr unsigned kSyncEventFlags = hipEventDisableTiming | hipEventReleaseToDevice;

struct sbr_ctx {
    int device = 0;
    // n-device context (sbr_init_multi): the per-device contexts, RCCL communicator and
    // rank buffers live in `multi`; the host-pointer sweeps fan out over them
    sbr_multi* multi = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    // learning workspaces: slot 0 for single sweeps; a pipelined batch rotates through
    // kLearnSlots slots, each learned on its own highest-priority stream, so the
    // learning of the next kLearnSlots-1 batches (latency-bound: 32 waves each) runs
    // concurrently with the equilibrium of the current one
    // (workspace slots and streams are separate counts: grid k learns into slot k mod
    // kLearnSlots on stream k mod kLearnStreams)
    static constexpr int kLearnSlots = 3; // slot 0: single sweeps; slots 0, 1: batch groups
    static constexpr int kLearnStreams = 3; // learning streams (with the context stream: within GPU_MAX_HW_QUEUES = 4)
    // the hetero batch pipeline alternates two of these slots' streams/events; single sweeps
    // run their column chunks on the streams with slot events 0..kLearnStreams-1
    static_assert(kLearnStreams >= 2 && kLearnSlots >= kLearnStreams, "kLearnSlots >= kLearnStreams >= 2");
    size_t ws_beta[kLearnSlots] = {}, ws_cap[kLearnSlots] = {};
    sbr::LearnBufs LW[kLearnSlots]{};
    int last_slot = 0;
    int64_t last_off = 0; // column offset of the last grid inside its (grouped) learning slot
    hipStream_t lstream[kLearnStreams] = {};
    hipEvent_t ev_in = nullptr, ev_learned[kLearnSlots] = {}, ev_eq[kLearnSlots] = {};
    // fork/join fences between HIP's null stream and `stream`, and the end of the last call
    // (whatever stream it ran on) that every call waits for (CallFence)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_last = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    // hetero learning workspace; H2 is the second slot of a pipelined hetero batch
    size_t hs_col = 0, hs_cap = 0, hs_K = 0;
    sbr::HeteroBufs H{};
    size_t hs2_col = 0, hs2_cap = 0, hs2_K = 0;
    sbr::HeteroBufs H2{};
    // social-learning workspace (sbr_social.hip): per point 5 knot buffers + n_cmp
    size_t so_pts = 0, so_cap = 0, so_cmp = 0;
    double *so_ws = nullptr, *so_cmpo = nullptr, *so_xi = nullptr;
    int32_t *so_n_old = nullptr, *so_live = nullptr, *so_work[2] = {nullptr, nullptr}, *so_count = nullptr;
    uint32_t *so_slots = nullptr, *so_bits = nullptr;
    int64_t* so_steps = nullptr;
    // promotion pool (sbr::SocialPool); so_count = [list 0, list 1, pool used, pool live] and, from
    // word 4, three 64-bit counters: point-iterates per mode (sbr_social_schedule_stats)
    size_t pl_slots = 0, pl_cap = 0, pl_cmp = 0;
    double *pl_ws = nullptr, *pl_cmpo = nullptr, *pl_xi = nullptr;
    int32_t *pl_n_old = nullptr, *pl_live = nullptr, *pl_it = nullptr, *pl_ready = nullptr;
    uint32_t *pl_perm = nullptr, *pl_bits = nullptr;
    int64_t *pl_steps = nullptr, *pl_pts = nullptr;
    int32_t* so_count_host = nullptr; // pinned
    double* het_aw_path = nullptr;      // set only inside sbr_hetero_point_paths
    double *so_path_t = nullptr, *so_path_G = nullptr, *so_path_aw = nullptr; // set only inside sbr_social_point_paths
    int32_t* so_path_n = nullptr;
    int32_t so_path_cap = 0;
    sbr::SocialArgs* so_args_dev = nullptr;  // {main, pool} arguments of the iterate kernel
    sbr::SocialArgs* so_args_host = nullptr; // pinned staging for them
    int64_t so_promoted = 0, so_rerun = 0; // last sweep: points promoted into the pool / re-run larger
    int64_t so_sched[3] = {0, 0, 0};       // last sweep: point-iterates per mode (multi-point, one-point, pool)
    // sbr_set_social_schedule (tests and A/B of the schedule; −1: built in)
    int32_t so_coop_max = -1, so_waves = -1, so_inner = -1;
    int64_t so_budget = 0;            // workspace bytes (0: 60 % of free HBM)
    int64_t* so_prof = nullptr;       // SBR_FLAG_DIAG_SOCIAL_PROF: [pts][8]
    size_t so_prof_pts = 0;
    std::vector<int64_t> so_prof_acc; // host sums over the chunks of the last sweep
    // host-API staging
    void* stage = nullptr;
    size_t stage_bytes = 0;
    // pinned landing buffer of the host-pointer sweeps' results: one DMA copy at full PCIe rate,
    // then a multi-threaded host copy into the caller's (pageable) arrays
    void* res_pin = nullptr;
    size_t res_pin_bytes = 0;
    // sbr_equilibrium_on_knots: the caller's knot grid and its hazard path stay resident between
    // calls, keyed by value (n, t, G and β, η, p, λ); the device block and its pinned host mirror
    // share one layout (KnotLayout), so each transfer is one contiguous copy
    char* kn_dev = nullptr;
    char* kn_pin = nullptr;
    size_t kn_cap_k = 0, kn_cap_u = 0;
    bool kn_valid = false;
    int64_t kn_n = 0;
    double kn_key[4] = {};
    std::vector<double> kn_t, kn_G, kn_hr; // host copies of the resident knots and HR
    std::vector<double> kn_pdf;            // sbr_equilibrium_on_knots_pdf's pdf values (empty: βG(1 − G))
    int32_t kn_m = 0, kn_ntau = 0;         // knots <= η; τ̄ entries (0: the hazard's BoundsError)
    // single-u calls: mapped, coherent host memory the kernel reads t_end / u from and writes the
    // results and paths to (no copy launches per call) — host view and device view
    double* kn_zc = nullptr;
    double* kn_zc_dev = nullptr;
    size_t kn_zc_cap = 0; // doubles
    // sbr_hetero_equilibrium_on_knots: the same for a LearningResultsHetero (knots, K group CDFs,
    // the K hazard paths), keyed by K, n, t, G, βs, dist, η, p, λ
    char* hk_dev = nullptr;
    char* hk_pin = nullptr;
    size_t hk_cap_k = 0, hk_cap_u = 0;
    bool hk_valid = false;
    int64_t hk_n = 0;
    int32_t hk_K = 0, hk_ntau = 0;
    std::vector<double> hk_key, hk_t, hk_G, hk_hr;
    int lds_cap = 0, lds_cap_b = 0;
    int lds_smem = 0;
    // kernel timing (HIP event pairs on the launching stream), opt-in via sbr_timing_enable
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<hipEvent_t> ev_grid; // per grid of the last baseline batch: results complete
    std::vector<hipEvent_t> ev_hn;   // per equilibrium launch of a baseline batch: its hazards normalised
    int64_t n_grid = 0;
    int64_t bt_budget = 0; // baseline batch learning workspaces, bytes (0: 40 % of free + held HBM)
    int64_t pt_budget = 0; // learning workspace of a list of models (sbr_solve_points), bytes (0: the same default)
    // sbr_sweep_econ: HR rows, τ̄ counters and status words of the hazard classes in flight
    // (ec_rows rows of stride ec_ld: classes per chunk × columns), and its budget in bytes
    double* ec_hr = nullptr;
    int32_t* ec_cnt = nullptr; // n_tau [ec_rows], n_le [ec_rows], status [ec_rows]
    size_t ec_rows = 0, ec_ld = 0;
    int64_t ec_budget = 0; // 0: 40 % of the free plus the already held HBM
    // sbr_sweep_hetero_econ: the K HR rows and K running-integral rows, τ̄ counters and status words of
    // the hazard classes in flight (he_rows rows of stride he_ld = K × the learning stride: classes
    // per chunk × columns); its budget is ec_budget
    double *he_hr = nullptr, *he_hrI = nullptr;
    int32_t* he_cnt = nullptr; // n_tau [he_rows], n_le [he_rows], status [he_rows]
    size_t he_rows = 0, he_ld = 0;
    int32_t he_slab = 0; // sbr_set_hetero_econ_slab: knots of the equilibrium launches' LDS slab (0: het_lds())
    size_t ev_used = 0;
    struct TRec {
        int kind; // 0 learning (+ hazard), 1 equilibrium
        hipEvent_t a, b;
        int count; // launches the span covers (a pipelined batch times its equilibria as one span)
    };
    std::vector<TRec> trec;
    // phases of the last host-pointer baseline sweep while timing is enabled (sbr_host_phases):
    // H2D, kernels, D2H (HIP events on the stream), the early-exit post-pass and the whole call
    // (host clock), milliseconds
    double ph_ms[5] = {};
    // the last chunked single sweep while timing is enabled: per chunk, events at its learning
    // end and its equilibrium end, and the sweep start (sbr_chunk_timeline)
    hipEvent_t ck_start = nullptr;
    std::vector<hipEvent_t> ck_ev;
    // readiness schedule of single sweeps: the learning kernel and the equilibrium workgroups
    // on streams with disjoint CU masks (hipExtStreamCreateWithCUMask), and the publication
    // queue [head, err, tail, pad, q[n_beta], hz_flag[n_beta]]
    hipStream_t rs_learn = nullptr, rs_eq = nullptr;
    int rs_state = 0; // 0 untried, 1 available, -1 unavailable (chunked schedule instead)
    bool rs_used = false; // the last run_baseline took the readiness schedule
    int32_t* rq = nullptr;
    size_t rq_cap = 0;
    hipEvent_t ev_rin = nullptr, ev_rq = nullptr, ev_rl = nullptr, ev_re = nullptr;
};

namespace sbr_capi {

constexpr int kDefaultCap = 65536; // the longest Fig 5 tail (β ≈ 2000) needs 20k knots below η

inline int fail(sbr_ctx* c, int code, const char* what, hipError_t e = hipSuccess)
{
    if (c) {
        c->err = what;
        if (e != hipSuccess) { c->err += ": "; c->err += hipGetErrorString(e); }
    }
    return code;
}

#define HIP_TRY(ctx, expr, code)                                  \
    do {                                                          \
        hipError_t _e = (expr);                                   \
        if (_e != hipSuccess) return fail((ctx), (code), #expr, _e); \
    } while (0)

// Every entry point runs inside a CallFence:
//  * it is ordered after the previous call on this context, whatever stream that one used
//    (a *_dev call on a caller stream X followed by a host-pointer call on the private
//    stream would otherwise let the learning kernel rewrite LW[0] while X still reads it);
//  * a NULL stream argument of a *_dev entry point names HIP's null stream (torch's default
//    stream): the work runs on the context's non-blocking stream, fenced to the null stream
//    on both sides (it starts after earlier null-stream work, and null-stream work enqueued
//    after the call starts after it) without putting the kernels on the null stream's queue.
// Fence failures are reported (SBR_EDEVICE), never dropped.
struct CallFence {
    sbr_ctx* c;
    bool null_stream;
    hipStream_t s;
    CallFence(sbr_ctx* c_, void* stream, bool dev)
        : c(c_), null_stream(dev && stream == nullptr), s(dev && stream ? (hipStream_t)stream : c_->stream)
    {
    }
    int begin()
    {
        if (null_stream) {
            HIP_TRY(c, hipEventRecord(c->ev_fork, nullptr), SBR_EDEVICE);
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_fork, 0), SBR_EDEVICE);
        }
        if (c->have_last && c->last_stream != s) HIP_TRY(c, hipStreamWaitEvent(s, c->ev_last, 0), SBR_EDEVICE);
        return SBR_OK;
    }
    int end(int rc)
    {
        // recorded after a failure too: later calls still order after whatever was enqueued
        hipError_t e = hipEventRecord(c->ev_last, s);
        if (e == hipSuccess) {
            c->have_last = true;
            c->last_stream = s;
        }
        if (null_stream && e == hipSuccess) {
            e = hipEventRecord(c->ev_join, c->stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(nullptr, c->ev_join, 0);
        }
        if (rc == SBR_OK && e != hipSuccess) return fail(c, SBR_EDEVICE, "stream fence", e);
        return rc;
    }
};

// run body(stream) inside a CallFence (dev: `stream` is a caller stream or NULL = null stream;
// host-pointer entry points pass dev = false and run on the private stream)
template <class F>
int fenced(sbr_ctx* c, void* stream, bool dev, F&& body)
{
    CallFence f(c, stream, dev);
    int rc = f.begin();
    if (rc) return rc;
    rc = body(f.s);
    return f.end(rc);
}

// ξ_guess (solver.jl:413,441) is honoured by sbr_equilibrium_on_knots, which solves on the caller's
// whole knot grid; the sweeps' truncated learning (DESIGN.md §Truncated learning) and the
// extensions' own bisections start at the reference's defaults, so they refuse a guess
inline int refuse_guess(sbr_ctx* c, const sbr_opts* o)
{
    if (o && (o->flags & SBR_FLAG_XI_GUESS))
        return fail(c, SBR_EARG, "xi_guess: only sbr_equilibrium_on_knots takes a first iterate");
    return SBR_OK;
}

// EconomicParameters / LearningParameters scalar checks (model.jl:31-35, 71-76)
inline bool scalars_valid(double x0, double p, double kappa, double lambda)
{
    return x0 >= 0.0 && p >= 0.0 && p <= 1.0 && kappa > 0.0 && kappa < 1.0 && lambda > 0.0;
}

// every value of the per-column arrays a[0 .. n) is positive, else SBR_EARG with the family's `what`
inline int check_positive(sbr_ctx* c, int64_t n, std::initializer_list<const double*> arrays, const char* what)
{
    for (const double* a : arrays)
        for (int64_t i = 0; i < n; i++)
            if (!(a[i] > 0.0)) return fail(c, SBR_EARG, what);
    return SBR_OK;
}

inline int check_u(sbr_ctx* c, const double* u, int64_t n_u, const char* what = "ArgumentError: u must be non-negative")
{
    for (int64_t j = 0; j < n_u; j++)
        if (!(u[j] >= 0.0)) return fail(c, SBR_EARG, what);
    return SBR_OK;
}

// the six result fields a *_dev entry point writes unconditionally (iters is optional)
inline bool has_fields(const sbr_result_soa* out)
{
    return out && out->xi && out->tau_in_unc && out->tau_out_unc && out->aw_max && out->tol && out->status;
}

inline sbr_opts resolve(const sbr_opts* o)
{
    sbr_opts r;
    sbr_default_opts(&r);
    if (o) {
        r = *o;
        // a zero field is the default (a zero-filled sbr_opts is the reference's defaults)
        if (!(r.ode_reltol > 0.0)) r.ode_reltol = 2.220446049250313e-16;
        if (!(r.ode_abstol > 0.0)) r.ode_abstol = 2.220446049250313e-16;
        if (r.knot_capacity <= 0) r.knot_capacity = kDefaultCap;
        if (r.ode_maxiters <= 0) r.ode_maxiters = SBR_DEFAULT_ODE_MAXITERS;
        // the device ODE loops count a solve's steps in int32 (sbr_ode.h OdeOut)
        if (r.ode_maxiters > INT32_MAX) r.ode_maxiters = INT32_MAX;
        if (r.bisect_max_iters <= 0) r.bisect_max_iters = 100;
        if (r.hetero_max_iters <= 0) r.hetero_max_iters = 500;
    }
    return r;
}

// hetero equilibrium LDS slab (doubles): knot times + per-group HR summaries of one column,
// capped so that SBR_HET_MINW = 2 workgroups share a CU's 160 KB (2 x (79.5 KB + the kernel's
// static LDS)); config 4 with Rosenbrock23 after the switch: n <= 7.9k knots
constexpr int kHetLds = 10176;
inline int het_lds(const sbr_ctx* c) { return c->lds_cap * 3 < kHetLds ? c->lds_cap * 3 : kHetLds; }
// the group counts every heterogeneity entry point takes (K = 1, 2, 3, 4, 8: specialised kernels,
// the others: sbr_hetero_wide.hip / sbr_hetero_learn_wide.hip)
inline bool hetero_K_ok(int32_t K) { return K >= 1 && K <= SBR_HETERO_MAX_K; }
static_assert(SBR_HETERO_MAX_K == 16, "kHeteroKMsg names the limit");
constexpr const char* kHeteroKMsg =
    "K must be between 1 and 16 (SBR_HETERO_MAX_K): the learning solve's Rosenbrock23 branch, a K x K LU, is "
    "pinned against the oracle up to 16 groups";
inline bool hetero_wide(const sbr_opts& o) { return (o.flags & SBR_FLAG_HETERO_WIDE) != 0; }

// Device buffers of a workspace: free_dev frees and nulls each pointer; alloc_dev allocates the
// (pointer, bytes) pairs in order, SBR_ENOMEM at the first that does not fit.
template <class... P>
void free_dev(P*&... p)
{
    ((p ? (void)hipFree(p) : (void)0, p = nullptr), ...);
}
struct DevBuf {
    void** p;
    size_t bytes;
    template <class T>
    DevBuf(T*& p_, size_t b) : p((void**)&p_), bytes(b) {}
};
inline int alloc_dev(sbr_ctx* c, std::initializer_list<DevBuf> bufs)
{
    for (const DevBuf& b : bufs) HIP_TRY(c, hipMalloc(b.p, b.bytes), SBR_ENOMEM);
    return SBR_OK;
}

// Workspaces of the context, grow-only (ensure_*) and released by sbr_free (free_*); each is
// defined in its family's file.
// sbr_capi_baseline.hip: learning slots, the pipelined sweeps' streams, sbr_sweep_econ's class rows
void free_learn(sbr_ctx* c, int slot);
size_t learn_ld(size_t cap);
int ensure_learn(sbr_ctx* c, size_t n_beta, size_t cap, int slot = 0, bool hri = false);
int ensure_pipe_streams(sbr_ctx* c);
void free_econ(sbr_ctx* c);
int ensure_econ(sbr_ctx* c, size_t rows, size_t ld);
void strip_hazard_status(uint32_t* status, int64_t n);
// sbr_capi_hetero.hip
void free_hetero(sbr_ctx* c);
int ensure_hetero(sbr_ctx* c, size_t n_col, size_t cap, size_t K);
void copy_hetero_paths(const double* src, bool run, int K, int64_t n, int64_t cap, double* aw_total,
                       double* aw_groups);
// sbr_capi_social.hip
void free_social(sbr_ctx* c);
int ensure_social(sbr_ctx* c, size_t pts, size_t cap, size_t n_cmp);
void free_pool(sbr_ctx* c);
int ensure_pool(sbr_ctx* c, size_t slots, size_t cap, size_t n_cmp);
// sbr_capi.hip: timing records of sbr_timing_enable (no-ops while timing is off)
hipEvent_t next_event(sbr_ctx* c);
hipEvent_t tstart(sbr_ctx* c, hipStream_t s);
void tend(sbr_ctx* c, hipStream_t s, int kind, hipEvent_t a, int count = 1);

}  // namespace sbr_capi

// device-pointer entry points address one GPU's HBM: they need a single-device context
#define SBR_SINGLE_DEVICE(c)                                                                                \
    do {                                                                                                    \
        if ((c) && (c)->multi)                                                                              \
            return fail((c), SBR_EARG, "device-pointer entry points need a single-device context "          \
                                       "(sbr_multi_child)");                                                \
    } while (0)
// per-device diagnostics (timings, learning statistics, social counters) describe one
// device's last sweep: on an n-device context they would report rank 0's shard as if it
// were the grid, so they are refused there — ask the rank's child context instead
#define SBR_PER_DEVICE_DIAG(c)                                                                              \
    do {                                                                                                    \
        if ((c) && (c)->multi)                                                                              \
            return fail((c), SBR_EARG, "per-device diagnostic: call it on sbr_multi_child(ctx, rank)");    \
    } while (0)
// single-point / diagnostic entry points on an n-device context run on its rank 0
#define SBR_ON_RANK0(c, call)                                                                               \
    do {                                                                                                    \
        if ((c) && (c)->multi) {                                                                            \
            sbr_ctx* const c0_ = sbr_multi_child((c), 0);                                                   \
            sbr_ctx* const parent_ = (c);                                                                   \
            sbr_ctx* c = c0_;                                                                               \
            const int rc_ = (call);                                                                         \
            parent_->err = rc_ ? std::string(sbr_last_error(c0_)) : std::string();                          \
            return rc_;                                                                                     \
        }                                                                                                   \
    } while (0)

