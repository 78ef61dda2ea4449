// sbr_capi_social.hip — the social-learning extension's entry points of the C API: its workspace
// and promotion pool, the schedule's settings and statistics, the fixed-point passes and the sweeps.
#include "sbr_hostio.h"

using namespace sbr_capi;

namespace sbr_capi {

// so_count: four int32 counters, then the three 64-bit mode counters of the schedule statistics
constexpr int kSoSched = 4, kSoCountWords = kSoSched + 2 * 3;

void free_social(sbr_ctx* c)
{
    free_dev(c->so_ws, c->so_cmpo, c->so_xi, c->so_n_old, c->so_live, c->so_work[0], c->so_work[1], c->so_count,
             c->so_slots, c->so_bits, c->so_steps);
    c->so_pts = c->so_cap = c->so_cmp = 0;
}

int ensure_social(sbr_ctx* c, size_t pts, size_t cap, size_t n_cmp)
{
    if (pts <= c->so_pts && cap == c->so_cap && n_cmp <= c->so_cmp) return SBR_OK;
    free_social(c);
    // so_ws: the wave-blocked layout (sbr_social.hip BView), whole 64-point groups
    const int rc = alloc_dev(c, {{c->so_ws, ((pts + 63) / 64) * 64 * 5 * cap * 8}, {c->so_cmpo, pts * n_cmp * 8},
                                 {c->so_xi, pts * 8}, {c->so_n_old, pts * 4}, {c->so_live, pts * 4},
                                 {c->so_work[0], pts * 4}, {c->so_work[1], pts * 4},
                                 {c->so_count, kSoCountWords * 4}, {c->so_slots, pts * 4}, {c->so_bits, pts * 4},
                                 {c->so_steps, pts * 8}});
    if (rc) return rc;
    if (!c->so_count_host) HIP_TRY(c, hipHostMalloc(&c->so_count_host, kSoCountWords * 4), SBR_ENOMEM);
    if (!c->so_args_dev) HIP_TRY(c, hipMalloc(&c->so_args_dev, 2 * sizeof(sbr::SocialArgs)), SBR_ENOMEM);
    if (!c->so_args_host) HIP_TRY(c, hipHostMalloc(&c->so_args_host, 2 * sizeof(sbr::SocialArgs)), SBR_ENOMEM);
    c->so_pts = pts;
    c->so_cap = cap;
    c->so_cmp = n_cmp;
    return SBR_OK;
}

void free_pool(sbr_ctx* c)
{
    free_dev(c->pl_ws, c->pl_cmpo, c->pl_xi, c->pl_n_old, c->pl_live, c->pl_it, c->pl_ready, c->pl_perm, c->pl_bits,
             c->pl_steps, c->pl_pts);
    c->pl_slots = c->pl_cap = c->pl_cmp = 0;
}

int ensure_pool(sbr_ctx* c, size_t slots, size_t cap, size_t n_cmp)
{
    if (slots <= c->pl_slots && cap == c->pl_cap && n_cmp <= c->pl_cmp) return SBR_OK;
    free_pool(c);
    slots = (slots + 63) & ~(size_t)63;
    const int rc = alloc_dev(c, {{c->pl_ws, slots * 5 * cap * 8}, {c->pl_cmpo, slots * n_cmp * 8},
                                 {c->pl_xi, slots * 8}, {c->pl_n_old, slots * 4}, {c->pl_live, slots * 4},
                                 {c->pl_it, slots * 4}, {c->pl_ready, slots * 4}, {c->pl_perm, slots * 4},
                                 {c->pl_bits, slots * 4}, {c->pl_steps, slots * 8}, {c->pl_pts, slots * 8}});
    if (rc) return rc;
    c->pl_slots = slots;
    c->pl_cap = cap;
    c->pl_cmp = n_cmp;
    return SBR_OK;
}

}  // namespace sbr_capi

extern "C" {

int sbr_social_prof_read(sbr_ctx* c, int64_t* out8)
{
    SBR_PER_DEVICE_DIAG(c);
    if (!c || !out8) return SBR_EARG;
    for (int k = 0; k < 8; k++) out8[k] = k < (int)c->so_prof_acc.size() ? c->so_prof_acc[k] : 0;
    return SBR_OK;
}

int sbr_social_overflow_stats(sbr_ctx* c, int64_t* promoted, int64_t* rerun)
{
    SBR_PER_DEVICE_DIAG(c);
    if (!c) return SBR_EARG;
    if (promoted) *promoted = c->so_promoted;
    if (rerun) *rerun = c->so_rerun;
    return SBR_OK;
}

int sbr_social_schedule_stats(sbr_ctx* c, int64_t* out3)
{
    SBR_PER_DEVICE_DIAG(c);
    if (!c || !out3) return SBR_EARG;
    for (int k = 0; k < 3; k++) out3[k] = c->so_sched[k];
    return SBR_OK;
}

int sbr_set_social_schedule(sbr_ctx* c, int32_t coop_max, int32_t waves, int32_t inner)
{
    if (!c || waves == 0 || inner == 0) return SBR_EARG;
    for (int r = 0; c->multi && r < sbr_multi_size(c); r++)
        (void)sbr_set_social_schedule(sbr_multi_child(c, r), coop_max, waves, inner);
    c->so_coop_max = coop_max < 0 ? -1 : coop_max;
    c->so_waves = waves < 0 ? -1 : waves;
    c->so_inner = inner < 0 ? -1 : inner;
    return SBR_OK;
}

int sbr_social_plan(int32_t n_pts, int32_t live, int32_t coop_max, int32_t waves, int32_t* out4)
{
    if (!out4 || n_pts < 1 || live < 0 || live > n_pts || waves == 0) return SBR_EARG;
    const sbr::SocialPlan pl = sbr::social_plan(n_pts, coop_max, waves < 0 ? -1 : waves);
    out4[0] = pl.nbs;
    out4[1] = pl.nmain;
    out4[2] = sbr::social_plan_lanes(live, pl.nbs, pl.nmain);
    out4[3] = pl.nmain; // main blocks of the launch (the promotion pool's blocks follow them)
    return SBR_OK;
}

int sbr_social_plan_lanes(int32_t n_pts, int32_t coop_max, int32_t waves, int64_t n, const int32_t* live,
                          int32_t* lanes)
{
    if (n_pts < 1 || waves == 0 || n < 0 || (n > 0 && (!live || !lanes))) return SBR_EARG;
    const sbr::SocialPlan pl = sbr::social_plan(n_pts, coop_max, waves < 0 ? -1 : waves);
    for (int64_t i = 0; i < n; i++) {
        if (live[i] < 0 || live[i] > n_pts) return SBR_EARG;
        lanes[i] = sbr::social_plan_lanes(live[i], pl.nbs, pl.nmain);
    }
    return SBR_OK;
}

int sbr_set_social_workspace(sbr_ctx* c, int64_t bytes)
{
    if (!c || bytes < 0) return SBR_EARG;
    for (int r = 0; c->multi && r < sbr_multi_size(c); r++) (void)sbr_set_social_workspace(sbr_multi_child(c, r), bytes);
    c->so_budget = bytes;
    return SBR_OK;
}

}  // extern "C"

namespace {
constexpr int kSocialDefaultCap = 98304;  // ≈1.4× the typical longest iterate on config 5 (≈70k knots)
constexpr int kSocialMaxCap = 1 << 22;    // overflow retries grow 4× per pass up to this
constexpr int64_t kPoolSlots = 256;       // promotion pool slots (points that outgrow the capacity)
constexpr int kSocialInner = 16; // fixed-point iterates per launch (compaction in between)
constexpr int kSocialBulk = 2;   // launches of kSocialInner iterates before the shorter ones
constexpr int kSocialInner2 = 8; // iterates per launch after the bulk launches

int social_checks(sbr_ctx* c, const double* beta, const double* eta, const double* u, int64_t n_beta, int64_t n_u,
                  double x0, double p, double kappa, double lambda, const double* cmp, int32_t n_cmp, double tol,
                  int32_t max_iter, sbr_result_soa* out)
{
    if (!c || !out || !beta || !eta || !u || !cmp) return SBR_EARG;
    if (!has_fields(out)) return fail(c, SBR_EARG, "result arrays");
    if (n_beta <= 0 || n_u <= 0 || n_beta * n_u > (int64_t(1) << 40)) return fail(c, SBR_EARG, "grid size");
    if (n_cmp < 1 || max_iter < 1 || !(tol > 0.0)) return fail(c, SBR_EARG, "n_cmp / max_iter / tol");
    if (!scalars_valid(x0, p, kappa, lambda)) return fail(c, SBR_EARG, "ArgumentError: x0/p/kappa/lambda");
    return SBR_OK;
}

// one pass of the whole fixed point over points [0, n_total) (list == nullptr)
// or over the global point indices list[0 .. n_total), chunked by workspace
// size; poll > 0 reads the live counts after every launch and stops early.
// Points whose iterate outgrows `cap` are promoted into the pool (16× the
// capacity) and redo that iterate from the pool blocks of the same or the next launch.
int run_social_pass(sbr_ctx* c, hipStream_t s, const double* beta, const double* eta, double x0, const double* u,
                    int64_t n_u, double p, double kappa, double lambda, const double* cmp, int32_t n_cmp, double tol,
                    int32_t max_iter, const sbr_opts& o, sbr_result_soa* out, int32_t* fp_iters, int64_t* rk_steps,
                    int poll, size_t cap, size_t pcap, const int64_t* list, int64_t n_total)
{
    const size_t per_pt = 5 * cap * 8 + (size_t)n_cmp * 8 + 64;
    const size_t per_slot = 5 * pcap * 8 + (size_t)n_cmp * 8 + 64;
    int64_t budget = c->so_budget, pbudget = 0;
    {
        size_t fr = 0, tot = 0;
        HIP_TRY(c, hipMemGetInfo(&fr, &tot), SBR_EDEVICE);
        const double avail = (double)fr + (double)c->so_pts * (5 * c->so_cap * 8 + c->so_cmp * 8 + 64) +
                             (double)c->pl_slots * (5 * c->pl_cap * 8 + c->pl_cmp * 8 + 64);
        if (budget <= 0) budget = (int64_t)(avail * 0.6);
        pbudget = (int64_t)(avail * 0.15);
    }
    int64_t chunk = budget / (int64_t)per_pt;
    if (chunk < 64 && !list) return fail(c, SBR_ENOMEM, "social workspace budget below 64 points");
    if (chunk < 1) chunk = 1; // overflow retries: at least one point at a time
    if (chunk > (1 << 30)) chunk = 1 << 30;
    if (chunk >= n_total) chunk = n_total;
    else if (chunk >= 64) chunk &= ~(int64_t)63; // whole wave groups
    int rc = ensure_social(c, (size_t)chunk, cap, (size_t)n_cmp);
    if (rc) return rc;
    // pool: up to kPoolSlots slots (whole wave groups) within its budget
    int64_t nslots = pcap > cap ? pbudget / (int64_t)per_slot : 0;
    if (nslots > kPoolSlots) nslots = kPoolSlots;
    if (nslots > chunk) nslots = chunk;
    if (nslots >= 64) nslots &= ~(int64_t)63;
    if (nslots > 0) {
        rc = ensure_pool(c, (size_t)nslots, pcap, (size_t)n_cmp);
        if (rc) return rc;
    }
    const bool prof = (o.flags & SBR_FLAG_DIAG_SOCIAL_PROF) != 0;
    if (prof && c->so_prof_pts < (size_t)chunk) {
        if (c->so_prof) (void)hipFree(c->so_prof);
        c->so_prof = nullptr;
        c->so_prof_pts = 0;
        HIP_TRY(c, hipMalloc(&c->so_prof, (size_t)chunk * 64), SBR_ENOMEM);
        c->so_prof_pts = (size_t)chunk;
    }
    for (int64_t pt0 = 0; pt0 < n_total; pt0 += chunk) {
        const int32_t npts = (int32_t)((n_total - pt0) < chunk ? (n_total - pt0) : chunk);
        sbr::SocialArgs a{};
        a.beta = beta; a.eta = eta; a.u = u; a.cmp = cmp;
        a.pt0 = list ? 0 : pt0; a.pts = list ? list + pt0 : nullptr;
        a.n_pts = npts; a.n_u = (int32_t)n_u; a.n_cmp = n_cmp;
        a.max_iter = max_iter; a.bisect_max_iters = o.bisect_max_iters; a.cap = (int32_t)cap;
        a.maxiters = o.ode_maxiters;
        a.x0 = x0; a.p = p; a.kappa = kappa; a.lam = lambda; a.tol = tol; a.rtol = o.ode_reltol; a.atol = o.ode_abstol;
        a.ws = c->so_ws; a.cmpo = c->so_cmpo; a.n_old = c->so_n_old; a.slots = c->so_slots; a.xi_new = c->so_xi;
        a.bits = c->so_bits; a.steps = c->so_steps; a.live = c->so_live; a.work = c->so_work[0];
        a.count = c->so_count;
        a.out = sbr::ResultSoA{out->xi, out->tau_in_unc, out->tau_out_unc, out->aw_max, out->tol, out->status,
                               out->iters};
        a.fp_iters = fp_iters;
        a.steps_out = rk_steps;
        a.prof = prof ? c->so_prof : nullptr;
        a.path_t = c->so_path_t; a.path_G = c->so_path_G; a.path_aw = c->so_path_aw; a.path_n = c->so_path_n;
        a.path_cap = c->so_path_cap;
        a.sched = (unsigned long long*)(c->so_count + kSoSched);
        a.pool = sbr::SocialPool{};
        sbr::SocialArgs b{}; // the pool's own arguments (n_pts = 0: no pool blocks)
        if (nslots > 0) {
            a.pool = sbr::SocialPool{c->pl_ws,    (int32_t)pcap, (int32_t)nslots, c->so_count + 2, c->so_count + 3,
                                     c->pl_pts,   c->pl_n_old,   c->pl_perm,      c->pl_xi,        c->pl_bits,
                                     c->pl_steps, c->pl_live,    c->pl_it,        c->pl_ready};
            b = a;
            b.pt0 = 0; b.pts = c->pl_pts; b.n_pts = (int32_t)nslots; b.cap = (int32_t)pcap;
            b.ws = c->pl_ws; b.cmpo = c->pl_cmpo; b.n_old = c->pl_n_old; b.slots = c->pl_perm; b.xi_new = c->pl_xi;
            b.bits = c->pl_bits; b.steps = c->pl_steps; b.live = c->pl_live; b.work = nullptr; b.count = nullptr;
            b.prof = nullptr;
            b.pool = sbr::SocialPool{};
            b.it_cur = c->pl_it; b.ready = c->pl_ready; b.n_live = c->so_count + 3;
            HIP_TRY(c, hipMemsetAsync(c->pl_ready, 0, (size_t)nslots * 4, s), SBR_EDEVICE);
        }
        // pool allocator + live, and this chunk's mode counters
        HIP_TRY(c, hipMemsetAsync(c->so_count + 2, 0, (kSoCountWords - 2) * 4, s), SBR_EDEVICE);
        // (the staging buffer is reused by the next chunk only after this one's final sync)
        c->so_args_host[0] = a;
        c->so_args_host[1] = b;
        HIP_TRY(c, hipMemcpyAsync(c->so_args_dev, c->so_args_host, 2 * sizeof(sbr::SocialArgs),
                                  hipMemcpyHostToDevice, s),
                SBR_EDEVICE);
        if (prof) HIP_TRY(c, hipMemsetAsync(c->so_prof, 0, (size_t)npts * 64, s), SBR_EDEVICE);
        hipEvent_t t0 = tstart(c, s);
        HIP_TRY(c, sbr::launch_social_init(a, s), SBR_EDEVICE);
        tend(c, s, 0, t0);
        t0 = tstart(c, s);
        // kSocialInner iterates per launch; a point promoted during a launch redoes that
        // iterate in the same or the next launch: one launch past max_iter drains the pool
        // The first kSocialBulk launches run kSocialInner iterates each (the bulk: most points
        // converge around iterate 35); later launches run kSocialInner2, so the survivors are
        // re-spread over the waves (fewer points per wave, then one: the whole-wave mode) sooner.
        const int drain_inner = c->so_inner >= 1 ? c->so_inner : kSocialInner;
        std::vector<int> inner;
        for (int done = 0, q = 0; done < max_iter; q++) {
            const int m = c->so_inner >= 1 ? c->so_inner : (q < kSocialBulk ? kSocialInner : kSocialInner2);
            inner.push_back(m);
            done += m;
        }
        const int n_launch = (int)inner.size();
        static const bool trace = getenv("SBR_SOCIAL_TRACE") != nullptr;
        const auto tr0 = std::chrono::steady_clock::now();
        int q = 0, it = 1;
        for (; q < n_launch; it += inner[q], q++) {
            const int k = q & 1;
            HIP_TRY(c, sbr::launch_social_iter(a, b, c->so_args_dev, it, inner[q], c->so_work[k],
                                               c->so_count + k, c->so_work[k ^ 1], c->so_count + (k ^ 1), c->so_coop_max, c->so_waves, s),
                    SBR_EDEVICE);
            if ((poll > 0 || trace) && q + 1 < n_launch) {
                HIP_TRY(c, hipMemcpyAsync(c->so_count_host, c->so_count, 4 * 4, hipMemcpyDeviceToHost, s),
                        SBR_EDEVICE);
                HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
                if (trace) // diagnostics: the fixed point's timeline (live points after each launch)
                    fprintf(stderr, "sbr_social_trace launch=%d t=%.3f live=%d pool_used=%d pool_live=%d\n", q,
                                 std::chrono::duration<double>(std::chrono::steady_clock::now() - tr0).count(),
                                 c->so_count_host[k ^ 1], c->so_count_host[2], c->so_count_host[3]);
                if (poll > 0 && c->so_count_host[k ^ 1] == 0 && c->so_count_host[3] == 0) { q++; break; }
            }
        }
        // Pool drain.  A point promoted during a launch restarts at its promotion iterate in the
        // next launch, so it can trail the main worklist by up to one launch's iterates (16) and
        // still be live once the main list has reached max_iter: drain launches of kSocialInner
        // iterates run until the pool has no live point (bounded: each advances every pool point
        // by kSocialInner iterates towards max_iter).
        for (int d = 0; nslots > 0 && d <= max_iter / drain_inner + 1; d++, it += drain_inner, q++) {
            HIP_TRY(c, hipMemcpyAsync(c->so_count_host, c->so_count, 4 * 4, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
            HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
            if (c->so_count_host[3] == 0) break;
            const int k = q & 1;
            HIP_TRY(c, sbr::launch_social_iter(a, b, c->so_args_dev, it, drain_inner, c->so_work[k],
                                               c->so_count + k, c->so_work[k ^ 1], c->so_count + (k ^ 1), c->so_coop_max, c->so_waves, s),
                    SBR_EDEVICE);
            if (trace)
                fprintf(stderr, "sbr_social_trace drain=%d pool_live_before=%d\n", d, c->so_count_host[3]);
        }
        tend(c, s, 1, t0);
        // promotions of this chunk (diagnostics), the pool's live count, and the sync that frees
        // the argument staging
        HIP_TRY(c, hipMemcpyAsync(c->so_count_host + 2, c->so_count + 2, (kSoCountWords - 2) * 4, hipMemcpyDeviceToHost, s),
                SBR_EDEVICE);
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        for (int m = 0; m < 3; m++) {
            int64_t v;
            memcpy(&v, c->so_count_host + kSoSched + 2 * m, 8);
            c->so_sched[m] += v;
        }
        // the drain is bounded by max_iter; a pool point still live past it would leave its results
        // unwritten — never returned as if solved
        if (nslots > 0 && c->so_count_host[3] != 0)
            return fail(c, SBR_EDEVICE, "social sweep: promoted points still live after the pool drain");
        if (nslots > 0) {
            const int64_t used = c->so_count_host[2];
            c->so_promoted += used < nslots ? used : nslots;
        }
        if (prof) {
            std::vector<int64_t> h((size_t)npts * 8);
            HIP_TRY(c, hipMemcpyAsync(h.data(), c->so_prof, h.size() * 8, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
            HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
            for (size_t i = 0; i < h.size(); i++) c->so_prof_acc[i & 7] += h[i];
        }
    }
    return SBR_OK;
}

size_t pool_cap(size_t cap) { return cap * 16 < (size_t)kSocialMaxCap ? cap * 16 : (size_t)kSocialMaxCap; }

// Every point at the default knot capacity with a 16× promotion pool, then the
// (rare) points that outgrew the pool or found it full, from scratch, at 4× the
// pool capacity, up to kSocialMaxCap: the results are those of an unbounded
// grid.  Finding them synchronises `s` once.
int run_social(sbr_ctx* c, hipStream_t s, const double* beta, const double* eta, double x0, const double* u,
               int64_t n_beta, int64_t n_u, double p, double kappa, double lambda, const double* cmp, int32_t n_cmp,
               double tol, int32_t max_iter, const sbr_opts& o, sbr_result_soa* out, int32_t* fp_iters,
               int64_t* rk_steps, int poll)
{
    const int64_t n_total = n_beta * n_u;
    size_t cap = o.pad > 0 ? (size_t)o.pad : (size_t)kSocialDefaultCap;
    cap = (cap + 15) & ~(size_t)15; // 16-knot lines of the wave-blocked layout
    if (cap > (size_t)kSocialMaxCap) cap = (size_t)kSocialMaxCap;
    c->so_prof_acc.assign(8, 0);
    c->so_promoted = c->so_rerun = 0;
    c->so_sched[0] = c->so_sched[1] = c->so_sched[2] = 0;
    int rc = run_social_pass(c, s, beta, eta, x0, u, n_u, p, kappa, lambda, cmp, n_cmp, tol, max_iter, o, out,
                             fp_iters, rk_steps, poll, cap, pool_cap(cap), nullptr, n_total);
    if (rc) return rc;
    std::vector<uint32_t> st((size_t)n_total);
    int64_t* dlist = nullptr;
    size_t reached = pool_cap(cap);
    while (reached < (size_t)kSocialMaxCap) {
        HIP_TRY(c, hipMemcpyAsync(st.data(), out->status, (size_t)n_total * 4, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        std::vector<int64_t> idx;
        for (int64_t g = 0; g < n_total; g++)
            if (st[(size_t)g] & SBR_KNOT_OVERFLOW) idx.push_back(g);
        if (idx.empty()) break;
        c->so_rerun += (int64_t)idx.size();
        cap = reached * 4 < (size_t)kSocialMaxCap ? reached * 4 : (size_t)kSocialMaxCap;
        reached = cap;
        if (dlist) (void)hipFree(dlist);
        dlist = nullptr;
        HIP_TRY(c, hipMalloc(&dlist, idx.size() * 8), SBR_ENOMEM);
        hipError_t e = hipMemcpyAsync(dlist, idx.data(), idx.size() * 8, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { (void)hipFree(dlist); return fail(c, SBR_EDEVICE, "overflow list", e); }
        rc = run_social_pass(c, s, beta, eta, x0, u, n_u, p, kappa, lambda, cmp, n_cmp, tol, max_iter, o, out,
                             fp_iters, rk_steps, poll, cap, cap, dlist, (int64_t)idx.size());
        if (rc) { (void)hipFree(dlist); return rc; }
    }
    if (dlist) {
        (void)hipStreamSynchronize(s);
        (void)hipFree(dlist);
    }
    return SBR_OK;
}
}  // namespace

extern "C" {

int sbr_sweep_social_dev(sbr_ctx* c, void* stream, const double* beta, const double* eta, double x0, const double* u,
                         int64_t n_beta, int64_t n_u, double p, double kappa, double lambda, const double* cmp_grid,
                         int32_t n_cmp, double tol, int32_t max_iter, const sbr_opts* opts, sbr_result_soa* out,
                         int32_t* fp_iters, int64_t* rk_steps)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    SBR_SINGLE_DEVICE(c);
    int rc = social_checks(c, beta, eta, u, n_beta, n_u, x0, p, kappa, lambda, cmp_grid, n_cmp, tol, max_iter, out);
    if (rc) return rc;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    sbr_opts o = resolve(opts);
    return fenced(c, stream, true, [&](hipStream_t s) {
        return run_social(c, s, beta, eta, x0, u, n_beta, n_u, p, kappa, lambda, cmp_grid, n_cmp, tol, max_iter, o,
                          out, fp_iters, rk_steps, 0);
    });
}

int sbr_social_point_paths(sbr_ctx* c, double beta, double eta, double x0, double u, double p, double kappa,
                           double lambda, const double* cmp_grid, int32_t n_cmp, double tol, int32_t max_iter,
                           const sbr_opts* opts, double* res, uint32_t* status, int32_t* fp_iters, double* t,
                           double* G, double* aw_old, int64_t cap, int64_t* n_knots)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    SBR_ON_RANK0(c, sbr_social_point_paths(c, beta, eta, x0, u, p, kappa, lambda, cmp_grid, n_cmp, tol, max_iter, opts, res, status, fp_iters, t, G, aw_old, cap, n_knots));
    if (!c || !res || !status || !t || !G || cap <= 0 || cap > (int64_t(1) << 30)) return SBR_EARG;
    double* d = nullptr;
    const size_t kc = (size_t)cap;
    HIP_TRY(c, hipMalloc(&d, (3 * kc + 8) * 8), SBR_ENOMEM);
    c->so_path_t = d;
    c->so_path_G = d + kc;
    c->so_path_aw = aw_old ? d + 2 * kc : nullptr;
    c->so_path_n = (int32_t*)(d + 3 * kc);
    c->so_path_cap = (int32_t)cap;
    hipError_t e = hipMemset(c->so_path_n, 0, 4);
    double xi, tin, tout, aw, tl;
    int64_t steps = 0;
    sbr_result_soa out{&xi, &tin, &tout, &aw, &tl, status, nullptr};
    int rc = e == hipSuccess ? sbr_sweep_social(c, &beta, &eta, x0, &u, 1, 1, p, kappa, lambda, cmp_grid, n_cmp, tol,
                                                max_iter, opts, &out, fp_iters, &steps)
                             : fail(c, SBR_EDEVICE, "hipMemset", e);
    c->so_path_t = c->so_path_G = c->so_path_aw = nullptr;
    c->so_path_n = nullptr;
    c->so_path_cap = 0;
    int32_t n = 0;
    if (rc == SBR_OK) {
        e = hipMemcpy(&n, d + 3 * kc, 4, hipMemcpyDeviceToHost);
        const int64_t m = n < 0 ? 0 : n;
        if (e == hipSuccess && m > 0) e = hipMemcpy(t, d, (size_t)m * 8, hipMemcpyDeviceToHost);
        if (e == hipSuccess && m > 0) e = hipMemcpy(G, d + kc, (size_t)m * 8, hipMemcpyDeviceToHost);
        if (e == hipSuccess && m > 0 && aw_old) e = hipMemcpy(aw_old, d + 2 * kc, (size_t)m * 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(c, SBR_EDEVICE, "social path copy", e);
    }
    (void)hipFree(d);
    if (rc) return rc;
    res[0] = xi; res[1] = tin; res[2] = tout; res[3] = aw; res[4] = tl;
    if (n_knots) *n_knots = n < 0 ? -n : n;
    if (n < 0) return fail(c, SBR_EARG, "path capacity too small");
    return SBR_OK;
}

static int multi_sweep_social(sbr_ctx* c, const Inputs& in, double x0, int64_t n_beta, int64_t n_u, double p,
                              double kappa, double lambda, int32_t n_cmp, double tol, int32_t max_iter,
                              const sbr_opts& o, sbr_result_soa* out, int32_t* fp_iters, int64_t* rk_steps)
{
    std::vector<FieldSpec> fs = result_fields(out);
    fs.push_back({fp_iters, 4, 1});
    fs.push_back({rk_steps, 8, 1});
    auto run = [&](sbr_ctx* kid, hipStream_t s, int64_t nc, const DevInputs& d, const std::vector<void*>& f) -> int {
        sbr_result_soa ro = rank_results(f);
        return sbr_sweep_social_dev(kid, s, d[0], d[1], x0, d[2], nc, n_u, p, kappa, lambda, d[3], n_cmp, tol,
                                    max_iter, &o, &ro, (int32_t*)f[7], (int64_t*)f[8]);
    };
    return fan_out(c, in, n_beta, n_u, fs, o, run);
}

int sbr_sweep_social(sbr_ctx* c, const double* beta, const double* eta, double x0, const double* u, int64_t n_beta,
                     int64_t n_u, double p, double kappa, double lambda, const double* cmp_grid, int32_t n_cmp,
                     double tol, int32_t max_iter, const sbr_opts* opts, sbr_result_soa* out, int32_t* fp_iters,
                     int64_t* rk_steps)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    int rc = social_checks(c, beta, eta, u, n_beta, n_u, x0, p, kappa, lambda, cmp_grid, n_cmp, tol, max_iter, out);
    if (!rc) rc = check_positive(c, n_beta, {beta, eta}, "ArgumentError: beta/eta must be positive");
    if (!rc) rc = check_u(c, u, n_u);
    if (rc) return rc;
    const Inputs in{cols(beta), cols(eta), shared(u, (size_t)n_u), cols(cmp_grid, (size_t)n_cmp)};
    if (c->multi)
        return multi_sweep_social(c, in, x0, n_beta, n_u, p, kappa, lambda, n_cmp, tol, max_iter, resolve(opts), out,
                                  fp_iters, rk_steps);
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    sbr_opts o = resolve(opts);
    const size_t np = (size_t)(n_beta * n_u);
    void* dres;
    rc = ensure_io(c, in, (size_t)n_beta, result_bytes(np, true, true), &dres);
    if (rc) return rc;
    const auto d = in.dev(c->stage, (size_t)n_beta);
    int64_t* dsteps;
    int32_t* dfp;
    const sbr::ResultSoA rs = carve_results(dres, np, &dsteps, &dfp);
    return fenced(c, nullptr, false, [&](hipStream_t s) -> int {
        rc = in.stage(c, c->stage, (size_t)n_beta, s);
        if (rc) return rc;
        sbr_result_soa r{rs.xi, rs.tau_in_unc, rs.tau_out_unc, rs.aw_max, rs.tol, rs.status, rs.iters};
        rc = run_social(c, s, d[0], d[1], x0, d[2], n_beta, n_u, p, kappa, lambda, d[3], n_cmp, tol, max_iter, o, &r, dfp,
                        dsteps, 8);
        if (!rc) rc = copy_out(c, s, out, rs, np);
        if (!rc) rc = copy_out(c, s, {{fp_iters, dfp, np * 4}, {rk_steps, dsteps, np * 8}});
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        return SBR_OK;
    });
}

}  // extern "C"
