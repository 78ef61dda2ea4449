// sbr_capi_hetero.hip — the heterogeneity extension's entry points of the C API: its learning
// workspaces, sbr_learn_hetero, the sweeps (single, pipelined batch, host-pointer), the one-point
// paths and the product with the economic parameters (sbr_sweep_hetero_econ).
#include "sbr_hostio.h"

using namespace sbr_capi;

namespace sbr_capi {

static void free_hetero_bufs(sbr::HeteroBufs& H, size_t& col, size_t& cap, size_t& K)
{
    free_dev(H.t, H.G, H.hr, H.hrI, H.n_knots, H.n_tau, H.n_le, H.status, H.n_accept, H.n_reject);
    H = sbr::HeteroBufs{};
    col = cap = K = 0;
}

static void free_hetero_econ(sbr_ctx* c)
{
    free_dev(c->he_hr, c->he_hrI, c->he_cnt);
    c->he_rows = c->he_ld = 0;
}

void free_hetero(sbr_ctx* c)
{
    free_hetero_bufs(c->H, c->hs_col, c->hs_cap, c->hs_K);
    free_hetero_bufs(c->H2, c->hs2_col, c->hs2_cap, c->hs2_K);
    free_hetero_econ(c);
}

// sbr_sweep_hetero_econ's class rows: `rows` (classes per chunk × columns) of K hazard rows and K
// running-integral rows (ld = K × the learning stride doubles each) and three words
static int ensure_hetero_econ(sbr_ctx* c, size_t rows, size_t ld)
{
    if (rows <= c->he_rows && ld == c->he_ld) return SBR_OK;
    free_hetero_econ(c);
    const int rc = alloc_dev(c, {{c->he_hr, rows * ld * sizeof(double)}, {c->he_hrI, rows * ld * sizeof(double)},
                                 {c->he_cnt, rows * 3 * sizeof(int32_t)}});
    if (rc) return rc;
    c->he_rows = rows;
    c->he_ld = ld;
    return SBR_OK;
}

static int ensure_hetero_bufs(sbr_ctx* c, sbr::HeteroBufs& H, size_t& hcol, size_t& hcap, size_t& hK, size_t n_col,
                              size_t cap, size_t K)
{
    if (n_col <= hcol && cap == hcap && K == hK) return SBR_OK;
    free_hetero_bufs(H, hcol, hcap, hK);
    const size_t ld = learn_ld(cap); // padded rows, as for the baseline workspaces
    const size_t row = n_col * ld * 8;
    const int rc = alloc_dev(c, {{H.t, row}, {H.G, row * K}, {H.hr, row * K}, {H.hrI, row * K},
                                 {H.n_knots, n_col * 4}, {H.n_tau, n_col * 4}, {H.n_le, n_col * 4},
                                 {H.status, n_col * 4}, {H.n_accept, n_col * 4}, {H.n_reject, n_col * 4}});
    if (rc) return rc;
    H.cap = (int32_t)ld;
    H.lim = (int32_t)cap;
    hcol = n_col;
    hcap = cap;
    hK = K;
    return SBR_OK;
}

int ensure_hetero(sbr_ctx* c, size_t n_col, size_t cap, size_t K)
{
    return ensure_hetero_bufs(c, c->H, c->hs_col, c->hs_cap, c->hs_K, n_col, cap, K);
}

// path mode's rows (AW_total, then AW_OUT_k and AW_IN_k, each n long) into the caller's
// aw_total [n] and aw_groups [2K][cap]; NaN rows without a run (get_AW_hetero returns nothing)
void copy_hetero_paths(const double* src, bool run, int K, int64_t n, int64_t cap, double* aw_total,
                       double* aw_groups)
{
    for (int r = 0; r <= 2 * K; r++) {
        double* dst = r == 0 ? aw_total : (aw_groups ? aw_groups + (size_t)(r - 1) * cap : nullptr);
        if (!dst) continue;
        if (run) memcpy(dst, src + (size_t)r * n, (size_t)n * 8);
        else for (int64_t i = 0; i < n; i++) dst[i] = NAN;
    }
}

}  // namespace sbr_capi

// LearningParametersHetero checks (heterogeneity_model.jl:33-41) of a sweep's K weights and
// n_col × K learning rates
static int hetero_params_check(sbr_ctx* c, int32_t K, const double* betas, const double* dist, int64_t n_col)
{
    double dsum = 0.0;
    for (int k = 0; k < K; k++) {
        if (!(dist[k] >= 0.0)) return fail(c, SBR_EARG, "ArgumentError: distribution weights must be non-negative");
        dsum = dsum + dist[k];
    }
    if (!(fabs(dsum - 1.0) < 1e-10)) return fail(c, SBR_EARG, "ArgumentError: distribution must sum to 1");
    return check_positive(c, n_col * K, {betas}, "ArgumentError: all learning rates must be positive");
}

extern "C" {

int sbr_learn_hetero(sbr_ctx* c, int32_t K, const double* betas, const double* dist, const double* t_end, double x0,
                     int64_t n_col, const sbr_opts* opts, double* t_out, double* G_out, int64_t cap, int32_t* n_knots,
                     uint32_t* status)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    SBR_ON_RANK0(c, sbr_learn_hetero(c, K, betas, dist, t_end, x0, n_col, opts, t_out, G_out, cap, n_knots, status));
    if (!c || !betas || !dist || !t_end || n_col <= 0 || n_col > (1 << 30) || cap <= 0) return SBR_EARG;
    if (!hetero_K_ok(K)) return fail(c, SBR_EARG, kHeteroKMsg);
    int rc = hetero_params_check(c, K, betas, dist, n_col);
    if (!rc) rc = check_positive(c, n_col, {t_end}, "ArgumentError: End time must be greater than start time");
    if (rc) return rc;
    if (!(x0 >= 0.0)) return fail(c, SBR_EARG, "ArgumentError: Initial condition must be non-negative");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    sbr_opts o = resolve(opts);
    if (cap < o.knot_capacity) o.knot_capacity = (int32_t)cap;
    rc = ensure_hetero(c, (size_t)n_col, (size_t)o.knot_capacity, (size_t)K);
    if (rc) return rc;
    const Inputs in{cols(betas, (size_t)K), shared(dist, (size_t)K), cols(t_end)};
    rc = ensure_stage(c, in.bytes((size_t)n_col));
    if (rc) return rc;
    const auto d = in.dev(c->stage, (size_t)n_col);
    return fenced(c, nullptr, false, [&](hipStream_t s) -> int {
        rc = in.stage(c, c->stage, (size_t)n_col, s);
        if (rc) return rc;
        // the knot grid runs to t_end whatever η is (the learning stage of a sweep streams
        // the hazard for η alongside; here η = t_end only sizes that unused stream)
        sbr::LearnArgs la{x0, o.ode_reltol, o.ode_abstol, 0.5, 1.0, o.ode_maxiters, (int32_t)n_col, 0, 0};
        sbr::HeteroEqArgs ea{0.5, 1e-12, 1, o.hetero_max_iters, het_lds(c), 0, 0, nullptr};
        sbr::ResultSoA r{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        HIP_TRY(c, sbr::launch_hetero(K, d[0], d[1], d[2], d[2], nullptr, la, ea, c->H, r, nullptr, nullptr, s, 0),
                SBR_EDEVICE);
        const size_t w = (size_t)o.knot_capacity, ld = (size_t)c->H.cap;
        if (t_out)
            HIP_TRY(c, hipMemcpy2DAsync(t_out, (size_t)cap * 8, c->H.t, ld * 8, w * 8, (size_t)n_col, hipMemcpyDeviceToHost, s),
                    SBR_EDEVICE);
        if (G_out)
            HIP_TRY(c, hipMemcpy2DAsync(G_out, (size_t)cap * K * 8, c->H.G, ld * K * 8, w * K * 8, (size_t)n_col,
                                        hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        if (n_knots) HIP_TRY(c, hipMemcpyAsync(n_knots, c->H.n_knots, (size_t)n_col * 4, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        if (status) HIP_TRY(c, hipMemcpyAsync(status, c->H.status, (size_t)n_col * 4, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        strip_hazard_status(status, n_col);
        return SBR_OK;
    });
}

int sbr_sweep_hetero_dev(sbr_ctx* c, void* stream, int32_t K, const double* betas, const double* dist,
                         const double* eta, const double* t_end, double x0, const double* u, int64_t n_col,
                         int64_t n_u, double p, double kappa, double lambda, const sbr_opts* opts,
                         sbr_result_soa* out, double* tau_in, double* tau_out)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    SBR_SINGLE_DEVICE(c);
    if (!c || !out || !out->xi || !out->aw_max || !out->tol || !out->status) return SBR_EARG;
    if (!hetero_K_ok(K)) return fail(c, SBR_EARG, kHeteroKMsg);
    if (n_col <= 0 || n_u <= 0 || n_col > (1 << 30) || n_u > (1 << 30)) return fail(c, SBR_EARG, "grid size");
    if (!scalars_valid(x0, p, kappa, lambda)) return fail(c, SBR_EARG, "ArgumentError: x0/p/kappa/lambda");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    sbr_opts o = resolve(opts);
    int rc = ensure_hetero(c, (size_t)n_col, (size_t)o.knot_capacity, (size_t)K);
    if (rc) return rc;
    return fenced(c, stream, true, [&](hipStream_t s) -> int {
        sbr::LearnArgs la{x0, o.ode_reltol, o.ode_abstol, p, lambda, o.ode_maxiters, (int32_t)n_col, 0, 0};
        sbr::HeteroEqArgs ea{kappa, 1e-12, (int32_t)n_u, o.hetero_max_iters, het_lds(c),
                             (o.flags & SBR_FLAG_EXHAUSTIVE) ? 1 : 0, (o.flags >> 8) & 7, c->het_aw_path};
        sbr::ResultSoA r{out->xi, nullptr, nullptr, out->aw_max, out->tol, out->status, out->iters};
        hipEvent_t t0 = tstart(c, s);
        HIP_TRY(c, sbr::launch_hetero(K, betas, dist, eta, t_end, u, la, ea, c->H, r, tau_in, tau_out, s, 0), SBR_EDEVICE);
        tend(c, s, 0, t0);
        t0 = tstart(c, s);
        HIP_TRY(c, sbr::launch_hetero(K, betas, dist, eta, t_end, u, la, ea, c->H, r, tau_in, tau_out, s, 1, hetero_wide(o)),
                SBR_EDEVICE);
        tend(c, s, 1, t0);
        return SBR_OK;
    });
}

int sbr_sweep_hetero_batch_dev(sbr_ctx* c, void* stream, int64_t n_batch, int32_t K, const double* betas,
                               const double* dist, const double* eta, const double* t_end, double x0, const double* u,
                               int64_t n_col, int64_t n_u, double p, double kappa, double lambda, const sbr_opts* opts,
                               sbr_result_soa* out, double* tau_in, double* tau_out)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    SBR_SINGLE_DEVICE(c);
    if (!c || !out || !out->xi || !out->aw_max || !out->tol || !out->status || !betas || !dist || !eta || !t_end || !u)
        return SBR_EARG;
    if (!hetero_K_ok(K)) return fail(c, SBR_EARG, kHeteroKMsg);
    if (n_batch <= 0 || n_col <= 0 || n_u <= 0 || n_col > (1 << 30) || n_u > (1 << 30))
        return fail(c, SBR_EARG, "grid size");
    if (!scalars_valid(x0, p, kappa, lambda)) return fail(c, SBR_EARG, "ArgumentError: x0/p/kappa/lambda");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    sbr_opts o = resolve(opts);
    const size_t cap = (size_t)o.knot_capacity;
    int rc = ensure_hetero(c, (size_t)n_col, cap, (size_t)K);
    if (!rc && n_batch > 1) rc = ensure_hetero_bufs(c, c->H2, c->hs2_col, c->hs2_cap, c->hs2_K, (size_t)n_col, cap, (size_t)K);
    if (!rc) rc = ensure_pipe_streams(c);
    if (rc) return rc;
    return fenced(c, stream, true, [&](hipStream_t s) -> int {
        sbr::LearnArgs la{x0, o.ode_reltol, o.ode_abstol, p, lambda, o.ode_maxiters, (int32_t)n_col, 0, 0};
        sbr::HeteroEqArgs ea{kappa, 1e-12, (int32_t)n_u, o.hetero_max_iters, het_lds(c),
                             (o.flags & SBR_FLAG_EXHAUSTIVE) ? 1 : 0, (o.flags >> 8) & 7, nullptr};
        const size_t np = (size_t)n_col * (size_t)n_u;
        HIP_TRY(c, hipEventRecord(c->ev_in, s), SBR_EDEVICE);
        for (int k = 0; k < 2; k++) HIP_TRY(c, hipStreamWaitEvent(c->lstream[k], c->ev_in, 0), SBR_EDEVICE);
        for (int64_t k = 0; k < n_batch; k++) {
            const int slot = (int)(k & 1);
            hipStream_t ls = c->lstream[slot];
            const sbr::HeteroBufs& H = slot ? c->H2 : c->H;
            const double* bk = betas + k * n_col * K;
            const double* ek = eta + k * n_col;
            const double* tk = t_end + k * n_col;
            // the slot's previous reader (equilibrium of batch k - 2) must be done
            if (k >= 2) HIP_TRY(c, hipStreamWaitEvent(ls, c->ev_eq[slot], 0), SBR_EDEVICE);
            hipEvent_t t0 = tstart(c, ls);
            sbr::ResultSoA r{out->xi + k * np, nullptr, nullptr, out->aw_max + k * np, out->tol + k * np,
                             out->status + k * np, out->iters ? out->iters + k * np : nullptr};
            double* ti = tau_in ? tau_in + k * np * K : nullptr;
            double* to = tau_out ? tau_out + k * np * K : nullptr;
            HIP_TRY(c, sbr::launch_hetero(K, bk, dist, ek, tk, u, la, ea, H, r, ti, to, ls, 0), SBR_EDEVICE);
            tend(c, ls, 0, t0);
            HIP_TRY(c, hipEventRecord(c->ev_learned[slot], ls), SBR_EDEVICE);
            HIP_TRY(c, hipStreamWaitEvent(s, c->ev_learned[slot], 0), SBR_EDEVICE);
            t0 = tstart(c, s);
            HIP_TRY(c, sbr::launch_hetero(K, bk, dist, ek, tk, u, la, ea, H, r, ti, to, s, 1, hetero_wide(o)), SBR_EDEVICE);
            tend(c, s, 1, t0);
            HIP_TRY(c, hipEventRecord(c->ev_eq[slot], s), SBR_EDEVICE);
        }
        return SBR_OK;
    });
}

int sbr_hetero_point_paths(sbr_ctx* c, int32_t K, const double* betas, const double* dist, double eta, double t_end,
                           double x0, double u, double p, double kappa, double lambda, const sbr_opts* opts,
                           double* res, uint32_t* status, double* tau_in, double* tau_out, double* t, double* G,
                           double* aw_total, double* aw_groups, int64_t cap, int64_t* n_knots)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    SBR_ON_RANK0(c, sbr_hetero_point_paths(c, K, betas, dist, eta, t_end, x0, u, p, kappa, lambda, opts, res, status, tau_in, tau_out, t, G, aw_total, aw_groups, cap, n_knots));
    if (!c || !res || !status || !betas || !dist) return SBR_EARG;
    if (!hetero_K_ok(K)) return fail(c, SBR_EARG, kHeteroKMsg);
    double dsum = 0.0;
    for (int k = 0; k < K; k++) {
        if (!(dist[k] >= 0.0)) return fail(c, SBR_EARG, "ArgumentError: distribution weights must be non-negative");
        if (!(betas[k] > 0.0)) return fail(c, SBR_EARG, "ArgumentError: all learning rates must be positive");
        dsum = dsum + dist[k];
    }
    if (!(fabs(dsum - 1.0) < 1e-10)) return fail(c, SBR_EARG, "ArgumentError: distribution must sum to 1");
    if (!scalars_valid(x0, p, kappa, lambda) || !(eta > 0) || !(t_end > 0) || !(u >= 0))
        return fail(c, SBR_EARG, "ArgumentError");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    sbr_opts o = resolve(opts);
    const size_t kc = (size_t)o.knot_capacity;
    int rc = ensure_stage(c, (2 * (size_t)K + 3 + 4 + 2 * (size_t)K + (1 + 2 * (size_t)K) * kc) * 8 + 512);
    if (rc) return rc;
    double* d = (double*)c->stage;
    double *dbeta = d, *ddist = d + K, *deta = d + 2 * K, *dtend = deta + 1, *du = dtend + 1;
    double* dres = du + 1; // xi, aw, tol
    uint32_t* dst = (uint32_t*)(dres + 3);
    double* dtin = dres + 4;
    double* dtout = dtin + K;
    double* dpath = dtout + K;
    return fenced(c, nullptr, false, [&](hipStream_t s) -> int {
        const double hin[3] = {eta, t_end, u};
        HIP_TRY(c, hipMemcpyAsync(dbeta, betas, (size_t)K * 8, hipMemcpyHostToDevice, s), SBR_EDEVICE);
        HIP_TRY(c, hipMemcpyAsync(ddist, dist, (size_t)K * 8, hipMemcpyHostToDevice, s), SBR_EDEVICE);
        HIP_TRY(c, hipMemcpyAsync(deta, hin, 24, hipMemcpyHostToDevice, s), SBR_EDEVICE);
        sbr_result_soa r{dres, nullptr, nullptr, dres + 1, dres + 2, dst, nullptr};
        c->het_aw_path = dpath;
        rc = sbr_sweep_hetero_dev(c, s, K, dbeta, ddist, deta, dtend, x0, du, 1, 1, p, kappa, lambda, &o, &r, dtin, dtout);
        c->het_aw_path = nullptr;
        if (rc) return rc;
        double* dgrp = dpath + kc; // AW_OUT_k / AW_IN_k rows of stride kc
        if (aw_groups)
            HIP_TRY(c, sbr::launch_hetero_aw_groups(K, c->H.t, c->H.G, c->H.n_knots, (int)kc, dres, dtin, dtout, dst,
                                                    dgrp, kc, s), SBR_EDEVICE);
        int32_t n = 0;
        HIP_TRY(c, hipMemcpyAsync(res, dres, 24, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        HIP_TRY(c, hipMemcpyAsync(status, dst, 4, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        if (tau_in) HIP_TRY(c, hipMemcpyAsync(tau_in, dtin, (size_t)K * 8, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        if (tau_out) HIP_TRY(c, hipMemcpyAsync(tau_out, dtout, (size_t)K * 8, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        HIP_TRY(c, hipMemcpyAsync(&n, c->H.n_knots, 4, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        if (n_knots) *n_knots = n;
        if (n > cap) return fail(c, SBR_EARG, "path capacity too small");
        if (t) HIP_TRY(c, hipMemcpy(t, c->H.t, (size_t)n * 8, hipMemcpyDeviceToHost), SBR_EDEVICE);
        if (G) HIP_TRY(c, hipMemcpy(G, c->H.G, (size_t)n * K * 8, hipMemcpyDeviceToHost), SBR_EDEVICE);
        if (aw_total || aw_groups) {
            const bool run = (*status & SBR_RUN) != 0;
            std::vector<double> h(run ? (size_t)n * (1 + 2 * K) : 0);
            for (int r = 0; run && r <= 2 * K; r++)
                HIP_TRY(c, hipMemcpy(h.data() + (size_t)r * n, r == 0 ? dpath : dgrp + (size_t)(r - 1) * kc,
                                     (size_t)n * 8, hipMemcpyDeviceToHost), SBR_EDEVICE);
            copy_hetero_paths(h.data(), run, K, n, cap, aw_total, aw_groups);
        }
        return SBR_OK;
    });
}

static int multi_sweep_hetero(sbr_ctx* c, const Inputs& in, int32_t K, double x0, int64_t n_col, int64_t n_u,
                              double p, double kappa, double lambda, const sbr_opts& o, sbr_result_soa* out,
                              double* tau_in, double* tau_out)
{
    const std::vector<FieldSpec> fs = {{out->xi, 8, 1},    {out->aw_max, 8, 1}, {out->tol, 8, 1},
                                       {out->status, 4, 1}, {out->iters, 4, 1},  {tau_in, 8, (size_t)K},
                                       {tau_out, 8, (size_t)K}};
    auto run = [&](sbr_ctx* kid, hipStream_t s, int64_t nc, const DevInputs& d, const std::vector<void*>& f) -> int {
        sbr_result_soa ro{(double*)f[0], nullptr, nullptr, (double*)f[1], (double*)f[2], (uint32_t*)f[3],
                          (int32_t*)f[4]};
        return sbr_sweep_hetero_dev(kid, s, K, d[0], d[1], d[2], d[3], x0, d[4], nc, n_u, p, kappa, lambda, &o, &ro,
                                    (double*)f[5], (double*)f[6]);
    };
    return fan_out(c, in, n_col, n_u, fs, o, run);
}

int sbr_sweep_hetero(sbr_ctx* c, int32_t K, const double* betas, const double* dist, const double* eta,
                     const double* t_end, double x0, const double* u, int64_t n_col, int64_t n_u, double p,
                     double kappa, double lambda, const sbr_opts* opts, sbr_result_soa* out, double* tau_in,
                     double* tau_out)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    if (!c || !out || !betas || !dist || !eta || !t_end || !u) return SBR_EARG;
    if (!hetero_K_ok(K)) return fail(c, SBR_EARG, kHeteroKMsg); // before dist[0 .. K) is read
    if (n_col <= 0 || n_u <= 0) return fail(c, SBR_EARG, "grid size");
    int rc = hetero_params_check(c, K, betas, dist, n_col);
    if (!rc) rc = check_positive(c, n_col, {eta, t_end}, "ArgumentError: eta/t_end");
    if (!rc) rc = check_u(c, u, n_u);
    if (rc) return rc;
    const Inputs in{cols(betas, (size_t)K), shared(dist, (size_t)K), cols(eta), cols(t_end), shared(u, (size_t)n_u)};
    if (c->multi)
        return multi_sweep_hetero(c, in, K, x0, n_col, n_u, p, kappa, lambda, resolve(opts), out, tau_in, tau_out);
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    // the result block: xi, aw_max, tol | status, iters | tau_in, tau_out (K per point)
    const size_t np = (size_t)n_col * (size_t)n_u;
    void* dres;
    rc = ensure_io(c, in, (size_t)n_col, np * (3 * 8 + 2 * 4 + 2 * (size_t)K * 8), &dres);
    if (rc) return rc;
    const auto d = in.dev(c->stage, (size_t)n_col);
    double *dxi = (double*)dres, *daw = dxi + np, *dtol = daw + np;
    uint32_t* dst = (uint32_t*)(dtol + np);
    int32_t* dit = (int32_t*)(dst + np);
    double* dtin = (double*)(dit + np);
    double* dtout = dtin + np * K;
    return fenced(c, nullptr, false, [&](hipStream_t s) -> int {
        rc = in.stage(c, c->stage, (size_t)n_col, s);
        if (rc) return rc;
        sbr_result_soa r{dxi, nullptr, nullptr, daw, dtol, dst, dit};
        rc = sbr_sweep_hetero_dev(c, s, K, d[0], d[1], d[2], d[3], x0, d[4], n_col, n_u, p, kappa, lambda, opts, &r,
                                  tau_in ? dtin : nullptr, tau_out ? dtout : nullptr);
        if (!rc)
            rc = copy_out(c, s, {{out->xi, dxi, np * 8}, {out->aw_max, daw, np * 8}, {out->tol, dtol, np * 8},
                                 {out->status, dst, np * 4}, {out->iters, dit, np * 4},
                                 {tau_in, dtin, np * K * 8}, {tau_out, dtout, np * K * 8}});
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        return SBR_OK;
    });
}

}  // extern "C"

// ---------------------------------------------------------------------------
// sbr_sweep_hetero_econ: K groups × p × λ × κ × u
// ---------------------------------------------------------------------------
namespace {

// workspace bytes (sbr.h: sbr_sweep_hetero_econ): a column's learning rows, and what a (column,
// class) pair counts for against the budget
size_t hetero_learn_bytes(size_t cap, size_t K) { return (1 + 3 * K) * cap * sizeof(double) + 6 * sizeof(int32_t); }
size_t hetero_class_bytes(size_t cap, size_t K) { return 2 * K * cap * sizeof(double) + 3 * sizeof(int32_t); }

// All in stream order on s: the learning launch of sbr_sweep_hetero once (its streamed hazard rows
// are not read), then per chunk of hazard classes (p[a], λ[b]) the hazard launch — one wave per
// (column, class) — and the equilibrium launches over the κ × u planes.  A chunk's hazards start
// after the previous chunk's equilibria (they share the class rows); no host synchronisation.
// Timing records: kind 0 = the learning launch, kind 1 = the hazard and equilibrium launches.
int run_hetero_econ(sbr_ctx* c, hipStream_t s, int32_t K, const double* betas, const double* dist, const double* eta,
                    const double* t_end, double x0, const double* u, int64_t n_col, int64_t n_u, const double* p,
                    int64_t n_p, const double* lambda, int64_t n_lambda, const double* kappa, int64_t n_kappa,
                    const sbr_opts& o, const sbr::ResultSoA& out, double* tin, double* tout)
{
    const size_t cap = (size_t)o.knot_capacity;
    const int64_t n_class = n_p * n_lambda, plane = n_kappa * n_u;
    size_t freeb = 0, total = 0;
    (void)hipMemGetInfo(&freeb, &total);
    const size_t held = c->hs_col * hetero_learn_bytes(c->hs_cap, c->hs_K) + 2 * c->he_rows * c->he_ld * sizeof(double);
    const double budget = c->ec_budget > 0 ? (double)c->ec_budget : 0.4 * (double)(freeb + held);
    const double left = budget - (double)n_col * (double)hetero_learn_bytes(cap, (size_t)K);
    int64_t per = left > 0.0
                      ? (int64_t)std::min(left / ((double)n_col * (double)hetero_class_bytes(cap, (size_t)K)), 65535.0)
                      : 1;
    per = std::max<int64_t>(1, std::min<int64_t>(per, n_class));
    // one equilibrium launch holds the chunk's (column, class) pairs × the plane's tiles
    while (per > 1 && !sbr::hetero_econ_grid(n_col, per, plane, 64)) per = (per + 1) / 2;
    if (!sbr::hetero_econ_grid(n_col, per, plane, 64)) return fail(c, SBR_EARG, "grid size");
    int rc = ensure_hetero(c, (size_t)n_col, cap, (size_t)K);
    if (rc) return rc;
    const sbr::HeteroBufs& L = c->H;
    const size_t ld = (size_t)K * (size_t)L.cap;
    // a workspace that already holds enough rows of this stride is used as it is
    for (;;) {
        rc = ensure_hetero_econ(c, (size_t)(per * n_col), ld);
        if (rc == SBR_OK) break;
        free_hetero_econ(c);
        if (per == 1) return rc;
        (void)hipGetLastError(); // the failed hipMalloc's error must not surface at the next launch check
        per = (per + 1) / 2;
    }
    // p and λ are per class: the learning launch's streamed hazard (any valid pair) is a by-product
    sbr::LearnArgs la{x0, o.ode_reltol, o.ode_abstol, 0.5, 1.0, o.ode_maxiters, (int32_t)n_col, 0, 0};
    const int slab = c->he_slab > 0 ? std::min<int>(c->he_slab, het_lds(c)) : het_lds(c);
    sbr::HeteroEqArgs ea{0.0, 1e-12, (int32_t)plane, o.hetero_max_iters, slab, (o.flags & SBR_FLAG_EXHAUSTIVE) ? 1 : 0,
                         (o.flags >> 8) & 7, nullptr};
    hipEvent_t t0 = tstart(c, s);
    HIP_TRY(c, sbr::launch_hetero(K, betas, dist, eta, t_end, u, la, ea, L, out, tin, tout, s, 0), SBR_EDEVICE);
    tend(c, s, 0, t0);
    t0 = tstart(c, s);
    int launches = 0;
    for (int64_t g0 = 0; g0 < n_class; g0 += per) {
        const int64_t ng = std::min<int64_t>(per, n_class - g0);
        const size_t rows = (size_t)(per * n_col);
        const sbr::HeteroEconArgs e{p, lambda, kappa, (int32_t)n_p, (int32_t)n_lambda, (int32_t)n_kappa, (int32_t)n_u,
                                    (int32_t)n_col, (int32_t)g0, (int32_t)ng, c->he_hr, c->he_hrI, c->he_cnt,
                                    c->he_cnt + rows, (uint32_t*)(c->he_cnt + 2 * rows)};
        HIP_TRY(c, sbr::launch_hazard_hetero_econ(K, betas, dist, eta, L, e, s), SBR_EDEVICE);
        HIP_TRY(c, sbr::launch_equilibrium_hetero_econ(K, dist, eta, t_end, u, ea, L, e, out, tin, tout, s,
                                                       hetero_wide(o)), SBR_EDEVICE);
        launches += 3;
    }
    tend(c, s, 1, t0, launches);
    return SBR_OK;
}

// the checks sbr_sweep_hetero_econ and sbr_sweep_hetero_econ_dev share, before any array is looked at
int hetero_econ_checks(sbr_ctx* c, const sbr_opts* opts, int32_t K, double x0, int64_t n_col, int64_t n_u, int64_t n_p,
                       int64_t n_lambda, int64_t n_kappa)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    if (!c) return SBR_EARG;
    if (!hetero_K_ok(K)) return fail(c, SBR_EARG, kHeteroKMsg);
    const int64_t lim = 1 << 30;
    if (n_col <= 0 || n_u <= 0 || n_p <= 0 || n_lambda <= 0 || n_kappa <= 0 || n_col > lim || n_u > lim ||
        n_p > lim || n_lambda > lim || n_kappa > lim || n_p * n_lambda > lim || n_kappa * n_u > lim)
        return fail(c, SBR_EARG, "grid size");
    if (!(x0 >= 0.0)) return fail(c, SBR_EARG, "ArgumentError: Initial condition must be non-negative");
    return SBR_OK;
}

// K groups × p × λ × κ × u on n devices: column i to rank i mod N with its n_p·n_lambda·n_kappa·n_u
// points (and K buffers per point), the four axes to every rank
int multi_sweep_hetero_econ(sbr_ctx* c, const Inputs& in, int32_t K, double x0, int64_t n_col, int64_t n_u,
                            int64_t n_p, int64_t n_lambda, int64_t n_kappa, const sbr_opts& o, sbr_result_soa* out,
                            double* tau_in, double* tau_out)
{
    const std::vector<FieldSpec> fs = {{out->xi, 8, 1},    {out->aw_max, 8, 1}, {out->tol, 8, 1},
                                       {out->status, 4, 1}, {out->iters, 4, 1},  {tau_in, 8, (size_t)K},
                                       {tau_out, 8, (size_t)K}};
    auto run = [&](sbr_ctx* kid, hipStream_t s, int64_t nc, const DevInputs& d, const std::vector<void*>& f) -> int {
        sbr_result_soa ro{(double*)f[0], nullptr, nullptr, (double*)f[1], (double*)f[2], (uint32_t*)f[3],
                          (int32_t*)f[4]};
        return sbr_sweep_hetero_econ_dev(kid, s, K, d[0], d[1], d[2], d[3], x0, d[4], nc, n_u, d[5], n_p, d[6],
                                         n_lambda, d[7], n_kappa, &o, &ro, (double*)f[5], (double*)f[6]);
    };
    return fan_out(c, in, n_col, n_p * n_lambda * n_kappa * n_u, fs, o, run);
}

}  // namespace

extern "C" {

int sbr_sweep_hetero_econ_dev(sbr_ctx* c, void* stream, int32_t K, const double* betas, const double* dist,
                              const double* eta, const double* t_end, double x0, const double* u, int64_t n_col,
                              int64_t n_u, const double* p, int64_t n_p, const double* lambda, int64_t n_lambda,
                              const double* kappa, int64_t n_kappa, const sbr_opts* opts, sbr_result_soa* out,
                              double* tau_in, double* tau_out)
{
    int rc = hetero_econ_checks(c, opts, K, x0, n_col, n_u, n_p, n_lambda, n_kappa);
    if (rc) return rc;
    SBR_SINGLE_DEVICE(c);
    if (!betas || !dist || !eta || !t_end || !u || !p || !lambda || !kappa || !out || !out->xi || !out->aw_max ||
        !out->tol || !out->status)
        return fail(c, SBR_EARG, "null array");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    const sbr_opts o = resolve(opts);
    const sbr::ResultSoA r{out->xi, nullptr, nullptr, out->aw_max, out->tol, out->status, out->iters};
    return fenced(c, stream, true, [&](hipStream_t s) {
        return run_hetero_econ(c, s, K, betas, dist, eta, t_end, x0, u, n_col, n_u, p, n_p, lambda, n_lambda, kappa,
                               n_kappa, o, r, tau_in, tau_out);
    });
}

int sbr_sweep_hetero_econ(sbr_ctx* c, int32_t K, const double* betas, const double* dist, const double* eta,
                          const double* t_end, double x0, const double* u, int64_t n_col, int64_t n_u,
                          const double* p, int64_t n_p, const double* lambda, int64_t n_lambda, const double* kappa,
                          int64_t n_kappa, const sbr_opts* opts, sbr_result_soa* out, double* tau_in, double* tau_out)
{
    int rc = hetero_econ_checks(c, opts, K, x0, n_col, n_u, n_p, n_lambda, n_kappa);
    if (rc) return rc;
    if (!betas || !dist || !eta || !t_end || !u || !p || !lambda || !kappa || !out) return fail(c, SBR_EARG, "null array");
    rc = hetero_params_check(c, K, betas, dist, n_col);
    if (!rc) rc = check_positive(c, n_col, {eta, t_end}, "ArgumentError: eta/t_end");
    if (!rc) rc = check_u(c, u, n_u);
    if (rc) return rc;
    for (int64_t a = 0; a < n_p; a++)
        if (!(p[a] >= 0.0 && p[a] <= 1.0)) return fail(c, SBR_EARG, "ArgumentError: p must be in [0, 1]");
    rc = check_positive(c, n_lambda, {lambda}, "ArgumentError: lambda must be positive");
    if (rc) return rc;
    for (int64_t k = 0; k < n_kappa; k++)
        if (!(kappa[k] > 0.0 && kappa[k] < 1.0)) return fail(c, SBR_EARG, "ArgumentError: kappa must be in (0, 1)");
    const sbr_opts o = resolve(opts);
    const Inputs in{cols(betas, (size_t)K),       shared(dist, (size_t)K), cols(eta),
                    cols(t_end),                  shared(u, (size_t)n_u),  shared(p, (size_t)n_p),
                    shared(lambda, (size_t)n_lambda), shared(kappa, (size_t)n_kappa)};
    if (c->multi)
        return multi_sweep_hetero_econ(c, in, K, x0, n_col, n_u, n_p, n_lambda, n_kappa, o, out, tau_in, tau_out);
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    // the result block: xi, aw_max, tol | status, iters | tau_in, tau_out (K per point)
    const size_t np = (size_t)n_col * (size_t)(n_p * n_lambda) * (size_t)(n_kappa * n_u);
    void* dres;
    rc = ensure_io(c, in, (size_t)n_col, np * (3 * 8 + 2 * 4 + 2 * (size_t)K * 8), &dres);
    if (rc) return rc;
    const auto d = in.dev(c->stage, (size_t)n_col);
    double *dxi = (double*)dres, *daw = dxi + np, *dtol = daw + np;
    uint32_t* dst = (uint32_t*)(dtol + np);
    int32_t* dit = (int32_t*)(dst + np);
    double* dtin = (double*)(dit + np);
    double* dtout = dtin + np * K;
    return fenced(c, nullptr, false, [&](hipStream_t s) -> int {
        rc = in.stage(c, c->stage, (size_t)n_col, s);
        if (rc) return rc;
        const sbr::ResultSoA r{dxi, nullptr, nullptr, daw, dtol, dst, dit};
        rc = run_hetero_econ(c, s, K, d[0], d[1], d[2], d[3], x0, d[4], n_col, n_u, d[5], n_p, d[6], n_lambda, d[7],
                             n_kappa, o, r, tau_in ? dtin : nullptr, tau_out ? dtout : nullptr);
        if (rc) return rc;
        // the kernels finish before the first byte reaches the caller's arrays: a launch that failed
        // on the device leaves them as they were
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        rc = copy_out(c, s, {{out->xi, dxi, np * 8}, {out->aw_max, daw, np * 8}, {out->tol, dtol, np * 8},
                             {out->status, dst, np * 4}, {out->iters, dit, np * 4},
                             {tau_in, dtin, np * K * 8}, {tau_out, dtout, np * K * 8}});
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        return SBR_OK;
    });
}

int sbr_set_hetero_econ_slab(sbr_ctx* c, int32_t knots)
{
    if (!c || knots < 0) return SBR_EARG;
    for (int r = 0; c->multi && r < sbr_multi_size(c); r++) sbr_multi_child(c, r)->he_slab = knots; // every rank's own
    c->he_slab = knots;
    return SBR_OK;
}

}  // extern "C"
