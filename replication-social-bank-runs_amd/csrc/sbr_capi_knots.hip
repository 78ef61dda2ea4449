// sbr_capi_knots.hip — equilibria on the caller's own knot grid: sbr_equilibrium_on_knots (and its
// _pdf variant) and sbr_hetero_equilibrium_on_knots, each with its resident device block.
#include "sbr_hostio.h"

using namespace sbr_capi;

namespace {

// byte offsets of sbr_equilibrium_on_knots' device block (and of its pinned mirror) for ck knots
// and cu u values: [counters | β, η | t, G, pdf (packed by the call's n) | HR | t_end, u | results,
// paths]
struct KnotLayout {
    size_t sc, tg, hr, u, res, bytes;
    KnotLayout(size_t ck, size_t cu)
    {
        sc = 64;
        tg = 128;
        hr = tg + 24 * ck;
        u = hr + 8 * (ck + 8);
        res = u + 8 * (cu + 8);
        bytes = res + 8 * (6 * cu + 3 * (ck + 1)) + 256;
    }
};

int ensure_knots(sbr_ctx* c, size_t n, size_t n_u)
{
    if (n <= c->kn_cap_k && n_u <= c->kn_cap_u) return SBR_OK;
    size_t ck = c->kn_cap_k > 4096 ? c->kn_cap_k : 4096, cu = c->kn_cap_u > 64 ? c->kn_cap_u : 64;
    while (ck < n) ck *= 2;
    while (cu < n_u) cu *= 2;
    // each buffer freed once and nulled (a second hipHostFree of the same pointer leaves a sticky
    // error that the next HIP_TRY reports against an unrelated launch)
    if (c->kn_dev) (void)hipFree(c->kn_dev);
    if (c->kn_pin) (void)hipHostFree(c->kn_pin);
    if (c->kn_zc) (void)hipHostFree(c->kn_zc);
    c->kn_dev = c->kn_pin = nullptr;
    c->kn_zc = c->kn_zc_dev = nullptr;
    c->kn_cap_k = c->kn_cap_u = 0;
    c->kn_valid = false;
    const KnotLayout K(ck, cu);
    HIP_TRY(c, hipMalloc(&c->kn_dev, K.bytes), SBR_ENOMEM);
    HIP_TRY(c, hipHostMalloc(&c->kn_pin, K.bytes), SBR_ENOMEM);
    c->kn_cap_k = ck;
    c->kn_cap_u = cu;
    // [t_end, u, results (8 doubles), AW_cum / AW_OUT / AW_IN (ck + 1 each)]
    const size_t zc = 16 + 3 * (ck + 1);
    HIP_TRY(c, hipHostMalloc(&c->kn_zc, zc * 8, hipHostMallocMapped | hipHostMallocCoherent), SBR_ENOMEM);
    HIP_TRY(c, hipHostGetDevicePointer((void**)&c->kn_zc_dev, c->kn_zc, 0), SBR_EDEVICE);
    c->kn_zc_cap = zc;
    return SBR_OK;
}

// sbr_hetero_equilibrium_on_knots' device block (and pinned mirror) for ck knots, cu u values and
// K <= SBR_HETERO_MAX_K groups: [counters | βs, dist, η | t, G packed by the call's n | HR, I (K·ck
// each) | t_end, u | results, buffers, AW_total path]
struct HeteroKnotLayout {
    size_t sc, tg, hr, hri, u, res, bytes;
    HeteroKnotLayout(size_t ck, size_t cu)
    {
        constexpr size_t KM = SBR_HETERO_MAX_K;
        sc = 64;
        tg = 512; // sc + (2·KM + 1) doubles, rounded up
        static_assert(64 + 8 * (2 * KM + 1) <= 512, "βs, dist, η in front of the knots");
        hr = tg + 8 * ck * (KM + 1);
        hri = hr + 8 * ck * KM;
        u = hri + 8 * ck * KM;
        res = u + 8 * (cu + 8);
        bytes = res + 8 * (5 * cu + 2 * KM * cu + (2 * KM + 1) * ck) + 256; // path mode: AW_total + 2K group rows
    }
};

int ensure_hetero_knots(sbr_ctx* c, size_t n, size_t n_u)
{
    if (n <= c->hk_cap_k && n_u <= c->hk_cap_u) return SBR_OK;
    size_t ck = c->hk_cap_k > 8192 ? c->hk_cap_k : 8192, cu = c->hk_cap_u > 64 ? c->hk_cap_u : 64;
    while (ck < n) ck *= 2;
    while (cu < n_u) cu *= 2;
    if (c->hk_dev) (void)hipFree(c->hk_dev);
    if (c->hk_pin) (void)hipHostFree(c->hk_pin);
    c->hk_dev = c->hk_pin = nullptr;
    c->hk_cap_k = c->hk_cap_u = 0;
    c->hk_valid = false;
    const HeteroKnotLayout Lh(ck, cu);
    HIP_TRY(c, hipMalloc(&c->hk_dev, Lh.bytes), SBR_ENOMEM);
    HIP_TRY(c, hipHostMalloc(&c->hk_pin, Lh.bytes), SBR_ENOMEM);
    c->hk_cap_k = ck;
    c->hk_cap_u = cu;
    return SBR_OK;
}

}  // namespace

extern "C" {

int sbr_hetero_equilibrium_on_knots(sbr_ctx* c, int32_t K, const double* t, const double* G, int64_t n,
                                    const double* betas, const double* dist, double eta, double t_end, const double* u,
                                    int64_t n_u, double p, double kappa, double lambda, const sbr_opts* opts,
                                    sbr_result_soa* out, double* tau_in, double* tau_out, double* hr, double* aw_total,
                                    double* aw_groups, int64_t cap, int64_t* n_tau)
{
    if (int rc = refuse_guess(c, opts)) return rc;
    SBR_ON_RANK0(c, sbr_hetero_equilibrium_on_knots(c, K, t, G, n, betas, dist, eta, t_end, u, n_u, p, kappa, lambda, opts, out, tau_in, tau_out, hr, aw_total, aw_groups, cap, n_tau));
    if (!c || !t || !G || !betas || !dist || !u || !out) return SBR_EARG;
    if (!hetero_K_ok(K)) return fail(c, SBR_EARG, kHeteroKMsg);
    if (n < 1 || n > (1 << 24) || n_u < 1 || n_u > (1 << 24)) return fail(c, SBR_EARG, "knot / u count");
    double dsum = 0.0;
    for (int k = 0; k < K; k++) {
        if (!(dist[k] >= 0.0)) return fail(c, SBR_EARG, "ArgumentError: distribution weights must be non-negative");
        if (!(betas[k] > 0.0)) return fail(c, SBR_EARG, "ArgumentError: all learning rates must be positive");
        dsum = dsum + dist[k];
    }
    if (!(fabs(dsum - 1.0) < 1e-10)) return fail(c, SBR_EARG, "ArgumentError: distribution must sum to 1");
    if (!scalars_valid(0.0, p, kappa, lambda) || !(eta > 0) || !(t_end > 0))
        return fail(c, SBR_EARG, "ArgumentError: eta/t_end/p/kappa/lambda");
    for (int64_t j = 0; j < n_u; j++)
        if (!(u[j] >= 0.0)) return fail(c, SBR_EARG, "ArgumentError: u must be non-negative");
    if (!(t[0] == t[0])) return fail(c, SBR_EARG, "ArgumentError: knots must be sorted");
    for (int64_t i = 0; i + 1 < n; i++)
        if (!(t[i] <= t[i + 1])) return fail(c, SBR_EARG, "ArgumentError: knots must be sorted");
    const bool paths = aw_total || aw_groups;
    if (paths && n_u != 1) return fail(c, SBR_EARG, "the AW paths need n_u == 1");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    const sbr_opts o = resolve(opts);
    int rc = ensure_hetero_knots(c, (size_t)n, (size_t)n_u);
    if (rc) return rc;
    const HeteroKnotLayout Lh(c->hk_cap_k, c->hk_cap_u);
    // the explicit-grid hazard (heterogeneity_solver.jl:255, solver.jl:163-164): τ̄ = knots <= η,
    // then η; pdf(η) is a BoundsError before the first knot or past the last one
    int64_t m = 0;
    while (m < n && t[m] <= eta) m++;
    const bool hz_oob = m == 0 || (m == n && !(n >= 2 && t[n - 1] == eta));
    const int64_t ntau = hz_oob ? 0 : m + 1;
    if ((hr && ntau > cap) || (paths && n > cap)) return fail(c, SBR_EARG, "path capacity too small");
    std::vector<double> key;
    key.reserve(2 * (size_t)K + 5);
    key.push_back((double)K);
    key.insert(key.end(), betas, betas + K);
    key.insert(key.end(), dist, dist + K);
    key.push_back(eta);
    key.push_back(p);
    key.push_back(lambda);
    const bool hit = c->hk_valid && c->hk_n == n && c->hk_K == K && c->hk_key == key &&
                     memcmp(c->hk_t.data(), t, (size_t)n * 8) == 0 &&
                     memcmp(c->hk_G.data(), G, (size_t)n * K * 8) == 0;
    char* D = c->hk_dev;
    char* H = c->hk_pin;
    int32_t* dcnt = (int32_t*)D;
    double* dsc = (double*)(D + Lh.sc); // βs [K], dist [K], η
    double* dtg = (double*)(D + Lh.tg);
    const size_t ck = c->hk_cap_k;
    const sbr::HeteroBufs HB{dtg, dtg + n, (double*)(D + Lh.hr), (double*)(D + Lh.hri), dcnt, dcnt + 1, dcnt + 2,
                             (uint32_t*)(dcnt + 3), dcnt + 4, dcnt + 5, (int32_t)ck, (int32_t)ck};
    double* du = (double*)(D + Lh.u); // [t_end, u...]
    double* dres = (double*)(D + Lh.res);
    const size_t nu = (size_t)n_u;
    // results: xi, aw, tol [n_u] | status, iters [n_u] int32 | tau_in, tau_out [n_u][K] |
    // path mode: AW_total [n], AW_OUT_k [K][n], AW_IN_k [K][n]
    double* dtin = dres + 4 * nu;
    double* dtout = dtin + nu * K;
    double* dpath = dtout + nu * K;
    const size_t res_bytes = (4 * nu + 2 * nu * K + (paths ? (size_t)n * (1 + 2 * K) : 0)) * 8;
    if (!hit) c->hk_valid = false;
    rc = fenced(c, nullptr, false, [&](hipStream_t s) -> int {
        sbr::LearnArgs la{0.0, o.ode_reltol, o.ode_abstol, p, lambda, o.ode_maxiters, 1, 0, 0, nullptr, nullptr};
        if (!hit) {
            memset(H, 0, Lh.tg);
            int32_t* hc = (int32_t*)H;
            hc[0] = (int32_t)n;
            double* hs = (double*)(H + Lh.sc);
            memcpy(hs, betas, (size_t)K * 8);
            memcpy(hs + K, dist, (size_t)K * 8);
            hs[2 * K] = eta;
            memcpy(H + Lh.tg, t, (size_t)n * 8);
            memcpy(H + Lh.tg + (size_t)n * 8, G, (size_t)n * K * 8);
            HIP_TRY(c, hipMemcpyAsync(D, H, Lh.tg + (size_t)n * (K + 1) * 8, hipMemcpyHostToDevice, s), SBR_EDEVICE);
            HIP_TRY(c, sbr::launch_hetero(K, dsc, dsc + K, dsc + 2 * K, nullptr, nullptr, la, sbr::HeteroEqArgs{},
                                          HB, sbr::ResultSoA{}, nullptr, nullptr, s, 2), SBR_EDEVICE);
            for (int k = 0; k < K && ntau > 0; k++)
                HIP_TRY(c, hipMemcpyAsync(H + Lh.hr + (size_t)k * ck * 8, D + Lh.hr + (size_t)k * ck * 8,
                                          (size_t)ntau * 8, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
            HIP_TRY(c, hipMemcpyAsync(H, D, 32, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        }
        double* hu = (double*)(H + Lh.u);
        hu[0] = t_end;
        memcpy(hu + 1, u, nu * 8);
        HIP_TRY(c, hipMemcpyAsync(du, hu, (nu + 1) * 8, hipMemcpyHostToDevice, s), SBR_EDEVICE);
        sbr::HeteroEqArgs ea{kappa, 1e-12, (int32_t)n_u, o.hetero_max_iters, het_lds(c),
                             (o.flags & SBR_FLAG_EXHAUSTIVE) ? 1 : 0, (o.flags >> 8) & 7, aw_total ? dpath : nullptr};
        const sbr::ResultSoA r{dres, nullptr, nullptr, dres + nu, dres + 2 * nu, (uint32_t*)(dres + 3 * nu),
                               (int32_t*)(dres + 3 * nu) + nu};
        HIP_TRY(c, sbr::launch_hetero(K, dsc, dsc + K, dsc + 2 * K, du, du + 1, la, ea, HB, r, dtin, dtout, s, 1,
                                      hetero_wide(o)), SBR_EDEVICE);
        if (aw_groups)
            HIP_TRY(c, sbr::launch_hetero_aw_groups(K, dtg, dtg + n, dcnt, (int)n, dres, dtin, dtout,
                                                    (const uint32_t*)(dres + 3 * nu), dpath + n, (size_t)n, s),
                    SBR_EDEVICE);
        HIP_TRY(c, hipMemcpyAsync(H + Lh.res, D + Lh.res, res_bytes, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        return SBR_OK;
    });
    if (rc) return rc;
    if (!hit) {
        const int32_t* hc = (const int32_t*)H;
        if (hc[1] != (int32_t)ntau) return fail(c, SBR_EDEVICE, "hetero hazard grid length mismatch");
        c->hk_t.assign(t, t + n);
        c->hk_G.assign(G, G + n * K);
        c->hk_hr.assign((size_t)K * ntau, 0.0);
        for (int k = 0; k < K; k++)
            memcpy(c->hk_hr.data() + (size_t)k * ntau, H + Lh.hr + (size_t)k * ck * 8, (size_t)ntau * 8);
        c->hk_key = key;
        c->hk_n = n;
        c->hk_K = K;
        c->hk_ntau = (int32_t)ntau;
        c->hk_valid = true;
    }
    const double* hres = (const double*)(H + Lh.res);
    if (out->xi) memcpy(out->xi, hres, nu * 8);
    if (out->aw_max) memcpy(out->aw_max, hres + nu, nu * 8);
    if (out->tol) memcpy(out->tol, hres + 2 * nu, nu * 8);
    if (out->status) memcpy(out->status, hres + 3 * nu, nu * 4);
    if (out->iters) memcpy(out->iters, (const int32_t*)(hres + 3 * nu) + nu, nu * 4);
    if (tau_in) memcpy(tau_in, hres + 4 * nu, nu * K * 8);
    if (tau_out) memcpy(tau_out, hres + 4 * nu + nu * K, nu * K * 8);
    if (n_tau) *n_tau = ntau;
    if (hr)
        for (int k = 0; k < K; k++) memcpy(hr + (size_t)k * cap, c->hk_hr.data() + (size_t)k * ntau, (size_t)ntau * 8);
    if (paths) {
        const bool run = (((const uint32_t*)(hres + 3 * nu))[0] & SBR_RUN) != 0;
        copy_hetero_paths(hres + 4 * nu + 2 * nu * K, run, K, n, cap, aw_total, aw_groups);
    }
    return SBR_OK;
}

}  // extern "C"

namespace {

// sbr_equilibrium_on_knots (pdf == nullptr: the learning pdf βG(1 − G) of the knots' G) and
// sbr_equilibrium_on_knots_pdf (the caller's pdf values on the same knots)
int on_knots(sbr_ctx* c, const double* t, const double* G, const double* pdf, int64_t n, double beta, double eta,
             double t_end, const double* u, int64_t n_u, double p, double kappa, double lambda, const sbr_opts* opts,
             sbr_result_soa* out, double* tau, double* hr, double* aw_cum, double* aw_out, double* aw_in, int64_t cap,
             int64_t* n_tau)
{
    if (!c || !t || !G || !u || !out) return SBR_EARG;
    if (n < 1 || n > (1 << 26) || n_u < 1 || n_u > (1 << 24)) return fail(c, SBR_EARG, "knot / u count");
    if (!scalars_valid(0.0, p, kappa, lambda) || !(beta > 0) || !(eta > 0) || !(t_end > 0))
        return fail(c, SBR_EARG, "ArgumentError: beta/eta/t_end/p/kappa/lambda");
    for (int64_t j = 0; j < n_u; j++)
        if (!(u[j] >= 0.0)) return fail(c, SBR_EARG, "ArgumentError: u must be non-negative");
    // Interpolations' gridded knots must be sorted (and not NaN)
    if (!(t[0] == t[0])) return fail(c, SBR_EARG, "ArgumentError: knots must be sorted");
    for (int64_t i = 0; i + 1 < n; i++)
        if (!(t[i] <= t[i + 1])) return fail(c, SBR_EARG, "ArgumentError: knots must be sorted");
    const bool want_aw = aw_cum || aw_out || aw_in;
    if (want_aw && n_u != 1) return fail(c, SBR_EARG, "AW paths need n_u == 1");
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    const sbr_opts o = resolve(opts);
    int rc = ensure_knots(c, (size_t)n, (size_t)n_u);
    if (rc) return rc;
    const KnotLayout K(c->kn_cap_k, c->kn_cap_u);
    // the hazard grid as solver.jl:155-161 builds it (knots are sorted: the .<= η mask is a
    // prefix), and its BoundsError: pdf(η) outside [t_1, t_n]
    int64_t m = 0;
    while (m < n && t[m] <= eta) m++;
    const bool push = m == 0 || t[m - 1] != eta;
    const bool hz_oob = m < n ? m == 0 : push;
    const int64_t ntau = hz_oob ? 0 : m + (push ? 1 : 0);
    if ((tau || hr || want_aw) && ntau > cap) return fail(c, SBR_EARG, "path capacity too small");
    const double key[4] = {beta, eta, p, lambda};
    const bool hit = c->kn_valid && c->kn_n == n && memcmp(c->kn_key, key, sizeof key) == 0 &&
                     memcmp(c->kn_t.data(), t, (size_t)n * 8) == 0 && memcmp(c->kn_G.data(), G, (size_t)n * 8) == 0 &&
                     (pdf ? c->kn_pdf.size() == (size_t)n && memcmp(c->kn_pdf.data(), pdf, (size_t)n * 8) == 0
                          : c->kn_pdf.empty());
    char* D = c->kn_dev;
    char* H = c->kn_pin;
    int32_t* dcnt = (int32_t*)D; // n_knots, n_tau, n_le, status, n_accept, n_reject
    double* dsc = (double*)(D + K.sc);
    double* dtg = (double*)(D + K.tg);
    const sbr::LearnBufs L{dtg, dtg + n, (double*)(D + K.hr), nullptr, dcnt, dcnt + 1, dcnt + 2,
                           (uint32_t*)(dcnt + 3), dcnt + 4, dcnt + 5, (int32_t)c->kn_cap_k, (int32_t)c->kn_cap_k};
    double* du = (double*)(D + K.u); // [t_end, u_0 .. u_{n_u-1}]
    double* dres = (double*)(D + K.res);
    const size_t res_bytes = (size_t)n_u * 48 + (want_aw ? (size_t)ntau * 24 : 0);
    if (!hit) c->kn_valid = false; // the resident copy is being replaced
    rc = fenced(c, nullptr, false, [&](hipStream_t s) -> int {
        if (!hit) {
            int32_t* hc = (int32_t*)H;
            memset(H, 0, K.tg);
            hc[0] = (int32_t)n;
            hc[2] = (int32_t)m;
            double* hs = (double*)(H + K.sc);
            hs[0] = beta;
            hs[1] = eta;
            memcpy(H + K.tg, t, (size_t)n * 8);
            memcpy(H + K.tg + (size_t)n * 8, G, (size_t)n * 8);
            if (pdf) memcpy(H + K.tg + (size_t)n * 16, pdf, (size_t)n * 8);
            HIP_TRY(c, hipMemcpyAsync(D, H, K.tg + (size_t)n * (pdf ? 24 : 16), hipMemcpyHostToDevice, s), SBR_EDEVICE);
            sbr::LearnArgs la{0.0, o.ode_reltol, o.ode_abstol, p, lambda, o.ode_maxiters, 1, 0, 0, nullptr, nullptr};
            la.pdf = pdf ? dtg + 2 * n : nullptr;
            HIP_TRY(c, sbr::launch_hazard(dsc, dsc + 1, la, L, 1, s), SBR_EDEVICE);
            if (ntau > 0)
                HIP_TRY(c, hipMemcpyAsync(H + K.hr, D + K.hr, (size_t)ntau * 8, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
            HIP_TRY(c, hipMemcpyAsync(H, D, 32, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        }
        const size_t nu = (size_t)n_u;
        if (n_u == 1) {
            // one point: the whole workgroup on it (latency), inputs read from and results written
            // to mapped host memory — one launch, no copies
            double* z = c->kn_zc;
            double* zd = c->kn_zc_dev;
            z[0] = t_end;
            z[1] = u[0];
            const sbr::ResultSoA r{zd + 2, zd + 3, zd + 4, zd + 5, zd + 6, (uint32_t*)(zd + 7), (int32_t*)(zd + 7) + 1};
            double* zp = zd + 16;
            sbr::EqArgs ea{kappa, 1, o.bisect_max_iters, c->lds_cap, want_aw ? zp : nullptr,
                           (o.flags & SBR_FLAG_EXHAUSTIVE) ? 1 : 0, (o.flags >> 8) & 0x17,
                           want_aw ? zp + ntau : nullptr, want_aw ? zp + 2 * ntau : nullptr, 1, dres};
            if (o.flags & SBR_FLAG_XI_GUESS) ea.xi_guess = o.xi_guess;
            HIP_TRY(c, sbr::launch_point_coop(L, dsc + 1, zd, zd + 1, ea, r, s), SBR_EDEVICE);
        } else {
            double* hu = (double*)(H + K.u);
            hu[0] = t_end;
            memcpy(hu + 1, u, nu * 8);
            HIP_TRY(c, hipMemcpyAsync(du, hu, (nu + 1) * 8, hipMemcpyHostToDevice, s), SBR_EDEVICE);
            const sbr::ResultSoA r{dres, dres + nu, dres + 2 * nu, dres + 3 * nu, dres + 4 * nu,
                                   (uint32_t*)(dres + 5 * nu), (int32_t*)(dres + 5 * nu) + nu};
            if ((o.flags & SBR_FLAG_XI_GUESS) && o.xi_guess == o.xi_guess) {
                // ξ_guess: the single-point kernel, one workgroup per u, in one launch (its plain
                // first-iterate bisection; the sweep kernel carries no guess path, it would cost the
                // sweeps registers)
                sbr::EqArgs ea{kappa, 1, o.bisect_max_iters, c->lds_cap, nullptr,
                               (o.flags & SBR_FLAG_EXHAUSTIVE) ? 1 : 0, (o.flags >> 8) & 0x17, nullptr, nullptr, 1};
                ea.xi_guess = o.xi_guess;
                HIP_TRY(c, sbr::launch_point_coop(L, dsc + 1, du, du + 1, ea, r, s, (int)nu), SBR_EDEVICE);
            } else {
                sbr::EqArgs ea{kappa, (int32_t)n_u, o.bisect_max_iters, c->lds_cap_b, nullptr,
                               (o.flags & SBR_FLAG_EXHAUSTIVE) ? 1 : 0, (o.flags >> 8) & 0x17, nullptr, nullptr, 1};
                HIP_TRY(c, sbr::launch_equilibrium(L, dsc + 1, du, du + 1, ea, r, 1, s, n <= c->lds_cap_b ? 1 : 2),
                        SBR_EDEVICE);
            }
            HIP_TRY(c, hipMemcpyAsync(H + K.res, D + K.res, res_bytes, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        }
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        return SBR_OK;
    });
    if (rc) return rc;
    if (!hit) {
        const int32_t* hc = (const int32_t*)H;
        // the device's hazard grid must be the one sized above (a bug guard)
        if (hc[1] != (int32_t)ntau) return fail(c, SBR_EDEVICE, "hazard grid length mismatch");
        c->kn_t.assign(t, t + n);
        c->kn_G.assign(G, G + n);
        if (pdf) c->kn_pdf.assign(pdf, pdf + n);
        else c->kn_pdf.clear();
        const double* hh = (const double*)(H + K.hr);
        c->kn_hr.assign(hh, hh + ntau);
        memcpy(c->kn_key, key, sizeof key);
        c->kn_n = n;
        c->kn_m = (int32_t)m;
        c->kn_ntau = (int32_t)ntau;
        c->kn_valid = true;
    }
    const size_t nu = (size_t)n_u;
    // n_u == 1: the mapped block [t_end, u, xi, τ̄_IN, τ̄_OUT, AW_max, tol, status | iters, pad, paths]
    const double* hr_ = n_u == 1 ? c->kn_zc + 2 : (const double*)(H + K.res);
    scatter_results(hr_, nu, out);
    if (n_tau) *n_tau = ntau;
    if (tau) {
        memcpy(tau, t, (size_t)m * 8);
        if (ntau > m) tau[m] = eta;
    }
    if (hr) memcpy(hr, c->kn_hr.data(), (size_t)ntau * 8);
    if (want_aw) { // n_u == 1
        const bool run = (((const uint32_t*)(hr_ + 5))[0] & SBR_RUN) != 0;
        const double* hp = c->kn_zc + 16;
        double* dst[3] = {aw_cum, aw_out, aw_in};
        for (int k = 0; k < 3; k++) {
            if (!dst[k]) continue;
            if (run) memcpy(dst[k], hp + k * ntau, (size_t)ntau * 8);
            else for (int64_t i = 0; i < ntau; i++) dst[k][i] = NAN;
        }
    }
    return SBR_OK;
}

}  // namespace

extern "C" {

int sbr_equilibrium_on_knots(sbr_ctx* c, const double* t, const double* G, int64_t n, double beta, double eta,
                             double t_end, const double* u, int64_t n_u, double p, double kappa, double lambda,
                             const sbr_opts* opts, sbr_result_soa* out, double* tau, double* hr, double* aw_cum,
                             double* aw_out, double* aw_in, int64_t cap, int64_t* n_tau)
{
    SBR_ON_RANK0(c, sbr_equilibrium_on_knots(c, t, G, n, beta, eta, t_end, u, n_u, p, kappa, lambda, opts, out, tau, hr, aw_cum, aw_out, aw_in, cap, n_tau));
    return on_knots(c, t, G, nullptr, n, beta, eta, t_end, u, n_u, p, kappa, lambda, opts, out, tau, hr, aw_cum,
                    aw_out, aw_in, cap, n_tau);
}

int sbr_equilibrium_on_knots_pdf(sbr_ctx* c, const double* t, const double* G, const double* pdf, int64_t n,
                                 double eta, double t_end, const double* u, int64_t n_u, double p, double kappa,
                                 double lambda, const sbr_opts* opts, sbr_result_soa* out, double* tau, double* hr,
                                 double* aw_cum, double* aw_out, double* aw_in, int64_t cap, int64_t* n_tau)
{
    SBR_ON_RANK0(c, sbr_equilibrium_on_knots_pdf(c, t, G, pdf, n, eta, t_end, u, n_u, p, kappa, lambda, opts, out, tau, hr, aw_cum, aw_out, aw_in, cap, n_tau));
    if (!pdf) return c ? fail(c, SBR_EARG, "pdf values missing") : SBR_EARG;
    // β only forms the default pdf; 1.0 passes the argument check and keys nothing else
    return on_knots(c, t, G, pdf, n, 1.0, eta, t_end, u, n_u, p, kappa, lambda, opts, out, tau, hr, aw_cum,
                    aw_out, aw_in, cap, n_tau);
}

}  // extern "C"
