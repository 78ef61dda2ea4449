// sbr_capi.hip — the extern "C" boundary of libsbr (declared in include/sbr.h).
//
// A context owns one HIP device, one stream and a grow-only HBM workspace
// (knot slabs sized n_beta × knot_capacity).  Host-pointer entry points stage
// inputs, run the device pipeline and copy results back synchronously;
// *_dev entry points only enqueue on the caller's stream.
//
// This file: context lifecycle, options, diagnostics, the selftest kernels and
// sbr_apply_early_exit.  The sweeps live by family in sbr_capi_baseline.hip, sbr_capi_hetero.hip,
// sbr_capi_social.hip and sbr_capi_knots.hip; sbr_ctx.h holds the context and what they share,
// sbr_hostio.h the host-pointer sweeps' staging and readback.
#include "sbr_hostio.h"

using namespace sbr_capi;

namespace sbr_capi {

hipEvent_t next_event(sbr_ctx* c)
{
    if (c->ev_used == c->ev_pool.size()) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, kTimingEventFlags) != hipSuccess) return nullptr;
        c->ev_pool.push_back(e);
    }
    return c->ev_pool[c->ev_used++];
}

hipEvent_t tstart(sbr_ctx* c, hipStream_t s)
{
    if (!c->timing) return nullptr;
    hipEvent_t e = next_event(c);
    if (e) (void)hipEventRecord(e, s);
    return e;
}

void tend(sbr_ctx* c, hipStream_t s, int kind, hipEvent_t a, int count)
{
    if (!c->timing || !a) return;
    hipEvent_t e = next_event(c);
    if (!e) return;
    (void)hipEventRecord(e, s);
    c->trec.push_back({kind, a, e, count});
}

}  // namespace sbr_capi

namespace {

// n columns' counters and status from column `off` of a learning workspace (LearnBufs / HeteroBufs)
template <class Bufs>
int learn_stats(sbr_ctx* c, const Bufs& B, int64_t off, int64_t n, int32_t* n_knots, int32_t* n_tau,
                int32_t* n_accept, int32_t* n_reject, uint32_t* status)
{
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    HIP_TRY(c, hipDeviceSynchronize(), SBR_EDEVICE);
    struct { void* h; const void* d; } cp[] = {{n_knots, B.n_knots + off}, {n_tau, B.n_tau + off},
                                               {n_accept, B.n_accept + off}, {n_reject, B.n_reject + off},
                                               {status, B.status + off}};
    for (auto& x : cp)
        if (x.h) HIP_TRY(c, hipMemcpy(x.h, x.d, (size_t)n * 4, hipMemcpyDeviceToHost), SBR_EDEVICE);
    return SBR_OK;
}

}  // namespace

hipStream_t sbr_ctx_stream(sbr_ctx* c) { return c ? c->stream : nullptr; }

extern "C" {

void sbr_default_opts(sbr_opts* o)
{
    o->ode_reltol = 2.220446049250313e-16;
    o->ode_abstol = 2.220446049250313e-16;
    o->ode_maxiters = SBR_DEFAULT_ODE_MAXITERS;
    o->bisect_max_iters = 100;
    o->early_exit_nan_run = 5;
    o->knot_capacity = kDefaultCap;
    o->hetero_max_iters = 500;
    o->flags = 0;
    o->pad = 0;
    o->xi_guess = __builtin_nan(""); // compute_ξ's default first iterate, the midpoint (solver.jl:309)
}

int sbr_init(int device, sbr_ctx** out)
{
    if (!out) return SBR_EARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return SBR_EDEVICE;
    sbr_ctx* c = new sbr_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, kSyncEventFlags) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, kSyncEventFlags) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_last, kSyncEventFlags) != hipSuccess) {
        delete c;
        return SBR_EDEVICE;
    }
    int smem = 0;
    (void)hipDeviceGetAttribute(&smem, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
    if (smem <= 0) smem = 65536;
    c->lds_smem = smem;
    // per 64 staged knots: t, G, HR (3·64) + HR block max/min (2) + their prefix/suffix tables (4)
    // + 8-knot G prefix-max/suffix-min (16); 1 KiB slack
    c->lds_cap = (int)(((long)(smem - 1024) * 64) / (8 * (3 * 64 + 6 + 16)));
    // baseline equilibrium kernel: t, G (2·64) + summaries per 64 knots, two workgroups per CU
    c->lds_cap_b = (int)(((long)(smem / 2 - 1024) * 64) / (8 * (2 * 64 + 6 + 16)));
    *out = c;
    return SBR_OK;
}

int sbr_init_multi(int n_gpus, const int* devices, sbr_ctx** out)
{
    if (!out) return SBR_EARG;
    *out = nullptr;
    if (n_gpus <= 0) return SBR_EARG;
    sbr_ctx* c = new sbr_ctx();
    std::vector<sbr_ctx*> kids;
    std::string err;
    const int rc = sbr_multi_impl::create(n_gpus, devices, &c->multi, kids, err);
    if (rc != SBR_OK) {
        delete c;
        return rc;
    }
    c->device = kids[0]->device;
    *out = c;
    return SBR_OK;
}

int sbr_multi_size(const sbr_ctx* c) { return c ? sbr_multi_impl::size(c->multi) : 0; }

sbr_ctx* sbr_multi_child(sbr_ctx* c, int rank)
{
    if (!c) return nullptr;
    if (!c->multi) return rank == 0 ? c : nullptr;
    return sbr_multi_impl::child(c->multi, rank);
}

int sbr_free(sbr_ctx* c)
{
    if (!c) return SBR_OK;
    if (c->multi) {
        sbr_multi_impl::destroy(c->multi);
        delete c;
        return SBR_OK;
    }
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (hipStream_t ls : c->lstream)
        if (ls) (void)hipStreamSynchronize(ls);
    for (int k = 0; k < sbr_ctx::kLearnSlots; k++) free_learn(c, k);
    free_hetero(c);
    free_social(c);
    free_pool(c);
    free_econ(c);
    free_dev(c->so_prof, c->so_args_dev, c->rq, c->stage, c->kn_dev, c->hk_dev);
    for (void* h : {(void*)c->so_count_host, (void*)c->so_args_host, c->res_pin, (void*)c->kn_pin, (void*)c->kn_zc,
                    (void*)c->hk_pin})
        if (h) (void)hipHostFree(h);
    for (hipStream_t rs : {c->rs_learn, c->rs_eq})
        if (rs) { (void)hipStreamSynchronize(rs); (void)hipStreamDestroy(rs); }
    for (hipStream_t ls : c->lstream)
        if (ls) (void)hipStreamDestroy(ls);
    for (hipEvent_t e : {c->ev_in, c->ev_fork, c->ev_join, c->ev_last, c->ev_rin, c->ev_rq, c->ev_rl, c->ev_re})
        if (e) (void)hipEventDestroy(e);
    for (int k = 0; k < sbr_ctx::kLearnSlots; k++)
        for (hipEvent_t e : {c->ev_learned[k], c->ev_eq[k]})
            if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_grid) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_hn) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(c->stream);
    delete c;
    return SBR_OK;
}

const char* sbr_last_error(const sbr_ctx* c)
{
    // an n-device sweep's failure is copied into c->err by fail(); no fallback to the
    // multi layer's message, which would resurface after a later success
    return c ? c->err.c_str() : "null context";
}

int sbr_chunk_timeline(sbr_ctx* c, void* stream, int32_t* n_chunks, double* ms)
{
    SBR_PER_DEVICE_DIAG(c);
    if (!c || !n_chunks) return SBR_EARG;
    *n_chunks = 0;
    if (!c->ck_start || c->ck_ev.empty()) return SBR_OK;
    HIP_TRY(c, hipStreamSynchronize((hipStream_t)stream), SBR_EDEVICE);
    for (hipStream_t ls : c->lstream)
        if (ls) HIP_TRY(c, hipStreamSynchronize(ls), SBR_EDEVICE);
    const int nk = (int)c->ck_ev.size() / 2;
    for (int k = 0; k < nk; k++)
        for (int e = 0; e < 2; e++) {
            float a = -1.f;
            hipEvent_t ev = c->ck_ev[2 * k + e];
            if (ev && hipEventElapsedTime(&a, c->ck_start, ev) != hipSuccess) a = -1.f;
            if (ms) ms[2 * k + e] = ev ? (double)a : -1.0;
        }
    *n_chunks = nk;
    return SBR_OK;
}

int sbr_host_phases(sbr_ctx* c, double* ms5)
{
    if (!c || !ms5) return SBR_EARG;
    const double* ph = c->multi ? sbr_multi_impl::phases(c->multi) : c->ph_ms;
    for (int k = 0; k < 5; k++) ms5[k] = ph[k];
    return SBR_OK;
}

int sbr_last_schedule(sbr_ctx* c, int32_t* schedule)
{
    SBR_PER_DEVICE_DIAG(c);
    if (!c || !schedule) return SBR_EARG;
    *schedule = c->rs_used ? 1 : 0;
    return SBR_OK;
}

int sbr_timing_enable(sbr_ctx* c, int on)
{
    SBR_PER_DEVICE_DIAG(c);
    if (!c) return SBR_EARG;
    c->timing = on != 0;
    c->ev_used = 0;
    c->trec.clear();
    return SBR_OK;
}

int sbr_timing_read(sbr_ctx* c, void* stream, double* learn_ms, double* eq_ms, int32_t* n_calls)
{
    SBR_PER_DEVICE_DIAG(c);
    if (!c) return SBR_EARG;
    hipStream_t s = (hipStream_t)stream; // NULL = HIP null stream
    HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
    HIP_TRY(c, hipStreamSynchronize(c->stream), SBR_EDEVICE); // host-pointer sweeps time on it
    double a = 0.0, b = 0.0;
    int32_t n = 0;
    for (hipStream_t ls : c->lstream)
        if (ls) HIP_TRY(c, hipStreamSynchronize(ls), SBR_EDEVICE);
    for (hipStream_t rs : {c->rs_learn, c->rs_eq})
        if (rs) HIP_TRY(c, hipStreamSynchronize(rs), SBR_EDEVICE);
    for (const auto& r : c->trec) {
        float t = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&t, r.a, r.b), SBR_EDEVICE);
        if (r.kind == 0) a += t;
        else { b += t; n += r.count; }
    }
    if (learn_ms) *learn_ms = a;
    if (eq_ms) *eq_ms = b;
    if (n_calls) *n_calls = n;
    c->ev_used = 0;
    c->trec.clear();
    return SBR_OK;
}

int sbr_learn_stats(sbr_ctx* c, int64_t n_beta, int32_t* n_knots, int32_t* n_tau, int32_t* n_accept,
                    int32_t* n_reject, uint32_t* status)
{
    SBR_PER_DEVICE_DIAG(c);
    if (!c || n_beta <= 0 || (size_t)(n_beta + c->last_off) > c->ws_beta[c->last_slot]) return SBR_EARG;
    // the last grid of a grouped learning slot
    return learn_stats(c, c->LW[c->last_slot], c->last_off, n_beta, n_knots, n_tau, n_accept, n_reject, status);
}

int sbr_hetero_learn_stats(sbr_ctx* c, int64_t n_col, int32_t* n_knots, int32_t* n_tau, int32_t* n_accept,
                           int32_t* n_reject, uint32_t* status)
{
    SBR_PER_DEVICE_DIAG(c);
    if (!c || n_col <= 0 || (size_t)n_col > c->hs_col) return SBR_EARG;
    return learn_stats(c, c->H, 0, n_col, n_knots, n_tau, n_accept, n_reject, status);
}

int sbr_device_info(sbr_ctx* c, int32_t* lds_bytes_per_block, int32_t* lds_knot_capacity, int32_t* cu_count)
{
    SBR_ON_RANK0(c, sbr_device_info(c, lds_bytes_per_block, lds_knot_capacity, cu_count));
    if (!c) return SBR_EARG;
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
    if (lds_bytes_per_block) *lds_bytes_per_block = c->lds_smem;
    if (lds_knot_capacity) *lds_knot_capacity = c->lds_cap;
    if (cu_count) *cu_count = cus;
    return SBR_OK;
}

void sbr_apply_early_exit(int64_t n_beta, int64_t n_u, int32_t threshold, sbr_result_soa* r)
{
    for (int64_t b = 0; b < n_beta; b++) {
        int32_t cnt = 0;
        for (int64_t j = 0; j < n_u; j++) {
            const int64_t o = b * n_u + j;
            if (cnt >= threshold) {
                r->xi[o] = NAN;
                r->aw_max[o] = NAN;
                r->tol[o] = INFINITY;
                r->status[o] = SBR_SKIPPED_EARLY_EXIT;
                continue;
            }
            if (r->status[o] & SBR_RUN) cnt = 0;
            else cnt++;
        }
    }
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Diagnostics: evaluate the shared deterministic math on the device so tests
// can check host/device bit equality of sbr_exp / sbr_log / sbr_pow_pos.
// ---------------------------------------------------------------------------
namespace {
__global__ void detmath_kernel(const double* x, const double* y, int n, double* e, double* l, double* pw)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    e[i] = sbr_exp(x[i]);
    l[i] = sbr_log(x[i]);
    pw[i] = sbr_pow_pos(x[i], y[i]);
}

__global__ void fastpow_kernel(const double* x, const double* y, int n, double* out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = sbr_fastpow(x[i], y[i]);
}
}  // namespace

extern "C" int sbr_selftest_fastpow(sbr_ctx* c, const double* x, const double* y, int n, double* out)
{
    SBR_ON_RANK0(c, sbr_selftest_fastpow(c, x, y, n, out));
    if (!c || n <= 0 || !x || !y || !out) return SBR_EARG;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    int rc = ensure_stage(c, (size_t)n * 3 * 8);
    if (rc) return rc;
    return fenced(c, nullptr, false, [&](hipStream_t s) -> int {
        double* d = (double*)c->stage;
        HIP_TRY(c, hipMemcpyAsync(d, x, n * 8, hipMemcpyHostToDevice, s), SBR_EDEVICE);
        HIP_TRY(c, hipMemcpyAsync(d + n, y, n * 8, hipMemcpyHostToDevice, s), SBR_EDEVICE);
        hipLaunchKernelGGL(fastpow_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d, d + n, n, d + 2 * n);
        HIP_TRY(c, hipGetLastError(), SBR_EDEVICE);
        HIP_TRY(c, hipMemcpyAsync(out, d + 2 * n, n * 8, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        return SBR_OK;
    });
}

extern "C" int sbr_selftest_detmath(sbr_ctx* c, const double* x, const double* y, int n, double* e, double* l,
                                    double* pw)
{
    SBR_ON_RANK0(c, sbr_selftest_detmath(c, x, y, n, e, l, pw));
    if (!c || n <= 0) return SBR_EARG;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, SBR_EDEVICE, "hipSetDevice");
    int rc = ensure_stage(c, (size_t)n * 5 * 8);
    if (rc) return rc;
    double* d = (double*)c->stage;
    return fenced(c, nullptr, false, [&](hipStream_t s) -> int {
        HIP_TRY(c, hipMemcpyAsync(d, x, n * 8, hipMemcpyHostToDevice, s), SBR_EDEVICE);
        HIP_TRY(c, hipMemcpyAsync(d + n, y, n * 8, hipMemcpyHostToDevice, s), SBR_EDEVICE);
        hipLaunchKernelGGL(detmath_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d, d + n, n, d + 2 * n, d + 3 * n,
                           d + 4 * n);
        HIP_TRY(c, hipGetLastError(), SBR_EDEVICE);
        HIP_TRY(c, hipMemcpyAsync(e, d + 2 * n, n * 8, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        HIP_TRY(c, hipMemcpyAsync(l, d + 3 * n, n * 8, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        HIP_TRY(c, hipMemcpyAsync(pw, d + 4 * n, n * 8, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
        HIP_TRY(c, hipStreamSynchronize(s), SBR_EDEVICE);
        return SBR_OK;
    });
}
