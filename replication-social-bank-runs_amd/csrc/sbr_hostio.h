// sbr_hostio.h — host plumbing of the host-pointer sweeps (sbr_capi_*.hip): one description of a
// call's input arrays that gives every staged size and device pointer, the result block behind
// them, its pinned readback, and the n-device fan-out of the same description.  Host-only.
#pragma once

#include "sbr_ctx.h"
#include "sbr_hostcopy.h"

namespace sbr_capi {

inline int ensure_stage(sbr_ctx* c, size_t bytes)
{
    if (bytes <= c->stage_bytes) return SBR_OK;
    if (c->stage) (void)hipFree(c->stage);
    c->stage = nullptr;
    c->stage_bytes = 0;
    HIP_TRY(c, hipMalloc(&c->stage, bytes), SBR_ENOMEM);
    c->stage_bytes = bytes;
    return SBR_OK;
}

inline int ensure_res_pin(sbr_ctx* c, size_t bytes)
{
    if (bytes <= c->res_pin_bytes) return SBR_OK;
    if (c->res_pin) (void)hipHostFree(c->res_pin);
    c->res_pin = nullptr;
    c->res_pin_bytes = 0;
    HIP_TRY(c, hipHostMalloc(&c->res_pin, bytes), SBR_ENOMEM);
    c->res_pin_bytes = bytes;
    return SBR_OK;
}

// ---------------------------------------------------------------------------
// Inputs: the input arrays of a call, in the order they are staged.  An entry is per column
// (`w` doubles for each of the call's n columns) or shared by all columns (`w` doubles).  Sizes,
// device pointers, the single-device copies and a rank's share all come from this one list.
// ---------------------------------------------------------------------------
struct InputArray {
    const double* host;
    size_t w;
    bool per_col;
};
inline InputArray cols(const double* host, size_t w = 1) { return {host, w, true}; }
inline InputArray shared(const double* host, size_t len) { return {host, len, false}; }

constexpr int kMaxInputs = 10;
using DevInputs = std::array<const double*, kMaxInputs>; // device pointer of each entry

struct Inputs {
    InputArray a[kMaxInputs];
    int count = 0;
    Inputs(std::initializer_list<InputArray> l)
    {
        for (const InputArray& x : l) a[count++] = x;
    }
    size_t len(int k, size_t n) const { return a[k].per_col ? a[k].w * n : a[k].w; } // doubles of entry k
    size_t bytes(size_t n) const
    {
        size_t d = 0;
        for (int k = 0; k < count; k++) d += len(k, n);
        return d * 8;
    }
    // device pointers of the entries of n columns staged at `base`
    DevInputs dev(const void* base, size_t n) const
    {
        DevInputs p{};
        const double* at = (const double*)base;
        for (int k = 0; k < count; at += len(k, n), k++) p[k] = at;
        return p;
    }
    // single device: one copy per entry from the caller's memory, on s
    int stage(sbr_ctx* c, void* base, size_t n, hipStream_t s) const
    {
        const auto d = dev(base, n);
        for (int k = 0; k < count; k++)
            HIP_TRY(c, hipMemcpyAsync((void*)d[k], a[k].host, len(k, n) * 8, hipMemcpyHostToDevice, s), SBR_EDEVICE);
        return SBR_OK;
    }
    // rank r of N with nc columns (r, r + N, …): its share packed on the host, then one copy
    int stage_rank(void* base, int r, int N, int64_t nc) const
    {
        std::vector<double> h(bytes((size_t)nc) / 8);
        const auto d = dev(h.data(), (size_t)nc);
        for (int k = 0; k < count; k++) {
            if (a[k].per_col) sbr_shard::deal_cols(a[k].host, (int64_t)a[k].w, r, N, nc, (double*)d[k]);
            else memcpy((void*)d[k], a[k].host, a[k].w * 8);
        }
        return hipMemcpy(base, h.data(), h.size() * 8, hipMemcpyHostToDevice) == hipSuccess ? SBR_OK : SBR_EDEVICE;
    }
};

// the staging buffer of a host-pointer call: the inputs of n columns, then res_bytes of results
// on the next 256-byte boundary (*res)
inline int ensure_io(sbr_ctx* c, const Inputs& in, size_t n, size_t res_bytes, void** res)
{
    const size_t off = (in.bytes(n) + 255) & ~(size_t)255;
    const int rc = ensure_stage(c, off + res_bytes);
    if (rc == SBR_OK) *res = (char*)c->stage + off;
    return rc;
}

// ---------------------------------------------------------------------------
// The result block of np points: xi, tau_in_unc, tau_out_unc, aw_max, tol (double), then the
// sweep's int64 step counts where it has them (interest, social), status, iters, and social's
// fp_iters.  Up to and including iters it is one contiguous piece in sbr_result_soa's order
// for the sweeps without step counts.
// ---------------------------------------------------------------------------
inline size_t result_bytes(size_t np, bool steps = false, bool fp_iters = false)
{
    return np * (5 * 8 + (steps ? 8 : 0) + 4 + 4 + (fp_iters ? 4 : 0));
}

inline sbr::ResultSoA carve_results(void* blk, size_t np, int64_t** steps = nullptr, int32_t** fp_iters = nullptr)
{
    double* d = (double*)blk;
    char* at = (char*)(d + 5 * np);
    if (steps) {
        *steps = (int64_t*)at;
        at += np * 8;
    }
    uint32_t* status = (uint32_t*)at;
    int32_t* iters = (int32_t*)(status + np);
    if (fp_iters) *fp_iters = iters + np;
    return {d, d + np, d + 2 * np, d + 3 * np, d + 4 * np, status, iters};
}

// Pinned readback of a block without step counts: one DMA copy into c->res_pin (sized by
// ensure_res_pin(result_bytes(np)); iters only when the caller asked for it) …
inline int readback_enqueue(sbr_ctx* c, const void* blk, size_t np, bool iters, hipStream_t s)
{
    HIP_TRY(c, hipMemcpyAsync(c->res_pin, blk, np * (5 * 8 + 4 + (iters ? 4 : 0)), hipMemcpyDeviceToHost, s),
            SBR_EDEVICE);
    return SBR_OK;
}

// … and, once s has synchronised, scatter_results(c->res_pin, np, out): the fields of a host
// copy of the block into the caller's non-null arrays, on several host threads when it is large
// (nothing is written before the synchronisation succeeded)
inline void scatter_results(const void* blk, size_t np, const sbr_result_soa* out)
{
    const char* P = (const char*)blk;
    std::vector<std::array<size_t, 3>> pieces;
    double* hs[5] = {out->xi, out->tau_in_unc, out->tau_out_unc, out->aw_max, out->tol};
    for (int k = 0; k < 5; k++)
        if (hs[k]) pieces.push_back({(size_t)hs[k], (size_t)(P + (size_t)k * np * 8), np * 8});
    if (out->status) pieces.push_back({(size_t)out->status, (size_t)(P + 5 * np * 8), np * 4});
    if (out->iters) pieces.push_back({(size_t)out->iters, (size_t)(P + 5 * np * 8 + np * 4), np * 4});
    sbr_host::parallel_copy(pieces);
}

// Direct readback (interest, hetero, social): one copy per field the caller asked for, on s
struct OutField {
    void* host;
    const void* dev;
    size_t bytes;
};
inline int copy_out(sbr_ctx* c, hipStream_t s, std::initializer_list<OutField> fields)
{
    for (const OutField& f : fields)
        if (f.host) HIP_TRY(c, hipMemcpyAsync(f.host, f.dev, f.bytes, hipMemcpyDeviceToHost, s), SBR_EDEVICE);
    return SBR_OK;
}

// the seven fields of the device SoA d into the caller's out
inline int copy_out(sbr_ctx* c, hipStream_t s, const sbr_result_soa* out, const sbr::ResultSoA& d, size_t np)
{
    return copy_out(c, s, {{out->xi, d.xi, np * 8}, {out->tau_in_unc, d.tau_in_unc, np * 8},
                           {out->tau_out_unc, d.tau_out_unc, np * 8}, {out->aw_max, d.aw_max, np * 8},
                           {out->tol, d.tol, np * 8}, {out->status, d.status, np * 4}, {out->iters, d.iters, np * 4}});
}

inline sbr::ResultSoA device_soa(const sbr_result_soa* o)
{
    return {o->xi, o->tau_in_unc, o->tau_out_unc, o->aw_max, o->tol, o->status, o->iters};
}

inline void early_exit(const sbr_opts& o, int64_t n_line, int64_t n_u, sbr_result_soa* out)
{
    if (o.early_exit_nan_run > 0 && out->status && out->xi && out->aw_max && out->tol)
        sbr_apply_early_exit(n_line, n_u, o.early_exit_nan_run, out);
}

// ---------------------------------------------------------------------------
// n-device contexts: the host-pointer sweeps fan out over the ranks (sbr_multi.hip).
// Inputs of column i go to rank i mod N; each rank runs the single-device *_dev
// entry point on its GPU; the packed results come back over RCCL or by direct copies.
// ---------------------------------------------------------------------------
using sbr_multi_impl::FieldSpec;

// the fields of an sbr_result_soa, one value per point each …
inline std::vector<FieldSpec> result_fields(const sbr_result_soa* o)
{
    return {{o->xi, 8, 1},  {o->tau_in_unc, 8, 1}, {o->tau_out_unc, 8, 1}, {o->aw_max, 8, 1},
            {o->tol, 8, 1}, {o->status, 4, 1},     {o->iters, 4, 1}};
}
// … and a rank's sbr_result_soa from the device pointers run() gets for them
inline sbr_result_soa rank_results(const std::vector<void*>& f)
{
    return {(double*)f[0], (double*)f[1], (double*)f[2], (double*)f[3], (double*)f[4], (uint32_t*)f[5], (int32_t*)f[6]};
}

// n_col columns of per_col points each over the ranks: every rank stages its share of `in`, and
// run(child, stream, nc, d, f) enqueues its nc columns' sweep on the staged inputs' device
// pointers d[k] and the fields' device pointers f[k]
template <class Run>
int fan_out(sbr_ctx* c, const Inputs& in, int64_t n_col, int64_t per_col, const std::vector<FieldSpec>& fields,
            const sbr_opts& o, Run&& run)
{
    const int N = sbr_multi_impl::size(c->multi);
    const int64_t cmax = (n_col + N - 1) / N;
    auto stage = [&](int r, int64_t nc, void* dev, hipStream_t) { return in.stage_rank(dev, r, N, nc); };
    auto go = [&](int, int64_t nc, sbr_ctx* kid, hipStream_t s, void* dev, const std::vector<void*>& f) -> int {
        return run(kid, s, nc, in.dev(dev, (size_t)nc), f);
    };
    const int rc = sbr_multi_impl::run_sharded(c->multi, n_col, per_col, fields, in.bytes((size_t)cmax), stage, go,
                                               (o.flags & SBR_FLAG_RCCL_GATHER) != 0);
    return rc ? fail(c, rc, sbr_multi_impl::last_error(c->multi)) : SBR_OK;
}

}  // namespace sbr_capi
