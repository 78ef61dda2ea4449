// sbr_econ_dev.h — what the kernels of the economic-parameter products share (sbr_econ.hip,
// sbr_interest_econ.hip): a hazard class's view of the learning buffers and its parameter rule.
#pragma once

#include "sbr_device.h"
#include "sbr_kernels.h"

namespace sbr {

// the learning buffers as class k of the chunk sees them: the column's knots, the class's rows
__device__ __forceinline__ LearnBufs econ_class_bufs(const LearnBufs& L, const EconArgs& e, const int k)
{
    LearnBufs C = L;
    const size_t r0 = (size_t)k * (size_t)e.n_beta;
    C.hr = e.hr + r0 * (size_t)L.cap;
    C.n_tau = e.n_tau + r0;
    C.n_le = e.n_le + r0;
    C.status = e.status + r0;
    return C;
}

// EconomicParameters' rules for p and λ (model.jl:71-76); a NaN breaks its rule
__device__ __forceinline__ bool econ_class_bad(const double p, const double lam)
{
    return !(p >= 0.0 && p <= 1.0) || !(lam > 0.0);
}

}  // namespace sbr
