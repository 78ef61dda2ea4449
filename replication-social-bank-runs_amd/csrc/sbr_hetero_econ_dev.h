// sbr_hetero_econ_dev.h — what the kernels of sbr_sweep_hetero_econ share (sbr_hetero_econ.hip,
// sbr_hetero_econ_wide.hip): a hazard class's parameter rule.
#pragma once

#include "sbr_device.h"
#include "sbr_kernels.h"

namespace sbr {

// EconomicParameters' rules for p and λ (model.jl:71-76); a NaN breaks its rule
__device__ __forceinline__ bool hetero_econ_class_bad(const double p, const double lam)
{
    return !(p >= 0.0 && p <= 1.0) || !(lam > 0.0);
}

}  // namespace sbr
