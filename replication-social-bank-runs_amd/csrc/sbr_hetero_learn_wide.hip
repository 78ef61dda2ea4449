// sbr_hetero_learn_wide.hip — the heterogeneity learning wave and hazard pass (sbr_hetero_learn_dev.h)
// instantiated for the group counts sbr_hetero.hip does not specialise: K = 5, 6, 7 and 9 … 16
// (SBR_HETERO_MAX_K).  The same templates, so the same operation sequence — the K×K row-distributed
// LU included — as the K = 1, 2, 3, 4, 8 kernels; kernels of their own name and translation unit,
// so that adding them leaves the machine code (and the per-kernel code hashes) of
// learn_hetero_wave_kernel / hazard_hetero_kernel as they were.
#define SBR_HET_LEARN_KERNEL learn_hetero_wide_kernel
#define SBR_HET_HAZARD_KERNEL hazard_hetero_wide_kernel
#include "sbr_hetero_learn_dev.h"

namespace sbr {

template <int K>
static hipError_t launch_learn_wide_k(const double* betas, const double* dist, const double* eta, const double* t_end,
                                      const LearnArgs& la, const HeteroBufs& L, hipStream_t s, int phase)
{
    if (phase == 2) // hazards of knots already in L (caller knots)
        hipLaunchKernelGGL(hazard_hetero_wide_kernel<K>, dim3(la.n_beta), dim3(64), 0, s, betas, dist, eta, la, L);
    else
        hipLaunchKernelGGL(learn_hetero_wide_kernel<K>, dim3((la.n_beta + kHetLearnWG - 1) / kHetLearnWG),
                           dim3(64 * kHetLearnWG), 0, s, betas, dist, eta, t_end, la, L);
    return hipGetLastError();
}

hipError_t launch_hetero_learn_wide(int K, const double* betas, const double* dist, const double* eta,
                                    const double* t_end, const LearnArgs& la, const HeteroBufs& L, hipStream_t s,
                                    int phase)
{
    if (phase != 0 && phase != 2) return hipErrorInvalidValue;
    switch (K) {
    case 5: return launch_learn_wide_k<5>(betas, dist, eta, t_end, la, L, s, phase);
    case 6: return launch_learn_wide_k<6>(betas, dist, eta, t_end, la, L, s, phase);
    case 7: return launch_learn_wide_k<7>(betas, dist, eta, t_end, la, L, s, phase);
    case 9: return launch_learn_wide_k<9>(betas, dist, eta, t_end, la, L, s, phase);
    case 10: return launch_learn_wide_k<10>(betas, dist, eta, t_end, la, L, s, phase);
    case 11: return launch_learn_wide_k<11>(betas, dist, eta, t_end, la, L, s, phase);
    case 12: return launch_learn_wide_k<12>(betas, dist, eta, t_end, la, L, s, phase);
    case 13: return launch_learn_wide_k<13>(betas, dist, eta, t_end, la, L, s, phase);
    case 14: return launch_learn_wide_k<14>(betas, dist, eta, t_end, la, L, s, phase);
    case 15: return launch_learn_wide_k<15>(betas, dist, eta, t_end, la, L, s, phase);
    case 16: return launch_learn_wide_k<16>(betas, dist, eta, t_end, la, L, s, phase);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace sbr
