// sbr_social_plan.h — the launch arithmetic of the social iterate kernel, stated once:
// launch_social_iter (host) sizes the grid with it, social_iter_kernel (device) derives each
// wave's lane count from it, and sbr_social_plan exports it for the CPU tests.
//
// A launch has `nmain` main blocks (one wave each) followed by the promotion pool's blocks.
// While at most `nmain` points are live every point gets a whole wave (L = 1, SocialRhsCoop);
// above that the first `nbs` waves share the worklist, L = ⌈live / nbs⌉ consecutive entries per
// wave, one per lane (SocialRhsRing).  The ring holds kRingLanes lanes, so nbs is never below
// ⌈n_pts / kRingLanes⌉ whatever number of waves is asked for: every worklist entry has a lane.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SBR_PLAN_HD __host__ __device__
#else
#define SBR_PLAN_HD
#endif

namespace sbr {

constexpr int kRingLanes = 32; // lanes a multi-point wave may use (the plan makes L <= this)
constexpr int kSocialWaves = 1024; // one wave per SIMD (2048 waves, two per SIMD, were slower: r04_u)
// live points up to which every point gets a whole wave (SocialRhsCoop), in rounds of the
// kSocialWaves resident ones, instead of ⌈live/kSocialWaves⌉ points per wave
constexpr int kSocialCoopMax = 4096;

struct SocialPlan {
    int nbs;   // waves that share the worklist in the multi-point mode
    int nmain; // main blocks of the launch: live <= nmain runs one point per wave
};

// coop_max < 0: kSocialCoopMax; waves < 1: kSocialWaves (the schedule override of
// sbr_set_social_schedule passes its values here, −1 when unset)
SBR_PLAN_HD inline SocialPlan social_plan(int n_pts, int coop_max, int waves)
{
    if (coop_max < 0) coop_max = kSocialCoopMax;
    if (waves < 1) waves = kSocialWaves;
    // main blocks: one wave per SIMD of the MI355X (4 × 256), at least one wave per kRingLanes
    // points and no more than one per point
    int nbs = (n_pts + kRingLanes - 1) / kRingLanes; // L = ⌈live / nbs⌉ <= kRingLanes (the ring's lanes)
    nbs = nbs > waves ? nbs : waves;
    nbs = nbs < n_pts ? nbs : (n_pts > 0 ? n_pts : 1);
    // nbs multi-point waves, or up to coop_max one-point waves
    coop_max = coop_max < n_pts ? coop_max : n_pts;
    return SocialPlan{nbs, nbs > coop_max ? nbs : coop_max};
}

// lanes per wave for `live` worklist entries: 1 = one point per wave (the whole wave runs it)
SBR_PLAN_HD inline int social_plan_lanes(int live, int nbs, int nmain)
{
    int L = live <= nmain ? 1 : (live + nbs - 1) / nbs;
    // social_plan's nbs >= ⌈n_pts / kRingLanes⌉ >= ⌈live / kRingLanes⌉ keeps L within the ring;
    // the clamp stops a change of that arithmetic from letting lanes share ring slots (which
    // in_ring() would trust)
    return L < 1 ? 1 : (L > kRingLanes ? kRingLanes : L);
}

} // namespace sbr
