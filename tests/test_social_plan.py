"""The launch arithmetic of the social iterate kernel (csrc/sbr_social_plan.h), through the
exported host functions sbr_social_plan / sbr_social_plan_lanes — no GPU needed.

launch_social_iter sizes the grid with this arithmetic and social_iter_kernel derives each wave's
lane count L from it.  A wave's LDS ring holds 32 lanes, and a worklist entry past nbs·L is never
run, so whatever schedule is asked for: 1 <= L <= 32, and every live entry has a lane."""
import numpy as np
import pytest

import sbr

RING_LANES, WAVES, COOP_MAX = 32, 1024, 4096  # kRingLanes, kSocialWaves, kSocialCoopMax

SMALL = range(1, 4201)
LARGE = (8192, 32768, 1 << 20)


def _schedules(n_pts):
    return ((-1, -1), (0, 1), (0, 61), (0, n_pts), (4096, 1))


def _check(n_pts, live, coop_max, waves):
    """The plan's properties for one chunk size and schedule, at every entry of `live`."""
    pl = sbr.social_plan(n_pts, int(live[-1]), coop_max, waves)
    nbs, nmain, grid = pl["nbs"], pl["nmain"], pl["grid"]
    L = sbr.social_plan_lanes(n_pts, live, coop_max, waves).astype(np.int64)
    tag = (n_pts, coop_max, waves, pl)
    assert L[-1] == pl["L"], tag  # the scalar and the array entry point agree
    assert nbs >= 1 and nbs >= -(-n_pts // RING_LANES), tag
    assert grid >= max(nbs, nmain), tag
    assert ((L >= 1) & (L <= RING_LANES)).all(), tag
    assert ((L == 1) == (live <= nmain)).all(), tag
    multi = L > 1
    assert (nbs * L[multi] >= live[multi]).all(), tag  # every worklist entry has a lane
    assert (live[~multi] <= nmain).all(), tag          # one point per wave: a block for every entry
    return pl, L


def _old_plan(n_pts, live):
    """The formulas as launch_social_iter and social_iter_kernel stated them before the shared header."""
    nbs = (n_pts + 32 - 1) // 32
    nbs = nbs if nbs > 1024 else 1024
    nbs = nbs if nbs < n_pts else (n_pts if n_pts > 0 else 1)
    coop_max = 4096 if 4096 < n_pts else n_pts
    nmain = nbs if nbs > coop_max else coop_max
    L = np.where(live <= nmain, 1, (live + nbs - 1) // nbs)
    L = np.where(L < 1, 1, np.where(L > 32, 32, L))
    return nbs, nmain, L, nmain


def test_plan_properties_every_size_to_4200():
    for n_pts in SMALL:
        live = np.arange(1, n_pts + 1, dtype=np.int64)
        for coop_max, waves in _schedules(n_pts):
            _check(n_pts, live, coop_max, waves)


@pytest.mark.parametrize("n_pts", LARGE)
def test_plan_properties_large_chunks(n_pts):
    """Strided live counts, plus the counts around every threshold the arithmetic has."""
    edges = [1, 2, 61, 62, WAVES - 1, WAVES, WAVES + 1, COOP_MAX - 1, COOP_MAX, COOP_MAX + 1, n_pts - 1, n_pts]
    nbs_min = -(-n_pts // RING_LANES)
    edges += [nbs_min * k + d for k in (1, 2, 31, 32) for d in (-1, 0, 1)]
    live = np.unique(np.concatenate([np.arange(1, n_pts + 1, 251), edges]))
    live = live[(live >= 1) & (live <= n_pts)].astype(np.int64)
    for coop_max, waves in _schedules(n_pts):
        _check(n_pts, live, coop_max, waves)


def test_default_plan_equals_the_previous_formulas():
    for n_pts in list(SMALL) + list(LARGE) + [1 << 30]:
        step = 1 if n_pts <= 4200 else 251
        live = np.unique(np.concatenate([np.arange(1, n_pts + 1, step), [n_pts]])).astype(np.int64)
        if n_pts > 4200:
            live = live[:: max(1, len(live) // 5000)]
        nbs, nmain, L, grid = _old_plan(n_pts, live)
        pl = sbr.social_plan(n_pts, int(live[-1]))
        assert (pl["nbs"], pl["nmain"], pl["grid"]) == (nbs, nmain, grid), n_pts
        assert np.array_equal(sbr.social_plan_lanes(n_pts, live), L), n_pts
    # the figures the GPU tests of the multi-point path rely on (tests/test_gpu_social_bulk.py)
    assert sbr.social_plan(4160, 4160) == dict(nbs=1024, nmain=4096, L=5, grid=4096)
    assert sbr.social_plan(4096, 4096)["L"] == 1 and sbr.social_plan(4097, 4097)["L"] == 5
    assert sbr.social_plan(32768, 32768)["L"] == 32 and sbr.social_plan(32768, 4096)["L"] == 1


def test_override_plans_of_the_gpu_cases():
    assert sbr.social_plan(65, 65, 0, 1) == dict(nbs=3, nmain=3, L=22, grid=3)
    assert sbr.social_plan(65, 61, 0, 1)["L"] == 21
    assert sbr.social_plan(65, 65, 0, 61) == dict(nbs=61, nmain=61, L=2, grid=61)
    assert sbr.social_plan(65, 61, 0, 61)["L"] == 1
    assert sbr.social_plan(64, 64, 0, 1) == dict(nbs=2, nmain=2, L=32, grid=2)
    assert sbr.social_plan(9, 9, 0, 1) == dict(nbs=1, nmain=1, L=9, grid=1)
    assert sbr.social_plan(325, 325, 0, 1) == dict(nbs=11, nmain=11, L=30, grid=11)


def test_plan_rejects_bad_arguments():
    for args in ((0, 0, -1, -1), (5, 6, -1, -1), (5, -1, -1, -1), (5, 5, -1, 0)):
        with pytest.raises(sbr.ArgumentError):
            sbr.social_plan(*args)
    L = sbr.load()
    assert L.sbr_set_social_schedule(None, 0, 1, 1) == sbr._lib.SBR_EARG
    assert L.sbr_social_schedule_stats(None, None) == sbr._lib.SBR_EARG
