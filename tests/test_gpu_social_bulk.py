"""GPU parity of the social sweep's multi-point-per-wave path (sbr_social.hip
social_iterate<false>: SocialRhsRing's per-lane LDS ring, the pairwise hazard / crossing scan,
the pairwise damping loop, promote() called from several lanes of a wave, WalkerV, and the
worklist split w = block·L + lane) against the CPU oracle, bit for bit on every output field,
status bit, bisection count and fixed-point iteration count.

The built-in schedule gives every point a whole wave (social_iterate<true>) until more than
4,096 points are live, so the other GPU tests — at most 1,024 points — never reach this path.
Here Engine.social_schedule(coop_max, waves, inner) forces it on small grids (the schedule does
not change results), one test runs 4,160 points under the built-in schedule, and every case
asserts with Engine.social_schedule_stats() which mode ran its point-iterates, so that a case
cannot pass through the one-point path.

Grid G65: 5 β × 13 u of BASELINE config 5's axes (65 points, odd, so the last wave is partial),
η = 30/0.9, p = 0.99, κ = λ = 0.25, the 1000-point comparison grid.  The oracle runs once per
(tol, max_iter) for the module (< 1.5 s each); larger grids repeat G65's u axis and their
reference is G65's result repeated, which also pins that a point's bits do not depend on its
lane, wave or ring slot.

The 64-point case (L = 32, the ring's full lane count) is a 4 β × 16 u grid of G65 points —
G65's last four β rows, its 13 u and three of them again — because the sweep takes
rectangular grids only, which 65 − 1 points are not.

Wall times on the MI355X (pytest --durations=0; the module takes 15 s, target <= 10 s a test and
<= 60 s the module): OOB 4.0 s, g65[e] 2.4 s, g65[a] 1.6 s + 1.6 s setup (the oracle runs),
g65[b] 1.1 s, default schedule above 4,096 points 1.0 s, promotion[4096] 1.0 s, full ring 1.0 s,
g65[c] 0.6 s, pool exhausted 0.3 s, promotion[8192] 0.3 s.  A multi-point lane at this low
occupancy takes about 2.5 µs per RK step, not the 17 µs of config 5's full load.

Left out: tests/golden/config5_sample.npz (32 points, full workload) under schedule (0, 1, −1).
It is bitwise equal to the fixture there too (1,360 point-iterates in lanes, 80 in one-point
waves), but takes 44 s against 21 s under the built-in schedule — over the budget of a test.
"""
import numpy as np
import pytest

import sbr

pytestmark = pytest.mark.gpu

FIELDS = ("xi", "tau_in_unc", "tau_out_unc", "aw_max", "tol")
ETA = 30.0 / 0.9
P, KAPPA, LAM = 0.99, 0.25, 0.25
S = sbr.STATUS

BETA_AXIS = 1.0 / sbr.julia_range("0.01", "2", 512)
U_AXIS = sbr.julia_range("0.001", "1", 512)
CMP = sbr.julia_range(0.0, ETA, 1000)
G65_B = [0, 40, 128, 300, 511]
G65_U = [0, 2, 3, 6, 25, 60, 100, 140, 200, 255, 300, 400, 511]
# the knot-overflow grid of test_gpu_social.py::test_social_knot_overflow_promotion_and_rerun
PROMO_B, PROMO_U = [0, 128, 511], [25, 140, 511]
# (β[40], u[6]) ends in the reference's BoundsError (tools/social_oob_scan.py); its 8 neighbours do not
OOB_B, OOB_U = [0, 40, 128], [2, 6, 25]


def assert_bitwise(a, b, name):
    a = np.asarray(a)
    b = np.asarray(b)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)
    if not same.all():
        idx = np.argwhere(~same)[:5]
        raise AssertionError(f"{name}: {int((~same).sum())} mismatches, e.g. "
                             f"{[(tuple(i), a[tuple(i)], b[tuple(i)]) for i in idx]}")


def _compare(g, o):
    for k in FIELDS:
        assert_bitwise(g[k], o[k], k)
    assert_bitwise(g["status"], o["status"], "status")
    assert_bitwise(g["iters"], o["iters"], "bisection iterations")
    assert_bitwise(g["fp_iters"], o["fp_iters"], "fixed-point iterations")


def _sweep(engine, bi, ui, tol, max_iter, **kw):
    return engine.sweep_social(BETA_AXIS[bi], ETA, U_AXIS[ui], P, KAPPA, LAM, cmp=CMP, tol=tol, max_iter=max_iter,
                               **kw)


def _take(o, rows, cols):
    """The results of the grid rows × cols (indices into o's axes, repeats allowed)."""
    return {k: v[np.ix_(rows, cols)] for k, v in o.items()}


@pytest.fixture(scope="module")
def ref(oracle):
    """Oracle results per (β indices, u indices, tol, max_iter), computed once and read-only."""
    cache = {}

    def get(bi, ui, tol, max_iter):
        key = (tuple(bi), tuple(ui), tol, max_iter)
        if key not in cache:
            o = oracle.sweep_social(BETA_AXIS[bi], ETA, U_AXIS[ui], P, KAPPA, LAM, CMP, tol=tol, max_iter=max_iter,
                                    stats=True)
            for v in o.values():
                v.setflags(write=False)
            cache[key] = o
        return cache[key]

    return get


@pytest.fixture(scope="module")
def default_run(engine, ref):
    """The same sweeps under the built-in schedule (every point a whole wave: stats[0] == 0),
    for rk_steps, which the oracle does not return; each checked against the oracle."""
    cache = {}

    def get(bi, ui, tol, max_iter):
        key = (tuple(bi), tuple(ui), tol, max_iter)
        if key not in cache:
            g = _sweep(engine, bi, ui, tol, max_iter)
            o = ref(bi, ui, tol, max_iter)
            assert engine.social_schedule_stats() == [0, int(o["fp_iters"].sum()), 0]
            _compare(g, o)
            cache[key] = g
        return cache[key]

    return get


def _g65_facts(o, tol, max_iter):
    """The properties of the oracle's result that the cases below exist for."""
    fp, st = o["fp_iters"], o["status"]
    if (tol, max_iter) == (0.48, 3):
        early = np.zeros((5, 13), bool)
        early[4, :4] = True  # β index 511, the first four u
        assert np.array_equal(fp == 2, early) and np.array_equal(fp == 3, ~early)
        assert (st == (S["SBR_RUN"] | S["SBR_CONVERGED"])).any()
        assert (st == (S["SBR_NO_RUN_HR_BELOW_U"] | S["SBR_CONVERGED"])).any()
        odd = (o["n_knots"] % 2).mean()  # the pairwise loops' odd-n tails and even-n ends
        assert 0.3 < odd < 0.7, odd
        steps = (o["n_accept"] + o["n_reject"]).max()  # the time budget: the longest last iterate
        assert 1.5e5 < steps < 3.5e5, steps
    elif (tol, max_iter) == (0.18, 4):
        maxiter = st == (S["SBR_NO_RUN_MAXITER"] | S["SBR_SOCIAL_NOT_CONVERGED"])
        assert maxiter.sum() == 1 and (fp == 4).all()
        assert ((st[~maxiter] & S["SBR_CONVERGED"]) != 0).all()
    elif (tol, max_iter) == (0.48, 2):
        assert (fp == 2).all() and ((o["n_knots"] % 2) == 1).any() and ((o["n_knots"] % 2) == 0).any()


CASES = {
    # name: (schedule, tol, max_iter, live counts → L of each launch's plan, stats)
    "a_one_iterate_per_launch": ((0, 1, 1), 0.48, 3, {65: 22, 61: 21}, [191, 0, 0]),
    "b_one_launch_idle_lanes": ((0, 1, -1), 0.48, 3, {65: 22}, [191, 0, 0]),
    "c_multi_to_one_point_transition": ((0, 61, 1), 0.48, 3, {65: 2, 61: 1}, [130, 61, 0]),
    "e_bisection_maxiter_point": ((0, 1, -1), 0.18, 4, {65: 22}, [260, 0, 0]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_bulk_g65(engine, ref, default_run, case):
    """G65 through multi-point waves.  a: nbs = 3, L = 22 then 21, three launches with a
    compaction after the four early retirements.  b: one launch, so the four points that
    converge at iterate 2 retire while their wave neighbours go on (idle lanes beside running
    ones).  c: L = 2 for iterates 1–2 (65 live > 61), one point per wave for iterate 3 (61
    live): the multi→one-point transition across a compaction.  e: a point whose bisection ends
    SBR_NO_RUN_MAXITER inside a multi-point wave."""
    sched, tol, max_iter, lanes, stats = CASES[case]
    o = ref(G65_B, G65_U, tol, max_iter)
    _g65_facts(o, tol, max_iter)
    assert stats[0] + stats[1] == o["fp_iters"].sum()
    for live, L in lanes.items():
        assert sbr.social_plan(65, live, sched[0], sched[1])["L"] == L
    with engine.social_schedule(*sched):
        g = _sweep(engine, G65_B, G65_U, tol, max_iter)
        got = engine.social_schedule_stats()
    assert got == stats, f"point-iterates per mode {got}, expected {stats}: the case ran another path"
    _compare(g, o)
    assert_bitwise(g["rk_steps"], default_run(G65_B, G65_U, tol, max_iter)["rk_steps"], "rk_steps")


def test_bulk_full_ring_32_lanes(engine, ref, default_run):
    """d: 64 points in two waves of L = 32 lanes, the ring's full lane count (see the module
    docstring for the grid), max_iter = 2."""
    rows, cols = [1, 2, 3, 4], list(range(13)) + [4, 8, 12]
    bi, ui = [G65_B[r] for r in rows], [G65_U[c] for c in cols]
    full = ref(G65_B, G65_U, 0.48, 2)
    _g65_facts(full, 0.48, 2)
    o = _take(full, rows, cols)
    assert sbr.social_plan(64, 64, 0, 1) == dict(nbs=2, nmain=2, L=32, grid=2)
    with engine.social_schedule(0, 1, -1):
        g = _sweep(engine, bi, ui, 0.48, 2)
        got = engine.social_schedule_stats()
    assert got == [128, 0, 0], got
    _compare(g, o)
    assert_bitwise(g["rk_steps"], _take(default_run(G65_B, G65_U, 0.48, 2), rows, cols)["rk_steps"], "rk_steps")


def test_bulk_oob_point_in_a_multi_point_wave(engine, ref, default_run):
    """The reference's BoundsError (SBR_OOB) in one lane of a nine-lane wave: (β[40], u[6])
    stops at iterate 8 with SBR_OOB | SBR_SOCIAL_NOT_CONVERGED, its eight neighbours do not."""
    o = ref(OOB_B, OOB_U, 1e-4, 8)
    oob = (o["status"] & S["SBR_OOB"]) != 0
    centre = np.zeros((3, 3), bool)
    centre[1, 1] = True
    assert np.array_equal(oob, centre) and (o["fp_iters"] == 8).all()
    assert o["status"][1, 1] == S["SBR_OOB"] | S["SBR_SOCIAL_NOT_CONVERGED"]
    assert sbr.social_plan(9, 9, 0, 1)["L"] == 9
    with engine.social_schedule(0, 1, -1):
        g = _sweep(engine, OOB_B, OOB_U, 1e-4, 8)
        got = engine.social_schedule_stats()
    assert got == [72, 0, 0], got
    assert np.array_equal((g["status"] & S["SBR_OOB"]) != 0, centre)
    _compare(g, o)
    assert_bitwise(g["rk_steps"], default_run(OOB_B, OOB_U, 1e-4, 8)["rk_steps"], "rk_steps")


@pytest.mark.parametrize("cap", [4096, 8192])
def test_bulk_promotion_from_lanes(engine, oracle, ref, default_run, cap):
    """Every lane of a wave whose point has started overflows the knot capacity in iterate 1
    (>= 18,029 knots) and calls promote() in the same wave (in the one-point path only lane 0
    does); the pool redoes the iterates.  At 8192 knots that is all nine lanes.  At 4096 the
    three β = 100 points never start: their AW_0 (the baseline learning, 4,536 knots) already
    overflows in the init kernel, whatever the schedule, so six lanes promote and three points
    are re-run from scratch — also through lanes.  Results equal the oracle, rk_steps the
    default-capacity, default-schedule run."""
    o = ref(PROMO_B, PROMO_U, 1e-4, 2)
    n_aw0 = np.array([len(oracle.learn_logistic(b, ETA, 1e-4)[0]) for b in BETA_AXIS[PROMO_B]])
    assert (o["fp_iters"] == 2).all() and (o["n_knots"] > 8192).all() and (n_aw0 <= 8192).all()
    rerun = 3 * int((n_aw0 > cap).sum())
    assert rerun == {4096: 3, 8192: 0}[cap]
    assert sbr.social_plan(9, 9, 0, 1)["L"] == 9 and sbr.social_plan(3, 3, 0, 1)["L"] == 3
    with engine.social_schedule(0, 1, -1):
        g = _sweep(engine, PROMO_B, PROMO_U, 1e-4, 2, knot_capacity=cap)
        got = engine.social_schedule_stats()
        over = engine.social_overflow_stats()
    assert over == dict(promoted=9 - rerun, rerun=rerun), over
    # iterate 1 attempted by the lanes of the points that started, then both iterates of each of
    # them by pool waves; both iterates of the re-run points by lanes
    assert got == [9 - rerun + 2 * rerun, 0, 2 * (9 - rerun)], got
    _compare(g, o)
    assert not (g["status"] & S["SBR_KNOT_OVERFLOW"]).any()
    assert_bitwise(g["rk_steps"], default_run(PROMO_B, PROMO_U, 1e-4, 2)["rk_steps"], "rk_steps")


def test_bulk_pool_exhausted_from_lanes(engine, oracle, ref):
    """325 points (G65's u axis five times) at 4096 knots, max_iter = 1.  The 65 β = 100 points
    overflow in the init kernel (AW_0 has 4,536 knots); the lanes of the other 260, spread over
    ten waves, all overflow in iterate 1 and race for the pool's 256 slots.  Those that find the
    pool full retire with SBR_KNOT_OVERFLOW and are re-run from scratch at a larger capacity
    with the init overflows."""
    reps = 5
    o65 = ref(G65_B, G65_U, 0.48, 1)
    assert (o65["n_knots"] > 4096).all() and (o65["fp_iters"] == 1).all()
    n_aw0 = np.array([len(oracle.learn_logistic(b, ETA, 1e-4)[0]) for b in BETA_AXIS[G65_B]])
    started = 13 * reps * int((n_aw0 <= 4096).sum())
    assert started == 260
    o = {k: np.tile(v, (1, reps)) for k, v in o65.items()}
    assert sbr.social_plan(325, 325, 0, 1)["L"] == 30
    with engine.social_schedule(0, 1, -1):
        g = _sweep(engine, G65_B, G65_U * reps, 0.48, 1, knot_capacity=4096)
        got = engine.social_schedule_stats()
        over = engine.social_overflow_stats()
    assert over["promoted"] + over["rerun"] == 325 and over["promoted"] > 0 and over["rerun"] > 0, over
    assert over["promoted"] < started, (over, "the pool had a slot for every lane that overflowed")
    # every started point once in a lane, the promoted ones again in the pool, the rest — and the
    # init overflows — once more in lanes
    assert got == [started + over["rerun"], 0, over["promoted"]], (got, over)
    assert not (g["status"] & S["SBR_KNOT_OVERFLOW"]).any()
    _compare(g, o)


def test_bulk_default_schedule_above_4096_points(engine, ref, default_run):
    """No override: 4,160 points (G65's u axis 64 times) exceed the 4,096 live points up to
    which a point gets a whole wave, so the built-in schedule runs L = 5 lanes in each of 1,024
    waves.  If the workspace had chunked the grid below 4,097 points, the mode counts say so."""
    reps = 64
    o65 = ref(G65_B, G65_U, 0.48, 2)
    _g65_facts(o65, 0.48, 2)
    o = {k: np.tile(v, (1, reps)) for k, v in o65.items()}
    assert sbr.social_plan(65 * reps, 65 * reps) == dict(nbs=1024, nmain=4096, L=5, grid=4096)
    g = _sweep(engine, G65_B, G65_U * reps, 0.48, 2, workspace_bytes=0)
    got = engine.social_schedule_stats()
    want = [int(o["fp_iters"].sum()), 0, 0]
    assert got == want, (f"point-iterates per mode {got}, expected {want}: the sweep did not run as one chunk of "
                         "4,160 points through multi-point waves (workspace too small?)")
    _compare(g, o)
    steps = np.tile(default_run(G65_B, G65_U, 0.48, 2)["rk_steps"], (1, reps))
    assert_bitwise(g["rk_steps"], steps, "rk_steps")


def test_schedule_override_does_not_outlive_its_block(engine):
    """The session's engine is back on the built-in schedule after every `with` block above:
    nine points run one per wave again."""
    with pytest.raises(RuntimeError):
        with engine.social_schedule(0, 1, 1):
            raise RuntimeError("leave the block by an exception")
    _sweep(engine, PROMO_B, PROMO_U, 0.48, 1)
    assert engine.social_schedule_stats() == [0, 9, 0]
