"""GPU parity of every ODE loop with sbr_opts.ode_reltol / ode_abstol / ode_maxiters / knot_capacity
off their defaults, against the CPU oracle run with the same options: every result field, status
bit, bisection count (and rk_steps / fp_iters where a sweep reports them) bit for bit.

At the reference's eps() tolerances the scalar integrator never leaves Tsit5 and no solve comes
near an iteration cap, so the default-option tests never run
  * the Rosenbrock23 branch of ode_scalar in the sweep learning kernel (plain sink, fused-hazard
    sink, the batch's LDS ring), the points kernel, the interest value function (ValueRhs::jac,
    the ros23_dense arm of the saver) and the social forced ODE;
  * SBR_ODE_MAXITERS anywhere on the device, and the equilibrium kernels on a grid it cut short;
  * a value-function solve that stops before the end of the HR grid (n_v < n_tau);
  * columns of 11 to 62 knots in the sweep kernels (block summaries, AW window, ring flushes);
  * SBR_KNOT_OVERFLOW outside the social sweep.
Each test first asserts ON THE ORACLE'S OUTPUT that its inputs reach the path it is for (the
"coverage" assertions: status counts, knot counts, stiff bits measured on the oracle), so a test
whose inputs stopped reaching the path fails instead of passing for nothing.

Option sets are (rtol, atol, ode_maxiters); E = eps(), M = 1,000,000 (the defaults).  The oracle
runs once per (case, option set) for the module; every run takes under 0.2 s.

Shapes: the baseline grid is 7 β × 33 u.  A 7-column sweep takes the one-stream schedule, so the
three-chunk schedule (≥ 192 columns) and the readiness schedule (≥ 64 columns) run on the same
seven β repeated to 196 columns, their reference the 7-column result repeated; the batch's LDS
ring needs a first learning launch of ≥ 256 waves, here 11 grids × 1,536 columns of 21 distinct β.

Wall time on the MI355X: 3.7 s for the module's 95 cases (the slowest 0.4 s; 1.7 s of set-up is
the session's first engine).
"""
import numpy as np
import pytest

import sbr

pytestmark = pytest.mark.gpu

FIELDS = ("xi", "tau_in_unc", "tau_out_unc", "aw_max", "tol")
S = sbr.STATUS
E = float(np.finfo(np.float64).eps)
M = 1_000_000
P, KAPPA, LAM = 0.5, 0.6, 0.01
ETA, T_END = 15.0, 30.0

RUN, CONV, HRLOW, COLLAPSE, BMAX, FALSE_EQ = (S["SBR_RUN"], S["SBR_CONVERGED"], S["SBR_NO_RUN_HR_BELOW_U"],
                                              S["SBR_NO_RUN_COLLAPSE"], S["SBR_NO_RUN_MAXITER"], S["SBR_FALSE_EQ"])
OOB, MAXIT, STIFF, OVER, NOTCONV = (S["SBR_OOB"], S["SBR_ODE_MAXITERS"], S["SBR_STIFF_SWITCH"],
                                    S["SBR_KNOT_OVERFLOW"], S["SBR_SOCIAL_NOT_CONVERGED"])
TRUNC = S["SBR_ENGINE_TRUNC"]

TOL_SETS = [(1e-10, 1e-10, M), (1e-6, 1e-6, M), (1e-3, 1e-3, M), (1e-6, 1e-12, M)]
BASE_SETS = TOL_SETS + [(E, E, 500), (E, E, 1500), (1e-6, 1e-6, 30), (1e-6, 1e-6, 45)]
INTEREST_SETS = TOL_SETS + [(E, E, 5000), (1e-6, 1e-6, 60), (1e-6, 1e-6, 20)]
HETERO_SETS = [(1e-8, 1e-8, M), (1e-4, 1e-4, M), (E, E, 800), (1e-8, 1e-8, 60)]
SOCIAL_SETS = [(1e-8, 1e-8, M), (1e-5, 1e-5, M), (E, E, 2000), (1e-8, 1e-8, 150)]

BASE_BETA = np.array([0.5, 1.0, 3.0, 7.3, 61.654026637430945, 250.0, 1e4])
BASE_U = sbr.julia_range("0.0", "1.5", 33)
INT_BETA = np.array([0.5, 1.0, 3.0, 61.654026637430945])
INT_U = np.linspace(0.0, 0.55, 12)
INT_RD = [(0.06, 0.1), (5.0, 50.0)]
HET_U = np.linspace(0.0, 1.0, 17)
HET_COLS = {4: np.array([[0.25, 0.5, 1.0, 2.0], [0.1, 1.0, 5.0, 25.0]]),
            8: np.array([[0.1, 0.2, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0]]),
            1: np.array([[1.0]])}
SOC_BETA = np.array([0.5, 1.0, 3.0, 8.0])
SOC_U = np.array([0.02, 0.1, 0.3, 0.6])
SOC_MAX_ITER = 40


def _id(o):
    return f"{o[0]:.0e}-{o[1]:.0e}-{o[2]}"


def dev_kw(o):
    return dict(ode_rtol=o[0], ode_atol=o[1], ode_maxiters=o[2])


def ora_kw(o):
    return dict(rtol=o[0], atol=o[1], ode_maxiters=o[2])


def assert_bitwise(a, b, name):
    a = np.asarray(a)
    b = np.asarray(b)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)
    if not same.all():
        idx = np.argwhere(~same)[:5]
        raise AssertionError(f"{name}: {int((~same).sum())} mismatches, e.g. "
                             f"{[(tuple(i), a[tuple(i)], b[tuple(i)]) for i in idx]}")


def compare(g, o, what, extra=()):
    for k in (*FIELDS, "status", "iters", *extra):
        if k in o:
            assert_bitwise(g[k], o[k], f"{what} {k}")


def count(st, v):
    return int((np.asarray(st) == v).sum())


def rows(o, idx):
    """Rows idx (repeats allowed) of every per-point array of an oracle result."""
    return {k: v[idx] for k, v in o.items() if k != "n_knots"}


# ------------------------------------------------------------------------------------ baseline
def baseline_coverage(o, opts):
    """What the option set is in the list for, measured on the oracle's result o (7 × 33)."""
    st, nk = o["status"], o["n_knots"]
    assert not (st & TRUNC).any()
    if opts[2] == M:
        # β ≥ 3 hands over to Rosenbrock23, β ≤ 1 stays on Tsit5 — at every tolerance of the list
        assert ((st[2:] & STIFF) != 0).all() and not (st[:2] & STIFF).any()
        assert not (st & MAXIT).any()
    if opts == (1e-6, 1e-6, M):
        assert nk.min() == 31 and nk.max() == 62
    if opts == (1e-3, 1e-3, M):
        assert nk.min() == 11 and nk.max() == 36
        assert (st & FALSE_EQ).any()
    if opts == (1e-6, 1e-12, M):
        # an engine that swapped rtol and atol would give the knot counts of (1e-12, 1e-6)
        assert nk.tolist() == [60, 73, 84, 88, 88, 89, 91]
    if opts == (E, E, 500):
        assert (st == (OOB | MAXIT)).all()
    if opts == (E, E, 1500):
        assert count(st, CONV | HRLOW | MAXIT) == 28  # 0x206
        assert count(st, COLLAPSE | MAXIT) == 5 and count(st, OOB | MAXIT) == 198
        # the β = 0.5 column: its solve reaches η well before step 1500 and the cap before t_end
        assert (st[0] & (RUN | CONV | HRLOW | COLLAPSE)).all() and (st[0] & MAXIT).all()
    if opts == (1e-6, 1e-6, 30):
        assert count(st, OOB | MAXIT) == 198 and not (st[0] & MAXIT).any()
    if opts == (1e-6, 1e-6, 45):
        assert count(st, RUN | CONV | MAXIT) >= 1
        for v in (COLLAPSE | MAXIT, BMAX | MAXIT, OOB | MAXIT):
            assert count(st, v) >= 1, hex(v)
        assert not (st & STIFF).any()  # cut before the hand-over the uncapped solve makes


@pytest.fixture(scope="module")
def base_ref(oracle):
    """oracle.sweep_baseline of β × BASE_U per (β tuple, option set): computed once, read-only."""
    cache = {}

    def get(opts, beta=BASE_BETA, u=BASE_U):
        key = (opts, tuple(beta), tuple(u))
        if key not in cache:
            o = oracle.sweep_baseline(np.asarray(beta), ETA, T_END, np.asarray(u), P, KAPPA, LAM, **ora_kw(opts))
            if np.array_equal(beta, BASE_BETA) and np.array_equal(u, BASE_U):
                baseline_coverage(o, opts)
            for v in o.values():
                v.setflags(write=False)
            cache[key] = o
        return cache[key]

    return get


@pytest.mark.parametrize("schedule", ["default", "exhaustive", "ready"])
@pytest.mark.parametrize("opts", BASE_SETS, ids=_id)
def test_baseline_sweep(engine, base_ref, opts, schedule):
    """The sweep learning kernel (plain sink) and the equilibrium kernel on its short, stiff or
    capped columns: 7 columns (one stream), then 196 columns (three chunks; with
    SBR_FLAG_READY_SWEEP the readiness schedule, asserted taken)."""
    o = base_ref(opts)
    kw = dict(dev_kw(opts), exhaustive=schedule == "exhaustive",
              flags=sbr._lib.SBR_FLAG_READY_SWEEP if schedule == "ready" else 0)
    g = engine.sweep_baseline(sbr.BaselineGrid(BASE_BETA, BASE_U, ETA, T_END, p=P, kappa=KAPPA, lam=LAM), **kw)
    compare(g, o, f"7 columns, {schedule}")
    idx = np.tile(np.arange(7), 28)
    g = engine.sweep_baseline(sbr.BaselineGrid(BASE_BETA[idx], BASE_U, ETA, T_END, p=P, kappa=KAPPA, lam=LAM), **kw)
    assert engine.last_schedule() == (1 if schedule == "ready" else 0)
    compare(g, rows(o, idx), f"196 columns, {schedule}")


@pytest.mark.parametrize("opts", BASE_SETS, ids=_id)
def test_baseline_single_point_grid(engine, oracle, opts):
    for beta in (1.0, 61.654026637430945):
        o = oracle.sweep_baseline([beta], ETA, T_END, [0.05], P, KAPPA, LAM, **ora_kw(opts))
        g = engine.sweep_baseline(sbr.BaselineGrid([beta], [0.05], ETA, T_END, p=P, kappa=KAPPA, lam=LAM),
                                  **dev_kw(opts))
        compare(g, o, f"1 × 1, β = {beta}")


@pytest.mark.parametrize("opts", BASE_SETS, ids=_id)
def test_solve_points_equals_sweep(engine, base_ref, opts):
    """The points kernel on the flattened grid (every point its own learning solve)."""
    o = base_ref(opts)
    nb, nu = len(BASE_BETA), len(BASE_U)
    g = engine.solve_points(np.repeat(BASE_BETA, nu), np.tile(BASE_U, nb), ETA, T_END, P, KAPPA, LAM, **dev_kw(opts))
    compare(g, {k: v.reshape(-1) for k, v in rows(o, slice(None)).items()}, "points")


def _batch(engine, torch, betas, opts, **kw):
    dev = torch.device("cuda", 0)
    nbat, nb = betas.shape
    nu = len(BASE_U)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)  # noqa: E731
    out = {f: torch.empty(nbat, nb * nu, dtype=torch.float64, device=dev) for f in FIELDS}
    out["status"] = torch.empty(nbat, nb * nu, dtype=torch.int32, device=dev)
    out["iters"] = torch.empty(nbat, nb * nu, dtype=torch.int32, device=dev)
    engine.sweep_baseline_batch_dev(t(betas), t(np.full(betas.shape, ETA)), t(np.full(betas.shape, T_END)),
                                    t(BASE_U), P, KAPPA, LAM, 1e-4, out,
                                    stream=torch.cuda.current_stream(dev).cuda_stream, **dev_kw(opts), **kw)
    torch.cuda.synchronize(dev)
    g = {f: out[f].cpu().numpy().reshape(nbat, nb, nu) for f in (*FIELDS, "iters")}
    g["status"] = out["status"].cpu().numpy().view(np.uint32).reshape(nbat, nb, nu)
    return g


BATCH_SCALE = (1.0, 0.8, 1.7)  # three grids whose β rows differ


@pytest.mark.parametrize("opts", BASE_SETS, ids=_id)
def test_baseline_batch(engine, base_ref, opts):
    """The pipelined batch: the learning kernel's fused-hazard sink (3 grids × 7 columns, direct
    stores), then its LDS ring with the 16-entry flushes and the tail flush (11 grids × 1,536
    columns = 264 learning waves, heads-first: columns of 11 to 1,501 knots, most of them fewer
    than one flush) — the 21 distinct columns of the three small grids, repeated."""
    torch = pytest.importorskip("torch")
    three = [base_ref(opts, BASE_BETA * s) for s in BATCH_SCALE]
    betas = np.stack([BASE_BETA * s for s in BATCH_SCALE])
    g = _batch(engine, torch, betas, opts)
    for k in range(3):
        compare({f: v[k] for f, v in g.items()}, three[k], f"batch grid {k}")
    # 11 × 1536 columns: column c of grid k is distinct column (5 k + c) mod 21
    allb = betas.reshape(-1)
    ref = {f: np.concatenate([o[f] for o in three]) for f in (*FIELDS, "status", "iters")}
    idx = (5 * np.arange(11)[:, None] + np.arange(1536)[None, :]) % 21
    g = _batch(engine, torch, allb[idx], opts, knot_capacity=4096)
    for k in range(11):
        compare({f: v[k] for f, v in g.items()}, rows(ref, idx[k]), f"ring batch grid {k}")


@pytest.mark.parametrize("stop", [False, True])
@pytest.mark.parametrize("maxiters", [1, 2, 50])
def test_learning_maxiters(engine, oracle, maxiters, stop):
    """A learning solve cut after 1, 2 and 50 iterations: maxiters + 1 knots, the oracle's."""
    to, Go, so = oracle.learn_logistic(1.0, T_END, maxiters=maxiters)
    assert len(to) == maxiters + 1 and so["status"] == MAXIT and to[-1] < ETA
    ((t, G, st),) = engine.learn_baseline([1.0], ETA, T_END, stop_after_eta=stop, ode_maxiters=maxiters)
    assert_bitwise(t, to, "t")
    assert_bitwise(G, Go, "G")
    assert st == MAXIT


# ------------------------------------------------------------------------------------ interest
def interest_coverage(oracle, o, opts, rd):
    st = o["status"]
    assert not (st & TRUNC).any()
    if opts == (1e-6, 1e-6, M) and rd == (5.0, 50.0):
        # the value function's own stiff branch: these two learning solves never switch
        for b in (0.5, 1.0):
            assert oracle.learn_logistic(b, T_END, rtol=1e-6, atol=1e-6)[2]["nswitch"] == 0
        assert ((st[:2] & STIFF) != 0).all()
    if opts == (E, E, 5000):
        # learning completes (≤ 2,893 steps); V stops at 5,000 steps, before the end of the HR grid
        hit = (st == (CONV | HRLOW | MAXIT)) & (o["rk_steps"] == 5000)
        assert hit.sum() >= 46 and o["rk_steps"].max() == 5000
    if opts == (1e-6, 1e-6, 60) and rd == (0.06, 0.1):
        for v in (0x3, 0x208, 0x803, 0xa03, 0xa06, 0xa10):
            assert count(st, v) >= 1, hex(v)
    if opts == (1e-6, 1e-6, 60) and rd == (5.0, 50.0):
        assert count(st, 0xa03) == 12 and count(st, 0xa06) == 36
    if opts == (1e-6, 1e-6, 20):
        assert ((st & MAXIT) != 0).all() and count(st, OOB | MAXIT) >= 36


@pytest.mark.parametrize("rd", INT_RD, ids=lambda rd: f"r{rd[0]}-d{rd[1]}")
@pytest.mark.parametrize("opts", INTEREST_SETS, ids=_id)
def test_interest_sweep(engine, oracle, opts, rd):
    """The three options govern the learning solve and the value function alike (InterestArgs)."""
    o = oracle.sweep_interest(INT_BETA, ETA, T_END, INT_U, P, KAPPA, LAM, rd[0], rd[1], **ora_kw(opts))
    interest_coverage(oracle, o, opts, rd)
    g = engine.sweep_interest(INT_BETA, ETA, T_END, INT_U, P, KAPPA, LAM, rd[0], rd[1], **dev_kw(opts))
    compare(g, o, "interest", extra=("rk_steps",))


@pytest.mark.parametrize("rd,n_v", [((0.06, 0.1), 25), ((5.0, 50.0), 7)])
def test_interest_point_paths_short_v(engine, oracle, rd, n_v):
    """n_v < n_tau: V stops at 60 steps, 25 (7) values into the 31-entry HR grid."""
    opts = (1e-6, 1e-6, 60)
    o = oracle.interest_point(1.0, ETA, T_END, 0.05, P, KAPPA, LAM, rd[0], rd[1], **ora_kw(opts))
    assert len(o["V"]) == n_v and len(o["hr_tau"]) == 31
    g = engine.interest_point_paths(1.0, ETA, T_END, 0.05, P, KAPPA, LAM, rd[0], rd[1], **dev_kw(opts))
    assert g["status"] == o["status"]
    for k in (*FIELDS, "hr_tau", "hr", "V", "aw_cum"):
        assert_bitwise(g[k], o[k], k)


# ------------------------------------------------------------------------------------ hetero
def _het(K):
    cols = HET_COLS[K]
    dist = np.full(K, 1.0 / K)
    return cols, dist, ETA / (cols @ dist)


@pytest.mark.parametrize("K", [4, 8, 1])
@pytest.mark.parametrize("opts", HETERO_SETS, ids=_id)
def test_hetero(engine, oracle, opts, K):
    cols, dist, eta = _het(K)
    o = oracle.sweep_hetero(cols, dist, eta, T_END, HET_U, P, KAPPA, LAM, **ora_kw(opts))
    st = o["status"]
    if opts[2] != M:
        assert (st == (OOB | MAXIT)).all()
    elif K == 4 and opts == (1e-4, 1e-4, M):
        assert (st & STIFF).any() and not (st & STIFF).all()
    lr = engine.learn_hetero(cols, dist, T_END, **dev_kw(opts))
    for c in range(len(cols)):
        to, Go, so = oracle.learn_hetero(cols[c], dist, T_END, **ora_kw(opts))
        n = int(lr["n_knots"][c])
        assert n == len(to) == o["n_knots"][c]
        assert_bitwise(lr["t"][c, :n], to, f"t column {c}")
        assert_bitwise(lr["G"][c, :n], Go, f"G column {c}")
        assert lr["status"][c] == so["status"]
    g = engine.sweep_hetero(cols, dist, eta, T_END, HET_U, P, KAPPA, LAM, **dev_kw(opts))
    compare(g, o, f"hetero K = {K}")


# ------------------------------------------------------------------------------------ social
@pytest.fixture(scope="module")
def social_ref(oracle):
    cache = {}
    cmp = np.stack([sbr.julia_range(0.0, ETA, 1000)] * len(SOC_BETA))

    def get(opts):
        if opts not in cache:
            o = oracle.sweep_social(SOC_BETA, ETA, SOC_U, P, KAPPA, LAM, cmp, max_iter=SOC_MAX_ITER, **ora_kw(opts))
            st = o["status"]
            if opts[2] == M:
                assert count(st, NOTCONV | STIFF | RUN | CONV) >= 1  # 0x1803: a forced iterate went stiff
            if opts == (E, E, 2000):
                assert (st == (NOTCONV | MAXIT | OOB)).all()  # 0x1280: the initial logistic solve is cut
            if opts == (1e-8, 1e-8, 150):
                assert count(st, 0x1280) >= 1 and count(st, 0x1a80) >= 1
            cache[opts] = o
        return cache[opts]

    return get


@pytest.mark.parametrize("lanes", [False, True], ids=["default-schedule", "point-per-lane"])
@pytest.mark.parametrize("opts", SOCIAL_SETS, ids=_id)
def test_social(engine, social_ref, opts, lanes):
    """The options govern the initial logistic solve and every forced iterate, under the built-in
    schedule (a wave per point) and with one point per lane."""
    o = social_ref(opts)
    if lanes:
        with engine.social_schedule(coop_max=0, waves=1):
            g = engine.sweep_social(SOC_BETA, ETA, SOC_U, P, KAPPA, LAM, max_iter=SOC_MAX_ITER, **dev_kw(opts))
            stats = engine.social_schedule_stats()
        assert stats[0] > 0 and stats[1] == 0, stats
    else:
        g = engine.sweep_social(SOC_BETA, ETA, SOC_U, P, KAPPA, LAM, max_iter=SOC_MAX_ITER, **dev_kw(opts))
    compare(g, o, "social", extra=("fp_iters",))


# ------------------------------------------------------------------------------------ knot capacity
CAP_BETA = np.array([0.5, 1.0, 3.0])
CAP_U = BASE_U[::4]


@pytest.fixture(scope="module")
def cap_ref(oracle):
    """Per column of CAP_BETA: the unconstrained oracle result, and the result on the first 1,500
    oracle knots OR-ed with SBR_KNOT_OVERFLOW (what a column that overflows a capacity of 1,500
    must give).  β = 1 has 2,308 knots ≤ η and 2,848 in all: 1,500 is below the η prefix of the
    β = 1 and β = 3 columns, 4,096 above every full count."""
    full = oracle.sweep_baseline(CAP_BETA, ETA, T_END, CAP_U, P, KAPPA, LAM)
    assert full["n_knots"].max() < 4096 and not (full["status"] & (OVER | OOB)).any()
    cut = {k: np.empty_like(v) for k, v in full.items() if k != "n_knots"}
    for b, beta in enumerate(CAP_BETA):
        t, G, _ = oracle.learn_logistic(float(beta), T_END)
        if beta >= 1.0:
            assert (t <= ETA).sum() > 1500
        for j, u in enumerate(CAP_U):
            r = oracle.equilibrium(t[:1500], G[:1500], float(beta), ETA, T_END, float(u), P, KAPPA, LAM)
            for k in FIELDS:
                cut[k][b, j] = r[k]
            cut["status"][b, j] = r["status"] | OVER
            cut["iters"][b, j] = r["iters"]
    assert (cut["status"][1:] == (OOB | OVER)).all()
    return full, cut


def _cap_expected(g, full, cut):
    """Row by row: the overflow expectation where the device reports an overflow, the untouched
    result otherwise.  β = 1 and β = 3 must overflow; whether β = 0.5 (2,309 knots in all, 1,055
    of them ≤ η) does depends on where the engine stops its learning, which is not pinned here."""
    over = (g["status"] & OVER) != 0
    assert over[1:].all()
    assert over[0].all() or not over[0].any()
    return {k: np.where(over, cut[k], full[k]) for k in cut}


@pytest.mark.parametrize("entry", ["sweep", "points", "interest"])
def test_knot_capacity(engine, oracle, cap_ref, entry):
    full, cut = cap_ref
    nb, nu = len(CAP_BETA), len(CAP_U)

    def run(cap):
        if entry == "sweep":
            return engine.sweep_baseline(sbr.BaselineGrid(CAP_BETA, CAP_U, ETA, T_END, p=P, kappa=KAPPA, lam=LAM),
                                         knot_capacity=cap)
        if entry == "points":
            g = engine.solve_points(np.repeat(CAP_BETA, nu), np.tile(CAP_U, nb), ETA, T_END, P, KAPPA, LAM,
                                    knot_capacity=cap)
            return {k: v.reshape(nb, nu) for k, v in g.items()}
        # r = 0 is the baseline through the interest kernel
        return engine.sweep_interest(CAP_BETA, ETA, T_END, CAP_U, P, KAPPA, LAM, 0.0, 0.1, knot_capacity=cap)

    g = run(1500)
    compare(g, _cap_expected(g, full, cut), f"{entry}, capacity 1500")
    compare(run(4096), {k: v for k, v in full.items() if k != "n_knots"}, f"{entry}, capacity 4096")


def test_knot_capacity_interest_value_function(engine, oracle, cap_ref):
    """r > 0: an overflowing column's hazard is the BoundsError before any value function runs (no
    knot at η), so its points are the baseline's SBR_OOB | SBR_KNOT_OVERFLOW with no RK steps; a
    column within the capacity is the unconstrained interest result."""
    _, cut = cap_ref
    o = oracle.sweep_interest(CAP_BETA, ETA, T_END, CAP_U, P, KAPPA, LAM, 0.06, 0.1)
    g = engine.sweep_interest(CAP_BETA, ETA, T_END, CAP_U, P, KAPPA, LAM, 0.06, 0.1, knot_capacity=1500)
    over = (g["status"] & OVER) != 0
    assert over[1:].all() and (over[0].all() or not over[0].any())
    exp = {k: np.where(over, cut[k], o[k]) for k in cut}
    exp["rk_steps"] = np.where(over, 0, o["rk_steps"])
    compare(g, exp, "interest r > 0, capacity 1500", extra=("rk_steps",))
    compare(engine.sweep_interest(CAP_BETA, ETA, T_END, CAP_U, P, KAPPA, LAM, 0.06, 0.1, knot_capacity=4096), o,
            "interest r > 0, capacity 4096", extra=("rk_steps",))


def test_knot_capacity_hetero(engine, oracle):
    """The K = 4 column (0.1, 1, 5, 25): 6,175 knots, 2,210 of them ≤ η, at a capacity of 2,000."""
    cols, dist, eta = _het(4)
    c, cap = 1, 2000
    t, G, so = oracle.learn_hetero(cols[c], dist, T_END)
    assert (t <= eta[c]).sum() > cap
    assert so["t_switch"] > t[cap]  # the hand-over to Rosenbrock23 comes after the last knot that fits
    o = oracle.hetero_equilibrium_knots(t[:cap], G[:cap], cols[c], dist, eta[c], T_END, HET_U, P, KAPPA, LAM)
    lr = engine.learn_hetero(cols[c:], dist, T_END, cap=cap)
    assert lr["n_knots"][0] == cap and lr["status"][0] == OVER
    assert_bitwise(lr["t"][0, :cap], t[:cap], "t")
    assert_bitwise(lr["G"][0, :cap], G[:cap], "G")
    g = engine.sweep_hetero(cols[c:], dist, eta[c:], T_END, HET_U, P, KAPPA, LAM, knot_capacity=cap)
    for k in ("xi", "aw_max", "tol", "iters", "tau_in_unc", "tau_out_unc"):
        assert_bitwise(g[k][0], o[k], k)
    assert_bitwise(g["status"][0], o["status"] | OVER, "status")
    # and a capacity above the full count changes nothing
    full = oracle.sweep_hetero(cols, dist, eta, T_END, HET_U, P, KAPPA, LAM)
    assert full["n_knots"].max() < 8192
    compare(engine.sweep_hetero(cols, dist, eta, T_END, HET_U, P, KAPPA, LAM, knot_capacity=8192), full, "hetero 8192")
