"""Seeded draws across the parameter space for every kernel family (not a test module).

The other cases of the suite sit near the paper's values (x0 = 1e-4, p = 0.5, κ = 0.6, λ = 0.01, η = 15,
t_end = 30, an ascending u axis).  Here every family is drawn from numpy.random.default_rng(SEEDS[family]):
    β = 10^U(−2, 3.5), t_end = 10^U(0, 2), η = t_end with probability ½ else t_end·U(0.02, 1),
    x0 = 10^U(−12, −0.05), p, κ ~ U(0.02, 0.98), λ = 10^U(−4, −0.3),
    u = 10^U(−4, 3.5), not sorted, with exact duplicates and one u = 0,
    interest: r = 0 or 10^U(−3, 0) and δ = 10^U(−2, 0.3), redrawn until r < δ (interest_rate_model.jl:48-50),
    heterogeneity: K uniform in 1..16, group rates β·10^U(−1, 1) unsorted, shares from a Dirichlet draw,
    social: β = 10^U(−1, 2), η = 10^U(0.3, 1.6), cmp = range(0, η, 1000), tol = 1e-4, max_iter = 6.
A *call* is one invocation of a sweep entry point.  The C ABI fixes what a call can vary: β, η and t_end
are per column, u is per lane, and x0, p, κ, λ (and r, δ) are scalars of the call (axes in the econ
families, per point in sbr_solve_points).  A family is therefore a list of calls, each with its own
scalars; the points family draws all seven parameters per point.

Two choices follow from x0 and κ being scalars of a call.  (1) The u range reaches 10^3.5, the top of the
β range.  A column's outcome changes with u from runs over failed bisections to "hazard below u"; under
a u range that ends at 3.2 the columns with β above ~10 never reach the last class, and with one κ per
call only a fifth to under a half of the full waves hold three classes.  (2) x0 is stratified: the 33-u
call of a sweep family and the small second plane of an econ family draw x0 above ½, and the baseline
family has sixteen four-column calls with x0 in the top decade 10^U(−1, −0.05).  A plain x0 draw lands
above ½ once in fifty calls, and false equilibria need a CDF that starts high: without the stratum they
hold under 2 % of the baseline points.

Shapes are the smallest at which the paths exist: 65 u (a full wave and a one-lane wave, BLOCK = 256),
one call with 33 u (BLOCK = 64), 70 columns (two learning waves, the second partial), 193 = 64·3 + 1
columns (run_baseline's chunked schedule), and 5 u × 13 κ planes (65 points: the full wave of a plane
holds all 13 κ).

Invalid lanes: the device-pointer entry points cannot read their axes on the host, so a lane whose own
u (κ, p, λ in the econ families) breaks its rule ends with the sentinel include/sbr.h documents —
SBR_ARG_INVALID, NaN, tol = Inf, 0 iterations — and its neighbours are untouched.  The oracle does not
validate (u = −0.1 comes back RUN | CONVERGED), so each call carries ``u`` (valid everywhere; what the
oracle and the host-pointer entry points get) and ``u_bad`` (at most 5 % of the lanes replaced by u < 0
or NaN; what the *_dev entry points get), and ``expected_dev`` overlays the sentinel on the oracle's
result.  An econ plane has no 5 % of an axis: there the device call runs once clean and once more with
bad axis elements (``spoil_axes``).  The social grid carries no invalid lane: sbr_sweep_social_dev
neither documents nor implements a per-lane sentinel, so an invalid u has no defined answer there.

Every family's ``premise`` is a function of the oracle's result alone; tests/test_random_cases.py
asserts it on the CPU, tests/test_gpu_random.py holds the kernels to the oracle bit for bit.  No point
is excluded from any comparison (EXCLUDED is empty)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

RUN, CONVERGED, BELOW, COLLAPSE, MAXITER, FALSE_EQ, OOB = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x80
ARG_INVALID, NOT_CONVERGED = 0x400, 0x1000
CLASSES = ("RUN", "BELOW", "COLLAPSE", "MAXITER", "FALSE_EQ", "OOB", "OTHER")

# a family whose premise fails (numpy's stream changed, a range was edited) gets another seed here; the
# thresholds of ``premise`` stay
SEEDS = dict(baseline=4, points=1, econ=2, interest=1, interest_econ=2, hetero=3, hetero_econ=1, social=1)
FIELDS = ("xi", "tau_in_unc", "tau_out_unc", "aw_max", "tol")
ALL = (*FIELDS, "status", "iters")
HFIELDS = ("xi", "aw_max", "tol", "tau_in_unc", "tau_out_unc", "status", "iters")
SOCIAL_TOL, SOCIAL_MAX_ITER = 1e-4, 6
U_LOG10 = (-4.0, 3.5)
EXCLUDED = {}  # family -> [(call, column, lane, reason)]: points left out of the comparison.  None.


# ------------------------------------------------------------------------------------------------
# the distributions
def draw_columns(rng, n: int):
    beta = 10.0 ** rng.uniform(-2.0, 3.5, n)
    t_end = 10.0 ** rng.uniform(0.0, 2.0, n)
    eta = np.where(rng.random(n) < 0.5, t_end, t_end * rng.uniform(0.02, 1.0, n))
    return beta, eta, t_end


def draw_x0(rng, high=False) -> float:
    """high: False — the whole range; True — above ½; "decade" — the top decade 10^U(−1, −0.05)."""
    lo = {False: -12.0, True: float(np.log10(0.5)), "decade": -1.0}[high]
    return float(10.0 ** rng.uniform(lo, -0.05))


def draw_econ(rng, n=None):
    """p, κ, λ (scalars, or n of each)."""
    p, kappa = rng.uniform(0.02, 0.98, n), rng.uniform(0.02, 0.98, n)
    lam = 10.0 ** rng.uniform(-4.0, -0.3, n)
    return (float(p), float(kappa), float(lam)) if n is None else (p, kappa, lam)


def draw_u(rng, n: int) -> np.ndarray:
    """n unsorted u with max(1, n // 20) exact duplicates and one u = 0."""
    u = 10.0 ** rng.uniform(U_LOG10[0], U_LOG10[1], n)
    k = max(1, n // 20)
    pick = rng.choice(n, 2 * k + 1, replace=False)
    u[pick[k:2 * k]] = u[pick[:k]]
    u[pick[2 * k]] = 0.0
    return u


def spoil_u(rng, u: np.ndarray):
    """u with max(1, 5 % of the lanes) replaced by u < 0 or NaN, and those lanes."""
    n = len(u)
    bad = np.sort(rng.choice(n, max(1, (5 * n) // 100), replace=False))
    ub = u.copy()
    for k, j in enumerate(bad):
        ub[j] = np.nan if k % 2 else -(10.0 ** rng.uniform(*U_LOG10))
    return ub, bad


def draw_rate(rng, zero: bool):
    """(r, δ) with 0 <= r < δ."""
    while True:
        r = 0.0 if zero else float(10.0 ** rng.uniform(-3.0, 0.0))
        delta = float(10.0 ** rng.uniform(-2.0, 0.3))
        if r < delta:
            return r, delta


def _sweep_call(rng, family, name, ncol, nu, high=False, **kw) -> dict:
    beta, eta, t_end = draw_columns(rng, ncol)
    p, kappa, lam = draw_econ(rng)
    u = draw_u(rng, nu)
    u_bad, bad = spoil_u(rng, u)
    return dict(family=family, seed=SEEDS[family], name=name, beta=beta, eta=eta, t_end=t_end, x0=draw_x0(rng, high),
                p=p, kappa=kappa, lam=lam, u=u, u_bad=u_bad, bad=bad, **kw)


# ------------------------------------------------------------------------------------------------
# the families
def baseline() -> list:
    """70 × 65, 6 × 33 (x0 above ½), 193 × 65, eight two-column calls for more (x0, p, κ, λ) and sixteen
    four-column calls with x0 in the top decade."""
    rng = np.random.default_rng(SEEDS["baseline"])
    # 193 = 64·kSweepChunks + 1 columns (csrc/sbr_capi_baseline.hip: kSweepChunks = sbr_ctx::kLearnStreams = 3),
    # the fewest that run_baseline cuts into chunks; tests/test_gpu_random.py asserts that it did
    shapes = [("waves70", 70, 65, False), ("block64", 6, 33, True), ("chunked193", 193, 65, False)]
    shapes += [(f"pair{k}", 2, 65, False) for k in range(8)] + [(f"high{k}", 4, 65, "decade") for k in range(16)]
    return [_sweep_call(rng, "baseline", *s) for s in shapes]


def interest() -> list:
    """70 × 65 at r > 0, 6 × 33 at r = 0 (x0 above ½), and twelve two-column calls, every third at r = 0."""
    rng = np.random.default_rng(SEEDS["interest"])
    shapes = [("waves70", 70, 65, False, False), ("block64", 6, 33, True, True)]
    shapes += [(f"pair{k}", 2, 65, False, k % 3 == 2) for k in range(12)]
    out = []
    for name, ncol, nu, high, zero in shapes:
        c = _sweep_call(rng, "interest", name, ncol, nu, high)
        c["r"], c["delta"] = draw_rate(rng, zero)
        out.append(c)
    return out


def points() -> dict:
    """130 points, all seven parameters per point; ``bad``: six lanes with one invalid parameter each."""
    rng = np.random.default_rng(SEEDS["points"])
    n = 130
    beta, eta, t_end = draw_columns(rng, n)
    p, kappa, lam = draw_econ(rng, n)
    u = draw_u(rng, n)
    c = dict(family="points", seed=SEEDS["points"], name="list130", x0=draw_x0(rng),
             args=dict(beta=beta, eta=eta, t_end=t_end, u=u, p=p, kappa=kappa, lam=lam))
    lanes = np.sort(rng.choice(n, 6, replace=False))
    spoil = [("u", -0.1), ("u", float("nan")), ("kappa", 1.0), ("kappa", 0.0), ("p", 1.5), ("lam", 0.0)]
    c["args_bad"] = {k: v.copy() for k, v in c["args"].items()}
    for j, (k, v) in zip(lanes, spoil):
        c["args_bad"][k][j] = v
    c["bad"] = lanes
    return c


def _econ_axes(rng, c: dict):
    p, _, lam = draw_econ(rng, 2)
    c.update(p=p, lam=lam, kappa=rng.uniform(0.02, 0.98, 13))


# the planes of an econ family: 8 columns at a plain x0, and 2 columns whose CDF starts above ½
ECON_PLANES = (("plane65", 8, False), ("plane65_high", 2, True))


def econ() -> list:
    """8 and 2 (x0 above ½) columns × 2 p × 2 λ × 13 κ × 5 u."""
    rng = np.random.default_rng(SEEDS["econ"])
    out = []
    for name, ncol, high in ECON_PLANES:
        c = _sweep_call(rng, "econ", name, ncol, 5, high)
        _econ_axes(rng, c)
        out.append(c)
    return out


def interest_econ() -> list:
    """8 and 2 (x0 above ½) columns × 2 p × 2 λ × 2 rate pairs (r = 0 and r > 0) × 13 κ × 5 u."""
    rng = np.random.default_rng(SEEDS["interest_econ"])
    out = []
    for name, ncol, high in ECON_PLANES:
        c = _sweep_call(rng, "interest_econ", name, ncol, 5, high)
        _econ_axes(rng, c)
        pairs = [draw_rate(rng, True), draw_rate(rng, False)]
        c["r"], c["delta"] = np.array([q[0] for q in pairs]), np.array([q[1] for q in pairs])
        out.append(c)
    return out


def _groups(rng, c: dict, K: int):
    c["K"] = K
    c["betas"] = c["beta"][:, None] * 10.0 ** rng.uniform(-1.0, 1.0, (len(c["beta"]), K))
    d = rng.dirichlet(np.ones(K))
    d[-1] = 1.0 - d[:-1].sum()
    c["dist"] = d


def hetero() -> list:
    """16 columns × 65 u, K drawn per column: one call per K value that was drawn."""
    rng = np.random.default_rng(SEEDS["hetero"])
    Ks = rng.integers(1, 17, 16)
    out = []
    for K in sorted(set(int(k) for k in Ks)):
        c = _sweep_call(rng, "hetero", f"K{K}", int((Ks == K).sum()), 65)
        _groups(rng, c, K)
        out.append(c)
    return out


def hetero_econ() -> list:
    """Two calls of 4 columns × 2 p × 2 λ × 13 κ × 5 u: a K with a specialised kernel, and one without; and
    one of 2 columns, any K, whose group CDFs start above ½ (x0 above ½)."""
    rng = np.random.default_rng(SEEDS["hetero_econ"])
    wide = (5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16)
    out = []
    for tag, pool, ncol, high in (("", (2, 3, 4, 8), 4, False), ("", wide, 4, False), ("_high", tuple(range(1, 17)), 2, True)):
        K = int(rng.choice(pool))
        c = _sweep_call(rng, "hetero_econ", f"plane65_K{K}{tag}", ncol, 5, high)
        _econ_axes(rng, c)
        _groups(rng, c, K)
        out.append(c)
    return out


def social() -> dict:
    """8 β × 9 u."""
    from sbr import julia_range

    rng = np.random.default_rng(SEEDS["social"])
    beta = 10.0 ** rng.uniform(-1.0, 2.0, 8)
    eta = 10.0 ** rng.uniform(0.3, 1.6, 8)
    p, kappa, lam = draw_econ(rng)
    return dict(family="social", seed=SEEDS["social"], name="grid8x9", beta=beta, eta=eta, t_end=eta, x0=draw_x0(rng),
                p=p, kappa=kappa, lam=lam, u=draw_u(rng, 9), cmp=np.stack([julia_range(0.0, float(e), 1000) for e in eta]),
                tol=SOCIAL_TOL, max_iter=SOCIAL_MAX_ITER)


def spoil_axes(c: dict) -> list:
    """Two spoiled copies of an econ-family call for the *_dev entry points, with the mask of the points
    that end as SBR_ARG_INVALID (over the call's point axes): one bad κ and one bad u; one bad p and one
    bad λ (three of the four hazard classes)."""
    rate = ("r",) if "r" in c and np.ndim(c["r"]) else ()
    axes = ("p", "lam", *rate, "kappa", "u")
    shape = (len(c["beta"]),) + tuple(len(c[k]) for k in axes)
    out = []
    for spoil in ({"kappa": (4, 1.0), "u": (2, float("nan"))}, {"p": (1, -0.25), "lam": (0, 0.0)}):
        q = dict(c, **{k: np.array(c[k], float) for k in spoil})
        mask = np.zeros(shape, bool)
        for k, (i, v) in spoil.items():
            q[k][i] = v
            idx = [slice(None)] * len(shape)
            idx[1 + axes.index(k)] = i
            mask[tuple(idx)] = True
        out.append((q, mask))
    return out


# ------------------------------------------------------------------------------------------------
# the oracle's answers
def _stack(rows: list, shape: tuple, tail: dict = None) -> dict:
    """rows = [(index into the axes between column and u, oracle sweep result)] stacked into the econ
    layouts (column, …, u)."""
    out = {}
    for idx, r in rows:
        for k, v in r.items():
            if k == "n_knots":
                out[k] = v
                continue
            extra = v.shape[2:]
            if k not in out:
                out[k] = np.empty(shape + extra, v.dtype)
            out[k][(slice(None), *idx)] = v
    return out


def oracle_call(O, c: dict) -> dict:
    """The oracle's result of a call on its valid u, in the layout of the call's entry point."""
    f = c["family"]
    col = (c.get("beta"), c.get("eta"), c.get("t_end"))
    if f == "baseline":
        return O.sweep_baseline(*col, c["u"], c["p"], c["kappa"], c["lam"], c["x0"])
    if f == "interest":
        return O.sweep_interest(*col, c["u"], c["p"], c["kappa"], c["lam"], c["r"], c["delta"], c["x0"])
    if f == "hetero":
        return O.sweep_hetero(c["betas"], c["dist"], c["eta"], c["t_end"], c["u"], c["p"], c["kappa"], c["lam"], c["x0"])
    if f == "social":
        return O.sweep_social(c["beta"], c["eta"], c["u"], c["p"], c["kappa"], c["lam"], c["cmp"], c["x0"], tol=c["tol"],
                              max_iter=c["max_iter"])
    if f == "points":
        return oracle_points(O, c["args"], c["x0"])
    # the econ layouts: one oracle sweep per (p, λ[, rate], κ).  The sweeps are independent and the oracle
    # threads over columns only, so they run side by side, each on one thread
    nb, nu = len(c["beta"]), len(c["u"])
    P, L, Kp = c["p"], c["lam"], c["kappa"]
    rates = list(zip(c["r"], c["delta"])) if f == "interest_econ" else [None]
    todo = [(a, b, d, k) for a in range(len(P)) for b in range(len(L)) for d in range(len(rates)) for k in range(len(Kp))]

    def one(i):
        a, b, d, k = i
        pl = (float(P[a]), float(Kp[k]), float(L[b]))
        if f == "econ":
            return O.sweep_baseline(*col, c["u"], *pl, c["x0"], nthreads=1)
        if f == "hetero_econ":
            return O.sweep_hetero(c["betas"], c["dist"], c["eta"], c["t_end"], c["u"], *pl, c["x0"], nthreads=1)
        return O.sweep_interest(*col, c["u"], *pl, float(rates[d][0]), float(rates[d][1]), c["x0"], nthreads=1)

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        res = list(pool.map(one, todo))
    if f != "interest_econ":
        return _stack([((a, b, k), r) for (a, b, _, k), r in zip(todo, res)], (nb, len(P), len(L), len(Kp), nu))
    steps = np.empty((nb, len(P), len(L), len(rates), nu), np.int64)
    for (a, b, d, k), r in zip(todo, res):
        rk = r.pop("rk_steps")
        if k == 0:
            steps[:, a, b, d] = rk
        else:  # one value function serves every κ
            assert np.array_equal(steps[:, a, b, d], rk), (a, b, d, k)
    out = _stack(list(zip(todo, res)), (nb, len(P), len(L), len(rates), len(Kp), nu))
    out["rk_steps"] = steps
    return out


def oracle_points(O, a: dict, x0: float) -> dict:
    n = len(a["beta"])
    rows = [O.sweep_baseline([a["beta"][i]], a["eta"][i], a["t_end"][i], [a["u"][i]], float(a["p"][i]),
                             float(a["kappa"][i]), float(a["lam"][i]), x0) for i in range(n)]
    return {k: np.array([r[k].reshape(-1)[0] for r in rows]) for k in (*ALL, "n_knots")}


def expected_dev(ref: dict, mask, rk_mask=None) -> dict:
    """``ref`` with the SBR_ARG_INVALID sentinel on the points of ``mask`` (over the point axes).
    ``rk_mask``: sbr_sweep_interest_econ's rk_steps has no κ axis and is 0 only where u, p, λ or the rate
    pair is at fault — the mask over its own axes."""
    out = {k: np.array(v) for k, v in ref.items() if k != "n_knots"}
    for k, v in out.items():
        m = rk_mask if (k == "rk_steps" and rk_mask is not None) else mask
        if k == "status":
            v[m] = ARG_INVALID
        elif k in ("iters", "fp_iters", "rk_steps"):
            v[m] = 0
        elif k == "tol":
            v[m] = np.inf
        else:
            v[m] = np.nan
    return out


def lane_mask(c: dict, shape: tuple) -> np.ndarray:
    """The lanes ``bad`` of a sweep call (every column) or of the points list."""
    m = np.zeros(shape, bool)
    m[..., c["bad"]] = True
    return m


# ------------------------------------------------------------------------------------------------
# what a draw contains
def class_of(status) -> np.ndarray:
    """Index into CLASSES per point."""
    st = np.asarray(status, np.uint32)
    out = np.full(st.shape, CLASSES.index("OTHER"))
    for name, bit in (("MAXITER", MAXITER), ("COLLAPSE", COLLAPSE), ("BELOW", BELOW), ("RUN", RUN), ("FALSE_EQ", FALSE_EQ),
                      ("OOB", OOB)):
        out[(st & bit) != 0] = CLASSES.index(name)
    return out


def class_counts(statuses) -> dict:
    cl = np.concatenate([class_of(s).reshape(-1) for s in statuses])
    return {name: int((cl == i).sum()) for i, name in enumerate(CLASSES)}


def column_stats(O, calls) -> dict:
    """Of the logistic columns of ``calls``: how many have fewer than 16 knots, end below ½, start above ½,
    have more than 2,500 knots; and the knot-count range."""
    n, lo, hi = [], [], []
    for c in calls:
        for b, te in zip(c["beta"], c["t_end"]):
            t, G, _ = O.learn_logistic(float(b), float(te), c["x0"])
            n.append(len(t))
            lo.append(G[0])
            hi.append(G[-1])
    n, lo, hi = np.array(n), np.array(lo), np.array(hi)
    return dict(columns=len(n), few=int((n < 16).sum()), ends_low=int((hi < 0.5).sum()), starts_high=int((lo > 0.5).sum()),
                many=int((n > 2500).sum()), n_min=int(n.min()), n_max=int(n.max()))


def wave_mixing(c: dict, status) -> tuple:
    """(full waves, full waves with at least three outcome classes) of a sweep call: a column's lanes are
    dealt to waves 64 at a time in the order laid out."""
    cl = class_of(status).reshape(len(c["beta"]), -1)
    full = mixed = 0
    for row in cl:
        for w in range(len(row) // 64):
            full += 1
            mixed += len(set(row[64 * w:64 * w + 64].tolist())) >= 3
    return full, mixed


def share_premise(counts: dict, names, share=0.02) -> list:
    """The classes of ``names`` that hold less than ``share`` of the points (empty: the premise holds)."""
    total = sum(counts.values())
    return [k for k in names if counts[k] < share * total]


# ------------------------------------------------------------------------------------------------
# the failure report
def describe(c: dict, idx: tuple) -> str:
    """Every parameter of the point ``idx`` of call ``c`` at full precision: enough to rebuild it."""
    f = c["family"]
    head = f"family {f}, seed {c['seed']}, call {c['name']}, x0 = {c['x0']!r}"
    if f == "points":
        return head + f", point {idx[0]}: " + ", ".join(f"{k} = {float(v[idx[0]])!r}" for k, v in c["_args"].items())
    col, lane = idx[0], idx[-1]
    par = [f"column {col}, lane {lane}", f"u = {float(c['_u'][lane])!r}", f"eta = {float(c['eta'][col])!r}",
           f"t_end = {float(c['t_end'][col])!r}"]
    if "betas" in c:
        par += [f"K = {c['K']}", f"betas = {c['betas'][col].tolist()!r}", f"dist = {c['dist'].tolist()!r}"]
    else:
        par.append(f"beta = {float(c['beta'][col])!r}")
    axes = [k for k in ("p", "lam", "r", "kappa") if k in c and np.ndim(c[k])]
    for k in ("p", "lam", "r", "delta", "kappa", "tol", "max_iter"):
        if k not in c:
            continue
        if np.ndim(c[k]):
            i = idx[1 + axes.index("r" if k == "delta" else k)]
            par.append(f"{k}[{i}] = {float(c[k][i])!r}")
        else:
            par.append(f"{k} = {c[k]!r}")
    return head + ", " + ", ".join(par)


def assert_equal(got: dict, ref: dict, c: dict, what: str, fields, u=None, args=None) -> None:
    """Every field of ``fields`` equal bit for bit (NaN = NaN); the first mismatch is reported in full."""
    c = dict(c, _u=c.get("u") if u is None else u, _args=c.get("args") if args is None else args)
    for k in fields:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape, (c["family"], c["name"], what, k, a.shape, b.shape)
        same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)
        if same.all():
            continue
        idx = tuple(int(i) for i in np.argwhere(~same)[0])
        pt = idx[:len(idx) - 1] if k.startswith("tau_") and "betas" in c else idx  # group buffers: (…, K)
        if k == "rk_steps" and c["family"] == "interest_econ":  # no κ axis
            pt = (*idx[:-1], 0, idx[-1])
        fmt = (lambda v: hex(int(v))) if k == "status" else (lambda v: repr(v.item()))
        raise AssertionError(f"{what}: {k}{list(idx)} = {fmt(a[idx])}, expected {fmt(b[idx])} ({int((~same).sum())} "
                             f"mismatches in {k}); " + describe(c, pt))


# ------------------------------------------------------------------------------------------------
# a family's calls with the oracle's answers, computed once per session and read-only
FAMILIES = ("baseline", "points", "econ", "interest", "interest_econ", "hetero", "hetero_econ", "social")
_cache = {}


def calls_of(family: str) -> list:
    c = globals()[family]()
    return c if isinstance(c, list) else [c]


def reference(O, family: str) -> tuple:
    """(calls, oracle results) of a family."""
    if family not in _cache:
        calls = calls_of(family)
        refs = [oracle_call(O, c) for c in calls]
        for r in refs:
            for v in r.values():
                v.setflags(write=False)
        _cache[family] = (calls, refs)
    return _cache[family]


def premise(O, family: str) -> tuple:
    """(facts, failures) of a family's draw, from the oracle's results alone: the class counts and what
    else the family is drawn for; ``failures`` names every condition the draw misses (empty: it holds).
      - each of RUN, HR below u, COLLAPSE, MAXITER and OOB holds at least 2 % of the points; baseline and
        heterogeneity also FALSE_EQ; social, whose inner bisection rarely fails, RUN, HR below u and OOB;
      - baseline / interest columns: at least 4 with fewer than 16 knots, 4 whose CDF ends below ½, 2 that
        start above ½, 8 with more than 2,500 knots; the ten columns of an econ family cannot hold 18 such
        columns: there at least 2 that start above ½ and one of each other kind (hetero-econ, whose group
        CDFs are no logistic columns: at least 2 columns whose groups start above ½);
      - baseline: at least half of the full waves hold three outcome classes or more;
      - interest: at least a third of the columns at r > 0, a point above 10,000 value-function steps;
      - social: at least 10 points converge before max_iter and at least 10 do not."""
    calls, refs = reference(O, family)
    facts = dict(points=int(sum(r["status"].size for r in refs)), classes=class_counts([r["status"] for r in refs]))
    fails = []
    need = [k for k in CLASSES[:6] if k != "FALSE_EQ" or family in ("baseline", "hetero")]
    if family == "social":
        need = ["RUN", "BELOW", "OOB"]
    fails += [f"class {k} below 2 %" for k in share_premise(facts["classes"], need)]
    if family in ("baseline", "interest", "econ", "interest_econ"):
        s = facts["columns"] = column_stats(O, calls)
        small = family.endswith("econ")
        for k, n in (("few", 1 if small else 4), ("ends_low", 1 if small else 4), ("starts_high", 2),
                     ("many", 1 if small else 8)):
            if s[k] < n:
                fails.append(f"columns: {k} = {s[k]} < {n}")
    if family == "baseline":
        fm = [wave_mixing(c, r["status"]) for c, r in zip(calls, refs)]
        facts["waves"] = (sum(f for f, _ in fm), sum(m for _, m in fm))
        if 2 * facts["waves"][1] < facts["waves"][0]:
            fails.append(f"wave mixing {facts['waves']}")
    if family == "hetero_econ":
        facts["starts_high"] = sum(len(c["beta"]) for c in calls if c["x0"] > 0.5)
        if facts["starts_high"] < 2:
            fails.append(f"{facts['starts_high']} columns start above ½")
    if family in ("interest", "interest_econ"):
        pos = sum(len(c["beta"]) for c in calls if np.any(np.asarray(c["r"]) > 0))
        facts["r_positive_columns"] = pos
        facts["max_steps"] = max(int(r["rk_steps"].max()) for r in refs)
        if 3 * pos < facts.get("columns", {}).get("columns", 0):
            fails.append(f"{pos} columns at r > 0")
        if facts["max_steps"] <= 10000:
            fails.append(f"longest value function {facts['max_steps']} steps")
    if family == "social":
        st, fp = refs[0]["status"], refs[0]["fp_iters"]
        conv = ((st & NOT_CONVERGED) == 0) & (fp < calls[0]["max_iter"])
        facts["converged_early"], facts["not_converged"] = int(conv.sum()), int(((st & NOT_CONVERGED) != 0).sum())
        if facts["converged_early"] < 10 or facts["not_converged"] < 10:
            fails.append(f"social: {facts['converged_early']} converge early, {facts['not_converged']} do not")
    if family == "points":
        facts["n_knots"] = (int(refs[0]["n_knots"].min()), int(refs[0]["n_knots"].max()))
    assert not EXCLUDED.get(family), "exclusions are capped at 1 % and must be named"
    return facts, fails
