"""Caller knots on which is_valid_equilibrium_hetero (heterogeneity_solver.jl:175-210) says no, the
variants that move the deciding knot pair through the kernels' 64-knot blocks, and a plain numpy
restatement of solve_equilibrium_hetero's classes on such knots (not a test module).

The invalid class was not reached through the learning ODE, so the knots are
uncoupled logistic group CDFs on a uniform grid, G_k(t) = (1 − 1e-4)/(1 + e^{−s_k(t − m_k)}), two
parameter sets found by a random search.  ``expected`` takes the per-group buffers from the result
under test and decides everything after them itself, by np.interp: the class, ξ as the root of the
nondecreasing AW(ξ), the validity path on the knots ≤ ξ and its above → not-above pairs.  A point is
usable only where no path value lies within 1e-9 of κ, so that rounding cannot decide a knot.

tests/test_hetero_invalid.py holds the oracle to it, tests/test_gpu_hetero_invalid.py the kernels."""
import math

import numpy as np

from continuum_cases import INFO_BITS, STATUS_OF

T = 10.0
MARGIN = 1e-9
INVALID = STATUS_OF["invalid"][0]
U_GRID = np.exp(np.linspace(math.log(0.01), math.log(5.0), 32))

SEED_A = dict(
    n=700, m=[0.6784224301410351, 3.3834709123098916, 7.201780306295425],
    s=[1.486158102416506, 13.140645685547506, 7.922532709450296],
    betas=[8.456549964437537, 16.623688477703734, 5.015002142898275],
    dist=[0.19588918288422294, 0.6332450259771615, 0.17086579113861555],
    eta=8.050939180450424, p=0.2762388689088321, lam=0.03563931171494257, kappa=0.6515173888809076,
    u_invalid=[float(U_GRID[3]), float(U_GRID[4]), float(U_GRID[5])], pair=(419, 420), m_knots=494)
SEED_B = dict(
    n=300, m=[1.1826415814763251, 6.935236643478714], s=[2.531171348058492, 13.495355004931959],
    betas=[8.624950839895362, 18.6454823851753], dist=[0.33824024231058997, 0.6617597576894101],
    eta=9.414057921965675, p=0.2855564026420253, lam=0.4714528334287237, kappa=0.3042533150311858,
    u_invalid=[0.11085686234929189], pair=(193, 194), m_knots=203)
assert abs(SEED_A["u_invalid"][0] - 0.01824696527569518) < 1e-15


def seed_case(seed: dict, name: str) -> dict:
    t = np.linspace(0.0, T, seed["n"])
    G = (1.0 - 1e-4) / (1.0 + np.exp(-np.array(seed["s"])[None, :] * (t[:, None] - np.array(seed["m"])[None, :])))
    return dict(name=name, t=t, G=np.ascontiguousarray(G), betas=np.array(seed["betas"]), dist=np.array(seed["dist"]),
                eta=seed["eta"], t_end=T, p=seed["p"], lam=seed["lam"], kappa=seed["kappa"],
                u=np.array(seed["u_invalid"][:1]))


def solve(solver, c: dict, **kw) -> dict:
    """``solver``: oracle.hetero_equilibrium_knots or a wrapper of the engine's call with its signature."""
    return solver(c["t"], c["G"], c["betas"], c["dist"], c["eta"], c["t_end"], c["u"], c["p"], c["kappa"], c["lam"], **kw)


# ------------------------------------------------------------------------------------------------
# the numpy restatement
def expected(c: dict, tin, tout) -> dict:
    """One point's class after its buffers: cls, xi, m (knots ≤ ξ), pairs (indices i of above →
    not-above pairs (i, i + 1)), path, above and usable."""
    t, G, dist, kappa = c["t"], c["G"], c["dist"], c["kappa"]
    K = len(dist)
    tin, tout = np.asarray(tin, float), np.asarray(tout, float)
    assert np.isfinite(tin).all() and np.isfinite(tout).all()
    out = dict(cls="below", xi=math.nan, m=0, pairs=np.zeros(0, int), usable=True)
    if (tin == tout).all():  # solve_equilibrium_hetero :266
        return out

    def Gk(k, x):
        assert np.all(x <= t[-1])  # np.interp clamps where the reference's interpolant throws
        return np.interp(x, t, G[:, k])

    def AW(x, shift=0.0):  # compute_ξ_hetero :87-97
        return sum(dist[k] * (Gk(k, min(tout[k], x) + shift) - Gk(k, min(tin[k], x) + shift)) for k in range(K))

    out["cls"] = "norun"
    cap = AW(2.0 * tout.max())
    if abs(cap - kappa) < MARGIN:
        out["usable"] = False
    if cap < kappa:
        return out
    lo, hi = 0.0, 2.0 * tout.max()  # AW is nondecreasing, AW(lo) < κ ≤ AW(hi): plain bisection to the last bit
    while True:
        mid = 0.5 * (lo + hi)
        if not lo < mid < hi:
            break
        lo, hi = (lo, mid) if AW(mid) >= kappa else (mid, hi)
    xi = hi
    out["xi"] = xi
    j = int(np.searchsorted(t, xi, side="right")) - 1  # searchsortedlast, 0-based
    eps = t[min(j + 1, len(t) - 1)] - t[j]
    rise = AW(xi, eps) - AW(xi)
    if abs(rise) < MARGIN:
        out["usable"] = False
    if rise < 0.0:  # :101, :123
        out["cls"] = "false"
        return out
    # is_valid_equilibrium_hetero :175-210
    if np.abs(t - xi).min() < MARGIN:
        out["usable"] = False
    g = t[t <= xi]
    path = np.zeros(len(g))
    for k in range(K):
        tI = max(0.0, xi - tin[k])
        path += dist[k] * (Gk(k, g) - Gk(k, np.maximum(0.0, g - tI)))
    above = path > kappa
    pairs = np.flatnonzero(above[:-1] & ~above[1:])
    if np.abs(path - kappa).min() < MARGIN:
        out["usable"] = False
    out.update(cls="invalid" if len(pairs) else "run", m=len(g), pairs=pairs, path=path, above=above)
    return out


def expected_all(c: dict, res: dict) -> list:
    return [expected(c, res["tau_in_unc"][j], res["tau_out_unc"][j]) for j in range(len(c["u"]))]


def check_against_numpy(c: dict, res: dict, what: str = "") -> list:
    """Status, sentinels and, on a run, ξ of a result against the numpy restatement; the classes."""
    exp = expected_all(c, res)
    for j, e in enumerate(exp):
        w = (what, c["name"], j, e["cls"])
        assert e["usable"], w
        st = int(res["status"][j]) & ~INFO_BITS
        assert st in STATUS_OF[e["cls"]], (w, hex(st))
        assert np.isfinite(res["tau_in_unc"][j]).all() and np.isfinite(res["tau_out_unc"][j]).all(), w
        if e["cls"] == "run":
            assert abs(res["xi"][j] - e["xi"]) <= 1e-9 and np.isfinite(res["aw_max"][j]) and res["tol"][j] <= 1e-12, w
        else:
            assert np.isnan(res["xi"][j]) and np.isnan(res["aw_max"][j]), w
            assert res["tol"][j] == (0.0 if e["cls"] == "below" else np.inf), w
    return [e["cls"] for e in exp]


# ------------------------------------------------------------------------------------------------
# knot surgery: every inserted knot lies on the chord of its segment, so the interpolant the
# reference evaluates is unchanged (up to rounding) and only knot indices move
def insert_midpoints(c: dict, segments, per_segment=1, name=None) -> dict:
    """A copy of c with ``per_segment`` equally spaced chord knots inside each segment (i, i + 1), i
    in ``segments``."""
    t, G = c["t"], c["G"]
    seg = set(int(i) for i in segments)
    tn, Gn = [], []
    for i in range(len(t)):
        tn.append(t[i])
        Gn.append(G[i])
        if i in seg:
            for r in range(1, per_segment + 1):
                f = r / (per_segment + 1.0)
                tn.append(t[i] + f * (t[i + 1] - t[i]))
                Gn.append(G[i] + f * (G[i + 1] - G[i]))
    out = dict(c, t=np.array(tn), G=np.ascontiguousarray(np.array(Gn)))
    assert np.all(np.diff(out["t"]) > 0)
    if name:
        out["name"] = name
    return out


def drop_knots(c: dict, idx, name=None) -> dict:
    keep = np.ones(len(c["t"]), bool)
    keep[list(idx)] = False
    out = dict(c, t=c["t"][keep], G=np.ascontiguousarray(c["G"][keep]))
    if name:
        out["name"] = name
    return out


def split_groups(c: dict, copies, name) -> dict:
    """Group k becomes copies[k] groups with its rate and its G column, its share split unevenly."""
    cols, betas, dist = [], [], []
    for k, r in enumerate(copies):
        w = np.arange(1.0, r + 1.0)
        w /= w.sum()
        for q in range(r):
            cols.append(c["G"][:, k])
            betas.append(c["betas"][k])
            dist.append(c["dist"][k] * w[q])
    return dict(c, name=name, G=np.ascontiguousarray(np.stack(cols, axis=1)), betas=np.array(betas), dist=np.array(dist))


def block_kinds(c: dict, e: dict, tin) -> list:
    """The kernels' verdict per 64-knot block of the knots ≤ ξ, restated (csrc/sbr_hetero.hip, validity
    check; G nondecreasing): "N" where the upper bound Σ dist_k (G_k[i1] − G_k[hl_k]) + 1e-14 ≤ κ (every
    knot not above κ), "A" where the lower bound Σ dist_k (G_k[i0] − G_k[min(hh_k + 1, n − 1)]) − 1e-14 > κ
    (every knot above), else "E" (evaluated knot by knot); hl_k, hh_k are the brackets of
    max(0, t[i0] − τ_I,k) and max(0, t[i1] − τ_I,k)."""
    t, G, dist, n = c["t"], c["G"], c["dist"], len(c["t"])
    tI = np.maximum(0.0, e["xi"] - np.asarray(tin, float))
    kinds = []
    for i0 in range(0, e["m"], 64):
        i1 = min(i0 + 64, e["m"]) - 1
        lb = ub = 0.0
        for k in range(len(dist)):
            hl = max(int(np.searchsorted(t, max(0.0, t[i0] - tI[k]), side="right")) - 1, 0)
            hh = max(int(np.searchsorted(t, max(0.0, t[i1] - tI[k]), side="right")) - 1, 0)
            lb += dist[k] * (G[i0, k] - G[min(hh + 1, n - 1), k])
            ub += dist[k] * (G[i1, k] - G[hl, k])
        kinds.append("N" if ub + 1e-14 <= c["kappa"] else "A" if lb - 1e-14 > c["kappa"] else "E")
    return kinds


def decided_by_bounds(O, base: dict, back: int, per_segment: int, segments: int, before: str, name: str) -> dict:
    """A case whose verdict the block bounds alone give: the last above knot is the last knot of a block
    of kind ``before`` ("A", or "E" ending above: either leaves `prev` set) and the next block is "N",
    so no knot of the pair's second half is evaluated.  The seeds' dips are shallow (0.0089 and 0.0053
    below κ) and begin at depth 0, where no bound can decide; so the knots from ``back`` before the pair
    up to one before the dip's deepest knot are removed, which puts the pair's second knot deep in the
    dip, and the segments after it get ``per_segment`` chord knots each, which makes a block's rise of
    Σ dist_k G_k smaller than the dip's depth."""
    i, e = the_pair(O, base)
    deepest = i + int(np.argmin(e["path"][i:]))
    c = drop_knots(base, range(i - back + 1, deepest - 1))
    c = insert_midpoints(c, range(i - back + 1, i - back + 1 + segments), per_segment=per_segment)
    c = at_block_position(O, c, 63, name)
    res = solve(O, c)
    i2, e2 = the_pair(O, c)
    kinds = block_kinds(c, e2, res["tau_in_unc"][0])
    b = i2 // 64
    assert i2 % 64 == 63 and kinds[b] == before and kinds[b + 1] == "N" and e2["above"][i2], (name, i2, kinds)
    assert not e2["above"][64 * (b + 1):64 * (b + 2)].any() and 64 * (b + 2) <= e2["m"], name
    return c


def the_pair(O, c: dict, j=0):
    """(i, e): the single above → not-above pair (i, i + 1) of point j, which must be invalid and usable."""
    res = solve(O, c)
    e = expected(c, res["tau_in_unc"][j], res["tau_out_unc"][j])
    assert e["cls"] == "invalid" and e["usable"] and len(e["pairs"]) == 1, (c["name"], e["cls"], e["usable"], e["pairs"])
    assert int(res["status"][j]) & ~INFO_BITS == INVALID, (c["name"], hex(int(res["status"][j])))
    return int(e["pairs"][0]), e


def at_block_position(O, c: dict, pos: int, name: str) -> dict:
    """c with knots inserted in its first segments so that the pair (i, i + 1) has i mod 64 == pos."""
    i, _ = the_pair(O, c)
    out = insert_midpoints(c, range((pos - i) % 64), name=name)
    i2, _ = the_pair(O, out)
    assert i2 % 64 == pos and i2 == i + (pos - i) % 64, (name, i, i2)
    return out


def build(O) -> list:
    """Every variant, each re-verified by ``expected`` on the oracle's buffers and asserted to have the
    property it is named for.  O is oracle.hetero_equilibrium_knots."""
    A, B = seed_case(SEED_A, "A"), seed_case(SEED_B, "B")
    for c, s in ((A, SEED_A), (B, SEED_B)):
        i, e = the_pair(O, c)
        assert (i, i + 1) == s["pair"] and e["m"] == s["m_knots"], (c["name"], i, e["m"])
    cases = [A, B]
    # block positions: the pair inside a block, across a boundary, starting a block
    for pos in (62, 63, 0, 1):
        cases.append(at_block_position(O, A, pos, f"A pair at {pos} mod 64"))
        cases.append(at_block_position(O, B, pos, f"B pair at {pos} mod 64"))
    # whole blocks of not-above knots after the pair (the grid ×4 up to ξ), the pair inside a block: the
    # pair's own block is evaluated, the blocks after it are never reached
    i, e = the_pair(O, A)
    c = at_block_position(O, insert_midpoints(A, range(i + 1, e["m"] - 1), per_segment=3), 20,
                          "A x4 after the pair, pair at 20 mod 64")
    i2, e2 = the_pair(O, c)
    first = 64 * (i2 // 64 + 1)
    assert first + 64 <= e2["m"] and not e2["above"][first:first + 64].any(), c["name"]
    cases.append(c)
    # bounds only: a block that the upper bound puts not above κ, directly after a block that ends above κ
    # (`ub <= kappa` with `prev` set): after an "every knot above" block and after an evaluated one
    cases.append(decided_by_bounds(O, A, 0, 127, 2, "E", "A bounds decide after an evaluated block"))
    cases.append(decided_by_bounds(O, A, 3, 127, 2, "A", "A bounds decide after an above block"))
    cases.append(decided_by_bounds(O, B, 0, 127, 1, "E", "B bounds decide after an evaluated block"))
    cases.append(decided_by_bounds(O, B, 3, 127, 1, "A", "B bounds decide after an above block"))
    # the pair in the last, partial block before ξ: B has it there; A after thinning the knots up to ξ
    i, e = the_pair(O, B)
    assert i >= 64 * ((e["m"] - 1) // 64) and e["m"] % 64 != 0
    i, e = the_pair(O, A)
    thin = drop_knots(A, [q for q in range(i + 2, e["m"] - 1) if (q - i) % 3 != 0])
    c = at_block_position(O, thin, 5, "A thinned, pair in the last partial block")
    i2, e2 = the_pair(O, c)
    assert i2 >= 64 * ((e2["m"] - 1) // 64) and e2["m"] % 64 != 0, (i2, e2["m"])
    cases.append(c)
    # a dip that does not cross: κ scaled down until the path's minimum after its hump clears κ by 1e-6
    for c0 in (A, B):
        for f in (0.97, 0.95, 0.93, 0.9, 0.85, 0.8):
            c = dict(c0, kappa=c0["kappa"] * f, name=f"{c0['name']} dip above kappa*{f}")
            res = solve(O, c)
            e = expected(c, res["tau_in_unc"][0], res["tau_out_unc"][0])
            if e["cls"] != "run" or not e["usable"]:
                continue
            first = int(np.argmax(e["above"]))
            d = np.diff(e["path"][first:])
            if e["above"].any() and (d < 0).any() and e["path"][first:].min() > c["kappa"] + 1e-6:
                cases.append(c)
                break
        else:
            raise AssertionError(f"no dip without a crossing on seed {c0['name']}")
    # more groups: equal-rate copies with split shares (K = 5, 9, 16 run the group-looped kernel)
    for copies in ((1, 3, 1), (5, 3, 1), (5, 6, 5)):
        c = split_groups(A, copies, f"A split into K={sum(copies)}")
        the_pair(O, c)
        cases.append(c)
        cases.append(at_block_position(O, c, 63, f"A split into K={sum(copies)}, pair at 63 mod 64"))
    # a non-monotone tail beyond ξ: G alternates between 1 − 2⁻⁵³ and 1 on the last 40 knots
    c = dict(A, name="A non-monotone tail", G=A["G"].copy())
    c["G"][-40:, :] = np.where(np.arange(40)[:, None] % 2 == 0, 1.0 - 2.0 ** -53, 1.0)
    i, e = the_pair(O, c)
    assert c["t"][-40] > e["xi"] and (np.diff(c["G"], axis=0) < 0).any()
    cases.append(c)
    # residency and mixed classes: invalid, run and below points in one launch
    ub = SEED_B["u_invalid"][0]
    for c0, u in ((A, U_GRID[[2, 3, 4, 5, 7, 11, 15, 31]]),
                  (B, np.array([U_GRID[4], U_GRID[5], U_GRID[10], 0.9 * ub, ub, 1.25 * ub, U_GRID[14], U_GRID[17]]))):
        c = dict(c0, u=np.ascontiguousarray(u), name=f"{c0['name']} mixed u")
        cls = check_against_numpy(c, solve(O, c), "build")
        assert {"invalid", "run", "norun", "below"} <= set(cls) and cls.count("invalid") == 3, (c["name"], cls)
        cases.append(c)
    # one NaN beyond every lookup of the points that end before AW_max: the per-knot path
    base = dict(A, u=np.array(SEED_A["u_invalid"] + [60.0]), name="A three invalid, one below")
    c = dict(base, name="A with a NaN in the last knot", G=A["G"].copy())
    c["G"][-1, 2] = np.nan
    r0, r1 = solve(O, base), solve(O, c)
    cls = check_against_numpy(base, r0, "build")
    assert cls == ["invalid"] * 3 + ["below"], cls
    for k in ("xi", "aw_max", "tol", "status", "iters", "tau_in_unc", "tau_out_unc"):
        assert np.array_equal(r0[k], r1[k], equal_nan=True), k
    c["no_numpy"] = True  # np.interp would read the NaN; the equal oracle result above stands for it
    cases += [base, c]
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        assert 200 <= len(c["t"]) <= 3000 and len(c["u"]) <= 8
        if not c.get("no_numpy"):
            check_against_numpy(c, solve(O, c), "build")
    return cases
