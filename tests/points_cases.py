"""The seeded list of models the sbr_solve_points tests share (not a test module).

L70: N = 70 points — more than one wave of learning lanes, the second wave partial — with
every parameter drawn per point, and seven fixed points: 0-2 the Fig 3 main / bis / ter
equilibria, 3 an η past t_end (the hazard's BoundsError), 64-66 one β in one wave with three
different (p, κ, λ)."""
import numpy as np

ARGS = ("beta", "eta", "t_end", "u", "p", "kappa", "lam")
FIELDS = ("xi", "tau_in_unc", "tau_out_unc", "aw_max", "tol")
ALL = (*FIELDS, "status", "iters")
X0 = 1e-4


def seeded(n: int, seed: int) -> dict:
    """n points from the L70 distributions (the order of the draws is part of the list)."""
    rng = np.random.default_rng(seed)
    beta = 10.0 ** rng.uniform(-1, 4, n)
    carry = rng.random(n) < 0.5
    eta = np.where(carry, 15.0, 15.0 / beta)
    t_end = np.where(carry, 30.0, 2 * eta)
    u = rng.uniform(0.001, 1.0, n)
    p = rng.uniform(0.05, 0.99, n)
    kappa = rng.uniform(0.05, 0.95, n)
    lam = 10.0 ** rng.uniform(-3, 0, n)
    return dict(beta=beta, eta=eta, t_end=t_end, u=u, p=p, kappa=kappa, lam=lam)


def l70() -> dict:
    pts = seeded(70, 0)
    # (β, η, t_end, u, p, κ, λ): 0-2 = Fig 3 main / bis / ter, 3 = η past t_end
    fixed = {0: (1, 15, 30, .1, .5, .6, .01), 1: (3, 15, 30, .1, .5, .6, .01), 2: (1, 15, 30, .01, .5, .6, .01),
             3: (1, 15, 10, .1, .5, .6, .01),
             64: (1, 15, 30, .1, .5, .6, .01), 65: (1, 15, 30, .1, .9, .6, .01), 66: (1, 15, 30, .1, .5, .3, .2)}
    for i, vals in fixed.items():
        for k, v in zip(ARGS, vals):
            pts[k][i] = v
    return pts


def oracle_points(O, pts: dict) -> dict:
    """Point i = oracle.sweep_baseline([β_i], η_i, t_end_i, [u_i], p_i, κ_i, λ_i): (n,) arrays."""
    n = len(pts["beta"])
    rows = [O.sweep_baseline([pts["beta"][i]], pts["eta"][i], pts["t_end"][i], [pts["u"][i]], float(pts["p"][i]),
                             float(pts["kappa"][i]), float(pts["lam"][i]), X0) for i in range(n)]
    return {k: np.array([r[k].reshape(-1)[0] for r in rows]) for k in (*ALL, "n_knots")}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)


def assert_same(a, b, name):
    bad = ~same(a, b)
    assert not bad.any(), f"{name}: {int(bad.sum())} mismatches at {np.flatnonzero(bad)[:8]}"
