"""The grids the sbr_sweep_interest_econ tests share (not a test module).

I4: four columns — the Fig 3 main, a fast β, a column whose η lies past its t_end (the hazard's
BoundsError) and a β whose 28k knots do not fit the LDS slab — times 2 p × 2 λ × 3 rate pairs × 3 κ ×
6 u = 864 points, 192 of them value functions at r > 0.  The reference value of the product is one
oracle interest sweep per (p, λ, rate, κ), stacked into sbr_sweep_interest_econ's layout
(n_beta, n_p, n_lam, n_rate, n_kappa, n_u); rk_steps has no κ axis, and the oracle's must agree
across κ before it is stacked."""
import numpy as np

from econ_cases import ALL, FIELDS, X0, counts, freeze  # noqa: F401

WITH_STEPS = (*ALL, "rk_steps")

I4 = dict(beta=np.array([1.0, 3.0, 1.0, 1456.1990328251586]),
          eta=np.full(4, 15.0),
          t_end=np.array([30.0, 30.0, 10.0, 30.0]),
          u=np.array([0, .02, .05, .1, .3, .6]),
          p=np.array([.5, .9]),
          lam=np.array([.01, .2]),
          r=np.array([0, .06, .02]),
          delta=np.array([.1, .1, .5]),
          kappa=np.array([.3, .6, .9]))

_DTYPES = {"status": np.uint32, "iters": np.int32}


def shape_of(g: dict) -> tuple:
    return tuple(np.atleast_1d(g[k]).size for k in ("beta", "p", "lam", "r", "kappa", "u"))


def oracle_interest_econ(O, g: dict, **kw) -> dict:
    """[i, a, b, d, c, :] = row i of oracle.sweep_interest(β, η, t_end, u, p[a], κ[c], λ[b], r[d], δ[d]);
    rk_steps [i, a, b, d, :], asserted equal for every κ."""
    nb, n_p, nl, nr, nk, nu = shape_of(g)
    out = {k: np.empty((nb, n_p, nl, nr, nk, nu), _DTYPES.get(k, float)) for k in ALL}
    out["rk_steps"] = np.empty((nb, n_p, nl, nr, nu), np.int64)
    rates = list(zip(np.atleast_1d(g["r"]), np.atleast_1d(g["delta"])))
    for a, pa in enumerate(np.atleast_1d(g["p"])):
        for b, lb in enumerate(np.atleast_1d(g["lam"])):
            for d, (rd, dd) in enumerate(rates):
                for c, kc in enumerate(np.atleast_1d(g["kappa"])):
                    r = O.sweep_interest(g["beta"], g["eta"], g["t_end"], g["u"], float(pa), float(kc), float(lb),
                                         float(rd), float(dd), X0, **kw)
                    for k in ALL:
                        out[k][:, a, b, d, c, :] = r[k]
                    if c == 0:
                        out["rk_steps"][:, a, b, d, :] = r["rk_steps"]
                    else:  # one value function serves every κ
                        assert np.array_equal(out["rk_steps"][:, a, b, d, :], r["rk_steps"]), (a, b, d, c)
    return out
