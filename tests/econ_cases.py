"""The grids the sbr_sweep_econ tests share (not a test module).

E6: six columns — a slow, the Fig 3 main and bis, a fast β, a column whose η lies past its t_end
(the hazard's BoundsError) and a β whose 28k knots do not fit the LDS slab — times 4 p × 3 λ × 4 κ ×
12 u = 3,456 points.  The reference value of the product is one oracle β × u sweep per (p, λ, κ),
stacked into sbr_sweep_econ's layout (n_beta, n_p, n_lam, n_kappa, n_u)."""
import numpy as np

FIELDS = ("xi", "tau_in_unc", "tau_out_unc", "aw_max", "tol")
ALL = (*FIELDS, "status", "iters")
X0 = 1e-4

E6 = dict(beta=np.array([0.3, 1.0, 3.0, 40.0, 1.0, 1456.1990328251586]),
          eta=np.full(6, 15.0),
          t_end=np.array([30.0, 30.0, 30.0, 30.0, 10.0, 30.0]),
          u=np.array([0, .01, .05, .1, .2, .3, .4, .55, .7, .85, 1.0, 1.5]),
          p=np.array([.05, .5, .9, 1.0]),
          lam=np.array([.001, .01, .2]),
          kappa=np.array([.05, .3, .6, .95]))


def shape_of(g: dict) -> tuple:
    return tuple(np.atleast_1d(g[k]).size for k in ("beta", "p", "lam", "kappa", "u"))


def oracle_econ(O, g: dict, early_exit: int = 0, **kw) -> dict:
    """[i, a, b, c, :] = row i of oracle.sweep_baseline(β, η, t_end, u, p[a], κ[c], λ[b]) (with
    oracle.apply_early_exit per (a, b, c) when early_exit > 0); n_knots per column."""
    nb, n_p, nl, nk, nu = shape_of(g)
    out = {k: np.empty((nb, n_p, nl, nk, nu), np.uint32 if k == "status" else (np.int32 if k == "iters" else float))
           for k in ALL}
    for a, pa in enumerate(np.atleast_1d(g["p"])):
        for b, lb in enumerate(np.atleast_1d(g["lam"])):
            for c, kc in enumerate(np.atleast_1d(g["kappa"])):
                r = O.sweep_baseline(g["beta"], g["eta"], g["t_end"], g["u"], float(pa), float(kc), float(lb), X0,
                                     **kw)
                out["n_knots"] = r["n_knots"]
                if early_exit > 0:
                    r = O.apply_early_exit(r, early_exit)
                for k in ALL:
                    out[k][:, a, b, c, :] = r[k]
    return out


def freeze(d: dict) -> dict:
    for v in d.values():
        v.setflags(write=False)
    return d


def counts(status) -> dict:
    v, n = np.unique(np.asarray(status), return_counts=True)
    return {int(a): int(b) for a, b in zip(v, n)}
