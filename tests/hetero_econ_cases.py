"""The grids the sbr_sweep_hetero_econ tests share (not a test module).

H3(K): the three columns of sbr.hetero_config4(3, 12, K) (2.8k–5.3k knots at K = 2, 5.1k–7.9k at
K = 5, 8 and 16, all past the stiff switch) times 12 u × 2 p × 2 λ × 3 κ = 432 points.  The reference value of the product is one oracle
sweep_hetero per (p, λ, κ), stacked into sbr_sweep_hetero_econ's layout
(n_col, n_p, n_lam, n_kappa, n_u) with the group buffers (…, K)."""
import functools

import numpy as np

import oracle as O
import sbr

FIELDS = ("xi", "aw_max", "tol", "tau_in_unc", "tau_out_unc", "status", "iters")
U12 = np.array([0, .01, .05, .1, .2, .3, .4, .55, .7, .85, 1.0, 1.5])
P2 = np.array([.5, .9])
LAM2 = np.array([.01, .1])
KAPPA3 = np.array([.15, .3, .6])

# oracle status counts of H3(K), measured on the CPU oracle
H3_COUNTS = {2: {0x803: 328, 0x806: 6, 0x808: 23, 0x810: 59, 0x880: 16},
             8: {0x803: 326, 0x806: 30, 0x808: 6, 0x810: 62, 0x880: 8},
             5: {0x803: 340, 0x806: 30, 0x808: 53, 0x810: 9},
             16: {0x803: 332, 0x806: 30, 0x808: 64, 0x810: 6}}


def grid(n_s: int, n_u: int, K: int, u=None, p=P2, lam=LAM2, kappa=KAPPA3) -> dict:
    """The columns of hetero_config4(n_s, n_u, K) with the given axes (u: the grid's own if None)."""
    g = sbr.hetero_config4(n_s, n_u, K)
    return dict(betas=g.betas, dist=g.dist, eta=g.eta, t_end=g.t_end, u=g.u if u is None else np.asarray(u, float),
                p=p, lam=lam, kappa=kappa, x0=g.x0)


def h3(K: int) -> dict:
    return grid(3, 12, K, u=U12)


def shape_of(g: dict) -> tuple:
    return (len(g["betas"]),) + tuple(np.atleast_1d(g[k]).size for k in ("p", "lam", "kappa", "u"))


def oracle_hetero_econ(Or, g: dict, **kw) -> dict:
    """[c, a, b, k, :] = row c of oracle.sweep_hetero(βs, dist, η, t_end, u, p[a], κ[k], λ[b]); the group
    buffers [c, a, b, k, :, :]; n_knots per column and, for the property the design rests on,
    n_knots_all[a, b, k, c]."""
    nc, n_p, nl, nk, nu = shape_of(g)
    K = np.atleast_2d(g["betas"]).shape[1]
    out = {}
    for f in FIELDS:
        dt = np.uint32 if f == "status" else (np.int32 if f == "iters" else float)
        out[f] = np.empty((nc, n_p, nl, nk, nu) + ((K,) if f.startswith("tau_") else ()), dt)
    out["n_knots_all"] = np.empty((n_p, nl, nk, nc), np.int64)
    for a, pa in enumerate(np.atleast_1d(g["p"])):
        for b, lb in enumerate(np.atleast_1d(g["lam"])):
            for k, kk in enumerate(np.atleast_1d(g["kappa"])):
                r = Or.sweep_hetero(g["betas"], g["dist"], g["eta"], g["t_end"], g["u"], float(pa), float(kk),
                                    float(lb), g["x0"], **kw)
                out["n_knots"] = r["n_knots"]
                out["n_knots_all"][a, b, k] = r["n_knots"]
                for f in FIELDS:
                    out[f][:, a, b, k] = r[f]
    return out


def freeze(d: dict) -> dict:
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def h3_oracle(K: int):
    """(grid, oracle stack) of H3(K), computed once per session and read-only."""
    g = h3(K)
    return g, freeze(oracle_hetero_econ(O, g))


def counts(status) -> dict:
    v, n = np.unique(np.asarray(status), return_counts=True)
    return {int(a): int(b) for a, b in zip(v, n)}


def same(a, b) -> np.ndarray:
    a, b = np.asarray(a), np.asarray(b)
    return (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)


def assert_bitwise(got: dict, ref: dict, name: str, fields=FIELDS, where=None) -> None:
    """All seven fields equal bit for bit (NaN = NaN); `where`: a mask over the five point axes."""
    for f in fields:
        a, b = np.asarray(got[f]), np.asarray(ref[f])
        assert a.shape == b.shape, (name, f, a.shape, b.shape)
        if where is not None:
            a, b = a[where], b[where]
        ok = same(a, b)
        assert ok.all(), (name, f, int((~ok).sum()))
