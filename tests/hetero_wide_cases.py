"""Grids of the K = 1 … 16 heterogeneity tests (tests/test_hetero_wide_oracle.py, no GPU, and
tests/test_gpu_hetero_wide.py) with their oracle results: each computed once per session,
shared between the two files and read-only."""
import functools

import numpy as np

import oracle as O
import sbr

# group counts without a specialised kernel: below 8, odd, above 8, and the limit
WIDE_K = (5, 7, 9, 12, 16)
# oracle run points of hetero_config4(6, 24, K) (of 144)
CONFIG4_RUNS = {5: 142, 7: 140, 9: 139, 12: 139, 16: 139}
FIELDS = ("xi", "aw_max", "tol", "tau_in_unc", "tau_out_unc", "status", "iters")


def _freeze(d: dict) -> dict:
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def oracle_sweep(g) -> dict:
    return _freeze(O.sweep_hetero(g.betas, g.dist, g.eta, g.t_end, g.u, g.p, g.kappa, g.lam, g.x0))


@functools.lru_cache(maxsize=None)
def config4(n_s: int, n_u: int, K: int):
    """(grid, oracle sweep) of sbr.hetero_config4(n_s, n_u, K)."""
    g = sbr.hetero_config4(n_s, n_u, K)
    return g, oracle_sweep(g)


@functools.lru_cache(maxsize=None)
def script():
    g = sbr.hetero_script_grid()
    return g, oracle_sweep(g)


@functools.lru_cache(maxsize=None)
def unequal_k10():
    """K = 10 with unequal shares and unsorted rates; t_end = 2η of the s = 1 column, so the
    bisection of some points probes past the last knot (the interpolant's BoundsError)."""
    rng = np.random.default_rng(0)
    base = 0.125 * 100.0 ** (rng.permutation(10) / 9)
    d = rng.random(10) + 0.2
    d /= d.sum()
    d[-1] = 1.0 - d[:-1].sum()
    s = np.array([1.0, 3.0, 20.0])
    t_end = 60.0 / float(np.sum(d * base))
    g = sbr.HeteroGrid(s[:, None] * base, d, sbr.julia_range("0.001", "1", 24), eta_bar=30.0, t_end=t_end, p=0.9,
                       kappa=0.3, lam=0.1, name="hetero_K10_unequal")
    return g, oracle_sweep(g)


@functools.lru_cache(maxsize=None)
def learned(n_s: int, n_u: int, K: int, col: int):
    """(t, G, info) of the oracle's solve_SInetwork_hetero on one config-4 column."""
    g = sbr.hetero_config4(n_s, n_u, K)
    t, G, info = O.learn_hetero(g.betas[col], g.dist, g.t_end[col])
    t.setflags(write=False)
    G.setflags(write=False)
    return t, G, info


def same(a, b) -> np.ndarray:
    a, b = np.asarray(a), np.asarray(b)
    return (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)


def assert_bitwise(got: dict, ref: dict, name: str, fields=FIELDS) -> None:
    for f in fields:
        assert got[f].shape == ref[f].shape, (name, f, got[f].shape, ref[f].shape)
        ok = same(got[f], ref[f])
        assert ok.all(), (name, f, int((~ok).sum()))
