"""Heterogeneity models with any number of groups 1 <= K <= 16 (SBR_HETERO_MAX_K) on the GPU: the
group-looped equilibrium kernel (sbr_hetero_wide.hip) and the learning / hazard / per-group-curve
kernels at every K, bit for bit against the CPU oracle on xi, aw_max, tol, the per-group buffers,
status and iters.  tests/test_hetero_wide_oracle.py asserts what the grids contain."""
import ctypes

import numpy as np
import pytest

import sbr
from hetero_wide_cases import FIELDS, WIDE_K, assert_bitwise, config4, learned, same, script, unequal_k10
from sbr import _lib

pytestmark = pytest.mark.gpu

S = sbr.STATUS


def sweep(engine, g, **kw):
    return engine.sweep_hetero(g.betas, g.dist, g.eta, g.t_end, g.u, g.p, g.kappa, g.lam, g.x0, **kw)


@pytest.mark.parametrize("K", WIDE_K)
def test_config4_equals_oracle(engine, K):
    """Learning (Rosenbrock23 with a K×K LU in every column), hazards and equilibria of a K-group
    grid with drawdown columns, the iteration cap (K = 7) and the collapse exit (the others)."""
    g, o = config4(6, 24, K)
    assert_bitwise(sweep(engine, g), o, g.name)


def test_unequal_shares_unsorted_rates_bounds_error(engine):
    g, o = unequal_k10()
    assert_bitwise(sweep(engine, g), o, g.name)


@pytest.mark.parametrize("case", ["script", (8, 20, 2), (10, 30, 4), (24, 48, 8)], ids=str)
def test_wide_kernel_equals_specialised(engine, case):
    """SBR_FLAG_HETERO_WIDE at the K that have a specialised equilibrium kernel: the same results
    from both kernels, equal to the oracle; at K = 8 also with SBR_FLAG_EXHAUSTIVE (linear crossing
    scans instead of the HR block summaries)."""
    g, o = script() if case == "script" else config4(*case)
    w = sweep(engine, g, wide=True)
    assert_bitwise(w, o, f"{g.name} wide vs oracle")
    assert_bitwise(w, sweep(engine, g), f"{g.name} wide vs specialised")
    if g.K == 8:
        assert_bitwise(sweep(engine, g, wide=True, exhaustive=True), o, f"{g.name} wide exhaustive")


@pytest.mark.parametrize("shape", [(2, 300, 12), (9, 5, 6)], ids=str)
def test_tiles_and_tails(engine, shape):
    """300 u at K = 12: three 128-lane workgroups per column, the last partly filled; 9 columns of
    5 u at K = 6: the column count no multiple of the XCD interleave of 8, fewer u than a wave."""
    g, o = config4(*shape)
    assert_bitwise(sweep(engine, g), o, g.name)


def refined(t, G):
    """The knots with their midpoints (2n − 1 knots) and the group CDFs interpolated there."""
    tm = np.empty(2 * len(t) - 1)
    tm[0::2], tm[1::2] = t, 0.5 * (t[:-1] + t[1:])
    Gm = np.empty((len(tm), G.shape[1]))
    Gm[0::2], Gm[1::2] = G, 0.5 * (G[:-1] + G[1:])
    return tm, Gm


def check_knots(a, o, name, paths):
    assert_bitwise(a, o, name)
    if paths:
        assert a["n_tau"] == o["n_hr"], name
        assert same(a["hr"], o["hr"]).all(), (name, "hr")
        if o["status"][0] & S["SBR_RUN"]:
            assert same(a["aw_total"], o["aw_total"]).all(), (name, "aw_total")


def test_slab_overflow_runs_from_global_memory(engine, oracle):
    """A K = 12 column on caller knots refined past the LDS slab: the global-memory launch."""
    g = sbr.hetero_config4(2, 4, 12)
    t, G, _ = learned(2, 4, 12, 1)
    tm, Gm = refined(t, G)
    slab = min(3 * engine.device_info()["lds_knot_capacity"], 10176)  # het_lds() of sbr_ctx.h
    assert len(t) <= slab < len(tm)
    args = (g.betas[1], g.dist, g.eta[1], g.t_end[1])
    u = np.array([0.02, 0.05, 0.3, 0.9])
    a = engine.hetero_equilibrium_on_knots(tm, Gm, *args, u, g.p, g.kappa, g.lam, paths=False)
    o = oracle.hetero_equilibrium_knots(tm, Gm, *args, u, g.p, g.kappa, g.lam)
    assert ((o["status"] & S["SBR_RUN"]) > 0).any()
    check_knots(a, o, "refined K=12", paths=False)
    a = engine.hetero_equilibrium_on_knots(tm, Gm, *args, 0.05, g.p, g.kappa, g.lam)
    o = oracle.hetero_equilibrium_knots(tm, Gm, *args, 0.05, g.p, g.kappa, g.lam)
    check_knots(a, o, "refined K=12 paths", paths=True)


def test_k16_learning_bitwise(engine):
    g = sbr.hetero_config4(2, 4, 16)
    t, G, info = learned(2, 4, 16, 1)
    a = engine.learn_hetero(np.atleast_2d(g.betas[1]), g.dist, g.t_end[1])
    n = int(a["n_knots"][0])
    assert n == len(t) == 5907
    assert np.array_equal(a["t"][0, :n], t) and np.array_equal(a["G"][0, :n], G)
    assert int(a["status"][0]) & ~S["SBR_STIFF_SWITCH"] == info["status"] & ~S["SBR_STIFF_SWITCH"]


def test_k16_point_paths_and_knots(engine, oracle):
    """sbr_hetero_point_paths and sbr_hetero_equilibrium_on_knots at K = 16: AW_total, the
    2 × 16 per-group curves and the 16 hazard rows."""
    g = sbr.hetero_config4(2, 4, 16)
    args = (g.betas[1], g.dist, g.eta[1], g.t_end[1])
    a = engine.hetero_point_paths(*args, 0.05, g.p, g.kappa, g.lam)
    b = oracle.hetero_point_paths(*args, 0.05, g.p, g.kappa, g.lam)
    assert b["status"] == S["SBR_RUN"] | S["SBR_CONVERGED"] | S["SBR_STIFF_SWITCH"]
    assert a["status"] == b["status"]
    for k in ("xi", "aw_max", "tol", "tau_in_unc", "tau_out_unc", "t", "G", "aw_total", "aw_out", "aw_in"):
        x, y = np.atleast_1d(a[k]), np.atleast_1d(b[k])
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), k
    assert a["aw_out"].shape == (16, len(a["t"]))
    t, G, _ = learned(2, 4, 16, 1)
    for u in (0.05, 0.9):
        a = engine.hetero_equilibrium_on_knots(t, G, *args, u, g.p, g.kappa, g.lam)
        o = oracle.hetero_equilibrium_knots(t, G, *args, u, g.p, g.kappa, g.lam)
        assert a["hr"].shape[0] == 16
        check_knots(a, o, f"K=16 u={u}", paths=True)
        if u == 0.05:
            assert np.array_equal(a["aw_out"], b["aw_out"]) and np.array_equal(a["aw_in"], b["aw_in"])


def test_k12_pipelined_batch_equals_single_sweeps(engine):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    full, _ = config4(6, 24, 12)
    subs = [full.subset(np.arange(k, 6, 2)) for k in range(2)]
    nbat, nc, nu, K = 2, 3, len(full.u), 12
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out = {f: torch.empty(nbat, nc * nu, dtype=torch.float64, device=dev) for f in ("xi", "aw_max", "tol")}
    out["status"] = torch.empty(nbat, nc * nu, dtype=torch.int32, device=dev)
    out["iters"] = torch.empty(nbat, nc * nu, dtype=torch.int32, device=dev)
    engine.sweep_hetero_batch_dev(K, t(np.stack([g.betas for g in subs])), t(full.dist),
                                  t(np.stack([g.eta for g in subs])), t(np.stack([g.t_end for g in subs])),
                                  t(full.u), full.p, full.kappa, full.lam, full.x0, out,
                                  stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    for k, g in enumerate(subs):
        ref = sweep(engine, g, with_groups=False)
        got = {f: out[f][k].cpu().numpy().reshape(nc, nu) for f in ("xi", "aw_max", "tol", "iters")}
        got["status"] = out["status"][k].cpu().numpy().view(np.uint32).reshape(nc, nu)
        assert_bitwise(got, ref, f"batch {k}", fields=("xi", "aw_max", "tol", "status", "iters"))


def _hetero_calls(L, ctx, K):
    """Every heterogeneity entry point called with K groups on valid-looking arguments; the
    device-pointer ones get host arrays, which a refused K never reads."""
    n = 17
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    betas, dist = np.full(n, 1.0), np.full(n, 1.0 / max(K, 1))
    one, u = np.array([10.0]), np.array([0.1])
    tk, Gk = np.array([0.0, 10.0]), np.full((2, n), 0.5)
    res = {k: np.empty(4) for k in ("xi", "aw_max", "tol")}
    st, it = np.empty(4, np.uint32), np.empty(4, np.int32)
    soa = _lib.ResultSoA(P(res["xi"]), None, None, P(res["aw_max"]), P(res["tol"]), P(st), P(it))
    opts = _lib.default_opts()
    o, r = ctypes.byref(opts), ctypes.byref(soa)
    nk, nt = ctypes.c_int64(), ctypes.c_int64()
    buf = np.empty(64)
    return {
        "sbr_sweep_hetero": lambda: L.sbr_sweep_hetero(ctx, K, P(betas), P(dist), P(one), P(one), 1e-4, P(u), 1, 1,
                                                       0.9, 0.3, 0.1, o, r, None, None),
        "sbr_sweep_hetero_dev": lambda: L.sbr_sweep_hetero_dev(ctx, None, K, P(betas), P(dist), P(one), P(one), 1e-4,
                                                               P(u), 1, 1, 0.9, 0.3, 0.1, o, r, None, None),
        "sbr_sweep_hetero_batch_dev": lambda: L.sbr_sweep_hetero_batch_dev(ctx, None, 1, K, P(betas), P(dist), P(one),
                                                                           P(one), 1e-4, P(u), 1, 1, 0.9, 0.3, 0.1, o,
                                                                           r, None, None),
        "sbr_learn_hetero": lambda: L.sbr_learn_hetero(ctx, K, P(betas), P(dist), P(one), 1e-4, 1, o, None, None, 16,
                                                       None, None),
        "sbr_hetero_point_paths": lambda: L.sbr_hetero_point_paths(ctx, K, P(betas), P(dist), 5.0, 10.0, 1e-4, 0.1,
                                                                   0.9, 0.3, 0.1, o, P(buf), P(st), None, None, None,
                                                                   None, None, None, 16, ctypes.byref(nk)),
        "sbr_hetero_equilibrium_on_knots": lambda: L.sbr_hetero_equilibrium_on_knots(
            ctx, K, P(tk), P(Gk), 2, P(betas), P(dist), 5.0, 10.0, P(u), 1, 0.9, 0.3, 0.1, o, r, None, None, None,
            None, None, 16, ctypes.byref(nt)),
    }


@pytest.mark.parametrize("K", [0, 17])
def test_group_count_limits(engine, K):
    L = _lib.load()
    for name, call in _hetero_calls(L, engine._ctx, K).items():
        assert call() == _lib.SBR_EARG, (name, K)
        msg = L.sbr_last_error(engine._ctx)
        assert msg and b"16" in msg and b"Rosenbrock23" in msg, (name, K, msg)


def test_multi_context_refuses_k17(monkeypatch):
    monkeypatch.setenv("SBR_MULTI_SHARED_DEVICES", "1")
    m = sbr.Engine(n_gpus=2)
    try:
        with pytest.raises(_lib.ArgumentError, match="16"):
            m.sweep_hetero(np.full((2, 17), 1.0), np.full(17, 1.0 / 17), 5.0, 10.0, [0.1], 0.9, 0.3, 0.1)
    finally:
        m.close()


def test_zero_filled_opts_keep_the_specialised_k8_path(engine):
    """A zero-filled sbr_opts (no SBR_FLAG_HETERO_WIDE) at K = 8: the results of the defaults."""
    g, o = config4(24, 48, 8)
    L = _lib.load()
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    np_ = g.n_points
    out = {k: np.empty(np_) for k in ("xi", "aw_max", "tol")}
    out["status"], out["iters"] = np.empty(np_, np.uint32), np.empty(np_, np.int32)
    tin, tout = np.empty(np_ * 8), np.empty(np_ * 8)
    soa = _lib.ResultSoA(P(out["xi"]), None, None, P(out["aw_max"]), P(out["tol"]), P(out["status"]), P(out["iters"]))
    opts = _lib.Opts()  # zero-filled
    rc = L.sbr_sweep_hetero(engine._ctx, 8, P(g.betas), P(g.dist), P(g.eta), P(g.t_end), g.x0, P(g.u), len(g.eta),
                            len(g.u), g.p, g.kappa, g.lam, ctypes.byref(opts), ctypes.byref(soa), P(tin), P(tout))
    assert rc == 0, L.sbr_last_error(engine._ctx)
    got = {k: v.reshape(g.shape) for k, v in out.items()}
    got["tau_in_unc"], got["tau_out_unc"] = tin.reshape(*g.shape, 8), tout.reshape(*g.shape, 8)
    assert_bitwise(got, o, "zero-filled opts", fields=FIELDS)


def test_two_rank_rehearsal_k12(engine, monkeypatch):
    """The n-device fan-out (two ranks on the one GPU, SBR_MULTI_SHARED_DEVICES=1) at K = 12."""
    monkeypatch.setenv("SBR_MULTI_SHARED_DEVICES", "1")
    g, o = config4(6, 24, 12)
    m = sbr.Engine(n_gpus=2)
    try:
        a = sweep(m, g)
    finally:
        m.close()
    assert_bitwise(a, sweep(engine, g), "two ranks vs one device")
    assert_bitwise(a, o, "two ranks vs oracle")
