"""sbr_sweep_hetero_econ on the GPU: K groups × p × λ × κ × u in one call, each column learned once and
each hazard class formed once, bit for bit (all seven fields, the group buffers included) against
one oracle sweep_hetero per (p, λ, κ) on the grids H3(K) (tests/hetero_econ_cases.py), and through
every route of the call: the specialised and the group-looped kernels, degenerate axes, tile and
wave boundaries, chunked classes, the global-memory launch, the exhaustive flag, a non-default ODE
cap, device pointers on a caller's stream, argument errors, the n-rank fan-out."""
import ctypes
import functools

import numpy as np
import pytest

import sbr
from hetero_econ_cases import (FIELDS, H3_COUNTS, P2, U12, assert_bitwise, counts, freeze, grid, h3_oracle,
                               oracle_hetero_econ, shape_of)

pytestmark = pytest.mark.gpu

S = sbr.STATUS
CAP = 16384


@functools.lru_cache(maxsize=None)
def _gpu_h3(eng, K: int, wide: bool = False):
    """eng.sweep_hetero_econ on H3(K), computed once (read-only): test 1 checks it against the oracle,
    the other routes are compared with it."""
    g, _ = h3_oracle(K)
    return freeze(eng.sweep_hetero_econ(**g, wide=wide))


@pytest.mark.parametrize("K,wide", [(2, False), (8, False), (5, False), (16, False), (8, True)])
def test_h3_oracle_parity(engine, K, wide):
    g, ref = h3_oracle(K)
    assert shape_of(g) == (3, 2, 2, 3, 12)
    # what the grid covers, asserted on the oracle's output before anything is compared
    assert counts(ref["status"]) == H3_COUNTS[K]
    r = _gpu_h3(engine, K, wide)
    assert r["xi"].shape == (3, 2, 2, 3, 12) and r["tau_in_unc"].shape == (3, 2, 2, 3, 12, K)
    assert_bitwise(r, ref, f"H3({K}) wide={wide}")


@pytest.mark.parametrize("K", [4, 7])
def test_degenerate_axes_equal_the_sweep(engine, K):
    g = sbr.hetero_config4(6, 24, K)
    sw = engine.sweep_hetero(g.betas, g.dist, g.eta, g.t_end, g.u, g.p, g.kappa, g.lam, g.x0)
    r = engine.sweep_hetero_econ(g.betas, g.dist, g.eta, g.t_end, g.u, g.p, g.kappa, g.lam, g.x0)
    for f in FIELDS:
        assert r[f].shape == (6, 1, 1, 1, 24) + ((K,) if f.startswith("tau_") else ())
    assert_bitwise({f: r[f].reshape(sw[f].shape) for f in FIELDS}, sw, f"K = {K}")


# oracle status counts of the one-column planes below, measured on the CPU oracle
TILE_COUNTS = {(2, 30, 37): {0x803: 593, 0x808: 382, 0x810: 98, 0x880: 37},
               (5, 30, 37): {0x803: 744, 0x808: 204, 0x810: 162},
               (2, 3, 5): {0x803: 10, 0x808: 3, 0x810: 2},
               (5, 3, 5): {0x803: 9, 0x808: 3, 0x810: 3}}


@pytest.mark.parametrize("K,wide,n_kappa,n_u", [(2, False, 30, 37), (5, True, 30, 37), (2, False, 3, 5),
                                                (5, True, 3, 5)])
def test_tile_and_wave_boundaries(engine, oracle, K, wide, n_kappa, n_u):
    # 30 × 37 = 1,110 points: more than four 256-lane tiles, and the 37-long u rows make every wave
    # straddle κ rows; 3 × 5 = 15 points: the 64-lane path
    g = grid(3, 12, K, u=np.linspace(.001, 1, n_u), p=.9, lam=.1, kappa=np.linspace(.02, .98, n_kappa))
    g = {k: (v[1:2] if k in ("betas", "eta", "t_end") else v) for k, v in g.items()}  # one column
    ref = oracle_hetero_econ(oracle, g)
    assert counts(ref["status"]) == TILE_COUNTS[K, n_kappa, n_u]
    r = engine.sweep_hetero_econ(**g, wide=wide)
    assert r["xi"].shape == (1, 1, 1, n_kappa, n_u)
    assert_bitwise(r, ref, f"K = {K}, {n_kappa} x {n_u}")


def test_chunked_classes_give_the_same_results(engine):
    # include/sbr.h: the learning rows, then (2 × K × knot_capacity × 8 + 12) bytes per column and class
    K, nc = 8, 3
    engine.set_econ_workspace(nc * ((1 + 3 * K) * CAP * 8 + 24) + 3 * nc * (2 * K * CAP * 8 + 12) + 64)  # 3 + 1 classes
    try:
        g, _ = h3_oracle(K)
        r = engine.sweep_hetero_econ(**g, knot_capacity=CAP)
    finally:
        engine.set_econ_workspace(0)
    assert_bitwise(r, _gpu_h3(engine, K), "3 + 1 classes")


@pytest.mark.parametrize("K", [8, 5])
def test_global_memory_launch(engine, K):
    g, ref = h3_oracle(K)
    assert (ref["n_knots_all"] > 4096).all()  # every column is beyond the 4,096-knot slab
    engine.set_hetero_econ_slab(4096)
    try:
        r = engine.sweep_hetero_econ(**g)
    finally:
        engine.set_hetero_econ_slab(0)
    assert_bitwise(r, _gpu_h3(engine, K), f"K = {K}, slab 4096")


@pytest.mark.parametrize("K", [8, 5])
def test_exhaustive_gives_the_same_results(engine, K):
    g, _ = h3_oracle(K)
    r = engine.sweep_hetero_econ(**g, exhaustive=True)
    assert_bitwise(r, _gpu_h3(engine, K), f"K = {K}, exhaustive")


def test_non_default_ode_cap(engine, oracle):
    g = grid(3, 12, 8, u=U12, p=P2, kappa=np.array([.3, .6]), lam=.1)
    o = oracle_hetero_econ(oracle, g, ode_maxiters=6000)
    # the columns are cut past η: SBR_ODE_MAXITERS rides on solved points
    assert o["n_knots"].tolist() == [5145, 5149, 5157]
    assert [counts(o["status"][c, 1, 0, 0]) for c in range(3)] == [{0xa03: 12}, {0xa03: 11, 0xa80: 1},
                                                                  {0xa03: 9, 0xa80: 3}]
    r = engine.sweep_hetero_econ(**g, ode_maxiters=6000)
    assert r["xi"].shape == (3, 2, 1, 2, 12)
    assert_bitwise(r, o, "ode_maxiters = 6000")
    o = oracle_hetero_econ(oracle, g, ode_maxiters=3000)
    assert counts(o["status"]) == {0xa80: 144}  # every column cut before η
    r = engine.sweep_hetero_econ(**g, ode_maxiters=3000)
    assert_bitwise(r, o, "ode_maxiters = 3000")


def test_device_call_on_a_caller_stream(engine):
    import torch

    K = 8
    g0, _ = h3_oracle(K)
    host = _gpu_h3(engine, K)
    shape = shape_of(g0)
    n = int(np.prod(shape))
    dev = torch.device("cuda", engine.device)

    def run(g):
        ins = {k: torch.tensor(np.ascontiguousarray(np.atleast_1d(v)).reshape(-1), dtype=torch.float64, device=dev)
               for k, v in g.items() if k != "x0"}
        out = {k: torch.full((n,), -7.0, dtype=torch.float64, device=dev) for k in ("xi", "aw_max", "tol")}
        out["status"] = torch.zeros(n, dtype=torch.int32, device=dev)
        out["iters"] = torch.full((n,), -7, dtype=torch.int32, device=dev)
        for k in ("tau_in_unc", "tau_out_unc"):
            out[k] = torch.full((n * K,), -7.0, dtype=torch.float64, device=dev)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        engine.sweep_hetero_econ_dev(K, **ins, x0=g["x0"], out=out, stream=s.cuda_stream)
        s.synchronize()
        r = {k: v.cpu().numpy().reshape(shape + ((K,) if k.startswith("tau_") else ())) for k, v in out.items()}
        r["status"] = r["status"].view(np.uint32)
        return r

    assert_bitwise(run(g0), host, "device call")
    # one bad element per axis: exactly the points on those hyperplanes carry the sentinel
    q = {k: np.array(v, copy=True) for k, v in g0.items()}
    q["p"][1] = 1.5
    q["kappa"][0] = 1.0
    q["lam"][1] = float("nan")
    q["u"][7] = -0.1
    bad = np.zeros(shape, bool)
    bad[:, 1] = True
    bad[:, :, 1] = True
    bad[:, :, :, 0] = True
    bad[..., 7] = True
    assert int(bad.sum()) == n - 3 * 1 * 1 * 2 * 11
    r = run(q)
    assert (r["status"][bad] == S["SBR_ARG_INVALID"]).all()
    for k in ("xi", "aw_max", "tau_in_unc", "tau_out_unc"):
        assert np.isnan(r[k][bad]).all(), k
    assert np.isposinf(r["tol"][bad]).all() and (r["iters"][bad] == 0).all()
    assert_bitwise(r, host, "points off the bad hyperplanes", where=~bad)


def test_host_argument_errors_write_nothing(engine):
    K = 8
    g0, _ = h3_oracle(K)
    n = int(np.prod(shape_of(g0)))

    def filled():
        out = {k: np.full(n, -7.0) for k in ("xi", "aw_max", "tol")}
        out["status"] = np.full(n, 0xDEAD, np.uint32)
        out["iters"] = np.full(n, -7, np.int32)
        out["tau_in_unc"] = np.full(n * K, -7.0)
        out["tau_out_unc"] = np.full(n * K, -7.0)
        return out

    def untouched(out):
        return (all((out[k] == -7.0).all() for k in ("xi", "aw_max", "tol", "tau_in_unc", "tau_out_unc"))
                and (out["status"] == 0xDEAD).all() and (out["iters"] == -7).all())

    for axis, i, v in (("p", 1, 1.5), ("p", 0, -0.1), ("kappa", 0, 1.0), ("kappa", 2, 0.0), ("lam", 1, 0.0),
                       ("lam", 1, float("nan")), ("u", 7, -0.1), ("betas", (0, 0), 0.0)):
        q = {k: np.array(a, copy=True) for k, a in g0.items()}
        q[axis][i] = v
        out = filled()
        with pytest.raises(sbr.ArgumentError):
            engine.sweep_hetero_econ(**q, out=out)
        assert untouched(out), (axis, i, v)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    a = {k: np.ascontiguousarray(v, np.float64) for k, v in g0.items() if k != "x0"}

    def call(K_, betas, n_p, flags=0):
        out = filled()
        soa = sbr._lib.ResultSoA(P(out["xi"]), None, None, P(out["aw_max"]), P(out["tol"]), P(out["status"]),
                                 P(out["iters"]))
        opts = sbr._lib.default_opts(early_exit_nan_run=0, knot_capacity=CAP, flags=flags)
        rc = engine._L.sbr_sweep_hetero_econ(engine._ctx, K_, P(betas), P(a["dist"]), P(a["eta"]), P(a["t_end"]),
                                             g0["x0"], P(a["u"]), 3, 12, P(a["p"]), n_p, P(a["lam"]), 2, P(a["kappa"]),
                                             3, ctypes.byref(opts), ctypes.byref(soa), P(out["tau_in_unc"]),
                                             P(out["tau_out_unc"]))
        return rc, out

    wide = np.ascontiguousarray(np.repeat(a["betas"], 3, axis=1)[:, :17])  # K = 17: beyond SBR_HETERO_MAX_K
    for K_, betas, n_p, flags in ((17, wide, 2, 0), (K, a["betas"], 2, sbr._lib.SBR_FLAG_XI_GUESS),
                                  (K, a["betas"], 0, 0)):
        rc, out = call(K_, betas, n_p, flags)
        assert rc == sbr._lib.SBR_EARG and untouched(out), (K_, n_p, flags)


def test_three_rank_rehearsal_on_a_shared_device(engine, monkeypatch):
    K = 8
    g, _ = h3_oracle(K)
    one = _gpu_h3(engine, K)
    monkeypatch.setenv("SBR_MULTI_SHARED_DEVICES", "1")
    m = sbr.Engine(n_gpus=3)
    try:
        assert m.n_gpus == 3
        r = m.sweep_hetero_econ(**g)
    finally:
        m.close()
    assert_bitwise(r, one, "three ranks")
