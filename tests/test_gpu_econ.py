"""sbr_sweep_econ on the GPU: β × p × λ × κ × u in one call, each β learned once, bit for bit against
one oracle β × u sweep per (p, λ, κ) on the grid E6 (tests/econ_cases.py), and through every route
of the call: degenerate axes, tile and wave boundaries, chunked classes, the exhaustive flag, a
non-default ODE cap, device pointers on a caller's stream, argument errors, the n-rank fan-out."""
import numpy as np
import pytest

import sbr
from econ_cases import ALL, E6, FIELDS, X0, counts, freeze, oracle_econ, shape_of
from points_cases import assert_same

pytestmark = pytest.mark.gpu

S = sbr.STATUS
CAP = 65536
SHAPE = shape_of(E6)
N = int(np.prod(SHAPE))


@pytest.fixture(scope="module")
def ref(oracle):
    """The oracle's E6, computed once (read-only): 48 β × u sweeps."""
    return freeze(oracle_econ(oracle, E6))


@pytest.fixture(scope="module")
def ref5(oracle):
    """... with the early-exit rule (threshold 5) applied per (p, λ, κ)."""
    return freeze(oracle_econ(oracle, E6, early_exit=5))


@pytest.fixture(scope="module")
def gpu(engine):
    """engine.sweep_econ on E6, computed once (read-only): test 1 checks it against the oracle, the
    other routes are compared with it."""
    return freeze(engine.sweep_econ(**E6, x0=X0))


def test_e6_oracle_parity(engine, ref, ref5, gpu):
    assert SHAPE == (6, 4, 3, 4, 12) and N == 3456
    # what the grid covers, asserted on the oracle's output before anything is compared
    assert counts(ref["status"]) == {0x3: 1541, 0x6: 800, 0x8: 393, 0x10: 145, 0x20: 1, 0x80: 576}
    assert (ref["status"][4] == 0x80).all()  # column 4: η past t_end
    assert ref["n_knots"].tolist() == [1321, 2848, 2893, 2883, 1507, 28051]
    assert abs(ref["xi"][1, 1, 1, 2, 3] - 10.215439283) <= 5e-9  # the Fig 3 equilibrium
    assert int(((ref5["status"] & S["SBR_SKIPPED_EARLY_EXIT"]) != 0).sum()) == 928
    # column 5 runs from global memory: its knots do not fit the LDS slab
    (t5, _, _), = engine.learn_baseline(E6["beta"][5:6], E6["eta"][5:6], E6["t_end"][5:6], X0, stop_after_eta=True)
    assert len(t5) > engine.device_info()["lds_knot_capacity"]
    for k in ALL:
        assert gpu[k].shape == SHAPE
        assert_same(gpu[k], ref[k], k)
    g5 = engine.sweep_econ(**E6, x0=X0, early_exit=5)
    for k in ALL:
        assert_same(g5[k], ref5[k], f"{k} (early_exit = 5)")


def test_degenerate_axes_equal_the_sweep(engine):
    grid = sbr.fig5_grid(24, n_u=40)
    for ee in (0, 5):
        sw = engine.sweep_baseline(grid, early_exit=ee)
        r = engine.sweep_econ(grid.beta, grid.eta, grid.t_end, grid.u, grid.p, grid.kappa, grid.lam, x0=grid.x0,
                              early_exit=ee)
        for k in ALL:
            assert r[k].shape == (24, 1, 1, 1, 40)
            assert_same(r[k].reshape(24, 40), sw[k], f"{k} (early_exit = {ee})")


def test_tile_and_wave_boundaries(engine, oracle):
    # the plane's 120 × 37 = 4,440 points exceed the 4,096-point tile, and the 37-long u rows make
    # every wave straddle κ rows
    g = dict(beta=np.array([1.0, 3.0]), eta=np.full(2, 15.0), t_end=np.full(2, 30.0), p=.5, lam=.01,
             kappa=np.linspace(.02, .98, 120), u=np.linspace(.001, 1, 37))
    o = oracle_econ(oracle, g)
    assert counts(o["status"]) == {0x3: 2052, 0x6: 5760, 0x8: 701, 0x10: 367}
    r = engine.sweep_econ(**g, x0=X0)
    for k in ALL:
        assert r[k].shape == (2, 1, 1, 120, 37)
        assert_same(r[k], o[k], k)


def test_chunked_classes_give_the_same_results(engine, gpu):
    # include/sbr.h: the learning rows, then (knot_capacity × 8 + 12) bytes per column and class
    nb = SHAPE[0]
    engine.set_econ_workspace(nb * (4 * CAP * 8 + 24) + 5 * nb * (CAP * 8 + 12) + 64)  # 5 of 12 classes: 5 + 5 + 2
    try:
        r = engine.sweep_econ(**E6, x0=X0, knot_capacity=CAP)
    finally:
        engine.set_econ_workspace(0)
    for k in ALL:
        assert_same(r[k], gpu[k], k)


def test_exhaustive_gives_the_same_results(engine, gpu):
    r = engine.sweep_econ(**E6, x0=X0, exhaustive=True)
    for k in ALL:
        assert_same(r[k], gpu[k], k)


def test_non_default_ode_cap(engine, oracle):
    g = dict(beta=np.array([1.0, 40.0]), eta=np.full(2, 15.0), t_end=np.full(2, 30.0), p=np.array([.5, .9]),
             kappa=np.array([.3, .6]), lam=.01, u=E6["u"])
    o = oracle_econ(oracle, g, ode_maxiters=2500)
    # column 0 is cut past η (SBR_ODE_MAXITERS rides on solved points), column 1 before η
    assert counts(o["status"][0]) == {0x203: 21, 0x206: 26, 0x208: 1}
    assert counts(o["status"][1]) == {0x280: 48}
    r = engine.sweep_econ(**g, x0=X0, ode_maxiters=2500)
    for k in ALL:
        assert r[k].shape == (2, 2, 1, 2, 12)
        assert_same(r[k], o[k], k)


def test_device_call_on_a_caller_stream(engine, gpu):
    import torch

    dev = torch.device("cuda", engine.device)

    def run(g):
        ins = {k: torch.tensor(np.atleast_1d(v), dtype=torch.float64, device=dev) for k, v in g.items()}
        out = {k: torch.full((N,), -7.0, dtype=torch.float64, device=dev) for k in FIELDS}
        out["status"] = torch.zeros(N, dtype=torch.int32, device=dev)
        out["iters"] = torch.full((N,), -7, dtype=torch.int32, device=dev)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        engine.sweep_econ_dev(**ins, x0=X0, out=out, stream=s.cuda_stream)
        s.synchronize()
        r = {k: v.cpu().numpy().reshape(SHAPE) for k, v in out.items()}
        r["status"] = r["status"].view(np.uint32)
        return r

    r = run(E6)
    for k in ALL:
        assert_same(r[k], gpu[k], k)
    # one bad element per axis: exactly the points on those hyperplanes are SBR_ARG_INVALID
    q = {k: v.copy() for k, v in E6.items()}
    q["p"][2] = 1.5
    q["kappa"][0] = 1.0
    q["lam"][1] = float("nan")
    q["u"][7] = -0.1
    bad = np.zeros(SHAPE, bool)
    bad[:, 2] = True
    bad[:, :, 1] = True
    bad[:, :, :, 0] = True
    bad[..., 7] = True
    assert int(bad.sum()) == N - 6 * 3 * 2 * 3 * 11
    r = run(q)
    assert (r["status"][bad] == S["SBR_ARG_INVALID"]).all()
    for k in ("xi", "tau_in_unc", "tau_out_unc", "aw_max"):
        assert np.isnan(r[k][bad]).all(), k
    assert np.isposinf(r["tol"][bad]).all() and (r["iters"][bad] == 0).all()
    for k in ALL:
        assert_same(r[k][~bad], gpu[k][~bad], k)


def test_host_argument_errors_write_nothing(engine):
    def filled():
        out = {k: np.full(N, -7.0) for k in FIELDS}
        out["status"] = np.full(N, 0xDEAD, np.uint32)
        out["iters"] = np.full(N, -7, np.int32)
        return out

    def untouched(out):
        return (all((out[k] == -7.0).all() for k in FIELDS) and (out["status"] == 0xDEAD).all()
                and (out["iters"] == -7).all())

    for axis, i, v in (("p", 2, 1.5), ("p", 0, -0.1), ("kappa", 0, 1.0), ("kappa", 3, 0.0), ("lam", 1, 0.0),
                       ("lam", 1, float("nan")), ("u", 7, -0.1), ("beta", 0, 0.0)):
        q = {k: a.copy() for k, a in E6.items()}
        q[axis][i] = v
        out = filled()
        with pytest.raises(sbr.ArgumentError):
            engine.sweep_econ(**q, x0=X0, out=out)
        assert untouched(out), (axis, i, v)
    out = filled()
    with pytest.raises(sbr.ArgumentError):
        engine.sweep_econ(**E6, x0=X0, out=out, flags=sbr._lib.SBR_FLAG_XI_GUESS)
    assert untouched(out)
    # n_p = 0 at the C boundary (an empty axis)
    import ctypes

    out = filled()
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    soa = sbr._lib.ResultSoA(*[P(out[k]) for k in (*FIELDS, "status", "iters")])
    opts = sbr._lib.default_opts(early_exit_nan_run=0)
    rc = engine._L.sbr_sweep_econ(engine._ctx, P(E6["beta"]), P(E6["eta"]), P(E6["t_end"]), X0, P(E6["u"]), 6, 12,
                                  P(E6["p"]), 0, P(E6["lam"]), 3, P(E6["kappa"]), 4, ctypes.byref(opts),
                                  ctypes.byref(soa))
    assert rc == sbr._lib.SBR_EARG and untouched(out)
    out = filled()
    with pytest.raises(sbr.ArgumentError):
        engine.sweep_econ(**{**E6, "p": np.empty(0)}, x0=X0, out={k: v[:0] for k, v in out.items()})
    assert untouched(out)


def test_three_rank_rehearsal_on_a_shared_device(gpu, monkeypatch):
    monkeypatch.setenv("SBR_MULTI_SHARED_DEVICES", "1")
    m = sbr.Engine(n_gpus=3)
    try:
        assert m.n_gpus == 3
        r = m.sweep_econ(**E6, x0=X0)
    finally:
        m.close()
    for k in ALL:
        assert_same(r[k], gpu[k], k)
