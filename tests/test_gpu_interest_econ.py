"""sbr_sweep_interest_econ on the GPU: β × p × λ × (r, δ) × κ × u of the interest-rate extension in one
call, each β learned and each value function integrated once, bit for bit against one oracle
interest sweep per (p, λ, rate, κ) on the grid I4 (tests/interest_econ_cases.py), rk_steps included,
and through every route of the call: degenerate axes, the r = 0 pair, wave and tile boundaries,
non-default ODE options, chunked classes, the exhaustive flag, the diagnostic stop flags, the
caller's own result arrays, device pointers on a caller's stream, argument errors, the n-rank
fan-out."""
import ctypes

import numpy as np
import pytest

import sbr
from econ_cases import E6
from interest_econ_cases import ALL, FIELDS, I4, WITH_STEPS, X0, counts, freeze, oracle_interest_econ, shape_of
from points_cases import assert_same

pytestmark = pytest.mark.gpu

S = sbr.STATUS
CAP = 65536
SHAPE = shape_of(I4)
SSHAPE = (*SHAPE[:4], SHAPE[5])
N, NS = int(np.prod(SHAPE)), int(np.prod(SSHAPE))
MAXIT = S["SBR_ODE_MAXITERS"]


@pytest.fixture(scope="module")
def ref(oracle):
    """The oracle's I4, computed once (read-only): 36 interest sweeps."""
    return freeze(oracle_interest_econ(oracle, I4))


@pytest.fixture(scope="module")
def gpu(engine):
    """engine.sweep_interest_econ on I4, computed once (read-only): test 1 checks it against the
    oracle, the other routes are compared with it."""
    return freeze(engine.sweep_interest_econ(**I4, x0=X0))


def same_everywhere(r, want, what=""):
    for k in WITH_STEPS:
        assert r[k].shape == want[k].shape, k
        assert_same(r[k], want[k], f"{k}{what}")


def test_i4_oracle_parity(engine, ref, gpu):
    assert SHAPE == (4, 2, 2, 3, 3, 6) and N == 864 and NS == 288
    # what the grid covers, asserted on the oracle's output before anything is compared
    st, xi = ref["status"], ref["xi"]
    assert counts(st) == {0x3: 494, 0x80: 216, 0x6: 78, 0x8: 46, 0x10: 30}
    assert (st[2] == 0x80).all()  # column 2: η past t_end
    assert int(((I4["r"] > 0)[None, None, None, :, None] & np.ones(SSHAPE, bool)).sum()) == 192
    assert int((st[..., 0, :] != st[..., 2, :]).sum()) == 55  # κ = .3 against κ = .9
    both = (st[..., 0, :] & st[..., 1, :] & S["SBR_RUN"]) != 0
    assert int(both.sum()) == 177 and (xi[..., 0, :][both] != xi[..., 1, :][both]).all()  # κ = .3 against .6
    both = (st[:, :, :, 1] & st[:, :, :, 2] & S["SBR_RUN"]) != 0
    assert int(both.sum()) == 158  # the rates (.06, .1) against (.02, .5)
    assert int((xi[:, :, :, 1][both] != xi[:, :, :, 2][both]).sum()) == 144
    assert (ref["rk_steps"][:, :, :, 0] == 0).all() and (ref["rk_steps"][[0, 1, 3]][:, :, :, 1:] > 0).all()
    # column 3 runs from global memory: its knots do not fit the LDS slab
    (t3, _, _), = engine.learn_baseline(I4["beta"][3:4], I4["eta"][3:4], I4["t_end"][3:4], X0, stop_after_eta=True)
    assert len(t3) > engine.device_info()["lds_knot_capacity"]
    for k in ALL:
        assert gpu[k].shape == SHAPE
    assert gpu["rk_steps"].shape == SSHAPE
    same_everywhere(gpu, ref)


@pytest.mark.parametrize("rate", [(.06, .1), (0.0, .1)])
def test_degenerate_axes_equal_the_sweep(engine, rate):
    grid = sbr.fig5_grid(8, n_u=24)
    sw = engine.sweep_interest(grid.beta, grid.eta, grid.t_end, grid.u, grid.p, grid.kappa, grid.lam, *rate,
                               x0=grid.x0)
    r = engine.sweep_interest_econ(grid.beta, grid.eta, grid.t_end, grid.u, grid.p, grid.kappa, grid.lam, *rate,
                                   x0=grid.x0)
    assert (sw["rk_steps"] > 0).any() == (rate[0] > 0)
    for k in ALL:
        assert r[k].shape == (8, 1, 1, 1, 1, 24)
        assert_same(r[k].reshape(8, 24), sw[k], k)
    assert r["rk_steps"].shape == (8, 1, 1, 1, 24)
    assert_same(r["rk_steps"].reshape(8, 24), sw["rk_steps"], "rk_steps")


def test_the_zero_rate_pair_is_the_baseline_product(engine):
    base = engine.sweep_econ(**E6, x0=X0, early_exit=0)
    r = engine.sweep_interest_econ(**E6, r=0.0, delta=0.1, x0=X0)
    assert base["xi"].size == 3456
    for k in ALL:
        assert r[k].shape == (6, 4, 3, 1, 4, 12)
        assert_same(r[k][:, :, :, 0], base[k], k)
    assert (r["rk_steps"] == 0).all()


def test_waves_straddle_rates(engine, oracle):
    # 3 rates × 37 u = 111 lanes: every wave straddles a rate boundary, 5 κ per lane
    g = dict(beta=np.array([1.0, 3.0]), eta=np.full(2, 15.0), t_end=np.full(2, 30.0), p=.5, lam=.01,
             r=np.array([.06, 0.0, .02]), delta=np.array([.1, .3, .5]), kappa=np.array([.1, .3, .5, .7, .9]),
             u=np.linspace(.001, 1, 37))
    o = oracle_interest_econ(oracle, g)
    assert o["xi"].shape == (2, 1, 1, 3, 5, 37)
    assert all((o["status"][:, 0, 0, d] & S["SBR_RUN"]).any() for d in range(3))
    same_everywhere(engine.sweep_interest_econ(**g, x0=X0), o)


def test_a_plane_of_more_than_one_tile(engine, oracle):
    # one column × 70 rates × 60 u = 4,200 lanes, more than EQ_TILE, one κ; 1e-6 keeps it cheap
    kw = dict(rtol=1e-6, atol=1e-6)
    g = dict(beta=np.array([1.0]), eta=np.array([15.0]), t_end=np.array([30.0]), p=.5, lam=.01, kappa=.6,
             r=np.linspace(0.0, .0966, 70), delta=np.linspace(.1, .8, 70), u=np.linspace(0, .6, 60))
    assert (g["r"] < g["delta"]).all()
    o = oracle_interest_econ(oracle, g, **kw)
    assert o["xi"].shape == (1, 1, 1, 70, 1, 60) and o["rk_steps"].size == 4200
    assert len(counts(o["status"])) >= 3 and (o["status"] & S["SBR_RUN"]).any()
    same_everywhere(engine.sweep_interest_econ(**g, x0=X0, ode_rtol=1e-6, ode_atol=1e-6), o)


@pytest.mark.parametrize("cap", [1_000_000, 60])
def test_non_default_ode_options(engine, oracle, cap):
    g = {**I4, "p": .5, "lam": .01, "kappa": np.array([.3, .6]), "r": np.array([.06, 5.0]),
         "delta": np.array([.1, 50.0])}
    o = oracle_interest_econ(oracle, g, rtol=1e-6, atol=1e-6, ode_maxiters=cap)
    st = o["status"]
    if cap == 60:
        # the cap cuts the learning solves and the value functions: SBR_ODE_MAXITERS rides on points
        # that still ran and on points that did not
        run = (st & S["SBR_RUN"]) != 0
        assert ((st[run] & MAXIT) != 0).any() and ((st[~run] & MAXIT) != 0).any()
        assert {0x803, 0x206, 0xA80, 0xA10} <= set(counts(st[:, 0, 0, 0, 1]))  # (.06, .1), κ = .6
    else:
        assert not (st & MAXIT).any() and (st & S["SBR_RUN"]).any()
    r = engine.sweep_interest_econ(**g, x0=X0, ode_rtol=1e-6, ode_atol=1e-6, ode_maxiters=cap)
    same_everywhere(r, o, f" (cap {cap})")


def test_chunked_classes_give_the_same_results(engine, gpu):
    # include/sbr.h: the learning rows, then (knot_capacity × 8 + 12) bytes per column and class
    nb = SHAPE[0]
    engine.set_econ_workspace(nb * (4 * CAP * 8 + 24) + 3 * nb * (CAP * 8 + 12) + 64)  # 3 of 4 classes: 3 + 1
    try:
        r = engine.sweep_interest_econ(**I4, x0=X0, knot_capacity=CAP)
    finally:
        engine.set_econ_workspace(0)
    same_everywhere(r, gpu)


def test_exhaustive_gives_the_same_results(engine, gpu):
    same_everywhere(engine.sweep_interest_econ(**I4, x0=X0, exhaustive=True), gpu)


def test_device_call_on_a_caller_stream(engine, gpu):
    import torch

    dev = torch.device("cuda", engine.device)

    def run(g):
        ins = {k: torch.tensor(np.atleast_1d(v), dtype=torch.float64, device=dev) for k, v in g.items()}
        out = {k: torch.full((N,), -7.0, dtype=torch.float64, device=dev) for k in FIELDS}
        out["status"] = torch.zeros(N, dtype=torch.int32, device=dev)
        out["iters"] = torch.full((N,), -7, dtype=torch.int32, device=dev)
        out["rk_steps"] = torch.full((NS,), -7, dtype=torch.int64, device=dev)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        engine.sweep_interest_econ_dev(**ins, x0=X0, out=out, stream=s.cuda_stream)
        s.synchronize()
        r = {k: v.cpu().numpy().reshape(SSHAPE if k == "rk_steps" else SHAPE) for k, v in out.items()}
        r["status"] = r["status"].view(np.uint32)
        return r

    same_everywhere(run(I4), gpu)
    # one bad element per axis: exactly the points on those hyperplanes are SBR_ARG_INVALID
    q = {k: v.copy() for k, v in I4.items()}
    q["p"][1] = 1.5
    q["lam"][0] = float("nan")
    q["kappa"][2] = 1.0
    q["u"][4] = -0.1
    q["r"][1] = q["delta"][1]
    bad = np.zeros(SHAPE, bool)
    bad[:, 1] = True
    bad[:, :, 0] = True
    bad[:, :, :, 1] = True
    bad[:, :, :, :, 2] = True
    bad[..., 4] = True
    assert int(bad.sum()) == N - 4 * 1 * 1 * 2 * 2 * 5
    sbad = bad[:, :, :, :, 0, :]  # rk_steps has no κ axis: the κ hyperplane is not in it
    assert int(sbad.sum()) == NS - 4 * 1 * 1 * 2 * 5
    r = run(q)
    assert (r["status"][bad] == S["SBR_ARG_INVALID"]).all()
    for k in ("xi", "tau_in_unc", "tau_out_unc", "aw_max"):
        assert np.isnan(r[k][bad]).all(), k
    assert np.isposinf(r["tol"][bad]).all() and (r["iters"][bad] == 0).all()
    assert (r["rk_steps"][sbad] == 0).all()
    for k in ALL:
        assert_same(r[k][~bad], gpu[k][~bad], k)
    assert_same(r["rk_steps"][~sbad], gpu["rk_steps"][~sbad], "rk_steps")


def filled():
    out = {k: np.full(N, -7.0) for k in FIELDS}
    out["status"] = np.full(N, 0xDEAD, np.uint32)
    out["iters"] = np.full(N, -7, np.int32)
    out["rk_steps"] = np.full(NS, -7, np.int64)
    return out


def untouched(out):
    return (all((out[k] == -7.0).all() for k in FIELDS) and (out["status"] == 0xDEAD).all()
            and (out["iters"] == -7).all() and (out["rk_steps"] == -7).all())


def test_caller_arrays_are_filled(engine, gpu):
    out = filled()
    r = engine.sweep_interest_econ(**I4, x0=X0, out=out)
    same_everywhere(r, gpu)
    for k in WITH_STEPS:  # the results are views of the caller's own arrays
        assert np.shares_memory(r[k], out[k]), k
        assert_same(out[k], gpu[k].reshape(-1), k)
    # rk_steps and iters are optional
    out = {k: v for k, v in filled().items() if k not in ("iters", "rk_steps")}
    r = engine.sweep_interest_econ(**I4, x0=X0, out=out)
    assert r["iters"] is None and r["rk_steps"] is None
    for k in (*FIELDS, "status"):
        assert_same(r[k], gpu[k], k)
    # an rk_steps array with a κ axis is refused before the call
    out = {**filled(), "rk_steps": np.full(N, -7, np.int64)}
    with pytest.raises(sbr.ArgumentError):
        engine.sweep_interest_econ(**I4, x0=X0, out=out)
    assert (out["rk_steps"] == -7).all() and (out["status"] == 0xDEAD).all()


@pytest.mark.parametrize("flag", ["SBR_FLAG_DIAG_STOP_AFTER_BUFFER", "SBR_FLAG_DIAG_STOP_AFTER_BISECT",
                                  "SBR_FLAG_DIAG_COUNT_AW_BLOCKS"])
def test_diagnostic_flags_pass_through_as_in_the_sweep(engine, gpu, flag):
    """I4's columns and u at p = .5, λ = .01, the rates (0, .1) and (.06, .1) and every κ: all seven
    fields and rk_steps equal engine.sweep_interest at the same flag.  What the sweep must show first
    follows from solve_point / solve_interest_point / solve_from_buffers: a stop after the buffers
    leaves status 0 (I4 has no learning or value-function bit) on every column with a hazard path, a
    stop after the bisection leaves status 0 exactly where the unflagged sweep has a run — the case
    in which solve_from_buffers returns without writing a status — and counting AW blocks changes
    no status."""
    f = getattr(sbr._lib, flag)
    g = {**I4, "p": .5, "lam": .01, "r": I4["r"][:2], "delta": I4["delta"][:2]}
    plain = gpu["status"][:, 0, 0, :2]
    sw = {k: np.empty((4, 2, 3, 6), gpu[k].dtype) for k in ALL}
    steps = np.empty((4, 2, 6), np.int64)
    for d in range(2):
        for c, kc in enumerate(I4["kappa"]):
            one = engine.sweep_interest(I4["beta"], I4["eta"], I4["t_end"], I4["u"], .5, float(kc), .01,
                                        float(I4["r"][d]), float(I4["delta"][d]), x0=X0, flags=f)
            for k in ALL:
                sw[k][:, d, c] = one[k]
            if c == 0:
                steps[:, d] = one["rk_steps"]
            else:
                assert np.array_equal(steps[:, d], one["rk_steps"])
    run = (plain & S["SBR_RUN"]) != 0
    assert run[:, 0].any() and run[:, 1].any() and not run[2].any()
    if flag.endswith("AFTER_BUFFER"):
        assert (sw["status"][[0, 1, 3]] == 0).all() and (sw["status"][2] == 0x80).all()
    elif flag.endswith("AFTER_BISECT"):
        assert (sw["status"][run] == 0).all() and np.array_equal(sw["status"][~run], plain[~run])
    else:
        assert np.array_equal(sw["status"], plain)
    r = engine.sweep_interest_econ(**g, x0=X0, flags=f)
    for k in ALL:
        assert r[k].shape == (4, 1, 1, 2, 3, 6)
        assert_same(r[k][:, 0, 0], sw[k], f"{k} ({flag})")
    assert_same(r["rk_steps"][:, 0, 0], steps, f"rk_steps ({flag})")


def test_host_argument_errors_write_nothing(engine):
    for axis, i, v in (("p", 1, 1.5), ("p", 0, -0.1), ("kappa", 0, 1.0), ("kappa", 2, 0.0), ("lam", 1, 0.0),
                       ("lam", 0, float("nan")), ("u", 4, -0.1), ("beta", 0, 0.0), ("r", 1, 0.1), ("r", 2, 0.7),
                       ("r", 0, -0.01), ("delta", 2, float("nan")), ("delta", 0, 0.0)):
        q = {k: a.copy() for k, a in I4.items()}
        q[axis][i] = v
        out = filled()
        with pytest.raises(sbr.ArgumentError):
            engine.sweep_interest_econ(**q, x0=X0, out=out)
        assert untouched(out), (axis, i, v)
    out = filled()
    with pytest.raises(sbr.ArgumentError):
        engine.sweep_interest_econ(**I4, x0=X0, out=out, flags=sbr._lib.SBR_FLAG_XI_GUESS)
    assert untouched(out)
    # n_rate = 0 at the C boundary (an empty axis)
    out = filled()
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    soa = sbr._lib.ResultSoA(*[P(out[k]) for k in (*FIELDS, "status", "iters")])
    opts = sbr._lib.default_opts(early_exit_nan_run=0)
    rc = engine._L.sbr_sweep_interest_econ(engine._ctx, P(I4["beta"]), P(I4["eta"]), P(I4["t_end"]), X0, P(I4["u"]),
                                           4, 6, P(I4["p"]), 2, P(I4["lam"]), 2, P(I4["r"]), P(I4["delta"]), 0,
                                           P(I4["kappa"]), 3, ctypes.byref(opts), ctypes.byref(soa),
                                           P(out["rk_steps"]))
    assert rc == sbr._lib.SBR_EARG and untouched(out)
    # more than 2^40 results (refused before any array is read), more columns than one device's launch takes
    rc = engine._L.sbr_sweep_interest_econ(engine._ctx, P(I4["beta"]), P(I4["eta"]), P(I4["t_end"]), X0, P(I4["u"]),
                                           1 << 30, 1 << 20, P(I4["p"]), 2, P(I4["lam"]), 2, P(I4["r"]),
                                           P(I4["delta"]), 1 << 10, P(I4["kappa"]), 3, ctypes.byref(opts),
                                           ctypes.byref(soa), P(out["rk_steps"]))
    assert rc == sbr._lib.SBR_EARG and untouched(out)
    wide = np.ones(65536)
    rc = engine._L.sbr_sweep_interest_econ(engine._ctx, P(wide), P(wide), P(wide), X0, P(I4["u"]), 65536, 1,
                                           P(I4["p"]), 1, P(I4["lam"]), 1, P(I4["r"]), P(I4["delta"]), 1,
                                           P(I4["kappa"]), 1, ctypes.byref(opts), ctypes.byref(soa),
                                           P(out["rk_steps"]))
    assert rc == sbr._lib.SBR_EARG and untouched(out)


def test_three_rank_rehearsal_on_a_shared_device(gpu, monkeypatch):
    monkeypatch.setenv("SBR_MULTI_SHARED_DEVICES", "1")
    m = sbr.Engine(n_gpus=3)
    try:
        assert m.n_gpus == 3
        r = m.sweep_interest_econ(**I4, x0=X0)
    finally:
        m.close()
    same_everywhere(r, gpu)
