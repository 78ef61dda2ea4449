"""sbr_solve_points on the GPU: a list of models, each point with its own (β, η, t_end, u, p, κ, λ),
bit for bit against the oracle's per-point value
    oracle.sweep_baseline([β_i], η_i, t_end_i, [u_i], p_i, κ_i, λ_i)
on the seeded list L70 (tests/points_cases.py), against the β × u sweep on a flattened grid, and
through every route of the call: bad points, chunked workspace, device pointers on a caller's
stream, the n-rank fan-out."""
import numpy as np
import pytest

import sbr
from points_cases import ALL, FIELDS, X0, assert_same, l70, oracle_points

pytestmark = pytest.mark.gpu

S = sbr.STATUS
CAP = 65536


@pytest.fixture(scope="module")
def pts():
    return l70()


@pytest.fixture(scope="module")
def ref(oracle, pts):
    """The oracle's L70, computed once (read-only)."""
    o = oracle_points(oracle, pts)
    for v in o.values():
        v.setflags(write=False)
    return o


@pytest.fixture(scope="module")
def gpu(engine, pts):
    """engine.solve_points on L70, computed once (read-only): test 1 checks it against the oracle,
    the other routes are compared with it."""
    g = engine.solve_points(**pts, x0=X0)
    for v in g.values():
        v.setflags(write=False)
    return g


def test_l70_oracle_parity(engine, pts, ref, gpu):
    st = ref["status"]
    # what the list covers, asserted on the oracle's output before anything is compared
    count = lambda bits: int((st == bits).sum())  # noqa: E731
    assert count(S["SBR_RUN"] | S["SBR_CONVERGED"]) == 52
    assert count(S["SBR_CONVERGED"] | S["SBR_NO_RUN_HR_BELOW_U"]) == 15
    assert count(S["SBR_OOB"]) == 1 and st[3] == S["SBR_OOB"]
    assert count(S["SBR_NO_RUN_MAXITER"]) == 1 and ref["iters"][st == S["SBR_NO_RUN_MAXITER"]].tolist() == [99]
    assert count(S["SBR_NO_RUN_COLLAPSE"]) == 1
    np.testing.assert_allclose(ref["xi"][[64, 65, 66]], [10.21543928, 9.67024035, 9.18615038], rtol=0, atol=5e-9)
    # point 49 runs from global memory: its knots do not fit the LDS slab
    assert st[49] == S["SBR_RUN"] | S["SBR_CONVERGED"] and ref["n_knots"][49] == 28051
    (t49, _, _), = engine.learn_baseline(pts["beta"][49:50], pts["eta"][49:50], pts["t_end"][49:50], X0,
                                         stop_after_eta=True)
    assert len(t49) > engine.device_info()["lds_knot_capacity"]
    for k in ALL:
        assert gpu[k].shape == (70,)
        assert_same(gpu[k], ref[k], k)
    for k in ALL:  # the same model twice in one list: identical results
        assert_same(gpu[k][0], gpu[k][64], f"{k} of points 0 and 64")


def test_flattened_grid_equals_the_sweep(engine):
    g = sbr.fig5_grid(500).subset([0, 124, 249, 374, 499])
    u = sbr.julia_range("0.001", "1", 37)
    grid = sbr.BaselineGrid(g.beta, u, g.eta, g.t_end, g.p, g.kappa, g.lam, g.x0)
    sw = engine.sweep_baseline(grid)
    r = engine.solve_points(np.repeat(grid.beta, 37), np.tile(u, 5), np.repeat(grid.eta, 37),
                            np.repeat(grid.t_end, 37), grid.p, grid.kappa, grid.lam, x0=grid.x0)
    for k in ALL:
        assert r[k].shape == (5 * 37,)
        assert_same(r[k], sw[k].reshape(-1), k)


def test_bad_points_touch_no_other_point(engine, pts, gpu):
    bad = {5: ("beta", 0.0), 10: ("t_end", 0.0), 20: ("eta", -1.0), 30: ("u", -0.1), 40: ("p", 1.5),
           50: ("kappa", 1.0), 60: ("lam", 0.0), 69: ("beta", float("nan"))}
    q = {k: v.copy() for k, v in pts.items()}
    for i, (k, v) in bad.items():
        q[k][i] = v
    r = engine.solve_points(**q, x0=X0)
    idx = np.array(sorted(bad))
    assert (r["status"][idx] == S["SBR_ARG_INVALID"]).all(), r["status"][idx]
    for k in ("xi", "tau_in_unc", "tau_out_unc", "aw_max"):
        assert np.isnan(r[k][idx]).all(), k
    assert np.isposinf(r["tol"][idx]).all() and (r["iters"][idx] == 0).all()
    keep = np.setdiff1d(np.arange(70), idx)
    assert len(keep) == 62
    for k in ALL:
        assert_same(r[k][keep], gpu[k][keep], k)
    # a call-level ArgumentError writes none of the caller's arrays
    out = {k: np.full(70, -7.0) for k in FIELDS}
    out["status"] = np.full(70, 0xDEAD, np.uint32)
    out["iters"] = np.full(70, -7, np.int32)
    with pytest.raises(sbr.ArgumentError):
        engine.solve_points(**pts, x0=-1.0, out=out)
    assert all((out[k] == -7.0).all() for k in FIELDS)
    assert (out["status"] == 0xDEAD).all() and (out["iters"] == -7).all()


def test_chunked_workspace_gives_the_same_results(engine, pts, gpu):
    engine.set_points_workspace(24 * (4 * CAP * 8 + 24))  # 24 points per chunk: 24 + 24 + 22
    try:
        r = engine.solve_points(**pts, x0=X0, knot_capacity=CAP)
    finally:
        engine.set_points_workspace(0)
    for k in ALL:
        assert_same(r[k], gpu[k], k)


def test_device_call_on_a_caller_stream(engine, pts, gpu):
    import torch

    dev = torch.device("cuda", engine.device)

    def run(n):
        ins = {k: torch.tensor(v[:n], dtype=torch.float64, device=dev) for k, v in pts.items()}
        out = {k: torch.full((n,), -7.0, dtype=torch.float64, device=dev) for k in FIELDS}
        out["status"] = torch.zeros(n, dtype=torch.int32, device=dev)
        out["iters"] = torch.full((n,), -7, dtype=torch.int32, device=dev)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        engine.solve_points_dev(**ins, x0=X0, out=out, stream=s.cuda_stream)
        s.synchronize()
        r = {k: v.cpu().numpy() for k, v in out.items()}
        r["status"] = r["status"].view(np.uint32)
        return r

    for n in (70, 1):
        r = run(n)
        for k in ALL:
            assert_same(r[k], gpu[k][:n], f"{k} (n = {n})")
    run(0)  # nothing to do, nothing written, no error


def test_three_rank_rehearsal_on_a_shared_device(pts, gpu, monkeypatch):
    monkeypatch.setenv("SBR_MULTI_SHARED_DEVICES", "1")
    m = sbr.Engine(n_gpus=3)
    try:
        assert m.n_gpus == 3
        r = m.solve_points(**pts, x0=X0)
    finally:
        m.close()
    for k in ALL:
        assert_same(r[k], gpu[k], k)
