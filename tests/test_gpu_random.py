"""Every kernel family on the seeded draws of tests/random_cases.py, on the GPU.

Parity: each family's calls through the host-pointer entry point and through the *_dev one, compared bit
for bit (NaN = NaN) with the CPU oracle on every output field, status, iters and fp_iters / rk_steps —
status words whole, learning bits included, as the families' own bitwise tests compare them.  The *_dev
calls carry the draw's invalid lanes (u < 0, NaN; in the econ planes a bad κ, p, λ): those end with the
SBR_ARG_INVALID sentinel of include/sbr.h, their wave neighbours with the oracle's bits.  Heterogeneity
runs once with the kernel specialised for its K and once with SBR_FLAG_HETERO_WIDE; the social grid under
the built-in schedule and forced through multi-point waves.

Neighbour independence (GPU against GPU): one drawn column's 65 u as drawn, sorted, reversed, under two
seeded permutations and with every second lane invalid, and eight of the points one per call: a point's
bits do not depend on the other lanes of its wave.  With the default options and SBR_FLAG_EXHAUSTIVE;
sbr_solve_points on its 130 points in drawn order and permuted.

A mismatch names the family, seed, call, column, lane and every parameter of the point (repr).

Wall times on the MI355X (pytest --durations=0, each family's oracle runs inside its parity test, once;
the module takes 28 s): sweep parity interest 8.0 s, hetero 2.4 s, baseline 0.3 s (+ 1.6 s engine
setup); social parity 4.8 s; econ parity interest_econ 1.5 s, hetero_econ 0.9 s, econ 0.03 s; points
parity 0.1 s; neighbour independence interest 3.7 s and 3.6 s (exhaustive), every other case <= 0.1 s."""
import ctypes

import numpy as np
import pytest

import random_cases as R
import sbr
from sbr import _lib
from sbr.engine import _dptr, _opts

pytestmark = pytest.mark.gpu

EXH = _lib.SBR_FLAG_EXHAUSTIVE


# ------------------------------------------------------------------------------------------------
# device-pointer plumbing
def _torch(engine):
    import torch

    return torch, torch.device("cuda", engine.device)


def _dev_in(engine, **arrays):
    torch, dev = _torch(engine)
    return {k: torch.tensor(np.ascontiguousarray(np.atleast_1d(v)), dtype=torch.float64, device=dev)
            for k, v in arrays.items()}


def _dev_out(engine, n, K=0, steps=0, fp=False, fields=R.FIELDS):
    torch, dev = _torch(engine)
    out = {k: torch.full((n,), -7.0, dtype=torch.float64, device=dev) for k in fields}
    out["status"] = torch.zeros(n, dtype=torch.int32, device=dev)
    out["iters"] = torch.full((n,), -7, dtype=torch.int32, device=dev)
    if K:
        out["tau_in_unc"] = torch.full((n * K,), -7.0, dtype=torch.float64, device=dev)
        out["tau_out_unc"] = torch.full((n * K,), -7.0, dtype=torch.float64, device=dev)
    if steps:
        out["rk_steps"] = torch.full((steps,), -7, dtype=torch.int64, device=dev)
    if fp:
        out["fp_iters"] = torch.full((n,), -7, dtype=torch.int32, device=dev)
    return out


def _dev_back(engine, out, shape, K=0, steps_shape=None):
    torch, dev = _torch(engine)
    torch.cuda.synchronize(dev)
    r = {}
    for k, v in out.items():
        a = v.cpu().numpy()
        if k == "status":
            a = a.view(np.uint32)
        if k.startswith("tau_") and K:
            r[k] = a.reshape(*shape, K)
        elif k == "rk_steps" and steps_shape is not None:
            r[k] = a.reshape(steps_shape)
        else:
            r[k] = a.reshape(shape)
    return r


# ------------------------------------------------------------------------------------------------
# one call of each family: host-pointer or device-pointer, on the u given
def run_baseline(engine, c, u, dev=False, flags=0):
    if not dev:
        grid = sbr.BaselineGrid(c["beta"], np.ascontiguousarray(u), c["eta"], c["t_end"], c["p"], c["kappa"], c["lam"],
                                c["x0"])
        return engine.sweep_baseline(grid, flags=flags)
    shape = (len(c["beta"]), len(u))
    out = _dev_out(engine, shape[0] * shape[1])
    engine.sweep_baseline_dev(**_dev_in(engine, beta=c["beta"], eta=c["eta"], t_end=c["t_end"], u=u), p=c["p"],
                              kappa=c["kappa"], lam=c["lam"], x0=c["x0"], out=out, flags=flags)
    return _dev_back(engine, out, shape)


def run_interest(engine, c, u, dev=False, flags=0):
    if not dev:
        return engine.sweep_interest(c["beta"], c["eta"], c["t_end"], u, c["p"], c["kappa"], c["lam"], c["r"], c["delta"],
                                     c["x0"], flags=flags)
    # Engine.sweep_interest_dev takes no flags: the C call, with sbr_opts.flags set
    shape = (len(c["beta"]), len(u))
    n = shape[0] * shape[1]
    out = _dev_out(engine, n, steps=n)
    ins = _dev_in(engine, beta=c["beta"], eta=c["eta"], t_end=c["t_end"], u=u)
    kind = {"status": "int32", "iters": "int32", "rk_steps": "int64"}
    P = {k: _dptr(v, k, kind.get(k, "float64"), n) for k, v in out.items()}
    soa = _lib.ResultSoA(*[P[k] for k in (*R.FIELDS, "status", "iters")])
    opts = _opts(early_exit_nan_run=0, bisect_max_iters=100, knot_capacity=65536, flags=flags)
    rc = engine._L.sbr_sweep_interest_dev(engine._ctx, None, _dptr(ins["beta"], "beta", "float64"),
                                          _dptr(ins["eta"], "eta", "float64", shape[0]),
                                          _dptr(ins["t_end"], "t_end", "float64", shape[0]), c["x0"],
                                          _dptr(ins["u"], "u", "float64"), shape[0], shape[1], c["p"], c["kappa"], c["lam"],
                                          c["r"], c["delta"], ctypes.byref(opts), ctypes.byref(soa), P["rk_steps"])
    _lib.check(rc, engine._ctx, "sbr_sweep_interest_dev")
    return _dev_back(engine, out, shape)


def run_hetero(engine, c, u, dev=False, flags=0, wide=False):
    if not dev:
        return engine.sweep_hetero(c["betas"], c["dist"], c["eta"], c["t_end"], u, c["p"], c["kappa"], c["lam"], c["x0"],
                                   exhaustive=bool(flags & EXH), wide=wide)
    # Engine.sweep_hetero_dev leaves the group buffers out: the C call, with them
    K, shape = c["K"], (len(c["eta"]), len(u))
    n = shape[0] * shape[1]
    out = _dev_out(engine, n, K=K, fields=("xi", "aw_max", "tol"))
    ins = _dev_in(engine, betas=c["betas"].reshape(-1), dist=c["dist"], eta=c["eta"], t_end=c["t_end"], u=u)
    P = {k: _dptr(v, k, "int32" if k in ("status", "iters") else "float64") for k, v in out.items()}
    soa = _lib.ResultSoA(P["xi"], None, None, P["aw_max"], P["tol"], P["status"], P["iters"])
    opts = _opts(knot_capacity=16384, flags=flags | (_lib.SBR_FLAG_HETERO_WIDE if wide else 0))
    rc = engine._L.sbr_sweep_hetero_dev(engine._ctx, None, K, _dptr(ins["betas"], "betas", "float64", shape[0] * K),
                                        _dptr(ins["dist"], "dist", "float64", K), _dptr(ins["eta"], "eta", "float64"),
                                        _dptr(ins["t_end"], "t_end", "float64", shape[0]), c["x0"],
                                        _dptr(ins["u"], "u", "float64"), shape[0], shape[1], c["p"], c["kappa"], c["lam"],
                                        ctypes.byref(opts), ctypes.byref(soa), P["tau_in_unc"], P["tau_out_unc"])
    _lib.check(rc, engine._ctx, "sbr_sweep_hetero_dev")
    return _dev_back(engine, out, shape, K=K)


def _econ_shape(c):
    rate = (len(c["r"]),) if c["family"] == "interest_econ" else ()
    return (len(c["eta"]), len(c["p"]), len(c["lam"]), *rate, len(c["kappa"]), len(c["u"]))


def run_econ(engine, c, dev=False, flags=0, wide=False):
    """sbr_sweep_econ / _interest_econ / _hetero_econ by the call's family."""
    f, shape = c["family"], _econ_shape(c)
    exh = bool(flags & EXH)
    ax = dict(u=c["u"], p=c["p"], kappa=c["kappa"], lam=c["lam"])
    if not dev:
        if f == "econ":
            return engine.sweep_econ(c["beta"], c["eta"], c["t_end"], **ax, x0=c["x0"], exhaustive=exh)
        if f == "interest_econ":
            return engine.sweep_interest_econ(c["beta"], c["eta"], c["t_end"], **ax, r=c["r"], delta=c["delta"],
                                              x0=c["x0"], exhaustive=exh)
        return engine.sweep_hetero_econ(c["betas"], c["dist"], c["eta"], c["t_end"], **ax, x0=c["x0"], exhaustive=exh,
                                        wide=wide)
    n = int(np.prod(shape))
    col = _dev_in(engine, eta=c["eta"], t_end=c["t_end"], **ax)
    if f == "econ":
        out = _dev_out(engine, n)
        engine.sweep_econ_dev(**_dev_in(engine, beta=c["beta"]), **col, x0=c["x0"], out=out, exhaustive=exh)
        return _dev_back(engine, out, shape)
    if f == "interest_econ":
        sshape = (*shape[:4], shape[5])
        out = _dev_out(engine, n, steps=int(np.prod(sshape)))
        engine.sweep_interest_econ_dev(**_dev_in(engine, beta=c["beta"], r=c["r"], delta=c["delta"]), **col, x0=c["x0"],
                                       out=out, exhaustive=exh)
        return _dev_back(engine, out, shape, steps_shape=sshape)
    out = _dev_out(engine, n, K=c["K"], fields=("xi", "aw_max", "tol"))
    engine.sweep_hetero_econ_dev(c["K"], **_dev_in(engine, betas=c["betas"].reshape(-1), dist=c["dist"]), **col,
                                 x0=c["x0"], out=out, exhaustive=exh, wide=wide)
    return _dev_back(engine, out, shape, K=c["K"])


def run_points(engine, c, args, dev=False, flags=0):
    if not dev:
        return engine.solve_points(**args, x0=c["x0"], flags=flags)
    n = len(args["u"])
    out = _dev_out(engine, n)
    engine.solve_points_dev(**_dev_in(engine, **args), x0=c["x0"], out=out, flags=flags)
    return _dev_back(engine, out, (n,))


def run_social(engine, c, dev=False):
    if not dev:
        return engine.sweep_social(c["beta"], c["eta"], c["u"], c["p"], c["kappa"], c["lam"], cmp=c["cmp"], x0=c["x0"],
                                   tol=c["tol"], max_iter=c["max_iter"])
    shape = (len(c["beta"]), len(c["u"]))
    n = shape[0] * shape[1]
    out = _dev_out(engine, n, fp=True)
    engine.sweep_social_dev(**_dev_in(engine, beta=c["beta"], eta=c["eta"], u=c["u"], cmp=c["cmp"]),
                            p=c["p"], kappa=c["kappa"], lam=c["lam"], x0=c["x0"], out=out, tol=c["tol"],
                            max_iter=c["max_iter"])
    return _dev_back(engine, out, shape)


SWEEP = {"baseline": (run_baseline, R.ALL), "interest": (run_interest, (*R.ALL, "rk_steps")),
         "hetero": (run_hetero, R.HFIELDS)}
ECON_FIELDS = {"econ": R.ALL, "interest_econ": (*R.ALL, "rk_steps"), "hetero_econ": R.HFIELDS}


# ------------------------------------------------------------------------------------------------
# parity with the oracle
@pytest.mark.parametrize("family", list(SWEEP))
def test_sweep_parity(engine, oracle, family):
    run, fields = SWEEP[family]
    calls, refs = R.reference(oracle, family)
    for c, ref in zip(calls, refs):
        variants = [dict(wide=False), dict(wide=True)] if family == "hetero" else [{}]
        for kw in variants:
            R.assert_equal(run(engine, c, c["u"], **kw), ref, c, f"host {kw}", fields)
            want = R.expected_dev(ref, R.lane_mask(c, ref["status"].shape))
            R.assert_equal(run(engine, c, c["u_bad"], dev=True, **kw), want, c, f"device {kw}", fields, u=c["u_bad"])


def test_the_193_column_call_is_chunked(engine, oracle):
    """64·kSweepChunks + 1 columns reach run_baseline's chunked schedule (a timed sweep records one
    learning end and one equilibrium end per chunk): if the constant grows, the call stays below the
    threshold, no timeline is recorded and the draw's shape has to grow with it.  On a context of its own,
    which holds no timeline of an earlier sweep."""
    calls, refs = R.reference(oracle, "baseline")
    i = [c["name"] for c in calls].index("chunked193")
    c, ref = calls[i], refs[i]
    assert len(c["beta"]) == 193
    own = sbr.Engine(engine.device)
    try:
        own.timing_enable(True)
        assert own.chunk_timeline() == []
        g = run_baseline(own, c, c["u"])
        chunks = own.chunk_timeline()
    finally:
        own.close()
    assert len(chunks) == 3 and all(0.0 <= a <= b for a, b in chunks), chunks
    R.assert_equal(g, ref, c, "host, timed", R.ALL)


@pytest.mark.parametrize("family", list(ECON_FIELDS))
def test_econ_parity(engine, oracle, family):
    fields = ECON_FIELDS[family]
    calls, refs = R.reference(oracle, family)
    for c, ref in zip(calls, refs):
        variants = [dict(wide=False), dict(wide=True)] if family == "hetero_econ" else [{}]
        for kw in variants:
            R.assert_equal(run_econ(engine, c, **kw), ref, c, f"host {kw}", fields)
            R.assert_equal(run_econ(engine, c, dev=True, **kw), ref, c, f"device {kw}", fields)
        for q, mask in R.spoil_axes(c):
            rk = None
            if family == "interest_econ":  # rk_steps has no κ axis: 0 where u, p or λ is at fault
                rk = np.zeros(ref["rk_steps"].shape, bool)
                for k, axis in (("u", 4), ("p", 1), ("lam", 2)):
                    for i in np.flatnonzero(~((q[k] == c[k]))):
                        idx = [slice(None)] * 5
                        idx[axis] = i
                        rk[tuple(idx)] = True
            R.assert_equal(run_econ(engine, q, dev=True), R.expected_dev(ref, mask, rk), q, "device, bad axis elements",
                           fields)


def test_points_parity(engine, oracle):
    (c,), (ref,) = R.reference(oracle, "points")
    R.assert_equal(run_points(engine, c, c["args"]), ref, c, "host", R.ALL)
    want = R.expected_dev(ref, R.lane_mask(c, (130,)))
    R.assert_equal(run_points(engine, c, c["args_bad"]), want, c, "host, bad lanes", R.ALL, args=c["args_bad"])
    R.assert_equal(run_points(engine, c, c["args_bad"], dev=True), want, c, "device, bad lanes", R.ALL,
                   args=c["args_bad"])


def test_social_parity(engine, oracle):
    (c,), (ref,) = R.reference(oracle, "social")
    fields = (*R.ALL, "fp_iters")
    total = int(ref["fp_iters"].sum())
    g = run_social(engine, c)
    assert engine.social_schedule_stats()[0] == 0  # the built-in schedule: every point a whole wave
    R.assert_equal(g, ref, c, "host, built-in schedule", fields)
    R.assert_equal(run_social(engine, c, dev=True), ref, c, "device", fields)
    with engine.social_schedule(0, 1, -1):  # multi-point waves, as tests/test_gpu_social_bulk.py forces them
        b = run_social(engine, c)
        stats = engine.social_schedule_stats()
    assert stats[0] > 0 and stats[0] + stats[1] >= total, (stats, total)
    R.assert_equal(b, ref, c, "host, multi-point waves", fields)
    R.assert_equal(b, g, c, "multi-point waves against the built-in schedule", (*fields, "rk_steps"))


# ------------------------------------------------------------------------------------------------
# neighbour independence
def _layouts(u):
    n = len(u)
    rng = np.random.default_rng(len(u))
    every_second = np.arange(n)
    return [("sorted", np.argsort(u, kind="stable"), None), ("reversed", np.arange(n)[::-1], None),
            ("permutation 1", rng.permutation(n), None), ("permutation 2", rng.permutation(n), None),
            ("every second lane invalid", every_second, every_second[1::2])]


def _one_column(c, col):
    q = dict(c, name=f"{c['name']}[column {col}]")
    for k in ("beta", "eta", "t_end", "betas"):
        if k in c:
            q[k] = np.ascontiguousarray(c[k][col:col + 1])
    return q


# the column of each family's first 65-u call with the most outcome classes among its lanes is found
# from the GPU's own result: no oracle is needed here
@pytest.mark.parametrize("flags", [0, EXH], ids=["default", "exhaustive"])
@pytest.mark.parametrize("family", list(SWEEP))
def test_neighbour_independence(engine, family, flags):
    run, fields = SWEEP[family]
    c0 = R.calls_of(family)[0]
    full = run(engine, c0, c0["u"], flags=flags)
    kinds = [len(set(R.class_of(row).tolist())) for row in full["status"]]
    col = int(np.argmax(kinds))
    c = _one_column(c0, col)
    u, n = c["u"], len(c["u"])
    base = run(engine, c, u, flags=flags)
    R.assert_equal(base, {k: full[k][col:col + 1] for k in fields}, c, "one column against its call", fields)
    for what, perm, bad in _layouts(u):
        v = u[perm].copy()
        keep = np.ones(n, bool)
        if bad is not None:
            v[bad] = np.where(np.arange(len(bad)) % 2 == 0, -1.0, np.nan)
            keep[bad] = False
        g = run(engine, c, v, dev=bad is not None, flags=flags)
        got = {k: g[k][:, keep] for k in fields}
        want = {k: base[k][:, perm][:, keep] for k in fields}
        R.assert_equal(got, want, c, f"layout {what}", fields, u=v[keep])
        if bad is not None:
            assert (g["status"][:, bad] == R.ARG_INVALID).all() and (g["iters"][:, bad] == 0).all()
    for j in np.linspace(0, n - 1, 8).astype(int):
        g = run(engine, c, u[j:j + 1], flags=flags)
        R.assert_equal(g, {k: base[k][:, j:j + 1] for k in fields}, c, f"lane {j} alone (n_u = 1)", fields, u=u[j:j + 1])


@pytest.mark.parametrize("flags", [0, EXH], ids=["default", "exhaustive"])
def test_neighbour_independence_econ(engine, flags):
    c = R.econ()[0]
    base = run_econ(engine, c, flags=flags)
    n = len(c["u"])
    for what, perm, bad in _layouts(c["u"]):
        q = dict(c, u=c["u"][perm].copy())
        keep = np.ones(n, bool)
        if bad is not None:
            q["u"][bad] = np.where(np.arange(len(bad)) % 2 == 0, -1.0, np.nan)
            keep[bad] = False
        g = run_econ(engine, q, dev=bad is not None, flags=flags)
        got = {k: g[k][..., keep] for k in R.ALL}
        want = {k: base[k][..., perm][..., keep] for k in R.ALL}
        R.assert_equal(got, want, dict(q, u=q["u"][keep]), f"layout {what}", R.ALL)
    kperm = np.random.default_rng(13).permutation(len(c["kappa"]))
    g = run_econ(engine, dict(c, kappa=c["kappa"][kperm]), flags=flags)
    R.assert_equal(g, {k: base[k][:, :, :, kperm] for k in R.ALL}, dict(c, kappa=c["kappa"][kperm]), "κ permuted", R.ALL)
    for j in range(n):  # every u alone: the 13-point plane of one u
        q = dict(c, u=c["u"][j:j + 1])
        R.assert_equal(run_econ(engine, q, flags=flags), {k: base[k][..., j:j + 1] for k in R.ALL}, q, f"u[{j}] alone", R.ALL)


@pytest.mark.parametrize("flags", [0, EXH], ids=["default", "exhaustive"])
def test_neighbour_independence_points(engine, flags):
    c = R.points()
    base = run_points(engine, c, c["args"], flags=flags)
    rng = np.random.default_rng(130)
    for what, perm in (("permutation 1", rng.permutation(130)), ("reversed", np.arange(130)[::-1])):
        args = {k: np.ascontiguousarray(v[perm]) for k, v in c["args"].items()}
        g = run_points(engine, c, args, flags=flags)
        R.assert_equal(g, {k: base[k][perm] for k in R.ALL}, c, f"list {what}", R.ALL, args=args)
    for j in np.linspace(0, 129, 8).astype(int):
        args = {k: v[j:j + 1] for k, v in c["args"].items()}
        R.assert_equal(run_points(engine, c, args, flags=flags), {k: base[k][j:j + 1] for k in R.ALL}, c,
                       f"point {j} alone", R.ALL, args=args)
