"""The integrator options off their defaults, without a GPU: the oracle that tests/test_gpu_ode_opts.py
compares the device with still solves the ODE at loose tolerances (its stiff branch included), tells
rtol from atol, and the Engine keywords ode_rtol / ode_atol / ode_maxiters land in the sbr_opts
fields of the same meaning on every entry point."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import sbr
from sbr import _lib
from sbr import engine as engine_mod

X0 = 1e-4
BETAS = (0.5, 1.0, 3.0, 61.654026637430945, 1e4)


@pytest.mark.parametrize("tol", [1e-10, 1e-6, 1e-3])
def test_oracle_loose_tolerance_solves_the_logistic_ode(oracle, tol):
    """max |G − closed form| ≤ 100·tol on every knot, G(t) = 1 / (1 + (1 − x0)/x0 · e^{−βt}).

    Measured max error / tol (β = 0.5, 1, 3, 61.65, 1e4; the last three hand over to Rosenbrock23):
      tol 1e-10:  7.08   7.14   7.43  10.38  17.63
      tol 1e-6:   5.81   6.05   7.74  33.49  33.49
      tol 1e-3:   2.36   2.27   2.53   2.53   2.53
    The bound of 100 leaves a factor of 3 over the largest for the libm of another host."""
    stiff = []
    for beta in BETAS:
        t, G, st = oracle.learn_logistic(beta, 30.0, rtol=tol, atol=tol)
        exact = 1.0 / (1.0 + ((1.0 - X0) / X0) * np.exp(-beta * t))
        err = np.abs(G - exact).max()
        print(f"tol {tol:g} β {beta:g}: {len(t)} knots, max error {err / tol:.2f} tol, nswitch {st['nswitch']}")
        assert err <= 100.0 * tol, (beta, err / tol)
        assert t[-1] == 30.0 and st["status"] & ~sbr.STATUS["SBR_STIFF_SWITCH"] == 0
        stiff.append(st["nswitch"] > 0)
    assert stiff == [False, False, True, True, True]  # the stiff branch is part of what is checked


def test_oracle_tells_rtol_from_atol(oracle):
    """(rtol, atol) = (1e-6, 1e-12) and (1e-12, 1e-6) give different knots on every column, so a
    device that swapped the two cannot equal the oracle at the unequal option set."""
    for beta in BETAS:
        t, G, _ = oracle.learn_logistic(beta, 30.0, rtol=1e-6, atol=1e-12)
        ts, Gs, _ = oracle.learn_logistic(beta, 30.0, rtol=1e-12, atol=1e-6)
        assert len(t) != len(ts) or not np.array_equal(t, ts), beta
    a = oracle.sweep_baseline(BETAS, 15.0, 30.0, [0.05, 0.3], 0.5, 0.6, 0.01, rtol=1e-6, atol=1e-12)
    b = oracle.sweep_baseline(BETAS, 15.0, 30.0, [0.05, 0.3], 0.5, 0.6, 0.01, rtol=1e-12, atol=1e-6)
    assert (a["n_knots"] != b["n_knots"]).all()


def test_oracle_options_are_per_call(oracle):
    """No process-wide setter: a loose call between two default calls leaves them bit-identical."""
    args = ([1.0, 3.0], 15.0, 30.0, [0.05, 0.3], 0.5, 0.6, 0.01)
    a = oracle.sweep_baseline(*args)
    loose = oracle.sweep_baseline(*args, rtol=1e-3, atol=1e-3, ode_maxiters=20)
    b = oracle.sweep_baseline(*args)
    assert (loose["n_knots"] < a["n_knots"]).all()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---------------------------------------------------------------------------- Engine keywords
class _RecordingLib:
    """Stands in for libsbr: every entry point returns SBR_OK and records the sbr_opts it was
    handed (the ctypes.byref argument that wraps an Opts)."""

    def __init__(self):
        self.seen = []

    def __getattr__(self, name):
        def call(*args):
            for a in args:
                o = getattr(a, "_obj", None)
                if isinstance(o, _lib.Opts):
                    self.seen.append((name, o.ode_reltol, o.ode_abstol, o.ode_maxiters))
            return 0

        return call


@pytest.fixture()
def recording_engine(monkeypatch):
    """An Engine with no device behind it: the wrappers run up to the C call and past it."""
    eng = sbr.Engine.__new__(sbr.Engine)
    eng._ctx, eng._L, eng._knot_opts, eng._multi, eng.device = None, _RecordingLib(), {}, False, 0
    # the *_dev wrappers take CUDA tensors; here they get CPU tensors and null pointers
    monkeypatch.setattr(engine_mod, "_dptr", lambda *a, **k: None)
    monkeypatch.setattr(engine_mod, "_out_ptrs", lambda out, fields, n, required=(): [None] * len(fields))
    return eng


def _calls(eng, torch):
    """name -> a call of every wrapper the options were added to, taking the ODE keywords."""
    grid = sbr.BaselineGrid([1.0, 2.0], [0.1, 0.2, 0.3], 15.0, 30.0)
    one = torch.zeros(2, dtype=torch.float64)
    two = torch.zeros((3, 2), dtype=torch.float64)
    het = torch.zeros((3, 2, 4), dtype=torch.float64)
    dist = [0.25] * 4
    bk = [[0.25, 0.5, 1.0, 2.0]]
    e = (0.5, 0.6, 0.01)
    return {
        "sweep_baseline": lambda **k: eng.sweep_baseline(grid, **k),
        "sweep_baseline_dev": lambda **k: eng.sweep_baseline_dev(one, one, one, one, *e, 1e-4, {}, **k),
        "sweep_baseline_batch_dev": lambda **k: eng.sweep_baseline_batch_dev(two, two, two, one, *e, 1e-4, {}, **k),
        "solve_points": lambda **k: eng.solve_points([1.0, 2.0], 0.1, 15.0, 30.0, *e, **k),
        "solve_points_dev": lambda **k: eng.solve_points_dev(one, one, one, one, one, one, one, 1e-4, {}, **k),
        "solve_point_paths": lambda **k: eng.solve_point_paths(1.0, 15.0, 30.0, 0.1, *e, cap=64, **k),
        "sweep_interest": lambda **k: eng.sweep_interest([1.0], 15.0, 30.0, [0.1], *e, 0.06, 0.1, **k),
        "sweep_interest_dev": lambda **k: eng.sweep_interest_dev(one, one, one, one, *e, 0.06, 0.1, 1e-4, {}, **k),
        "interest_point_paths": lambda **k: eng.interest_point_paths(1.0, 15.0, 30.0, 0.1, *e, 0.06, 0.1, cap=64,
                                                                     **k),
        "sweep_hetero": lambda **k: eng.sweep_hetero(bk, dist, 15.0, 30.0, [0.1], *e, **k),
        "sweep_hetero_dev": lambda **k: eng.sweep_hetero_dev(4, het[0], one, one, one, one, *e, 1e-4, {}, **k),
        "sweep_hetero_batch_dev": lambda **k: eng.sweep_hetero_batch_dev(4, het, one, two, two, one, *e, 1e-4, {},
                                                                         **k),
        "learn_hetero": lambda **k: eng.learn_hetero(bk, dist, 30.0, cap=64, **k),
        "hetero_point_paths": lambda **k: eng.hetero_point_paths(bk[0], dist, 15.0, 30.0, 0.1, *e, cap=64, **k),
        "sweep_social": lambda **k: eng.sweep_social([1.0], 15.0, [0.1], *e, **k),
        "sweep_social_dev": lambda **k: eng.sweep_social_dev(one, one, one, *e, two, 1e-4, {}, **k),
        "social_point_paths": lambda **k: eng.social_point_paths(1.0, 15.0, 0.1, *e, cap=64, **k),
    }


def test_engine_keywords_reach_sbr_opts(recording_engine):
    torch = pytest.importorskip("torch")
    eng = recording_engine
    d = _lib.default_opts()
    default = (d.ode_reltol, d.ode_abstol, d.ode_maxiters)
    for name, call in _calls(eng, torch).items():
        sig = inspect.signature(getattr(sbr.Engine, name)).parameters
        assert all(sig[k].default is None for k in ("ode_rtol", "ode_atol", "ode_maxiters")), name
        eng._L.seen.clear()
        call()
        assert [s[1:] for s in eng._L.seen] == [default], (name, eng._L.seen)
        eng._L.seen.clear()
        # three different values: a wrapper that crossed two of them is caught
        call(ode_rtol=1e-5, ode_atol=1e-9, ode_maxiters=77)
        assert [s[1:] for s in eng._L.seen] == [(1e-5, 1e-9, 77)], (name, eng._L.seen)
        eng._L.seen.clear()
        call(ode_atol=1e-9)
        assert [s[1:] for s in eng._L.seen] == [(default[0], 1e-9, default[2])], (name, eng._L.seen)
    # learn_baseline keeps tol (reltol = abstol = tol) and gains the cap
    eng._L.seen.clear()
    eng.learn_baseline([1.0], 15.0, 30.0, cap=64)
    eng.learn_baseline([1.0], 15.0, 30.0, cap=64, tol=1e-7, ode_maxiters=5)
    eng.learn_baseline([1.0], 15.0, 30.0, cap=64, ode_maxiters=9)
    assert [s[1:] for s in eng._L.seen] == [default, (1e-7, 1e-7, 5), (default[0], default[1], 9)]


def test_opts_struct_matches_the_header():
    """The three fields lead sbr_opts in the header's order and types (include/sbr.h)."""
    f = _lib.Opts._fields_[:3]
    assert [n for n, _ in f] == ["ode_reltol", "ode_abstol", "ode_maxiters"]
    assert [t for _, t in f] == [ctypes.c_double, ctypes.c_double, ctypes.c_int64]
    src = _lib.HEADER.read_text()
    body = src[:src.index("} sbr_opts;")]
    body = body[body.rindex("typedef struct {"):]
    fields = re.findall(r"^\s*(double|int64_t|int32_t)\s+(\w+);", body, re.M)
    assert fields[:3] == [("double", "ode_reltol"), ("double", "ode_abstol"), ("int64_t", "ode_maxiters")]
    assert [n for _, n in fields] == [n for n, _ in _lib.Opts._fields_]
