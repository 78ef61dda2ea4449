"""sbr_solve_points without a GPU: the three entry points are declared in include/sbr.h and
exported by libsbr, a null context is refused before any device work, and
sbr.points_from_models hands over each model's own resolved η and tspan."""
import ctypes

import numpy as np
import pytest

import sbr
from sbr import _lib

SYMBOLS = ("sbr_solve_points", "sbr_solve_points_dev", "sbr_set_points_workspace")


def test_points_symbols_declared_and_exported():
    syms = sbr.header_symbols()
    L = sbr.load()
    for s in SYMBOLS:
        assert s in syms, f"{s} is not declared in include/sbr.h"
        assert hasattr(L, s), f"libsbr.so does not export {s}"
        assert s in _lib._SIGS, f"{s} has no ctypes signature"


def test_null_context_is_an_argument_error():
    L = sbr.load()
    a = np.ones(2)
    P = a.ctypes.data_as(ctypes.c_void_p)
    soa = _lib.ResultSoA()
    opts = _lib.default_opts()
    assert L.sbr_solve_points(None, P, P, P, 1e-4, P, P, P, P, 2, ctypes.byref(opts), ctypes.byref(soa)) == _lib.SBR_EARG
    assert L.sbr_solve_points_dev(None, None, P, P, P, 1e-4, P, P, P, P, 2, ctypes.byref(opts),
                                  ctypes.byref(soa)) == _lib.SBR_EARG
    assert L.sbr_set_points_workspace(None, 0) == _lib.SBR_EARG


def test_points_from_models_keeps_resolved_eta_and_tspan():
    base = sbr.ModelParameters.make()                      # η = 15, tspan = (0, 30)
    fresh = sbr.ModelParameters.make(beta=3.0)             # η = η_bar / β = 5, tspan = (0, 10)
    bis = sbr.ModelParameters.modify(base, beta=3.0)       # copy-modify: η = 15, tspan = (0, 30) carried over
    ter = sbr.ModelParameters.modify(base, u=0.01, p=0.9, kappa=0.3, lam=0.2)
    a = sbr.points_from_models([base, fresh, bis, ter])
    assert set(a) == {"beta", "u", "eta", "t_end", "p", "kappa", "lam", "x0"}
    for k in ("beta", "u", "eta", "t_end", "p", "kappa", "lam"):
        assert a[k].dtype == np.float64 and a[k].shape == (4,), k
    assert a["beta"].tolist() == [1.0, 3.0, 3.0, 1.0]
    assert a["eta"].tolist() == [15.0, 5.0, 15.0, 15.0]
    assert a["t_end"].tolist() == [30.0, 10.0, 30.0, 30.0]
    assert a["u"].tolist() == [0.1, 0.1, 0.1, 0.01]
    assert a["p"].tolist() == [0.5, 0.5, 0.5, 0.9]
    assert a["kappa"].tolist() == [0.6, 0.6, 0.6, 0.3]
    assert a["lam"].tolist() == [0.01, 0.01, 0.01, 0.2]
    assert a["x0"] == 1e-4
    for m, e, t in zip((base, fresh, bis, ter), a["eta"], a["t_end"]):
        assert e == m.economic.eta and t == m.learning.tspan[1]


def test_points_from_models_refuses_mixed_x0():
    base = sbr.ModelParameters.make()
    other = sbr.ModelParameters.modify(base, x0=1e-3)
    with pytest.raises(sbr.ArgumentError):
        sbr.points_from_models([base, other])
    assert sbr.points_from_models([other, other])["x0"] == 1e-3
