"""sbr_sweep_econ without a GPU: the three entry points are declared in include/sbr.h and exported
by libsbr with ctypes signatures, a null context is refused before any device work, and
sbr.comparative_statics hands over the model's own resolved η and tspan around the swept axes."""
import ctypes

import numpy as np
import pytest

import sbr
from sbr import _lib

SYMBOLS = ("sbr_sweep_econ", "sbr_sweep_econ_dev", "sbr_set_econ_workspace")


def test_econ_symbols_declared_and_exported():
    syms = sbr.header_symbols()
    L = sbr.load()
    for s in SYMBOLS:
        assert s in syms, f"{s} is not declared in include/sbr.h"
        assert hasattr(L, s), f"libsbr.so does not export {s}"
        assert s in _lib._SIGS, f"{s} has no ctypes signature"


def test_null_context_is_an_argument_error():
    L = sbr.load()
    a = np.full(2, 0.5)
    P = a.ctypes.data_as(ctypes.c_void_p)
    soa = _lib.ResultSoA()
    opts = _lib.default_opts()
    assert L.sbr_sweep_econ(None, P, P, P, 1e-4, P, 2, 2, P, 2, P, 2, P, 2, ctypes.byref(opts),
                            ctypes.byref(soa)) == _lib.SBR_EARG
    assert L.sbr_sweep_econ_dev(None, None, P, P, P, 1e-4, P, 2, 2, P, 2, P, 2, P, 2, ctypes.byref(opts),
                                ctypes.byref(soa)) == _lib.SBR_EARG
    assert L.sbr_set_econ_workspace(None, 0) == _lib.SBR_EARG


def test_comparative_statics_rejects_an_unknown_axis():
    m = sbr.ModelParameters.make()
    for bad in ({"eta": [1.0, 2.0]}, {"beta": [1.0]}, {"lambda_": [0.1]}, {"u": [0.1], "kapa": [0.3]}):
        with pytest.raises(sbr.ArgumentError):
            sbr.econ_from_model(m, **bad)
        with pytest.raises(sbr.ArgumentError):  # before any engine is looked for
            sbr.comparative_statics(m, None, **bad)


def test_comparative_statics_keeps_resolved_eta_and_tspan():
    base = sbr.ModelParameters.make()                      # η = 15, tspan = (0, 30)
    fresh = sbr.ModelParameters.make(beta=3.0)             # η = η_bar / β = 5, tspan = (0, 10)
    bis = sbr.ModelParameters.modify(base, beta=3.0)       # copy-modify: η = 15, tspan = (0, 30) carried over
    ter = sbr.ModelParameters.modify(base, u=0.01, p=0.9, kappa=0.3, lam=0.2)
    kap = [0.3, 0.6]
    for m, beta, eta, t_end in ((base, 1.0, 15.0, 30.0), (fresh, 3.0, 5.0, 10.0), (bis, 3.0, 15.0, 30.0)):
        a = sbr.econ_from_model(m, kappa=kap, u=np.linspace(0, 1, 5))
        assert set(a) == {"beta", "eta", "t_end", "u", "p", "kappa", "lam", "x0"}
        assert (a["beta"], a["eta"], a["t_end"], a["x0"]) == (beta, eta, t_end, 1e-4)
        assert a["eta"] == m.economic.eta and a["t_end"] == m.learning.tspan[1]
        assert (a["p"], a["lam"]) == (0.5, 0.01) and a["kappa"] is kap
        # what Engine.sweep_econ passes to the C call
        ax = sbr.econ_axes(**{k: v for k, v in a.items() if k != "x0"})
        for k, want in (("beta", [beta]), ("eta", [eta]), ("t_end", [t_end]), ("p", [0.5]), ("lam", [0.01]),
                        ("kappa", kap), ("u", [0, .25, .5, .75, 1.0])):
            assert ax[k].dtype == np.float64 and ax[k].flags["C_CONTIGUOUS"] and ax[k].tolist() == want, k
    a = sbr.econ_from_model(ter, lam=[0.1, 0.2, 0.3])
    assert (a["u"], a["p"], a["kappa"]) == (0.01, 0.9, 0.3) and a["lam"] == [0.1, 0.2, 0.3]
    with pytest.raises(sbr.ArgumentError):
        sbr.econ_axes([1.0, 2.0], [15.0, 15.0, 15.0], 30.0, 0.1, 0.5, 0.6, 0.01)
    with pytest.raises(sbr.ArgumentError):
        sbr.econ_axes(1.0, 15.0, 30.0, np.zeros((2, 2)), 0.5, 0.6, 0.01)
