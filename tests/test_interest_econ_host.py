"""sbr_sweep_interest_econ without a GPU: both entry points are declared in include/sbr.h and
exported by libsbr with ctypes signatures, a null context is refused before any device work, and
the Python axis checks hold (r and δ are pairs of one length, every axis one-dimensional)."""
import ctypes

import numpy as np
import pytest

import sbr
from sbr import _lib

SYMBOLS = ("sbr_sweep_interest_econ", "sbr_sweep_interest_econ_dev")


def test_interest_econ_symbols_declared_and_exported():
    syms = sbr.header_symbols()
    L = sbr.load()
    for s in SYMBOLS:
        assert s in syms, f"{s} is not declared in include/sbr.h"
        assert hasattr(L, s), f"libsbr.so does not export {s}"
        assert s in _lib._SIGS, f"{s} has no ctypes signature"


def test_null_context_is_an_argument_error():
    L = sbr.load()
    a = np.full(2, 0.5)
    d = np.full(2, 0.7)
    P, D = a.ctypes.data_as(ctypes.c_void_p), d.ctypes.data_as(ctypes.c_void_p)
    soa = _lib.ResultSoA()
    opts = _lib.default_opts()
    assert L.sbr_sweep_interest_econ(None, P, P, P, 1e-4, P, 2, 2, P, 2, P, 2, P, D, 2, P, 2, ctypes.byref(opts),
                                     ctypes.byref(soa), None) == _lib.SBR_EARG
    assert L.sbr_sweep_interest_econ_dev(None, None, P, P, P, 1e-4, P, 2, 2, P, 2, P, 2, P, D, 2, P, 2,
                                         ctypes.byref(opts), ctypes.byref(soa), None) == _lib.SBR_EARG


def test_axis_checks():
    ax = sbr.interest_econ_axes([1.0, 3.0], 15.0, 30.0, [0.0, 0.1, 0.2], 0.5, [0.3, 0.6], 0.01, [0.0, 0.06], [0.1, 0.1])
    assert {k: v.tolist() for k, v in ax.items()} == dict(
        beta=[1.0, 3.0], eta=[15.0, 15.0], t_end=[30.0, 30.0], u=[0.0, 0.1, 0.2], p=[0.5], kappa=[0.3, 0.6],
        lam=[0.01], r=[0.0, 0.06], delta=[0.1, 0.1])
    assert all(v.dtype == np.float64 and v.flags["C_CONTIGUOUS"] and v.ndim == 1 for v in ax.values())
    # scalars are one pair
    ax = sbr.interest_econ_axes(1.0, 15.0, 30.0, 0.1, 0.5, 0.6, 0.01, 0.06, 0.1)
    assert (ax["r"].tolist(), ax["delta"].tolist()) == ([0.06], [0.1])
    with pytest.raises(sbr.ArgumentError):  # r and δ of unequal length
        sbr.interest_econ_axes(1.0, 15.0, 30.0, 0.1, 0.5, 0.6, 0.01, [0.0, 0.06], [0.1])
    with pytest.raises(sbr.ArgumentError):
        sbr.interest_econ_axes(1.0, 15.0, 30.0, 0.1, 0.5, 0.6, 0.01, 0.06, [0.1, 0.5])
    for bad in (dict(r=np.zeros((2, 2)), delta=np.ones((2, 2))), dict(u=np.zeros((2, 2))), dict(kappa=[[0.3], [0.6]])):
        args = dict(beta=1.0, eta=15.0, t_end=30.0, u=0.1, p=0.5, kappa=0.6, lam=0.01, r=0.06, delta=0.1)
        with pytest.raises(sbr.ArgumentError):  # a 2-D axis
            sbr.interest_econ_axes(**{**args, **bad})
