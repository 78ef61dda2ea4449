"""sbr_sweep_hetero_econ without a GPU: the two entry points and the slab setter are declared in
include/sbr.h and exported by libsbr with ctypes signatures, the SBREngine.jl wrapper's ccall has the
header's arity, a null context is refused before any device work, oracle_hetero_econ stacks in the
documented index order, and — the property the design rests on — the oracle's group buffers and
knot counts do not depend on κ."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import sbr
from hetero_econ_cases import H3_COUNTS, KAPPA3, LAM2, P2, U12, counts, h3_oracle, same, shape_of
from sbr import _lib

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "sbr.h"
ENGINE_JL = REPO / "replication-social-bank-runs_amd" / "julia" / "SBREngine.jl"
SYMBOLS = ("sbr_sweep_hetero_econ", "sbr_sweep_hetero_econ_dev", "sbr_set_hetero_econ_slab")


def _arity(sym: str) -> int:
    src = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(r"\bint\s+" + sym + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{sym} is not declared in include/sbr.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_symbols_declared_and_exported():
    syms = sbr.header_symbols()
    L = sbr.load()
    for s in SYMBOLS:
        assert s in syms, f"{s} is not declared in include/sbr.h"
        assert hasattr(L, s), f"libsbr.so does not export {s}"
        assert s in _lib._SIGS, f"{s} has no ctypes signature"
        assert len(_lib._SIGS[s][1]) == _arity(s), s
    assert (_arity(SYMBOLS[0]), _arity(SYMBOLS[1]), _arity(SYMBOLS[2])) == (20, 21, 2)


def test_julia_wrapper_ccall_arity_matches_the_header():
    src = ENGINE_JL.read_text()
    m = re.search(r"ccall\(\(:sbr_sweep_hetero_econ, libsbr\),\s*Cint,\s*\(", src)
    assert m, "SBREngine.jl has no ccall of sbr_sweep_hetero_econ"
    i, depth = m.end(), 1
    while depth:
        depth += {"(": 1, ")": -1}.get(src[i], 0)
        i += 1
    types = [t for t in re.split(r",(?![^{]*\})", src[m.end():i - 1]) if t.strip()]
    assert len(types) == _arity("sbr_sweep_hetero_econ")
    # … and as many values as types
    j, depth = i, 1
    k = src.index(",", i) + 1
    while depth:
        depth += {"(": 1, ")": -1}.get(src[j], 0)
        j += 1
    values = [v for v in src[k:j - 1].split(",") if v.strip()]
    assert len(values) == len(types)
    assert "function sweep_hetero_econ(" in src


def test_null_context_is_an_argument_error():
    L = sbr.load()
    a = np.full(4, 0.5)
    P = a.ctypes.data_as(ctypes.c_void_p)
    soa = _lib.ResultSoA()
    opts = _lib.default_opts()
    assert L.sbr_sweep_hetero_econ(None, 2, P, P, P, P, 1e-4, P, 2, 2, P, 2, P, 2, P, 2, ctypes.byref(opts),
                                   ctypes.byref(soa), None, None) == _lib.SBR_EARG
    assert L.sbr_sweep_hetero_econ_dev(None, None, 2, P, P, P, P, 1e-4, P, 2, 2, P, 2, P, 2, P, 2, ctypes.byref(opts),
                                       ctypes.byref(soa), None, None) == _lib.SBR_EARG
    assert L.sbr_set_hetero_econ_slab(None, 0) == _lib.SBR_EARG


def test_axis_checks():
    ax = sbr.hetero_econ_axes(3, [5.0, 6.0, 7.0], 30.0, [0.0, 0.1], 0.9, [0.3, 0.6], 0.1)
    assert {k: v.tolist() for k, v in ax.items()} == dict(eta=[5.0, 6.0, 7.0], t_end=[30.0] * 3, u=[0.0, 0.1], p=[0.9],
                                                          kappa=[0.3, 0.6], lam=[0.1])
    assert all(v.dtype == np.float64 and v.flags["C_CONTIGUOUS"] and v.ndim == 1 for v in ax.values())
    with pytest.raises(sbr.ArgumentError):
        sbr.hetero_econ_axes(3, [5.0, 6.0], 30.0, 0.1, 0.9, 0.3, 0.1)
    with pytest.raises(sbr.ArgumentError):
        sbr.hetero_econ_axes(3, 5.0, 30.0, 0.1, 0.9, np.zeros((2, 2)), 0.1)


def test_oracle_stack_index_order(oracle):
    g, ref = h3_oracle(2)
    assert shape_of(g) == (3, 2, 2, 3, 12) and counts(ref["status"]) == H3_COUNTS[2]
    # element (c, a, b, k, j) by hand: column 2, p[1], λ[0], κ[1], u[4] (every index differs from its
    # neighbours', and the point is a run)
    c, a, b, k, j = 2, 1, 0, 1, 4
    one = oracle.sweep_hetero(g["betas"][c:c + 1], g["dist"], g["eta"][c:c + 1], g["t_end"][c:c + 1], U12[j:j + 1],
                              float(P2[a]), float(KAPPA3[k]), float(LAM2[b]), g["x0"])
    for f in ("xi", "aw_max", "tol", "status", "iters"):
        assert same(ref[f][c, a, b, k, j], one[f][0, 0]).all(), f
        # the flat offset the C layout documents
        flat = (((c * 2 + a) * 2 + b) * 3 + k) * 12 + j
        assert same(ref[f].reshape(-1)[flat], one[f][0, 0]).all(), f
    for f in ("tau_in_unc", "tau_out_unc"):
        assert same(ref[f][c, a, b, k, j], one[f][0, 0]).all(), f
        assert same(ref[f].reshape(-1, 2)[flat], one[f][0, 0]).all(), f
    assert one["status"][0, 0] == 0x803 and np.isfinite(one["xi"][0, 0])


def test_oracle_buffers_and_knots_do_not_depend_on_kappa():
    _, ref = h3_oracle(2)
    for f in ("tau_in_unc", "tau_out_unc"):
        assert same(ref[f], ref[f][:, :, :, :1]).all(), f
        assert np.isfinite(ref[f]).any()
    assert (ref["n_knots_all"] == ref["n_knots_all"][0, 0, 0]).all()
    # … while they do depend on the hazard class
    assert not same(ref["tau_in_unc"][:, 0], ref["tau_in_unc"][:, 1]).all()
