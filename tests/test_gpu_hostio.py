"""The host-pointer sweeps' staging and readback (csrc/sbr_hostio.h): every family's host-pointer
entry point on one Engine, in a sequence where a larger call precedes a smaller one and the sizes
are odd, bit for bit against the same family's *_dev entry point on torch tensors (which stages
nothing); optional result fields left NULL, with guard words behind every array passed; and the
phases sbr_host_phases reports for a single-device sweep."""
import ctypes

import numpy as np
import pytest

import sbr
from points_cases import FIELDS, assert_same
from sbr import _lib
from sbr.engine import _opts, _ptr

pytestmark = pytest.mark.gpu

X0, P, KAPPA, LAM = 1e-4, 0.5, 0.6, 0.01
ETA, T_END = 15.0, 30.0
BETA5 = 1.0 / sbr.julia_range("0.05", "1", 5)       # 20 … 1
U7 = sbr.julia_range("0.001", "1", 7)
BETA11 = 1.0 / sbr.julia_range("0.02", "2", 11)     # the list of models: n = 11
U11 = sbr.julia_range("0.001", "0.9", 11)
SOA = (*FIELDS, "status", "iters")
GUARD = 0xA5


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


def _dev_out(n, extra=()):
    """Result tensors of n points for a *_dev call, filled with a pattern no result has."""
    import torch

    out = {k: torch.full((n,), -7.0, dtype=torch.float64, device="cuda") for k in FIELDS}
    out["status"] = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    out["iters"] = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    for k in extra:
        out[k] = torch.full((n,), -7, dtype=torch.int64 if k == "rk_steps" else torch.int32, device="cuda")
    return out


def _host(out, keys):
    import torch

    torch.cuda.synchronize()
    r = {k: out[k].cpu().numpy() for k in keys}
    r["status"] = r["status"].view(np.uint32)
    return r


def _compare(name, host, dev, keys):
    for k in keys:
        assert_same(np.asarray(host[k]).reshape(-1), dev[k].reshape(-1), f"{name}: {k}")


def test_staging_reuse_across_families_and_sizes(engine):
    import torch

    grid57 = sbr.BaselineGrid(BETA5, U7, ETA, T_END, p=P, kappa=KAPPA, lam=LAM, x0=X0)
    grid34 = sbr.BaselineGrid(BETA5[1:4], U7[2:6], ETA, T_END, p=P, kappa=KAPPA, lam=LAM, x0=X0)
    so_eta = 30.0 / 0.9
    so_beta = 1.0 / sbr.julia_range("0.01", "2", 512)[[0, 200, 511]]
    so_u = sbr.julia_range("0.001", "1", 512)[[10, 300]]
    so_cmp = np.stack([sbr.julia_range(0.0, so_eta, 1000)] * 3)
    pts = dict(beta=BETA11, u=U11, eta=np.full(11, ETA), t_end=np.full(11, T_END), p=np.linspace(0.3, 0.9, 11),
               kappa=np.linspace(0.2, 0.8, 11), lam=np.full(11, LAM))
    het_betas = np.outer(BETA5, [0.5, 1.0, 2.0])
    het_dist = np.array([0.3, 0.4, 0.3])
    ec = dict(beta=BETA5[:3], eta=np.full(3, ETA), t_end=np.full(3, T_END), u=U7[:5], p=np.array([0.5, 0.9]),
              kappa=np.array([0.3, 0.6]), lam=np.array([LAM]))

    # the host-pointer calls, in this order on the one engine
    h = {}
    h["baseline 5x7"] = engine.sweep_baseline(grid57)
    h["social 3x2"] = engine.sweep_social(so_beta, so_eta, so_u, 0.99, 0.25, 0.25, cmp=so_cmp, x0=X0, max_iter=3)
    h["points 11"] = engine.solve_points(**pts, x0=X0)
    h["hetero K=3 5x7"] = engine.sweep_hetero(het_betas, het_dist, ETA, T_END, U7, P, KAPPA, LAM, x0=X0)
    h["econ 3x2x1x2x5"] = engine.sweep_econ(**ec, x0=X0)
    h["interest 5x7"] = engine.sweep_interest(BETA5, ETA, T_END, U7, P, KAPPA, LAM, 0.06, 0.1, x0=X0)
    h["baseline 3x4"] = engine.sweep_baseline(grid34)
    assert 35 % 2 == 1 and 11 % 2 == 1 and (3 * 5 + 7) * 8 % 256 != 0 and 7 * 11 * 8 % 256 != 0

    # the same inputs through the *_dev entry points
    for name, g in (("baseline 5x7", grid57), ("baseline 3x4", grid34)):
        out = _dev_out(g.n_points)
        engine.sweep_baseline_dev(_dev(g.beta), _dev(g.eta), _dev(g.t_end), _dev(g.u), P, KAPPA, LAM, X0, out)
        _compare(name, h[name], _host(out, SOA), SOA)

    out = _dev_out(6, extra=("fp_iters", "rk_steps"))
    engine.sweep_social_dev(_dev(so_beta), _dev(np.full(3, so_eta)), _dev(so_u), 0.99, 0.25, 0.25, _dev(so_cmp), X0,
                            out, max_iter=3)
    keys = (*SOA, "fp_iters", "rk_steps")
    _compare("social 3x2", h["social 3x2"], _host(out, keys), keys)

    out = _dev_out(11)
    engine.solve_points_dev(**{k: _dev(v) for k, v in pts.items()}, x0=X0, out=out)
    _compare("points 11", h["points 11"], _host(out, SOA), SOA)

    out = _dev_out(35)
    tin = torch.full((35 * 3,), -7.0, dtype=torch.float64, device="cuda")
    tout = torch.full((35 * 3,), -7.0, dtype=torch.float64, device="cuda")
    soa = _lib.ResultSoA(out["xi"].data_ptr(), None, None, out["aw_max"].data_ptr(), out["tol"].data_ptr(),
                         out["status"].data_ptr(), out["iters"].data_ptr())
    opts = _opts(knot_capacity=16384)
    hb, hd, he, ht, hu = (_dev(a) for a in (het_betas, het_dist, np.full(5, ETA), np.full(5, T_END), U7))
    rc = engine._L.sbr_sweep_hetero_dev(engine._ctx, None, 3, hb.data_ptr(), hd.data_ptr(), he.data_ptr(),
                                        ht.data_ptr(), X0, hu.data_ptr(), 5, 7, P, KAPPA, LAM, ctypes.byref(opts),
                                        ctypes.byref(soa), tin.data_ptr(), tout.data_ptr())
    assert rc == 0, engine._L.sbr_last_error(engine._ctx)
    keys = ("xi", "aw_max", "tol", "status", "iters")
    d = _host(out, keys)
    d["tau_in_unc"], d["tau_out_unc"] = tin.cpu().numpy(), tout.cpu().numpy()
    _compare("hetero K=3 5x7", h["hetero K=3 5x7"], d, (*keys, "tau_in_unc", "tau_out_unc"))

    out = _dev_out(3 * 2 * 1 * 2 * 5)
    engine.sweep_econ_dev(**{k: _dev(v) for k, v in ec.items()}, x0=X0, out=out)
    _compare("econ 3x2x1x2x5", h["econ 3x2x1x2x5"], _host(out, SOA), SOA)

    out = _dev_out(35, extra=("rk_steps",))
    engine.sweep_interest_dev(_dev(BETA5), _dev(np.full(5, ETA)), _dev(np.full(5, T_END)), _dev(U7), P, KAPPA, LAM,
                              0.06, 0.1, X0, out)
    keys = (*SOA, "rk_steps")
    _compare("interest 5x7", h["interest 5x7"], _host(out, keys), keys)


def _guarded(n, dtype):
    """An n-element array with 8 guard elements behind it (one buffer): (whole buffer, the array)."""
    buf = np.empty(n + 8, dtype)
    buf.view(np.uint8)[:] = GUARD
    return buf, buf[:n]


def _host_call(engine, family, n, drop):
    """The family's host-pointer entry point through the C ABI with the result fields in `drop`
    passed as NULL; returns {field: array} of the others after checking every guard word."""
    L, o = engine._L, _opts()
    bufs = {k: _guarded(n, np.float64) for k in FIELDS if k not in drop}
    bufs["status"] = _guarded(n, np.uint32)
    if "iters" not in drop:
        bufs["iters"] = _guarded(n, np.int32)
    soa = _lib.ResultSoA(*[_ptr(bufs[k][1]) if k in bufs else None for k in SOA])
    c = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
    if family == "baseline":
        ins = [c(BETA5), c(np.full(5, ETA)), c(np.full(5, T_END)), c(U7)]
        rc = L.sbr_sweep_baseline(engine._ctx, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), X0, _ptr(ins[3]), 5, 7, P,
                                  KAPPA, LAM, ctypes.byref(o), ctypes.byref(soa))
    elif family == "points":
        ins = [c(BETA11), c(np.full(11, ETA)), c(np.full(11, T_END)), c(U11), c(np.linspace(0.3, 0.9, 11)),
               c(np.linspace(0.2, 0.8, 11)), c(np.full(11, LAM))]
        rc = L.sbr_solve_points(engine._ctx, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), X0, _ptr(ins[3]),
                                _ptr(ins[4]), _ptr(ins[5]), _ptr(ins[6]), 11, ctypes.byref(o), ctypes.byref(soa))
    else:  # econ: 5 β × 1 × 1 × 1 × 7 u, the 5 × 7 shape
        ins = [c(BETA5), c(np.full(5, ETA)), c(np.full(5, T_END)), c(U7), c([P]), c([LAM]), c([KAPPA])]
        rc = L.sbr_sweep_econ(engine._ctx, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), X0, _ptr(ins[3]), 5, 7,
                              _ptr(ins[4]), 1, _ptr(ins[5]), 1, _ptr(ins[6]), 1, ctypes.byref(o), ctypes.byref(soa))
    assert rc == 0, (family, drop, L.sbr_last_error(engine._ctx))
    for k, (buf, _) in bufs.items():
        assert (buf[n:].view(np.uint8) == GUARD).all(), f"{family} without {drop}: guard behind {k} overwritten"
    return {k: a.copy() for k, (_, a) in bufs.items()}


@pytest.mark.parametrize("family,n", [("baseline", 35), ("points", 11), ("econ", 35)])
def test_optional_outputs(engine, family, n):
    full = _host_call(engine, family, n, drop=())
    assert set(full) == set(SOA)
    for drop in (("iters",), ("tau_in_unc", "tau_out_unc")):
        part = _host_call(engine, family, n, drop=drop)
        assert set(part) == set(SOA) - set(drop)
        for k in part:
            assert_same(part[k], full[k], f"{family} without {drop}: {k}")


def test_single_device_host_phases(engine):
    grid = sbr.BaselineGrid(BETA5, U7, ETA, T_END, p=P, kappa=KAPPA, lam=LAM, x0=X0)
    engine.timing_enable(True)
    try:
        engine.sweep_baseline(grid)
        ph = engine.host_phases()
    finally:
        engine.timing_enable(False)
    assert list(ph) == ["h2d", "kernels", "d2h", "host_copy_early_exit", "call"]
    for k, v in ph.items():
        assert np.isfinite(v) and v >= 0.0, (k, ph)
    for k in ("h2d", "kernels", "d2h", "host_copy_early_exit"):
        assert ph["call"] >= ph[k], (k, ph)
