"""GPU parity of sbr_equilibrium_on_knots[_pdf] on the hostile caller knots of
tests/knots_hostile_cases.py — G with decreases around the drawdown bound, NaN, values outside [0, 2],
repeated knot times, oscillating / negative / non-finite pdfs, u tied to hazard values, time axes outside
the `rcp_ok` and `moderate` ranges, one- and two-knot grids — against the oracle's plain linear scans,
bit for bit (NaN equal to NaN) on every field, the status bits and the iteration count, on five paths:
the LDS kernel's pruned vector call, the same with SBR_FLAG_EXHAUSTIVE, the same with the AW evaluation
counter (SBR_FLAG_DIAG_COUNT_AW_BLOCKS: a column whose statistics forbid both the scan and the branch
and bound evaluates every hazard entry), the single-point kernel with its hazard and AW paths, and, for
eight cases, the global-memory kernel on the knots refined past the LDS slab.  After each case the clean
column must give its clean bits again (the resident knots and hazard are replaced by value)."""
import numpy as np
import pytest

import knots_hostile_cases as H
from sbr import _lib
from test_gpu_knots import check_point, same

pytestmark = pytest.mark.gpu

_cache = {}


def _cases(oracle):
    if "cases" not in _cache:
        _cache["cases"] = {c["name"]: c for c in H.cases(oracle)}
    return _cache["cases"]


def _reference(oracle, name, refined=False):
    """The oracle's 64 answers (with paths) of a case, computed once."""
    key = (name, refined)
    if key not in _cache:
        c = _cases(oracle)[name]
        knots = H.refine(c["t"], c["G"], c["pdf"]) if refined else (c["t"], c["G"], c["pdf"])
        _cache[key] = (knots, [H.solve(oracle, c, u, *knots) for u in c["u"]])
    return _cache[key]


def _call(engine, c, knots, u, **kw):
    t, G, pdf = knots
    return engine.equilibrium_on_knots(t, G, c["beta"], c["eta"], c["t_end"], u, c["p"], c["kappa"], c["lam"],
                                       pdf=pdf, **kw)


def _check_vector(g, ref, what, iters=True):
    for j, o in enumerate(ref):
        for f in H.FIELDS:
            assert same(g[f][j], o[f]), (what, j, f, g[f][j], o[f])
        assert int(g["status"][j]) == o["status"], (what, j, hex(int(g["status"][j])), hex(o["status"]))
        if iters or not (o["status"] & H.RUN):
            assert int(g["iters"][j]) == o["iters"], (what, j, int(g["iters"][j]), o["iters"])


def _lds_cap_b(engine):
    """The baseline equilibrium kernel's LDS knot capacity (sbr_create: half the block's LDS, 1 KiB slack)."""
    return ((engine.device_info()["lds_bytes_per_block"] // 2 - 1024) * 64) // (8 * (2 * 64 + 6 + 16))


@pytest.mark.parametrize("name", H.NAMES)
def test_hostile_knots_bitwise(engine, oracle, name):
    c = _cases(oracle)[name]
    knots, ref = _reference(oracle, name)
    assert len(c["t"]) <= _lds_cap_b(engine)  # the LDS kernel
    st = np.array([o["status"] for o in ref], np.uint32)
    run = (st & H.RUN) != 0
    ntau = ref[0]["n_hr"]

    # the vector call: pruned, exhaustive, counted
    g = _call(engine, c, knots, c["u"], paths=False)
    _check_vector(g, ref, (name, "pruned"))
    g = _call(engine, c, knots, c["u"], paths=False, exhaustive=True)
    _check_vector(g, ref, (name, "exhaustive"))
    g = _call(engine, c, knots, c["u"], paths=False, flags=_lib.SBR_FLAG_DIAG_COUNT_AW_BLOCKS)
    _check_vector(g, ref, (name, "counted"), iters=False)
    count = g["iters"][run]
    print(f"{name}: {int(run.sum())} run points, {int(count.sum())} AW evaluations of {int(run.sum()) * ntau} "
          f"(n_tau = {ntau}), dispatch {c['expect']}")
    if c["expect"] == "exhaustive":
        assert (count == ntau).all(), (name, count, ntau)
    else:
        assert (count >= 1).all(), (name, count)

    # the single-point kernel with paths: a run point, a trivial no-run, a failed bisection, anything else
    failed = (st & (H.COLLAPSE | H.MAXITER)) != 0
    below = (st & H.BELOW) != 0
    picks = [int(np.argmax(m)) for m in (run, below, failed, ~(run | below | failed)) if m.any()]
    assert picks
    for j in picks:
        one = _call(engine, c, knots, float(c["u"][j]))
        check_point(one, ref[j], (name, "single", j))

    # the global-memory kernel: the knots refined past the LDS slab
    if c["gmem"]:
        kr, rr = _reference(oracle, name, refined=True)
        info = engine.device_info()
        assert len(kr[0]) > _lds_cap_b(engine)
        assert len(kr[0]) > info["lds_knot_capacity"] // 2 or len(kr[0]) > 4432
        g = _call(engine, c, kr, c["u"], paths=False)
        _check_vector(g, rr, (name, "global memory"))
        assert any(o["status"] & H.RUN for o in rr), name

    # the clean column afterwards: its own bits
    clean = _cases(oracle)["clean"]
    kc, rc = _reference(oracle, "clean")
    g = _call(engine, clean, kc, clean["u"], paths=False)
    _check_vector(g, rc, (name, "clean afterwards"))
