"""The hostile caller knots of tests/knots_hostile_cases.py, on the oracle alone (CPU): every case has the
property it is named for (the kernel's summary statistics restated in numpy, and the AW_max dispatch
that follows from them), the oracle answers all 64 u of it, and — unless the case is one where no point
can run — at least 16 points run or end as a false equilibrium and at least 8 end otherwise, so that no
case degenerates into 64 trivial no-runs.  tests/test_gpu_knots_hostile.py holds the kernels to these
answers."""
import numpy as np
import pytest

import knots_hostile_cases as H


@pytest.fixture(scope="module")
def cases(oracle):
    return {c["name"]: c for c in H.cases(oracle)}


def test_case_list_is_the_parametrized_one(cases):
    assert list(cases) == H.NAMES


def test_global_memory_cases(cases):
    """The cases the GPU test also refines past the LDS slab (the global-memory kernel)."""
    assert sorted(n for n, c in cases.items() if c["gmem"]) == sorted(
        ["dd_above", "nonmono_crowded", "nan_past_eta", "t_rep_last", "pdf_fast_sin", "ties", "scale_2^70", "scale_2^74"])


@pytest.mark.parametrize("name", H.NAMES)
def test_premise_and_class_counts(oracle, cases, name):
    c = cases[name]
    s = H.stats(c["t"], c["G"])
    assert c["premise"](s), (name, {k: v for k, v in s.items()})
    assert c["expect"] in ("exhaustive", "pruned", "any")
    if c["expect"] != "any":
        assert H.branch(s) == c["expect"], (name, s)
    assert len(c["u"]) == 64 and (c["u"] >= 0.0).all()
    assert np.all(np.diff(c["t"]) >= 0) and np.isfinite(c["t"]).all()
    assert s["n"] <= 3600  # inside the baseline kernel's LDS slab; the GPU test refines past it
    res = [H.solve(oracle, c, u) for u in c["u"]]
    st = np.array([r["status"] for r in res], np.uint32)
    run, below, col, mxi, other = H.classes(st)
    print(f"{name}: n = {s['n']}, run/false-eq {run}, HR below u {below}, collapse {col}, max-iter {mxi}, "
          f"other {other}; ndec {s['ndec']}, dd {s['dd']:.3g}, noscan {s['noscan']}, near1 {s['near1']}, "
          f"dispatch {H.branch(s)}")
    for r in res:
        ok = bool(r["status"] & H.RUN)
        assert np.isnan(r["xi"]) != ok and np.isnan(r["aw_max"]) != ok, (name, hex(r["status"]))
    if c["cap"]:
        assert run >= 16 and 64 - run >= 8, (name, run, below, col, mxi, other)
    else:
        assert run == 0, name
