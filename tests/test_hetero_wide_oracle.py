"""What the K = 5 … 16 grids of tests/test_gpu_hetero_wide.py contain, asserted on the CPU oracle
(no GPU): the GPU tests compare against these results bit for bit, so they cover a path only if
the oracle's results here take it — the Rosenbrock23 branch with a K×K LU at every size, the
CDF drawdown, the bisection's iteration cap and collapse exit, the interpolant's BoundsError."""
import numpy as np
import pytest

import sbr
from hetero_wide_cases import CONFIG4_RUNS, WIDE_K, config4, learned, unequal_k10

S = sbr.STATUS


@pytest.mark.parametrize("K", WIDE_K)
def test_config4_grids_reach_every_path(K):
    g, o = config4(6, 24, K)
    st = o["status"]
    assert st.shape == (6, 24) and g.K == K
    assert int(((st & S["SBR_RUN"]) > 0).sum()) == CONFIG4_RUNS[K]
    # every column's learning switched to Rosenbrock23: a K×K LU was factored
    assert ((st & S["SBR_STIFF_SWITCH"]) > 0).all()
    # column 0: an ulp-sized decrease in some group CDF (the drawdown), column 5: none
    _, G0, i0 = learned(6, 24, K, 0)
    _, G5, i5 = learned(6, 24, K, 5)
    assert i0["nstiff"] > 0 and i5["nstiff"] > 0
    d0 = np.diff(G0, axis=0)
    # ulp-sized: rounding noise of the saturated tail, under 100 spacings of the doubles below 1
    assert (d0 < 0).any() and d0[d0 < 0].min() > -100 * 2.0 ** -53
    assert not (np.diff(G5, axis=0) < 0).any()
    if K == 7:
        cap = (st & S["SBR_NO_RUN_MAXITER"]) > 0
        assert cap.any() and (o["iters"][cap] == 499).all()
    else:
        assert ((st & S["SBR_NO_RUN_COLLAPSE"]) > 0).any()


def test_unequal_shares_unsorted_rates_bounds_error():
    g, o = unequal_k10()
    assert g.K == 10 and o["status"].shape == (3, 24)
    assert (np.diff(g.betas[0]) < 0).any() and len(set(g.dist)) == 10
    run = (o["status"] & S["SBR_RUN"]) > 0
    assert int(run.sum()) == 68
    assert ((o["status"][~run] & S["SBR_OOB"]) > 0).all() and int((~run).sum()) == 4


def test_k16_column_has_stiff_knots():
    t, G, info = learned(2, 4, 16, 1)
    assert len(t) == 5907 and G.shape == (5907, 16)
    assert info["nswitch"] > 0 and info["nstiff"] > 0
