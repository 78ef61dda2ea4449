"""Timing of sbr_solve_points_dev against the route a list had before it (not part of bench.py).

For N = 4,096 and 65,536 points drawn with rng(1) from the distributions of the test list L70
(tests/points_cases.py), knot_capacity = 32768:
  (a) solve_points_dev, every parameter per point;
  (b) solve_points_dev with uniform scalars: β, η, t_end per point, one (u, p, κ, λ);
  (c) the earlier route for (b): sweep_baseline_dev with n_beta = N, n_u = 1,
      alternating with (b) in the same process.
Each variant: 5 warm-up and 20 timed calls on one stream, timed with device events around each
call, a synchronise at the end.  Reports medians and spreads, the SBR_KNOT_OVERFLOW count and
whether (b) and (c) agree bit for bit; writes profiles/points_bench.json and prints it.
"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "replication-social-bank-runs_amd"))
import sbr  # noqa: E402
from sbr import provenance  # noqa: E402

WARMUP, REPEATS, CAP, X0 = 5, 20, 32768, 1e-4
UNIFORM = dict(u=0.1, p=0.5, kappa=0.6, lam=0.01)
ARGS = ("beta", "eta", "t_end", "u", "p", "kappa", "lam")


def draw(n: int) -> dict:
    rng = np.random.default_rng(1)
    beta = 10.0 ** rng.uniform(-1, 4, n)
    carry = rng.random(n) < 0.5
    eta = np.where(carry, 15.0, 15.0 / beta)
    t_end = np.where(carry, 30.0, 2 * eta)
    return dict(beta=beta, eta=eta, t_end=t_end, u=rng.uniform(0.001, 1.0, n), p=rng.uniform(0.05, 0.99, n),
                kappa=rng.uniform(0.05, 0.95, n), lam=10.0 ** rng.uniform(-3, 0, n))


def stats(ms) -> dict:
    ms = np.asarray(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()),
                ms=[round(float(x), 4) for x in ms])


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    eng = sbr.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    sp = stream.cuda_stream
    over = sbr.STATUS["SBR_KNOT_OVERFLOW"]
    res = dict(tool="tools/points_bench.py", warmup=WARMUP, repeats=REPEATS, knot_capacity=CAP, uniform=UNIFORM,
               device=torch.cuda.get_device_name(dev), libsbr_points_kernel_sha=provenance.kernel_code_sha("points_kernel"),
               sizes={})
    for n in (4096, 65536):
        host = draw(n)
        mixed = {k: torch.from_numpy(host[k]).to(dev) for k in ARGS}
        unif = dict(mixed, **{k: torch.full((n,), v, dtype=torch.float64, device=dev) for k, v in UNIFORM.items()})
        u1 = torch.tensor([UNIFORM["u"]], dtype=torch.float64, device=dev)

        def new_out():
            o = {k: torch.empty(n, dtype=torch.float64, device=dev) for k in sbr.engine.RESULT_FIELDS}
            o["status"] = torch.empty(n, dtype=torch.int32, device=dev)
            o["iters"] = torch.empty(n, dtype=torch.int32, device=dev)
            return o

        outs = {v: new_out() for v in "abc"}
        calls = {
            "a": lambda: eng.solve_points_dev(**mixed, x0=X0, out=outs["a"], stream=sp, knot_capacity=CAP),
            "b": lambda: eng.solve_points_dev(**unif, x0=X0, out=outs["b"], stream=sp, knot_capacity=CAP),
            "c": lambda: eng.sweep_baseline_dev(mixed["beta"], mixed["eta"], mixed["t_end"], u1, UNIFORM["p"],
                                                UNIFORM["kappa"], UNIFORM["lam"], X0, outs["c"], stream=sp,
                                                knot_capacity=CAP),
        }
        stream.wait_stream(torch.cuda.current_stream(dev))

        def timed(names):
            """WARMUP + REPEATS rounds over `names` in turn; per name the REPEATS event times (ms)."""
            ev = {v: [] for v in names}
            with torch.cuda.stream(stream):
                for r in range(WARMUP + REPEATS):
                    for v in names:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        calls[v]()
                        e1.record(stream)
                        if r >= WARMUP:
                            ev[v].append((e0, e1))
            stream.synchronize()
            return {v: [a.elapsed_time(b) for a, b in ev[v]] for v in names}

        t = timed(["a"])
        t.update(timed(["b", "c"]))  # (c) alternates with (b)
        st = {v: outs[v]["status"].cpu().numpy().view(np.uint32) for v in "abc"}
        same = True
        for k in (*sbr.engine.RESULT_FIELDS, "status", "iters"):
            x, y = outs["b"][k].cpu().numpy(), outs["c"][k].cpu().numpy()
            same &= bool(((x == y) | ((x != x) & (y != y))).all())
        entry = {v: stats(t[v]) for v in "abc"}
        for v in "abc":
            entry[v]["knot_overflow_points"] = int(((st[v] & over) != 0).sum())
            entry[v]["run_points"] = int(((st[v] & sbr.STATUS["SBR_RUN"]) != 0).sum())
        entry["b_equals_c_bitwise"] = same
        entry["b_median_le_c_max"] = entry["b"]["median_ms"] <= entry["c"]["max_ms"]
        res["sizes"][str(n)] = entry
    eng.close()
    out = REPO / "profiles" / "points_bench.json"
    out.write_text(json.dumps(res, indent=1) + "\n")
    slim = {n: {**{v: {k: e[v][k] for k in ("median_ms", "min_ms", "max_ms", "knot_overflow_points")} for v in "abc"},
                **{k: e[k] for k in ("b_equals_c_bitwise", "b_median_le_c_max")}} for n, e in res["sizes"].items()}
    print(json.dumps(slim))


if __name__ == "__main__":
    main()
