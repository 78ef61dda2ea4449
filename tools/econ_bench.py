"""Timing of sbr_sweep_econ_dev against the two routes a β × p × λ × κ × u product had before it
(not part of bench.py).

Two shapes, knot_capacity = 65536:
  (A) sbr.fig5_grid(64) columns × p (4) × λ (4) × κ (8) × u (256);
  (B) one column (β = 1, η = 15, t_end = 30) × p (16) × λ (16) × κ (16) × u (64).
For each shape:
  (new)    sweep_econ_dev;
  (loop)   sweep_baseline_dev once per (p, λ, κ) into slices of a staging tensor, alternating with
           (new) in the same process;
  (points) solve_points_dev on the flattened product, for (B) only.
Each variant: 5 warm-up and 20 timed calls on one stream, timed with device events around each
call, a synchronise at the end.  Reports medians and spreads and whether the variants agree bit for
bit after reindexing; writes profiles/econ_bench.json (or --out) and prints a summary.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "replication-social-bank-runs_amd"))
import sbr  # noqa: E402
from sbr import provenance  # noqa: E402

WARMUP, REPEATS, CAP, X0 = 5, 20, 65536, 1e-4
FIELDS = (*sbr.engine.RESULT_FIELDS, "status", "iters")


def shapes() -> dict:
    g = sbr.fig5_grid(64)
    a = dict(beta=g.beta, eta=g.eta, t_end=g.t_end, p=np.linspace(.2, .95, 4), lam=np.geomspace(.002, .2, 4),
             kappa=np.linspace(.1, .9, 8), u=np.linspace(.001, 1.0, 256))
    b = dict(beta=np.array([1.0]), eta=np.array([15.0]), t_end=np.array([30.0]), p=np.linspace(.05, 1.0, 16),
             lam=np.geomspace(.001, .5, 16), kappa=np.linspace(.05, .95, 16), u=np.linspace(.001, 1.0, 64))
    return {"A": a, "B": b}


def stats(ms) -> dict:
    ms = np.asarray(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()),
                ms=[round(float(x), 4) for x in ms])


def same(x, y) -> bool:
    return bool(((x == y) | ((x != x) & (y != y))).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "econ_bench.json"))
    ap.add_argument("--shapes", default="A,B")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    eng = sbr.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    sp = stream.cuda_stream
    res = dict(tool="tools/econ_bench.py", warmup=WARMUP, repeats=REPEATS, knot_capacity=CAP,
               device=torch.cuda.get_device_name(dev),
               libsbr_equilibrium_econ_kernel_sha=provenance.kernel_code_sha("equilibrium_econ_kernel"),
               libsbr_equilibrium_kernel_sha=provenance.kernel_code_sha("equilibrium_kernel"), shapes={})
    for name, host in shapes().items():
        if name not in args.shapes.split(","):
            continue
        d = {k: torch.from_numpy(np.ascontiguousarray(v, np.float64)).to(dev) for k, v in host.items()}
        nb, n_p, nl, nk, nu = (host[k].size for k in ("beta", "p", "lam", "kappa", "u"))
        n = nb * n_p * nl * nk * nu
        variants = ["new", "loop"] + (["points"] if name == "B" else [])

        def new_out(shape):
            o = {k: torch.empty(shape, dtype=torch.float64, device=dev) for k in sbr.engine.RESULT_FIELDS}
            o["status"] = torch.empty(shape, dtype=torch.int32, device=dev)
            o["iters"] = torch.empty(shape, dtype=torch.int32, device=dev)
            return o

        outs = {"new": new_out((nb, n_p, nl, nk, nu)), "loop": new_out((n_p, nl, nk, nb, nu))}
        combos = [(a, b, c) for a in range(n_p) for b in range(nl) for c in range(nk)]
        slices = {abc: {k: v[abc] for k, v in outs["loop"].items()} for abc in combos}
        hp, hl, hk = (host[k].tolist() for k in ("p", "lam", "kappa"))

        def loop():
            for (a, b, c), o in slices.items():
                eng.sweep_baseline_dev(d["beta"], d["eta"], d["t_end"], d["u"], hp[a], hk[c], hl[b], X0, o, stream=sp,
                                       knot_capacity=CAP)

        calls = {"new": lambda: eng.sweep_econ_dev(**d, x0=X0, out=outs["new"], stream=sp, knot_capacity=CAP),
                 "loop": loop}
        if "points" in variants:
            outs["points"] = new_out((n,))
            mesh = torch.meshgrid(d["beta"], d["p"], d["lam"], d["kappa"], d["u"], indexing="ij")
            flat = {k: m.reshape(-1).contiguous() for k, m in zip(("beta", "p", "lam", "kappa", "u"), mesh)}
            flat["eta"] = d["eta"].repeat_interleave(n // nb)
            flat["t_end"] = d["t_end"].repeat_interleave(n // nb)
            calls["points"] = lambda: eng.solve_points_dev(**flat, x0=X0, out=outs["points"], stream=sp,
                                                           knot_capacity=CAP)
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

        t = timed(["new", "loop"])  # (loop) alternates with (new)
        if "points" in variants:
            t.update(timed(["points"]))
        entry = {v: stats(t[v]) for v in variants}
        entry["points_total"] = n
        entry["combinations"] = len(combos)
        st = outs["new"]["status"].cpu().numpy().view(np.uint32)
        entry["run_points"] = int(((st & sbr.STATUS["SBR_RUN"]) != 0).sum())
        entry["knot_overflow_points"] = int(((st & sbr.STATUS["SBR_KNOT_OVERFLOW"]) != 0).sum())
        entry["new_equals_loop_bitwise"] = all(
            same(outs["new"][k], outs["loop"][k].permute(3, 0, 1, 2, 4)) for k in FIELDS)
        if "points" in variants:
            entry["new_equals_points_bitwise"] = all(
                same(outs["new"][k].reshape(-1), outs["points"][k]) for k in FIELDS)
        fastest_old = min(entry[v]["min_ms"] for v in variants if v != "new")
        entry["fastest_repeat_of_the_faster_old_route_ms"] = fastest_old
        entry["new_median_below_it"] = entry["new"]["median_ms"] < fastest_old
        res["shapes"][name] = entry
    eng.close()
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    slim = {s: {k: (v if not isinstance(v, dict) else {q: v[q] for q in ("median_ms", "min_ms", "max_ms")})
                for k, v in e.items()} for s, e in res["shapes"].items()}
    print(json.dumps(slim))


if __name__ == "__main__":
    main()
