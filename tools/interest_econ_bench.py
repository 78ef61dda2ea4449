"""Timing of sbr_sweep_interest_econ_dev against the route a β × p × λ × (r, δ) × κ × u product of the
interest-rate extension had before it (not part of bench.py).

Two shapes, knot_capacity = 65536, default tolerances (every value function at eps()):
  (A) a κ-heavy policy map: sbr.fig5_grid(64) columns × 1 p × 1 λ × 2 rates × 16 κ × 64 u;
  (B) one column (β = 1, η = 15, t_end = 30) × 4 p × 4 λ × 4 rates (one of them r = 0) × 4 κ × 64 u.
For each shape:
  (new)   sweep_interest_econ_dev;
  (loop)  sweep_interest_dev once per (p, λ, rate, κ) into slices of a staging tensor, alternating
          with (new) in the same process.
Each variant: --warmup warm-up and --repeats timed calls on one stream, timed with device events
around each call, a synchronise after each round.  Reports medians and spreads, the ratio beside n_κ
and the number of sweeps in the loop, and whether the variants agree bit for bit after reindexing
(rk_steps: every κ of the loop against the one value of (new)); writes
profiles/interest_econ_bench.json (or --out) and prints a summary.
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

CAP, X0 = 65536, 1e-4
FIELDS = (*sbr.engine.RESULT_FIELDS, "status", "iters")


def shapes() -> dict:
    g = sbr.fig5_grid(64)
    a = dict(beta=g.beta, eta=g.eta, t_end=g.t_end, p=np.array([.5]), lam=np.array([.01]),
             r=np.array([.02, .06]), delta=np.array([.1, .1]), kappa=np.linspace(.1, .9, 16),
             u=np.linspace(.001, .6, 64))
    b = dict(beta=np.array([1.0]), eta=np.array([15.0]), t_end=np.array([30.0]), p=np.linspace(.2, .95, 4),
             lam=np.geomspace(.002, .2, 4), r=np.array([0.0, .02, .06, .02]), delta=np.array([.1, .1, .1, .5]),
             kappa=np.linspace(.2, .8, 4), u=np.linspace(.001, .6, 64))
    return {"A": a, "B": b}


def stats(ms) -> dict:
    ms = np.asarray(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()),
                ms=[round(float(x), 4) for x in ms])


def same(x, y) -> bool:
    return bool(((x == y) | ((x != x) & (y != y))).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "interest_econ_bench.json"))
    ap.add_argument("--shapes", default="A,B")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    eng = sbr.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    sp = stream.cuda_stream
    res = dict(tool="tools/interest_econ_bench.py", warmup=args.warmup, repeats=args.repeats, knot_capacity=CAP,
               device=torch.cuda.get_device_name(dev),
               libsbr_interest_econ_kernel_sha=provenance.kernel_code_sha("interest_econ_kernel"),
               libsbr_equilibrium_kernel_sha=provenance.kernel_code_sha("equilibrium_kernel"), shapes={})
    for name, host in shapes().items():
        if name not in args.shapes.split(","):
            continue
        d = {k: torch.from_numpy(np.ascontiguousarray(v, np.float64)).to(dev) for k, v in host.items()}
        nb, n_p, nl, nr, nk, nu = (host[k].size for k in ("beta", "p", "lam", "r", "kappa", "u"))

        def new_out(shape, sshape):
            o = {k: torch.empty(shape, dtype=torch.float64, device=dev) for k in sbr.engine.RESULT_FIELDS}
            o["status"] = torch.empty(shape, dtype=torch.int32, device=dev)
            o["iters"] = torch.empty(shape, dtype=torch.int32, device=dev)
            o["rk_steps"] = torch.empty(sshape, dtype=torch.int64, device=dev)
            return o

        outs = {"new": new_out((nb, n_p, nl, nr, nk, nu), (nb, n_p, nl, nr, nu)),
                "loop": new_out((n_p, nl, nr, nk, nb, nu), (n_p, nl, nr, nk, nb, nu))}
        combos = [(a, b, r, c) for a in range(n_p) for b in range(nl) for r in range(nr) for c in range(nk)]
        slices = {q: {k: v[q] for k, v in outs["loop"].items()} for q in combos}
        hp, hl, hr, hd, hk = (host[k].tolist() for k in ("p", "lam", "r", "delta", "kappa"))

        def loop():
            for (a, b, r, c), o in slices.items():
                eng.sweep_interest_dev(d["beta"], d["eta"], d["t_end"], d["u"], hp[a], hk[c], hl[b], hr[r], hd[r], X0,
                                       o, stream=sp, knot_capacity=CAP)

        calls = {"new": lambda: eng.sweep_interest_econ_dev(**d, x0=X0, out=outs["new"], stream=sp,
                                                            knot_capacity=CAP),
                 "loop": loop}
        stream.wait_stream(torch.cuda.current_stream(dev))
        t = {v: [] for v in calls}
        with torch.cuda.stream(stream):
            for rnd in range(args.warmup + args.repeats):  # (loop) alternates with (new)
                ev = {}
                for v in calls:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    calls[v]()
                    e1.record(stream)
                    ev[v] = (e0, e1)
                stream.synchronize()
                ms = {v: a.elapsed_time(b) for v, (a, b) in ev.items()}
                print(f"shape {name} round {rnd}{' (warm-up)' if rnd < args.warmup else ''}: "
                      + ", ".join(f"{v} {x:.2f} ms" for v, x in ms.items()), flush=True)
                if rnd >= args.warmup:
                    for v in calls:
                        t[v].append(ms[v])
        entry = {v: stats(t[v]) for v in calls}
        entry["points_total"] = nb * n_p * nl * nr * nk * nu
        entry["n_kappa"] = nk
        entry["sweeps_in_the_loop"] = len(combos)
        entry["value_functions_new"] = nb * n_p * nl * int((host["r"] > 0).sum()) * nu
        entry["value_functions_loop"] = entry["value_functions_new"] * nk
        entry["loop_median_over_new_median"] = entry["loop"]["median_ms"] / entry["new"]["median_ms"]
        st = outs["new"]["status"].cpu().numpy().view(np.uint32)
        entry["run_points"] = int(((st & sbr.STATUS["SBR_RUN"]) != 0).sum())
        entry["knot_overflow_points"] = int(((st & sbr.STATUS["SBR_KNOT_OVERFLOW"]) != 0).sum())
        entry["rk_steps_max"] = int(outs["new"]["rk_steps"].max())
        entry["new_equals_loop_bitwise"] = all(
            same(outs["new"][k], outs["loop"][k].permute(4, 0, 1, 2, 3, 5)) for k in FIELDS) and same(
            outs["new"]["rk_steps"].unsqueeze(4).expand(nb, n_p, nl, nr, nk, nu),
            outs["loop"]["rk_steps"].permute(4, 0, 1, 2, 3, 5))
        assert entry["new_equals_loop_bitwise"], f"shape {name}: (new) and (loop) differ"
        entry["new_median_below_the_fastest_loop_repeat"] = entry["new"]["median_ms"] < entry["loop"]["min_ms"]
        res["shapes"][name] = entry
    eng.close()
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    slim = {s: {k: (v if not isinstance(v, dict) else {q: v[q] for q in ("median_ms", "min_ms", "max_ms")})
                for k, v in e.items()} for s, e in res["shapes"].items()}
    print(json.dumps(slim))


if __name__ == "__main__":
    main()
