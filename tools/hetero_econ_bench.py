"""Timing of sbr_sweep_hetero_econ_dev against the route a K-group p × λ × κ × u product had before
it: one sbr_sweep_hetero_dev per (p, λ, κ) (not part of bench.py).

Two shapes, knot_capacity = 16384:
  (A) sbr.hetero_config4(64, 256, 8) columns × p (2) × λ (2) × κ (8) × u (256): 524,288 points, 32
      combinations, the kernels specialised for K = 8;
  (B) the same at K = 12: the group-looped kernels.
For each shape:
  (new)   sweep_hetero_econ_dev;
  (loop)  sweep_hetero_dev once per (p, λ, κ) into slices of a staging tensor, alternating with (new)
          in the same process.
Each variant: 5 warm-up and 20 timed calls on one stream, timed with device events around each call,
a synchronise at the end.  Reports medians and spreads and whether the variants agree bit for bit
after reindexing; writes profiles/hetero_econ_bench.json (or --out) and prints a summary.
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

WARMUP, REPEATS, CAP = 5, 20, 16384
FIELDS = ("xi", "aw_max", "tol", "status", "iters")


def shapes() -> dict:
    out = {}
    for name, K in (("A", 8), ("B", 12)):
        g = sbr.hetero_config4(64, 256, K)
        out[name] = dict(K=K, x0=g.x0, betas=g.betas, dist=g.dist, eta=g.eta, t_end=g.t_end, u=g.u,
                         p=np.array([.5, .9]), lam=np.array([.01, .1]), kappa=np.linspace(.15, .85, 8))
    return out


def stats(ms) -> dict:
    ms = np.asarray(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()),
                ms=[round(float(x), 4) for x in ms])


def same(x, y) -> bool:
    return bool(((x == y) | ((x != x) & (y != y))).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "hetero_econ_bench.json"))
    ap.add_argument("--shapes", default="A,B")
    ap.add_argument("--warmup", type=int, default=WARMUP)
    ap.add_argument("--repeats", type=int, default=REPEATS)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    eng = sbr.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    sp = stream.cuda_stream
    res = dict(tool="tools/hetero_econ_bench.py", warmup=args.warmup, repeats=args.repeats, knot_capacity=CAP,
               device=torch.cuda.get_device_name(dev),
               kernel_sha={k: provenance.kernel_code_sha(k) for k in (
                   "equilibrium_hetero_econ_kernel", "equilibrium_hetero_econ_wide_kernel",
                   "hazard_hetero_econ_kernel", "equilibrium_hetero_kernel", "equilibrium_hetero_wide_kernel",
                   "learn_hetero_wave_kernel", "learn_hetero_wide_kernel")}, shapes={})
    for name, host in shapes().items():
        if name not in args.shapes.split(","):
            continue
        K, x0 = host["K"], host["x0"]
        d = {k: torch.from_numpy(np.ascontiguousarray(v, np.float64).reshape(-1)).to(dev) for k, v in host.items()
             if k not in ("K", "x0")}
        nc, nu = host["eta"].size, host["u"].size
        n_p, nl, nk = (host[k].size for k in ("p", "lam", "kappa"))

        def new_out(shape):
            o = {k: torch.empty(shape, dtype=torch.float64, device=dev) for k in ("xi", "aw_max", "tol")}
            o["status"] = torch.empty(shape, dtype=torch.int32, device=dev)
            o["iters"] = torch.empty(shape, dtype=torch.int32, device=dev)
            return o

        outs = {"new": new_out((nc, n_p, nl, nk, nu)), "loop": new_out((n_p, nl, nk, nc, nu))}
        combos = [(a, b, c) for a in range(n_p) for b in range(nl) for c in range(nk)]
        slices = {abc: {k: v[abc] for k, v in outs["loop"].items()} for abc in combos}
        hp, hl, hk = (host[k].tolist() for k in ("p", "lam", "kappa"))

        def loop():
            for (a, b, c), o in slices.items():
                eng.sweep_hetero_dev(K, d["betas"], d["dist"], d["eta"], d["t_end"], d["u"], hp[a], hk[c], hl[b], x0, o,
                                     stream=sp, knot_capacity=CAP)

        calls = {"new": lambda: eng.sweep_hetero_econ_dev(K, **d, x0=x0, out=outs["new"], stream=sp,
                                                          knot_capacity=CAP),
                 "loop": loop}
        stream.wait_stream(torch.cuda.current_stream(dev))
        ev = {v: [] for v in calls}
        with torch.cuda.stream(stream):
            for r in range(args.warmup + args.repeats):
                for v in calls:  # (loop) alternates with (new)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    calls[v]()
                    e1.record(stream)
                    if r >= args.warmup:
                        ev[v].append((e0, e1))
        stream.synchronize()
        entry = {v: stats([a.elapsed_time(b) for a, b in ev[v]]) for v in calls}
        entry["K"] = K
        entry["points_total"] = nc * n_p * nl * nk * nu
        entry["combinations"] = len(combos)
        st = outs["new"]["status"].cpu().numpy().view(np.uint32)
        entry["run_points"] = int(((st & sbr.STATUS["SBR_RUN"]) != 0).sum())
        entry["new_equals_loop_bitwise"] = all(same(outs["new"][k], outs["loop"][k].permute(3, 0, 1, 2, 4))
                                               for k in FIELDS)
        entry["loop_over_new"] = entry["loop"]["median_ms"] / entry["new"]["median_ms"]
        entry["fastest_repeat_of_the_loop_ms"] = entry["loop"]["min_ms"]
        entry["new_median_below_it"] = entry["new"]["median_ms"] < entry["loop"]["min_ms"]
        res["shapes"][name] = entry
    eng.close()
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    slim = {s: {k: (v if not isinstance(v, dict) else {q: v[q] for q in ("median_ms", "min_ms", "max_ms")})
                for k, v in e.items()} for s, e in res["shapes"].items()}
    print(json.dumps(slim))


if __name__ == "__main__":
    main()
