"""Timing of the group-looped heterogeneity equilibrium path (not part of bench.py).

On sbr.hetero_config4(256, 256, K) (65,536 equilibria), device tensors, sweep_hetero_dev:
  (a) K = 8: the specialised kernels (wide=False) alternating with SBR_FLAG_HETERO_WIDE
      (wide=True) in the same process — what the LDS-resident group state and the every-knot
      AW_max / validity pass cost against equilibrium_hetero_kernel<8>;
  (b) K = 5, 12, 16 (no specialised kernel: the wide path) beside the CPU oracle's OpenMP sweep
      of the same grid on this host's CPUs (bench.py's cpu_baseline convention: one timed call),
      with the bitwise comparison of the two.
Each GPU variant: 5 warm-up and 20 timed calls on one stream, timed with device events around
each call, a synchronise at the end.  Reports medians and spreads; writes
profiles/hetero_wide_bench.json and prints a summary line.
"""
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "replication-social-bank-runs_amd"))
sys.path.insert(0, str(REPO / "oracle"))
import oracle as O  # noqa: E402
import sbr  # noqa: E402
from sbr import provenance  # noqa: E402

WARMUP, REPEATS, N_S, N_U = 5, 20, 256, 256
FIELDS = ("xi", "aw_max", "tol", "status", "iters")


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
    threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or min(16, os.cpu_count() or 1)
    res = dict(tool="tools/hetero_wide_bench.py", warmup=WARMUP, repeats=REPEATS, grid=[N_S, N_U],
               device=torch.cuda.get_device_name(dev), oracle_threads=threads,
               code_sha={k: provenance.kernel_code_sha(k) for k in
                         ("equilibrium_hetero_wide_kernel", "equilibrium_hetero_kernel", "learn_hetero_wide_kernel",
                          "learn_hetero_wave_kernel")}, K={})

    def run(K, variants, oracle):
        g = sbr.hetero_config4(N_S, N_U, K)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        d = dict(betas=t(g.betas), dist=t(g.dist), eta=t(g.eta), t_end=t(g.t_end), u=t(g.u))
        n = g.n_points

        def new_out():
            o = {k: torch.empty(n, dtype=torch.float64, device=dev) for k in ("xi", "aw_max", "tol")}
            o["status"] = torch.empty(n, dtype=torch.int32, device=dev)
            o["iters"] = torch.empty(n, dtype=torch.int32, device=dev)
            return o

        outs = {v: new_out() for v in variants}
        call = lambda v: eng.sweep_hetero_dev(K, d["betas"], d["dist"], d["eta"], d["t_end"], d["u"], g.p, g.kappa,  # noqa: E731
                                              g.lam, g.x0, outs[v], stream=sp, wide=variants[v])
        stream.wait_stream(torch.cuda.current_stream(dev))
        ev = {v: [] for v in variants}
        with torch.cuda.stream(stream):
            for r in range(WARMUP + REPEATS):
                for v in variants:  # the variants alternate
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    call(v)
                    e1.record(stream)
                    if r >= WARMUP:
                        ev[v].append((e0, e1))
        stream.synchronize()
        entry = {v: stats([a.elapsed_time(b) for a, b in ev[v]]) for v in variants}
        host = {v: {k: outs[v][k].cpu().numpy() for k in FIELDS} for v in variants}
        for v in variants:
            host[v]["status"] = host[v]["status"].view(np.uint32)
            entry[v]["run_points"] = int(((host[v]["status"] & sbr.STATUS["SBR_RUN"]) != 0).sum())
        same = lambda x, y: bool(((x == y) | ((x != x) & (y != y))).all())  # noqa: E731
        names = list(variants)
        if len(names) == 2:
            entry["variants_equal_bitwise"] = all(same(host[names[0]][k], host[names[1]][k]) for k in FIELDS)
            entry["wide_over_specialised"] = entry["wide"]["median_ms"] / entry["specialised"]["median_ms"]
        if oracle:
            t0 = time.perf_counter()
            o = O.sweep_hetero(g.betas, g.dist, g.eta, g.t_end, g.u, g.p, g.kappa, g.lam, g.x0, nthreads=threads)
            entry["oracle_ms"] = (time.perf_counter() - t0) * 1e3
            entry["gpu_equals_oracle_bitwise"] = all(same(host[names[0]][k], o[k].ravel()) for k in FIELDS)
            entry["oracle_over_gpu"] = entry["oracle_ms"] / entry[names[0]]["median_ms"]
        res["K"][str(K)] = entry

    run(8, {"specialised": False, "wide": True}, oracle=False)
    for K in (5, 12, 16):
        run(K, {"wide": False}, oracle=True)  # no specialised kernel at these K: the wide path
    eng.close()
    out = REPO / "profiles" / "hetero_wide_bench.json"
    out.write_text(json.dumps(res, indent=1) + "\n")
    slim = {K: {k: (v if not isinstance(v, dict) else {f: v[f] for f in ("median_ms", "min_ms", "max_ms")})
                for k, v in e.items()} for K, e in res["K"].items()}
    print(json.dumps(slim))


if __name__ == "__main__":
    main()
