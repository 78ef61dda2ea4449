"""bench.py --gpus N starts N rank processes itself when no launcher set WORLD_SIZE (the
driver's scaling runs), refuses a world that disagrees with --gpus, and a launched run reports
n_gpus from the process group.  CPU only: the rank processes join a gloo group."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_plan_two_ranks():
    env = {"PATH": "/usr/bin", "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    plan = bench.launch_plan(["--gpus", "2", "--steps", "3"], env, 29511)
    assert len(plan) == 2
    for r, (cmd, e) in enumerate(plan):
        assert cmd[0] == sys.executable and cmd[-4:] == ["--gpus", "2", "--steps", "3"]
        assert cmd[-5].endswith("bench.py")
        assert (e["WORLD_SIZE"], e["RANK"], e["LOCAL_RANK"]) == ("2", str(r), str(r))
        assert (e["MASTER_ADDR"], e["MASTER_PORT"]) == ("127.0.0.1", "29511")
        assert e["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and e["PATH"] == "/usr/bin"


def test_no_plan_under_a_launcher_or_for_one_gpu():
    assert bench.launch_plan(["--gpus", "8"], {"WORLD_SIZE": "8"}, 1) == []
    assert bench.launch_plan(["--gpus", "1"], {}, 1) == []
    assert bench.launch_plan([], {}, 1) == []


def test_world_must_match_gpus():
    assert bench.world_of(2, {"WORLD_SIZE": "2", "RANK": "1", "LOCAL_RANK": "1"}) == (2, 1, 1)
    assert bench.world_of(1, {}) == (1, 0, 0)
    with pytest.raises(SystemExit):
        bench.world_of(2, {"WORLD_SIZE": "3", "RANK": "0"})
    with pytest.raises(SystemExit):
        bench.world_of(4, {})  # a rank without a launcher's world cannot claim 4 GPUs


@pytest.mark.parametrize("n", [2, 3])
def test_launched_run_reports_the_world(n):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", str(n), "--workload",
                        "launchcheck"], env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1  # rank 0 only
    assert lines[0]["n_gpus"] == n and lines[0]["rank_sum"] == n * (n - 1) // 2
    assert lines[0]["parallelism"] == f"beta-column shards x{n}"


def test_plain_run_switches_off_the_full_legs(monkeypatch):
    """Without --full neither the cpu_baseline leg nor the oracle check runs; with it each is
    still switched off by its own option."""
    def parsed(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        return bench.parse()

    a = parsed("--gpus", "1", "--steps", "3", "--warmup", "1")
    assert not a.full and a.no_cpu_baseline and a.no_verify and a.dump_outputs == ""
    a = parsed("--full")
    assert a.full and not a.no_cpu_baseline and not a.no_verify
    a = parsed("--full", "--no-cpu-baseline", "--dump-outputs", "d")
    assert a.no_cpu_baseline and not a.no_verify and a.dump_outputs == "d"


def test_dump_outputs_writes_exact_float64_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs: finite float64 files, integers widened exactly (status through its unsigned
    view), NaN / inf of a float field coded beside it so that the caller's array is rebuilt exactly;
    a grid past the budget is cut to one seeded sample of points, the same in every field and
    from run to run."""
    import numpy as np
    import torch

    n = 1000
    rng = np.random.default_rng(0)
    xi = rng.random(n)
    xi[::7] = np.nan
    xi[1::7] = np.inf
    xi[2::7] = -np.inf
    fields = {"xi": torch.from_numpy(xi), "status": torch.from_numpy((np.arange(n) - 2 ** 31).astype(np.int32)),
              "iters": np.arange(n, dtype=np.int32)}
    bench.dump_outputs(str(tmp_path / "whole"), fields)
    got = {p.stem: np.load(p) for p in (tmp_path / "whole").glob("*.npy")}
    assert sorted(got) == ["iters", "status", "xi", "xi_nonfinite"]
    assert all(np.isfinite(v).all() for v in got.values())
    assert all(v.dtype == (np.float32 if k == "xi_nonfinite" else np.float64) for k, v in got.items())

    def rebuilt(v, code):
        return np.where(code == 0, v, np.select([code == 1, code == 2, code == 3], [np.nan, np.inf, -np.inf], 0.0))

    assert np.array_equal(rebuilt(got["xi"], got["xi_nonfinite"]), xi, equal_nan=True)
    assert np.array_equal(got["xi"] == 0, ~np.isfinite(xi))
    assert np.array_equal(got["status"], np.arange(n, dtype=np.float64) + 2 ** 31)
    assert np.array_equal(got["iters"], np.arange(n))

    monkeypatch.setattr(bench, "DUMP_BUDGET", (8 * 4 + 4) * 100)  # 100 points: 3 fields, the index, one code
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), fields)
    a = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    b = {p.stem: np.load(p) for p in (tmp_path / "b").glob("*.npy")}
    assert sorted(a) == ["iters", "sample_index", "status", "xi", "xi_nonfinite"]
    assert sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy")) <= (8 * 4 + 4) * 100 + 5 * 128
    idx = a["sample_index"].astype(np.int64)
    assert len(idx) == 100 and len(set(idx)) == 100 and np.all(np.diff(idx) > 0)
    assert np.array_equal(rebuilt(a["xi"], a["xi_nonfinite"]), xi[idx], equal_nan=True)
    assert np.array_equal(a["iters"], idx)
    assert all(np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]) for k in a)


def test_mismatched_world_is_refused():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--workload",
                        "launchcheck"], env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode != 0 and "mismatched world" in p.stderr
