"""bench.py's launcher logic without a GPU: `--gpus N` starts its own ranks, picks the job BASELINE.json names for
several GPUs, and refuses to print a figure for a GPU count it did not run on.  `--dump-outputs` against a stub engine;
one plain run with a dump on the GPU."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_workload_resolution():
    import bench
    assert bench.resolve_workload(None, 1) == ("c3", 1_000_000, "weak")            # the N=1 headline: configs[2]
    assert bench.resolve_workload(None, 8) == ("c4", 1_250_000, "strong")          # configs[3]: 10M cells over 8 GPUs
    assert bench.resolve_workload(None, 2) == ("c4", 5_000_000, "strong")
    assert bench.resolve_workload("c5", 4) == ("c5", 2_500_000, "strong")          # configs[4]
    assert bench.resolve_workload("c3", 4) == ("c3", 1_000_000, "weak")
    assert bench.resolve_workload("c5", 1) == ("c5", 1_250_000, "weak")            # one GPU: the 8-GPU shard


def test_self_launch_command():
    import bench
    cmd = bench.self_launch(["--gpus", "4", "--steps", "3"], 4)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    i = cmd.index("--master-addr")
    assert cmd[i + 1] == "127.0.0.1" and 1024 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"] and cmd[-5].endswith("bench.py")


def _run(args, env_extra):
    env = dict(os.environ, **env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env, timeout=600)


def test_mismatched_world_size_is_an_error():
    """Launched with WORLD_SIZE=1 but --gpus 2 (how the round-2 line came to say n_gpus: 1): non-zero exit, no JSON line."""
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and r.stdout.strip() == "" and "refusing" in r.stderr


def test_missing_gpus_are_an_error():
    """No (or too few) devices: exit code 3 instead of a line for fewer GPUs.  (Runs on the CPU-only build container.)"""
    import torch
    if torch.cuda.device_count() >= 1:
        import pytest
        pytest.skip("a GPU is visible")
    r = _run(["--gpus", "1", "--steps", "1", "--warmup", "0"], {})
    assert r.returncode == 3 and r.stdout.strip() == "" and "visible" in r.stderr


def test_new_options_and_step_count_check():
    """`--full` and `--dump-outputs` exist; a step count below one is refused before any work."""
    r = _run(["--help"], {})
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = _run(["--gpus", "1", "--steps", "0"], {})
    assert r.returncode == 2 and "--steps" in r.stderr


class _StubEngine:
    def __init__(self, N, d, K):
        self.cols = {"z": d, "r": K}

    def get_rows(self, which, rows):
        from harmonypy_amd import _capi
        import numpy as np
        cols = self.cols["z"] if which == _capi.HMX_Z_CORR else self.cols["r"]
        return np.repeat(np.asarray(rows, np.float32)[:, None], cols, axis=1)


class _StubHarmony:
    """What dump_outputs reads of a Harmony object, at a shape without a GPU: row j of the engine holds cell order[j]."""
    def __init__(self, N, d, K, B, rounds):
        import numpy as np
        self.N, self.d, self.K = N, d, K
        order = np.random.default_rng(1).permutation(N)
        self._rank = np.empty(N, np.int64)
        self._rank[order] = np.arange(N)
        self._engine = _StubEngine(N, d, K)
        self.Y = np.zeros((d, K), np.float32)
        self.O = self.E = np.zeros((K, B), np.float32)
        self.kmeans_rounds = [rounds, rounds]
        hist = list(np.arange(2 * rounds, dtype=np.float64))
        self.objective_kmeans = self.objective_kmeans_dist = self.objective_kmeans_entropy = self.objective_kmeans_cross = hist
        self.objective_harmony = [hist[rounds - 1], hist[-1]]


def test_dump_outputs_budget_and_sample(tmp_path):
    """At the widest configuration (configs[4] shard: 1.25 M cells, d = K = 200) the dump stays within 64 MB, every file is
    float32 / float64, the sampled rows are the same in every run and are fetched from the engine rows of those cells, and
    the histories are the last step's."""
    import numpy as np
    import bench
    N, d, B, K = bench.CONFIGS["c5"]
    files = {}
    for run in ("a", "b"):
        bench.dump_outputs(_StubHarmony(N, d, K, B, rounds=10), str(tmp_path / run))
        files[run] = {f.name: np.load(f) for f in sorted((tmp_path / run).iterdir())}
    total = sum(f.stat().st_size for f in (tmp_path / "a").iterdir())
    assert total <= 64 << 20, total
    a, b = files["a"], files["b"]
    assert set(a) == {"Z_corr_sample.npy", "R_sample.npy", "Y.npy", "O.npy", "E.npy", "objective_harmony.npy",
                      "objective_kmeans.npy", "objective_kmeans_dist.npy", "objective_kmeans_entropy.npy",
                      "objective_kmeans_cross.npy"}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    np.testing.assert_array_equal(a["Z_corr_sample.npy"], b["Z_corr_sample.npy"])
    z = a["Z_corr_sample.npy"]
    assert z.shape[1] == d and a["R_sample.npy"].shape == (z.shape[0], K) and 10_000 < z.shape[0] <= 65_536
    # the stub's rows carry the engine row they came from: the caller's cells, sorted, map onto them through _rank
    cells = np.sort(np.random.default_rng(0).choice(N, size=z.shape[0], replace=False))
    np.testing.assert_array_equal(z[:, 0], _StubHarmony(N, d, K, B, 10)._rank[cells].astype(np.float32))
    np.testing.assert_array_equal(a["objective_kmeans.npy"], np.arange(10, 20, dtype=np.float64))
    np.testing.assert_array_equal(a["objective_harmony.npy"], [19.0])


@pytest.mark.gpu
def test_plain_run_and_dump_outputs(tmp_path):
    """A plain run times exactly --steps steps and prints the contract fields without the --full diagnostics; its dump
    holds the last step's Z_corr / R sample, centroids, O, E and objective entries of that step."""
    import json
    import numpy as np
    out = tmp_path / "out"
    r = _run(["--gpus", "1", "--config", "c2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)], {})
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0
    assert not {"roofline", "convergence", "lisi", "cpu_baseline", "configs_1"} & set(line)
    N, d, B, K = 69_000, 50, 4, 30
    a = {f.stem: np.load(f) for f in out.iterdir()}
    assert sum(f.stat().st_size for f in out.iterdir()) <= 64 << 20
    assert a["Z_corr_sample"].shape == (65_536, d) and a["R_sample"].shape == (65_536, K)
    assert a["Y"].shape == (d, K) and a["O"].shape == (K, B) and a["E"].shape == (K, B)
    assert all(np.isfinite(x).all() for x in a.values())
    np.testing.assert_allclose(a["R_sample"].sum(axis=1), 1.0, atol=1e-4)
    assert a["objective_kmeans"].shape == (10,) and a["objective_harmony"][0] == a["objective_kmeans"][-1]
