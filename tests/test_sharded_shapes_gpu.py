"""Sharded engines against the unsharded oracle at the shapes of the sharded BASELINE configurations (`-m gpu`).

configs[3] is 10 M cells x 50 PCs, 16 batches, K = 100 over 8 GPUs; configs[4] is 10 M x 200 PCs, 32 batches, K = 200.  Here the
same shapes at 160 000 / 40 000 cells (an update block of 8 000 cells: about 500 tiles, a filled sweep grid, a stream of tiles
per rank), cut unevenly over 1 .. 8 engines that share the one GPU of the box (gloo for the collectives, the peer boxes inside
the persistent sweep for the per-block sums), on the device update order.  The checker is the UNSHARDED OracleHarmony on all
cells, fed the engine's update order through its NumPy restatement (oracle/device_order.py) and the same forced schedule --
computed once per job and reused by every rank count.  Tolerances are those of the single-engine bench path
(test_parity_gpu._bench_path_case): objectives 2e-5, R 1e-4 relative Frobenius, O rtol 1e-4 / atol 2e-3, Y 5e-6, Z_corr 1e-4
after every Harmony iteration; O, E, Y and the objective lists bit-identical on all ranks of a job.

After a case loses a rank (a signal, a time-out, any failure of a rank) the later cases of this file fail at once and start
nothing more on the GPU."""
import os

import numpy as np
import pytest

from _shard_worker import synthetic_job
from conftest import assert_z_close, z_errors
from test_parity_gpu import _device_perm_source
from test_sharded_cpu import launch

pytestmark = pytest.mark.gpu

SEED = 11                                   # the engine seed: keys the device update order
ROUNDS = (3, 2)                             # forced k-means rounds of the two Harmony iterations
C4 = dict(N=160_000, d=50, B=16, K=100)     # configs[3]'s shape
C5 = dict(N=40_000, d=200, B=32, K=200)     # configs[4]'s shape: the wide kernels
OFF = dict(N=30_000, d=100, B=3, K=150)     # a wide shape off the tile sizes

_ORACLES = {}      # job key -> the oracle's snapshots
_STITCHED = {}     # job key -> {label: the last iteration of an engine run}, for the comparison between rank counts
_LOST = []         # the first case that lost a rank


def _key(job, ridge_dtype):
    return tuple(sorted(job.items())) + (np.dtype(ridge_dtype).name,)


def _oracle(job, ridge_dtype):
    """The unsharded oracle over all cells of `job` on the engine's device order: Y0 and, per Harmony iteration, R (cells x K),
    O, Y, the objective list so far and Z_corr."""
    key = _key(job, ridge_dtype)
    if key not in _ORACLES:
        from bench import quick_centroids
        from oracle.harmony_oracle import OracleHarmony, prepare_inputs
        Z, meta = synthetic_job(job)
        N, K = job["N"], job["K"]
        Y0 = quick_centroids(Z, K, seed=3, sample=20_000)
        p = prepare_inputs(Z, meta, ["batch"], nclust=K)
        oo = OracleHarmony(p["Z"], p["phi"], p["Pr_b"], p["sigma"], p["theta"], p["lamb"], K=K, run=False,
                           perm_source=_device_perm_source(N, SEED), forced_rounds=list(ROUNDS), ridge_dtype=ridge_dtype)
        oo.init_cluster(SEED, Y0)
        its = []
        for _ in ROUNDS:
            oo.cluster()
            snap = dict(R=np.ascontiguousarray(oo.R.T), O=oo.O.copy(), Y=oo.Y.copy(), objective_kmeans=list(oo.objective_kmeans))
            oo.moe_correct_ridge()
            snap["Z_corr"] = oo.result().copy()
            its.append(snap)
        _ORACLES[key] = dict(Y0=Y0, its=its, batch=meta["batch"].cat.codes.to_numpy())
    return _ORACLES[key]


def _run(job, cuts, tmp_path, label, timeout):
    """One sharded job on len(cuts) - 1 engines; the per-rank results.  Starts nothing once an earlier case has lost a rank."""
    if _LOST:
        pytest.fail(f"not started: the case '{_LOST[0]}' lost a rank earlier in this file")
    opts = dict(job, cuts=list(cuts), rounds=list(ROUNDS), seed=SEED)
    try:
        return launch("synthetic", label, tmp_path, world=len(cuts) - 1, opts=opts, timeout=timeout)
    except BaseException:
        _LOST.append(label)
        raise


def _check(job, cuts, tmp_path, label, ridge_dtype, timeout, peer=True):
    """Run the job, check every rank and the stitched arrays against the oracle, then against the other rank counts of the job."""
    want = _oracle(job, ridge_dtype)
    np.save(os.path.join(tmp_path, "Y0.npy"), want["Y0"])
    res = _run(job, cuts, tmp_path, label, timeout)
    world = len(res)
    assert [int(r["lo"]) for r in res] == list(cuts[:-1]) and [int(r["hi"]) for r in res] == list(cuts[1:])
    n_obj = 1
    for it, rounds in enumerate(ROUNDS):
        o = want["its"][it]
        n_obj += rounds
        for rk, r in enumerate(res):
            np.testing.assert_allclose(r["objective_kmeans"][:n_obj], o["objective_kmeans"][:n_obj], rtol=2e-5,
                                       err_msg=f"{label}: rank {rk}, iteration {it}")
        R = np.concatenate([r[f"R_{it}"] for r in res], axis=0)
        rel_r = float(np.linalg.norm(R - o["R"]) / np.linalg.norm(o["R"]))
        Z = np.concatenate([r[f"Z_corr_{it}"] for r in res], axis=0)
        rel_f, max_rel = z_errors(Z, o["Z_corr"])
        d_o, d_y = float(np.abs(res[0][f"O_{it}"] - o["O"]).max()), float(np.abs(res[0][f"Y_{it}"] - o["Y"]).max())
        d_obj = float(np.abs(np.asarray(res[0]["objective_kmeans"][:n_obj]) / np.asarray(o["objective_kmeans"][:n_obj]) - 1).max())
        print(f"{label} ({world} ranks) iteration {it}, {rounds} rounds: objectives {d_obj:.2e}  R relF={rel_r:.2e}  max|dO|={d_o:.2e}  "
              f"max|dY|={d_y:.2e}  Z_corr relF={rel_f:.2e} max={max_rel:.2e}")
        assert rel_r <= 1e-4, f"{label}: stitched R after iteration {it}: relF={rel_r:.2e}"
        for rk, r in enumerate(res):
            np.testing.assert_allclose(r[f"O_{it}"], o["O"], rtol=1e-4, atol=2e-3, err_msg=f"{label}: O on rank {rk}, iteration {it}")
            np.testing.assert_allclose(r[f"Y_{it}"], o["Y"], rtol=0, atol=5e-6, err_msg=f"{label}: Y on rank {rk}, iteration {it}")
            for name in ("O", "E", "Y"):
                np.testing.assert_array_equal(r[f"{name}_{it}"], res[0][f"{name}_{it}"], err_msg=f"{label}: {name} on rank {rk} vs rank 0")
        assert_z_close(Z, o["Z_corr"], what=f"{label}: stitched Z_corr after iteration {it}")
    for rk, r in enumerate(res):
        assert list(r["kmeans_rounds"]) == list(ROUNDS)
        for name in ("objective_kmeans", "objective_harmony"):
            np.testing.assert_array_equal(r[name], res[0][name], err_msg=f"{label}: {name} on rank {rk} vs rank 0")
        assert int(r["sweep_fallbacks"]) == 0, f"{label}: rank {rk} fell back {int(r['sweep_fallbacks'])} times"
        if world > 1:
            assert str(r["transport"]) == ("host+peer" if peer else "host"), f"{label}: rank {rk} runs on {r['transport']}"
    print(f"{label}: cells per rank {[int(r['hi']) - int(r['lo']) for r in res]}, batch groups held {[int(r['groups_held']) for r in res]} of "
          f"{int(res[0]['groups'])}, transport {str(res[0]['transport'])}, sweep_waits {[int(r['sweep_waits']) for r in res]}, "
          f"sweeps_bf16_pipe {[int(r['sweeps_bf16_pipe']) for r in res]}, sweeps_group_affine {[int(r['sweeps_group_affine']) for r in res]}")
    # the other rank counts of the same job: each is within the oracle tolerances of the oracle, so two of them are within twice those
    last = len(ROUNDS) - 1
    mine = dict(R=R, Y=res[0][f"Y_{last}"], O=res[0][f"O_{last}"], Z=Z, obj=np.asarray(res[0]["objective_kmeans"]))
    others = _STITCHED.setdefault(_key(job, ridge_dtype), {})
    for other_label, b in others.items():
        rel_r = float(np.linalg.norm(mine["R"] - b["R"]) / np.linalg.norm(b["R"]))
        rel_f, max_rel = z_errors(mine["Z"], b["Z"])
        d_y, d_obj = float(np.abs(mine["Y"] - b["Y"]).max()), float(np.abs(mine["obj"] / b["obj"] - 1).max())
        print(f"{label} vs {other_label}: objectives {d_obj:.2e}  R relF={rel_r:.2e}  max|dY|={d_y:.2e}  Z_corr relF={rel_f:.2e} max={max_rel:.2e}")
        assert d_obj <= 4e-5 and rel_r <= 2e-4 and d_y <= 1e-5 and rel_f <= 2e-4 and max_rel <= 2e-4, f"{label} vs {other_label}"
        np.testing.assert_allclose(mine["O"], b["O"], rtol=2e-4, atol=4e-3)
    others[label] = mine
    return res


# uneven cuts of configs[3]'s 160 000 cells (HMX_ROUND_WGS as in the bench tests of test_sharded_gpu.py: compute workgroups per engine
# such that the persistent sweeps of all engines are resident together on the one GPU)
C4_CUTS = {
    2: (100, [0, 57_143, 160_000]),
    4: (50, [0, 21_001, 70_007, 118_113, 160_000]),
    8: (28, [0, 9_001, 31_013, 50_000, 72_345, 90_017, 115_000, 139_999, 160_000]),
}


@pytest.mark.parametrize("world", [2, 4, 8])
def test_config4_shape_sharded_with_peer_exchange(world, tmp_path, monkeypatch):
    """configs[3]'s shape (160 000 x 50, 16 batches, K = 100: k_round<7,13>, classic tile map) on 2, 4 and 8 engines with uneven
    cuts; the per-block sums travel through the peer boxes inside the persistent sweep (gateway workgroups, 2- / 4- / 8-way flags):
    every rank reports host+peer, no fall-back, grid-wide waits; all numbers against the unsharded oracle (ridge in float64)."""
    wgs, cuts = C4_CUTS[world]
    monkeypatch.setenv("HMX_PEER_EXCHANGE", "1")
    monkeypatch.setenv("HMX_ROUND_WGS", str(wgs))
    res = _check(C4, cuts, tmp_path, f"configs[3] shape, {world} ranks, peer exchange", np.float64, timeout=600 + 60 * world)
    for rk, r in enumerate(res):
        assert int(r["sweep_waits"]) > 0 and int(r["sweeps_group_affine"]) == 0, f"rank {rk}"


def test_config4_shape_sharded_one_collective_per_block(tmp_path, monkeypatch):
    """The same job on 2 engines with HMX_PEER_EXCHANGE=0: one launch and one collective per update block."""
    monkeypatch.setenv("HMX_PEER_EXCHANGE", "0")
    monkeypatch.setenv("HMX_ROUND_WGS", "100")
    _check(C4, C4_CUTS[2][1], tmp_path, "configs[3] shape, 2 ranks, one collective per block", np.float64, timeout=720, peer=False)


def test_config4_shape_cells_ordered_by_batch(tmp_path, monkeypatch):
    """The cells ordered by batch before cutting, 4 engines: a rank holds a few of the 16 batch groups only (job-wide groups, local
    groups without a cell); the oracle gets the same order."""
    monkeypatch.setenv("HMX_PEER_EXCHANGE", "1")
    monkeypatch.setenv("HMX_ROUND_WGS", "50")
    job = dict(C4, sort_by_batch=1)
    res = _check(job, [0, 30_000, 65_000, 107_000, 160_000], tmp_path, "configs[3] shape by batch, 4 ranks", np.float64, timeout=840)
    held = [int(r["groups_held"]) for r in res]
    batch = _oracle(job, np.float64)["batch"]
    assert held == [np.unique(batch[int(r["lo"]):int(r["hi"])]).size for r in res] and all(int(r["groups"]) == 16 for r in res)
    assert max(held) <= 6 and sum(3 <= h <= 5 for h in held) >= 3, held     # (4, 4, 5 and 6 of the sixteen groups)
    for rk, r in enumerate(res):
        assert int(r["sweep_waits"]) > 0, f"rank {rk}"


def test_config4_shape_one_rank_of_37_cells(tmp_path, monkeypatch):
    """3 engines, the middle one with 37 cells: its share of most update blocks is empty or below one tile."""
    monkeypatch.setenv("HMX_PEER_EXCHANGE", "1")
    monkeypatch.setenv("HMX_ROUND_WGS", "50")
    res = _check(C4, [0, 70_001, 70_038, 160_000], tmp_path, "configs[3] shape, 3 ranks, one of 37 cells", np.float64, timeout=780)
    assert int(res[1]["hi"]) - int(res[1]["lo"]) == 37
    for rk, r in enumerate(res):
        assert int(r["sweep_waits"]) > 0, f"rank {rk}"


def test_config4_shape_world_of_one(tmp_path, monkeypatch):
    """`Shard` with a world of one: the sharded code path (classic map, collectives, saved O) without a partner."""
    monkeypatch.setenv("HMX_ROUND_WGS", "100")
    res = _check(C4, [0, 160_000], tmp_path, "configs[3] shape, world of one", np.float64, timeout=600)
    assert str(res[0]["transport"]).startswith("host") and int(res[0]["sweeps_group_affine"]) == 0, res[0]["transport"]


@pytest.mark.parametrize("name,job,cuts", [("configs[4] shape", C5, [0, 14_286, 40_000]), ("30 000 x 100, K = 150", OFF, [0, 10_715, 30_000])])
def test_wide_shapes_sharded(name, job, cuts, tmp_path, monkeypatch):
    """Wide shapes (K > 112 or d > 64) on 2 engines: a sharded engine has no persistent wide sweep, so every update block is one
    k_assign_wide3 launch with a collective behind it; the streaming R^T.Z pass is k_rtzw2b.  Oracle in its plain fp32 mode, as
    test_bench_path_parity_c5_shape uses at configs[4]'s shape (float64 ridge at the other one, as everywhere else).  The counters
    say the bf16-pipe instances ran in every sweep."""
    monkeypatch.setenv("HMX_PEER_EXCHANGE", "1")
    res = _check(job, cuts, tmp_path, f"{name}, 2 ranks", np.float32 if job is C5 else np.float64, timeout=900)
    for rk, r in enumerate(res):
        assert int(r["sweeps_bf16_pipe"]) == sum(ROUNDS) and int(r["rtz_bf16_pipe"]) > 0, (rk, int(r["sweeps_bf16_pipe"]), int(r["rtz_bf16_pipe"]))
