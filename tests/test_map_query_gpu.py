"""Reference mapping on the MI355X: hmx_reference_summary / hmx_map_query against the existing kernels (bit for bit) and
against the float64 restatement tests/map_oracle.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import map_oracle as MO
from conftest import ROOT, assert_z_close, load_case

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def _pbmc(vars_use):
    """Donor A mapped onto an oracle reference of donors B and C: (HarmonyReference, query data, query meta, oracle
    inputs of the query)."""
    from harmonypy_amd import HarmonyReference
    from test_map_query_cpu import pbmc_split
    oo, p, q_meta, Xq = pbmc_split(list(vars_use))
    S, m = MO.reference_summary(oo.R, oo.Z_corr)
    return HarmonyReference(S, m, oo.sigma, oo.N), Xq, q_meta, p


def _synthetic_wide(N_ref=4000, N=3000, d=20, K=120, seed=5):
    """A reference summary and a query for the wide regime (K > 112): clusters around K random directions."""
    from harmonypy_amd import HarmonyReference
    rng = np.random.default_rng(seed)
    dirs = rng.normal(size=(K, d))
    lab = rng.integers(0, K, size=N_ref)
    Zr = dirs[lab] * 3 + rng.normal(size=(N_ref, d)) * 0.3
    R = np.full((N_ref, K), 0.01 / K)
    R[np.arange(N_ref), lab] += 0.99
    ref = HarmonyReference.from_arrays(R, Zr, 0.1)
    lq = rng.integers(0, K, size=N)
    batch = rng.integers(0, 3, size=N)
    Xq = (dirs[lq] * 3 + rng.normal(size=(N, d)) * 0.3 + batch[:, None] * 0.4).astype(np.float32)
    meta = pd.DataFrame({"batch": [f"b{b}" for b in batch]})
    return ref, Xq, meta


def _oracle_map(Xq, meta, ref, vars_use, lamb=None):
    from oracle.harmony_oracle import prepare_inputs
    p = prepare_inputs(Xq, meta, vars_use, lamb=lamb, nclust=ref.K)
    return MO.map_query(p["Z"], p["phi"], p["Pr_b"], ref.cluster_sums, ref.cluster_mass, ref.sigma, p["lamb"],
                        p["lambda_estimation"], 0.2)


# ---------------------------------------------------------------------------------------------------------------------
# the mapping is the existing assignment and ridge with two terms added
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["one_var", "two_vars", "wide"])
def test_map_is_the_existing_path_plus_reference_terms(shape):
    """hmx_map_query's assignment is init_cluster(cluster_sums as float32 rows) bit for bit, and the reference terms
    hold for that call only: a plain ridge afterwards is bit-identical to init_cluster + moe_correct_ridge on a second
    engine with the same upload (v1 solve for one variable, the general solve for two, wide kernels for K > 112).

    (A literal zero reference cannot be mapped onto: its centroids are the sums at unit length.)"""
    from harmonypy_amd import map_query
    if shape == "wide":
        ref, Xq, meta = _synthetic_wide()
        vars_use = "batch"
    else:
        vars_use = ("donor",) if shape == "one_var" else ("donor", "tech")
        ref, Xq, meta, _ = _pbmc(vars_use)
        vars_use = list(vars_use)
    a = map_query(Xq, meta, ref, vars_use=vars_use, verbose=False)
    b = map_query(Xq, meta, ref, vars_use=vars_use, verbose=False)
    if shape == "wide":
        assert a.K > 112
    else:
        assert a._engine.V == (1 if shape == "one_var" else 2)
    Z_mapped = a.Z_corr
    # b: the same upload again (the map rewrote Z_cos, which the assignment reads), then the existing two steps
    b._upload(np.ascontiguousarray(Xq.T, dtype=np.float32), b._lamb)
    b._engine.enable_timing(True)
    b._engine.init_cluster(ref.cluster_sums.astype(np.float32))
    np.testing.assert_array_equal(a.R, b.R)
    from harmonypy_amd import _capi
    # O and T: the wide assignment adds its float64 group sums with atomics, in no fixed order (so does a second
    # init_cluster on the same engine): equal to the last ulp
    np.testing.assert_allclose(a._engine.get(_capi.HMX_O_GROUP), b._engine.get(_capi.HMX_O_GROUP), rtol=1e-14)
    np.testing.assert_allclose(a._engine.get(_capi.HMX_T_MASS), b._engine.get(_capi.HMX_T_MASS), rtol=1e-14)
    b._engine.moe_correct_ridge()
    times = b._engine.kernel_times()
    assert times["assign_init"][1] == 1 and times["ridge_solve"][1] == 1 and times["ridge_apply"][1] >= 1, times
    a._engine.moe_correct_ridge()
    for name in ("Z_corr", "Z_cos", "R"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)
    assert not np.array_equal(Z_mapped, a.Z_corr)                            # the reference terms did act on the map


# ---------------------------------------------------------------------------------------------------------------------
# the reference summary
# ---------------------------------------------------------------------------------------------------------------------
def _pbmc_default_run():
    from harmonypy_amd import harmony as H
    data, meta, vars_use, kw, g = load_case("pbmc_default")
    ho = H.run_harmony(data, meta, vars_use, verbose=False, _y0=g["Y0"],
                       _schedule=[int(r) for r in g["kmeans_rounds"]], **kw)
    return ho, g


def test_reference_summary_pbmc_default():
    torch = _torch()
    ho, g = _pbmc_default_run()
    ref = ho.reference()
    R, Z = ho.R.astype(np.float64), ho.Z_corr.astype(np.float64)
    S = R.T @ Z
    np.testing.assert_allclose(ref.cluster_sums, S, rtol=1e-5, atol=1e-5 * np.abs(S).max())
    np.testing.assert_allclose(ref.cluster_mass, R.sum(axis=0), rtol=1e-5)
    np.testing.assert_allclose(ref.cluster_mass, g["R_colsum"], rtol=3e-4, atol=3e-4)
    assert ref.n_cells == ho.N_global and ref.K == ho.K and ref.d == ho.d
    np.testing.assert_array_equal(ref.sigma, ho.sigma)
    # the engine stays drivable: a further iteration is the same with or without the summary in between
    other, _ = _pbmc_default_run()
    torch.manual_seed(7)
    ho.harmonize(1, verbose=False)
    torch.manual_seed(7)
    other.harmonize(1, verbose=False)
    for name in ("Z_corr", "R"):
        np.testing.assert_array_equal(getattr(ho, name), getattr(other, name), err_msg=name)
    assert ho.objective_harmony == other.objective_harmony


# ---------------------------------------------------------------------------------------------------------------------
# against the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["donor", "donor_tech", "lambda_est", "wide"])
def test_mapping_matches_oracle(case):
    from harmonypy_amd import map_query
    lamb = -1 if case == "lambda_est" else None
    if case == "wide":
        ref, Xq, meta = _synthetic_wide()
        vars_use = ["batch"]
    else:
        vu = ("donor", "tech") if case == "donor_tech" else ("donor",)
        ref, Xq, meta, _ = _pbmc(vu)
        vars_use = list(vu)
    q = map_query(Xq, meta, ref, vars_use=vars_use, lamb=lamb, verbose=False)
    R, X_corr, X_cos = _oracle_map(Xq, meta, ref, vars_use, lamb)
    np.testing.assert_allclose(q.R, R.T, rtol=2e-4, atol=1e-7)
    assert_z_close(q.Z_corr, X_corr.T, what="Z_corr")
    assert_z_close(q.Z_cos, X_cos.T, what="Z_cos")
    assert q.lambda_estimation == (lamb == -1)
    assert q.Y.shape == (q.d, q.K) and q.result().shape == (q.N, q.d)


def test_map_onto_a_finished_harmony_object():
    """reference= a finished Harmony: its device summary is used."""
    from harmonypy_amd import map_query
    ho, _ = _pbmc_default_run()
    data, meta, _, _, _ = load_case("pbmc_default")
    ref = ho.reference()
    a = map_query(data[:500], meta.iloc[:500].reset_index(drop=True), ho, vars_use="donor", verbose=False)
    b = map_query(data[:500], meta.iloc[:500].reset_index(drop=True), ref, vars_use="donor", verbose=False)
    np.testing.assert_array_equal(a.Z_corr, b.Z_corr)


# ---------------------------------------------------------------------------------------------------------------------
# device input and output
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["float32", "bfloat16", "float64", "float32_T"])
def test_device_input_matches_numpy_input(layout):
    from harmonypy_amd import map_query
    torch = _torch()
    ref, Xq, meta, _ = _pbmc(("donor", "tech"))
    dt = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float64": torch.float64, "float32_T": torch.float32}[layout]
    if layout == "float32_T":
        x = torch.from_numpy(np.ascontiguousarray(Xq.T)).to("cuda").T          # cells x d view of a d x cells tensor
    else:
        x = torch.from_numpy(Xq).to("cuda").to(dt)
    same = x.float().cpu().numpy()
    qd = map_query(x, meta, ref, vars_use=["donor", "tech"], verbose=False)
    qh = map_query(same, meta, ref, vars_use=["donor", "tech"], verbose=False)
    for name in ("Z_corr", "R", "Z_cos"):
        np.testing.assert_array_equal(getattr(qd, name), getattr(qh, name), err_msg=name)
        np.testing.assert_array_equal(qd.to_tensor(name).cpu().numpy(), getattr(qh, name), err_msg=name)
    with pytest.raises(ValueError):
        map_query(x, meta, ref, vars_use=["donor", "tech"], verbose=False, device="cuda:1")


# ---------------------------------------------------------------------------------------------------------------------
# edge sizes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["one_cell", "17_cells", "unused_level"])
def test_edge_sizes(case):
    from harmonypy_amd import map_query
    ref, Xq, meta, _ = _pbmc(("donor", "tech"))
    vars_use = ["tech"]
    if case == "one_cell":
        Xq, meta = Xq[:1], meta.iloc[:1].reset_index(drop=True)
    elif case == "17_cells":
        Xq, meta = Xq[:17], meta.iloc[:17].reset_index(drop=True)
    else:
        meta = meta.assign(tech=pd.Categorical(meta["tech"], categories=["v0", "v1", "v2", "v3", "v4"]))
    q = map_query(Xq, meta, ref, vars_use=vars_use, verbose=False)
    # the oracle sees the levels in use only: a declared level without cells must change nothing
    R, X_corr, X_cos = _oracle_map(Xq, meta.assign(tech=meta["tech"].astype(str)), ref, vars_use)
    assert q.B == len(set(meta["tech"].astype(str)))
    assert q.N == Xq.shape[0] and q.R.shape == (q.N, ref.K)
    np.testing.assert_allclose(q.R, R.T, rtol=2e-4, atol=1e-7)
    assert_z_close(q.Z_corr, X_corr.T, what="Z_corr")
    assert_z_close(q.Z_cos, X_cos.T, what="Z_cos")


# ---------------------------------------------------------------------------------------------------------------------
# a sharded reference: every rank gets the whole job's summary
# ---------------------------------------------------------------------------------------------------------------------
def test_sharded_reference_summary(tmp_path):
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="2", GLOO_SOCKET_IFNAME="lo")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_map_shard_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(out.decode(errors="replace"))
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed:\n{logs[r][-4000:]}"
    parts = [dict(np.load(os.path.join(tmp_path, f"rank{r}.npz"), allow_pickle=False)) for r in range(2)]
    for name in ("cluster_sums", "cluster_mass"):
        assert parts[0][name].tobytes() == parts[1][name].tobytes(), name
    assert int(parts[0]["n_cells"]) == int(parts[1]["n_cells"]) == 3500
    R = np.concatenate([p["R"] for p in parts]).astype(np.float64)
    Z = np.concatenate([p["Z_corr"] for p in parts]).astype(np.float64)
    S = R.T @ Z
    np.testing.assert_allclose(parts[0]["cluster_sums"], S, rtol=1e-5, atol=1e-5 * np.abs(S).max())
    np.testing.assert_allclose(parts[0]["cluster_mass"], R.sum(axis=0), rtol=1e-5)
