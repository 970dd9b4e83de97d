"""Reference mapping without a GPU: the float64 restatement (tests/map_oracle.py) against the Harmony oracle, the closed
forms the solve kernels evaluate, the HarmonyReference file format, map_query's argument checks and the export list."""
import os
import re

import numpy as np
import pandas as pd
import pytest

import map_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _pbmc():
    inp = np.load(os.path.join(GOLDEN, "pbmc_3500_inputs.npz"))
    meta = pd.DataFrame({"donor": inp["donor"].astype(str), "tech": inp["tech"].astype(str)})
    return inp["pcs"].astype(np.float32), meta


def _onehot(codes, n):
    Phi = np.zeros((n, len(codes)))
    Phi[codes, np.arange(len(codes))] = 1
    return Phi


def _random_problem(rng, N=400, d=12, K=6, levels=(3,)):
    X = rng.normal(size=(d, N)) + 2.0
    R = rng.random((K, N)) ** 3
    R /= R.sum(axis=0)
    codes = [rng.integers(0, L, size=N) for L in levels]
    Phi = np.concatenate([_onehot(c, L) for c, L in zip(codes, levels)], axis=0)
    return X, R, Phi, codes


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_vars", [False, True])
def test_zero_reference_is_the_oracle_ridge(two_vars):
    """No reference terms: map_oracle.correct is oracle/harmony_oracle.py's moe_correct_ridge (harmony.py:535-569)."""
    from oracle.harmony_oracle import OracleHarmony
    rng = np.random.default_rng(3)
    X, R, Phi, _ = _random_problem(rng, levels=(3, 2) if two_vars else (4,))
    B = Phi.shape[0]
    lamb = np.concatenate([[0.0], rng.uniform(0.5, 2.0, B)]).astype(np.float32)
    Pr_b = (Phi.sum(axis=1) / Phi.shape[1]).astype(np.float32)
    oo = OracleHarmony(X.astype(np.float32), Phi.astype(np.float32), Pr_b, np.full(R.shape[0], 0.1, np.float32),
                       np.zeros(B, np.float32), lamb, K=R.shape[0], run=False, ridge_dtype=np.float64)
    oo.R = R.astype(np.float32)
    oo.moe_correct_ridge()
    K = R.shape[0]
    X_corr, X_cos, _ = MO.correct(oo.Z_orig, oo.R, oo.Phi, MO.lambdas(oo.R, Pr_b, lamb, False, 0.2),
                                  np.zeros((K, X.shape[0])), np.zeros(K))
    rel = np.linalg.norm(X_corr - oo.Z_corr) / np.linalg.norm(oo.Z_corr)
    assert rel < 1e-6, rel          # the oracle rounds Z_corr to float32 at the end
    X_plain, _, _ = MO.correct(oo.Z_orig, oo.R, oo.Phi, MO.lambdas(oo.R, Pr_b, lamb, False, 0.2))
    assert np.linalg.norm(X_plain - X_corr) / np.linalg.norm(X_corr) < 1e-10


@pytest.mark.parametrize("case", ["one_var", "two_vars", "lambda_est"])
def test_closed_forms_equal_dense_solve(case):
    """The arrowhead form of k_ridge_solve_v1 and the group-table system of k_ridge_solve_general, with reference terms,
    equal the dense per-cluster solve."""
    rng = np.random.default_rng(11)
    levels = (3, 2) if case == "two_vars" else (4,)
    X, R, Phi, codes = _random_problem(rng, levels=levels)
    K, d = R.shape[0], X.shape[0]
    B = Phi.shape[0]
    ref_sums = rng.normal(size=(K, d)) * 300
    ref_mass = rng.uniform(50, 500, K)
    Pr_b = Phi.sum(axis=1) / Phi.shape[1]
    lamb = np.concatenate([[0.0], rng.uniform(0.5, 2.0, B)])
    lam = MO.lambdas(R, Pr_b, lamb, case == "lambda_est", 0.2)
    _, _, W_dense = MO.correct(X, R, Phi, lam, ref_sums, ref_mass)
    # group tables as the statistics pass leaves them
    combos, gid = np.unique(np.stack(codes, axis=1) + np.cumsum([0] + list(levels[:-1])), axis=0, return_inverse=True)
    gid = gid.reshape(-1)
    for k in range(K):
        O_g = np.array([R[k, gid == g].sum() for g in range(len(combos))])
        S_g = np.array([(X[:, gid == g] * R[k, gid == g]).sum(axis=1) for g in range(len(combos))])
        if case != "two_vars":
            O_b = np.zeros(B)
            S_b = np.zeros((B, d))
            O_b[combos[:, 0]] = O_g
            S_b[combos[:, 0]] = S_g
            W = MO.arrowhead_v1(S_b, O_b, lam[k], ref_sums[k], ref_mass[k])
        else:
            W = MO.general_system(S_g, O_g, combos, B, lam[k], ref_sums[k], ref_mass[k])
        np.testing.assert_allclose(W, W_dense[k], rtol=1e-9, atol=1e-9 * np.abs(W_dense[k]).max())


# ---------------------------------------------------------------------------------------------------------------------
# HarmonyReference
# ---------------------------------------------------------------------------------------------------------------------
def _reference(rng, K=7, d=5):
    from harmonypy_amd import HarmonyReference
    return HarmonyReference(rng.normal(size=(K, d)), rng.uniform(1, 9, K), rng.uniform(0.05, 0.2, K), 1234)


def test_reference_save_load_round_trip(tmp_path):
    from harmonypy_amd import HarmonyReference
    ref = _reference(np.random.default_rng(0))
    path = str(tmp_path / "ref.npz")
    ref.save(path)
    back = HarmonyReference.load(path)
    for name in ("cluster_sums", "cluster_mass", "sigma"):
        a, b = getattr(ref, name), getattr(back, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert back.n_cells == 1234 and back.K == 7 and back.d == 5
    assert back.centroids.dtype == np.float32 and back.centroids.shape == (7, 5)
    np.testing.assert_allclose(np.linalg.norm(back.centroids, axis=1), 1.0, rtol=1e-6)


@pytest.mark.parametrize("damage", ["sums_shape", "mass_shape", "sigma_dtype", "sums_dtype", "version", "extra", "missing"])
def test_reference_load_rejects_bad_files(tmp_path, damage):
    from harmonypy_amd import HarmonyReference
    ref = _reference(np.random.default_rng(1))
    a = dict(format_version=np.int64(1), cluster_sums=ref.cluster_sums, cluster_mass=ref.cluster_mass, sigma=ref.sigma,
             n_cells=np.int64(ref.n_cells))
    if damage == "sums_shape":
        a["cluster_sums"] = ref.cluster_sums[:-1]
    elif damage == "mass_shape":
        a["cluster_mass"] = ref.cluster_mass[:, None]
    elif damage == "sigma_dtype":
        a["sigma"] = ref.sigma.astype(np.float64)
    elif damage == "sums_dtype":
        a["cluster_sums"] = ref.cluster_sums.astype(np.float32)
    elif damage == "version":
        a["format_version"] = np.int64(2)
    elif damage == "extra":
        a["Y"] = ref.cluster_sums
    else:
        del a["sigma"]
    path = str(tmp_path / "bad.npz")
    np.savez(path, **a)
    with pytest.raises(ValueError):
        HarmonyReference.load(path)


def test_reference_from_arrays():
    from harmonypy_amd import HarmonyReference
    rng = np.random.default_rng(2)
    R = rng.random((300, 9)).astype(np.float32)
    Z = rng.normal(size=(300, 4)).astype(np.float32)
    ref = HarmonyReference.from_arrays(R, Z, 0.1)
    S = np.zeros((9, 4))
    for i in range(300):
        S += np.outer(R[i].astype(np.float64), Z[i].astype(np.float64))
    np.testing.assert_allclose(ref.cluster_sums, S, rtol=1e-12)
    np.testing.assert_allclose(ref.cluster_mass, R.astype(np.float64).sum(axis=0), rtol=1e-12)
    assert ref.sigma.dtype == np.float32 and ref.sigma.shape == (9,) and ref.n_cells == 300
    assert ref.cluster_sums.dtype == np.float64 and ref.cluster_mass.dtype == np.float64


# ---------------------------------------------------------------------------------------------------------------------
# map_query's arguments: every error before an engine exists (no GPU here: an engine would fail differently)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["d", "cells", "vars_use", "sigma", "device"])
def test_map_query_argument_errors(bad):
    from harmonypy_amd import map_query
    rng = np.random.default_rng(4)
    ref = _reference(rng, K=7, d=5)
    X = rng.normal(size=(40, 5)).astype(np.float32)
    meta = pd.DataFrame({"b": ["x", "y"] * 20})
    kw = dict(vars_use="b", verbose=False)
    if bad == "d":
        X = X[:, :4]
    elif bad == "cells":
        meta = meta.iloc[:39]
    elif bad == "vars_use":
        kw["vars_use"] = ["b", "nope"]
    elif bad == "sigma":
        kw["sigma"] = np.full(6, 0.1)
    else:
        kw["device"] = "cpu"
    with pytest.raises(ValueError):
        map_query(X, meta, ref, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the export list
# ---------------------------------------------------------------------------------------------------------------------
def test_map_exports_match_header_and_library():
    from harmonypy_amd import _capi
    src = open(os.path.join(ROOT, "include", "hmx_map.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(hmx_\w+)\(", src))
    assert set(_capi.MAP_EXPORTS) == declared and len(_capi.MAP_EXPORTS) == len(declared)
    assert not set(_capi.MAP_EXPORTS) & set(_capi.EXPORTS)
    assert not set(_capi.MAP_EXPORTS) & set(_capi.DEVICE_IO_EXPORTS)
    lib = _capi.load()
    for name in _capi.MAP_EXPORTS:
        getattr(lib, name)


# ---------------------------------------------------------------------------------------------------------------------
# end to end on pbmc_3500: donor A mapped onto a reference of donors B and C
# ---------------------------------------------------------------------------------------------------------------------
def pbmc_split(vars_use="donor"):
    """(reference oracle run on donors B + C, query X d x N, query meta, query Phi, Pr_b, lamb): shared with the GPU
    tests."""
    from oracle.harmony_oracle import oracle_run_harmony, prepare_inputs
    data, meta = _pbmc()
    is_ref = meta["donor"].to_numpy() != "A"
    ref_meta = meta[is_ref].reset_index(drop=True)
    oo = oracle_run_harmony(data[is_ref], ref_meta, "donor", random_state=0, ridge_dtype=np.float64)
    q_meta = meta[~is_ref].reset_index(drop=True)
    p = prepare_inputs(data[~is_ref], q_meta, vars_use)
    return oo, p, q_meta, data[~is_ref]


def _ilisi(X, donors):
    from oracle.lisi_oracle import compute_lisi
    codes = pd.Categorical(donors).codes
    return float(np.median(compute_lisi(np.asarray(X, np.float64), [codes], perplexity=30)[:, 0]))


def test_pbmc_mapping_mixes_donors():
    """Donor iLISI of [reference Z_corr; query] rises when the query is mapped."""
    oo, p, q_meta, Xq = pbmc_split()
    S, m = MO.reference_summary(oo.R, oo.Z_corr)
    R, X_corr, _ = MO.map_query(p["Z"], p["phi"], p["Pr_b"], S, m, oo.sigma, p["lamb"])
    assert np.allclose(R.sum(axis=0), 1.0)
    data, meta = _pbmc()
    is_ref = meta["donor"].to_numpy() != "A"
    donors = np.concatenate([meta["donor"].to_numpy()[is_ref], q_meta["donor"].to_numpy()])
    before = _ilisi(np.concatenate([oo.Z_corr.T, Xq]), donors)
    after = _ilisi(np.concatenate([oo.Z_corr.T, X_corr.T]), donors)
    print(f"donor iLISI (median): unmapped {before:.4f}, mapped {after:.4f}")
    assert after > before + 0.05, (before, after)
