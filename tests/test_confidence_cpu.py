"""Mapping confidence (ClusterMoments, mapping_score, cluster_mapping_score), what can be checked without a GPU: the
float64 restatement against NumPy's own weighted covariance and against the direct quadratic form, the conditioning of
every data set the GPU accuracy tests use, the file format, argument errors that must come before the library is asked
for a GPU, the C header and export list, and the new kernels in the built library (no spills, no scratch, no register
touched with a load in flight)."""
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_audit  # noqa: E402

from harmonypy_amd import ClusterMoments, _capi  # noqa: E402
from harmonypy_amd import confidence as CF  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import confidence_cases as CC  # noqa: E402
import confidence_oracle as CO  # noqa: E402

LIB = _capi.LIB_PATH
needs_lib = pytest.mark.skipif(not (kernel_audit.tools_available() and os.path.exists(LIB)),
                               reason="needs the ROCm LLVM tools and a built libhmx.so")


def _problem(seed=0, N=600, d=6, K=4):
    rng = np.random.default_rng(seed)
    Z = rng.normal(size=(N, d)) @ rng.normal(size=(d, d)) + rng.normal(size=d) * 5
    R = rng.random(size=(N, K)) ** 4
    R /= R.sum(axis=1, keepdims=True)
    return R, Z, rng


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_is_numpys_weighted_covariance():
    R, Z, _ = _problem()
    mass, mass_sq, mean, cov = CO.cluster_moments(R.T, Z)
    for k in range(R.shape[1]):
        want = np.cov(Z.T, aweights=R[:, k], ddof=1)
        assert np.max(np.abs(cov[k] - want)) <= 1e-12 * np.max(np.abs(want))
        np.testing.assert_allclose(mean[k], np.average(Z, axis=0, weights=R[:, k]), rtol=1e-12)
    np.testing.assert_allclose(mass, R.sum(axis=0), rtol=1e-14)
    np.testing.assert_allclose(mass_sq, (R ** 2).sum(axis=0), rtol=1e-14)


def test_oracle_with_hard_codes_is_the_sample_covariance():
    _, Z, rng = _problem(1)
    codes = rng.integers(0, 5, size=Z.shape[0])
    codes[codes == 3] = 0                                              # group 3 is empty
    mass, mass_sq, mean, cov = CO.cluster_moments(CO.code_weights(codes, 5), Z)
    for g in (0, 1, 2, 4):
        want = np.cov(Z[codes == g].T, ddof=1)
        assert np.max(np.abs(cov[g] - want)) <= 1e-12 * np.max(np.abs(want))
        assert mass[g] == mass_sq[g] == (codes == g).sum()
    assert mass[3] == 0 and np.isnan(mean[3]).all() and np.isnan(cov[3]).all()


def test_oracle_score_is_the_direct_quadratic_form():
    R, Z, rng = _problem(2)
    _, _, mean, cov = CO.cluster_moments(R.T, Z)
    X = Z[:50] + rng.normal(size=(50, Z.shape[1]))
    Rq = R[:50]
    for ridge in (0.0, 1e-2):
        direct = np.zeros(50)
        for k in range(R.shape[1]):
            P = np.linalg.inv(CO.regularised(cov[k], ridge))
            delta = X - mean[k]
            direct += Rq[:, k] * np.sqrt(np.einsum("ni,ij,nj->n", delta, P, delta))
        np.testing.assert_allclose(CO.per_cell_score(Rq, X, mean, cov, ridge), direct, rtol=1e-10)


def test_whitening_reproduces_the_oracle_distances():
    """The form the library evaluates, |T_k x - t_k|, on the host: equal to the oracle's triangular solve."""
    R, Z, rng = _problem(3)
    m = ClusterMoments.from_arrays(R, Z)
    X = Z[:40] * 1.5
    for ridge in (0.0, 1e-2):
        T, t, invalid = CF.whitening(m, ridge)
        assert not invalid and np.array_equal(T, np.tril(T))
        D = np.linalg.norm(np.einsum("kij,nj->kni", T, X) - t[:, None, :], axis=2)
        np.testing.assert_allclose(D, CO.distances(X, m.mean, m.cov, ridge), rtol=1e-10)


# ---------------------------------------------------------------------------------------------------------------------
# conditioning of the data sets of the GPU accuracy tests: oracle forward against oracle reversed, valid clusters
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["orig", "corr"])
def test_pbmc_split_is_well_conditioned(space):
    """Donor A onto donors B + C (the oracle's run and the oracle's mapping stand in for the engine's): every reference
    cluster is valid with ridge = 0 and the scores do not depend on the order of the cells beyond 1e-9, so no ridge is
    needed for this data set (measured: 3e-14 in both spaces)."""
    import map_oracle as MO
    from test_map_query_cpu import pbmc_split
    oo, p, _, _ = pbmc_split()
    S, m = MO.reference_summary(oo.R, oo.Z_corr)
    Rq, X_corr, _ = MO.map_query(p["Z"], p["phi"], p["Pr_b"], S, m, oo.sigma, p["lamb"])
    Zr, Xq = (oo.Z_orig.T, p["Z"].T) if space == "orig" else (oo.Z_corr.T, X_corr.T)
    for ridge in (0.0, 1e-2):
        invalid, rel = CC.conditioning(oo.R.T, Zr, Rq.T, Xq, ridge)
        print(f"pbmc/{space} ridge={ridge:g}: invalid {invalid}, forward vs reversed {rel:.2e}")
        assert not invalid and rel <= 1e-9


@pytest.mark.parametrize("name", sorted(CC.SYNTHETIC))
def test_synthetic_sets_are_well_conditioned(name):
    """The assignment formula on the generating centres stands in for a finished run's R."""
    Zr, _, Xq, _, centres = CC.synthetic(name)
    Rr = CC.soft_assignment(Zr.astype(np.float64), centres)
    Rq = CC.soft_assignment(Xq.astype(np.float64), centres)
    for ridge in (0.0, 1e-2):
        invalid, rel = CC.conditioning(Rr, Zr, Rq, Xq, ridge)
        print(f"{name} ridge={ridge:g}: invalid {invalid}, forward vs reversed {rel:.2e}")
        assert not invalid and rel <= 1e-9


def test_gaussian_reference_separates_a_novel_population():
    """The set of the GPU test "it means something", on the oracle: known cells score sqrt(d) within 10 %, every novel
    cell above the known cells' 99th percentile, the novel group above every known group."""
    Zr, lr, Xq, lq = CC.gaussian_reference()
    K, d = int(lr.max()) + 1, Zr.shape[1]
    R = np.full((len(lr), K), 1e-3 / K)
    R[np.arange(len(lr)), lr] += 1.0 - 1e-3
    _, _, mean, cov = CO.cluster_moments(R.T, Zr)
    assert not CO.invalid_clusters(cov)
    Rq = CC.soft_assignment(Xq.astype(np.float64), mean)
    s = CO.per_cell_score(Rq, Xq, mean, cov)
    known, novel = s[lq < K], s[lq == K]
    print(f"median known {np.median(known):.3f}, sqrt(d) {np.sqrt(d):.3f}, p99 known {np.percentile(known, 99):.3f}, min novel {novel.min():.3f}")
    assert abs(np.median(known) / np.sqrt(d) - 1) <= 0.10
    assert novel.min() > np.percentile(known, 99)
    n, g = CO.per_cluster_score(Rq, Xq, lq, K + 1, mean)
    assert np.all(np.isfinite(g)) and g[K] > g[:K].max()


# ---------------------------------------------------------------------------------------------------------------------
# ClusterMoments
# ---------------------------------------------------------------------------------------------------------------------
def test_from_arrays_matches_the_oracle():
    R, Z, _ = _problem(4)
    R[:, 2] = 0.0                                                      # a cluster without mass
    m = ClusterMoments.from_arrays(R, Z, space="corr")
    mass, mass_sq, mean, cov = CO.cluster_moments(R.T, Z)
    np.testing.assert_allclose(m.mass, mass, rtol=1e-14)
    np.testing.assert_allclose(m.mass_sq, mass_sq, rtol=1e-14)
    np.testing.assert_allclose(m.mean, mean, rtol=1e-12)
    np.testing.assert_allclose(m.cov, cov, rtol=1e-10, atol=1e-12)
    assert np.isnan(m.cov[2]).all() and np.isnan(m.mean[2]).all()
    assert (m.K, m.d, m.space, m.n_cells) == (R.shape[1], Z.shape[1], "corr", R.shape[0])
    with pytest.raises(ValueError, match="cells x K"):
        ClusterMoments.from_arrays(R[:-1], Z)
    with pytest.raises(ValueError, match="space"):
        ClusterMoments.from_arrays(R, Z, space="cos")


def _moments(seed=5):
    R, Z, _ = _problem(seed)
    return ClusterMoments.from_arrays(R, Z)


def test_moments_save_load_round_trip(tmp_path):
    m = _moments()
    path = tmp_path / "m.npz"
    m.save(path)
    b = ClusterMoments.load(path)
    for name in ("mass", "mass_sq", "mean", "cov"):
        assert getattr(b, name).dtype == np.float64
        np.testing.assert_array_equal(getattr(b, name), getattr(m, name))
    assert (b.space, b.n_cells) == (m.space, m.n_cells)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(["format_version", "mass", "mass_sq", "mean", "cov", "space", "n_cells"])


@pytest.mark.parametrize("damage", ["extra", "missing", "dtype", "version", "shape_cov", "shape_mass", "space", "scalar"])
def test_moments_load_rejects_bad_files(tmp_path, damage):
    m = _moments()
    a = dict(format_version=np.int64(1), mass=m.mass, mass_sq=m.mass_sq, mean=m.mean, cov=m.cov, space=np.str_("orig"),
             n_cells=np.int64(m.n_cells))
    if damage == "extra":
        a["sigma"] = np.zeros(m.K, np.float32)
    elif damage == "missing":
        del a["mass_sq"]
    elif damage == "dtype":
        a["cov"] = a["cov"].astype(np.float32)
    elif damage == "version":
        a["format_version"] = np.int64(2)
    elif damage == "shape_cov":
        a["cov"] = a["cov"][:, :-1]
    elif damage == "shape_mass":
        a["mass"] = a["mass"][:-1]
    elif damage == "space":
        a["space"] = np.str_("cos")
    elif damage == "scalar":
        a["n_cells"] = np.array([m.n_cells], np.int64)
    path = tmp_path / "bad.npz"
    with open(path, "wb") as f:
        np.savez(f, **a)
    with pytest.raises(ValueError):
        ClusterMoments.load(path)


def test_reference_file_format_is_untouched(tmp_path):
    """A ClusterMoments file is not a HarmonyReference file and the other way round."""
    from harmonypy_amd import HarmonyReference
    from harmonypy_amd import mapping
    assert mapping.FORMAT_VERSION == 1
    assert sorted(HarmonyReference._FIELDS) == ["cluster_mass", "cluster_sums", "format_version", "n_cells", "sigma"]
    m = _moments()
    m.save(tmp_path / "m.npz")
    with pytest.raises(ValueError):
        HarmonyReference.load(tmp_path / "m.npz")
    HarmonyReference(np.ones((3, 2)), np.ones(3), np.ones(3), 9).save(tmp_path / "r.npz")
    with pytest.raises(ValueError):
        ClusterMoments.load(tmp_path / "r.npz")


# ---------------------------------------------------------------------------------------------------------------------
# argument errors: before the library is loaded or a GPU is asked for
# ---------------------------------------------------------------------------------------------------------------------
class _FakeQuery:
    """What the scoring functions read of a HarmonyQuery before they reach the engine."""

    def __init__(self, N, K, d):
        self.N, self.K, self.d = N, K, d

    @property
    def _engine(self):
        raise AssertionError("the engine was asked for")


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_capi, "load", refuse)


def test_mapping_score_argument_errors(no_library):
    m = _moments()
    q = _FakeQuery(100, m.K, m.d)
    with pytest.raises(ValueError, match="clusters"):
        CF.mapping_score(_FakeQuery(100, m.K + 1, m.d), m)
    with pytest.raises(ValueError, match="PCs"):
        CF.mapping_score(_FakeQuery(100, m.K, m.d + 1), m)
    for ridge in (-1e-3, np.nan, np.inf, "1", None, True):
        with pytest.raises(ValueError, match="ridge"):
            CF.mapping_score(q, m, ridge=ridge)
    with pytest.raises(TypeError, match="ClusterMoments"):
        CF.mapping_score(q, (m.mean, m.cov))
    bad = ClusterMoments(m.mass, m.mass_sq, m.mean, m.cov)
    bad.cov[1, 0, 0] = np.nan
    with pytest.raises(ValueError, match=r"clusters \[1\] are not finite"):
        CF.mapping_score(q, bad)
    # a singular cluster: named, and the remedy with it
    R, Z, _ = _problem(6)
    R[:, 2] = 0.0
    R[:4, 2] = 1.0                                                     # 4 cells in 6 dimensions
    sing = ClusterMoments.from_arrays(R, Z)
    with pytest.raises(ValueError, match=r"clusters \[2\].*ridge > 0"):
        CF.mapping_score(q, sing)
    T, t, invalid = CF.whitening(sing, 1e-2)
    assert not invalid and np.all(np.isfinite(T)) and np.all(np.isfinite(t))


def test_cluster_mapping_score_argument_errors(no_library):
    m = _moments()
    q = _FakeQuery(100, m.K, m.d)
    groups = np.arange(100) % 3
    with pytest.raises(ValueError, match="clusters"):
        CF.cluster_mapping_score(_FakeQuery(100, m.K + 2, m.d), m, groups)
    with pytest.raises(ValueError, match="PCs"):
        CF.cluster_mapping_score(_FakeQuery(100, m.K, m.d - 1), m, groups)
    with pytest.raises(ValueError, match="entries"):
        CF.cluster_mapping_score(q, m, groups[:-1])
    with pytest.raises(ValueError, match="missing"):
        CF.cluster_mapping_score(q, m, pd.Series(["a"] * 99 + [None]))
    with pytest.raises(ValueError, match="ridge"):
        CF.cluster_mapping_score(q, m, groups, ridge=-1)
    with pytest.raises(ValueError, match="min_cells_per_dim"):
        CF.cluster_mapping_score(q, m, groups, min_cells_per_dim=-1)
    with pytest.raises(ValueError, match="space"):
        CF.query_moments(q, space="cos")


def test_package_exports():
    import harmonypy_amd
    assert "ClusterMoments" in harmonypy_amd.__all__ and harmonypy_amd.ClusterMoments is ClusterMoments
    assert harmonypy_amd.__version__ == "0.4.0"
    for name in ("cluster_moments", "mapping_score", "cluster_mapping_score"):
        assert callable(getattr(harmonypy_amd.mapping.HarmonyQuery, name))
    assert callable(harmonypy_amd.Harmony.cluster_moments)


# ---------------------------------------------------------------------------------------------------------------------
# the C interface and the kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_score_exports():
    src = open(os.path.join(ROOT, "include", "hmx_score.h")).read()
    declared = re.findall(r"\bint (hmx_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert sorted(declared) == sorted(_capi.SCORE_EXPORTS) and len(set(declared)) == len(declared)
    for lst in (_capi.EXPORTS, _capi.DEVICE_IO_EXPORTS, _capi.MAP_EXPORTS, _capi.KNN_EXPORTS):
        assert not set(lst) & set(_capi.SCORE_EXPORTS)
    for h in ("hmx.h", "hmx_device_io.h", "hmx_map.h", "hmx_knn.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert not set(re.findall(r"\b(hmx_[a-z_0-9]+)\s*\(", text)) & set(_capi.SCORE_EXPORTS), h
    assert _capi.HMX_ABI_VERSION == 8
    assert re.search(r"#define\s+HMX_ABI_VERSION\s+8\b", open(os.path.join(ROOT, "include", "hmx.h")).read())


@pytest.mark.skipif(not os.path.exists(LIB), reason="needs a built libhmx.so")
def test_library_exports_the_score_entry_points():
    lib = _capi.load()
    for name in _capi.SCORE_EXPORTS:
        assert hasattr(lib, name)
    assert len(lib.hmx_cluster_moments.argtypes) == 8 and len(lib.hmx_mapping_score.argtypes) == 7
    assert lib.hmx_abi_version() == 8


@needs_lib
@pytest.mark.parametrize("prefix,mfma", [("k_mom", ("k_mom_sums", "k_mom_cov", "k_mom_cov_tILi4E")),
                                         ("k_mscore", ("k_mscoreE", "k_mscore_tILi4E"))])
def test_score_kernels_exist_without_spills_or_scratch(prefix, mfma):
    rows = {r["name"]: r for r in kernel_audit.audit(LIB, prefix)}
    assert rows
    for stem in mfma:
        hit = [r for n, r in rows.items() if stem in n]
        assert hit and all(r["mfma"] > 0 for r in hit), stem
    for r in rows.values():
        assert r["vgpr_spill_count"] == 0, f"{r['name']}: {r['vgpr_spill_count']} spilled VGPRs"
        assert r["private_segment_fixed_size"] == 0 and r.get("scratch", 0) == 0, f"{r['name']} uses scratch"
        assert r["group_segment_fixed_size"] == 0 and r["flat"] == 0, r["name"]
        assert "k_rtz3ILi" not in r["name"] and "k_knn" not in r["name"]


@needs_lib
def test_score_kernels_touch_no_register_with_a_load_in_flight():
    # k_mom_sums, k_mom_fold1, k_mom_fold2, k_mom_cov + k_mom_cov_t<1..4>; k_mscore + k_mscore_t<1..4>
    for prefix, n in (("k_mom", 8), ("k_mscore", 5)):
        hz = kernel_audit.inflight_hazards(LIB, prefix)
        assert len(hz) == n
        assert not {k: v for k, v in hz.items() if v}
