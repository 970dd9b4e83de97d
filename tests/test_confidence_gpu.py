"""Mapping confidence on the MI355X: hmx_cluster_moments / hmx_mapping_score and the Python layer over them against the
float64 restatement tests/confidence_oracle.py, which is fed the engine's own state (R, Z_orig / Z_corr read back through
the existing properties) -- so only the new kernels are under test.

Tolerances.  mass, mass_sq and mean are float64 sums of exactly converted terms: 1e-12 relative (a mean's coordinate
against sum |w z| / mass, see check_moments).  The covariance error is
max |dcov_ij| / sqrt(cov_ii cov_jj), the score error |dscore| / score.  Both were measured on the MI355X for every case
below (the table is in DESIGN.md, "Mapping confidence"); the bounds are 8 x the largest measured value of their kind,
room for another summation order on another build or grid, and far below the cap of 1e-6.  Every test prints its
figures before it asserts.  Every data set passes the conditioning check of test_confidence_cpu.py (oracle forward
against oracle reversed within 1e-9, every reference cluster valid with ridge = 0), and the check is repeated here on
the engine's own state before a tolerance is applied."""
import functools

import numpy as np
import pandas as pd
import pytest

import confidence_cases as CC
import confidence_oracle as CO

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-12
COV_TOL = 8 * 1.44e-14         # largest measured over the reference runs, the 1237-cell query and the hard codes (C3 shape)
COV_TOL_13_CELLS = 8 * 4.33e-13   # the 13-cell query alone: clusters that hang on one cell, whose unbiasing factor
#                                   1 - mass_sq / mass^2 cancels on the host -- kept apart so that it does not loosen the rest
SCORE_TOL = 8 * 1.96e-13       # largest measured: pbmc, corrected space, ridge 0 (5.6e-14 .. 2.0e-13 over five runs: run_harmony is
#                                not bit-reproducible and this state has clusters of mass 10 in 30 dimensions); <= 8.4e-14 elsewhere
assert max(COV_TOL, COV_TOL_13_CELLS, SCORE_TOL) <= 1e-6


def _torch():
    import torch
    return torch


def cov_error(cov, ref):
    """max over clusters and entries of |dcov_ij| / sqrt(cov_ii cov_jj)."""
    dg = np.sqrt(np.einsum("kii->ki", ref))
    return float(np.max(np.abs(cov - ref) / (dg[:, :, None] * dg[:, None, :])))


def rel_error(a, ref):
    return float(np.max(np.abs(a - ref) / np.abs(ref)))


def check_moments(m, W, Z, what, cov_tol=None):
    """ClusterMoments m against the oracle on the weights W (G x N) and the cells Z (N x d); groups without mass must be
    NaN on both sides.  mass, mass_sq: relative.  mean: element by element, |d mean_j| against sum_i |w_i z_ij| / mass --
    the relative error wherever a coordinate's terms share a sign, and the floor that any summation order needs where
    they cancel (a coordinate near zero cannot be held relative to itself)."""
    cov_tol = COV_TOL if cov_tol is None else cov_tol
    mass, mass_sq, mean, cov = CO.cluster_moments(W, Z)
    ok = mass > 0
    e_mass, e_sq = rel_error(m.mass[ok], mass[ok]), rel_error(m.mass_sq[ok], mass_sq[ok])
    scale = (np.abs(W[ok]) @ np.abs(Z)) / mass[ok][:, None]
    e_mean = float(np.max(np.abs(m.mean[ok] - mean[ok]) / scale))
    full = ok & np.isfinite(cov).all(axis=(1, 2))
    e_cov = cov_error(m.cov[full], cov[full]) if full.any() else 0.0
    print(f"[moments] {what}: mass {e_mass:.2e} mass_sq {e_sq:.2e} mean {e_mean:.2e} cov {e_cov:.3e} (groups {len(mass)}, "
          f"with mass {int(ok.sum())})")
    assert np.all(m.mass[~ok] == 0) and np.isnan(m.mean[~ok]).all() and np.isnan(m.cov[~ok]).all()
    assert np.isnan(m.cov[ok & ~full]).all()
    assert e_mass <= SUM_TOL and e_sq <= SUM_TOL and e_mean <= SUM_TOL
    assert e_cov <= cov_tol
    assert np.array_equal(m.cov[full], np.swapaxes(m.cov[full], 1, 2))
    return e_cov


@functools.lru_cache(maxsize=None)
def _case(name):
    """(finished reference Harmony, mapped HarmonyQuery, query data) of a data set."""
    from harmonypy_amd import map_query, run_harmony
    if name == "pbmc":
        from test_map_query_cpu import _pbmc
        data, meta = _pbmc()
        is_ref = meta["donor"].to_numpy() != "A"
        ho = run_harmony(data[is_ref], meta[is_ref].reset_index(drop=True), "donor", verbose=False)
        Xq, mq, vu = data[~is_ref], meta[~is_ref].reset_index(drop=True), "donor"
    else:
        Zr, mr, Xq, mq, _ = CC.synthetic(name)
        K = CC.SYNTHETIC[name][3]
        ho = run_harmony(Zr, mr, "batch", nclust=K, max_iter_harmony=2, verbose=False)
        vu = "batch"
    q = map_query(Xq, mq, ho, vars_use=vu, verbose=False)
    return ho, q, Xq, mq, vu


def _state(obj, space):
    return obj.R.astype(np.float64), (obj.Z_orig if space == "orig" else obj.Z_corr).astype(np.float64)


CASES = ["pbmc", "c3", "wide", "d100", "d10", "d40"]   # tiles per side of the tuned kernels: 2, 4, 2, generic, 1, 3


# ---------------------------------------------------------------------------------------------------------------------
# 1. moments
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["orig", "corr"])
@pytest.mark.parametrize("case", CASES)
def test_reference_moments(case, space):
    ho, _, _, _, _ = _case(case)
    m = ho.cluster_moments(space)
    R, Z = _state(ho, space)
    assert m.space == space and m.n_cells == ho.N and m.K == ho.K and m.d == ho.d
    check_moments(m, R.T, Z, f"{case}/{space} N={ho.N} K={ho.K} d={ho.d}")


@pytest.mark.parametrize("n", [13, 1237])
def test_moments_of_small_and_ragged_queries(n):
    """N < 16 and an N that is no multiple of 16, mapped onto the replayed golden run (bit-reproducible, so the figures
    are too: with 13 cells some clusters hang on one cell and their unbiasing factor 1 - mass_sq / mass^2 cancels)."""
    from harmonypy_amd import map_query
    ho, data, meta = _golden()
    q = map_query(data[:n], meta.iloc[:n].reset_index(drop=True), ho.reference(), vars_use="donor", verbose=False)
    assert q.N == n
    for space in ("orig", "corr"):
        R, Z = _state(q, space)
        check_moments(q.cluster_moments(space), R.T, Z, f"pbmc query N={n}/{space}",
                      cov_tol=COV_TOL_13_CELLS if n == 13 else COV_TOL)


@pytest.mark.parametrize("n_groups", [1, 7, 300])
def test_moments_by_group_codes(n_groups):
    _, q, _, _, _ = _case("c3")
    rng = np.random.default_rng(n_groups)
    codes = rng.integers(0, n_groups, size=q.N)
    empty = n_groups // 2 if n_groups > 1 else None
    if empty is not None:
        codes[codes == empty] = 0
    groups = pd.Categorical.from_codes(codes, categories=[f"g{i}" for i in range(n_groups)])
    for space in ("orig", "corr"):
        m = q.cluster_moments(space, groups=groups)
        assert m.K == n_groups
        check_moments(m, CO.code_weights(codes, n_groups), _state(q, space)[1], f"c3 codes G={n_groups}/{space}")
        if empty is not None:
            assert m.mass[empty] == 0 and np.isnan(m.cov[empty]).all()
        np.testing.assert_array_equal(m.mass, np.bincount(codes, minlength=n_groups))
        np.testing.assert_array_equal(m.mass_sq, m.mass)


# ---------------------------------------------------------------------------------------------------------------------
# 2. per-cell score
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ridge", [0.0, 1e-2])
@pytest.mark.parametrize("space", ["orig", "corr"])
@pytest.mark.parametrize("case", CASES)
def test_mapping_score_matches_oracle(case, space, ridge):
    ho, q, _, _, _ = _case(case)
    m = ho.cluster_moments(space)
    Rr, Zr = _state(ho, space)
    Rq, Xq = _state(q, space)
    invalid, cond = CC.conditioning(Rr, Zr, Rq, Xq, ridge)
    print(f"[conditioning] {case}/{space} ridge={ridge:g}: invalid {invalid}, forward vs reversed {cond:.2e}")
    assert not invalid and cond <= 1e-9
    _, _, mean, cov = CO.cluster_moments(Rr.T, Zr)
    want = CO.per_cell_score(Rq, Xq, mean, cov, ridge)
    got = q.mapping_score(m, ridge=ridge)
    assert got.dtype == np.float64 and got.shape == (q.N,)
    err = rel_error(got, want)
    print(f"[score] {case}/{space} ridge={ridge:g}: {err:.3e} (median score {np.median(got):.3f}, sqrt(d) {np.sqrt(q.d):.3f})")
    assert np.all(np.isfinite(got))
    assert err <= SCORE_TOL
    t = q.mapping_score(m, ridge=ridge, as_tensor=True)
    assert t.dtype == _torch().float64 and t.is_cuda
    np.testing.assert_array_equal(t.cpu().numpy(), got)


SMALL_QUERY_RIDGES = (0.0, 1e-2)


def small_query_scores(n, space, ridge):
    """(invalid clusters, conditioning, engine scores, tensor scores, oracle scores) of the first n cells of the golden
    data mapped onto the replayed golden run: N < 16 (most lanes of the score kernel's wave are clamped copies of the
    last cell, kept out by the guarded store) and an N that is no multiple of 16."""
    from harmonypy_amd import map_query
    ho, data, meta = _golden()
    q = map_query(data[:n], meta.iloc[:n].reset_index(drop=True), ho.reference(), vars_use="donor", verbose=False)
    Rr, Zr = _state(ho, space)
    Rq, Xq = _state(q, space)
    invalid, cond = CC.conditioning(Rr, Zr, Rq, Xq, ridge)
    if invalid:
        return invalid, cond, None, None, None
    m = ho.cluster_moments(space)
    _, _, mean, cov = CO.cluster_moments(Rr.T, Zr)
    want = CO.per_cell_score(Rq, Xq, mean, cov, ridge)
    got = q.mapping_score(m, ridge=ridge)
    return invalid, cond, got, q.mapping_score(m, ridge=ridge, as_tensor=True).cpu().numpy(), want


@pytest.mark.parametrize("ridge", SMALL_QUERY_RIDGES)
@pytest.mark.parametrize("space", ["orig", "corr"])
@pytest.mark.parametrize("n", [13, 1237])
def test_mapping_score_of_small_and_ragged_queries(n, space, ridge):
    invalid, cond, got, tensor, want = small_query_scores(n, space, ridge)
    print(f"[conditioning] golden N={n}/{space} ridge={ridge:g}: invalid {invalid}, forward vs reversed {cond:.2e}")
    assert not invalid and cond <= 1e-9
    assert got.shape == (n,) and got.dtype == np.float64 and np.all(np.isfinite(got))
    err = rel_error(got, want)
    print(f"[score] golden N={n}/{space} ridge={ridge:g}: {err:.3e}")
    assert err <= SCORE_TOL
    np.testing.assert_array_equal(tensor, got)


def test_a_finished_harmony_serves_as_moments():
    ho, q, _, _, _ = _case("pbmc")
    np.testing.assert_array_equal(q.mapping_score(ho), q.mapping_score(ho.cluster_moments("orig")))


@pytest.mark.parametrize("layout", ["bfloat16", "float16", "float64"])
def test_device_query_scores_like_the_same_values_from_the_host(layout):
    from harmonypy_amd import map_query
    torch = _torch()
    ho, _, Xq, mq, vu = _case("pbmc")
    m = ho.cluster_moments("orig")
    dt = {"bfloat16": torch.bfloat16, "float16": torch.float16, "float64": torch.float64}[layout]
    wide = torch.zeros((Xq.shape[0], 2 * Xq.shape[1] + 3), dtype=dt, device="cuda")
    x = wide[:, 1:2 * Xq.shape[1] + 1:2]                                   # a strided view
    x.copy_(torch.from_numpy(Xq).to("cuda"))
    same = x.float().cpu().numpy()
    qd = map_query(x, mq, ho, vars_use=vu, verbose=False)
    qh = map_query(same, mq, ho, vars_use=vu, verbose=False)
    sd, sh = qd.mapping_score(m, ridge=1e-2), qh.mapping_score(m, ridge=1e-2)
    np.testing.assert_array_equal(sd, sh)
    np.testing.assert_array_equal(qd.mapping_score(m, ridge=1e-2, as_tensor=True).cpu().numpy(), sh)
    want = CO.per_cell_score(qh.R.astype(np.float64), same.astype(np.float64), m.mean, m.cov, 1e-2)
    err = rel_error(sh, want)
    print(f"[score] pbmc device {layout}: {err:.3e}")
    assert err <= SCORE_TOL


# ---------------------------------------------------------------------------------------------------------------------
# 3. per-cluster score
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pbmc", "c3"])
def test_cluster_mapping_score_matches_oracle(case):
    ho, q, _, _, _ = _case(case)
    m = ho.cluster_moments("orig")
    rng = np.random.default_rng(1)
    big = max(1, q.N // (3 * q.d))                                  # groups of ~3 d cells, and one far too small
    codes = rng.integers(0, big, size=q.N)
    small = big
    codes[: q.d] = small                                            # d cells < 2 d
    names = np.array([f"c{i:03d}" for i in range(big + 1)])
    df = q.cluster_mapping_score(m, names[codes], ridge=1e-2)
    assert list(df.columns) == ["n_cells", "score"] and list(df.index) == sorted(set(names[codes]))
    Rq, Xq = _state(q, "orig")
    n, want = CO.per_cluster_score(Rq, Xq, codes, big + 1, m.mean, ridge=1e-2)
    np.testing.assert_array_equal(df["n_cells"].to_numpy(), n)
    got = df["score"].to_numpy()
    assert np.isnan(got[small]) and np.isnan(want[small])
    ok = ~np.isnan(want)
    assert ok.sum() >= big - 1 and np.array_equal(np.isnan(got), np.isnan(want))
    err = rel_error(got[ok], want[ok])
    print(f"[cluster score] {case}: {err:.3e} over {int(ok.sum())} groups")
    assert err <= SCORE_TOL
    # a lower threshold lets the small group through
    df2 = q.cluster_mapping_score(m, names[codes], ridge=1e-2, min_cells_per_dim=1)
    assert np.isfinite(df2["score"].to_numpy()[small])


# ---------------------------------------------------------------------------------------------------------------------
# 4. it means something
# ---------------------------------------------------------------------------------------------------------------------
def test_novel_population_stands_out():
    from harmonypy_amd import ClusterMoments, HarmonyReference, map_query
    Zr, lr, Xq, lq = CC.gaussian_reference()
    K, d = int(lr.max()) + 1, Zr.shape[1]
    R = np.full((len(lr), K), 1e-3 / K)
    R[np.arange(len(lr)), lr] += 1.0 - 1e-3
    ref = HarmonyReference.from_arrays(R, Zr, 0.1)
    m = ClusterMoments.from_arrays(R, Zr)
    q = map_query(Xq, pd.DataFrame({"b": ["q"] * len(lq)}), ref, vars_use=None, verbose=False)
    s = q.mapping_score(m)
    known, novel = s[lq < K], s[lq == K]
    print(f"[meaning] median known {np.median(known):.3f} (sqrt(d) {np.sqrt(d):.3f}), 99th pct known {np.percentile(known, 99):.3f}, "
          f"min novel {novel.min():.3f}")
    assert abs(np.median(known) / np.sqrt(d) - 1) <= 0.10
    assert novel.min() > np.percentile(known, 99)
    df = q.cluster_mapping_score(m, lq)
    print(df)
    assert df["score"].to_numpy()[K] > df["score"].to_numpy()[:K].max()


# ---------------------------------------------------------------------------------------------------------------------
# 5. nothing moved
# ---------------------------------------------------------------------------------------------------------------------
def _snapshot(obj):
    from harmonypy_amd import _capi
    return {"R": obj.R, "Z_corr": obj.Z_corr, "Z_cos": obj.Z_cos, "O": obj._engine.get(_capi.HMX_O_GROUP)}


def _replayed_pbmc_run():
    """The pbmc_default golden run with its recorded centroids and round schedule: bit-reproducible, so two of them are
    twins (as tests/test_map_query_gpu.py uses it)."""
    from conftest import load_case
    from harmonypy_amd import run_harmony
    data, meta, vars_use, kw, g = load_case("pbmc_default")
    ho = run_harmony(data, meta, vars_use, verbose=False, _y0=g["Y0"], _schedule=[int(r) for r in g["kmeans_rounds"]], **kw)
    return ho, data, meta


@functools.lru_cache(maxsize=None)
def _golden():
    """One replayed golden run shared by the tests that only read it."""
    return _replayed_pbmc_run()


def test_the_engines_do_not_move():
    from harmonypy_amd import map_query
    ho, data, meta = _replayed_pbmc_run()
    twin, _, _ = _replayed_pbmc_run()                                # never computes a score
    ref_before = ho.reference()
    Xq, mq = data[:700], meta.iloc[:700].reset_index(drop=True)
    q = map_query(Xq, mq, ref_before, vars_use="donor", verbose=False)
    qtwin = map_query(Xq, mq, ref_before, vars_use="donor", verbose=False)
    for a, b in ((ho, twin), (q, qtwin)):
        for name in ("Z_corr", "R"):
            np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=f"the twins differ from the start: {name}")
    before_ref, before_q = _snapshot(ho), _snapshot(q)
    m = ho.cluster_moments("orig")
    ho.cluster_moments("corr")
    q.cluster_moments("corr", groups=mq["donor"].to_numpy())
    q.mapping_score(m, ridge=1e-2)
    q.mapping_score(m, ridge=1e-2, as_tensor=True)
    q.cluster_mapping_score(m, np.arange(q.N) % 3, ridge=1e-2)
    for name, a in _snapshot(ho).items():
        np.testing.assert_array_equal(a, before_ref[name], err_msg=f"reference {name}")
    for name, a in _snapshot(q).items():
        np.testing.assert_array_equal(a, before_q[name], err_msg=f"query {name}")
    ref_after = ho.reference()
    np.testing.assert_array_equal(ref_after.cluster_sums, ref_before.cluster_sums)
    np.testing.assert_array_equal(ref_after.cluster_mass, ref_before.cluster_mass)
    for a, b in ((ho, twin), (q, qtwin)):
        a._engine.moe_correct_ridge()
        b._engine.moe_correct_ridge()
        for name in ("Z_corr", "Z_cos", "R"):
            np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_singular_cluster_is_refused_until_regularised():
    from harmonypy_amd import ClusterMoments
    ho, q, _, _, _ = _case("pbmc")
    R, Z = _state(ho, "orig")
    R = R.copy()
    R[:, 3] = 0.0
    R[: q.d - 2, 3] = 1.0                                            # d - 2 cells: fewer than d + 1
    m = ClusterMoments.from_arrays(R, Z)
    with pytest.raises(ValueError, match=r"clusters \[3\].*ridge"):
        q.mapping_score(m)
    s = q.mapping_score(m, ridge=1e-2)
    assert np.all(np.isfinite(s)) and np.all(s > 0)
    want = CO.per_cell_score(q.R.astype(np.float64), q.Z_orig.astype(np.float64), m.mean, m.cov, 1e-2)
    err = rel_error(s, want)
    print(f"[score] pbmc with a regularised singular cluster: {err:.3e}")
    assert err <= SCORE_TOL


def test_sharded_engine_gets_the_state_error():
    from harmonypy_amd import _capi
    ho, q, _, _, _ = _case("pbmc")
    m = ho.cluster_moments("orig")
    q._engine.set_host_allreduce(lambda buf: None)                   # what a rank of a sharded job installs
    try:
        for call in (lambda: q.cluster_moments("orig"), lambda: q.mapping_score(m)):
            with pytest.raises(_capi.HmxError, match="shard") as ei:
                call()
            assert ei.value.code == _capi.HMX_ERR_STATE
    finally:
        q._engine.set_host_allreduce(None)
    assert np.all(np.isfinite(q.mapping_score(m, ridge=1e-2)))


def test_shape_mismatch_is_refused_before_the_library(monkeypatch):
    from harmonypy_amd import ClusterMoments, _capi
    ho, q, _, _, _ = _case("pbmc")
    m = ho.cluster_moments("orig")

    def refuse(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_capi.Engine, "mapping_score", refuse)
    monkeypatch.setattr(_capi.Engine, "cluster_moments", refuse)
    fewer_k = ClusterMoments(m.mass[:-1], m.mass_sq[:-1], m.mean[:-1], m.cov[:-1])
    fewer_d = ClusterMoments(m.mass, m.mass_sq, m.mean[:, :-1], m.cov[:, :-1, :-1])
    for bad, msg in ((fewer_k, "clusters"), (fewer_d, "PCs")):
        with pytest.raises(ValueError, match=msg):
            q.mapping_score(bad)
        with pytest.raises(ValueError, match=msg):
            q.cluster_mapping_score(bad, np.zeros(q.N, dtype=int))
    with pytest.raises(ValueError, match="ridge"):
        q.mapping_score(m, ridge=-1.0)
    with pytest.raises(ValueError, match="entries"):
        q.cluster_mapping_score(m, np.zeros(q.N - 1, dtype=int))
