"""Label transfer (knn_predict / knn_query), what can be checked without a GPU: the float64 restatement against sklearn and
against hand-built tie cases, the C entry points' header and exports, the new kernel instances in the built library (no
spills, no scratch), and argument errors that must come before the library is asked for a GPU."""
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_audit  # noqa: E402

from harmonypy_amd import _capi  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_oracle as KO  # noqa: E402

LIB = _capi.LIB_PATH
needs_lib = pytest.mark.skipif(not (kernel_audit.tools_available() and os.path.exists(LIB)),
                               reason="needs the ROCm LLVM tools and a built libhmx.so")
CAPS = (256, 1024, 4096)


@pytest.mark.parametrize("nq,nr,d,k", [(40, 300, 7, 5), (25, 500, 50, 30), (3, 17, 1, 17), (60, 2100, 12, 121)])
def test_oracle_agrees_with_sklearn(nq, nr, d, k):
    sk = pytest.importorskip("sklearn.neighbors")
    rng = np.random.default_rng(nq * 1000 + d)
    R = rng.normal(size=(nr, d)) * 2
    Q = rng.normal(size=(nq, d)) * 2
    dist, idx = KO.knn_cross(Q, R, k)
    sd, si = sk.NearestNeighbors(n_neighbors=k, algorithm="brute").fit(R).kneighbors(Q)
    np.testing.assert_array_equal(idx, si)
    np.testing.assert_allclose(dist, sd, rtol=1e-12)


def test_distance_ties_go_to_the_smaller_index():
    R = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0], [3.0, 3.0], [1.0, 0.0]])
    dist, idx = KO.knn_cross(np.zeros((1, 2)), R, 5)
    np.testing.assert_array_equal(idx[0], [0, 1, 2, 3, 5])
    np.testing.assert_array_equal(dist[0], [1.0] * 5)
    # duplicated rows: the copy with the smaller index ranks first, wherever it sits
    dist, idx = KO.knn_cross(np.array([[1.0, 0.1]]), R, 3)
    np.testing.assert_array_equal(idx[0, :2], [0, 5])


def test_vote_majority_and_ties():
    codes = np.array([0, 1, 2, 1, 2, 3000])
    # majority: two votes for 1
    pred, prob = KO.vote(np.array([[0, 1, 3, 2, 5]]), codes)
    assert pred[0] == 1 and prob[0] == 2 / 5
    # 1 and 2 tie with two votes each: 2's nearest member ranks first (rank 0)
    pred, prob = KO.vote(np.array([[2, 1, 3, 4, 0]]), codes)
    assert pred[0] == 2 and prob[0] == 2 / 5
    # all different: the nearest neighbour's category
    pred, prob = KO.vote(np.array([[5, 0, 1, 2]]), codes)
    assert pred[0] == 3000 and prob[0] == 1 / 4
    pred, prob = KO.vote(np.array([[1]]), codes)
    assert pred[0] == 1 and prob[0] == 1.0


def test_header_declares_the_knn_exports():
    hdr = open(os.path.join(ROOT, "include", "hmx_knn.h")).read()
    declared = set(re.findall(r"\bint (hmx_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_capi.KNN_EXPORTS)
    others = [_capi.EXPORTS, _capi.DEVICE_IO_EXPORTS, _capi.MAP_EXPORTS]
    for lst in others:
        assert not set(lst) & set(_capi.KNN_EXPORTS)
    for h in ("hmx.h", "hmx_device_io.h", "hmx_map.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert not set(re.findall(r"\b(hmx_[a-z_0-9]+)\s*\(", text)) & set(_capi.KNN_EXPORTS), h
    assert _capi.HMX_ABI_VERSION == 8


@pytest.mark.skipif(not os.path.exists(LIB), reason="needs a built libhmx.so")
def test_library_exports_the_knn_entry_points():
    lib = _capi.load()
    for name in _capi.KNN_EXPORTS:
        assert hasattr(lib, name)
    assert len(lib.hmx_knn_predict.argtypes) == 21
    assert lib.hmx_abi_version() == 8


@pytest.fixture(scope="module")
def knn_rows():
    return {r["name"]: r for r in kernel_audit.audit(LIB, "k_knn")}


@needs_lib
@pytest.mark.parametrize("ks16", range(1, 21))
def test_search_instances_exist_without_spills(knn_rows, ks16):
    qt = 4 if ks16 <= 4 else 2 if ks16 <= 8 else 1
    for cap in CAPS:
        name = f"_ZN12_GLOBAL__N_112k_knn_searchILi{ks16}ELi{qt}ELi{cap}EEEv13KnnSearchArgs"
        assert name in knn_rows, f"k_knn_search<{ks16}, {qt}, {cap}> missing"
        r = knn_rows[name]
        assert r["vgpr_spill_count"] == 0, f"{name}: {r['vgpr_spill_count']} spilled VGPRs"
        assert r["private_segment_fixed_size"] == 0 and r.get("scratch", 0) == 0, f"{name} uses scratch"
        assert r["group_segment_fixed_size"] + 4 * cap * 8 <= 160 * 1024, name
        assert r["mfma"] >= 4 * ks16


@needs_lib
def test_finish_and_centre_kernels_do_not_spill(knn_rows):
    finish = [n for n in knn_rows if "k_knn_finish" in n]
    assert len(finish) == 3                                                    # 128-, 512- and 2048-entry rankings
    assert any("k_knn_center" in n for n in knn_rows)
    assert len(knn_rows) == 20 * 3 + 3 + 1
    for r in knn_rows.values():
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0 and r.get("scratch", 0) == 0, r["name"]
        assert r["group_segment_fixed_size"] <= 64 * 1024, r["name"]


@needs_lib
def test_knn_kernels_touch_no_register_with_a_load_in_flight():
    hz = kernel_audit.inflight_hazards(LIB, "k_knn")
    assert len(hz) == 20 * 3 + 3 + 1
    assert not {k: v for k, v in hz.items() if v}


# ---- argument errors: ValueError before the library is loaded or a GPU is asked for ---------------------------------

@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_capi, "load", refuse)


def _sets(nq=20, nr=50, d=8):
    rng = np.random.default_rng(0)
    return rng.normal(size=(nq, d)), rng.normal(size=(nr, d)), pd.DataFrame({"t": rng.integers(0, 3, nr).astype(str)})


@pytest.mark.parametrize("k,msg", [(51, "n_neighbors = 51, n_samples_fit = 50"), (0, r"\[1, 2040\]"), (2041, r"\[1, 2040\]"),
                                   (2.5, "integer")])
def test_bad_k_is_refused(no_library, k, msg):
    from harmonypy_amd import knn_predict, knn_query
    Q, R, meta = _sets()
    with pytest.raises(ValueError, match=msg):
        knn_query(Q, R, k)
    with pytest.raises(ValueError, match=msg):
        knn_predict(Q, R, meta, "t", k=k)


def test_k_above_2040_is_refused_on_a_large_reference(no_library):
    from harmonypy_amd import knn_query
    rng = np.random.default_rng(1)
    with pytest.raises(ValueError, match=r"\[1, 2040\]"):
        knn_query(rng.normal(size=(3, 2)), rng.normal(size=(3000, 2)), 2041)


def test_shape_errors_are_refused(no_library):
    from harmonypy_amd import knn_predict, knn_query
    Q, R, meta = _sets()
    with pytest.raises(ValueError, match="features"):
        knn_query(Q[:, :5], R, 3)
    rng = np.random.default_rng(2)
    with pytest.raises(ValueError, match="320"):
        knn_query(rng.normal(size=(4, 321)), rng.normal(size=(9, 321)), 3)
    with pytest.raises(ValueError, match="cells x features"):
        knn_query(Q[0], R, 3)
    with pytest.raises(ValueError, match="ref_meta"):
        knn_predict(Q, R, meta.iloc[:-1], "t", k=3)
    with pytest.raises(ValueError, match="not in ref_meta"):
        knn_predict(Q, R, meta, ["t", "nope"], k=3)


def test_missing_labels_are_refused(no_library):
    from harmonypy_amd import knn_predict
    Q, R, meta = _sets()
    meta.loc[7, "t"] = None
    with pytest.raises(ValueError, match="missing"):
        knn_predict(Q, R, meta, "t", k=3)


def test_bad_device_name_is_refused(no_library):
    from harmonypy_amd import knn_query
    Q, R, _ = _sets()
    with pytest.raises(ValueError, match="MI355X"):
        knn_query(Q, R, 3, device="cpu")
