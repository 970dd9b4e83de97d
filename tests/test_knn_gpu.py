"""Label transfer on the MI355X (`-m gpu`): knn_query / knn_predict against the float64 restatement tests/knn_oracle.py
(indices and votes exactly, distances to 1e-12), the reference slicing against the unsliced search, device input
against NumPy input bit for bit, compute_lisi's neighbours, and a mapped query end to end."""
import numpy as np
import pandas as pd
import pytest

import knn_oracle as KO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}


def _hm():
    import harmonypy_amd as hm
    return hm


def _sets(nq, nr, d, seed):
    """Clustered query and reference sets with duplicated reference rows (distance ties), query rows that sit on
    reference rows (distance 0), and three label columns: 4 categories, >= 3000 categories, 2 categories."""
    rng = np.random.default_rng(seed)
    cent = rng.normal(size=(6, d)) * 2
    R = cent[rng.integers(0, 6, nr)] + rng.normal(size=(nr, d))
    Q = cent[rng.integers(0, 6, nq)] + rng.normal(size=(nq, d))
    if nr >= 4:
        dup = rng.choice(nr, size=max(1, nr // 10), replace=False)
        R[dup] = R[rng.integers(0, nr, dup.size)]
        on = rng.choice(nq, size=max(1, nq // 10), replace=False)
        Q[on] = R[rng.integers(0, nr, on.size)]
    meta = pd.DataFrame({
        "type": rng.integers(0, 4, nr).astype(str),
        "fine": [f"c{v}" for v in rng.integers(0, 3500, nr)],
        "side": rng.integers(0, 2, nr).astype(str),
    })
    return Q, R, meta


def _check_against_oracle(Q, R, meta, k, res):
    df, dist, idx = res
    want_d, want_i = KO.knn_cross(Q, R, k)
    np.testing.assert_array_equal(idx, want_i)
    np.testing.assert_allclose(dist, want_d, rtol=1e-12, atol=0)
    for col in meta.columns:
        cat = pd.Categorical(meta[col])
        pred, prob = KO.vote(want_i, cat.codes)
        got = df[col]
        assert isinstance(got.dtype, pd.CategoricalDtype) and list(got.cat.categories) == list(cat.categories)
        np.testing.assert_array_equal(got.cat.codes.to_numpy(), pred)
        np.testing.assert_array_equal(df[col + "_prob"].to_numpy(), prob)


CASES = [  # (n_q, n_ref, d, k): sizes off the 16 / 256 grids, n_ref < 16, every list-size boundary of k
    (1, 13, 7, 5), (37, 13, 1, 13), (301, 1000, 1, 1), (300, 1531, 7, 5), (257, 2100, 30, 120), (199, 1777, 50, 121),
    (123, 3001, 64, 504), (77, 2500, 65, 505), (40, 2049, 200, 2040), (90, 1200, 208, 30), (90, 1300, 209, 5),
    (33, 2047, 320, 2040), (100, 1000, 320, 121),
]


@pytest.mark.parametrize("nq,nr,d,k", CASES)
def test_matches_oracle(nq, nr, d, k):
    hm = _hm()
    Q, R, meta = _sets(nq, nr, d, seed=nq + nr + d + k)
    res = hm.knn_predict(Q, R, meta, list(meta.columns), k=k, return_neighbors=True)
    assert isinstance(res[1], np.ndarray) and res[1].dtype == np.float64 and res[2].dtype == np.int32
    assert len(res[0]) == nq and list(res[0].columns) == ["type", "type_prob", "fine", "fine_prob", "side", "side_prob"]
    _check_against_oracle(Q, R, meta, k, res)


@pytest.mark.parametrize("nq,nr,d,k", [(300, 1531, 7, 5), (77, 2500, 65, 505), (33, 2047, 320, 2040)])
def test_forced_slices_match_the_oracle(nq, nr, d, k):
    hm = _hm()
    Q, R, meta = _sets(nq, nr, d, seed=7 * d + k)
    for slices in (1, 3, 10):
        res = hm.knn_predict(Q, R, meta, list(meta.columns), k=k, return_neighbors=True, _slices=slices)
        _check_against_oracle(Q, R, meta, k, res)


def test_slicing_changes_nothing_and_the_automatic_choice_slices_small_queries():
    hm = _hm()
    from harmonypy_amd import _capi
    lib = _capi.load()
    assert lib.hmx_knn_slices(0, 2000, 200_000, 50, 5) > 1             # a small query against a large reference
    assert lib.hmx_knn_slices(0, 1_000_000, 1_000_000, 50, 5) == 1      # a query that fills the GPU alone
    assert lib.hmx_knn_slices(0, 10, 100, 50, 5) == 1                   # too small a reference to cut
    rng = np.random.default_rng(11)
    R = torch.from_numpy(rng.normal(size=(60_000, 50))).float().cuda()
    Q = torch.from_numpy(rng.normal(size=(700, 50))).float().cuda()
    assert lib.hmx_knn_slices(0, 700, 60_000, 50, 30) > 1
    meta = pd.DataFrame({"t": rng.integers(0, 9, 60_000).astype(str)})
    one = hm.knn_predict(Q, R, meta, "t", k=30, return_neighbors=True, _slices=1)
    for slices in (0, 5, 64):
        other = hm.knn_predict(Q, R, meta, "t", k=30, return_neighbors=True, _slices=slices)
        pd.testing.assert_frame_equal(one[0], other[0])
        assert torch.equal(one[1], other[1]) and torch.equal(one[2], other[2])
    want_d, want_i = KO.knn_cross(Q[:50].double().cpu().numpy(), R.double().cpu().numpy(), 30)
    np.testing.assert_array_equal(one[2][:50].cpu().numpy(), want_i)


def _layout(V, dtype, layout):
    """A cells x features device tensor of dtype holding V (rounded to dtype), in the given memory layout."""
    n, d = V.shape
    t = torch.from_numpy(V).to(dtype)
    if layout == "contiguous":
        return t.cuda()
    if layout == "T":                                        # .T of a features x cells tensor: cell stride 1
        return t.T.contiguous().cuda().T
    if layout == "colslice":                                 # a column slice of a wider matrix
        wide = torch.randn(n, d + 7, dtype=torch.float64).to(dtype)
        wide[:, 3:3 + d] = t
        return wide.cuda()[:, 3:3 + d]
    if layout == "rows":                                     # every other row of a taller matrix
        tall = torch.randn(2 * n, d, dtype=torch.float64).to(dtype)
        tall[::2] = t
        return tall.cuda()[::2]
    raise ValueError(layout)


@pytest.mark.parametrize("layout", ["contiguous", "T", "colslice", "rows"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_device_input_matches_numpy_input(dt, layout):
    hm = _hm()
    Q, R, meta = _sets(333, 2222, 30, seed=5)
    q = _layout(Q, DTYPES[dt], layout)
    r = _layout(R, DTYPES[dt], "T" if layout == "contiguous" else "contiguous")
    qh, rh = q.double().cpu().numpy(), r.double().cpu().numpy()
    want = hm.knn_predict(qh, rh, meta, list(meta.columns), k=10, return_neighbors=True)
    got = hm.knn_predict(q, r, meta, list(meta.columns), k=10, return_neighbors=True)
    pd.testing.assert_frame_equal(got[0], want[0])
    for g, w, dtype in ((got[1], want[1], torch.float64), (got[2], want[2], torch.int32)):
        assert isinstance(g, torch.Tensor) and g.device == q.device and g.dtype == dtype
        np.testing.assert_array_equal(g.cpu().numpy(), w)
    # one set on the device, the other on the host: read on the device
    dq, iq = hm.knn_query(q, rh, 10)
    assert isinstance(dq, torch.Tensor) and dq.device == q.device
    np.testing.assert_array_equal(dq.cpu().numpy(), want[1])
    np.testing.assert_array_equal(iq.cpu().numpy(), want[2])
    dh, ih = hm.knn_query(torch.from_numpy(qh).to(DTYPES["f64"]), r, 10)   # a CPU tensor and a device tensor
    np.testing.assert_array_equal(ih.cpu().numpy(), want[2])


def test_dlpack_producer_and_non_default_stream():
    hm = _hm()
    Q, R, meta = _sets(500, 3000, 50, seed=9)
    want = hm.knn_predict(Q.astype(np.float32).astype(np.float64), R.astype(np.float32).astype(np.float64), meta,
                          ["fine"], k=7, return_neighbors=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        # produced on the side stream and read there: the call must be ordered behind the copies queued on it
        q = torch.from_numpy(Q).cuda(non_blocking=True).float()
        r = torch.from_numpy(R).cuda(non_blocking=True).float() * 1.0

        class Producer:                                          # not a torch.Tensor: only the DLPack protocol
            def __dlpack__(self, **kw):
                return r.__dlpack__(**kw)

            def __dlpack_device__(self):
                return r.__dlpack_device__()

        df, dist, idx = hm.knn_predict(q, Producer(), meta, ["fine"], k=7, return_neighbors=True)
        out = idx + 0                                            # later work on the stream sees the results
    s.synchronize()
    pd.testing.assert_frame_equal(df, want[0])
    np.testing.assert_array_equal(out.cpu().numpy(), want[2])
    np.testing.assert_array_equal(dist.cpu().numpy(), want[1])


def test_other_device_ordinal_is_refused():
    hm = _hm()
    q = torch.zeros((4, 3), device="cuda:0")
    with pytest.raises(ValueError, match="cuda:0"):
        hm.knn_query(q, np.zeros((5, 3)), 2, device="cuda:1")


def test_self_search_reproduces_compute_lisi_neighbours():
    hm = _hm()
    rng = np.random.default_rng(3)
    X = rng.normal(size=(1500, 20)) + rng.integers(0, 5, 1500)[:, None] * 2.0   # no duplicated rows
    meta = pd.DataFrame({"a": rng.integers(0, 3, 1500).astype(str)})
    _, ld, li = hm.compute_lisi(X, meta, ["a"], perplexity=10, return_neighbors=True)   # 29 neighbours, self dropped
    dist, idx = hm.knn_query(X, X, 30)
    np.testing.assert_array_equal(idx[:, 0], np.arange(1500))
    np.testing.assert_array_equal(idx[:, 1:], li)
    np.testing.assert_array_equal(dist[:, 1:], ld)


def _labelled(seed=3, spread=1.0, shift=6.0):
    """Six cell types in 20 PCs; a reference of two batches shifted against each other, a query shifted further."""
    rng = np.random.default_rng(seed)
    T, d = 6, 20
    cent = rng.normal(size=(T, d)) * spread

    def cells(n, sh):
        t = rng.integers(0, T, n)
        return cent[t] + rng.normal(size=(n, d)) + sh, t
    sd = rng.normal(size=(3, d))
    sd /= np.linalg.norm(sd, axis=1, keepdims=True)
    Xa, ta = cells(1500, sd[0])
    Xb, tb = cells(1500, -sd[0])
    Xq, tq = cells(800, sd[1] * shift)
    types = np.array(list("ABCDEF"))
    meta = pd.DataFrame({"batch": np.repeat(["r0", "r1"], 1500), "type": types[np.concatenate([ta, tb])]})
    return np.vstack([Xa, Xb]).astype(np.float32), meta, Xq.astype(np.float32), types[tq]


def test_mapped_query_gets_the_reference_labels():
    hm = _hm()
    Xr, meta, Xq, truth = _labelled()
    ho = hm.run_harmony(Xr, meta, ["batch"], verbose=False, random_state=0)
    ref = ho.reference()
    q = hm.map_query(Xq, pd.DataFrame({"cell": np.arange(len(Xq))}), ref, verbose=False)
    zr = ho.to_tensor("Z_corr")
    df = q.knn_predict(zr, meta, ["type"], k=5)
    same = hm.knn_predict(q.to_tensor("Z_corr"), zr, meta, ["type"], k=5)
    pd.testing.assert_frame_equal(df, same)
    acc = float((df["type"].astype(str).to_numpy() == truth).mean())
    raw = hm.knn_predict(torch.from_numpy(Xq).cuda(), zr, meta, ["type"], k=5)
    acc_raw = float((raw["type"].astype(str).to_numpy() == truth).mean())
    assert acc >= 0.95 and acc > acc_raw, (acc, acc_raw)
    assert ((df["type_prob"] > 0) & (df["type_prob"] <= 1)).all()
