"""compute_lisi on device tensors and on embeddings of 209..320 features (`-m gpu`).

Device input is read in place (hmx_compute_lisi_device: k_lisi_load) and converted to float64 exactly, so every result --
neighbour indices, distances and LISI -- must equal the NumPy path's on ``X.double().cpu().numpy()`` bit for bit.  The
data has no duplicate points; ties in distance are broken by index on both paths (and in the oracle).  The wide
embeddings are checked against the oracle's float64 brute-force search."""
import numpy as np
import pandas as pd
import pytest

from oracle import lisi_oracle as LO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}


def _hm():
    import harmonypy_amd as hm
    return hm


def _data(n, d, seed, offset=0.0):
    rng = np.random.default_rng(seed)
    cent = rng.normal(size=(8, d)) * 3
    X = cent[rng.integers(0, 8, n)] + rng.normal(size=(n, d)) + offset
    meta = pd.DataFrame({"a": rng.integers(0, 4, n).astype(str), "b": rng.integers(0, 3, n).astype(str)})
    return X, meta


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


def _assert_same(dev_res, host_res, x):
    if isinstance(host_res, tuple):
        assert isinstance(dev_res, tuple) and len(dev_res) == 3
        for got, want, dt in zip(dev_res, host_res, (torch.float64, torch.float64, torch.int32)):
            assert isinstance(got, torch.Tensor) and got.device == x.device and got.dtype == dt
            assert tuple(got.shape) == want.shape
            np.testing.assert_array_equal(got.cpu().numpy(), want)
    else:
        assert isinstance(dev_res, torch.Tensor) and dev_res.device == x.device and dev_res.dtype == torch.float64
        assert tuple(dev_res.shape) == host_res.shape
        np.testing.assert_array_equal(dev_res.cpu().numpy(), host_res)


@pytest.mark.parametrize("layout", ["contiguous", "T", "colslice", "rows"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_device_input_matches_host_input(dt, layout):
    hm = _hm()
    V, meta = _data(1500, 30, 1)
    x = _layout(V, DTYPES[dt], layout)
    assert x.shape == (1500, 30)
    host_x = x.double().cpu().numpy()
    for rn in (True, False):
        want = hm.compute_lisi(host_x, meta, ["a", "b"], 20, return_neighbors=rn)
        got = hm.compute_lisi(x, meta, ["a", "b"], 20, return_neighbors=rn)
        _assert_same(got, want, x)


def test_dlpack_producer_is_read_in_place():
    hm = _hm()
    V, meta = _data(900, 12, 2)
    x = torch.from_numpy(V).float().cuda()

    class Producer:                                          # not a torch.Tensor: only the DLPack protocol
        def __dlpack__(self, **kw):
            return x.__dlpack__(**kw)

        def __dlpack_device__(self):
            return x.__dlpack_device__()

    want = hm.compute_lisi(x.double().cpu().numpy(), meta, ["a"], 15, return_neighbors=True)
    _assert_same(hm.compute_lisi(Producer(), meta, ["a"], 15, return_neighbors=True), want, x)


@pytest.mark.parametrize("d", [209, 250, 320])
@pytest.mark.parametrize("perp", [30, 100, 400])              # 256-, 1024- and 4096-entry candidate lists
def test_wide_embeddings_are_exact(d, perp):
    hm = _hm()
    n = 2500
    V, meta = _data(n, d, 10 + d + perp, offset=50.0)          # off-centre on purpose
    lab = pd.Categorical(meta["a"]).codes
    X32 = V.astype(np.float32)
    Xh = X32.astype(np.float64)
    dist, idx = LO.knn_exact(Xh, perp * 3)
    want = np.array([1.0 / LO.simpson_cell(dist[i, 1:], lab[idx[i, 1:]], perp) for i in range(0, n, 13)])
    x = torch.from_numpy(X32).cuda()
    for res in (hm.compute_lisi(Xh, meta, ["a"], perp, return_neighbors=True),
                tuple(t.cpu().numpy() for t in hm.compute_lisi(x, meta, ["a"], perp, return_neighbors=True))):
        out, kd, ki = res
        np.testing.assert_array_equal(ki, idx[:, 1:])
        np.testing.assert_allclose(kd, dist[:, 1:], rtol=1e-12)
        np.testing.assert_allclose(out[::13, 0], want, rtol=1e-9)


@pytest.mark.parametrize("d", [30, 250])
def test_end_to_end_on_the_device(d):
    hm = _hm()
    n = 3000
    rng = np.random.default_rng(d)
    batch = rng.integers(0, 3, n)
    cent = rng.normal(size=(10, d)) * 3
    Z = (cent[rng.integers(0, 10, n)] + rng.normal(size=(n, d)) + batch[:, None] * 0.7).astype(np.float32)
    meta = pd.DataFrame({"batch": [f"b{i}" for i in batch]})
    ho = hm.run_harmony(torch.from_numpy(Z).cuda(), meta, "batch", nclust=20, max_iter_harmony=2, verbose=False)
    t = ho.to_tensor("Z_corr")
    got = hm.compute_lisi(t, meta, ["batch"], return_neighbors=True)
    want = hm.compute_lisi(ho.Z_corr, meta, ["batch"], return_neighbors=True)
    _assert_same(got, want, t)


def test_device_path_never_calls_the_host_entry_point(monkeypatch):
    hm = _hm()
    from harmonypy_amd import _capi
    V, meta = _data(800, 40, 3)
    want = hm.compute_lisi(V, meta, ["a"], 10)
    lib = _capi.load()

    def refuse(*a, **k):
        raise AssertionError("hmx_compute_lisi (host copy of X) was called")
    monkeypatch.setattr(lib, "hmx_compute_lisi", refuse)
    x = torch.from_numpy(V).cuda()
    _assert_same(hm.compute_lisi(x, meta, ["a"], 10), want, x)
    with pytest.raises(AssertionError):
        hm.compute_lisi(V, meta, ["a"], 10)


def test_cpu_tensor_takes_the_host_path():
    hm = _hm()
    V, meta = _data(700, 16, 6)
    want = hm.compute_lisi(V, meta, ["a"], 10, return_neighbors=True)
    got = hm.compute_lisi(torch.from_numpy(V), meta, ["a"], 10, return_neighbors=True)
    for g, w in zip(got, want):
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype
        np.testing.assert_array_equal(g, w)


def _busy(n=6):
    """Queue some milliseconds of work on the current stream."""
    a = torch.randn(4096, 4096, device="cuda")
    for _ in range(n):
        a = a @ a
        a = a / a.abs().max()
    return a


def test_stream_ordering():
    hm = _hm()
    V, meta = _data(3000, 50, 4)
    x = V.astype(np.float32)
    want_out, want_kd, want_ki = hm.compute_lisi(x.astype(np.float64), meta, ["a", "b"], 30, return_neighbors=True)
    src = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        # produced on the side stream behind a busy queue, consumed by the very next call and after it, on that
        # stream, without any synchronisation of our own
        _busy()
        z = torch.empty_like(src)
        z.copy_(src)
        out, kd, ki = hm.compute_lisi(z, meta, ["a", "b"], 30, return_neighbors=True)
        out2 = (out * 2.0).cpu().numpy()
        kd2 = (kd + 1.0).cpu().numpy()
        ki2 = (ki + 1).cpu().numpy()
    np.testing.assert_array_equal(out2, want_out * 2.0)
    np.testing.assert_array_equal(kd2, want_kd + 1.0)
    np.testing.assert_array_equal(ki2, want_ki + 1)


def test_argument_errors_before_any_device_work(monkeypatch):
    hm = _hm()
    from harmonypy_amd import _capi
    V, meta = _data(500, 8, 5)
    x = torch.from_numpy(V).float().cuda()
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_capi, "load", refuse)
    cases = [
        (x.reshape(1, 500, 8), {}),                         # 3-D
        (x.to(torch.int32), {}),                            # integer dtype
        (x[:-1], {}),                                       # rows != metadata rows
        (x.T, {}),                                          # features x cells: no transposition guess
        (x, {"device": "cuda:1"}),                          # another ordinal
        (x, {"device": "cpu"}),
        (x, {"perplexity": 681}),                           # beyond the largest candidate list
        (x, {"perplexity": 200}),                           # 600 neighbours of 500 cells
    ]
    for bad, kw in cases:
        with pytest.raises(ValueError):
            hm.compute_lisi(bad, meta, ["a"], **kw)
    meta_na = meta.copy()
    meta_na.loc[3, "a"] = None
    with pytest.raises(ValueError):
        hm.compute_lisi(x, meta_na, ["a"])
