"""Device tensors in, device tensors out (`-m gpu`): run_harmony / Harmony read an embedding that lives on the GPU in
place (hmx_upload_device: k_io_load) and Harmony.to_tensor writes results into device tensors (hmx_copy_out_device:
k_io_store).

Everything is compared bit for bit against the NumPy path on the same fp32 values: the state the upload builds (Z_orig,
Z_cos, Z_corr before any iteration), whole runs (Z_corr, R, Y, objectives, k-means rounds) and to_tensor against the
NumPy properties.  Whole runs are made reproducible by fixing the initial centroids and the k-means round schedule
(``_y0`` / ``_schedule``, as the parity tests do): the k-means initialisation is where repeated runs of the same input
part (sklearn's multi-threaded fit on the host, the device k-means above 200 k cells).  With both fixed, 20 repeated
NumPy runs of every case below were bit-identical."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT, assert_z_close, load_case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _hm():
    from harmonypy_amd import harmony as H
    return H


def _synthetic(N, d, B, seed):
    rng = np.random.default_rng(seed)
    batch = rng.integers(0, B, size=N)
    centres = rng.normal(size=(12, d)) * 3.0
    Z = centres[rng.integers(0, 12, size=N)] + rng.normal(size=(N, d)) + batch[:, None] * 0.7
    meta = pd.DataFrame({"batch": [f"b{i}" for i in batch]})
    return Z.astype(np.float64), meta


def _unit_centroids(Z, K):
    """d x K initial centroids: K evenly spaced cells, unit length (a fixed stand-in for the k-means initialisation)."""
    Y = np.asarray(Z[np.linspace(0, Z.shape[0] - 1, K).astype(np.int64)], np.float64)
    return np.ascontiguousarray((Y / np.linalg.norm(Y, axis=1, keepdims=True)).T, dtype=np.float32)


def _case(name):
    """(data N x d float64, meta, vars_use, kwargs): initial centroids and round schedule fixed."""
    if name.startswith("pbmc"):
        data, meta, vars_use, kw, g = load_case(name)
        kw = dict(kw, _y0=g["Y0"], _schedule=[int(r) for r in g["kmeans_rounds"]])
        return np.asarray(data, np.float64), meta, vars_use, kw
    # synthetic cases: epsilons that never stop early, so every k-means call runs max_iter_kmeans rounds
    fixed = dict(epsilon_cluster=0.0, epsilon_harmony=-1e30, random_state=0)
    if name == "wide":          # d = K = 200: the wide kernels
        Z, meta = _synthetic(20_000, 200, 6, seed=5)
        return Z, meta, ["batch"], dict(nclust=200, max_iter_harmony=2, max_iter_kmeans=4, _y0=_unit_centroids(Z, 200), **fixed)
    if name == "large":         # above 200 k cells: the device update order (device k-means: test_device_kmeans_on_device_input)
        Z, meta = _synthetic(250_000, 30, 5, seed=6)
        return Z, meta, ["batch"], dict(nclust=40, max_iter_harmony=2, max_iter_kmeans=5, _y0=_unit_centroids(Z, 40), **fixed)
    if name == "pcs320":        # 320 PCs: the smallest LDS slab of the slab kernels (32 cells)
        Z, meta = _synthetic(3_000, 320, 3, seed=7)
        return Z, meta, ["batch"], dict(nclust=12, max_iter_harmony=1, max_iter_kmeans=2, _y0=_unit_centroids(Z, 12), **fixed)
    raise KeyError(name)


def _layout(x, layout):
    """A device tensor holding the cells x features matrix x (torch, on the GPU) in the given layout.  Strides of the
    d x N matrix the engine reads: cell stride 1 takes the LDS slab kernel, feature stride 1 the row kernel."""
    N, d = x.shape
    if layout == "nxd":                 # contiguous N x d: feature stride 1
        return x.contiguous()
    if layout == "dxn":                 # contiguous d x N (the reference's orientation): cell stride 1
        return x.T.contiguous()
    if layout == "t_of_dxn":            # .T of a row-major d x N: an N x d view with cell stride 1
        return x.T.contiguous().T
    if layout == "t_of_nxd":            # .T of a row-major N x d: a d x N view with feature stride 1
        return x.contiguous().T
    if layout == "slice":               # [:, :d] of a wider N x (d + 14): feature stride 1, cell stride d + 14
        wide = torch.full((N, d + 14), 1000.0, dtype=x.dtype, device=x.device)
        wide[:, :d] = x
        return wide[:, :d]
    raise KeyError(layout)


def _uses_slab(t, N):
    """Whether the engine reads t through the slab kernel (cell stride 1 once oriented d x N)."""
    v = t if t.shape[1] == N else t.T
    return v.stride(1) == 1 and v.stride(0) != 1


def _device_input(data, dtype, layout):
    """(device tensor, the NumPy array the host path gets for the same values)."""
    t = torch.from_numpy(data).to(dtype).to("cuda")
    host = data if dtype == torch.float64 else t.float().cpu().numpy()
    return _layout(t, layout), host


def _run(x, meta, vars_use, kw):
    H = _hm()
    return H.run_harmony(x, meta, vars_use, verbose=False, **kw)


def _assert_same_run(ho, ref):
    """Whole runs: bit for bit."""
    for k in ("Z_corr", "R", "Y"):
        np.testing.assert_array_equal(getattr(ho, k), getattr(ref, k), err_msg=k)
    for k in ("objective_harmony", "objective_kmeans", "kmeans_rounds"):
        np.testing.assert_array_equal(np.asarray(getattr(ho, k)), np.asarray(getattr(ref, k)), err_msg=k)


def _assert_same_upload(ho, ref):
    """The state the upload built (no iteration ran): byte for byte."""
    for name in ("Z_orig", "Z_cos", "Z_corr"):
        np.testing.assert_array_equal(getattr(ho, name), getattr(ref, name), err_msg=name)


CASES = [
    ("pbmc_default", torch.float32, "nxd"), ("pbmc_default", torch.float32, "dxn"),
    ("pbmc_default", torch.float32, "t_of_dxn"), ("pbmc_default", torch.float32, "t_of_nxd"),
    ("pbmc_default", torch.float32, "slice"),
    ("pbmc_default", torch.float64, "nxd"), ("pbmc_default", torch.float64, "dxn"),
    ("pbmc_default", torch.float16, "slice"), ("pbmc_default", torch.float16, "dxn"),
    ("pbmc_default", torch.bfloat16, "nxd"), ("pbmc_default", torch.bfloat16, "dxn"), ("pbmc_default", torch.bfloat16, "t_of_nxd"),
    ("pbmc_two_vars", torch.float32, "dxn"), ("pbmc_two_vars", torch.float64, "slice"),
    ("pbmc_lambda_est", torch.float32, "t_of_dxn"), ("pbmc_lambda_est", torch.bfloat16, "nxd"),
    ("wide", torch.float64, "nxd"), ("wide", torch.float32, "dxn"), ("wide", torch.float16, "slice"),
    ("large", torch.float64, "t_of_nxd"), ("large", torch.float32, "dxn"), ("large", torch.bfloat16, "t_of_dxn"),
    ("large", torch.bfloat16, "slice"),
    ("pcs320", torch.float32, "dxn"), ("pcs320", torch.bfloat16, "t_of_dxn"), ("pcs320", torch.float64, "nxd"),
]

_BASELINES = {}


def _baseline(name, dtype):
    """(NumPy-path run, the NumPy upload state without iterations, inputs) for the values the device tensor holds."""
    key = (name, dtype)
    if key not in _BASELINES:
        data, meta, vars_use, kw = _case(name)
        _, host = _device_input(data, dtype, "nxd")
        torch.cuda.synchronize()
        _BASELINES.clear()                      # one baseline alive at a time (the large case holds 250 k cells)
        _BASELINES[key] = (_run(host, meta, vars_use, kw), _run(host, meta, vars_use, dict(kw, max_iter_harmony=0)),
                           data, meta, vars_use, kw)
    return _BASELINES[key]


@pytest.mark.parametrize("name,dtype,layout", CASES, ids=[f"{c}-{str(t).split('.')[-1]}-{l}" for c, t, l in CASES])
def test_device_input_matches_numpy_input(name, dtype, layout):
    ref, ref0, data, meta, vars_use, kw = _baseline(name, dtype)
    x, _ = _device_input(data, dtype, layout)
    assert _uses_slab(x, data.shape[0]) == (layout in ("dxn", "t_of_dxn"))
    ho0 = _run(x, meta, vars_use, dict(kw, max_iter_harmony=0))
    assert "upload_device" in ho0.timing and "upload" not in ho0.timing
    _assert_same_upload(ho0, ref0)
    if name == "pcs320":                    # copy-out through the 32-cell slab as well
        out = torch.full((ho0.d + 3, ho0.N), 7.5, device="cuda")
        ho0.to_tensor("Z_cos", out=out[1:1 + ho0.d].T)
        o = out.cpu().numpy()
        np.testing.assert_array_equal(o[1:1 + ho0.d].T, ref0.Z_cos)
        assert (o[0] == 7.5).all() and (o[1 + ho0.d:] == 7.5).all()
    del ho0
    ho = _run(x, meta, vars_use, kw)
    _assert_same_run(ho, ref)


def test_device_kmeans_on_device_input():
    """Above 200 k cells without fixed centroids the initial k-means runs on the device, over the Z_cos the device upload
    built; the k-means initialisation is not bit-reproducible run to run, so the result is held to the project's Z_corr
    bar against the NumPy run."""
    data, meta, vars_use, kw = _case("large")
    kw = {k: v for k, v in kw.items() if k != "_y0"}
    x = data.astype(np.float32)
    ref = _run(x, meta, vars_use, kw)
    ho = _run(torch.from_numpy(x).cuda().T.contiguous(), meta, vars_use, kw)
    assert "kmeans_lloyd" in ho.timing and "upload_device" in ho.timing
    assert ho.kmeans_rounds == ref.kmeans_rounds
    assert_z_close(ho.Z_corr, ref.Z_corr)


def test_no_host_upload_of_the_embedding(monkeypatch):
    from harmonypy_amd import _capi
    data, meta, vars_use, kw, _ = load_case("pbmc_short")

    def refuse(*a, **k):
        raise AssertionError("Engine.upload called for a device tensor")
    monkeypatch.setattr(_capi.Engine, "upload", refuse)
    ho = _run(torch.from_numpy(np.asarray(data, np.float32)).cuda(), meta, vars_use, kw)
    assert "upload_device" in ho.timing
    assert np.isfinite(ho.Z_corr).all()


def _small_run(source="device"):
    data, meta, vars_use, kw, _ = load_case("pbmc_short")
    x = np.asarray(data, np.float32)
    return _run(torch.from_numpy(x).cuda() if source == "device" else x, meta, vars_use, kw)


@pytest.mark.parametrize("source", ["device", "numpy"])
def test_to_tensor_matches_the_numpy_properties(source):
    ho = _small_run(source)
    for which in ("Z_corr", "Z_orig", "Z_cos", "R"):
        t = ho.to_tensor(which)
        assert t.dtype == torch.float32 and t.device == torch.device("cuda", 0) and t.is_contiguous()
        np.testing.assert_array_equal(t.cpu().numpy(), getattr(ho, which), err_msg=which)
    N, d, K = ho.N, ho.d, ho.K
    # a d x N buffer, written through its N x d transpose
    buf = torch.full((d, N), -3.0, device="cuda")
    assert ho.to_tensor("Z_corr", out=buf.T) is not None
    np.testing.assert_array_equal(buf.cpu().numpy(), ho.Z_corr.T)
    # column slices of wider matrices pre-filled with a sentinel: the sentinel columns survive
    for which, cols in (("Z_corr", d), ("R", K)):
        wide = torch.full((N, cols + 9), 7.5, device="cuda")
        out = ho.to_tensor(which, out=wide[:, 4:4 + cols])
        assert out.data_ptr() == wide[:, 4:].data_ptr()
        w = wide.cpu().numpy()
        np.testing.assert_array_equal(w[:, 4:4 + cols], getattr(ho, which), err_msg=which)
        assert (w[:, :4] == 7.5).all() and (w[:, 4 + cols:] == 7.5).all(), which
    # a d x N slice of a taller matrix written column by column (cell stride 1, feature stride of the big matrix)
    tall = torch.full((d + 5, N), 7.5, device="cuda")
    ho.to_tensor("Z_cos", out=tall[2:2 + d].T)
    t = tall.cpu().numpy()
    np.testing.assert_array_equal(t[2:2 + d].T, ho.Z_cos)
    assert (t[:2] == 7.5).all() and (t[2 + d:] == 7.5).all()
    with pytest.raises(ValueError):
        ho.to_tensor("Y")
    with pytest.raises(ValueError):
        ho.to_tensor("Z_corr", out=torch.empty((N, d + 1), device="cuda"))
    with pytest.raises(ValueError):
        ho.to_tensor("Z_corr", out=torch.empty((N, d), device="cuda", dtype=torch.float64))


def _busy(n=6):
    """Queue some milliseconds of work on the current stream."""
    a = torch.randn(4096, 4096, device="cuda")
    for _ in range(n):
        a = a @ a
        a = a / a.abs().max()
    return a


def test_stream_ordering_in_and_out():
    data, meta, vars_use, kw = _case("pbmc_short")
    x = np.asarray(data, np.float32)
    ref = _run(x, meta, vars_use, kw)
    src = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        # produced on the side stream behind a busy queue, consumed by the very next call: the engine must wait for it
        _busy()
        z = torch.empty_like(src)
        z.copy_(src)
        ho = _run(z, meta, vars_use, kw)
    np.testing.assert_array_equal(ho.Z_orig, x)           # what the engine read is the finished copy
    _assert_same_run(ho, ref)
    out_side = torch.cuda.Stream()
    with torch.cuda.stream(out_side):
        _busy()
        t = ho.to_tensor("Z_corr")            # ordered on out_side: no synchronisation of our own
        y = t * 2.0
        back = y.cpu().numpy()
    np.testing.assert_array_equal(back, ho.Z_corr * 2.0)


def test_argument_errors_before_any_engine(monkeypatch):
    from harmonypy_amd import _capi
    data, meta, vars_use, kw, _ = load_case("pbmc_short")
    N, d = data.shape

    def refuse(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(_capi.Engine, "__init__", refuse)
    H = _hm()
    x = torch.from_numpy(np.asarray(data, np.float32)).cuda()
    for bad in (x.to(torch.int32), x[:, 0], x[:-1], x.reshape(1, N, d)):
        with pytest.raises(ValueError):
            H.run_harmony(bad, meta, vars_use, verbose=False, **kw)
    with pytest.raises(ValueError):
        H.run_harmony(x, meta, vars_use, verbose=False, device="cuda:1", **kw)
    with pytest.raises(ValueError):
        H.run_harmony(x, meta, vars_use, verbose=False, device="cpu", **kw)


def _launch(case, outdir, source, world=2, timeout=600):
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="2", GLOO_SOCKET_IFNAME="lo")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_device_io_shard_worker.py"), case,
                                       str(outdir), source], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(out.decode(errors="replace"))
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed:\n{logs[r][-4000:]}"
    return [dict(np.load(os.path.join(outdir, f"rank{r}.npz"), allow_pickle=False)) for r in range(world)]


@pytest.mark.parametrize("case", ["pbmc_default", "pbmc_two_vars"])
def test_sharded_device_slices_match_sharded_numpy_slices(case, tmp_path):
    """Two processes on one GPU over gloo, each passing its slice; the stitched results of the device and the NumPy runs."""
    (tmp_path / "numpy").mkdir()
    (tmp_path / "device").mkdir()
    host = _launch(case, tmp_path / "numpy", "numpy")
    dev = _launch(case, tmp_path / "device", "device")
    for a, b in zip(host, dev):
        assert (int(a["lo"]), int(a["hi"])) == (int(b["lo"]), int(b["hi"]))
    for a, b in zip(host, dev):                             # each rank's upload state: byte for byte
        for name in ("Z_orig", "Z_cos"):
            np.testing.assert_array_equal(b[name], a[name], err_msg=name)
    Zh = np.concatenate([r["Z_corr"] for r in host], axis=0)
    Zd = np.concatenate([r["Z_corr"] for r in dev], axis=0)
    np.testing.assert_array_equal(Zd, Zh)                   # the whole run (centroids and schedule fixed, as in the worker)
    assert_z_close(Zd, load_case(case)[4]["Z_corr"])        # and the reference's result
