"""``compute_lisi`` with the reference's signature (harmonypy/lisi.py:24-66), computed on the MI355X.

The neighbour search (the reference: sklearn's kd-tree, lisi.py:53-54), the perplexity search and
the Simpson index (``compute_simpson``, lisi.py:69-133) run as HIP kernels behind
``hmx_compute_lisi`` (include/hmx.h), or ``hmx_compute_lisi_device`` (include/hmx_device_io.h) for an
embedding that already lives on the GPU.  There is no CPU path.
"""
from __future__ import annotations

from typing import Iterable

import numpy as np
import pandas as pd

from . import _capi
from .harmony import _as_device_tensor, _device_dtype, _engine_device

_MAX_NEIGHBOURS = 2040   # 3 * perplexity of the largest candidate list (include/hmx.h, hmx_compute_lisi)


def _device_index(device):
    if device is None or device == "cuda":
        return 0
    s = str(device)
    if s.startswith("cuda:"):
        return int(s.split(":", 1)[1])
    raise ValueError(f"harmonypy_amd runs on the MI355X only (device='cuda' or 'cuda:n'), got {device!r}")


def _label_codes(metadata, label_colnames, n):
    codes = np.empty((len(label_colnames), n), dtype=np.int32)
    for i, label in enumerate(label_colnames):
        cat = pd.Categorical(metadata[label])                                   # lisi.py:63
        if (cat.codes < 0).any():
            raise ValueError(f"metadata[{label!r}] has missing values")
        codes[i] = cat.codes
    return codes


def compute_lisi(
    X: np.array,
    metadata: pd.DataFrame,
    label_colnames: Iterable[str],
    perplexity: float = 30,
    device=None,
    return_neighbors: bool = False,
):
    """Local Inverse Simpson Index of every row of ``X`` for each column of ``metadata`` named in
    ``label_colnames``; returns an ``n_cells x n_labels`` float64 array like the reference.

    ``return_neighbors=True`` also returns the ``3*perplexity - 1`` nearest neighbours of every cell
    (distances, indices), nearest first -- what the reference gets from ``knn.kneighbors`` after
    dropping the first column (lisi.py:55-60).

    ``X`` may also live on the GPU: a 2-D ``torch.Tensor`` on a HIP device, or any ``__dlpack__`` producer on
    ROCm, of float32 / float16 / bfloat16 / float64 and any strides (``pcs[:, :50]``, ``.T`` of a features x
    cells tensor, ``x[::2]``).  It is cells x features as for NumPy input (no transposition guess) and is
    read in place on its device (``device=None`` follows it; a ``device`` naming another ordinal is a
    ValueError); the host never holds a copy.  Every element converts to float64 exactly, so the results
    equal those of ``X.double().cpu().numpy()``.  They come back as tensors on that device -- LISI float64,
    neighbour distances float64 and indices int32 -- ordered on the current stream: the call runs behind the
    work queued there and later work there sees the results.

    Limits of this build: ``X`` has at most 320 features (HMX_MAX_PCS, as ``run_harmony``), and
    ``3 * perplexity <= 2040`` neighbours (perplexity <= 680; the reference takes any): a larger
    value raises ``ValueError``.  Up to 120 neighbours (perplexity 40; the default is 30) the search keeps 256
    candidates per cell, up to 504 it keeps 1024, beyond 4096 -- each step costs memory (8 bytes x candidates x cells)
    and speed.
    """
    if isinstance(label_colnames, str):
        label_colnames = [label_colnames]
    label_colnames = list(label_colnames)
    Xd = _as_device_tensor(X)
    if Xd is not None:
        return _compute_lisi_device(Xd, metadata, label_colnames, perplexity, device, return_neighbors)
    Xv = X.values if hasattr(X, "values") and not callable(X.values) else X   # (a CPU tensor's .values is a method)
    Xv = np.ascontiguousarray(Xv, dtype=np.float64)
    if Xv.ndim != 2:
        raise ValueError("X must be a cells x features matrix")
    n, d = Xv.shape
    if metadata.shape[0] != n:
        raise ValueError("X and metadata do not have the same number of cells")
    codes = _label_codes(metadata, label_colnames, n)
    nn = int(perplexity * 3)                                                    # lisi.py:53
    lib = _capi.load()
    out = np.empty((n, len(label_colnames)), dtype=np.float64)
    kd = ki = None
    if return_neighbors:
        kd = np.empty((n, max(nn - 1, 0)), dtype=np.float64)
        ki = np.empty((n, max(nn - 1, 0)), dtype=np.int32)
    rc = lib.hmx_compute_lisi(_device_index(device), _capi._ptr(Xv), n, d, _capi._ptr(codes), len(label_colnames),
                              float(perplexity), _capi._ptr(out), _capi._ptr(kd), _capi._ptr(ki))
    _raise_on_error(lib, rc)
    return (out, kd, ki) if return_neighbors else out


def _raise_on_error(lib, rc):
    if rc < 0:
        msg = lib.hmx_last_error().decode(errors="replace")
        if "n_neighbors" in msg or msg.startswith("perplexity"):
            raise ValueError(msg)                                               # what sklearn raises for the reference / this build's limit
        raise _capi.HmxError(f"libhmx: {msg} (code {rc})", code=int(rc))


def _compute_lisi_device(Xd, metadata, label_colnames, perplexity, device, return_neighbors):
    """compute_lisi of a cells x features device tensor: hmx_compute_lisi_device on the current stream of its device,
    results into fresh tensors there.  Every argument is checked before any device work."""
    import torch
    dtype = _device_dtype(Xd, "X")
    dev = _engine_device(device, Xd, "X")
    n, d = Xd.shape
    if metadata.shape[0] != n:
        raise ValueError(f"X {tuple(Xd.shape)} is cells x features; metadata has {metadata.shape[0]} cells")
    codes = _label_codes(metadata, label_colnames, n)
    nn = int(perplexity * 3)                                                    # lisi.py:53
    # hmx_compute_lisi_device makes these checks too, with the same messages: here they come before the outputs exist
    if not (perplexity > 0 and 2 <= nn <= _MAX_NEIGHBOURS):
        raise ValueError(f"perplexity: 3*perplexity must lie in [2, {_MAX_NEIGHBOURS}] neighbours in this build (got {nn})")
    if nn > n:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {nn}, n_samples_fit = {n}")
    lib = _capi.load()
    tdev = torch.device("cuda", dev)
    with torch.cuda.device(tdev):
        out = torch.empty((n, len(label_colnames)), dtype=torch.float64, device=tdev)
        kd = ki = None
        if return_neighbors:
            kd = torch.empty((n, nn - 1), dtype=torch.float64, device=tdev)
            ki = torch.empty((n, nn - 1), dtype=torch.int32, device=tdev)
        rc = lib.hmx_compute_lisi_device(dev, Xd.data_ptr(), dtype, n, d, Xd.stride(0), Xd.stride(1),
                                         torch.cuda.current_stream(tdev).cuda_stream, _capi._ptr(codes),
                                         len(label_colnames), float(perplexity), out.data_ptr(),
                                         kd.data_ptr() if kd is not None else None,
                                         ki.data_ptr() if ki is not None else None)
    _raise_on_error(lib, rc)
    return (out, kd, ki) if return_neighbors else out
