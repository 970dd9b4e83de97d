"""Label transfer from a reference to query cells: ``knn_predict`` and ``knn_query``, as Symphony's ``knnPredict`` after
``mapQuery`` (Kang et al., Nat. Commun. 12, 5890, 2021).

For every query cell the k nearest reference cells (exact Euclidean, nearest first, ties by the smaller reference index)
and per label column a majority vote over their labels.  The search and the vote run on the MI355X behind
``hmx_knn_predict`` (include/hmx_knn.h); there is no CPU path.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from . import _capi
from .harmony import _as_device_tensor, _device_dtype
from .lisi import _MAX_NEIGHBOURS, _device_index, _label_codes, _raise_on_error


def _host_matrix(x, name):
    """A host matrix (NumPy, a CPU tensor, a DataFrame) as float64, every element converted exactly."""
    if hasattr(x, "detach") and hasattr(x, "double"):                            # a CPU torch tensor, bfloat16 included
        x = x.detach().double().numpy()
    elif hasattr(x, "values") and not callable(x.values):
        x = x.values
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError(f"{name} must be a cells x features matrix, got {x.ndim} dimension(s)")
    return x


def _resolve(query, reference, k, device):
    """Checks every argument that needs no GPU; returns (Qd, Rd, host Q, host R, device ordinal or None for host data, k,
    reference cells)."""
    Qd, Rd = _as_device_tensor(query), _as_device_tensor(reference)
    Qh = _host_matrix(query, "query") if Qd is None else None
    Rh = _host_matrix(reference, "reference") if Rd is None else None
    for t, name in ((Qd, "query"), (Rd, "reference")):
        if t is not None:
            _device_dtype(t, name)
    nq, dq = (Qd if Qd is not None else Qh).shape
    nr, dr = (Rd if Rd is not None else Rh).shape
    if dq != dr:
        raise ValueError(f"query has {dq} features, reference {dr}: both must live in the same space")
    if not 1 <= dq <= _capi.HMX_MAX_PCS:
        raise ValueError(f"the embedding must have 1..{_capi.HMX_MAX_PCS} features (HMX_MAX_PCS), got {dq}")
    if nq < 1 or nr < 1:
        raise ValueError("query and reference must hold at least one cell each")
    if isinstance(k, bool) or int(k) != k:
        raise ValueError(f"k must be an integer, got {k!r}")
    k = int(k)
    if not 1 <= k <= _MAX_NEIGHBOURS:
        raise ValueError(f"k must lie in [1, {_MAX_NEIGHBOURS}] in this build (got {k})")
    if k > nr:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, n_samples_fit = {nr}")
    owners = {t.device.index if t.device.index is not None else 0 for t in (Qd, Rd) if t is not None}
    if len(owners) > 1:
        raise ValueError(f"query and reference live on different devices (cuda:{sorted(owners)[0]} and cuda:{sorted(owners)[1]})")
    dev = None
    if owners:
        dev = owners.pop()
        if device is not None and ":" in str(device) and _device_index(device) != dev:
            raise ValueError(f"device={device!r} but the data lives on cuda:{dev}")
    else:
        _device_index(device)                                                   # a bad device name fails here
    return Qd, Rd, Qh, Rh, dev, k, nr


def _strides(t):
    # a dimension of one element may carry any stride: give the library a valid one
    return tuple(st if n > 1 else 1 for st, n in zip(t.stride(), t.shape))


def _run(resolved, device, codes, slices):
    """hmx_knn_predict on the current stream of the data's device (``resolved``: what _resolve returned).  Returns
    (pred, prob, dist, idx) as device tensors (pred / prob None without labels) and whether the inputs were all on the
    host.  ``slices``: hmx_knn_predict's (0 = automatic)."""
    import torch
    Qd, Rd, Qh, Rh, dev, k, _ = resolved
    on_host = dev is None
    if on_host:
        dev = _device_index(device)
    tdev = torch.device("cuda", dev)
    n_labels = 0 if codes is None else codes.shape[0]
    lib = _capi.load()
    with torch.cuda.device(tdev):
        # a host set is copied to the device exactly, as float64
        Q = Qd if Qd is not None else torch.from_numpy(np.ascontiguousarray(Qh)).to(tdev)
        R = Rd if Rd is not None else torch.from_numpy(np.ascontiguousarray(Rh)).to(tdev)
        nq, d = Q.shape
        nr = R.shape[0]
        pred = prob = None
        if n_labels:
            pred = torch.empty((nq, n_labels), dtype=torch.int32, device=tdev)
            prob = torch.empty((nq, n_labels), dtype=torch.float64, device=tdev)
        dist = torch.empty((nq, k), dtype=torch.float64, device=tdev)
        idx = torch.empty((nq, k), dtype=torch.int32, device=tdev)
        (qsc, qsf), (rsc, rsf) = _strides(Q), _strides(R)
        rc = lib.hmx_knn_predict(dev, Q.data_ptr(), _device_dtype(Q, "query"), nq, qsc, qsf,
                                 R.data_ptr(), _device_dtype(R, "reference"), nr, rsc, rsf, d, k, int(slices),
                                 torch.cuda.current_stream(tdev).cuda_stream,
                                 _capi._ptr(codes), n_labels,
                                 pred.data_ptr() if pred is not None else None,
                                 prob.data_ptr() if prob is not None else None, dist.data_ptr(), idx.data_ptr())
        _raise_on_error(lib, rc)
    return pred, prob, dist, idx, on_host


def knn_query(query, reference, k, device=None, _slices=0):
    """The ``k`` reference cells nearest to every query cell: ``(dist, idx)``, each ``n_query x k``, nearest first.

    Exact Euclidean distances (float64, from direct differences, the square root as sklearn's ``kneighbors`` reports
    it), ties broken by the smaller reference index.  ``query`` and ``reference`` are cells x features with the same
    features: NumPy arrays or CPU tensors, or 2-D tensors on a HIP device (or ROCm ``__dlpack__`` producers) of float32 /
    float16 / bfloat16 / float64 with any strides, read in place.  Every element converts to float64 exactly, so device
    input gives what NumPy input of the same values gives, bit for bit.  If either set lives on a device, both are read
    there (a host set is copied there; a set on another device is a ValueError) and the results are device tensors
    (float64 / int32), ordered on that device's current stream; otherwise they are NumPy arrays.  ``device``: the GPU for
    host input (``'cuda'`` or ``'cuda:n'``).  Limits: 1..320 features, ``1 <= k <= min(n_reference, 2040)``."""
    _, _, dist, idx, on_host = _run(_resolve(query, reference, k, device), device, None, _slices)
    return (dist.cpu().numpy(), idx.cpu().numpy()) if on_host else (dist, idx)


def knn_predict(query, reference, ref_meta, label_colnames, k=5, device=None, return_neighbors=False, _slices=0):
    """Transfer the reference's labels to the query by a vote of the ``k`` nearest reference cells (Symphony's
    ``knnPredict``).

    Returns a ``pandas.DataFrame`` with one row per query cell and, for every ``L`` in ``label_colnames``, a column ``L``
    (categorical, with the categories of ``pd.Categorical(ref_meta[L])``): the category with the most votes among the
    cell's ``k`` neighbours, and a column ``L + "_prob"`` (float64): that category's votes / k.  Tied categories go to
    the one whose nearest member is the nearer neighbour (deterministic, unlike R's ``class::knn``, which picks at
    random).  ``ref_meta`` has one row per reference cell; a missing label value is a ValueError.

    ``query`` / ``reference`` / ``k`` / ``device`` as for ``knn_query``, whose neighbours the vote uses;
    ``return_neighbors=True`` returns ``(df, dist, idx)`` with them."""
    if isinstance(label_colnames, str):
        label_colnames = [label_colnames]
    label_colnames = list(label_colnames)
    if not label_colnames:
        raise ValueError("label_colnames is empty")
    resolved = _resolve(query, reference, k, device)
    nr = resolved[-1]
    if ref_meta.shape[0] != nr:
        raise ValueError(f"reference has {nr} cells, ref_meta {ref_meta.shape[0]} rows")
    missing = [c for c in label_colnames if c not in ref_meta.columns]
    if missing:
        raise ValueError(f"label columns {missing} not in ref_meta's columns")
    codes = _label_codes(ref_meta, label_colnames, nr)
    pred, prob, dist, idx, on_host = _run(resolved, device, codes, _slices)
    pred_h, prob_h = pred.cpu().numpy(), prob.cpu().numpy()
    cols = {}
    for i, label in enumerate(label_colnames):
        cats = pd.Categorical(ref_meta[label]).categories
        cols[label] = pd.Categorical.from_codes(pred_h[:, i], categories=cats)
        cols[label + "_prob"] = prob_h[:, i]
    df = pd.DataFrame(cols)
    if not return_neighbors:
        return df
    return (df, dist.cpu().numpy(), idx.cpu().numpy()) if on_host else (df, dist, idx)
