"""Reference mapping: place new query cells onto a finished Harmony reference without running Harmony on the union.

The reference is compressed into per-cluster sums of its final state (``HarmonyReference``: K x (d + 1) numbers).
``map_query`` soft-assigns the query to the reference's centroids in the corrected space and moves it by one
mixture-of-experts ridge step whose intercept carries the reference's mass, as in Symphony (Kang et al., Nat. Commun.
12, 5890, 2021): the query moves, the reference does not.  The per-cell work runs in ``libhmx.so``
(``include/hmx_map.h``); the formulation is in DESIGN.md, section "Reference mapping".
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from . import _capi
from .harmony import (Harmony, _EngineArrays, _engine_device, _prepare_inputs, _validate_arguments,
                      build_layout, logger)

FORMAT_VERSION = 1


class HarmonyReference:
    """The summary of a finished reference that query cells are mapped onto.

    ``cluster_sums`` (K x d float64) = sum_i R[k,i] Z_corr[:,i], ``cluster_mass`` (K float64) = sum_i R[k,i] -- from the
    last soft assignment R and the corrected embedding Z_corr after the last ridge; ``sigma`` (K float32) the reference's
    per-cluster sigma; ``n_cells`` its number of cells.  ``Harmony.reference()`` computes it on the device,
    ``from_arrays`` from any R and Z_corr (harmonypy's own included)."""

    def __init__(self, cluster_sums, cluster_mass, sigma, n_cells):
        self.cluster_sums = np.array(cluster_sums, dtype=np.float64)
        self.cluster_mass = np.array(cluster_mass, dtype=np.float64)
        self.sigma = np.array(sigma, dtype=np.float32)
        self.n_cells = int(n_cells)
        K = self.cluster_mass.shape[0] if self.cluster_mass.ndim == 1 else -1
        if self.cluster_sums.ndim != 2 or self.cluster_sums.shape[0] != K or self.sigma.shape != (K,):
            raise ValueError(f"cluster_sums {self.cluster_sums.shape}, cluster_mass {self.cluster_mass.shape} and sigma "
                             f"{self.sigma.shape} must be K x d, K and K")

    @property
    def K(self):
        return self.cluster_sums.shape[0]

    @property
    def d(self):
        return self.cluster_sums.shape[1]

    @property
    def centroids(self):
        """The reference's clusters in the corrected space: the rows of cluster_sums at unit length (K x d float32)."""
        return (self.cluster_sums / np.linalg.norm(self.cluster_sums, axis=1, keepdims=True)).astype(np.float32)

    @classmethod
    def from_arrays(cls, R, Z_corr, sigma):
        """From a finished reference's R (cells x K) and Z_corr (cells x d), in float64 on the host."""
        R = np.asarray(R, dtype=np.float64)
        Z = np.asarray(Z_corr, dtype=np.float64)
        if R.ndim != 2 or Z.ndim != 2 or R.shape[0] != Z.shape[0]:
            raise ValueError(f"R {R.shape} and Z_corr {Z.shape} must be cells x K and cells x d")
        sigma = np.asarray(sigma, dtype=np.float32)
        if sigma.ndim == 0:
            sigma = np.repeat(sigma, R.shape[1])
        return cls(R.T @ Z, R.sum(axis=0), sigma, R.shape[0])

    # ---- file format: an .npz of exactly these arrays ---------------------------------------------------------
    _FIELDS = {"format_version": np.int64, "cluster_sums": np.float64, "cluster_mass": np.float64, "sigma": np.float32,
               "n_cells": np.int64}

    def save(self, path):
        """Write the summary as an .npz (``format_version``, ``cluster_sums``, ``cluster_mass``, ``sigma``, ``n_cells``)."""
        with open(path, "wb") as f:
            np.savez(f, format_version=np.int64(FORMAT_VERSION), cluster_sums=self.cluster_sums,
                     cluster_mass=self.cluster_mass, sigma=self.sigma, n_cells=np.int64(self.n_cells))

    @classmethod
    def load(cls, path):
        """Read a file written by ``save``; ValueError for a different set of arrays, dtypes, shapes or version."""
        with np.load(path, allow_pickle=False) as z:
            if sorted(z.files) != sorted(cls._FIELDS):
                raise ValueError(f"{path}: expected the arrays {sorted(cls._FIELDS)}, found {sorted(z.files)}")
            a = {k: z[k] for k in z.files}
        for k, dt in cls._FIELDS.items():
            if a[k].dtype != dt:
                raise ValueError(f"{path}: {k} is {a[k].dtype}, expected {np.dtype(dt)}")
        for k in ("format_version", "n_cells"):
            if a[k].shape != ():
                raise ValueError(f"{path}: {k} must be a scalar")
        if int(a["format_version"]) != FORMAT_VERSION:
            raise ValueError(f"{path}: format version {int(a['format_version'])}, this build reads {FORMAT_VERSION}")
        S, m, s = a["cluster_sums"], a["cluster_mass"], a["sigma"]
        if S.ndim != 2 or m.shape != (S.shape[0],) or s.shape != (S.shape[0],):
            raise ValueError(f"{path}: cluster_sums {S.shape}, cluster_mass {m.shape} and sigma {s.shape} must be K x d, K and K")
        return cls(S, m, s, int(a["n_cells"]))


def map_query(data_mat, meta_data, reference, vars_use=None, lamb=None, alpha=0.2, sigma=None, device=None, verbose=True):
    """Map query cells onto a finished reference: returns a ``HarmonyQuery`` whose ``Z_corr`` lies in the reference's
    corrected space.  The reference does not move.

    ``data_mat``: the query in the reference's PC space, as ``run_harmony`` takes it (NumPy, a CPU tensor, or a tensor on
    a HIP device of float32 / float16 / bfloat16 / float64 with any strides, read in place); cells x PCs or PCs x cells.
    ``meta_data``: the query's cells x variables.  ``reference``: a ``HarmonyReference`` or a finished ``Harmony``.
    ``vars_use``: the query's batch column(s); None treats the whole query as one batch.  ``lamb`` / ``alpha``: as in
    ``run_harmony`` (``lamb=-1`` estimates lambda from the query's own expected mass).  ``sigma``: per-cluster sigma
    (scalar or K values), default the reference's."""
    ref = reference.reference() if isinstance(reference, Harmony) else reference
    if not isinstance(ref, HarmonyReference):
        raise TypeError(f"reference must be a HarmonyReference or a finished Harmony, got {type(reference).__name__}")
    N = meta_data.shape[0]
    shape = tuple(data_mat.shape) if hasattr(data_mat, "shape") else np.shape(data_mat)
    if len(shape) != 2 or N not in shape:
        raise ValueError(f"data_mat {shape} and meta_data ({N} cells) do not have the same number of cells")
    d = shape[0] if shape[1] == N else shape[1]
    if d != ref.d:
        raise ValueError(f"the query has {d} PCs, the reference {ref.d}: project the query into the reference's PC space")
    if vars_use is None:
        vars_use = ["_query"]
        meta_data = pd.DataFrame({"_query": np.zeros(N, dtype=np.int8)})
    names = [vars_use] if isinstance(vars_use, str) else list(vars_use)
    missing = [v for v in names if v not in meta_data.columns]
    if missing:
        raise ValueError(f"vars_use {missing} not in meta_data's columns")
    if sigma is None:
        sigma = ref.sigma
    sigma = np.asarray(sigma, dtype=np.float32)
    if sigma.ndim == 0:
        sigma = np.repeat(sigma, ref.K)
    if sigma.shape != (ref.K,):
        raise ValueError(f"sigma has {sigma.size} entries, the reference has {ref.K} clusters")
    if not (np.all(np.isfinite(ref.cluster_sums)) and np.all(np.isfinite(ref.cluster_mass))):
        raise ValueError("the reference's cluster_sums / cluster_mass are not finite")
    _validate_arguments(ref.K, 1.0, meta_data, vars_use)
    p = _prepare_inputs(data_mat, meta_data, vars_use, theta=0, lamb=lamb, sigma=sigma, nclust=ref.K)
    dev = _engine_device(device, p["Z"] if p["on_device"] else None)
    if verbose:
        logger.info(f"Mapping {N} query cells onto a reference of {ref.n_cells} cells (K={ref.K}, d={ref.d}) on device {dev}")
    return HarmonyQuery(p, ref, alpha, dev)


class HarmonyQuery(_EngineArrays):
    """Query cells mapped onto a reference (``map_query``).  ``Z_corr`` / ``Z_orig`` / ``Z_cos`` / ``R`` (cells x d or
    K, NumPy) and ``to_tensor`` as on ``Harmony``; ``Y`` the reference's centroids (d x K) as the engine used them."""

    def __init__(self, p, reference, alpha, device_id):
        Z = p["Z"]
        self.d, self.N = Z.shape
        self.K = reference.K
        self._device_id = device_id
        self._offset = 0
        self.alpha = alpha
        self.lambda_estimation = bool(p["lambda_estimation"])
        codes = p["codes"]
        self.B = codes.n_batches
        self._Pr_b = np.asarray(p["Pr_b"], dtype=np.float32)
        self._theta = np.zeros(self.B, dtype=np.float32)
        self._sigma = np.asarray(p["sigma"], dtype=np.float32)
        self._lamb = np.asarray(p["lamb"], dtype=np.float32)
        if not self.lambda_estimation and self._lamb.shape != (self.B + 1,):
            raise ValueError("lamb must have B+1 entries (intercept first)")
        (self._group_cols, self._order, _gid,
         self._static_cells, self._static_tile_grp) = build_layout(codes.codes)
        self._engine = _capi.Engine(self.N, self.d, self.K, self.B, self._group_cols.shape[0], codes.codes.shape[1], 1,
                                    lambda_estimation=self.lambda_estimation, alpha=alpha, device_id=device_id)
        self._upload(Z, None if self.lambda_estimation else self._lamb)
        self._engine.map_query(reference.cluster_sums, reference.cluster_mass)

    @property
    def lamb(self):
        return self._lamb.copy()

    @property
    def sigma(self):
        return self._sigma.copy()

    def result(self):
        """The mapped query as a NumPy array (N x d)."""
        return self.Z_corr

    def knn_predict(self, reference_Z_corr, ref_meta, label_colnames, k=5, return_neighbors=False):
        """The reference's labels transferred to the mapped query: ``knn_predict(self.to_tensor("Z_corr"),
        reference_Z_corr, ...)`` (see there).  ``reference_Z_corr``: the reference's corrected embedding, cells x PCs
        (``Harmony.to_tensor("Z_corr")`` keeps it on the device), with ``ref_meta`` one row per reference cell."""
        from .knn import knn_predict
        return knn_predict(self.to_tensor("Z_corr"), reference_Z_corr, ref_meta, label_colnames, k=k,
                           return_neighbors=return_neighbors)

    def cluster_moments(self, space="orig", groups=None):
        """``ClusterMoments`` of the query's cells in ``space`` ("orig": the query's PCs as given, "corr": mapped): under
        its soft assignment to the reference's clusters, or, with ``groups`` (one label per cell, anything
        ``pd.Categorical`` takes), per group in the order of the categories.  A group without cells has NaN moments."""
        from .confidence import query_moments
        return query_moments(self, space, groups)

    def mapping_score(self, moments, ridge=0.0, as_tensor=False):
        """Per-cell mapping confidence (Symphony's per-cell mapping metric): ``score[j] = sum_k R[j,k] D[k,j]`` with
        ``D[k,j]`` the Mahalanobis distance of query cell j from reference cluster k, ``sqrt((x_j - mean_k)^T (cov_k +
        ridge (tr cov_k / d) I)^-1 (x_j - mean_k))``.  Low: the cell lies inside the reference clusters it was assigned to
        (for Gaussian clusters D^2 averages d); high: the reference has nothing like it.

        ``moments``: the reference's ``ClusterMoments`` (``Harmony.cluster_moments``, ``ClusterMoments.from_arrays``,
        ``ClusterMoments.load``) or the finished ``Harmony`` itself (its ``cluster_moments("orig")``); the query is
        measured in the space the moments were taken in.  Returns N float64 in the caller's cell order: NumPy, or with
        ``as_tensor`` a tensor on the engine's device, ordered on the current stream, with the same bits.  ValueError
        for a K or d mismatch, non-finite moments, a negative ridge, or clusters whose covariance is not positive
        definite (``ridge > 0`` regularises them)."""
        from .confidence import mapping_score
        return mapping_score(self, moments, ridge, as_tensor)

    def cluster_mapping_score(self, moments, groups, ridge=0.0, min_cells_per_dim=2):
        """Per-cluster mapping confidence (Symphony's per-cluster mapping metric) for the query groups ``groups`` (one
        label per cell: the query's own clustering, predicted labels): the Mahalanobis distance of every reference
        cluster mean from the group's mean in the group's own covariance (+ ridge (tr / d) I), averaged with the
        group's mean soft assignment.  Returns a DataFrame indexed by the categories of ``pd.Categorical(groups)`` with
        ``n_cells`` and ``score``; NaN for a group of fewer than ``min_cells_per_dim * d`` cells or with a covariance
        that is not positive definite."""
        from .confidence import cluster_mapping_score
        return cluster_mapping_score(self, moments, groups, ridge, min_cells_per_dim)
