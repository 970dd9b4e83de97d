"""Mapping confidence: did a mapped query cell (a query cluster) land where the reference has cells?

Symphony's mapping metrics (Kang et al., Nat. Commun. 12, 5890, 2021) on the engine's state: ``ClusterMoments`` holds the
reference's weighted mean and unbiased weighted covariance per soft cluster; ``HarmonyQuery.mapping_score`` is every
query cell's Mahalanobis distance to the reference's clusters, weighted by its soft assignment;
``HarmonyQuery.cluster_mapping_score`` the distance of the reference's cluster means from a query group in that group's
own covariance.  The per-cell sums run in ``libhmx.so`` (``include/hmx_score.h``) in float64; the K (or G) small
factorisations run here in float64 NumPy.  The formulation is in DESIGN.md, section "Mapping confidence".
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from . import _capi

FORMAT_VERSION = 1
SPACES = {"orig": _capi.HMX_Z_ORIG, "corr": _capi.HMX_Z_CORR}


def _check_space(space):
    if space not in SPACES:
        raise ValueError(f"space={space!r}: expected 'orig' (the PCs before correction) or 'corr' (Z_corr)")
    return space


class ClusterMoments:
    """Per-cluster moments of a weighted set of cells: ``mass`` = sum_i w, ``mass_sq`` = sum_i w^2 (G), ``mean`` (G x d),
    ``cov`` (G x d x d, the unbiased weighted covariance: ``np.cov(Z.T, aweights=w, ddof=1)``), all float64; ``space``
    the embedding they were taken in ("orig" / "corr") and ``n_cells``.  ``Harmony.cluster_moments`` /
    ``HarmonyQuery.cluster_moments`` compute them on the device, ``from_arrays`` from any R and Z."""

    def __init__(self, mass, mass_sq, mean, cov, space="orig", n_cells=0):
        self.mass = np.array(mass, dtype=np.float64)
        self.mass_sq = np.array(mass_sq, dtype=np.float64)
        self.mean = np.array(mean, dtype=np.float64)
        self.cov = np.array(cov, dtype=np.float64)
        self.space = _check_space(str(space))
        self.n_cells = int(n_cells)
        G = self.mass.shape[0] if self.mass.ndim == 1 else -1
        d = self.mean.shape[1] if self.mean.ndim == 2 else -1
        if self.mass_sq.shape != (G,) or self.mean.shape != (G, d) or self.cov.shape != (G, d, d):
            raise ValueError(f"mass {self.mass.shape}, mass_sq {self.mass_sq.shape}, mean {self.mean.shape} and cov "
                             f"{self.cov.shape} must be G, G, G x d and G x d x d")

    @property
    def K(self):
        return self.mean.shape[0]

    @property
    def d(self):
        return self.mean.shape[1]

    @classmethod
    def from_arrays(cls, R, Z, space="orig"):
        """From a soft assignment R (cells x K) and an embedding Z (cells x d), in float64 on the host."""
        R = np.asarray(R, dtype=np.float64)
        Z = np.asarray(Z, dtype=np.float64)
        if R.ndim != 2 or Z.ndim != 2 or R.shape[0] != Z.shape[0]:
            raise ValueError(f"R {R.shape} and Z {Z.shape} must be cells x K and cells x d")
        K, d = R.shape[1], Z.shape[1]
        mass, mass_sq = R.sum(axis=0), (R * R).sum(axis=0)
        mean, cov = np.full((K, d), np.nan), np.full((K, d, d), np.nan)
        for k in range(K):
            if not mass[k] > 0:
                continue
            mean[k] = R[:, k] @ Z / mass[k]
            C = Z - mean[k]
            with np.errstate(divide="ignore", invalid="ignore"):
                cov[k] = (C.T * R[:, k]) @ C / mass[k] / (1.0 - mass_sq[k] / mass[k] ** 2)
        return cls(mass, mass_sq, mean, cov, space, R.shape[0])

    # ---- file format: an .npz of exactly these arrays ---------------------------------------------------------
    _FIELDS = {"format_version": np.int64, "mass": np.float64, "mass_sq": np.float64, "mean": np.float64,
               "cov": np.float64, "space": np.str_, "n_cells": np.int64}

    def save(self, path):
        """Write the moments as an .npz (``format_version``, ``mass``, ``mass_sq``, ``mean``, ``cov``, ``space``,
        ``n_cells``)."""
        with open(path, "wb") as f:
            np.savez(f, format_version=np.int64(FORMAT_VERSION), mass=self.mass, mass_sq=self.mass_sq, mean=self.mean,
                     cov=self.cov, space=np.str_(self.space), n_cells=np.int64(self.n_cells))

    @classmethod
    def load(cls, path):
        """Read a file written by ``save``; ValueError for a different set of arrays, dtypes, shapes or version."""
        with np.load(path, allow_pickle=False) as z:
            if sorted(z.files) != sorted(cls._FIELDS):
                raise ValueError(f"{path}: expected the arrays {sorted(cls._FIELDS)}, found {sorted(z.files)}")
            a = {k: z[k] for k in z.files}
        for k, dt in cls._FIELDS.items():
            if (a[k].dtype.kind != "U") if dt is np.str_ else (a[k].dtype != dt):
                raise ValueError(f"{path}: {k} is {a[k].dtype}, expected {np.dtype(dt)}")
        for k in ("format_version", "n_cells", "space"):
            if a[k].shape != ():
                raise ValueError(f"{path}: {k} must be a scalar")
        if int(a["format_version"]) != FORMAT_VERSION:
            raise ValueError(f"{path}: format version {int(a['format_version'])}, this build reads {FORMAT_VERSION}")
        if str(a["space"]) not in SPACES:
            raise ValueError(f"{path}: space is {str(a['space'])!r}, expected one of {sorted(SPACES)}")
        m, m2, mu, cov = a["mass"], a["mass_sq"], a["mean"], a["cov"]
        if m.ndim != 1 or mu.ndim != 2 or m2.shape != m.shape or mu.shape[0] != m.shape[0] or \
                cov.shape != (mu.shape[0], mu.shape[1], mu.shape[1]):
            raise ValueError(f"{path}: mass {m.shape}, mass_sq {m2.shape}, mean {mu.shape} and cov {cov.shape} must be "
                             "G, G, G x d and G x d x d")
        return cls(m, m2, mu, cov, str(a["space"]), int(a["n_cells"]))


def _check_ridge(ridge):
    if isinstance(ridge, bool) or not isinstance(ridge, (int, float, np.integer, np.floating)) or \
            not np.isfinite(ridge) or ridge < 0:
        raise ValueError(f"ridge must be a finite number >= 0, got {ridge!r}")
    return float(ridge)


def _cholesky(cov, ridge):
    """Lower Cholesky factor of cov + ridge * (tr cov / d) * I, or None when a pivot is not positive."""
    d = cov.shape[0]
    if not np.all(np.isfinite(cov)):
        return None
    try:
        L = np.linalg.cholesky(cov + ridge * (np.trace(cov) / d) * np.eye(d))
    except np.linalg.LinAlgError:
        return None
    return L if np.all(np.isfinite(L)) and np.all(np.diagonal(L) > 0) else None


def whitening(moments, ridge=0.0):
    """(T K x d x d, t K x d, invalid): per cluster T_k = L_k^-1 (lower triangular), L_k L_k^T = cov_k + ridge (tr cov_k / d)
    I, and t_k = T_k mean_k, so that |T_k x - t_k| is the Mahalanobis distance of x from the cluster.  ``invalid`` lists
    the clusters whose factorisation met a non-positive pivot (their T_k, t_k are NaN)."""
    K, d = moments.K, moments.d
    T, t, invalid = np.full((K, d, d), np.nan), np.full((K, d), np.nan), []
    eye = np.eye(d)
    for k in range(K):
        L = _cholesky(moments.cov[k], ridge)
        if L is not None:
            Tk = np.tril(np.linalg.solve(L, eye))
            if np.all(np.isfinite(Tk)):
                T[k], t[k] = Tk, Tk @ moments.mean[k]
                continue
        invalid.append(k)
    return T, t, invalid


def _as_moments(query, moments):
    """The ClusterMoments of ``moments`` (a finished Harmony gives its cluster_moments("orig")), checked against the
    query's K and d."""
    from .harmony import Harmony
    if not isinstance(moments, (ClusterMoments, Harmony)):
        raise TypeError(f"moments must be a ClusterMoments or a finished Harmony, got {type(moments).__name__}")
    if moments.K != query.K:                                   # a Harmony has K and d too: no GPU work before these
        raise ValueError(f"the moments have {moments.K} clusters, the query was mapped onto {query.K}")
    if moments.d != query.d:
        raise ValueError(f"the moments have {moments.d} PCs, the query {query.d}")
    return moments.cluster_moments("orig") if isinstance(moments, Harmony) else moments


def mapping_score(query, moments, ridge=0.0, as_tensor=False):
    """``HarmonyQuery.mapping_score`` (see there)."""
    ridge = _check_ridge(ridge)
    moments = _as_moments(query, moments)
    if not (np.all(np.isfinite(moments.mean)) and np.all(np.isfinite(moments.cov))):
        bad = sorted(set(np.nonzero(~np.isfinite(moments.mean).all(axis=1) | ~np.isfinite(moments.cov).all(axis=(1, 2)))[0].tolist()))
        raise ValueError(f"the moments of clusters {bad} are not finite (clusters without mass?)")
    T, t, invalid = whitening(moments, ridge)
    if invalid:
        raise ValueError(f"the covariance of clusters {invalid} is not positive definite with ridge={ridge:g} (fewer effective "
                         "cells than dimensions, or no spread along some direction): pass ridge > 0, e.g. ridge=1e-2")
    which = SPACES[moments.space]
    if not as_tensor:
        return query._engine.mapping_score(which, T, t)
    import torch
    dev = torch.device("cuda", query._device_id)
    out = torch.empty(query.N, dtype=torch.float64, device=dev)
    query._engine.mapping_score(which, T, t, out_ptr=out.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    return out


def _group_codes(groups, N):
    cat = groups if isinstance(groups, pd.Categorical) else pd.Categorical(np.asarray(groups))
    if len(cat) != N:
        raise ValueError(f"groups has {len(cat)} entries, the query {N} cells")
    if (cat.codes < 0).any():
        raise ValueError("groups has missing values")
    if len(cat.categories) > 4096:
        raise ValueError(f"groups has {len(cat.categories)} categories, at most 4096 are supported")
    return cat, np.ascontiguousarray(cat.codes, dtype=np.int32)


def query_moments(query, space="orig", groups=None):
    """``HarmonyQuery.cluster_moments`` (see there)."""
    _check_space(space)
    if groups is None:
        return ClusterMoments(*query._engine.cluster_moments(SPACES[space]), space, query.N)
    cat, codes = _group_codes(groups, query.N)
    return ClusterMoments(*query._engine.cluster_moments(SPACES[space], codes, len(cat.categories)), space, query.N)


def _mean_assignment(query, codes, G, chunk=1 << 18):
    """rbar[g, k] = mean of R[j, k] over the cells of group g (float64, on the device; G x K on the host)."""
    import torch
    R = query.to_tensor("R")
    idx = torch.from_numpy(codes.astype(np.int64)).to(R.device)
    acc = torch.zeros((G, query.K), dtype=torch.float64, device=R.device)
    for s in range(0, query.N, chunk):
        acc.index_add_(0, idx[s:s + chunk], R[s:s + chunk].double())
    n = np.bincount(codes, minlength=G).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return acc.cpu().numpy() / n[:, None]


def cluster_mapping_score(query, moments, groups, ridge=0.0, min_cells_per_dim=2):
    """``HarmonyQuery.cluster_mapping_score`` (see there)."""
    ridge = _check_ridge(ridge)
    if isinstance(min_cells_per_dim, bool) or not isinstance(min_cells_per_dim, (int, float, np.integer, np.floating)) or \
            not min_cells_per_dim >= 0:
        raise ValueError(f"min_cells_per_dim must be a number >= 0, got {min_cells_per_dim!r}")
    moments = _as_moments(query, moments)
    if not np.all(np.isfinite(moments.mean)):
        raise ValueError("the moments' cluster means are not finite (clusters without mass?)")
    cat, codes = _group_codes(groups, query.N)
    G, d = len(cat.categories), query.d
    mass, _, mean_q, cov_q = query._engine.cluster_moments(SPACES[moments.space], codes, G)
    n = np.rint(mass).astype(np.int64)
    rbar = _mean_assignment(query, codes, G) if G else np.zeros((0, query.K))
    score = np.full(G, np.nan)
    for g in range(G):
        if n[g] < min_cells_per_dim * d or n[g] < 2:
            continue
        L = _cholesky(cov_q[g], ridge)
        if L is None:
            continue
        y = np.linalg.solve(L, (moments.mean - mean_q[g]).T)
        score[g] = float(rbar[g] @ np.sqrt((y * y).sum(axis=0)))
    return pd.DataFrame({"n_cells": n, "score": score}, index=cat.categories)
