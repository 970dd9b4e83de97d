#!/usr/bin/env python3
"""Wall-clock of the mapping-confidence stage (cluster_moments, mapping_score) at the sizes it is built for, beside the
same two computations in PyTorch float64 on the same GPU: one JSON line per (case, computation, path) on stdout.

    python scripts/time_mapping_score.py [--cases c3,c4] [--repeats 3] [--no-torch]

  c3 : 1 M reference x 1 M query cells x 50 PCs, K = 100
  c4 : 1.25 M reference x 1.25 M query cells x 200 PCs, K = 200 (the shard shape of the largest benchmark configuration)
Reference and query are seeded Gaussian clusters, both placed on a K-cluster summary with ``map_query`` (a mapped query
is a clustered engine like a finished run, and costs a fraction of one), so R, Z_orig and Z_corr are resident as they are
after ``run_harmony`` / ``map_query``.  The PyTorch path is what a user would write today from ``to_tensor`` outputs:
float64 ``baddbmm`` / ``bmm`` over chunks of cells so that the K x chunk x d temporaries fit.  Every timed call ends in a
device synchronise; a host clock around it; one warm-up, then the median of ``--repeats``.  Per-kernel times come from
a separate run under ``rocprofv3 --kernel-trace --stats -- python scripts/time_mapping_score.py --repeats 1 --no-torch``.
Needs an MI355X."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"c3": (1_000_000, 1_000_000, 50, 100), "c4": (1_250_000, 1_250_000, 200, 200)}


def _cells(torch, n, d, seed, cent):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lab = torch.randint(0, cent.shape[0], (n,), device="cuda", generator=g)
    return cent[lab] + 0.5 * torch.randn((n, d), device="cuda", generator=g)


def torch_moments(torch, R, Z, chunk):
    """(mass, mass_sq, mean, cov) in float64, two passes over chunks of cells, centred."""
    K, d = R.shape[1], Z.shape[1]
    mass = torch.zeros(K, dtype=torch.float64, device=R.device)
    mass_sq = torch.zeros_like(mass)
    sums = torch.zeros((K, d), dtype=torch.float64, device=R.device)
    for s in range(0, R.shape[0], chunk):
        r, z = R[s:s + chunk].double(), Z[s:s + chunk].double()
        mass += r.sum(0)
        mass_sq += (r * r).sum(0)
        sums += r.T @ z
    mean = sums / mass[:, None]
    acc = torch.zeros((K, d, d), dtype=torch.float64, device=R.device)
    for s in range(0, R.shape[0], chunk):
        r, z = R[s:s + chunk].double(), Z[s:s + chunk].double()
        c = z[None] - mean[:, None]                                   # K x chunk x d
        acc.baddbmm_((c * r.T[:, :, None]).transpose(1, 2), c)
    cov = acc / mass[:, None, None] / (1 - mass_sq / mass ** 2)[:, None, None]
    return mass, mass_sq, mean, cov


def torch_score(torch, R, Z, mean, T, chunk):
    out = torch.empty(R.shape[0], dtype=torch.float64, device=R.device)
    Tt = T.transpose(1, 2).contiguous()
    for s in range(0, R.shape[0], chunk):
        r, z = R[s:s + chunk].double(), Z[s:s + chunk].double()
        y = torch.bmm(z[None] - mean[:, None], Tt)                   # K x chunk x d
        out[s:s + chunk] = (r.T * y.norm(dim=2)).sum(0)
    return out


def _timed(torch, fn, repeats):
    fn()
    torch.cuda.synchronize()
    laps = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        laps.append(time.perf_counter() - t0)
    return float(np.median(laps)), laps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3,c4")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="time the library alone (for a kernel trace)")
    args = ap.parse_args()
    import pandas as pd
    import torch
    from harmonypy_amd import HarmonyReference, map_query
    from harmonypy_amd.confidence import whitening
    for name in args.cases.split(","):
        n_ref, n_q, d, K = CASES[name]
        g = torch.Generator(device="cuda").manual_seed(0)
        cent = torch.randn((K, d), device="cuda", generator=g, dtype=torch.float32) * 3
        summary = HarmonyReference(cent.double().cpu().numpy() * (n_ref / K), np.full(K, n_ref / K), np.full(K, 0.1), n_ref)
        ref = map_query(_cells(torch, n_ref, d, 1, cent), pd.DataFrame({"b": np.zeros(n_ref, np.int8)}), summary, verbose=False)
        qry = map_query(_cells(torch, n_q, d, 2, cent), pd.DataFrame({"b": np.zeros(n_q, np.int8)}), summary, verbose=False)
        torch.cuda.synchronize()
        cfg = {"reference_cells": n_ref, "query_cells": n_q, "d": d, "K": K}

        def emit(metric, path, med, laps, flops, **extra):
            print(json.dumps({"metric": metric, "case": name, "path": path, "value": round(med, 4), "unit": "s",
                              "higher_is_better": False, "laps_s": [round(x, 4) for x in laps], "config": cfg,
                              "flops_2NKd2": flops, "tflops_of_2NKd2": round(flops / med / 1e12, 2), **extra}), flush=True)

        box = {}
        med, laps = _timed(torch, lambda: box.__setitem__("m", ref.cluster_moments("orig")), args.repeats)
        emit("cluster_moments_seconds", "hip", med, laps, 2 * n_ref * K * d * d)
        m = box["m"]
        t0 = time.perf_counter()
        T, t, invalid = whitening(m, 0.0)
        host_s = time.perf_counter() - t0
        assert not invalid
        med, laps = _timed(torch, lambda: box.__setitem__("s", qry.mapping_score(m, as_tensor=True)), args.repeats)
        emit("mapping_score_seconds", "hip", med, laps, 2 * n_q * K * d * d, host_factorisations_s=round(host_s, 4))
        if args.no_torch:
            del ref, qry
            torch.cuda.empty_cache()
            continue
        chunk = max(1024, (1 << 28) // (K * d * 8) // 1024 * 1024)     # K x chunk x d float64 temporaries of 256 MiB
        R, Z = ref.to_tensor("R"), ref.to_tensor("Z_orig")
        med, laps = _timed(torch, lambda: box.__setitem__("tm", torch_moments(torch, R, Z, chunk)), args.repeats)
        cov_t = box["tm"][3].cpu().numpy()
        dg = np.sqrt(np.einsum("kii->ki", cov_t))
        agree = float(np.max(np.abs(m.cov - cov_t) / (dg[:, :, None] * dg[:, None, :])))
        emit("cluster_moments_seconds", "torch_float64", med, laps, 2 * n_ref * K * d * d, chunk=chunk, cov_difference=agree)
        del R, Z
        R, Z = qry.to_tensor("R"), qry.to_tensor("Z_orig")
        mean_t, T_t = torch.from_numpy(m.mean).cuda(), torch.from_numpy(T).cuda()
        med, laps = _timed(torch, lambda: box.__setitem__("ts", torch_score(torch, R, Z, mean_t, T_t, chunk)), args.repeats)
        agree = float((box["ts"] - box["s"]).abs().div(box["s"]).max())
        emit("mapping_score_seconds", "torch_float64", med, laps, 2 * n_q * K * d * d, chunk=chunk, score_difference=agree)
        del R, Z, ref, qry, box
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
