#!/usr/bin/env python3
"""Wall-clock of label transfer (knn_predict) at the sizes it is built for: one JSON line per case on stdout.

    python scripts/time_knn_predict.py [--cases a5,a30,b,c] [--repeats 3]

  a5 / a30 : 1 M query x 1 M reference cells x 50 PCs, k = 5 / k = 30
  b        : 10 k query x 1 M reference x 50, k = 5 (the reference cut into slices)
  c        : 100 k query x 10 M reference x 50, k = 5
Both sets are float32 device tensors (seeded Gaussian clusters, the query a second sample of the same population), with
one label column of 20 categories.  Every timed call ends in a device synchronise; a host clock around it; one warm-up,
then the median of ``--repeats``.  Per-kernel times come from a separate run under
``rocprofv3 --kernel-trace --stats -- python scripts/time_knn_predict.py --repeats 1``.  Needs an MI355X."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"a5": (1_000_000, 1_000_000, 5), "a30": (1_000_000, 1_000_000, 30), "b": (10_000, 1_000_000, 5),
         "c": (100_000, 10_000_000, 5)}
D = 50


def _cells(torch, n, seed, cent):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lab = torch.randint(0, cent.shape[0], (n,), device="cuda", generator=g)
    return cent[lab] + torch.randn((n, D), device="cuda", generator=g), lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a5,a30,b,c")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import pandas as pd
    import torch
    from harmonypy_amd import _capi, knn_predict
    lib = _capi.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    cent = torch.randn((20, D), device="cuda", generator=g) * 3
    for name in args.cases.split(","):
        nq, nr, k = CASES[name]
        R, rlab = _cells(torch, nr, 1, cent)
        Q, _ = _cells(torch, nq, 2, cent)
        meta = pd.DataFrame({"type": rlab.cpu().numpy().astype(np.int32)})
        torch.cuda.synchronize()

        def one():
            df = knn_predict(Q, R, meta, ["type"], k=k)
            torch.cuda.synchronize()
            return df
        one()
        laps = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            one()
            laps.append(time.perf_counter() - t0)
        print(json.dumps({
            "metric": "knn_predict_seconds", "case": name, "value": round(float(np.median(laps)), 4), "unit": "s",
            "higher_is_better": False, "laps_s": [round(x, 4) for x in laps],
            "config": {"query_cells": nq, "reference_cells": nr, "d": D, "k": k, "input": "float32 device tensors"},
            "slices": int(lib.hmx_knn_slices(0, nq, nr, D, k)),
            "search_flops": 2 * nq * nr * D,
        }), flush=True)
        del R, Q, rlab
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
