#!/usr/bin/env python3
"""Wall-clock of reference mapping at BASELINE.json configs[2]'s shape (C3): one JSON line on stdout.

    python scripts/time_map_query.py [--cells 1000000] [--repeats 3]

1. A reference: synthetic 1M cells x 50 PCs, 8 batches, K=100 (bench.synthetic_dataset, seed 0), harmonized with a fixed
   round schedule.
2. ``Harmony.reference()`` (one R^T.Z_corr pass and the copy of the K x (d+1) summary to the host).
3. ``map_query`` of a second seeded population sample of the same size from a float32 device tensor (engine set-up,
   upload, assignment, ridge statistics, solve, apply).
Every timed call ends in a device synchronise; a host clock around it; one warm-up, then the median of ``--repeats``.
The engine's own per-family kernel times (hmx_kernel_times, HIP events) of one further call are reported beside them.
Needs an MI355X."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_s(fn, repeats):
    fn()                                                  # warm-up
    laps = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        laps.append(time.perf_counter() - t0)
    return float(np.median(laps)), laps


def _families(engine, names):
    t = engine.kernel_times()
    return {n: {"ms": round(t[n][0], 4), "launches": t[n][1]} for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    from bench import synthetic_dataset
    from harmonypy_amd import map_query, run_harmony

    N, d, B, K = args.cells, 50, 8, 100
    Z, meta = synthetic_dataset(N, d, B, K, seed=0)
    t0 = time.perf_counter()
    ho = run_harmony(Z, meta, "batch", nclust=K, max_iter_harmony=2, verbose=False, random_state=0, _schedule=[5, 5])
    t_ref_build = time.perf_counter() - t0

    t_summary, laps_summary = _median_s(ho.reference, args.repeats)
    ref = ho.reference()
    ho._engine.enable_timing(True)
    ho.reference()
    fam_summary = _families(ho._engine, ["ridge_stats"])
    ho._engine.enable_timing(False)

    Zq, meta_q = synthetic_dataset(N, d, B, K, seed=0, cell_seed=1)
    xq = torch.from_numpy(Zq).to("cuda")
    torch.cuda.synchronize()
    box = {}

    def one_map():
        box["q"] = map_query(xq, meta_q, ref, vars_use="batch", verbose=False)
        torch.cuda.synchronize()

    t_map, laps_map = _median_s(one_map, args.repeats)
    q = box["q"]
    q._engine.enable_timing(True)
    q._engine.map_query(ref.cluster_sums, ref.cluster_mass)   # the library call alone, on the uploaded query
    fam_map = _families(q._engine, ["assign_init", "block_table", "ridge_stats", "ridge_solve", "ridge_apply"])
    q._engine.enable_timing(False)
    t_lib, laps_lib = _median_s(lambda: q._engine.map_query(ref.cluster_sums, ref.cluster_mass), args.repeats)

    print(json.dumps({
        "metric": "map_query_seconds", "value": round(t_map, 4), "unit": "s", "higher_is_better": False,
        "config": {"reference_cells": N, "query_cells": N, "d": d, "batches": B, "K": K, "query_input": "float32 device tensor"},
        "reference_build_s": round(t_ref_build, 3),
        "reference_summary_s": round(t_summary, 5), "reference_summary_laps_s": [round(x, 5) for x in laps_summary],
        "reference_summary_kernels": fam_summary,
        "map_query_s": round(t_map, 4), "map_query_laps_s": [round(x, 4) for x in laps_map],
        "hmx_map_query_s": round(t_lib, 5), "hmx_map_query_laps_s": [round(x, 5) for x in laps_lib],
        "hmx_map_query_kernels": fam_map,
    }))


if __name__ == "__main__":
    main()
