"""One rank of a sharded reference whose summary is taken with Harmony.reference(); launched by
tests/test_map_query_gpu.py as ``python tests/_map_shard_worker.py <outdir>`` with RANK / WORLD_SIZE / MASTER_ADDR /
MASTER_PORT in the environment (gloo rendezvous on 127.0.0.1).  The pbmc_default replay (golden Y0 and round schedule)
over two slices of the cells; every rank writes <outdir>/rank<r>.npz with its summary and its slices of R and Z_corr.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    outdir = sys.argv[1]
    import torch.distributed as dist
    from conftest import load_case
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    data, meta, vars_use, kw, g = load_case("pbmc_default")
    N = data.shape[0]
    cuts = np.linspace(0, N, world + 1).astype(int)
    if world > 1:
        cuts[1] = max(1, cuts[1] - N // 7)
    lo, hi = cuts[rank], cuts[rank + 1]
    from harmonypy_amd import Shard
    from harmonypy_amd import harmony as H
    os.environ["HMX_UPDATE_ORDER"] = "torch"
    ho = H.run_harmony(data[lo:hi].astype(np.float32), meta.iloc[lo:hi].reset_index(drop=True), vars_use, verbose=False,
                       shard=Shard(transport="host"), _y0=g["Y0"], _schedule=[int(r) for r in g["kmeans_rounds"]], **kw)
    ref = ho.reference()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), lo=lo, hi=hi, cluster_sums=ref.cluster_sums,
             cluster_mass=ref.cluster_mass, n_cells=ref.n_cells, R=ho.R, Z_corr=ho.Z_corr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
