"""One rank of a sharded run whose inputs and outputs live on the GPU; launched by tests/test_device_io_gpu.py as
``python tests/_device_io_shard_worker.py <case> <outdir> <source>`` with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT
in the environment (gloo rendezvous on 127.0.0.1).

source
  numpy    this rank's slice of the embedding as a NumPy array (the host path)
  device   the same slice as a torch tensor on the GPU, d x N and strided (a .T view); the result is read back with
           Harmony.to_tensor
Every rank writes <outdir>/rank<r>.npz with its slice of Z_corr and of the upload state (Z_orig, Z_cos).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    case, outdir, source = sys.argv[1:4]
    import torch
    import torch.distributed as dist
    from conftest import load_case
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()

    data, meta, vars_use, kw, g = load_case(case)
    N = data.shape[0]
    cuts = np.linspace(0, N, world + 1).astype(int)
    if world > 1:
        cuts[1] = max(1, cuts[1] - N // 7)
    lo, hi = cuts[rank], cuts[rank + 1]
    Z_loc, meta_loc = data[lo:hi].astype(np.float32), meta.iloc[lo:hi].reset_index(drop=True)
    rounds = [int(r) for r in g["kmeans_rounds"]]

    from harmonypy_amd import Shard
    from harmonypy_amd import harmony as H
    os.environ["HMX_UPDATE_ORDER"] = "torch"
    shard = Shard(transport="host")
    if source == "device":
        x = torch.from_numpy(np.ascontiguousarray(Z_loc.T)).to("cuda").T      # N x d view of a d x N tensor
    else:
        x = Z_loc
    # the upload state first (no iteration), then the whole run
    h0 = H.run_harmony(x, meta_loc, vars_use, verbose=False, shard=shard, _y0=g["Y0"], **dict(kw, max_iter_harmony=0))
    Z_orig, Z_cos = h0.Z_orig, h0.Z_cos
    del h0
    ho = H.run_harmony(x, meta_loc, vars_use, verbose=False, shard=shard, _y0=g["Y0"], _schedule=rounds, **kw)
    if source == "device":
        assert "upload_device" in ho.timing and "upload" not in ho.timing
        Z_corr = ho.to_tensor("Z_corr").cpu().numpy()
    else:
        Z_corr = ho.Z_corr
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), lo=lo, hi=hi, Z_corr=Z_corr, Z_orig=Z_orig, Z_cos=Z_cos)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
