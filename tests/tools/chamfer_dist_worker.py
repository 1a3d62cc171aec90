"""Launched by tests/test_gpu_mesh_metrics.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `hip_ops.chamfer_distance` of two clouds of 10 001 and
7 777 points -- ragged slices of the queries on every rank, one all-gather per direction -- must return the single-rank
floats and `dist2_*` arrays byte for byte on EVERY rank.  Prints CHAMFER_DIST_OK on rank 0."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from nerfmeshes_amd import dist as nd  # noqa: E402
from tests import gpu_support as gs  # noqa: E402


def main():
    rank, world, dev = nd.init_from_env()
    from nerfmeshes_amd import hip_ops
    rng = np.random.default_rng(2024)                                # the same clouds on every rank
    x = torch.from_numpy(rng.standard_normal((10_001, 3)).astype(np.float32)).to(dev)
    y = torch.from_numpy((rng.standard_normal((7_777, 3)) * 1.5 + 0.25).astype(np.float32)).to(dev)
    x[17] = float("nan")                                             # a row without a winner travels as +inf
    got = hip_ops.chamfer_distance(x, y)
    want = gs.single_rank(lambda: hip_ops.chamfer_distance(x, y))
    for k in ("chamfer", "x_to_y", "y_to_x"):
        assert isinstance(got[k], float) and np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (rank, k, got[k], want[k])
    for k, n in (("dist2_x", 10_001), ("dist2_y", 7_777)):
        a, b = got[k].cpu().numpy(), want[k].cpu().numpy()
        assert a.shape == (n,) and a.dtype == np.float32 and a.tobytes() == b.tobytes(), f"rank {rank}: {k} differs from one rank's"
    assert got["x_to_y"] == float("inf") and np.isfinite(got["y_to_x"])
    torch.cuda.synchronize()
    # every rank passed: only then does rank 0 report
    flag = torch.ones(1, device=dev)
    nd.all_reduce(flag)
    if rank == 0:
        assert int(flag.item()) == world
        print(f"CHAMFER_DIST_OK world={world} y_to_x={got['y_to_x']}", flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
