"""Launched by tests/test_gpu_mc.py under `python -m torch.distributed.run --nproc-per-node N` with
`NERFMESHES_RANKS_PER_GPU=N` (N ranks sharing one GPU over gloo): `dist.marching_cubes_sharded` of a 3 x 4 x 4 grid whose value
is its axis-0 index, at a level outside the range, at the maximum (in range, nothing cut) and at 0.5.  Every rank must see what
`hip_ops.marching_cubes` of the whole grid gives at that level: its two errors with their texts, then -- the ranks still in
step after two raised errors -- its mesh bit for bit.  At 3 ranks the two cube layers leave one rank without a slab.
Prints MC_ERRORS_DIST_OK on rank 0."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from nerfmeshes_amd import dist as nd, hip_ops  # noqa: E402

OUTSIDE = (ValueError, "Surface level must be within volume data range.")
NOTHING_CUT = (RuntimeError, "No surface found at the given iso value.")


def outcome(fn):
    """the mesh `fn` returns, or the type and the text of what it raises"""
    try:
        return fn()[:4]
    except (ValueError, RuntimeError) as e:
        return type(e), str(e)


def main():
    rank, world, dev = nd.init_from_env()
    n0, n1, n2 = 3, 4, 4
    full = torch.arange(n0, dtype=torch.float32, device=dev)[:, None, None].expand(n0, n1, n2).contiguous()
    query = lambda p_lo, p_hi: full[p_lo:p_hi].reshape(-1)   # noqa: E731
    for level, want in ((5.0, OUTSIDE), (2.0, NOTHING_CUT), (0.5, None)):
        whole = outcome(lambda: hip_ops.marching_cubes(full, level))
        sharded = outcome(lambda: nd.marching_cubes_sharded(query, n0, n1, n2, lambda *slab: level))
        if want is not None:
            assert len(whole) == 2 and whole == want, f"level {level}: the whole grid gives {whole}"
            assert len(sharded) == 2 and sharded == want, f"level {level}, rank {rank}: the slabs give {sharded}"
            continue
        assert len(whole) == 4 and len(sharded) == 4 and whole[0].shape[0] > 0, f"level {level}: no mesh: {whole} / {sharded}"
        for name, a, b in zip(("vertices", "faces", "normals", "values"), sharded, whole):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), f"level {level}, rank {rank}: {name} differ"
    torch.cuda.synchronize()
    if rank == 0:
        print(f"MC_ERRORS_DIST_OK world={world} vertices={int(whole[0].shape[0])}", flush=True)
    nd.shutdown()


if __name__ == "__main__":
    main()
