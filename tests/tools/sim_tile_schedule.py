#!/usr/bin/env python3
"""Static stride against a tile queue for the skipping render kernel, simulated on the CPU (no GPU needed).

    python tests/tools/sim_tile_schedule.py [--view 0] [--chunks 4] [--chunk 65536] [--cus 256] [--json]

`mlp_kernel3<..., SKIP>` runs a tile (8 adjacent rays x 16 consecutive samples) without density in about 0.83 of the time of a
full one, and in ray-tile order tile `it` is depth slot `it % slots` of ray block `it // slots`.  This tool takes the benchmark
scene (seeded weights, orbit view), sends ONE proxy ray per 8-ray block through the oracle (coarse pass, composite, inverse-CDF
resampling, fine pass), calls a tile empty when the proxy ray's 16 samples of that depth slot all have sigma <= 0, and schedules
the tiles of every chunk's coarse and fine launch twice:

  static   grid = 4 x CUs workgroups, workgroup b runs tiles b, b + grid, ...; the workgroups are dispatched in order, each to
           the CU slot that frees first (one resident workgroup per CU for the 8x256 network)
  queue    grid = CUs workgroups, each takes the next unclaimed tile whenever it finishes one

and prints the makespan of both over the perfectly balanced time (sum of tile times / CUs).  One proxy ray per block
overstates emptiness a little (a block is empty only if all 8 rays are), which the measured skipped-tile share corrects for
when the two are compared; the tile times are parameters (--t-full / --t-empty, microseconds)."""
import argparse
import heapq
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from nerfmeshes_amd import synthetic as S  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402

MLP_KW = dict(num_layers=8, hidden_size=256, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
SIDE, NEAR, FAR, NUM_COARSE, NUM_FINE = 800, 2.0, 6.0, 64, 128


def tile_empty(sigma):
    """(blocks, samples) sigma of the proxy rays -> (blocks * samples / 16,) bool in the kernel's tile order."""
    blocks, samples = sigma.shape
    dense = ~(sigma <= 0.0)
    return ~dense.reshape(blocks, samples // 16, 16).any(-1).reshape(-1)


def persistent_grid(wg_iters, resident):
    grid = min(wg_iters, resident * 4)
    if wg_iters > grid:
        rounds = -(-wg_iters // grid)
        grid = -(-wg_iters // rounds)
    return grid


def makespan_static(cost, cus):
    """In-order greedy dispatch of the strided workgroups onto `cus` slots.  Returns (makespan, shortest and longest workgroup)."""
    grid = persistent_grid(len(cost), cus)
    wg = np.array([cost[b::grid].sum() for b in range(grid)])
    free = [0.0] * cus
    heapq.heapify(free)
    end = 0.0
    for t in wg:
        done = heapq.heappop(free) + t
        end = max(end, done)
        heapq.heappush(free, done)
    return end, float(wg.min()), float(wg.max())


def makespan_queue(cost, cus):
    """`cus` workgroups, each claiming the next tile in order whenever it is free."""
    free = [0.0] * min(cus, len(cost))
    heapq.heapify(free)
    end = 0.0
    for t in cost:
        done = heapq.heappop(free) + t
        end = max(end, done)
        heapq.heappush(free, done)
    return end


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--view", type=int, default=0)
    ap.add_argument("--chunks", type=int, default=4, help="how many chunks of the view, spread evenly over it")
    ap.add_argument("--chunk", type=int, default=65536, help="rays per render call (bench.py --chunk)")
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--t-full", type=float, default=263.0, help="microseconds of a tile that runs the colour branch")
    ap.add_argument("--t-empty", type=float, default=218.0, help="microseconds of a tile that skips it")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()

    w = S.make_scene_weights(**MLP_KW)
    spec, rs = O.MLPSpec(**MLP_KW), O.RenderSpec(num_coarse=NUM_COARSE, num_fine=NUM_FINE)
    origin, dirs = O.get_ray_bundle(SIDE, SIDE, S.LEGO_FOCAL_800, S.orbit_poses(args.view + 1)[args.view])
    origin, dirs = torch.as_tensor(origin).reshape(1, 3), torch.as_tensor(dirs).reshape(-1, 3)
    n_chunks = -(-dirs.shape[0] // args.chunk)
    picks = sorted({int(round(i * (n_chunks - 1) / max(args.chunks - 1, 1))) for i in range(min(args.chunks, n_chunks))})
    out = {"view": args.view, "cus": args.cus, "t_full_us": args.t_full, "t_empty_us": args.t_empty, "chunks": []}
    busy = {"static": 0.0, "queue": 0.0, "ideal": 0.0}
    for c in picks:
        d = dirs[c * args.chunk:(c + 1) * args.chunk][::8].contiguous()          # the first ray of every 8-ray block
        with torch.no_grad():
            coarse, fine = O.render(w, w, spec, spec, rs, origin, d, NEAR, FAR)
        rec = {"chunk": c, "ray_blocks": int(d.shape[0])}
        for name, b in (("coarse", coarse), ("fine", fine)):
            empty = tile_empty(b["radiance"][..., 3].numpy())
            cost = np.where(empty, args.t_empty, args.t_full)
            ideal = cost.sum() / args.cus
            static, wg_lo, wg_hi = makespan_static(cost, args.cus)
            queue = makespan_queue(cost, args.cus)
            slots = b["radiance"].shape[1] // 16
            rec[name] = {"tiles": int(cost.size), "empty_share": float(empty.mean()),
                         "empty_share_per_depth_slot": [float(x) for x in empty.reshape(-1, slots).mean(0)],
                         "ideal_ms": ideal / 1e3, "static_ms": static / 1e3, "queue_ms": queue / 1e3,
                         "static_over_ideal": static / ideal - 1.0, "queue_over_ideal": queue / ideal - 1.0,
                         "static_workgroup_ms": [wg_lo / 1e3, wg_hi / 1e3]}
            busy["static"] += static
            busy["queue"] += queue
            busy["ideal"] += ideal
        out["chunks"].append(rec)
    out["tail_idle_share_static"] = 1.0 - busy["ideal"] / busy["static"]
    out["tail_idle_share_queue"] = 1.0 - busy["ideal"] / busy["queue"]
    out["predicted_gain_of_queue"] = busy["static"] / busy["queue"] - 1.0
    if args.json:
        print(json.dumps(out))
        return
    for rec in out["chunks"]:
        for name in ("coarse", "fine"):
            r = rec[name]
            print(f"chunk {rec['chunk']:2d} {name:6s} {r['tiles']:6d} tiles, {100 * r['empty_share']:5.1f} % empty | ideal {r['ideal_ms']:7.2f} ms | "
                  f"static +{100 * r['static_over_ideal']:.2f} % (workgroups {r['static_workgroup_ms'][0]:.2f} .. {r['static_workgroup_ms'][1]:.2f} ms) | "
                  f"queue +{100 * r['queue_over_ideal']:.2f} %")
    print(f"tail idle: static {100 * out['tail_idle_share_static']:.2f} %, queue {100 * out['tail_idle_share_queue']:.2f} % of the kernel time; "
          f"predicted gain of the queue {100 * out['predicted_gain_of_queue']:.2f} %")


if __name__ == "__main__":
    main()
