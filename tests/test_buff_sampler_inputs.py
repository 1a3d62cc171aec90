"""What tests/test_gpu_buff_sampler.py rests on, checked without a GPU (tests/buff_cases.py).

Each generator is named for a path of the sampler's kernels: more rays than a launch holds, refined voxel sets on which the two tie
orders differ, unsorted depths that are not rising (sort 3), entry depths on which introsort falls back to heap sort, more crossed boxes
than a 64-lane chunk, the edges of the sizes, directions with zeros.  Whether an input reaches its path depends on seeds and constants
only, so it is asserted here: a change of either cannot make the GPU tests vacuous unnoticed."""
import numpy as np
import pytest
import torch

from oracle import introsort as IS
from tests import buff_cases as B


def test_long_batch_outnumbers_the_launches_and_mixes_crossing_counts():
    c = B.long_batch()
    rays = c.dirs.shape[0]
    assert rays == 20001 and rays > B.STABLE_RAYS_IN_FLIGHT and rays % 4 == 1 and c.voxels.shape[0] == 343 and c.samples == 33
    counts = B.crossing_counts(c)
    hit, miss = int((counts > 0).sum()), int((counts == 0).sum())
    print("long batch: hit", hit, "miss", miss, "crossing counts", sorted(set(counts.tolist())))       # 13774, 6227, 0 .. 13
    assert 2 * hit >= rays and 10 * miss >= rays
    assert set(range(1, 11)) <= set(counts.tolist())
    # a wave's next ray (one launch's worth of rays further on: 16384, or 32 per CU of a 256-CU part) mostly has another crossing
    # count: leftover LDS state of another length is the rule
    for stride in (B.STABLE_RAYS_IN_FLIGHT, B.REFERENCE_RAYS_PER_CU * 256):
        assert float((counts[stride:] != counts[:-stride]).float().mean()) > 0.5
    for mode in B.MODES:
        z, idx, mask = B.expected(c, mode)
        assert z.shape == idx.shape == (rays, 33) and np.array_equal(mask, (counts > 0).numpy())


@pytest.mark.parametrize("which", B.REFINED_SETS)
def test_refined_sets_tell_the_tie_orders_apart(which):
    c = B.refined(which)
    n = c.voxels.shape[0]
    edges = sorted(set(np.round((c.voxels[:, 1] - c.voxels[:, 0]).reshape(-1).double().numpy(), 5).tolist()))
    assert (n, edges) == {"sampled_tree": (1531, [0.05, 0.1]), "tree_after1": (1120, [0.05]), "three_level": (578, [0.05, 0.1, 0.2])}[which]
    assert c.dirs.shape[0] == 1500 and c.samples == 192
    if which == "sampled_tree":
        assert n % 64 == 59
    zs, ids, ms = B.expected(c, "stable")
    zr, idr, mr = B.expected(c, "reference")
    hit = ms
    differ = int((ids[hit] != idr[hit]).any(1).sum())
    print(which, "hit", int(hit.sum()), "of 1500; ids of the two orders differ on", differ)      # 1485 / 1372, 1034 / 645, 1377 / 1160
    assert np.array_equal(ms, mr) and hit.sum() >= 0.6 * 1500
    assert differ >= 0.4 * hit.sum()
    assert np.array_equal(zs[hit], zr[hit])
    assert np.array_equal(B.expected(c, "random")[2], ms)


def test_three_level_set_is_built_as_described():
    root = B.grid(6)
    assert int((root.mean(1).norm(dim=-1) < 0.55).sum()) == 88
    vox = B.three_level_voxels()
    size = np.round((vox[:, 1, 0] - vox[:, 0, 0]).double().numpy(), 5)
    assert [int((size == e).sum()) for e in (0.2, 0.1, 0.05)] == [48, 290, 240] and vox.shape[0] == 578
    assert bool((vox[:, 1] > vox[:, 0]).all())
    volume = float((vox[:, 1] - vox[:, 0]).prod(-1).double().sum())
    assert abs(volume - 88 * 0.2 ** 3) < 1e-6, "the boxes tile the 88 kept cells"
    # children follow the tree's formula: the first child starts at its parent's corner, the last ends at the opposite one
    kids = B.subdivide(root[5])
    assert len(kids) == 8 and torch.equal(kids[0][0], root[5][0]) and torch.equal(kids[7][1], root[5][1])
    assert torch.equal(torch.stack(kids), torch.stack(B.subdivide(root[5], 2))) and torch.equal(B.grid(2), torch.stack(B.subdivide(B.grid(1)[0])))


@pytest.mark.parametrize("samples", [192, 512])
def test_overlapping_boxes_reach_sort_3(samples):
    c = B.overlapping(samples)
    assert c.voxels.shape[0] == 64 + 125 + 22 == 211 and c.dirs.shape[0] == 1000
    for ties in ("stable", "reference"):
        z, mask = B.unsorted_depths(c, ties)
        ze, _, me = B.expected(c, ties)
        assert not bool(torch.isnan(z).any()) and np.array_equal(mask.numpy(), me)
        hit = int(mask.sum())
        real = int(B.not_rising(z)[mask].sum())
        print("overlapping", samples, ties, "hit", hit, "rows that need the real sort", real)                      # 1000, 1000
        assert hit >= 900 and real >= 0.95 * hit
        assert np.array_equal(torch.sort(z, dim=-1, stable=True).values.numpy()[me], ze[me])
    ids_s, ids_r = B.expected(c, "stable")[1], B.expected(c, "reference")[1]
    assert not np.array_equal(ids_s, ids_r)
    if samples == 512:
        # long runs of rising depths with a few stragglers: on some rays sort 3 itself runs out of depth and heap-sorts
        falls = []
        for row in B.unsorted_depths(c, "reference")[0].tolist():
            stats = {}
            IS.introsort(row, IS.comp_asc, stats)
            falls.append(stats["heap_fallbacks"])
        print("overlapping 512: rays whose sort 3 reaches the heap fallback:", sum(f > 0 for f in falls))           # 14 of 1000
        assert any(falls)


def test_root_grid_alone_never_reaches_sort_3():
    c = B.grid12_for_sort3()
    for ties in ("stable", "reference"):
        z, mask = B.unsorted_depths(c, ties)
        assert int(mask.sum()) == 1000 and int(B.not_rising(z)[mask].sum()) == 0
        assert np.array_equal(z.numpy(), B.expected(c, ties)[0])


@pytest.mark.parametrize("n", B.KILLER_SLABS + (400,))
def test_killer_slabs_reach_the_heap_fallback(n):
    c = B.killer_slabs(n)
    rank = B.killer_ranks(n)
    assert sorted(rank) == list(range(n)) and c.dirs.shape[0] == 24 and c.far == 1.6 and c.samples == 192
    tmin, tmax, crossed = B.slab_test(c)
    assert not bool(torch.isnan(tmin).any()) and not bool(torch.isnan(tmax).any())
    assert bool(crossed.all()), "every ray crosses all n slabs"
    # the entry depths are ordered like the adversary's keys
    assert bool((torch.argsort(tmin, dim=-1, stable=True) == torch.argsort(torch.tensor(rank))[None]).all())
    falls = B.heap_fallbacks(c)
    print("killer slabs", n, "heap fallbacks per ray", falls)                                                      # 1 on every ray
    assert len(falls) == 24 and min(falls) >= 1
    stats = {}
    IS.introsort(list(range(n)), IS.comp_asc, stats)
    assert stats["heap_fallbacks"] == 0, "slabs in x order never reach it"
    if n == 500:
        assert B.REFERENCE_FAST_HITS < n <= B.MAX_HITS      # the second pass, with room for 512


def test_ordered_slabs_cross_more_than_a_chunk_and_more_than_the_cap():
    c = B.ordered_slabs(200)
    counts = B.crossing_counts(c)
    assert c.dirs.shape[0] == 48 and int(counts.min()) > 64 and int(counts.max()) == 200 and len(set(counts.tolist())) >= 4
    assert int(B.crossing_counts(B.ordered_slabs(600)).max()) > B.MAX_HITS
    # the same input as test_buff_reference_order_many_crossed_boxes
    g = torch.Generator().manual_seed(200)
    o = torch.tensor([-0.75, 0.0, 0.0]).repeat(48, 1) + 0.05 * torch.randn(48, 3, generator=g)
    assert torch.equal(o, c.origins)
    xs = torch.linspace(-0.6, 0.6, 201)
    assert torch.equal(c.voxels[:, 0, 0], xs[:-1]) and torch.equal(c.voxels[:, 1, 0], xs[1:])


def test_size_edges():
    assert B.SAMPLE_COUNTS == (1, 2, 63, 64, 65, 511, 512) and B.VOXEL_COUNTS == (1, 2, 16, 17, 63, 64, 65, 128, 129)
    for s in B.SAMPLE_COUNTS:
        c = B.sample_counts(s)
        assert c.voxels.shape[0] == 1728 and c.dirs.shape[0] == 200 and c.samples == s
    assert int((B.crossing_counts(B.sample_counts(1)) > 0).sum()) == 200
    for n in B.VOXEL_COUNTS:
        c = B.voxel_counts(n)
        hits = int((B.crossing_counts(c) > 0).sum())
        print("voxel count", n, "hit", hits, "of 200")                                                             # 13 .. 129
        assert c.voxels.shape[0] == n and c.samples == 48 and 0 < hits < 200
        if n > 2:
            assert len({tuple(v.reshape(-1).tolist()) for v in c.voxels}) == n
    for extra in (0, 1):
        c = B.limit_grid(extra)
        counts = B.crossing_counts(c)
        assert c.voxels.shape[0] == B.REFERENCE_MAX_VOXELS + extra and c.dirs.shape[0] == 64
        assert int(counts.min()) > 0 and int(counts.max()) <= B.REFERENCE_FAST_HITS                              # 7 .. 38
    assert len({tuple(v.reshape(-1).tolist()) for v in B.limit_grid(0).voxels}) == 8192


def test_axis_parallel_rays():
    c = B.axis_parallel()
    assert (1.0 / c.dirs[7, 0]).item() == float("-inf") and (1.0 / c.dirs[0, 0]).item() == float("inf")
    assert int((c.dirs == 0).sum()) == 18 and int(torch.signbit(c.dirs[c.dirs == 0]).sum()) == 3
    tmin, tmax, crossed = B.slab_test(c)
    assert bool(torch.isinf(tmin).any()) and not bool(torch.isnan(tmin).any()) and not bool(torch.isnan(tmax).any())
    counts = crossed.sum(-1).tolist()
    assert set(counts) <= {3, 4} and counts[:7] == [3, 3, 3, 4, 3, 3, 3]
    for mode in B.MODES:
        z, _, mask = B.expected(c, mode)
        assert mask.all() and np.isfinite(z).all()


def test_draws_stay_clear_of_the_documented_deviation():
    for c in (B.sample_counts(1), B.sample_counts(2), B.long_batch()):
        u_pick, u_pos = B.draws(c)
        assert u_pick.dtype == torch.float64 and u_pos.dtype == torch.float32 and u_pick.shape == u_pos.shape == (c.dirs.shape[0], c.samples)
        assert float(u_pick.min()) >= B.MIN_PICK and float(u_pick.max()) < 1.0 and float(u_pos.max()) < 1.0
    assert B.draws(B.long_batch())[0][7, :4].tolist() == [1e-7, 1.0 - 2.0 ** -53, 0.5, 1.0 / 3.0]


def test_integration_input_is_exact_and_covers_the_skips():
    memm, idx, w, mw = B.integrate_inputs()
    n = B.INTEGRATE_VOXELS
    assert idx.numel() == 200000 and n == 1531
    for x in (w, mw):
        assert torch.equal(x * 4096, (x * 4096).round()) and float(x.min()) >= 0 and float(x.max()) < 1
    assert int((idx == B.INTEGRATE_PILE).sum()) > 40000 and int((idx == -1).sum()) > 1000 and int((idx == n).sum()) > 1000
    assert len(set(idx[(idx >= 0) & (idx < n)].tolist())) == n, "every voxel receives samples"
    dead = torch.arange(n) % 13 == 5
    ok = (idx >= 0) & (idx < n)
    assert bool((w[ok & (idx % 13 == 5)] > 0).all()) and not bool(mw[ok & (idx % 13 == 5)].any())
    # the sums are exact in fp64: any order gives the same bits
    flat = idx[ok]
    perm = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(1))
    a = np.bincount(flat.numpy(), weights=w[ok].double().numpy(), minlength=n)
    b = np.bincount(flat[perm].numpy(), weights=w[ok][perm].double().numpy(), minlength=n)
    assert np.array_equal(a, b) and np.array_equal(a * 4096, np.round(a * 4096))
    for counter in (1, 7):
        e = B.integrate_expected(memm, counter, idx, w, mw)
        assert np.array_equal(e[dead.numpy()], memm.numpy()[dead.numpy()]) and (e[~dead.numpy()] != memm.numpy()[~dead.numpy()]).all()
        z = torch.zeros(())
        ref = B.O.buff_integrate(memm, counter, torch.where(ok, idx, 0), torch.where(ok, w, z), torch.where(ok, mw, z))
        assert np.array_equal(ref.numpy(), e), "the restatement is the oracle's integration"
