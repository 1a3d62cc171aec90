"""Inputs, CPU references and predicates of the BuFF voxel sampler's bit-exact tests (nerfmeshes_amd/csrc/buff_tree.hip), shared by
tests/test_buff_sampler_inputs.py (no GPU) and tests/test_gpu_buff_sampler.py.  Nothing here touches the GPU.

The three per-ray kernels -- buff_intersect_kernel (ids="stable"), buff_random_kernel and buff_reference_ids_kernel (ids="reference")
-- promise the oracle's depths and voxel ids bit for bit.  Every generator below is named for the kernel path it reaches:

    long_batch        more rays than either launch holds at once: the second iteration of the per-ray loops, LDS state left over
                      from a ray with another crossing count
    refined           voxel sets of mixed sizes whose count is no multiple of 64, where the two tie orders really differ
    overlapping       boxes that overlap: the unsorted sample depths are not rising, so sort 3 of the reference order is a real sort
    killer_slabs      slabs listed in an order on which introsort's partitioning degenerates: the heap-sort fallback of sort 1
    ordered_slabs     more than 64 (and more than 512) crossed boxes
    sample_counts, voxel_counts, limit_grid     the edges of the sizes
    axis_parallel     directions with components of exactly +-0

The reference is oracle.nerf_oracle on the CPU (dense (R, N, 3) tensors: evaluated in chunks of ORACLE_CHUNK rays, once per case and
mode).  All comparisons are np.array_equal; there is no tolerance in this file."""
import collections
import functools

import numpy as np
import torch

from oracle import introsort as IS
from oracle import nerf_oracle as O

NEAR, FAR = 0.0, 1.2
SLAB_FAR = 1.6
ORACLE_CHUNK = 2048
MIN_PICK = 1e-7          # below 1.7e-9 the random kernel deviates from the reference on purpose (buff_tree.hip, buff_random_kernel)
MODES = ("stable", "reference", "random")

# what the host code launches at most (nm_buff_intersect_ex / nm_buff_intersect_random in buff_tree.hip):
STABLE_RAYS_IN_FLIGHT = 4096 * 4                 # stable and random kernels: at most 4096 blocks of four one-ray waves
REFERENCE_RAYS_PER_CU = 32                       # reference order: at most CUs * min(32, LDS / per-ray bytes) one-wave blocks
MAX_HITS = 512                                   # BUFF_MAX_HITS / REF_MAX_HITS
REFERENCE_FAST_HITS = 128                        # REF_FAST_HITS: a ray that crosses more repeats the call with room for 512
MAX_SAMPLES = 512
REFERENCE_MAX_VOXELS = 8192

SAMPLE_COUNTS = (1, 2, 63, 64, 65, 511, 512)     # spad boundaries; 512: depth 18 in sort 3
VOXEL_COUNTS = (1, 2, 16, 17, 63, 64, 65, 128, 129)   # 16 / 17: the introsort threshold; 63 / 64 / 65, 128 / 129: npad
KILLER_SLABS = (300, 500)
REFINED_SETS = ("sampled_tree", "tree_after1", "three_level")

Case = collections.namedtuple("Case", "name voxels origins dirs near far samples seed")


def shell_rays(count, seed, spread=1.0):
    """The rays of test_buff_intersect_vs_oracle: origins on a shell of radius 0.7 .. 1.3, looking at a random point of
    (rand - 0.5) * spread."""
    g = torch.Generator().manual_seed(seed)
    o = torch.nn.functional.normalize(torch.randn(count, 3, generator=g), dim=-1) * (0.7 + 0.6 * torch.rand(count, 1, generator=g))
    d = torch.nn.functional.normalize((torch.rand(count, 3, generator=g) - 0.5) * spread - o, dim=-1)
    return o, d


def slab_rays(count, seed, scale=None):
    """The rays of test_buff_reference_order_many_crossed_boxes: from in front of the slabs' -x face along +x, ray r oblique in
    proportion to scale[r] (that test: linspace(0, 1, count))."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.linspace(0, 1, count) if scale is None else scale
    o = torch.tensor([-0.75, 0.0, 0.0]).repeat(count, 1) + 0.05 * torch.randn(count, 3, generator=g)
    d = torch.nn.functional.normalize(torch.tensor([1.0, 0.0, 0.0]) + 0.3 * torch.randn(count, 3, generator=g) * scale[:, None], dim=-1)
    return o, d


def draws(case):
    """(u_pick (R, S) float64 >= MIN_PICK, u_pos (R, S) float32) of a case; the first columns hold the edges of the CDF."""
    g = torch.Generator().manual_seed(1000 + case.seed)
    rays = case.dirs.shape[0]
    u_pick = torch.rand(rays, case.samples, dtype=torch.float64, generator=g).clamp_(min=MIN_PICK)
    edges = torch.tensor([MIN_PICK, 1.0 - 2.0 ** -53, 0.5, 1.0 / 3.0], dtype=torch.float64)[:case.samples]
    u_pick[:, :edges.numel()] = edges
    return u_pick, torch.rand(rays, case.samples, generator=g)


def _chunks(case):
    rays = case.dirs.shape[0]
    for a in range(0, rays, ORACLE_CHUNK):
        yield slice(a, min(rays, a + ORACLE_CHUNK))


_expected = {}


def expected(case, mode):
    """(z, idx, mask) of the oracle as numpy arrays, computed once per case and mode and never written to."""
    key = (case.name, mode)
    if key not in _expected:
        parts = []
        u_pick, u_pos = draws(case) if mode == "random" else (None, None)
        for rows in _chunks(case):
            if mode == "random":
                parts.append(O.buff_intersect_random(case.voxels, case.origins[rows], case.dirs[rows], case.near, case.far, u_pick[rows], u_pos[rows]))
            else:
                parts.append(O.buff_intersect(case.voxels, case.origins[rows], case.dirs[rows], case.near, case.far, case.samples, ties=mode))
        out = tuple(torch.cat([p[k] for p in parts]).numpy() for k in range(3))
        for a in out:
            a.setflags(write=False)
        _expected[key] = out
    return _expected[key]


def slab_test(case):
    """(tmin, tmax, crossed) of every ray and box, each (R, N)."""
    parts = [O._buff_slab_test(case.voxels, case.origins[rows], case.dirs[rows], case.near, case.far) for rows in _chunks(case)]
    return tuple(torch.cat([p[k] for p in parts]) for k in range(3))


def crossing_counts(case):
    return slab_test(case)[2].sum(-1)


def unsorted_depths(case, ties="stable"):
    """The sample depths as the sampler places them, BEFORE its last sort (oracle.nerf_oracle.buff_intersect up to `z`, restated
    over the shared slab test) -> (z (R, S), ray_mask (R,)).  Sort 3 of the reference order is the identity, and the kernel skips
    it, exactly where a row of these is strictly rising."""
    stable = {"stable": True, "reference": False}[ties]
    zs, masks = [], []
    for rows in _chunks(case):
        tmin, tmax, mask = O._buff_slab_test(case.voxels, case.origins[rows], case.dirs[rows], case.near, case.far)
        R, N = tmin.shape
        order = torch.sort(tmin, dim=-1, stable=stable)
        inter = torch.stack((tmin, tmax), -1).gather(-2, order.indices[..., None].expand(R, N, 2))
        mask_sorted = mask.gather(-1, order.indices)
        start = torch.sort(mask_sorted.long(), dim=-1, descending=True, stable=stable)
        res = torch.zeros_like(inter)
        res[start.values.bool()] = inter[mask_sorted]
        cums = torch.cumsum(res[..., 1] - res[..., 0], -1)
        samples = torch.linspace(0, 1.0, case.samples) * cums[..., -1][..., None]
        bucket = torch.searchsorted(cums, samples)
        first = torch.searchsorted(bucket, bucket, right=False)
        zs.append(res[..., 0].gather(-1, bucket) + (samples - samples.gather(-1, first)))
        masks.append(mask.sum(-1) > 0)
    return torch.cat(zs), torch.cat(masks)


def not_rising(z):
    """Rows with a tie, an inversion or a NaN between neighbours: the rows on which the kernel runs the real sort 3."""
    return ~(z[:, 1:] > z[:, :-1]).all(-1)


def heap_fallbacks(case):
    """Per ray: how often libstdc++'s introsort over the ray's entry depths (sort 1) reaches its heap-sort fallback."""
    tmin = slab_test(case)[0]
    out = []
    for row in tmin.tolist():
        stats = {}
        IS.introsort(row, IS.comp_asc, stats)
        out.append(stats["heap_fallbacks"])
    return out


# ---------------------------------------------------------------------------------------------------------------- voxel sets

def subdivide(box, count=2):
    """Children of a (2, 3) box as the tree makes them: lo + (i, g, h) / count * extent, x-major / z-fastest."""
    lo, extent = box[0], box[1] - box[0]
    out = []
    for i in range(count):
        for g in range(count):
            for h in range(count):
                a = torch.tensor([i, g, h], dtype=torch.float) / count * extent
                b = torch.tensor([i + 1, g + 1, h + 1], dtype=torch.float) / count * extent
                out.append(torch.stack((lo + a, lo + b), 0))
    return out


@functools.lru_cache(maxsize=None)
def grid(side):
    return O.buff_initial_voxels(NEAR, FAR, side)


@functools.lru_cache(maxsize=None)
def three_level_voxels(seed=5):
    """6^3 root cells with the centre within 0.55 of the origin (88), 40 of them split 2x2x2, every third child of 10 of those split
    again, shuffled: 578 boxes with edges 0.2, 0.1 and 0.05."""
    root = grid(6)
    kept = root[root.mean(1).norm(dim=-1) < 0.55]
    g = torch.Generator().manual_seed(seed)
    chosen = torch.randperm(kept.shape[0], generator=g).tolist()
    split, deep = set(chosen[:40]), set(chosen[:10])
    out = []
    for i, box in enumerate(kept):
        if i not in split:
            out.append(box)
            continue
        for c, kid in enumerate(subdivide(box)):
            if i in deep and c % 3 == 0:
                out.extend(subdivide(kid))
            else:
                out.append(kid)
    vox = torch.stack(out, 0)
    return vox[torch.randperm(vox.shape[0], generator=g)]


def _golden(name, key):
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")) as g:
        return torch.from_numpy(g[key].astype(np.float32))


@functools.lru_cache(maxsize=None)
def refined_voxels(which):
    if which == "sampled_tree":
        return _golden("buff_sampled_tree", "voxels_after")
    if which == "tree_after1":
        return _golden("buff_tree", "voxels_after1")
    assert which == "three_level", which
    return three_level_voxels()


@functools.lru_cache(maxsize=None)
def overlapping_voxels(seed=9):
    """The 4^3 grid, the 5^3 grid and every third box of the 4^3 grid once more (duplicates), shuffled: 211 boxes.  Where boxes
    overlap, the crossed length exceeds the span of depths, so samples of one box reach behind the entry of the next."""
    vox = torch.cat((grid(4), grid(5), grid(4)[::3]), 0)
    return vox[torch.randperm(vox.shape[0], generator=torch.Generator().manual_seed(seed))]


def slab_voxels(n, rank=None):
    """n slabs tiling [-0.6, 0.6]^3 along x; box i of the list is the rank[i]-th slab counted from -x (default: in order)."""
    xs = torch.linspace(-0.6, 0.6, n + 1)
    rank = torch.arange(n) if rank is None else torch.as_tensor(rank, dtype=torch.long)
    lo = torch.stack([xs[:-1][rank], torch.full((n,), -0.6), torch.full((n,), -0.6)], -1)
    hi = torch.stack([xs[1:][rank], torch.full((n,), 0.6), torch.full((n,), 0.6)], -1)
    return torch.stack([lo, hi], 1)


@functools.lru_cache(maxsize=None)
def killer_ranks(n):
    """x-rank of every slab such that the entry depths of a ray along +x are ordered like oracle.introsort.quicksort_killer(n)
    (items the adversary leaves undecided share one value: they keep their list order)."""
    vals = torch.tensor(IS.quicksort_killer(n), dtype=torch.float64)
    rank = torch.empty(n, dtype=torch.long)
    rank[torch.sort(vals, stable=True).indices] = torch.arange(n)
    return tuple(rank.tolist())


def box_grid(nx, ny, nz):
    """nx * ny * nz boxes tiling [-0.6, 0.6]^3, x-major / z-fastest."""
    ex, ey, ez = (torch.linspace(-0.6, 0.6, n + 1) for n in (nx, ny, nz))
    i, g, h = torch.meshgrid(torch.arange(nx), torch.arange(ny), torch.arange(nz), indexing="ij")
    lo = torch.stack([ex[i], ey[g], ez[h]], -1).reshape(-1, 3)
    hi = torch.stack([ex[i + 1], ey[g + 1], ez[h + 1]], -1).reshape(-1, 3)
    return torch.stack([lo, hi], 1)


# --------------------------------------------------------------------------------------------------------------------- cases

@functools.lru_cache(maxsize=None)
def long_batch():
    o, d = shell_rays(20001, 20001, spread=2.2)
    return Case("long_batch", grid(7), o, d, NEAR, FAR, 33, 1)


def rows_of(case, rows):
    """The rays `rows` of a case as a case of their own (the draws are the caller's to slice)."""
    return case._replace(name=f"{case.name}[{rows.start}:{rows.stop}]", origins=case.origins[rows], dirs=case.dirs[rows])


@functools.lru_cache(maxsize=None)
def refined(which):
    o, d = shell_rays(1500, 1500 + REFINED_SETS.index(which))
    return Case(f"refined-{which}", refined_voxels(which), o, d, NEAR, FAR, 192, 2 + REFINED_SETS.index(which))


@functools.lru_cache(maxsize=None)
def overlapping(samples):
    o, d = shell_rays(1000, 1000)
    return Case(f"overlapping-s{samples}", overlapping_voxels(), o, d, NEAR, FAR, samples, 10)


@functools.lru_cache(maxsize=None)
def grid12_for_sort3():
    """Why `overlapping` exists: on the product's own root grid the depths arrive rising (one seed in nine has a single row with a
    tie among 1000), so the kernel's identity shortcut wins and sort 3 does not run."""
    o, d = shell_rays(1000, 12)
    return Case("grid12-sort3", grid(12), o, d, NEAR, FAR, 192, 11)


@functools.lru_cache(maxsize=None)
def killer_slabs(n):
    """n slabs in the adversary's order; 24 rays of the many-crossed-boxes generator, the first 24 of its 48 (the less oblique half:
    every one of them leaves through the +x face, so it crosses all n slabs)."""
    o, d = slab_rays(24, n, scale=torch.linspace(0, 1, 48)[:24])
    return Case(f"killer-slabs-{n}", slab_voxels(n, killer_ranks(n)), o, d, NEAR, SLAB_FAR, 192, 20)


@functools.lru_cache(maxsize=None)
def ordered_slabs(n):
    """test_buff_reference_order_many_crossed_boxes' input."""
    o, d = slab_rays(48, n)
    return Case(f"ordered-slabs-{n}", slab_voxels(n), o, d, NEAR, SLAB_FAR, 192, 30)


@functools.lru_cache(maxsize=None)
def sample_counts(samples):
    o, d = shell_rays(200, 200)
    return Case(f"grid12-s{samples}", grid(12), o, d, NEAR, FAR, samples, 40)


@functools.lru_cache(maxsize=None)
def voxel_counts(n):
    """The first n boxes of a seeded permutation of the 12^3 grid; for n <= 2 the root box, n times."""
    o, d = shell_rays(200, 200 + n)
    if n <= 2:
        vox = grid(1).repeat(n, 1, 1)
    else:
        vox = grid(12)[torch.randperm(12 ** 3, generator=torch.Generator().manual_seed(n))[:n]]
    return Case(f"grid12-n{n}", vox, o, d, NEAR, FAR, 48, 50)


@functools.lru_cache(maxsize=None)
def limit_grid(extra=0):
    """16 x 16 x 32 = 8192 boxes, the most the reference order takes, plus `extra` repeated ones."""
    vox = box_grid(16, 16, 32)
    o, d = shell_rays(64, 64)
    return Case(f"limit-grid+{extra}", torch.cat((vox, vox[:extra]), 0), o, d, NEAR, FAR, 48, 60)


@functools.lru_cache(maxsize=None)
def axis_parallel():
    """Rays along an axis or in an axis plane through the 5^3 grid: 1 / 0 = +inf, 1 / -0 = -inf.  The first seven rays are listed;
    the last three repeat rays 0, 2 and 3 with one zero written as -0.0 (the sign of a zero selects the box's other corner)."""
    o = torch.tensor([[.05, .07, .9], [.05, .9, .07], [-.9, .11, .13], [.3, .31, .95], [0, 0, .9], [.12, 0, .9], [.24, .24, .9],
                      [.05, .07, .9], [-.9, .11, .13], [.3, .31, .95]])
    d = torch.tensor([[0, 0, -1], [0, -1, 0], [1, 0, 0], [0, -.6, -.8], [0, 0, -1], [0, 0, -1], [0, 0, -1],
                      [-0.0, 0, -1], [1, 0, -0.0], [-0.0, -.6, -.8]])
    return Case("axis-parallel", grid(5), o, d, NEAR, FAR, 16, 70)


# ----------------------------------------------------------------------------------------------- nm_tree_integrate, exactly

INTEGRATE_VOXELS = 1531
INTEGRATE_SHAPE = (1000, 200)
INTEGRATE_PILE = 700                  # the voxel a quarter of the samples pile onto


@functools.lru_cache(maxsize=None)
def integrate_inputs(seed=3):
    """(memm (N,), idx (K, S) int64, weights, mask_weights) with 200 000 samples: a quarter of them on voxel INTEGRATE_PILE, the
    others spread over all voxels, one in fifty out of range (-1 or N); voxels v with v % 13 == 5 receive weight but no mask weight.
    Weights and mask weights are multiples of 2^-12 below 1: every fp64 sum is exact, whatever the order of the atomics."""
    g = torch.Generator().manual_seed(seed)
    n, shape = INTEGRATE_VOXELS, INTEGRATE_SHAPE
    idx = torch.randint(0, n, shape, generator=g)
    idx[torch.rand(shape, generator=g) < 0.25] = INTEGRATE_PILE
    bad = torch.rand(shape, generator=g) < 0.02
    idx[bad] = torch.where(torch.rand(shape, generator=g) < 0.5, torch.tensor(-1), torch.tensor(n))[bad]
    w = torch.randint(0, 4096, shape, generator=g).float() / 4096
    mw = torch.randint(0, 4096, shape, generator=g).float() / 4096
    mw[torch.rand(shape, generator=g) < 0.3] = 0.0
    mw[idx % 13 == 5] = 0.0
    w[(idx % 13 == 5) & (w == 0)] = 0.5
    memm = torch.randn(n, generator=g)
    return memm, idx, w, mw


def integrate_expected(memm, counter, idx, w, mw):
    """numpy restatement of nm_tree_integrate: fp64 sums per voxel, float32(acc) / float32(freq) where freq > 0, the running mean
    m + (mean - m) / counter in float32."""
    n = memm.shape[0]
    idx, w, mw = idx.numpy().reshape(-1), w.numpy().reshape(-1).astype(np.float64), mw.numpy().reshape(-1).astype(np.float64)
    ok = (idx >= 0) & (idx < n)
    acc = np.bincount(idx[ok], weights=w[ok], minlength=n)
    freq = np.bincount(idx[ok], weights=mw[ok], minlength=n).astype(np.float32)
    m = memm.numpy().astype(np.float32)
    seen = freq > 0
    mean = acc.astype(np.float32)[seen] / freq[seen]
    out = m.copy()
    out[seen] = m[seen] + (mean - m[seen]) / np.float32(counter)
    assert out.dtype == np.float32
    return out
