"""The BuFF voxel sampler's three per-ray kernels (nerfmeshes_amd/csrc/buff_tree.hip) on the MI355X against the CPU oracle, bit for bit,
on the paths the golden vectors and tests/test_gpu_models.py do not reach: a second iteration of the per-ray loops, the real sort 3 of
the reference order, its heap-sort fallback, more than 64 crossed boxes (and more than 512: the overflow report and its reset), refined
voxel sets, the edges of the sizes, directions with zeros; and nm_tree_integrate on sums that are exact.

Inputs and references live in tests/buff_cases.py; tests/test_buff_sampler_inputs.py checks without a GPU that every input reaches the
path it is named for.  The rules of comparison are those of tests/test_gpu_models.py:

    ids="reference"   mask, z and idx of every row, hit or not (at least one ray of the batch hits)
    ids="stable"      mask of every row, z and idx of the rows that hit
    random            as stable, and the rows that miss are zero-filled; draws u_pick >= 1e-7 (below 1.7e-9 the kernel deviates from
                      the reference on purpose, see buff_random_kernel)"""
import numpy as np
import pytest
import torch

from tests import buff_cases as B
from tests.gpu_support import ops  # noqa: F401

pytestmark = pytest.mark.gpu


def _run(ops, case, mode, rows=slice(None)):
    """(z, idx, mask) of the kernel of `mode` on the rays `rows` of a case, as numpy arrays."""
    vox, o, d = case.voxels.cuda(), case.origins[rows].cuda(), case.dirs[rows].cuda()
    if mode == "random":
        u_pick, u_pos = B.draws(case)
        out = ops.buff_intersect_random(vox, o, d, case.near, case.far, u_pick[rows].cuda(), u_pos[rows].cuda())
    else:
        out = ops.buff_intersect(vox, o, d, case.near, case.far, case.samples, ids=mode)
    return tuple(x.cpu().numpy() for x in out)


def _differing_rows(a, b):
    rows = np.nonzero((a != b).reshape(a.shape[0], -1).any(1))[0]
    return f"{rows.size} of {a.shape[0]} rows differ, the first: {rows[:8].tolist()}"


def _check(case, mode, got):
    z, idx, mask = got
    ze, ie, me = B.expected(case, mode)
    assert z.dtype == np.float32 and idx.dtype == np.int64 and z.shape == ze.shape and idx.shape == ie.shape
    assert np.array_equal(mask, me), (case.name, mode, "mask", _differing_rows(mask, me))
    assert me.any(), "a batch without a hit compares nothing"
    rows = slice(None) if mode == "reference" else me
    assert np.array_equal(z[rows], ze[rows]), (case.name, mode, "z", _differing_rows(z[rows], ze[rows]))
    assert np.array_equal(idx[rows], ie[rows]), (case.name, mode, "idx", _differing_rows(idx[rows], ie[rows]))
    if mode == "random":
        assert not z[~me].any() and not idx[~me].any(), "rows of rays that cross nothing are zero-filled"


@pytest.mark.parametrize("mode", B.MODES)
def test_long_batch_second_loop_iteration(ops, mode):
    """20001 rays: more than the 4096 blocks of four rays of the stable and random kernels and more than the 32 one-ray blocks per CU of
    the reference order, so every wave takes a second ray whose crossing count differs from its first one's.  A ray's rows do not
    depend on the batch it is part of."""
    case = B.long_batch()
    rays = case.dirs.shape[0]
    assert rays > B.STABLE_RAYS_IN_FLIGHT
    assert rays > B.REFERENCE_RAYS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count
    got = _run(ops, case, mode)
    _check(case, mode, got)
    rows = slice(5000, 5100)
    alone = _run(ops, case, mode, rows)
    for a, b, what in zip(alone, got, ("z", "idx", "mask")):
        assert np.array_equal(a, b[rows]), (mode, what, _differing_rows(a, b[rows]))


@pytest.mark.parametrize("mode", B.MODES)
@pytest.mark.parametrize("which", B.REFINED_SETS)
def test_refined_trees(ops, which, mode):
    """Voxels of two and three sizes in shuffled order, counts that are no multiple of 64; the two tie orders give different ids on
    more than 40 % of the rays that hit."""
    case = B.refined(which)
    _check(case, mode, _run(ops, case, mode))


@pytest.mark.parametrize("mode", ["reference", "stable"])
@pytest.mark.parametrize("samples", [192, 512])
def test_overlapping_boxes_sort_3(ops, samples, mode):
    """Overlapping boxes: the depths arrive out of order and with ties on every ray, so the reference order runs its third sort
    (WaveSort::loop and final_slot over the samples, the gather through p_ix) where the identity shortcut always won before; the
    stable kernel's rank sorts see ties among the boxes (duplicates) and among the samples.  At 512 samples sort 3 itself runs out of
    depth on 14 of the rays and takes the heap fallback."""
    case = B.overlapping(samples)
    _check(case, mode, _run(ops, case, mode))


@pytest.mark.parametrize("n", B.KILLER_SLABS)
def test_heap_fallback(ops, n):
    """n slabs along x, listed in the order of McIlroy's adversary against introsort: sort 1 of the reference order runs out of depth
    and heap-sorts a range on lane 0 (WaveSort::loop, depth == 0), and final_slot's window of 15 has to hold behind it.  Every ray
    crosses all n slabs: 500 takes the second pass with room for 512, and the stable and random kernels work through eight chunks of
    64 crossed boxes, twelve short of their cap."""
    case = B.killer_slabs(n)
    _check(case, "reference", _run(ops, case, "reference"))
    _check(case, "stable", _run(ops, case, "stable"))
    _check(case, "random", _run(ops, case, "random"))


@pytest.mark.parametrize("mode", ["stable", "random"])
def test_more_than_64_crossed_boxes(ops, mode):
    """107 to 200 crossed boxes: the fp64 carry of the cumulative length across 64-lane chunks, rank sorts over several chunks."""
    case = B.ordered_slabs(200)
    _check(case, mode, _run(ops, case, mode))


@pytest.mark.parametrize("mode", ["stable", "random"])
def test_overflow_is_reported_and_reset(ops, mode):
    """More than 512 crossed boxes are an error that names the limit; the flag is cleared with it, the next call succeeds."""
    with pytest.raises(Exception, match="512"):
        _run(ops, B.ordered_slabs(600), mode)
    case = B.ordered_slabs(200)
    _check(case, mode, _run(ops, case, mode))


@pytest.mark.parametrize("mode", B.MODES)
@pytest.mark.parametrize("samples", B.SAMPLE_COUNTS)
def test_sample_counts(ops, samples, mode):
    case = B.sample_counts(samples)
    _check(case, mode, _run(ops, case, mode))


@pytest.mark.parametrize("mode", B.MODES)
def test_too_many_samples_raise(ops, mode):
    case = B.sample_counts(512)._replace(name="grid12-s513", samples=513)
    with pytest.raises(Exception, match="512"):
        _run(ops, case, mode)


@pytest.mark.parametrize("mode", B.MODES)
@pytest.mark.parametrize("n", B.VOXEL_COUNTS)
def test_voxel_counts(ops, n, mode):
    """Around the introsort threshold (16 / 17) and the padding of the box arrays (63 / 64 / 65, 128 / 129); every batch has rays that
    miss, whose id in the reference order is the box in one slot that depends on n alone."""
    case = B.voxel_counts(n)
    _check(case, mode, _run(ops, case, mode))


@pytest.mark.parametrize("mode", B.MODES)
def test_most_voxels_of_the_reference_order(ops, mode):
    """8192 boxes: the largest LDS layout of the reference order, introsort depth 26."""
    case = B.limit_grid(0)
    _check(case, mode, _run(ops, case, mode))


def test_one_voxel_too_many_for_the_reference_order(ops):
    case = B.limit_grid(1)
    with pytest.raises(Exception, match="8192"):
        _run(ops, case, "reference")
    _check(case, "stable", _run(ops, case, "stable"))


@pytest.mark.parametrize("mode", B.MODES)
def test_axis_parallel_rays(ops, mode):
    """Direction components of exactly +0 and -0 (the centre pixel of an axis-aligned camera): infinite slab distances, no NaN."""
    case = B.axis_parallel()
    _check(case, mode, _run(ops, case, mode))


@pytest.mark.parametrize("counter", [1, 7])
def test_tree_integrate_exact(ops, counter):
    """nm_tree_integrate where every fp64 sum is exact (weights are multiples of 2^-12), so the order of the atomics cannot show:
    200 000 samples, a quarter on one voxel, ids -1 and N skipped, voxels with weight but no mask weight untouched."""
    memm, idx, w, mw = B.integrate_inputs()
    want = B.integrate_expected(memm, counter, idx, w, mw)
    got = ops.tree_integrate(memm.clone().cuda(), counter, idx.cuda(), w.cuda(), mw.cuda()).cpu().numpy()
    assert np.array_equal(got, want), _differing_rows(got, want)
