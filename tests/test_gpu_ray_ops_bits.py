"""The compositing kernels and the ray generators of nerfmeshes_amd/csrc/ray_ops.hip reproduce, bit for bit, what
tests/golden/composite_bits.json recorded (tests/composite_bits.py says of what and how; tests/golden/README.md when)."""
import pytest

from tests import composite_bits as CB
from tests import composite_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from nerfmeshes_amd import hip_ops, train_ops
    return hip_ops, train_ops


@pytest.fixture(scope="module")
def want():
    return CB.recorded()


def _mismatches(got, want, where):
    if isinstance(want, dict):
        assert sorted(got) == sorted(want), where
        return [m for k in want for m in _mismatches(got[k], want[k], f"{where} {k}")]
    return [] if got == want else [where]


def test_every_case_is_recorded(want):
    assert sorted(want["composite"]) == sorted(CC.case_id(c) for c in CC.CASES)
    assert sorted(want["rays"]) == ["ndc_rays", "ray_bundle", "ray_bundle_first3_count29", "view_rays_ndc"]


@pytest.mark.parametrize("case", CC.CASES, ids=CC.case_id)
def test_composite_reproduces_the_recorded_bits(ops, want, case):
    bad = _mismatches(CB.composite_entry(*ops, case), want["composite"][CC.case_id(case)], CC.case_id(case))
    assert not bad, f"outputs whose bits changed: {bad}"


def test_ray_generators_reproduce_the_recorded_bits(ops, want):
    bad = _mismatches(CB.ray_entries(ops[0]), want["rays"], "rays")
    assert not bad, f"outputs whose bits changed: {bad}"
