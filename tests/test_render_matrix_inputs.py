"""The inputs of test_gpu_render_matrix.py's margin case, rebuilt without a GPU (ray termination).

That case is worth something only while its tiles really lie in the band where the compositor's fp32 transmittance is denormal or
has just become 0: tiles the kernel's rule (`att < -160`) finds, tiles that are dead although the rule does not find them, and
tiles with a denormal transmittance in front of them.  The coarse pass's inputs depend on constants only (sigma 109, 520 ray blocks,
spans 2 .. 6, 64 samples, unit directions), so the same four conditions are asserted here with the CPU tool's own functions: a
change of the constants cannot make the GPU test vacuous unnoticed.  A rule that is too eager (-140, say) fails here already."""
import numpy as np

from tests import render_cases as RC


def test_margin_case_has_tiles_on_both_sides_of_the_rule():
    near, far, f = RC.margin_inputs()
    assert f.shape == (520 * 8, 64) and f.dtype == np.float32
    tiles, exact, rule, not_by_rule, denormal = RC.margin_counts(f)      # asserts check_rule_is_safe
    print(f"{tiles} tiles, {exact} exactly dead, {rule} dead by the rule, {not_by_rule} dead but not by the rule, "
          f"{denormal} with a denormal front on all 8 rays")
    assert tiles == 2080
    assert rule > 0
    assert exact > rule and not_by_rule == exact - rule
    assert denormal > 0


def test_denormal_front_tiles_counts_whole_blocks_only():
    """8 rays x 32 samples, a factor of 2^-8 per sample: T in front of slot 1 is 2^-128 (denormal) on every ray; with one ray's
    factors at 1 the tile no longer counts, and at 2^-10 per sample T is 0 there."""
    f = np.full((8, 32), 2.0 ** -8, dtype=np.float32)
    assert RC.denormal_front_tiles(f).tolist() == [[False, True]]
    g = f.copy()
    g[3] = 1.0
    assert RC.denormal_front_tiles(g).tolist() == [[False, False]]
    assert RC.denormal_front_tiles(np.full((8, 32), 2.0 ** -10, dtype=np.float32)).tolist() == [[False, False]]


def test_skip_masks_of_the_matrix_networks():
    """models.py:37: layers_xyz[i] takes the encoding again where i % skip_step == 0, i > 0 and i != num_layers - 1."""
    def mask(L, step):
        return RC.skip_mask(dict(num_layers=L, skip_step=step))
    assert mask(8, 4) == 0b10000
    assert mask(2, 4) == 0
    assert mask(3, 1) == 0b10
    assert mask(5, 2) == 0b100
    assert mask(10, 3) == 0b1001000
    assert mask(4, 2) == 0b100
